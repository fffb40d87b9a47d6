// rtw_cli -- host driver mirroring the reference's main.rs (flags main.rs:32-87,
// defaults main.rs:20-29) and raytracing::complex (raytracing/mod.rs:54-126):
// builds the scene, runs Camera::threaded_render on the GPU, writes img.ppm.
//
// Extra flags (the reference hard-codes or time-seeds these): --depth (MAX_DEPTH,
// mod.rs:43), --seed (both XorShift::default seeds, mod.rs:67 / camera.rs:255),
// --scene (the other builders of mod.rs), --out, --mode parity|fast (fast: the
// f32 statistical mode), --gpus N|LIST (N: the first N devices; LIST: comma-
// separated device indices, repeats allowed; default: every visible device -- the
// reference's pool takes every core, camera.rs:253), --device-ppm (a one-device
// render whose frame stays in HBM: the file's text is made there, rtw_format_ppm_device,
// and is the same file byte for byte), --png (a one-device render encoded to a PNG file on
// the device, rtw_png_device; written to img.png unless --out names a file; takes
// precedence over the PPM), --passes N (fast mode, one device: the lattice in N strided
// passes whose sums add up to the same file, each pass's kernel time printed) and
// --preview-dir DIR (with it: the running mean after every pass as DIR/pass_%04u.png, the
// headless stand-in for the reference's preview window), --adaptive TOL (fast mode, one
// device: every pixel sampled until the relative standard error of its mean is <= TOL or the
// lattice is used up, rtw_session_render_fast_adaptive; --min-samples M and --batch B set the
// first round's and the later rounds' samples per pixel), --denoise [LEVELS] (fast mode, one
// device: the frame through the guided a-trous filter, rtw_session_render_fast_denoised; without
// --adaptive at tolerance 0, so every pixel gets the whole lattice), --motion (fast mode, one
// device: the bouncing scene, the final scene with its small diffuse spheres moving while the
// shutter is open, rtw_session_set_scene_moving; every fast option and output applies, but
// --denoise, which the library refuses for a moving scene). --preview is accepted and
// ignored: the winit window itself (application/mod.rs) is out of scope.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rtw_host.h"

namespace {

struct Config {  // main.rs:13-29
    uint32_t height = 1080, width = 1920, sample_sqrt = 10, depth = 0;
    bool preview = false;
    std::string scene = "complex", out = "img.ppm";
    unsigned __int128 seed = 0;
    bool seed_set = false;
    bool fast = false;
    bool device_ppm = false;
    bool png = false, out_set = false;
    uint32_t passes = 0;  // > 0: progressive fast mode
    std::string preview_dir;
    bool adaptive = false;
    double tol = 0.;
    uint32_t min_samples = 16, batch = 16;
    bool denoise = false;
    uint32_t levels = 5;
    bool motion = false;
    std::vector<int> devices;  // empty: every visible device (--device-ppm: device 0)
};

bool parse_u32(const char *s, uint32_t &v);

// --gpus N (the first N devices) or a comma-separated device list ("0,0,1")
bool parse_gpus(const char *s, std::vector<int> &out) {
    if (!s || !*s) return false;
    out.clear();
    const bool list = std::strchr(s, ',') != nullptr;
    std::string cur;
    for (const char *p = s;; ++p) {
        if (*p == ',' || !*p) {
            uint32_t v = 0;
            if (!parse_u32(cur.c_str(), v) || v > 65535) return false;
            out.push_back(static_cast<int>(v));
            cur.clear();
            if (!*p) break;
        } else {
            cur.push_back(*p);
        }
    }
    if (!list) {  // a count
        const int n = out[0];
        if (n == 0) return false;
        out.clear();
        for (int d = 0; d < n; ++d) out.push_back(d);
    }
    return true;
}

// Rust's str::parse::<usize>() (main.rs:37-39): an optional '+', then decimal
// digits only (no whitespace, no sign '-', no base prefix).
bool parse_dec(const char *s, unsigned __int128 max, unsigned __int128 &v) {
    if (!s) return false;
    if (*s == '+') ++s;
    if (!*s) return false;
    unsigned __int128 x = 0;
    for (; *s; ++s) {
        if (*s < '0' || *s > '9') return false;
        const unsigned d = static_cast<unsigned>(*s - '0');
        if (x > (max - d) / 10) return false;
        x = x * 10 + d;
    }
    v = x;
    return true;
}
bool parse_u32(const char *s, uint32_t &v) {
    unsigned __int128 x = 0;
    if (!parse_dec(s, 0xffffffffu, x)) return false;
    v = static_cast<uint32_t>(x);
    return true;
}

Config parse_args(int argc, char **argv) {
    Config c;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        const char *next = i + 1 < argc ? argv[i + 1] : nullptr;
        auto need = [&](uint32_t &dst, const char *usage) {
            if (!parse_u32(next, dst)) {
                std::fprintf(stderr, "Usage: %s <number>\n", usage);
                std::exit(1);
            }
        };
        if (a == "--height" || a == "-h") need(c.height, "--height");
        else if (a == "--width" || a == "-w") need(c.width, "--width");
        else if (a == "--samplesqrt" || a == "-s") need(c.sample_sqrt, "--samplesqrt");
        else if (a == "--depth" || a == "-d") need(c.depth, "--depth");
        else if (a == "--preview" || a == "-p") c.preview = true;
        else if (a == "--seed") {  // decimal, up to 2^128 - 1 (XorShift state is a u128)
            if (!parse_dec(next, ~static_cast<unsigned __int128>(0), c.seed)) {
                std::fprintf(stderr, "Usage: --seed <decimal number>\n");
                std::exit(1);
            }
            c.seed_set = true;
        }
        else if (a == "--scene" && next) c.scene = next;
        else if (a == "--out" && next) c.out = next, c.out_set = true;
        else if (a == "--mode" && next) {
            if (std::strcmp(next, "fast") && std::strcmp(next, "parity")) {
                std::fprintf(stderr, "Usage: --mode parity|fast\n");
                std::exit(1);
            }
            c.fast = !std::strcmp(next, "fast");
        }
        else if (a == "--gpus") {
            if (!parse_gpus(next, c.devices)) {
                std::fprintf(stderr, "Usage: --gpus <count> | <device,device,...>\n");
                std::exit(1);
            }
        }
        else if (a == "--device-ppm") c.device_ppm = true;
        else if (a == "--png") c.png = true;
        else if (a == "--passes") need(c.passes, "--passes");
        else if (a == "--preview-dir" && next) c.preview_dir = next;
        else if (a == "--adaptive") {
            char *end = nullptr;
            c.tol = next ? std::strtod(next, &end) : -1.;
            if (!next || end == next || *end || !(c.tol >= 0.)) {
                std::fprintf(stderr, "Usage: --adaptive <tolerance, e.g. 0.05>\n");
                std::exit(1);
            }
            c.adaptive = true;
        }
        else if (a == "--denoise") {  // the level count is optional
            c.denoise = true;
            uint32_t v = 0;
            if (parse_u32(next, v)) c.levels = v;
        }
        else if (a == "--motion") c.motion = true;
        else if (a == "--min-samples") need(c.min_samples, "--min-samples");
        else if (a == "--batch") need(c.batch, "--batch");
        else if (a == "--help") {
            std::printf("Use the application like this:\n");
            std::printf("\t-h --height\t:\tSet the height of the image\n");
            std::printf("\t--width -w\t:\tSet the width of the image\n");
            std::printf("\t--samplesqrt -s\t:\tSet the sqrt of the samples used for the image\n");
            std::printf("\t--preview -p\t:\tSet whether a preview window is displayed (ignored)\n");
            std::printf("\t--depth -d\t:\tMax bounce depth (reference: 10)\n");
            std::printf("\t--seed N\t:\tXorShift seed (decimal) for scene and render (reference: wall-clock ms)\n");
            std::printf("\t--scene NAME\t:\tcomplex | simple | threads | super_simple | three_lambertian\n");
            std::printf("\t--out PATH\t:\tOutput file (reference: img.ppm; with --png: img.png)\n");
            std::printf("\t--mode M\t:\tparity (f64, bit-exact; default) | fast (f32, statistical)\n");
            std::printf("\t--gpus N|LIST\t:\tthe first N GPUs, or device indices 0,1,.. (default: every GPU)\n");
            std::printf("\t--device-ppm\t:\tone GPU; the frame stays in HBM and the PPM text is made there\n");
            std::printf("\t--png\t\t:\tone GPU; the frame is encoded to a PNG file there; takes precedence over the PPM\n");
            std::printf("\t--passes N\t:\tfast mode, one GPU: render in N passes over the whole lattice (same file)\n");
            std::printf("\t--preview-dir D\t:\twith --passes: the image so far after each pass as D/pass_NNNN.png\n");
            std::printf("\t--adaptive TOL\t:\tfast mode, one GPU: sample each pixel to a relative standard error of TOL\n");
            std::printf("\t--min-samples M\t:\twith --adaptive: samples every pixel gets first (default 16)\n");
            std::printf("\t--batch B\t:\twith --adaptive: samples per listed pixel and round (default 16)\n");
            std::printf("\t--denoise [L]\t:\tfast mode, one GPU: filter the frame with L a-trous levels (default 5)\n");
            std::printf("\t--motion\t:\tfast mode, one GPU: the final scene with bouncing spheres and motion blur\n");
            std::exit(0);
        }
    }
    if (!c.preview_dir.empty() && !c.passes) c.passes = 1;
    if (c.passes && (!c.fast || c.device_ppm || c.devices.size() > 1)) {
        std::fprintf(stderr, "--passes and --preview-dir need --mode fast on one device, without --device-ppm\n");
        std::exit(1);
    }
    if (c.adaptive && (!c.fast || c.passes || c.devices.size() > 1)) {
        std::fprintf(stderr, "--adaptive needs --mode fast on one device, without --passes\n");
        std::exit(1);
    }
    if (c.denoise && (!c.fast || c.passes || c.devices.size() > 1)) {
        std::fprintf(stderr, "--denoise needs --mode fast on one device, without --passes\n");
        std::exit(1);
    }
    if (c.scene == "bouncing") c.motion = true;  // the scene is its motion: never rendered standing still
    if (c.motion) {
        if (!c.fast || c.devices.size() > 1) {
            std::fprintf(stderr, "--motion (--scene bouncing) needs --mode fast on one device\n");
            std::exit(1);
        }
        c.scene = "bouncing";
        // a moving scene lives in a session: the plain render takes the one-device route whose
        // PPM text is made on the device (the same file byte for byte)
        if (!c.png && !c.passes && !c.adaptive && !c.denoise) c.device_ppm = true;
    }
    if ((c.device_ppm || c.png) && c.devices.size() > 1) {  // the frame of a multi-device render is gathered on the host
        std::fprintf(stderr, "%s needs a one-device render: --gpus selects %zu devices\n",
                     c.png ? "--png" : "--device-ppm", c.devices.size());
        std::exit(1);
    }
    if (c.png && !c.out_set) c.out = "img.png";
    if (!c.seed_set)  // XorShift::default(): milliseconds since the Unix epoch
        c.seed = static_cast<unsigned long long>(
            std::chrono::duration_cast<std::chrono::milliseconds>(
                std::chrono::system_clock::now().time_since_epoch())
                .count());
    return c;
}

std::string dec(unsigned __int128 v) {
    std::string r;
    do {
        r.insert(r.begin(), static_cast<char>('0' + static_cast<int>(v % 10)));
        v /= 10;
    } while (v);
    return r;
}

}  // namespace

int main(int argc, char **argv) {
    const Config cfg = parse_args(argc, argv);
    if (cfg.preview) std::fprintf(stderr, "note: --preview is not supported; rendering headless\n");
    try {
        const rtw_u128 seed{static_cast<uint64_t>(cfg.seed), static_cast<uint64_t>(cfg.seed >> 64)};
        rtw::BuiltScene b = rtw::build_scene(cfg.scene, seed, cfg.height, cfg.width, cfg.depth);
        std::printf(
            "\n            Multithreaded rendering\n            Making an image of format:\n"
            "                %u by %u\n                %u samples\n                %u max depth\n\n",
            b.cam.width(), b.cam.height(), cfg.sample_sqrt * cfg.sample_sqrt, b.cam.d.max_depth);
        rtw_stats st{};
        const auto t0 = std::chrono::steady_clock::now();
        if (cfg.adaptive || cfg.denoise) {
            std::vector<float> f32;
            rtw_adaptive_info info{};
            const rtw_denoise_params dn{cfg.levels, 5u, 0xBu, 4.f};
            double denoise_ms = 0.;
            const std::string file = rtw::render_adaptive_device(
                b.cam, *b.world, cfg.sample_sqrt, seed, cfg.devices.empty() ? 0 : cfg.devices[0], cfg.tol, 0.05,
                cfg.min_samples, cfg.batch, cfg.png ? 2 : (cfg.device_ppm ? 1 : 0), &f32, &info, &st,
                cfg.denoise ? &dn : nullptr, &denoise_ms);
            if (cfg.denoise) std::printf("denoise: %u levels, filter %.3f ms\n", cfg.levels, denoise_ms);
            std::printf("adaptive: %u rounds, %llu samples, %.2f mean samples per pixel\n", info.rounds,
                        static_cast<unsigned long long>(info.samples),
                        static_cast<double>(info.samples) / static_cast<double>(st.pixels ? st.pixels : 1));
            if (cfg.png || cfg.device_ppm) {
                FILE *f = std::fopen(cfg.out.c_str(), "wb");
                if (!f) throw rtw::Error(RTW_E_ARG, "cannot create " + cfg.out);
                const bool short_write = std::fwrite(file.data(), 1, file.size(), f) != file.size();
                if (std::fclose(f) != 0 || short_write) throw rtw::Error(RTW_E_ARG, "short write");
            } else {
                const std::vector<double> fb(f32.begin(), f32.end());
                const int rc = rtw_write_ppm(cfg.out.c_str(), fb.data(), b.cam.width(), b.cam.height());
                if (rc != RTW_OK) throw rtw::Error(rc, rtw_last_error());
            }
        } else if (cfg.passes) {
            std::vector<float> f32, ms;
            const std::string png = rtw::render_progressive_device(b.cam, *b.world, cfg.sample_sqrt, seed,
                                                                   cfg.devices.empty() ? 0 : cfg.devices[0], cfg.passes,
                                                                   cfg.preview_dir, cfg.png, &f32, &ms, &st);
            for (size_t p = 0; p < ms.size(); ++p) std::printf("pass %zu: kernel %.3f ms\n", p, ms[p]);
            if (cfg.png) {
                FILE *f = std::fopen(cfg.out.c_str(), "wb");
                if (!f) throw rtw::Error(RTW_E_ARG, "cannot create " + cfg.out);
                const bool short_write = std::fwrite(png.data(), 1, png.size(), f) != png.size();
                if (std::fclose(f) != 0 || short_write) throw rtw::Error(RTW_E_ARG, "short write");
            } else {
                const std::vector<double> fb(f32.begin(), f32.end());
                const int rc = rtw_write_ppm(cfg.out.c_str(), fb.data(), b.cam.width(), b.cam.height());
                if (rc != RTW_OK) throw rtw::Error(rc, rtw_last_error());
            }
        } else if (cfg.png || cfg.device_ppm) {
            uint64_t wide = 0;
            const int device = cfg.devices.empty() ? 0 : cfg.devices[0];
            const std::string text =
                cfg.png ? rtw::render_png_device(b.cam, *b.world, cfg.sample_sqrt, seed, cfg.fast, device, -1, &st)
                        : rtw::render_ppm_device(b.cam, *b.world, cfg.sample_sqrt, seed, cfg.fast, device, &st, &wide);
            FILE *f = std::fopen(cfg.out.c_str(), "wb");
            if (!f) throw rtw::Error(RTW_E_ARG, "cannot create " + cfg.out);
            const bool short_write = std::fwrite(text.data(), 1, text.size(), f) != text.size();
            if (std::fclose(f) != 0 || short_write) throw rtw::Error(RTW_E_ARG, "short write");
        } else if (cfg.fast) {
            rtw::FlatScene flat;
            b.world->flatten(flat);
            std::vector<float> f32(static_cast<size_t>(b.cam.width()) * b.cam.height() * 3);
            int rc = rtw_threaded_render_multi_fast(
                &b.cam.d, flat.spheres.data(), static_cast<uint32_t>(flat.spheres.size()), flat.materials.data(),
                static_cast<uint32_t>(flat.materials.size()), cfg.sample_sqrt, seed,
                cfg.devices.empty() ? nullptr : cfg.devices.data(), static_cast<uint32_t>(cfg.devices.size()),
                f32.data(), &st);
            if (rc != RTW_OK) throw rtw::Error(rc, rtw_last_error());
            const std::vector<double> fb(f32.begin(), f32.end());
            rc = rtw_write_ppm(cfg.out.c_str(), fb.data(), b.cam.width(), b.cam.height());
            if (rc != RTW_OK) throw rtw::Error(rc, rtw_last_error());
        } else {
            rtw::Camera::threaded_render(b.cam, *b.world, cfg.sample_sqrt, seed, cfg.out.c_str(), &st, cfg.devices);
        }
        const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        std::printf("Finished succesfully: %s (%.3f s wall, kernel %.3f ms, %.1f Msamples/s, seed %s)\n",
                    cfg.out.c_str(), s, st.kernel_ms, st.samples / st.kernel_ms / 1e3, dec(cfg.seed).c_str());
    } catch (const rtw::Error &e) {
        // main.rs:106-110: the render thread's error is printed, and main still
        // returns Ok(()) -- exit status 0, as the reference
        std::fprintf(stderr, "\nRender thread errored with %s\n", e.what());
    }
    return 0;
}
