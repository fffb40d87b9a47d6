// rtw_fast_denoise.hip -- fast-mode frames denoised on the device by an edge-stopping a-trous
// filter that the frame's own variance and first-hit guides drive (definitions in rtw_capi.h,
// design and measurements in DESIGN 3.12). Three kernels:
//   * rtw_fast_guides: the pixel-centre ray of every shard pixel to its first hit; one float4
//     (shading normal, kind << 30 | sphere) per pixel. Persistent like the other fast-mode
//     kernels (scene in LDS when it fits, rtw_fast_dev.h's scene_hit); a wave claims 8x8 pixel
//     tiles from the launch's cursor, so its 64 rays enter the BVH side by side.
//   * rtw_dn_prepare: sums, counts and moments to (r, g, b, variance of the mean of r+g+b).
//   * rtw_dn_level: one a-trous level, 5x5 taps at step t = 2^l. At step t the image is t^2
//     interleaved sub-lattices (x = a, y = b mod t) and a tap never leaves its pixel's
//     sub-lattice, so a 256-thread workgroup takes a 16x16 tile of ONE sub-lattice: it stages
//     the tile and a halo of 2 (20x20 colour records + 20x20 guide records = 12.8 KB) into
//     LDS with float4 loads at stride t, and all 25 taps and the 3x3 variance prefilter are
//     ds_read_b128 at offsets known at compile time. Every level has the same LDS footprint
//     and inner loop; only the global stride changes. 400 records are read per 256 written.
//     A wave's 16 lanes of one b128 pass are 16 consecutive records of a tile row, 64
//     consecutive dwords: no bank conflict whatever the row pitch, so the rows are not padded.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <mutex>

#include "rtw_fast_denoise.h"
#include "rtw_fast_dev.h"
#include "rtw_internal.h"

namespace rtw_fast {
namespace {

typedef unsigned __int128 u128;

// ---- guides
template <bool kLds>
__global__ __launch_bounds__(kBlock, 2) void rtw_fast_guides(const GuideParams A) {
    extern __shared__ __attribute__((aligned(16))) float4 lds[];
    const FastParams &P = A.f;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    uint16_t *stk = reinterpret_cast<uint16_t *>(lds) + tid;  // slot j at stk[j * kBlock]
    const float4 *geo, *mat, *nodes;
    const uint32_t *kind;
    stage_scene<kLds>(P, lds, tid, geo, mat, nodes, kind);
    uint32_t visits = 0, wvisits = 0, written = 0, iters = 0;
    for (;;) {
        uint32_t tile = 0;
        if (lane == 0) tile = atomicAdd(P.cursor, 1u);
        tile = __builtin_amdgcn_readfirstlane(tile);
        if (tile >= A.n_tiles) break;
        ++iters;
        const uint32_t ty = tile / A.tiles_x, tx = tile - ty * A.tiles_x;
        const uint32_t x = tx * 8u + (lane & 7u), lr = ty * 8u + (lane >> 3);
        if (x < P.W && lr < P.n_rows) {
            const uint32_t pix = lr * P.W + x;
            Rng rng;
            Seg g;
            start_path(P, pix, 0u, rng, g);  // s = 0, no defocus: the centre ray, nothing drawn
            float best;
            int hid;
            scene_hit(P, geo, nodes, g, best, hid, stk, visits, wvisits);
            float4 rec = make_float4(g.ex, g.ey, g.ez, __uint_as_float(0xffffffffu));
            if (hid >= 0) {  // trace_segment's shading normal
                const float4 S = geo[hid];
                const float px = fmaf(best, g.ex, g.ox), py = fmaf(best, g.ey, g.oy), pz = fmaf(best, g.ez, g.oz);
                const float ir = __builtin_amdgcn_rcpf(S.w);
                float nx = (px - S.x) * ir, ny = (py - S.y) * ir, nz = (pz - S.z) * ir;
                if (!(fmaf(g.ex, nx, fmaf(g.ey, ny, g.ez * nz)) < 0.f)) nx = -nx, ny = -ny, nz = -nz;
                rec = make_float4(nx, ny, nz, __uint_as_float((kind[hid] << 30) | static_cast<uint32_t>(hid)));
            }
            A.guides[pix] = rec;
            ++written;
        }
    }
    add_counters(P, lane, WaveStats{written, visits, iters, wvisits}, written, true);
}

// ---- the filter
struct DnParams {
    const float4 *src;     // the level's input plane
    const float4 *guides;
    float4 *dst;           // its output plane (unless last)
    float *out_rgb, *out_var;  // the last stage's outputs (out_var, preview nullable)
    uint32_t *preview;
    uint32_t W, rows;
    uint32_t log2t, sub_x, tiles_x, tiles_y;  // step 2^log2t; min(t, W) sub-lattice columns; 16x16 tiles of one
    uint32_t normal_log2, mask, last;
    float sigma_l;
};

__device__ __forceinline__ void emit(const DnParams &A, uint64_t p, const float4 c) {
    A.out_rgb[p * 3u + 0] = c.x, A.out_rgb[p * 3u + 1] = c.y, A.out_rgb[p * 3u + 2] = c.z;
    if (A.out_var) A.out_var[p] = c.w;
    if (A.preview) A.preview[p] = preview_u8(c.x) | (preview_u8(c.y) << 8) | (preview_u8(c.z) << 16) | 0xff000000u;
}

// D to the nearest double (ties to even): the top 64 bits with the rest folded into bit 0,
// which lies below the 53-bit rounding position, then scaled.
__device__ __forceinline__ double u128_to_double(u128 D) {
    const unsigned long long hi = static_cast<unsigned long long>(D >> 64), lo = static_cast<unsigned long long>(D);
    if (hi == 0) return static_cast<double>(lo);
    const int sh = __builtin_clzll(hi);
    const u128 n = D << sh;
    unsigned long long top = static_cast<unsigned long long>(n >> 64);
    if (static_cast<unsigned long long>(n)) top |= 1ull;
    return ldexp(static_cast<double>(top), 64 - sh);
}

__global__ __launch_bounds__(256) void rtw_dn_prepare(const unsigned long long *__restrict__ acc,
                                                      const uint32_t *__restrict__ counts,
                                                      const unsigned long long *__restrict__ mom, uint64_t npix,
                                                      const DnParams A) {
    const uint64_t p = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    if (p >= npix) return;
    const uint32_t n = counts[p];
    const double dn = static_cast<double>(n);
    float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
    if (n) c.x = mean_f32(acc[p * 3u], dn), c.y = mean_f32(acc[p * 3u + 1], dn), c.z = mean_f32(acc[p * 3u + 2], dn);
    if (n == 1) {
        const float L = (c.x + c.y) + c.z;
        c.w = L * L;
    } else if (n >= 2) {
        const ulonglong2 m = reinterpret_cast<const ulonglong2 *>(mom)[p];
        const u128 D = static_cast<u128>(n) * m.y - static_cast<u128>(m.x) * m.x;
        c.w = static_cast<float>(u128_to_double(D) * (1. / 4294967296.) / (dn * dn * static_cast<double>(n - 1u)));
    }
    if (A.last) emit(A, p, c);
    else A.dst[p] = c;
}

constexpr int kTile = 16, kHalo = 2, kSpan = kTile + 2 * kHalo;  // 20 records a staged row
constexpr float kLog2e = 1.44269504088896340736f;

__global__ __launch_bounds__(kTile * kTile) __attribute__((amdgpu_waves_per_eu(8, 8))) void rtw_dn_level(const DnParams A) {
    __shared__ float4 sc[kSpan * kSpan], sg[kSpan * kSpan];
    const uint32_t tid = threadIdx.x;
    // workgroup -> (sub-lattice (a, b), tile of it)
    const uint32_t per = A.tiles_x * A.tiles_y;
    const uint32_t sub = blockIdx.x / per, tile = blockIdx.x - sub * per;
    const uint32_t b = sub / A.sub_x, a = sub - b * A.sub_x;
    const uint32_t tyi = tile / A.tiles_x, txi = tile - tyi * A.tiles_x;
    const long long t = 1ll << A.log2t, W = A.W, rows = A.rows;
    // image coordinates of the staged square's first record (may lie left of / above the image)
    const long long x0 = a + (static_cast<long long>(txi) * kTile - kHalo) * t;
    const long long y0 = b + (static_cast<long long>(tyi) * kTile - kHalo) * t;
    for (uint32_t r = tid; r < kSpan * kSpan; r += kTile * kTile) {
        const uint32_t sy = r / kSpan, sx = r - sy * kSpan;
        const long long x = x0 + sx * t, y = y0 + sy * t;
        // outside the buffer: a zero normal makes every weight on the record 0
        float4 c = make_float4(0.f, 0.f, 0.f, 0.f), g = c;
        if (x >= 0 && x < W && y >= 0 && y < rows) c = A.src[y * W + x], g = A.guides[y * W + x];
        sc[r] = c, sg[r] = g;
    }
    __syncthreads();
    const int lx = tid & (kTile - 1), ly = tid / kTile;
    const long long x = x0 + (lx + kHalo) * t, y = y0 + (ly + kHalo) * t;
    if (x >= W || y >= rows) return;
    const int ci = (ly + kHalo) * kSpan + lx + kHalo;
    const float4 cp = sc[ci], gp = sg[ci];
    const uint32_t tagp = __float_as_uint(gp.w);
    float4 o = cp;
    if ((A.mask >> (tagp >> 30)) & 1u) {
        // the (1,2,1)x(1,2,1) average of v over the taps inside the buffer
        const bool in_x[3] = {x - t >= 0, true, x + t < W}, in_y[3] = {y - t >= 0, true, y + t < rows};
        float num = 0.f, den = 0.f;
#pragma unroll
        for (int j = -1; j <= 1; ++j)
#pragma unroll
            for (int i = -1; i <= 1; ++i) {
                const float k = static_cast<float>((2 - (i < 0 ? -i : i)) * (2 - (j < 0 ? -j : j)));
                if (in_x[i + 1] && in_y[j + 1]) num += k * sc[ci + j * kSpan + i].w, den += k;
            }
        const float gv = num / den;
        // exp(-|dL| / (sigma_l sqrt(g) + 1e-6)) = exp2(|dL| * ninv)
        const float ninv = -kLog2e * __builtin_amdgcn_rcpf(fmaf(A.sigma_l, __builtin_sqrtf(gv), 1e-6f));
        const float Lp = (cp.x + cp.y) + cp.z;
        const uint32_t nl = A.normal_log2;
        float sw = 0.f, sr = 0.f, sgn = 0.f, sb = 0.f, sv = 0.f;
        // a row of 5 taps per trip (10 ds_read_b128 at fixed offsets from the row's address): the
        // rows stay a loop so that a row's records, not all 50, are live at once
#pragma unroll 1
        for (int j = -2; j <= 2; ++j) {
            const float hj = j == 0 ? 3.f / 8.f : (j == 1 || j == -1 ? 1.f / 4.f : 1.f / 16.f);
            const float4 *rc = sc + ci + j * kSpan, *rg = sg + ci + j * kSpan;
#pragma unroll
            for (int i = -2; i <= 2; ++i) {
                constexpr float h[5] = {1.f / 16.f, 1.f / 4.f, 3.f / 8.f, 1.f / 4.f, 1.f / 16.f};
                const float4 cq = rc[i], gq = rg[i];
                float d = fmaxf(0.f, fmaf(gp.x, gq.x, fmaf(gp.y, gq.y, gp.z * gq.z)));
                for (uint32_t k = 0; k < nl; ++k) d *= d;
                const float Lq = (cq.x + cq.y) + cq.z;
                float w = (h[i + 2] * hj) * d * __builtin_amdgcn_exp2f(fabsf(Lp - Lq) * ninv);
                if (__float_as_uint(gq.w) != tagp) w = 0.f;
                sw += w;
                sr = fmaf(w, cq.x, sr), sgn = fmaf(w, cq.y, sgn), sb = fmaf(w, cq.z, sb);
                sv = fmaf(w * w, cq.w, sv);
            }
        }
        const float iw = 1.f / sw;
        o = make_float4(sr * iw, sgn * iw, sb * iw, sv * iw * iw);
    }
    const uint64_t p = static_cast<uint64_t>(y * W + x);
    if (A.last) emit(A, p, o);
    else A.dst[p] = o;
}

}  // namespace

hipError_t launch_guides(const GuideParams &A, int n_cu, hipStream_t st, bool scene_lds) {
    const bool nothing = A.n_tiles == 0;
    // a wave starts on a tile of 64 pixels
    return launch_persistent(rtw_fast_guides<true>, rtw_fast_guides<false>, A, A.f, nothing, 5, kBlock, kLdsCap, n_cu, st,
                             scene_lds);
}

}  // namespace rtw_fast

// ------------------------------------------------------------------- host ---
namespace {

// The filter's two ping-pong planes per device, grow-only, owned by the library.
struct DnCtx {
    int device = 0;
    std::mutex mu;  // one call at a time per device
    float4 *d = nullptr;
    size_t cap = 0;  // pixels per plane
    hipEvent_t ev_done = nullptr;
    hipStream_t last_stream = nullptr;
    bool pending = false;  // ev_done was recorded on last_stream

    ~DnCtx() {
        (void)hipSetDevice(device);
        (void)hipDeviceSynchronize();
        if (d) (void)hipFree(d);
        if (ev_done) (void)hipEventDestroy(ev_done);
    }
};

std::mutex g_mu;
std::map<int, DnCtx *> g_ctx;

DnCtx *context(int device) {
    std::lock_guard<std::mutex> lock(g_mu);
    auto it = g_ctx.find(device);
    if (it != g_ctx.end()) {
        HIPCHECK(hipSetDevice(device));
        return it->second;
    }
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) throw rtw::Error(RTW_E_NO_DEVICE, "no HIP device");
    if (device < 0 || device >= n) throw rtw::Error(RTW_E_NO_DEVICE, "device index out of range");
    HIPCHECK(hipSetDevice(device));
    auto *c = new DnCtx();
    c->device = device;
    try {
        HIPCHECK(hipEventCreateWithFlags(&c->ev_done, hipEventDisableTiming));
    } catch (...) {
        delete c;
        throw;
    }
    g_ctx[device] = c;
    return c;
}

void denoise(int device, const unsigned long long *acc, const uint32_t *counts, const unsigned long long *mom,
             const float *guides, uint32_t width, uint32_t rows, const rtw_denoise_params *params, float *out_rgb,
             float *out_var, uint8_t *preview, hipStream_t st) {
    if (!acc || !counts || !mom || !guides || !out_rgb) throw rtw::Error(RTW_E_ARG, "null argument");
    if (reinterpret_cast<uintptr_t>(mom) % 16 || reinterpret_cast<uintptr_t>(guides) % 16)
        throw rtw::Error(RTW_E_ARG, "mom or guides buffer not 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(preview) % 4) throw rtw::Error(RTW_E_ARG, "preview buffer not 4-byte aligned");
    const rtw_denoise_params q = rtw::checked_denoise_params(params);
    if (width == 0 || rows == 0) throw rtw::Error(RTW_E_EMPTY_IMAGE, "image height and width must be > 0");
    const uint64_t npix = static_cast<uint64_t>(width) * rows;
    if (npix >= (1ull << 31)) throw rtw::Error(RTW_E_UNSUPPORTED, "denoise: image of 2^31 pixels or more");
    DnCtx *c = context(device);
    std::lock_guard<std::mutex> lock(c->mu);
    if (q.levels && npix > c->cap) {
        HIPCHECK(hipDeviceSynchronize());  // nothing in flight reads the old planes
        if (c->d) HIPCHECK(hipFree(c->d));
        c->d = nullptr, c->cap = 0;
        HIPCHECK(hipMalloc(&c->d, 2 * npix * sizeof(float4)));
        c->cap = npix;
    }
    // a call on another stream than the previous one waits for it on the device
    if (c->pending && c->last_stream != st) HIPCHECK(hipStreamWaitEvent(st, c->ev_done, 0));
    float4 *plane[2] = {c->d, c->d + c->cap};
    rtw_fast::DnParams A{};
    A.guides = reinterpret_cast<const float4 *>(guides);
    A.out_rgb = out_rgb, A.out_var = out_var, A.preview = reinterpret_cast<uint32_t *>(preview);
    A.W = width, A.rows = rows;
    A.normal_log2 = q.normal_log2, A.mask = q.filter_mask, A.sigma_l = q.sigma_l;
    A.dst = plane[0], A.last = q.levels == 0;
    hipLaunchKernelGGL(rtw_fast::rtw_dn_prepare, dim3(static_cast<uint32_t>((npix + 255) / 256)), dim3(256), 0, st, acc,
                       counts, mom, npix, A);
    for (uint32_t l = 0; l < q.levels; ++l) {
        const uint32_t t = 1u << l;
        A.src = plane[l & 1u], A.dst = plane[(l & 1u) ^ 1u], A.last = l + 1 == q.levels;
        A.log2t = l, A.sub_x = std::min(t, width);
        // the longest sub-lattice row and column, in 16-tiles
        A.tiles_x = ((width + t - 1) / t + rtw_fast::kTile - 1) / rtw_fast::kTile;
        A.tiles_y = ((rows + t - 1) / t + rtw_fast::kTile - 1) / rtw_fast::kTile;
        const uint64_t blocks = static_cast<uint64_t>(A.sub_x) * std::min(t, rows) * A.tiles_x * A.tiles_y;
        hipLaunchKernelGGL(rtw_fast::rtw_dn_level, dim3(static_cast<uint32_t>(blocks)), dim3(rtw_fast::kTile * rtw_fast::kTile),
                           0, st, A);
    }
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipEventRecord(c->ev_done, st));
    c->last_stream = st, c->pending = true;
}

}  // namespace

namespace rtw {

rtw_denoise_params checked_denoise_params(const rtw_denoise_params *p) {
    const rtw_denoise_params q = p ? *p : rtw_denoise_params{5u, 5u, 0xBu, 4.f};
    if (q.levels > 8 || q.normal_log2 > 8 || q.filter_mask > 15u)
        throw Error(RTW_E_ARG, "denoise: levels > 8, normal_log2 > 8 or filter_mask > 15");
    if (!std::isfinite(q.sigma_l) || q.sigma_l < 0.f) throw Error(RTW_E_ARG, "denoise: sigma_l negative or not finite");
    return q;
}

void denoise_shutdown() {
    DeviceGuard guard;
    std::lock_guard<std::mutex> lock(g_mu);
    for (auto &kv : g_ctx) delete kv.second;
    g_ctx.clear();
}

}  // namespace rtw

extern "C" int rtw_denoise_fast(int device, const unsigned long long *acc_device, const uint32_t *counts_device,
                                const unsigned long long *mom_device, const float *guides_device, uint32_t width,
                                uint32_t rows, const rtw_denoise_params *params, float *out_rgb_device,
                                float *out_var_device, uint8_t *preview_rgba8_device, void *hip_stream) {
    DeviceGuard device_guard;
    try {
        denoise(device, acc_device, counts_device, mom_device, guides_device, width, rows, params, out_rgb_device,
                out_var_device, preview_rgba8_device, static_cast<hipStream_t>(hip_stream));
        return RTW_OK;
    } catch (const rtw::Error &e) {
        rtw::set_error(e.what());
        return e.code;
    } catch (const std::exception &e) {
        rtw::set_error(e.what());
        return RTW_E_ARG;
    }
}
