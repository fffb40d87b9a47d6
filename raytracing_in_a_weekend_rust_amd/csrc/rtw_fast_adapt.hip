// rtw_fast_adapt.hip -- adaptive fast mode: samples go only to the pixels that still need
// them. Three pieces (definitions in rtw_capi.h, design in DESIGN 3.11):
//   * rtw_fast_acc_list: the next m lattice samples of every pixel of a device list, added
//     to the 32.32 sums, the luminance moments and the per-pixel counts. The list's length
//     is read on the device, so a round is launched without the host knowing it.
//   * rtw_adapt_flag / _dilate / _scan / _emit: the exact 128-bit convergence test per
//     pixel packed one bit per pixel, its 3x3 dilation, and the compaction of the listed
//     pixels into an ascending index list (ballot, popcount, one scan, mbcnt rank).
//   * rtw_fast_resolve_counts: rtw_fast_resolve with the divisor read per pixel.
// The per-sample code is rtw_fast_dev.h's, called and not copied: a sample has the bits it
// has in the one-shot render, so the sums of a pixel that reached the lattice's end are
// rtw_session_render_fast's.
//
// The list kernel is rtw_fast_acc_ring's scheme (rtw_fast_acc.hip) with per-slot sample
// ranges: a persistent wave claims list entries in chunks from one cursor atomic and keeps a
// ring of kListRing pixels in flight. The ring state (pixel, first ordinal, count after the
// round, samples outstanding per slot; the slot being handed out and its next ordinal) is
// wave-uniform, in scalar registers. Idle lanes take the next ordinals of the newest slot
// by ballot + mbcnt; a lane whose path ends adds R, G, B, q and q^2 to the slot's five u64
// sums in LDS (LDS atomics), and a slot whose samples are all back is flushed by six lanes:
// five plain read-add-writes and the count's store. A pixel is in a list at most once and a
// list entry belongs to one wave, so nothing needs an HBM atomic, and a pixel outside the
// list is never touched. m >= 16 keeps two waves' worth of samples in the ring; below that
// 8 m lanes are busy (first rounds use min_samples >= 2, later ones the batch, 16 by
// default: a second kernel for small m would serve no caller of the driver).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "rtw_fast_adapt.h"
#include "rtw_fast_dev.h"
#include "rtw_host.h"
#include "rtw_internal.h"
#include "rtw_png.h"

namespace rtw_fast {
namespace {

typedef unsigned __int128 u128;

// ---- samples for the pixels of a list: what rtw_fast_dev.h's ring scheduler claims, adds
// and flushes here
struct List {
    struct Job {
        uint32_t pix, first, end;  // the pixel's ordinals [first, end); end is its count after the round
    };
    static constexpr uint32_t kRing = kListRing, kSums = kListSums;
    const ListParams &A;
    const uint32_t npix, n_ent, chunk;
    ChunkCursor cursor;
    uint32_t served = 0, traced = 0;
    __device__ __forceinline__ Claim claim(uint32_t lane, Job &j) {
        uint32_t e;
        if (!cursor.next(A.f, lane, chunk, n_ent, e)) return Claim::kDone;
        const uint32_t p = A.list ? __builtin_amdgcn_readfirstlane(A.list[e]) : e;
        ++served;
        // an entry that is no pixel of the shard, or a pixel at the lattice's end, gets nothing
        const uint32_t n0 = p < npix ? __builtin_amdgcn_readfirstlane(A.counts[p]) : A.f.n_off;
        if (n0 >= A.f.n_off) return Claim::kSkip;
        j = Job{p, n0, n0 + min(A.m, A.f.n_off - n0)};
        traced += j.end - j.first;
        return Claim::kJob;
    }
    __device__ __forceinline__ uint32_t count(const Job &j) const { return j.end - j.first; }
    // ordinal i is lattice sample (i k_mul) mod n_off; i, k_mul < 2^16: the product fits 32 bits
    __device__ __forceinline__ uint32_t lattice(const Job &j, uint32_t i) const {
        return ((j.first + i) * A.k_mul) % A.f.n_off;
    }
    static __device__ __forceinline__ void add(unsigned long long *a, unsigned long long r, unsigned long long g,
                                               unsigned long long b) {
        const unsigned long long q = min((r + g + b) >> 16, (1ull << 24) - 1ull);
        RgbSums::add(a, r, g, b);
        atomicAdd(a + 3, q);
        atomicAdd(a + 4, q * q);
    }
    // six lanes: five plain read-add-writes and the count's store
    __device__ __forceinline__ void flush(uint32_t lane, const Job &j, const unsigned long long *a) const {
        const uint64_t p = j.pix;
        if (lane < 3) A.acc[p * 3u + lane] += a[lane];
        else if (lane < kListSums) A.mom[p * 2u + (lane - 3u)] += a[lane];
        else if (lane == kListSums) A.counts[p] = j.end;
    }
};

template <bool kLds, bool kMove>
__global__ __launch_bounds__(kBlock, 2) void rtw_fast_acc_list(const ListParams A) {
    const FastParams &P = A.f;
    const uint32_t npix = P.n_rows * P.W;
    // a list of distinct pixels is no longer than the shard; a null list is every pixel
    const uint32_t n_ent = A.list ? min(__builtin_amdgcn_readfirstlane(*A.n_list), npix) : npix;
    // entries per cursor atomic: the launcher's chunk, less for a list too short to give every
    // wave of the grid one (a short list spread over few waves is a long tail of serial paths)
    const uint32_t chunk = min(A.chunk, max(1u, n_ent / (gridDim.x * kWaves)));
    // every workgroup before this one has a chunk per wave to claim: nothing is left here
    if (blockIdx.x != 0 && static_cast<uint64_t>(blockIdx.x) * kWaves * chunk >= n_ent) return;
    List u{A, npix, n_ent, chunk, {}};
    uint32_t flushed;
    const WaveStats w = run_ring<kLds, kMove>(P, u, flushed);
    // [2] counts every pixel that needs nothing more from this launch: the served entries, and
    // once the pixels outside the list
    unsigned long long done = u.served;
    if (blockIdx.x == 0 && threadIdx.x < 64u) done += npix - n_ent;
    add_counters(P, threadIdx.x & 63u, w, done, false, u.traced);
}

// ---- selection
// conv(p) of rtw_capi.h, in unsigned 128-bit arithmetic (mod 2^128). For sums the list
// kernel built: A < 2^40, B < 2^64, D = n B - A^2 in [0, 2^80), D 2^16 < 2^96;
// E = (A + n F) >> 8 < 2^33, T^2 (n - 1) E^2 < 2^32 2^16 2^66 = 2^114.
__device__ __forceinline__ bool converged(uint32_t n, unsigned long long A, unsigned long long B, uint32_t T,
                                          uint32_t F) {
    if (T == 0 || n < 2) return false;
    const u128 D = static_cast<u128>(n) * B - static_cast<u128>(A) * A;
    const u128 E = (static_cast<u128>(A) + static_cast<u128>(n) * F) >> 8;
    return (D << 16) <= static_cast<u128>(static_cast<unsigned long long>(T) * T * (n - 1u)) * E * E;
}

constexpr uint32_t kSelBlock = 256, kScanBlock = 1024;

// u(p) and n < N, one bit per pixel each: a wave's ballot is one u64 store
__global__ __launch_bounds__(kSelBlock) void rtw_adapt_flag(const uint32_t *__restrict__ counts,
                                                            const unsigned long long *__restrict__ mom, uint32_t npix,
                                                            uint32_t n_words, uint32_t N, uint32_t T, uint32_t F,
                                                            unsigned long long *__restrict__ ubits,
                                                            unsigned long long *__restrict__ live) {
    const uint32_t p = blockIdx.x * kSelBlock + threadIdx.x;
    bool lv = false, u = false;
    if (p < npix) {
        const uint32_t n = counts[p];
        lv = n < N;
        if (lv) {
            const ulonglong2 m = reinterpret_cast<const ulonglong2 *>(mom)[p];
            u = !converged(n, m.x, m.y, T, F);
        }
    }
    const uint64_t bu = __ballot(u), bl = __ballot(lv);
    const uint32_t w = p >> 6;
    if ((threadIdx.x & 63u) == 0 && w < n_words) ubits[w] = bu, live[w] = bl;
}

// listed(p) from the three rows of u bits around p; per wave the bits and their popcount
__global__ __launch_bounds__(kSelBlock) void rtw_adapt_dilate(const unsigned long long *__restrict__ ubits,
                                                              const unsigned long long *__restrict__ live,
                                                              uint32_t npix, uint32_t n_words, uint32_t W, uint32_t rows,
                                                              unsigned long long *__restrict__ lbits,
                                                              uint32_t *__restrict__ wcount) {
    const uint32_t p = blockIdx.x * kSelBlock + threadIdx.x;
    bool listed = false;
    if (p < npix && ((live[p >> 6] >> (p & 63u)) & 1ull)) {
        const uint32_t y = p / W, x = p - y * W;
        const uint32_t x0 = x ? x - 1u : 0u, x1 = min(x + 1u, W - 1u);
        const uint32_t y0 = y ? y - 1u : 0u, y1 = min(y + 1u, rows - 1u);
        unsigned long long any = 0;
        for (uint32_t yy = y0; yy <= y1; ++yy)
            for (uint32_t xx = x0; xx <= x1; ++xx) {
                const uint32_t q = yy * W + xx;
                any |= ubits[q >> 6] >> (q & 63u);
            }
        listed = any & 1ull;
    }
    const uint64_t bl = __ballot(listed);
    const uint32_t w = p >> 6;
    if ((threadIdx.x & 63u) == 0 && w < n_words) lbits[w] = bl, wcount[w] = static_cast<uint32_t>(__builtin_popcountll(bl));
}

// exclusive scan of the per-wave counts in place, by one workgroup; the total to *n_list
__global__ __launch_bounds__(kScanBlock) void rtw_adapt_scan(uint32_t *__restrict__ wcount, uint32_t n_words,
                                                             uint32_t *__restrict__ n_list) {
    __shared__ uint32_t part[kScanBlock];
    const uint32_t tid = threadIdx.x;
    const uint32_t per = (n_words + kScanBlock - 1u) / kScanBlock;
    const uint32_t b = min(tid * per, n_words), e = min(b + per, n_words);
    uint32_t sum = 0;
    for (uint32_t i = b; i < e; ++i) sum += wcount[i];
    part[tid] = sum;
    __syncthreads();
    for (uint32_t o = 1; o < kScanBlock; o <<= 1) {  // inclusive scan of the threads' sums
        const uint32_t v = tid >= o ? part[tid - o] : 0u;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    uint32_t run = part[tid] - sum;
    for (uint32_t i = b; i < e; ++i) {
        const uint32_t c = wcount[i];
        wcount[i] = run;
        run += c;
    }
    if (tid == kScanBlock - 1u) *n_list = part[tid];
}

// each listed index at its wave's offset + its rank among the wave's listed lanes
__global__ __launch_bounds__(kSelBlock) void rtw_adapt_emit(const unsigned long long *__restrict__ lbits,
                                                            const uint32_t *__restrict__ woff, uint32_t npix,
                                                            uint32_t *__restrict__ list) {
    const uint32_t p = blockIdx.x * kSelBlock + threadIdx.x;
    if (p >= npix) return;
    const uint64_t b = lbits[p >> 6];
    if ((b >> (p & 63u)) & 1ull) list[woff[p >> 6] + rank_in(b)] = p;
}

// ---- sums to images with a per-pixel divisor: one thread per pixel
__global__ __launch_bounds__(256) void rtw_fast_resolve_counts(const unsigned long long *__restrict__ acc,
                                                               const uint32_t *__restrict__ counts, uint64_t n_pixels,
                                                               float *__restrict__ out, uint32_t *__restrict__ preview,
                                                               uint32_t n_off, unsigned long long *__restrict__ full) {
    const uint64_t p = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    const uint32_t n = p < n_pixels ? counts[p] : 0u;
    if (full) {  // wave-uniform branch: the ballot sees every lane
        const uint64_t at_end = __ballot(p < n_pixels && n >= n_off);
        if ((threadIdx.x & 63u) == 0 && at_end) atomicAdd(full, static_cast<unsigned long long>(__builtin_popcountll(at_end)));
    }
    if (p < n_pixels) resolve_pixel(acc, p, static_cast<double>(n), out, preview);
}

}  // namespace

hipError_t launch_accumulate_list(const ListParams &A_in, int n_cu, hipStream_t st, bool scene_lds) {
    ListParams A = A_in;
    // entries a wave claims per cursor atomic: about 256 samples' worth, never more than 16
    A.chunk = std::min(16u, std::max(1u, 256u / std::max(A.m, 1u)));
    // a wave starts on one pixel: no more workgroups than the shard could give work to
    if (A.f.move)
        return launch_persistent(rtw_fast_acc_list<true, true>, rtw_fast_acc_list<false, true>, A, A.f, false, 6, kWaves,
                                 kListLdsCap, n_cu, st, scene_lds);
    return launch_persistent(rtw_fast_acc_list<true, false>, rtw_fast_acc_list<false, false>, A, A.f, false, 6, kWaves,
                             kListLdsCap, n_cu, st, scene_lds);
}

hipError_t launch_resolve_counts(const unsigned long long *acc, const uint32_t *counts, uint64_t n_pixels,
                                 float *out_rgb, uint32_t *preview_rgba8, uint32_t n_off, unsigned long long *full,
                                 hipStream_t st) {
    const uint32_t blocks = static_cast<uint32_t>((n_pixels + 255) / 256);
    hipLaunchKernelGGL(rtw_fast_resolve_counts, dim3(blocks), dim3(256), 0, st, acc, counts, n_pixels, out_rgb,
                       preview_rgba8, n_off, full);
    return hipGetLastError();
}

}  // namespace rtw_fast

// ------------------------------------------------------------------- host ---
namespace {

// The selection's per-device scratch, grow-only, owned by the library: three bit planes
// (u, n < N, listed) of one u64 per 64 pixels, and the per-wave counts / offsets.
struct AdaptCtx {
    int device = 0;
    std::mutex mu;  // one call at a time per device
    char *d = nullptr;
    size_t words_cap = 0;
    hipEvent_t ev_done = nullptr;
    hipStream_t last_stream = nullptr;
    bool pending = false;  // ev_done was recorded on last_stream

    ~AdaptCtx() {
        (void)hipSetDevice(device);
        (void)hipDeviceSynchronize();
        if (d) (void)hipFree(d);
        if (ev_done) (void)hipEventDestroy(ev_done);
    }
};

std::mutex g_mu;
std::map<int, AdaptCtx *> g_ctx;

AdaptCtx *context(int device) {
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
    auto *c = new AdaptCtx();
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

int adaptive_select(int device, const uint32_t *counts, const unsigned long long *mom, uint32_t width, uint32_t rows,
                    uint32_t N, uint32_t tol_q16, uint32_t floor_q16, uint32_t *list_out, uint32_t *n_list_out,
                    hipStream_t st) {
    if (!counts || !mom || !list_out || !n_list_out) throw rtw::Error(RTW_E_ARG, "null argument");
    if (reinterpret_cast<uintptr_t>(mom) % 16) throw rtw::Error(RTW_E_ARG, "mom buffer not 16-byte aligned");
    if (N == 0 || tol_q16 > 65535u || floor_q16 > (1u << 24))
        throw rtw::Error(RTW_E_ARG, "N is 0, tol_q16 > 65535 or floor_q16 > 2^24");
    if (N > 65535u) throw rtw::Error(RTW_E_UNSUPPORTED, "adaptive fast mode: more than 65535 samples per pixel");
    if (width == 0 || rows == 0) throw rtw::Error(RTW_E_EMPTY_IMAGE, "image height and width must be > 0");
    if (static_cast<uint64_t>(width) * rows >= (1ull << 32) - (1u << 24))
        throw rtw::Error(RTW_E_UNSUPPORTED, "adaptive fast mode: image too large");
    const uint32_t npix = width * rows, n_words = (npix + 63u) / 64u;
    AdaptCtx *c = context(device);
    std::lock_guard<std::mutex> lock(c->mu);
    if (n_words > c->words_cap) {
        HIPCHECK(hipDeviceSynchronize());  // nothing in flight reads the old buffer
        if (c->d) HIPCHECK(hipFree(c->d));
        c->d = nullptr, c->words_cap = 0;
        HIPCHECK(hipMalloc(&c->d, static_cast<size_t>(n_words) * (3 * sizeof(unsigned long long) + sizeof(uint32_t))));
        c->words_cap = n_words;
    }
    // a call on another stream than the previous one waits for it on the device
    if (c->pending && c->last_stream != st) HIPCHECK(hipStreamWaitEvent(st, c->ev_done, 0));
    unsigned long long *ubits = reinterpret_cast<unsigned long long *>(c->d), *live = ubits + c->words_cap,
                       *lbits = live + c->words_cap;
    uint32_t *wcount = reinterpret_cast<uint32_t *>(lbits + c->words_cap);
    const dim3 grid((npix + rtw_fast::kSelBlock - 1u) / rtw_fast::kSelBlock), block(rtw_fast::kSelBlock);
    hipLaunchKernelGGL(rtw_fast::rtw_adapt_flag, grid, block, 0, st, counts, mom, npix, n_words, N, tol_q16, floor_q16,
                       ubits, live);
    hipLaunchKernelGGL(rtw_fast::rtw_adapt_dilate, grid, block, 0, st, ubits, live, npix, n_words, width, rows, lbits,
                       wcount);
    hipLaunchKernelGGL(rtw_fast::rtw_adapt_scan, dim3(1), dim3(rtw_fast::kScanBlock), 0, st, wcount, n_words, n_list_out);
    hipLaunchKernelGGL(rtw_fast::rtw_adapt_emit, grid, block, 0, st, lbits, wcount, npix, list_out);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipEventRecord(c->ev_done, st));
    c->last_stream = st, c->pending = true;
    return RTW_OK;
}

}  // namespace

namespace rtw {

void adapt_shutdown() {
    DeviceGuard guard;
    std::lock_guard<std::mutex> lock(g_mu);
    for (auto &kv : g_ctx) delete kv.second;
    g_ctx.clear();
}

uint32_t tol_to_q16(double v, uint32_t max) {
    if (!(v > 0.)) return 0;
    const double q = std::floor(v * 65536. + 0.5);
    return q >= static_cast<double>(max) ? max : static_cast<uint32_t>(q);
}

std::string render_adaptive_device(const Camera &cam, const Scene &world, uint32_t samples_sqrt, rtw_u128 seed,
                                   int device, double tol, double floor, uint32_t min_samples, uint32_t batch, int output,
                                   std::vector<float> *frame, rtw_adaptive_info *info, rtw_stats *stats,
                                   const rtw_denoise_params *denoise, double *denoise_ms) {
    DeviceGuard guard;
    FlatScene flat;
    world.flatten(flat);
    rtw_session *s = nullptr;
    void *d_fb = nullptr;
    auto ok = [](int64_t rc) {
        if (rc < 0) throw Error(static_cast<int>(rc), last_error());
        return rc;
    };
    try {
        ok(rtw_session_create(device, &s));
        ok(rtw_session_set_scene_moving(s, flat.spheres.data(), static_cast<uint32_t>(flat.spheres.size()),
                                        flat.moving ? flat.center1.data() : nullptr,  // null: rtw_session_set_scene
                                        flat.materials.data(), static_cast<uint32_t>(flat.materials.size())));
        const uint32_t w = cam.width(), h = cam.height();
        const uint64_t n = std::max<uint64_t>(static_cast<uint64_t>(w) * h * 3, 1);
        HIPCHECK(hipSetDevice(device));
        HIPCHECK(hipMalloc(&d_fb, n * sizeof(float)));
        if (denoise)
            ok(rtw_session_render_fast_denoised(s, &cam.d, samples_sqrt, seed, nullptr, tol_to_q16(tol, 65535u),
                                                tol_to_q16(floor, 1u << 24), min_samples, batch, denoise,
                                                static_cast<float *>(d_fb), nullptr, nullptr, nullptr, info, denoise_ms));
        else
            ok(rtw_session_render_fast_adaptive(s, &cam.d, samples_sqrt, seed, nullptr, tol_to_q16(tol, 65535u),
                                                tol_to_q16(floor, 1u << 24), min_samples, batch,
                                                static_cast<float *>(d_fb), nullptr, nullptr, info));
        if (stats) {  // the driver's totals in the shape the one-shot renders report
            *stats = rtw_stats{};
            stats->pixels = static_cast<uint64_t>(w) * h;
            stats->samples = info->samples;
            stats->kernel_ms = info->kernel_ms + info->select_ms;
            stats->main_kernel_ms = info->kernel_ms;
        }
        std::string file;
        if (output == 0) {
            frame->resize(static_cast<size_t>(w) * h * 3);
            HIPCHECK(hipMemcpy(frame->data(), d_fb, frame->size() * sizeof(float), hipMemcpyDeviceToHost));
        } else if (output == 1) {  // the PPM text made on the device
            file.assign(n * 4 + 64, '\0');
            int64_t len = ok(rtw_format_ppm_device(device, d_fb, 1, w, h, nullptr, &file[0], file.size(), nullptr));
            if (static_cast<uint64_t>(len) > file.size()) {
                file.resize(static_cast<size_t>(len));
                len = ok(rtw_format_ppm_device(device, d_fb, 1, w, h, nullptr, &file[0], file.size(), nullptr));
            }
            file.resize(static_cast<size_t>(len));
        } else {  // PNG
            const uint64_t filtered = (1 + 3ull * w) * h;
            file.assign(filtered + (filtered / kPngTile + 1) * kPngStoredHead + kPngHead + kPngTail, '\0');
            file.resize(static_cast<size_t>(ok(rtw_png_device(device, d_fb, 1, w, h, -1, nullptr, &file[0], file.size()))));
        }
        (void)hipFree(d_fb);
        rtw_session_destroy(s);
        return file;
    } catch (...) {
        if (d_fb) (void)hipFree(d_fb);
        rtw_session_destroy(s);
        throw;
    }
}

}  // namespace rtw

#define RTW_ADAPT_GUARD(body)             \
    DeviceGuard device_guard_;            \
    try {                                 \
        body;                             \
        return RTW_OK;                    \
    } catch (const rtw::Error &e) {       \
        rtw::set_error(e.what());         \
        return e.code;                    \
    } catch (const std::exception &e) {   \
        rtw::set_error(e.what());         \
        return RTW_E_ARG;                 \
    }

extern "C" {

uint32_t rtw_lattice_stride(uint32_t N) {
    if (N <= 2) return 1;
    const double x = static_cast<double>(N) * ((std::sqrt(5.) - 1.) / 2.);
    uint32_t lo = static_cast<uint32_t>(x), hi = lo + 1;  // 1 <= lo < x < hi <= N - 1 ... both ends are coprime to N
    while (rtw::gcd_u32(lo, N) != 1) --lo;
    while (rtw::gcd_u32(hi, N) != 1) ++hi;
    return x - static_cast<double>(lo) <= static_cast<double>(hi) - x ? lo : hi;
}

int rtw_adaptive_select(int device, const uint32_t *counts_device, const unsigned long long *mom_device, uint32_t width,
                        uint32_t rows, uint32_t N, uint32_t tol_q16, uint32_t floor_q16, uint32_t *list_out_device,
                        uint32_t *n_list_out_device, void *hip_stream) {
    RTW_ADAPT_GUARD(adaptive_select(device, counts_device, mom_device, width, rows, N, tol_q16, floor_q16,
                                    list_out_device, n_list_out_device, static_cast<hipStream_t>(hip_stream)))
}

int rtw_resolve_fast_counts(int device, const unsigned long long *acc_device, const uint32_t *counts_device,
                            uint32_t width, uint32_t rows, float *out_rgb_device, uint8_t *preview_rgba8_device,
                            void *hip_stream) {
    RTW_ADAPT_GUARD({
        if (!acc_device || !counts_device || (!out_rgb_device && !preview_rgba8_device))
            throw rtw::Error(RTW_E_ARG, "null argument");
        if (width == 0 || rows == 0) throw rtw::Error(RTW_E_EMPTY_IMAGE, "image height and width must be > 0");
        if (reinterpret_cast<uintptr_t>(preview_rgba8_device) % 4)
            throw rtw::Error(RTW_E_ARG, "preview buffer not 4-byte aligned");
        HIPCHECK(hipSetDevice(device));
        HIPCHECK(rtw_fast::launch_resolve_counts(acc_device, counts_device, static_cast<uint64_t>(width) * rows,
                                                 out_rgb_device, reinterpret_cast<uint32_t *>(preview_rgba8_device), 0,
                                                 nullptr, static_cast<hipStream_t>(hip_stream)));
    })
}

}  // extern "C"
