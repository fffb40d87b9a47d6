// rtw_fast_acc.hip -- progressive fast mode: a subset of the lattice samples of every
// pixel added to caller-owned 32.32 fixed-point sums, and the resolve of those sums to
// the f32 mean frame and a linear RGBA8 preview (rtw_session_accumulate_fast,
// rtw_resolve_fast). A sample's colour depends only on (seed, global pixel, k) and the
// sums are integers, so any split of the lattice into passes adds up to the one-shot
// render's sums bit for bit (rtw_fast.hip; the per-sample code is rtw_fast_dev.h).
//
// The work item is one sample, and a pass of k_count samples per pixel must fill a
// wave's 64 lanes whether k_count is 1 or 529. The one-shot kernel's ring of 4 pixels
// fills 4 k_count lanes; a ring wide enough for k_count = 1 needs 64 pixels x 3 u64 =
// 1.5 KB of sums per wave, 12 KB per workgroup, and the final scene leaves 9.7 KB
// beside its tables and stacks with two workgroups on a CU. So the sums live where
// there is room for them:
//   * k_count < kAccLaneMax: a lane owns a pixel. It traces the pixel's k_count samples
//     one after the other with the sums in six registers, adds them to the buffer
//     (it is the pixel's only writer: a plain read-add-write) and takes the next pixel
//     from the global cursor. Idle lanes of a wave draw their pixels with one atomic.
//     No LDS beside the scene, no ring state, every lane busy while pixels remain.
//   * k_count >= kAccLaneMax: a wave shares a ring of kAccRing pixels as the one-shot
//     kernel does (wave-uniform ring state in scalar registers, sums in LDS under u64
//     atomics); 8 x 16 samples are two waves' worth, so a lane whose path ends finds the
//     next sample at once. The cursor is one address for every wave and its atomics
//     serialise (12 ns each measured: 9.8 ms for the 810 000 pixels of the bench image,
//     the one-shot kernel's floor below 120 samples per pixel), so a wave claims pixels
//     in chunks of about 256 samples' worth. A finished pixel's three sums are added to
//     the buffer by three lanes: a pixel belongs to one wave per launch, so again no HBM
//     atomics.
#include <algorithm>

#include "rtw_fast_dev.h"

namespace rtw_fast {
namespace {

// ---- a lane owns a pixel (k_count < kAccLaneMax)
template <bool kLds, bool kMove>
__global__ __launch_bounds__(kBlock, 2) void rtw_fast_acc_lane(const AccParams A) {
    extern __shared__ __attribute__((aligned(16))) float4 lds[];
    const FastParams &P = A.f;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    uint16_t *stk = reinterpret_cast<uint16_t *>(lds) + tid;  // slot j at stk[j * kBlock]
    const float4 *geo, *mat, *nodes;
    const uint32_t *kind;
    Motion mo{};  // kMove: the velocity rows and the time of the lane's sample (rtw_fast_dev.h)
    stage_scene<kLds, kMove>(P, lds, tid, geo, mat, nodes, kind, &mo.vel);
    mo.kind = kind;
    const uint64_t npix = static_cast<uint64_t>(P.n_rows) * P.W;
    const float cmax = P.cmax;
    bool exhausted = false;  // wave-uniform: the cursor has passed the last pixel
    // lane state: its pixel, the index of the sample in flight, the pixel's sums
    uint32_t pix = kFree, ki = 0;
    bool path = false;
    unsigned long long sr = 0, sg = 0, sb = 0;
    Seg g{};
    float tr = 0.f, tg = 0.f, tb = 0.f;
    uint32_t depth = 0;
    Rng rng{1u, 0u};
    uint32_t segs = 0, visits = 0, written = 0, iters = 0, wvisits = 0;
    for (;;) {
        // ---- idle lanes draw consecutive pixels with one atomic
        if (!exhausted) {
            const uint64_t need = __ballot(pix == kFree);
            if (need) {
                const uint32_t cnt = static_cast<uint32_t>(__builtin_popcountll(need));
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(P.cursor, cnt);
                base = __builtin_amdgcn_readfirstlane(base);
                const uint64_t mine = static_cast<uint64_t>(base) + rank_in(need);
                if (pix == kFree && mine < npix) pix = static_cast<uint32_t>(mine), ki = 0, sr = sg = sb = 0;
                exhausted = static_cast<uint64_t>(base) + cnt >= npix;
            }
        }
        if (pix != kFree && !path) {
            start_path<kMove>(P, pix, A.k_first + ki * A.k_step, rng, g, &mo.t);
            tr = tg = tb = 1.f;
            depth = 0;
            path = true;
        }
        if (__ballot(path) == 0) break;  // no pixel left for any lane
        ++iters;
        // ---- one segment per busy lane
        float cr = 0.f, cg = 0.f, cb = 0.f;
        if (path && trace_segment<kMove>(P, geo, mat, kind, nodes, g, rng, tr, tg, tb, depth, stk, segs, visits, wvisits,
                                         cr, cg, cb, mo)) {
            sr += to_fixed(cr, cmax), sg += to_fixed(cg, cmax), sb += to_fixed(cb, cmax);
            path = false;
            if (++ki == A.k_count) {  // the pixel's only writer in this launch
                unsigned long long *d = A.acc + static_cast<uint64_t>(pix) * 3u;
                d[0] += sr, d[1] += sg, d[2] += sb;
                pix = kFree;
                ++written;
            }
        }
    }
    add_counters(P, lane, WaveStats{segs, visits, iters, wvisits}, written, true);
}

// ---- a wave shares a ring of pixels (k_count >= kAccLaneMax): rtw_fast_dev.h's scheduler;
// chunked pixels, the pass's samples, and the three sums added to the buffer by three lanes
struct Pass : RgbSums {
    struct Job {
        uint32_t pix;
    };
    static constexpr uint32_t kRing = kAccRing;
    const AccParams &A;
    const uint32_t npix;
    ChunkCursor cursor;
    __device__ __forceinline__ Claim claim(uint32_t lane, Job &j) {
        return cursor.next(A.f, lane, A.chunk, npix, j.pix) ? Claim::kJob : Claim::kDone;
    }
    __device__ __forceinline__ uint32_t count(const Job &) const { return A.k_count; }
    __device__ __forceinline__ uint32_t lattice(const Job &, uint32_t i) const { return A.k_first + i * A.k_step; }
    __device__ __forceinline__ void flush(uint32_t lane, const Job &j, const unsigned long long *a) const {
        if (lane < 3) A.acc[static_cast<uint64_t>(j.pix) * 3u + lane] += a[lane];
    }
};

template <bool kLds, bool kMove>
__global__ __launch_bounds__(kBlock, 2) void rtw_fast_acc_ring(const AccParams A) {
    Pass u{{}, A, A.f.n_rows * A.f.W, {}};
    uint32_t written;
    const WaveStats w = run_ring<kLds, kMove>(A.f, u, written);
    add_counters(A.f, threadIdx.x & 63u, w, written, false);
}

// ---- sums to images: one thread per pixel
__global__ __launch_bounds__(256) void rtw_fast_resolve(const unsigned long long *__restrict__ acc, double n,
                                                        uint64_t n_pixels, float *__restrict__ out,
                                                        uint32_t *__restrict__ preview) {
    const uint64_t p = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    if (p < n_pixels) resolve_pixel(acc, p, n, out, preview);
}

}  // namespace

hipError_t launch_accumulate(const AccParams &A_in, int n_cu, hipStream_t st, bool scene_lds) {
    AccParams A = A_in;
    const FastParams &P = A.f;
    // ring pixels a wave claims per cursor atomic: about 256 samples' worth, 1 from 256 samples
    // per pixel on (the one-shot kernel's hand-out), never more than 16
    A.chunk = std::min(16u, std::max(1u, 256u / std::max(A.k_count, 1u)));
    const bool nothing = P.n_rows == 0 || P.W == 0 || A.k_count == 0;
    // a wave starts on 64 pixels (lane) or 1 (ring): no more workgroups than have work
    const bool lane = A.k_count < kAccLaneMax;
    if (P.move)
        return launch_persistent(lane ? rtw_fast_acc_lane<true, true> : rtw_fast_acc_ring<true, true>,
                                 lane ? rtw_fast_acc_lane<false, true> : rtw_fast_acc_ring<false, true>, A, P, nothing, 5,
                                 lane ? kBlock : kWaves, kAccLdsCap, n_cu, st, scene_lds);
    return launch_persistent(lane ? rtw_fast_acc_lane<true, false> : rtw_fast_acc_ring<true, false>,
                             lane ? rtw_fast_acc_lane<false, false> : rtw_fast_acc_ring<false, false>, A, P, nothing, 5,
                             lane ? kBlock : kWaves, kAccLdsCap, n_cu, st, scene_lds);
}

hipError_t launch_resolve(const unsigned long long *acc, uint64_t n_samples, uint64_t n_pixels, float *out_rgb,
                          uint32_t *preview_rgba8, hipStream_t st) {
    const uint32_t blocks = static_cast<uint32_t>((n_pixels + 255) / 256);
    hipLaunchKernelGGL(rtw_fast_resolve, dim3(blocks), dim3(256), 0, st, acc, static_cast<double>(n_samples), n_pixels,
                       out_rgb, preview_rgba8);
    return hipGetLastError();
}

}  // namespace rtw_fast
