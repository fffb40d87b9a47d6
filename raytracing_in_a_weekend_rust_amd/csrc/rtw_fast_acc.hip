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

// Scene tables and the BVH into LDS behind the per-lane stacks (as rtw_fast_render).
template <bool kLds>
__device__ __forceinline__ void stage_scene(const FastParams &P, float4 *lds, uint32_t tid, const float4 *&geo,
                                            const float4 *&mat, const float4 *&nodes, const uint32_t *&kind) {
    geo = P.geo, mat = P.mat, nodes = P.nodes, kind = P.kind;
    if constexpr (kLds) {
        float4 *g = lds + P.n_stack * kBlock * sizeof(uint16_t) / sizeof(float4);
        float4 *m = g + P.n_sph, *nd = m + P.n_sph;
        uint32_t *kd = reinterpret_cast<uint32_t *>(nd + P.n_node * rtw_accel::kNodeF4);
        for (uint32_t i = tid; i < P.n_sph; i += kBlock) g[i] = P.geo[i], m[i] = P.mat[i], kd[i] = P.kind[i];
        for (uint32_t i = tid; i < P.n_node * rtw_accel::kNodeF4; i += kBlock) nd[i] = P.nodes[i];
        geo = g, mat = m, nodes = nd, kind = kd;
        __syncthreads();
    }
}

__device__ __forceinline__ uint32_t rank_in(uint64_t mask) {  // set bits of mask below this lane
    return __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(mask >> 32),
                                     __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(mask), 0u));
}

// statistics: one atomic per wave and counter (FastParams::counters)
__device__ __forceinline__ void add_counters(const FastParams &P, uint32_t lane, uint32_t segs, uint32_t visits,
                                             uint32_t written, uint32_t iters, uint32_t wvisits, bool lane_written) {
    unsigned long long sg = segs, vs = visits, wv = wvisits, wr = written;
    for (int o = 32; o > 0; o >>= 1) {
        sg += __shfl_xor(sg, o);
        vs += __shfl_xor(vs, o);
        wv += __shfl_xor(wv, o);
        if (lane_written) wr += __shfl_xor(wr, o);  // else wave-uniform already
    }
    if (lane == 0) {
        atomicAdd(P.counters + 0, sg);
        atomicAdd(P.counters + 1, vs);
        atomicAdd(P.counters + 2, wr);
        atomicAdd(P.counters + 3, static_cast<unsigned long long>(iters));
        atomicAdd(P.counters + 4, wv);
    }
}

// ---- a lane owns a pixel (k_count < kAccLaneMax)
template <bool kLds>
__global__ __launch_bounds__(kBlock, 2) void rtw_fast_acc_lane(const AccParams A) {
    extern __shared__ __attribute__((aligned(16))) float4 lds[];
    const FastParams &P = A.f;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    uint16_t *stk = reinterpret_cast<uint16_t *>(lds) + tid;  // slot j at stk[j * kBlock]
    const float4 *geo, *mat, *nodes;
    const uint32_t *kind;
    stage_scene<kLds>(P, lds, tid, geo, mat, nodes, kind);
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
            start_path(P, pix, A.k_first + ki * A.k_step, rng, g);
            tr = tg = tb = 1.f;
            depth = 0;
            path = true;
        }
        if (__ballot(path) == 0) break;  // no pixel left for any lane
        ++iters;
        // ---- one segment per busy lane
        float cr = 0.f, cg = 0.f, cb = 0.f;
        if (path && trace_segment(P, geo, mat, kind, nodes, g, rng, tr, tg, tb, depth, stk, segs, visits, wvisits, cr, cg,
                                  cb)) {
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
    add_counters(P, lane, segs, visits, written, iters, wvisits, true);
}

// ---- a wave shares a ring of pixels (k_count >= kAccLaneMax)
template <bool kLds>
__global__ __launch_bounds__(kBlock, 2) void rtw_fast_acc_ring(const AccParams A) {
    extern __shared__ __attribute__((aligned(16))) float4 lds[];
    __shared__ unsigned long long acc[kWaves][kAccRing][3];
    const FastParams &P = A.f;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint16_t *stk = reinterpret_cast<uint16_t *>(lds) + tid;
    const float4 *geo, *mat, *nodes;
    const uint32_t *kind;
    stage_scene<kLds>(P, lds, tid, geo, mat, nodes, kind);
    const uint32_t npix = P.n_rows * P.W;
    const float cmax = P.cmax;
    // wave-uniform ring state: pixel and samples in flight per slot, the slot being
    // handed out (cs), its pixel and the next sample index of it
    uint32_t pixs[kAccRing], outst[kAccRing];
#pragma unroll
    for (uint32_t s = 0; s < kAccRing; ++s) pixs[s] = kFree, outst[s] = 0;
    uint32_t cs = kFree, cur_pix = 0, next = 0;
    uint32_t claim = 0, claim_end = 0;  // the wave's pixels claimed from the cursor and not yet started
    bool exhausted = false;
    Seg g{};
    float tr = 0.f, tg = 0.f, tb = 0.f;
    uint32_t depth = 0, slot = kFree;
    Rng rng{1u, 0u};
    uint32_t segs = 0, visits = 0, written = 0, iters = 0, wvisits = 0;
    for (;;) {
        // ---- hand out samples of the newest pixel to idle lanes
        for (;;) {
            const uint64_t need = __ballot(slot == kFree);
            if (need == 0) break;
            if (cs == kFree || next >= A.k_count) {
                if (exhausted) break;
                uint32_t f = kFree;
#pragma unroll
                for (uint32_t s = 0; s < kAccRing; ++s)
                    if (f == kFree && pixs[s] == kFree) f = s;
                if (f == kFree) break;
                if (claim == claim_end) {  // A.chunk pixels per atomic: every wave draws from one address
                    uint32_t c = 0;
                    if (lane == 0) c = atomicAdd(P.cursor, A.chunk);
                    c = __builtin_amdgcn_readfirstlane(c);
                    if (c >= npix) {
                        exhausted = true;
                        break;
                    }
                    claim = c, claim_end = min(c + A.chunk, npix);
                }
                const uint32_t p = claim++;
#pragma unroll
                for (uint32_t s = 0; s < kAccRing; ++s)
                    if (s == f) pixs[s] = p, outst[s] = 0;
                if (lane < 3) acc[wave][f][lane] = 0ull;
                __builtin_amdgcn_wave_barrier();
                cs = f, cur_pix = p, next = 0;
            }
            const uint32_t rank = rank_in(need);
            const uint32_t avail = A.k_count - next;
            if (slot == kFree && rank < avail) {
                start_path(P, cur_pix, A.k_first + (next + rank) * A.k_step, rng, g);
                tr = tg = tb = 1.f;
                depth = 0;
                slot = cs;
            }
            const uint32_t took = min(static_cast<uint32_t>(__builtin_popcountll(need)), avail);
            next += took;
#pragma unroll
            for (uint32_t s = 0; s < kAccRing; ++s)
                if (s == cs) outst[s] += took;
        }
        if (__ballot(slot != kFree) == 0) break;  // nothing handed out: the shard is done
        ++iters;
        // ---- one segment per busy lane; finished samples into their pixel's sum
        float cr = 0.f, cg = 0.f, cb = 0.f;
        const bool fin = slot != kFree && trace_segment(P, geo, mat, kind, nodes, g, rng, tr, tg, tb, depth, stk, segs,
                                                        visits, wvisits, cr, cg, cb);
        if (fin) {
            unsigned long long *a = acc[wave][slot];
            atomicAdd(a + 0, to_fixed(cr, cmax));
            atomicAdd(a + 1, to_fixed(cg, cmax));
            atomicAdd(a + 2, to_fixed(cb, cmax));
        }
#pragma unroll
        for (uint32_t s = 0; s < kAccRing; ++s)
            outst[s] -= static_cast<uint32_t>(__builtin_popcountll(__ballot(fin && slot == s)));
        if (fin) slot = kFree;
        // ---- pixels whose samples are all handed out and finished: add to the buffer
#pragma unroll
        for (uint32_t s = 0; s < kAccRing; ++s) {
            if (pixs[s] != kFree && outst[s] == 0 && (s != cs || next >= A.k_count)) {
                __builtin_amdgcn_wave_barrier();
                if (lane < 3) A.acc[static_cast<uint64_t>(pixs[s]) * 3u + lane] += acc[wave][s][lane];
                pixs[s] = kFree;
                ++written;
                if (s == cs) cs = kFree;
            }
        }
    }
    add_counters(P, lane, segs, visits, written, iters, wvisits, false);
}

// ---- sums to images: one thread per pixel
__device__ __forceinline__ uint32_t preview_u8(float mean) {  // Rust's `(mean as f64 * 255.) as u8`
    const double v = static_cast<double>(mean) * 255.;
    return v >= 255. ? 255u : (v > 0. ? static_cast<uint32_t>(v) : 0u);  // NaN -> 0
}

__global__ __launch_bounds__(256) void rtw_fast_resolve(const unsigned long long *__restrict__ acc, double n,
                                                        uint64_t n_pixels, float *__restrict__ out,
                                                        uint32_t *__restrict__ preview) {
    const uint64_t p = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    if (p >= n_pixels) return;
    float m[3];
#pragma unroll
    for (uint32_t c = 0; c < 3; ++c)  // the one-shot kernel's expression (rtw_fast.hip), an IEEE f64 divide
        m[c] = static_cast<float>(static_cast<double>(acc[p * 3u + c]) * (1. / 4294967296.) / n);
    if (out) out[p * 3u + 0] = m[0], out[p * 3u + 1] = m[1], out[p * 3u + 2] = m[2];
    if (preview) preview[p] = preview_u8(m[0]) | (preview_u8(m[1]) << 8) | (preview_u8(m[2]) << 16) | 0xff000000u;
}

}  // namespace

size_t acc_lds_bytes(uint32_t n_sph, uint32_t n_node, uint32_t n_stack, bool *scene_in_lds) {
    const size_t stacks = static_cast<size_t>(n_stack) * kBlock * sizeof(uint16_t);
    const size_t scene = static_cast<size_t>(n_sph) * (2 * sizeof(float4) + sizeof(uint32_t)) +
                         static_cast<size_t>(n_node) * rtw_accel::kNodeF4 * sizeof(float4);
    *scene_in_lds = stacks + scene <= kAccLdsCap;
    return *scene_in_lds ? stacks + scene : (stacks ? stacks : 16);
}

hipError_t launch_accumulate(const AccParams &A_in, int n_cu, hipStream_t st, bool scene_lds) {
    AccParams A = A_in;
    const FastParams &P = A.f;
    // ring pixels a wave claims per cursor atomic: about 256 samples' worth, 1 from 256 samples
    // per pixel on (the one-shot kernel's hand-out), never more than 16
    A.chunk = std::min(16u, std::max(1u, 256u / std::max(A.k_count, 1u)));
    hipError_t e = hipMemsetAsync(P.cursor, 0, sizeof(uint32_t), st);
    if (e == hipSuccess) e = hipMemsetAsync(P.counters, 0, 5 * sizeof(unsigned long long), st);
    if (e != hipSuccess) return e;
    if (P.n_rows == 0 || P.W == 0 || A.k_count == 0) return hipSuccess;
    const bool by_lane = A.k_count < kAccLaneMax;
    const uint64_t npix = static_cast<uint64_t>(P.n_rows) * P.W;
    // a wave starts on 64 pixels (lane) or 1 (ring): no more workgroups than have work
    const uint64_t per_block = by_lane ? kBlock : kWaves;
    const uint32_t blocks = static_cast<uint32_t>(
        std::min<uint64_t>(static_cast<uint64_t>(n_cu > 0 ? n_cu : 256) * 2, (npix + per_block - 1) / per_block));
    bool in_lds = false;
    size_t lds = acc_lds_bytes(P.n_sph, P.n_node, P.n_stack, &in_lds);
    if (!scene_lds && in_lds) {
        in_lds = false;
        lds = P.n_stack ? static_cast<size_t>(P.n_stack) * kBlock * sizeof(uint16_t) : 16;
    }
    if (by_lane) {
        if (in_lds) hipLaunchKernelGGL(rtw_fast_acc_lane<true>, dim3(blocks), dim3(kBlock), lds, st, A);
        else hipLaunchKernelGGL(rtw_fast_acc_lane<false>, dim3(blocks), dim3(kBlock), lds, st, A);
    } else {
        if (in_lds) hipLaunchKernelGGL(rtw_fast_acc_ring<true>, dim3(blocks), dim3(kBlock), lds, st, A);
        else hipLaunchKernelGGL(rtw_fast_acc_ring<false>, dim3(blocks), dim3(kBlock), lds, st, A);
    }
    return hipGetLastError();
}

hipError_t launch_resolve(const unsigned long long *acc, uint64_t n_samples, uint64_t n_pixels, float *out_rgb,
                          uint32_t *preview_rgba8, hipStream_t st) {
    const uint32_t blocks = static_cast<uint32_t>((n_pixels + 255) / 256);
    hipLaunchKernelGGL(rtw_fast_resolve, dim3(blocks), dim3(256), 0, st, acc, static_cast<double>(n_samples), n_pixels,
                       out_rgb, preview_rgba8);
    return hipGetLastError();
}

}  // namespace rtw_fast
