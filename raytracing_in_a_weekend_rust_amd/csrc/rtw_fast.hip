// rtw_fast.hip -- f32 fast mode of the sampling path (rtw_fast.h).
//
// Same model as the parity kernel (rtw_render.hip): get_ray with the stratified
// lattice and the defocus disk (camera.rs:400-456), Scene::hit's closest sphere
// from t = 0.01 (hittable.rs:131-143, sphere.rs:39-71, camera.rs:387), the three
// materials with the reference's quirks (materials.rs:22-111: Lambertian's
// near_zero without abs, vec3.rs:246-250; Metal always scatters and always draws;
// Dielectric draws only when it can refract), black at the depth cap, the sky
// gradient on a miss (camera.rs:376-398). Differences, by design:
//   * f32 arithmetic (FMA allowed) instead of f64, so paths diverge from the
//     reference after a few bounces and the gate is statistical;
//   * random numbers: xoroshiro64** (Blackman & Vigna), one stream per
//     (global pixel, lattice sample) seeded by SplitMix64's finaliser, instead of
//     one XorShift chain per pixel (random.rs:33-69). A pixel's samples are
//     independent, so one wave traces 64 of them at once;
//   * random_unit_vec and the unit-disk sample draw their distributions directly
//     (no rejection loop, whose retries diverge across a wave);
//   * the pixel mean is summed in 32.32 fixed point (LDS u64 atomics): exact and
//     order-free, so a render is deterministic and any shard reproduces the
//     unsharded pixels bit-for-bit. Per-sample colours are clamped to [0, cmax]
//     (NaN -> 0) to keep the sum in range; the reference's scenes stay in [0, 1].
//
// Execution: a persistent grid (two 512-thread workgroups per CU, scene tables +
// BVH in LDS). Each wave takes pixels from a global counter and keeps a ring of
// up to kRing pixels in flight: a lane whose path ends starts the next sample of
// the newest pixel at once, so lanes stay busy until the image runs out. A pixel
// is written when all its samples are handed out and finished. The scheduler and
// the per-sample code are rtw_fast_dev.h's; this file says what the one-shot render
// claims (one pixel per cursor atomic, the whole lattice) and writes (the f32 mean).
#include "rtw_fast.h"

#include "rtw_fast_dev.h"

namespace rtw_fast {
namespace {

struct OneShot : RgbSums {
    struct Job {
        uint32_t pix;
    };
    static constexpr uint32_t kRing = 4;
    const FastParams &P;
    const uint32_t npix;
    __device__ __forceinline__ Claim claim(uint32_t lane, Job &j) const {
        uint32_t p = 0;
        if (lane == 0) p = atomicAdd(P.cursor, 1u);
        j.pix = __builtin_amdgcn_readfirstlane(p);
        return j.pix < npix ? Claim::kJob : Claim::kDone;
    }
    __device__ __forceinline__ uint32_t count(const Job &) const { return P.n_off; }
    __device__ __forceinline__ uint32_t lattice(const Job &, uint32_t i) const { return i; }
    __device__ __forceinline__ void flush(uint32_t lane, const Job &j, const unsigned long long *a) const {
        if (lane < 3) P.out[static_cast<uint64_t>(j.pix) * 3u + lane] = mean_f32(a[lane], static_cast<double>(P.n_off));
    }
};

// kMove: the motion-blur instantiation (rtw_fast_dev.h: Motion)
template <bool kLds, bool kMove>
__global__ __launch_bounds__(kBlock, 2) void rtw_fast_render(const FastParams P) {
    OneShot u{{}, P, P.n_rows * P.W};
    uint32_t written;
    const WaveStats w = run_ring<kLds, kMove>(P, u, written);
    add_counters(P, threadIdx.x & 63u, w, written, false);
}

}  // namespace

size_t lds_bytes(uint32_t n_sph, uint32_t n_node, uint32_t n_stack, uint32_t cap, bool *scene_in_lds,
                 uint32_t n_mov) {
    const size_t stacks = static_cast<size_t>(n_stack) * kBlock * sizeof(uint16_t);
    const size_t scene = static_cast<size_t>(n_sph) * (2 * sizeof(float4) + sizeof(uint32_t)) +
                         static_cast<size_t>(n_node) * rtw_accel::kNodeF4 * sizeof(float4) +
                         static_cast<size_t>(n_mov) * sizeof(float4);
    *scene_in_lds = stacks + scene <= cap;
    return *scene_in_lds ? stacks + scene : (stacks ? stacks : 16);
}

hipError_t launch(const FastParams &P, int n_cu, hipStream_t st, bool scene_lds) {
    // a wave starts on one pixel: no more workgroups than have work
    const bool nothing = P.n_rows == 0 || P.W == 0;
    if (P.move)
        return launch_persistent(rtw_fast_render<true, true>, rtw_fast_render<false, true>, P, P, nothing, 5, kWaves,
                                 kLdsCap, n_cu, st, scene_lds);
    return launch_persistent(rtw_fast_render<true, false>, rtw_fast_render<false, false>, P, P, nothing, 5, kWaves,
                             kLdsCap, n_cu, st, scene_lds);
}

}  // namespace rtw_fast
