// rtw_fast.h -- the f32 "fast mode" render: the same camera,
// scene, materials and depth rule as the reference's ray_color (camera.rs:376-398),
// computed in f32 with independent random streams per (pixel, sample), so that a
// pixel's samples run in parallel instead of as one serial chain. Not bit-exact
// by design: its gate is statistical against the f64 parity render.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace rtw_fast {

// Launch parameters (host-derived camera values as f32; scene tables on device).
struct FastParams {
    float p00[3], du[3], dv[3];  // get_ray: pixel_loc = (pixel00 + i du) + j dv
    float from[3], ddu[3], ddv[3];  // look_from, defocus disk basis
    float pos0[3], ldx[3], ldy[3];  // offset_lattice (camera.rs:422-450)
    uint32_t defocus;               // 1: origins on the defocus disk (camera.rs:406-410)
    uint32_t W, s, n_off, max_depth;
    uint32_t row_begin, row_step, n_rows;
    uint32_t n_sph, n_node, n_always;
    uint32_t n_stack;  // per-lane stack slots (stack_slots(depth)); 0 with n_node = 0
    float cmax;        // per-sample colour clamp of the fixed-point sum (2^32 n_off cmax < 2^63)
    uint64_t seed_mix; // render seed folded to 64 bits
    const float4 *geo;      // {cx, cy, cz, r} per sphere
    const float4 *mat;      // Lambertian/Metal {albedo, fuzz}; Dielectric {1/ir, ir, r0^2, 0}
    const uint32_t *kind;   // RTW_LAMBERTIAN / RTW_METAL / RTW_DIELECTRIC per sphere
    const float4 *nodes;    // rtw_accel.h 4-wide nodes (n_node = 0: brute-force scan)
    const uint32_t *always; // spheres tested before the walk (rtw_accel.h)
    float *out;             // n_rows x W x 3 f32
    uint32_t *cursor;       // pixel hand-out counter (zeroed by the launcher)
    unsigned long long *counters;  // [0] segments, [1] node visits, [2] pixels written, [3] wave iterations,
                                   // [4] wave-level walk iterations
    // motion blur (last, so every field above keeps its offset): the moving kernels
    // run when move != 0; bits 8..23 of a mover's kind word hold its row of vel plus one
    const float4 *vel;   // {vx, vy, vz, 0} per moving sphere, v = f32(center1 - center0)
    uint32_t n_mov;      // rows of vel
    uint32_t t_stride;   // rtw_lattice_stride(n_off): sample k's time stratum is (k t_stride) mod n_off
    uint32_t move, _pad;
};

constexpr uint32_t kBlock = 512;   // 8 waves per workgroup, two per CU (LDS-bound: 640 measured 25% slower)
constexpr uint32_t kMaxStack = 32;  // per-lane BVH stack cap (u16 node ids)
constexpr uint32_t kLdsCap = 79 * 1024;  // two workgroups per CU (160 KB), with the static ring sums

// Stack slots a walk of a BVH of this depth needs: 3 pending siblings per level
// + the top write (the root is level 0). Deeper trees than kMaxStack allows scan.
// The scene tables follow the stacks: n_stack x kBlock x 2 bytes stays 16-aligned.
static_assert(kBlock % 8 == 0, "stack area alignment");
constexpr uint32_t stack_slots(uint32_t depth) { return 3 * depth + 2; }

// Dynamic LDS bytes of a launch: the stacks, plus the scene tables when both fit below
// the kernel's cap (*scene_in_lds; kLdsCap, kAccLdsCap, kListLdsCap); otherwise the kernel
// reads the scene from global memory. n_mov: the velocity rows a moving launch stages too.
size_t lds_bytes(uint32_t n_sph, uint32_t n_node, uint32_t n_stack, uint32_t cap, bool *scene_in_lds,
                 uint32_t n_mov = 0);

// Enqueues the render (zeroes the cursor and counters first).
hipError_t launch(const FastParams &P, int n_cu, hipStream_t st, bool scene_lds = true);

// ---- progressive accumulation (rtw_fast_acc.hip)
// Lattice samples k_first + i k_step (i < k_count) of every pixel of the shard, added
// to the caller's 32.32 fixed-point sums. f.out is unused; f.n_off and f.cmax are the
// whole lattice's, so a sample has the bits it has in the one-shot render.
struct AccParams {
    FastParams f;
    uint32_t k_first, k_step, k_count;
    uint32_t chunk;  // ring: pixels a wave claims per cursor atomic (set by launch_accumulate)
    unsigned long long *acc;  // n_rows x W x 3 u64
};

// Below this k_count a lane owns a whole pixel (sums in registers); from it on, a wave
// shares a ring of kAccRing pixels (sums in LDS), kAccRing * kAccLaneMax >= 2 x 64 lanes.
constexpr uint32_t kAccLaneMax = 16;
constexpr uint32_t kAccRing = 8;
// two workgroups per CU with the ring sums (8 waves x kAccRing x 3 u64) beside them
constexpr uint32_t kAccLdsCap = 80 * 1024 - (kBlock / 64) * kAccRing * 3 * 8;

// Enqueues the accumulation (zeroes the cursor and counters first); k_count = 0 launches nothing.
hipError_t launch_accumulate(const AccParams &A, int n_cu, hipStream_t st, bool scene_lds = true);

// Sums to the f32 mean frame and/or the linear RGBA8 preview (either may be null).
hipError_t launch_resolve(const unsigned long long *acc, uint64_t n_samples, uint64_t n_pixels, float *out_rgb,
                          uint32_t *preview_rgba8, hipStream_t st);

}  // namespace rtw_fast
