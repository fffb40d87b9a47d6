// rtw_fast_dev.h -- device code shared by every fast-mode kernel (rtw_fast.hip, the one-shot
// render; rtw_fast_acc.hip, the progressive accumulate; rtw_fast_adapt.hip, the adaptive list
// accumulate): random streams, get_ray, the closest hit, the shading step and the fixed-point
// clamp, the staging of the scene into LDS, the ring scheduler of the three kernels that keep
// a wave's pixels in a ring, the counters, the resolve of sums to a pixel, and the launch.
// One definition of each, called and not copied, so a sample has the same bits on every route.
#pragma once

#include <algorithm>

#include "rtw_accel.h"
#include "rtw_capi.h"
#include "rtw_fast.h"

namespace rtw_fast {
namespace {

constexpr uint32_t kWaves = kBlock / 64;
constexpr uint32_t kFree = 0xffffffffu;

struct Rng {
    uint32_t a, b;
};

__device__ __forceinline__ uint64_t fmix64(uint64_t z) {  // SplitMix64's finaliser
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ Rng rng_for(uint64_t mix, uint64_t pix, uint32_t k) {
    const uint64_t z = fmix64(fmix64(mix ^ (pix * 0x9e3779b97f4a7c15ull)) + k);
    Rng r{static_cast<uint32_t>(z), static_cast<uint32_t>(z >> 32)};
    if ((r.a | r.b) == 0u) r.a = 1u;
    return r;
}
// xoroshiro64**
__device__ __forceinline__ uint32_t rnext(Rng &r) {
    const uint32_t s0 = r.a;
    uint32_t s1 = r.b;
    const uint32_t res = __builtin_rotateleft32(s0 * 0x9E3779BBu, 5) * 5u;
    s1 ^= s0;
    r.a = __builtin_rotateleft32(s0, 26) ^ s1 ^ (s1 << 9);
    r.b = __builtin_rotateleft32(s1, 13);
    return res;
}
// next_bound(-1, 1) (random.rs:54-59) on a 24-bit uniform; next_01 (40-52)
__device__ __forceinline__ float rcoord(Rng &r) {
    return fmaf(static_cast<float>(rnext(r) >> 8), 1.1920928955078125e-07f, -1.f);  // 2^-23
}
__device__ __forceinline__ float r01(Rng &r) {
    return static_cast<float>(rnext(r) >> 8) * 5.9604644775390625e-08f;  // 2^-24
}
// random_unit_vec (vec3.rs:219-232) draws uniformly on the unit sphere by rejection;
// fast mode draws the same distribution directly (z uniform in [-1, 1], azimuth
// uniform: Archimedes), with no divergent retry loop. v_sin/v_cos take revolutions.
__device__ __forceinline__ void unit_vec(Rng &r, float &x, float &y, float &z) {
    z = rcoord(r);
    const float t = r01(r);
    const float s = __builtin_sqrtf(fmaxf(fmaf(-z, z, 1.f), 0.f));
    x = s * __builtin_amdgcn_cosf(t), y = s * __builtin_amdgcn_sinf(t);
}
// random_vec_in_unit_disk (vec3.rs:270-277), uniform in the open disk, directly
__device__ __forceinline__ void disk_vec(Rng &r, float &x, float &y) {
    const float rad = __builtin_sqrtf(r01(r)), t = r01(r);
    x = rad * __builtin_amdgcn_cosf(t), y = rad * __builtin_amdgcn_sinf(t);
}

// A segment: origin, unit direction, t_min = 0.01 |d| in distance units.
struct Seg {
    float ox, oy, oz, ex, ey, ez, tmin;
};

// Motion blur. A sample has a time t in [0, 1), one register per lane for the
// whole path, and a moving sphere is at c(t) = fmaf(t, v, c0) per component: sphere_at is the
// one expression, used by the closest hit and by the shading normal alike. Only movers have a
// velocity: bits 8..23 of a sphere's kind word hold its row of the velocity table plus one
// (0: the sphere stands still, and its record is the static kernels'). The static
// instantiations (kMove = false) read neither the word nor the table nor t.
struct Motion {
    const uint32_t *kind;
    const float4 *vel;
    float t;
};
constexpr uint32_t kKindMask = 3u;  // the material of a kind word

template <bool kMove>
__device__ __forceinline__ float4 sphere_at(const float4 *__restrict__ geo, const Motion &mo, uint32_t i) {
    float4 S = geo[i];
    if constexpr (kMove) {
        const uint32_t m = (mo.kind[i] >> 8) & 0xffffu;
        if (m) {
            const float4 V = mo.vel[m - 1u];
            S.x = fmaf(mo.t, V.x, S.x), S.y = fmaf(mo.t, V.y, S.y), S.z = fmaf(mo.t, V.z, S.z);
        }
    }
    return S;
}

// The time of lattice sample k of global pixel gpix (rtw_capi.h, rtw_fast_sample_time): the
// stratum j = (k g) mod N of [0, 1) rotated by a hash of the pixel. g = P.t_stride and
// N = P.n_off are wave-uniform; nothing is drawn from the sample's stream.
__device__ __forceinline__ float sample_time(const FastParams &P, uint64_t gpix, uint32_t k) {
    const uint32_t N = P.n_off;
    const uint32_t j = static_cast<uint32_t>(static_cast<uint64_t>(k) * P.t_stride % N);
    const uint32_t base = static_cast<uint32_t>(((2ull * j + 1ull) << 23) / N);
    const uint64_t h = fmix64(fmix64(P.seed_mix ^ (gpix * 0x9e3779b97f4a7c15ull)) + (1ull << 32)) >> 40;
    const uint32_t t24 = (base + static_cast<uint32_t>(h)) & 0xffffffu;
    return static_cast<float>(t24) * 5.9604644775390625e-08f;  // 2^-24: exact
}

// Sphere::hit (sphere.rs:39-71) in distance units along the unit direction, with
// the discriminant from the closest-approach vector (r^2 - |oc - hb e|^2: no
// cancellation against |oc|^2 for big spheres) and the stable root pair.
__device__ __forceinline__ void sphere_test(const float4 S, int i, const Seg &g, float &best, int &hid) {
    const float ocx = g.ox - S.x, ocy = g.oy - S.y, ocz = g.oz - S.z;
    const float hb = fmaf(ocx, g.ex, fmaf(ocy, g.ey, ocz * g.ez));
    const float lx = fmaf(-hb, g.ex, ocx), ly = fmaf(-hb, g.ey, ocy), lz = fmaf(-hb, g.ez, ocz);
    const float rr = S.w * S.w;
    const float disc = rr - fmaf(lx, lx, fmaf(ly, ly, lz * lz));
    if (!(disc >= 0.f)) return;
    const float sq = __builtin_sqrtf(disc);
    const float c = fmaf(ocx, ocx, fmaf(ocy, ocy, fmaf(ocz, ocz, -rr)));
    const float q = -hb - copysignf(sq, hb);
    const float t0 = c * __builtin_amdgcn_rcpf(q), t1 = q;
    const float tn = fminf(t0, t1), tf = fmaxf(t0, t1);
    const float t = tn >= g.tmin ? tn : tf;
    if (t >= g.tmin && t < best) best = t, hid = i;
}

// Per-segment slab setup for the 4-wide BVH of rtw_accel.h (its boxes are
// padded for the parity walk; that padding only adds a few box hits here).
__device__ __forceinline__ void walk_ray(const Seg &g, rtw_accel::WalkRay &r) {
    using namespace rtw_accel;
    const float mo = fmax3(fabsf(g.ox), fabsf(g.oy), fabsf(g.oz));
    r.ox = g.ox, r.oy = g.oy, r.oz = g.oz, r.ex = g.ex, r.ey = g.ey, r.ez = g.ez;
    r.neg = (g.ex < 0.f ? 1u : 0u) | (g.ey < 0.f ? 2u : 0u) | (g.ez < 0.f ? 4u : 0u);
    r.ix = rcp32(clamp_dir(g.ex)), r.iy = rcp32(clamp_dir(g.ey)), r.iz = rcp32(clamp_dir(g.ez));
    const float pad = kPadK * mo + 1e-30f;
    const float alx = -(g.ox + pad) * r.ix, ahx = -(g.ox - pad) * r.ix;
    const float aly = -(g.oy + pad) * r.iy, ahy = -(g.oy - pad) * r.iy;
    const float alz = -(g.oz + pad) * r.iz, ahz = -(g.oz - pad) * r.iz;
    const bool nx = r.neg & 1u, ny = r.neg & 2u, nz = r.neg & 4u;
    r.anx = nx ? ahx : alx, r.afx = nx ? alx : ahx;
    r.any = ny ? ahy : aly, r.afy = ny ? aly : ahy;
    r.anz = nz ? ahz : alz, r.afz = nz ? alz : ahz;
    r.tmin = g.tmin * 0.999f;
    r.negG = 0.f;
}

// Closest hit: the "always" spheres, then the BVH walk testing leaf spheres as
// they are reached (the running best is the walk's cut), or a linear scan.
template <bool kMove = false>
__device__ __forceinline__ void scene_hit(const FastParams &P, const float4 *__restrict__ geo,
                                          const float4 *__restrict__ nodes, const Seg &g, float &best,
                                          int &hid, uint16_t *stk, uint32_t &visits, uint32_t &wvisits,
                                          const Motion &mo = Motion{}) {
    best = INFINITY, hid = -1;
    if (P.n_node == 0) {
        for (uint32_t i = 0; i < P.n_sph; ++i) sphere_test(sphere_at<kMove>(geo, mo, i), static_cast<int>(i), g, best, hid);
        return;
    }
    for (uint32_t a = 0; a < P.n_always; ++a) {
        const uint32_t i = P.always[a];
        sphere_test(sphere_at<kMove>(geo, mo, i), static_cast<int>(i), g, best, hid);
    }
    if (!(rtw_accel::fmax3(fabsf(g.ox), fabsf(g.oy), fabsf(g.oz)) <= rtw_accel::kGuardBvh)) {
        for (uint32_t i = 0; i < P.n_sph; ++i) sphere_test(sphere_at<kMove>(geo, mo, i), static_cast<int>(i), g, best, hid);
        return;
    }
    rtw_accel::WalkRay r;
    walk_ray(g, r);
    const uint32_t sx = r.neg & 1u, sy = (r.neg >> 1) & 1u, sz = r.neg >> 2;
    const uint32_t oct_shift = 8u * (r.neg & 3u);
    const bool oct_hi = r.neg >= 4u;
    uint16_t *top = stk;
    uint32_t cur = 0;
    for (;;) {
        ++visits;
#ifdef RTW_FAST_DIAG
        // wave-level walk iterations, counted by the first active lane (diagnostic
        // builds: the count costs 2%; 9.4 per wave-iteration against 5.4 visits per lane)
        if (static_cast<int>(__lane_id()) == __builtin_ctzll(__builtin_amdgcn_read_exec())) ++wvisits;
#endif
        uint32_t off;
        asm("v_mul_u32_u24 %0, 0x90, %1" : "=v"(off) : "v"(cur));
        const float4 *N = reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(nodes) + off);
        const float4 nX = N[sx], fX = N[sx ^ 1u], nY = N[2u + sy], fY = N[3u - sy], nZ = N[4u + sz],
                     fZ = N[5u - sz], qc = N[6], qo = N[7];
        uint32_t hit = 0;
        hit |= rtw_accel::slab_hit4(nX, nY, nZ, fX, fY, fZ, r, best);
        const uint32_t r01w = rtw_accel::as_u32(qc.x), r23w = rtw_accel::as_u32(qc.y);
        const uint32_t masks = rtw_accel::as_u32(qc.z);
        hit &= masks;
        uint32_t lmask = hit & (masks >> 4);
        const uint32_t inner = hit & ~lmask & 15u;
        while (lmask) {
            const uint32_t j = static_cast<uint32_t>(__builtin_ctz(lmask));
            lmask &= lmask - 1u;
            const uint32_t k = ((j & 2u ? r23w : r01w) >> (16u * (j & 1u))) & 0xffffu;
            sphere_test(sphere_at<kMove>(geo, mo, k), static_cast<int>(k), g, best, hid);
        }
        const uint32_t ord = ((oct_hi ? rtw_accel::as_u32(qo.y) : rtw_accel::as_u32(qo.x)) >> oct_shift) & 0xffu;
        const uint64_t refs = (static_cast<uint64_t>(r23w) << 32) | r01w;
        for (int t = 3; t >= 0; --t) {  // far to near: the nearest ends on top
            const uint32_t j = (ord >> (2 * t)) & 3u;
            *top = static_cast<uint16_t>(refs >> (16u * j));
            top += __builtin_amdgcn_ubfe(inner, j, 1u) * kBlock;
        }
        if (top == stk) break;
        top -= kBlock;
        cur = *top;
    }
}

// get_ray (camera.rs:400-420) for lattice sample k of shard pixel pix: seeds the
// sample's stream and sets the primary segment; a moving launch also gets the sample's time.
template <bool kMove = false>
__device__ __forceinline__ void start_path(const FastParams &P, uint32_t pix, uint32_t k, Rng &rng, Seg &g,
                                           float *t = nullptr) {
    const uint32_t lr = pix / P.W, x = pix - lr * P.W;
    const uint32_t y = P.row_begin + lr * P.row_step;
    rng = rng_for(P.seed_mix, static_cast<uint64_t>(y) * P.W + x, k);
    if constexpr (kMove) *t = sample_time(P, static_cast<uint64_t>(y) * P.W + x, k);
    const float fx = static_cast<float>(x), fy = static_cast<float>(y);
    float sx = fmaf(P.dv[0], fy, fmaf(P.du[0], fx, P.p00[0]));
    float sy = fmaf(P.dv[1], fy, fmaf(P.du[1], fx, P.p00[1]));
    float sz = fmaf(P.dv[2], fy, fmaf(P.du[2], fx, P.p00[2]));
    if (P.s == 0) {
        sx += P.pos0[0], sy += P.pos0[1], sz += P.pos0[2];
    } else {
        const uint32_t ly = k / P.s, lx = k - ly * P.s;
        const float fly = static_cast<float>(ly), flx = static_cast<float>(lx);
        sx += fmaf(P.ldx[0], flx, fmaf(P.ldy[0], fly, P.pos0[0]));
        sy += fmaf(P.ldx[1], flx, fmaf(P.ldy[1], fly, P.pos0[1]));
        sz += fmaf(P.ldx[2], flx, fmaf(P.ldy[2], fly, P.pos0[2]));
    }
    g.ox = P.from[0], g.oy = P.from[1], g.oz = P.from[2];
    if (P.defocus) {  // defocus_disk_sample (camera.rs:452-456)
        float px, py;
        disk_vec(rng, px, py);
        g.ox = fmaf(P.ddv[0], py, fmaf(P.ddu[0], px, g.ox));
        g.oy = fmaf(P.ddv[1], py, fmaf(P.ddu[1], px, g.oy));
        g.oz = fmaf(P.ddv[2], py, fmaf(P.ddu[2], px, g.oz));
    }
    const float dx = sx - g.ox, dy = sy - g.oy, dz = sz - g.oz;
    const float sa = __builtin_sqrtf(fmaf(dx, dx, fmaf(dy, dy, dz * dz)));
    const float inv = __builtin_amdgcn_rcpf(sa);
    g.ex = dx * inv, g.ey = dy * inv, g.ez = dz * inv, g.tmin = 0.01f * sa;
}

// One segment of a lane's path (camera.rs:376-398): true when the path ends, with
// its colour in (cr, cg, cb); otherwise the next segment is in g.
template <bool kMove = false>
__device__ __forceinline__ bool trace_segment(const FastParams &P, const float4 *__restrict__ geo,
                                              const float4 *__restrict__ mat, const uint32_t *__restrict__ kind,
                                              const float4 *__restrict__ nodes, Seg &g, Rng &rng, float &tr,
                                              float &tg, float &tb, uint32_t &depth, uint16_t *stk, uint32_t &segs,
                                              uint32_t &visits, uint32_t &wvisits, float &cr, float &cg, float &cb,
                                              const Motion &mo = Motion{}) {
    if (depth >= P.max_depth) return true;  // black at the depth cap
    float best;
    int hid;
    ++segs;
    scene_hit<kMove>(P, geo, nodes, g, best, hid, stk, visits, wvisits, mo);
    if (hid < 0) {
        const float a = 0.5f * (g.ey + 1.f);  // sky (camera.rs:392-396)
        cr = tr * ((1.f - a) + a * 0.5f), cg = tg * ((1.f - a) + a * 0.7f), cb = tb;
        return true;
    }
    const float4 S = sphere_at<kMove>(geo, mo, static_cast<uint32_t>(hid)), M = mat[hid];
    const uint32_t kd = kMove ? kind[hid] & kKindMask : kind[hid];
    const float px = fmaf(best, g.ex, g.ox), py = fmaf(best, g.ey, g.oy), pz = fmaf(best, g.ez, g.oz);
    const float ir = __builtin_amdgcn_rcpf(S.w);
    float nx = (px - S.x) * ir, ny = (py - S.y) * ir, nz = (pz - S.z) * ir;
    const bool front = fmaf(g.ex, nx, fmaf(g.ey, ny, g.ez * nz)) < 0.f;  // hittable.rs:64-81
    if (!front) nx = -nx, ny = -ny, nz = -nz;
    const float en = fmaf(g.ex, nx, fmaf(g.ey, ny, g.ez * nz));
    // reflect(unit(dir), n) (vec3.rs:252-257)
    const float rx = fmaf(-2.f * en, nx, g.ex), ry = fmaf(-2.f * en, ny, g.ey), rz = fmaf(-2.f * en, nz, g.ez);
    float dx, dy, dz;
    if (kd != RTW_DIELECTRIC) {
        float ux, uy, uz;
        unit_vec(rng, ux, uy, uz);
        if (kd == RTW_LAMBERTIAN) {  // materials.rs:22-37, near_zero without abs
            dx = nx + ux, dy = ny + uy, dz = nz + uz;
            if (dx < 1e-8f && dy < 1e-8f && dz < 1e-8f) dx = nx, dy = ny, dz = nz;
        } else {  // Metal, materials.rs:52-63
            dx = fmaf(M.w, ux, rx), dy = fmaf(M.w, uy, ry), dz = fmaf(M.w, uz, rz);
        }
        tr *= M.x, tg *= M.y, tb *= M.z;
    } else {  // Dielectric, materials.rs:83-111
        const float ratio = front ? M.x : M.y;
        const float cth = fminf(-en, 1.f);
        const float sth = __builtin_sqrtf(fmaxf(1.f - cth * cth, 0.f));
        bool refl = ratio * sth > 1.f;
        if (!refl) {
            const float x = 1.f - cth;
            const float r = M.z + (1.f - M.z) * (x * ((x * x) * (x * x)));
            refl = r > r01(rng);
        }
        if (refl) {
            dx = rx, dy = ry, dz = rz;
        } else {  // refract (vec3.rs:259-268)
            const float qx = ratio * fmaf(cth, nx, g.ex), qy = ratio * fmaf(cth, ny, g.ey),
                        qz = ratio * fmaf(cth, nz, g.ez);
            const float par = -__builtin_sqrtf(fabsf(1.f - fmaf(qx, qx, fmaf(qy, qy, qz * qz))));
            dx = fmaf(par, nx, qx), dy = fmaf(par, ny, qy), dz = fmaf(par, nz, qz);
        }
    }
    const float sa = __builtin_sqrtf(fmaf(dx, dx, fmaf(dy, dy, dz * dz)));
    const float inv = __builtin_amdgcn_rcpf(sa);
    g.ox = px, g.oy = py, g.oz = pz;
    g.ex = dx * inv, g.ey = dy * inv, g.ez = dz * inv, g.tmin = 0.01f * sa;
    ++depth;
    return false;
}

// A finished sample's channel in the 32.32 fixed point of the pixel sums.
__device__ __forceinline__ unsigned long long to_fixed(float c, float cmax) {
    return static_cast<unsigned long long>(fminf(fmaxf(c, 0.f), cmax) * 4294967296.f);  // 2^32
}

// Scene tables and the BVH into LDS behind the per-lane stacks.
// A moving launch keeps its velocity rows between the nodes and the kind words (16-aligned).
template <bool kLds, bool kMove = false>
__device__ __forceinline__ void stage_scene(const FastParams &P, float4 *lds, uint32_t tid, const float4 *&geo,
                                            const float4 *&mat, const float4 *&nodes, const uint32_t *&kind,
                                            const float4 **vel = nullptr) {
    geo = P.geo, mat = P.mat, nodes = P.nodes, kind = P.kind;
    if constexpr (kMove) *vel = P.vel;
    if constexpr (kLds) {
        float4 *g = lds + P.n_stack * kBlock * sizeof(uint16_t) / sizeof(float4);
        float4 *m = g + P.n_sph, *nd = m + P.n_sph;
        float4 *tail = nd + P.n_node * rtw_accel::kNodeF4;
        if constexpr (kMove) {
            for (uint32_t i = tid; i < P.n_mov; i += kBlock) tail[i] = P.vel[i];
            *vel = tail, tail += P.n_mov;
        }
        uint32_t *kd = reinterpret_cast<uint32_t *>(tail);
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

// What a wave counted. segs, visits and wvisits are per lane; iters is wave-uniform.
struct WaveStats {
    uint32_t segs = 0, visits = 0, iters = 0, wvisits = 0;
};

// statistics: one atomic per wave and counter (FastParams::counters). done: the pixels that
// need nothing more from this launch, per lane (per_lane) or wave-uniform already; traced: the
// list kernel's samples ([5]; < 0: the launch has no such counter).
__device__ __forceinline__ void add_counters(const FastParams &P, uint32_t lane, const WaveStats &w,
                                             unsigned long long done, bool per_lane, long long traced = -1) {
    unsigned long long sg = w.segs, vs = w.visits, wv = w.wvisits;
    for (int o = 32; o > 0; o >>= 1) {
        sg += __shfl_xor(sg, o);
        vs += __shfl_xor(vs, o);
        wv += __shfl_xor(wv, o);
        if (per_lane) done += __shfl_xor(done, o);
    }
    if (lane == 0) {
        atomicAdd(P.counters + 0, sg);
        atomicAdd(P.counters + 1, vs);
        atomicAdd(P.counters + 2, done);
        atomicAdd(P.counters + 3, static_cast<unsigned long long>(w.iters));
        atomicAdd(P.counters + 4, wv);
        if (traced >= 0) atomicAdd(P.counters + 5, static_cast<unsigned long long>(traced));
    }
}

// ---- the ring scheduler
// A persistent wave keeps a ring of Use::kRing jobs in flight; a job is some samples of one
// pixel. Idle lanes take the next samples of the newest job (ballot + mbcnt), so a lane whose
// path ends starts another at once; a finished sample goes into the job's Use::kSums u64 sums
// in LDS (LDS atomics: exact and order-free), and a job whose samples are all handed out and
// back is flushed. The ring state (the jobs, their samples in flight, the job being handed
// out and its next ordinal) is wave-uniform, in scalar registers. A Use says what differs:
//   Job                   at least {pix}: the pixel, kFree in a free slot
//   kRing, kSums          ring slots per wave, u64 sums per slot
//   claim(lane, job)      the wave's next job from the launch's cursor: kJob, kSkip (the entry
//                         needs nothing) or kDone (the cursor has passed the end)
//   count(job)            its samples; lattice(job, i): the lattice sample k of its ordinal i
//   add(sums, r, g, b)    a finished sample's 32.32 colour into a slot's sums
//   flush(lane, job, sums)  the finished job's sums to global memory
enum class Claim { kJob, kSkip, kDone };

// The hand-out most kernels use: a wave claims `chunk` consecutive entries per cursor atomic
// (every wave draws from one address, and its atomics serialise).
struct ChunkCursor {
    uint32_t at = 0, end = 0;  // the wave's entries claimed and not yet started
    __device__ __forceinline__ bool next(const FastParams &P, uint32_t lane, uint32_t chunk, uint32_t n, uint32_t &e) {
        if (at == end) {
            uint32_t c = 0;
            if (lane == 0) c = atomicAdd(P.cursor, chunk);
            c = __builtin_amdgcn_readfirstlane(c);
            if (c >= n) return false;
            at = c, end = min(c + chunk, n);
        }
        e = at++;
        return true;
    }
};

// R, G, B sums: what a slot holds unless the Use adds to them.
struct RgbSums {
    static constexpr uint32_t kSums = 3;
    static __device__ __forceinline__ void add(unsigned long long *a, unsigned long long r, unsigned long long g,
                                               unsigned long long b) {
        atomicAdd(a + 0, r);
        atomicAdd(a + 1, g);
        atomicAdd(a + 2, b);
    }
};

// Runs the calling wave until the cursor is exhausted and its ring is empty; returns its
// counts and, in flushed, the jobs it flushed. Every wave of the workgroup must call it.
template <bool kLds, bool kMove, class Use>
__device__ __forceinline__ WaveStats run_ring(const FastParams &P, Use &u, uint32_t &flushed) {
    using Job = typename Use::Job;
    constexpr uint32_t kRing = Use::kRing;
    extern __shared__ __attribute__((aligned(16))) float4 lds[];
    __shared__ unsigned long long acc[kWaves][kRing][Use::kSums];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    // per-lane stack column: slot j at stk[j * kBlock]
    uint16_t *stk = reinterpret_cast<uint16_t *>(lds) + tid;
    const float4 *geo, *mat, *nodes;
    const uint32_t *kind;
    Motion mo{};
    stage_scene<kLds, kMove>(P, lds, tid, geo, mat, nodes, kind, &mo.vel);
    mo.kind = kind;
    const float cmax = P.cmax;
    // wave-uniform ring state
    Job jobs[kRing], cur{};
    uint32_t outst[kRing];
#pragma unroll
    for (uint32_t s = 0; s < kRing; ++s) jobs[s].pix = kFree, outst[s] = 0;
    uint32_t cs = kFree, next = 0;
    bool exhausted = false;
    // lane path state
    Seg g{};
    float tr = 0.f, tg = 0.f, tb = 0.f;
    uint32_t depth = 0, slot = kFree;
    Rng rng{1u, 0u};
    WaveStats w;
    flushed = 0;
    for (;;) {
        // ---- hand out samples of the newest job to idle lanes
        for (;;) {
            const uint64_t need = __ballot(slot == kFree);
            if (need == 0) break;
            if (cs == kFree || next >= u.count(cur)) {
                if (exhausted) break;
                uint32_t f = kFree;
#pragma unroll
                for (uint32_t s = 0; s < kRing; ++s)
                    if (f == kFree && jobs[s].pix == kFree) f = s;
                if (f == kFree) break;
                Job j;
                const Claim c = u.claim(lane, j);
                if (c == Claim::kDone) {
                    exhausted = true;
                    break;
                }
                if (c == Claim::kSkip) continue;
#pragma unroll
                for (uint32_t s = 0; s < kRing; ++s)
                    if (s == f) jobs[s] = j, outst[s] = 0;
                if (lane < Use::kSums) acc[wave][f][lane] = 0ull;
                __builtin_amdgcn_wave_barrier();
                cs = f, cur = j, next = 0;
            }
            const uint32_t rank = rank_in(need);
            const uint32_t avail = u.count(cur) - next;
            if (slot == kFree && rank < avail) {
                start_path<kMove>(P, cur.pix, u.lattice(cur, next + rank), rng, g, &mo.t);
                tr = tg = tb = 1.f;
                depth = 0;
                slot = cs;
            }
            const uint32_t took = min(static_cast<uint32_t>(__builtin_popcountll(need)), avail);
            next += took;
#pragma unroll
            for (uint32_t s = 0; s < kRing; ++s)
                if (s == cs) outst[s] += took;
        }
        if (__ballot(slot != kFree) == 0) break;  // nothing handed out: the launch's work is done
        ++w.iters;
        // ---- one segment per busy lane; finished samples into their job's sums
        float cr = 0.f, cg = 0.f, cb = 0.f;
        const bool fin = slot != kFree && trace_segment<kMove>(P, geo, mat, kind, nodes, g, rng, tr, tg, tb, depth, stk,
                                                               w.segs, w.visits, w.wvisits, cr, cg, cb, mo);
        if (fin) Use::add(acc[wave][slot], to_fixed(cr, cmax), to_fixed(cg, cmax), to_fixed(cb, cmax));
#pragma unroll
        for (uint32_t s = 0; s < kRing; ++s)
            outst[s] -= static_cast<uint32_t>(__builtin_popcountll(__ballot(fin && slot == s)));
        if (fin) slot = kFree;
        // ---- jobs whose samples are all handed out and finished
#pragma unroll
        for (uint32_t s = 0; s < kRing; ++s) {
            if (jobs[s].pix != kFree && outst[s] == 0 && (s != cs || next >= u.count(cur))) {
                __builtin_amdgcn_wave_barrier();
                u.flush(lane, jobs[s], acc[wave][s]);
                jobs[s].pix = kFree;
                ++flushed;
                if (s == cs) cs = kFree;
            }
        }
    }
    return w;
}

// ---- sums to images
__device__ __forceinline__ uint32_t preview_u8(float mean) {  // Rust's `(mean as f64 * 255.) as u8`
    const double v = static_cast<double>(mean) * 255.;
    return v >= 255. ? 255u : (v > 0. ? static_cast<uint32_t>(v) : 0u);  // NaN -> 0
}

// A 32.32 sum over n samples to the f32 mean: an IEEE f64 divide, the same on every route.
__device__ __forceinline__ float mean_f32(unsigned long long sum, double n) {
    return static_cast<float>(static_cast<double>(sum) * (1. / 4294967296.) / n);
}

// Pixel p of the sums divided by n (0: the pixel resolves to 0) to the frame and/or the preview.
__device__ __forceinline__ void resolve_pixel(const unsigned long long *__restrict__ acc, uint64_t p, double n,
                                              float *__restrict__ out, uint32_t *__restrict__ preview) {
    float m[3];
#pragma unroll
    for (uint32_t c = 0; c < 3; ++c) m[c] = n > 0. ? mean_f32(acc[p * 3u + c], n) : 0.f;
    if (out) out[p * 3u + 0] = m[0], out[p * 3u + 1] = m[1], out[p * 3u + 2] = m[2];
    if (preview) preview[p] = preview_u8(m[0]) | (preview_u8(m[1]) << 8) | (preview_u8(m[2]) << 16) | 0xff000000u;
}

// ---- the launch the persistent kernels share: the cursor and n_counters counters zeroed,
// then (unless `nothing` is to be done) two workgroups per CU, no more than have work when a
// workgroup starts on per_block pixels; the kernel with the scene in LDS when it fits below
// cap and scene_lds allows it (A/B: RTW_FAST_LDS=0 under RTW_AB reads the scene from HBM).
template <class Params>
hipError_t launch_persistent(void (*in_lds_kernel)(Params), void (*global_kernel)(Params), const Params &A,
                             const FastParams &P, bool nothing, uint32_t n_counters, uint64_t per_block, uint32_t cap,
                             int n_cu, hipStream_t st, bool scene_lds) {
    hipError_t e = hipMemsetAsync(P.cursor, 0, sizeof(uint32_t), st);
    if (e == hipSuccess) e = hipMemsetAsync(P.counters, 0, n_counters * sizeof(unsigned long long), st);
    if (e != hipSuccess || nothing) return e;
    const uint64_t npix = static_cast<uint64_t>(P.n_rows) * P.W;
    const uint32_t blocks = static_cast<uint32_t>(
        std::min<uint64_t>(static_cast<uint64_t>(n_cu > 0 ? n_cu : 256) * 2, (npix + per_block - 1) / per_block));
    bool in_lds = false;
    size_t lds = lds_bytes(P.n_sph, P.n_node, P.n_stack, cap, &in_lds, P.move ? P.n_mov : 0u);
    if (!scene_lds && in_lds) {
        in_lds = false;
        lds = P.n_stack ? static_cast<size_t>(P.n_stack) * kBlock * sizeof(uint16_t) : 16;
    }
    hipLaunchKernelGGL(in_lds ? in_lds_kernel : global_kernel, dim3(blocks), dim3(kBlock), lds, st, A);
    return hipGetLastError();
}

}  // namespace
}  // namespace rtw_fast
