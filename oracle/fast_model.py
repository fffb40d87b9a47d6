"""TEST INFRASTRUCTURE ONLY -- an f64 model of one sample of f32 fast mode
(csrc/rtw_fast_dev.h), for tests/test_fast_model.py and tests/test_gpu_fast_samples.py.

A fast-mode sample is a pure function of (scene, camera, seed, global pixel, lattice
index k), and its random numbers come from an integer generator. This module draws the
same numbers and traces the path with the geometry and materials of oracle/pyoracle.py,
the reference's own formulation (unnormalised directions, t >= 0.01 in parameter units,
the textbook quadratic, first minimum wins, near_zero without abs), in f64. It restates
nothing of the kernel's arithmetic; only the stream contract below is shared with it
(DESIGN 3.10). Needs numpy, no GPU and no library.

The contract
  Stream of sample (global pixel pix = y*W + x, lattice index k):
      z = fmix64(fmix64(seed_mix ^ pix*0x9e3779b97f4a7c15) + k)    (mod 2^64)
      seed_mix = lo ^ hi*0x9e3779b97f4a7c15 of the u128 seed, fmix64 = SplitMix64's finaliser;
      state (a, b) = (low 32 bits, high 32 bits) of z, (0, 0) becomes (1, 0);
      generator xoroshiro64**.
  Uniforms: u01 = (next >> 8) * 2^-24, coord = (next >> 8) * 2^-23 - 1.
  Draw order: with defocus_angle > 0 the disk sample first (rad = sqrt(u01), then the
      angle u01 in revolutions); each Lambertian or Metal hit (fuzz 0 included) one unit
      vector (z = coord, then the azimuth u01 in revolutions); each Dielectric hit one
      u01, and only when it is not in total internal reflection.
  Lattice: offset k is offset_lattice(pixel_delta_v, pixel_delta_u, s)[k], that is
      pos0 + ldx*(k mod s) + ldy*(k div s) with ldx = delta_v/s, ldy = delta_u/s; s = 0
      gives the pixel centre.
  Inputs: camera and scene values are rounded to f32 where fast_params and set_scene
      round them (numpy.float32(x) back to float; 1/ir and r0^2 formed in f64, then
      rounded). The kernel rounds the lattice's generators pos0, ldx, ldy; the model
      rounds offset_lattice's f64 offset k, a few f32 ulps of a sub-pixel length away.
      Everything after that is f64. The sample's colour is clamped to [0, cmax],
      cmax = f32(min(65536, 2^31 / samples per pixel)).
"""
from __future__ import annotations

import math
import types

import numpy as np

from . import pyoracle as po

M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15
TAU = 2.0 * math.pi


def f32(x: float) -> float:
    return float(np.float32(x))


def f32v(v):
    return (f32(v[0]), f32(v[1]), f32(v[2]))


# ------------------------------------------------------------------ streams --
def fmix64(z: int) -> int:
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def seed_mix(seed: int) -> int:
    lo, hi = seed & M64, (seed >> 64) & M64
    return lo ^ ((hi * GOLD) & M64)


def rotl32(x: int, r: int) -> int:
    return ((x << r) | (x >> (32 - r))) & 0xFFFFFFFF


class Stream:
    """The stream of one sample: xoroshiro64** from the state the contract gives."""

    def __init__(self, mix: int, pix: int, k: int):
        z = fmix64((fmix64(mix ^ ((pix * GOLD) & M64)) + k) & M64)
        self.a, self.b = z & 0xFFFFFFFF, z >> 32
        if self.a == 0 and self.b == 0:
            self.a = 1

    def next_u32(self) -> int:
        s0, s1 = self.a, self.b
        res = (rotl32((s0 * 0x9E3779BB) & 0xFFFFFFFF, 5) * 5) & 0xFFFFFFFF
        s1 ^= s0
        self.a = rotl32(s0, 26) ^ s1 ^ ((s1 << 9) & 0xFFFFFFFF)
        self.b = rotl32(s1, 13)
        return res

    def next_01(self) -> float:
        return (self.next_u32() >> 8) * 2.0 ** -24

    def next_coord(self) -> float:
        return (self.next_u32() >> 8) * 2.0 ** -23 - 1.0


def unit_vec(r: Stream):
    z = r.next_coord()
    t = r.next_01()
    s = math.sqrt(1.0 - z * z)
    return (s * math.cos(TAU * t), s * math.sin(TAU * t), z)


def disk_vec(r: Stream):
    rad = math.sqrt(r.next_01())
    t = r.next_01()
    return (rad * math.cos(TAU * t), rad * math.sin(TAU * t), 0.0)


# ------------------------------------------------------------------- inputs --
def rounded_camera(cam):
    """The fields get_ray reads, rounded as fast_params rounds them."""
    return types.SimpleNamespace(
        pixel00=f32v(cam.pixel00), pixel_delta_u=f32v(cam.pixel_delta_u), pixel_delta_v=f32v(cam.pixel_delta_v),
        look_from=f32v(cam.look_from), defocus_disk_u=f32v(cam.defocus_disk_u),
        defocus_disk_v=f32v(cam.defocus_disk_v), defocus_angle=cam.defocus_angle)


def rounded_scene(objs):
    """[(center, radius, material, glass)] rounded as set_scene rounds fast mode's rows;
    glass = (1/ir, ir, r0^2) for a Dielectric, else None."""
    out = []
    for center, radius, (kind, albedo, fuzz, ir) in objs:
        glass = None
        if kind == po.DIELECTRIC:
            r0 = (1.0 - ir) / (1.0 + ir)
            glass = (f32(1.0 / ir), f32(ir), f32(r0 * r0))
        out.append((f32v(center), f32(radius), (kind, f32v(albedo), f32(fuzz), f32(ir)), glass))
    return out


def lattice_offset(cam, samples_sqrt: int, k: int):
    return f32v(po.offset_lattice(cam.pixel_delta_v, cam.pixel_delta_u, samples_sqrt)[k])


def cmax(samples_sqrt: int) -> float:
    return f32(min(65536.0, 2147483648.0 / float(max(1, samples_sqrt * samples_sqrt))))


# ---------------------------------------------------------------- the scene --
class Prepared:
    """A (camera, scene, samples_sqrt, seed) ready for sample(): the rounded inputs and,
    for scene_hit, numpy columns of the spheres."""

    def __init__(self, cam, objs, samples_sqrt: int, seed: int):
        self.cam, self.rcam = cam, rounded_camera(cam)
        self.scene = rounded_scene(objs)
        self.objs = [(c, r, i) for i, (c, r, _, _) in enumerate(self.scene)]
        self.s, self.mix = samples_sqrt, seed_mix(seed)
        self.n_off = max(1, samples_sqrt * samples_sqrt)
        self.offsets = [lattice_offset(cam, samples_sqrt, k) for k in range(self.n_off)]
        self.cmax = cmax(samples_sqrt)
        self.C = np.array([c for c, _, _, _ in self.scene], dtype=np.float64).reshape(-1, 3)
        self.R2 = np.array([r * r for _, r, _, _ in self.scene], dtype=np.float64)

    def hit(self, orig, d):
        """pyoracle.scene_hit over the spheres the segment's line can touch. The cut is
        the quadratic's discriminant with a margin of 1e-9 of its terms, far above their
        rounding: what it drops, sphere_hit would reject, so the result is scene_hit's
        (tests/test_fast_model.py compares them)."""
        if not self.objs:
            return None
        oc = np.asarray(orig) - self.C
        dv = np.asarray(d)
        a = float(dv @ dv)
        hb = oc @ dv
        oc2 = np.einsum("ij,ij->i", oc, oc)
        hb2 = hb * hb
        disc = hb2 - a * (oc2 - self.R2)
        keep = np.nonzero(~(disc < -1e-9 * (hb2 + a * (oc2 + self.R2))))[0]
        return po.scene_hit([self.objs[i] for i in keep], orig, d)


def _jiggle(v, perturb):
    if perturb is None:
        return v
    eps, rng = perturb
    return tuple(c * (1.0 + eps * rng.uniform(-1.0, 1.0)) for c in v)


def sample_prepared(P: Prepared, x: int, y: int, k: int, perturb=None):
    rnd = Stream(P.mix, y * P.cam.width + x, k)
    orig, d = po.get_ray(P.rcam, x, y, P.offsets[k], rnd, disk=disk_vec)
    d = _jiggle(d, perturb)
    att, segs = (1.0, 1.0, 1.0), 0
    rgb = (0.0, 0.0, 0.0)  # black at the depth cap (camera.rs:381-383)
    for _ in range(P.cam.max_depth):
        segs += 1
        hit = P.hit(orig, d)
        if hit is None:
            rgb = po.mulv(att, po.sky(d))
            break
        rec, i = hit
        _, _, m, glass = P.scene[i]
        orig, d, a = po.scatter(m, d, rec, rnd, unit_vec=unit_vec, glass=glass)
        orig, d = _jiggle(orig, perturb), _jiggle(d, perturb)
        att = po.mulv(att, a)
    return tuple(min(max(c, 0.0), P.cmax) for c in rgb), segs


def sample(cam, objs, samples_sqrt, seed, x, y, k, perturb=None):
    """(rgb, segments) of lattice sample k of pixel (x, y). perturb = (eps, rng): every
    component of the primary direction and of every scattered origin and direction is
    multiplied by 1 + eps * rng.uniform(-1, 1) (the stability probe of the tests)."""
    return sample_prepared(Prepared(cam, objs, samples_sqrt, seed), x, y, k, perturb)


def table(cam, objs, samples_sqrt, seed, rows=None, perturb=None):
    """{(x, y, k): (rgb, segments)} of every sample of the image, or of the given rows."""
    P = Prepared(cam, objs, samples_sqrt, seed)
    rows = range(cam.height) if rows is None else rows
    return {(x, y, k): sample_prepared(P, x, y, k, perturb)
            for y in rows for x in range(cam.width) for k in range(P.n_off)}
