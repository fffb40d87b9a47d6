"""The cases of the per-sample check of f32 fast mode against oracle/fast_model.py, and the
rule that says which samples must agree. Shared by tests/test_fast_model.py (CPU: the rule's
cap on every case) and tests/test_gpu_fast_samples.py (GPU: the comparison).

f32 flips decisions that f64 does not (a grazing hit, a Schlick comparison, the threshold of
total internal reflection), and after a flip the two paths have nothing in common. So the
model classifies its own samples, without looking at the kernel: a sample is stable if in
RUNS perturbed model runs at EPS (oracle/fast_model.py: perturb) the segment count is
unchanged and every channel stays within T/4 of the unperturbed run. T = 2^-10 per channel,
a quarter of an 8-bit step at full scale, is "agree". The caps (tests hold them, they are
not measurements): at most UNSTABLE_CAP of a case's samples unstable; at most DISAGREE_CAP of
the stable ones further than T from the GPU; the mean signed difference over the stable
ones within T/8; over all samples within T/8 + 4 sqrt(D)/N, D the samples beyond T; the
launches' segment total within max_depth * D of the model's.
"""
import functools
import random

from oracle import fast_model as fm
from oracle import pyoracle as po

T = 2.0 ** -10
EPS = 2.0 ** -15
RUNS = 3
PROBE_SEED = 0x5EED
UNSTABLE_CAP = 0.10
DISAGREE_CAP = 0.01

SEED = 1764892800123
SEED_HI = (0x0123456789ABCDEF << 64) | SEED  # the high half reaches seed_mix

L, M, D = po.LAMBERTIAN, po.METAL, po.DIELECTRIC


def custom_scene():
    """The scene of test_fast_custom_scene_statistical (hollow glass with a negative radius,
    ir = 1/1.33, Metal with fuzz 1) with a Metal of fuzz 0 and a Lambertian in front."""
    glass = (D, (0.0, 0.0, 0.0), 0.0, 1.5)
    return [((0.0, -100.5, -1.0), 100.0, (L, (0.8, 0.8, 0.0), 0.0, 0.0)),
            ((0.0, 0.0, -1.0), 0.5, (M, (0.9, 0.9, 0.9), 1.0, 0.0)),
            ((-1.0, 0.0, -1.0), 0.5, glass),
            ((-1.0, 0.0, -1.0), -0.4, glass),
            ((1.0, 0.0, -1.0), 0.5, (D, (0.0, 0.0, 0.0), 0.0, 1.0 / 1.33)),
            ((0.55, -0.25, -0.2), 0.25, (M, (0.7, 0.6, 0.5), 0.0, 0.0)),
            ((-0.55, -0.25, -0.2), 0.25, (L, (0.4, 0.2, 0.1), 0.0, 0.0))]


def custom_camera(h, w, depth):
    return po.Camera(h, w, depth, 1.0, 60.0, (0.0, 0.5, 1.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 2.0, 2.0)


def scan_scene():
    """A scene that leaves fast mode without BVH nodes (stats().accel == 0), within f32's
    reach: a sphere with a radius above kHugeRatio (16) times the median radius is tested
    before the walk ("always"), and more than kMaxAlways (16) of those make
    rtw_accel::build give up, so every segment scans. 18 beads of radius 0.03 hold the
    median down; the ground and a 4x4 grid of radius 0.5 are the 17 "always" spheres."""
    objs = [((0.0, -100.5, -1.0), 100.0, (L, (0.5, 0.6, 0.4), 0.0, 0.0))]
    mats = [(L, (0.7, 0.3, 0.3), 0.0, 0.0), (M, (0.8, 0.8, 0.9), 0.25, 0.0), (D, (0.0, 0.0, 0.0), 0.0, 1.5),
            (M, (0.9, 0.7, 0.4), 0.0, 0.0)]
    for j in range(4):
        for i in range(4):
            objs.append(((-1.8 + 1.2 * i, 0.0, -1.0 - 1.2 * j), 0.5, mats[(i + j) % 4]))
    for b in range(18):
        objs.append(((-2.3 + 0.27 * b, -0.47, -0.3 - 0.21 * (b % 5)), 0.03, mats[b % 4]))
    return objs


def scan_camera(h, w, depth):
    return po.Camera(h, w, depth, 1.0, 50.0, (0.3, 1.2, 2.5), (0.0, 0.0, -2.0), (0.0, 1.0, 0.0), 1.0, 4.5)


def builtin(name, defocus=None):
    def make(h, w, depth):
        cam, objs = po.scene_builtin(name, SEED, h, w, depth)
        if defocus is not None:
            cam = po.Camera(h, w, depth, cam.focal_length, cam.fov, cam.look_from, cam.look_to, cam.vup, defocus,
                            cam.focus_dist)
        return cam, objs
    return make


def made(camera, scene):
    return lambda h, w, depth: (camera(h, w, depth), scene())


# name: (scene, h, w, max_depth, samples_sqrt, seed, shard (row_begin, row_step, n_rows) or None)
CASES = {
    # stage 1, depth 1: sky or black -- the pixel grid, lattice, disk, global pixel index, silhouettes
    "d1_final_9x16_s3": (builtin("complex"), 9, 16, 1, 3, SEED, None),
    "d1_final_shard_9x16_s3": (builtin("complex"), 9, 16, 1, 3, SEED_HI, (1, 3, 3)),
    "d1_three_nodefocus_7x11_s2": (builtin("three_lambertian", defocus=0.0), 7, 11, 1, 2, SEED, None),
    "d1_final_7x5_s0": (builtin("complex"), 7, 5, 1, 0, SEED, None),
    "d1_final_7x5_s1": (builtin("complex"), 7, 5, 1, 1, SEED_HI, None),
    # stage 2, depth 2: one scatter, then sky -- each material's outgoing direction
    "d2_custom_12x20_s2": (made(custom_camera, custom_scene), 12, 20, 2, 2, SEED, None),
    # full depth
    "final_12x20_s2_d50": (builtin("complex"), 12, 20, 50, 2, SEED, None),
    "simple_12x20_s2_d25": (builtin("simple"), 12, 20, 25, 2, SEED, None),
    "custom_12x20_s2_d30": (made(custom_camera, custom_scene), 12, 20, 30, 2, SEED_HI, None),
    # the linear scan (no BVH nodes)
    "scan_12x20_s2_d50": (made(scan_camera, scan_scene), 12, 20, 50, 2, SEED, None),
    # 16 samples a pixel: render_fast's ring kernel against the per-pixel mean
    "ring_final_8x12_s4_d50": (builtin("complex"), 8, 12, 50, 4, SEED, None),
}
DEPTH1 = [n for n in CASES if n.startswith("d1_")]


class Case:
    """A case's model table, computed once: samples {(x, y, k): (rgb, segments)} over the
    shard's rows (global y) and the keys the rule calls stable."""

    def __init__(self, name):
        make, self.h, self.w, self.depth, self.s, self.seed, self.shard = CASES[name]
        self.name = name
        self.cam, self.objs = make(self.h, self.w, self.depth)
        self.n_off = max(1, self.s * self.s)
        b, step, n = self.shard or (0, 1, self.h)
        self.rows = [b + i * step for i in range(n)]
        self.samples = fm.table(self.cam, self.objs, self.s, self.seed, rows=self.rows)
        rng = random.Random(PROBE_SEED)
        self.stable = set(self.samples)
        for _ in range(RUNS):
            probe = fm.table(self.cam, self.objs, self.s, self.seed, rows=self.rows, perturb=(EPS, rng))
            for key, (rgb, segs) in probe.items():
                ref, ref_segs = self.samples[key]
                if segs != ref_segs or max(abs(a - b) for a, b in zip(rgb, ref)) > T / 4:
                    self.stable.discard(key)
        self.segments = sum(segs for _, segs in self.samples.values())


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


# ------------------------------------------------------------- the GPU side --
def gpu_session(c):
    """(Session, rtw_camera) of a case: the same scene and camera through the library."""
    import raytracing_in_a_weekend_rust_amd as rtw
    world = rtw.SceneBuilder()
    for center, radius, (kind, albedo, fuzz, ir) in c.objs:
        mat = rtw.Lambertian(albedo) if kind == L else rtw.Metal(albedo, fuzz) if kind == M else rtw.Dielectric(ir)
        world.add(rtw.Sphere.new_world_obj(*center, radius, mat))
    p = c.cam
    cam = rtw.Camera.new(c.h, c.w, c.depth, p.focal_length, p.fov, p.look_from, p.look_to, p.vup, p.defocus_angle,
                         p.focus_dist).raw
    assert cam.pixel00.tup() == p.pixel00 and cam.pixel_delta_v.tup() == p.pixel_delta_v
    sess = rtw.Session(0)
    sess.set_scene(*world.build().flatten())
    return sess, cam


def gpu_samples(c):
    """({(x, y, k): rgb}, segments, accel) from one accumulate_fast(k, 1, 1) per k into fresh
    zero sums: the 32.32 sum of one sample is its f32 colour times 2^32."""
    import torch
    sess, cam = gpu_session(c)
    st = torch.cuda.current_stream().cuda_stream
    out, segments = {}, 0
    for k in range(c.n_off):
        acc = torch.zeros((len(c.rows), c.w, 3), dtype=torch.int64, device="cuda:0")
        sess.accumulate_fast(cam, c.s, c.seed, acc.data_ptr(), k, 1, 1, shard=c.shard, stream=st)
        stats = sess.stats()
        assert stats.samples == len(c.rows) * c.w
        segments += stats.segments
        rgb = acc.cpu().numpy().astype("float64") * 2.0 ** -32
        for r, y in enumerate(c.rows):
            for x in range(c.w):
                out[(x, y, k)] = tuple(rgb[r, x])
    return out, segments, stats.accel


def agreement(c, gpu, segments):
    """The figures the conditions are stated on, as a JSON-ready dict."""
    import numpy as np
    keys = sorted(c.samples)
    diff = np.array([gpu[k] for k in keys]) - np.array([c.samples[k][0] for k in keys])  # gpu - model
    worst = np.abs(diff).max(axis=1)
    stable = np.array([k in c.stable for k in keys])
    agree = worst <= T
    n = len(keys)
    return {
        "case": c.name, "samples": n, "stable": int(stable.sum()), "unstable_share": 1. - stable.sum() / n,
        "stable_disagreeing": int((stable & ~agree).sum()),
        "stable_disagreeing_share": float((stable & ~agree).sum() / max(1, stable.sum())),
        "agree_max_diff": float(worst[agree].max()), "agree_mean_diff": float(worst[agree].mean()),
        "D": int((~agree).sum()),
        "stable_mean_signed": [float(v) for v in diff[stable].mean(axis=0)],
        "all_mean_signed": [float(v) for v in diff.mean(axis=0)],
        "segments_gpu": int(segments), "segments_model": c.segments, "max_depth": c.depth,
    }
