"""Denoised fast mode (rtw_session_guides_fast, rtw_denoise_fast, rtw_session_render_fast_denoised):
the filter against one numpy evaluation of rtw_capi.h's definitions on synthetic buffers, the
guides against oracle/fast_model.py's f64 closest hit, the driver against its steps by hand."""
import functools
import os
import random
import subprocess
import types
from fractions import Fraction

import numpy as np
import pytest
import torch

import raytracing_in_a_weekend_rust_amd as rtw
from oracle import fast_model as fm
from oracle import pyoracle as po
from tests import fast_cases as fc
from tests.test_gpu_png import decode

pytestmark = pytest.mark.gpu
SEED = fc.SEED
H5 = (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16)


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # a copy: the cached inputs are read-only


def shifted(a, dy, dx):
    """a[y + dy, x + dx], zero where that lies outside."""
    h, w = a.shape[:2]
    out = np.zeros_like(a)
    if abs(dy) < h and abs(dx) < w:
        out[max(-dy, 0):h - max(dy, 0), max(-dx, 0):w - max(dx, 0)] = a[max(dy, 0):h + min(dy, 0), max(dx, 0):w + min(dx, 0)]
    return out


def reference(acc, counts, mom, normals, tags, levels, normal_log2, mask, sigma_l, dtype):
    """rtw_capi.h's prepare and levels: Python ints for D, then `dtype`. Returns (rgb, v, C0)."""
    h, w = counts.shape
    n = counts.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        rgb = np.where(counts[..., None] > 0, np.float32(acc.astype(np.float64) * 2.0 ** -32 / n[..., None]), np.float32(0))
    rgb = rgb.astype(dtype)
    L1 = (rgb[..., 0] + rgb[..., 1]) + rgb[..., 2]
    v = np.zeros((h, w), dtype)
    for y, x in np.ndindex(h, w):
        k, A, B = int(counts[y, x]), int(mom[y, x, 0]), int(mom[y, x, 1])
        if k == 1:
            v[y, x] = L1[y, x] * L1[y, x]
        elif k >= 2:
            D = (k * B - A * A) % (1 << 128)
            v[y, x] = np.float32(float(D) * 2.0 ** -32 / (float(k) * float(k) * float(k - 1)))
    C = np.concatenate([rgb, v[..., None]], axis=2)
    C0 = C.copy()
    nrm, inside = normals.astype(dtype), np.ones((h, w), dtype)
    filtered = ((mask >> (tags >> 30)) & 1).astype(bool)
    for lv in range(levels):
        t = 1 << lv
        num, den = np.zeros((h, w), dtype), np.zeros((h, w), dtype)
        for j in (-1, 0, 1):
            for i in (-1, 0, 1):
                k = dtype((2 - abs(i)) * (2 - abs(j)))
                num, den = num + k * shifted(C[..., 3], j * t, i * t), den + k * shifted(inside, j * t, i * t)
        scale = dtype(sigma_l) * np.sqrt(num / den) + dtype(1e-6)
        L = (C[..., 0] + C[..., 1]) + C[..., 2]
        sw, sc, sv = np.zeros((h, w), dtype), np.zeros((h, w, 3), dtype), np.zeros((h, w), dtype)
        for j in range(-2, 3):
            for i in range(-2, 3):
                Cq, nq = shifted(C, j * t, i * t), shifted(nrm, j * t, i * t)
                d = np.maximum((nrm * nq).sum(axis=2, dtype=dtype), 0)
                for _ in range(normal_log2):
                    d = d * d
                same = (shifted(tags, j * t, i * t) == tags) & (shifted(inside, j * t, i * t) > 0)
                Lq = (Cq[..., 0] + Cq[..., 1]) + Cq[..., 2]
                wgt = dtype(H5[i + 2] * H5[j + 2]) * same * d * np.exp(-np.abs(L - Lq) / scale)
                sw, sc, sv = sw + wgt, sc + wgt[..., None] * Cq[..., :3], sv + wgt * wgt * Cq[..., 3]
        new = np.concatenate([sc / sw[..., None], (sv / (sw * sw))[..., None]], axis=2)
        C = np.where(filtered[..., None], new, C)
    return C[..., :3], C[..., 3], C0


@functools.lru_cache(maxsize=None)
def synthetic(h, w):
    """Seeded buffers: tags in rectangular blobs over a sky (every kind where there is room), unit
    normals that vary smoothly inside a blob, counts from {0, 1, 2, 7, 400}, and sums and moments
    of that many samples around the blob's colour."""
    rng = np.random.default_rng(h * 1000 + w)
    tags = np.full((h, w), 0xFFFFFFFF, np.int64)
    base = np.tile(rng.uniform(0.2, 0.9, 3), (h, w, 1))
    nrm = np.tile(rng.normal(size=3), (h, w, 1))
    yy, xx = np.mgrid[0:h, 0:w]
    for b in range(9):
        y0, x0 = rng.integers(0, h), rng.integers(0, w)
        y1, x1 = y0 + rng.integers(1, h // 2 + 2), x0 + rng.integers(1, w // 2 + 2)
        tags[y0:y1, x0:x1] = ((b % 3) << 30) | int(rng.integers(0, 500))
        base[y0:y1, x0:x1] = rng.uniform(0.05, 0.95, 3)
        nrm[y0:y1, x0:x1] = rng.normal(size=3)
    for c in range(3):  # a gradient per tag keeps the normals smooth inside a blob and apart across blobs
        nrm[..., c] += 0.02 * ((tags % 7 - 3) * xx + (tags % 5 - 2) * yy) / (1 + c)
    nrm /= np.linalg.norm(nrm, axis=2, keepdims=True)
    counts = rng.choice(np.array([0, 1, 2, 7, 400], np.uint32), (h, w))
    acc, mom = np.zeros((h, w, 3), np.uint64), np.zeros((h, w, 2), np.uint64)
    for k in (1, 2, 7, 400):
        at = counts == k
        S = (base[at][:, None, :] * rng.uniform(0.6, 1.4, (at.sum(), k, 3)) * 2.0 ** 32).astype(np.uint64)
        q = np.minimum(S.sum(axis=2) >> np.uint64(16), np.uint64((1 << 24) - 1))
        acc[at], mom[at] = S.sum(axis=1), np.stack([q.sum(axis=1), (q * q).sum(axis=1)], axis=1)
    guides = np.concatenate([nrm.astype(np.float32), tags.astype(np.uint32).view(np.float32)[..., None]], axis=2)
    out = acc, counts, mom, guides, tags
    for a in out:
        a.setflags(write=False)
    return out


def run_filter(h, w, preview=False, **prm):
    acc, counts, mom, guides, _ = synthetic(h, w)
    bufs = [dev(acc.view(np.int64)), dev(counts.view(np.int32)), dev(mom.view(np.int64)), dev(guides)]
    out = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
    var = torch.zeros((h, w), dtype=torch.float32, device="cuda:0")
    pre = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0")
    rtw.denoise_fast(*(b.data_ptr() for b in bufs), (h, w), out_ptr=out.data_ptr(), var_ptr=var.data_ptr(),
                     preview_ptr=pre.data_ptr() if preview else 0, stream=stream(), **prm)
    return out.cpu().numpy(), var.cpu().numpy(), pre.cpu().numpy(), bufs


@pytest.mark.parametrize("mask", [0xB, 0xF])
@pytest.mark.parametrize("levels", [1, 3, 5])
@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (23, 37), (35, 273)])
def test_filter_against_the_f64_reference(h, w, levels, mask):
    acc, counts, mom, guides, tags = synthetic(h, w)
    assert (h, w) == (1, 1) or {0, 1, 2, 3} == set(np.unique(tags >> 30))
    want, want_v, _ = reference(acc, counts, mom, guides[..., :3], tags, levels, 5, mask, 4.0, np.float64)
    r32, v32, c0 = reference(acc, counts, mom, guides[..., :3], tags, levels, 5, mask, 4.0, np.float32)
    got, got_v, _, _ = run_filter(h, w, levels=levels, filter_mask=mask)
    floor = 2.0 ** -20 * want.max()
    tol, tol_v = (max(8 * np.abs(a - b).max(), floor) for a, b in ((r32, want), (v32, want_v)))
    err, err_v = np.abs(got - want).max(), np.abs(got_v - want_v).max()
    print("f32 vs f64 reference: rgb %.3g var %.3g; kernel: rgb %.3g var %.3g" % (tol / 8, tol_v / 8, err, err_v))
    assert np.isfinite(got).all() and err <= tol and err_v <= tol_v
    passed = ((mask >> (tags >> 30)) & 1) == 0
    assert np.array_equal(got[passed], c0[passed][:, :3]) and np.array_equal(got_v[passed], c0[passed][:, 3])
    assert mask == 0xF or passed.any() or (h, w) == (1, 1)


@pytest.mark.parametrize("h,w", [(3, 5), (23, 37)])
def test_no_levels_is_the_resolve_by_counts(h, w):
    acc, counts, mom, _, _ = synthetic(h, w)
    got, got_v, got_p, bufs = run_filter(h, w, preview=True, levels=0)
    out = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
    pre = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0")
    rtw.resolve_fast_counts(bufs[0].data_ptr(), bufs[1].data_ptr(), (h, w), out.data_ptr(), pre.data_ptr(), stream=stream())
    assert np.array_equal(got, out.cpu().numpy()) and np.array_equal(got_p, pre.cpu().numpy()) and got.any()
    for y, x in np.ndindex(h, w):
        n, A, B = int(counts[y, x]), int(mom[y, x, 0]), int(mom[y, x, 1])
        L = sum(Fraction(float(c)) for c in got[y, x])
        want = 0 if n == 0 else L * L if n == 1 else Fraction(n * B - A * A, (1 << 32) * n * n * (n - 1))
        assert abs(Fraction(float(got_v[y, x])) - want) <= want * Fraction(1, 1 << 22), (y, x, n)


def inside_glass(h, w, depth):
    objs = [((0.0, 0.0, 0.0), 1.0, (po.DIELECTRIC, (0.0, 0.0, 0.0), 0.0, 1.5)),
            ((0.3, 0.0, -0.5), 0.2, (po.LAMBERTIAN, (0.4, 0.2, 0.1), 0.0, 0.0)),
            ((0.0, -101.0, 0.0), 100.0, (po.LAMBERTIAN, (0.5, 0.5, 0.5), 0.0, 0.0))]
    return po.Camera(h, w, depth, 1.0, 70.0, (0.0, 0.0, 0.2), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 0.6, 1.0), objs


GUIDE_CASES = {"complex": fc.builtin("complex"), "simple": fc.builtin("simple"), "inside_glass": inside_glass}


@functools.lru_cache(maxsize=None)
def guide_truth(name, h=20, w=33):
    """The case and, per pixel, [(tag, normal)] of the unperturbed centre ray and fc.RUNS jiggled ones."""
    cam, objs = GUIDE_CASES[name](h, w, 10)
    P = fm.Prepared(cam, objs, 0, SEED)
    rc = fm.rounded_camera(cam)
    rc.defocus_angle = 0.0  # no disk: the origin is look_from
    rng = random.Random(fc.PROBE_SEED)
    runs = {}
    for y in range(h):
        for x in range(w):
            orig, d0 = po.get_ray(rc, x, y, P.offsets[0], None)
            runs[(x, y)] = []
            for r in range(1 + fc.RUNS):
                d = d0 if r == 0 else fm._jiggle(d0, (fc.EPS, rng))
                hit = P.hit(orig, d)
                runs[(x, y)].append((0xFFFFFFFF, po.unit(d)) if hit is None else
                                    ((P.scene[hit[1]][2][0] << 30) | hit[1], hit[0][2]))
    return types.SimpleNamespace(cam=cam, objs=objs, h=h, w=w, depth=10), runs


@pytest.mark.parametrize("name", list(GUIDE_CASES))
def test_guides_against_the_f64_closest_hit(name):
    c, runs = guide_truth(name)
    sess, cam = fc.gpu_session(c)
    g = torch.zeros((c.h, c.w, 4), dtype=torch.float32, device="cuda:0")
    sess.guides_fast(cam, g.data_ptr(), stream=stream())
    st = sess.stats()
    assert st.pixels == st.segments == c.h * c.w
    g = g.cpu().numpy()
    got_tag, unstable, flipped = g[..., 3].view(np.uint32), 0, 0
    for (x, y), rr in runs.items():
        if len({t for t, _ in rr}) > 1:
            unstable += 1
            assert got_tag[y, x] in {t for t, _ in rr}
            continue
        move = max(abs(a - b) for _, nr in rr[1:] for a, b in zip(nr, rr[0][1]))
        assert got_tag[y, x] == rr[0][0], (x, y)
        assert np.abs(g[y, x, :3] - rr[0][1]).max() <= max(2.0 ** -12, 4 * move), (x, y)
        flipped += rr[0][0] >> 30 == 2
    assert unstable <= 0.05 * len(runs) and (name != "inside_glass" or flipped > len(runs) // 2)


@pytest.mark.parametrize("tol", [0.0, 0.1])
def test_driver_is_its_steps_by_hand(tol):
    h, w, s, m0, batch = 24, 40, 4, 4, 4
    cam, sph, n, mt, nm = rtw.builtin_scene("complex", SEED, h, w, 12)
    sess = rtw.Session(0)
    sess.set_scene(sph, n, mt, nm)
    frame, var, counts, info = sess.render_fast_denoised(cam.raw, s, SEED, tol, min_samples=m0, batch=batch)
    acc = torch.zeros((h, w, 3), dtype=torch.int64, device="cuda:0")
    mom = torch.zeros((h, w, 2), dtype=torch.int64, device="cuda:0")
    cnt, lst = (torch.zeros((h, w), dtype=torch.int32, device="cuda:0") for _ in range(2))
    n_list = torch.zeros((1,), dtype=torch.int32, device="cuda:0")
    ptrs = acc.data_ptr(), mom.data_ptr(), cnt.data_ptr()
    sess.accumulate_fast_list(cam.raw, s, SEED, *ptrs, m0, stream=stream())
    while True:
        rtw.adaptive_select(cnt.data_ptr(), mom.data_ptr(), (h, w), s * s, rtw.to_q16(tol, 65535), rtw.to_q16(0.05, 1 << 24),
                            lst.data_ptr(), n_list.data_ptr(), stream=stream())
        if n_list.item() == 0:
            break
        sess.accumulate_fast_list(cam.raw, s, SEED, *ptrs, batch, list_ptr=lst.data_ptr(), n_list_ptr=n_list.data_ptr(),
                                  stream=stream())
    g = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
    want, want_v = torch.zeros_like(frame), torch.zeros_like(var)
    sess.guides_fast(cam.raw, g.data_ptr(), stream=stream())
    rtw.denoise_fast(acc.data_ptr(), cnt.data_ptr(), mom.data_ptr(), g.data_ptr(), (h, w), out_ptr=want.data_ptr(),
                     var_ptr=want_v.data_ptr(), stream=stream())
    assert torch.equal(frame, want) and torch.equal(var, want_v) and torch.equal(counts, cnt) and want.any()
    assert info["samples"] == cnt.sum().item() and info["denoise_ms"] > 0 and (tol == 0) == bool((cnt == s * s).all())


def test_cli_denoise_writes_the_filtered_frame(tmp_path):
    h, w, s = 24, 40, 4
    cam, sph, n, mt, nm = rtw.builtin_scene("complex", SEED, h, w, 12)
    sess = rtw.Session(0)
    sess.set_scene(sph, n, mt, nm)
    frame, _, _, _ = sess.render_fast_denoised(cam.raw, s, SEED)
    cli, out = os.path.join(os.path.dirname(rtw.LIB_PATH), "rtw_cli"), tmp_path / "cli.png"
    base = [cli, "-h", str(h), "-w", str(w), "-s", str(s), "-d", "12", "--seed", str(SEED), "--gpus", "1"]
    r = subprocess.run(base + ["--mode", "fast", "--denoise", "--png", "--out", str(out)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "denoise: 5 levels" in r.stdout, r.stderr
    png = rtw.png_device(frame.data_ptr(), frame.shape, fast=True, stream=stream())
    assert np.array_equal(decode(out.read_bytes())[0], decode(png)[0])
    r = subprocess.run(base + ["--mode", "fast", "--denoise", "--passes", "2"], capture_output=True, text=True, timeout=30)
    assert r.returncode == 1 and "--denoise" in r.stderr


P16 = 4096  # a non-null, 16-byte aligned address: the checks come before any device work


@pytest.mark.parametrize("code,ptrs,shape,prm", [
    (-1, (0, P16, P16, P16, P16), (4, 6), {}), (-1, (P16, 0, P16, P16, P16), (4, 6), {}),
    (-1, (P16, P16, 0, P16, P16), (4, 6), {}), (-1, (P16, P16, P16, 0, P16), (4, 6), {}),
    (-1, (P16, P16, P16, P16, 0), (4, 6), {}), (-1, (P16, P16, P16 + 8, P16, P16), (4, 6), {}),
    (-1, (P16, P16, P16, P16 + 4, P16), (4, 6), {}), (-1, (P16,) * 5, (4, 6), dict(levels=9)),
    (-1, (P16,) * 5, (4, 6), dict(normal_log2=9)), (-1, (P16,) * 5, (4, 6), dict(filter_mask=16)),
    (-1, (P16,) * 5, (4, 6), dict(sigma_l=-1.0)), (-1, (P16,) * 5, (4, 6), dict(sigma_l=float("nan"))),
    (-2, (P16,) * 5, (0, 6), {}), (-2, (P16,) * 5, (4, 0), {})])
def test_argument_errors_come_before_device_work(code, ptrs, shape, prm):
    with pytest.raises(rtw.RtwError) as e:
        rtw.denoise_fast(*ptrs[:4], shape, out_ptr=ptrs[4], **prm)
    assert e.value.code == code
