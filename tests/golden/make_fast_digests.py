"""Pins the bits of f32 fast mode (tests/test_gpu_fast_golden.py).

Every other fast-mode test compares the library with itself (a split of the lattice with the
one-shot frame, the list kernel with single-sample passes), so a change that moved all routes
alike would pass them. This writes the SHA-256 of the raw buffer bytes (little-endian, as
they lie in device memory) that each route produces on the smallest shapes where it can
still go wrong, to fast_digests.json, with the `hipcc --version` line and the ARCH of the
library that made them. Needs a gfx950 GPU and the built library.

Routes (seed 1764892800123, final scene `complex` at depth 50 unless said otherwise):
  one-shot render_fast: 17x29 at s=0 and s=1, 20x33 at s=3, 18x32 at s=8 (64 samples: more
      than a wave over the 4 ring slots); a scene without BVH nodes (the linear scan,
      stats().accel == 0) at 12x12, s=3; depth 1 and shard (row_begin 1, row_step 3) of
      20x33 at s=3. Every non-empty built-in scene gets BVH nodes, so the scan's scene is
      three walls of radius 1e7 (Lambertian floor, metal back, glass side): spheres that
      large are tested before the walk ("always", rtw_accel.h) and no node is left.
  accumulate_fast: the whole lattice by the lane kernel (20x33, s=3: 9 samples < 16) and by
      the ring kernel (18x32, s=8); one strided pass (k_first 1, k_step 3, k_count 21)
  accumulate_fast_list (18x32, s=8, k_mul = lattice_stride(64)): the null list with m=4,
      then m=40; an explicit list (every third pixel, one index >= npix, one pixel already
      at N) likewise. Sums, moments and counts after each round.
  resolve_fast and resolve_fast_counts with both outputs, from the sums above.
sampled() is every case that traces samples; the test runs it a second time with the scene
read from global memory (RTW_AB=1 RTW_FAST_LDS=0) and wants the same digests.

Fast mode is f32 with FMA contraction allowed, so the bits belong to the compiler as well as
to the source: a compiler upgrade may legitimately move them. The test does not skip on a
toolchain mismatch; when it fails after an upgrade and `hipcc` in fast_digests.json differs
from the installed one, check that the library's own comparisons (test_gpu_fast.py,
test_gpu_progressive.py, test_gpu_adaptive.py) still pass, then regenerate on the GPU:

    python tests/golden/make_fast_digests.py
"""
import hashlib
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

import raytracing_in_a_weekend_rust_amd as rtw  # noqa: E402

SEED = 1764892800123
PATH = os.path.join(ROOT, "tests", "golden", "fast_digests.json")


def sha(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def stream():
    return torch.cuda.current_stream().cuda_stream


def session(scene, h, w, depth):
    cam, sph, n, mt, nm = rtw.builtin_scene(scene, SEED, h, w, depth)
    sess = rtw.Session(0)
    sess.set_scene(sph, n, mt, nm)
    return sess, cam.raw


def zeros(*shape, dtype=torch.int64):
    return torch.zeros(shape, dtype=dtype, device="cuda:0")


def scan_session(scene, h, w, depth):
    world = rtw.SceneBuilder()
    world.add(rtw.Sphere.new_world_obj(0., -1e7 - 0.5, -1., 1e7, rtw.Lambertian((0.8, 0.6, 0.2))))
    world.add(rtw.Sphere.new_world_obj(0., 0., -1e7 - 3., 1e7, rtw.Metal((0.7, 0.8, 0.9), 0.3)))
    world.add(rtw.Sphere.new_world_obj(-1e7 - 1.5, 0., -1., 1e7, rtw.Dielectric(1.5)))
    cam = rtw.Camera.new(h, w, depth, 1.0, 90., (0., 0., 0.), (0., 0., -1.), (0., 1., 0.), 0.5, 2.)
    sess = rtw.Session(0)
    sess.set_scene(*world.build().flatten())
    return sess, cam.raw


def one_shot(scene, h, w, depth, s, shard=None, accel=None):
    sess, cam = (scan_session if scene == "scan" else session)(scene, h, w, depth)
    out = zeros(shard[2] if shard else h, w, 3, dtype=torch.float32)
    sess.render_fast(cam, s, SEED, out.data_ptr(), stream=stream(), shard=shard)
    assert out.any() and (accel is None or sess.stats().accel == accel)
    return sha(out)


def list_rounds(sess, cam, s, h, w, lst, counts):
    """m=4 then m=40 on fresh sums; returns the digests and the final (acc, counts)."""
    acc, mom, out = zeros(h, w, 3), zeros(h, w, 2), {}
    n_list = torch.tensor([0 if lst is None else len(lst)], dtype=torch.int32, device="cuda:0")
    for m in (4, 40):
        sess.accumulate_fast_list(cam, s, SEED, acc.data_ptr(), mom.data_ptr(), counts.data_ptr(), m, None,
                                  0 if lst is None else lst.data_ptr(), n_list.data_ptr(), stream=stream())
        out["m%d" % m] = {"sums": sha(acc), "moments": sha(mom), "counts": sha(counts)}
    return out, acc, counts


def sampled(keep=None):
    """Digests of every case that traces samples. keep: a dict that receives the device
    buffers resolved() starts from."""
    d = {}
    for h, w, s in ((17, 29, 0), (17, 29, 1), (20, 33, 3), (18, 32, 8)):
        d["one_shot_%dx%d_s%d" % (h, w, s)] = one_shot("complex", h, w, 50, s, accel=2)
    d["one_shot_scan_12x12_s3"] = one_shot("scan", 12, 12, 50, 3, accel=0)
    d["one_shot_depth1_shard_20x33_s3"] = one_shot("complex", 20, 33, 1, 3, shard=(1, 3, 6))

    sess, cam = session("complex", 20, 33, 50)
    acc = zeros(20, 33, 3)
    sess.accumulate_fast(cam, 3, SEED, acc.data_ptr(), stream=stream())
    d["accumulate_lane_20x33_s3"] = sha(acc)

    h, w, s = 18, 32, 8
    n, npix = s * s, h * w
    sess, cam = session("complex", h, w, 50)
    whole = zeros(h, w, 3)
    sess.accumulate_fast(cam, s, SEED, whole.data_ptr(), stream=stream())
    d["accumulate_ring_18x32_s8"] = sha(whole)
    acc = zeros(h, w, 3)
    sess.accumulate_fast(cam, s, SEED, acc.data_ptr(), 1, 3, 21, stream=stream())
    d["accumulate_pass_1_3_21_18x32_s8"] = sha(acc)

    d["list_null_18x32_s8"], _, _ = list_rounds(sess, cam, s, h, w, None, zeros(h, w, dtype=torch.int32))
    lst = torch.cat([torch.arange(0, npix, 3), torch.tensor([npix + 5])]).to(torch.int32).cuda()
    counts = zeros(h, w, dtype=torch.int32)
    counts.view(-1)[3] = n  # listed, and already at the lattice's end
    d["list_explicit_18x32_s8"], lacc, lcounts = list_rounds(sess, cam, s, h, w, lst, counts)
    assert whole.any() and lacc.any() and 0 < (lcounts == 0).sum() < npix
    if keep is not None:
        keep.update(whole=whole, n=n, list_acc=lacc, list_counts=lcounts, shape=(h, w))
    return d


def resolved(keep):
    h, w = keep["shape"]
    d = {}
    for name in ("resolve_fast", "resolve_fast_counts"):
        frame, preview = zeros(h, w, 3, dtype=torch.float32), zeros(h, w, 4, dtype=torch.uint8)
        if name == "resolve_fast":
            rtw.resolve_fast(keep["whole"].data_ptr(), (h, w), keep["n"], frame.data_ptr(), preview.data_ptr(),
                             stream=stream())
        else:
            rtw.resolve_fast_counts(keep["list_acc"].data_ptr(), keep["list_counts"].data_ptr(), (h, w),
                                    frame.data_ptr(), preview.data_ptr(), stream=stream())
        d[name + "_18x32"] = {"frame": sha(frame), "preview": sha(preview)}
    return d


def digests():
    keep = {}
    d = sampled(keep)
    d.update(resolved(keep))
    return d


def toolchain():
    try:
        out = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--version"], capture_output=True,
                             text=True, timeout=60).stdout
        hipcc = next((ln.strip() for ln in out.splitlines() if ln.startswith("HIP version")), out.splitlines()[0].strip())
    except (OSError, IndexError, subprocess.SubprocessError):
        hipcc = "unknown"
    m = re.search(r"abi \d+, (.*), build", rtw.api.lib.rtw_version().decode())
    return {"hipcc": hipcc, "ARCH": m.group(1) if m else "unknown"}


def main():
    out = {**toolchain(), "seed": SEED, "digests": digests()}
    with open(PATH, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d cases, %s, %s" % (os.path.basename(PATH), len(out["digests"]), out["hipcc"], out["ARCH"]))


if __name__ == "__main__":
    main()
