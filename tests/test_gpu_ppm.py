"""The output stage on the device (rtw_quantise_device / rtw_format_ppm_device,
csrc/rtw_ppm.hip): a frame in HBM becomes the reference's RGB8 values and P3 text
(color.rs:196-247), byte for byte what the oracle's formatter (a pow call per
channel; checker only) writes for the same values."""
import math
import os
import subprocess

import numpy as np
import pytest

import raytracing_in_a_weekend_rust_amd as rtw
from oracle import oracle_ctypes as orc
from tests.golden_io import load

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

T = 4096  # channels per text tile (rtw_ppm.h kPpmTile); T % 3 == 1, so 3*W is T - 1 or T + 2 at best


def check(fb, wide_expected=0):
    """Device text and RGB8 of `fb` (f32: fast-mode frame, compared on the widened values)."""
    dev = torch.from_numpy(fb).to("cuda:0")
    fast = fb.dtype == np.float32
    ref = orc.format_ppm(fb.astype(np.float64))
    text, wide = rtw.format_ppm_device(dev.data_ptr(), fb.shape, fast=fast)
    assert wide == wide_expected
    assert text == ref
    want = np.array([min(int(v), 255) for v in ref.split()[4:]], dtype=np.uint8).reshape(fb.shape)
    img, wide = rtw.quantise_device(dev.data_ptr(), fb.shape, fast=fast)
    assert wide == wide_expected and np.array_equal(img, want)
    out = torch.zeros(fb.shape, dtype=torch.uint8, device="cuda:0")
    _, wide = rtw.quantise_device(dev.data_ptr(), fb.shape, fast=fast, out_dev_ptr=out.data_ptr())
    assert wide == wide_expected and np.array_equal(out.cpu().numpy(), want)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("h,w", [
    (1, 1), (3, 5),            # one pack; rows that end inside a lane's 4-pack (3*W % 4 = 3)
    (1, 1365), (1, 1366),      # 3*W = T - 1 and T + 2: either side of a tile boundary
    (2, 1365),                 # the first row ends one channel before the boundary
    (24, 199),                 # 3.5 tiles, every row ends inside a tile
])
def test_shapes(h, w, dtype):
    rng = np.random.default_rng(1000 * h + w)
    check((rng.random((h, w, 3)) ** 4).astype(dtype))  # 1-, 2- and 3-digit values


def test_every_threshold():
    """T_k +- 300 ulps (k = 1..255; the device reads pow's own byte within 64 ulps of
    T_k), random values, and the specials that are not above 1."""
    def q(b):
        return int(math.pow(float(np.array([b], dtype=np.uint64).view(np.float64)[0]), 1. / 2.2) * 255.)
    t, lo = [], 0
    for k in range(1, 256):  # T_k: the smallest double whose value is >= k, by bisection over bit patterns
        hi = int(np.array([1.0]).view(np.uint64)[0])
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if q(mid) >= k else (mid, hi)
        t.append(hi)
    near = (np.array(t, dtype=np.int64)[:, None] + np.arange(-300, 301)[None, :]).ravel().view(np.float64)
    near = near[near <= 1.0]  # T_255 is one ulp below 1
    rng = np.random.default_rng(11)
    vals = np.concatenate([near, rng.random(300_000), rng.random(200_000) ** 8,
                           [0.0, -0.0, 1.0, np.nextafter(1.0, 0.0), 5e-324, -1e-300, math.nan]])
    vals = np.concatenate([vals, np.zeros((-len(vals)) % 3000)])
    check(vals.reshape(-1, 1000, 3))


def test_wide_fallback():
    rng = np.random.default_rng(5)
    fb = rng.random((40, 30, 3)) * 1.2
    fb[1, 2] = [math.inf, 1e300, 3.0]
    fb[7, 0, 1] = math.nan
    check(fb, wide_expected=np.count_nonzero(fb > 1))


def test_from_a_render():
    fix = load("render_complex_16x9_s1_d10")
    seed = int(fix["seed"], 16)
    cam, sph, n, mt, nm = rtw.builtin_scene(fix["scene"], seed, fix["height"], fix["width"], fix["max_depth"])
    sess = rtw.Session(0)
    sess.set_scene(sph, n, mt, nm)
    stream = torch.cuda.current_stream().cuda_stream
    out = torch.zeros((9, 16, 3), dtype=torch.float64, device="cuda:0")
    sess.render(cam.raw, fix["samples_sqrt"], seed, out.data_ptr(), stream=stream)
    text, wide = rtw.format_ppm_device(out.data_ptr(), out.shape, stream=stream)
    assert (text.decode(), wide) == (fix["ppm"], 0)
    fast = torch.zeros((9, 16, 3), dtype=torch.float32, device="cuda:0")
    sess.render_fast(cam.raw, 2, seed, fast.data_ptr(), stream=stream)
    text, wide = rtw.format_ppm_device(fast.data_ptr(), fast.shape, fast=True, stream=stream)
    assert text == rtw.format_ppm(fast.cpu().numpy().astype(np.float64)) and wide == 0
    sess.close()


@pytest.mark.parametrize("mode", ["parity", "fast"])
def test_cli_device_ppm_writes_the_same_file(tmp_path, mode):
    cli = os.path.join(os.path.dirname(rtw.LIB_PATH), "rtw_cli")
    files = []
    for flags in ([], ["--device-ppm"]):
        out = tmp_path / f"img{len(flags)}.ppm"
        r = subprocess.run([cli, "-h", "18", "-w", "32", "-s", "3", "-d", "12", "--seed", "1764892800123",
                            "--mode", mode, "--gpus", "1", "--out", str(out), *flags],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "Finished succesfully" in r.stdout, r.stderr
        files.append(out.read_bytes())
    assert files[0] == files[1] and files[0].startswith(b"P3\n32 18\n255\n")
