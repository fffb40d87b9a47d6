"""The device PNG encoder (rtw_png_device / rtw_png_rgb8_device, csrc/rtw_png.hip):
every file is taken apart with the standard library alone (chunk CRCs by binascii,
the IDAT by zlib.decompress, which checks every code and the Adler-32) and must
decode to the RGB8 image that went in."""
import binascii
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import raytracing_in_a_weekend_rust_amd as rtw
from tests.golden_io import load

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

T = rtw.PNG_TILE  # filtered bytes per deflate tile; a filtered row is 1 + 3W bytes, so T - 1 and T + 2 at best


def decode(png):
    """(image, filtered stream) of a PNG made of IHDR, one IDAT, IEND with filters 0-2."""
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    chunks, p = [], 8
    while p < len(png):
        n = int.from_bytes(png[p:p + 4], "big")
        body = png[p + 4:p + 8 + n]
        assert binascii.crc32(body) == int.from_bytes(png[p + 8 + n:p + 12 + n], "big")
        chunks.append((body[:4], body[4:]))
        p += 12 + n
    assert [c[0] for c in chunks] == [b"IHDR", b"IDAT", b"IEND"] and chunks[2][1] == b""
    w, h, *rest = struct.unpack(">IIBBBBB", chunks[0][1])
    assert rest == [8, 2, 0, 0, 0]  # 8-bit, RGB, deflate, filter method 0, no interlace
    raw = zlib.decompress(chunks[1][1])
    rows = np.frombuffer(raw, np.uint8).reshape(h, 1 + 3 * w)
    img = np.zeros((h, w, 3), np.uint8)
    for y in range(h):
        f, r = rows[y, 0], rows[y, 1:].reshape(w, 3)
        assert f <= 2
        if f == 1:
            r = np.cumsum(r, axis=0, dtype=np.uint8)
        if f == 2 and y:
            r = r + img[y - 1]
        img[y] = r
    return img, raw


def encode(img, filter=None):
    dev = torch.from_numpy(img).to("cuda:0")
    png = rtw.png_device(dev.data_ptr(), img.shape, rgb8=True, filter=filter)
    out, raw = decode(png)
    st = rtw.png_device_stats()
    assert np.array_equal(out, img)
    assert (st["png_bytes"], st["filtered_bytes"], st["tiles"]) == (len(png), len(raw), -(-len(raw) // T))
    return png, raw, st


@pytest.mark.parametrize("h,w", [
    (1, 1), (1, 2), (3, 5),
    (1, (T - 2) // 3), (1, (T + 1) // 3),  # one filtered row of T - 1 and of T + 2 bytes
    (2, (T - 2) // 3),                     # the first row ends one byte before the tile boundary
    (3, 796),                              # 3.5 tiles, every row straddles a boundary
    (400, 64),
])
def test_random_bytes_every_shape(h, w):
    """Incompressible: the tiles fall back to stored blocks and the file stays near the stream's size."""
    img = np.random.default_rng(1000 * h + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    png, raw, st = encode(img)
    assert len(png) <= len(raw) + 16 * st["tiles"] + 128
    if len(raw) > 2 * T:
        assert st["stored_tiles"] >= st["tiles"] - 1 and len(zlib.compress(raw)) >= len(raw)  # zlib stores it too


def gradient(h=40, w=300):
    y, x, c = np.meshgrid(np.arange(h), np.arange(w), np.arange(3), indexing="ij")
    return ((2 * x + 3 * y + 40 * c + np.random.default_rng(3).integers(0, 3, (h, w, 3))) & 255).astype(np.uint8)


def reference_filters(img):
    """The per-row rule on the CPU: least sum of |signed residual| among None, Sub, Up; ties to the lower type."""
    a = img.reshape(img.shape[0], -1).astype(np.int64)
    left, up = np.zeros_like(a), np.zeros_like(a)
    left[:, 3:], up[1:] = a[:, :-3], a[:-1]
    cost = [np.abs(((r + 128) & 255) - 128).sum(axis=1) for r in (a, a - left, a - up)]
    return np.bincount(np.argmin(np.stack(cost), axis=0), minlength=3)


def test_one_colour_needs_the_matches():
    img = np.full((400, 64, 3), (200, 30, 77), dtype=np.uint8)
    png, raw, _ = encode(img)
    assert len(png) < len(raw) / 16  # a Huffman-only encoder cannot go below 1/8


def test_run_ladder():
    """Runs of every length 1..600 end to end: the splits at 258, remainders of 1 and 2, runs across tile edges."""
    runs = np.concatenate([np.full(k, 1 + k % 250, dtype=np.uint8) for k in range(1, 601)])
    img = np.zeros(86 * 700 * 3, dtype=np.uint8)
    img[:runs.size] = runs
    png, raw, st = encode(img.reshape(86, 700, 3), filter=0)
    assert st["stored_tiles"] == 0 and len(png) < len(raw) / 8


def test_fibonacci_histogram():
    """Counts 1, 1, 2, .. 6765 of 20 symbols: a Huffman code of the whole image would be 19 bits deep."""
    fib = [1, 1]
    while len(fib) < 20:
        fib.append(fib[-1] + fib[-2])
    vals = np.repeat(np.arange(1, 21, dtype=np.uint8), fib)
    np.random.default_rng(8).shuffle(vals)
    encode(vals[:100 * 59 * 3].reshape(100, 59, 3), filter=0)


def test_adaptive_filter_follows_the_rule():
    img = gradient()
    want = reference_filters(img)
    assert want[1] + want[2] > img.shape[0] / 2  # the input is one a predictor helps
    _, _, st = encode(img)
    assert [st["rows_none"], st["rows_sub"], st["rows_up"]] == list(want)


@pytest.mark.parametrize("f", [0, 1, 2])
def test_forced_filter(f):
    img = gradient()
    _, raw, st = encode(img, filter=f)
    assert set(raw[::1 + 3 * img.shape[1]]) == {f} and st[("rows_none", "rows_sub", "rows_up")[f]] == img.shape[0]


def test_from_a_render():
    fix = load("render_complex_16x9_s1_d10")
    seed = int(fix["seed"], 16)
    cam, sph, n, mt, nm = rtw.builtin_scene(fix["scene"], seed, fix["height"], fix["width"], fix["max_depth"])
    sess = rtw.Session(0)
    sess.set_scene(sph, n, mt, nm)
    stream = torch.cuda.current_stream().cuda_stream
    for fast, dtype in ((False, torch.float64), (True, torch.float32)):
        out = torch.zeros((9, 16, 3), dtype=dtype, device="cuda:0")
        (sess.render_fast if fast else sess.render)(cam.raw, 2, seed, out.data_ptr(), stream=stream)
        png = rtw.png_device(out.data_ptr(), out.shape, fast=fast, stream=stream)
        want, _ = rtw.quantise_device(out.data_ptr(), out.shape, fast=fast, stream=stream)
        assert np.array_equal(decode(png)[0], want) and want.any()
    sess.close()


@pytest.mark.parametrize("mode", ["parity", "fast"])
def test_cli_png_holds_the_ppm_values(tmp_path, mode):
    cli = os.path.join(os.path.dirname(rtw.LIB_PATH), "rtw_cli")
    outs = [tmp_path / "img.ppm", tmp_path / "img.png"]
    for out, flags in zip(outs, ([], ["--png"])):
        r = subprocess.run([cli, "-h", "18", "-w", "32", "-s", "3", "-d", "12", "--seed", "1764892800123",
                            "--mode", mode, "--gpus", "1", "--out", str(out), *flags],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "Finished succesfully" in r.stdout, r.stderr
    want = np.array([min(int(v), 255) for v in outs[0].read_text().split()[4:]], dtype=np.uint8)
    assert np.array_equal(decode(outs[1].read_bytes())[0], want.reshape(18, 32, 3))


def test_an_independent_decoder_agrees():
    Image = pytest.importorskip("PIL.Image")
    import io
    img = gradient()
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(encode(img)[0])).convert("RGB")), img)
