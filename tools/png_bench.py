"""Times the device PNG encoder (rtw_png_device) against what a user does without it
(rtw_quantise_host, then the same per-row filter rule in numpy, then zlib at level 1 and
at level 6) and, for context, the P3 text route (rtw_format_ppm_device), in one process on
one GPU, alternating the routes; medians of --reps timed calls after --warmup. Frames: the
headline render (complex, 1200x675, s10, d50) in parity (f64) and fast (f32) mode, and one
4096x2304 fast-mode render (s2, d10). Every device PNG is decoded (stdlib) and compared
with rtw_quantise_host's image before it is timed. Sizes: the device file against the host
route's, and against zlib's Z_RLE and default strategies on the same filtered stream.
One JSON line per frame, printed and written to profiles/png_device/png_bench.jsonl.

    python tools/png_bench.py [--reps 15] [--warmup 3] [--small]
"""
import argparse
import binascii
import ctypes as C
import json
import os
import statistics
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import raytracing_in_a_weekend_rust_amd as rtw  # noqa: E402
from raytracing_in_a_weekend_rust_amd._capi import check, lib  # noqa: E402

HEAD = b"\x89PNG\r\n\x1a\n"


def chunk(kind, data):
    return len(data).to_bytes(4, "big") + kind + data + binascii.crc32(kind + data).to_bytes(4, "big")


def host_filter(img):
    """The filtered stream by the encoder's rule (least sum of |signed residual| among None, Sub, Up)."""
    h = img.shape[0]
    a = img.reshape(h, -1)
    left, up = np.zeros_like(a), np.zeros_like(a)
    left[:, 3:], up[1:] = a[:, :-3], a[:-1]
    res = np.stack([a, a - left, a - up])  # uint8: wraps as the filters do
    pick = np.argmin(np.abs(res.view(np.int8).astype(np.int16)).sum(axis=2), axis=0)
    out = np.empty((h, 1 + a.shape[1]), dtype=np.uint8)
    out[:, 0] = pick
    out[:, 1:] = res[pick, np.arange(h)]
    return out.tobytes()


def host_png(img, level):
    h, w = img.shape[:2]
    ihdr = w.to_bytes(4, "big") + h.to_bytes(4, "big") + bytes([8, 2, 0, 0, 0])
    return HEAD + chunk(b"IHDR", ihdr) + chunk(b"IDAT", zlib.compress(host_filter(img), level)) + chunk(b"IEND", b"")


def decode(png, h, w):
    """The image and the filtered stream of a device PNG (filters 0-2), CRCs checked."""
    assert png[:8] == HEAD
    p, idat = 8, None
    while p < len(png):
        n = int.from_bytes(png[p:p + 4], "big")
        assert binascii.crc32(png[p + 4:p + 8 + n]) == int.from_bytes(png[p + 8 + n:p + 12 + n], "big")
        if png[p + 4:p + 8] == b"IDAT":
            idat = png[p + 8:p + 8 + n]
        p += 12 + n
    raw = zlib.decompress(idat)
    rows = np.frombuffer(raw, np.uint8).reshape(h, 1 + 3 * w)
    img = np.zeros((h, w, 3), np.uint8)
    for y in range(h):
        r = rows[y, 1:].reshape(w, 3)
        if rows[y, 0] == 1:
            r = np.cumsum(r, axis=0, dtype=np.uint8)
        elif rows[y, 0] == 2 and y:
            r = r + img[y - 1]
        img[y] = r
    return img, raw


def deflated(raw, strategy):
    c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, strategy)
    return len(c.compress(raw) + c.flush())


def measure(name, dev, reps, warmup):
    h, w = dev.shape[0], dev.shape[1]
    fast = dev.dtype == torch.float32
    ptr = C.c_void_p(dev.data_ptr())
    rgb8 = np.empty((h, w, 3), dtype=np.uint8)
    text = np.empty(12 * h * w + 64, dtype=np.uint8)
    sizes = {}

    def device_route():
        sizes["device"] = len(rtw.png_device(dev.data_ptr(), dev.shape, fast=fast))

    def quantise_route():
        check(lib.rtw_quantise_host(0, ptr, int(fast), w, h, C.c_void_p(rgb8.ctypes.data), None, None))

    def host_route(level):
        quantise_route()
        sizes["host_zlib%d" % level] = len(host_png(rgb8, level))

    def ppm_route():
        check(lib.rtw_format_ppm_device(0, ptr, int(fast), w, h, None, text.ctypes.data_as(C.c_char_p), text.size,
                                        None))

    quantise_route()
    png = rtw.png_device(dev.data_ptr(), dev.shape, fast=fast)
    img, raw = decode(png, h, w)
    assert np.array_equal(img, rgb8), "the device PNG does not decode to the quantised frame"
    assert decode(host_png(rgb8, 1), h, w)[1] == raw, "the host route filters differently"
    routes = {"device_ms": device_route, "host_zlib1_ms": lambda: host_route(1), "host_zlib6_ms": lambda: host_route(6),
              "quantise_rgb8_ms": quantise_route, "ppm_device_ms": ppm_route}
    stages = ["quantise_ms", "filter_ms", "plan_ms", "scan_ms", "emit_ms", "finish_ms", "download_ms"]
    times = {k: [] for k in routes}
    kern = {k: [] for k in stages}
    for it in range(warmup + reps):
        for k, fn in routes.items():  # alternating: every route sees the same box
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e3
            if it >= warmup:
                times[k].append(dt)
                if k == "device_ms":
                    st = rtw.png_device_stats(0)
                    for kk in stages:
                        kern[kk].append(st[kk])
    med = {k: round(statistics.median(v), 4) for k, v in {**times, **{"kernel_" + k: v for k, v in kern.items()}}.items()}
    st = rtw.png_device_stats(0)
    line = {"frame": name, "width": w, "height": h, "dtype": "f32" if fast else "f64",
            "rgb8_bytes": 3 * h * w, "filtered_bytes": len(raw), "png_bytes": len(png),
            "host_zlib1_bytes": sizes["host_zlib1"], "host_zlib6_bytes": sizes["host_zlib6"],
            "zlib_rle_bytes": deflated(raw, zlib.Z_RLE), "zlib_default_bytes": deflated(raw, zlib.Z_DEFAULT_STRATEGY),
            "tiles": st["tiles"], "stored_tiles": st["stored_tiles"],
            "rows": [st["rows_none"], st["rows_sub"], st["rows_up"]], "reps": reps, "warmup": warmup, **med,
            "device_over_host_zlib1": round(med["device_ms"] / med["host_zlib1_ms"], 4),
            "min": {k: round(min(v), 4) for k, v in times.items()},
            "max": {k: round(max(v), 4) for k, v in times.items()}, "build_id": rtw.build_id()}
    print(json.dumps(line), flush=True)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="tiny frames (a rehearsal of the script; nothing is written)")
    a = ap.parse_args()
    hh, ww, s, big = (27, 48, 2, (96, 128)) if a.small else (675, 1200, 10, (2304, 4096))
    sess = rtw.Session(0)
    lines = []

    def render(h, w, s, depth, dtype):
        cam, sph, n, mt, nm = rtw.builtin_scene("complex", rtw.DEFAULT_SEED, h, w, depth)
        sess.set_scene(sph, n, mt, nm)
        fb = torch.zeros((h, w, 3), dtype=dtype, device="cuda:0")
        (sess.render_fast if dtype == torch.float32 else sess.render)(cam.raw, s, rtw.DEFAULT_SEED, fb.data_ptr())
        sess.stats()
        return fb

    lines.append(measure("headline_parity", render(hh, ww, s, 50, torch.float64), a.reps, a.warmup))
    lines.append(measure("headline_fast", render(hh, ww, s, 50, torch.float32), a.reps, a.warmup))
    lines.append(measure("fast_%dx%d" % (big[1], big[0]), render(big[0], big[1], 2, 10, torch.float32),
                         max(5, a.reps // 3), a.warmup))
    sess.close()
    if not a.small:
        out = os.path.join(ROOT, "profiles", "png_device")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "png_bench.jsonl"), "w") as f:
            f.writelines(json.dumps(x) + "\n" for x in lines)


if __name__ == "__main__":
    main()
