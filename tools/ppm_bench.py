"""Times the device output stage (rtw_format_ppm_device, rtw_quantise_host) against the
host route it can replace (download the frame, then rtw_format_ppm), in one process on
one GPU, alternating the two routes; medians of --reps timed calls after --warmup.
Frames: the headline render (complex, 1200x675, s10, d50) in parity (f64) and fast
(f32) mode, and one random 4096x2304 f64 frame. Every device text is compared with the
host writer's before it is timed. Prints one JSON line per frame.

    python tools/ppm_bench.py [--reps 15] [--warmup 3] [--small]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import raytracing_in_a_weekend_rust_amd as rtw  # noqa: E402
from raytracing_in_a_weekend_rust_amd._capi import check, lib  # noqa: E402


def measure(name, dev, reps, warmup):
    h, w = dev.shape[0], dev.shape[1]
    fast = dev.dtype == torch.float32
    host = torch.empty(dev.shape, dtype=dev.dtype)  # pageable, as a caller's buffer is
    text_d = np.empty(12 * h * w + 64, dtype=np.uint8)
    text_h = np.empty_like(text_d)
    rgb8 = np.empty((h, w, 3), dtype=np.uint8)
    p_d, p_h = text_d.ctypes.data_as(C.c_char_p), text_h.ctypes.data_as(C.c_char_p)

    def device_route():
        return check(lib.rtw_format_ppm_device(0, C.c_void_p(dev.data_ptr()), int(fast), w, h, None, p_d,
                                               text_d.size, None))

    def download():
        host.copy_(dev)
        torch.cuda.synchronize()

    def host_route():
        download()
        fb = host.numpy() if not fast else host.numpy().astype(np.float64)  # the CLI widens f32 the same way
        return check(lib.rtw_format_ppm(fb.ctypes.data_as(C.POINTER(C.c_double)), w, h, p_h, text_h.size))

    def quantise_route():
        check(lib.rtw_quantise_host(0, C.c_void_p(dev.data_ptr()), int(fast), w, h, C.c_void_p(rgb8.ctypes.data),
                                    None, None))

    n = device_route()
    assert n == host_route() and np.array_equal(text_d[:n], text_h[:n]), "device text differs from the host writer's"
    routes = {"device_ms": device_route, "host_ms": host_route, "quantise_rgb8_ms": quantise_route,
              "download_frame_ms": download}
    times = {k: [] for k in routes}
    kern = {"quantise_ms": [], "scan_ms": [], "emit_ms": [], "download_ms": []}
    for it in range(warmup + reps):
        for k, fn in routes.items():  # alternating: every route sees the same box
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e3
            if it >= warmup:
                times[k].append(dt)
            if k == "device_ms" and it >= warmup:
                st = rtw.ppm_device_stats(0)
                for kk in kern:
                    kern[kk].append(st[kk])
    med = {k: round(statistics.median(v), 4) for k, v in {**times, **{"kernel_" + k: v for k, v in kern.items()}}.items()}
    st = rtw.ppm_device_stats(0)
    print(json.dumps({"frame": name, "width": w, "height": h, "dtype": "f32" if fast else "f64",
                      "frame_bytes": dev.numel() * dev.element_size(), "text_bytes": int(n), "tiles": st["tiles"],
                      "reps": reps, "warmup": warmup, **med,
                      "device_over_host": round(med["device_ms"] / med["host_ms"], 4),
                      "min": {k: round(min(v), 4) for k, v in times.items()},
                      "max": {k: round(max(v), 4) for k, v in times.items()},
                      "build_id": rtw.build_id()}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="tiny frames (a rehearsal of the script)")
    a = ap.parse_args()
    hh, ww, s, big = (27, 48, 2, (96, 128)) if a.small else (675, 1200, 10, (2304, 4096))
    cam, sph, n, mt, nm = rtw.builtin_scene("complex", rtw.DEFAULT_SEED, hh, ww, 50)
    sess = rtw.Session(0)
    sess.set_scene(sph, n, mt, nm)
    f64 = torch.zeros((hh, ww, 3), dtype=torch.float64, device="cuda:0")
    f32 = torch.zeros((hh, ww, 3), dtype=torch.float32, device="cuda:0")
    sess.render(cam.raw, s, rtw.DEFAULT_SEED, f64.data_ptr())
    sess.stats()
    sess.render_fast(cam.raw, s, rtw.DEFAULT_SEED, f32.data_ptr())
    sess.stats()
    measure("headline_parity", f64, a.reps, a.warmup)
    measure("headline_fast", f32, a.reps, a.warmup)
    del f64, f32
    gen = torch.Generator(device="cuda:0").manual_seed(7)
    rnd = torch.rand((big[0], big[1], 3), dtype=torch.float64, device="cuda:0", generator=gen)
    measure("random_%dx%d" % (big[1], big[0]), rnd, max(5, a.reps // 2), a.warmup)
    sess.close()


if __name__ == "__main__":
    main()
