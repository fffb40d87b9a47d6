"""Times denoised fast mode (rtw_session_render_fast_denoised) against the raw frame of the same
route and against the uniform rtw_session_render_fast frames, on the final scene (complex,
1200x675, depth 50), in one process on one GPU. The error is taken as tools/adaptive_bench.py
takes it: against a fast-mode render at s = 64 (4096 samples per pixel) with another seed, on
8-bit values round(255 sqrt(clamp(x, 0, 1))): RMSE and the 99th percentile of |delta| over all
channels. A timed call is host wall time from the enqueue to the end of a stream synchronise;
every route runs once per repetition, the routes alternating; medians of --reps after --warmup,
with the spread beside them. Lines written (one JSON object each, printed and appended to --out):
  uniform   render_fast at s = 1..23: time, error (the frames of equal time come from these)
  route     uniform s = 1, 2, 4, 8, 11, 23 (tolerance 0) and adaptive tol 0.2 / 0.1 / 0.05 (s = 23),
            each raw and denoised: time, the guides' and the filter's time on their own, error,
            and the uniform frame of about equal total time beside the denoised one
  levels    rtw_denoise_fast alone at levels = 0..8 (HIP events): the cumulative time, the
            differences (level l's kernel) and the bytes the algorithm moves per second

    python tools/denoise_bench.py [--reps 7] [--warmup 2] [--small] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import raytracing_in_a_weekend_rust_amd as rtw  # noqa: E402

SEED = rtw.DEFAULT_SEED
UNIFORM = (1, 2, 4, 8, 11, 23)
TOLS = (0.2, 0.1, 0.05)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--small", action="store_true", help="a tiny image (a rehearsal of the script; nothing is written)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise", "bench.jsonl"))
    a = ap.parse_args()
    h, w, big, s_ref = (27, 48, 5, 9) if a.small else (675, 1200, 23, 64)
    uniform_s = tuple(s for s in UNIFORM if s <= big)
    cam, sph, n, mt, nm = rtw.builtin_scene("complex", SEED, h, w, 50)
    sess = rtw.Session(0)
    sess.set_scene(sph, n, mt, nm)
    st = torch.cuda.current_stream().cuda_stream
    frame = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")

    def to8(x):
        return (x.clamp(0, 1).sqrt() * 255).round()

    ref = torch.zeros_like(frame)
    sess.render_fast(cam.raw, s_ref, SEED + 1, ref.data_ptr(), stream=st)
    torch.cuda.synchronize()
    ref8 = to8(ref)

    def error(x):
        d = (to8(x) - ref8).abs().flatten()
        return {"rmse8": round(d.square().mean().sqrt().item(), 4), "p99_8": d.kthvalue(int(0.99 * d.numel())).values.item()}

    def uniform(s):
        sess.render_fast(cam.raw, s, SEED, frame.data_ptr(), stream=st)
        return frame, {}

    def raw(s, tol):
        f, _, info = sess.render_fast_adaptive(cam.raw, s, SEED, tol)
        return f, info

    def denoised(s, tol):
        f, _, _, info = sess.render_fast_denoised(cam.raw, s, SEED, tol)
        return f, dict(info, guides_ms=sess.stats().main_kernel_ms)

    routes = {("uniform", s, 0.0): (lambda s=s: uniform(s)) for s in range(1, big + 1)}
    for s, tol in [(s, 0.0) for s in uniform_s] + [(big, t) for t in TOLS]:
        routes[("raw", s, tol)] = lambda s=s, tol=tol: raw(s, tol)
        routes[("denoised", s, tol)] = lambda s=s, tol=tol: denoised(s, tol)
    times, extra, err = {k: [] for k in routes}, {k: [] for k in routes}, {}
    for it in range(a.warmup + a.reps):
        for k, fn in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f, info = fn()
            torch.cuda.synchronize()
            if it >= a.warmup:
                times[k].append((time.perf_counter() - t0) * 1e3)
                extra[k].append(info)
            if k not in err:
                err[k] = error(f)
    med = {k: round(statistics.median(v), 3) for k, v in times.items()}
    spread = {k: [round(min(v), 3), round(max(v), 3)] for k, v in times.items()}
    base = {"width": w, "height": h, "ref_samples_sqrt": s_ref, "reps": a.reps, "warmup": a.warmup,
            "build_id": rtw.build_id()}
    lines, uni = [], {}
    for s in range(1, big + 1):
        k = ("uniform", s, 0.0)
        uni[s] = {"s": s, "ms": med[k], "min_max": spread[k], **err[k]}
        lines.append({"case": "uniform", **base, **uni[s]})
    for (kind, s, tol) in [k for k in routes if k[0] == "denoised"]:
        kd, kr = (kind, s, tol), ("raw", s, tol)
        line = {"case": "route", **base, "s": s, "tol": tol, "mean_spp": round(extra[kd][-1]["samples"] / (h * w), 2),
                "raw": {"ms": med[kr], "min_max": spread[kr], **err[kr]},
                "denoised": {"ms": med[kd], "min_max": spread[kd], **err[kd],
                             "guides_ms": round(statistics.median(x["guides_ms"] for x in extra[kd]), 4),
                             "filter_ms": round(statistics.median(x["denoise_ms"] for x in extra[kd]), 4)}}
        line["uniform_equal_time"] = min(uni.values(), key=lambda u: abs(u["ms"] - med[kd]))
        # the cheapest uniform frame that is at least as good as the denoised one (null: none up to s = big)
        good = [u for u in uni.values() if u["rmse8"] <= err[kd]["rmse8"]]
        line["uniform_equal_error"] = min(good, key=lambda u: u["ms"]) if good else None
        lines.append(line)

    # the filter alone, by level count, on the buffers of a 4-sample frame
    acc = torch.zeros((h, w, 3), dtype=torch.int64, device="cuda:0")
    mom = torch.zeros((h, w, 2), dtype=torch.int64, device="cuda:0")
    cnt = torch.zeros((h, w), dtype=torch.int32, device="cuda:0")
    gd = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
    sess.accumulate_fast_list(cam.raw, 2, SEED, acc.data_ptr(), mom.data_ptr(), cnt.data_ptr(), 4, stream=st)
    sess.guides_fast(cam.raw, gd.data_ptr(), stream=st)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    by_levels = {lv: [] for lv in range(9)}
    for it in range(a.warmup + a.reps):
        for lv in by_levels:
            ev[0].record()
            rtw.denoise_fast(acc.data_ptr(), cnt.data_ptr(), mom.data_ptr(), gd.data_ptr(), (h, w), levels=lv,
                             out_ptr=frame.data_ptr(), stream=st)
            ev[1].record()
            torch.cuda.synchronize()
            if it >= a.warmup:
                by_levels[lv].append(ev[0].elapsed_time(ev[1]))
    cum = [statistics.median(by_levels[lv]) for lv in by_levels]
    # a level reads 400 colour and 400 guide records per 256 pixels and writes one record per pixel
    level_bytes = h * w * (2 * 16 * 400 / 256 + 16)
    lines.append({"case": "levels", **base, "cumulative_ms": [round(x, 4) for x in cum],
                  "min_max": [[round(min(v), 4), round(max(v), 4)] for v in by_levels.values()],
                  "level_ms": [round(cum[i + 1] - cum[i], 4) for i in range(8)],
                  "level_gb_per_s": [round(level_bytes / max(cum[i + 1] - cum[i], 1e-6) / 1e6, 1) for i in range(8)]})
    for line in lines:
        print(json.dumps(line), flush=True)
    if not a.small:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            f.writelines(json.dumps(x) + "\n" for x in lines)


if __name__ == "__main__":
    main()
