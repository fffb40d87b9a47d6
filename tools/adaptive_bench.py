"""Times adaptive fast mode (rtw_session_render_fast_adaptive) against the uniform
rtw_session_render_fast on the final scene (complex, 1200x675, depth 50, s = 23), in one
process on one GPU, and measures both against a converged reference frame: a fast-mode render
at s = 64 (4096 samples per pixel) with another seed. A timed call is host wall time from the
enqueue to the end of a stream synchronise; every route runs once per repetition, the routes
alternating; medians of --reps after --warmup. The error is taken on 8-bit values,
round(255 sqrt(clamp(x, 0, 1))): RMSE and the 99th percentile of |delta| over all channels.
Lines written (one JSON object each, printed and collected in --out):
  uniform   render_fast at s = 3..23: time, samples, error
  adaptive  one per tolerance: time, rounds, samples, kernel and select time, error, and the
            uniform frames of about equal samples and of about equal time beside it
  tol0      the tolerance-0 route (every pixel to N, the one-shot frame) over render_fast
  round     a full-list m = 16 round over accumulate_fast with k_count = 16 (kernel times)

    python tools/adaptive_bench.py [--reps 7] [--warmup 2] [--small] [--out FILE]
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
TOLS = (0.2, 0.1, 0.05, 0.03, 0.02, 0.01)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--small", action="store_true", help="a tiny image (a rehearsal of the script; nothing is written)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive", "bench.jsonl"))
    a = ap.parse_args()
    h, w, big, s_ref = (27, 48, 5, 9) if a.small else (675, 1200, 23, 64)
    n_big = big * big
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
        return frame, {"samples": h * w * s * s}

    def adaptive(tol):
        f, counts, info = sess.render_fast_adaptive(cam.raw, big, SEED, tol)
        return f, info

    acc = torch.zeros((h, w, 3), dtype=torch.int64, device="cuda:0")
    mom = torch.zeros((h, w, 2), dtype=torch.int64, device="cuda:0")
    cnt = torch.zeros((h, w), dtype=torch.int32, device="cuda:0")

    def round_list():
        acc.zero_(), mom.zero_(), cnt.zero_()
        sess.accumulate_fast_list(cam.raw, big, SEED, acc.data_ptr(), mom.data_ptr(), cnt.data_ptr(), 16, stream=st)
        return None, {"kernel_ms": sess.stats().main_kernel_ms}

    def round_uniform():
        acc.zero_()
        sess.accumulate_fast(cam.raw, big, SEED, acc.data_ptr(), 0, 1, 16, stream=st)
        return None, {"kernel_ms": sess.stats().main_kernel_ms}

    routes = {("uniform", s): (lambda s=s: uniform(s)) for s in range(3, big + 1)}
    routes.update({("adaptive", t): (lambda t=t: adaptive(t)) for t in TOLS + (0.0,)})
    routes[("round", "list")] = round_list
    routes[("round", "uniform")] = round_uniform
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
            if f is not None and k not in err:
                err[k] = error(f)
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: [round(min(v), 3), round(max(v), 3)] for k, v in times.items()}
    base = {"width": w, "height": h, "samples_sqrt": big, "ref_samples_sqrt": s_ref, "reps": a.reps, "warmup": a.warmup,
            "build_id": rtw.build_id()}
    lines = []
    uni = {}
    for s in range(3, big + 1):
        k = ("uniform", s)
        uni[s] = {"s": s, "ms": round(med[k], 3), "min_max": spread[k], "samples": h * w * s * s, **err[k]}
        lines.append({"case": "uniform", **base, **uni[s]})
    for t in TOLS:
        k = ("adaptive", t)
        info = extra[k][-1]
        line = {"case": "adaptive", **base, "tol": t, "ms": round(med[k], 3), "min_max": spread[k],
                "rounds": info["rounds"], "samples": info["samples"], "mean_spp": round(info["samples"] / (h * w), 2),
                "pixels_full": info["pixels_full"],
                "kernel_ms": round(statistics.median(x["kernel_ms"] for x in extra[k]), 3),
                "select_ms": round(statistics.median(x["select_ms"] for x in extra[k]), 3),
                "select_ms_per_round": round(statistics.median(x["select_ms"] / x["selects"] for x in extra[k]), 4),
                **err[k]}
        line["uniform_equal_samples"] = min(uni.values(), key=lambda u: abs(u["samples"] - line["samples"]))
        line["uniform_equal_time"] = min(uni.values(), key=lambda u: abs(u["ms"] - line["ms"]))
        lines.append(line)
    k0, kb = ("adaptive", 0.0), ("uniform", big)
    assert extra[k0][-1]["samples"] == h * w * n_big
    lines.append({"case": "tol0", **base, "ms": round(med[k0], 3), "render_fast_ms": round(med[kb], 3),
                  "over_render_fast": round(med[k0] / med[kb], 4), "rounds": extra[k0][-1]["rounds"],
                  "kernel_ms": round(statistics.median(x["kernel_ms"] for x in extra[k0]), 3),
                  "select_ms": round(statistics.median(x["select_ms"] for x in extra[k0]), 3)})
    kl, ku = (statistics.median(x["kernel_ms"] for x in extra[("round", r)]) for r in ("list", "uniform"))
    lines.append({"case": "round", **base, "m": 16, "list_kernel_ms": round(kl, 4), "accumulate_kernel_ms": round(ku, 4),
                  "over_accumulate": round(kl / ku, 4), "list_wall_ms": round(med[("round", "list")], 3),
                  "accumulate_wall_ms": round(med[("round", "uniform")], 3)})
    for line in lines:
        print(json.dumps(line), flush=True)
    if not a.small:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.writelines(json.dumps(x) + "\n" for x in lines)


if __name__ == "__main__":
    main()
