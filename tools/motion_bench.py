"""Cost of motion blur in fast mode, one process, routes alternated round by round:
  static   the final scene through the static kernels (rtw_session_render_fast)
  forced   the same scene through the moving kernels (RTW_FAST_MOVE=1 under RTW_AB=1): the
           variant itself, with no velocity read taken
  bouncing rtw_scene_bouncing through rtw_session_set_scene_moving: movers and swept bounds
Prints one JSON line per render and a summary line (medians, min..max) and appends them to
--out. Needs a GPU: python tools/motion_bench.py --rounds 7 --out profiles/motion/bench.jsonl
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import raytracing_in_a_weekend_rust_amd as rtw  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1200)
    ap.add_argument("--height", type=int, default=675)
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--samples-sqrt", type=int, default=23)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    seed = rtw.DEFAULT_SEED
    cam, sph, n, mt, nm = rtw.builtin_scene("complex", seed, a.height, a.width, a.depth)
    static = rtw.Session(0)
    static.set_scene(sph, n, mt, nm)
    bcam, bsph, bn, c1, bmt, bnm = rtw.bouncing_scene(seed, a.height, a.width, a.depth)
    bouncing = rtw.Session(0)
    bouncing.set_scene_moving(bsph, bn, c1, bmt, bnm)
    out = torch.empty((a.height, a.width, 3), dtype=torch.float32, device="cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    routes = {"static": (static, {}), "forced": (static, {"RTW_AB": "1", "RTW_FAST_MOVE": "1"}), "bouncing": (bouncing, {})}
    lines, ms = [], {r: [] for r in routes}
    frames = {}
    for rnd in range(-a.warmup, a.rounds):
        for name, (sess, env) in routes.items():
            os.environ.update(env)
            sess.render_fast(cam.raw, a.samples_sqrt, seed, out.data_ptr(), stream=st)
            s = sess.stats()  # waits for the render
            for k in env:
                del os.environ[k]
            frames.setdefault(name, out.clone())
            if rnd < 0:
                continue
            ms[name].append(s.main_kernel_ms)
            lines.append({"route": name, "round": rnd, "kernel_ms": s.main_kernel_ms, "segments": s.segments,
                          "node_visits": s.node_visits, "lds_bytes": s.lds_bytes, "accel": s.accel,
                          "width": a.width, "height": a.height, "depth": a.depth, "samples_sqrt": a.samples_sqrt,
                          "build": rtw.build_id()})
            print(json.dumps(lines[-1]), flush=True)
    med = {r: statistics.median(v) for r, v in ms.items()}
    summary = {"summary": True, "rounds": a.rounds, "build": rtw.build_id(),
               "forced_equals_static_bits": bool(torch.equal(frames["forced"], frames["static"])),
               **{f"{r}_ms_median": med[r] for r in ms}, **{f"{r}_ms_range": [min(v), max(v)] for r, v in ms.items()},
               "forced_over_static": med["forced"] / med["static"], "bouncing_over_static": med["bouncing"] / med["static"]}
    print(json.dumps(summary), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "a") as f:
            for line in lines + [summary]:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
