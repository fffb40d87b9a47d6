"""Times progressive fast mode (rtw_session_accumulate_fast + rtw_resolve_fast) against the
one-shot rtw_session_render_fast on the final scene (complex, 1200x675, depth 50), in one
process on one GPU, the routes alternating; medians of --reps timed calls after --warmup.
A timed call is host wall time from the enqueue to the end of a stream synchronise; the
accumulate routes include zeroing the sums and the resolve. Cases:
  spread    render_fast against itself (what a ratio of 1 looks like here)
  low       s = 1, 2, 3: the whole lattice in one accumulate + resolve against render_fast
  high      s = 23: one pass of 529 samples per pixel against render_fast
  passes    s = 23 in 16, 64 and 529 strided passes, each followed by a resolve with both
            outputs, against render_fast; the median pass of the 529 is the preview's frame time
Before a route is timed its final frame must be array_equal to the one-shot frame.
One JSON line per case, printed and written to --out.

    python tools/progressive_bench.py [--reps 9] [--warmup 2] [--small] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--small", action="store_true", help="a tiny image (a rehearsal of the script; nothing is written)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "progressive", "bench.jsonl"))
    a = ap.parse_args()
    h, w, big = (27, 48, 5) if a.small else (675, 1200, 23)
    cam, sph, n, mt, nm = rtw.builtin_scene("complex", SEED, h, w, 50)
    sess = rtw.Session(0)
    sess.set_scene(sph, n, mt, nm)
    st = torch.cuda.current_stream().cuda_stream
    want = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
    got = torch.zeros_like(want)
    acc = torch.zeros((h, w, 3), dtype=torch.int64, device="cuda:0")
    pre = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0")
    pass_ms = []

    def one_shot(s, out=got):
        sess.render_fast(cam.raw, s, SEED, out.data_ptr(), stream=st)
        return sess.stats()

    def progressive(s, passes):
        acc.zero_()
        done, n_off, last = 0, max(1, s * s), None
        for p in range(passes):
            sess.accumulate_fast(cam.raw, s, SEED, acc.data_ptr(), p, passes, stream=st)
            done += (n_off - p + passes - 1) // passes
            if passes > 1:  # a viewer's pass: wait for it, then both outputs
                last = sess.stats()
                pass_ms.append(last.kernel_ms)
            rtw.resolve_fast(acc.data_ptr(), (h, w), done, got.data_ptr(), pre.data_ptr() if passes > 1 else 0, 0, st)
        return last or sess.stats()

    def case(name, s, routes, reps):
        one_shot(s, want)
        stats = {}
        for k, fn in routes.items():  # a route that renders another frame records no time
            got.zero_()
            stats[k] = fn()
            torch.cuda.synchronize()
            assert torch.equal(got, want) and want.any(), "%s/%s: not the one-shot frame" % (name, k)
        times = {k: [] for k in routes}
        for it in range(a.warmup + reps):
            for k, fn in routes.items():
                pass_ms.clear()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if it >= a.warmup:
                    times[k].append((time.perf_counter() - t0) * 1e3)
        samples = h * w * max(1, s * s)
        line = {"case": name, "width": w, "height": h, "samples_sqrt": s, "reps": reps, "warmup": a.warmup,
                "build_id": rtw.build_id()}
        for k, v in times.items():
            med = statistics.median(v)
            line[k] = {"ms": round(med, 4), "min": round(min(v), 4), "max": round(max(v), 4),
                       "msamples_per_s": round(samples / med / 1e3, 1)}
        for k in ("one_shot", "accumulate"):  # per launch: the last pass of a progressive route
            if k in stats:
                line[k]["wave_iterations_per_sample"] = round(stats[k].wave_iterations / stats[k].samples, 4)
        base = line["one_shot"]["ms"]
        line["over_one_shot"] = {k: round(line[k]["ms"] / base, 4) for k in routes if k != "one_shot"}
        print(json.dumps(line), flush=True)
        return line

    lines = [case("spread_s%d" % s, s, {"one_shot": lambda: one_shot(s), "one_shot_again": lambda: one_shot(s)}, a.reps)
             for s in (2, big)]
    for s in (1, 2, 3):
        lines.append(case("low_s%d" % s, s, {"one_shot": lambda: one_shot(s), "accumulate": lambda: progressive(s, 1)},
                          a.reps))
    lines.append(case("high_s%d" % big, big,
                      {"one_shot": lambda: one_shot(big), "accumulate": lambda: progressive(big, 1)}, a.reps))
    for passes in (16, 64, big * big):
        line = case("passes_%d" % passes, big, {"one_shot": lambda: one_shot(big),
                                                "passes": lambda: progressive(big, passes)}, max(3, a.reps // 3))
        line["pass_kernel_ms_median"] = round(statistics.median(pass_ms), 4)  # of the last timed run
        print(json.dumps({"case": line["case"], "pass_kernel_ms_median": line["pass_kernel_ms_median"]}), flush=True)
        lines.append(line)
    sess.close()
    if not a.small:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.writelines(json.dumps(x) + "\n" for x in lines)


if __name__ == "__main__":
    main()
