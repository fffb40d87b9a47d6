"""Records how f32 fast mode agrees with oracle/fast_model.py, sample by sample, for every
case of tests/fast_cases.py: one JSON line per case (the figures tests/test_gpu_fast_samples.py
asserts on) to profiles/fast_model/agreement.jsonl, or to the path given. Needs a gfx950
GPU and the built library.

    python tools/fast_model_agreement.py [out.jsonl]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import fast_cases as fc  # noqa: E402


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "fast_model", "agreement.jsonl")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        for name in fc.CASES:
            c = fc.case(name)
            gpu, segments, accel = fc.gpu_samples(c)
            a = fc.agreement(c, gpu, segments)
            a.update(accel=accel, T=fc.T, eps=fc.EPS)
            f.write(json.dumps(a) + "\n")
            f.flush()
            print(json.dumps(a), flush=True)


if __name__ == "__main__":
    main()
