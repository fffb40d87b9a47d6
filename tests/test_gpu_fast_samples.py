"""f32 fast mode sample by sample against oracle/fast_model.py, an f64 model that draws the
same random numbers. accumulate_fast(k, 1, 1) into zero sums returns each
sample's colour exactly, so the kernel's per-sample path (rtw_fast_dev.h) is compared with
a plain reference of the same operation, not with itself and not statistically. Only
samples whose path sits on a decision boundary may differ; tests/fast_cases.py holds the
rule that names them from the model alone, the caps and the cases. The figures of each case
are printed before they are asserted (tools/fast_model_agreement.py records them)."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import fast_cases as fc
from tests.fast_cases import T

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def run(name):
    c = fc.case(name)
    gpu, segments, accel = fc.gpu_samples(c)
    a = fc.agreement(c, gpu, segments)
    a["accel"] = accel
    print(a)
    return c, gpu, a


@pytest.mark.parametrize("name", list(fc.CASES))
def test_stable_samples_agree(name):
    """Conditions 2 and 3: at most 1% of the stable samples further than T from the model,
    and no systematic offset hiding under T."""
    c, _, a = run(name)
    assert a["stable"] >= (1. - fc.UNSTABLE_CAP) * a["samples"]
    assert a["stable_disagreeing"] <= fc.DISAGREE_CAP * a["stable"], a
    assert max(abs(v) for v in a["stable_mean_signed"]) <= T / 8, a


@pytest.mark.parametrize("name", list(fc.CASES))
def test_common_random_numbers_bias(name):
    """Condition 4: over all samples, unstable ones included, the same random numbers on both
    sides; a sample beyond T moves the sum by at most 1 (colours are <= 1 here)."""
    c, gpu, a = run(name)
    assert max(max(v) for v in gpu.values()) <= 1. and max(max(v[0]) for v in c.samples.values()) <= 1.
    bound = T / 8 + 4. * math.sqrt(a["D"]) / a["samples"]
    assert max(abs(v) for v in a["all_mean_signed"]) <= bound, (a, bound)


@pytest.mark.parametrize("name", list(fc.CASES))
def test_segment_count(name):
    """Condition 5: the launches' segments against the model's; equal when no sample differs."""
    c, _, a = run(name)
    assert abs(a["segments_gpu"] - a["segments_model"]) <= c.depth * a["D"], a
    if name in fc.DEPTH1:
        assert a["segments_gpu"] == a["samples"]


def test_routes_taken():
    """The final scene walks the BVH; the scan scene is left without nodes."""
    assert run("final_12x20_s2_d50")[2]["accel"] == 2
    assert run("ring_final_8x12_s4_d50")[2]["accel"] == 2
    assert run("scan_12x20_s2_d50")[2]["accel"] == 0


def test_one_shot_frame_is_the_mean_of_the_model():
    """render_fast (16 samples a pixel: the ring kernel) against the model's per-pixel mean:
    every pixel whose samples are all stable within T, and condition 4 over the frame."""
    c, _, a = run("ring_final_8x12_s4_d50")
    sess, cam = fc.gpu_session(c)
    out = torch.zeros((c.h, c.w, 3), dtype=torch.float32, device="cuda:0")
    sess.render_fast(cam, c.s, c.seed, out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    assert sess.stats().segments == a["segments_gpu"]
    frame = out.cpu().numpy().astype(np.float64)
    want = np.zeros_like(frame)
    all_stable = np.ones((c.h, c.w), dtype=bool)
    for (x, y, k), (rgb, _) in c.samples.items():
        want[y, x] += rgb
        all_stable[y, x] &= (x, y, k) in c.stable
    want /= c.n_off
    diff = frame - want
    worst = np.abs(diff).max(axis=2)
    print("pixels all stable: %d of %d, their worst difference %.3g, frame mean signed %s"
          % (all_stable.sum(), all_stable.size, worst[all_stable].max(), diff.reshape(-1, 3).mean(axis=0)))
    assert all_stable.any()
    assert worst[all_stable].max() <= T
    bound = T / 8 + 4. * math.sqrt(a["D"]) / a["samples"]
    assert np.abs(diff.reshape(-1, 3).mean(axis=0)).max() <= bound
