"""The bits of f32 fast mode against stored digests (tests/golden/fast_digests.json, made by
tests/golden/make_fast_digests.py, whose docstring lists the cases and says when and how to
regenerate). The other fast-mode tests compare the library's routes with each other; this one
notices a change that moves all of them alike. No skip on a toolchain mismatch: the stored
`hipcc` line is printed beside a failure."""
import json

import pytest

from tests.golden import make_fast_digests as fd

pytestmark = pytest.mark.gpu

with open(fd.PATH) as f:
    GOLDEN = json.load(f)


def flat(d, prefix=""):
    out = {}
    for k, v in d.items():
        out.update(flat(v, prefix + k + ".") if isinstance(v, dict) else {prefix + k: v})
    return out


@pytest.fixture(scope="module")
def computed():
    return flat(fd.digests())


def test_every_stored_case_is_computed(computed):
    assert GOLDEN["seed"] == fd.SEED and sorted(computed) == sorted(flat(GOLDEN["digests"]))


@pytest.mark.parametrize("case", sorted(flat(GOLDEN["digests"])))
def test_digest(computed, case):
    assert computed[case] == flat(GOLDEN["digests"])[case], "fixture made with %s for %s" % (GOLDEN["hipcc"], GOLDEN["ARCH"])


def test_scene_read_from_global_memory_gives_the_same_bits(monkeypatch, computed):
    monkeypatch.setenv("RTW_AB", "1")  # the knob is read only under RTW_AB (rtw_internal.h)
    monkeypatch.setenv("RTW_FAST_LDS", "0")
    glob = flat(fd.sampled())
    assert len(glob) == 6 + 3 + 2 * 2 * 3
    for case, digest in glob.items():
        assert digest == computed[case], case
        assert digest == flat(GOLDEN["digests"])[case], case
