"""CPU-only: every scratch-size function of the C ABI returns what the commit recorded in tests/golden/scratch_sizes.json
returned (the table was written from a build of THAT commit by tests/golden/capture_scratch_sizes.py), for the product
build and for the keybits14 build, valid and invalid sizes alike; and the Python size helpers are the library's."""
import json
import os
import sys

import pytest

from dfu3d_amd import _build, _lib, stages

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import capture_scratch_sizes as cap  # noqa: E402


@pytest.fixture(scope="module")
def tables():
    want = json.load(open(os.path.join(HERE, "golden", "scratch_sizes.json")))
    _lib.lib()                                           # builds the product library if it is stale
    got = cap.capture(_build.OUT, _build.build_variant("keybits14"), want["commit"])
    return want, got


def test_size_functions_return_what_the_recorded_commit_returned(tables):
    want, got = tables
    assert len(want["commit"]) == 40
    assert set(want) == set(got) and len(want) == 10
    n = 0
    for key in want:
        if key == "commit":
            continue
        assert len(want[key]) == len(got[key]) > 0, key
        for (args_w, res_w), (args_g, res_g) in zip(want[key], got[key]):
            assert args_w == list(args_g), key               # the same grid, in the same order
            assert res_w == res_g, (key, args_w)
            n += 1
    assert n > 1500


def test_grid_holds_the_cases_that_matter(tables):
    want, _ = tables
    bp = {tuple(a): r for a, r in want["backproject_scratch_words/product"]}
    bp14 = {tuple(a): r for a, r in want["backproject_scratch_words/keybits14"]}
    bench = (96, 900, 1600, 1 << 18, 100, cap.BENCH_E)
    assert bp[bench][0] == 0 and bp[bench][1] == 2 * 96 * 900 * 1600 and bp14[bench][2] > bp[bench][2]   # queue_cap differs
    assert bp[(1, 180, 320, 1 << 17, 100, cap.BENCH_E)][0] == 0 and bp[(3, 225, 400, 1 << 16, 1, 65)][0] == 0
    assert bp[(0, 900, 1600, 1 << 18, 100, cap.BENCH_E)][0] == -1
    ws = {tuple(a): r for a, r in want["workspace_bytes[stage -1..12]"]}
    for dense in (0, 1):
        for stat in (0, 1):
            assert (96, 900, 1600, 8, 34720, 1 << 18, 6144, 100, 96 << 17, cap.BENCH_E, dense, stat) in ws
            assert (12, 180, 320, 5, 4096, 1 << 17, 6144, 100, 513, cap.BENCH_E, dense, stat) in ws
    assert {a[0] for a, _ in want["rf_shadow_bytes"]} >= {1, 511, 512, 513, 96 << 17, 0, -1}


@pytest.mark.parametrize("P", [p for p in cap.POOLS if p > 0])
def test_python_size_helpers_are_the_librarys(P):
    L = _lib.lib()
    assert stages.shadow_floats(P) * 4 == L.dfu3d_rf_shadow_bytes(P)
    assert stages.rf_queue_ints(P) == L.dfu3d_rf_queue_ints(P)


def test_python_does_not_retype_the_header_macros():
    text = open(os.path.join(os.path.dirname(HERE), "dfu3d_amd", "stages.py")).read()
    assert "9699456" not in text
    with pytest.raises(_lib.Dfu3dError):
        stages.shadow_floats(0)
    with pytest.raises(_lib.Dfu3dError):
        stages.rf_queue_ints(-1)
