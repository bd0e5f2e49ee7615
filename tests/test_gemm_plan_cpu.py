"""mit_gemm_plan -- the launch plan mit_gemm itself runs (csrc/gemm.hip plan_gemm) -- against decisions
recorded before the planner was unified: tests/golden/gemm_plan_cases.json, one named case per branch
(each return code, split-K and its refusals, each variant's override, the tiles hints, the LayerNorm fold /
row statistics forcing the 256 kernel, the activation-with-operand and generic-epilogue fallbacks, argmax).
No GPU: the planner makes no HIP call and never dereferences the (fake) pointers."""
import ctypes
import json
import os

import pytest

import native

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_plan_cases.json")) as f:
    CASES = json.load(f)["cases"]


@pytest.fixture(scope="module")
def lib():
    lib = native.load_library()
    yield lib
    assert lib.mit_gemm_set_variant(0) == 0


def test_fixture_covers_every_branch():
    assert len({c["name"] for c in CASES}) == len(CASES) >= 36
    assert {c["tile"] for c in CASES} == {0, 64, 65, 128, 256}
    assert {c["variant"] for c in CASES} == {0, 1, 2, 3, 4}
    assert any(c["ksplit"] > 1 for c in CASES) and {c["args"].get("tiles", 0) for c in CASES} == {0, 128, 256}


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_plan_matches_recorded_decision(lib, case):
    assert lib.mit_gemm_set_variant(case["variant"]) == 0
    g = native.GemmArgs(**case["args"])
    ks = ctypes.c_int(-1)
    tile = lib.mit_gemm_plan(ctypes.byref(g), ctypes.byref(ks))
    assert (tile, ks.value) == (case["tile"], case["ksplit"])
    assert lib.mit_gemm_plan(ctypes.byref(g), None) == case["tile"]  # ksplit is optional
