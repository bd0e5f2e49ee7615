"""The GEMM memory-contract harness (tests/gemm_contract.py) without a GPU:
  * every case of the table plans onto the kernel family it names (mit_gemm_plan on placeholder addresses of the
    case's alignment), so a dispatch change cannot silently move a case onto another kernel;
  * the harness catches a subtly wrong kernel: fake_gemm, a torch GEMM on the same guarded strided buffers,
    passes the case's check as it is and fails it with each injected fault (a store into a pad column, past row
    M or into the head guard, K rounded up on read, residual / aux / dropout index formed with the wrong
    leading dimension, row sums of the wrong operand, accumulate ignored);
  * mit_gemm rejects a residual / aux whose leading dimension is below N (validation precedes any launch; no
    call here reaches one)."""
import ctypes

import pytest
import torch

import gemm_contract as gc
import native

ALL = gc.CASES + gc.GROUPED["plain"] + gc.GROUPED["acc"]
MIT_ERR_INVALID = 1


@pytest.fixture(scope="module")
def lib():
    lib = native.load_library()
    yield lib
    assert lib.mit_gemm_set_variant(0) == 0


def test_table_covers_the_families_and_paths():
    fam = {c.family for c in gc.CASES}
    assert fam == {"f32", "rs", "128", "splitk", "256", "256w", "argmax"}
    assert {c.plan for c in gc.CASES} == {(64, 1), (65, 1), (128, 1), (128, 2), (256, 1)}
    for c in ALL:  # every leading dimension is padded, and the epilogue operands' differ from ldc and each other
        ea, eb = (c.K if c.al == 0 else c.M), (c.K if c.bl == 0 else c.N)
        assert c.lda > ea and c.ldb > eb and c.ldc > c.N and c.lda - ea != c.ldb - eb, c.id
        if c.residual and not c.res_is_c:
            assert c.ldr > c.N and c.ldr != c.ldc, c.id
        if c.aux:
            assert c.ld_aux > c.N and c.ld_aux not in (c.ldc, c.ldr), c.id
    # the bf16 kernels' scalar epilogue: N % 8, ldc % 8 and a C off its 16-byte alignment, per family that has one
    ways = {"rs": {"N", "ldc", "C"}, "128": {"N", "ldc"}, "256": {"N", "C"}}
    for f, want in ways.items():
        bf = [c for c in gc.CASES if c.family == f]
        got = {w for c in bf for w, off in (("N", c.N % 8), ("ldc", c.N % 8 == 0 and c.ldc % 8), ("C", c.mis_c)) if off}
        assert got == want and any(c.N % 8 == 0 and c.ldc % 8 == 0 and not c.mis_c for c in bf), f
    assert {(c.al, c.bl) for c in gc.CASES if c.family == "f32"} == {(0, 0), (0, 1), (1, 0), (1, 1)}


@pytest.mark.parametrize("case", gc.CASES, ids=[c.id for c in gc.CASES])
def test_case_plans_onto_its_family(lib, case):
    assert lib.mit_gemm_set_variant(case.variant) == 0
    g = gc.placeholder_args(case, native)
    ks = ctypes.c_int(-1)
    tile = lib.mit_gemm_plan(ctypes.byref(g), ctypes.byref(ks))
    assert (tile, ks.value) == case.plan
    if case.family == "256w":  # its variant-0 twin runs the 256 kernel as well
        assert lib.mit_gemm_set_variant(0) == 0
        assert lib.mit_gemm_plan(ctypes.byref(g), ctypes.byref(ks)) == 256 and ks.value == 1


def test_grouped_launch_splits_its_first_problem_only(lib):
    """mit_gemm_grouped_ws_bytes = the header + one slab: of (136, 72, 1032), split in two; K = 264 / 520 do not split."""
    for cases in gc.GROUPED.values():
        arr = (native.GemmArgs * len(cases))(*[gc.placeholder_args(c, native) for c in cases])
        slab = (4 * 2 * 136 * 72 + 4 * 2 * 136 + 255) // 256 * 256
        assert lib.mit_gemm_grouped_ws_bytes(arr, len(cases)) == 4096 + slab


def test_strided_layout():
    for dtype, esz in ((torch.bfloat16, 2), (torch.float32, 4)):
        for mis in (0, 1, 3):
            whole, view = gc.strided(5, 7, 11, dtype, gc.SENTINEL, mis)
            assert whole.numel() == 64 + mis + 5 * 11 + 64 and view.shape == (5, 7) and view.stride() == (11, 1)
            assert (view.data_ptr() - mis * esz) % 16 == 0 and (whole == gc.SENTINEL).all()
            assert view.data_ptr() - whole.data_ptr() == (64 + mis) * esz
    whole, view = gc.strided(3, 4, 6, torch.float32, gc.NAN)
    assert torch.isnan(whole).all()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_untouched_sees_every_region(dtype):
    whole, view = gc.strided(4, 5, 9, dtype, gc.NAN)  # NaN fill: compared as bits
    spec = (64, 4, 5, 9)
    before = whole.clone()
    view.fill_(1.0)
    gc.untouched(whole, spec, before)  # the window may change
    for idx in (0, 63, 64 + 5, 64 + 8, 64 + 3 * 9 + 5, 64 + 4 * 9, whole.numel() - 1):
        w = whole.clone()
        w[idx] = 2.0
        with pytest.raises(AssertionError):
            gc.untouched(w, spec, before)


_refs = {}


def _run(case, fault):
    torch.manual_seed(0)
    t = gc.make_tensors(case)
    gc.snapshot(t)
    if case.id not in _refs:  # one float64 reference per case, shared by its faults
        _refs[case.id] = gc.reference(case, t)
    gc.fake_gemm(case, t, fault)
    gc.check(case, t, _refs[case.id])


@pytest.mark.parametrize("case", [c for c in ALL if not c.argmax], ids=lambda c: c.id)
def test_faultless_fake_gemm_passes(case):
    _run(case, None)


_FAULT_CASES = [(f, c) for f in gc.FAULTS for c in ALL if gc.fault_applies(c, f)]


def test_every_fault_has_cases_in_every_family_that_can_show_it():
    for f in gc.FAULTS:
        assert any(ff == f for ff, _ in _FAULT_CASES), f
    fams = lambda f: {c.family for ff, c in _FAULT_CASES if ff == f}
    assert fams("pad_column") == fams("past_row_m") == fams("head_guard") == {c.family for c in ALL} - {"argmax"}
    assert fams("res_ldc") >= {"f32", "rs", "128", "256"} and fams("aux_ldr") >= {"f32", "rs", "128", "256"}
    assert fams("drop_ldc") >= {"f32", "rs", "128"} and fams("rowsum_b") >= {"f32", "splitk", "grouped"}
    assert fams("no_accumulate") >= {"f32", "rs", "128", "splitk", "grouped"}


@pytest.mark.parametrize("fault,case", _FAULT_CASES, ids=[f"{f}-{c.id}" for f, c in _FAULT_CASES])
def test_injected_fault_is_caught(fault, case):
    with pytest.raises(AssertionError):
        _run(case, fault)


def _reject_args(**kw):
    # small valid f32 NT problem on placeholder addresses; every call below is rejected before any launch
    g = native.GemmArgs(native.F32, 0, 0, 8, 8, 8, 0x10000, 8, 0x20000, 8, 0x30000, 8, 1.0)
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def _err(lib):
    return (lib.mit_last_error() or b"").decode()


def test_gemm_rejects_short_residual_and_aux_leading_dimensions(lib):
    # (each call also accumulates into a non-f32 output, which a later check rejects: should the check under test
    # be missing, the call still launches nothing and fails here on the message)
    late = dict(accumulate=1, out_f32=0)
    g = _reject_args(residual=0x40000, ldr=7, **late)
    assert lib.mit_gemm(ctypes.byref(g), None) == MIT_ERR_INVALID and "ldr too small" in _err(lib)
    g = _reject_args(residual=0x40000, ldr=0, **late)  # a zero-initialised struct with only `residual` set
    assert lib.mit_gemm(ctypes.byref(g), None) == MIT_ERR_INVALID and "ldr too small" in _err(lib)
    g = _reject_args(aux=0x40000, ld_aux=7, **late)
    assert lib.mit_gemm(ctypes.byref(g), None) == MIT_ERR_INVALID and "ld_aux too small" in _err(lib)
    # absent operands: their leading dimensions are not looked at. The call gets past them to the next check
    # in line (accumulate into a non-f32 output), which names itself.
    g = _reject_args(dtype=native.BF16, ldr=0, ld_aux=0, accumulate=1, out_f32=0)
    assert lib.mit_gemm(ctypes.byref(g), None) == MIT_ERR_INVALID
    assert "accumulate" in _err(lib) and "too small" not in _err(lib)
    # present and long enough: likewise
    g = _reject_args(dtype=native.BF16, residual=0x40000, ldr=8, aux=0x50000, ld_aux=8, accumulate=1, out_f32=0)
    assert lib.mit_gemm(ctypes.byref(g), None) == MIT_ERR_INVALID
    assert "accumulate" in _err(lib) and "too small" not in _err(lib)
