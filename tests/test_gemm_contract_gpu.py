"""mit_gemm / mit_gemm_grouped on guarded, strided operands (tests/gemm_contract.py): every kernel family behind
plan_gemm (f32, register-streaming, 128 with and without split-K, 256 and its five epilogue stages, the
one-wave-per-SIMD 256, the argmax epilogue) and the grouped launch, each with every leading dimension padded
and different, on the vector and on the scalar epilogue path. One launch per case: the plan of the captured
args is the case's, the result matches the float64 reference of the header's formula, nothing outside an
output's window is written (head guard, pad columns of live rows, tail guard) and no input is written at all.
Inputs are NaN outside their windows. Every call is a valid call.

Bounds: gemm_contract's docstring. Each figure is printed before it is asserted (pytest -s / -rA shows them).
Measured worst case per family on an MI355X, as a fraction of max|ref| (bound):
  f32 kernel          C 2.0e-7, rowsum 9.5e-8 (1e-5)
  register-streaming  bf16 out 3.6e-3 (1e-2), f32 out 1.1e-7 (1e-5)
  128                 bf16 out 3.4e-3 (1e-2), f32 out 6.4e-8 (1e-5), GELU f32 out 1.4e-7 (2e-5)
  128 split-K         bf16 out 3.7e-3 (1e-2), f32 out 2.0e-7, rowsum 3.4e-8 (1e-3)
  256                 bf16 out 3.3e-3 (1e-2), f32 out 1.1e-7 (1e-5), GELU f32 out 1.1e-7 (2e-5), statistics 9.9e-8 (1e-4)
  256w                bf16 out 2.4e-3 (1e-2), statistics 1.0e-7 (1e-4); bitwise equal to the 256 kernel
  grouped             C 3.5e-7, rowsum 4.4e-8 (1e-3)"""
import ctypes

import pytest
import torch

import gemm_contract as gc
import native as N

pytestmark = pytest.mark.gpu


class _Probe:
    def __init__(self):
        self.args = []

    def before(self, *a):
        pass

    def after(self, g):
        self.args.append(g)


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    N.load_library()
    try:
        yield
    finally:
        N.set_gemm_probe(None)
        N.gemm_set_variant(0)
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:  # a GPU fault poisons the process: launch nothing more on it
        pytest.exit(f"GPU error after a GEMM contract case, run ended: {e}", returncode=3)


def _mask(n, p, seed, site):
    out = torch.empty(n, device="cuda")
    N.dropout_mask(n, p, seed, site, out)
    return out


def _launch(case, t, variant, ws):
    """one mit_gemm launch of the case under `variant`; returns the plan of the args it was called with"""
    probe = _Probe()
    N.set_gemm_probe(probe)
    N.gemm_set_variant(variant)
    args, kw = gc.gemm_kwargs(case, t)
    N.gemm(*args, workspace=ws, **kw)
    torch.cuda.synchronize()
    assert len(probe.args) == 1
    return N.gemm_plan(probe.args[0])


@pytest.mark.parametrize("case", gc.CASES, ids=[c.id for c in gc.CASES])
def test_gemm_contract(case):
    t = gc.make_tensors(case, "cuda", _mask)
    if case.ln:  # the statistics of the strided A rows, as the encoder's layer 0 makes them
        N.row_stats64(t["A"].view, t["ln_stats"].view, rows=case.M, cols=case.K, ldx=case.lda)
    ws = N.gemm_workspace(case.M, case.N, case.K, "cuda") if case.workspace else None
    gc.snapshot(t)
    ref = gc.reference(case, t)
    assert _launch(case, t, case.variant, ws) == case.plan
    gc.check(case, t, ref)
    if case.family == "256w":  # bitwise equal to the 256 kernel (variant 0) on the same strided buffers
        t0 = dict(t, C=t["C"].twin())
        if case.stats:
            t0["stats_out"] = t["stats_out"].twin()
        assert _launch(case, t0, 0, ws) == (256, 1)
        gc.check(case, t0, ref)
        assert torch.equal(t["C"].whole.view(torch.int16), t0["C"].whole.view(torch.int16))
        if case.stats:
            assert torch.equal(t["stats_out"].whole.view(torch.int32), t0["stats_out"].whole.view(torch.int32))


@pytest.mark.parametrize("kind", ["plain", "acc"])
def test_gemm_grouped_contract(kind):
    """mit_gemm_grouped on strided operands and outputs, three problems in one launch (the first split in two):
    alpha and accumulate honoured (native._dw_args fixes them at 1 / 0, so the args are built here)."""
    cases = gc.GROUPED[kind]
    ts = [gc.make_tensors(c, "cuda") for c in cases]
    arr = (N.GemmArgs * len(cases))()
    for i, (c, t) in enumerate(zip(cases, ts)):
        arr[i] = N.GemmArgs(N.BF16, c.al, c.bl, c.M, c.N, c.K, N.ptr(t["A"].view), c.lda, N.ptr(t["B"].view), c.ldb,
                            N.ptr(t["C"].view), c.ldc, c.alpha, None, N.ACT_NONE, None, 0, None, 0, 1.0, 0.0, None, 0, 1,
                            1 if c.accumulate else 0, N.ptr(t["rowsum"].view), None, 0)
    lib = N.lib()
    wsb = lib.mit_gemm_grouped_ws_bytes(arr, len(cases))
    assert wsb > 4096  # a split-K slab: the reduce launch runs too
    ws = torch.empty(wsb // 4 + 64, device="cuda")
    refs = []
    for c, t in zip(cases, ts):
        gc.snapshot(t)
        refs.append(gc.reference(c, t))
    rc = lib.mit_gemm_grouped(arr, len(cases), None, 0, N.ptr(ws), wsb, N.stream_ptr())
    assert rc == 0, lib.mit_last_error()
    torch.cuda.synchronize()
    for c, t, ref in zip(cases, ts, refs):
        gc.check(c, t, ref)
