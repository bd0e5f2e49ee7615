"""csrc/norm.hip's entry points on guarded, strided operands (tests/ln_contract.py): every kernel family and NV
instance behind mit_layernorm_fwd / mit_layernorm_bwd (pair, wide, vec4, scalar; both dtypes; both sides of the
512 / 520, 1024 / 1032 and 2048 limits; each alignment rule alone), row counts around the forward's 4-row, the
pair kernel's 8-row and the backward's 8-row blocks, r with and without dropout, an ignored r_drop_p, z / mean /
rstd NULL, eps 1e-5 and 1e-12, dr NULL / with dropout, dx aliasing dy, the deferred parameter reduction;
mit_layernorm_param_grads alone through its unrolled loop and tail; mit_layernorm_fwd_x32 (both NV, y bf16 / f32,
z none / separate / x itself); mit_residual_out past its grid cap; mit_row_stats64 with one and two passes.
Two launches per entry point and case: mit_layernorm_plan of the launched arguments is the case's, the results are
within the bounds of ln_contract's docstring of the float64 reference, the exact properties hold (a constant row's
y is beta, dr is dx or 0, deferred = fused parameter gradients, exact z / y of the f32-stream kernels), nothing
outside an output's window is written, no input is written, and the second launch is bitwise equal to the first.
Inputs are NaN outside their windows. Every call is a valid call.

Each figure is printed before it is asserted (pytest -s / -rA shows them). Measured worst on an MI355X, in
ln_contract's units (bound); bf16 outputs: the part past 2^-8 |ref|:
  y f32 0.83, bf16 0.31 (27.7); z f32 0.88, bf16 0.20 (3.54); mean 0.52 (15.5); rstd 0.92 (39.5)
  dx f32 1.00, dr f32 1.22, both bf16 0.03 (6.96); dgamma 1.54 (7.11); dbeta 1.25 (4.69)
  mit_layernorm_param_grads alone 1.58 (9.55); mit_layernorm_fwd_x32 y f32 0.77, bf16 0.05 (27.7)
  mit_row_stats64 mean 0 (1), M2 0.21 (5.25)
The bounds come from sequential float32 summation; the kernels sum over a 64-lane tree and sit near one unit."""
import pytest
import torch

import ln_contract as lc
import native as N

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    N.load_library()
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:  # a GPU fault poisons the process: launch nothing more on it
        pytest.exit(f"GPU error after a LayerNorm contract case, run ended: {e}", returncode=3)


def _mask(n, p, seed, site):
    out = torch.empty(n, device="cuda")
    N.dropout_mask(n, p, seed, site, out)
    return out


class NativeOps:
    """libmit_hip.so on the case's buffers; every method ends synchronised (the harness reads the buffers next)"""

    def fwd(self, c, t, drop_p=None):
        ldx, ldr, ldy = c.lds
        N.layernorm_fwd(t.v("x"), t.row("gamma"), t.row("beta"), c.eps, t.v("y"), r=t.v("r"),
                        drop_p=c.drop_p if drop_p is None else drop_p, seed=t.seed, site=c.site, z=t.v("z"),
                        mean=t.row("mean"), rstd=t.row("rstd"), rows=c.rows, cols=c.cols, ldx=ldx, ldr=ldr, ldy=ldy)
        torch.cuda.synchronize()

    def bwd(self, c, t, deferred=False):
        dx = t.v("dy") if c.alias_dx else t.v("dx")
        assert t.v("bz").shape == (c.rows, c.cols) and t.v("bz").stride(0) == c.cols  # native.layernorm_bwd reads them
        N.layernorm_bwd(t.v("dy"), t.v("bz"), t.row("bmean"), t.row("brstd"), t.row("gamma"), dx,
                        None if deferred else t.row("dgamma"), None if deferred else t.row("dbeta"), t.row("ws"),
                        dr=t.v("dr"), drop_p=c.bwd_drop_p, seed=t.seed, site=c.site)
        torch.cuda.synchronize()

    def pgrad(self, c, t):
        N.layernorm_param_grads(c.rows, c.cols, t.row("ws"), t.row("dgamma"), t.row("dbeta"))
        torch.cuda.synchronize()

    def x32(self, c, t):
        ldx, ldr, ldy = c.lds
        z = t.v("x") if c.z == "alias" else t.v("z")
        N.layernorm_fwd_x32(t.v("x"), t.row("gamma"), t.row("beta"), c.eps, t.v("y"), r=t.v("r"), z=z, rows=c.rows,
                            cols=c.cols, ldx=ldx, ldr=ldr, ldy=ldy)
        torch.cuda.synchronize()

    def resout(self, c, t):
        ldx, ldr, ldy = c.lds
        N.residual_out(t.v("x"), t.v("r"), t.v("y"), rows=c.rows, cols=c.cols, ldx=ldx, ldr=ldr, ldy=ldy)
        torch.cuda.synchronize()

    def stats64(self, c, t):
        N.row_stats64(t.v("x"), t.row("out"), rows=c.rows, cols=c.cols, ldx=c.lds[0])
        torch.cuda.synchronize()


@pytest.mark.parametrize("case", lc.CASES, ids=[c.id for c in lc.CASES])
def test_layernorm_contract(case):
    c = case
    t = lc.make_tensors(c, "cuda", _mask)
    if c.op == "ln":
        assert lc.planned(c, t, N) == (c.fwd, c.bwd)  # the decision functions the launches below go through
    lc.run_case(c, t, NativeOps(), twice=True)
