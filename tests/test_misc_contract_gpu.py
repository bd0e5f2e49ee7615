"""csrc/misc.hip's entry points on guarded buffers (tests/misc_contract.py): both cross-entropy kernels on both
sides of 10240 (V % 8 != 0 with the masked tail, f32, row_loss NULL, a misaligned pointer, ld = 523, 256-thread
tails; rows 1 / 4 / 5 / 9; every 3rd / every / no row ignored; want_grad 0; loss_sum starting at 3.5),
mit_count_targets past its block cap, mit_embed_fwd (both dtypes, dropout, seeds NULL / above 2^32, past the grid
cap), all five embed_plan_kernel instances against a stable sort, mit_embed_bwd planned (d 8 / 128 / 520 / 1024,
runs of 1 / 15 / 16 / 17 / 33 rows, PAD, all PAD, a sentinel-filled dtable) and atomic, mit_colsum (M around 128,
N around 256, ld, accumulate, M = 0), mit_grad_norm on either side of max_norm, mit_adamw one step from a given
state and a five-step chain, mit_im2col / mit_vit_assemble in both families, mit_cast_f32 on special values,
mit_dropout_mask against the host hash, mit_scalar_div, mit_step_inc.
Two launches per case: the planned family is the case's, the results are within the bounds of misc_contract's
docstring of the float64 reference, the exact properties hold, nothing outside an output's window is written, no
input is written, and the second launch is bitwise equal to the first (float-atomic outputs apart). Inputs are NaN
outside their windows. Every call is a valid call.

Each figure is printed before it is asserted (pytest -s / -rA shows them). Measured worst on an MI355X, in
misc_contract's units (bound); bf16 outputs: the part past 2^-8 |ref|:
  cross-entropy  row_loss 0.84 (20.8); loss_sum 0.60 (6.68); gradient f32 0.61, bf16 0 (2.0)
  embedding      forward f32 0.87, bf16 0 (5.20); backward 1.59 planned and atomic (7.84)
  colsum 2.49 (9.97); norm 0.52 (3.21); coef 1.00 (4.54)
  adamw          m 0.43 (1.97); v 1.01 (4.03); p 0.87 (4.04); p after the five-step chain 0.37 (8.09)
colsum, the AdamW moments and the cross-entropy losses land on the float32 emulation's own figures (the same
operations in the same order); the f32 cross-entropy gradient spends 0.61 of its 2.0 units, less than half of the
margin, on __expf and the reciprocal of the sum."""
import math

import pytest
import torch

import misc_contract as mc
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
        pytest.exit(f"GPU error after a misc contract case, run ended: {e}", returncode=3)


def _mask(n, p, seed, site):
    out = torch.empty(n, device="cuda")
    N.dropout_mask(n, p, seed, site, out)
    torch.cuda.synchronize()
    return out


class NativeOps:
    """libmit_hip.so on the case's buffers; every method ends synchronised (the harness reads the buffers next)"""

    def ce(self, c, t):
        N.cross_entropy(t.v("logits"), t.row("targets"), mc.CE_IGNORE, t.row("count"), t.row("loss_sum"), c.want_grad,
                        rows=c.rows, V=c.cols, ld=c.ld, row_loss=t.row("row_loss"))
        torch.cuda.synchronize()

    def count(self, c, t):
        N.count_targets(t.row("targets"), 0, t.row("count"), n=c.cols)
        torch.cuda.synchronize()

    def embfwd(self, c, t):
        N.embed_fwd(t.row("tokens"), t.v("table"), math.sqrt(c.cols), t.v("pe"), t.row("out"), drop_p=c.drop_p,
                    seed=t.row("seed"), site=c.site, B=c.B, T=c.T, d=c.cols)
        torch.cuda.synchronize()

    def embplan(self, c, t):
        N.embed_plan(t.row("tokens"), t.row("plan"), n=c.cols)
        torch.cuda.synchronize()

    def embbwd(self, c, t):
        n = c.B * c.T
        if c.planned:
            N.embed_plan(t.row("tokens"), t.row("plan"), n=n)
        N.embed_bwd(t.row("tokens"), t.v("dx"), math.sqrt(c.cols), t.v("dtable"), mc.PAD, drop_p=c.drop_p,
                    seed=t.row("seed"), site=c.site, plan=t.row("plan") if c.planned else None, B=c.B, T=c.T, d=c.cols)
        torch.cuda.synchronize()

    def colsum(self, c, t):
        assert c.rows == 0 or t.row("ws").numel() == N.colsum_ws_floats(c.rows, c.cols)
        N.colsum(t.v("dy"), c.rows, c.cols, t.row("out"), t.row("ws"), ld=c.ld, accumulate=c.accumulate)
        torch.cuda.synchronize()

    def gnorm(self, c, t):
        assert t.row("ws").numel() == N.grad_norm_ws_floats(c.cols)
        N.grad_norm(t.row("grads"), t.x["max_norm"], t.row("ws"), t.row("norm_out"), n=c.cols)
        torch.cuda.synchronize()

    def adamw(self, c, t):
        N.adamw(t.row("p"), t.row("g"), t.row("m"), t.row("v"), t.row("shadow"), t.row("norm_out"), t.row("lr"),
                t.row("step"), mc.B1, mc.B2, mc.EPS, c.wd, n=c.cols)
        torch.cuda.synchronize()

    def adamchain(self, c, t):
        g0 = t.b["g"].view.clone()
        for s, lr in enumerate(mc.CHAIN_LR, start=1):
            N.step_inc(t.row("step"))
            t.row("lr").fill_(lr)  # lr lives in device memory: changed between steps without a new argument
            t.b["g"].view.copy_(g0 * s)
            self.adamw(c, t)
        t.b["g"].view.copy_(g0)
        torch.cuda.synchronize()

    def im2col(self, c, t):
        C, H, W, P, kpad = c.geom
        N.im2col(t.row("img"), t.v("out"), P, kpad, shape=(c.B, C, H, W))
        torch.cuda.synchronize()

    def assemble(self, c, t):
        np_, E = c.geom
        N.vit_assemble(t.v("patch"), t.row("cls"), t.v("pos"), t.v("h"), c.B, np_, E)
        torch.cuda.synchronize()

    def cast(self, c, t):
        N.cast_f32(t.row("src"), t.row("dst"))
        torch.cuda.synchronize()

    def mask(self, c, t):
        N.dropout_mask(c.cols, c.drop_p, t.row("seed"), c.site, t.row("out"))
        torch.cuda.synchronize()

    def sdiv(self, c, t):
        N.scalar_div(t.row("a"), t.row("b"), t.row("out"))
        torch.cuda.synchronize()

    def stepinc(self, c, t):
        N.step_inc(t.row("step"))
        torch.cuda.synchronize()


@pytest.mark.parametrize("case", mc.CASES, ids=[c.id for c in mc.CASES])
def test_misc_contract(case):
    c = case
    t = mc.make_tensors(c, "cuda", _mask)
    if mc.expected_plan(c) is not None:
        assert mc.planned(c, t, N) == mc.expected_plan(c)  # the decision functions the launches below go through
    mc.run_case(c, t, NativeOps(), twice=True)
