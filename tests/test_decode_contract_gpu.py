"""csrc/decode.hip's entry points on guarded buffers (tests/decode_contract.py): mit_attention_decode in its three
families (one block per (batch, head) in f32 and bf16 at every head dim and around every slab of keys; the one-block-
per-image kernels, with and without non-temporal loads, at every Lk where the two-buffer prefetch loop changes shape;
every mask, hot keys, the model's and the cross-attention's layouts, o_batch / tok_batch / rows between batches, Lk
ignored with pos, B = 0), mit_kv_store and mit_embed_decode (both dtypes, one row past the grid cap), mit_greedy_pick
on its vector and scalar paths (every reason alone; +inf / NaN behind V; ties within a thread, across threads and
waves; NaN, -inf, +-0), mit_greedy_pick_advance (three steps), mit_greedy_pick_keys (B past 1024), every
instantiation of mit_decode_gemm in both launch shapes (strides one at a time, K on either side of the wave-count
switch and at the odd step counts, the cache write with the LN operand, statistics that give every term of the merge
weight, the argmax keys slot by slot), mit_decode_layernorm, and a producer -> consumer chain on device statistics.
Two launches per case: the planned family is the case's, the results are within the bounds of decode_contract's
docstring of the float64 reference, the exact properties hold, nothing outside an output's window is written, no
input is written, and the second launch is bitwise equal to the first. Inputs are NaN outside their windows. Every
call is a valid call.

Each figure is printed before it is asserted (pytest -s / -rA shows them). Measured worst on an MI355X, in
decode_contract's units (bound); bf16 outputs: the part past 2^-8 |ref|:
  attention o    f32 0.22 (attn-bhf32-hot-last), bf16 0.09 (attn-rows_nt-hot-mid)                    (2.60)
  gemm C, z_out  1.32 (gemm-ln-relu-M64-N56-K504-Cz, z_out); C2 of the chain 0                       (6.29)
  stats_out      mean 1.19, M2 0.56, merged mean 1.19, merged variance 0.41                          (10.31)
  decode_layernorm out 0.42 (ln-M4-W1024)                                                            (1.67)
The attention spends a tenth of its bound: exp2f and the fused multiply-adds of the kernels are no worse than the
emulation's separate roundings. The LN-operand GEMM and decode_layernorm land on the float32 emulation's own figures
(the rounding of LN(z) to bf16 decides them, and it is the same arithmetic). No case came near its bound and the
exact contracts held everywhere: no kernel bug was found.
"""
import ctypes

import pytest
import torch

import decode_contract as dc
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
        pytest.exit(f"GPU error after a decode contract case, run ended: {e}", returncode=3)


def _dt(c):
    return N.BF16 if c.dtype == "bf16" else N.F32


class NativeOps:
    """libmit_hip.so on the case's buffers; every launch ends synchronised (the harness reads the buffers next)"""

    def launch(self, c, t):
        getattr(self, c.op)(c, t)
        torch.cuda.synchronize()

    def attn(self, c, t):
        a = dc.attn_plan_args(c, t)
        G = t.x["G"]
        N._check(N.lib().mit_attention_decode(_dt(c), a["B"], a["H"], a["Dh"], a["q"], a["q_batch"], a["k"], a["k_row"],
                                              a["k_batch"], a["v"], a["v_row"], a["v_batch"], a["o"], a["o_batch"],
                                              a["Lk"], a["pos"], a["key_tokens"], G["tok_batch"], c.pad_idx, G["scale"],
                                              N.stream_ptr()), "mit_attention_decode")

    def kvstore(self, c, t):
        G = t.x["G"]
        N._check(N.lib().mit_kv_store(_dt(c), c.B, c.n, t.ptr("src"), G["s_batch"], t.ptr("cache"), G["c_row"],
                                      G["c_batch"], t.ptr("pos"), N.stream_ptr()), "mit_kv_store")

    def embed(self, c, t):
        N._check(N.lib().mit_embed_decode(_dt(c), c.B, c.n, t.ptr("ids"), t.x["G"]["ld_ids"], t.ptr("pos"),
                                          t.ptr("table"), t.x["scale"], t.ptr("pe"), t.ptr("out"), N.stream_ptr()),
                 "mit_embed_decode")

    def pick(self, c, t):
        N._check(N.lib().mit_greedy_pick(t.x["B"], c.V, t.ptr("logits"), t.x["ld"], t.ptr("ids"), c.T, t.ptr("pos"),
                                         t.x["end_id"], t.x["pad_id"], t.ptr("finished"), t.ptr("n_finished"),
                                         N.stream_ptr()), "mit_greedy_pick")

    def pickadv(self, c, t):
        for _ in range(c.steps):
            N._check(N.lib().mit_greedy_pick_advance(t.x["B"], c.V, t.ptr("logits"), t.x["ld"], t.ptr("ids"), c.T,
                                                     t.ptr("pos"), t.x["end_id"], t.x["pad_id"], t.ptr("finished"),
                                                     t.ptr("n_finished"), t.ptr("ticket"), N.stream_ptr()),
                     "mit_greedy_pick_advance")

    def pickkeys(self, c, t):
        N._check(N.lib().mit_greedy_pick_keys(c.B, t.ptr("keys"), t.ptr("ids"), c.T, t.ptr("pos"), t.x["end_id"],
                                              t.x["pad_id"], t.ptr("finished"), t.ptr("n_finished"), N.stream_ptr()),
                 "mit_greedy_pick_keys")

    def gemm(self, c, t):
        g = dc.gemm_args(c, t, N)
        N._check(N.lib().mit_decode_gemm(ctypes.byref(g), N.stream_ptr()), "mit_decode_gemm")

    argmax = gemm

    def ln(self, c, t):
        N._check(N.lib().mit_decode_layernorm(c.M, c.W, t.ptr("z"), t.x["ldz"], t.ptr("stats"), t.ptr("gamma"),
                                              t.ptr("beta"), c.eps, t.ptr("out"), t.x["ldo"], N.stream_ptr()),
                 "mit_decode_layernorm")

    def chain(self, c, t):
        M, Nn, K = c.M, c.N, c.K
        g = N.DecodeGemmArgs()          # producer: z = A W1^T + bias + r, with the per-tile row statistics
        g.M, g.N, g.K, g.A, g.lda, g.B, g.ldb, g.bias = M, Nn, K, t.ptr("A"), K, t.ptr("B"), K, t.ptr("bias")
        g.r_mode, g.r, g.ldr, g.eps = 1, t.ptr("r"), Nn, c.eps
        g.z_out, g.ldz, g.stats_out = t.ptr("z_out"), Nn, t.ptr("stats_out")
        p = N.decode_gemm_plan(g)
        assert (p.a_mode, p.r_mode, p.waves) == (0, 1, 4)
        N._check(N.lib().mit_decode_gemm(ctypes.byref(g), N.stream_ptr()), "mit_decode_gemm")
        h = N.DecodeGemmArgs()          # consumer: C2 = LN(z) W2^T from the statistics on the device
        h.M, h.N, h.K, h.A, h.lda, h.B, h.ldb = M, 64, Nn, t.ptr("z_out"), Nn, t.ptr("B2"), Nn
        h.a_stats, h.a_gamma, h.a_beta, h.eps = t.ptr("stats_out"), t.ptr("gamma"), t.ptr("beta"), c.eps
        h.C, h.ldc = t.ptr("C2"), 64
        p = N.decode_gemm_plan(h)
        assert (p.a_mode, p.r_mode, p.waves) == (1, 0, 8)
        N._check(N.lib().mit_decode_gemm(ctypes.byref(h), N.stream_ptr()), "mit_decode_gemm")


@pytest.mark.parametrize("case", dc.CASES, ids=[c.id for c in dc.CASES])
def test_decode_contract(case):
    c = case
    t = dc.make_tensors(c, "cuda")
    dc.check_plan(c, t, N)  # the decision functions the launches below go through
    dc.run_case(c, t, NativeOps(), twice=True)
