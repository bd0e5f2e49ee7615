"""mit_attention_fwd / mit_attention_bwd on guarded, strided operands (tests/attn_contract.py): every kernel family
behind the two dispatch functions of csrc/attention.hip (generic, attn_fwd_mfma, attn_fwd_head with and without
dropout; generic, the dq / dkv MFMA pair, attn_bwd_head) on both sides of every dispatch boundary, under no mask,
causal alone, key_tokens alone (the decoder's cross-attention) and both, with leading / interior / whole-tile /
all-but-one padding, in the product's q|k|v and layered K|V layouts with and without rows between the batches,
with operands off the MFMA kernels' alignment, with keys that outscore the rest by ~100 in the first tile, a
middle chunk and the ragged tail, with scores of standard deviation 4, and with a fully masked row.
Two launches per case and direction: mit_attention_plan of the launched arguments is the case's, the results
match the float64 reference of the header's formula per (batch, head) slice, dk / dv are exactly zero at padded
and unseen keys, nothing outside an output's windows is written, no input is written at all, and the second
launch is bitwise equal to the first. Inputs are NaN outside their windows; padded keys hold +-1e4 K and V rows.
Every call is a valid call.

Bounds: attn_contract's docstring. Each figure is printed before it is asserted (pytest -s / -rA shows them).
Measured worst (batch, head) slice per family on an MI355X, as a fraction of the slice's max|ref| (bound):
  forward  generic        bf16 o 3.6e-3 (2e-2), lse 1.9e-7 (1e-3); f32 o 1.2e-6 (1e-4), lse 5.2e-7 (1e-5)
           attn_fwd_mfma  o 4.1e-3 (2e-2), lse 2.9e-7 (1e-3)
           attn_fwd_head  o 3.8e-3 (2e-2), lse 1.6e-4 (1e-3: the denominator sums bf16-rounded p); with
                          dropout o 4.6e-3, lse 1.4e-7
  backward generic        bf16 dq 5.6e-3, dk 5.3e-3, dv 3.5e-3 (4e-2); f32 dq 1.7e-6, dk 1.6e-6, dv 1.6e-6 (2e-4)
           dq / dkv MFMA  dq 5.8e-3, dk 8.0e-3, dv 5.6e-3 (4e-2)
           attn_bwd_head  dq 8.7e-3, dk 8.6e-3, dv 5.1e-3 (4e-2)
The hot-key cases give o exactly (one key holds all the weight) and lse within 6e-7."""
import pytest
import torch

import attn_contract as ac
import native as N

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    N.load_library()
    try:
        yield
    finally:
        N.attention_set_index_limit(0.0)
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:  # a GPU fault poisons the process: launch nothing more on it
        pytest.exit(f"GPU error after an attention contract case, run ended: {e}", returncode=3)


def _mask(n, p, seed, site):
    out = torch.empty(n, device="cuda")
    N.dropout_mask(n, p, seed, site, out)
    return out


def _twice(case, t, names, launch, what):
    launch()
    torch.cuda.synchronize()
    first = ac.output_bits(t, names)
    launch()
    torch.cuda.synchronize()
    ac.same_bits(t, names, first, f"{case.id} {what}")


@pytest.mark.parametrize("case", ac.CASES, ids=[c.id for c in ac.CASES])
def test_attention_contract(case):
    c = case
    t = ac.make_tensors(c, "cuda", _mask)
    ref = ac.reference(c, t)
    dt = N.BF16 if c.dtype == "bf16" else N.F32
    a, g = ac.attn_structs(c, t, N)
    N.attention_set_index_limit(c.index_limit)
    assert ac.planned(c, t, N) == ac.declared(c)  # the decision functions the two launches below go through
    ac.snapshot(t)
    _twice(c, t, ac.FWD_OUT, lambda: N.attention_fwd(dt, c.B, c.H, c.Lq, c.Lk, a, Dh=c.Dh), "forward")
    ac.check_fwd(c, t, ref)
    if c.bwd:
        ac.snapshot(t)
        _twice(c, t, ac.BWD_OUT, lambda: N.attention_bwd(dt, c.B, c.H, c.Lq, c.Lk, a, g, Dh=c.Dh), "backward")
        ac.check_bwd(c, t, ref)
