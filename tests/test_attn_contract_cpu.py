"""The attention contract harness (tests/attn_contract.py) without a GPU:
  * its float64 reference equals F.scaled_dot_product_attention in float64 with the materialised float mask
    (and autograd's gradients), on every case without dropout and without a fully masked row;
  * every case plans onto the kernel families it names (mit_attention_plan on the case's CPU buffers: same
    strides and alignment, nothing dereferenced), every family and both sides of every boundary of
    csrc/attention.hip's dispatch are hit, and mit_attention_set_index_limit is honoured;
  * the harness catches a subtly wrong kernel: fake_attention, a torch attention on the same guarded buffers,
    passes every case as it is, stays within half of every value bound in its bf16-emulation mode, and fails
    the named case with each injected fault."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import attn_contract as ac
import native

CASES = ac.CASES
_cache = {}


def _tensors_and_ref(case):
    """one set of buffers and one float64 reference per case, shared (the inputs are never written)"""
    if case.id not in _cache:
        t = ac.make_tensors(case)
        _cache[case.id] = (t, ac.reference(case, t))
    return _cache[case.id]


@pytest.fixture(scope="module")
def lib():
    lib = native.load_library()
    yield lib
    assert lib.mit_attention_set_index_limit(0.0) == 0


def _run_fake(case, **kw):
    t, ref = _tensors_and_ref(case)
    for name in ("o", "lse", "dq", "dkv", "delta"):  # fresh outputs
        t.bufs[name].whole.fill_(ac.SENTINEL)
    ac.snapshot(t)
    ac.fake_attention(case, t, **kw)
    fig = ac.check_fwd(case, t, ref)
    if case.bwd:
        ac.snapshot(t)
        ac.fake_attention(case, t, backward=True, **kw)
        fig.update(ac.check_bwd(case, t, ref))
    return fig


@pytest.mark.parametrize("case", [c for c in CASES if c.drop_p == 0 and c.pad != "row0"], ids=lambda c: c.id)
def test_reference_equals_sdpa(case):
    c = case
    t, ref = _tensors_and_ref(c)
    q, k, v, dout = (ac._heads(t.v[n].double(), c.H).clone().requires_grad_(n != "dout") for n in ac.INPUTS)
    mask = torch.zeros(c.B, 1, c.Lq, c.Lk, dtype=torch.float64).masked_fill(ac.dead_keys(c, t.tok), float("-inf"))
    o = F.scaled_dot_product_attention(q, k, v, attn_mask=mask, scale=c.scale)
    torch.testing.assert_close(ref["o"], o.detach(), rtol=1e-10, atol=1e-10)
    s = (q.detach() @ k.detach().transpose(-1, -2)) * c.scale + mask
    torch.testing.assert_close(ref["lse"], torch.logsumexp(s, -1), rtol=1e-12, atol=1e-12)
    if c.bwd:
        o.backward(dout)
        for name, x in (("dq", q), ("dk", k), ("dv", v)):
            torch.testing.assert_close(ref[name], x.grad, rtol=1e-9, atol=1e-9, msg=lambda m: f"{name}: {m}")


def test_reference_of_a_fully_masked_row():
    c = ac.BY_ID["row0-mfma-40x70"]
    _, ref = _tensors_and_ref(c)
    nan_rows = torch.isnan(ref["o"]).all(-1)  # [B, H, Lq]
    want = torch.zeros(c.B, c.H, c.Lq, dtype=torch.bool)
    want[1, :, 0] = True
    assert torch.equal(nan_rows, want) and torch.equal(torch.isnan(ref["o"]).any(-1), want)
    assert torch.equal(ref["lse"] == float("-inf"), want) and torch.isfinite(ref["lse"][~want]).all()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_case_plans_onto_its_families(lib, case):
    t, _ = _tensors_and_ref(case)
    assert lib.mit_attention_set_index_limit(case.index_limit) == 0
    try:
        assert ac.planned(case, t, native) == ac.declared(case)
    finally:
        assert lib.mit_attention_set_index_limit(0.0) == 0


def test_plan_honours_the_index_limit_and_rejects_nulls(lib):
    c = ac.BY_ID["idx64-drop-63x65"]
    t, _ = _tensors_and_ref(c)
    assert ac.planned(c, t, native)[0] == "head_drop" and ac.planned(c, t, native)[3] == "head"  # default limit 2^32
    n = c.B * c.H * c.Lq * c.Lk
    try:
        assert lib.mit_attention_set_index_limit(float(n)) == 0  # B*H*Lq*Lk >= limit: the 64-bit-index kernels
        assert ac.planned(c, t, native)[0] == "generic" and ac.planned(c, t, native)[3] == "mfma"
        assert lib.mit_attention_set_index_limit(float(n + 1)) == 0
        assert ac.planned(c, t, native)[0] == "head_drop"
    finally:
        assert lib.mit_attention_set_index_limit(0.0) == 0
    assert lib.mit_attention_plan(native.BF16, 2, 3, 4, 4, 64, None, None, None) == 1
    assert b"null pointer" in lib.mit_last_error()
    a, _ = ac.attn_structs(c, t, native)
    out = native.AttnPlan()
    assert lib.mit_attention_plan(native.BF16, 2, 3, 4, 4, 48, ctypes.byref(a), None, ctypes.byref(out)) == 1
    assert b"head_dim" in lib.mit_last_error()
    p = native.attention_plan(native.BF16, c.B, c.H, c.Lq, c.Lk, a, None)  # no grads: the backward is not planned
    assert p.bwd == -1 and p.bwd_nw == 0


def test_table_hits_every_family_and_both_sides_of_every_boundary():
    cs = CASES
    assert {c.fwd for c in cs} == set(ac.FWD_FAMILIES) and {c.bwd for c in cs} == set(ac.BWD_FAMILIES) | {None}
    mf = [c for c in cs if c.dtype == "bf16" and c.Dh == 64 and c.layout in ("sep", "self", "self+16", "cross", "cross+16")
          and c.index_limit == 0]  # MFMA-eligible operands
    assert all(c.fwd != "generic" and c.bwd != "generic" for c in mf)
    head = [c for c in mf if c.fwd in ("head", "head_drop")]
    assert all(not c.causal and c.pad is None and c.Lk <= ac.HK_MAX for c in head)
    # HK_MAX: Lk = 640 on attn_fwd_head, 641 on attn_fwd_mfma, both without a mask
    assert any(c.Lk == ac.HK_MAX for c in head)
    assert any(c.fwd == "mfma" and c.Lk == ac.HK_MAX + 1 and not c.causal and c.pad is None for c in mf)
    # a mask of either kind alone, and both, send a head shape to attn_fwd_mfma
    small = [c for c in mf if c.fwd == "mfma" and c.Lk <= ac.HK_MAX]
    assert {(c.causal, c.pad is not None) for c in small} == {(True, False), (False, True), (True, True)}
    # the 8 / 16 wave cap at lkp = 320: more than 8 query tiles on both sides of it, and under dropout
    assert any(c.lkp == ac.HEAD8_LKP and c.nw == 8 and c.Lq > 128 for c in head)
    assert any(c.lkp == ac.HEAD8_LKP + 16 and c.nw > 8 and c.fwd == "head" for c in head)
    assert any(c.lkp > ac.HEAD8_LKP and c.nw == 8 and c.Lq > 128 and c.fwd == "head_drop" for c in head)
    assert any(c.nw == 16 and c.Lq > 256 for c in head)  # more query tiles than waves at the cap of 16
    assert {(c.lkp % 64) // 16 for c in head} == {0, 1, 2, 3}  # every length of the 16-key-tile tail
    # attn_bwd_head's limits: Lq <= 64 and Lk <= 256, each from both sides
    hb = [c for c in mf if c.bwd == "head"]
    assert any(c.Lq == 64 and c.Lk == ac.HB_MAXK for c in hb)
    assert any(c.bwd == "mfma" and c.Lq == 65 and c.Lk == ac.HB_MAXK for c in mf)
    assert any(c.bwd == "mfma" and c.Lq == 64 and c.Lk == ac.HB_MAXK + 1 for c in mf)
    assert {c.bwd_lkp - c.Lk >= 16 for c in hb} == {True, False}  # attn_bwd_head stages 32-row multiples
    for fam in ("head", "mfma"):  # each backward family under no mask, causal, key_tokens alone, dropout
        b = [c for c in mf if c.bwd == fam]
        assert any(not c.causal and c.pad is None and not c.drop_p for c in b), fam
        assert any(c.causal and c.pad is None for c in b) and any(c.pad and not c.causal for c in b), fam
        assert any(c.drop_p for c in b), fam
    # the alignment rules, each alone; the 64-bit dropout indices
    assert {(c.layout, c.fwd, c.bwd) for c in cs if c.layout in ("qrow4", "kptr2", "orow4", "dqrow2")} == {
        ("qrow4", "generic", "generic"), ("kptr2", "generic", "generic"), ("orow4", "head", "generic"),
        ("orow4", "mfma", "generic"), ("dqrow2", "head", "generic")}
    assert any(c.index_limit and c.fwd == "generic" and c.bwd == "mfma" for c in cs)
    # the generic kernels: every head_dim and dtype under causal + key_tokens, key_tokens alone, dropout, a strided layout
    gen = [c for c in cs if c.fwd == "generic" and c.bwd == "generic" and c.layout in ("sep", "cross", "cross+16", "self+16")]
    combos = {(c.dtype, c.Dh) for c in gen}
    assert combos == {("bf16", 16), ("bf16", 32), ("bf16", 128), ("f32", 16), ("f32", 32), ("f32", 64), ("f32", 128)}
    for dt, dh in combos:
        g = [c for c in gen if (c.dtype, c.Dh) == (dt, dh)]
        assert any(c.causal and c.pad for c in g) and any(c.pad and not c.causal for c in g)
        assert any(c.drop_p for c in g) and any(c.layout != "sep" for c in g)
    # padding patterns on three or more key tiles; hot keys in each position on each forward family
    assert {c.pad for c in cs if c.Lk > 128 and c.pad} >= {"trail", "lead", "holes", "tile1", "tile0", "one"}
    assert {(c.hot, c.fwd) for c in cs if c.hot} == {(w, f) for w in ("first", "mid", "tail") for f in ("head", "mfma", "generic")}
    for c in cs:  # no row is fully masked except where the case says so
        if c.pad:
            dead = ac.dead_keys(c, ac._tokens(c)).all(-1)
            assert bool(dead.any()) == (c.pad == "row0"), c.id
    assert all(c.bwd is None for c in cs if c.hot or c.pad == "row0")


def test_buffers_are_nan_outside_the_windows_and_big_at_padded_keys():
    c = ac.BY_ID["cross+16-tok-63x197"]
    t, _ = _tensors_and_ref(c)
    kv = t.bufs["kv"]
    r = t.reg["k"]
    assert kv.whole[:ac.GUARD].isnan().all() and kv.whole[-ac.GUARD:].isnan().all()
    for b in range(c.B):  # every layer's data; then the gap rows (after the last batch: one row)
        rows = kv.whole[kv.base + b * r.batch:kv.base + b * r.batch + (c.Lk + 1) * r.row].view(c.Lk + 1, r.row)
        assert rows[c.Lk:].isnan().all() and rows[:c.Lk].isfinite().all()
    assert kv.whole[kv.base + c.Lk * r.row:kv.base + r.batch].isnan().all() and r.batch == (c.Lk + 16) * r.row
    b, j = (t.tok == ac.PAD_IDX).nonzero()[0].tolist()
    assert (t.v["k"][b, j].float().abs() > 0.9 * ac.BIG).all() and (t.v["v"][b, j].float().abs() > 0.9 * ac.BIG).all()
    assert r.row == 6 * c.W and r.off == 2 * c.W and t.reg["v"].off == 3 * c.W
    s = ac.BY_ID["self-causal-trail-63x63"]
    rs = ac.regions(s)[0]
    assert [rs[n].off for n in "qkv"] == [0, s.W, 2 * s.W] and rs["q"].row == 3 * s.W and rs["o"].row == s.W
    assert rs["dk"].buf == rs["dv"].buf and rs["dv"].off == s.W
    tok = t.bufs["tok"]
    assert (tok.whole[tok.base + c.Lk:tok.base + t.tok_batch] == ac.LIVE_TOKEN).all()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_faultless_fake_attention_passes(case):
    _run_fake(case)


@pytest.mark.parametrize("case", [c for c in CASES if c.dtype == "bf16"], ids=lambda c: c.id)
def test_bf16_emulation_stays_within_half_of_every_bound(case):
    fig = _run_fake(case, emulate_bf16=True)
    tol = ac.TOL["bf16"]
    for what, ratio in fig.items():
        bound = tol["o"] if what == "o" else tol["lse"] if what == "lse" else tol["grad"]
        assert ratio <= 0.5 * bound, f"{case.id} {what}: {ratio:.3e} against half of {bound}"


def test_every_fault_names_a_case_it_applies_to():
    assert set(ac.FAULT_CASE) == set(ac.FAULTS)
    for f, cid in ac.FAULT_CASE.items():
        assert ac.fault_applies(ac.BY_ID[cid], f), (f, cid)


@pytest.mark.parametrize("fault", ac.FAULTS)
def test_injected_fault_is_caught(fault):
    with pytest.raises(AssertionError):
        _run_fake(ac.BY_ID[ac.FAULT_CASE[fault]], fault=fault)
