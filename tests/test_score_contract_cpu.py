"""Caption scoring without a GPU: the C ABI's argument checks and the plan query (mit_score_rows, mit_score_rows_plan,
mit_score_sequences), the float64 reference against its float32 emulation on every case (BOUND_LOGPROB), the
properties the cases promise, and the host plumbing (candidate forms, ranking, the command line) over a stub model."""
import ctypes
import json

import numpy as np
import pytest
import torch

import native as N
import score_contract as sc


# ------------------------------------------------------------------------------------------------
# argument checks: before anything is recorded or launched
# ------------------------------------------------------------------------------------------------
def _buf():
    buf = (ctypes.c_double * 64)()
    return buf, ctypes.addressof(buf)


def _rows(**kw):
    lib = N.load_library()
    buf, a = _buf()
    d = dict(dtype=N.BF16, R=2, V=16, logits=a, ld=16, targets=a, ignore=0, tlp=a, rank=a)
    d.update(kw)
    return lib.mit_score_rows(d["dtype"], d["R"], d["V"], d["logits"], d["ld"], d["targets"], d["ignore"], d["tlp"],
                              d["rank"], None)


def _seqs(**kw):
    lib = N.load_library()
    buf, a = _buf()
    d = dict(n_seq=2, T=3, tlp=a, rank=a, out=a, tokens=a, hits=a)
    d.update(kw)
    return lib.mit_score_sequences(d["n_seq"], d["T"], d["tlp"], d["rank"], d["out"], d["tokens"], d["hits"], None)


@pytest.mark.parametrize("kw,word", [
    (dict(dtype=2), "dtype"), (dict(V=0), "vocabulary"), (dict(V=1 << 31, ld=1 << 31), "vocabulary"),
    (dict(ld=15), "ld"), (dict(R=-1), "row count"), (dict(R=1 << 31), "row count"), (dict(logits=None), "null"),
    (dict(targets=None), "null"), (dict(tlp=None), "null"),
])
def test_rows_rejects(kw, word):
    assert _rows(**kw) == 1
    assert word.encode() in N.lib().mit_last_error()


def test_rows_rejects_misaligned_elements_and_takes_empty_batches():
    buf, a = _buf()
    assert _rows(logits=a + 1) == 1 and b"aligned" in N.lib().mit_last_error()
    assert _rows(dtype=N.F32, logits=a + 2) == 1 and b"aligned" in N.lib().mit_last_error()
    assert _rows(R=0) == 0 and _rows(R=0, rank=None) == 0        # nothing launched: no GPU needed
    assert _seqs(n_seq=0) == 0


@pytest.mark.parametrize("kw,word", [
    (dict(n_seq=-1), "sequence count"), (dict(n_seq=1 << 31), "sequence count"), (dict(T=0), "sequence length"),
    (dict(tlp=None), "null"), (dict(out=None), "null"), (dict(rank=None), "need rank"),
    (dict(rank=None, hits=None), "need rank"),
])
def test_sequences_rejects(kw, word):
    assert _seqs(**kw) == 1
    assert word.encode() in N.lib().mit_last_error()


def test_rejected_calls_are_not_recorded():
    """the checks run before MIT_RECORD: a rejected call leaves a recording plan empty"""
    lib = N.load_library()
    lib.mit_plan_begin()
    assert _rows(V=0) == 1 and _rows(logits=None) == 1 and _seqs(T=0) == 1
    plan = lib.mit_plan_end()
    try:
        assert lib.mit_plan_size(plan) == 0
    finally:
        lib.mit_plan_destroy(plan)


def test_plan_query_needs_no_gpu_and_follows_dtype_and_row_length():
    buf, a = _buf()
    for c in sc.CASES:
        for ptr in (a, a + 2 * (c.dtype == "bf16") + 4 * (c.dtype == "f32")):          # aligned or not: one family
            got = N.lib().mit_score_rows_plan(sc._CODE[c.dtype], c.R, c.V, ptr, c.ld)
            assert got == sc.plan_expected(c.dtype, c.V), c.id
    assert N.score_rows_plan(N.BF16, 4, sc.REGS_MAX_V, None, sc.REGS_MAX_V) == -1      # logits NULL
    lib = N.lib()
    assert lib.mit_score_rows_plan(N.BF16, 4, sc.REGS_MAX_V, a, sc.REGS_MAX_V) == N.SCORE_REGS
    assert lib.mit_score_rows_plan(N.BF16, 4, sc.REGS_MAX_V + 1, a, sc.REGS_MAX_V + 1) == N.SCORE_STREAM
    assert lib.mit_score_rows_plan(N.F32, 4, 7, a, 7) == N.SCORE_STREAM
    assert lib.mit_score_rows_plan(N.BF16, 0, 7, a, 7) == N.SCORE_REGS                 # R = 0 is a valid call
    for bad in (dict(dtype=2), dict(V=0), dict(ld=6), dict(R=-1), dict(ptr=a + 1)):
        d = dict(dtype=N.BF16, R=4, V=7, ptr=a, ld=7)
        d.update(bad)
        assert lib.mit_score_rows_plan(d["dtype"], d["R"], d["V"], d["ptr"], d["ld"]) == -1, bad
    assert (N.SCORE_STREAM, N.SCORE_REGS) == (sc.SCORE_STREAM, sc.SCORE_REGS)


def test_run_score_cross_attention_shape_runs_the_head_kernel():
    """run_score's cross-attention at configs[1]: B batches of C*T queries (q / o batch stride C*T*d) over the
    image's S = 197 keys is the unmasked head-resident kernel for C = 1 and C = 5 alike (mit_attention_plan, no GPU);
    the self-attention over B*C sequences stays on the causal MFMA kernel"""
    d, L, S, T, H, B = 512, 6, 197, 100, 8, 256
    p = 1 << 20
    for C in (1, 5):
        ca = N.AttnArgs(p, d, C * T * d, p, L * 2 * d, S * L * 2 * d, p + 2 * d, L * 2 * d, S * L * 2 * d, p, d, C * T * d,
                        p, None, 0, 0, 0, 0.125, 0.0, None, 0)
        plan = N.attention_plan(N.BF16, B, H, C * T, S, ca, Dh=64)
        assert plan.fwd == N.ATTN_FWD_HEAD and plan.fwd_lkp == 208 and plan.fwd_nw == min(8, -(-C * T // 16))
        sa = N.AttnArgs(p, 3 * d, T * 3 * d, p + 2 * d, 3 * d, T * 3 * d, p + 4 * d, 3 * d, T * 3 * d, p, d, T * d, p, p, T,
                        0, 1, 0.125, 0.0, None, 0)
        assert N.attention_plan(N.BF16, B * C, H, T, T, sa, Dh=64).fwd == N.ATTN_FWD_MFMA


# ------------------------------------------------------------------------------------------------
# the cases, the reference, the emulation
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rows():
    return {c.id: sc.make_rows(c) for c in sc.CASES}


def test_cases_cover_what_the_contract_names():
    cs = sc.CASES
    for dt in ("bf16", "f32"):
        mine = [c for c in cs if c.dtype == dt]
        assert {c.V for c in mine} >= {1, 7, 64, 509, 10000, sc.REGS_MAX_V, sc.REGS_MAX_V + 1, 33000}
        assert any(c.V == 10000 and c.ld == 10048 for c in mine)
        assert any(c.ld == c.V for c in mine) and any(c.ld > c.V for c in mine)
        assert {c.T for c in mine} >= {1, 5}
        assert any(c.mis for c in mine) and any(not c.rank for c in mine) and any(c.ignore == 0 for c in mine)
        assert {sc.plan_expected(dt, c.V) for c in mine} == ({0, 1} if dt == "bf16" else {0})
    assert len({c.id for c in cs}) == len(cs)


def test_rows_hold_the_patterns_and_leave_no_freedom(rows):
    """targets at column 0 and V - 1, ignored rows of NaN, -inf columns, exact ties on both sides of the target,
    +0.0 / -0.0 ties; every column is an exact tie with the target or at least MARGIN away; the values are exact in
    the case's dtype"""
    for c in sc.CASES:
        x, tg = rows[c.id]
        assert torch.equal(x[tg != c.ignore], x[tg != c.ignore].to(sc._TORCH[c.dtype]).float())
        seen = set()
        for r in range(c.R):
            t = int(tg[r])
            if t == c.ignore:
                seen.add("ignored" if torch.isnan(x[r]).all() else "ignored-live")
                continue
            assert 0 <= t < c.V and torch.isfinite(x[r, t]) and not torch.isnan(x[r]).any()
            gap = (x[r] - x[r, t]).abs()
            assert (gap[gap > 0] >= sc.MARGIN).all(), (c.id, r, float(gap[gap > 0].min()))
            tie = (x[r] == x[r, t])
            seen |= {"first"} if t == 0 else set()
            seen |= {"last"} if t == c.V - 1 else set()
            if tie[:t].any() and tie[t + 1:].any():
                seen.add("ties")
                if float(x[r, t]) == 0.0 and (torch.signbit(x[r][tie]).any() and not torch.signbit(x[r][tie]).all()):
                    seen.add("zeros")
            if torch.isinf(x[r]).any():
                seen.add("neginf")
        want = {"last", "ignored"} | ({"first"} if c.ignore != 0 else {"ignored-live"})
        if c.V >= 7:
            want |= {"ties", "zeros", "neginf"}
        assert seen >= want, (c.id, want - seen)
        if c.T > 1:                       # a sequence mixes scored and ignored rows
            ign = (tg == c.ignore).view(c.n_seq, c.T)
            assert (ign.any(1) & ~ign.all(1)).any(), c.id
    for dt in ("bf16", "f32"):           # the aligned and the misaligned case share their rows
        a, b = rows[f"{dt}-V509-T5-ld512"], rows[f"{dt}-V509-T5-mis1"]
        assert torch.equal(a[0].nan_to_num(7.0), b[0].nan_to_num(7.0)) and torch.equal(a[1], b[1])


def test_reference_is_sane(rows):
    for c in sc.CASES:
        x, tg = rows[c.id]
        ref = sc.rows_reference(x, tg, c.ignore)
        for r in range(c.R):
            t = int(tg[r])
            if t == c.ignore:
                assert ref["logprob"][r] == 0 and ref["rank"][r] == -1
                continue
            lsm = torch.log_softmax(x[r].double(), 0)
            assert abs(float(ref["logprob"][r] - lsm[t])) < 1e-9 and ref["logprob"][r] <= 0
            order = sorted(range(c.V), key=lambda v: (-float(x[r, v]) + 0.0, v)) if c.V <= 509 else None
            if order is not None:
                assert order.index(t) == int(ref["rank"][r]), (c.id, r)
            assert (int(ref["rank"][r]) == 0) == (int(torch.argmax(x[r])) == t), (c.id, r)
            k = 5
            assert (int(ref["rank"][r]) < k) == (t in torch.topk(x[r], min(k, c.V)).indices.tolist()) or \
                bool((x[r] == x[r, t]).sum() > 1), (c.id, r)


def test_emulation_sets_the_bound():
    """BOUND_LOGPROB is 4 x the worst figure of the float32 emulation (both summation orders) over all cases"""
    worst = sc.emulation_figures()
    figure = max(f for f, _ in worst.values())
    print({k: (f"{f:.3f}", cid) for k, (f, cid) in worst.items()}, "BOUND_LOGPROB", sc.BOUND_LOGPROB)
    # 5 %: torch's float32 exp may differ by an ulp between CPU kernels, which moves the summation's rounding
    assert 0.95 * sc.BOUND_LOGPROB <= 4 * figure <= 1.05 * sc.BOUND_LOGPROB, \
        f"BOUND_LOGPROB {sc.BOUND_LOGPROB:.3f} is not 4 x the emulation's worst figure {figure:.3f}"


def test_sequences_reference():
    tlp = np.array([-1.5, -0.25, 0.0, -3.0, 0.0, 0.0], dtype=np.float32)
    rank = np.array([0, 3, -1, 0, -1, -1], dtype=np.int32)
    s, n, h = sc.sequences_reference(tlp, rank, 3)
    assert s.dtype == np.float32 and s.tolist() == [-1.75, -3.0] and n.tolist() == [2, 1] and h.tolist() == [1, 1]
    s1, n1, h1 = sc.sequences_reference(tlp, rank, 1)
    assert s1.tolist() == tlp.tolist() and n1.tolist() == [1, 1, 0, 1, 0, 0] and h1.tolist() == [1, 0, 0, 1, 0, 0]
    assert sc.sequences_reference(tlp, None, 3)[1] is None
    # the float32 order matters: the reference keeps it
    x = np.array([1e8, 1.0, -1e8, 1.0], dtype=np.float32)
    assert sc.sequences_reference(x, None, 4)[0].tolist() == [1.0]
    assert sc.sequences_reference(x, None, 4, np.float64)[0].tolist() == [2.0]


def test_guarded_buffers_of_a_case():
    c = sc.BY_ID["bf16-V7-T5-ld10"]
    t = sc.make(c)
    lg = t.a["logits"]
    w = lg.win(0, c.R, c.ld, c.ld)[:-1]                 # all but the last row: V values then ld - V NaN
    assert torch.isnan(w[:, c.V:]).all() and lg.whole.dtype == torch.bfloat16
    assert not t.a["logits"].allowed.any() and not t.a["targets"].allowed.any()
    assert int(t.a["tlp"].allowed.sum()) == c.R and int(t.a["seq_hits"].allowed.sum()) == c.n_seq
    assert "rank" not in sc.make(sc.BY_ID["bf16-V509-T5-ld512-rankFalse"]).a


# ------------------------------------------------------------------------------------------------
# host plumbing over a stub model
# ------------------------------------------------------------------------------------------------
class _Stub:
    device = "cpu"

    def __init__(self):
        self.calls = []

    def score_captions(self, chunk, cand, start, end):
        self.calls.append((chunk.shape[0], cand, start, end))
        B = chunk.shape[0]
        per = cand if isinstance(cand[0][0], (list, tuple)) else [cand] * B
        lp = torch.tensor([[-float(sum(c)) for c in img] for img in per])
        n = torch.tensor([[len(c) + 1 for c in img] for img in per], dtype=torch.int32)
        return lp, n, torch.zeros_like(n)


def test_rank_scores_follows_rank_beams():
    import inference
    from model import rank_beams
    lps, ns = [-6.0, -4.0, -4.0, -9.0], [3, 2, 4, 9]
    for lp_ in (0.0, 0.5, 1.0, 2.0):
        rows = inference.rank_scores(lps, ns, lp_)
        want = rank_beams([[i] for i in range(4)], lps, ns, 4, lp_, return_all=True)[0]
        assert [r[0] for r in rows] == [ids[0] for ids, _ in want], lp_
        for c, lp, n, s in rows:
            assert lp == lps[c] and n == ns[c] and s == lps[c] / ns[c] ** lp_
    assert [r[0] for r in inference.rank_scores([-1.0, -1.0], [2, 2])] == [0, 1]        # ties to the lower index


def test_score_captions_batches_images_and_cuts_per_image_candidates():
    import inference
    imgs = torch.zeros(5, 3, 4, 4)
    flat = [[5, 6], [7], [1, 1, 1]]
    m = _Stub()
    out = inference.score_captions(m, imgs, flat, batch_size=2, start_token_id=2, end_token_id=3)
    assert [(n, c) for n, c, _, _ in m.calls] == [(2, flat), (2, flat), (1, flat)] and m.calls[0][2:] == (2, 3)
    assert len(out) == 5 and all([r[0] for r in rows] == [2, 1, 0] for rows in out)
    per = [[[i], [i + 1, 1]] for i in range(5)]
    m = _Stub()
    out = inference.score_captions(m, imgs, per, batch_size=2, length_penalty=1.0)
    assert [c for _, c, _, _ in m.calls] == [per[0:2], per[2:4], per[4:5]]
    assert out[3][0] == (0, -3.0, 2, -1.5) and out[3][1] == (1, -5.0, 3, -5.0 / 3)
    with pytest.raises(ValueError):
        inference.score_captions(m, imgs, per[:4])


def test_command_line_score_file(tmp_path):
    import inference
    ap = inference.build_parser()
    base = ["--image_path", "a.png", "--checkpoint_path", "c.pt"]
    assert ap.parse_args(base).score_file is None
    p = tmp_path / "cands.json"
    p.write_text(json.dumps([[4, 5], [6]]))
    args = ap.parse_args(base + ["--score_file", str(p)])
    assert inference.load_score_file(args.score_file) == [[4, 5], [6]]
    assert "score_file" not in inference.decode_options(args)
    for extra in (["--beam_size", "3"], ["--temperature", "0.7"]):
        with pytest.raises(SystemExit):
            inference.main(base + ["--score_file", str(p)] + extra)
    p.write_text(json.dumps({"a": 1}))
    with pytest.raises(ValueError):
        inference.load_score_file(str(p))
