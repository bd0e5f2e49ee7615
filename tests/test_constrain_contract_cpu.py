"""Constrained decoding without a GPU: the reference against hand-written rows, the C ABI's argument checks
(mit_logits_constrain), DecodeConstraints and the command-line plumbing, and the constrained greedy trajectories of the
pinned CPU oracle that the GPU decodes are compared with (every free step decided by more than 2 TAU)."""
import ctypes
import re

import numpy as np
import pytest
import torch

import constrain_contract as cc
import fixtures as FX
import native as N
from test_capi import HEADER

INF = float("inf")


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32).tolist()


def _ref(row, hist, **kw):
    return cc.constrain_reference(np.array(row, dtype=np.float32), hist, **kw)


# ------------------------------------------------------------------------------------------------
# 1. the reference, one tiny row per rule
# ------------------------------------------------------------------------------------------------
def test_reference_repetition_penalty():
    row = [2.0, -2.0, 0.0, -0.0, -INF, 3.0, 1.0]
    th = np.float32(1.3)
    rinv = np.float32(1.0) / th
    # token 0 three times: changed once; 9 and -1 are outside [0, 7): skipped; token 6 is not in the history
    got = _ref(row, [0, 1, 0, 2, 3, 4, 0, 9, -1], theta=1.3)
    want = [np.float32(2.0) * rinv, np.float32(-2.0) * th, np.float32(0.0) * th, np.float32(-0.0) * th, -INF, 3.0, 1.0]
    assert _bits(got) == _bits(want)
    assert np.signbit(got[3]) and not np.signbit(got[2])          # -0.0 and 0.0 take the l * theta case
    assert got[0] != np.float32(2.0) * rinv * rinv
    assert _bits(_ref(row, [0, 1, 0], theta=1.0)) == _bits(row)
    got = _ref(row, [0, 1], theta=0.8)                           # theta < 1 rewards repetition
    assert got[0] == np.float32(2.0) * (np.float32(1.0) / np.float32(0.8)) > 2.0 and got[1] == np.float32(-2.0) * np.float32(0.8)


def test_reference_no_repeat_ngram():
    row = [1.0] * 8
    banned = lambda out: [i for i, x in enumerate(out) if x == -INF]  # noqa: E731
    h = [2, 5, 6, 2, 5, 7, 2, 5]
    assert banned(_ref(row, h, n=3)) == [6, 7]                    # (2, 5) was followed by 6 and by 7
    assert banned(_ref(row, h, n=2)) == [6, 7]                    # 5 was followed by 6 and by 7
    assert banned(_ref(row, h, n=1)) == [2, 5, 6, 7]              # n = 1 bans the whole history
    assert banned(_ref(row, h, n=4)) == []                        # (7, 2, 5) has not occurred before
    assert banned(_ref(row, [2, 5, 6, 2, 5, 7, 6, 2, 5], n=4)) == [7]
    assert banned(_ref(row, [3], n=2)) == [] and banned(_ref(row, [3], n=1)) == [3]
    assert banned(_ref(row, [3, 3], n=3)) == []                   # p + 1 < n: off
    assert banned(_ref(row, [3, 3, 3], n=3)) == [3]               # p + 1 == n: the first window already counts
    assert banned(_ref(row, [9, 4, 9], n=2)) == [4]               # ids outside [0, V) compare, but are never banned
    assert banned(_ref(row, [4, 9, 4], n=2)) == []
    assert banned(_ref(row, h, n=0)) == []


def test_reference_min_length_suppress_and_forced():
    row = [0.5, 1.5, -1.0, 2.5]
    assert _bits(_ref(row, [0, 1], min_length=2, end=3)) == _bits([0.5, 1.5, -1.0, -INF])      # p = 1 < 2
    assert _bits(_ref(row, [0, 1, 1], min_length=2, end=3)) == _bits(row)                      # p = 2: END allowed
    assert _bits(_ref(row, [0], min_length=5, end=7)) == _bits(row)                            # END outside [0, V)
    assert _bits(_ref(row, [0], suppress=(1, 2, 9, -1))) == _bits([0.5, -INF, -INF, 2.5])
    assert _bits(_ref(row, [0], forced_token=2)) == _bits([-INF, -INF, 0.0, -INF])
    assert _bits(_ref(row, [0], forced_token=-1)) == _bits(row)
    assert _bits(_ref(row, [0], forced_token=4)) == _bits(row)                                 # outside [0, V): free
    lsm = torch.log_softmax(torch.from_numpy(_ref(row, [0], forced_token=2)).double(), 0)
    assert float(lsm[2]) == 0.0                                                                # a prompt costs nothing


def test_reference_ordering():
    row = [2.0, 3.0, -1.0, 4.0]
    # a ban beats a penalty: token 1 is penalised (in the history) and banned (bigram 0 -> 1), token 3 penalised
    # and suppressed; token 0 only penalised
    got = _ref(row, [3, 0, 1, 0], theta=1.3, n=2, suppress=(3,))
    rinv = np.float32(1.0) / np.float32(1.3)
    assert _bits(got) == _bits([np.float32(2.0) * rinv, -INF, -1.0, -INF])
    # forcing beats everything, a banned token included
    got = _ref(row, [3, 0, 1, 0], theta=1.3, n=2, min_length=9, end=2, suppress=(1, 3), forced_token=1)
    assert _bits(got) == _bits([-INF, 0.0, -INF, -INF])


def test_cases_cover_what_the_contract_names():
    cs = cc.CASES
    assert len({c.id for c in cs}) == len(cs)
    for V in cc.CON_V:
        for R in cc.CON_R:
            sub = [c for c in cs if c.V == V and c.R == R]
            assert {c.theta for c in sub} >= set(cc.CON_THETA) and {c.n for c in sub} >= set(cc.CON_N)
    assert {c.p for c in cs} >= {0, 1, 2, 3, 20, 300}
    for n in cc.CON_N[1:]:
        assert {c.p for c in cs if c.n == n} >= {max(n - 2, 0), n - 1, 20}
    assert any(c.p == 300 and (c.ld_tok == 512) for c in cs)
    assert any(c.min_length == c.p + 1 for c in cs) and any(c.min_length == c.p and c.p > 0 for c in cs)
    assert {c.forced for c in cs} == {"none", "free", "banned", "beyond"} and {c.sup for c in cs} == {"none", "overlap"}
    assert {c.group for c in cs} >= {1, 3, 8}


def test_cases_are_built_as_described():
    """duplicates and out-of-range ids in the histories, special values under the history's tokens, NaN finished rows
    and padding, an ancestry that crosses slots, forced rows that become one-hot"""
    seen = dict(dup=0, oor=0, negzero=0, neginf=0, cross=0, onehot=0, ban_on_penalty=0, end_banned=0)
    for c in cc.CASES:
        t = cc.make_case(c)
        for r in range(c.R):
            h, w = t.x["hist"][r], t.x["want"][r]
            if h is None:
                assert torch.isnan(t.x["logits"][r]).all()
                continue
            seen["dup"] += len(set(h)) < len(h)
            seen["oor"] += any(v >= c.V or v < 0 for v in h)
            row = t.x["logits"][r].numpy()
            inr = [v for v in h if 0 <= v < c.V]
            seen["negzero"] += any(row[v] == 0 and np.signbit(row[v]) for v in inr)
            seen["neginf"] += any(row[v] == -INF for v in inr)
            seen["onehot"] += int((w == -INF).sum() == c.V - 1 and (w == 0).sum() == 1)
            seen["ban_on_penalty"] += c.theta != 1.0 and any(w[v] == -INF and row[v] != -INF for v in inr)
            seen["end_banned"] += c.p < c.min_length and w[t.x["end_id"]] == -INF
            assert not np.isnan(w).any()
        if c.group > 1:
            anc = t.a["anc"].win(0, c.R, c.p + 1, t.x["ld_tok"])
            seen["cross"] += bool((anc != torch.arange(c.R).view(-1, 1) % c.group).any())
    assert all(v > 0 for v in seen.values()), seen


# ------------------------------------------------------------------------------------------------
# 2. argument checks: before anything is recorded or launched, without a GPU
# ------------------------------------------------------------------------------------------------
def _call(**kw):
    lib = N.load_library()
    buf = (ctypes.c_double * 64)()
    a = ctypes.addressof(buf)
    d = dict(R=4, V=16, logits=a, ld=16, tok=a, ld_tok=8, pos=a, group=1, anc=None, ld_anc=0, finished=None, theta=1.0,
             n=0, ml=0, end=1, suppress=None, n_suppress=0, forced=None, ld_forced=0)
    d.update(kw)
    return lib.mit_logits_constrain(d["R"], d["V"], d["logits"], d["ld"], d["tok"], d["ld_tok"], d["pos"], d["group"],
                                    d["anc"], d["ld_anc"], d["finished"], d["theta"], d["n"], d["ml"], d["end"],
                                    d["suppress"], d["n_suppress"], d["forced"], d["ld_forced"], None)


_BUF = (ctypes.c_double * 8)()
_A = ctypes.addressof(_BUF)


@pytest.mark.parametrize("kw,word", [
    (dict(logits=None), "null"), (dict(tok=None), "null"), (dict(pos=None), "null"),
    (dict(theta=0.0), "repetition_penalty"), (dict(theta=-1.0), "repetition_penalty"),
    (dict(theta=float("nan")), "repetition_penalty"), (dict(theta=float("inf")), "repetition_penalty"),
    (dict(n=-1), "no_repeat_ngram"), (dict(ml=-1), "min_length"), (dict(n_suppress=-1), "n_suppress"),
    (dict(ld=15), "ld"), (dict(group=0), "group"), (dict(group=3, anc=_A, ld_anc=8), "groups"),
    (dict(n_suppress=2, suppress=None), "suppress"),
])
def test_rejects(kw, word):
    assert _call(**kw) == 1                                        # MIT_ERR_INVALID
    assert word.encode() in N.lib().mit_last_error()


def test_empty_batch_is_a_no_op_and_rejections_are_not_recorded():
    assert _call(R=0) == 0                                         # nothing launched: no GPU needed
    lib = N.lib()
    lib.mit_plan_begin()
    assert _call(theta=0.0) == 1 and _call(logits=None) == 1
    plan = lib.mit_plan_end()
    try:
        assert lib.mit_plan_size(plan) == 0
    finally:
        lib.mit_plan_destroy(plan)


def test_binding_matches_the_header():
    assert callable(N.logits_constrain)
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decl = re.search(r"int\s+mit_logits_constrain\s*\(([^)]*)\)", src).group(1)
    params = [p.strip() for p in decl.split(",")]
    res, args = N.SIGNATURES["mit_logits_constrain"]
    assert res is ctypes.c_int and len(args) == len(params) == 20
    for p, a in zip(params, args):
        want = ctypes.c_void_p if "*" in p else {"long": ctypes.c_long, "float": ctypes.c_float,
                                                  "int64_t": ctypes.c_int64}[p.split()[0]]
        assert a is want, (p, a)
    assert N.ABI_VERSION == 9


# ------------------------------------------------------------------------------------------------
# 3. DecodeConstraints, decode_options, the parser
# ------------------------------------------------------------------------------------------------
def test_decode_constraints_value():
    from decoder import DecodeConstraints as DC
    d = DC()
    assert (d.repetition_penalty, d.no_repeat_ngram, d.min_length, d.suppress, d.prompts) == (1.0, 0, 0, (), None)
    assert not d.active() and not DC(prompts=[]).active() and not DC(prompts=[[], []]).active()
    for kw in (dict(repetition_penalty=1.2), dict(no_repeat_ngram=2), dict(min_length=1), dict(suppress=[3]),
               dict(prompts=[4, 5]), dict(prompts=[[], [4]])):
        assert DC(**kw).active(), kw
    assert DC(prompts=[4, 5]).image_prompts(3) == [[4, 5]] * 3
    assert DC(prompts=[[4], [], [5, 6]]).image_prompts(3) == [[4], [], [5, 6]]
    assert DC(prompts=[[4], [], [5, 6]]).rows(1, 3).prompts == [[], [5, 6]]
    assert DC(prompts=[4, 5], suppress=(1,)).rows(1, 3).prompts == [4, 5]
    DC(1.3, 3, 4, (0, 1), [[7, 8], [9]]).validate(V=10, max_len=3, end_id=5, B=2)
    for kw, word in [(dict(repetition_penalty=0.0), "repetition_penalty"),
                     (dict(repetition_penalty=float("inf")), "repetition_penalty"),
                     (dict(no_repeat_ngram=-1), "no_repeat_ngram"), (dict(min_length=-2), "min_length"),
                     (dict(suppress=[10]), "suppress"), (dict(suppress=[-1]), "suppress"),
                     (dict(prompts=[10]), "prompt"), (dict(prompts=[[1], [-1]]), "prompt"),
                     (dict(prompts=[1, 5]), "END"), (dict(prompts=[1, 2, 3]), "max_len"),
                     (dict(prompts=[[1], [2], [3]]), "images")]:
        with pytest.raises(ValueError, match=word):
            DC(**kw).validate(V=10, max_len=3, end_id=5, B=2)


class _Stub:
    device = "cpu"

    def __init__(self):
        self.calls = []

    def generate_batch(self, chunk, start, end, **kw):
        self.calls.append(("greedy", chunk.shape[0], kw))
        return [[start, 7, end]] * chunk.shape[0]

    def generate_beam_batch(self, chunk, start, end, **kw):
        self.calls.append(("beam", chunk.shape[0], kw))
        return [[start, 8, end]] * chunk.shape[0]

    def generate_sample_batch(self, chunk, start, end, **kw):
        self.calls.append(("sample", chunk.shape[0], kw))
        return [[start, 9, end]] * chunk.shape[0]


def test_command_line_round_trip():
    import inference
    ap = inference.build_parser()
    base = ["--image_path", "a.png", "--checkpoint_path", "c.pt"]
    o = inference.decode_options(ap.parse_args(base))
    assert not {"repetition_penalty", "no_repeat_ngram_size", "min_length", "suppress_tokens", "prompts"} & set(o)
    flags = ["--repetition_penalty", "1.2", "--no_repeat_ngram_size", "3", "--min_length", "5", "--suppress_tokens",
             "0", "1", "3", "--prompt_ids", "11", "12"]
    want = dict(repetition_penalty=1.2, no_repeat_ngram_size=3, min_length=5, suppress_tokens=(0, 1, 3), prompts=[11, 12])
    for extra, kind in (([], "greedy"), (["--beam_size", "3"], "beam"), (["--temperature", "0.8"], "sample")):
        o = inference.decode_options(ap.parse_args(base + flags + extra))
        assert {k: o[k] for k in want} == want
        m = _Stub()
        out = inference.generate_captions(m, torch.zeros(3, 3, 4, 4), start_token_id=2, end_token_id=3, max_len=9, **o)
        assert len(out) == 3 and [k for k, _, _ in m.calls] == [kind]
        assert {k: m.calls[0][2][k] for k in want} == want


def test_generate_captions_cuts_per_image_prompts_with_the_batches():
    import inference
    m = _Stub()
    prompts = [[10], [11, 12], [], [13], [14]]
    inference.generate_captions(m, torch.zeros(5, 3, 4, 4), start_token_id=2, end_token_id=3, max_len=9, batch_size=2,
                                prompts=prompts, min_length=4)
    assert [kw["prompts"] for _, _, kw in m.calls] == [prompts[0:2], prompts[2:4], prompts[4:5]]
    assert all(kw["min_length"] == 4 and "repetition_penalty" not in kw for _, _, kw in m.calls)
    m = _Stub()
    inference.generate_captions(m, torch.zeros(2, 3, 4, 4), start_token_id=2, end_token_id=3, max_len=9)
    assert not {"repetition_penalty", "no_repeat_ngram_size", "min_length", "suppress_tokens", "prompts"} & \
        set(m.calls[0][2])                                         # defaults: today's call, keyword for keyword


# ------------------------------------------------------------------------------------------------
# 4. the end-to-end inputs are decided
# ------------------------------------------------------------------------------------------------
def test_oracle_trajectories_are_decided():
    """tiny_vit_patches, 4 images, START 2, END 69, max_len 12: the constrained greedy decode over the CPU oracle. In
    every setting every free step's top-1 / top-2 margin after the constraints exceeds 2 TAU = 2e-3 (no step is left
    out), and every setting changes at least one image's ids against the unconstrained run. Measured smallest margins:
    off 2.57e-2, n2 2.57e-2, theta1.3 2.57e-2, minlen8 4.69e-3, combined (with the prompts e2e_settings keeps: two tokens for every image) 1.51e-2."""
    res = cc.e2e_settings(FX)
    off = [r["ids"] for r in res["off"][1]]
    assert len(off) == 4
    for name, (kw, rows) in res.items():
        ms = [m for r in rows for m in r["margins"]]
        changed = [b for b, r in enumerate(rows) if r["ids"] != off[b]]
        print(f"{name}: smallest margin {min(ms):.3e} over {len(ms)} free steps; images changed {changed}; "
              f"ids {[r['ids'] for r in rows]}; prompts {kw.get('prompts')}")
        assert min(ms) > 2 * cc.TAU, f"{name}: a step is decided by only {min(ms):.3e}"
        for r in rows:
            assert r["ids"][0] == cc.E2E_START and len(r["ids"]) <= cc.E2E_MAX_LEN
        if name != "off":
            assert changed, f"{name} changes no image's ids"
    kw, rows = res["combined"]
    assert sum(1 for p in kw["prompts"] if p) >= 2, kw["prompts"]
    for p, r in zip(kw["prompts"], rows):
        ids = r["ids"]
        assert ids[1:1 + len(p)] == p and cc.E2E_END not in p
        body = ids[:-1] if ids[-1] == cc.E2E_END else ids
        free = body[1 + len(p):]
        assert not set(free) & {0, 1, 2, 3}, ids                                  # suppressed
        assert cc.E2E_END not in ids[1:7], ids                                    # min_length 6: END from column 7 on
        tri = [tuple(body[i:i + 3]) for i in range(len(body) - 2)]
        assert len(tri) == len(set(tri)), ids                                     # no trigram twice (n = 3)
    # min_length = 8 alone: END first in column 9
    for r in res["minlen8"][1]:
        assert cc.E2E_END not in r["ids"][1:9]
    for r in res["n2"][1]:
        body = r["ids"][:-1] if r["ids"][-1] == cc.E2E_END else r["ids"]
        bi = list(zip(body, body[1:]))
        assert len(bi) == len(set(bi)), r["ids"]
