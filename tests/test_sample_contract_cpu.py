"""Sampling without a GPU: the C ABI's argument checks (mit_sample_pick, mit_sample_uniform), the float64 reference
and its float32 emulation on every pick case (margins, TAU_U), the statistics of the counter hash, the oracle's own
sampled trajectory for the committed seed, and the generate_captions / command-line plumbing over a stub model."""
import ctypes

import numpy as np
import pytest
import torch

import fixtures as FX
import native as N
import sample_contract as sc


# ------------------------------------------------------------------------------------------------
# argument checks: before anything is recorded or launched
# ------------------------------------------------------------------------------------------------
def _pick(**kw):
    lib = N.load_library()
    buf = (ctypes.c_double * 64)()
    a = ctypes.addressof(buf)
    d = dict(R=2, V=16, logits=a, ld=16, T=1.0, top_k=0, top_p=1.0, seed=None, row0=0, uniforms=None, ids=a, ld_ids=4,
             pos=a, end=1, pad=0, finished=a, n_finished=a, logprob=None, length=None, ticket=a)
    d.update(kw)
    return lib.mit_sample_pick(d["R"], d["V"], d["logits"], d["ld"], d["T"], d["top_k"], d["top_p"], d["seed"],
                               d["row0"], d["uniforms"], d["ids"], d["ld_ids"], d["pos"], d["end"], d["pad"],
                               d["finished"], d["n_finished"], d["logprob"], d["length"], d["ticket"], None)


@pytest.mark.parametrize("kw,word", [
    (dict(T=0.0), "temperature"), (dict(T=-1.0), "temperature"), (dict(T=float("nan")), "temperature"),
    (dict(top_p=0.0), "top_p"), (dict(top_p=float("nan")), "top_p"), (dict(top_k=-1), "top_k"),
    (dict(V=0), "vocabulary"), (dict(V=1 << 31, ld=1 << 31), "vocabulary"), (dict(ld=15), "ld"),
    (dict(ld_ids=1), "two columns"), (dict(logits=None), "null"), (dict(ids=None), "null"), (dict(pos=None), "null"),
    (dict(finished=None), "null"), (dict(n_finished=None), "null"), (dict(ticket=None), "null"), (dict(R=-1), "row count"),
])
def test_pick_rejects(kw, word):
    assert _pick(**kw) == 1
    assert word.encode() in N.lib().mit_last_error()


def test_pick_rejects_misaligned_logits_and_takes_empty_batches():
    buf = (ctypes.c_double * 64)()
    assert _pick(logits=ctypes.addressof(buf) + 2) == 1 and b"aligned" in N.lib().mit_last_error()
    assert _pick(R=0) == 0          # nothing launched: no GPU needed
    lib = N.lib()
    assert lib.mit_sample_uniform(0, 0, None, ctypes.addressof(buf), ctypes.addressof(buf), None) == 0
    assert lib.mit_sample_uniform(4, 0, None, None, ctypes.addressof(buf), None) == 1
    assert lib.mit_sample_uniform(4, 0, None, ctypes.addressof(buf), None, None) == 1
    assert lib.mit_sample_uniform(-1, 0, None, ctypes.addressof(buf), ctypes.addressof(buf), None) == 1


def test_rejected_calls_are_not_recorded():
    """the checks run before MIT_RECORD: a rejected call leaves a recording plan empty"""
    lib = N.load_library()
    lib.mit_plan_begin()
    assert _pick(T=0.0) == 1
    assert lib.mit_sample_uniform(4, 0, None, None, None, None) == 1
    plan = lib.mit_plan_end()
    try:
        assert lib.mit_plan_size(plan) == 0
    finally:
        lib.mit_plan_destroy(plan)


# ------------------------------------------------------------------------------------------------
# the reference, the emulation, the cases
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    return {c.id: sc.make_pick(c) for c in sc.PICK_CASES}


def test_cases_cover_what_the_contract_names():
    cs = sc.PICK_CASES
    assert {c.V for c in cs} >= set(sc.PICK_V) and {c.R for c in cs} >= set(sc.PICK_R)
    assert {c.T for c in cs} >= set(sc.PICK_T) and {c.top_p for c in cs} >= set(sc.PICK_P)
    for V in sc.PICK_V:
        assert {c.top_k for c in cs if c.V == V} >= {0, 1, 3, 50, V}
    assert {c.kind for c in cs} >= {"mix", "tie", "neginf", "u0", "end", "allfinished"}
    assert any(c.mis and c.ld_pad for c in cs) and any(not c.mis and not c.ld_pad and c.V % 4 == 0 for c in cs)
    assert any(c.V > 12288 for c in cs) and any(c.V == 12288 for c in cs)      # both sides of the LDS row limit
    assert len({c.id for c in cs}) == len(cs)


def test_margins_leave_a_float32_kernel_no_freedom(built):
    """every float margin of every live row of every case is at least 2 TAU_U; a top-k gap is positive or an exact
    tie by construction; finished rows hold NaN logits"""
    assert sc.TAU_U > 0
    for c in sc.PICK_CASES:
        t = built[c.id]
        for r, ref in enumerate(t.x["refs"]):
            if ref is None:
                assert int(t.x["fin0"][r]) and torch.isnan(t.x["logits"][r]).all()
                continue
            assert ref["margin_u"] >= 2 * sc.TAU_U, (c.id, r, ref["margin_u"])
            assert ref["margin_p"] >= 2 * sc.TAU_U, (c.id, r, ref["margin_p"])
            assert ref["margin_k"] > 0 or c.kind == "tie", (c.id, r)
    assert all(r["margin_k"] == 0 for c in sc.PICK_CASES if c.kind == "tie" for r in built[c.id].x["refs"])
    assert any(t.x["fin0"].any() and not t.x["fin0"].all() for t in built.values())
    assert any(float(u) == 0.0 for c in sc.PICK_CASES if c.kind == "u0" for u in built[c.id].x["us"])
    assert any(torch.isinf(built[c.id].x["logits"]).any() for c in sc.PICK_CASES if c.kind == "neginf")
    assert any(r is not None and r["token"] == built[c.id].x["end_id"] for c in sc.PICK_CASES if c.kind == "end"
               for r in built[c.id].x["refs"])


def test_reference_is_sane(built):
    for c in sc.PICK_CASES:
        t = built[c.id]
        for r, ref in enumerate(t.x["refs"]):
            if ref is None:
                continue
            row = t.x["logits"][r]
            k1, k2 = set(ref["K1"].tolist()), set(ref["K2"].tolist())
            assert k2 <= k1 and len(k2) >= 1 and ref["token"] in k2                 # nested, never empty
            assert len(k1) == (c.top_k if 0 < c.top_k < c.V else c.V)
            assert abs(ref["probs"].sum() - 1.0) < 1e-12 and (ref["probs"] >= 0).all()
            assert abs(ref["lse"] - float(torch.logsumexp(row.double(), 0))) < 1e-9
            if c.top_k == 1:
                assert ref["token"] == int(torch.argmax(row)) and len(k2) == 1
            if t.x["top_p"] >= 1.0:
                assert k2 == k1
            else:
                w = np.exp((row.double().numpy() - float(row.max())) / float(np.float32(c.T)))
                mass = w[ref["K2"]].sum() / ref["Z1"]
                assert mass >= t.x["top_p"] > mass - w[ref["K2"][-1]] / ref["Z1"]   # the SHORTEST prefix reaching top_p


def test_emulation_picks_what_float64_picks_and_sets_tau_u():
    """the float32 emulation (both summation orders) picks the float64 token on every case, and TAU_U is 4 x its
    worst running-sum deviation (emulation_figures asserts the picks)"""
    worst = sc.emulation_figures()
    figure = max(f for f, _ in worst.values())
    print({k: (f"{f:.3e}", cid) for k, (f, cid) in worst.items()}, "TAU_U", sc.TAU_U)
    # 5 %: numpy's float32 exp may differ by an ulp between CPU kernels, which moves the summation's rounding
    assert 0.95 * sc.TAU_U <= 4 * figure <= 1.05 * sc.TAU_U, \
        f"TAU_U {sc.TAU_U:.3e} is not 4 x the emulation's worst figure {figure:.3e}"


def test_top_p_and_u_are_taken_at_float32():
    row = torch.tensor([2.0, 1.0, 0.0, -1.0])
    a = sc.pick_reference(row, 0.7, 0, 0.9, 0.3)
    b = sc.pick_reference(row, float(np.float32(0.7)), 0, float(np.float32(0.9)), float(np.float32(0.3)))
    assert a["token"] == b["token"] and a["margin_u"] == b["margin_u"] and a["margin_p"] == b["margin_p"]


# ------------------------------------------------------------------------------------------------
# the hash
# ------------------------------------------------------------------------------------------------
def test_hash_statistics():
    """seeds 0..63, R = 256, p = 0..99: mean, 16-bin chi-square, neighbour correlations, and the words two seeds
    share, counted at the same (row, position): two seeds must not hand a row the same draws. (As SETS of values two
    seeds' 25 600 words can overlap by up to ~100: p enters below bit 7 only, so one pair of rows whose inner words
    agree above it shares a word for every pair of positions -- different rows at different positions, harmless.)
    Measured: mean 0.0041, chi-square 35.0, correlation 0.013, 0 shared."""
    R, P = 256, 100
    words = {}
    worst = dict(mean=0.0, chi2=0.0, corr=0.0, shared=0)
    for seed in range(64):
        h = np.stack([sc.hash_words(seed, 0, R, p) for p in range(P)], 1)          # [R, P]
        u = (h >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
        assert (u >= 0).all() and (u < 1).all()
        worst["mean"] = max(worst["mean"], abs(u.mean() - 0.5))
        cnt = np.bincount((u * 16).astype(int).ravel(), minlength=16)
        e = R * P / 16
        worst["chi2"] = max(worst["chi2"], float(((cnt - e) ** 2 / e).sum()))
        cp = np.corrcoef(u[:, :-1].ravel(), u[:, 1:].ravel())[0, 1]
        cr = np.corrcoef(u[:-1].ravel(), u[1:].ravel())[0, 1]
        worst["corr"] = max(worst["corr"], abs(cp), abs(cr))
        words[seed] = h
    for a in range(64):
        for b in range(a + 1, 64):
            worst["shared"] = max(worst["shared"], int((words[a] == words[b]).sum()))
    print(worst)
    assert worst["mean"] <= 0.01 and worst["chi2"] <= 50 and worst["corr"] <= 0.03 and worst["shared"] <= 4, worst


def test_hash_rows_positions_and_wide_seeds():
    u = sc.uniform_reference(5, 0, 40, 3)
    assert np.array_equal(sc.uniform_reference(5, 7, 33, 3), u[7:])                 # row0 shifts rows
    assert not np.array_equal(sc.uniform_reference(5, 0, 40, 4), u)
    assert np.array_equal(sc.uniform_reference(None, 0, 40, 3), sc.uniform_reference(0, 0, 40, 3))
    for s in (1 << 32, (1 << 32) + 5, (1 << 63) + 5, (1 << 64) - 1):
        assert not np.array_equal(sc.uniform_reference(s, 0, 40, 3), sc.uniform_reference(s & 0xFFFFFFFF, 0, 40, 3))
    assert u.dtype == np.float32
    # seeds 0, 1, 2 do not hand out one stream on permuted rows (the dropout hash's key fold would)
    a, b = sc.hash_words(0, 0, 256, 0), sc.hash_words(1, 0, 256, 0)
    assert np.intersect1d(a, b).size <= 1


# ------------------------------------------------------------------------------------------------
# the oracle's own trajectory for the committed seed
# ------------------------------------------------------------------------------------------------
def test_oracle_trajectory_is_decided():
    """under 5 % of the oracle's own sampled steps for E2E_SEED could flip under a logit error of TAU = 1e-3, so the
    GPU decode (within TAU of the oracle) has room for its 10 %; teacher-forced logits reproduce the trajectory"""
    traj = sc.oracle_trajectory(FX, sc.E2E_SEED)
    share = sc.undecided_share(traj)
    n = sum(len(r) for _, r in traj)
    print(f"seed {sc.E2E_SEED}: {share:.3f} of {n} steps undecided; ids {[i for i, _ in traj]}")
    assert share < 0.05 and n >= 4 * 4
    assert len({tuple(i) for i, _ in traj}) > 1
    ids, refs = traj[1]
    again, lsm = sc.oracle_steps(FX, ids, 1, sc.E2E_SEED)
    assert lsm.shape[0] == len(ids) - 1
    assert [r["token"] for r in again] == ids[1:] == [r["token"] for r in refs]


# ------------------------------------------------------------------------------------------------
# generate_captions / command line over a stub model
# ------------------------------------------------------------------------------------------------
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
        return [[start, 9 + kw["image_offset"] + i, end] for i in range(chunk.shape[0])]


def test_generate_captions_routes_sampling_with_the_chunk_offset():
    import inference
    imgs = torch.zeros(5, 3, 4, 4)
    m = _Stub()
    out = inference.generate_captions(m, imgs, start_token_id=2, end_token_id=3, max_len=6, batch_size=2,
                                      temperature=0.7, top_k=5, top_p=0.9, seed=11)
    assert [p for p, _ in out] == [[9 + i] for i in range(5)]
    assert [(k, n, kw["image_offset"]) for k, n, kw in m.calls] == [("sample", 2, 0), ("sample", 2, 2), ("sample", 1, 4)]
    assert all(kw["temperature"] == 0.7 and kw["top_k"] == 5 and kw["top_p"] == 0.9 and kw["seed"] == 11 and
               kw["max_len"] == 6 for _, _, kw in m.calls)
    m = _Stub()
    inference.generate_captions(m, imgs, start_token_id=2, end_token_id=3, max_len=6)
    inference.generate_captions(m, imgs, start_token_id=2, end_token_id=3, max_len=6, beam_size=3, length_penalty=0.5)
    assert [k for k, _, _ in m.calls] == ["greedy", "beam"] and m.calls[1][2]["length_penalty"] == 0.5
    with pytest.raises(ValueError):
        inference.generate_captions(m, imgs, beam_size=3, temperature=1.0)


def test_command_line_flags():
    import inference
    ap = inference.build_parser()
    base = ["--image_path", "a.png", "--checkpoint_path", "c.pt"]
    o = inference.decode_options(ap.parse_args(base))
    assert o == dict(batch_size=256, beam_size=None, length_penalty=0.0, temperature=None, top_k=0, top_p=1.0, seed=0)
    o = inference.decode_options(ap.parse_args(base + ["--temperature", "0.7", "--top_k", "40", "--top_p", "0.95",
                                                       "--seed", "12", "--batch_size", "8"]))
    assert o == dict(batch_size=8, beam_size=None, length_penalty=0.0, temperature=0.7, top_k=40, top_p=0.95, seed=12)
    o = inference.decode_options(ap.parse_args(base + ["--beam_size", "4", "--length_penalty", "0.6"]))
    assert o["beam_size"] == 4 and o["length_penalty"] == 0.6 and o["temperature"] is None
    with pytest.raises(SystemExit):
        inference.main(base + ["--beam_size", "3", "--temperature", "1.0"])
    m = _Stub()
    inference.generate_captions(m, torch.zeros(2, 3, 4, 4), **o)          # the options are generate_captions keywords
    assert m.calls[0][0] == "beam" and m.calls[0][2]["beam_size"] == 4
