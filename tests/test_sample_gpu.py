"""Sampling on the GPU (csrc/sample.hip and the decode built on it), against tests/sample_contract.py:
mit_sample_pick case by case (exact picks / state / guards, logprob within beam_contract.BOUND_SCORE, a second launch
bitwise), mit_sample_uniform bitwise against the restated hash, the hash-driven pick's frequencies, the fp32 sampled
decode step by step against the pinned oracle's logits, and the bf16 decode against the model's own teacher-forced
forward."""
import math

import numpy as np
import pytest
import torch

import beam_contract as bc
import fixtures as FX
import native as N
import sample_contract as sc
from model_util import build_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
_MODELS = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    N.load_library()
    yield
    _MODELS.clear()
    torch.cuda.empty_cache()


def _model(name, dtype):
    if (name, dtype) not in _MODELS:
        meta, _ = FX.load(name)
        _MODELS[(name, dtype)] = (build_model(meta, dtype)[0], meta)
    return _MODELS[(name, dtype)]


def _seed_t(seed):
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    return torch.tensor([s - (1 << 64) if s >= (1 << 63) else s], dtype=torch.int64, device=DEV)


# ------------------------------------------------------------------------------------------------
# mit_sample_pick
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c.id for c in sc.PICK_CASES])
def test_pick(cid):
    """Tokens, finished, length, the n_finished increment, pos and ticket: exact (every float margin of the case is
    at least 2 TAU_U = 2.06e-4 of probability mass). logprob within BOUND_SCORE = 11.4 units of u (|logprob_in| +
    |logit| + |lse|); measured worst over the cases: 0.557 (pick-u0-V7). Guards (NaN ld padding, NaN rows of finished rows, ids columns other than p + 1, the state of
    finished rows): bitwise untouched. A second launch from restored inputs: bitwise the same."""
    c = sc.PICK_BY_ID[cid]
    t = sc.make_pick(c).to(DEV)
    t.snapshot()
    assert sc.launch_pick(N, c, t) == 0, N.lib().mit_last_error()
    torch.cuda.synchronize()
    fig = sc.check_pick(c, t)
    print(f"{cid}: logprob figure {fig:.3f} (bound {bc.BOUND_SCORE:.2f})")
    assert fig <= bc.BOUND_SCORE, f"{cid}: logprob off by {fig:.2f} units (bound {bc.BOUND_SCORE:.2f})"
    first = {k: a.bits().cpu().clone() for k, a in t.a.items()}
    t.restore()
    assert sc.launch_pick(N, c, t) == 0
    torch.cuda.synchronize()
    for k, a in t.a.items():
        assert torch.equal(a.bits().cpu(), first[k]), f"{cid}: {k} differs between two launches"


def test_uniform_export():
    """mit_sample_uniform is the header's rule bit for bit (seeds at and above 2^32, several row0 and positions),
    and mit_sample_pick without `uniforms` picks what it picks with the export supplied."""
    R = 300
    out = torch.empty(R, dtype=torch.float32, device=DEV)
    for seed in (None, 0, 1, 12345, 1 << 32, (1 << 32) + 1, (1 << 63) + 7, (1 << 64) - 1):
        for row0 in (0, 7, 1 << 20):
            for p in (0, 1, 99):
                pos = torch.tensor([p], dtype=torch.int64, device=DEV)
                N.sample_uniform(R, row0, None if seed is None else _seed_t(seed), pos, out)
                want = sc.uniform_reference(seed, row0, R, p)
                assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32)), (seed, row0, p)
    V, R, row0, p = 509, 64, 11, 4
    g = torch.Generator().manual_seed(3)
    logits = (torch.randn(R, V, generator=g) * 3).to(DEV)
    seed = _seed_t((1 << 40) + 9)
    picks = []
    for use_export in (False, True):
        ids = torch.zeros(R, 8, dtype=torch.int64, device=DEV)
        pos = torch.tensor([p], dtype=torch.int64, device=DEV)
        fin = torch.zeros(R, dtype=torch.int32, device=DEV)
        nf = torch.zeros(1, dtype=torch.int32, device=DEV)
        ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
        u = None
        if use_export:
            u = torch.empty(R, dtype=torch.float32, device=DEV)
            N.sample_uniform(R, row0, seed, pos, u)
        N.sample_pick(logits, V, 0.9, 40, 0.95, None if use_export else seed, row0, u, ids, pos, -1, 0, fin, nf, None,
                      None, ticket)
        torch.cuda.synchronize()
        assert int(pos) == p + 1 and int(ticket) == 0
        picks.append(ids[:, p + 1].cpu())
    assert torch.equal(picks[0], picks[1]) and len(set(picks[0].tolist())) > 8


@pytest.mark.parametrize("top_k", [0, 3])
def test_frequencies(top_k):
    """V = 7, one logits row repeated over 4096 rows, drawn with the hash at T = 1.3: every row's pick is
    pick_reference at that row's exported u, except rows within 2 TAU_U of a boundary (at most 0.5 % of the rows;
    12 TAU_U = 0.12 % expected; measured 8 and 3 of 4096); the empirical frequencies lie within 5 standard errors of
    the probabilities (measured worst: 2.5)."""
    V, R, T, p, row0 = 7, 4096, 1.3, 17, 5
    row = torch.tensor([1.5, -0.25, 0.75, 2.0, -1.0, 0.5, 1.25])
    logits = row.repeat(R, 1).contiguous().to(DEV)
    seed = _seed_t(2024)
    pos = torch.tensor([p], dtype=torch.int64, device=DEV)
    u = torch.empty(R, dtype=torch.float32, device=DEV)
    N.sample_uniform(R, row0, seed, pos, u)
    ids = torch.zeros(R, p + 3, dtype=torch.int64, device=DEV)
    fin = torch.zeros(R, dtype=torch.int32, device=DEV)
    nf = torch.zeros(1, dtype=torch.int32, device=DEV)
    ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
    lp = torch.zeros(R, dtype=torch.float32, device=DEV)
    N.sample_pick(logits, V, T, top_k, 1.0, seed, row0, None, ids, pos, -1, 0, fin, nf, lp, None, ticket)
    torch.cuda.synchronize()
    got = ids[:, p + 1].cpu().tolist()
    us = u.cpu().numpy()
    assert np.array_equal(us, sc.uniform_reference(2024, row0, R, p))
    left_out = 0
    for r in range(R):
        ref = sc.pick_reference(row, T, top_k, 1.0, float(us[r]))
        if ref["margin_u"] < 2 * sc.TAU_U:
            left_out += 1
            continue
        assert got[r] == ref["token"], f"row {r}: u = {us[r]!r} picked {got[r]}, reference {ref['token']}"
    assert left_out <= 0.005 * R, f"{left_out} rows within 2 TAU_U of a boundary"
    ref = sc.pick_reference(row, T, top_k, 1.0, 0.5)
    prob = np.zeros(V)
    prob[ref["tokens"]] = ref["probs"]
    freq = np.bincount(np.array(got), minlength=V) / R
    se = np.sqrt(prob * (1 - prob) / R)
    print(f"top_k {top_k}: {left_out} rows left out; frequencies {freq.round(4).tolist()} for {prob.round(4).tolist()}")
    assert (np.abs(freq - prob) <= 5 * se).all(), (freq, prob, se)
    lsm = torch.log_softmax(row.double(), 0)
    assert torch.allclose(lp.cpu().double(), lsm[torch.tensor(got)], atol=1e-5)


def test_steps_advance_pos_once_each():
    """Three picks in a row on one state (the second and third recorded as a launch plan and replayed): pos 0 -> 3,
    each column written once with the hash's pick at that position, logprob and length accumulated."""
    R, V, L, T, top_k, top_p, row0 = 7, 509, 8, 0.8, 20, 0.9, 3
    logits_c = torch.randn(R, V, generator=torch.Generator().manual_seed(5)) * 4
    for seed in range(64):       # a seed whose three draws are decided for every row (found on the CPU)
        refs = [[sc.pick_reference(logits_c[r], T, top_k, top_p, float(sc.uniform_reference(seed, row0 + r, 1, p)[0]))
                 for r in range(R)] for p in range(3)]
        if all(min(x["margin_u"], x["margin_p"]) >= 2 * sc.TAU_U for step in refs for x in step):
            break
    else:
        raise AssertionError("no decided seed")
    logits = logits_c.to(DEV)
    ids = torch.full((R, L), 7, dtype=torch.int64, device=DEV)
    pos = torch.zeros(1, dtype=torch.int64, device=DEV)
    fin = torch.zeros(R, dtype=torch.int32, device=DEV)
    nf = torch.zeros(1, dtype=torch.int32, device=DEV)
    ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
    lp = torch.zeros(R, dtype=torch.float32, device=DEV)
    length = torch.zeros(R, dtype=torch.int32, device=DEV)
    st = _seed_t(seed)

    def step():
        N.sample_pick(logits, V, T, top_k, top_p, st, row0, None, ids, pos, -1, 0, fin, nf, lp, length, ticket)
    step()
    prog = N.record(step)
    prog.run()
    torch.cuda.synchronize()
    assert int(pos) == 3 and int(ticket) == 0 and int(nf) == 0
    want = torch.full((R, L), 7, dtype=torch.int64)
    for p in range(3):
        want[:, p + 1] = torch.tensor([x["token"] for x in refs[p]])
    assert torch.equal(ids.cpu(), want)
    assert (length.cpu() == 3).all()
    want_lp = torch.tensor([sum(refs[p][r]["logit"] - refs[p][r]["lse"] for p in range(3)) for r in range(R)])
    assert (lp.cpu().double() - want_lp).abs().max() < 1e-4


# ------------------------------------------------------------------------------------------------
# end to end, fp32
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny_vit_cls", "tiny_clip336_patches"])
def test_top_k_1_is_generate_batch(name):
    m, meta = _model(name, torch.float32)
    img = FX.inputs(meta, 0)[0]
    imgs = torch.cat([img, img.flip(-1), img * 0.5])
    for end in (3, -1):
        greedy = m.generate_batch(imgs, 2, end, max_len=14)
        for seed in (0, 99):
            out = m.generate_sample_batch(imgs, 2, end, max_len=14, temperature=0.7, top_k=1, seed=seed,
                                          return_logprob=True)
            assert [o[0][0] for o in out] == greedy
            assert all(math.isfinite(o[0][1]) and o[0][1] < 0 for o in out)
        assert m.generate_sample_batch(imgs, 2, end, max_len=14, temperature=0.7, top_k=1, seed=5) == greedy


def test_sampled_steps_are_the_oracles():
    """tiny_vit_patches (procedural weights), 4 images, max_len 12, top_k = 3, T = 0.5, the committed seed: for every
    produced sequence one teacher-forced oracle forward; at each step the produced token is pick_reference of the
    oracle's logits at u(seed, row, p), except steps a logit error of TAU = 1e-3 could flip (at most 10 % of them; the
    oracle's own trajectory has under 5 %, tests/test_sample_contract_cpu.py; measured: 0 of 27 left out); logprob
    within steps x 1e-3."""
    m, meta = _model(sc.E2E_FIXTURE, torch.float32)
    imgs = sc.e2e_images(FX)
    out = m.generate_sample_batch(imgs, sc.E2E_START, sc.E2E_END, max_len=sc.E2E_MAX_LEN, temperature=sc.E2E_T,
                                  top_k=sc.E2E_TOP_K, seed=sc.E2E_SEED, return_logprob=True)
    steps = left_out = 0
    for b, ((ids, lp),) in enumerate(out):
        assert ids[0] == sc.E2E_START and 2 <= len(ids) <= sc.E2E_MAX_LEN
        assert sc.E2E_END not in ids[1:-1] and (ids[-1] == sc.E2E_END or len(ids) == sc.E2E_MAX_LEN)
        refs, lsm = sc.oracle_steps(FX, ids, b, sc.E2E_SEED)
        for p, ref in enumerate(refs):
            steps += 1
            if sc.undecided(ref, sc.E2E_T):
                left_out += 1
            else:
                assert ids[p + 1] == ref["token"], f"image {b} step {p}: {ids[p + 1]} != {ref['token']} ({ids})"
        want_lp = float(sum(lsm[p, ids[p + 1]] for p in range(len(ids) - 1)))    # of the PRODUCED tokens
        assert abs(lp - want_lp) <= (len(ids) - 1) * 1e-3, f"image {b}: logprob {lp} against the oracle's {want_lp}"
    print(f"{left_out} of {steps} steps undecided")
    assert left_out <= 0.10 * steps
    one = m.generate_sample(imgs[2], sc.E2E_START, sc.E2E_END, max_len=sc.E2E_MAX_LEN, temperature=sc.E2E_T,
                            top_k=sc.E2E_TOP_K, seed=sc.E2E_SEED, image_offset=2)
    assert one == out[2][0][0]


def test_batch_cut_and_launch_modes(monkeypatch):
    """5 images x 3 samples decoded together; each image alone with image_offset = b gives the same ids;
    generate_captions gives the same ids at batch_size 2 and 5; plan, graph and eager launches agree bitwise;
    different seeds differ somewhere, the same seed twice does not. A SampleState's cross-attention K/V holds one
    memory per image."""
    import inference
    m, meta = _model(sc.E2E_FIXTURE, torch.float32)
    img = FX.inputs(meta, 0)[0]
    imgs = torch.cat([img, img.flip(-1), img * 0.5])[:5]
    assert imgs.shape[0] == 5
    kw = dict(max_len=14, temperature=0.9, top_k=20, top_p=0.95, seed=7)
    runs = {}
    for mode in ("eager", "plan", "graph"):
        monkeypatch.setenv("MIT_DECODE_LAUNCH", mode)
        runs[mode] = m.generate_sample_batch(imgs, 2, 69, num_samples=3, use_graph=mode != "eager", check_every=4, **kw)
    assert runs["eager"] == runs["plan"] == runs["graph"]
    assert m.generate_sample_batch(imgs, 2, 69, num_samples=3, **kw) == runs["plan"]
    both = runs["plan"]
    assert len(both) == 5 and all(len(x) == 3 for x in both)
    for b in range(5):
        alone = m.generate_sample_batch(imgs[b:b + 1], 2, 69, num_samples=3, image_offset=b, **kw)[0]
        assert [i for i, _ in alone] == [i for i, _ in both[b]], b
        assert all(abs(x - y) < 1e-4 for (_, x), (_, y) in zip(alone, both[b]))
    other = m.generate_sample_batch(imgs, 2, 69, num_samples=3, **dict(kw, seed=8))
    assert any(a[0] != b[0] for x, y in zip(other, both) for a, b in zip(x, y))
    assert any(len({tuple(i) for i, _ in x}) > 1 for x in both), "the samples of an image never differ"
    cap = {bs: inference.generate_captions(m, imgs, start_token_id=2, end_token_id=69, max_len=14, batch_size=bs,
                                           temperature=0.9, top_k=20, top_p=0.95, seed=7) for bs in (2, 5)}
    assert cap[2] == cap[5]
    single = m.generate_sample_batch(imgs, 2, 69, **kw)
    assert [p for p, _ in cap[5]] == [inference.postprocess_ids(s, 2, 69) for s in single]


def test_samples_share_the_image_memory():
    """N = 3: the state's K/V has images * S rows (not rows * S) and sample n of image b is the N = 1 decode of that
    image at global row b * 3 + n"""
    m, meta = _model(sc.E2E_FIXTURE, torch.float32)
    imgs = sc.e2e_images(FX)[:2]
    m.eval()
    mem, mem_ld, S, _, _ = m._encode_memory(imgs.to(m.device).float())
    stt = m.decoder.sample_begin(mem, mem_ld, S, 2, 3, 10, 2, 69, temperature=0.8, top_k=10, seed=3)
    assert stt.kv.shape[1] == 2 * S and stt.B == 6 and stt.group == 3 and stt.K == 0
    assert stt.logprob.shape == (6,) and stt.length.dtype == torch.int32 and int(stt.ticket) == 0
    for _ in range(9):
        m.decoder.sample_step(stt)
    rows = stt.token_lists()
    assert int(stt.pos) == 9 and int(stt.ticket) == 0
    for b in range(2):
        for n in range(3):
            one = m.generate_sample_batch(imgs[b:b + 1], 2, 69, max_len=10, temperature=0.8, top_k=10, seed=3,
                                          image_offset=b * 3 + n)[0]
            assert one == rows[b * 3 + n], (b, n)


# ------------------------------------------------------------------------------------------------
# end to end, bf16: self-consistency with the model's own teacher-forced forward
# ------------------------------------------------------------------------------------------------
# the bf16 noise floor of "decode step vs full forward" per generated token and the images it was measured on:
# tests/test_beam_gpu.py (profiles/beam_bench.txt)
from test_beam_gpu import BF16_STEP_DEV, _bf16_images  # noqa: E402


@pytest.mark.parametrize("name", list(BF16_STEP_DEV))
def test_bf16_logprob_is_the_models_own(name):
    """Every row's logprob is the sum over its tokens of log_softmax of the model's teacher-forced full forward on
    the sampled ids, within 2 x BF16_STEP_DEV per generated token (measured worst: 6.7e-3 / 3.5e-3 / 9.4e-3 per token
    against bounds of 2.96e-2 / 3.54e-2 / 3.40e-2); nothing follows a row's first END.
    cfg1_gen_cls: B = 86, 3 samples -> R = 258 rows, V = 10000, d = 512, max_len 32."""
    m, meta = _model(name, torch.bfloat16)
    imgs, L = _bf16_images(name, meta)
    imgs = imgs.to(DEV)
    Ns, start = 3, 2
    B = imgs.shape[0]
    greedy = torch.tensor(m.generate_batch(imgs, start, -1, max_len=L))[:, 2:]
    end = int(torch.mode(greedy.flatten()).values)
    m.eval()
    mem, mem_ld, S, _, _ = m._encode_memory(imgs.float())
    stt = m.decoder.sample_begin(mem, mem_ld, S, B, Ns, L, start, end, temperature=1.0, top_k=50, top_p=0.95, seed=1)
    assert stt.kv.shape[1] == B * S
    for _ in range(L - 1):
        m.decoder.sample_step(stt)
    ids = stt.ids
    lp, length, fin = stt.logprob.cpu().double(), stt.length.cpu(), stt.finished.cpu()
    assert int(fin.sum()) > 0 and int(fin.sum()) == int(stt.n_finished)
    with torch.no_grad():
        lsm = torch.log_softmax(m(imgs.repeat_interleave(Ns, 0), ids[:, :-1].contiguous()).float(), -1)
        tokp = lsm.gather(-1, ids[:, 1:, None]).squeeze(-1).double().cpu()
    ids_c = ids.cpu()
    worst = 0.0
    for r in range(B * Ns):
        n = int(length[r])
        row = ids_c[r].tolist()
        if fin[r]:
            assert row[n] == end and end not in row[1:n] and all(x == 0 for x in row[n + 1:]), (r, row)
        else:
            assert n == L - 1 and end not in row[1:], (r, row)
        want = float(tokp[r, :n].sum())
        err = abs(float(lp[r]) - want) / n
        worst = max(worst, err)
        assert err <= 2 * BF16_STEP_DEV[name], f"row {r}: logprob {float(lp[r]):.4f}, teacher-forced {want:.4f} " \
                                               f"over {n} tokens ({err:.3e} per token)"
    print(f"{name}: worst |logprob - teacher-forced| per token {worst:.3e} (bound {2 * BF16_STEP_DEV[name]:.3e}), "
          f"{int(fin.sum())} of {B * Ns} rows finished, END {end}")
    assert len({tuple(r) for r in ids_c.tolist()}) > B, "the samples of an image never differ"
