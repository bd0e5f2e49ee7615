"""Beam search on the GPU (csrc/beam.hip and the decode built on it), against tests/beam_contract.py:
mit_beam_select case by case (exact picks / state / ancestry / guards, scores within BOUND_SCORE, a second launch
bitwise), mit_attention_decode_beam against the float64 gathered attention within decode_contract.BOUND["attn"] (and
bitwise against mit_attention_decode where the two run the same arithmetic), the fp32 beam decode step by step against
the textbook algorithm over the pinned oracle, and the bf16 beam decode against the model's own teacher-forced forward."""
import pytest
import torch

import beam_contract as bc
import decode_contract as dc
import fixtures as FX
import native as N
from model_util import build_model

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    N.load_library()
    yield
    _MODELS.clear()          # the module's models (cfg1 among them) do not stay on the device for later modules
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------
# mit_beam_select
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c.id for c in bc.SEL_CASES])
def test_select(cid):
    """Picks, parents, finished / length / n_finished / pos, tok column p + 1, the permuted ancestor rows: exact.
    Guards (NaN ld padding, NaN rows of finished slots, tok / anc columns past p + 1): bitwise untouched. Scores
    within BOUND_SCORE = 11.4 units of u (|score| + |logit| + |lse|); measured worst over the cases: 0.249
    (sel-mix-V10000-K1-B5). A second launch on the same inputs: bitwise the same outputs."""
    c = bc.SEL_BY_ID[cid]
    t = bc.make_select(c).to(DEV)
    nws = N.beam_select_ws_bytes(c.B, c.K, c.V)
    ws = torch.full((nws // 8 + 2,), -1, dtype=torch.int64, device=DEV)      # all-ones: NaN (score, token) pairs
    t.snapshot()
    assert bc.launch_select(N, c, t, ws[:nws // 8]) == 0, N.lib().mit_last_error()
    torch.cuda.synchronize()
    fig = bc.check_select(c, t)
    print(f"{cid}: score figure {fig:.3f} (bound {bc.BOUND_SCORE:.2f}), margin {t.x['ref']['margin']:.3e}")
    assert fig <= bc.BOUND_SCORE, f"{cid}: score off by {fig:.2f} units (bound {bc.BOUND_SCORE:.2f})"
    assert (ws[nws // 8:] == -1).all(), "workspace written past mit_beam_select_ws_bytes"
    first = {k: a.bits().cpu().clone() for k, a in t.a.items()}
    t.restore()
    ws.fill_(-1)
    assert bc.launch_select(N, c, t, ws[:nws // 8]) == 0
    torch.cuda.synchronize()
    for k, a in t.a.items():
        assert torch.equal(a.bits().cpu(), first[k]), f"{cid}: {k} differs between two launches"


def test_select_steps_advance_pos_once_each():
    """Three selections in a row on one state (recorded as a launch plan and replayed): pos 0 -> 3, every step's
    column written, the start state handled (only slot 0 finite)."""
    B, K, V, T = 3, 3, 509, 8
    g = torch.Generator().manual_seed(5)
    score = torch.full((B, K), float("-inf"))
    score[:, 0] = 0
    score = score.view(-1).to(DEV)
    tok = torch.full((B * K, T), 7, dtype=torch.int64, device=DEV)
    anc = torch.zeros(B * K, T, dtype=torch.int32, device=DEV)
    anc[:, 0] = torch.arange(K, dtype=torch.int32).repeat(B)
    pos = torch.zeros(1, dtype=torch.int64, device=DEV)
    fin = torch.zeros(B * K, dtype=torch.int32, device=DEV)
    length = torch.zeros(B * K, dtype=torch.int32, device=DEV)
    nf = torch.zeros(1, dtype=torch.int32, device=DEV)
    ws = torch.empty(N.beam_select_ws_bytes(B, K, V) // 8, dtype=torch.int64, device=DEV)
    logits = (torch.randn(B * K, V, generator=g) * 3).to(DEV)
    ref = dict(score=score.cpu().double(), finished=fin.cpu(), length=length.cpu(), tok=tok.cpu(), anc=anc.cpu())

    def step():
        N.beam_select(logits, V, score, tok, anc, pos, 1, 0, fin, length, nf, ws, B, K)
    step()
    prog = N.record(step)
    prog.run()
    torch.cuda.synchronize()
    for p in range(3):
        ref = bc.select_reference(logits.cpu(), ref["score"], ref["finished"], ref["length"], ref["tok"], ref["anc"], p,
                                  K, 1, 0)
        assert ref["margin"] > bc.TAU
    assert int(pos) == 3
    assert torch.equal(tok.cpu(), ref["tok"]) and torch.equal(anc.cpu(), ref["anc"])
    assert torch.equal(fin.cpu(), ref["finished"]) and torch.equal(length.cpu(), ref["length"])
    assert int(nf) == ref["n_finished"]
    assert (score.cpu().double() - ref["score"]).abs().max() < 1e-4


# ------------------------------------------------------------------------------------------------
# mit_attention_decode_beam
# ------------------------------------------------------------------------------------------------
SHAPES = {"f32-192": (torch.float32, 3, 64), "bf16-512": (torch.bfloat16, 8, 64), "f32-dh16": (torch.float32, 12, 16)}
PAD = 0


def _attn_case(shape, Lk, group, seed, images=5):
    """Slot-ordered cache [R, Lmax, 2d] with a random ancestor table (repeats included): K / V rows at j > pos and
    in slots no row of the image references are NaN; anc at j > pos is poison; PAD tokens sit only in rows a
    DIFFERENT slot reads through the table (its own row's token is live)."""
    dtype, H, Dh = SHAPES[shape]
    d, R, Lmax = H * Dh, images * group, Lk + 5
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(R, 3 * d, generator=g)
    cache = torch.randn(R, Lmax, 2 * d, generator=g)
    anc = torch.randint(0, group, (R, Lmax), generator=g, dtype=torch.int32)
    tok = torch.randint(1, 50, (R, Lmax), generator=g)
    idx = bc.gather_index(R, Lk, group, anc)
    used = torch.zeros(R, Lmax, dtype=torch.bool)
    used[idx, torch.arange(Lk)[None, :].expand(R, Lk)] = True
    cache[~used] = float("nan")                 # j > pos, and slots nobody descends from
    if Lk > 2 and group > 1:
        for r in range(0, R, 2):                # a PAD that row r reaches only through its ancestor's row
            j = 1 + r % (Lk - 1)
            src = int(idx[r, j])
            if src != r:
                tok[src, j] = PAD
    anc[:, Lk:] = torch.tensor([10 ** 6, -7, 1 << 30, -(1 << 31), 99], dtype=torch.int32)[:Lmax - Lk]
    return dict(dtype=dtype, H=H, Dh=Dh, d=d, R=R, Lmax=Lmax, Lk=Lk, group=group, qkv=qkv.to(DEV, dtype),
                cache=cache.to(DEV, dtype), anc=anc.to(DEV), tok=tok.to(DEV),
                pos=torch.tensor([Lk - 1], dtype=torch.int64, device=DEV), idx=idx)


def _run_gathered(a, anc=True):
    d, R, Lmax = a["d"], a["R"], a["Lmax"]
    o = torch.full((R, d + 8), dc.SENTINEL, dtype=a["dtype"], device=DEV)
    cache = a["cache"]
    N.attention_decode_beam(a["qkv"], 3 * d, cache, 2 * d, Lmax * 2 * d, cache[:, :, d:], 2 * d, Lmax * 2 * d, o, d + 8,
                            R, a["H"], pos=a["pos"], group=a["group"], anc=a["anc"] if anc else None,
                            key_tokens=a["tok"], tok_batch=Lmax, pad_idx=PAD, scale=a["Dh"] ** -0.5, Dh=a["Dh"])
    torch.cuda.synchronize()
    assert (o[:, d:] == dc.SENTINEL).all(), "columns past H * Dh of o written"
    return o[:, :d]


def _check_attn(name, got, ref, unit, dtype):
    figs = []
    dc.check_float(name, "attn", got.cpu(), ref, unit, dtype == torch.bfloat16, figs)
    fig = figs[0][2] if figs else 0.0
    print(f"{name}: figure {fig:.3f} (bound {dc.BOUND['attn']:.3f})")
    assert fig <= dc.BOUND["attn"], f"{name}: {fig:.3f} units > {dc.BOUND['attn']:.3f}"


@pytest.mark.parametrize("group", [1, 3, 4])
@pytest.mark.parametrize("Lk", [1, 7, 33, 64, 197])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_attention_gathered(shape, Lk, group):
    """Self-attention through the ancestor table against the float64 gathered reference (measured worst figure:
    0.352 units, attn-f32-dh16-Lk7-g3; bound 2.596), inputs untouched, and -- where mit_attention_decode_plan reports the same family
    for physically gathered operands -- bitwise mit_attention_decode on them."""
    a = _attn_case(shape, Lk, group, seed=1000 * Lk + group)
    before = {k: a[k].clone() for k in ("qkv", "cache", "anc", "tok", "pos")}
    got = _run_gathered(a)
    for k, v in before.items():
        assert torch.equal(a[k].view(torch.uint8), v.view(torch.uint8)), f"input {k} written"
    d, R, H, Dh, Lmax = a["d"], a["R"], a["H"], a["Dh"], a["Lmax"]
    cache = a["cache"].cpu().float()
    k4 = cache[:, :, :d].reshape(R, Lmax, H, Dh)
    v4 = cache[:, :, d:].reshape(R, Lmax, H, Dh)
    q = a["qkv"][:, :d].cpu().float().view(R, H, Dh)
    ref, unit = bc.gathered_attention(q, k4, v4, Lk, group, a["anc"].cpu(), a["tok"].cpu(), PAD, Dh ** -0.5)
    assert not torch.isnan(ref).any(), "the case masks every key of a row"
    _check_attn(f"attn-{shape}-Lk{Lk}-g{group}", got, ref, unit, a["dtype"])
    # the same keys physically gathered, through mit_attention_decode
    j = torch.arange(Lk)[None, :].expand(R, Lk)
    phys = torch.zeros_like(a["cache"])
    phys[:, :Lk] = a["cache"][a["idx"].to(DEV), j.to(DEV)]
    ptok = torch.full_like(a["tok"], 3)
    ptok[:, :Lk] = a["tok"][a["idx"].to(DEV), j.to(DEV)]
    code = N.dtype_code(a["qkv"])
    o2 = torch.empty(R, d, dtype=a["dtype"], device=DEV)
    fam = N.attention_decode_plan(code, R, H, Dh, a["qkv"].data_ptr(), 3 * d, phys.data_ptr(), 2 * d, Lmax * 2 * d,
                                  phys[:, :, d:].data_ptr(), 2 * d, Lmax * 2 * d, o2.data_ptr(), d,
                                  pos=a["pos"].data_ptr(), key_tokens=ptok.data_ptr())
    mine = N.attention_decode_beam_plan(code, R, H, Dh, a["qkv"].data_ptr(), 3 * d, a["cache"].data_ptr(), 2 * d,
                                        Lmax * 2 * d, a["cache"][:, :, d:].data_ptr(), 2 * d, Lmax * 2 * d,
                                        o2.data_ptr(), d, pos=a["pos"].data_ptr(), group=group,
                                        anc=a["anc"].data_ptr(), ld_anc=Lmax, key_tokens=a["tok"].data_ptr())
    assert mine == dc.ATTN_BH and fam == (dc.ATTN_ROWS if shape == "bf16-512" else dc.ATTN_BH)
    if fam == mine:
        N.attention_decode(a["qkv"], 3 * d, phys, 2 * d, Lmax * 2 * d, phys[:, :, d:], 2 * d, Lmax * 2 * d, o2, d, R, H,
                           pos=a["pos"], key_tokens=ptok, tok_batch=Lmax, pad_idx=PAD, scale=Dh ** -0.5, Dh=Dh)
        torch.cuda.synchronize()
        assert torch.equal(got.contiguous().view(torch.uint8), o2.view(torch.uint8)), \
            "gathered call differs bitwise from mit_attention_decode on gathered operands"


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("Lk", [7, 197])
def test_attention_group1_is_attention_decode(shape, Lk):
    """group = 1 without a table: bitwise mit_attention_decode (whatever family that launches)"""
    a = _attn_case(shape, Lk, 1, seed=Lk)
    a["cache"] = torch.nan_to_num(a["cache"], nan=0.5)
    a["tok"][1, 0] = PAD
    got = _run_gathered(a, anc=False)
    d, R, Lmax = a["d"], a["R"], a["Lmax"]
    o2 = torch.empty(R, d, dtype=a["dtype"], device=DEV)
    N.attention_decode(a["qkv"], 3 * d, a["cache"], 2 * d, Lmax * 2 * d, a["cache"][:, :, d:], 2 * d, Lmax * 2 * d, o2, d,
                       R, a["H"], pos=a["pos"], key_tokens=a["tok"], tok_batch=Lmax, pad_idx=PAD, scale=a["Dh"] ** -0.5,
                       Dh=a["Dh"])
    torch.cuda.synchronize()
    assert torch.equal(got.contiguous().view(torch.uint8), o2.view(torch.uint8))


@pytest.mark.parametrize("group", [3, 4])
@pytest.mark.parametrize("S", [1, 197])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_attention_shared_cross(shape, S, group):
    """The `group` beams of an image read ONE cross-attention K / V [images, S, 2d] at a fixed Lk: against float64
    (measured worst figure: 0.167 units, cross-f32-dh16-S197-g4), and against mit_attention_decode on the K / V replicated per row."""
    dtype, H, Dh = SHAPES[shape]
    d, images = H * Dh, 5
    R = images * group
    g = torch.Generator().manual_seed(S + group)
    q = torch.randn(R, d, generator=g).to(DEV, dtype)
    kv = torch.randn(images, S + 2, 2 * d, generator=g)
    kv[:, S:] = float("nan")                      # rows at j >= Lk are never read
    kv = kv.to(DEV, dtype)
    o = torch.empty(R, d, dtype=dtype, device=DEV)
    rb = (S + 2) * 2 * d
    N.attention_decode_beam(q, d, kv, 2 * d, rb, kv[:, :, d:], 2 * d, rb, o, d, R, H, Lk=S, group=group,
                            scale=Dh ** -0.5, Dh=Dh)
    torch.cuda.synchronize()
    c = kv.cpu().float()
    ref, unit = bc.gathered_attention(q.cpu().float().view(R, H, Dh), c[:, :, :d].reshape(images, S + 2, H, Dh),
                                      c[:, :, d:].reshape(images, S + 2, H, Dh), S, group, None, None, PAD, Dh ** -0.5)
    _check_attn(f"cross-{shape}-S{S}-g{group}", o, ref, unit, dtype)
    if shape != "bf16-512":   # the same family (block per (row, head)): bitwise on replicated K / V
        rep = kv.repeat_interleave(group, 0).contiguous()
        o2 = torch.empty_like(o)
        N.attention_decode(q, d, rep, 2 * d, rb, rep[:, :, d:], 2 * d, rb, o2, d, R, H, Lk=S, scale=Dh ** -0.5, Dh=Dh)
        torch.cuda.synchronize()
        assert torch.equal(o.view(torch.uint8), o2.view(torch.uint8))


# ------------------------------------------------------------------------------------------------
# end to end, fp32: the textbook algorithm over the pinned oracle, step by step
# ------------------------------------------------------------------------------------------------
_MODELS = {}


def _model(name, dtype):
    if (name, dtype) not in _MODELS:
        meta, _ = FX.load(name)
        _MODELS[(name, dtype)] = (build_model(meta, dtype)[0], meta)
    return _MODELS[(name, dtype)]


def _begin(m, imgs, K, max_len, start, end):
    m.eval()
    mem, mem_ld, S, _, _ = m._encode_memory(imgs.to(m.device).float())
    return m.decoder.beam_begin(mem, mem_ld, S, imgs.shape[0], K, max_len, start, end)


@pytest.mark.parametrize("K,end", bc.E2E_CASES)
def test_beam_fp32_every_step_equals_the_reference(K, end):
    """tiny_vit_patches (procedural weights), 4 images decoded together: after EVERY step, for every image and slot,
    the ids, finished and length equal the reference's (whose every decision margin is > 1e-3, checked on the CPU)
    and the scores are within steps x 1e-3; the final ranking and cut of generate_beam_batch equal the reference's."""
    m, meta = _model(bc.E2E_FIXTURE, torch.float32)
    imgs = bc.e2e_images(FX)
    refs = bc.e2e_reference(FX, K, end)
    L = bc.E2E_MAX_LEN
    stt = _begin(m, imgs, K, L, bc.E2E_START, end)
    worst = 0.0
    for s in range(L - 1):
        m.decoder.beam_step(stt)
        ids = stt.beam_ids().cpu()
        sc, fin, ln = stt.score.cpu().view(-1, K), stt.finished.cpu().view(-1, K), stt.length.cpu().view(-1, K)
        assert int(stt.pos) == s + 1
        for b, ref in enumerate(refs):
            st = ref["steps"][min(s, len(ref["steps"]) - 1)]
            extra = s - min(s, len(ref["steps"]) - 1)      # the image finished earlier: its beams only gain PADs
            want = [row + [0] * extra for row in st["ids"]]
            assert ids[b, :, :s + 2].tolist() == want, f"step {s} image {b}: {ids[b, :, :s + 2].tolist()} != {want}"
            assert fin[b].tolist() == st["finished"] and ln[b].tolist() == st["length"], (s, b)
            err = max(abs(float(sc[b, k]) - st["score"][k]) for k in range(K))
            worst = max(worst, err / (s + 1))
            assert err <= (s + 1) * 1e-3, f"step {s} image {b}: score off by {err:.2e}"
        assert int(stt.n_finished) == int(fin.sum())
    print(f"K={K} END={end}: worst score error per step {worst:.2e}")
    out = m.generate_beam_batch(imgs, bc.E2E_START, end, max_len=L, beam_size=K, return_all=True)
    best = m.generate_beam_batch(imgs, bc.E2E_START, end, max_len=L, beam_size=K)
    for b, ref in enumerate(refs):
        order = bc.rank_slots(ref["score"], ref["length"])
        assert [i for i, _ in out[b]] == [ref["ids"][k] for k in order]
        assert all(abs(s - ref["score"][k]) <= L * 1e-3 for (_, s), k in zip(out[b], order))
        assert best[b] == ref["ids"][order[0]]
    one = m.generate_beam(imgs[1], bc.E2E_START, end, max_len=L, beam_size=K)
    assert one == best[1]


@pytest.mark.parametrize("name", ["tiny_vit_cls", "tiny_clip336_patches"])
def test_one_beam_is_generate_batch(name):
    m, meta = _model(name, torch.float32)
    img = FX.inputs(meta, 0)[0]
    imgs = torch.cat([img, img.flip(-1), img * 0.5])
    for end in (3, -1):
        assert m.generate_beam_batch(imgs, 2, end, max_len=14, beam_size=1) == m.generate_batch(imgs, 2, end, max_len=14)


def test_batch_of_five_equals_each_alone_and_launch_modes_agree(monkeypatch):
    """5 images decoded together give each image's own result (ids exactly; scores to rounding: the GEMMs may tile
    R = 15 and R = 3 rows differently); launch plan, hipGraph and eager launches of one batch agree bitwise."""
    m, meta = _model(bc.E2E_FIXTURE, torch.float32)
    img = FX.inputs(meta, 0)[0]
    imgs = torch.cat([img, img.flip(-1), img * 0.5])[:5]
    assert imgs.shape[0] == 5
    runs = {}
    for mode in ("eager", "plan", "graph"):
        monkeypatch.setenv("MIT_DECODE_LAUNCH", mode)
        runs[mode] = m.generate_beam_batch(imgs, 2, 69, max_len=16, beam_size=3, return_all=True,
                                           use_graph=mode != "eager", check_every=4)
    assert runs["eager"] == runs["plan"] == runs["graph"]
    for b in range(5):
        alone = m.generate_beam_batch(imgs[b:b + 1], 2, 69, max_len=16, beam_size=3, return_all=True)[0]
        assert [i for i, _ in alone] == [i for i, _ in runs["plan"][b]], b
        assert all(abs(x - y) < 1e-4 for (_, x), (_, y) in zip(alone, runs["plan"][b]))


# ------------------------------------------------------------------------------------------------
# end to end, bf16: self-consistency with the model's own teacher-forced forward
# ------------------------------------------------------------------------------------------------
# Worst per-step |log_softmax(decode logits)[token] - log_softmax(full forward logits)[token]| of the UNFUSED greedy
# decode (MIT_DECODE_FUSED=0, stt.logits) of the commit before beam search, on the same images and max_len (measured
# once, tools/beam_bench.py --deviation; profiles/beam_bench.txt): the bf16 noise floor of "decode step vs full
# forward". A beam's score may differ from the teacher-forced sum by 2 x that per generated token (the factor covers
# the head GEMM's other tile choice at R rows); wrong ancestry or a wrong reorder misses by whole nats.
BF16_STEP_DEV = {"tiny_vit_patches": 1.478e-2, "tiny_vit_v509": 1.772e-2, "cfg1_gen_cls": 1.700e-2}


def _bf16_images(name, meta):
    if name == "cfg1_gen_cls":
        import procedural as P
        imgs = P.make_images(meta["n_images"], meta["image_size"], meta["image_seed"])
        rest = P.make_images(86 - meta["n_images"], meta["image_size"], meta["image_seed"] + 1000)
        return torch.cat([imgs, rest]), 32
    img = FX.inputs(meta, 0)[0]
    return torch.cat([img, img.flip(-1), img * 0.5]), 20


@pytest.mark.parametrize("name", list(BF16_STEP_DEV))
def test_beam_bf16_scores_are_the_models_own(name):
    """Every returned beam's score is the sum over its tokens of log_softmax of the model's teacher-forced full
    forward on that beam's ids, within 2 x BF16_STEP_DEV per generated token (measured worst: 7.3e-3 / 9.8e-3 / 1.37e-2 per token against
    bounds of 2.96e-2 / 3.54e-2 / 3.40e-2); nothing follows a beam's first END.
    cfg1_gen_cls: B = 86, K = 3 -> R = 258 rows (a GEMM row tail), V = 10000, d = 512, max_len 32."""
    m, meta = _model(name, torch.bfloat16)
    imgs, L = _bf16_images(name, meta)
    imgs = imgs.to(DEV)
    K, start = 3, 2
    B = imgs.shape[0]
    # an END the model does produce now and then (the most frequent non-first greedy token), so finished beams
    # take part; found from one greedy pass
    greedy = torch.tensor(m.generate_batch(imgs, start, -1, max_len=L))[:, 2:]
    end = int(torch.mode(greedy.flatten()).values)
    stt = _begin(m, imgs, K, L, start, end)
    for _ in range(L - 1):
        m.decoder.beam_step(stt)
    ids = stt.beam_ids().view(B * K, L)
    score, length, fin = stt.score.cpu().double(), stt.length.cpu(), stt.finished.cpu()
    assert int(fin.sum()) > 0 and int(fin.sum()) == int(stt.n_finished)
    with torch.no_grad():
        tf_in = ids[:, :-1].contiguous()
        lsm = torch.log_softmax(m(imgs.repeat_interleave(K, 0), tf_in).float(), -1)       # [R, L-1, V]
        tokp = lsm.gather(-1, ids[:, 1:, None]).squeeze(-1).double().cpu()                 # [R, L-1]
    ids_c = ids.cpu()
    worst = 0.0
    for r in range(B * K):
        n = int(length[r])
        row = ids_c[r].tolist()
        if fin[r]:
            assert row[n] == end and end not in row[1:n] and all(x == 0 for x in row[n + 1:]), (r, row)
        else:
            assert n == L - 1 and end not in row[1:], (r, row)
        want = float(tokp[r, :n].sum())
        err = abs(float(score[r]) - want) / n
        worst = max(worst, err)
        assert err <= 2 * BF16_STEP_DEV[name], f"row {r}: score {float(score[r]):.4f}, teacher-forced {want:.4f} " \
                                               f"over {n} tokens ({err:.3e} per token)"
    print(f"{name}: worst |score - teacher-forced| per token {worst:.3e} (bound {2 * BF16_STEP_DEV[name]:.3e}), "
          f"{int(fin.sum())} of {B * K} beams finished, END {end}")
    out = m.generate_beam_batch(imgs, start, end, max_len=L, beam_size=K, return_all=True)
    sc = score.view(B, K)
    for b in range(B):
        assert all(abs(x - y) < 1e-3 for (_, x), y in zip(out[b], sorted(sc[b].tolist(), reverse=True)))


# ------------------------------------------------------------------------------------------------
# public surface
# ------------------------------------------------------------------------------------------------
def test_generate_captions_beam_and_greedy():
    import inference
    m, meta = _model("tiny_vit_cls", torch.float32)
    img = FX.inputs(meta, 0)[0]
    imgs = torch.cat([img, img.flip(-1)])
    dec = lambda ids: " ".join(f"t{i}" for i in ids)  # noqa: E731
    kw = dict(decode=dec, start_token_id=2, end_token_id=3, max_len=12)
    greedy = inference.generate_captions(m, imgs, **kw)
    want = [inference.postprocess_ids(s, 2, 3) for s in m.generate_batch(imgs, 2, 3, max_len=12)]
    assert [p for p, _ in greedy] == want and inference.generate_captions(m, imgs, beam_size=None, **kw) == greedy
    for bs in (256, 1):
        got = inference.generate_captions(m, imgs, beam_size=3, batch_size=bs, **kw)
        beams = m.generate_beam_batch(imgs, 2, 3, max_len=12, beam_size=3)
        assert len(got) == len(beams)
        for (p, text), b in zip(got, beams):
            w = inference.postprocess_ids(b, 2, 3)
            assert p == w and text == inference.clean_text(dec(w))
    lp = inference.generate_captions(m, imgs, beam_size=3, length_penalty=1.0, **kw)
    assert [p for p, _ in lp] == [inference.postprocess_ids(b, 2, 3)
                                  for b in m.generate_beam_batch(imgs, 2, 3, max_len=12, beam_size=3, length_penalty=1.0)]
