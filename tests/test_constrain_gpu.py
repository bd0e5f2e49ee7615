"""Constrained decoding on the GPU (csrc/constrain.hip and the decodes built on it), against
tests/constrain_contract.py: mit_logits_constrain case by case (rows bitwise the reference's, guards bitwise untouched,
a second launch bitwise), the ancestry cases against their physically gathered twins, the fp32 constrained decodes
(greedy, one beam, top_k = 1) against the pinned oracle's trajectories, "off means off", and the exact properties of
the bf16 fused decodes."""
import pytest
import torch

import beam_contract as bc
import constrain_contract as cc
import fixtures as FX
import native as N
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


# ------------------------------------------------------------------------------------------------
# 5. mit_logits_constrain
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c.id for c in cc.CASES])
def test_constrain(cid):
    """Every live row bitwise the numpy reference's (each changed value is one f32 multiply, -inf or 0.0); the NaN ld
    padding, the NaN rows of finished rows and every input (tok, anc, pos, finished, suppress, forced, with their
    sentinels): bitwise untouched. A second launch from restored inputs: bitwise the same."""
    c = cc.BY_ID[cid]
    t = cc.make_case(c).to(DEV)
    t.snapshot()
    assert cc.launch(N, c, t) == 0, N.lib().mit_last_error()
    torch.cuda.synchronize()
    cc.check_case(c, t)
    first = {k: a.bits().cpu().clone() for k, a in t.a.items()}
    t.restore()
    assert cc.launch(N, c, t) == 0
    torch.cuda.synchronize()
    for k, a in t.a.items():
        assert torch.equal(a.bits().cpu(), first[k]), f"{cid}: {k} differs between two launches"


@pytest.mark.parametrize("cid", [c.id for c in cc.CASES if c.group > 1])
def test_ancestry_equals_gathered_history(cid):
    """The same case with every row's history gathered physically into tok and anc = NULL gives bitwise the same rows"""
    c = cc.BY_ID[cid]
    cpu = cc.make_case(c)
    t = cc.make_case(c).to(DEV)
    g = cc.gathered(c, cpu).to(DEV)
    t.snapshot(), g.snapshot()
    assert cc.launch(N, c, t) == 0 and cc.launch(N, c, g, use_anc=False) == 0, N.lib().mit_last_error()
    torch.cuda.synchronize()
    cc.check_case(c, g)
    assert torch.equal(t.a["logits"].bits().cpu(), g.a["logits"].bits().cpu())


def test_recorded_and_wrapped():
    """native.logits_constrain on tensors, recorded into a launch plan and replayed at a later position: every replay
    reads the device position anew"""
    R, V, L = 3, 64, 8
    g = torch.Generator().manual_seed(1)
    base = torch.randn(R, V, generator=g)
    tok_c = torch.randint(0, 6, (R, L), generator=g)
    logits = base.clone().to(DEV)
    tok = tok_c.to(DEV)
    pos = torch.tensor([2], dtype=torch.int64, device=DEV)
    sup = torch.tensor([7, 8], dtype=torch.int64, device=DEV)
    kw = dict(repetition_penalty=1.3, no_repeat_ngram=2, min_length=4, end_id=9, suppress=sup)
    prog = N.record(lambda: N.logits_constrain(logits, V, tok, pos, **kw))
    assert prog.launches() == 1
    for p in (2, 5):
        logits.copy_(base)
        pos.fill_(p)
        prog.run()
        torch.cuda.synchronize()
        for r in range(R):
            want = cc.constrain_reference(base[r].numpy(), tok_c[r, :p + 1].tolist(), 1.3, 2, 4, 9, (7, 8))
            assert torch.equal(logits[r].cpu().view(torch.int32), torch.from_numpy(want).view(torch.int32)), (p, r)


# ------------------------------------------------------------------------------------------------
# 6. fp32 end to end against the oracle's constrained trajectories
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cc.E2E_SETTINGS))
def test_fp32_decodes_are_the_oracles(name):
    """tiny_vit_patches, 4 images, max_len 12: generate_batch, generate_beam_batch(beam_size=1) and
    generate_sample_batch(top_k=1) all reduce to the constrained argmax, every step of which the oracle decides by
    more than 2 TAU (tests/test_constrain_contract_cpu.py): the ids are exactly the oracle's. The beam score and the
    sample logprob are the float64 sum of log_softmax(constrained oracle row)[token] within steps x TAU (the bound of
    the fp32 beam and sample end-to-end tests, beam_contract.TAU per step; only free steps count, a forced step adds
    exactly 0). Measured worst: 8e-6."""
    m, meta = _model(cc.sc.E2E_FIXTURE, torch.float32)
    imgs = cc.sc.e2e_images(FX)
    kw, rows = cc.e2e_settings(FX)[name]
    want = [r["ids"] for r in rows]
    a = (imgs, cc.E2E_START, cc.E2E_END)
    assert m.generate_batch(*a, max_len=cc.E2E_MAX_LEN, **kw) == want
    beam = m.generate_beam_batch(*a, max_len=cc.E2E_MAX_LEN, beam_size=1, return_all=True, **kw)
    samp = m.generate_sample_batch(*a, max_len=cc.E2E_MAX_LEN, temperature=0.7, top_k=1, seed=3, return_logprob=True,
                                   **kw)
    assert [b[0][0] for b in beam] == want
    assert [s[0][0] for s in samp] == want
    for b, r in enumerate(rows):
        bound = len(r["margins"]) * bc.TAU
        for kind, got in (("beam score", beam[b][0][1]), ("sample logprob", samp[b][0][1])):
            print(f"{name} image {b}: {kind} {got:.6f}, oracle {r['score']:.6f} (bound {bound:.1e})")
            assert abs(got - r["score"]) <= bound, f"{name} image {b}: {kind} {got} against the oracle's {r['score']}"
    if name == "combined":      # the single-image wrappers and a two-group decode take the same arguments
        one = dict(kw, prompts=kw["prompts"][2])
        assert m.generate_beam(imgs[2], cc.E2E_START, cc.E2E_END, max_len=cc.E2E_MAX_LEN, beam_size=1, **one) == want[2]
        assert m.generate_sample(imgs[2], cc.E2E_START, cc.E2E_END, max_len=cc.E2E_MAX_LEN, top_k=1, **one) == want[2]
        assert m.generate_batch(*a, max_len=cc.E2E_MAX_LEN, streams=2, **kw) == want


def test_generate_captions_obeys_the_constraints():
    """inference.generate_captions with the command line's options (decode_options), greedy, --beam_size and
    --temperature alike, cut into batches of 3: every processed caption starts with the prompt, holds no suppressed
    token and no trigram twice, and is at least min_length tokens long (END is cut off by the post-processing)."""
    import inference
    m, meta = _model(cc.sc.E2E_FIXTURE, torch.float32)
    imgs = cc.sc.e2e_images(FX)
    ap = inference.build_parser()
    base = ["--image_path", "a.png", "--checkpoint_path", "c.pt", "--batch_size", "3", "--no_repeat_ngram_size", "3",
            "--min_length", "5", "--suppress_tokens", "0", "1", "3", "439", "--prompt_ids", "27", "162"]
    for extra in ([], ["--beam_size", "3"], ["--temperature", "0.9", "--top_k", "20", "--seed", "2"]):
        o = inference.decode_options(ap.parse_args(base + extra))
        caps = inference.generate_captions(m, imgs, start_token_id=cc.E2E_START, end_token_id=cc.E2E_END, max_len=14,
                                           **o)
        assert len(caps) == 4
        for ids, _ in caps:
            assert ids[:2] == [27, 162] and len(ids) >= 5 and cc.E2E_END not in ids, (extra, ids)
            assert not set(ids[2:]) & {0, 1, 3, 439}, (extra, ids)
            tri = [tuple(([cc.E2E_START] + ids)[i:i + 3]) for i in range(len(ids) - 1)]
            assert len(tri) == len(set(tri)), (extra, ids)


# ------------------------------------------------------------------------------------------------
# 7. off means off
# ------------------------------------------------------------------------------------------------
OFF = dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0, suppress_tokens=(), prompts=None)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_off_means_off(dtype):
    """With default arguments every generate_* returns what it returns without the new keywords, and a recorded step
    has the same number of launches with inactive constraints as without any (the greedy step keeps the head's folded
    argmax); active constraints add exactly the one launch (and on the fused greedy step trade the folded argmax for
    the GEMM, the constraint launch and the pick: one more)."""
    from decoder import DecodeConstraints
    m, meta = _model(cc.sc.E2E_FIXTURE, dtype)
    imgs = cc.sc.e2e_images(FX).to(DEV)
    a = (imgs, cc.E2E_START, cc.E2E_END)
    assert m.generate_batch(*a, max_len=12, **OFF) == m.generate_batch(*a, max_len=12)
    assert m.generate_beam_batch(*a, max_len=12, beam_size=3, return_all=True, **OFF) == \
        m.generate_beam_batch(*a, max_len=12, beam_size=3, return_all=True)
    assert m.generate_sample_batch(*a, max_len=12, temperature=0.9, top_k=20, seed=4, return_logprob=True, **OFF) == \
        m.generate_sample_batch(*a, max_len=12, temperature=0.9, top_k=20, seed=4, return_logprob=True)
    m.eval()
    mem, mem_ld, S, _, _ = m._encode_memory(imgs.float())
    dec = m.decoder
    B = imgs.shape[0]
    on = DecodeConstraints(no_repeat_ngram=2, prompts=[5])
    begins = {
        "greedy": (lambda c: dec.decode_begin(mem, mem_ld, S, B, 12, 2, 69, constraints=c), dec.decode_step),
        "beam": (lambda c: dec.beam_begin(mem, mem_ld, S, B, 3, 12, 2, 69, constraints=c), dec.beam_step),
        "sample": (lambda c: dec.sample_begin(mem, mem_ld, S, B, 2, 12, 2, 69, temperature=0.9, constraints=c),
                   dec.sample_step),
    }
    for kind, (begin, step) in begins.items():
        n = {}
        for label, c in (("none", None), ("inactive", DecodeConstraints()), ("active", on)):
            stt = begin(c)
            assert (stt.cons is None) == (label != "active")
            step(stt)
            n[label] = N.record(lambda: step(stt)).launches()
            torch.cuda.synchronize()
            assert int(stt.pos) == 2
        print(f"{kind} {dtype}: launches per recorded step {n}")
        assert n["inactive"] == n["none"]
        assert n["active"] == n["none"] + 1


# ------------------------------------------------------------------------------------------------
# 8. bf16, fused step: exact properties
# ------------------------------------------------------------------------------------------------
def _violations(ids, prompt, suppress, min_length, end):
    """the properties a constrained sequence must have; returns the names of the violated ones"""
    bad = []
    if ids[1:1 + len(prompt)] != list(prompt):
        bad.append("prompt")
    body = ids[:ids.index(end, 1)] if end in ids[1:] else ids
    if set(body[1 + len(prompt):]) & set(suppress):
        bad.append("suppressed")
    if end in ids[1:min_length + 1]:
        bad.append("early END")
    bi = list(zip(body, body[1:]))
    if len(bi) != len(set(bi)):
        bad.append("repeated bigram")
    return bad


def test_bf16_fused_properties():
    """tiny_vit_patches in bf16 (the fused step), 5 images, max_len 16, n = 2, min_length = 6, suppress {0, 1, 3}, one
    two-token prompt for all images; greedy, beams K = 3 (along each beam's own ids) and sampling (N = 2, T = 1). Every
    returned sequence starts with START and the prompt, holds no suppressed token, no END before column 7 and no
    bigram twice before END. The unconstrained runs violate a property other than the prompt somewhere, or the test
    would show nothing."""
    m, meta = _model(cc.sc.E2E_FIXTURE, torch.bfloat16)
    img = FX.inputs(meta, 0)[0]
    imgs = torch.cat([img, img.flip(-1), img * 0.5])[:5].to(DEV)
    assert imgs.shape[0] == 5
    start, end, L = cc.E2E_START, cc.E2E_END, 16
    prompt, suppress, ml = [27, 162], (0, 1, 3), 6
    kw = dict(no_repeat_ngram_size=2, min_length=ml, suppress_tokens=suppress, prompts=prompt)

    def runs(**k):
        g = m.generate_batch(imgs, start, end, max_len=L, **k)
        b = m.generate_beam_batch(imgs, start, end, max_len=L, beam_size=3, return_all=True, **k)
        s = m.generate_sample_batch(imgs, start, end, max_len=L, temperature=1.0, num_samples=2, seed=11, **k)
        return dict(greedy=g, beam=[ids for img_ in b for ids, _ in img_], sample=[ids for img_ in s for ids, _ in img_])
    con, free = runs(**kw), runs()
    assert m.decoder.decode_begin(*m._encode_memory(imgs.float())[:3], 5, L, start, end).fused
    assert len(con["greedy"]) == 5 and len(con["beam"]) == 15 and len(con["sample"]) == 10
    for kind, seqs in con.items():
        for ids in seqs:
            assert ids[0] == start and 2 <= len(ids) <= L
            assert _violations(ids, prompt, suppress, ml, end) == [], (kind, ids)
    seen = {kind: sorted({v for ids in seqs for v in _violations(ids, [], suppress, ml, end)})
            for kind, seqs in free.items()}
    print(f"unconstrained violations: {seen}")
    assert any(seen.values()), "the unconstrained runs obey every property: the settings constrain nothing here"
    # per-image prompts on the beams: each image's K beams carry its own prompt
    per = [[27], [27, 162], [], [341, 264], [9]]
    out = m.generate_beam_batch(imgs, start, end, max_len=L, beam_size=3, return_all=True, prompts=per, min_length=ml)
    for b, beams in enumerate(out):
        for ids, score in beams:
            assert ids[1:1 + len(per[b])] == per[b] and end not in ids[1:ml + 1], (b, ids)
            assert score == score and score > float("-inf")
