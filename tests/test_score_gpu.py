"""Caption scoring at the model level (ImageToTextModel.score_captions / score_tokens, TransformerDecoder.run_score,
inference.score_captions, train.evaluate_metrics) on the tiny ViT fixtures: B = 2 images, C = 3 ragged candidates
drawn with a fixed seed.

The yardstick is code that was there before: model.forward on the images repeated C times, then log_softmax and a
gather on the host in float64. (The fixtures pin logits, not the decoder's memory, so oracle.ref_cpu.decoder_forward
has nothing to start from here; model.forward is itself pinned to the reference by tests/test_model_gpu.py.)"""
import pytest
import torch

import fixtures as FX
import native as N
from model_util import build_model

pytestmark = pytest.mark.gpu
NAMES = ["tiny_vit_cls", "tiny_vit_patches"]
START, END, PAD = 1, 2, 0
B, C = 2, 3
_MODELS = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    N.load_library()
    yield
    _MODELS.clear()
    _REF.clear()
    torch.cuda.empty_cache()


def _model(name, dtype):
    if (name, dtype) not in _MODELS:
        meta, _ = FX.load(name)
        m = build_model(meta, dtype)[0]
        m.eval()
        _MODELS[(name, dtype)] = (m, meta)
    return _MODELS[(name, dtype)]


def _images(meta):
    return FX.inputs(meta, 0)[0][:B].contiguous()


LENGTHS = [[9, 4, 6], [3, 7, 5]]   # ragged; with START the longest gives T = 10 decoder positions (7 does not divide it)


def _candidates(meta, seed=5):
    """B lists of C id lists of LENGTHS ids drawn from [3, V): no START / END / PAD inside"""
    g = torch.Generator().manual_seed(seed)
    V = meta["dec"]["vocab"]
    return [[torch.randint(3, V, (n,), generator=g).tolist() for n in img] for img in LENGTHS]


def _padded(cands, extra=0):
    """[B, C, L] START .. END sequences padded with PAD (+ `extra` PAD columns)"""
    seqs = [[START] + c + [END] for img in cands for c in img]
    L = max(len(s) for s in seqs) + extra
    out = torch.full((len(seqs), L), PAD, dtype=torch.int64)
    for i, s in enumerate(seqs):
        out[i, :len(s)] = torch.tensor(s)
    return out.view(len(cands), len(cands[0]), L)


def _replicated(m, images, seq):
    """The existing path: forward on the images repeated C times, then float64 log_softmax and gather on the host.
    Returns per position [B, C, T]: target log-probability (0 at PAD targets), scored mask, argmax == target, and the
    top-2 logit margin."""
    b, c, L = seq.shape
    tokens, targets = seq[:, :, :-1].reshape(b * c, L - 1), seq[:, :, 1:]
    with torch.no_grad():
        logits = m.forward(images.repeat_interleave(c, 0), tokens).double().cpu().view(b, c, L - 1, -1)
    lsm = torch.log_softmax(logits, -1)
    mask = targets != PAD
    lp = lsm.gather(-1, targets.unsqueeze(-1)).squeeze(-1) * mask
    top = logits.topk(2, -1).values
    return lp, mask, logits.argmax(-1) == targets, top[..., 0] - top[..., 1]


_REF = {}


def _ref(name, dtype):
    """the replicated forward of the fixture's candidates, computed once per (fixture, dtype)"""
    if (name, dtype) not in _REF:
        m, meta = _model(name, dtype)
        _REF[(name, dtype)] = _replicated(m, _images(meta), _padded(_candidates(meta)))
    return _REF[(name, dtype)]


@pytest.mark.parametrize("name", NAMES)
def test_fp32_matches_the_replicated_forward(name):
    """logprob within tokens x 1e-3 (the per-logit tolerance of test_forward_fp32_matches_reference), tokens exact,
    the per-position rank-0 flag exact wherever the top-2 margin exceeds 1e-4, hits = the rank-0 positions"""
    m, meta = _model(name, torch.float32)
    lp, n, hits, tlp, rank = m.score_captions(_images(meta), _candidates(meta), START, END, return_tokens=True)
    ref_lp, mask, ref_hit, margin = _ref(name, torch.float32)
    assert lp.dtype == torch.float32 and n.dtype == torch.int32 and hits.dtype == torch.int32 and lp.is_cuda
    assert tuple(lp.shape) == (B, C) and tuple(tlp.shape) == tuple(mask.shape) == tuple(rank.shape)
    assert torch.equal(n.cpu().long(), mask.sum(-1))
    err = (lp.cpu().double() - ref_lp.sum(-1)).abs()
    print(f"{name}: fp32 logprob err {err.max():.2e} (bound {float(n.min()) * 1e-3:.1e} .. {float(n.max()) * 1e-3:.1e}), "
          f"per token {(tlp.cpu().double() - ref_lp).abs().max():.2e}")
    assert (err <= n.cpu().double() * 1e-3).all()
    assert torch.equal((rank.cpu() >= 0), mask) and (tlp.cpu()[~mask] == 0).all()
    safe = mask & (margin > 1e-4)
    assert safe.sum() >= 0.9 * mask.sum()
    assert torch.equal((rank.cpu() == 0)[safe], ref_hit[safe])
    assert torch.equal(hits.cpu().long(), (rank.cpu() == 0).sum(-1))


@pytest.mark.parametrize("name", NAMES)
def test_bf16_within_twice_the_bf16_forward_distance(name):
    """the worst per-token |score - replicated bf16 forward| is at most 2 x the worst per-token distance between the
    replicated bf16 forward and the fp32 forward (both measured here, on the same inputs): scoring and the bf16
    forward are one bf16 rounding of the same quantity apart. Measured: see DESIGN.md 5.1f."""
    m, meta = _model(name, torch.bfloat16)
    lp, n, hits, tlp, rank = m.score_captions(_images(meta), _candidates(meta), START, END, return_tokens=True)
    ref16, mask, _, _ = _ref(name, torch.bfloat16)
    ref32 = _ref(name, torch.float32)[0]
    dist = float((ref16 - ref32).abs().max())
    err = float((tlp.cpu().double() - ref16).abs().max())
    print(f"{name}: bf16 per-token |score - bf16 forward| {err:.3e}, |bf16 forward - fp32 forward| {dist:.3e}")
    assert err <= 2 * dist
    assert torch.equal(n.cpu().long(), mask.sum(-1)) and torch.equal(hits.cpu().long(), (rank.cpu() == 0).sum(-1))
    assert (lp.cpu().double() - tlp.cpu().double().sum(-1)).abs().max() < 1e-4


@pytest.mark.parametrize("name,dtype", [(NAMES[0], torch.bfloat16), (NAMES[1], torch.bfloat16), (NAMES[1], torch.float32)])
def test_invariants(name, dtype):
    """bitwise on logprob: head_rows 1 / 7 (no multiple of T) / default; a permutation of the candidates permutes
    the outputs; trailing PAD columns change nothing; the tensor form is the list form. One candidate alone agrees
    with its row of the C = 3 call within the bf16 bound (another cross-attention shape, another T)."""
    m, meta = _model(name, dtype)
    images, cands = _images(meta), _candidates(meta)
    base = m.score_captions(images, cands, START, END, return_tokens=True)
    T = base[3].shape[-1]
    assert 7 % T and m.decoder.default_head_rows(B * C * T) == B * C * T
    for hr in (1, 7):
        got = m.score_captions(images, cands, START, END, return_tokens=True, head_rows=hr)
        for a, b in zip(base, got):
            assert torch.equal(a, b), f"head_rows {hr}"
    perm = [2, 0, 1]
    got = m.score_captions(images, [[img[i] for i in perm] for img in cands], START, END)
    for a, b in zip(base[:3], got):
        assert torch.equal(a[:, perm], b)
    for extra in (0, 3):
        got = m.score_captions(images, _padded(cands, extra), START, END, return_tokens=True)
        assert got[3].shape[-1] == T + extra
        for a, b in zip(base[:3], got[:3]):
            assert torch.equal(a, b), f"{extra} extra PAD columns"
        assert torch.equal(got[3][..., :T], base[3]) and (got[4][..., T:] == -1).all()
    # bare ids, ids with START, ids with START and END: one candidate
    full = [[[START] + c + [END] for c in img] for img in cands]
    half = [[[START] + c for c in img] for img in cands]
    for form in (full, half):
        assert torch.equal(m.score_captions(images, form, START, END)[0], base[0])
    # a flat list scores the same candidates against every image
    flat = m.score_captions(images, cands[0], START, END)
    assert torch.equal(flat[0][0], base[0][0]) and tuple(flat[0].shape) == (B, C)
    ref16, ref32 = _ref(name, torch.bfloat16)[0], _ref(name, torch.float32)[0]
    bound = 2 * float((ref16 - ref32).abs().max())
    for c in range(C):
        one = m.score_captions(images, [[img[c]] for img in cands], START, END, return_tokens=True)
        t1 = one[3].shape[-1]
        assert torch.equal(one[1][:, 0], base[1][:, c])
        assert float((one[3][:, 0] - base[3][:, c, :t1]).abs().max()) <= bound, c


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_inference_ranking_and_batching(dtype):
    """the order is rank_beams' rule on the model's own (logprob, tokens); batch_size 1 and 2 give the same result.
    fp32: the same bits (every fp32 kernel computes a row the same way at any row count). bf16: the same order and
    token counts, and log-probabilities within the bf16 bound of the tests above -- the bf16 GEMM dispatch goes by
    the row count (197 encoder rows of one image run the register-streaming kernel, 394 rows of two the 128-tile
    kernel, with another summation order), so an image's features, and model.forward's logits with them, move in
    their last bf16 bits with the batch the image is in; scoring inherits exactly that."""
    import inference
    from model import rank_beams
    m, meta = _model(NAMES[1], dtype)
    images, cands = _images(meta), _candidates(meta)
    lp, n, _ = m.score_captions(images, cands, START, END)
    kw = dict(start_token_id=START, end_token_id=END)
    bound = 2 * float((_ref(NAMES[1], torch.bfloat16)[0] - _ref(NAMES[1], torch.float32)[0]).abs().max())
    for pen in (0.0, 1.0):
        both = inference.score_captions(m, images, cands, batch_size=2, length_penalty=pen, **kw)
        ones = inference.score_captions(m, images, cands, batch_size=1, length_penalty=pen, **kw)
        if dtype == torch.float32:
            assert both == ones
        else:
            worst = max(abs(x[1] - y[1]) / x[2] for a, b in zip(both, ones) for x, y in zip(a, b))
            print(f"tiny_vit_patches: bf16 batch_size 1 vs 2: worst |logprob difference| per token {worst:.3e} "
                  f"(bound {bound:.3e})")
            assert [[(r[0], r[2]) for r in rows] for rows in both] == [[(r[0], r[2]) for r in rows] for rows in ones]
            assert worst <= bound
        for b, rows in enumerate(both):
            want = rank_beams([[c] for c in range(C)], lp[b].tolist(), n[b].tolist(), C, pen, return_all=True)[0]
            assert [r[0] for r in rows] == [ids[0] for ids, _ in want]
            for c, l_, n_, s in rows:
                assert l_ == float(lp[b, c]) and n_ == int(n[b, c]) and s == l_ / n_ ** pen
    if dtype == torch.float32:
        flat = inference.score_captions(m, images, cands[0], batch_size=1, **kw)
        assert flat[0] == inference.score_captions(m, images, cands, **kw)[0]


def test_evaluate_metrics_is_the_token_weighted_eval_loss():
    """two batches with different numbers of non-PAD targets: loss = the token-weighted mean of eval_loss over the
    same batches within 1e-3 (the fp32 tolerance per token), perplexity = exp(loss), accuracy from the ranks"""
    import math
    import train
    m, meta = _model(NAMES[1], torch.float32)
    imgs, dec_in, tgt = FX.inputs(meta, 0)
    batches = [dict(images=imgs[i:i + 2], decoder_input_tokens=dec_in[i:i + 2], target_tokens=tgt[i:i + 2])
               for i in (0, 2)]
    counts = [int((b["target_tokens"] != PAD).sum()) for b in batches]
    assert counts[0] != counts[1]
    losses = [float(m.eval_loss(b["images"], b["decoder_input_tokens"], b["target_tokens"])) for b in batches]
    want = sum(l_ * c for l_, c in zip(losses, counts)) / sum(counts)
    was = m.training
    got = train.evaluate_metrics(m, batches)
    assert m.training == was
    print(f"evaluate_metrics {got}, token-weighted eval_loss {want:.6f}, per-batch mean {sum(losses) / 2:.6f}")
    assert got["tokens"] == sum(counts) and abs(got["loss"] - want) <= 1e-3
    assert abs(got["perplexity"] - math.exp(got["loss"])) <= 1e-9 * got["perplexity"]
    hits = sum(int(m.score_tokens(b["images"].to(m.device), b["decoder_input_tokens"], b["target_tokens"])[2].sum())
               for b in batches)
    assert got["token_accuracy"] == hits / sum(counts) and 0 <= got["token_accuracy"] <= 1


def test_rejections_raise_before_any_launch():
    m, meta = _model(NAMES[0], torch.bfloat16)
    images, cands = _images(meta), _candidates(meta)
    V, gen = meta["dec"]["vocab"], m._gen
    bad = [
        [[[5, 6], [], [7]]] * B,                                  # an empty candidate
        [[[5, 6], [V], [7]]] * B,                                 # an id past the vocabulary
        [[[5, 6], [-1], [7]]] * B,
        [[[5, 6], [7]], [[5, 6], [7], [8]]],                      # unequal candidate counts
        [cands[0]] * (B + 1),                                     # a list per image, one list too many
        [[[5] * (m.decoder.max_seq_len + 1)]] * B,                # more positions than max_seq_len
        [],
        torch.zeros(B, C, dtype=torch.int64),                     # not [B, C, L]
        torch.zeros(B, C, 4, dtype=torch.int64),                  # all PAD: empty candidates
    ]
    for caps in bad:
        with pytest.raises(ValueError):
            m.score_captions(images, caps, START, END)
    with pytest.raises(ValueError):
        m.score_captions(images, cands, START, END, head_rows=0)
    with pytest.raises(ValueError):
        m.score_tokens(images.to(m.device), torch.ones(B + 1, 4, dtype=torch.int64), torch.ones(B + 1, 4, dtype=torch.int64))
    assert m._gen == gen, "a rejected call reached the encoder"
    m.score_captions(images, cands, START, END)
    assert m._gen == gen + 1
