"""Sampled and constrained rolling-batch captioning end to end on the GPU (ImageToTextModel.generate_stream /
generate_stream_iter, inference.generate_captions(stream_slots=...)): EXACTLY the static decoders' results -- the ids
of generate_sample_batch / generate_batch list for list and the sampled log-probabilities bit for bit -- for every
slot count, poll interval, chunking and launch mode, the fused and the unfused bf16 step, fp32, FP8 cross-attention
K/V, per-image caps and per-image prompts. The static decoders are pinned to the oracle by tests/test_sample_gpu.py and
tests/test_constrain_gpu.py; no tolerance appears here.

Every comparison first asserts, through the library's plan queries (stream_contract.gemm_families), that the step and
head GEMMs of both sides take the same kernel family at the compared row counts: the bf16 GEMM family goes by row
count, and equality is promised per family. The same holds in front of the token steps: the encoder, projection and
cross-attention K/V GEMMs go by the rows of an encoder chunk (stream_contract.chunk_families)."""
import os

import pytest
import torch

import fixtures as FX
import native as N
import rolling_contract as rc
import stream_contract as st
from model_util import build_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
START, END, NEVER, MAX_LEN = rc.START, rc.END, rc.NEVER, rc.MAX_LEN
BASE = dict(temperature=0.7, top_k=20, top_p=0.9)
PLAIN = dict(temperature=1.0, top_k=0, top_p=1.0)
_MODELS, _REF = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    N.load_library()
    yield
    _MODELS.clear()
    _REF.clear()
    torch.cuda.empty_cache()


def _model(dtype):
    if dtype not in _MODELS:
        meta, _ = FX.load(rc.E2E_FIXTURE)
        m = build_model(meta, dtype)[0]
        m.eval()
        _MODELS[dtype] = m
    return _MODELS[dtype]


def _images():
    if "imgs" not in _REF:
        _REF["imgs"] = rc.e2e_images(FX).to(DEV)
    return _REF["imgs"]


def _same_family(m, rows_a, rows_b):
    """the caveat of the contract: both sides' step and head GEMMs take the same family at these row counts"""
    fused = m.dtype == torch.bfloat16 and os.environ.get("MIT_DECODE_FUSED", "1") != "0"
    a, b = st.gemm_families(N, m.decoder, rows_a, fused), st.gemm_families(N, m.decoder, rows_b, fused)
    assert a == b, f"GEMM families differ between {rows_a} and {rows_b} rows: choose other row counts\n{a}\n{b}"


def _same_chunk_family(m, *sizes):
    """... and so do the GEMMs in front of the token steps (encoder, projection, cross-attention K/V) at every size an
    encoder chunk takes, against the static decoders' batch of all 20 images"""
    def fam(n):
        k = ("chunk", m.dtype, n)
        if k not in _REF:
            _REF[k] = st.chunk_families(N, m, _images()[:n])
        return _REF[k]
    for n in sizes:
        assert fam(n) == fam(20), f"GEMM families of a chunk of {n} images differ from those of 20 images"


def _static_sample(m, key, end=END, **kw):
    """generate_sample_batch on the 20 images with (ids, logprob) pairs, once per (model, options)"""
    k = ("sample", key, end, tuple(sorted((a, str(b)) for a, b in kw.items())))
    if k not in _REF:
        _REF[k] = m.generate_sample_batch(_images(), START, end, max_len=MAX_LEN, return_logprob=True, **kw)
    return _REF[k]


def _bits(pairs):
    """[[(ids, logprob)]] with the logprob as its float32 bit pattern: equality is then bitwise"""
    return [[(ids, torch.tensor(lp, dtype=torch.float32).view(torch.int32).item()) for ids, lp in per] for per in pairs]


def _check_sampled(m, tag, sampling, N_, slots, **kw):
    want = _static_sample(m, tag, num_samples=N_, seed=11, **sampling, **{k: v for k, v in kw.items()
                                                                          if k == "kv_dtype"})
    _same_family(m, 20 * N_, slots)
    # an encoder chunk is `slots` images; ONE image (197 memory rows <= 256) would take the register-streaming GEMM
    # family where the static batch takes the tile kernels: one slot is fed by chunks of two
    if slots == 1:
        kw = dict(kw, encode_batch=2, pool=2)
    chunk = kw.get("encode_batch", min(slots, 20))
    _same_chunk_family(m, chunk, 20 % chunk or chunk)
    got = m.generate_stream(_images(), START, END, max_len=MAX_LEN, num_samples=N_, seed=11, slots=slots,
                            return_logprob=True, **sampling, **kw)
    assert [[ids for ids, _ in per] for per in got] == [[ids for ids, _ in per] for per in want], "ids"
    assert _bits(got) == _bits(want), "log-probabilities differ in bits"
    assert len({len(ids) for per in want for ids, _ in per}) > 1, "the samples' lengths are ragged"


# one axis at a time around the base case (bf16 fused, temperature 0.7 / top_k 20 / top_p 0.9, N 3, 4 slots)
@pytest.mark.parametrize("sampling,N_,slots,check_every", [
    (BASE, 3, 4, None), (PLAIN, 3, 4, None), (BASE, 1, 4, None), (BASE, 3, 1, None), (BASE, 3, 3, None),
    (BASE, 3, 32, None), (BASE, 3, 4, 1), (BASE, 3, 4, 3)],
    ids=["base", "plain", "N1", "slots1", "slots3", "slots32", "every1", "every3"])
def test_sampled_stream_bf16(sampling, N_, slots, check_every):
    _check_sampled(_model(torch.bfloat16), "bf16", sampling, N_, slots, check_every=check_every)


def test_sampled_stream_fp32():
    _check_sampled(_model(torch.float32), "f32", BASE, 3, 4)
    _check_sampled(_model(torch.float32), "f32", PLAIN, 1, 3)


def test_sampled_stream_unfused(monkeypatch):
    monkeypatch.setenv("MIT_DECODE_FUSED", "0")
    _check_sampled(_model(torch.bfloat16), "bf16-unfused", BASE, 3, 4)


def test_sampled_stream_fp8_kv():
    _check_sampled(_model(torch.bfloat16), "bf16", BASE, 3, 4, kv_dtype="fp8")


def test_caps():
    """END never produced and max_lens[i] = (7 i) % 19 + 1: item (i, n) is the static row cut at its cap, whatever the
    model samples -- refills guaranteed; cap 1 yields [START] and takes no slot."""
    m = _model(torch.bfloat16)
    caps = [(7 * i) % 19 + 1 for i in range(20)]
    full = _static_sample(m, "bf16", end=NEVER, num_samples=3, seed=5, **BASE)
    _same_family(m, 60, 4)
    _same_chunk_family(m, 4)
    got = m.generate_stream(_images(), START, NEVER, max_len=MAX_LEN, num_samples=3, seed=5, slots=4, max_lens=caps,
                            **BASE)
    assert [[ids for ids, _ in per] for per in got] == [[ids[:c] for ids, _ in per] for per, c in zip(full, caps)]
    i1 = caps.index(1)
    assert [ids for ids, _ in got[i1]] == [[START]] * 3 and [lp for _, lp in got[i1]] == [0.0] * 3
    assert m.last_rolling_schedule.admits > 1


def test_chunks_and_image_offset():
    m = _model(torch.bfloat16)
    imgs = _images()
    want = _static_sample(m, "bf16", num_samples=3, seed=11, **BASE)
    _same_family(m, 60, 4)
    _same_chunk_family(m, 4, 3, 2)
    kw = dict(max_len=MAX_LEN, num_samples=3, seed=11, slots=4, return_logprob=True, **BASE)
    got = m.generate_stream([imgs[:7], imgs[7:8], imgs[8:]], START, END, **kw)
    assert _bits(got) == _bits(want)
    got = m.generate_stream(imgs, START, END, encode_batch=3, pool=6, **kw)
    assert _bits(got) == _bits(want)
    # a split dataset: the second half with its global image numbers
    a = m.generate_stream(imgs[:8], START, END, **kw)
    b = m.generate_stream(imgs[8:], START, END, image_offset=8, **kw)
    assert _bits(a + b) == _bits(want)
    assert m.generate_stream(torch.empty(0, *imgs.shape[1:]), START, END, **kw) == []


PROMPTS = [[[], [5], [7, 11, 13]][i % 3] for i in range(20)]          # per-image prompts of lengths 0, 1 and 3
CONSTRAINTS = {
    "theta": dict(repetition_penalty=1.3),
    "ngram": dict(no_repeat_ngram_size=2),
    "minlen": dict(min_length=8),
    "suppress": dict(suppress_tokens=(0, 1, 2, 3, 69)),
    "prompts": dict(prompts=PROMPTS),
    "shared-prompt": dict(prompts=[9, 4]),
    "all": dict(repetition_penalty=1.2, no_repeat_ngram_size=3, min_length=6, suppress_tokens=(0, 1, 3),
                prompts=PROMPTS),
}


@pytest.mark.parametrize("name", list(CONSTRAINTS))
def test_constrained_greedy(name):
    kw = CONSTRAINTS[name]
    for dtype in (torch.bfloat16, torch.float32) if name == "all" else (torch.bfloat16,):
        m = _model(dtype)
        want = m.generate_batch(_images(), START, END, max_len=MAX_LEN, **kw)
        for slots in (4, 3):
            _same_family(m, 20, slots)
            _same_chunk_family(m, slots, 20 % slots or slots)
            got = m.generate_stream(_images(), START, END, max_len=MAX_LEN, slots=slots, **kw)
            assert got == want, (name, dtype, slots)
        for i, p in enumerate(PROMPTS if "prompts" in kw and name != "shared-prompt" else []):
            assert want[i][1:1 + len(p)] == p


def test_unconstrained_greedy():
    m = _model(torch.bfloat16)
    want = m.generate_batch(_images(), START, END, max_len=MAX_LEN)
    assert m.generate_stream(_images(), START, END, max_len=MAX_LEN, slots=4) == want
    it = m.generate_stream_iter(_images()[:2], START, END, max_len=MAX_LEN, slots=4)
    assert all(lp is None and n == 0 for _, n, _, lp in it)


def test_constrained_sampled():
    m = _model(torch.bfloat16)
    kw = dict(CONSTRAINTS["all"], num_samples=2, seed=3, **BASE)
    want = m.generate_sample_batch(_images(), START, END, max_len=MAX_LEN, return_logprob=True, **kw)
    _same_family(m, 40, 4)
    _same_chunk_family(m, 4)
    got = m.generate_stream(_images(), START, END, max_len=MAX_LEN, slots=4, return_logprob=True, **kw)
    assert _bits(got) == _bits(want)
    for i, p in enumerate(PROMPTS):
        assert all(ids[1:1 + len(p)] == p for ids, _ in got[i])


def test_launch_modes_agree(monkeypatch):
    m = _model(torch.bfloat16)
    kw = dict(CONSTRAINTS["theta"], num_samples=2, seed=3, **BASE)
    want = _bits(m.generate_sample_batch(_images(), START, END, max_len=MAX_LEN, return_logprob=True, **kw))
    _same_family(m, 40, 3)
    _same_chunk_family(m, 3, 2)
    run = lambda **o: _bits(m.generate_stream(_images(), START, END, max_len=MAX_LEN, slots=3,   # noqa: E731
                                              return_logprob=True, **kw, **o))
    assert run(use_graph=False) == want
    for launch in ("eager", "graph", "plan"):
        monkeypatch.setenv("MIT_DECODE_LAUNCH", launch)
        assert run() == want, launch


def test_iter_yields_in_completion_order():
    """Image 0 (cap 10) and image 1 (cap 3) are admitted together into the four slots: image 1's samples come first."""
    m = _model(torch.bfloat16)
    got = list(m.generate_stream_iter(_images()[:3], START, NEVER, max_len=MAX_LEN, slots=4, num_samples=2, seed=1,
                                      check_every=1, max_lens=[10, 3, 5], **PLAIN))
    assert sorted((i, n) for i, n, _, _ in got) == [(i, n) for i in range(3) for n in range(2)]
    order = [(i, n) for i, n, _, _ in got]
    assert max(order.index((1, 0)), order.index((1, 1))) < min(order.index((0, 0)), order.index((0, 1)))
    assert all(len(ids) == [10, 3, 5][i] and isinstance(lp, float) for i, _, ids, lp in got)


def test_rejections_come_before_any_launch():
    """Raised by the call itself, not by the first next(): nothing was encoded, allocated or launched."""
    m = _model(torch.float32)
    imgs = _images()
    for kw in (dict(beam_size=3), dict(method="beam"), dict(streams=2), dict(temperature=0.0), dict(temperature=-1.0),
               dict(temperature=1.0, top_p=0.0), dict(temperature=1.0, top_k=-1), dict(temperature=1.0, num_samples=0),
               dict(num_samples=2), dict(slots=0), dict(max_lens=[0] * 20), dict(max_lens=[3] * 19 + [MAX_LEN + 1]),
               dict(max_len=m.decoder.pe.shape[0] + 1), dict(repetition_penalty=0.0), dict(no_repeat_ngram_size=-1),
               dict(suppress_tokens=(10 ** 6,)), dict(prompts=[END]), dict(prompts=list(range(3, 3 + MAX_LEN))),
               dict(image_offset=-1)):
        with pytest.raises(ValueError):
            m.generate_stream_iter(imgs, START, END, **{"max_len": MAX_LEN, **kw})
    with pytest.raises(ValueError, match="bfloat16"):
        m.generate_stream_iter(imgs, START, END, max_len=MAX_LEN, kv_dtype="fp8")
    # per-image lists are checked chunk by chunk, before that chunk's launches
    it = m.generate_stream_iter(imgs, START, END, max_len=MAX_LEN, slots=4, prompts=[[5]] * 19)
    with pytest.raises(ValueError, match="prompts"):
        list(it)
    it = m.generate_stream_iter(imgs, START, END, max_len=MAX_LEN, slots=4, prompts=[[5]] * 19 + [[END]])
    with pytest.raises(ValueError, match="END"):
        list(it)
    it = m.generate_stream_iter(imgs, START, END, max_len=MAX_LEN, slots=4, max_lens=[5] * 19)
    with pytest.raises(ValueError, match="max_lens"):
        list(it)


def test_generate_captions_stream_slots():
    import inference
    m = _model(torch.bfloat16)
    imgs = _images()
    common = dict(start_token_id=START, end_token_id=END, max_len=MAX_LEN, batch_size=8)
    _same_family(m, 8, 4)
    _same_chunk_family(m, 8, 4)           # batch_size = 8 on both sides: chunks of 8, 8 and 4 images
    for kw in (dict(temperature=0.8, top_k=20, seed=3), dict(), dict(repetition_penalty=1.2, prompts=PROMPTS),
               dict(temperature=1.0, min_length=4, prompts=[9])):
        base = inference.generate_captions(m, imgs, **common, **kw)
        got = inference.generate_captions(m, imgs, **common, stream_slots=4, **kw)
        assert got == base and len(base) == 20, kw
    with pytest.raises(ValueError, match="stream_slots"):
        inference.generate_captions(m, imgs, **common, stream_slots=4, beam_size=3)
    with pytest.raises(ValueError, match="stream_slots"):
        inference.generate_captions(m, imgs, **common, stream_slots=4, rolling_slots=4)
