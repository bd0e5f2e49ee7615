"""Rolling-batch captioning end to end on the GPU (ImageToTextModel.generate_rolling / generate_rolling_iter,
inference.generate_captions(rolling_slots=...)): exactly generate_batch's ids -- and in fp32 the oracle's, which
tests/test_rolling_contract_cpu.py shows pinned -- for every slot count and poll interval, plan and eager launches,
the fused and the unfused bf16 step, FP8 cross-attention K/V, per-image caps, and the argument rejections."""
import pytest
import torch

import fixtures as FX
import native as N
import rolling_contract as rc
from model_util import build_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
START, END, NEVER, MAX_LEN = rc.START, rc.END, rc.NEVER, rc.MAX_LEN
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


def _model(dtype, name=rc.E2E_FIXTURE):
    if (name, dtype) not in _MODELS:
        meta, _ = FX.load(name)
        m = build_model(meta, dtype)[0]
        m.eval()
        _MODELS[(name, dtype)] = m
    return _MODELS[(name, dtype)]


def _images(name=rc.E2E_FIXTURE):
    return rc.e2e_images(FX, name).to(DEV)


def _static(m, key, end, **kw):
    """generate_batch on the 20 images, once per (model, END, options)"""
    if key not in _REF:
        _REF[key] = m.generate_batch(_images(), START, end, max_len=MAX_LEN, **kw)
    return _REF[key]


@pytest.mark.parametrize("check_every", [1, 3])
@pytest.mark.parametrize("slots", rc.SLOTS)
def test_fp32_ids_are_the_oracles_and_generate_batchs(slots, check_every):
    m = _model(torch.float32)
    want = [rc.cut(r, END) for r in rc.oracle(FX)[0]]
    assert [len(r) for r in want] == rc.e2e_lengths()
    assert _static(m, "f32", END) == want
    assert m.generate_rolling(_images(), START, END, max_len=MAX_LEN, slots=slots, check_every=check_every) == want


def test_plan_and_eager_launches_agree(monkeypatch):
    m = _model(torch.float32)
    want = _static(m, "f32", END)
    assert m.generate_rolling(_images(), START, END, max_len=MAX_LEN, slots=3, use_graph=False) == want
    for launch in ("eager", "graph", "plan"):
        monkeypatch.setenv("MIT_DECODE_LAUNCH", launch)
        assert m.generate_rolling(_images(), START, END, max_len=MAX_LEN, slots=3) == want, launch


@pytest.mark.parametrize("fused", ["1", "0"], ids=["fused", "unfused"])
def test_bf16_equals_generate_batch(monkeypatch, fused):
    """Exact equality, list for list: a row's arithmetic does not depend on its neighbours or their positions."""
    monkeypatch.setenv("MIT_DECODE_FUSED", fused)
    m = _model(torch.bfloat16)
    for kv in (None, "fp8"):
        kw = {} if kv is None else {"kv_dtype": kv}
        want = m.generate_batch(_images(), START, END, max_len=MAX_LEN, **kw)
        assert m.generate_rolling(_images(), START, END, max_len=MAX_LEN, slots=4, **kw) == want, (fused, kv)


@pytest.mark.parametrize("fixture", [rc.E2E_FIXTURE, "tiny_vit_v509"])
def test_caps(fixture):
    """max_lens[i] = (7 i) % 19 + 1 (1 included) with END never produced: result i is generate_batch's row cut there;
    tiny_vit_v509: a vocabulary that is no multiple of 8 (the head's argmax epilogue)."""
    m = _model(torch.bfloat16, fixture)
    imgs = _images(fixture)
    caps = [(7 * i) % 19 + 1 for i in range(imgs.shape[0])]
    full = m.generate_batch(imgs, START, NEVER, max_len=MAX_LEN)
    got = m.generate_rolling(imgs, START, NEVER, max_len=MAX_LEN, slots=4, max_lens=caps)
    assert got == [r[:c] for r, c in zip(full, caps)]
    assert got[caps.index(1)] == [START]


def test_iter_yields_in_completion_order():
    m = _model(torch.float32)
    want = _static(m, "f32", END)
    imgs = _images()
    got = list(m.generate_rolling_iter([imgs[:7], imgs[7:8], imgs[8:]], START, END, max_len=MAX_LEN, slots=4,
                                       check_every=1))
    assert sorted(i for i, _ in got) == list(range(20))
    assert all(ids == want[i] for i, ids in got)
    order = [i for i, _ in got]
    # image 0 (6 ids) is admitted with image 1 (4 ids) and yielded after it; image 6 never ends and, admitted
    # long before image 9 (4 ids), is yielded after it
    assert order.index(1) < order.index(0) and order.index(9) < order.index(6)
    assert m.generate_rolling(torch.empty(0, *imgs.shape[1:]), START, END, max_len=MAX_LEN) == []
    assert m.generate_rolling([], START, END, max_len=MAX_LEN) == []


def test_generate_captions_rolling_slots():
    import inference
    m = _model(torch.bfloat16)
    imgs = _images()
    base = inference.generate_captions(m, imgs, start_token_id=START, end_token_id=END, max_len=MAX_LEN, batch_size=8)
    roll = inference.generate_captions(m, imgs, start_token_id=START, end_token_id=END, max_len=MAX_LEN, batch_size=8,
                                       rolling_slots=4)
    assert roll == base and len(base) == 20
    for kw in (dict(beam_size=3), dict(temperature=1.0), dict(min_length=2), dict(prompts=[5]),
               dict(repetition_penalty=1.2), dict(no_repeat_ngram_size=2), dict(suppress_tokens=(7,))):
        with pytest.raises(ValueError, match="rolling_slots"):
            inference.generate_captions(m, imgs, start_token_id=START, end_token_id=END, max_len=MAX_LEN,
                                        rolling_slots=4, **kw)


def test_rejections_come_before_any_launch():
    m = _model(torch.float32)
    imgs = _images()
    for kw in (dict(repetition_penalty=1.3), dict(no_repeat_ngram_size=2), dict(min_length=3),
               dict(suppress_tokens=(4,)), dict(prompts=[5, 6]), dict(streams=2), dict(slots=0), dict(slots=-1),
               dict(max_lens=[0] * 20), dict(max_lens=[3] * 19 + [MAX_LEN + 1], max_len=MAX_LEN),
               dict(max_len=m.decoder.pe.shape[0] + 1)):
        with pytest.raises(ValueError):
            m.generate_rolling_iter(imgs, START, END, **{"max_len": MAX_LEN, **kw})
    with pytest.raises(ValueError, match="bfloat16"):
        m.generate_rolling_iter(imgs, START, END, max_len=MAX_LEN, kv_dtype="fp8")
