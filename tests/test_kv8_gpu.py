"""FP8 cross-attention K/V on the GPU (csrc/kv8.hip and the decode built on it), against tests/kv8_contract.py:
mit_kv_quantize_fp8 bitwise against the CPU reference quantiser on guarded buffers, mit_attention_decode_fp8 against
decode_contract's float64 attention on the dequantised values within decode_contract.BOUND["attn"] (and against the
project's own bf16 kernels on the same values), and the decode end to end: the fp8 state, the quantised decode against
a bf16 state that holds the dequantised K/V, every launch option, and the default path left as it was."""
import pytest
import torch

import decode_contract as dc
import fixtures as FX
import kv8_contract as kc
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


# ------------------------------------------------------------------------------------------------
# mit_kv_quantize_fp8
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c.id for c in kc.QCASES])
def test_quantize(cid):
    """Bytes and scales bitwise the CPU reference's (pad columns in both buffers, batch strides wider than S rows,
    an all-zero group, a group whose amax is exactly 448 * 2^3, e4m3 subnormals and a subnormal tie, -0); src is NaN
    outside its windows; nothing outside dst's and the scales' windows is written, src is unchanged; a second launch
    is bitwise equal."""
    c = kc.Q_BY_ID[cid]
    t = kc.make_quant(c).to(DEV)
    t.snapshot()
    assert kc.launch_quant(N, c, t) == 0, N.lib().mit_last_error()
    torch.cuda.synchronize()
    kc.check_quant(c, t)
    first = {k: a.bits().cpu().clone() for k, a in t.a.items()}
    t.restore()
    assert kc.launch_quant(N, c, t) == 0
    torch.cuda.synchronize()
    for k, a in t.a.items():
        assert torch.equal(a.bits().cpu(), first[k]), f"{cid}: {k} differs between two launches"


def test_quantize_is_recordable():
    c = kc.QCASES[1]
    t = kc.make_quant(c).to(DEV)
    t.snapshot()
    prog = N.record(lambda: N._check(kc.launch_quant(N, c, t), "mit_kv_quantize_fp8"))
    assert prog.launches() == 1
    t.restore()
    prog.run()
    torch.cuda.synchronize()
    kc.check_quant(c, t)


# ------------------------------------------------------------------------------------------------
# mit_attention_decode_fp8
# ------------------------------------------------------------------------------------------------
def _run_attn(c, repeat=False):
    t = kc.make_attn(c, repeat=repeat).to(DEV)
    t.snapshot()
    assert kc.launch_attn(N, c, t) == 0, N.lib().mit_last_error()
    torch.cuda.synchronize()
    return t


@pytest.mark.parametrize("cid", [c.id for c in kc.ACASES])
def test_attention(cid):
    """Against the float64 attention on the dequantised values in decode_contract's attn unit, bound BOUND["attn"] =
    2.596 (K / V bytes 0x7F = NaN in pad columns, rows j >= Lk and between the images; NaN scales and q outside
    their windows); o outside its windows untouched, inputs unchanged, a second launch bitwise equal; the planned
    family is the case's. group > 1 against group = 1 on physically repeated K / V and scales: BITWISE, since one
    kernel per family serves both (a block per row, or per (row, head), reads image r / group)."""
    c = kc.A_BY_ID[cid]
    t = _run_attn(c)
    assert N.lib().mit_attention_decode_fp8_plan(*kc.attn_args(c, t)) == c.family
    fig = kc.check_attn(c, t)
    print(f"{cid}: figure {fig:.3f} (bound {kc.BOUND['attn']:.3f})")
    assert fig <= kc.BOUND["attn"], f"{cid}: {fig:.3f} units > {kc.BOUND['attn']:.3f}"
    first = {k: a.bits().cpu().clone() for k, a in t.a.items()}
    t.restore()
    assert kc.launch_attn(N, c, t) == 0
    torch.cuda.synchronize()
    for k, a in t.a.items():
        assert torch.equal(a.bits().cpu(), first[k]), f"{cid}: {k} differs between two launches"
    if c.group > 1:
        t1 = _run_attn(c, repeat=True)
        assert t1.x["group"] == 1 and t1.x["K8"].shape[0] == c.R
        kc.check_attn(c, t1)
        assert torch.equal(kc.attn_output(c, t1).view(torch.int16), kc.attn_output(c, t).view(torch.int16)), \
            f"{cid}: group = {c.group} differs bitwise from group = 1 on repeated K / V"


@pytest.mark.parametrize("cid", ["rows-H8-Dh64-R6-g3-Lk197", "bh-H3-Dh32-R4-g2-Lk70"])
def test_attention_against_the_bf16_kernels(cid):
    """attention_decode_beam (group > 1: the block-per-(row, head) bf16 family) and attention_decode (the K / V
    repeated per row: the bf16 ROWS_NT family at H * Dh = 512) in bf16 on the dequantised K | V: each is within
    BOUND["attn"] of the same float64 reference, so they agree with the fp8 kernel within the sum of the bounds."""
    c = kc.A_BY_ID[cid]
    t = _run_attn(c)
    X = t.x
    ref, unit = kc.reference_attn(c, t)
    got8 = kc.attn_output(c, t).double()
    images, W, Dh = c.R // c.group, X["W"], c.Dh
    Kd = kc.dequantize_ref(X["K8"], X["ks"]).reshape(images, c.Lk, W)
    Vd = kc.dequantize_ref(X["V8"], X["vs"]).reshape(images, c.Lk, W)
    kv = torch.cat([Kd, Vd], -1).to(torch.bfloat16)
    assert torch.equal(kv.double(), torch.cat([Kd, Vd], -1)), "a dequantised value is not exact in bf16"
    kv = kv.to(DEV)
    q = X["q"].reshape(c.R, W).to(DEV)
    rb = c.Lk * 2 * W
    outs = {}
    o = torch.empty(c.R, W, dtype=torch.bfloat16, device=DEV)
    N.attention_decode_beam(q, W, kv, 2 * W, rb, kv[:, :, W:], 2 * W, rb, o, W, c.R, c.H, Lk=c.Lk, group=c.group,
                            scale=X["scale"], Dh=Dh)
    outs["attention_decode_beam"] = o.cpu()
    rep = kv.repeat_interleave(c.group, 0).contiguous()
    o2 = torch.empty_like(o)
    N.attention_decode(q, W, rep, 2 * W, rb, rep[:, :, W:], 2 * W, rb, o2, W, c.R, c.H, Lk=c.Lk, scale=X["scale"], Dh=Dh)
    torch.cuda.synchronize()
    outs["attention_decode"] = o2.cpu()
    for name, ob in outs.items():
        figs = []
        dc.check_float(name, "attn", ob, ref, unit, True, figs)
        assert figs[0][2] <= dc.BOUND["attn"], (name, figs)
        # both within the bound of one reference (past their own bf16 output roundings): within the sum of each other
        slack = 2 * dc.BOUND["attn"] * unit + 2 * dc.BF16_REL * ref.abs()
        assert bool(((ob.double() - got8).abs() <= slack).all()), name


# ------------------------------------------------------------------------------------------------
# the decode
# ------------------------------------------------------------------------------------------------
FIXTURE = "tiny_vit_patches"
START, NEVER, MAX_LEN = 2, 10 ** 6, 12


def _model(name=FIXTURE):
    if name not in _MODELS:
        meta, _ = FX.load(name)
        m = build_model(meta, torch.bfloat16)[0]
        m.eval()
        _MODELS[name] = (m, meta)
    return _MODELS[name]


def _images(meta):
    img = FX.inputs(meta, 0)[0]
    return torch.cat([img, img.flip(-1), img * 0.5, img.flip(-2)], 0)[:4].to(DEV)


def _memory(m, imgs):
    return m._encode_memory(imgs.float())


def test_state_holds_bytes_and_scales_only():
    """kv_dtype = "fp8": uint8 kv8 [L, images*S, 2d], f32 kv_scale [L, images, 2H] of powers of two, no kv tensor;
    the default state: kv in the decoder's dtype, no kv8; a float32 decoder refuses."""
    m, meta = _model()
    imgs = _images(meta)
    mem, mem_ld, S, _, _ = _memory(m, imgs)
    dec, B = m.decoder, imgs.shape[0]
    d, L, H = dec.d, dec.L, dec.H
    for begin, rows in ((lambda **kw: dec.decode_begin(mem, mem_ld, S, B, MAX_LEN, START, NEVER, **kw), B),
                        (lambda **kw: dec.beam_begin(mem, mem_ld, S, B, 3, MAX_LEN, START, NEVER, **kw), 3 * B),
                        (lambda **kw: dec.sample_begin(mem, mem_ld, S, B, 2, MAX_LEN, START, NEVER, **kw), 2 * B)):
        stt = begin(kv_dtype="fp8")
        assert stt.kv is None and stt.kv_dtype == "fp8" and stt.B == rows
        assert stt.kv8.dtype == torch.uint8 and tuple(stt.kv8.shape) == (L, B * S, 2 * d)
        assert stt.kv_scale.dtype == torch.float32 and tuple(stt.kv_scale.shape) == (L, B, 2 * H)
        assert (torch.frexp(stt.kv_scale.cpu())[0] == 0.5).all()
        ref = begin()
        assert ref.kv8 is None and ref.kv_scale is None and ref.kv_dtype == "bf16"
        assert ref.kv.dtype == torch.bfloat16 and tuple(ref.kv.shape) == (L, B * S, 2 * d)
        # the state's bytes and scales are the reference quantiser's of the default state's bf16 K | V
        x = ref.kv.cpu().view(L * B, S, 2 * H, dec.hd)
        q8, sc = kc.quantize_ref(x)
        assert torch.equal(stt.kv8.cpu().view(L * B, S, 2 * H, dec.hd), q8)
        assert torch.equal(stt.kv_scale.cpu().view(L * B, 2 * H), sc)
        assert torch.equal(begin(kv_dtype="bf16").kv, ref.kv)
    m32 = build_model(meta, torch.float32)[0]
    m32.eval()
    mem32, ld32, S32, _, _ = _memory(m32, imgs)
    with pytest.raises(ValueError, match="bfloat16 decoder"):
        m32.decoder.decode_begin(mem32, ld32, S32, B, MAX_LEN, START, NEVER, kv_dtype="fp8")


def test_quantised_decode_is_the_bf16_decode_on_dequantised_kv():
    """generate_sample_batch(top_k = 1, kv_dtype = "fp8") against a bf16 SampleState whose kv was overwritten after
    sample_begin with the dequantised kv8 * scale and which is driven step by step: per image the ids agree up to the
    first position where the overwritten run's top-1 - top-2 logit margin is below 3e-2 (the bf16 near-tie threshold
    of tests/test_decode_gpu.py), and at least one image is compared over its whole length."""
    m, meta = _model()
    imgs = _images(meta)
    B = imgs.shape[0]
    got = m.generate_sample_batch(imgs, START, NEVER, max_len=MAX_LEN, temperature=1.0, top_k=1, seed=0, kv_dtype="fp8")
    mem, mem_ld, S, _, _ = _memory(m, imgs)
    dec = m.decoder
    s8 = dec.sample_begin(mem, mem_ld, S, B, 1, MAX_LEN, START, NEVER, top_k=1, kv_dtype="fp8")
    stt = dec.sample_begin(mem, mem_ld, S, B, 1, MAX_LEN, START, NEVER, top_k=1)
    L, H, hd = dec.L, dec.H, dec.hd
    deq = kc.dequantize_ref(s8.kv8.cpu().view(L * B, S, 2 * H, hd), s8.kv_scale.cpu().view(L * B, 2 * H))
    stt.kv.copy_(deq.view(L, B * S, 2 * dec.d).to(torch.bfloat16))
    margins = []
    for _ in range(MAX_LEN - 1):
        dec.sample_step(stt)
        top2 = stt.logits[:, :dec.V].float().topk(2, dim=1).values
        margins.append((top2[:, 0] - top2[:, 1]).cpu())
    want = stt.ids.cpu().tolist()
    margins = torch.stack(margins, 1)                       # [B, steps]: the step that produced column j + 1
    whole = 0
    for b in range(B):
        stop = next((j for j in range(MAX_LEN - 1) if margins[b, j] < 3e-2), MAX_LEN - 1)
        print(f"image {b}: compared {stop} of {MAX_LEN - 1} steps; smallest margin {float(margins[b].min()):.3e}")
        assert got[b][:stop + 1] == want[b][:stop + 1], (b, got[b], want[b], margins[b])
        whole += stop == MAX_LEN - 1
    assert whole >= 1, f"no image compared over its whole length: {margins}"


def test_same_ids_under_every_launch_option(monkeypatch):
    """generate_batch(kv_dtype = "fp8"): identical ids with MIT_DECODE_LAUNCH = plan / graph / eager, streams = 1 / 2,
    the fused step and MIT_DECODE_FUSED = 0; valid ids ending as token_lists documents; through the environment
    (MIT_DECODE_KV) the same. Beam search (3 beams) and sampling (3 samples) run on the fp8 state, return the
    documented shapes and are deterministic over two calls."""
    m, meta = _model()
    imgs = _images(meta)
    B, V, end = imgs.shape[0], m.decoder.V, 3
    one = m.generate_batch(imgs, START, end, max_len=MAX_LEN, kv_dtype="fp8")
    assert len(one) == B
    for ids in one:
        assert ids[0] == START and 2 <= len(ids) <= MAX_LEN and all(0 <= i < V for i in ids)
        assert end not in ids[1:-1] and (ids[-1] == end or len(ids) == MAX_LEN)
    for launch in ("plan", "graph", "eager"):
        monkeypatch.setenv("MIT_DECODE_LAUNCH", launch)
        for streams in (1, 2):
            assert m.generate_batch(imgs, START, end, max_len=MAX_LEN, kv_dtype="fp8", streams=streams) == one, \
                (launch, streams)
    monkeypatch.delenv("MIT_DECODE_LAUNCH")
    # the unfused step body (its LayerNorms round differently; test_fused_and_unfused_fp8_steps_agree compares the two
    # bodies step by step with the near-tie margin): on these images it picks the very same ids
    monkeypatch.setenv("MIT_DECODE_FUSED", "0")
    unfused = m.generate_batch(imgs, START, end, max_len=MAX_LEN, kv_dtype="fp8")
    assert unfused == one, (unfused, one)
    monkeypatch.setenv("MIT_DECODE_LAUNCH", "eager")
    assert m.generate_batch(imgs, START, end, max_len=MAX_LEN, kv_dtype="fp8", streams=2) == unfused
    monkeypatch.delenv("MIT_DECODE_LAUNCH")
    monkeypatch.delenv("MIT_DECODE_FUSED")
    assert [u[0] for u in unfused] == [START] * B and all(0 <= i < V for u in unfused for i in u)
    monkeypatch.setenv("MIT_DECODE_KV", "fp8")
    assert m.generate_batch(imgs, START, end, max_len=MAX_LEN) == one
    monkeypatch.delenv("MIT_DECODE_KV")
    beams = [m.generate_beam_batch(imgs, START, end, max_len=MAX_LEN, beam_size=3, return_all=True, kv_dtype="fp8")
             for _ in range(2)]
    assert beams[0] == beams[1] and len(beams[0]) == B and all(len(x) == 3 for x in beams[0])
    assert all(ids[0] == START and all(0 <= i < V for i in ids) for x in beams[0] for ids, _ in x)
    best = m.generate_beam_batch(imgs, START, end, max_len=MAX_LEN, beam_size=3, kv_dtype="fp8")
    assert best == [x[0][0] for x in beams[0]]
    kw = dict(max_len=MAX_LEN, num_samples=3, temperature=0.9, top_k=20, seed=7, kv_dtype="fp8")
    samples = [m.generate_sample_batch(imgs, START, end, **kw) for _ in range(2)]
    assert samples[0] == samples[1] and len(samples[0]) == B and all(len(x) == 3 for x in samples[0])
    assert all(ids[0] == START and all(0 <= i < V for i in ids) for x in samples[0] for ids, _ in x)


def test_fused_and_unfused_fp8_steps_agree(monkeypatch):
    """An fp8 DecodeState on the fused step and one on the unfused step (MIT_DECODE_FUSED = 0), driven token by token
    on a shared prefix as tests/test_decode_gpu.py::test_fused_decode_step_matches_unfused drives the bf16 ones: the
    two pick the same id in every row whose unfused top-1 - top-2 logit margin exceeds that test's 0.05 (the bf16
    rounding of the LayerNorm outputs), and at least one row is compared at every step of its length."""
    m, meta = _model()
    imgs = _images(meta)
    mem, mem_ld, S, _, _ = _memory(m, imgs)
    dec, B = m.decoder, imgs.shape[0]
    monkeypatch.setenv("MIT_DECODE_FUSED", "1")
    a = dec.decode_begin(mem, mem_ld, S, B, MAX_LEN, START, NEVER, kv_dtype="fp8")
    monkeypatch.setenv("MIT_DECODE_FUSED", "0")
    b = dec.decode_begin(mem, mem_ld, S, B, MAX_LEN, START, NEVER, kv_dtype="fp8")
    assert a.fused and not b.fused and a.kv8 is not None and b.kv8 is not None
    assert torch.equal(a.kv8, b.kv8) and torch.equal(a.kv_scale, b.kv_scale)
    always = torch.ones(B, dtype=torch.bool)
    checked = 0
    for t in range(MAX_LEN - 1):
        dec.decode_step(a)
        dec.decode_step(b)
        top2 = b.logits[:, :dec.V].float().topk(2, dim=1).values
        safe = (top2[:, 0] - top2[:, 1]) > 0.05
        assert torch.equal(a.ids[safe, t + 1], b.ids[safe, t + 1]), (t, a.ids, b.ids, top2)
        checked += int(safe.sum())
        always &= safe.cpu()
        assert a.pos.item() == b.pos.item() == t + 1
        b.ids.copy_(a.ids)  # share the prefix (near-ties may pick differently)
    print(f"{checked} of {B * (MAX_LEN - 1)} picks compared; rows compared at every step: {always.tolist()}")
    assert bool(always.any()), "no row compared over its whole length"


def test_default_path_is_untouched(monkeypatch):
    """kv_dtype = None and "bf16" give the same ids, and the recorded step program of the default state has the
    launches it had before FP8 K/V existed: the fused greedy step is embed_decode + 8 per layer (self_in, self
    attention, self_out, cross_q, cross attention, cross_out, linear1, linear2) + decode_layernorm + the head GEMM +
    greedy_pick_keys = 8 L + 4 (20 for this L = 2 fixture, 52 at L = 6), the unfused one embed_decode + 12 per
    layer (the same eight, kv_store and three LayerNorms) + the head + greedy_pick + step_inc = 12 L + 4 (28 here).
    Both counts are the parent commit's, from its decode_step. The fp8 step has exactly as many: one cross-attention
    launch per layer replaced by one."""
    monkeypatch.delenv("MIT_DECODE_KV", raising=False)
    m, meta = _model()
    imgs = _images(meta)
    assert m.generate_batch(imgs, START, NEVER, max_len=MAX_LEN) == \
        m.generate_batch(imgs, START, NEVER, max_len=MAX_LEN, kv_dtype="bf16")
    mem, mem_ld, S, _, _ = _memory(m, imgs)
    dec, B = m.decoder, imgs.shape[0]
    L = dec.L
    assert L == 2
    for fused, want in (("1", 20), ("0", 28)):
        monkeypatch.setenv("MIT_DECODE_FUSED", fused)
        for kv_dtype in (None, "fp8"):
            stt = dec.decode_begin(mem, mem_ld, S, B, MAX_LEN, START, NEVER, kv_dtype=kv_dtype)
            dec.decode_step(stt)
            prog = N.record(lambda: dec.decode_step(stt))
            assert prog.launches() == want, (fused, kv_dtype, prog.launches())
