"""FP8 cross-attention K/V without a GPU (tests/kv8_contract.py): the reference quantiser's properties, the planned
kernel family of mit_attention_decode_fp8 and one rejected call per argument rule of it and of mit_kv_quantize_fp8
(validation precedes any launch; synthetic aligned addresses, nothing is dereferenced), resolve_kv_dtype, the command
line, and generate_captions passing kv_dtype on."""
import pytest
import torch

import kv8_contract as kc
import native

BASE = 0x7F0000000000   # synthetic addresses: 16-B aligned, never dereferenced


# ------------------------------------------------------------------------------------------------
# the reference quantiser
# ------------------------------------------------------------------------------------------------
def _inputs():
    out = []
    for si, sigma in enumerate(kc.SIGMAS):
        for (S, Dh) in kc.GROUP_SHAPES:
            out.append((f"sigma{sigma:g}-S{S}-Dh{Dh}", kc.gaussian_groups(sigma, 2, S, 3, Dh, seed=si * 10 + S)))
    z = torch.zeros(1, 5, 2, 16, dtype=torch.bfloat16)
    z[0, :, 1] = kc.gaussian_groups(1.0, 1, 5, 1, 16, seed=3)[0, :, 0]
    z[0, 2, 0, 4] = -0.0
    out.append(("zero-group", z))
    out.append(("single-element", torch.tensor([[[[-0.3]]]], dtype=torch.bfloat16)))   # Dh = 1: the formula alone
    for k in (-20, 0, 9):   # amax exactly 448 * 2^k (m = 1.75: the edge) and one bf16 step above it
        for top in (448.0, 450.0):
            x = kc.gaussian_groups(20.0, 1, 4, 1, 16, seed=k + 50).float().clamp(-400, 400)
            x[0, 1, 0, 2] = -top
            out.append((f"amax-{top:g}x2^{k}", (x * 2.0 ** k).to(torch.bfloat16)))
    return out


INPUTS = _inputs()


@pytest.mark.parametrize("name,x", INPUTS, ids=[n for n, _ in INPUTS])
def test_reference_quantiser_properties(name, x):
    q, s = kc.quantize_ref(x)
    assert q.dtype == torch.uint8 and q.shape == x.shape and s.shape == (x.shape[0], x.shape[2])
    m, _ = torch.frexp(s)
    assert (m == 0.5).all(), "a scale is not a power of two"
    assert not ((q & 0x7F) == 0x7F).any(), "a NaN byte (0x7F / 0xFF)"
    v8 = q.view(torch.float8_e4m3fn).float()
    amax8 = v8.abs().amax(dim=(1, 3))
    amax = x.float().abs().amax(dim=(1, 3))
    nz = amax > 0
    # q = x / scale before the rounding: its largest magnitude is in (224, 448]. (The byte it rounds to can be 224
    # itself: e4m3's step there is 16, and amax = 1.76 * 2^X scales to 225.3.)
    top = (amax / s)[nz]
    assert ((top > 224) & (top <= 448)).all(), top
    assert ((amax8[nz] >= 224) & (amax8[nz] <= 448)).all(), amax8
    assert (amax8[~nz] == 0).all() and (s[~nz] == 1).all()
    deq = kc.dequantize_ref(q, s)
    assert torch.equal(deq.to(torch.bfloat16).double(), deq), "a dequantised value is not exact in bf16"
    # quantising the dequantised values: the same values always, and the same bytes and scale in every group but
    # those whose largest byte rounded DOWN to 224 (amax = m 2^X with m in (1.75, 1.8125]: the dequantised amax is
    # 1.75 * 2^X, which the formula gives the next smaller scale -- bytes twice as large, the same products)
    q2, s2 = kc.quantize_ref(deq.to(torch.bfloat16))
    assert torch.equal(kc.dequantize_ref(q2, s2), deq), "quantising the dequantised values changes a value"
    same = (amax8 != 224)[:, None, :, None].expand_as(q)
    assert torch.equal(q2[same], q[same]) and torch.equal(s2[amax8 != 224], s[amax8 != 224]), \
        "quantising the dequantised values changes bytes or scales"
    edge = amax8 == 224
    assert torch.equal(s2[edge] * 2, s[edge])
    # -0 keeps its sign; relative error at most 1/17 where the byte is not an e4m3 subnormal
    xf = x.double()
    neg0 = (xf == 0) & torch.signbit(xf)
    assert (q[neg0] == 0x80).all()
    normal = v8.abs() >= kc.E4M3_MIN_NORMAL
    rel = ((deq - xf).abs() / xf.abs().clamp_min(1e-300))[normal]
    assert rel.numel() == 0 or float(rel.max()) <= 1 / 17 + 1e-12, float(rel.max())
    if name.startswith("amax-448"):
        assert int((q & 0x7F).max()) == 0x7E                # 448 itself: e = X - 8
    if name.startswith("amax-450"):                          # one bf16 step above 1.75 * 2^X: e = X - 7
        assert float((amax / s).max()) == 225.0 and float(amax8.max()) == 224.0


def test_quantiser_case_inputs_cover_the_edges():
    for c in kc.QCASES:
        x = kc.quant_input(c)
        q, s = kc.quantize_ref(x)
        assert float(s[0, 0]) == 8.0 and int(q[0, c.S // 2, 0, 3]) == 0xFE          # -448: amax = 448 * 2^3
        assert int(q[0, 0, 0, 5]) == 0x02 and int(q[0, 0, 0, 6]) == 0x02 and int(q[0, 0, 0, 7]) == 0x80
        if c.B * c.G > 1:
            assert float(s[-1, -1]) == 1.0 and not (q[-1, :, -1] & 0x7F).any() and int(q[-1, 0, -1, 1]) == 0x80


# ------------------------------------------------------------------------------------------------
# mit_attention_decode_fp8_plan
# ------------------------------------------------------------------------------------------------
def _attn(fn="plan", **kw):
    a = dict(R=6, H=8, Dh=64, q=BASE, q_batch=512, k=BASE + 0x10000, k_row=1024, k_batch=0x40000, v=BASE + 0x10200,
             v_row=1024, v_batch=0x40000, k_scale=BASE + 0x800000, v_scale=BASE + 0x800080, scale_batch=64,
             o=BASE + 0x900000, o_batch=512, Lk=197, group=3)
    a.update(kw)
    args = (a["R"], a["H"], a["Dh"], a["q"], a["q_batch"], a["k"], a["k_row"], a["k_batch"], a["v"], a["v_row"],
            a["v_batch"], a["k_scale"], a["v_scale"], a["scale_batch"], a["o"], a["o_batch"])
    if fn == "plan":
        return native.attention_decode_fp8_plan(*args, Lk=a["Lk"], group=a["group"])
    return native.lib().mit_attention_decode_fp8(*args, a["Lk"], a["group"], 0.125, None)


def test_attention_fp8_plan_families():
    native.load_library()
    assert (native.DECODE_ATTN_FP8_BH, native.DECODE_ATTN_FP8_ROWS) == (kc.FP8_BH, kc.FP8_ROWS)
    for Dh in (16, 32, 64, 128):
        assert _attn(H=512 // Dh, Dh=Dh) == kc.FP8_ROWS
        assert _attn(H=512 // Dh, Dh=Dh, group=1) == kc.FP8_ROWS
        assert _attn(H=3, Dh=Dh) == kc.FP8_BH
    assert _attn(H=4, Dh=64) == kc.FP8_BH and _attn(H=16, Dh=64) == kc.FP8_BH
    assert _attn(scale_batch=8) == kc.FP8_ROWS                # scale_batch = H: K and V scales in two arrays
    assert _attn(R=0) == kc.FP8_ROWS                         # planned, though nothing is launched
    assert _attn(v_scale=BASE + 0x80000C, H=3, Dh=16) == kc.FP8_BH   # scales need 4-B alignment only
    for c in kc.ACASES:
        assert _attn(R=c.R, H=c.H, Dh=c.Dh, Lk=c.Lk, group=c.group) == c.family, c.id


ATTN_REJECTIONS = [
    ("null-q", dict(q=None), b"null pointer"), ("null-k", dict(k=None), b"null pointer"),
    ("null-v", dict(v=None), b"null pointer"), ("null-o", dict(o=None), b"null pointer"),
    ("null-k-scale", dict(k_scale=None), b"null pointer"), ("null-v-scale", dict(v_scale=None), b"null pointer"),
    ("heads-zero", dict(H=0), b"bad extents"), ("rows-negative", dict(R=-3), b"bad extents"),
    ("scale-batch-short", dict(scale_batch=7), b"scale_batch"), ("scale-batch-negative", dict(scale_batch=-16), b"scale_batch"),
    ("head-dim-48", dict(Dh=48), b"head_dim"), ("lk-zero", dict(Lk=0), b"Lk > 0"), ("lk-negative", dict(Lk=-3), b"Lk > 0"),
    ("group-zero", dict(group=0), b"group"), ("rows-not-whole-groups", dict(R=7), b"whole groups"),
    ("q-misaligned", dict(q=BASE + 8), b"16-B aligned"), ("k-misaligned", dict(k=BASE + 0x10008), b"16-B aligned"),
    ("v-misaligned", dict(v=BASE + 0x10204), b"16-B aligned"), ("o-misaligned", dict(o=BASE + 0x900008), b"16-B aligned"),
    ("q-batch-odd", dict(q_batch=516), b"16-B aligned"), ("k-row-odd", dict(k_row=1032), b"16-B aligned"),
    ("k-batch-odd", dict(k_batch=0x40008), b"16-B aligned"), ("v-row-odd", dict(v_row=1028), b"16-B aligned"),
    ("v-batch-odd", dict(v_batch=0x40001), b"16-B aligned"), ("o-batch-odd", dict(o_batch=516), b"16-B aligned"),
    ("scale-misaligned", dict(k_scale=BASE + 0x800002), b"4-B aligned"),
]


@pytest.mark.parametrize("rid,change,frag", ATTN_REJECTIONS, ids=[r[0] for r in ATTN_REJECTIONS])
def test_attention_fp8_rejections(rid, change, frag):
    lib = native.load_library()
    assert _attn(**change) == -1
    assert frag in lib.mit_last_error()
    assert _attn(fn="launch", **change) == 1                 # the entry point: same decision, nothing launched
    assert frag in lib.mit_last_error()


# ------------------------------------------------------------------------------------------------
# mit_kv_quantize_fp8 rejections
# ------------------------------------------------------------------------------------------------
def _quant(**kw):
    a = dict(B=2, S=197, G=16, Dh=64, src=BASE, s_row=1024, s_batch=197 * 1024, dst=BASE + 0x1000000, d_row=1024,
             d_batch=197 * 1024, scales=BASE + 0x2000000)
    a.update(kw)
    return native.lib().mit_kv_quantize_fp8(a["B"], a["S"], a["G"], a["Dh"], a["src"], a["s_row"], a["s_batch"], a["dst"],
                                            a["d_row"], a["d_batch"], a["scales"], None)


QUANT_REJECTIONS = [
    ("null-src", dict(src=None), b"null pointer"), ("null-dst", dict(dst=None), b"null pointer"),
    ("null-scales", dict(scales=None), b"null pointer"), ("head-dim-24", dict(Dh=24), b"head_dim"),
    ("B-negative", dict(B=-1), b"bad extents"), ("G-zero", dict(G=0), b"bad extents"),
    ("src-misaligned", dict(src=BASE + 8), b"16-B aligned"), ("dst-misaligned", dict(dst=BASE + 0x1000008), b"16-B aligned"),
    ("s-row-odd", dict(s_row=1028), b"16-B aligned"), ("s-batch-odd", dict(s_batch=197 * 1024 + 4), b"16-B aligned"),
    ("d-row-odd", dict(d_row=1032), b"16-B aligned"), ("d-batch-odd", dict(d_batch=197 * 1024 + 8), b"16-B aligned"),
    ("scales-misaligned", dict(scales=BASE + 0x2000002), b"4-B aligned"),
]


@pytest.mark.parametrize("rid,change,frag", QUANT_REJECTIONS, ids=[r[0] for r in QUANT_REJECTIONS])
def test_quantize_fp8_rejections(rid, change, frag):
    lib = native.load_library()
    assert _quant(**change) == 1
    assert frag in lib.mit_last_error()


def test_empty_calls_launch_nothing():
    native.load_library()
    assert _quant(B=0) == 0 and _quant(S=0) == 0             # no GPU here: a launch would fail
    assert _attn(fn="launch", R=0) == 0


# ------------------------------------------------------------------------------------------------
# resolve_kv_dtype, the command line, generate_captions
# ------------------------------------------------------------------------------------------------
def test_resolve_kv_dtype(monkeypatch):
    from decoder import resolve_kv_dtype
    monkeypatch.delenv("MIT_DECODE_KV", raising=False)
    assert resolve_kv_dtype() == "bf16" and resolve_kv_dtype(None) == "bf16"
    assert resolve_kv_dtype("fp8") == "fp8" and resolve_kv_dtype("bf16") == "bf16"
    assert resolve_kv_dtype(None, torch.float32) == "bf16" and resolve_kv_dtype("bf16", torch.float32) == "bf16"
    monkeypatch.setenv("MIT_DECODE_KV", "fp8")
    assert resolve_kv_dtype() == "fp8"
    assert resolve_kv_dtype("bf16") == "bf16"                 # the argument wins
    monkeypatch.setenv("MIT_DECODE_KV", "int4")
    with pytest.raises(ValueError, match="int4"):
        resolve_kv_dtype()
    assert resolve_kv_dtype("fp8") == "fp8"
    monkeypatch.delenv("MIT_DECODE_KV")
    with pytest.raises(ValueError, match="fp16"):
        resolve_kv_dtype("fp16")
    with pytest.raises(ValueError, match="bfloat16 decoder"):
        resolve_kv_dtype("fp8", torch.float32)
    monkeypatch.setenv("MIT_DECODE_KV", "fp8")
    with pytest.raises(ValueError, match="float32"):
        resolve_kv_dtype(None, torch.float32)


def test_command_line_carries_kv_dtype():
    import inference
    ap = inference.build_parser()
    base = ["--image_path", "a.png", "--checkpoint_path", "c.pt"]
    assert "kv_dtype" not in inference.decode_options(ap.parse_args(base))
    assert inference.decode_options(ap.parse_args(base + ["--kv_dtype", "fp8"]))["kv_dtype"] == "fp8"
    assert inference.decode_options(ap.parse_args(base + ["--kv_dtype", "bf16"]))["kv_dtype"] == "bf16"
    with pytest.raises(SystemExit):
        ap.parse_args(base + ["--kv_dtype", "int8"])


class _Stub:
    device = "cpu"

    def __init__(self):
        self.calls = []

    def generate_batch(self, chunk, start, end, **kw):
        self.calls.append(("greedy", kw))
        return [[start, 7, end]] * chunk.shape[0]

    def generate_beam_batch(self, chunk, start, end, **kw):
        self.calls.append(("beam", kw))
        return [[start, 8, end]] * chunk.shape[0]

    def generate_sample_batch(self, chunk, start, end, **kw):
        self.calls.append(("sample", kw))
        return [[start, 9, end]] * chunk.shape[0]


@pytest.mark.parametrize("extra,kind", [({}, "greedy"), (dict(beam_size=3), "beam"), (dict(temperature=0.8), "sample")])
def test_generate_captions_passes_kv_dtype_on(extra, kind):
    import inference
    imgs = torch.zeros(3, 3, 4, 4)
    m = _Stub()
    inference.generate_captions(m, imgs, start_token_id=2, end_token_id=3, max_len=9, batch_size=2, kv_dtype="fp8", **extra)
    assert [k for k, _ in m.calls] == [kind, kind] and all(kw["kv_dtype"] == "fp8" for _, kw in m.calls)
    m = _Stub()
    inference.generate_captions(m, imgs, start_token_id=2, end_token_id=3, max_len=9, **extra)
    assert [k for k, _ in m.calls] == [kind] and "kv_dtype" not in m.calls[0][1]     # absent when not given
