"""The contract of csrc/kv8.hip (include/mit_hip.h: mit_kv_quantize_fp8, mit_attention_decode_fp8 and its plan query):
the CPU reference quantiser / dequantiser written from the header's formula, and the case tables and guarded buffers
of tests/test_kv8_contract_cpu.py and tests/test_kv8_gpu.py. Buffers, guards, NaN poison, SENTINEL and the float
measure are decode_contract's / gemm_contract's (imported, not copied).

Numerics. A scale is a power of two and e4m3 has 4 significant bits, so byte * scale is exact in bf16: the quantised
attention is the bf16 attention on the dequantised values. The attention outputs are therefore measured against
decode_contract's float64 reference (beam_contract.gathered_attention: the same formula with the `group` rows of an
image on one K / V) evaluated on the dequantised values, in decode_contract's attn unit and within its BOUND["attn"];
no tolerance of this file's own. The quantiser is exact: bytes and scales bitwise.

Poison. K / V bytes outside their windows (pad columns, rows j >= Lk, the gaps between images, margins) hold 0x7F,
which decodes to NaN; scales outside their windows and q outside its window are NaN; o holds SENTINEL."""
import math
from dataclasses import dataclass

import torch

import beam_contract as bc
import decode_contract as dc
from decode_contract import BOUND, Arr, check_float  # noqa: F401  (re-exported to the tests)
from gemm_contract import GUARD, NAN, SENTINEL  # noqa: F401

FP8_BH, FP8_ROWS = 3, 4          # mit_attention_decode_fp8_plan (MIT_DECODE_ATTN_FP8_*)
E4M3_MAX = 448.0
E4M3_MIN_NORMAL = 2.0 ** -6
NAN_BYTE = 0x7F                  # e4m3fn NaN (0xFF with the sign)


# ------------------------------------------------------------------------------------------------
# the reference quantiser
# ------------------------------------------------------------------------------------------------
def quantize_ref(x):
    """x bf16 [B, S, G, Dh] -> (bytes uint8 [B, S, G, Dh], scales f32 [B, G]), the header's formula: per (b, g)
    amax = max |x| = m 2^X with m in [1, 2); e = X - 8 if m <= 1.75 else X - 7, clamped to [-64, 64], 0 for amax = 0;
    scale = 2^e; byte = e4m3fn_rne(x 2^-e)."""
    assert x.dtype == torch.bfloat16 and x.dim() == 4
    xf = x.float()
    amax = xf.abs().amax(dim=(1, 3))                        # [B, G]
    m, ex = torch.frexp(amax)                               # amax = m 2^ex, m in [0.5, 1)
    e = torch.where(2 * m <= 1.75, ex - 9, ex - 8).clamp(-64, 64)
    e = torch.where(amax == 0, torch.zeros_like(e), e)
    one = torch.ones_like(amax)
    scale, inv = torch.ldexp(one, e), torch.ldexp(one, -e)
    q = (xf * inv[:, None, :, None]).to(torch.float8_e4m3fn).view(torch.uint8)
    return q, scale


def dequantize_ref(q, scale):
    """bytes [B, S, G, Dh], scales [B, G] -> float64 values (each exact in bf16)"""
    return q.view(torch.float8_e4m3fn).double() * scale.double()[:, None, :, None]


def gaussian_groups(sigma, B, S, G, Dh, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, S, G, Dh, generator=g) * sigma).to(torch.bfloat16)


SIGMAS = (1e-3, 0.03, 1.0, 37.0, 1e4)
GROUP_SHAPES = ((1, 16), (197, 64), (7, 128))   # (S, Dh)


class Arr8(Arr):
    """An Arr of bytes: its bit view is the tensor itself (gemm_contract's integer views start at 2 bytes)."""

    def bits(self, t=None):
        return self.whole if t is None else t

    def to(self, device):
        a = Arr8(self.n, self.dtype, 0, self.margin, self.misalign, device)
        a.whole.copy_(self.whole)
        a.allowed = self.allowed
        return a


# ------------------------------------------------------------------------------------------------
# mit_kv_quantize_fp8: cases and buffers
# ------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class QCase:
    B: int
    S: int
    G: int
    Dh: int
    s_pad: int = 16      # pad columns of a src row (elements)
    d_pad: int = 32      # pad columns of a dst row (bytes)
    gap: int = 2         # rows between two images, in both buffers

    @property
    def id(self):
        return f"q-B{self.B}-S{self.S}-G{self.G}-Dh{self.Dh}"


QCASES = [QCase(1, 1, 2, 16), QCase(3, 7, 4, 32), QCase(2, 65, 16, 64), QCase(2, 197, 16, 64), QCase(1, 9, 2, 128)]
Q_BY_ID = {c.id: c for c in QCASES}


def quant_input(c, seed=0):
    """bf16 [B, S, G, Dh]: Gaussian groups whose magnitudes spread over 2^-10 .. 2^13, group (0, 0) with amax exactly
    448 * 2^3 (the m <= 1.75 edge: e = 3, the largest byte 0x7E) and two values that land in e4m3's subnormals,
    group (B-1, G-1) all zero (with a -0), and a -0 in a non-zero group."""
    g = torch.Generator().manual_seed(1000 + seed + c.S * 7 + c.G)
    x = torch.randn(c.B, c.S, c.G, c.Dh, generator=g)
    ex = torch.randint(-10, 14, (c.B, 1, c.G, 1), generator=g)
    x = (x * torch.ldexp(torch.ones(()), ex)).to(torch.bfloat16)
    x[0, :, 0] = x[0, :, 0].float().clamp(-3000, 3000).to(torch.bfloat16)
    x[0, c.S // 2, 0, 3] = -3584.0                          # 448 * 2^3
    x[0, 0, 0, 5] = 2.0 ** -5                               # / 2^3 = 2^-8: an e4m3 subnormal, exact
    x[0, 0, 0, 6] = 1.5 * 2.0 ** -6                         # / 2^3 = 1.5 * 2^-9: a subnormal tie, to even (2^-8)
    if c.B * c.G > 1:
        x[c.B - 1, :, c.G - 1] = 0.0
        x[c.B - 1, 0, c.G - 1, 1] = -0.0
    x[0, 0, 0, 7] = -0.0
    return x


def make_quant(c, seed=0):
    """(tensors, geometry): src bf16 NaN outside its windows, dst bytes SENTINEL-like 0xA5 outside its windows
    (allowed: exactly the G*Dh bytes of each of the S rows of each image), scales f32 [B, G] between NaN margins."""
    x = quant_input(c, seed)
    W = c.G * c.Dh
    s_row, d_row = W + c.s_pad, W + c.d_pad
    s_batch, d_batch = (c.S + c.gap) * s_row, (c.S + c.gap) * d_row
    t = dc.Tensors()
    src = t.new("src", c.B * s_batch, torch.bfloat16, NAN, margin=s_row)
    dst = t.a["dst"] = Arr8(c.B * d_batch, torch.uint8, 0xA5, margin=d_row)
    sc = t.new("scales", c.B * c.G, torch.float32, NAN, margin=8)
    for b in range(c.B):
        src.win(b * s_batch, c.S, W, s_row).copy_(x[b].reshape(c.S, W))
        dst.allow(b * d_batch, c.S, W, d_row)
    sc.allow(0, 1, c.B * c.G, c.B * c.G)
    t.x.update(x=x, W=W, s_row=s_row, d_row=d_row, s_batch=s_batch, d_batch=d_batch)
    return t


def launch_quant(N, c, t):
    X = t.x
    return N.lib().mit_kv_quantize_fp8(c.B, c.S, c.G, c.Dh, t.ptr("src"), X["s_row"], X["s_batch"], t.ptr("dst"),
                                       X["d_row"], X["d_batch"], t.ptr("scales"), N.stream_ptr())


def check_quant(c, t):
    """bytes and scales bitwise the reference's; guards and inputs untouched"""
    X = t.x
    want_q, want_s = quantize_ref(X["x"])
    dst, sc = t.a["dst"], t.a["scales"]
    whole = dst.whole.cpu()
    for b in range(c.B):
        got = whole.as_strided((c.S, X["W"]), (X["d_row"], 1), dst.off + b * X["d_batch"])
        assert torch.equal(got, want_q[b].reshape(c.S, X["W"])), \
            f"{c.id}: image {b}: {int((got != want_q[b].reshape(c.S, X['W'])).sum())} byte(s) differ from the reference"
    got_s = sc.whole.cpu()[sc.off:sc.off + c.B * c.G].view(c.B, c.G)
    assert torch.equal(got_s.view(torch.int32), want_s.view(torch.int32)), f"{c.id}: scales {got_s} != {want_s}"
    for k, a in t.a.items():
        a.check(f"{c.id}: {k}")


# ------------------------------------------------------------------------------------------------
# mit_attention_decode_fp8: cases and buffers
# ------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class ACase:
    H: int
    Dh: int
    R: int
    group: int
    Lk: int
    hot: bool = False
    state: bool = False      # the strides of the real decode state: rows of exactly 2d bytes, images back to back

    @property
    def family(self):
        return FP8_ROWS if self.H * self.Dh == 512 else FP8_BH

    @property
    def id(self):
        return (f"{'rows' if self.family == FP8_ROWS else 'bh'}-H{self.H}-Dh{self.Dh}-R{self.R}-g{self.group}-Lk{self.Lk}"
                + ("-hot" if self.hot else "") + ("-state" if self.state else ""))


def _acases():
    cs = []
    # ROWS: one wave only (1, 8), exactly one block per wave (64), a ragged last block (63, 65), two register
    # buffers in use (197)
    for Dh in (16, 64, 128):
        for Lk in (1, 8, 63, 64, 65, 197):
            for R, group in ((1, 1), (6, 1), (6, 3)):
                cs.append(ACase(512 // Dh, Dh, R, group, Lk))
    for H, Dh in ((2, 16), (3, 32), (2, 128)):
        for Lk in (1, 5, 70):
            for R, group in ((3, 1), (4, 2)):
                cs.append(ACase(H, Dh, R, group, Lk))
    cs.append(ACase(8, 64, 2, 1, 70, hot=True))
    cs.append(ACase(3, 32, 2, 1, 70, hot=True))
    cs.append(ACase(8, 64, 6, 3, 197, state=True))
    cs.append(ACase(3, 16, 4, 2, 10, state=True))
    return cs


ACASES = _acases()
A_BY_ID = {c.id: c for c in ACASES}
assert len(A_BY_ID) == len(ACASES)


def attn_inputs(c, seed=0):
    """q bf16 [R, H, Dh]; K8, V8 bytes [images, Lk, H, Dh] and their scales [images, H] from the reference quantiser.
    Head (b, h)'s K and V magnitudes are 2^a and 2^b with a, b walking over the 15 exponents that put the scales
    on 2^-9 .. 2^5; q of that head is scaled by 2^-a, so the scores stay those of unit Gaussians."""
    images = c.R // c.group
    g = torch.Generator().manual_seed(77 + seed + 1000 * c.Lk + 10 * c.H + c.group)
    idx = torch.arange(images * c.H).view(images, c.H)
    ka, va = (idx * 4 + 1) % 15 - 2, (idx * 7 + 5) % 15 - 2           # magnitudes 2^-2 .. 2^12
    two = lambda e: torch.ldexp(torch.ones(()), e)                      # noqa: E731
    q = torch.randn(c.R, c.H, c.Dh, generator=g) * two(-ka).repeat_interleave(c.group, 0)[..., None]
    K = torch.randn(images, c.Lk, c.H, c.Dh, generator=g) * two(ka)[:, None, :, None]
    V = torch.randn(images, c.Lk, c.H, c.Dh, generator=g) * two(va)[:, None, :, None]
    q = q.to(torch.bfloat16)
    if c.hot:   # attn-bhf32-hot-first: key 0 scores about 100, key 1 about 99, every other key about N(0, 1)
        assert c.group == 1 and c.Lk >= 2
        qd = q.double()
        a = 100.0 / (c.Dh ** -0.5 * (qd * qd).sum(-1))
        for jj, f in ((0, 1.0), (1, 0.99)):
            K[:, jj] = (qd * (a * f)[..., None]).float()
    K8, ks = quantize_ref(K.to(torch.bfloat16))
    V8, vs = quantize_ref(V.to(torch.bfloat16))
    return q, K8, ks, V8, vs


def make_attn(c, seed=0, repeat=False):
    """Guarded buffers of a case. repeat: the K / V bytes and scales physically repeated per row, for a group = 1
    call that must equal the group = c.group call."""
    q, K8, ks, V8, vs = attn_inputs(c, seed)
    group = c.group
    if repeat:
        K8, V8 = K8.repeat_interleave(group, 0), V8.repeat_interleave(group, 0)
        ks, vs = ks.repeat_interleave(group, 0), vs.repeat_interleave(group, 0)
        group = 1
    images, W, H = c.R // group, c.H * c.Dh, c.H
    extra, gap, pad, spad, opad, qpad = (0, 0, 0, 0, 0, 0) if c.state else (3, 1, 16, 4, 8, 16)
    row = 2 * W + pad                                   # K | V | pad, V at k + W
    kv_batch = (c.Lk + extra + gap) * row
    q_batch, o_batch, scale_batch = W + qpad, W + opad, 2 * H + spad
    t = dc.Tensors()
    qa = t.new("q", c.R * q_batch, torch.bfloat16, NAN, margin=q_batch)
    qa.win(0, c.R, W, q_batch).copy_(q.reshape(c.R, W))
    kv = t.a["kv"] = Arr8(images * kv_batch, torch.uint8, NAN_BYTE, margin=row)
    sc = t.new("scales", images * scale_batch, torch.float32, NAN, margin=scale_batch)
    for b in range(images):
        kv.win(b * kv_batch, c.Lk, W, row).copy_(K8[b].reshape(c.Lk, W))
        kv.win(b * kv_batch + W, c.Lk, W, row).copy_(V8[b].reshape(c.Lk, W))
    sc.win(0, images, H, scale_batch).copy_(ks)
    sc.win(H, images, H, scale_batch).copy_(vs)
    o = t.new("o", c.R * o_batch, torch.bfloat16, SENTINEL, margin=o_batch)
    o.allow(0, c.R, W, o_batch)
    t.x.update(q=q, K8=K8, ks=ks, V8=V8, vs=vs, W=W, row=row, kv_batch=kv_batch, q_batch=q_batch, o_batch=o_batch,
               scale_batch=scale_batch, group=group, scale=dc.f32r(c.Dh ** -0.5))
    return t


def attn_args(c, t):
    """the arguments of mit_attention_decode_fp8(_plan) up to `group`, in order"""
    X = t.x
    return (c.R, c.H, c.Dh, t.ptr("q"), X["q_batch"], t.ptr("kv"), X["row"], X["kv_batch"], t.ptr("kv", X["W"]), X["row"],
            X["kv_batch"], t.ptr("scales"), t.ptr("scales", c.H), X["scale_batch"], t.ptr("o"), X["o_batch"], c.Lk,
            X["group"])


def launch_attn(N, c, t):
    return N.lib().mit_attention_decode_fp8(*attn_args(c, t), t.x["scale"], N.stream_ptr())


def attn_output(c, t):
    o = t.a["o"]
    return o.whole.cpu().as_strided((c.R, t.x["W"]), (t.x["o_batch"], 1), o.off)


def reference_attn(c, t):
    """(o [R, W] float64, unit [R, W]): decode_contract's float64 attention and unit on the dequantised values"""
    X = t.x
    Kd, Vd = dequantize_ref(X["K8"], X["ks"]), dequantize_ref(X["V8"], X["vs"])
    return bc.gathered_attention(X["q"].double(), Kd, Vd, c.Lk, X["group"], None, None, 0, X["scale"])


def check_attn(c, t):
    """the attn figure of the case (decode_contract.check_float), after the guards"""
    for k, a in t.a.items():
        a.check(f"{c.id}: {k}")
    ref, unit = reference_attn(c, t)
    assert not torch.isnan(ref).any()
    figs = []
    check_float(c.id, "attn", attn_output(c, t), ref, unit, True, figs)
    return figs[0][2]


if __name__ == "__main__":
    for c in QCASES:
        q, s = quantize_ref(quant_input(c))
        print(c.id, "scale exponents", sorted({int(math.log2(v)) for v in s.flatten().tolist()}))
    print(len(ACASES), "attention cases")
