"""The memory and mask contract of mit_attention_fwd / mit_attention_bwd (include/mit_hip.h), as a case table and
a harness, in the manner of tests/gemm_contract.py (whose `strided` buffers and bitwise comparison it reuses).

Every operand and output of a case lives in a guarded buffer (`ABuf`): a 64-element head guard, the live span
(the batches at their batch stride, plus one more row), a 64-element tail guard. A case's `layout` names, per
tensor, the buffer, the column offset, the row stride and the batch stride (`regions`): q/k/v as column slices
of one [B*T, 3*H*Dh] buffer (the decoder's and encoder's self-attention), K/V as layer 1 of a three-layer
[B*S, 3*2*H*Dh] buffer (the decoder's cross-attention), both again with 16 rows between the batches, padded rows
of different widths per tensor ("sep"), and four layouts that fail the MFMA kernels' alignment rules. dk and dv
are always strided views of one buffer. Inputs are NaN outside their windows (pad columns, rows between
batches, the row after the last, guards; a kernel that loads one and relies on p = 0 to cancel it fails:
0 * NaN = NaN), the other layers of a shared K/V buffer are finite, outputs hold a finite sentinel, key_tokens
outside the window are live tokens. K and V rows of padded keys hold +-1e4: a masked key that leaks cannot pass.

`reference` evaluates the header's formula in float64 on the CPU from the dtype-rounded windows (mask rule, lse,
dropout through the mask mit_dropout_mask gives, gradients in closed form), `check_fwd` / `check_bwd` compare
per (batch, head) slice and verify the exact properties (zero dk / dv at padded and unseen keys, nothing written
outside an output's windows, no input written), `fake_attention` is a torch implementation of the same contract
on the same buffers with a bf16-emulation mode and injectable faults (tests/test_attn_contract_cpu.py shows each
fault is caught without a GPU).

Bounds, per (batch, head) slice against max(max|ref| of the slice, 1e-3), those of test_attention_fwd_bwd:
  bf16: o 2e-2, lse 1e-3, dq / dk / dv 4e-2;  f32: o 1e-4, lse 1e-5, dq / dk / dv 2e-4.
"""
import zlib
from dataclasses import dataclass

import torch

import gemm_contract as gc
from gemm_contract import GUARD, NAN, SENTINEL

_TORCH = {"bf16": torch.bfloat16, "f32": torch.float32}
PAD_IDX = 0
LIVE_TOKEN = 7
BIG = 1.0e4
TOL = {"bf16": dict(o=2e-2, lse=1e-3, grad=4e-2), "f32": dict(o=1e-4, lse=1e-5, grad=2e-4)}
FWD_FAMILIES = ("generic", "mfma", "head", "head_drop")  # mit_attn_plan.fwd 0..3
BWD_FAMILIES = ("generic", "mfma", "head")               # mit_attn_plan.bwd 0..2
# csrc/attention.hip's dispatch constants
HK_MAX, HB_MAXK, HEAD8_LKP = 640, 256, 320


# ------------------------------------------------------------------------------------------------
# the case table
# ------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    id: str
    Lq: int
    Lk: int
    fwd: str            # the forward family the case is meant to run (FWD_FAMILIES)
    bwd: str = None     # the backward family (BWD_FAMILIES); None: forward only
    nw: int = 0         # attn_fwd_head: waves per workgroup and staged key rows (0 for the other families)
    lkp: int = 0
    dtype: str = "bf16"
    Dh: int = 64
    causal: bool = False
    pad: str = None     # key padding pattern (_tokens); None: no key_tokens
    drop_p: float = 0.0
    layout: str = "sep"
    hot: str = None     # first | mid | tail: where the two keys that outscore the rest by ~100 sit
    qscale: float = 1.0
    index_limit: float = 0.0  # mit_attention_set_index_limit for the case
    B: int = 2
    H: int = 3
    site: int = 5

    @property
    def W(self):
        return self.H * self.Dh

    @property
    def scale(self):
        return self.Dh ** -0.5

    @property
    def bwd_lkp(self):
        return (self.Lk + 31) // 32 * 32 if self.bwd == "head" else 0


def _bwd_of(Lq, Lk):
    return "head" if Lq <= 64 and Lk <= HB_MAXK else "mfma"


def _build_cases():
    cs = []

    def add(id, Lq, Lk, fwd, bwd="auto", **kw):
        if bwd == "auto":
            bwd = _bwd_of(Lq, Lk)
        cs.append(Case(id, Lq, Lk, fwd, bwd, **kw))

    # ---- attn_fwd_head (no mask, Lk <= 640): nw = min(ceil(Lq / 16), 8 if lkp <= 320 or dropout else 16) ----
    for Lq, Lk, nw, lkp in [(1, 1, 1, 16), (17, 15, 2, 16), (16, 16, 1, 16), (63, 65, 4, 80),  # smallest, ragged
                            (33, 150, 3, 160),    # two chunks and a 32-key tail
                            (20, 300, 2, 304),    # four chunks and a 48-key tail
                            (64, 320, 4, 320),    # the last lkp at which the workgroup is capped at 8 waves
                            (129, 320, 8, 320),   # ... with 9 query tiles over those 8
                            (65, 321, 5, 336),    # lkp = 336: the cap is 16
                            (129, 321, 9, 336),   # ... and a ninth wave runs
                            (272, 336, 16, 336),  # 17 query tiles over 16 waves
                            (20, 640, 2, 640)]:   # HK_MAX
        add(f"head-{Lq}x{Lk}", Lq, Lk, "head", nw=nw, lkp=lkp)
    add("head-drop-63x65", 63, 65, "head_drop", nw=4, lkp=80, drop_p=0.1)
    add("head-drop-129x321", 129, 321, "head_drop", nw=8, lkp=336, drop_p=0.1)  # dropout: 8 waves at any lkp
    add("head-drop-64x256", 64, 256, "head_drop", nw=4, lkp=256, drop_p=0.1)    # attn_bwd_head at both its limits
    add("idx64-drop-63x65", 63, 65, "generic", "mfma", drop_p=0.1, index_limit=1.0)  # 64-bit mask indices
    # ---- attn_fwd_mfma ----
    add("mfma-63x641", 63, 641, "mfma")  # past HK_MAX
    for L in (63, 65, 130):
        add(f"mfma-causal-{L}x{L}", L, L, "mfma", causal=True)
    add("mfma-causal-40x70", 40, 70, "mfma", causal=True)  # keys 40..69 are seen by no query
    add("mfma-causal-70x40", 70, 40, "mfma", causal=True)
    add("mfma-causal-64x257", 64, 257, "mfma", causal=True)
    add("mfma-tok-63x197", 63, 197, "mfma", pad="trail")
    add("mfma-tok-65x64", 65, 64, "mfma", pad="trail")
    add("mfma-tok-drop-63x577", 63, 577, "mfma", pad="lead", drop_p=0.1)
    add("mfma-tok-63x577", 63, 577, "mfma", pad="holes")
    add("mfma-tok-63x33", 63, 33, "mfma", pad="trail")
    add("mfma-causal-63x32", 63, 32, "mfma", causal=True)
    add("bwd-mfma-65x256", 65, 256, "head", nw=5, lkp=256)  # Lq past attn_bwd_head's 64
    add("bwd-mfma-64x257", 64, 257, "head", nw=4, lkp=272)  # Lk past its 256
    for p in ("trail", "holes", "tile1", "one"):  # three key tiles; key 0 stays live: no row is fully masked
        add(f"mfma-causal-{p}-130x130", 130, 130, "mfma", causal=True, pad=p)
    for p in ("lead", "tile0", "one", "tile1", "holes"):  # four key tiles
        add(f"mfma-{p}-63x197", 63, 197, "mfma", pad=p)
    add("mfma-causal-drop-trail-63x63", 63, 63, "mfma", causal=True, pad="trail", drop_p=0.1)
    # ---- the product's layouts ----
    add("self-causal-trail-63x63", 63, 63, "mfma", causal=True, pad="trail", layout="self")
    add("self+16-causal-trail-63x63", 63, 63, "mfma", causal=True, pad="trail", layout="self+16")
    add("self-80x80", 80, 80, "head", nw=5, lkp=80, layout="self")
    add("self+16-80x80", 80, 80, "head", nw=5, lkp=80, layout="self+16")
    add("cross-63x197", 63, 197, "head", nw=4, lkp=208, layout="cross")
    add("cross+16-63x197", 63, 197, "head", nw=4, lkp=208, layout="cross+16")
    add("cross-tok-63x197", 63, 197, "mfma", pad="trail", layout="cross")
    add("cross+16-tok-63x197", 63, 197, "mfma", pad="trail", layout="cross+16")
    add("cross+16-drop-63x577", 63, 577, "head_drop", nw=4, lkp=592, drop_p=0.1, layout="cross+16")
    # ---- operands off the MFMA kernels' alignment: bf16 head_dim 64 on the generic kernels ----
    add("qrow4-33x70", 33, 70, "generic", "generic", layout="qrow4")    # q_row % 8 == 4
    add("kptr2-33x70", 33, 70, "generic", "generic", layout="kptr2")    # k moved by 2 elements
    add("orow4-33x70", 33, 70, "head", "generic", nw=3, lkp=80, layout="orow4")  # o_row % 8 == 4: fine for the forward
    add("orow4-causal-33x70", 33, 70, "mfma", "generic", causal=True, layout="orow4")
    add("dqrow2-33x70", 33, 70, "head", "generic", nw=3, lkp=80, layout="dqrow2")  # dq_row % 4 == 2
    # ---- generic kernels ----
    for dt, dh in [("bf16", 16), ("bf16", 32), ("bf16", 128), ("f32", 16), ("f32", 32), ("f32", 64), ("f32", 128)]:
        g = dict(dtype=dt, Dh=dh)
        add(f"gen-{dt}-d{dh}-causal-trail", 33, 70, "generic", "generic", causal=True, pad="trail", **g)
        add(f"gen-{dt}-d{dh}-lead-cross+16", 33, 70, "generic", "generic", pad="lead", layout="cross+16", **g)
        add(f"gen-{dt}-d{dh}-drop-cross", 33, 70, "generic", "generic", drop_p=0.1, layout="cross", **g)
    add("gen-f32-d64-self-causal-holes", 70, 70, "generic", "generic", dtype="f32", causal=True, pad="holes", layout="self+16")
    # ---- score range: two keys outscore the rest by ~100 (forward only) ----
    for where in ("first", "mid", "tail"):
        add(f"hot-{where}-head-63x197", 63, 197, "head", None, nw=4, lkp=208, hot=where)
        add(f"hot-{where}-head-20x300", 20, 300, "head", None, nw=2, lkp=304, hot=where)
        add(f"hot-{where}-mfma-63x641", 63, 641, "mfma", None, hot=where)
        add(f"hot-{where}-gen-f32-33x150", 33, 150, "generic", None, dtype="f32", hot=where)
    # ---- scores of standard deviation ~4 (forward and backward) ----
    add("std4-head-63x197", 63, 197, "head", nw=4, lkp=208, qscale=4.0)
    add("std4-mfma-causal-65x130", 65, 130, "mfma", causal=True, qscale=4.0)
    add("std4-gen-f32-33x70", 33, 70, "generic", "generic", dtype="f32", qscale=4.0)
    # ---- a fully masked row: causal, key 0 padded in batch 1 (forward only) ----
    add("row0-mfma-40x70", 40, 70, "mfma", None, causal=True, pad="row0")
    add("row0-gen-f32-40x70", 40, 70, "generic", None, dtype="f32", causal=True, pad="row0")
    add("row0-gen-bf16-d32-40x70", 40, 70, "generic", None, Dh=32, causal=True, pad="row0")
    assert len({c.id for c in cs}) == len(cs)
    return cs


CASES = _build_cases()
BY_ID = {c.id: c for c in CASES}


def _tokens(c):
    """int64 [B, Lk] tokens of the case's padding pattern (PAD_IDX = padded); batch 0 and batch 1 differ."""
    tok = torch.full((c.B, c.Lk), LIVE_TOKEN, dtype=torch.int64)
    Lk = c.Lk
    for b in range(c.B):
        if c.pad == "trail":  # batch 0 keeps every key
            if b > 0:
                tok[b, max(1, (Lk * 3) // 5 - b):] = PAD_IDX
        elif c.pad == "lead":
            tok[b, :min(Lk - 1, 5 + 30 * b)] = PAD_IDX
        elif c.pad == "holes":
            tok[b, 1 + b::3] = PAD_IDX
            tok[b, Lk // 2:Lk // 2 + 9] = PAD_IDX
        elif c.pad == "tile1":
            tok[b, 64:128] = PAD_IDX
            if b > 0:
                tok[b, 130:140] = PAD_IDX
        elif c.pad == "tile0":
            tok[b, :64 + b] = PAD_IDX
        elif c.pad == "one":
            tok[b, :] = PAD_IDX
            tok[b, 0 if c.causal else (Lk - 2 if b == 0 else 70)] = LIVE_TOKEN
        elif c.pad == "row0":
            if b == 1:
                tok[b, 0] = PAD_IDX
                tok[b, 50:] = PAD_IDX
        else:
            raise ValueError(c.pad)
    return tok


def dead_keys(c, tok):
    """bool [B, 1, Lq, Lk]: the header's mask rule (key j of batch b is masked for query i iff j > i under causal
    or key_tokens[b, j] == pad_idx)."""
    dead = torch.zeros(c.B, 1, c.Lq, c.Lk, dtype=torch.bool)
    if c.causal:
        dead |= torch.triu(torch.ones(c.Lq, c.Lk, dtype=torch.bool), diagonal=1)
    if tok is not None:
        dead |= (tok == PAD_IDX)[:, None, None, :]
    return dead


# ------------------------------------------------------------------------------------------------
# layouts and guarded buffers
# ------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Region:
    buf: str
    off: int    # column offset inside a row
    row: int    # row stride
    batch: int  # batch stride
    rows: int   # L


def regions(c):
    """tensor name -> Region, and buffer name -> misalignment in elements, of the case's layout."""
    W, Lq, Lk = c.W, c.Lq, c.Lk
    base, _, plus = c.layout.partition("+")
    extra = int(plus) if plus else 0
    pad = 8 if c.dtype == "bf16" else 3
    r, mis = {}, {}

    def put(name, buf, off, row, rows):
        r[name] = Region(buf, off, row, (rows + extra) * row, rows)

    if base == "self":  # q | k | v column slices of one [B*T, 3W] buffer; o, dq with row stride W
        assert Lq == Lk
        for i, n in enumerate("qkv"):
            put(n, "qkv", i * W, 3 * W, Lq)
        orow = dorow = dqrow = W
    elif base == "cross":  # K | V of layer 1 in a [B*S, 3 * 2W] buffer
        put("q", "q", 0, W, Lq)
        put("k", "kv", 2 * W, 6 * W, Lk)
        put("v", "kv", 3 * W, 6 * W, Lk)
        orow = dorow = dqrow = W
    else:
        assert base in ("sep", "qrow4", "kptr2", "orow4", "dqrow2"), base
        put("q", "q", 0, W + (4 if base == "qrow4" else pad), Lq)
        put("k", "k", 0, W + 2 * pad, Lk)
        put("v", "v", 0, W + 3 * pad, Lk)
        if base == "kptr2":
            mis["k"] = 2
        orow = W + (4 if base == "orow4" else pad)
        dorow = W + 2 * pad
        dqrow = W + (2 if base == "dqrow2" else 3 * pad)
    put("o", "o", 0, orow, Lq)
    put("dout", "dout", 0, dorow, Lq)
    put("dq", "dq", 0, dqrow, Lq)
    put("dk", "dkv", 0, 2 * W + pad, Lk)
    put("dv", "dkv", W, 2 * W + pad, Lk)
    return r, mis


class ABuf:
    """One guarded buffer: whole = flat [GUARD + mis | span | GUARD]; `before` = the snapshot before a launch."""

    def __init__(self, span, dtype, fill, mis=0, device="cpu"):
        self.whole, _ = gc.strided(1, span, span, dtype, fill, mis, device)
        self.base = GUARD + mis
        self.live = torch.zeros(self.whole.numel(), dtype=torch.bool, device=device)  # inside a tensor's window
        self.before = None

    def _strided(self, t, shape, strides, off):
        return t.as_strided(shape, strides, t.storage_offset() + self.base + off)

    def view(self, reg, B, W, more_rows=0, row=None):
        """[B, rows (+ more_rows), W] of the region (row: another row stride, for a fault)"""
        row = row or reg.row
        return self._strided(self.whole, (B, reg.rows + more_rows, W), (reg.batch, row, 1), reg.off)

    def claim(self, reg, B, W):
        self._strided(self.live, (B, reg.rows, W), (reg.batch, reg.row, 1), reg.off).fill_(True)

    def snapshot(self):
        self.before = self.whole.clone()

    def _bits(self, t):
        return t.view(gc._INT[t.element_size()])

    def check_untouched(self, name):
        bad = (self._bits(self.whole) != self._bits(self.before)) & ~self.live
        if bad.any():
            i = int(bad.nonzero()[0])
            raise AssertionError(f"{name}: {int(bad.sum())} element(s) outside the output windows written; first at "
                                 f"{i - self.base} from the first window's start: {self.whole[i].item()} was "
                                 f"{self.before[i].item()}")

    def check_unchanged(self, name):
        assert torch.equal(self._bits(self.whole), self._bits(self.before)), f"{name}: an input buffer was written"


INPUTS = ("q", "k", "v", "dout")
FWD_OUT = ("o", "lse")
BWD_OUT = ("dq", "dk", "dv", "delta")


class Tensors:
    """bufs: name -> ABuf; reg: tensor -> Region; v: tensor -> its [B, L, W] (lse / delta: [B, H, Lq]; tok:
    [B, Lk]) view; seed, drop ([B, H, Lq, Lk] keep-multipliers or None)."""

    def buf_of(self, name):
        return self.bufs[self.reg[name].buf]


def _hot_keys(c):
    Lk = c.Lk
    return {"first": (1, min(14, Lk - 1)), "mid": (Lk // 2, Lk // 2 + 17), "tail": (Lk - 1, Lk - 2)}[c.hot]


def make_tensors(case, device="cpu", mask_fn=None):
    """The guarded buffers of the case, seeded by its id. mask_fn(n, p, seed, site) -> f32 [n] keep-multipliers
    (mit_dropout_mask on the GPU); without it a synthetic Bernoulli mask."""
    c = case
    g = torch.Generator().manual_seed(zlib.crc32(c.id.encode()))
    dt = _TORCH[c.dtype]
    B, H, Dh, W, Lq, Lk = c.B, c.H, c.Dh, c.W, c.Lq, c.Lk
    reg, mis = regions(c)
    outputs = {"o", "dq", "dkv"}
    t = Tensors()
    t.reg, t.bufs, t.v = dict(reg), {}, {}
    spans = {}
    for r in reg.values():  # the batches at their stride plus one more row
        spans[r.buf] = max(spans.get(r.buf, 0), (B - 1) * r.batch + (r.rows + 1) * r.row)
    for name, span in spans.items():
        t.bufs[name] = ABuf(span, dt, SENTINEL if name in outputs else NAN, mis.get(name, 0), device)
    if "kv" in t.bufs:  # the other layers' K | V: finite live data
        b = t.bufs["kv"]
        r = reg["k"]
        allcols = Region("kv", 0, r.row, r.batch, r.rows)
        b.view(allcols, B, r.row).copy_(torch.randn(B, Lk, r.row, generator=g).to(dt))
    q = torch.randn(B, Lq, H, Dh, generator=g) * c.qscale
    k = torch.randn(B, Lk, H, Dh, generator=g)
    v = torch.randn(B, Lk, H, Dh, generator=g)
    dout = torch.randn(B, Lq, H, Dh, generator=g)
    if c.hot:  # even queries see key j0 at ~ +100, odd queries key j1
        j0, j1 = _hot_keys(c)
        s = 1.0 / c.scale  # scale * s * 100 = 100
        q[:, 0::2, :, 0] = s
        q[:, 1::2, :, 1] = s
        k[:, j0, :, 0] = 100.0
        k[:, j1, :, 1] = 100.0
    tok = _tokens(c) if c.pad else None
    if tok is not None:  # padded keys: large finite K and V rows
        padded = tok == PAD_IDX
        sign = torch.where(torch.arange(Dh) % 2 == 0, 1.0, -1.0)
        k[padded] = BIG * sign
        v[padded] = -BIG * sign
    for name, x in (("q", q), ("k", k), ("v", v), ("dout", dout)):
        r = reg[name]
        L = r.rows
        view = t.bufs[r.buf].view(r, B, W)
        view.copy_(x.reshape(B, L, W).to(dt))
        t.v[name] = view
    for name in ("o", "dq", "dk", "dv"):
        r = reg[name]
        t.v[name] = t.bufs[r.buf].view(r, B, W)
        t.bufs[r.buf].claim(r, B, W)
    for name in ("lse", "delta"):
        n = B * H * Lq
        r = Region(name, 0, n, n, 1)
        t.reg[name] = r
        t.bufs[name] = ABuf(2 * n, torch.float32, SENTINEL, 0, device)
        t.v[name] = t.bufs[name].view(r, 1, n).view(B, H, Lq)
        t.bufs[name].claim(r, 1, n)
    t.tok_batch = Lk + 3
    t.tok = None
    if tok is not None:
        r = Region("tok", 0, t.tok_batch, t.tok_batch, 1)
        t.reg["tok"] = r
        t.bufs["tok"] = ABuf(B * t.tok_batch + t.tok_batch, torch.int64, LIVE_TOKEN, 0, device)
        t.v["tok"] = t.bufs["tok"].view(r, B, Lk)[:, 0, :]
        t.v["tok"].copy_(tok)
        t.tok = t.v["tok"]
    t.seed = torch.tensor([1234 + c.site], dtype=torch.int64, device=device)
    t.drop = None
    if c.drop_p > 0:
        n = B * H * Lq * Lk
        if mask_fn is not None:
            m = mask_fn(n, c.drop_p, t.seed, c.site)
        else:
            m = (torch.rand(n, generator=g) >= c.drop_p).float().to(device) / (1.0 - c.drop_p)
        t.drop = m.view(B, H, Lq, Lk)
    return t


def snapshot(t):
    for b in t.bufs.values():
        b.snapshot()


def attn_structs(case, t, native):
    """(AttnArgs, AttnGrads) of the case on its buffers: what mit_attention_fwd / _bwd / _plan are called with.
    On CPU buffers the addresses have the case's alignment and mit_attention_plan dereferences none."""
    c, r, v = case, t.reg, t.v
    a = native.attn_args(v["q"], r["q"].row, r["q"].batch, v["k"], r["k"].row, r["k"].batch, v["v"], r["v"].row,
                         r["v"].batch, v["o"], r["o"].row, r["o"].batch, lse=v["lse"], key_tokens=t.tok,
                         tok_batch=t.tok_batch, pad_idx=PAD_IDX, causal=c.causal, scale=c.scale, drop_p=c.drop_p,
                         seed=t.seed if c.drop_p > 0 else None, site=c.site)
    g = native.attn_grads(v["dout"], r["dout"].row, r["dout"].batch, v["dq"], r["dq"].row, r["dq"].batch, v["dk"],
                          r["dk"].row, r["dk"].batch, v["dv"], r["dv"].row, r["dv"].batch, v["delta"])
    return a, g


def planned(case, t, native):
    """(fwd family, nw, lkp, bwd family, bwd lkp) mit_attention_plan gives for the case's arguments"""
    a, g = attn_structs(case, t, native)
    p = native.attention_plan(native.BF16 if case.dtype == "bf16" else native.F32, case.B, case.H, case.Lq, case.Lk,
                              a, g if case.bwd else None, Dh=case.Dh)
    return (FWD_FAMILIES[p.fwd], p.fwd_nw, p.fwd_lkp, BWD_FAMILIES[p.bwd] if case.bwd else None, p.bwd_lkp)


def declared(case):
    return (case.fwd, case.nw, case.lkp, case.bwd, case.bwd_lkp)


# ------------------------------------------------------------------------------------------------
# the contract
# ------------------------------------------------------------------------------------------------
def _heads(x, H):  # [B, L, H*Dh] -> [B, H, L, Dh]
    B, L, W = x.shape
    return x.reshape(B, L, H, W // H).transpose(1, 2)


def _rows(x):  # [B, H, L, Dh] -> [B, L, H*Dh]
    B, H, L, Dh = x.shape
    return x.transpose(1, 2).reshape(B, L, H * Dh)


def _forward(q, k, v, dead, drop, scale, round_p=False, no_rescale=False):
    """s = scale q k^T (-inf where dead); lse = log sum exp s; P = exp(s - lse); O = (P o M) V. A fully masked row:
    lse = -inf, P and O NaN. Returns (o, lse, p, pd = P o M)."""
    s = ((q @ k.transpose(-1, -2)) * scale).masked_fill(dead, float("-inf"))
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    pd = p if drop is None else p * drop
    if round_p:
        pd = pd.bfloat16().to(p.dtype)
    if not no_rescale:
        return pd @ v, lse, p, pd
    # the fault: an online softmax over 64-key tiles that forgets to rescale what it has when the maximum rises
    m = torch.full(s.shape[:-1], float("-inf"), dtype=s.dtype)
    acc = torch.zeros(*s.shape[:-1], v.shape[-1], dtype=s.dtype)
    l = torch.zeros(s.shape[:-1], dtype=s.dtype)
    for j0 in range(0, s.shape[-1], 64):
        st = s[..., j0:j0 + 64]
        m = torch.maximum(m, st.amax(-1))
        e = torch.exp(st - m[..., None])
        e = torch.where(torch.isnan(e), torch.zeros_like(e), e)
        if drop is not None:
            acc = acc + (e * drop[..., j0:j0 + 64]) @ v[..., j0:j0 + 64, :]
        else:
            acc = acc + e @ v[..., j0:j0 + 64, :]
        l = l + e.sum(-1)
    return acc / l[..., None], m + torch.log(l), p, pd


def _backward(q, k, v, o, dout, p, pd, drop, scale, round_ds=False):
    """dV = (P o M)^T dO; dP = (dO V^T) o M; delta = rowsum(dO o O); dS = P o (dP - delta); dQ = scale dS K;
    dK = scale dS^T Q."""
    dv = pd.transpose(-1, -2) @ dout
    dp = dout @ v.transpose(-1, -2)
    if drop is not None:
        dp = dp * drop
    delta = (dout * o).sum(-1)
    ds = p * (dp - delta[..., None])
    if round_ds:
        ds = ds.bfloat16().to(p.dtype)
    return scale * (ds @ k), scale * (ds.transpose(-1, -2) @ q), dv, delta


def reference(case, t):
    """float64 CPU evaluation from the dtype-rounded windows: o, dq [B, H, Lq, Dh], dk, dv [B, H, Lk, Dh],
    lse, delta [B, H, Lq], dead [B, 1, Lq, Lk]."""
    c = case
    q, k, v, dout = (_heads(t.v[n].detach().cpu().double(), c.H) for n in INPUTS)
    tok = t.tok.cpu() if t.tok is not None else None
    dead = dead_keys(c, tok)
    drop = t.drop.cpu().double() if t.drop is not None else None
    o, lse, p, pd = _forward(q, k, v, dead, drop, c.scale)
    ref = dict(o=o, lse=lse, dead=dead, tok=tok)
    if c.bwd:
        ref["dq"], ref["dk"], ref["dv"], ref["delta"] = _backward(q, k, v, o, dout, p, pd, drop, c.scale)
    return ref


def _close(case, what, got, ref, tol, figures):
    """max|err| <= tol * max(max|ref|, 1e-3) per (batch, head) slice ([B, H, ...]); NaN / -inf exactly where the
    reference has them."""
    got = got.detach().cpu().double()
    nan_r, inf_r = torch.isnan(ref), torch.isinf(ref)
    assert torch.equal(torch.isnan(got), nan_r), \
        f"{case.id} {what}: {int((torch.isnan(got) != nan_r).sum())} element(s) NaN where the reference is not, or not " \
        f"NaN where it is"
    assert torch.equal(got[inf_r], ref[inf_r]), f"{case.id} {what}: not -inf where the reference is"
    special = nan_r | inf_r
    got = torch.where(special, torch.zeros_like(got), got)
    ref = torch.where(special, torch.zeros_like(ref), ref)
    dims = tuple(range(2, ref.dim()))
    err = (got - ref).abs().amax(dims)
    scale = ref.abs().amax(dims).clamp_min(1e-3)
    ratio = (err / scale).max().item()
    print(f"ATTN {case.id} [{case.fwd}/{case.bwd}] {what}: worst slice {ratio:.3e} of max|ref| (bound {tol:g})")
    figures[what] = ratio
    assert ratio <= tol, f"{case.id} {what}: {ratio:.3e} of the slice's max|ref| (bound {tol})"


def check_fwd(case, t, ref):
    """o and lse against the reference; o / lse untouched outside their windows; no input written. Returns the
    measured figures."""
    c, fig = case, {}
    tol = TOL[c.dtype]
    _close(c, "o", _heads(t.v["o"], c.H), ref["o"], tol["o"], fig)
    _close(c, "lse", t.v["lse"], ref["lse"], tol["lse"], fig)
    for name in ("o", "lse"):
        t.buf_of(name).check_untouched(f"{c.id} {name}")
    for name, b in t.bufs.items():
        if name not in ("o", "lse"):
            b.check_unchanged(f"{c.id} {name} (forward)")
    return fig


def check_bwd(case, t, ref):
    """dq / dk / dv / delta against the reference; dk and dv exactly zero at padded keys and at keys no query
    sees; outputs untouched outside their windows; no input (o and lse included) written."""
    c, fig = case, {}
    tol = TOL[c.dtype]
    dk, dv = _heads(t.v["dk"], c.H), _heads(t.v["dv"], c.H)
    unseen = ref["dead"].all(2)[:, 0]  # [B, Lk]: padded, or past the last query under causal
    for name, x in (("dk", dk), ("dv", dv)):
        z = x.detach().cpu().transpose(1, 2)[unseen]  # [n, H, Dh]
        assert (z == 0).all(), f"{c.id} {name}: {int((z != 0).sum())} nonzero element(s) at keys no query sees " \
                               f"(max |{z.abs().max().item():.3e}|)"
    _close(c, "dq", _heads(t.v["dq"], c.H), ref["dq"], tol["grad"], fig)
    _close(c, "dk", dk, ref["dk"], tol["grad"], fig)
    _close(c, "dv", dv, ref["dv"], tol["grad"], fig)
    for name in ("dq", "dk", "delta"):
        t.buf_of(name).check_untouched(f"{c.id} {name}")
    outs = {t.reg[n].buf for n in BWD_OUT}
    for name, b in t.bufs.items():
        if name not in outs:
            b.check_unchanged(f"{c.id} {name} (backward)")
    return fig


def output_bits(t, names):
    return [t.buf_of(n).whole.clone() for n in names]


def same_bits(t, names, first, what):
    for n, w in zip(names, first):
        b = t.buf_of(n)
        assert torch.equal(b._bits(b.whole), b._bits(w)), f"{what}: {n} differs between two identical launches"


# ------------------------------------------------------------------------------------------------
# a torch attention on the guarded buffers with injectable faults (the harness's self-check)
# ------------------------------------------------------------------------------------------------
FAULTS = ("ignore_tokens", "o_row_lq", "dq_row_lq", "kv_row_lk", "dk_at_pad", "no_rescale", "packed_stride")
# the case that must catch each fault
FAULT_CASE = {"ignore_tokens": "cross-tok-63x197", "o_row_lq": "cross+16-63x197", "dq_row_lq": "self-causal-trail-63x63",
              "kv_row_lk": "head-63x65", "dk_at_pad": "mfma-tok-63x33", "no_rescale": "hot-tail-head-63x197",
              "packed_stride": "self-80x80"}


def fault_applies(case, fault):
    c = case
    return {"ignore_tokens": c.pad is not None and not c.causal, "o_row_lq": True, "dq_row_lq": c.bwd is not None,
            "kv_row_lk": True, "dk_at_pad": c.bwd is not None and c.pad is not None, "no_rescale": c.Lk > 64,
            "packed_stride": regions(c)[0]["q"].row != c.W}[fault]


def fake_attention(case, t, emulate_bf16=False, fault=None, backward=False):
    """The contract in torch on the guarded buffers, writing o / lse (backward: dq / dk / dv / delta from the o and
    lse in the buffers) as a kernel would. emulate_bf16: f32 math on the rounded inputs, P o M rounded to bf16
    before PV, o rounded, delta from the rounded o, dS rounded to bf16. `fault` (one of FAULTS) makes it subtly
    wrong in the way a kernel could be."""
    c = case
    assert fault is None or fault_applies(c, fault)
    mt = torch.float32 if emulate_bf16 else torch.float64
    B, H, W = c.B, c.H, c.W
    reg = t.reg

    def load(name):
        r, b = reg[name], t.buf_of(name)
        if fault == "packed_stride" and name == "q":  # the row stride a packed [B, L, W] tensor would have
            return _heads(b.view(r, B, W, row=W).to(mt), H)
        if fault == "kv_row_lk" and name in ("k", "v"):  # one more row, to be cancelled by p = 0
            return _heads(b.view(r, B, W, more_rows=1).to(mt), H)
        return _heads(t.v[name].to(mt), H)

    q, k, v, dout = (load(n) for n in INPUTS)
    tok = t.tok
    if fault == "ignore_tokens":
        tok = None
    dead = dead_keys(c, tok)
    drop = t.drop.to(mt) if t.drop is not None else None
    if fault == "kv_row_lk":
        dead = torch.cat([dead, torch.ones(B, 1, c.Lq, 1, dtype=torch.bool)], -1)
        if drop is not None:
            drop = torch.cat([drop, torch.ones(B, H, c.Lq, 1, dtype=mt)], -1)
    o, lse, p, pd = _forward(q, k, v, dead, drop, c.scale, round_p=emulate_bf16, no_rescale=fault == "no_rescale")
    if not backward:
        t.v["o"].copy_(_rows(o).to(t.v["o"].dtype))
        t.v["lse"].copy_(lse.float())
        if fault == "o_row_lq":  # a 16-row tile's stray row
            t.buf_of("o").view(reg["o"], B, W, more_rows=1)[:, c.Lq, :4] = 1.0
        return
    o = _heads(t.v["o"].to(mt), H)  # what the forward left, rounded
    dq, dk, dv, delta = _backward(q, k, v, o, dout, p, pd, drop, c.scale, round_ds=emulate_bf16)
    if fault == "kv_row_lk":
        dk, dv = dk[:, :, :c.Lk], dv[:, :, :c.Lk]
    for name, x in (("dq", dq), ("dk", dk), ("dv", dv)):
        t.v[name].copy_(_rows(x).to(t.v[name].dtype))
    t.v["delta"].copy_(delta.float())
    if fault == "dq_row_lq":
        t.buf_of("dq").view(reg["dq"], B, W, more_rows=1)[:, c.Lq, :4] = 1.0
    if fault == "dk_at_pad":  # a masked key's gradient that is small rather than zero
        b, j = (t.tok == PAD_IDX).nonzero()[0].tolist()
        t.v["dk"][b, j, 1] = 1e-3 * ref_scale(dk)


def ref_scale(x):
    return float(x.abs().max())
