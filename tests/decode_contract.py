"""The contract of csrc/decode.hip's entry points (include/mit_hip.h) -- mit_attention_decode, mit_kv_store,
mit_embed_decode, mit_greedy_pick / _advance / _keys, mit_decode_gemm, mit_decode_layernorm -- as a case table and a
harness, in the manner of tests/misc_contract.py and tests/ln_contract.py (gemm_contract's guarded `strided` buffers,
GUARD, NAN, SENTINEL and its bitwise comparison).

Buffers. Every operand and output of a case is an `Arr`: [GUARD | margin | data | margin | GUARD] elements, the data
16-B aligned (moved by `misalign` elements where the case is about that). Inputs are NaN everywhere but in their
windows: pad columns, the rows between batches, rows past the last, the margins and the guards; outputs hold SENTINEL.
The margins are at least one row of the buffer's widest stride, so a kernel that is wrong by one row or column reads
poison or writes outside its window, and cannot fault. After a launch every element outside an output's window is
bitwise what it was, and so is every input (pos where it is const, key_tokens, finished rows that were 1). Index
inputs that must not be read point at in-bounds poison: ids columns other than *pos hold the index of a NaN table
row, key_tokens at j >= Lk and between batches hold a live token (so the NaN K / V row behind it would count).

`reference_*` evaluate the header's formulas in float64 from the dtype-rounded windows. `FakeOps` implements the same
contract in torch on the same buffers: mode "f64", or a float32 emulation whose sums are true float32 loops (`fsum`:
"seq" one element after the other, "tree" the kernels' orders: 8-element lane partials and xor trees, per-wave
online-softmax states merged in wave order, per-wave K-step partial tiles), with named injectable faults (FAULTS:
fault -> the cases that must catch it; tests/test_decode_contract_cpu.py).

Units. u = 2^-23. Floating outputs are measured against the float64 reference in conditioning units:
  attn    o[b, h, i]: u (1 + A) sum_j p_j |v_ji|,  A = max over live keys of sum_i |q_i k_ji| scale log2(e) (the
          size of the exp2 argument: its rounding error is relative to it, and exp2 turns it into a relative error of p)
  gemm    C / z_out[m, n]: u (sum_k |a'_k b_nk| + |bias_n| + R), R = |r| (r_mode 1) or (|z - mu| + 2 |mu|) rstd |gamma|
          + |beta| (r_mode 2: the mean carries u |mu|); with the LN operand a' = bf16(LN(z)) the float32 error e_k of
          LN(z)_k (the ln unit below) decides which way a'_k rounds: on average it passes the rounding unchanged,
          + sum_k e_k |b_nk|, and one operand per output may sit on the other side of a bf16 tie than the float64
          reference's, + 2^-8 max_k |a'_k b_nk|
  stats   against the float64 (mean, M2) of the tile of z_out AS WRITTEN: mean u mean_c |v|;
          M2 u sum_c (dv^2 + 2 |dv| (|v| + |mean|)); merged over the row (float64 Chan merge of the written pairs)
          against the row's float64 mean / variance in the sum of the tiles' units
  ln      mit_decode_layernorm out[m, k]: u ((|z - mu| + 2 |mu|) rstd |gamma| + |beta|)
bf16 outputs: only the part of the error past 2^-8 |ref| (the output rounding) is measured.
BOUND[kind] = 4 x the worst float32 FakeOps figure over all cases of the kind and both orders (`python
tests/decode_contract.py` prints them); the factor is ln_contract's: the GPU's exp2f, rsqrtf and MFMA accumulation
order differ from the emulation by a small factor, and no kernel may be sloppier than that.
Exact, no tolerance: kv_store (bitwise copy), embed_decode (the float32 value table * scale + pe, fused or unfused,
in bf16 the round-to-nearest-even of one of the two), every pick, ids / finished / n_finished / pos / ticket, the
argmax keys slot by slot (`pack_key`), the cache row against the bf16 C columns, NaN rows of attention, guards,
inputs, and the second launch against the first.
"""
import math
from dataclasses import dataclass

import torch

import gemm_contract as gc
from gemm_contract import GUARD, NAN, SENTINEL

_TORCH = {"bf16": torch.bfloat16, "f32": torch.float32}
ULP = 2.0 ** -23
BF16_REL = 2.0 ** -8
L2E = 1.4426950408889634
NEG_BIG = -1e30
ATTN_BH, ATTN_ROWS, ATTN_ROWS_NT = 0, 1, 2   # mit_attention_decode_plan
FAMILY = {"bh": ATTN_BH, "rows": ATTN_ROWS, "rows_nt": ATTN_ROWS_NT}
ARGMAX_SLOTS = 16
GRID_CAP = 8192 * 256       # elements one trip of kv_store's / embed_decode's grid-stride loop covers
LDS_LIMIT = 160 * 1024      # bytes of LDS a gfx950 workgroup can have
LIVE_TOK = 7
ACT_NONE, ACT_RELU = 0, 1
INT_SENT = -77              # sentinel of integer outputs

# 4 x the worst float32 FakeOps figure of the kind, in the units above (measured: seq / tree, and the case)
BOUND = {
    "attn": 4 * 0.649,   # 0.649 / 0.533 (attn-bhf32-hot-first)
    "gemm": 4 * 1.572,   # 1.572 / 1.572 (gemm-ln-relu-M63-N1024-K520-Cz, z_out)
    "stats": 4 * 2.578,  # 2.578 (gemm-ln-relu-M63-N1024-K520-Cz, mean) / 1.151 (gemm-ln-relu-M64-N56-K504-Cz, mean)
    "ln": 4 * 0.418,     # 0.418 / 0.418 (ln-M4-W1024)
}


def f32r(x):
    """x as the float32 the C ABI passes"""
    return float(torch.tensor(x, dtype=torch.float32))


def r8(v):
    return (v + 7) // 8 * 8


# ------------------------------------------------------------------------------------------------
# guarded buffers
# ------------------------------------------------------------------------------------------------
class Arr:
    """[GUARD + misalign | margin | n | margin | GUARD] elements filled with `fill`; `base` is the pointer a kernel
    gets (element 0 of the data), windows are (offset, rows, cols, ld) relative to it. `allowed` marks what a launch
    may write (nothing, for an input); `before` is the snapshot taken just before the launch."""

    def __init__(self, n, dtype, fill, margin=0, misalign=0, device="cpu"):
        margin = r8(margin)
        self.n, self.dtype, self.fill, self.margin, self.misalign = n, dtype, fill, margin, misalign
        tot = n + 2 * margin
        self.whole, v = gc.strided(1, tot, tot, dtype, fill, misalign, device)
        self.base = v[0][margin:]
        self.off = GUARD + misalign + margin
        self.allowed = torch.zeros(self.whole.numel(), dtype=torch.bool)
        self.before = None

    @property
    def esz(self):
        return self.whole.element_size()

    def ptr(self, off=0):
        return self.base.data_ptr() + off * self.esz

    def win(self, off, rows, cols, ld):
        return self.base.as_strided((rows, cols), (ld, 1), self.base.storage_offset() + off)

    def bwin(self, off, rows, cols, ld):
        """the window of the pre-launch snapshot, on the CPU"""
        return self.before.as_strided((rows, cols), (ld, 1), self.off + off)

    def allow(self, off, rows, cols, ld):
        assert self.off + off >= GUARD and self.off + off + (rows - 1) * ld + cols <= self.whole.numel() - GUARD
        self.allowed.as_strided((rows, cols), (ld, 1), self.off + off).fill_(True)

    def to(self, device):
        a = Arr(self.n, self.dtype, 0, self.margin, self.misalign, device)
        a.whole.copy_(self.whole)
        a.allowed = self.allowed
        return a

    def snapshot(self):
        self.before = self.whole.detach().cpu().clone()

    def bits(self, t=None):
        return (self.whole if t is None else t).view(gc._INT[self.esz])

    def check(self, name):
        """nothing outside the allowed windows was written"""
        bad = (self.bits().cpu() != self.bits(self.before)) & ~self.allowed
        if bad.any():
            i = int(bad.nonzero()[0])
            kind = "input" if not self.allowed.any() else "output"
            raise AssertionError(f"{name} ({kind}): {int(bad.sum())} element(s) outside its window written; first at "
                                 f"element {i - self.off} of the data ({self.whole[i].item()} was "
                                 f"{self.before[i].item()})")


class Tensors:
    def __init__(self):
        self.a, self.x, self.init = {}, {}, None

    def new(self, name, n, dtype, fill, margin=0, misalign=0):
        self.a[name] = Arr(n, dtype, fill, margin, misalign)
        return self.a[name]

    def to(self, device):
        if device != "cpu":
            self.a = {k: v.to(device) for k, v in self.a.items()}
        self.init = {k: v.whole.clone() for k, v in self.a.items()}
        return self

    def snapshot(self):
        for v in self.a.values():
            v.snapshot()

    def restore(self):
        for k, v in self.a.items():
            v.whole.copy_(self.init[k])

    def ptr(self, name, off=0):
        return self.a[name].ptr(off) if name in self.a else None


# ------------------------------------------------------------------------------------------------
# the case table
# ------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    id: str
    op: str            # attn | kvstore | embed | pick | pickadv | pickkeys | gemm | argmax | ln | chain
    kw: tuple = ()     # ((name, value), ...)

    def __getattr__(self, k):
        d = dict(object.__getattribute__(self, "kw"))
        if k in d:
            return d[k]
        if k in _DEFAULTS:
            return _DEFAULTS[k]
        raise AttributeError(k)


_DEFAULTS = dict(
    dtype="bf16", B=2,
    # attention
    family="bh", H=1, Dh=64, Lk=9, extra=3, mask="none", layout="model", hot=None, qscale=1.0, scale=None, pad_idx=0,
    use_pos=True, o_pad=0, tok_pad=0, gap=0,
    # kv_store / embed_decode
    n=8, pos=0, R=3, s_pad=0, c_pad=0, ids_pad=0,
    # picks
    V=8, ld_pad=0, mis=0, poison=None, n0=5, steps=1, T=6, adv=False,
    # gemm
    M=3, N=64, K=64, a_ln=False, act=ACT_NONE, r_mode=0, c_f32=False, outs="C", bias=True, lda_pad=0, ldb_pad=0,
    ldc_pad=0, ldz_pad=0, ldr_pad=0, cache=None, eps=1e-5, lnkind="plain", stats=False, W=64, ldo_pad=0,
    amode="rand",
)


def kpw(Dh):
    return 512 // Dh


def _mk(cs, id, op, **kw):
    cs.append(Case(id, op, tuple(sorted(kw.items()))))


def _build_cases():
    cs = []
    # ---------------- mit_attention_decode ----------------
    # bh: every (dtype, Dh) at every Lk around the KPW-key slabs of the four waves
    bh_heads = {"bf16": {16: 8, 32: 5, 64: 3, 128: 1}, "f32": {16: 2, 32: 3, 64: 2, 128: 1}}
    for dtype in ("f32", "bf16"):
        for Dh, H in bh_heads[dtype].items():
            k = kpw(Dh)
            for i, Lk in enumerate((1, k - 1, k, k + 1, 4 * k, 4 * k + 1, 8 * k + 3)):
                _mk(cs, f"attn-bh-{dtype}-d{Dh}-h{H}-lk{Lk}", "attn", family="bh", dtype=dtype, H=H, Dh=Dh, Lk=Lk,
                    B=2, mask=("none", "live")[i % 2], use_pos=i % 3 != 2)
    _mk(cs, "attn-bh-f32-d64-h8-w512-lk37", "attn", family="bh", dtype="f32", H=8, Dh=64, Lk=37, B=2)
    # rows / rows_nt: the two-buffer prefetch loop changes shape at Lk = 64 n + 8 w
    for fam in ("rows", "rows_nt"):
        for Dh in (16, 32, 64, 128):
            lks = (1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 192, 193, 197, 257) if Dh == 64 else (9, 65, 129, 197)
            for i, Lk in enumerate(lks):
                _mk(cs, f"attn-{fam}-d{Dh}-lk{Lk}", "attn", family=fam, H=512 // Dh, Dh=Dh, Lk=Lk, B=2,
                    mask=("none", "live")[i % 2], use_pos=fam == "rows",
                    layout="cross" if fam == "rows_nt" else "model")
    # masks on every family
    fams = [("bh", dict(family="bh", dtype="bf16", H=3, Dh=64)), ("bhf32", dict(family="bh", dtype="f32", H=2, Dh=32)),
            ("rows", dict(family="rows", H=8, Dh=64)), ("rows_nt", dict(family="rows_nt", H=4, Dh=128, use_pos=False,
                                                                       layout="cross"))]
    for fn, f in fams:
        slab = 70 if fn != "bhf32" else 150
        for mask, Lk, kw in (("first", 9, {}), ("first64", 70, {}), ("first64", 129, {}), ("slab", slab, {}),
                             ("tail", 21, {}), ("row_all", 13, dict(B=3)), ("pad3", 11, dict(pad_idx=3))):
            _mk(cs, f"attn-{fn}-mask-{mask}-lk{Lk}", "attn", **{**f, "Lk": Lk, "mask": mask, **kw})
    # hot keys, qscale
    for fn, f in fams:
        for hot in ("first", "mid", "last"):
            _mk(cs, f"attn-{fn}-hot-{hot}", "attn", **{**f, "Lk": 77, "hot": hot, "qscale": 3.0, "mask": "live"})
        _mk(cs, f"attn-{fn}-qscale8", "attn", **{**f, "Lk": 41, "qscale": 8.0})
        # layouts and arguments
        _mk(cs, f"attn-{fn}-o-batch-pad", "attn", **{**f, "Lk": 10, "o_pad": 24, "B": 3})
        _mk(cs, f"attn-{fn}-tok-batch-pad", "attn", **{**f, "Lk": 12, "tok_pad": 5, "mask": "tail", "B": 3})
        _mk(cs, f"attn-{fn}-gap16", "attn", **{**f, "Lk": 9, "gap": 16, "B": 3})
        _mk(cs, f"attn-{fn}-scale", "attn", **{**f, "Lk": 19, "scale": 0.3})
        _mk(cs, f"attn-{fn}-B0", "attn", **{**f, "Lk": 5, "B": 0})
    _mk(cs, "attn-bh-cross-layout", "attn", family="bh", dtype="bf16", H=3, Dh=64, Lk=23, layout="cross", use_pos=False)
    _mk(cs, "attn-rows-cross-layout-pos", "attn", family="rows", H=8, Dh=64, Lk=23, layout="cross")
    _mk(cs, "attn-rows_nt-model-layout", "attn", family="rows_nt", H=8, Dh=64, Lk=23, layout="model", use_pos=False)
    _mk(cs, "attn-rows_nt-key-tokens-no-pos", "attn", family="rows_nt", H=8, Dh=64, Lk=75, use_pos=False, mask="tail",
        layout="cross")
    # ---------------- mit_kv_store / mit_embed_decode ----------------
    for dtype in ("bf16", "f32"):
        for i, n in enumerate((8, 100, 1024)):
            for j, pos in enumerate((0, 2, 4)):
                pads = [dict(), dict(s_pad=8), dict(c_pad=16)][(i + j) % 3]
                _mk(cs, f"kvstore-{dtype}-n{n}-pos{pos}" + "".join(f"-{k}" for k in pads), "kvstore", dtype=dtype, n=n,
                    pos=pos, R=5, B=3, **pads)
                _mk(cs, f"embed-{dtype}-d{n}-pos{pos}" + ("-ids-pad" if (i + j) % 2 else ""), "embed", dtype=dtype, n=n,
                    pos=pos, R=5, B=3, ids_pad=3 if (i + j) % 2 else 0)
        _mk(cs, f"kvstore-{dtype}-past-cap-2049x1024", "kvstore", dtype=dtype, n=1024, pos=1, R=2, B=2049)
        _mk(cs, f"embed-{dtype}-past-cap-2049x1024", "embed", dtype=dtype, n=1024, pos=1, R=2, B=2049)
    # ---------------- mit_greedy_pick ----------------
    for V in (1, 3, 4, 5, 255, 256, 257, 1024, 1028, 4096, 4100, 10000, 10001):
        if V % 4 == 0:
            _mk(cs, f"pick-V{V}-vec", "pick", V=V)
            _mk(cs, f"pick-V{V}-vec-ld-pad-inf", "pick", V=V, ld_pad=4, poison="inf")
            _mk(cs, f"pick-V{V}-vec-ld-pad-nan", "pick", V=V, ld_pad=8, poison="nan")
            _mk(cs, f"pick-V{V}-scalar-ld-V+1-nan", "pick", V=V, ld_pad=1, poison="nan")
            _mk(cs, f"pick-V{V}-scalar-ptr-off-1-inf", "pick", V=V, ld_pad=4, mis=1, poison="inf")
        else:
            _mk(cs, f"pick-V{V}-scalar-V%4-inf", "pick", V=V, ld_pad=4 - V % 4, poison="inf")
            _mk(cs, f"pick-V{V}-scalar-V%4-nan", "pick", V=V, ld_pad=8 - V % 4, poison="nan")
    _mk(cs, "pick-V1024-vec-pos-T-2", "pick", V=1024, pos=4, T=6)
    for B in (1, 2, 65, 300):
        _mk(cs, f"pickadv-B{B}", "pickadv", V=260, B=B, adv=True, ld_pad=4, poison="nan")
    _mk(cs, "pickadv-B65-3-steps", "pickadv", V=1024, B=65, adv=True, steps=3, T=8)
    _mk(cs, "pickadv-B2-scalar-pos-T-2", "pickadv", V=257, B=2, adv=True, ld_pad=3, poison="inf", pos=4)
    # ---------------- mit_greedy_pick_keys ----------------
    for B in (1, 1023, 1024, 1025, 2049):
        _mk(cs, f"pickkeys-B{B}", "pickkeys", B=B, V=1088, pos=(0, 4)[B % 2])
    # ---------------- mit_decode_gemm ----------------
    # instantiations: A bf16 x (none r0 | relu r0 | none r1 | none r2), in both launch shapes (K < 512: 4 x 64; else
    # 8 x 32); A LN x (none | relu | f32 C), always 8 x 32
    epis = [("plain", dict()), ("relu", dict(act=ACT_RELU)), ("res", dict(r_mode=1)), ("lnres", dict(r_mode=2))]
    Ms = (1, 31, 32, 33, 63, 64, 65)
    Ns = (8, 56, 64, 72, 136, 1024, 1032)
    i = 0
    for K in (8, 24, 64, 72, 192, 504, 512, 520, 576, 1024, 1088, 1536, 2048):
        for en, e in epis:
            M, N = Ms[i % 7], Ns[(i * 3) % 7]
            if e.get("r_mode") == 2 and N > 1024:
                N = 136
            big = N >= 1024 and K >= 1024
            if big:
                N = (72, 136)[i % 2]     # keeps the case small; N >= 1024 runs with the K <= 576 cases
            outs = ("C", "z", "Cz")[i % 3]
            _mk(cs, f"gemm-{en}-M{M}-N{N}-K{K}-{outs}", "gemm", M=M, N=N, K=K, outs=outs, stats=outs != "C",
                bias=i % 4 != 3, lda_pad=8, ldb_pad=16, ldc_pad=8, ldz_pad=24, ldr_pad=16, **e)
            i += 1
    for K in (8, 24, 64, 72, 192, 504, 512, 520, 1024):
        for en, e in (("ln", dict()), ("ln-relu", dict(act=ACT_RELU)), ("ln-f32", dict(c_f32=True))):
            M, N = Ms[i % 7], Ns[(i * 3) % 7]
            if K >= 1024 and N >= 1024:
                N = 136
            outs = "C" if e.get("c_f32") else ("C", "z", "Cz")[i % 3]
            _mk(cs, f"gemm-{en}-M{M}-N{N}-K{K}-{outs}", "gemm", M=M, N=N, K=K, a_ln=True, outs=outs, stats=outs != "C",
                bias=i % 4 != 3, lda_pad=4, ldb_pad=8, ldc_pad=16, ldz_pad=8,
                lnkind=("plain", "mean50", "tiles")[i % 3], eps=(1e-5, 1e-12)[i % 2], **e)
            i += 1
    # every N and M at least once on each shape of the plain kernel
    for j, N in enumerate(Ns):
        _mk(cs, f"gemm-plain-M{Ms[j]}-N{N}-K72-all-ld", "gemm", M=Ms[j], N=N, K=72, outs="Cz", stats=True, lda_pad=8,
            ldb_pad=8, ldc_pad=8, ldz_pad=8)
        _mk(cs, f"gemm-res-M{Ms[6 - j]}-N{N}-K520", "gemm", M=Ms[6 - j], N=N, K=520, r_mode=1, ldr_pad=8)
    # strides one at a time (dense otherwise), and dense
    for which in ("lda", "ldb", "ldc", "ldz", "ldr", "none"):
        pads = {} if which == "none" else {which + "_pad": 8}
        _mk(cs, f"gemm-res-M33-N72-K72-only-{which}", "gemm", M=33, N=72, K=72, r_mode=1, outs="Cz", stats=True, **pads)
        _mk(cs, f"gemm-lnres-M33-N136-K520-only-{which}", "gemm", M=33, N=136, K=520, r_mode=2, outs="Cz", stats=True,
            lnkind="tiles", **pads)
    _mk(cs, "gemm-ln-M5-N72-K136-only-lda", "gemm", M=5, N=72, K=136, a_ln=True, lda_pad=4, lnkind="tiles")
    _mk(cs, "gemm-plain-M0", "gemm", M=0, N=64, K=64)
    # LayerNorm inputs that give every term weight
    for lnkind in ("mean50", "tiles"):
        for eps in (1e-5, 1e-12):
            _mk(cs, f"gemm-ln-{lnkind}-eps{eps:g}-K136", "gemm", M=5, N=64, K=136, a_ln=True, lnkind=lnkind, eps=eps)
            _mk(cs, f"gemm-lnres-{lnkind}-eps{eps:g}-N136", "gemm", M=5, N=136, K=64, r_mode=2, lnkind=lnkind, eps=eps,
                outs="Cz", stats=True)
    # the cache write: the bf16 A operand, and the LN operand (the real in_proj)
    for a_ln in (False, True):
        for kv0 in (0, 8, 72, 64):   # N / 3 = 64
            for pos in (0, 3):
                _mk(cs, f"gemm-{'ln' if a_ln else 'plain'}-cache-kv{kv0}-pos{pos}", "gemm", M=3, N=192, K=72, a_ln=a_ln,
                    cache=(kv0, pos, 16 if kv0 != 72 else 0), lda_pad=8, ldc_pad=8, lnkind="tiles")
    # ---------------- argmax epilogue: exact arithmetic ----------------
    for V in (7, 509, 1001, 1024, 1088):
        for M in (1, 70):
            for kind in ("rand", "neg", "one", "nan"):
                if M == 70 and kind in ("one", "nan") and V not in (509, 1088):
                    continue
                _mk(cs, f"argmax-V{V}-M{M}-{kind}", "argmax", M=M, N=V, K=72, amode=kind, lda_pad=8, ldb_pad=8)
    # ---------------- mit_decode_layernorm ----------------
    for i, W in enumerate((8, 64, 72, 512, 520, 1024)):
        for j, M in enumerate((1, 3, 4, 5)):
            _mk(cs, f"ln-M{M}-W{W}", "ln", M=M, W=W, ldz_pad=(0, 4)[(i + j) % 2], ldo_pad=(8, 0)[(i + j) % 2],
                lnkind=("plain", "mean50", "tiles")[(i + j) % 3], eps=(1e-5, 1e-12)[j % 2])
    # ---------------- producer -> consumer on device statistics ----------------
    _mk(cs, "chain-M33-N136-K72", "chain", M=33, N=136, K=72, lnkind="tiles")
    assert len({c.id for c in cs}) == len(cs)
    return cs


CASES = _build_cases()
BY_ID = {c.id: c for c in CASES}


# ------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------
def gen(c):
    import zlib
    return torch.Generator().manual_seed(zlib.crc32(c.id.encode()))


def rounded(x, dtype):
    return x.to(dtype).to(torch.float64) if dtype != torch.float64 else x


def pack_key(value, col):
    """the header's key: ord(value) << 32 | (0xFFFFFFFF - col); ord: the order-preserving u32 image of an f32, NaN
    largest. value: float32 tensor, col: int64 tensor; returns int64 holding the u64 bit pattern."""
    u = value.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    o = torch.where(u >= 0x80000000, (~u) & 0xFFFFFFFF, u | 0x80000000)
    o = torch.where(torch.isnan(value), torch.full_like(o, 0xFFFFFFFF), o)
    lo = 0xFFFFFFFF - col.to(torch.int64)
    hi = torch.where(o >= 0x80000000, o - (1 << 32), o)   # as the signed upper half
    return (hi << 32) | lo


def umax(keys, dim):
    """maximum in unsigned order of int64 bit patterns"""
    mn = torch.iinfo(torch.int64).min
    return (keys ^ mn).max(dim).values ^ mn


def argmax_of_keys(keys):
    """[slots, M] keys -> the column each row's largest key names (native.argmax_of_keys does the same)"""
    return 0xFFFFFFFF - (umax(keys, 0) & 0xFFFFFFFF)


def ref_argmax(row):
    """torch.argmax's rule on a 1-D float tensor: the first NaN, else the first maximal column (-0.0 == +0.0)"""
    nan = torch.isnan(row)
    if nan.any():
        return int(nan.nonzero()[0])
    return int((row == row.max()).nonzero()[0])


def fsum(x, dim, mode):
    """sum over dim as a true loop in x's dtype: "seq" element after element, "tree" pairwise halves (xor tree)"""
    x = x.movedim(dim, 0)
    if mode == "seq" or x.shape[0] <= 1:
        acc = torch.zeros_like(x[0])
        for i in range(x.shape[0]):
            acc = acc + x[i]
        return acc
    n = 1
    while n < x.shape[0]:
        n *= 2
    if n != x.shape[0]:
        x = torch.cat([x, torch.zeros((n - x.shape[0],) + x.shape[1:], dtype=x.dtype)])
    while x.shape[0] > 1:
        h = x.shape[0] // 2
        x = x[:h] + x[h:]
    return x[0]


def lane_sum(x, mode):
    """sum over the last dim (a head's Dh or a K block): seq, or 8-element lane partials then a tree over the lanes"""
    if mode == "seq" or x.shape[-1] % 8:
        return fsum(x, -1, "seq")
    part = fsum(x.reshape(x.shape[:-1] + (x.shape[-1] // 8, 8)), -1, "seq")
    return fsum(part, -1, "tree")


# ------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------
def attn_geom(c):
    W = c.H * c.Dh
    Lmax = c.Lk + c.extra
    if c.layout == "model":      # q a column slice of [B, 3W]; K | V the halves of [B, Lmax, 2W]
        row, k_off, v_off = 2 * W, 0, W
    else:                        # layer 1 of the cross-attention memory [B * S, 3 * 2W]
        row, k_off, v_off = 6 * W, 2 * W, 3 * W
    return dict(W=W, Lmax=Lmax, q_batch=3 * W, q_off=W, row=row, k_off=k_off, v_off=v_off,
                kv_batch=(Lmax + c.gap) * row, o_batch=W + c.o_pad, tok_batch=Lmax + c.tok_pad,
                scale=f32r(c.scale if c.scale is not None else c.Dh ** -0.5),
                lk_arg=Lmax + 50 if c.use_pos else c.Lk)


def attn_mask(c):
    """[B, Lk] bool: key is PAD"""
    B, Lk = max(c.B, 1), c.Lk
    m = torch.zeros(B, Lk, dtype=torch.bool)
    j = torch.arange(Lk)
    if c.mask == "first":
        m[:, 0] = True
    elif c.mask == "first64":
        m[:, :64] = True
    elif c.mask == "slab":       # every key of wave 1
        m[:] = ((j // kpw(c.Dh)) % 4 == 1) if c.family == "bh" else ((j // 8) % 8 == 1)
    elif c.mask == "tail":
        m[:, Lk - Lk // 3:] = True
        if B > 1:
            m[1, Lk // 2:] = True
    elif c.mask == "row_all":
        m[1] = True
        m[0, 2] = True
    elif c.mask == "pad3":
        m[:, 1] = True
        m[:, Lk - 1] = True
    return m


def make_attn(c):
    t, g, G = Tensors(), gen(c), attn_geom(c)
    dt = _TORCH[c.dtype]
    B, H, Dh, Lk, W = max(c.B, 1), c.H, c.Dh, c.Lk, G["W"]
    q = (torch.randn(B, H, Dh, generator=g) * c.qscale).to(dt)
    K = torch.randn(B, Lk, H, Dh, generator=g).to(dt)
    V = torch.randn(B, Lk, H, Dh, generator=g).to(dt)
    if c.hot:
        j0 = {"first": 0, "mid": Lk // 2, "last": Lk - 2}[c.hot]
        qd = q.double()
        a = 100.0 / (G["scale"] * (qd * qd).sum(-1))              # [B, H]: the hot keys score about 100
        for jj, f in ((j0, 1.0), (j0 + 1, 0.99)):
            K[:, jj] = (qd * (a * f)[..., None]).to(dt)
    mask = attn_mask(c)
    sign = torch.where(torch.arange(Lk) % 2 == 0, 1.0, -1.0)[None, :, None, None]
    K = torch.where(mask[:, :, None, None], (1e4 * sign).to(dt), K)
    V = torch.where(mask[:, :, None, None], (-1e4 * sign).to(dt), V)
    qa = t.new("q", B * G["q_batch"], dt, NAN, margin=G["q_batch"])
    qa.win(G["q_off"], B, W, G["q_batch"]).copy_(q.reshape(B, W))
    kv = t.new("kv", B * G["kv_batch"], dt, NAN, margin=G["row"])
    for b in range(B):
        kv.win(b * G["kv_batch"] + G["k_off"], Lk, W, G["row"]).copy_(K[b].reshape(Lk, W))
        kv.win(b * G["kv_batch"] + G["v_off"], Lk, W, G["row"]).copy_(V[b].reshape(Lk, W))
    o = t.new("o", B * G["o_batch"], dt, SENTINEL, margin=G["o_batch"])
    if c.B > 0:
        o.allow(0, B, W, G["o_batch"])
    if c.mask != "none":
        live = 0 if c.pad_idx != 0 else LIVE_TOK
        tok = t.new("tok", B * G["tok_batch"], torch.int64, live, margin=G["tok_batch"])
        tok.win(0, B, Lk, G["tok_batch"]).masked_fill_(mask, c.pad_idx)
    if c.use_pos:
        t.new("pos", 1, torch.int64, 0, margin=8).base[0] = Lk - 1
    t.x["G"] = G
    return t


def attn_windows(c, t):
    """(q [B, H, Dh], K, V [B, Lk, H, Dh], pad [B, Lk] or None) of the pre-launch snapshots, in their dtype"""
    G = t.x["G"]
    B, H, Dh, Lk, W = max(c.B, 1), c.H, c.Dh, c.Lk, G["W"]
    q = t.a["q"].bwin(G["q_off"], B, W, G["q_batch"]).reshape(B, H, Dh)
    K = torch.stack([t.a["kv"].bwin(b * G["kv_batch"] + G["k_off"], Lk, W, G["row"]) for b in range(B)])
    V = torch.stack([t.a["kv"].bwin(b * G["kv_batch"] + G["v_off"], Lk, W, G["row"]) for b in range(B)])
    pad = t.a["tok"].bwin(0, B, Lk, G["tok_batch"]) == c.pad_idx if "tok" in t.a else None
    return q, K.reshape(B, Lk, H, Dh), V.reshape(B, Lk, H, Dh), pad


def reference_attn(c, t):
    """(o [B, W] float64, unit [B, W])"""
    q, K, V, pad = attn_windows(c, t)
    q, K, V = q.double(), K.double(), V.double()
    sc = t.x["G"]["scale"]
    s = torch.einsum("bhd,bjhd->bhj", q, K) * sc
    A = torch.einsum("bhd,bjhd->bhj", q.abs(), K.abs()) * sc * L2E
    if pad is not None:
        s = s.masked_fill(pad[:, None, :], -math.inf)
        A = A.masked_fill(pad[:, None, :], 0.0)
    p = torch.softmax(s, -1)                       # a row of -inf only: NaN, as the header says
    o = torch.einsum("bhj,bjhd->bhd", p, V)
    unit = ULP * (1 + A.max(-1).values)[..., None] * torch.einsum("bhj,bjhd->bhd", p.nan_to_num(0.0), V.abs())
    B = q.shape[0]
    return o.reshape(B, -1), unit.reshape(B, -1)


def fake_attn(c, t, mode, faults):
    G = t.x["G"]
    if c.B <= 0:
        return
    B, H, Dh, W = c.B, c.H, c.Dh, G["W"]
    fdt = torch.float64 if mode == "f64" else torch.float32
    Lk = c.Lk if c.use_pos else G["lk_arg"]        # *pos + 1, or the argument
    if c.use_pos and "lk_arg_used" in faults:
        Lk = G["lk_arg"]
    Lk += ("one_key_more" in faults) - ("one_key_fewer" in faults)
    if Lk > G["Lmax"] + c.gap:                      # stay inside the buffer, as the guards promise a kernel
        Lk = G["Lmax"] + c.gap
    q = t.a["q"].win(G["q_off"], B, W, G["q_batch"]).reshape(B, H, Dh).to(fdt)
    K = torch.stack([t.a["kv"].win(b * G["kv_batch"] + G["k_off"], Lk, W, G["row"]) for b in range(B)])
    V = torch.stack([t.a["kv"].win(b * G["kv_batch"] + G["v_off"], Lk, W, G["row"]) for b in range(B)])
    K, V = K.reshape(B, Lk, H, Dh).to(fdt), V.reshape(B, Lk, H, Dh).to(fdt)
    pad = None
    if "tok" in t.a and "mask_ignored" not in faults:
        tb = G["Lmax"] if "tok_batch_lmax" in faults else G["tok_batch"]
        pad = t.a["tok"].win(0, B, Lk, tb) == (0 if "mask_vs_zero" in faults else c.pad_idx)
    sc = torch.tensor(G["scale"], dtype=fdt)
    l2e = torch.tensor(1.0 if "no_log2e" in faults else L2E, dtype=fdt)   # scores in exp2 units
    if Dh == 128 and "half_head" in faults:
        K = K.clone()
        K[..., 64:] = 0
    if mode == "tree":      # the kernels fold scale log2(e) into q
        s = lane_sum((q * (sc * l2e))[:, None] * K, "tree")           # [B, Lk, H]
    else:
        s = lane_sum(q[:, None] * K, "seq") * sc * l2e
    if pad is not None:
        s = s.masked_fill(pad[:, :, None], -math.inf)
    # the kernels' structure: each wave sweeps its slabs of `per` keys with an online softmax (one maximum and one
    # rescale per slab), the waves' states are merged in wave order
    nw, per = (4, kpw(Dh)) if c.family == "bh" else (8, 8)
    order = "tree" if mode == "tree" else "seq"
    big = torch.tensor(NEG_BIG, dtype=fdt)

    def merge(m, l, acc, m2, l2, acc2):
        mn = torch.maximum(m, m2)
        c1, c2 = torch.exp2(m - mn), torch.exp2(m2 - mn)
        if "no_rescale" in faults:
            c1 = torch.ones_like(c1)
        return mn, l * c1 + l2 * c2, acc * c1[..., None] + acc2 * c2[..., None]

    m, l, acc = big.expand(B, H), torch.zeros(B, H, dtype=fdt), torch.zeros(B, H, Dh, dtype=fdt)
    for w in range(nw):
        if w == nw - 1 and "wave_dropped" in faults:
            continue
        mw, lw, aw = big.expand(B, H), torch.zeros(B, H, dtype=fdt), torch.zeros(B, H, Dh, dtype=fdt)
        for j0 in range(w * per, Lk, nw * per):
            sw, Vw = s[:, j0:j0 + per], V[:, j0:j0 + per]
            bm = torch.maximum(sw.max(1).values, big)
            p = torch.exp2(sw - torch.maximum(mw, bm)[:, None])
            mw, lw, aw = merge(mw, lw, aw, torch.maximum(mw, bm), fsum(p, 1, order), fsum(p[..., None] * Vw, 1, order))
        m, l, acc = merge(m, l, acc, mw, lw, aw)
    o = acc * (1.0 / l)[..., None]
    if "all_masked_zero" in faults:
        o = o.nan_to_num(0.0)
    ob = W if "o_batch_w" in faults else G["o_batch"]
    t.a["o"].win(0, B, W, ob).copy_(o.reshape(B, W).to(_TORCH[c.dtype]))


def check_float(name, kind, got, ref, unit, bf16_out, figs):
    """figure = worst |got - ref| (past 2^-8 |ref| for a bf16 output) in `unit`s; NaN exactly where ref is NaN"""
    got, ref = got.double(), ref.double()
    gn, rn = torch.isnan(got), torch.isnan(ref)
    assert torch.equal(gn, rn), f"{name}: NaN at {int((gn != rn).sum())} element(s) where the reference differs " \
                                f"(got NaN: {int(gn.sum())}, reference NaN: {int(rn.sum())})"
    ok = ~rn
    if not ok.any():
        return
    err = (got - ref).abs()[ok]
    if bf16_out:
        err = (err - BF16_REL * ref.abs()[ok]).clamp_min(0.0)
    u = unit[ok].clamp_min(1e-300)
    fig = float((err / u).max())
    figs.append((kind, name, fig))


def check_attn(c, t, figs):
    if c.B <= 0:
        return
    G = t.x["G"]
    ref, unit = reference_attn(c, t)
    got = t.a["o"].whole.cpu().as_strided((c.B, G["W"]), (G["o_batch"], 1), t.a["o"].off)
    if c.mask == "row_all":
        assert torch.isnan(ref[1]).all() and not torch.isnan(ref[0]).any()
    check_float("o", "attn", got, ref, unit, c.dtype == "bf16", figs)


# ------------------------------------------------------------------------------------------------
# kv_store / embed_decode
# ------------------------------------------------------------------------------------------------
EMB_VOCAB, EMB_NAN_ROW = 5, 2


def store_geom(c):
    return dict(s_batch=c.n + c.s_pad, c_row=c.n + c.c_pad, c_batch=c.R * (c.n + c.c_pad), ld_ids=c.R + 1 + c.ids_pad)


def make_kvstore(c):
    t, g, G = Tensors(), gen(c), store_geom(c)
    dt = _TORCH[c.dtype]
    src = t.new("src", c.B * G["s_batch"], dt, NAN, margin=G["s_batch"])
    src.win(0, c.B, c.n, G["s_batch"]).copy_(torch.randn(c.B, c.n, generator=g).to(dt))
    cache = t.new("cache", c.B * G["c_batch"], dt, SENTINEL, margin=G["c_row"])
    cache.allow(c.pos * G["c_row"], c.B, c.n, G["c_batch"])
    t.new("pos", 1, torch.int64, 0, margin=8).base[0] = c.pos
    t.x["G"] = G
    return t


def fake_kvstore(c, t, mode, faults):
    G = t.x["G"]
    p = c.pos + ("row_pos_plus_1" in faults)
    src = t.a["src"].win(0, c.B, c.n, G["s_batch"])
    dst = t.a["cache"].win(p * G["c_row"], c.B, c.n, G["c_batch"])
    if "stops_at_grid_cap" in faults and c.B * c.n > GRID_CAP:
        nb = GRID_CAP // c.n
        dst[:nb].copy_(src[:nb])
    else:
        dst.copy_(src)


def check_kvstore(c, t, figs):
    G = t.x["G"]
    a = t.a["cache"]
    got = a.whole.cpu().as_strided((c.B, c.n), (G["c_batch"], 1), a.off + c.pos * G["c_row"])
    src = t.a["src"].bwin(0, c.B, c.n, G["s_batch"])
    it = gc._INT[a.esz]
    assert torch.equal(got.contiguous().view(it), src.contiguous().view(it)), \
        "cache row *pos is not a bitwise copy of src"


def make_embed(c):
    t, g, G = Tensors(), gen(c), store_geom(c)
    dt = _TORCH[c.dtype]
    d, T = c.n, c.R + 1
    table = torch.randn(EMB_VOCAB, d, generator=g).to(dt)
    table[EMB_NAN_ROW] = NAN
    t.new("table", EMB_VOCAB * d, dt, NAN, margin=d).win(0, EMB_VOCAB, d, d).copy_(table)
    ids = t.new("ids", c.B * G["ld_ids"], torch.int64, EMB_NAN_ROW, margin=G["ld_ids"])   # in-bounds poison
    live = torch.tensor([0, EMB_VOCAB - 1, 1, 3])[torch.arange(c.B) % 4]                   # first and last table rows
    ids.win(c.pos, c.B, 1, G["ld_ids"]).copy_(live[:, None])
    pe = t.new("pe", T * d, torch.float32, NAN, margin=d)
    pe.win(c.pos * d, 1, d, d).copy_(torch.randn(1, d, generator=g))
    t.new("out", c.B * d, dt, SENTINEL, margin=d).allow(0, c.B, d, d)
    t.new("pos", 1, torch.int64, 0, margin=8).base[0] = c.pos
    t.x["G"], t.x["scale"] = G, f32r(math.sqrt(d))
    return t


def fake_embed(c, t, mode, faults):
    G, d = t.x["G"], c.n
    idc = c.pos + ("ids_pos_plus_1" in faults)
    ids = t.a["ids"].win(idc, c.B, 1, G["ld_ids"])[:, 0]
    rows = t.a["table"].win(0, EMB_VOCAB, d, d)[ids].float()
    pe = t.a["pe"].win((0 if "pe_row_0" in faults else c.pos) * d, 1, d, d)
    out = (rows * torch.tensor(t.x["scale"], dtype=torch.float32) + pe).to(_TORCH[c.dtype])
    dst = t.a["out"].win(0, c.B, d, d)
    if "stops_at_grid_cap" in faults and c.B * d > GRID_CAP:
        nb = GRID_CAP // d
        dst[:nb].copy_(out[:nb])
    else:
        dst.copy_(out)


def check_embed(c, t, figs):
    G, d = t.x["G"], c.n
    ids = t.a["ids"].bwin(c.pos, c.B, 1, G["ld_ids"])[:, 0]
    rows = t.a["table"].bwin(0, EMB_VOCAB, d, d)[ids].double()
    pe = t.a["pe"].bwin(c.pos * d, 1, d, d).double()
    prod = rows * t.x["scale"]                                  # exact in float64 (24 x 24 bits)
    dt = _TORCH[c.dtype]
    fused = (prod + pe).float().to(dt)
    unfused = (prod.float().double() + pe).float().to(dt)
    a = t.a["out"]
    got = a.whole.cpu().as_strided((c.B, d), (d, 1), a.off)
    it = gc._INT[a.esz]
    g_, f_, u_ = (x.contiguous().view(it) for x in (got, fused, unfused))
    bad = (g_ != f_) & (g_ != u_)
    assert not bad.any(), f"{int(bad.sum())} element(s) are neither the fused nor the unfused float32 value; first " \
                          f"at {bad.nonzero()[0].tolist()}: {got[bad][0].item()} vs {fused[bad][0].item()}"


# ------------------------------------------------------------------------------------------------
# greedy picks
# ------------------------------------------------------------------------------------------------
def pick_rows(c, g):
    """the logit rows of a case: every pattern whose columns fit V; returns (rows [n, V] float32, names)"""
    V = c.V
    rows, names = [], []

    def base():
        return torch.randn(V, generator=g)

    def add(name, r):
        rows.append(r)
        names.append(name)

    def peaks(name, cols, val=50.0):
        if all(0 <= x < V for x in cols) and len(set(cols)) == len(cols):
            r = base()
            r[list(cols)] = val
            add(name, r)

    vec = pick_is_vector(c)
    tb = 4 if vec else 1            # columns of one thread's step; wave boundary: 64 threads
    peaks("max-0", (0,))
    peaks("max-last", (V - 1,))
    peaks("max-last-unfinished-twin", (V - 1,))
    peaks("max-last-finished", (V - 1,))
    peaks("thread-boundary-lo", (tb - 1,))
    peaks("thread-boundary-hi", (tb,))
    peaks("wave-boundary-lo", (64 * tb - 1,))
    peaks("wave-boundary-hi", (64 * tb,))
    peaks("tie-in-flight", (1024 + 5, 5, 2048 + 5, 3072 + 5) if vec else (256 + 5, 5, 512 + 5))
    peaks("tie-threads", (9, 5))
    peaks("tie-waves", (700, 300))
    peaks("tie-last-two", (V - 1, V - 2))
    add("all-equal", torch.full((V,), 1.5))
    add("all-neg-inf", torch.full((V,), -math.inf))
    peaks("pos-inf-twice", (V // 2, V // 3), math.inf)
    if V >= 5:
        r = base()
        r[1] = 60.0
        r[[3, V - 1]] = NAN
        add("nan-twice-after-larger", r)
        r = -base().abs() - 1.0
        r[2], r[4] = -0.0, 0.0
        add("neg-zero-before-pos-zero", r)
        r = -base().abs() - 1.0
        r[V - 2], r[V - 1] = 0.0, -0.0
        add("pos-zero-before-neg-zero", r)
    return torch.stack(rows), names


def pick_is_vector(c):
    """the device-side predicate of greedy_pick_kernel: 16-B loads"""
    return c.V % 4 == 0 and (c.V + c.ld_pad) % 4 == 0 and c.mis == 0


def make_pick(c):
    t, g = Tensors(), gen(c)
    V, ld, T = c.V, c.V + c.ld_pad, c.T
    rows, names = pick_rows(c, g)
    if c.op == "pickadv":
        rows = rows[torch.arange(c.B) % rows.shape[0]]
        names = [names[i % len(names)] for i in range(c.B)]
    B = rows.shape[0]
    poison = {None: NAN, "nan": NAN, "inf": math.inf}[c.poison]
    lg = t.new("logits", B * ld, torch.float32, poison, margin=ld + 8, misalign=c.mis)
    lg.win(0, B, V, ld).copy_(rows)
    ids = t.new("ids", B * T, torch.int64, INT_SENT, margin=T)
    for k in range(c.steps):
        ids.allow(c.pos + 1 + k, B, 1, T)
    fin = t.new("finished", B, torch.int32, 0, margin=8)
    fin.allow(0, 1, B, B)
    for i, nm in enumerate(names):
        if nm == "max-last-finished":
            fin.base[i] = 1
    t.new("n_finished", 1, torch.int32, 0, margin=8).base[0] = c.n0
    t.a["n_finished"].allow(0, 1, 1, 1)
    pos = t.new("pos", 1, torch.int64, 0, margin=8)
    pos.base[0] = c.pos
    if c.adv:
        pos.allow(0, 1, 1, 1)
        t.new("ticket", 1, torch.int32, 0, margin=8).allow(0, 1, 1, 1)
    t.x.update(B=B, ld=ld, end_id=V - 1 if V > 1 else 99, pad_id=-5)
    return t


def pick_expect(c, t, picks):
    """ids columns, finished, n_finished after c.steps steps with the same picks"""
    B = t.x["B"]
    fin = t.a["finished"].before[t.a["finished"].off:][:B].clone()
    nf = int(t.a["n_finished"].before[t.a["n_finished"].off])
    cols = []
    for _ in range(c.steps):
        col = torch.where(fin != 0, torch.tensor(t.x["pad_id"]), picks)
        newly = (fin == 0) & (picks == t.x["end_id"])
        nf += int(newly.sum())
        fin = torch.where(newly, torch.ones_like(fin), fin)
        cols.append(col)
    return torch.stack(cols, 1), fin, nf


def check_pick_state(c, t, picks):
    B, T = t.x["B"], c.T
    cols, fin, nf = pick_expect(c, t, picks)
    a = t.a["ids"]
    got = a.whole.cpu().as_strided((B, c.steps), (T, 1), a.off + c.pos + 1)
    bad = got != cols
    assert not bad.any(), f"{int(bad.sum())} pick(s) differ; first (row, step) {bad.nonzero()[0].tolist()}: " \
                          f"{got[bad][0].item()} expected {cols[bad][0].item()}"
    gf = t.a["finished"].whole.cpu()[t.a["finished"].off:][:B]
    assert torch.equal(gf, fin), f"finished differs at rows {(gf != fin).nonzero()[:4, 0].tolist()}"
    # a finished row that was 1 stays bitwise 1
    gn = int(t.a["n_finished"].whole.cpu()[t.a["n_finished"].off])
    assert gn == nf, f"n_finished {gn}, expected {nf}"
    if c.adv or c.op == "pickkeys":
        gp = int(t.a["pos"].whole.cpu()[t.a["pos"].off])
        assert gp == c.pos + c.steps, f"pos {gp}, expected {c.pos + c.steps}: it advances exactly once per step"
    if "ticket" in t.a:
        assert int(t.a["ticket"].whole.cpu()[t.a["ticket"].off]) == 0, "ticket is not left at 0"


def check_pick(c, t, figs):
    B, V, ld = t.x["B"], c.V, t.x["ld"]
    rows = t.a["logits"].bwin(0, B, V, ld)
    picks = torch.tensor([ref_argmax(rows[b]) for b in range(B)])
    check_pick_state(c, t, picks)


def fake_pick(c, t, mode, faults):
    B, V, ld, T = t.x["B"], c.V, t.x["ld"], c.T
    width = V
    if "pad_column_can_win" in faults:
        width = ld
    elif "vector_reads_past_v" in faults and pick_is_vector(c):
        width = min(ld, V + 4)
    rows = t.a["logits"].win(0, B, width, ld).clone()
    picks = []
    for b in range(B):
        r = rows[b]
        nan = torch.isnan(r)
        if nan.any() and "nan_ignored" not in faults:
            picks.append(int(nan.nonzero()[0]))
            continue
        r = torch.where(nan, torch.tensor(-math.inf), r)
        mx = r.max()
        hit = r == mx
        if "neg_zero_below" in faults and float(mx) == 0.0:
            pz = hit & ~torch.signbit(r)
            hit = pz if pz.any() else hit
        idx = hit.nonzero()[:, 0]
        picks.append(int(idx[-1] if "last_on_ties" in faults else idx[0]))
    picks = torch.tensor(picks)
    fin, nf, pos = t.a["finished"].base[:B], t.a["n_finished"].base, t.a["pos"].base
    ids = t.a["ids"].win(0, B, T, T)
    for _ in range(c.steps):
        p = int(pos[0])
        for b in range(B):
            if fin[b]:
                ids[b, p + 1] = t.x["pad_id"]
                if "finished_counted_again" in faults and int(picks[b]) == t.x["end_id"]:
                    nf[0] += 1
            else:
                ids[b, p + 1] = int(picks[b])
                if int(picks[b]) == t.x["end_id"]:
                    fin[b] = 1
                    nf[0] += 1
            if c.adv and "pos_per_block" in faults:
                pos[0] = p + 1 + b
        if c.adv and "pos_per_block" not in faults:
            pos[0] = p + 1


def make_pickkeys(c):
    """keys as a decode_gemm argmax head over V columns would leave them: slot = (column // 64) % 16"""
    t, g = Tensors(), gen(c)
    B, V, T = c.B, c.V, c.T
    vals = torch.randn(B, V, generator=g)
    win = (torch.arange(B) * 67 + 3) % V                     # the winners sit in different slots
    vals[torch.arange(B), win] = 40.0
    vals[0::7] -= 100.0                                      # rows whose maximum is negative
    if B > 4:
        vals[4, 70], vals[4, 700] = NAN, NAN                 # a NaN key: column 70 wins
    keys = torch.zeros(ARGMAX_SLOTS, B, dtype=torch.int64)
    col = torch.arange(V)
    pk = pack_key(vals, col[None, :].expand(B, V))
    for s in range(ARGMAX_SLOTS):
        sel = ((col // 64) % ARGMAX_SLOTS) == s
        keys[s] = umax(pk[:, sel], 1)
    ka = t.new("keys", ARGMAX_SLOTS * B, torch.int64, INT_SENT, margin=B + 8)
    ka.win(0, ARGMAX_SLOTS, B, B).copy_(keys)
    ka.allow(0, ARGMAX_SLOTS, B, B)
    t.new("ids", B * T, torch.int64, INT_SENT, margin=T).allow(c.pos + 1, B, 1, T)
    fin = t.new("finished", B, torch.int32, 0, margin=8)
    fin.allow(0, 1, B, B)
    fin.base[1::5] = 1
    t.new("n_finished", 1, torch.int32, 0, margin=8).base[0] = c.n0
    t.a["n_finished"].allow(0, 1, 1, 1)
    pos = t.new("pos", 1, torch.int64, 0, margin=8)
    pos.base[0] = c.pos
    pos.allow(0, 1, 1, 1)
    picks = torch.tensor([ref_argmax(vals[b]) for b in range(B)])
    end_id = int(picks[0])
    t.x.update(B=B, picks=picks, end_id=end_id, pad_id=-5)
    return t


def check_pickkeys(c, t, figs):
    B = c.B
    keys = t.a["keys"].bwin(0, ARGMAX_SLOTS, B, B).contiguous()
    assert torch.equal(argmax_of_keys(keys), t.x["picks"])
    check_pick_state(c, t, t.x["picks"])
    after = t.a["keys"].whole.cpu()[t.a["keys"].off:][:ARGMAX_SLOTS * B]
    assert not after.any(), f"{int((after != 0).sum())} key(s) not reset to 0"


def fake_pickkeys(c, t, mode, faults):
    B, T = c.B, c.T
    nb = min(B, 1024) if "rows_ge_1024_skipped" in faults else B
    keys = t.a["keys"].win(0, ARGMAX_SLOTS, B, B)
    best = umax(keys[:, :nb], 0)
    picks = 0xFFFFFFFF - (best & 0xFFFFFFFF)
    if "keys_not_reset" not in faults:
        keys[:, :nb] = 0
    fin, nf, pos = t.a["finished"].base[:B], t.a["n_finished"].base, t.a["pos"].base
    p = int(pos[0])
    col = t.a["ids"].win(p + 1, B, 1, T)[:, 0]
    done = fin[:nb] != 0
    col[:nb] = torch.where(done, torch.tensor(t.x["pad_id"]), picks)
    newly = ~done & (picks == t.x["end_id"])
    fin[:nb] = torch.where(newly, torch.ones_like(fin[:nb]), fin[:nb])
    nf[0] += int(newly.sum())
    pos[0] = p + 1


# ------------------------------------------------------------------------------------------------
# decode GEMM, argmax epilogue, decode LayerNorm
# ------------------------------------------------------------------------------------------------
def tiles_of(W):
    return (W + 63) // 64


def ln_input(c, rows, W, g):
    """f32 pre-LN sums that give every term of the merge weight"""
    z = torch.randn(rows, W, generator=g)
    if c.lnkind == "mean50":
        z = z + 50.0
    elif c.lnkind == "tiles":
        z = z + (6.0 * torch.randn(rows, tiles_of(W), generator=g)).repeat_interleave(64, 1)[:, :W]
    return z.float()


def host_stats(z):
    """per 64-column tile (mean, M2) of each row of z, float64 -> float32 [rows, P, 2]"""
    rows, W = z.shape
    out = torch.zeros(rows, tiles_of(W), 2, dtype=torch.float64)
    for p in range(tiles_of(W)):
        x = z[:, 64 * p:64 * p + 64].double()
        out[:, p, 0] = x.mean(1)
        out[:, p, 1] = ((x - x.mean(1, keepdim=True)) ** 2).sum(1)
    return out


def merge_stats(st, W, dt=torch.float64, faults=(), mode="seq"):
    """Chan's merge of [rows, P, 2] partials -> (mean, var) in dt, in the kernel's order"""
    st = st.to(dt)
    P = tiles_of(W)
    n = torch.tensor([min(64, W - 64 * p) for p in range(P)], dtype=dt)
    if "partial_tile_as_64" in faults:
        n = torch.full_like(n, 64.0)
    Wd = n.sum() if "partial_tile_as_64" in faults else torch.tensor(float(W), dtype=dt)
    mean = fsum(st[:, :, 0] * n, 1, "seq") / Wd
    dm = st[:, :, 0] - mean[:, None]
    extra = dm * dm * n
    if "dm2_dropped" in faults:
        extra = torch.zeros_like(extra)
    var = fsum(st[:, :, 1] + extra, 1, "seq") / Wd
    return mean, var


def gemm_geom(c):
    M, N, K = c.M, c.N, c.K
    G = dict(lda=K + c.lda_pad, ldb=K + c.ldb_pad, ldc=N + c.ldc_pad, ldz=N + c.ldz_pad, ldr=N + c.ldr_pad,
             Pa=tiles_of(K), Pn=tiles_of(N), has_C=c.op == "gemm" and "C" in c.outs,
             has_z=c.op == "gemm" and "z" in c.outs)
    if c.cache:
        kv0, pos, cpad = c.cache
        G.update(kv0=kv0, pos=pos, c_row=N - kv0 + cpad, R=4, c_batch=4 * (N - kv0 + cpad))
    return G


def make_gemm(c):
    t, g, G = Tensors(), gen(c), gemm_geom(c)
    M, N, K = c.M, c.N, c.K
    Mr = max(M, 1)
    bf = torch.bfloat16
    if c.a_ln:
        A = t.new("A", Mr * G["lda"], torch.float32, NAN, margin=G["lda"])
        z = ln_input(c, Mr, K, g)
        A.win(0, Mr, K, G["lda"]).copy_(z)
        t.new("a_stats", Mr * G["Pa"] * 2, torch.float32, NAN, margin=2 * G["Pa"]).base[:Mr * G["Pa"] * 2] = \
            host_stats(z).float().reshape(-1)
        t.new("a_gamma", K, torch.float32, NAN, margin=8).base[:K] = 1 + 0.1 * torch.randn(K, generator=g)
        t.new("a_beta", K, torch.float32, NAN, margin=8).base[:K] = 0.1 * torch.randn(K, generator=g)
    else:
        A = t.new("A", Mr * G["lda"], bf, NAN, margin=G["lda"])
        A.win(0, Mr, K, G["lda"]).copy_(torch.randn(Mr, K, generator=g).to(bf))
    Bm = t.new("B", N * G["ldb"], bf, NAN, margin=G["ldb"])
    Bm.win(0, N, K, G["ldb"]).copy_((torch.randn(N, K, generator=g) * 0.5).to(bf))
    if c.bias:
        t.new("bias", N, torch.float32, NAN, margin=8).base[:N] = torch.randn(N, generator=g)
    if c.r_mode == 1:
        t.new("r", Mr * G["ldr"], bf, NAN, margin=G["ldr"]).win(0, Mr, N, G["ldr"]).copy_(
            torch.randn(Mr, N, generator=g).to(bf))
    elif c.r_mode == 2:
        zr = ln_input(c, Mr, N, g)
        t.new("r", Mr * G["ldr"], torch.float32, NAN, margin=G["ldr"]).win(0, Mr, N, G["ldr"]).copy_(zr)
        t.new("r_stats", Mr * G["Pn"] * 2, torch.float32, NAN, margin=2 * G["Pn"]).base[:Mr * G["Pn"] * 2] = \
            host_stats(zr).float().reshape(-1)
        t.new("r_gamma", N, torch.float32, NAN, margin=8).base[:N] = 1 + 0.1 * torch.randn(N, generator=g)
        t.new("r_beta", N, torch.float32, NAN, margin=8).base[:N] = 0.1 * torch.randn(N, generator=g)
    if G["has_C"]:
        C = t.new("C", Mr * G["ldc"], torch.float32 if c.c_f32 else bf, SENTINEL, margin=G["ldc"])
        if M:
            C.allow(0, M, N, G["ldc"])
    if G["has_z"]:
        Z = t.new("z_out", Mr * G["ldz"], torch.float32, SENTINEL, margin=G["ldz"])
        if M:
            Z.allow(0, M, N, G["ldz"])
        if c.stats:
            t.new("stats_out", Mr * G["Pn"] * 2, torch.float32, SENTINEL, margin=2 * G["Pn"]).allow(
                0, 1, M * G["Pn"] * 2, M * G["Pn"] * 2)
    if c.cache:
        ca = t.new("cache", Mr * G["c_batch"], bf, SENTINEL, margin=G["c_row"])
        ca.allow(G["pos"] * G["c_row"], M, N - G["kv0"], G["c_batch"])
        t.new("pos", 1, torch.int64, 0, margin=8).base[0] = G["pos"]
    t.x["G"] = G
    return t


def ln_apply(z, mean, var, gamma, beta, eps, dt):
    rs = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=dt)) if dt == torch.float64 else \
        torch.rsqrt(var + torch.tensor(eps, dtype=dt))
    return (z - mean[:, None]) * rs[:, None] * gamma + beta, rs


def reference_gemm(c, t):
    """float64: dict(v [M, N] the pre-rounding value, unit [M, N])"""
    G = t.x["G"]
    M, N, K = c.M, c.N, c.K
    eps = f32r(c.eps)
    B = t.a["B"].bwin(0, N, K, G["ldb"]).double()
    flip = 0.0
    if c.a_ln:
        z = t.a["A"].bwin(0, M, K, G["lda"]).double()
        st = t.a["a_stats"].before[t.a["a_stats"].off:][:M * G["Pa"] * 2].reshape(M, G["Pa"], 2).double()
        mean, var = merge_stats(st, K)
        ga = t.a["a_gamma"].before[t.a["a_gamma"].off:][:K].double()
        be = t.a["a_beta"].before[t.a["a_beta"].off:][:K].double()
        a, rs = ln_apply(z, mean, var, ga, be, eps, torch.float64)
        e = ULP * (((z - mean[:, None]).abs() + 2 * mean.abs()[:, None]) * rs[:, None] * ga.abs() + be.abs())
        a = a.to(torch.bfloat16).double()
        flip = e @ B.abs().T + BF16_REL * torch.stack([(B.abs() * a[m].abs()).amax(-1) for m in range(M)])
    else:
        a = t.a["A"].bwin(0, M, K, G["lda"]).double()
    v = a @ B.T
    unit = a.abs() @ B.abs().T
    if c.bias:
        bias = t.a["bias"].before[t.a["bias"].off:][:N].double()
        v = v + bias
        unit = unit + bias.abs()
    if c.act == ACT_RELU:
        v = v.clamp_min(0.0)
    if c.r_mode == 1:
        r = t.a["r"].bwin(0, M, N, G["ldr"]).double()
        v, unit = v + r, unit + r.abs()
    elif c.r_mode == 2:
        zr = t.a["r"].bwin(0, M, N, G["ldr"]).double()
        st = t.a["r_stats"].before[t.a["r_stats"].off:][:M * G["Pn"] * 2].reshape(M, G["Pn"], 2).double()
        mean, var = merge_stats(st, N)
        ga = t.a["r_gamma"].before[t.a["r_gamma"].off:][:N].double()
        be = t.a["r_beta"].before[t.a["r_beta"].off:][:N].double()
        r, rs = ln_apply(zr, mean, var, ga, be, eps, torch.float64)
        v = v + r
        unit = unit + ((zr - mean[:, None]).abs() + 2 * mean.abs()[:, None]) * rs[:, None] * ga.abs() + be.abs()
    return v, ULP * unit + flip


def _ksteps(c, K, faults):
    """the 64-wide K-steps a launch sums, per wave (the launch shape's split), after the faults"""
    nw = 8 if (c.a_ln or K >= 512) and c.op != "argmax" else 4
    ns = (K + 63) // 64
    if "k_tail_dropped" in faults:
        ns = K // 64
    waves = [list(range(w, ns, nw)) for w in range(nw)]
    if "odd_step_dropped" in faults:
        waves = [s[:-1] if len(s) % 2 == 1 and len(s) >= 3 else s for s in waves]
    return waves


def fake_gemm(c, t, mode, faults):
    G = t.x["G"]
    M, N, K = c.M, c.N, c.K
    if M == 0:
        return
    dt = torch.float64 if mode == "f64" else torch.float32
    eps = f32r(c.eps)
    Ka = K + (8 if "a_pad_read" in faults and G["lda"] > K else 0)
    Bm = t.a["B"].win(0, N, K, G["ldb"]).to(dt)
    if c.a_ln:
        z = t.a["A"].win(0, M, K, G["lda"]).to(dt)
        st = t.a["a_stats"].base[:M * G["Pa"] * 2].reshape(M, G["Pa"], 2)
        mean, var = merge_stats(st, K, dt, faults)
        a, _ = ln_apply(z, mean, var, t.a["a_gamma"].base[:K].to(dt), t.a["a_beta"].base[:K].to(dt), eps, dt)
        a = a.to(torch.bfloat16).to(dt)
    else:
        a = t.a["A"].win(0, M, Ka, G["lda"]).to(dt)
        if Ka > K:
            Bm = torch.cat([Bm, torch.ones(N, Ka - K, dtype=dt)], 1)
    if "row_ge_m" in faults:
        a = a.clone()
        a[M - 1] = a[M - 1] + t.a["A"].win(M * G["lda"], 1, a.shape[1], G["lda"])[0].to(dt)
    a64, B64 = a.double(), Bm.double()

    def mfma(acc, s):
        """one K-step onto acc: two MFMAs of 32 k each; the 32 products (exact in float32) are summed in float64
        and rounded once -- the same on every host, whatever its BLAS does -- then added in acc's dtype"""
        for k0 in range(64 * s, min(64 * s + 64, a.shape[1]), 32):
            acc = acc + (a64[:, k0:k0 + 32] @ B64[:, k0:k0 + 32].T).to(dt)
        return acc

    waves = _ksteps(c, a.shape[1], faults)
    if mode == "tree":          # a partial tile per wave, summed in wave order
        v = torch.zeros(M, N, dtype=dt)
        for steps in waves:
            acc = torch.zeros(M, N, dtype=dt)
            for s in steps:
                acc = mfma(acc, s)
            v = v + acc
    else:                       # one accumulator over all K-steps in order
        v = torch.zeros(M, N, dtype=dt)
        for s in sorted(s for steps in waves for s in steps):
            v = mfma(v, s)
    pre_bias = v
    if c.bias:
        v = v + t.a["bias"].base[:N].to(dt)
    if c.act == ACT_RELU:
        v = v.clamp_min(0.0)
    if c.r_mode == 1:
        v = v + t.a["r"].win(0, M, N, G["ldr"]).to(dt)
    elif c.r_mode == 2:
        zr = t.a["r"].win(0, M, N, G["ldr"]).to(dt)
        mean, var = merge_stats(t.a["r_stats"].base[:M * G["Pn"] * 2].reshape(M, G["Pn"], 2), N, dt, faults)
        r, _ = ln_apply(zr, mean, var, t.a["r_gamma"].base[:N].to(dt), t.a["r_beta"].base[:N].to(dt), eps, dt)
        v = v + r
    if c.r_mode and "relu_after_residual" in faults:
        v = v.clamp_min(0.0)
    if c.op == "argmax":
        return v
    if G["has_C"]:
        out = v.to(torch.bfloat16) if c.c_f32 and "f32_c_through_bf16" in faults else v
        t.a["C"].win(0, M, N, G["ldc"]).copy_(out.to(t.a["C"].dtype))
    if G["has_z"]:
        t.a["z_out"].win(0, M, N, G["ldz"]).copy_(v.float())
        if c.stats:
            sv = (pre_bias if "stats_before_bias" in faults else v).float().to(dt)
            so = t.a["stats_out"].base[:M * G["Pn"] * 2].reshape(M, G["Pn"], 2)
            for p in range(G["Pn"]):
                x = sv[:, 64 * p:64 * p + 64]
                mp = fsum(x, 1, mode if mode != "f64" else "seq") / x.shape[1]
                so[:, p, 0] = mp.float()
                so[:, p, 1] = fsum((x - mp[:, None]) ** 2, 1, mode if mode != "f64" else "seq").float()
    if c.cache:
        kv0 = G["kv0"]
        row = G["pos"] + ("cache_row_pos_plus_1" in faults)
        shift = kv0 % 64 if "cache_col_mod_64" in faults else 0    # column n lands at n - kv0 + shift
        w = N - kv0 - shift
        t.a["cache"].win(row * G["c_row"] + shift, M, w, G["c_batch"]).copy_(v[:, kv0:kv0 + w].to(torch.bfloat16))
    return v


def check_stats(name, got, zw, W, figs):
    """got [M, P, 2] against the float64 per-tile (mean, M2) of the written zw [M, W], and merged against the row"""
    zw, got = zw.double(), got.double()
    want = host_stats(zw)
    um = torch.zeros_like(want[..., 0])
    u2 = torch.zeros_like(um)
    for p in range(tiles_of(W)):
        x = zw[:, 64 * p:64 * p + 64]
        mp = x.mean(1, keepdim=True)
        dv = (x - mp).abs()
        um[:, p] = ULP * x.abs().mean(1)
        u2[:, p] = ULP * (dv * dv + 2 * dv * (x.abs() + mp.abs())).sum(1)
    check_float(name + ".mean", "stats", got[..., 0], want[..., 0], um, False, figs)
    check_float(name + ".M2", "stats", got[..., 1], want[..., 1], u2, False, figs)
    mean, var = merge_stats(got, W)
    n = torch.tensor([min(64, W - 64 * p) for p in range(tiles_of(W))], dtype=torch.float64)
    rm = zw.mean(1)
    rv = ((zw - rm[:, None]) ** 2).mean(1)
    umean = (um * n).sum(1) / W
    check_float(name + ".merged-mean", "stats", mean, rm, umean, False, figs)
    dmabs = (want[..., 0] - rm[:, None]).abs()
    uvar = (u2 + 2 * dmabs * n * (um + umean[:, None])).sum(1) / W
    check_float(name + ".merged-var", "stats", var, rv, uvar, False, figs)


def check_gemm(c, t, figs):
    G = t.x["G"]
    M, N = c.M, c.N
    if M == 0:
        return
    v, unit = reference_gemm(c, t)
    if G["has_C"]:
        a = t.a["C"]
        got = a.whole.cpu().as_strided((M, N), (G["ldc"], 1), a.off)
        check_float("C", "gemm", got, v, unit, not c.c_f32, figs)
    if G["has_z"]:
        a = t.a["z_out"]
        zw = a.whole.cpu().as_strided((M, N), (G["ldz"], 1), a.off)
        check_float("z_out", "gemm", zw, v, unit, False, figs)
        if G["has_C"] and not c.c_f32:
            cw = t.a["C"].whole.cpu().as_strided((M, N), (G["ldc"], 1), t.a["C"].off)
            zb = zw.to(torch.bfloat16).contiguous()
            assert torch.equal(cw.contiguous().view(torch.int16), zb.view(torch.int16)), \
                "C is not the bf16 of z_out"
        if c.stats:
            so = t.a["stats_out"].whole.cpu()[t.a["stats_out"].off:][:M * G["Pn"] * 2].reshape(M, G["Pn"], 2)
            check_stats("stats_out", so, zw, N, figs)
    if c.cache:
        a, kv0 = t.a["cache"], G["kv0"]
        got = a.whole.cpu().as_strided((M, N - kv0), (G["c_batch"], 1), a.off + G["pos"] * G["c_row"])
        cw = t.a["C"].whole.cpu().as_strided((M, N), (G["ldc"], 1), t.a["C"].off)[:, kv0:]
        assert torch.equal(got.contiguous().view(torch.int16), cw.contiguous().view(torch.int16)), \
            "the cache row is not bitwise the bf16 C columns"


# ---- argmax: small-integer operands, exact in every order ----
def make_argmax(c):
    t, g, G = Tensors(), gen(c), gemm_geom(c)
    M, V, K = c.M, c.N, c.K
    bf = torch.bfloat16
    A = torch.randint(-3, 4, (M, K), generator=g).float()
    Bw = torch.randint(-3, 4, (V, K), generator=g).float()
    bias = torch.randint(-8, 9, (V,), generator=g).float()
    if c.amode == "neg":
        bias = bias - 4000.0
    elif c.amode == "one":
        bias[:] = -math.inf
        bias[V * 2 // 3] = 1.0
    elif c.amode == "nan":
        bias[[V // 2, V - 1]] = NAN
    # the first maximal column must win across blocks that share a slot: a tie between block 0 and the last block
    if c.amode == "rand" and V > 64:
        A[:, 0], Bw[:, 0] = 3.0, 0.0
        Bw[[5, V - 3], :] = 0.0
        Bw[[5, V - 3], 0] = 3.0
        bias[[5, V - 3]] = 3000.0
    t.new("A", M * G["lda"], bf, NAN, margin=G["lda"]).win(0, M, K, G["lda"]).copy_(A.to(bf))
    t.new("B", V * G["ldb"], bf, NAN, margin=G["ldb"]).win(0, V, K, G["ldb"]).copy_(Bw.to(bf))
    t.new("bias", V, torch.float32, NAN, margin=8).base[:V] = bias
    t.new("keys", ARGMAX_SLOTS * M, torch.int64, 0, margin=M + 8).allow(0, ARGMAX_SLOTS, M, M)
    t.x["G"] = G
    return t


def argmax_keys_of(v, slots=ARGMAX_SLOTS):
    """[slots, M] keys of the float32 logits v [M, V]: per slot the largest key over its 64-column blocks (0: none)"""
    M, V = v.shape
    col = torch.arange(V)
    pk = pack_key(v.float().contiguous(), col[None, :].expand(M, V))
    keys = torch.zeros(ARGMAX_SLOTS, M, dtype=torch.int64)
    for s in range(slots):
        sel = ((col // 64) % slots) == s
        if sel.any():
            keys[s] = umax(pk[:, sel], 1)
    return keys


def check_argmax(c, t, figs):
    G, M, V, K = t.x["G"], c.M, c.N, c.K
    a = t.a["A"].bwin(0, M, K, G["lda"]).double()
    Bw = t.a["B"].bwin(0, V, K, G["ldb"]).double()
    v = (a @ Bw.T + t.a["bias"].before[t.a["bias"].off:][:V].double()).float()   # exact: small integers
    want = argmax_keys_of(v)
    got = t.a["keys"].whole.cpu()[t.a["keys"].off:][:ARGMAX_SLOTS * M].reshape(ARGMAX_SLOTS, M)
    bad = got != want
    assert not bad.any(), f"{int(bad.sum())} slot key(s) differ; first (slot, row) {bad.nonzero()[0].tolist()}: " \
                          f"{got[bad][0].item():#x} expected {want[bad][0].item():#x}"
    picks = torch.tensor([ref_argmax(v[m]) for m in range(M)])
    assert torch.equal(argmax_of_keys(got), picks)


def fake_argmax(c, t, mode, faults):
    G, M, V = t.x["G"], c.M, c.N
    if "col_ge_v_can_win" in faults:
        # one more row of B enters the maximum
        G = dict(G)
        Bx = t.a["B"].win(0, V + 1, c.K, G["ldb"]).float()
        a = t.a["A"].win(0, M, c.K, G["lda"]).float()
        bias = torch.cat([t.a["bias"].base[:V], torch.zeros(1)])
        v = a @ Bx.T + bias
        keys = argmax_keys_of(v)
    else:
        v = fake_gemm(c, t, "f32" if mode == "f64" else mode, faults)
        keys = argmax_keys_of(v, 8 if "slot_mod_8" in faults else ARGMAX_SLOTS)
    cur = t.a["keys"].win(0, ARGMAX_SLOTS, M, M)
    cur.copy_(umax(torch.stack([cur, keys]), 0))       # atomic max onto what is there


# ---- mit_decode_layernorm ----
def make_ln(c):
    t, g = Tensors(), gen(c)
    M, W = c.M, c.W
    ldz, ldo, P = W + c.ldz_pad, W + c.ldo_pad, tiles_of(W)
    z = ln_input(c, M, W, g)
    t.new("z", M * ldz, torch.float32, NAN, margin=ldz).win(0, M, W, ldz).copy_(z)
    t.new("stats", M * P * 2, torch.float32, NAN, margin=2 * P).base[:M * P * 2] = host_stats(z).float().reshape(-1)
    t.new("gamma", W, torch.float32, NAN, margin=8).base[:W] = 1 + 0.1 * torch.randn(W, generator=g)
    t.new("beta", W, torch.float32, NAN, margin=8).base[:W] = 0.1 * torch.randn(W, generator=g)
    t.new("out", M * ldo, torch.bfloat16, SENTINEL, margin=ldo).allow(0, M, W, ldo)
    t.x.update(ldz=ldz, ldo=ldo, P=P)
    return t


def reference_ln(c, t):
    M, W, P = c.M, c.W, t.x["P"]
    z = t.a["z"].bwin(0, M, W, t.x["ldz"]).double()
    st = t.a["stats"].before[t.a["stats"].off:][:M * P * 2].reshape(M, P, 2).double()
    mean, var = merge_stats(st, W)
    ga = t.a["gamma"].before[t.a["gamma"].off:][:W].double()
    be = t.a["beta"].before[t.a["beta"].off:][:W].double()
    out, rs = ln_apply(z, mean, var, ga, be, f32r(c.eps), torch.float64)
    unit = ULP * (((z - mean[:, None]).abs() + 2 * mean.abs()[:, None]) * rs[:, None] * ga.abs() + be.abs())
    return out, unit


def fake_ln(c, t, mode, faults):
    M, W, P = c.M, c.W, t.x["P"]
    dt = torch.float64 if mode == "f64" else torch.float32
    z = t.a["z"].win(0, M, W, t.x["ldz"]).to(dt)
    mean, var = merge_stats(t.a["stats"].base[:M * P * 2].reshape(M, P, 2), W, dt, faults)
    out, _ = ln_apply(z, mean, var, t.a["gamma"].base[:W].to(dt), t.a["beta"].base[:W].to(dt), f32r(c.eps), dt)
    t.a["out"].win(0, M, W, t.x["ldo"]).copy_(out.to(torch.bfloat16))


def check_ln(c, t, figs):
    ref, unit = reference_ln(c, t)
    a = t.a["out"]
    got = a.whole.cpu().as_strided((c.M, c.W), (t.x["ldo"], 1), a.off)
    check_float("out", "ln", got, ref, unit, True, figs)


# ---- producer -> consumer on device statistics ----
def make_chain(c):
    """producer: z = A W1^T + b + r (z_out, stats_out, N columns); consumer: C2 = LN(z) W2^T (K2 = N)"""
    t, g = Tensors(), gen(c)
    M, N, K = c.M, c.N, c.K
    bf = torch.bfloat16
    P = tiles_of(N)
    t.new("A", M * K, bf, NAN, margin=K).win(0, M, K, K).copy_(torch.randn(M, K, generator=g).to(bf))
    t.new("B", N * K, bf, NAN, margin=K).win(0, N, K, K).copy_((torch.randn(N, K, generator=g) * 0.5).to(bf))
    t.new("bias", N, torch.float32, NAN, margin=8).base[:N] = \
        (6.0 * torch.randn(P, generator=g)).repeat_interleave(64)[:N] + torch.randn(N, generator=g)
    t.new("r", M * N, bf, NAN, margin=N).win(0, M, N, N).copy_(torch.randn(M, N, generator=g).to(bf))
    t.new("z_out", M * N, torch.float32, SENTINEL, margin=N).allow(0, M, N, N)
    t.new("stats_out", M * P * 2, torch.float32, SENTINEL, margin=2 * P).allow(0, 1, M * P * 2, M * P * 2)
    t.new("gamma", N, torch.float32, NAN, margin=8).base[:N] = 1 + 0.1 * torch.randn(N, generator=g)
    t.new("beta", N, torch.float32, NAN, margin=8).base[:N] = 0.1 * torch.randn(N, generator=g)
    t.new("B2", 64 * N, bf, NAN, margin=N).win(0, 64, N, N).copy_((torch.randn(64, N, generator=g) * 0.5).to(bf))
    t.new("C2", M * 64, bf, SENTINEL, margin=64).allow(0, M, 64, 64)
    t.x["P"] = P
    return t


def fake_chain(c, t, mode, faults):
    M, N, K, P = c.M, c.N, c.K, t.x["P"]
    dt = torch.float64 if mode == "f64" else torch.float32
    v = t.a["A"].win(0, M, K, K).to(dt) @ t.a["B"].win(0, N, K, K).to(dt).T + t.a["bias"].base[:N].to(dt) + \
        t.a["r"].win(0, M, N, N).to(dt)
    v = v.float()
    t.a["z_out"].win(0, M, N, N).copy_(v)
    st = host_stats(v).float()
    t.a["stats_out"].base[:M * P * 2] = st.reshape(-1)
    mean, var = merge_stats(st, N, dt, faults)
    a, _ = ln_apply(v.to(dt), mean, var, t.a["gamma"].base[:N].to(dt), t.a["beta"].base[:N].to(dt), f32r(c.eps), dt)
    out = a.to(torch.bfloat16).to(dt) @ t.a["B2"].win(0, 64, N, N).to(dt).T
    t.a["C2"].win(0, M, 64, 64).copy_(out.to(torch.bfloat16))


def check_chain(c, t, figs):
    """the consumer's C2 against float64 LN (row statistics of the z_out as written) -- the device statistics only
    enter through the kernel -- and the producer's stats_out against z_out"""
    M, N, P = c.M, c.N, t.x["P"]
    zw = t.a["z_out"].whole.cpu()[t.a["z_out"].off:][:M * N].reshape(M, N).double()
    so = t.a["stats_out"].whole.cpu()[t.a["stats_out"].off:][:M * P * 2].reshape(M, P, 2)
    check_stats("stats_out", so, zw, N, figs)
    mean = zw.mean(1)
    var = ((zw - mean[:, None]) ** 2).mean(1)
    ga = t.a["gamma"].before[t.a["gamma"].off:][:N].double()
    be = t.a["beta"].before[t.a["beta"].off:][:N].double()
    a, rs = ln_apply(zw, mean, var, ga, be, f32r(c.eps), torch.float64)
    e = ULP * (((zw - mean[:, None]).abs() + 2 * mean.abs()[:, None]) * rs[:, None] * ga.abs() + be.abs())
    a = a.to(torch.bfloat16).double()
    B2 = t.a["B2"].bwin(0, 64, N, N).double()
    ref = a @ B2.T
    unit = ULP * (a.abs() @ B2.abs().T) + e @ B2.abs().T + \
        BF16_REL * torch.stack([(B2.abs() * a[m].abs()).amax(-1) for m in range(M)])
    got = t.a["C2"].whole.cpu()[t.a["C2"].off:][:M * 64].reshape(M, 64)
    check_float("C2", "gemm", got, ref, unit, True, figs)


# ------------------------------------------------------------------------------------------------
# the harness
# ------------------------------------------------------------------------------------------------
_MAKE = dict(attn=make_attn, kvstore=make_kvstore, embed=make_embed, pick=make_pick, pickadv=make_pick,
             pickkeys=make_pickkeys, gemm=make_gemm, argmax=make_argmax, ln=make_ln, chain=make_chain)
_CHECK = dict(attn=check_attn, kvstore=check_kvstore, embed=check_embed, pick=check_pick, pickadv=check_pick,
              pickkeys=check_pickkeys, gemm=check_gemm, argmax=check_argmax, ln=check_ln, chain=check_chain)


def make_tensors(c, device="cpu"):
    return _MAKE[c.op](c).to(device)


class FakeOps:
    """the contract in torch, on the case's buffers. mode: f64 | seq | tree (float32 emulations); faults: names"""

    def __init__(self, mode="f64", faults=()):
        self.mode, self.faults = mode, frozenset(faults)
        unknown = self.faults - set(FAULTS)
        assert not unknown, unknown

    def launch(self, c, t):
        fn = dict(attn=fake_attn, kvstore=fake_kvstore, embed=fake_embed, pick=fake_pick, pickadv=fake_pick,
                  pickkeys=fake_pickkeys, gemm=fake_gemm, argmax=fake_argmax, ln=fake_ln, chain=fake_chain)[c.op]
        fn(c, t, self.mode, self.faults)


def run_case(c, t, ops, twice=False, show=True):
    """launch, check against the reference and the guards; twice: restore, launch again, compare bitwise.
    Returns the figures [(kind, name, value)]; asserts each against BOUND after printing it."""
    figs = []
    t.snapshot()
    ops.launch(c, t)
    for name, a in t.a.items():
        a.check(name)
    _CHECK[c.op](c, t, figs)
    for kind, name, fig in figs:
        if show:
            print(f"{c.id}: {name} {fig:.3f} units of {kind} (bound {BOUND[kind]:.3f})")
    for kind, name, fig in figs:
        assert fig <= BOUND[kind], f"{c.id}: {name} is {fig:.3f} units of {kind} off the float64 reference, " \
                                   f"bound {BOUND[kind]:.3f}"
    if twice:
        first = {k: a.whole.detach().cpu().clone() for k, a in t.a.items()}
        t.restore()
        t.snapshot()
        ops.launch(c, t)
        for k, a in t.a.items():
            assert torch.equal(a.bits().cpu(), a.bits(first[k])), f"{c.id}: {k} differs between two launches"
    return figs


# ------------------------------------------------------------------------------------------------
# plans
# ------------------------------------------------------------------------------------------------
def attn_plan_args(c, t):
    """the arguments of mit_attention_decode(_plan) after dtype, as a dict"""
    G = t.x["G"]
    kv = t.a["kv"]
    return dict(B=c.B, H=c.H, Dh=c.Dh, q=t.a["q"].ptr(G["q_off"]), q_batch=G["q_batch"], k=kv.ptr(G["k_off"]),
                k_row=G["row"], k_batch=G["kv_batch"], v=kv.ptr(G["v_off"]), v_row=G["row"], v_batch=G["kv_batch"],
                o=t.a["o"].ptr(), o_batch=G["o_batch"], Lk=G["lk_arg"], pos=t.ptr("pos"), key_tokens=t.ptr("tok"))


def planned_attn(c, t, N):
    a = attn_plan_args(c, t)
    return N.attention_decode_plan(N.BF16 if c.dtype == "bf16" else N.F32, a["B"], a["H"], a["Dh"], a["q"],
                                   a["q_batch"], a["k"], a["k_row"], a["k_batch"], a["v"], a["v_row"], a["v_batch"],
                                   a["o"], a["o_batch"], Lk=a["Lk"], pos=a["pos"], key_tokens=a["key_tokens"])


def gemm_args(c, t, N):
    """the DecodeGemmArgs of a gemm / argmax case"""
    G = t.x["G"]
    g = N.DecodeGemmArgs()
    g.M, g.N, g.K = c.M, c.N, c.K
    g.A, g.lda = t.ptr("A"), G["lda"]
    g.a_stats, g.a_gamma, g.a_beta = t.ptr("a_stats"), t.ptr("a_gamma"), t.ptr("a_beta")
    g.B, g.ldb, g.bias = t.ptr("B"), G["ldb"], t.ptr("bias")
    g.act, g.c_f32 = c.act, 1 if c.c_f32 else 0
    g.C, g.ldc = t.ptr("C"), G["ldc"]
    g.r_mode, g.r, g.ldr = c.r_mode, t.ptr("r"), G["ldr"]
    g.r_stats, g.r_gamma, g.r_beta = t.ptr("r_stats"), t.ptr("r_gamma"), t.ptr("r_beta")
    g.eps = c.eps
    g.z_out, g.ldz, g.stats_out = t.ptr("z_out"), G["ldz"], t.ptr("stats_out")
    if c.cache:
        g.cache, g.c_row, g.c_batch, g.kv_col0, g.pos = t.ptr("cache"), G["c_row"], G["c_batch"], G["kv0"], t.ptr("pos")
    if c.op == "argmax":
        g.argmax_keys = t.ptr("keys")
    return g


def expected_gemm_plan(c):
    """(a_mode, act, r_mode, c_f32, waves, block_rows, grid, lds_bytes) by the rules of the header and DESIGN.md"""
    arg = c.op == "argmax"
    wide = not arg and (c.a_ln or c.K >= 512)
    nw, bmr = (8, 32) if wide else (4, 64)
    red = nw * bmr * 68 * 4
    lds = max(bmr * (c.K * 2 + 16), red) if c.a_ln else red
    return (1 if c.a_ln else 0, c.act, 3 if arg else c.r_mode, 1 if c.c_f32 else 0, nw, bmr,
            ((c.M + bmr - 1) // bmr) * ((c.N + 63) // 64), lds)


def plan_tuple(p):
    return (p.a_mode, p.act, p.r_mode, p.c_f32, p.waves, p.block_rows, p.grid, p.lds_bytes)


def check_plan(c, t, N):
    """the planned family of the case is the case's own"""
    if c.op == "attn":
        assert planned_attn(c, t, N) == FAMILY[c.family], f"{c.id}: planned {planned_attn(c, t, N)}"
    elif c.op in ("gemm", "argmax"):
        p = N.decode_gemm_plan(gemm_args(c, t, N))
        assert p is not None, f"{c.id}: rejected: {N.lib().mit_last_error()}"
        assert plan_tuple(p) == expected_gemm_plan(c), f"{c.id}: planned {plan_tuple(p)}"
        assert p.lds_bytes <= LDS_LIMIT


# ------------------------------------------------------------------------------------------------
# faults of the fake: name -> the cases that must catch it
# ------------------------------------------------------------------------------------------------
FAULTS = {
    # attention
    "one_key_more": ["attn-bh-bf16-d16-h8-lk33", "attn-rows-d64-lk197", "attn-rows_nt-d64-lk64"],
    "one_key_fewer": ["attn-bh-f32-d64-h2-lk1", "attn-rows-d64-lk65", "attn-rows_nt-d128-lk9"],
    "mask_ignored": ["attn-bh-mask-first-lk9", "attn-rows-mask-slab-lk70", "attn-rows_nt-key-tokens-no-pos"],
    "mask_vs_zero": ["attn-bh-mask-pad3-lk11", "attn-rows-mask-pad3-lk11", "attn-rows_nt-mask-pad3-lk11"],
    "tok_batch_lmax": ["attn-bh-tok-batch-pad", "attn-rows-tok-batch-pad", "attn-rows_nt-tok-batch-pad"],
    "lk_arg_used": ["attn-bh-bf16-d64-h3-lk9", "attn-rows-d64-lk9"],
    "no_rescale": ["attn-bh-hot-last", "attn-rows-d64-lk257", "attn-rows-hot-last", "attn-rows_nt-hot-last"],
    "no_log2e": ["attn-bh-f32-d32-h3-lk17", "attn-rows-d64-lk7"],
    "half_head": ["attn-bh-bf16-d128-h1-lk5", "attn-rows-d128-lk9", "attn-rows_nt-d128-lk65"],
    "wave_dropped": ["attn-bh-bf16-d64-h3-lk32", "attn-rows-d64-lk64", "attn-rows_nt-d64-lk257"],
    "all_masked_zero": ["attn-bh-mask-row_all-lk13", "attn-rows-mask-row_all-lk13", "attn-rows_nt-mask-row_all-lk13"],
    "o_batch_w": ["attn-bh-o-batch-pad", "attn-rows-o-batch-pad", "attn-rows_nt-o-batch-pad"],
    # kv_store / embed_decode
    "row_pos_plus_1": ["kvstore-bf16-n8-pos0", "kvstore-f32-n1024-pos4-s_pad"],
    "stops_at_grid_cap": ["kvstore-bf16-past-cap-2049x1024", "kvstore-f32-past-cap-2049x1024",
                          "embed-bf16-past-cap-2049x1024", "embed-f32-past-cap-2049x1024"],
    "ids_pos_plus_1": ["embed-bf16-d8-pos0", "embed-f32-d100-pos0-ids-pad"],
    "pe_row_0": ["embed-bf16-d100-pos4-ids-pad", "embed-f32-d8-pos2-ids-pad"],
    # greedy_pick
    "last_on_ties": ["pick-V4096-vec", "pick-V257-scalar-V%4-inf", "pick-V4-vec"],
    "nan_ignored": ["pick-V5-scalar-V%4-nan", "pick-V1024-vec"],
    "vector_reads_past_v": ["pick-V256-vec-ld-pad-inf", "pick-V4-vec-ld-pad-nan"],
    "pad_column_can_win": ["pick-V1024-scalar-ld-V+1-nan", "pick-V3-scalar-V%4-inf", "pick-V4096-scalar-ptr-off-1-inf"],
    "neg_zero_below": ["pick-V5-scalar-V%4-inf", "pick-V10000-vec"],
    "finished_counted_again": ["pick-V256-vec", "pickadv-B65-3-steps"],
    "pos_per_block": ["pickadv-B2", "pickadv-B300"],
    # greedy_pick_keys
    "keys_not_reset": ["pickkeys-B1", "pickkeys-B1024"],
    "rows_ge_1024_skipped": ["pickkeys-B1025", "pickkeys-B2049"],
    # decode_gemm
    "k_tail_dropped": ["gemm-plain-M1-N8-K8-C", "gemm-plain-M33-N72-K72-all-ld", "gemm-res-M64-N56-K520"],
    "odd_step_dropped": ["gemm-plain-M64-N56-K1088-z", "gemm-plain-M32-N72-K1536-Cz", "gemm-lnres-M31-N72-K1088-z"],
    "a_pad_read": ["gemm-res-M33-N72-K72-only-lda"],
    "row_ge_m": ["gemm-plain-M1-N8-K8-C", "gemm-ln-M5-N72-K136-only-lda"],
    "dm2_dropped": ["gemm-ln-tiles-eps1e-05-K136", "gemm-lnres-tiles-eps1e-12-N136", "ln-M3-W512",
                    "chain-M33-N136-K72"],
    "partial_tile_as_64": ["gemm-ln-mean50-eps1e-05-K136", "gemm-lnres-mean50-eps1e-05-N136", "ln-M1-W72"],
    "relu_after_residual": ["gemm-res-M33-N72-K72-only-none", "gemm-lnres-M33-N136-K520-only-none"],
    "cache_col_mod_64": ["gemm-plain-cache-kv8-pos0", "gemm-ln-cache-kv72-pos3"],
    "cache_row_pos_plus_1": ["gemm-plain-cache-kv0-pos0", "gemm-ln-cache-kv64-pos3"],
    "f32_c_through_bf16": ["gemm-ln-f32-M32-N1032-K512-C", "gemm-ln-f32-M65-N136-K504-C"],
    "stats_before_bias": ["gemm-plain-M1-N8-K72-all-ld"],
    "slot_mod_8": ["argmax-V1088-M1-rand", "argmax-V1024-M70-rand"],
    "col_ge_v_can_win": ["argmax-V7-M1-rand", "argmax-V509-M70-rand", "argmax-V1001-M1-neg"],
}


def fake_figures(cases=None):
    """kind -> {mode: (worst figure, case id)} of the float32 FakeOps"""
    out = {}
    for c in cases or CASES:
        if c.op not in ("attn", "gemm", "ln", "chain"):
            continue
        for mode in ("seq", "tree"):
            t = make_tensors(c)
            t.snapshot()
            FakeOps(mode).launch(c, t)
            figs = []
            _CHECK[c.op](c, t, figs)
            for kind, name, fig in figs:
                cur = out.setdefault(kind, {}).get(mode, (0.0, None))
                if fig > cur[0]:
                    out[kind][mode] = (fig, c.id + ":" + name)
    return out


if __name__ == "__main__":
    for kind, d in sorted(fake_figures().items()):
        print(kind, {m: (round(v, 3), i) for m, (v, i) in d.items()})
