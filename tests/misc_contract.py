"""The contract of csrc/misc.hip's entry points (include/mit_hip.h) -- mit_cross_entropy, mit_count_targets,
mit_embed_fwd / _plan / _bwd, mit_colsum, mit_grad_norm, mit_adamw, mit_im2col, mit_vit_assemble, mit_cast_f32,
mit_dropout_mask, mit_scalar_div, mit_step_inc -- as a case table and a harness, in the manner of
tests/ln_contract.py (it reuses gemm_contract's guarded `Buf`, `untouched` and bitwise comparison).

Buffers. Every operand and output of a case is a gemm_contract.Buf with 64-element guards; inputs are NaN outside
their windows (integer inputs hold a valid index there), outputs hold a finite sentinel. ws, row_loss, plan,
norm_out, dtable, the AdamW vectors and every operand the kernels address densely (dx, table, pe, img, out of
im2col, patch / h of assemble) are exact-size; logits and colsum's dy carry ld = cols + 8 or + 16 except where the
case is about ld. Every case is a valid call: targets and token ids are in range, rejections are tested through
return codes (REJECTIONS) and never launched.

Inputs give every term weight. Cross-entropy: logits 3 randn plus a per-row offset in +-20; row 0's maximum sits
in its last valid column, row 1 is flat (all equal: its loss is log V), row 3 has one logit 60 above the rest;
targets sit at column 0, at V - 1 and at the start of the last 16-B chunk; `count` is the local count + 3 (the global
count of a data-parallel step). Gradients of mixed magnitude 1e-3 .. 1e3 for the norm, random (p, m, v >= 0) states
for AdamW.

`reference` evaluates the header's formulas in float64 from the dtype-rounded windows (dropout masks from
mit_dropout_mask on the GPU -- itself compared bit for bit with `host_mask`, an integer implementation of the
documented hash -- and a fixed torch mask on the CPU). `run_case` drives an `ops` object -- the native library in
tests/test_misc_contract_gpu.py, `FakeOps` (torch, with injectable faults) in tests/test_misc_contract_cpu.py.

Bounds. f32 quantities are measured in conditioning units (gs = 1 / count, p = softmax, mx = the row maximum):
  ce row loss   2^-23 (|lse| + |x_t|);   loss_sum 2^-23 (|loss_sum before| + sum_rows (|lse| + |x_t|))
  ce gradient   2^-23 gs p_j (1 + log2(e) (|x_j| + |mx|)), plus 2^-23 gs at the target (the exponent of the
                wave-per-row kernel is x_j log2(e) - (mx log2(e) + log2(se) - log2(gs)): one rounding of each term)
  embed_fwd     2^-23 (|table scale| + |pe|) mask   (the product and the sum round once each, or fuse)
  embed_bwd     2^-23 sum_positions |dx scale mask|  (+ 2^-23 |dtable before| on the atomic path)
  colsum        2^-23 (sum_m |dy| + |out before| with accumulate)
  norm          2^-23 norm;   coef 2^-23 coef
  adamw         m: 2^-23 (|m| + |g'|);  v: 2^-23 v';  p: 2^-23 (|p| + K step_size (|m'| + |m| + |g'|) / denom), K = 4
                (g' = coef g; m', v' the new moments; the quotient m' / denom passes through six roundings: v', its
                root, the two bias corrections, the sum with eps and the division)
BOUND[q] is 4 x the worst figure of FakeOps in float32 over the whole table, under both of its modes: "seq"
(sequential sums, exp / log as written in the header) and "tree" (the kernels' 64-lane tree, exp2 / log2 with the
folded exponent) -- `python tests/misc_contract.py` prints them; the margin covers a third summation order and the
hardware's exp2 / log2. bf16 outputs: |got - ref| <= 2^-8 |ref| + the f32 bound.
Exact, no tolerance: the sort plan, ignored rows (0), untouched rows / padding, want_grad == 0 (logits bitwise
unchanged), bitwise repeats of the deterministic paths, im2col, assemble, cast (against torch.Tensor.to; a NaN's
image is 0x7FC0, see `to_dtype`), mask, counts, coef == 1 where stated, the shadow (bf16 of the written p).
"""
import math
import zlib
from dataclasses import dataclass

import torch

import gemm_contract as gc
from gemm_contract import GUARD, NAN, SENTINEL, Buf

_TORCH = {"bf16": torch.bfloat16, "f32": torch.float32}
ULP = 2.0 ** -23
BF16_REL = 2.0 ** -8
L2E = 1.4426950408889634
CE_BLOCK, CE_ROWS = 0, 1        # mit_cross_entropy_plan
ELT_SCALAR, ELT_VEC8 = 0, 1     # mit_im2col_plan / mit_vit_assemble_plan
CE_IGNORE = -100
CE_ROWS_MAX_V = 10240           # CE_NCH * 512
PAD = 0
GRID_CAP = 8192 * 256           # elements one trip of the grid-stride loops covers
CS_ROWS = 128                   # rows per partial of mit_colsum
GN_BLOCKS = 1024                # mit_grad_norm_ws_floats


def f32r(x):
    """x as the float32 the C ABI passes"""
    return float(torch.tensor(x, dtype=torch.float32))


B1, B2, EPS = f32r(0.9), f32r(0.999), f32r(1e-8)  # the hyper-parameters as the kernel receives them
ADAM_K = 4.0
EMB_VOCAB = 50                  # embed_plan cases
BWD_RUNS = (1, 15, 16, 17, 33)  # rows of tokens 1..5 in the embed_bwd layouts (tokens 6, 7 absent)
BWD_VOCAB, BWD_PADS = 8, 6

# 4 x the worst FakeOps float32 figure over the table, in the units above (measured worst: seq / tree, and the case)
BOUND = {
    "ce_loss": 4 * 5.208,  # 5.208 (ce-block-10248) / 0.836 (ce-rows-10240)
    "ce_sum": 4 * 1.670,   # 1.670 (ce-rows-10240-dense) / 0.604 (ce-rows-509-nograd)
    "ce_grad": 4 * 0.500,  # 0.500 / 0.375 (ce-block-f32-512); bf16 outputs: 0 past 2^-8 |ref| in both modes
    "emb_fwd": 4 * 1.301,  # 1.301 / 1.301 (embfwd-f32-512-p0.1-seed-none); no sums: the modes agree
    "emb_bwd": 4 * 1.961,  # 1.961 / 1.961 (embbwd-atomic-f32-130-p0.1): runs are summed in position order in both
    "colsum": 4 * 2.492,   # 2.492 / 2.492 (colsum-f32-128x300-ld300): 128 rows one after the other in both
    "norm": 4 * 0.803,     # 0.803 / 0.803 (gnorm-262147-max0.5x)
    "coef": 4 * 1.135,     # 1.135 / 1.135 (gnorm-262147-max0.5x)
    "adam_m": 4 * 0.493,   # 0.493 / 0.493 (adamw-4098-norm-t1-wd0.1-coef0.25)
    "adam_v": 4 * 1.008,   # 1.008 / 1.008 (adamw-4098-shadow-t1000-wd0.1-coef1)
    "adam_p": 4 * 1.011,   # 1.011 / 1.011 (adamw-4098-norm-t1-wd0.1-coef0.25), with K = 4
}


# ------------------------------------------------------------------------------------------------
# the case table
# ------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    id: str
    op: str                # a method of `ops`: ce, count, embfwd, embplan, embbwd, colsum, gnorm, adamw, adamchain, ...
    dtype: str = "bf16"
    plan: int = None       # the family / key count the call must plan onto
    rows: int = 0          # ce rows, colsum M
    cols: int = 0          # ce V, colsum N, embedding d, vector length n
    ld: int = 0
    mis: tuple = ()        # ((buffer, elements moved off 16-B alignment), ...)
    row_loss: bool = True
    ignore: str = "third"  # ce: third | all | none
    want_grad: bool = True
    loss0: float = 0.0
    B: int = 0
    T: int = 0
    drop_p: float = 0.0
    seed: str = "small"    # none | small | big (above 2^32)
    site: int = 5
    layout: str = "runs"   # embbwd: runs | allpad
    planned: bool = True   # embbwd: with a plan / float atomics
    accumulate: bool = False
    geom: tuple = None     # im2col (C, H, W, P, kpad); assemble (np, E)
    gmode: str = "mixed"   # gnorm: mixed | zero
    max_norm: float = 2.0  # gnorm: a multiple of the reference norm when > 0 and gmode == mixed
    shadow: bool = True
    norm: bool = True
    coef: float = 1.0
    step: int = 1
    wd: float = 0.0
    lr: float = 1e-3

    def misalign(self, name):
        return dict(self.mis).get(name, 0)


def r8(v):
    return (v + 7) // 8 * 8


def kpt_of(n):
    """embed_plan_kernel<KPT>: the keys per thread mit_embed_plan sorts n positions with"""
    np2 = 1024
    while np2 < n:
        np2 *= 2
    return 0 if n == 0 else np2 // 1024


def _build_cases():
    cs = []

    def ce(id, dtype, rows, V, plan, ld=None, **kw):
        if ld is None:
            ld = r8(V) if V % 8 else V + (8 if len(cs) % 2 else 16)
        cs.append(Case("ce-" + id, "ce", dtype, plan, rows, V, ld, **kw))

    # ---- ce_rows_bf16: V % 8 == 0 (ld >= V, % 8), then V % 8 != 0 (ld = round8(V)); 10240 = 20 full chunks ----
    R = CE_ROWS
    ce("rows-8", "bf16", 1, 8, R, ignore="none")
    ce("rows-512", "bf16", 4, 512, R, loss0=3.5)
    ce("rows-520", "bf16", 5, 520, R, ignore="none")
    ce("rows-10240", "bf16", 9, 10240, R)
    ce("rows-7", "bf16", 5, 7, R)                   # a lone masked chunk
    ce("rows-509", "bf16", 9, 509, R, ignore="none", loss0=3.5)
    ce("rows-10233", "bf16", 4, 10233, R)           # a tail in the 20th chunk
    ce("rows-509-all-ignored", "bf16", 5, 509, R, ignore="all")
    ce("rows-512-all-ignored", "bf16", 4, 512, R, ignore="all", loss0=3.5)
    ce("rows-512-nograd", "bf16", 9, 512, R, want_grad=False)
    ce("rows-509-nograd", "bf16", 4, 509, R, ignore="none", want_grad=False, loss0=3.5)
    ce("rows-10240-dense", "bf16", 1, 10240, R, ld=10240, ignore="none")
    # ---- ce_kernel<T>: over the limit, and by fallback ----
    K = CE_BLOCK
    ce("block-10241", "bf16", 4, 10241, K, ld=10241 + 8)
    ce("block-10248", "bf16", 5, 10248, K, ignore="none", loss0=3.5)
    ce("block-f32-512", "f32", 9, 512, K)
    ce("block-f32-512-no-row-loss", "f32", 5, 512, K, row_loss=False, ignore="none", loss0=3.5)
    ce("block-bf16-512-no-row-loss", "bf16", 4, 512, K, row_loss=False)
    ce("block-bf16-512-misaligned", "bf16", 5, 512, K, mis=(("logits", 4),), ignore="none")
    ce("block-520-ld523", "bf16", 9, 520, K, ld=523, loss0=3.5)
    ce("block-f32-300", "f32", 4, 300, K)           # 256-thread tails
    ce("block-bf16-300-no-row-loss", "bf16", 1, 300, K, row_loss=False, ignore="none")
    ce("block-f32-509", "f32", 5, 509, K, ld=512, ignore="none")
    ce("block-f32-512-all-ignored", "f32", 5, 512, K, ignore="all", loss0=3.5)
    ce("block-bf16-509-all-ignored", "bf16", 4, 509, K, ld=515, ignore="all", row_loss=False)
    ce("block-bf16-512-nograd", "bf16", 4, 512, K, row_loss=False, want_grad=False, loss0=3.5)
    ce("block-f32-300-nograd", "f32", 9, 300, K, want_grad=False, ignore="none")
    # ---- mit_count_targets: 40000 is past the 64-block cap ----
    for n in (1, 255, 16385, 40000):
        cs.append(Case(f"count-{n}", "count", cols=n))
    # ---- mit_embed_fwd ----
    i = 0
    for dtype in ("bf16", "f32"):
        for d in (8, 130, 512):
            for p in (0.0, 0.1):
                seed = ("small", "big", "none")[i % 3]
                cs.append(Case(f"embfwd-{dtype}-{d}-p{p:g}-seed-{seed}", "embfwd", dtype, B=3, T=5, cols=d, drop_p=p,
                               seed=seed, site=(5, 0)[i % 2]))
                i += 1
    cs.append(Case("embfwd-past-cap-4x17x32768", "embfwd", "bf16", B=4, T=17, cols=32768, drop_p=0.1, seed="big"))
    # ---- mit_embed_plan: both sides of every key count per thread ----
    for n in (1, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 16384):
        cs.append(Case(f"embplan-{n}", "embplan", cols=n, plan=kpt_of(n)))
    # ---- mit_embed_bwd: planned (d % 8 == 0), then float atomics ----
    i = 0
    for dtype in ("bf16", "f32"):
        for d in (8, 128, 520, 1024):
            for p in (0.0, 0.1):
                cs.append(Case(f"embbwd-plan-{dtype}-{d}-p{p:g}", "embbwd", dtype, B=2, T=44, cols=d, drop_p=p,
                               seed=("small", "big", "none")[i % 3]))
                i += 1
        cs.append(Case(f"embbwd-plan-{dtype}-all-pad", "embbwd", dtype, B=2, T=5, cols=128, layout="allpad"))
        for d in (8, 130):
            for p in (0.0, 0.1):
                cs.append(Case(f"embbwd-atomic-{dtype}-{d}-p{p:g}", "embbwd", dtype, B=2, T=44, cols=d, drop_p=p,
                               planned=False))
        cs.append(Case(f"embbwd-atomic-{dtype}-all-pad", "embbwd", dtype, B=2, T=5, cols=130, layout="allpad",
                       planned=False))
    # ---- mit_colsum ----
    for dtype in ("bf16", "f32"):
        for M in (0, 1, 127, 128, 129, 257):
            for N in (1, 256, 300):
                for pad in (0, 8):
                    for acc in (False, True):
                        cs.append(Case(f"colsum-{dtype}-{M}x{N}-ld{N + pad}{'-acc' if acc else ''}", "colsum", dtype,
                                       rows=M, cols=N, ld=N + pad, accumulate=acc))
    # ---- mit_grad_norm ----
    for n in (1, 3, 4, 5, 1027, 262144 + 3):
        for mul in (0.5, 2.0):
            cs.append(Case(f"gnorm-{n}-max{mul:g}x", "gnorm", cols=n, max_norm=mul))
    cs.append(Case("gnorm-zero-grad", "gnorm", cols=1027, gmode="zero", max_norm=1.0))
    cs.append(Case("gnorm-max-norm-0", "gnorm", cols=1027, max_norm=0.0))
    cs.append(Case("gnorm-max-norm-neg", "gnorm", cols=5, max_norm=-1.0))
    # ---- mit_adamw: one step from a given state ----
    i = 0
    for n in (1, 3, 4, 7, 1024 * 4 + 2):
        for shadow in (True, False):
            for norm in (True, False):
                step, wd = (1, 2, 1000)[i % 3], (0.0, 0.1)[(i + i // 2) % 2]
                coef = (0.25, 1.0)[(i // 4) % 2] if norm else 1.0
                cs.append(Case(f"adamw-{n}{'-shadow' if shadow else ''}{'-norm' if norm else ''}-t{step}-wd{wd:g}"
                               f"-coef{coef:g}", "adamw", cols=n, shadow=shadow, norm=norm, coef=coef, step=step, wd=wd,
                               lr=(1e-3, 3e-4, 2.5e-2)[i % 3]))
                i += 1
    cs.append(Case("adamw-chain-5-steps", "adamchain", cols=1024 * 4 + 2, wd=0.1, lr=1e-3))
    # ---- mit_im2col: B = 2, H != W ----
    geoms = [((3, 32, 48, 16, 768), ELT_VEC8), ((3, 32, 48, 16, 776), ELT_VEC8), ((3, 28, 42, 14, 592), ELT_SCALAR),
             ((1, 16, 8, 8, 64), ELT_VEC8)]
    for g, fam in geoms:
        tag = "x".join(str(v) for v in g)
        cs.append(Case(f"im2col-bf16-{tag}", "im2col", "bf16", plan=fam, B=2, geom=g))
        cs.append(Case(f"im2col-f32-{tag}", "im2col", "f32", plan=ELT_SCALAR, B=2, geom=g))
    cs.append(Case("im2col-bf16-3x32x48x16x776-out-off-8B", "im2col", "bf16", plan=ELT_SCALAR, B=2,
                   geom=(3, 32, 48, 16, 776), mis=(("out", 4),)))
    # ---- mit_vit_assemble ----
    for dtype in ("bf16", "f32"):
        for E in (8, 96, 100):
            for np_ in (1, 6):
                fam = ELT_VEC8 if dtype == "bf16" and E % 8 == 0 else ELT_SCALAR
                cs.append(Case(f"assemble-{dtype}-np{np_}-E{E}", "assemble", dtype, plan=fam, B=2, geom=(np_, E)))
    cs.append(Case("assemble-bf16-np6-E96-h-off-8B", "assemble", "bf16", plan=ELT_SCALAR, B=2, geom=(6, 96),
                   mis=(("h", 4),)))
    # ---- cast, mask, scalars ----
    cs.append(Case("cast-bf16-specials", "cast", "bf16", cols=0))
    cs.append(Case("cast-bf16-1", "cast", "bf16", cols=1))
    cs.append(Case("cast-bf16-past-cap", "cast", "bf16", cols=GRID_CAP + 5))
    cs.append(Case("cast-f32-specials", "cast", "f32", cols=0))
    for p in (0.1, 0.5):
        for site in (0, 7):
            for seed in ("none", "small", "big"):
                cs.append(Case(f"mask-p{p:g}-site{site}-seed-{seed}", "mask", cols=4096, drop_p=p, site=site, seed=seed))
    cs.append(Case("scalar-div", "sdiv"))
    cs.append(Case("step-inc", "stepinc"))
    assert len({c.id for c in cs}) == len(cs)
    return cs


CASES = _build_cases()
BY_ID = {c.id: c for c in CASES}

# rejected calls: (id, entry point, a fragment of the message)
REJECTIONS = [
    ("gnorm-misaligned", "gnorm", b"16-B aligned"),
    ("adamw-p-misaligned", "adamw-p", b"16-B aligned"),
    ("adamw-g-misaligned", "adamw-g", b"16-B aligned"),
    ("adamw-m-misaligned", "adamw-m", b"16-B aligned"),
    ("adamw-v-misaligned", "adamw-v", b"16-B aligned"),
    ("adamw-shadow-misaligned", "adamw-shadow", b"8-B aligned"),
    ("ce-ld-short", "ce-ld", b"ld < V"),
    ("ce-null", "ce-null", b"null pointer"),
    ("im2col-H-not-multiple", "im2col-H", b"bad arguments"),
    ("im2col-kpad-short", "im2col-kpad", b"bad arguments"),
    ("assemble-null", "assemble-null", b"null pointer"),
    ("embplan-16385", "embplan-n", b"positions"),
    ("embbwd-plan-d-130", "embbwd-d", b"deterministic path"),
    ("colsum-ld-short", "colsum-ld", b"bad arguments"),
]


# ------------------------------------------------------------------------------------------------
# tensors of a case
# ------------------------------------------------------------------------------------------------
class Tensors:
    """b: name -> Buf; init: name -> the buffers' first contents; outputs: the names the entry point writes."""

    def __init__(self):
        self.b, self.init, self.outputs, self.mask, self.x = {}, {}, set(), None, {}

    def v(self, name):
        return self.b[name].view if name in self.b else None

    def row(self, name):
        return self.b[name].view[0] if name in self.b else None

    def restore(self):
        for n, b in self.b.items():
            b.whole.copy_(self.init[n])


SEEDS = {"none": None, "small": 5, "big": 2 ** 40 + 3}


def ce_targets(c):
    """row -> target column: 0, V - 1, the start of the last 16-B chunk, then spread; CE_IGNORE where ignored"""
    V = c.cols
    base = [0, V - 1, (V - 1) // 8 * 8, (V - 1) // 8 * 8, V // 3, V - 1, 0, V // 2, (V - 1) // 8 * 8 + (V - 1) % 8 // 2]
    tg = [base[r % len(base)] for r in range(c.rows)]
    if c.rows == 1:
        tg = [V - 1]
    for r in range(c.rows):
        if c.ignore == "all" or (c.ignore == "third" and r % 3 == 2):
            tg[r] = CE_IGNORE
    return torch.tensor(tg, dtype=torch.int64)


def embbwd_tokens(c, g):
    n = c.B * c.T
    if c.layout == "allpad":
        return torch.full((n,), PAD, dtype=torch.int64)
    ids = [PAD] * BWD_PADS
    for tok, run in enumerate(BWD_RUNS, start=1):
        ids += [tok] * run
    assert len(ids) == n
    return torch.tensor(ids, dtype=torch.int64)[torch.randperm(n, generator=g)]


def plan_tokens(n, g):
    tok = torch.randint(0, EMB_VOCAB, (n,), generator=g)
    tok[::17] = 7
    if n > 2:
        tok[1], tok[2] = 0, EMB_VOCAB - 1
    return tok


CAST_SPECIALS = [
    0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,  # ties: to even down, to even up, and their negatives
    0x3F808001, 0x3F807FFF,                          # just above / below a tie
    0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000,  # +-0, +-inf, NaN
    0x7F7FFFFF, 0xFF7FFFFF,                          # the largest float32: rounds to inf
    0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x807FFFFF, 0x00800000,  # subnormals, the smallest normal
    0x3F800000, 0x40490FDB,
]


def to_dtype(src, dtype):
    """torch.Tensor.to(dtype) of an f32 vector, with one thing pinned down: torch's CPU conversion of a NaN to
    bfloat16 gives 0x7FC0 on its scalar path and 0xFFFF on its vectorised one (which of the two depends on the host
    and on the element's position), so a NaN's image is taken as the upper half of its quieted bits instead."""
    out = src.to(dtype)
    if dtype == torch.bfloat16 and src.isnan().any():
        hi = ((src.view(torch.int32) >> 16) | 0x40).to(torch.int16).view(torch.bfloat16)
        out = torch.where(src.isnan(), hi, out)
    return out


def make_tensors(case, device="cpu", mask_fn=None):
    """The guarded buffers of the case, seeded by its id. mask_fn(n, p, seed, site) -> f32 [n] keep-multipliers
    (mit_dropout_mask on the GPU); without it a fixed Bernoulli mask."""
    c = case
    g = torch.Generator().manual_seed(zlib.crc32(c.id.encode()))
    t = Tensors()
    f32, i64 = torch.float32, torch.int64

    def put(name, rows, cols, ld, dtype, data=None, out=False, fill=None):
        if fill is None:
            fill = SENTINEL if (out and data is None) else NAN if dtype.is_floating_point else 1
        t.b[name] = Buf(rows, cols, ld, dtype, fill, c.misalign(name), device, data)
        if out:
            t.outputs.add(name)

    def vec(name, n, dtype, data=None, out=False, fill=None):
        put(name, 1, n, n, dtype, None if data is None else data.reshape(1, -1), out, fill)

    def seed_and_mask(n):
        s = SEEDS[c.seed]
        if s is not None:
            vec("seed", 1, i64, torch.tensor([s]))
        if c.drop_p > 0:
            if mask_fn is not None:
                t.mask = mask_fn(n, c.drop_p, t.row("seed"), c.site).cpu()
            else:
                t.mask = (torch.rand(n, generator=g) >= c.drop_p).float() / (1.0 - c.drop_p)

    dt = _TORCH[c.dtype]
    if c.op == "ce":
        rows, V = c.rows, c.cols
        x = 3 * torch.randn(rows, V, generator=g) + (torch.rand(rows, 1, generator=g) * 40 - 20)
        if rows >= 4:
            x[0, V - 1] = x[0].max() + 25.0  # the maximum in the last valid column
            x[1] = x[1, 0]                   # flat
            x[3, V // 2] = x[3].max() + 60.0  # peaked
        tg = ce_targets(c)
        put("logits", rows, V, c.ld, dt, x, out=c.want_grad)
        vec("targets", rows, i64, tg)
        vec("count", 1, f32, torch.tensor([float((tg != CE_IGNORE).sum()) + 3.0]))
        vec("loss_sum", 1, f32, torch.tensor([c.loss0]), out=True)
        if c.row_loss:
            vec("row_loss", rows, f32, out=True)
    elif c.op == "count":
        tg = torch.randint(0, 4, (c.cols,), generator=g)  # 0 = the ignored index, a quarter of them
        vec("targets", c.cols, i64, tg)
        vec("count", 1, f32, torch.tensor([2.0]), out=True)
    elif c.op == "embfwd":
        n, d = c.B * c.T, c.cols
        vocab = 11
        vec("tokens", n, i64, torch.randint(0, vocab, (n,), generator=g))
        put("table", vocab, d, d, dt, torch.randn(vocab, d, generator=g))
        put("pe", c.T + 2, d, d, f32, torch.randn(c.T + 2, d, generator=g))
        vec("out", n * d, dt, out=True)
        seed_and_mask(n * d)
    elif c.op == "embplan":
        n = c.cols
        vec("tokens", n, i64, plan_tokens(n, g))
        vec("plan", 2 * n, torch.int32, out=True, fill=-7)
    elif c.op == "embbwd":
        n, d = c.B * c.T, c.cols
        vec("tokens", n, i64, embbwd_tokens(c, g))
        put("dx", n, d, d, dt, torch.randn(n, d, generator=g) + 0.25)
        if c.planned:
            vec("plan", 2 * n, torch.int32, out=True, fill=-7)
            put("dtable", BWD_VOCAB, d, d, f32, out=True)
        else:
            put("dtable", BWD_VOCAB, d, d, f32, 0.5 * torch.randn(BWD_VOCAB, d, generator=g) + 1.0, out=True)
        seed_and_mask(n * d)
    elif c.op == "colsum":
        M, N = c.rows, c.cols
        put("dy", max(M, 1), N, c.ld, dt, torch.randn(max(M, 1), N, generator=g) + 0.3)
        vec("out", N, f32, torch.randn(N, generator=g) * 3 + 1.0, out=True)
        nws = (M + CS_ROWS - 1) // CS_ROWS * N
        vec("ws", max(nws, 1), f32, out=True)
    elif c.op == "gnorm":
        n = c.cols
        gr = torch.randn(n, generator=g) * 10 ** (torch.rand(n, generator=g) * 6 - 3)
        if c.gmode == "zero":
            gr.zero_()
        vec("grads", n, f32, gr)
        vec("ws", GN_BLOCKS, f32, out=True)
        vec("norm_out", 2, f32, out=True)
        mx = c.max_norm
        if c.gmode == "mixed" and mx > 0:
            mx = float(torch.tensor(mx * gr.double().norm().item(), dtype=f32))
        t.x["max_norm"] = mx
    elif c.op in ("adamw", "adamchain"):
        n = c.cols
        vec("p", n, f32, torch.randn(n, generator=g), out=True)
        vec("g", n, f32, torch.randn(n, generator=g) * 10 ** (torch.rand(n, generator=g) * 2 - 1))
        if c.op == "adamchain":
            vec("m", n, f32, torch.zeros(n), out=True)
            vec("v", n, f32, torch.zeros(n), out=True)
        else:
            vec("m", n, f32, 0.3 * torch.randn(n, generator=g), out=True)
            vec("v", n, f32, (0.3 * torch.randn(n, generator=g)) ** 2, out=True)
        if c.shadow:
            vec("shadow", n, torch.bfloat16, out=True)
        if c.norm:
            vec("norm_out", 2, f32, torch.tensor([7.0, c.coef]))
        vec("lr", 1, f32, torch.tensor([0.5]), out=c.op == "adamchain")  # changed before every launch
        vec("step", 1, i64, torch.tensor([0 if c.op == "adamchain" else c.step]), out=c.op == "adamchain")
    elif c.op == "im2col":
        C, H, W, P, kpad = c.geom
        vec("img", c.B * C * H * W, f32, torch.randn(c.B * C * H * W, generator=g))
        np_ = (H // P) * (W // P)
        put("out", c.B * np_, kpad, kpad, dt, out=True)
    elif c.op == "assemble":
        np_, E = c.geom
        put("patch", c.B * np_, E, E, dt, torch.randn(c.B * np_, E, generator=g))
        vec("cls", E, f32, torch.randn(E, generator=g))
        put("pos", np_ + 1, E, E, f32, torch.randn(np_ + 1, E, generator=g))
        put("h", c.B * (np_ + 1), E, E, dt, out=True)
    elif c.op == "cast":
        if c.cols == 0:
            src = torch.tensor([v - 2 ** 32 if v >= 2 ** 31 else v for v in CAST_SPECIALS], dtype=torch.int32).view(f32)
        else:
            src = torch.randn(c.cols, generator=g) * 10 ** (torch.rand(c.cols, generator=g) * 8 - 4)
        vec("src", src.numel(), f32, src)
        vec("dst", src.numel(), dt, out=True)
    elif c.op == "mask":
        s = SEEDS[c.seed]
        if s is not None:
            vec("seed", 1, i64, torch.tensor([s]))
        vec("out", c.cols, f32, out=True)
    elif c.op == "sdiv":
        vec("a", 1, f32, torch.tensor([7.25]))
        vec("b", 1, f32, torch.tensor([3.0]))
        vec("out", 1, f32, out=True)
    elif c.op == "stepinc":
        vec("step", 1, i64, torch.tensor([2 ** 33 + 41]), out=True)
    else:
        raise ValueError(c.op)
    t.init = {n: b.whole.clone() for n, b in t.b.items()}
    return t


# ------------------------------------------------------------------------------------------------
# the documented dropout hash on the host (csrc/common.h: site_key, key_fold, lowbias32, drop_threshold)
# ------------------------------------------------------------------------------------------------
M32 = 0xFFFFFFFF


def _mul32(x, k):
    """x * k mod 2^32 on int64 tensors holding 32-bit values, without overflowing 64 bits"""
    lo, hi = k & 0xFFFF, k >> 16
    return (x * lo + (((x * hi) & 0xFFFF) << 16)) & M32


def _lowbias32(x):
    x = x ^ (x >> 16)
    x = _mul32(x, 0x7feb352d)
    x = x ^ (x >> 15)
    x = _mul32(x, 0x846ca68b)
    return x ^ (x >> 16)


def host_mask(n, p, seed, site):
    """f32 [n]: the keep-multipliers of mit_dropout_mask(n, p, seed, site), from the header's rule"""
    key = (seed or 0) ^ ((0xD6E8FEB86659FD93 * (site + 1)) & 0xFFFFFFFFFFFFFFFF)
    k = (key & M32) ^ (((key >> 32) * 0x9E3779B9) & M32)
    idx = torch.arange(n, dtype=torch.int64)  # below 2^32: the index's high half is 0
    h = _lowbias32((idx & M32) ^ k)
    pf = torch.tensor(p, dtype=torch.float32)
    thresh = int(min(pf.double().item() * 4294967296.0, 4294967295.0))
    scale = (torch.tensor(1.0) / (torch.tensor(1.0) - pf)).float()
    return torch.where(h >= thresh, scale, torch.zeros((), dtype=torch.float32))


# ------------------------------------------------------------------------------------------------
# the contract in float64
# ------------------------------------------------------------------------------------------------
def unfold_index(c):
    """[B * np, kpad] int64: the flat index into img of every output column, -1 in the padding"""
    C, H, W, P, kpad = c.geom
    nph, npw = H // P, W // P
    row = torch.arange(c.B * nph * npw).view(-1, 1)
    col = torch.arange(kpad).view(1, -1)
    b, p = row // (nph * npw), row % (nph * npw)
    ch, ky, kx = col // (P * P), (col // P) % P, col % P
    y, x = (p // npw) * P + ky, (p % npw) * P + kx
    idx = ((b * C + ch) * H + y) * W + x
    return torch.where(col < C * P * P, idx, torch.full_like(idx, -1))


def stable_plan(tok):
    """int32 [2n]: positions in stable token order, then the run length at the first slot of each token"""
    n = tok.numel()
    perm = torch.sort(tok, stable=True).indices
    st = tok[perm]
    lens = torch.zeros(n, dtype=torch.int64)
    first = torch.ones(n, dtype=torch.bool)
    first[1:] = st[1:] != st[:-1]
    starts = first.nonzero().flatten()
    ends = torch.cat([starts[1:], torch.tensor([n])])
    lens[starts] = ends - starts
    return torch.cat([perm, lens]).to(torch.int32)


def adam_step64(p, g, m, v, lr, step, wd, coef):
    """torch/optim/adam.py _single_tensor_adam (decoupled weight decay) in float64, and the units"""
    g, wd = g * coef, f32r(wd)
    p1 = p * (1 - lr * wd)
    m1 = m + (1 - B1) * (g - m)
    v1 = v * B2 + (1 - B2) * g * g
    bc1, bc2 = 1 - B1 ** step, 1 - B2 ** step
    step_size = lr / bc1
    denom = v1.sqrt() / math.sqrt(bc2) + EPS
    p2 = p1 - step_size * (m1 / denom)
    u = dict(u_m=ULP * (m.abs() + g.abs()), u_v=ULP * v1,
             u_p=ULP * (p.abs() + ADAM_K * step_size * (m1.abs() + m.abs() + g.abs()) / denom))
    return p2, m1, v1, u


CHAIN_LR = (1e-3, 1e-3, 4e-4, 4e-4, 4e-4)  # lr changes at step 3


def reference(case, t):
    """float64 CPU evaluation of the header's formulas from the dtype-rounded windows (call before any launch)."""
    c = case
    d64 = lambda name: t.v(name).cpu().double()
    if c.op == "ce":
        x, tg = d64("logits"), t.row("targets").cpu()
        keep = tg != CE_IGNORE
        mx = x.amax(1)
        lse = mx + torch.log(torch.exp(x - mx[:, None]).sum(1))
        idx = tg.clamp_min(0)
        xt = x.gather(1, idx[:, None])[:, 0]
        loss = torch.where(keep, lse - xt, torch.zeros_like(lse))
        u_loss = ULP * (lse.abs() + xt.abs())
        gs = 1.0 / t.row("count").cpu().double().item()
        p = torch.exp(x - lse[:, None])
        onehot = torch.zeros_like(x).scatter_(1, idx[:, None], 1.0)
        grad = (p - onehot) * gs * keep[:, None]
        u_grad = ULP * gs * (p * (1 + L2E * (x.abs() + mx.abs()[:, None])) + onehot)
        return dict(loss=loss, u_loss=u_loss, keep=keep, grad=grad, u_grad=u_grad,
                    sum=c.loss0 + loss.sum(), u_sum=ULP * (abs(c.loss0) + (u_loss / ULP)[keep].sum()))
    if c.op == "count":
        return dict(count=2.0 + float((t.row("targets").cpu() != 0).sum()))
    if c.op == "embfwd":
        n, d = c.B * c.T, c.cols
        tok = t.row("tokens").cpu()
        scale = math.sqrt(d)
        a = d64("table")[tok] * float(torch.tensor(scale, dtype=torch.float32))
        pe = d64("pe")[torch.arange(n) % c.T]
        m = t.mask.double().view(n, d) if c.drop_p > 0 else torch.ones(n, d, dtype=torch.float64)
        return dict(out=((a + pe) * m).view(-1), u=(ULP * (a.abs() + pe.abs()) * m).view(-1), mask=m.view(-1))
    if c.op == "embplan":
        return dict(plan=stable_plan(t.row("tokens").cpu()))
    if c.op == "embbwd":
        n, d = c.B * c.T, c.cols
        tok = t.row("tokens").cpu()
        scale = float(torch.tensor(math.sqrt(d), dtype=torch.float32))
        m = t.mask.double().view(n, d) if c.drop_p > 0 else torch.ones(n, d, dtype=torch.float64)
        gq = d64("dx") * scale * m
        live = tok != PAD
        grad = torch.zeros(BWD_VOCAB, d, dtype=torch.float64).index_add_(0, tok[live], gq[live])
        mag = torch.zeros(BWD_VOCAB, d, dtype=torch.float64).index_add_(0, tok[live], gq[live].abs())
        present = torch.zeros(BWD_VOCAB, dtype=torch.bool)
        present[tok[live]] = True
        ref = dict(grad=grad, u=ULP * mag, present=present, plan=stable_plan(tok))
        if not c.planned:
            d0 = d64("dtable")
            ref.update(grad=d0 + grad, u=ULP * (mag + d0.abs()))
        return ref
    if c.op == "colsum":
        dy = d64("dy")[:c.rows]
        o0 = t.row("out").cpu().double()
        s, mag = dy.sum(0), dy.abs().sum(0)
        return dict(out=s + o0 if c.accumulate else s, u=ULP * (mag + (o0.abs() if c.accumulate else 0)))
    if c.op == "gnorm":
        norm = t.row("grads").cpu().double().norm().item()
        mx = t.x["max_norm"]
        coef = min(1.0, mx / (norm + 1e-6)) if mx > 0 else 1.0
        return dict(norm=norm, coef=coef)
    if c.op == "adamw":
        p2, m1, v1, u = adam_step64(t.row("p").cpu().double(), t.row("g").cpu().double(), t.row("m").cpu().double(),
                                    t.row("v").cpu().double(), float(torch.tensor(c.lr, dtype=torch.float32)), c.step,
                                    c.wd, c.coef if c.norm else 1.0)
        return dict(p=p2, m=m1, v=v1, **u)
    if c.op == "adamchain":
        p, g = t.row("p").cpu().double(), t.row("g").cpu().double()
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        tol = torch.zeros_like(p)
        for s, lr in enumerate(CHAIN_LR, start=1):
            p, m, v, u = adam_step64(p, g * s, m, v, float(torch.tensor(lr, dtype=torch.float32)), s, c.wd, c.coef)
            tol = tol + u["u_p"]
        return dict(p=p, m=m, v=v, u_chain=tol)
    if c.op == "im2col":
        idx = unfold_index(c)
        img = t.row("img").cpu()
        out = torch.where(idx >= 0, img[idx.clamp_min(0)], torch.zeros(()))
        return dict(out=out.to(_TORCH[c.dtype]))
    if c.op == "assemble":
        np_, E = c.geom
        patch = t.v("patch").cpu().float().view(c.B, np_, E)
        base = torch.cat([t.row("cls").cpu().view(1, 1, E).expand(c.B, 1, E), patch], 1)
        return dict(h=(base + t.v("pos").cpu()[None]).view(-1, E).to(_TORCH[c.dtype]))  # one f32 add, one rounding
    if c.op == "cast":
        return dict(dst=to_dtype(t.row("src").cpu(), _TORCH[c.dtype]))
    if c.op == "mask":
        return dict(out=host_mask(c.cols, c.drop_p, SEEDS[c.seed], c.site))
    if c.op == "sdiv":
        return dict(out=torch.tensor([7.25]) / torch.tensor([3.0]))
    if c.op == "stepinc":
        return dict(step=2 ** 33 + 42)
    raise ValueError(c.op)


# ------------------------------------------------------------------------------------------------
# checks
# ------------------------------------------------------------------------------------------------
def _cmp(case, what, got, ref, unit, key, fig, bf16=False, scale=1.0):
    """max (|got - ref| - [2^-8 |ref| for a bf16 output]) / unit <= scale * BOUND[key]; the figure is printed first"""
    got = got.detach().cpu().double()
    err = (got - ref).abs()
    if bf16:
        err = (err - BF16_REL * ref.abs()).clamp_min(0.0)
    unit = torch.as_tensor(unit, dtype=torch.float64).expand_as(err) if not torch.is_tensor(unit) else unit
    ratio = torch.where(err == 0, torch.zeros_like(err), err / unit.clamp_min(1e-45))
    worst = (ratio.max().item() if ratio.numel() else 0.0) if not torch.isnan(ratio).any() else float("nan")
    bound = scale * BOUND[key]
    print(f"MISC {case.id} {what}: worst {worst:.3f} units{' past 2^-8 |ref|' if bf16 else ''} (bound {bound:g})")
    fig[key + ("/bf16" if bf16 else "")] = max(fig.get(key + ("/bf16" if bf16 else ""), 0.0), worst)
    assert worst <= bound, f"{case.id} {what}: {worst:.3f} units (bound {bound:g}); max |err| " \
                           f"{(got - ref).abs().max().item():.3e}, max |ref| {ref.abs().max().item():.3e}"


def _bits(x):
    return x.contiguous().view(gc._INT[x.element_size()])


def _exact(case, what, got, ref):
    got, ref = got.detach().cpu(), ref.cpu()
    assert got.dtype == ref.dtype and got.shape == ref.shape, (case.id, what, got.dtype, ref.dtype, got.shape, ref.shape)
    bad = _bits(got) != _bits(ref)
    if bad.any():
        i = tuple(bad.nonzero()[0])
        hx = lambda x: f"{x[i].item()} (0x{_bits(x)[i].item() & (2 ** (8 * x.element_size()) - 1):x})"
        raise AssertionError(f"{case.id}: {int(bad.sum())} element(s) of {what} differ bitwise; first at {list(i)}: "
                             f"{hx(got)} != {hx(ref)}")


def ce_window_cols(c):
    """the columns of a row the call may write: V, or round8(V) on the wave-per-row kernel (zeros)"""
    return r8(c.cols) if (c.plan == CE_ROWS and c.want_grad) else c.cols


def check(case, t, ref):
    c, fig = case, {}
    b16 = c.dtype == "bf16"
    if c.op == "ce":
        V = c.cols
        if c.row_loss:
            rl = t.row("row_loss")
            _cmp(c, "row_loss", rl, ref["loss"], ref["u_loss"], "ce_loss", fig)
            assert (rl.cpu()[~ref["keep"]] == 0).all(), f"{c.id}: row_loss of an ignored row is not 0"
        _cmp(c, "loss_sum", t.row("loss_sum"), torch.as_tensor([ref["sum"]], dtype=torch.float64),
             torch.as_tensor([ref["u_sum"]], dtype=torch.float64), "ce_sum", fig)
        if c.want_grad:
            gv = t.v("logits")
            _cmp(c, "grad", gv, ref["grad"], ref["u_grad"], "ce_grad", fig, b16)
            ign = gv.cpu()[~ref["keep"]]
            assert (ign == 0).all(), f"{c.id}: {int((ign != 0).sum())} gradient element(s) of ignored rows are not 0"
            if c.plan == CE_ROWS and V % 8:
                L = t.b["logits"]
                tail = gc.window(L.whole, (L.spec[0], c.rows, r8(V), c.ld))[:, V:].cpu()
                assert (_bits(tail) == 0).all(), f"{c.id}: columns V..round8(V) are not +0"
        # want_grad == 0: logits is an input, held bit for bit by the guards below
    elif c.op == "count":
        assert t.row("count").cpu().item() == ref["count"], (c.id, t.row("count").cpu().item(), ref["count"])
    elif c.op == "embfwd":
        out = t.row("out")
        _cmp(c, "out", out, ref["out"], ref["u"], "emb_fwd", fig, b16)
        dropped = ref["mask"] == 0
        assert (out.cpu()[dropped] == 0).all(), f"{c.id}: a dropped element is not 0"
        assert c.drop_p == 0 or (dropped.any() and not dropped.all())
    elif c.op == "embplan":
        check_plan(c, t, ref)
    elif c.op == "embbwd":
        if c.planned:
            check_plan(c, t, ref)
        dt_ = t.v("dtable").cpu()
        pres = ref["present"]
        if pres.any():
            _cmp(c, "dtable", dt_[pres], ref["grad"][pres], ref["u"][pres], "emb_bwd", fig)
        if c.planned:
            sent = torch.full((), SENTINEL, dtype=torch.float32)
            got = dt_.cpu()
            assert (_bits(got[~pres]) == _bits(sent)).all(), f"{c.id}: a row of an absent token or of PAD was written"
            assert not (_bits(got[pres]) == _bits(sent)).any(), f"{c.id}: a present row holds unwritten elements"
        else:
            _exact(c, "rows of absent tokens and PAD", dt_.cpu()[~pres], gc.window(t.init["dtable"], t.b["dtable"].spec).cpu()[~pres])
    elif c.op == "colsum":
        _cmp(c, "out", t.row("out"), ref["out"], ref["u"], "colsum", fig)
    elif c.op == "gnorm":
        no = t.row("norm_out").cpu().double()
        _cmp(c, "norm", no[:1], torch.tensor([ref["norm"]], dtype=torch.float64), ULP * ref["norm"], "norm", fig)
        if ref["coef"] == 1.0:  # unclipped, a zero gradient, max_norm <= 0: exactly 1
            assert no[1].item() == 1.0, f"{c.id}: coef {no[1].item()!r} is not exactly 1"
        else:
            _cmp(c, "coef", no[1:], torch.tensor([ref["coef"]], dtype=torch.float64), ULP * ref["coef"], "coef", fig)
    elif c.op == "adamw":
        _cmp(c, "m", t.row("m"), ref["m"], ref["u_m"], "adam_m", fig)
        _cmp(c, "v", t.row("v"), ref["v"], ref["u_v"], "adam_v", fig)
        _cmp(c, "p", t.row("p"), ref["p"], ref["u_p"], "adam_p", fig)
        if c.shadow:
            _exact(c, "shadow", t.row("shadow"), t.row("p").cpu().to(torch.bfloat16))
    elif c.op == "adamchain":
        # five steps: each adds at most BOUND units of its own step to p; the moments' errors re-enter the next
        # update scaled by beta1 / beta2 < 1 and are of the size the unit's |m| term already counts: twice the sum
        _cmp(c, "p after 5 steps", t.row("p"), ref["p"], ref["u_chain"], "adam_p", fig, scale=2.0)
        _exact(c, "shadow", t.row("shadow"), t.row("p").cpu().to(torch.bfloat16))
        assert t.row("step").cpu().item() == len(CHAIN_LR)
    elif c.op == "im2col":
        _exact(c, "out", t.v("out"), ref["out"])
    elif c.op == "assemble":
        _exact(c, "h", t.v("h"), ref["h"])
    elif c.op == "cast":
        _exact(c, "dst", t.row("dst"), ref["dst"])
    elif c.op == "mask":
        out = t.row("out").cpu()
        _exact(c, "mask", out, ref["out"])
        kept = out != 0
        want = (torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(c.drop_p, dtype=torch.float32))).float()
        assert (_bits(out[kept]) == _bits(want)).all() and abs(kept.float().mean().item() - (1 - c.drop_p)) < 0.03
    elif c.op == "sdiv":
        _exact(c, "out", t.row("out"), ref["out"])
    elif c.op == "stepinc":
        assert t.row("step").cpu().item() == ref["step"]
    return fig


def check_plan(c, t, ref):
    got, want = t.row("plan").cpu(), ref["plan"]
    n = want.numel() // 2
    for k in ([0, 1, n - 1] if n > 1 else [0]):  # the first, second and last slot of the table, explicitly
        assert got[k].item() == want[k].item(), f"{c.id}: plan[{k}] = {got[k].item()}, stable sort {want[k].item()}"
    _exact(c, "plan", got, want)


def _guards(c, t):
    for name, b in t.b.items():
        if name in t.outputs:
            spec = b.spec
            if c.op == "ce" and name == "logits":
                spec = (spec[0], c.rows, ce_window_cols(c), c.ld)
            if c.op == "colsum" and name == "ws" and c.rows == 0:
                spec = (spec[0], 1, 0, 1)  # nothing of it may be written
            try:
                gc.untouched(b.whole, spec, b.before)
            except AssertionError as e:
                raise AssertionError(f"{c.id} {name}: {e}") from None
        else:
            b.check_unchanged(f"{c.id} {name}")


# outputs two identical launches need not agree on bit for bit (float atomics)
def _nondeterministic(c):
    if c.op == "ce" and not c.row_loss:
        return {"loss_sum"}
    if c.op == "embbwd" and not c.planned:
        return {"dtable"}
    return set()


def run_case(case, t, ops, ref=None, twice=False):
    """One case through `ops` (one method per op taking (case, t)): values, guards and exact properties; with `twice`
    the launch is repeated from the same inputs and must agree bit for bit. Returns the measured figures."""
    c = case
    ref = ref if ref is not None else reference(c, t)
    fn = getattr(ops, c.op)

    def prepare():
        t.restore()
        if c.op == "adamw":  # lr lives in device memory: the case changes it before the launch
            t.row("lr").fill_(c.lr)

    prepare()
    for b in t.b.values():
        b.snapshot()
    fn(c, t)
    if twice:
        first = {n: t.b[n].whole.clone() for n in t.outputs - _nondeterministic(c)}
        prepare()
        fn(c, t)
        for n, w in first.items():
            assert torch.equal(_bits(t.b[n].whole), _bits(w)), f"{c.id}: {n} differs between two identical launches"
    try:
        fig = check(c, t, ref)
        _guards(c, t)
    finally:
        t.restore()
    return fig


def planned(case, t, native):
    """the family / key count the native library plans for the case's buffers (host only)"""
    c = case
    dt = native.BF16 if c.dtype == "bf16" else native.F32
    if c.op == "ce":
        return native.cross_entropy_plan(dt, c.rows, c.cols, t.v("logits"), c.ld, t.row("row_loss"))
    if c.op == "im2col":
        C, H, W, P, kpad = c.geom
        return native.im2col_plan(dt, (c.B, C, H, W), P, t.row("img"), t.v("out"), kpad)
    if c.op == "assemble":
        np_, E = c.geom
        return native.vit_assemble_plan(dt, c.B, np_, E, t.v("patch"), t.row("cls"), t.v("pos"), t.v("h"))
    if c.op == "embplan":
        return native.embed_plan_keys_per_thread(c.cols)
    if c.op == "embbwd" and c.planned:
        return native.embed_plan_keys_per_thread(c.B * c.T)
    return None


def expected_plan(c):
    return 1 if (c.op == "embbwd" and c.planned) else c.plan


# ------------------------------------------------------------------------------------------------
# the contract in torch on the guarded buffers, with injectable faults (the harness's self-check)
# ------------------------------------------------------------------------------------------------
# fault -> the case(s) that must catch it
FAULT_CASE = {
    # cross-entropy
    "ce_tail_in_softmax": ["ce-rows-509", "ce-rows-7"], "ce_target_late": ["ce-rows-512", "ce-block-f32-512"],
    "ce_ignored_keep_grad": ["ce-rows-10240", "ce-block-f32-512"],
    "ce_local_count": ["ce-rows-520", "ce-block-10248"], "ce_drop_chunk20": ["ce-rows-10240", "ce-rows-10233"],
    "ce_sum_overwritten": ["ce-rows-512", "ce-block-520-ld523", "ce-block-f32-512-no-row-loss"],
    "ce_block_pad_zeroed": ["ce-block-520-ld523"], "ce_skip_row4": ["ce-rows-512", "ce-rows-10233"],
    "ce_flush_small": ["ce-rows-512", "ce-rows-10240", "ce-block-f32-512", "ce-block-10241"],
    "ce_nograd_writes": ["ce-rows-512-nograd", "ce-block-f32-300-nograd"],
    # embedding
    "emb_pe_flat": ["embfwd-bf16-8-p0-seed-small", "embfwd-f32-130-p0.1-seed-small"],
    "emb_mask_per_row": ["embfwd-bf16-130-p0.1-seed-small", "embbwd-plan-bf16-128-p0.1", "embbwd-atomic-f32-130-p0.1"],
    "emb_pad_written": ["embbwd-plan-bf16-128-p0.1", "embbwd-plan-f32-all-pad", "embbwd-atomic-bf16-8-p0"],
    "emb_drop_row17": ["embbwd-plan-bf16-8-p0", "embbwd-plan-f32-1024-p0.1"],
    "emb_first_512": ["embbwd-plan-bf16-520-p0", "embbwd-plan-f32-1024-p0.1"],
    "emb_plan_adds": ["embbwd-plan-bf16-128-p0.1", "embbwd-plan-f32-8-p0"],
    "emb_plan_unstable": ["embplan-1025", "embplan-16384", "embbwd-plan-f32-8-p0"],
    "emb_plan_kpt_half": ["embplan-4097", "embplan-8192"],  # embed_plan_kernel<4> launched where <8> is due
    "emb_fwd_cap": ["embfwd-past-cap-4x17x32768"],
    # colsum
    "cs_last_chunk_128": ["colsum-bf16-129x300-ld308", "colsum-f32-127x256-ld256"],
    "cs_no_accumulate": ["colsum-f32-128x1-ld1-acc", "colsum-bf16-257x300-ld308-acc"],
    "cs_ld_is_n": ["colsum-bf16-257x300-ld308", "colsum-f32-129x1-ld9-acc"],
    # gradient norm, AdamW
    "gn_skip_tail": ["gnorm-5-max0.5x", "gnorm-3-max2x", "adamw-7-shadow-t2-wd0.1-coef1", "adamw-3-t2-wd0-coef1"],
    "gn_no_clamp": ["gnorm-1027-max2x", "gnorm-zero-grad", "gnorm-max-norm-neg"],
    "ad_bc_step_minus_1": ["adamw-4-norm-t2-wd0.1-coef0.25", "adamw-chain-5-steps"],
    "ad_wd_after": ["adamw-4098-shadow-t1000-wd0.1-coef1", "adamw-chain-5-steps"],
    "ad_v_unclipped": ["adamw-4098-norm-t1-wd0.1-coef0.25"],
    "ad_shadow_old_p": ["adamw-4098-shadow-norm-t2-wd0-coef0.25", "adamw-chain-5-steps"],
    "ad_lr_stale": ["adamw-3-shadow-norm-t2-wd0-coef1"],
    # im2col / assemble
    "im_swap_nph_npw": ["im2col-bf16-3x32x48x16x768", "im2col-f32-3x28x42x14x592"],
    "im_pad_unwritten": ["im2col-bf16-3x32x48x16x776", "im2col-f32-3x28x42x14x592"],
    "as_cls_pos1": ["assemble-bf16-np6-E96", "assemble-f32-np1-E100"],
    # cast, mask
    "cast_truncates": ["cast-bf16-specials"], "cast_cap": ["cast-bf16-past-cap"],
    "mask_ignores_site": ["mask-p0.1-site7-seed-small"], "mask_seed_low_half": ["mask-p0.5-site0-seed-big"],
}
FAULTS = tuple(FAULT_CASE)


def _seq(v, dim):
    """the sum over `dim`, one term after the other in v's dtype"""
    acc = torch.zeros(v.shape[:dim % v.dim()] + v.shape[dim % v.dim() + 1:], dtype=v.dtype)
    for i in range(v.shape[dim]):
        acc = acc + v.select(dim, i)
    return acc


def _sum(v, mode):
    """sum over the last dim: torch's (f64), sequential, or per-lane sequential then a 64-lane butterfly"""
    if mode == "f64":
        return v.sum(-1)
    if mode == "seq":
        return _seq(v, -1)
    n = v.shape[-1]
    k = (n + 63) // 64
    w = torch.zeros(*v.shape[:-1], k * 64, dtype=v.dtype)
    w[..., :n] = v
    lane = _seq(w.view(*v.shape[:-1], k, 64), -2)
    for o in (32, 16, 8, 4, 2, 1):
        lane = lane[..., :o] + lane[..., o:2 * o]
    return lane[..., 0]


class FakeOps:
    """The contract in torch on the guarded buffers, writing what a kernel would. math: "f64", or float32 in one of
    two forms: "seq" (sequential sums; exp / log as the header writes them) and "tree" (64-lane tree sums; the
    wave-per-row cross-entropy's exp2 / log2 with the folded exponent). On a bf16 case the float32 modes are the
    bf16 emulation. `fault` (one of FAULTS) makes it subtly wrong in the way a kernel could be."""

    def __init__(self, math="f64", fault=None):
        self.math, self.fault = math, fault
        self.mt = torch.float64 if math == "f64" else torch.float32

    def _s(self, v):
        return _sum(v, self.math)

    # ---- cross-entropy ----
    def ce(self, c, t):
        f, mt = self.fault, self.mt
        rows, V = c.rows, c.cols
        L = t.b["logits"]
        x = L.view.to(mt)
        if f == "ce_tail_in_softmax" and V % 8:
            x = gc.window(L.whole, (L.spec[0], rows, r8(V), c.ld)).to(mt)
        if f == "ce_drop_chunk20" and V > 19 * 512:
            x = x[:, :19 * 512]
        tg = t.row("targets")
        keep = tg != CE_IGNORE
        idx = tg.clamp_min(0)
        mx = x.amax(1)
        rows_form = c.plan == CE_ROWS and self.math == "tree"
        if rows_form:
            mxl = mx * L2E
            e = torch.exp2(x * L2E - mxl[:, None])
        else:
            e = torch.exp(x - mx[:, None])
        se = self._s(e)
        lse = mx + torch.log(se)
        xt = L.view.to(mt).gather(1, idx[:, None])[:, 0]
        loss = torch.where(keep, lse - xt, torch.zeros_like(lse))
        live = rows - 1 if (f == "ce_skip_row4" and c.plan == CE_ROWS and rows % 4 == 0) else rows
        if c.row_loss:
            t.row("row_loss")[:live].copy_(loss[:live].float())
            tot = self._s(loss[:live].float().to(mt)[None])[0]
        else:
            tot = self._s(loss[None])[0]
        ls = t.row("loss_sum")
        ls.copy_((tot if f == "ce_sum_overwritten" else ls.to(mt)[0] + tot).float().view(1))
        if not c.want_grad:
            if f == "ce_nograd_writes":
                L.view[0, 0] = L.view[0, 0] + 1.0
            return
        cnt = keep.sum().to(mt) if f == "ce_local_count" else t.row("count").to(mt)[0]
        gs = (1.0 / cnt).to(mt)
        if rows_form:
            off = mxl + torch.log2(se) - torch.log2(gs)
            p = torch.exp2(x * L2E - off[:, None])
        else:
            p = e * (1.0 / se)[:, None] * gs
        if f == "ce_flush_small":
            p = torch.where(p < 1e-5 * p.amax(1, keepdim=True), torch.zeros_like(p), p)
        col = (idx + 1).clamp_max(x.shape[1] - 1) if f == "ce_target_late" else idx
        col = col.clamp_max(x.shape[1] - 1)
        onehot = torch.zeros_like(p).scatter_(1, col[:, None], 1.0)
        grad = p - onehot * gs
        if f != "ce_ignored_keep_grad":
            grad = grad * keep[:, None]
        out = gc.window(L.whole, (L.spec[0], rows, ce_window_cols(c), c.ld))
        if c.plan == CE_ROWS:
            out[:live].zero_()
        if f == "ce_block_pad_zeroed" and c.plan == CE_BLOCK:
            gc.window(L.whole, (L.spec[0], rows, c.ld, c.ld))[:rows - 1, V:].zero_()
        out[:live, :grad.shape[1]].copy_(grad[:live, :out.shape[1]].to(out.dtype))

    def count(self, c, t):
        t.row("count").add_(float((t.row("targets") != 0).sum()))

    # ---- embedding ----
    def _mask(self, c, t, n, d):
        if c.drop_p == 0:
            return None
        if self.fault == "emb_mask_per_row":
            return t.mask[:d].to(self.mt).view(1, d).expand(n, d)
        return t.mask.to(self.mt).view(n, d)

    def embfwd(self, c, t):
        f, mt = self.fault, self.mt
        n, d = c.B * c.T, c.cols
        tok = t.row("tokens")
        scale = torch.tensor(math.sqrt(d), dtype=torch.float32).to(mt)
        pos = torch.arange(n) % c.T
        if f == "emb_pe_flat":
            pos = torch.arange(n) % (c.T + 2)
        v = t.v("table").to(mt)[tok] * scale + t.v("pe").to(mt)[pos]
        m = self._mask(c, t, n, d)
        if m is not None:
            v = v * m
        v = v.reshape(-1).to(t.row("out").dtype)
        k = GRID_CAP if f == "emb_fwd_cap" else v.numel()
        t.row("out")[:k].copy_(v[:k])

    def _plan(self, c, t):
        tok = t.row("tokens")
        plan = stable_plan(tok)
        n = tok.numel()
        if self.fault == "emb_plan_unstable":
            perm = torch.sort(tok * n + (n - 1 - torch.arange(n))).indices
            plan[:n] = perm.to(torch.int32)
        if self.fault == "emb_plan_kpt_half" and kpt_of(n) == 8:  # only the first 4096 key slots are sorted
            plan[:4096] = stable_plan(tok[:4096])[:4096]
            plan[4096:n] = torch.arange(4096, n, dtype=torch.int32)
        t.row("plan").copy_(plan)

    def embplan(self, c, t):
        self._plan(c, t)

    def embbwd(self, c, t):
        f, mt = self.fault, self.mt
        n, d = c.B * c.T, c.cols
        tok = t.row("tokens")
        scale = torch.tensor(math.sqrt(d), dtype=torch.float32).to(mt)
        gq = t.v("dx").to(mt) * scale
        m = self._mask(c, t, n, d)
        if m is not None:
            gq = gq * m
        dtab = t.v("dtable")
        if not c.planned:
            for j in range(n):  # position order: one of the orders the atomics may take
                if tok[j] != PAD or f == "emb_pad_written":
                    dtab[tok[j]] = (dtab[tok[j]].to(mt) + gq[j]).float()
            return
        self._plan(c, t)
        plan = t.row("plan")
        for k in range(n):
            ln = int(plan[n + k])
            if ln == 0:
                continue
            pos = plan[k:k + ln].long()
            tk = int(tok[pos[0]])
            if tk == PAD and f != "emb_pad_written":
                continue
            if f == "emb_drop_row17" and ln > 16:
                pos = torch.cat([pos[:16], pos[17:]])
            acc = _seq(gq[pos], 0) if self.math != "f64" else gq[pos].sum(0)
            if f == "emb_first_512":
                acc = acc[:512]
            w = acc.numel()
            dtab[tk, :w] = (dtab[tk, :w].to(mt) + acc if f == "emb_plan_adds" else acc).float()

    # ---- column sums ----
    def colsum(self, c, t):
        f, mt = self.fault, self.mt
        M, N = c.rows, c.cols
        D = t.b["dy"]
        ld = N if f == "cs_ld_is_n" else c.ld
        flat = D.whole[D.spec[0]:]
        nch = (M + CS_ROWS - 1) // CS_ROWS
        ws = t.row("ws")
        total = torch.zeros(N, dtype=mt)
        for ch in range(nch):
            r0 = ch * CS_ROWS
            r1 = r0 + CS_ROWS if f == "cs_last_chunk_128" else min(M, r0 + CS_ROWS)
            idx = torch.arange(r0, r1).view(-1, 1) * ld + torch.arange(N).view(1, -1)
            idx = idx.clamp_max(flat.numel() - 1)  # past the buffer: the tail guard's last element (NaN)
            part = flat[idx].to(mt)
            s = _seq(part, 0) if self.math != "f64" else part.sum(0)
            ws[ch * N:(ch + 1) * N].copy_(s.float())
            total = total + (s.float().to(mt) if self.math != "f64" else s)
        out = t.row("out")
        out.copy_((out.to(mt) + total if (c.accumulate and f != "cs_no_accumulate") else total).float())

    # ---- gradient norm, AdamW ----
    def gnorm(self, c, t):
        f, mt = self.fault, self.mt
        g = t.row("grads").to(mt)
        n = g.numel()
        if f == "gn_skip_tail":
            g = g[:n // 4 * 4]
        sq = g * g
        if self.math == "f64":
            parts = torch.zeros(GN_BLOCKS, dtype=mt)
            parts[0] = sq.sum()
        else:  # 1024 partial sums in float32 (contiguous chunks in "seq", strided lanes in "tree"), then double
            k = (sq.numel() + GN_BLOCKS - 1) // GN_BLOCKS
            w = torch.zeros(k * GN_BLOCKS, dtype=mt)
            w[:sq.numel()] = sq
            parts = _seq(w.view(GN_BLOCKS, k), 1) if self.math == "seq" else _seq(w.view(k, GN_BLOCKS), 0)
        t.row("ws").copy_(parts.float())
        total = parts.float().double().sum().sqrt().to(mt if self.math == "f64" else torch.float32)
        mx = torch.tensor(t.x["max_norm"], dtype=total.dtype)
        coef = mx / (total + torch.tensor(1e-6, dtype=total.dtype))
        if f != "gn_no_clamp":
            if not bool(coef < 1.0):
                coef = torch.ones_like(coef)
            if t.x["max_norm"] <= 0:
                coef = torch.ones_like(coef)
        t.row("norm_out").copy_(torch.stack([total, coef]).float())

    def _adam(self, c, t, lr_stale=None):
        f, mt = self.fault, self.mt
        n = c.cols
        live = n // 4 * 4 if f == "gn_skip_tail" else n
        p, g, m, v = (t.row(k)[:live].to(mt) for k in ("p", "g", "m", "v"))
        coef = t.row("norm_out").to(mt)[1] if "norm_out" in t.b else torch.ones((), dtype=mt)
        lr = t.row("lr").to(mt)[0] if lr_stale is None else torch.tensor(lr_stale, dtype=mt)
        step = int(t.row("step")[0])
        b1, b2 = torch.tensor(B1, dtype=torch.float32).to(mt), torch.tensor(B2, dtype=torch.float32).to(mt)
        eps, wd = torch.tensor(EPS, dtype=torch.float32).to(mt), torch.tensor(c.wd, dtype=torch.float32).to(mt)
        tb = step - 1 if f == "ad_bc_step_minus_1" else step
        bc1 = torch.tensor(1.0 - float(b1) ** tb, dtype=mt)
        bc2 = torch.tensor(1.0 - float(b2) ** tb, dtype=mt)
        gk = g * coef
        p0 = p.clone()
        if f != "ad_wd_after":
            p = p * (1.0 - lr * wd)
        m1 = m + (1.0 - b1) * (gk - m)
        gv = g if f == "ad_v_unclipped" else gk
        v1 = v * b2 + (1.0 - b2) * gv * gv
        denom = v1.sqrt() / bc2.sqrt() + eps
        p = p - (lr / bc1) * (m1 / denom)
        if f == "ad_wd_after":
            p = p * (1.0 - lr * wd)
        t.row("p")[:live].copy_(p.float())
        t.row("m")[:live].copy_(m1.float())
        t.row("v")[:live].copy_(v1.float())
        if "shadow" in t.b:
            t.row("shadow")[:live].copy_((p0 if f == "ad_shadow_old_p" else p).float().to(torch.bfloat16))

    def adamw(self, c, t):
        self._adam(c, t, float(gc.window(t.init["lr"], t.b["lr"].spec)[0, 0]) if self.fault == "ad_lr_stale" else None)

    def adamchain(self, c, t):
        g0 = t.b["g"].view.clone()
        for s, lr in enumerate(CHAIN_LR, start=1):
            t.row("step").add_(1)
            t.row("lr").fill_(lr)
            t.b["g"].view.copy_(g0 * s)
            self._adam(c, t)
        t.b["g"].view.copy_(g0)

    # ---- im2col / assemble ----
    def im2col(self, c, t):
        f = self.fault
        C, H, W, P, kpad = c.geom
        idx = unfold_index(c)
        if f == "im_swap_nph_npw":
            nph, npw = H // P, W // P
            row = torch.arange(c.B * nph * npw).view(-1, 1)
            col = torch.arange(kpad).view(1, -1)
            b, p = row // (nph * npw), row % (nph * npw)
            ch, ky, kx = col // (P * P), (col // P) % P, col % P
            y, x = (p // nph) * P + ky, (p % nph) * P + kx
            idx = torch.where(col < C * P * P, (((b * C + ch) * H + y) * W + x) % (c.B * C * H * W), torch.full_like(row + col, -1))
        img = t.row("img")
        val = torch.where(idx >= 0, img[idx.clamp_min(0)], torch.zeros(())).to(t.v("out").dtype)
        if f == "im_pad_unwritten":
            t.v("out")[:, :C * P * P].copy_(val[:, :C * P * P])
        else:
            t.v("out").copy_(val)

    def assemble(self, c, t):
        np_, E = c.geom
        patch = t.v("patch").float().view(c.B, np_, E)
        base = torch.cat([t.row("cls").view(1, 1, E).expand(c.B, 1, E), patch], 1)
        pos = t.v("pos").clone()
        if self.fault == "as_cls_pos1":
            pos[0] = pos[1]
        t.v("h").copy_((base + pos[None]).view(-1, E).to(t.v("h").dtype))

    # ---- cast, mask, scalars ----
    def cast(self, c, t):
        src = t.row("src")
        if self.fault == "cast_truncates" and c.dtype == "bf16":
            val = (src.view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)
        else:
            val = to_dtype(src, t.row("dst").dtype)
        k = GRID_CAP if self.fault == "cast_cap" else val.numel()
        t.row("dst")[:k].copy_(val[:k])

    def mask(self, c, t):
        seed = SEEDS[c.seed]
        if self.fault == "mask_seed_low_half" and seed is not None:
            seed &= M32
        t.row("out").copy_(host_mask(c.cols, c.drop_p, seed, 0 if self.fault == "mask_ignores_site" else c.site))

    def sdiv(self, c, t):
        t.row("out").copy_(t.row("a") / t.row("b"))

    def stepinc(self, c, t):
        t.row("step").add_(1)


SLOW_F32 = ("embfwd-past-cap", "cast-bf16-past-cap")  # no sums in them: nothing to measure in float32


def measure():
    """the worst FakeOps float32 figures over the table, per quantity and mode (BOUND's source)"""
    import contextlib
    import io
    worst = {}
    for k in BOUND:  # nothing asserted on the values while they are measured
        BOUND[k] = float("inf")
    for c in CASES:
        if c.id.startswith(SLOW_F32):
            continue
        t = make_tensors(c)
        ref = reference(c, t)
        for mode in ("seq", "tree"):
            with contextlib.redirect_stdout(io.StringIO()):
                fig = run_case(c, t, FakeOps(mode), ref)
            for what, v in fig.items():
                k = (what, mode)
                if k not in worst or v > worst[k][0]:
                    worst[k] = (v, c.id)
    for k in sorted(worst):
        print(f"{k[0]:>14} {k[1]:>4}: {worst[k][0]:.3f}  ({worst[k][1]})")


if __name__ == "__main__":
    measure()
