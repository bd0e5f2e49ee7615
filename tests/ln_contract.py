"""The contract of csrc/norm.hip's entry points (include/mit_hip.h) -- mit_layernorm_fwd / _bwd / _param_grads,
mit_layernorm_fwd_x32, mit_residual_out, mit_row_stats64 -- as a case table and a harness, in the manner of
tests/gemm_contract.py (whose guarded `Buf`, `untouched` and bitwise comparison it reuses) and tests/attn_contract.py.

Buffers. Every operand and output of a case is a gemm_contract.Buf: 64-element guards around rows * ld elements of
which the [rows, cols] window is live. Inputs are NaN outside their windows, outputs hold a finite sentinel. The
leading dimensions all differ (bf16 cols + 8 / + 16 / + 24 for x / r / y, f32 + 4 / + 8 / + 12) except where a case
is about an alignment rule; z, mean, rstd, dgamma, dbeta and ws are exact-size (ws exactly
mit_layernorm_bwd_ws_floats floats), so a kernel that writes z at row stride ldy, a row at index `rows`, or one more
block of partials lands in a guard.

Inputs give every term of the formulas weight: per-row mean in +-8, per-row std in [0.05, 4], gamma = 1 + 0.3 randn,
dy with a per-row offset of order 1 (mean(g) and mean(g * xhat) are O(1) of dx), and one constant row of 2.0 (every
partial sum exact: y must equal beta bit for bit). The backward's z / mean / rstd are the float64 reference's,
rounded, so the backward is judged independently of the forward.

`reference` evaluates the header's formulas in float64 from the dtype-rounded windows (dropout mask from
mit_dropout_mask on the GPU, a fixed torch mask on the CPU, index row * cols + col). `run_case` drives an `ops`
object -- the native library in tests/test_ln_contract_gpu.py, `FakeOps` (torch, with injectable faults) in
tests/test_ln_contract_cpu.py -- through forward, backward, the deferred parameter reduction, and checks values,
guards (`untouched` on every output, `check_unchanged` on every input) and the exact properties.

Bounds. f32 quantities are measured in conditioning units:
  y, mean, rstd   u_row = 2^-23 max|z_row| rstd_row max|gamma|   (a one-ulp error of the row mean, seen in y)
  z               2^-23 (|x| + |dropout(r)|)
  dx, dr          2^-23 rstd_row (max|g| + mean|g| + max|xhat| mean|g xhat|),  g = dy gamma
  dgamma, dbeta   2^-23 sum_rows |dy xhat|,  2^-23 sum_rows |dy|  (param_grads alone: 2^-23 sum_blocks |partial|)
  row statistics  mean 2^-23 max|x_chunk|;  M2 2^-23 (M2 + max|x_chunk| sum|x - mean|)
BOUND[q] is 4 x the worst figure of FakeOps in float32 over the whole table, under both sequential summation and
the kernels' 64-lane tree (`python tests/ln_contract.py` prints them); the margin covers a third summation order.
bf16 outputs: |got - ref| <= 2^-8 |ref| + the f32 bound. z of mit_layernorm_fwd_x32 and y of mit_residual_out are
exact (one f32 add of a bf16 value; its bf16 rounding).
"""
import zlib
from dataclasses import dataclass

import torch

import gemm_contract as gc
from gemm_contract import GUARD, NAN, SENTINEL, Buf

_TORCH = {"bf16": torch.bfloat16, "f32": torch.float32}
FAMILIES = ("scalar", "vec4", "wide", "pair")  # mit_ln_plan.fwd / .bwd 0..3
BWD_ROWS = 8          # rows per block of the backward (csrc/norm.hip)
RESOUT_GRID_CAP = 8192 * 256  # 8-column chunks one trip of residual_out_kernel's grid covers
ULP = 2.0 ** -23
BF16_REL = 2.0 ** -8

# 4 x the worst FakeOps float32 figure over the table, in the units above (measured worst: sequential summation /
# 64-lane tree, and the case that gave it)
BOUND = {
    "y": 4 * 6.928,       # 6.928 (mode-dx-is-dy-vec4) / 0.976 (scalar-f32-200)
    "mean": 4 * 3.866,    # 3.866 / 0.589 (past-1280)
    "rstd": 4 * 9.874,    # 9.874 (pair-768-r) / 1.185 (scalar-bf16-1)
    "z": 4 * 0.884,       # 0.884 / 0.884 (vec4-f32-2048): the product r * 1 / (1 - p) and the sum round once each
    "dx": 4 * 1.739,      # 1.739 / 0.936 (vec4-f32-2048); dr is held to the same bound
    "dgamma": 4 * 1.777,  # 1.777 / 1.777 (align-x1)
    "dbeta": 4 * 1.173,   # 1.173 / 1.173 (vec4-f32-768)
    "pgrad": 4 * 2.388,   # 2.388 (pgrad-131x512) / 1.576 (pgrad-16x512)
    "stats_mean": 1.0,    # 0 / 0: every partial sum of 64 bf16 values was exact in f32; one unit allows one rounding
    "stats_m2": 4 * 1.312,  # 1.312 (stats64-5x1024) / 0.190 (stats64-1x1024)
}


# ------------------------------------------------------------------------------------------------
# the case table
# ------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    id: str
    op: str = "ln"         # ln | pgrad | x32 | resout | stats64
    dtype: str = "bf16"    # ln: the operand dtype; x32: y's dtype
    rows: int = 9
    cols: int = 512
    fwd: tuple = None      # (family, NV) the forward must plan onto
    bwd: tuple = None      # (family, NV) of the backward; None: forward only
    r: bool = False
    drop_p: float = 0.0
    z: str = "sep"         # "sep" | None; x32 also "alias" (z is x)
    mean: bool = True
    rstd: bool = True
    eps: float = 1e-5
    pad: tuple = None      # (ldx, ldr, ldy) - cols; None: the dtype's default
    mis: tuple = ()        # ((buffer, elements moved off 16-B alignment), ...)
    dr: bool = True
    alias_dx: bool = False  # dx is dy
    nblk: int = 0          # pgrad: block partials in ws
    site: int = 5

    @property
    def lds(self):
        p = self.pad or ((8, 16, 24) if self.dtype == "bf16" or self.op in ("resout", "stats64") else (4, 8, 12))
        return tuple(self.cols + e for e in p)

    def misalign(self, name):
        return dict(self.mis).get(name, 0)

    @property
    def bwd_drop_p(self):
        return self.drop_p if (self.r and self.dr) else 0.0


def nv_of(cols, per):
    nv = (cols + per - 1) // per
    return nv if nv <= 4 else 8 if nv <= 8 else 16 if nv <= 16 else 32


def _bwd_of(dtype, cols):
    """the backward family of dense, 16-B aligned operands"""
    if dtype == "bf16" and cols % 8 == 0 and cols <= 1024:
        return ("wide", 1 if cols <= 512 else 2)
    if cols % 256 == 0:
        return ("vec4", nv_of(cols, 256))
    return ("scalar", nv_of(cols, 64))


def _build_cases():
    cs = []

    def add(id, dtype, rows, cols, fwd, bwd="auto", **kw):
        if bwd == "auto":
            bwd = _bwd_of(dtype, cols)
        cs.append(Case(id, "ln", dtype, rows, cols, fwd, bwd, **kw))

    rd = dict(r=True, drop_p=0.1)
    # ---- ln_fwd_pair_kernel: bf16 256, and 768 with r; rows straddle the 8-row block of 4 waves x 2 rows ----
    add("pair-256", "bf16", 13, 256, ("pair", 1))
    add("pair-256-r", "bf16", 8, 256, ("pair", 1), r=True)
    add("pair-256-r-rows1", "bf16", 1, 256, ("pair", 1), r=True)
    add("pair-768-r", "bf16", 13, 768, ("pair", 3), r=True)
    add("pair-768-r-drop", "bf16", 8, 768, ("pair", 3), **rd)
    add("pair-768-r-drop-rows9", "bf16", 9, 768, ("pair", 3), **rd)
    add("pair-768-r-rows1", "bf16", 1, 768, ("pair", 3), r=True)
    add("pair-768-r-noz-nostats", "bf16", 5, 768, ("pair", 3), None, r=True, z=None, mean=False, rstd=False)
    # ---- ln_fwd_wide_kernel / ln_bwd_wide_kernel (bf16, cols % 8 == 0, cols <= 1024): NV 1 to 512, NV 2 above ----
    add("wide-8", "bf16", 9, 8, ("wide", 1), r=True)
    add("wide-136", "bf16", 5, 136, ("wide", 1), **rd)
    add("wide-512", "bf16", 13, 512, ("wide", 1), **rd)
    add("wide-520", "bf16", 9, 520, ("wide", 2), r=True)
    add("wide-768", "bf16", 13, 768, ("wide", 2))  # without r: the one-row form
    add("wide-1016", "bf16", 5, 1016, ("wide", 2), **rd)
    add("wide-1024", "bf16", 9, 1024, ("wide", 2), **rd)
    add("wide-512-rows1", "bf16", 1, 512, ("wide", 1), r=True)
    add("wide-1024-rows8", "bf16", 8, 1024, ("wide", 2))
    # ---- bf16 past the wide limit ----
    add("past-1032", "bf16", 5, 1032, ("scalar", 32), r=True)
    add("past-1280", "bf16", 9, 1280, ("vec4", 8), **rd)
    add("past-2040", "bf16", 5, 2040, ("scalar", 32))
    add("past-2048", "bf16", 9, 2048, ("vec4", 8), r=True)
    # ---- ln_fwd_kernel<float, NV, true>: NV 1, 2, 3, 4, 8 ----
    for i, (cols, nv) in enumerate([(256, 1), (512, 2), (768, 3), (1024, 4), (1280, 8), (2048, 8)]):
        add(f"vec4-f32-{cols}", "f32", (9, 13, 5, 8)[i % 4], cols, ("vec4", nv), **(rd if i % 2 else {}))
    # ---- ln_fwd_kernel<T, NV, false>: NV 1, 1, 1, 2, 3, 4, 8, 16, 32 in both dtypes (bf16 widths that are
    # multiples of 8 reach it with x and dy moved by one element) ----
    for i, cols in enumerate([1, 63, 64, 65, 130, 200, 260, 520, 1100]):
        nv = ("scalar", nv_of(cols, 64))
        rows = (9, 13, 5, 8, 1)[i % 5]
        add(f"scalar-f32-{cols}", "f32", rows, cols, nv, nv, **(rd if i % 2 else {}))
        off = dict(mis=(("x", 1), ("dy", 1))) if cols % 8 == 0 else {}
        add(f"scalar-bf16-{cols}", "bf16", rows, cols, nv, nv, **off, **(rd if i % 2 == 0 else {}))
    # ---- each alignment rule of the forward alone, at bf16 512 ----
    a = dict(r=True)
    add("align-x4", "bf16", 9, 512, ("vec4", 2), mis=(("x", 4),), **a)
    add("align-x1", "bf16", 9, 512, ("scalar", 8), mis=(("x", 1),), **a)
    add("align-ldx4", "bf16", 9, 512, ("vec4", 2), pad=(4, 16, 24), **a)
    add("align-ldx-odd", "bf16", 9, 512, ("scalar", 8), pad=(9, 16, 24), **a)
    add("align-ldr4", "bf16", 9, 512, ("vec4", 2), pad=(8, 12, 24), **a)
    add("align-y4", "bf16", 9, 512, ("vec4", 2), mis=(("y", 4),), **a)
    add("align-z4", "bf16", 9, 512, ("vec4", 2), mis=(("z", 4),), **a)
    add("align-gamma1", "bf16", 9, 512, ("scalar", 8), ("scalar", 8), mis=(("gamma", 1),), **a)
    add("align-f32-256-ldx6", "f32", 9, 256, ("scalar", 4), pad=(6, 8, 12), **a)
    # ---- ... and of the backward (dy / z / dx / dr / gamma) ----
    for name in ("dy", "bz", "dx", "dr"):
        add(f"align-bwd-{name}4", "bf16", 13, 512, ("wide", 1), ("vec4", 2), mis=((name, 4),), **rd)
    add("align-bwd-dy1", "bf16", 13, 512, ("wide", 1), ("scalar", 8), mis=(("dy", 1),), **rd)
    add("align-bwd-f32-dx1", "f32", 13, 256, ("vec4", 1), ("scalar", 4), mis=(("dx", 1),), **rd)
    # ---- modes ----
    add("mode-drop-without-r", "bf16", 9, 512, ("wide", 1), drop_p=0.1)
    add("mode-drop-without-r-f32", "f32", 9, 200, ("scalar", 4), drop_p=0.1)
    add("mode-no-z", "bf16", 9, 512, ("wide", 1), None, z=None, **rd)
    add("mode-no-mean", "bf16", 9, 1024, ("wide", 2), None, mean=False, **rd)
    add("mode-no-rstd", "f32", 9, 256, ("vec4", 1), None, rstd=False, **rd)
    add("mode-no-z-scalar", "f32", 5, 130, ("scalar", 3), None, z=None, mean=False, rstd=False, **rd)
    add("mode-eps1e-12-wide", "bf16", 9, 768, ("wide", 2), eps=1e-12)
    add("mode-eps1e-12-pair", "bf16", 9, 768, ("pair", 3), eps=1e-12, **rd)
    add("mode-eps1e-12-f32", "f32", 9, 200, ("scalar", 4), eps=1e-12, r=True)
    add("mode-no-dr", "bf16", 13, 768, ("pair", 3), dr=False, **rd)
    add("mode-no-dr-f32", "f32", 13, 256, ("vec4", 1), dr=False, **rd)
    add("mode-no-dr-scalar", "f32", 13, 130, ("scalar", 3), dr=False, **rd)
    add("mode-dx-is-dy", "bf16", 13, 1024, ("wide", 2), alias_dx=True, **rd)
    add("mode-dx-is-dy-f32", "f32", 13, 130, ("scalar", 3), alias_dx=True, **rd)
    add("mode-dx-is-dy-vec4", "f32", 9, 512, ("vec4", 2), alias_dx=True, dr=False)
    # ---- mit_layernorm_param_grads alone on a synthetic ws: the 4-way unrolled loop (nblk > 48) and its tail ----
    for nblk in (1, 16, 17, 49, 64, 65, 131):
        for cols in (8, 130, 512):
            cs.append(Case(f"pgrad-{nblk}x{cols}", "pgrad", "f32", BWD_ROWS * nblk - 3, cols, nblk=nblk))
    # ---- mit_layernorm_fwd_x32: NV 1 to 512, NV 2 above; y bf16 / f32; r; z none / separate / x itself ----
    x32 = [(8, "bf16", True, "sep"), (264, "f32", True, "alias"), (512, "bf16", False, None), (512, "f32", True, None),
           (520, "bf16", True, "alias"), (520, "f32", False, "sep"), (1024, "bf16", True, None), (1024, "f32", True, "sep"),
           (264, "bf16", False, "alias"), (1024, "bf16", False, "sep")]
    for i, (cols, ydt, r, z) in enumerate(x32):
        tag = f"x32-{cols}-{ydt}{'-r' if r else ''}-z{z or 'none'}"
        cs.append(Case(tag, "x32", ydt, (9, 5, 13, 8, 1)[i % 5], cols, r=r, z=z, pad=(0 if z else 8, 16, 24),
                       eps=1e-12 if i % 2 else 1e-5))
    # ---- mit_residual_out: small strided cases, and one past the grid cap of 8192 blocks ----
    cs.append(Case("resout-5x8-r", "resout", rows=5, cols=8, r=True))
    cs.append(Case("resout-9x264", "resout", rows=9, cols=264))
    cs.append(Case("resout-13x520-r", "resout", rows=13, cols=520, r=True))
    cs.append(Case("resout-past-cap-4100x4104-r", "resout", rows=4100, cols=4104, r=True, pad=(0, 0, 0)))
    # ---- mit_row_stats64: one and two 512-column passes, the second part-empty ----
    for cols in (64, 448, 512, 576, 1024):
        for rows in (1, 5):
            cs.append(Case(f"stats64-{rows}x{cols}", "stats64", rows=rows, cols=cols))
    assert len({c.id for c in cs}) == len(cs)
    assert all(c.rows <= 37 for c in cs if not c.id.startswith(("pgrad", "resout-past-cap")))
    return cs


CASES = _build_cases()
BY_ID = {c.id: c for c in CASES}
LN_CASES = [c for c in CASES if c.op == "ln"]

# rejected calls: (id, entry point, what differs from a valid 5 x 512 call with dense rows, a fragment of the message)
REJECTIONS = [
    ("fwd-cols-2056", "fwd", dict(cols=2056, ld=2056), b"out of range"),
    ("fwd-ldx-short", "fwd", dict(ldx=511), b"bad leading dim"),
    ("bwd-cols-2056", "bwd", dict(cols=2056), b"out of range"),
    ("bwd-dgamma-alone", "bwd", dict(dbeta=False), b"both"),
    ("bwd-dbeta-alone", "bwd", dict(dgamma=False), b"both"),
    ("x32-cols-12", "x32", dict(cols=12, ld=16), b"multiple of 8"),
    ("x32-cols-1032", "x32", dict(cols=1032, ld=1032), b"multiple of 8"),
    ("x32-ldy-516", "x32", dict(ldy=516), b"bad leading dim"),
    ("x32-z-with-strided-x", "x32", dict(ldx=520, z=True), b"needs ldx == cols"),
    ("x32-y-is-x", "x32", dict(y_is_x=True), b"alias"),
    ("stats64-cols-100", "stats64", dict(cols=100, ld=104), b"cols"),
    ("plan-cols-2056", "plan", dict(cols=2056, ld=2056), b"out of range"),
]


# ------------------------------------------------------------------------------------------------
# tensors of a case
# ------------------------------------------------------------------------------------------------
class Tensors:
    """b: name -> Buf; inputs / outputs: names; seed; mask (f32 keep-multipliers, flat, index row * cols + col)."""

    def __init__(self):
        self.b, self.outputs, self.seed, self.mask = {}, set(), None, None

    def v(self, name):
        return self.b[name].view if name in self.b else None

    def row(self, name):  # a [1, n] buffer's [n]
        return self.b[name].view[0] if name in self.b else None


def _rows(g, rows, cols):
    """[rows, cols] float32 with per-row mean in +-8 and per-row std in [0.05, 4] (log-uniform), and the stds"""
    mu = (torch.rand(rows, 1, generator=g) * 2 - 1) * 8
    sd = torch.exp(torch.rand(rows, 1, generator=g) * (torch.log(torch.tensor(4.0 / 0.05)))) * 0.05
    x = mu + sd * torch.randn(rows, cols, generator=g)
    return x, sd


def const_row(c):
    return c.rows - 2 if c.rows >= 3 else None


def make_tensors(case, device="cpu", mask_fn=None):
    """The guarded buffers of the case, seeded by its id. mask_fn(n, p, seed, site) -> f32 [n] keep-multipliers
    (mit_dropout_mask on the GPU); without it a fixed Bernoulli mask."""
    c = case
    g = torch.Generator().manual_seed(zlib.crc32(c.id.encode()))
    t = Tensors()
    rows, cols = c.rows, c.cols
    ldx, ldr, ldy = c.lds
    f32 = torch.float32

    def put(name, rws, cls, ld, dtype, data=None, out=False):
        t.b[name] = Buf(rws, cls, ld, dtype, SENTINEL if out else NAN, c.misalign(name), device, data)
        if out:
            t.outputs.add(name)

    if c.op == "pgrad":
        put("ws", 1, c.nblk * 2 * cols, c.nblk * 2 * cols, f32, torch.randn(1, c.nblk * 2 * cols, generator=g) + 0.3)
        put("dgamma", 1, cols, cols, f32, out=True)
        put("dbeta", 1, cols, cols, f32, out=True)
        return t
    if c.op == "stats64":
        x, _ = _rows(g, rows, cols)
        put("x", rows, cols, ldx, torch.bfloat16, x)
        put("out", 1, rows * (cols // 64) * 2, rows * (cols // 64) * 2, f32, out=True)
        return t
    if c.op == "resout":
        put("x", rows, cols, ldx, f32, torch.randn(rows, cols, generator=g) * 3)
        if c.r:
            put("r", rows, cols, ldr, torch.bfloat16, torch.randn(rows, cols, generator=g))
        put("y", rows, cols, ldy, torch.bfloat16, out=True)
        return t
    dt = f32 if c.op == "x32" else _TORCH[c.dtype]
    x, sd = _rows(g, rows, cols)
    rr = 0.5 * sd * torch.randn(rows, cols, generator=g) + 0.5
    k = const_row(c)
    if k is not None:
        x[k], rr[k] = 2.0, 0.0
    put("x", rows, cols, ldx, dt, x, out=(c.z == "alias"))
    if c.r:
        put("r", rows, cols, ldr, torch.bfloat16 if c.op == "x32" else dt, rr)
    put("gamma", 1, cols, cols, f32, (1 + 0.3 * torch.randn(cols, generator=g)).view(1, -1))
    put("beta", 1, cols, cols, f32, (0.5 * torch.randn(cols, generator=g)).view(1, -1))
    put("y", rows, cols, ldy, _TORCH[c.dtype], out=True)
    if c.z == "sep":
        put("z", rows, cols, cols, dt, out=True)
    if c.op == "x32":
        return t
    if c.mean:
        put("mean", 1, rows, rows, f32, out=True)
    if c.rstd:
        put("rstd", 1, rows, rows, f32, out=True)
    t.seed = torch.tensor([1234 + c.site], dtype=torch.int64, device=device)
    if c.drop_p > 0:
        n = rows * max(c.lds)
        if mask_fn is not None:
            t.mask = mask_fn(n, c.drop_p, t.seed, c.site)
        else:
            t.mask = (torch.rand(n, generator=g) >= c.drop_p).float().to(device) / (1.0 - c.drop_p)
    if c.bwd:
        fw = _forward64(c, t)  # the backward's inputs: the reference's z / mean / rstd, rounded
        dy = (torch.rand(rows, 1, generator=g) * 3 - 1.5) + torch.randn(rows, cols, generator=g)
        put("dy", rows, cols, cols, dt, dy, out=c.alias_dx)
        put("bz", rows, cols, cols, dt, fw["z"])
        put("bmean", 1, rows, rows, f32, fw["mean"].view(1, -1))
        put("brstd", 1, rows, rows, f32, fw["rstd"].view(1, -1))
        if not c.alias_dx:
            put("dx", rows, cols, cols, dt, out=True)
        if c.dr:
            put("dr", rows, cols, cols, dt, out=True)
        put("dgamma", 1, cols, cols, f32, out=True)
        put("dbeta", 1, cols, cols, f32, out=True)
        n = ws_floats(rows, cols)
        put("ws", 1, n, n, f32, out=True)
    return t


def ws_floats(rows, cols):
    """mit_layernorm_bwd_ws_floats"""
    return (rows + BWD_ROWS - 1) // BWD_ROWS * 2 * cols


def snapshot(t):
    for b in t.b.values():
        b.snapshot()


def mask2d(c, t, p, dtype=torch.float64):
    if not (c.r and p > 0):
        return None
    return t.mask[:c.rows * c.cols].view(c.rows, c.cols).cpu().to(dtype)


# ------------------------------------------------------------------------------------------------
# the contract in float64
# ------------------------------------------------------------------------------------------------
def _forward64(c, t):
    x = t.v("x").cpu().double()
    r = t.v("r").cpu().double() if c.r else None
    m = mask2d(c, t, c.drop_p)
    rm = None if r is None else (r if m is None else r * m)
    z = x if rm is None else x + rm
    mean = z.mean(1)
    var = ((z - mean[:, None]) ** 2).mean(1)
    rstd = 1.0 / torch.sqrt(var + c.eps)
    gamma, beta = t.row("gamma").cpu().double(), t.row("beta").cpu().double()
    y = (z - mean[:, None]) * rstd[:, None] * gamma + beta
    u_row = ULP * z.abs().amax(1) * rstd * gamma.abs().max()
    u_z = ULP * (x.abs() + (0 if rm is None else rm.abs()))
    return dict(z=z, mean=mean, rstd=rstd, y=y, u_row=u_row, u_z=u_z, beta=beta)


def _backward64(c, t):
    dy, z = t.v("dy").cpu().double(), t.v("bz").cpu().double()
    mean, rstd = t.row("bmean").cpu().double(), t.row("brstd").cpu().double()
    gamma = t.row("gamma").cpu().double()
    xh = (z - mean[:, None]) * rstd[:, None]
    g = dy * gamma
    s1, s2 = g.mean(1), (g * xh).mean(1)
    dx = rstd[:, None] * (g - s1[:, None] - xh * s2[:, None])
    m = mask2d(c, t, c.bwd_drop_p)
    u_dx = ULP * rstd * (g.abs().amax(1) + g.abs().mean(1) + xh.abs().amax(1) * (g * xh).abs().mean(1))
    return dict(dx=dx, dr=dx if m is None else dx * m, mask=m, dgamma=(dy * xh).sum(0), dbeta=dy.sum(0),
                u_dx=u_dx[:, None].expand_as(dx), u_dgamma=ULP * (dy * xh).abs().sum(0), u_dbeta=ULP * dy.abs().sum(0))


def reference(case, t):
    """float64 CPU evaluation of the header's formulas from the dtype-rounded windows (call before the launch)."""
    c = case
    if c.op == "pgrad":
        ws = t.row("ws").cpu().double().view(c.nblk, 2, c.cols)
        return dict(dgamma=ws[:, 0].sum(0), dbeta=ws[:, 1].sum(0), u_dgamma=ULP * ws[:, 0].abs().sum(0),
                    u_dbeta=ULP * ws[:, 1].abs().sum(0))
    if c.op == "stats64":
        x = t.v("x").cpu().double().view(c.rows, c.cols // 64, 64)
        st = gc.stats64(t.v("x").cpu())
        amax = x.abs().amax(-1)
        return dict(stats=st, u_mean=ULP * amax, u_m2=ULP * (st[..., 1] + amax * (x - st[..., :1]).abs().sum(-1)))
    if c.op == "resout":
        s = t.v("x").cpu().float()
        if c.r:
            s = s + t.v("r").cpu().float()  # one f32 add, then one rounding to bf16
        return dict(y=s.bfloat16())
    if c.op == "x32":
        z32 = t.v("x").cpu().float()
        if c.r:
            z32 = z32 + t.v("r").cpu().float()  # exact operands, one f32 rounding: what the kernel must store
        z = z32.double()
        mean = z.mean(1)
        rstd = 1.0 / torch.sqrt(((z - mean[:, None]) ** 2).mean(1) + c.eps)
        gamma, beta = t.row("gamma").cpu().double(), t.row("beta").cpu().double()
        return dict(z32=z32, y=(z - mean[:, None]) * rstd[:, None] * gamma + beta, beta=beta,
                    u_row=ULP * z.abs().amax(1) * rstd * gamma.abs().max())
    ref = _forward64(c, t)
    if c.bwd:
        ref.update(_backward64(c, t))
    return ref


def _cmp(case, what, got, ref, unit, key, fig, bf16=False):
    """max (|got - ref| - [2^-8 |ref| for a bf16 output]) / unit <= BOUND[key]; the figure is printed first"""
    got = got.detach().cpu().double()
    err = (got - ref).abs()
    if bf16:
        err = (err - BF16_REL * ref.abs()).clamp_min(0.0)
    ratio = err / unit.clamp_min(1e-30)
    worst = ratio.max().item() if not torch.isnan(ratio).any() else float("nan")
    print(f"LN {case.id} {what}: worst {worst:.3f} units{' past 2^-8 |ref|' if bf16 else ''} (bound {BOUND[key]:g})")
    fig[what] = max(fig.get(what, 0.0), worst)
    assert worst <= BOUND[key], f"{case.id} {what}: {worst:.3f} units (bound {BOUND[key]:g}); " \
                                f"max |err| {(got - ref).abs().max().item():.3e}, max |ref| {ref.abs().max().item():.3e}"


def _guards(case, t, written, stage):
    """outputs the stage wrote: untouched outside their windows; every other buffer: bit-identical"""
    for name, b in t.b.items():
        if name in written:
            b.check_untouched(f"{case.id} {name} ({stage})")
        else:
            b.check_unchanged(f"{case.id} {name} ({stage})")


def _bits(x):
    return x.contiguous().view(gc._INT[x.element_size()])


def check_fwd(case, t, ref):
    c, fig = case, {}
    b16 = c.dtype == "bf16"
    col = lambda u: u[:, None].expand(c.rows, c.cols)
    _cmp(c, "y", t.v("y"), ref["y"], col(ref["u_row"]), "y", fig, b16)
    k = const_row(c)
    if k is not None or c.cols == 1:  # a constant row: every partial sum exact, z - mean = 0, y = beta bit for bit
        rows = [k] if k is not None else list(range(c.rows))
        want = ref["beta"].to(t.v("y").dtype)
        for i in rows:
            assert torch.equal(_bits(t.v("y")[i].cpu()), _bits(want)), f"{c.id}: y of the constant row {i} is not beta"
    if c.z:
        _cmp(c, "z", t.v("z"), ref["z"], ref["u_z"], "z", fig, b16)
    if c.mean:
        _cmp(c, "mean", t.row("mean"), ref["mean"], ref["u_row"], "mean", fig)
    if c.rstd:
        _cmp(c, "rstd", t.row("rstd"), ref["rstd"], ref["u_row"], "rstd", fig)
    _guards(c, t, {"y", "z", "mean", "rstd"}, "forward")
    return fig


def check_bwd(case, t, ref, deferred=False):
    c, fig = case, {}
    b16 = c.dtype == "bf16"
    dx = t.v("dy") if c.alias_dx else t.v("dx")
    _cmp(c, "dx", dx, ref["dx"], ref["u_dx"], "dx", fig, b16)
    if c.dr:
        _cmp(c, "dr", t.v("dr"), ref["dr"], ref["u_dx"], "dx", fig, b16)
        # exactly dx times the mask's multiplier where it keeps (p = 0: dx everywhere), exactly 0 where it drops
        m = ref["mask"]
        dxc, drc = dx.cpu(), t.v("dr").cpu()
        if m is None:
            assert torch.equal(_bits(drc), _bits(dxc)), f"{c.id}: dr differs from dx without dropout"
        else:
            dropped = m == 0
            assert (drc[dropped] == 0).all(), f"{c.id}: {int((drc[dropped] != 0).sum())} dropped element(s) of dr nonzero"
            assert c.rows * c.cols < 256 or (dropped.any() and not dropped.all())  # the mask is a mask
            if not b16:  # f32: dx is stored unrounded, so dr = fl(dx * 1 / (1 - p)) can be told bit for bit
                want = dxc * m.float()
                assert torch.equal(_bits(drc[~dropped]), _bits(want[~dropped])), f"{c.id}: dr is not dx * mask where it keeps"
    if not deferred:
        _cmp(c, "dgamma", t.row("dgamma"), ref["dgamma"], ref["u_dgamma"], "dgamma", fig)
        _cmp(c, "dbeta", t.row("dbeta"), ref["dbeta"], ref["u_dbeta"], "dbeta", fig)
    written = {"dy" if c.alias_dx else "dx", "dr", "ws"} | (set() if deferred else {"dgamma", "dbeta"})
    _guards(c, t, written, "backward")
    return fig


# ------------------------------------------------------------------------------------------------
# driving an implementation through a case
# ------------------------------------------------------------------------------------------------
def _out_bits(t, names):
    return {n: t.b[n].whole.clone() for n in names if n in t.b}


def _same_bits(case, t, first, what):
    for n, w in first.items():
        assert torch.equal(_bits(t.b[n].whole), _bits(w)), f"{case.id}: {n} {what}"


def _launch(case, t, names, fn, twice):
    """fn(), and with `twice` again: the second launch's outputs are bit-equal to the first's"""
    fn()
    if twice:
        first = _out_bits(t, names)
        if case.alias_dx and "dy" in names:  # dx overwrote dy: restore the input for the second launch
            t.b["dy"].whole.copy_(t.b["dy"].before)
        if case.z == "alias":
            t.b["x"].whole.copy_(t.b["x"].before)
        fn()
        _same_bits(case, t, first, "differs between two identical launches")


def run_case(case, t, ops, ref=None, twice=False):
    """One case through `ops` (fwd / bwd / pgrad / x32 / resout / stats64 methods taking (case, t, **overrides)):
    values, guards and exact properties. Returns the measured figures."""
    c = case
    ref = ref if ref is not None else reference(c, t)
    for n in t.outputs:  # fresh outputs (aliased inputs are restored from their first snapshot by the caller)
        if n not in ("dy", "x"):
            t.b[n].whole.fill_(SENTINEL)
    snapshot(t)
    fig = {}
    if c.op == "pgrad":
        _launch(c, t, ("dgamma", "dbeta"), lambda: ops.pgrad(c, t), twice)
        _cmp(c, "dgamma", t.row("dgamma"), ref["dgamma"], ref["u_dgamma"], "pgrad", fig)
        _cmp(c, "dbeta", t.row("dbeta"), ref["dbeta"], ref["u_dbeta"], "pgrad", fig)
        _guards(c, t, {"dgamma", "dbeta"}, "param_grads")
    elif c.op == "stats64":
        _launch(c, t, ("out",), lambda: ops.stats64(c, t), twice)
        got = t.row("out").view(c.rows, c.cols // 64, 2)
        _cmp(c, "stats mean", got[..., 0], ref["stats"][..., 0], ref["u_mean"], "stats_mean", fig)
        _cmp(c, "stats M2", got[..., 1], ref["stats"][..., 1], ref["u_m2"], "stats_m2", fig)
        _guards(c, t, {"out"}, "row_stats64")
    elif c.op == "resout":
        _launch(c, t, ("y",), lambda: ops.resout(c, t), twice)
        bad = _bits(t.v("y").cpu()) != _bits(ref["y"])
        assert not bad.any(), f"{c.id}: {int(bad.sum())} element(s) of y differ from bf16(x + r); first at " \
                              f"{bad.nonzero()[0].tolist()}"
        _guards(c, t, {"y"}, "residual_out")
    elif c.op == "x32":
        x0 = t.b["x"].before
        _launch(c, t, ("y", "z", "x"), lambda: ops.x32(c, t), twice)
        b16 = c.dtype == "bf16"
        _cmp(c, "y", t.v("y"), ref["y"], ref["u_row"][:, None].expand(c.rows, c.cols), "y", fig, b16)
        k = const_row(c)
        if k is not None:
            assert torch.equal(_bits(t.v("y")[k].cpu()), _bits(ref["beta"].to(t.v("y").dtype))), f"{c.id}: constant row"
        if c.z:
            zv = t.v("x") if c.z == "alias" else t.v("z")
            assert torch.equal(_bits(zv.cpu()), _bits(ref["z32"])), f"{c.id}: z is not the f32 sum x + r"
        _guards(c, t, {"y", "z"} | ({"x"} if c.z == "alias" else set()), "fwd_x32")
        if c.z == "alias":
            t.b["x"].whole.copy_(x0)
    else:
        _launch(c, t, ("y", "z", "mean", "rstd"), lambda: ops.fwd(c, t), twice)
        fig.update(check_fwd(c, t, ref))
        if c.drop_p > 0 and not c.r:  # r_drop_p without r is ignored: bit-equal to the call with r_drop_p = 0
            first = _out_bits(t, ("y", "z", "mean", "rstd"))
            ops.fwd(c, t, drop_p=0.0)
            _same_bits(c, t, first, "changes with an r_drop_p that must be ignored (r is NULL)")
        if c.bwd:
            dy0 = t.b["dy"].before
            snapshot(t)
            names = ("dy" if c.alias_dx else "dx", "dr", "dgamma", "dbeta", "ws")
            _launch(c, t, names, lambda: ops.bwd(c, t), twice)
            fig.update(check_bwd(c, t, ref))
            fused = _out_bits(t, ("dy" if c.alias_dx else "dx", "dr", "dgamma", "dbeta"))
            # deferred parameter gradients: both NULL, then mit_layernorm_param_grads: bit-equal to the fused form
            for n in ("dx", "dr", "dgamma", "dbeta", "ws"):
                if n in t.b:
                    t.b[n].whole.fill_(SENTINEL)
            t.b["dy"].whole.copy_(dy0)
            snapshot(t)
            ops.bwd(c, t, deferred=True)
            check_bwd(c, t, ref, deferred=True)
            snapshot(t)
            ops.pgrad(c, t)
            _guards(c, t, {"dgamma", "dbeta"}, "param_grads after a deferred backward")
            _same_bits(c, t, fused, "of the deferred form differs from the fused form")
            t.b["dy"].whole.copy_(dy0)
    return fig


def planned(case, t, native):
    """((fwd family, NV), (bwd family, NV) or None): mit_layernorm_plan of the case's buffers"""
    c = case
    ldx, ldr, ldy = c.lds
    dt = native.BF16 if c.dtype == "bf16" else native.F32
    kw = dict(x=t.v("x"), ldx=ldx, r=t.v("r"), ldr=ldr, z=t.v("z"), y=t.v("y"), ldy=ldy, gamma=t.row("gamma"),
              beta=t.row("beta"))
    p = native.layernorm_plan(dt, c.rows, c.cols, **kw)
    out = [(FAMILIES[p.fwd], p.fwd_nv), None]
    assert p.bwd == -1 and p.bwd_nv == 0
    if c.bwd:
        dx = t.v("dy") if c.alias_dx else t.v("dx")
        p = native.layernorm_plan(dt, c.rows, c.cols, z=t.v("bz"), gamma=t.row("gamma"), dy=t.v("dy"), dx=dx, dr=t.v("dr"))
        assert p.fwd == -1 and p.fwd_nv == 0
        out[1] = (FAMILIES[p.bwd], p.bwd_nv)
    return tuple(out)


# ------------------------------------------------------------------------------------------------
# the contract in torch on the guarded buffers, with injectable faults (the harness's self-check)
# ------------------------------------------------------------------------------------------------
# fault -> the case(s) that must catch it
FAULT_CASE = {
    # forward formula
    "no_mean_sub": ["wide-768", "vec4-f32-512"], "var_ld": ["vec4-f32-768"], "var_nm1": ["wide-1024"],
    "no_eps": ["scalar-f32-200", "mode-eps1e-12-wide"],
    # forward memory
    "stats_pad": ["wide-520"], "y_across_ld": ["pair-256"], "z_at_ldy": ["wide-512"],
    # forward dropout
    "mask_ldr": ["pair-768-r-drop"], "drop_sum": ["wide-1024"],
    # forward row tails
    "pair_skip": ["pair-768-r-drop"], "row_rows": ["scalar-bf16-65"],
    # backward
    "no_s1": ["wide-768", "wide-1024", "vec4-f32-512"], "no_s2": ["wide-768", "wide-1024", "scalar-f32-130"],
    "dgamma_tail": ["wide-512"], "dbeta_masked": ["wide-1024"], "dr_unmasked": ["pair-768-r-drop"],
    "reduce_64": ["pgrad-65x130", "pgrad-131x512"], "ws_overrun": ["wide-768"],
    # the other entry points
    "x32_z_bf16": ["x32-1024-f32-r-zsep"], "x32_y_bf16": ["x32-512-f32-r-znone"],
    "resout_cap": ["resout-past-cap-4100x4104-r"],
    "stats_m2_var": ["stats64-5x448"], "stats_pass2": ["stats64-5x576", "stats64-1x1024"],
}
FAULTS = tuple(FAULT_CASE)


def _seq(v, dim):
    """the sum over `dim`, one term after the other in v's dtype (torch.sum is pairwise, and torch.cumsum
    accumulates float32 in double on the CPU)"""
    acc = torch.zeros(v.shape[:dim % v.dim()] + v.shape[dim % v.dim() + 1:], dtype=v.dtype)
    for i in range(v.shape[dim]):
        acc = acc + v.select(dim, i)
    return acc


def _sum(v, mode):
    """sum over the last dim: torch's (f64 / f32), sequential, or per-lane sequential then a 64-lane butterfly"""
    if mode in ("f64", "f32"):
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


def _restrided(buf, rows, cols, ld):
    flat = buf.whole
    return flat.as_strided((rows, cols), (ld, 1), flat.storage_offset() + buf.spec[0])


class FakeOps:
    """The contract in torch on the guarded buffers, writing what a kernel would. math: "f64", or float32 with
    torch's / sequential ("seq") / 64-lane-tree ("tree") summation -- on a bf16 case the float32 modes are the
    bf16 emulation (rounded inputs, f32 math, outputs rounded on the store). `fault` (one of FAULTS) makes it
    subtly wrong in the way a kernel could be."""

    def __init__(self, math="f64", fault=None):
        self.math, self.fault = math, fault
        self.mt = torch.float64 if math == "f64" else torch.float32

    def _s(self, v):
        return _sum(v, self.math)

    def fwd(self, c, t, drop_p=None):
        f, mt = self.fault, self.mt
        p = c.drop_p if drop_p is None else drop_p
        rows, cols = c.rows, c.cols
        ldx, ldr, ldy = c.lds
        x = t.v("x").to(mt)
        z = x
        if c.r:
            m = mask2d(c, t, p, mt)
            if f == "mask_ldr" and m is not None:
                m = t.mask.as_strided((rows, cols), (ldr, 1)).to(mt)
            r = t.v("r").to(mt)
            z = x + (r if m is None else r * m)
            if f == "drop_sum" and m is not None:
                z = (x + r) * m
        zs = _restrided(t.b["x"], rows, ldx, ldx).to(mt) if f == "stats_pad" else z
        n = ldx if f == "var_ld" else cols - 1 if f == "var_nm1" else cols
        mean = self._s(zs) / cols
        d = zs - mean[:, None]
        rstd = 1.0 / torch.sqrt(self._s(d * d) / n + (0.0 if f == "no_eps" else c.eps))
        gamma, beta = t.row("gamma").to(mt), t.row("beta").to(mt)
        y = ((z if f == "no_mean_sub" else z - mean[:, None]) * rstd[:, None] * gamma + beta).to(t.v("y").dtype)
        Y = t.b["y"]
        if f == "pair_skip" and rows % 2 == 0:
            Y.view[:rows - 1].copy_(y[:rows - 1])
        else:
            Y.view.copy_(y)
        if f == "y_across_ld":
            Y.whole[Y.spec[0] + cols] = 1.0
        if f == "row_rows":
            Y.whole[Y.spec[0] + rows * ldy] = 1.0
        if c.z:
            Z = t.b["z"]
            if f == "z_at_ldy":
                _restrided(Z, min(rows, 3), cols, ldy).copy_(z[:3].to(Z.view.dtype))
            else:
                Z.view.copy_(z.to(Z.view.dtype))
        if c.mean:
            t.row("mean").copy_(mean.float())
        if c.rstd:
            t.row("rstd").copy_(rstd.float())

    def bwd(self, c, t, deferred=False):
        f, mt = self.fault, self.mt
        rows, cols = c.rows, c.cols
        dy, z = t.v("dy").to(mt).clone(), t.v("bz").to(mt)  # a copy: dx may be written over dy
        mean, rstd, gamma = t.row("bmean").to(mt), t.row("brstd").to(mt), t.row("gamma").to(mt)
        xh = (z - mean[:, None]) * rstd[:, None]
        g = dy * gamma
        s1 = torch.zeros(rows, dtype=mt) if f == "no_s1" else self._s(g) / cols
        s2 = torch.zeros(rows, dtype=mt) if f == "no_s2" else self._s(g * xh) / cols
        dx = rstd[:, None] * (g - s1[:, None] - xh * s2[:, None])
        m = mask2d(c, t, c.bwd_drop_p, mt)
        dt = t.v("dy").dtype
        (t.v("dy") if c.alias_dx else t.v("dx")).copy_(dx.to(dt))
        if c.dr:
            dr = dx if (m is None or f == "dr_unmasked") else dx * m
            if m is not None and dt == torch.float32 and f != "dr_unmasked":  # as a kernel: from the f32 dx
                dr = dx.float() * m.float()
            t.v("dr").copy_(dr.to(dt))
        nblk = (rows + BWD_ROWS - 1) // BWD_ROWS
        W = t.b["ws"]
        ws = W.view[0].view(nblk, 2, cols)
        pg, pb = dy * xh, (dy * m if (f == "dbeta_masked" and m is not None) else dy)
        live = rows // BWD_ROWS * BWD_ROWS if (f == "dgamma_tail" and rows % BWD_ROWS) else rows
        for b in range(nblk):
            lo, hi = b * BWD_ROWS, min((b + 1) * BWD_ROWS, rows)
            ws[b, 0] = _seq(pg[lo:max(lo, min(hi, live))], 0).float()
            ws[b, 1] = _seq(pb[lo:hi], 0).float()
        if f == "ws_overrun":
            W.whole[W.spec[0] + nblk * 2 * cols:][:min(GUARD, 2 * cols)] = 0.0
        if not deferred:
            self.pgrad(c, t)

    def pgrad(self, c, t):
        nblk = c.nblk or (c.rows + BWD_ROWS - 1) // BWD_ROWS
        ws = t.row("ws").to(self.mt).view(nblk, 2 * c.cols)
        if self.fault == "reduce_64":
            ws = ws[:64]
        if self.math == "tree":  # 16 strided groups, each sequential, then the groups in order
            k = (ws.shape[0] + 15) // 16
            w = torch.zeros(k * 16, 2 * c.cols, dtype=ws.dtype)
            w[:ws.shape[0]] = ws
            s = _seq(_seq(w.view(k, 16, -1), 0), 0)
        else:
            s = _sum(ws.t(), self.math)
        t.row("dgamma").copy_(s[:c.cols].float())
        t.row("dbeta").copy_(s[c.cols:].float())

    def x32(self, c, t):
        f, mt = self.fault, self.mt
        z32 = t.v("x").float()
        if c.r:
            z32 = z32 + t.v("r").float()
        z = z32.to(mt)
        mean = self._s(z) / c.cols
        d = z - mean[:, None]
        rstd = 1.0 / torch.sqrt(self._s(d * d) / c.cols + c.eps)
        y = d * rstd[:, None] * t.row("gamma").to(mt) + t.row("beta").to(mt)
        if f == "x32_y_bf16":
            y = y.bfloat16()
        t.v("y").copy_(y.to(t.v("y").dtype))
        if c.z:
            (t.v("x") if c.z == "alias" else t.v("z")).copy_(z32.bfloat16().float() if f == "x32_z_bf16" else z32)

    def resout(self, c, t):
        s = t.v("x").float()
        if c.r:
            s = s + t.v("r").float()
        y = s.bfloat16()
        if self.fault == "resout_cap":  # one trip of the grid-stride loop
            per = c.cols // 8
            n = min(RESOUT_GRID_CAP, c.rows * per)
            full, rest = n // per, (n % per) * 8
            t.v("y")[:full].copy_(y[:full])
            if rest:
                t.v("y")[full, :rest].copy_(y[full, :rest])
        else:
            t.v("y").copy_(y)

    def stats64(self, c, t):
        x = t.v("x").to(self.mt).view(c.rows, c.cols // 64, 64)
        mean = self._s(x) / 64
        d = x - mean[..., None]
        m2 = self._s(d * d)
        if self.fault == "stats_m2_var":
            m2 = m2 / 64
        st = torch.stack([mean, m2], -1).float()
        out = t.row("out").view(c.rows, c.cols // 64, 2)
        if self.fault == "stats_pass2":
            out[:, :8].copy_(st[:, :8])
        else:
            out.copy_(st)


def measure():
    """the worst FakeOps float32 figures over the table, per quantity and summation order (BOUND's source)"""
    import contextlib
    import io
    worst = {}
    for k in BOUND:  # nothing asserted on the values while they are measured
        BOUND[k] = float("inf")
    for c in CASES:
        if c.id.startswith("resout-past"):
            continue
        t = make_tensors(c)
        ref = reference(c, t)
        for mode in ("seq", "tree"):
            with contextlib.redirect_stdout(io.StringIO()):
                try:
                    fig = run_case(c, t, FakeOps(mode), ref)
                except AssertionError as e:
                    print(e)
                    raise
            for what, v in fig.items():
                key = {"dr": "dx", "stats mean": "stats_mean", "stats M2": "stats_m2"}.get(what, what)
                if c.op == "pgrad":
                    key = "pgrad"
                k = (key, mode, "bf16" if (c.dtype == "bf16" and key in ("y", "z", "dx")) else "f32")
                if v > worst.get(k, (0.0, ""))[0] or k not in worst:
                    worst[k] = (v, c.id)
    for k in sorted(worst):
        print(f"{k[0]:>11} {k[1]:>4} {k[2]:>4}: {worst[k][0]:.3f}  ({worst[k][1]})")


if __name__ == "__main__":
    measure()
