"""The memory contract of mit_gemm / mit_gemm_grouped (include/mit_hip.h), as a case table and a harness.

Every operand and output of a case lives in a guarded, strided buffer (`strided`): a 64-element head guard,
rows * ld elements of which the [rows, cols] window is live, a 64-element tail guard. Inputs are NaN outside
the window (a kernel that loads a pad element and relies on a zero to cancel it fails: NaN * 0 = NaN), outputs
hold a finite sentinel. `reference` evaluates the header's formula in float64 on the CPU from the windows,
`check` compares and runs `untouched` on every buffer, `fake_gemm` is a torch implementation of the same
contract with injectable faults (tests/test_gemm_contract_cpu.py shows each fault is caught without a GPU).

CASES holds, per kernel family of csrc/gemm.hip, the smallest shapes at which its addressing can go wrong
(tiles: BM = BN = 128, BK = 64, B2 = 256, the f32 and register-streaming kernels 64 x 64), with every
leading dimension padded and different: bf16 lda/ldb = extent + 8 / + 16, ldc / ldr / ld_aux = N + 8 / + 16 /
+ 24; f32 +3 / +5 / +2 / +7 / +11.

Bounds (elementwise, against max|ref|, as _close in test_kernels_gpu.py):
  bf16 outputs 1e-2 (bf16 rounding is 2^-9 = 2e-3 of the value; also the split-K cases with a bf16 output),
  f32 outputs 1e-5, GELU with an f32 output 2e-5 (the one-exp GELU), split-K / grouped f32 C and rowsum 1e-3,
  row statistics 1e-4 of their largest entry against the statistics of the bf16 rows the kernel wrote.
"""
import zlib
from dataclasses import dataclass, replace

import torch
import torch.nn.functional as F

GUARD = 64
SENTINEL = -12288.0  # exact in bf16
NAN = float("nan")
LN_EPS = 1e-5
ARGMAX_SLOTS = 16
K_CONTIG, MN_CONTIG = 0, 1
ACT_NONE, ACT_RELU, ACT_GELU, ACT_QUICK_GELU = 0, 1, 2, 3
_TORCH = {"bf16": torch.bfloat16, "f32": torch.float32}
_INT = {2: torch.int16, 4: torch.int32, 8: torch.int64}


# ------------------------------------------------------------------------------------------------
# guarded strided buffers
# ------------------------------------------------------------------------------------------------
def strided(rows, cols, ld, dtype, fill, misalign=0, device="cpu"):
    """(whole, view): whole = flat [GUARD + misalign | rows * ld | GUARD] filled with `fill`; view = the
    [rows, cols] window with row stride ld, its first element 16-byte aligned and then moved by `misalign`
    elements."""
    assert ld >= cols and rows >= 1 and 0 <= misalign < 16
    esz = torch.empty(0, dtype=dtype).element_size()
    n = GUARD + misalign + rows * ld + GUARD
    base = torch.full((n + 16,), fill, dtype=dtype, device=device)
    shift = ((-(base.data_ptr() + GUARD * esz)) % 16) // esz
    whole = base[shift:shift + n]
    off = GUARD + misalign
    view = whole[off:off + rows * ld].view(rows, ld)[:, :cols]
    assert (view.data_ptr() - misalign * esz) % 16 == 0
    return whole, view


def window(flat, spec):
    off, rows, cols, ld = spec
    return flat[off:off + rows * ld].view(rows, ld)[:, :cols]


def untouched(whole, view_spec, before):
    """Every element of `whole` outside the window view_spec = (offset, rows, cols, ld) is bit-identical to
    `before`: the head guard, the pad columns of every row, the tail guard."""
    it = _INT[whole.element_size()]
    outside = torch.ones(whole.numel(), dtype=torch.bool, device=whole.device)
    window(outside, view_spec).fill_(False)
    bad = (whole.view(it) != before.view(it)) & outside
    if bad.any():
        off, rows, cols, ld = view_spec
        i = int(bad.nonzero()[0])
        where = "head guard" if i < off else "tail guard" if i >= off + rows * ld else \
            f"row {(i - off) // ld}, pad column {(i - off) % ld}"
        raise AssertionError(f"{int(bad.sum())} element(s) outside the window written; first at {i} ({where}): "
                             f"{whole[i].item()} was {before[i].item()}")


class Buf:
    """One guarded buffer of a case: whole / view / spec, and `before`, the snapshot taken just before the launch
    (the reference reads its inputs from the snapshots, so aliased and accumulated outputs are covered)."""

    def __init__(self, rows, cols, ld, dtype, fill, misalign=0, device="cpu", data=None):
        self.whole, self.view = strided(rows, cols, ld, dtype, fill, misalign, device)
        self.spec = (GUARD + misalign, rows, cols, ld)
        self.args = (rows, cols, ld, dtype, fill, misalign, device)
        self.before = None
        if data is not None:
            self.view.copy_(data.to(device))

    def snapshot(self):
        self.before = self.whole.clone()

    def data64(self):
        return window(self.before, self.spec).cpu().double()

    def twin(self):
        """A fresh buffer of the same geometry holding the pre-launch contents."""
        b = Buf(*self.args)
        b.whole.copy_(self.before)
        b.before = self.before
        return b

    def check_untouched(self, name):
        try:
            untouched(self.whole, self.spec, self.before)
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}") from None

    def check_unchanged(self, name):
        it = _INT[self.whole.element_size()]
        assert torch.equal(self.whole.view(it), self.before.view(it)), f"{name}: an input buffer was written"


# ------------------------------------------------------------------------------------------------
# the case table
# ------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    id: str
    family: str   # f32 | rs | 128 | splitk | 256 | 256w | argmax | grouped
    variant: int  # mit_gemm_set_variant
    plan: tuple   # the expected (mit_gemm_plan tile code, split-K factor)
    dtype: str    # operand dtype: bf16 | f32
    al: int
    bl: int
    M: int
    N: int
    K: int
    lda: int
    ldb: int
    ldc: int
    ldr: int
    ld_aux: int
    mis_a: int = 0
    mis_b: int = 0
    mis_c: int = 0
    tiles: int = 0
    bias: bool = False
    act: int = ACT_NONE
    residual: bool = False
    res_is_c: bool = False  # the residual aliases the output (dx += ...)
    aux: bool = False
    aux_scale: float = 1.0
    alpha: float = 1.0
    drop_p: float = 0.0
    site: int = 5
    accumulate: bool = False
    rowsum: bool = False
    out_f32: bool = False
    workspace: bool = False
    ln: bool = False
    stats: bool = False
    argmax: bool = False

    @property
    def tol(self):
        if not self.out_f32 and self.dtype == "bf16":
            return 1e-2
        if self.family in ("splitk", "grouped"):
            return 1e-3
        return 2e-5 if self.act == ACT_GELU else 1e-5

    @property
    def rowsum_tol(self):
        return 1e-5 if self.dtype == "f32" else 1e-3

    @property
    def out_dtype(self):
        return torch.float32 if self.out_f32 or self.dtype == "f32" else torch.bfloat16


def _case(id, family, variant, plan, dtype, al, bl, M, N, K, **kw):
    ea, eb = (K if al == K_CONTIG else M), (K if bl == K_CONTIG else N)
    if dtype == "f32":
        ld = dict(lda=ea + 3, ldb=eb + 5, ldc=N + 2, ldr=N + 7, ld_aux=N + 11, mis_a=1, mis_b=3, out_f32=True)
    else:
        ld = dict(lda=ea + 8, ldb=eb + 16, ldc=N + 8, ldr=N + 16, ld_aux=N + 24)
    ld.update(kw)
    if ld.get("res_is_c"):
        ld["ldr"] = ld["ldc"]
    return Case(id, family, variant, plan, dtype, al, bl, M, N, K, **ld)


_LAYOUTS = [("nt", 0, 0), ("nn", 0, 1), ("tt", 1, 0), ("tn", 1, 1)]


def _build_cases():
    cs = []
    # f32 parity kernel (plan code 64): 64 x 64 tiles, K-tiles of 16: two blocks each way, a ragged K-tile
    f32_epis = [("plain", {}), ("bias_relu_res", dict(bias=True, act=ACT_RELU, residual=True)),
                ("aux", dict(aux=True, aux_scale=1.25)), ("bias_relu_drop", dict(bias=True, act=ACT_RELU, drop_p=0.25)),
                ("acc", dict(accumulate=True, alpha=0.5)), ("rowsum", dict(rowsum=True))]
    for ln, al, bl in _LAYOUTS:
        for en, e in f32_epis:
            cs.append(_case(f"f32-{ln}-{en}", "f32", 0, (64, 1), "f32", al, bl, 70, 67, 19, **e))
    # register-streaming kernel (65, variant 3): K = 136 is three K slices (one wave idle), K = 584 ten (the
    # second-round loads of waves 0 / 1); each epilogue on the vector and on the scalar path
    rs_epis = [("relu_res", dict(bias=True, act=ACT_RELU, residual=True)), ("gelu_res", dict(bias=True, act=ACT_GELU, residual=True)),
               ("qgelu_res", dict(bias=True, act=ACT_QUICK_GELU, residual=True)),
               ("relu_drop", dict(bias=True, act=ACT_RELU, drop_p=0.1)), ("aux", dict(aux=True, aux_scale=1.5)),
               ("res_aux", dict(residual=True, aux=True, aux_scale=2.0)), ("f32", dict(out_f32=True)),
               ("f32_acc", dict(out_f32=True, accumulate=True, alpha=0.5))]
    for K in (136, 584):
        for en, e in rs_epis:
            cs.append(_case(f"rs-k{K}-vec-{en}", "rs", 3, (65, 1), "bf16", 0, 0, 70, 72, K, **e))
            cs.append(_case(f"rs-k{K}-n67-{en}", "rs", 3, (65, 1), "bf16", 0, 0, 70, 67, K, **e))
        e = dict(bias=True, act=ACT_RELU, residual=True)
        cs.append(_case(f"rs-k{K}-ldc75-relu_res", "rs", 3, (65, 1), "bf16", 0, 0, 70, 72, K, ldc=75, **e))
        cs.append(_case(f"rs-k{K}-cmis1-relu_res", "rs", 3, (65, 1), "bf16", 0, 0, 70, 72, K, mis_c=1, **e))
    # 128 x 128 kernel (variant 1): two tiles each way with 8 live rows / columns in the second; K = 72: the
    # second K-tile has 8 live columns
    nt_epis = [("plain", {}), ("relu", dict(bias=True, act=ACT_RELU)), ("relu_drop", dict(bias=True, act=ACT_RELU, drop_p=0.1)),
               ("gelu", dict(bias=True, act=ACT_GELU)), ("qgelu", dict(bias=True, act=ACT_QUICK_GELU)),
               ("gelu_drop", dict(bias=True, act=ACT_GELU, drop_p=0.1)),
               ("res_aux", dict(residual=True, aux=True, aux_scale=2.0)),
               ("f32_acc", dict(out_f32=True, accumulate=True, alpha=0.5))]
    for en, e in nt_epis:
        cs.append(_case(f"128-nt-{en}", "128", 1, (128, 1), "bf16", 0, 0, 136, 136, 72, **e))
    for ln, al, bl in _LAYOUTS[1:]:
        cs.append(_case(f"128-{ln}-plain", "128", 1, (128, 1), "bf16", al, bl, 136, 136, 72))
        cs.append(_case(f"128-{ln}-bias_relu", "128", 1, (128, 1), "bf16", al, bl, 136, 136, 72, bias=True, act=ACT_RELU))
    for en, e in [("plain", {}), ("relu_drop", dict(bias=True, act=ACT_RELU, drop_p=0.1)),
                  ("res_aux", dict(residual=True, aux=True, aux_scale=2.0))]:
        cs.append(_case(f"128-nt-n131-{en}", "128", 1, (128, 1), "bf16", 0, 0, 136, 131, 72, **e))
    cs.append(_case("128-nt-ldc139-bias_relu", "128", 1, (128, 1), "bf16", 0, 0, 136, 136, 72, ldc=139, bias=True, act=ACT_RELU))
    cs.append(_case("128-nt-ldc139-f32_acc", "128", 1, (128, 1), "bf16", 0, 0, 136, 136, 72, ldc=139, out_f32=True,
                    accumulate=True, alpha=0.5))
    cs.append(_case("128-nt-f32-gelu", "128", 1, (128, 1), "bf16", 0, 0, 136, 136, 72, out_f32=True, bias=True, act=ACT_GELU))
    # 128 kernel with split-K (K = 1032: two slices of 576 and 456) and its reduce launch
    sk = dict(workspace=True)
    cs.append(_case("splitk-nn-bf16", "splitk", 1, (128, 2), "bf16", 0, 1, 136, 136, 1032, **sk))
    cs.append(_case("splitk-tn-f32-rowsum-acc", "splitk", 1, (128, 2), "bf16", 1, 1, 136, 136, 1032, out_f32=True, rowsum=True,
                    alpha=0.5, accumulate=True, **sk))
    cs.append(_case("splitk-nn-bf16-ldc140", "splitk", 1, (128, 2), "bf16", 0, 1, 136, 136, 1032, ldc=140, **sk))
    cs.append(_case("splitk-nn-f32-ldc140", "splitk", 1, (128, 2), "bf16", 0, 1, 136, 136, 1032, ldc=140, out_f32=True, **sk))
    cs.append(_case("splitk-nn-bf16-ldc138-no-split", "splitk", 1, (128, 1), "bf16", 0, 1, 136, 136, 1032, ldc=138, **sk))
    # 256 x 256 kernel (variant 2), one case per epilogue stage
    for ln, al, bl in _LAYOUTS:
        cs.append(_case(f"256-reg-{ln}-f32", "256", 2, (256, 1), "bf16", al, bl, 264, 264, 72, out_f32=True))
    cs.append(_case("256-reg-nt-f32-gelu", "256", 2, (256, 1), "bf16", 0, 0, 264, 264, 72, out_f32=True, bias=True, act=ACT_GELU))
    cs.append(_case("256-reg-nt-n259-plain", "256", 2, (256, 1), "bf16", 0, 0, 264, 259, 72))
    cs.append(_case("256-reg-nt-n259-bias_gelu", "256", 2, (256, 1), "bf16", 0, 0, 264, 259, 72, bias=True, act=ACT_GELU))
    cs.append(_case("256-reg-nt-cmis1", "256", 2, (256, 1), "bf16", 0, 0, 264, 264, 72, mis_c=1))
    cs.append(_case("256-staged-bias_gelu", "256", 2, (256, 1), "bf16", 0, 0, 264, 264, 72, bias=True, act=ACT_GELU))
    cs.append(_case("256-ops-bias_res", "256", 2, (256, 1), "bf16", 0, 0, 264, 264, 72, bias=True, residual=True))
    cs.append(_case("256-ops-aux", "256", 2, (256, 1), "bf16", 0, 0, 264, 264, 72, aux=True, aux_scale=1.25))
    cs.append(_case("256-lnfold-bias", "256", 2, (256, 1), "bf16", 0, 0, 264, 264, 128, bias=True, ln=True))
    cs.append(_case("256-lnfold-bias_gelu", "256", 2, (256, 1), "bf16", 0, 0, 264, 264, 128, bias=True, act=ACT_GELU, ln=True))
    cs.append(_case("256-rowstats", "256", 2, (256, 1), "bf16", 0, 0, 264, 320, 72, bias=True, residual=True, res_is_c=True,
                    stats=True))
    # one-wave-per-SIMD 256 kernel (variant 4, tiles = 256): whole K-tiles
    w = dict(tiles=256)
    cs.append(_case("256w-staged-bias_gelu", "256w", 4, (256, 1), "bf16", 0, 0, 264, 264, 128, bias=True, act=ACT_GELU, **w))
    cs.append(_case("256w-lnfold-bias", "256w", 4, (256, 1), "bf16", 0, 0, 264, 264, 128, bias=True, ln=True, **w))
    cs.append(_case("256w-rowstats", "256w", 4, (256, 1), "bf16", 0, 0, 264, 320, 128, bias=True, residual=True, res_is_c=True,
                    stats=True, **w))
    # argmax keys folded into the 128 kernel's gathered epilogue (no C): exact small-integer operands
    cs.append(_case("argmax-n131", "argmax", 0, (128, 1), "bf16", 0, 0, 136, 131, 72, bias=True, argmax=True))
    assert len({c.id for c in cs}) == len(cs)
    assert all(c.M <= 320 and c.N <= 320 and c.K <= 1032 for c in cs)
    return cs


CASES = _build_cases()


def _grouped(alpha, accumulate):
    g = dict(out_f32=True, alpha=alpha, accumulate=accumulate)
    tag = "acc" if accumulate else "plain"
    return [_case(f"grouped-{tag}-136x72x1032", "grouped", 0, (128, 2), "bf16", 1, 1, 136, 72, 1032, ldc=76, rowsum=True, **g),
            _case(f"grouped-{tag}-72x136x264", "grouped", 0, (128, 1), "bf16", 1, 1, 72, 136, 264, rowsum=True, **g),
            _case(f"grouped-{tag}-8x8x520", "grouped", 0, (128, 1), "bf16", 1, 1, 8, 8, 520, rowsum=True, **g)]


# mit_gemm_grouped: three problems in one launch (the first splits K in two, the second and third do not);
# a second launch with alpha / accumulate on pre-filled outputs
GROUPED = {"plain": _grouped(1.0, False), "acc": _grouped(0.5, True)}


# ------------------------------------------------------------------------------------------------
# tensors of a case
# ------------------------------------------------------------------------------------------------
def make_tensors(case, device="cpu", mask_fn=None):
    """name -> Buf for every operand and output of the case (seeded by the case id), plus "seed" (int64 [1])
    and "mask" (f32 [M * ldc], the dropout keep-multipliers: mask_fn(n, p, seed, site) -- mit_dropout_mask on
    the GPU -- or a synthetic Bernoulli mask)."""
    c = case
    g = torch.Generator().manual_seed(zlib.crc32(c.id.encode()))
    dt, odt = _TORCH[c.dtype], c.out_dtype
    ar, ac = (c.M, c.K) if c.al == K_CONTIG else (c.K, c.M)
    br, bc = (c.N, c.K) if c.bl == K_CONTIG else (c.K, c.N)
    if c.argmax:
        a = torch.randint(-2, 3, (ar, ac), generator=g).float()
        b = torch.randint(-2, 3, (br, bc), generator=g).float()
    else:
        a = torch.randn(ar, ac, generator=g)
        if c.ln:
            a = 2 * a + 0.5
        b = torch.randn(br, bc, generator=g) / c.K ** 0.5
    t = {"A": Buf(ar, ac, c.lda, dt, NAN, c.mis_a, device, a), "B": Buf(br, bc, c.ldb, dt, NAN, c.mis_b, device, b)}
    if not c.argmax:
        prior = torch.randn(c.M, c.N, generator=g) if (c.accumulate or c.res_is_c) else None
        t["C"] = Buf(c.M, c.N, c.ldc, odt, SENTINEL, c.mis_c, device, prior)
    if c.bias:
        n8 = (c.N + 7) // 8 * 8 if c.argmax else c.N  # argmax: read in 8-float vectors up to round8(N)
        bias = torch.randint(-4, 5, (c.N,), generator=g).float() if c.argmax else torch.randn(c.N, generator=g)
        t["bias"] = Buf(1, n8, n8, torch.float32, NAN, 0, device)
        t["bias"].view[0, :c.N] = bias.to(device)
    if c.residual and not c.res_is_c:
        t["residual"] = Buf(c.M, c.N, c.ldr, dt, NAN, 0, device, torch.randn(c.M, c.N, generator=g))
    if c.aux:
        t["aux"] = Buf(c.M, c.N, c.ld_aux, dt, NAN, 0, device, torch.randn(c.M, c.N, generator=g))
    if c.rowsum:
        t["rowsum"] = Buf(1, c.M, c.M, torch.float32, SENTINEL, 0, device)
    if c.stats:
        n = c.M * (c.N // 64) * 2
        t["stats_out"] = Buf(1, n, n, torch.float32, SENTINEL, 0, device)
    if c.argmax:
        t["keys"] = Buf(1, ARGMAX_SLOTS * c.M, ARGMAX_SLOTS * c.M, torch.int64, 0, 0, device)
    if c.ln:
        # per-64-column (mean, M2) of A's bf16 rows (the GPU test overwrites it with mit_row_stats64's), and
        # the folded weight's column sums
        parts = c.K // 64
        x = window(t["A"].whole, t["A"].spec).double().view(c.M, parts, 64)
        m = x.mean(-1)
        st = torch.stack([m, ((x - m[..., None]) ** 2).sum(-1)], -1).float().reshape(1, -1)
        t["ln_stats"] = Buf(1, st.numel(), st.numel(), torch.float32, NAN, 0, device, st)
        bw = window(t["B"].whole, t["B"].spec).double()
        t["ln_colsum"] = Buf(1, c.N, c.N, torch.float32, NAN, 0, device, bw.sum(1).float().view(1, -1))
    if c.drop_p > 0:
        seed = torch.tensor([1234 + c.site], dtype=torch.int64, device=device)
        t["seed"] = seed
        n = c.M * c.ldc
        if mask_fn is not None:
            t["mask"] = mask_fn(n, c.drop_p, seed, c.site)
        else:
            t["mask"] = (torch.rand(n, generator=g) >= c.drop_p).float().to(device) / (1.0 - c.drop_p)
    return t


def bufs(t):
    return {k: v for k, v in t.items() if isinstance(v, Buf)}


def snapshot(t):
    for b in bufs(t).values():
        b.snapshot()


def gemm_kwargs(case, t):
    """native.gemm(*args, **kwargs) of the case on its tensors (the workspace is the caller's)."""
    c = case
    res = t["C"].view if c.res_is_c else (t["residual"].view if c.residual else None)
    args = (t["A"].view, t["B"].view, None if c.argmax else t["C"].view, c.M, c.N, c.K)
    kw = dict(a_layout=c.al, b_layout=c.bl, lda=c.lda, ldb=c.ldb, ldc=c.ldc, bias=t["bias"].view if c.bias else None,
              act=c.act, residual=res, ldr=c.ldr, aux=t["aux"].view if c.aux else None, ld_aux=c.ld_aux,
              aux_scale=c.aux_scale, alpha=c.alpha, drop_p=c.drop_p, seed=t.get("seed"), site=c.site,
              accumulate=c.accumulate, rowsum=t["rowsum"].view if c.rowsum else None,
              ln_stats=t["ln_stats"].view if c.ln else None, ln_colsum=t["ln_colsum"].view if c.ln else None,
              ln_eps=LN_EPS if c.ln else 0.0, stats_out=t["stats_out"].view if c.stats else None, tiles=c.tiles,
              argmax_keys=t["keys"].view if c.argmax else None)
    return args, kw


def placeholder_args(case, native, workspace_bytes=None):
    """mit_gemm_args of the case with placeholder addresses of the case's alignment (mit_gemm_plan never
    dereferences them): what native.gemm builds from gemm_kwargs."""
    c = case
    esz = 2 if c.dtype == "bf16" else 4
    osz = 4 if c.out_dtype == torch.float32 else 2
    base = iter(range(0x7F0000000000, 0x7F0100000000, 0x1000000))
    p = {k: next(base) for k in ("A", "B", "C", "bias", "res", "aux", "seed", "rowsum", "ws", "ln_stats", "ln_colsum",
                                 "stats", "keys")}
    pc = p["C"] + c.mis_c * osz
    res = pc if c.res_is_c else (p["res"] if c.residual else None)
    if workspace_bytes is None:
        workspace_bytes = max(native.gemm_workspace_bytes(c.M, c.N, c.K), 4096) + 16
    return native.GemmArgs(
        native.BF16 if c.dtype == "bf16" else native.F32, c.al, c.bl, c.M, c.N, c.K, p["A"] + c.mis_a * esz, c.lda,
        p["B"] + c.mis_b * esz, c.ldb, None if c.argmax else pc, c.ldc, c.alpha, p["bias"] if c.bias else None, c.act, res,
        c.ldr, p["aux"] if c.aux else None, c.ld_aux, c.aux_scale, c.drop_p, p["seed"] if c.drop_p > 0 else None, c.site,
        1 if c.out_dtype == torch.float32 else 0, 1 if c.accumulate else 0, p["rowsum"] if c.rowsum else None,
        p["ws"] if c.workspace else None, workspace_bytes if c.workspace else 0, p["ln_stats"] if c.ln else None,
        p["ln_colsum"] if c.ln else None, c.K // 64 if c.ln else 0, LN_EPS if c.ln else 0.0,
        p["stats"] if c.stats else None, c.tiles, p["keys"] if c.argmax else None)


# ------------------------------------------------------------------------------------------------
# the contract in float64
# ------------------------------------------------------------------------------------------------
def _act(v, act):
    if act == ACT_RELU:
        return F.relu(v)
    if act == ACT_GELU:
        return F.gelu(v)
    if act == ACT_QUICK_GELU:
        return v * torch.sigmoid(1.702 * v)
    return v


def _formula(c, A, B, bias, aux, mask, res, prior, colsum):
    """C = out(dropout(auxmask(act(alpha A B + bias))) + residual) on logical float64 operands A [M, K], B [K, N];
    mask [M, N] keep-multipliers; prior = the output's previous contents (accumulate)."""
    acc = A @ B
    if c.ln:  # rstd_m (sum_k x_mk B_kn - mean_m colsum_n) + bias_n
        mean, var = A.mean(1, keepdim=True), A.var(1, unbiased=False, keepdim=True)
        v = (acc - mean * colsum) / torch.sqrt(var + LN_EPS)
    else:
        v = c.alpha * acc
    if bias is not None:
        v = v + bias
    v = _act(v, c.act)
    if aux is not None:
        v = v * torch.where(aux > 0, c.aux_scale, 0.0)
    if mask is not None:
        v = v * mask
    if res is not None:
        v = v + res
    if c.accumulate:
        v = v + prior
    return v


def stats64(y):
    """per-64-column (mean, M2) of each row, float64 [R, C / 64, 2]"""
    R, C = y.shape
    x = y.double().view(R, C // 64, 64)
    m = x.mean(-1)
    return torch.stack([m, ((x - m[..., None]) ** 2).sum(-1)], -1)


def reference(case, tensors):
    """float64 CPU evaluation of the header's formula from the pre-launch snapshots of the strided windows:
    {"C": [M, N], "rowsum": [M] = sum_k A(m, k), "argmax": [M]}. The dropout mask is the one mit_dropout_mask
    gives at index m * N + n."""
    c, t = case, tensors
    A = t["A"].data64() if c.al == K_CONTIG else t["A"].data64().t()
    B = t["B"].data64().t() if c.bl == K_CONTIG else t["B"].data64()
    bias = t["bias"].data64()[0, :c.N] if c.bias else None
    out = {"rowsum": A.sum(1)}
    if c.argmax:
        out["argmax"] = (A @ B + bias).argmax(1)
        return out
    aux = t["aux"].data64() if c.aux else None
    res = t["C"].data64() if c.res_is_c else (t["residual"].data64() if c.residual else None)
    mask = t["mask"][:c.M * c.N].view(c.M, c.N).cpu().double() if c.drop_p > 0 else None
    colsum = t["ln_colsum"].data64()[0] if c.ln else None
    out["C"] = _formula(c, A, B, bias, aux, mask, res, t["C"].data64(), colsum)
    return out


def _close(got, ref, tol, what):
    scale = max(ref.abs().max().item(), 1e-3)
    err = (got.detach().cpu().double() - ref).abs().max().item()
    print(f"{what}: max err {err:.3e} = {err / scale:.3e} of max|ref| {scale:.3e} (bound {tol:g})")
    assert err <= tol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e} (tol {tol})"
    return err / scale


def check(case, tensors, ref):
    """The outputs against the reference, then every buffer's guards: outputs outside their window, inputs
    everywhere."""
    c, t = case, tensors
    if c.argmax:
        k = t["keys"].view[0].view(ARGMAX_SLOTS, c.M).cpu() ^ torch.iinfo(torch.int64).min  # unsigned order
        best = k.max(0).values ^ torch.iinfo(torch.int64).min
        got = 0xFFFFFFFF - (best & 0xFFFFFFFF)
        assert torch.equal(got, ref["argmax"]), f"{c.id}: {(got != ref['argmax']).sum().item()} rows pick another column"
    else:
        _close(t["C"].view, ref["C"], c.tol, f"{c.id} C")
    if c.rowsum:
        _close(t["rowsum"].view[0], ref["rowsum"], c.rowsum_tol, f"{c.id} rowsum")
    if c.stats:
        want = stats64(t["C"].view.detach().cpu())
        got = t["stats_out"].view[0].view(c.M, c.N // 64, 2)
        _close(got, want, 1e-4, f"{c.id} stats_out")
    outputs = {"C", "rowsum", "stats_out", "keys"}
    for name, b in bufs(t).items():
        if name in outputs:
            b.check_untouched(f"{c.id} {name}")
        else:
            b.check_unchanged(f"{c.id} {name}")


# ------------------------------------------------------------------------------------------------
# a torch GEMM on the strided windows with injectable faults (the harness's self-check)
# ------------------------------------------------------------------------------------------------
FAULTS = ("pad_column", "past_row_m", "head_guard", "k_round8", "res_ldc", "aux_ldr", "drop_ldc", "rowsum_b",
          "no_accumulate")


def fault_applies(case, fault):
    c = case
    return {"pad_column": not c.argmax and c.ldc > c.N, "past_row_m": not c.argmax, "head_guard": not c.argmax,
            "k_round8": c.al == K_CONTIG and not c.argmax, "res_ldc": c.residual and not c.res_is_c and c.ldr != c.ldc,
            "aux_ldr": c.aux and c.ld_aux != c.ldr, "drop_ldc": c.drop_p > 0 and c.ldc != c.N, "rowsum_b": c.rowsum,
            "no_accumulate": c.accumulate}[fault]


def _restrided(buf, rows, cols, ld):
    """the window re-read with another geometry (a kernel using the wrong leading dimension / extent)"""
    off = buf.spec[0]
    flat = buf.whole
    return flat.as_strided((rows, cols), (ld, 1), flat.storage_offset() + off).double()


def fake_gemm(case, tensors, fault=None):
    """The contract in torch on the strided windows, writing C / rowsum / stats_out like a kernel would; `fault`
    (one of FAULTS) makes it subtly wrong in the way a kernel could be."""
    c, t = case, tensors
    assert fault is None or fault_applies(c, fault)
    A = t["A"].view.double()
    B = t["B"].view.double()
    if fault == "k_round8":  # one more 8-wide chunk of every A row: pad (NaN) against zero-extended B
        k8 = (c.K + 8) // 8 * 8
        A = _restrided(t["A"], c.M, k8, c.lda)
        Bk = B if c.bl == K_CONTIG else B.t()  # [N, K]
        B = torch.cat([Bk, torch.zeros(c.N, k8 - c.K, dtype=torch.float64)], 1)
        B = B if c.bl == K_CONTIG else B.t()
    A = A if c.al == K_CONTIG else A.t()
    B = B.t() if c.bl == K_CONTIG else B
    bias = t["bias"].view[0, :c.N].double() if c.bias else None
    aux = res = mask = colsum = None
    if c.aux:
        aux = _restrided(t["aux"], c.M, c.N, c.ldr) if fault == "aux_ldr" else t["aux"].view.double()
    if c.res_is_c:
        res = t["C"].view.double()
    elif c.residual:
        res = _restrided(t["residual"], c.M, c.N, c.ldc) if fault == "res_ldc" else t["residual"].view.double()
    if c.drop_p > 0:
        m = t["mask"].double()
        mask = m.as_strided((c.M, c.N), (c.ldc, 1)) if fault == "drop_ldc" else m[:c.M * c.N].view(c.M, c.N)
    if c.ln:
        colsum = t["ln_colsum"].view[0].double()
    cc = replace(c, accumulate=False) if fault == "no_accumulate" else c
    v = _formula(cc, A, B, bias, aux, mask, res, t["C"].view.double(), colsum)
    C = t["C"]
    C.view.copy_(v.to(C.view.dtype))
    if c.rowsum:
        rs = B.sum(0)[torch.arange(c.M) % c.N] if fault == "rowsum_b" else A.sum(1)
        t["rowsum"].view[0].copy_(rs.float())
    if c.stats:
        t["stats_out"].view[0].copy_(stats64(C.view).float().reshape(-1))
    off = C.spec[0]
    if fault == "pad_column":
        C.whole[off + (c.M - 1) * c.ldc + c.N] = 1.0
    elif fault == "past_row_m":
        C.whole[off + c.M * c.ldc] = 1.0
    elif fault == "head_guard":
        C.whole[off - 1] = 1.0
