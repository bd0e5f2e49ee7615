"""The LayerNorm contract harness (tests/ln_contract.py) without a GPU:
  * its float64 reference equals F.layer_norm and autograd in float64;
  * every case plans onto the kernel family and NV instance it names (mit_layernorm_plan on the case's CPU
    buffers: same leading dimensions and alignment, nothing dereferenced), and the table hits every family, every
    NV instance and both sides of every boundary of csrc/norm.hip's dispatch, each alignment rule alone;
  * the harness catches a subtly wrong kernel: FakeOps, a torch implementation on the same guarded buffers,
    passes every case as it is, stays within every bound in float32 (on a bf16 case: the bf16 emulation) under
    sequential and 64-lane-tree summation, and fails the named case(s) with each injected fault;
  * the rejected calls return MIT_ERR_INVALID with their message (argument checks come before any launch)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import ln_contract as lc
import native

CASES = lc.CASES
_cache = {}


def _tensors_and_ref(case):
    """one set of buffers and one float64 reference per case, shared (run_case leaves the inputs as they were)"""
    if case.id not in _cache:
        t = lc.make_tensors(case)
        _cache[case.id] = (t, lc.reference(case, t))
    return _cache[case.id]


def _run_fake(case, math="f64", fault=None):
    t, ref = _tensors_and_ref(case)
    return lc.run_case(case, t, lc.FakeOps(math, fault), ref, twice=fault is None)


@pytest.mark.parametrize("case", [c for c in lc.LN_CASES if c.cols > 1], ids=lambda c: c.id)
def test_reference_equals_layer_norm_and_autograd(case):
    c = case
    t, ref = _tensors_and_ref(c)
    z = ref["z"].clone().requires_grad_(True)
    g = t.row("gamma").double().clone().requires_grad_(True)
    b = t.row("beta").double().clone().requires_grad_(True)
    y = F.layer_norm(z, (c.cols,), g, b, c.eps)
    torch.testing.assert_close(ref["y"], y.detach(), rtol=1e-9, atol=1e-9)
    torch.testing.assert_close(ref["mean"], z.detach().mean(1), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(ref["rstd"], torch.rsqrt(z.detach().var(1, unbiased=False) + c.eps), rtol=1e-12, atol=0)
    if not c.bwd:
        return
    # the backward's inputs are the forward's results rounded (z to the dtype, mean / rstd to f32): autograd at those
    # rounded z agrees with the closed form to the size of that rounding, and exactly on exact inputs (f64 below)
    t2 = lc.make_tensors(c)
    zb = t2.v("bz").double().requires_grad_(True)
    y2 = F.layer_norm(zb, (c.cols,), g, b, c.eps)
    y2.backward(t2.v("dy").double())
    t2.row("bmean").copy_(zb.detach().mean(1).float())
    t2.row("brstd").copy_(torch.rsqrt(zb.detach().var(1, unbiased=False) + c.eps).float())
    r2 = lc.reference(c, t2)
    scale = lambda x: x.abs().max().item()
    # mean / rstd carry an f32 rounding (2^-24 relative); xhat amplifies the mean's by |mean| rstd <= 8 / 0.05
    tol = 2.0 ** -24 * 8 / 0.05 * 8
    assert (r2["dx"] - zb.grad).abs().max().item() <= tol * scale(zb.grad)
    assert (r2["dgamma"] - g.grad).abs().max().item() <= tol * max(scale(g.grad), r2["u_dgamma"].max().item() / lc.ULP)
    torch.testing.assert_close(r2["dbeta"], b.grad, rtol=1e-12, atol=1e-9)


@pytest.mark.parametrize("case", lc.LN_CASES, ids=lambda c: c.id)
def test_case_plans_onto_its_family_and_nv(case):
    t, _ = _tensors_and_ref(case)
    assert lc.planned(case, t, native) == (case.fwd, case.bwd)


def test_table_hits_every_family_every_nv_and_both_sides_of_every_boundary():
    cs = lc.LN_CASES
    fwd = {(c.dtype,) + c.fwd for c in cs}
    bwd = {(c.dtype,) + c.bwd for c in cs if c.bwd}
    # every template instance csrc/norm.hip can launch
    assert {f[1:] for f in fwd if f[1] == "pair"} == {("pair", 1), ("pair", 3)}
    assert {f[1:] for f in fwd if f[1] == "wide"} == {("wide", 1), ("wide", 2)}
    assert {f[1:] for f in bwd if f[1] == "wide"} == {("wide", 1), ("wide", 2)}
    for side in (fwd, bwd):
        assert {f[2] for f in side if f[:2] == ("f32", "vec4")} == {1, 2, 3, 4, 8}
        assert {f[2] for f in side if f[:2] == ("bf16", "vec4")} >= {2, 8}
        for dt in ("f32", "bf16"):
            assert {f[2] for f in side if f[:2] == (dt, "scalar")} == {1, 2, 3, 4, 8, 16, 32}, (dt, side)
    # both sides of every boundary, on aligned bf16 operands with the default leading dimensions
    ok = [c for c in cs if c.dtype == "bf16" and not c.mis and c.pad is None and c.bwd]
    plain = {c.cols: c for c in ok if not c.r}
    with_r = {c.cols: c for c in ok if c.r}
    both = {**plain, **with_r}
    assert both[512].fwd == ("wide", 1) and both[520].fwd == ("wide", 2)            # NV 1 | 2 of the wide kernels
    assert both[512].bwd == ("wide", 1) and both[520].bwd == ("wide", 2)
    assert both[1024].fwd == ("wide", 2) and both[1032].fwd == ("scalar", 32)       # the wide limit
    assert both[1024].bwd == ("wide", 2) and both[1032].bwd == ("scalar", 32)
    assert both[1016].fwd == ("wide", 2) and both[1280].fwd == ("vec4", 8) and both[2040].fwd == ("scalar", 32)
    assert both[2048].fwd == ("vec4", 8) and both[2048].bwd == ("vec4", 8)          # MAXV_ALL: 2056 is rejected
    assert any(r[2].get("cols") == 2056 for r in lc.REJECTIONS if r[1] == "fwd")
    assert any(r[2].get("cols") == 2056 for r in lc.REJECTIONS if r[1] == "bwd")
    assert plain[256].fwd == ("pair", 1) and with_r[256].fwd == ("pair", 1)          # the pair widths
    assert plain[768].fwd == ("wide", 2) and with_r[768].fwd == ("pair", 3)
    assert both[8].fwd == ("wide", 1) and both[136].fwd == ("wide", 1)
    pair = [c for c in cs if c.fwd[0] == "pair"]
    assert {c.rows for c in pair} >= {1, 8, 9, 13} and any(c.drop_p for c in pair) and any(not c.z for c in pair)
    assert {c.rows for c in cs} == {1, 5, 8, 9, 13}  # around the 4-row forward, 8-row pair and backward blocks
    # each alignment rule alone
    rule = {c.id: (c.fwd, c.bwd) for c in cs if c.id.startswith("align-")}
    w1 = ("wide", 1)
    assert rule == {
        "align-x4": (("vec4", 2), w1), "align-x1": (("scalar", 8), w1), "align-ldx4": (("vec4", 2), w1),
        "align-ldx-odd": (("scalar", 8), w1), "align-ldr4": (("vec4", 2), w1), "align-y4": (("vec4", 2), w1),
        "align-z4": (("vec4", 2), w1), "align-gamma1": (("scalar", 8), ("scalar", 8)),
        "align-f32-256-ldx6": (("scalar", 4), ("vec4", 1)),
        "align-bwd-dy4": (w1, ("vec4", 2)), "align-bwd-bz4": (w1, ("vec4", 2)), "align-bwd-dx4": (w1, ("vec4", 2)),
        "align-bwd-dr4": (w1, ("vec4", 2)), "align-bwd-dy1": (w1, ("scalar", 8)),
        "align-bwd-f32-dx1": (("vec4", 1), ("scalar", 4))}
    for c in cs:
        if c.id.startswith("align-"):
            ldx, ldr, ldy = c.lds
            broken = len(c.mis) + (ldx % 8 != 0) + (ldr % 8 != 0) + (ldy % 8 != 0) if c.dtype == "bf16" else \
                len(c.mis) + (ldx % 4 != 0)
            assert broken == 1, c.id
    # modes
    assert any(c.drop_p and not c.r for c in cs) and any(c.r and c.drop_p for c in cs) and any(c.r and not c.drop_p for c in cs)
    assert any(not c.z for c in cs) and any(not c.mean and c.rstd for c in cs) and any(c.mean and not c.rstd for c in cs)
    assert {c.eps for c in cs} == {1e-5, 1e-12}
    for fam in ("scalar", "vec4", "wide"):
        b = [c for c in cs if c.bwd and c.bwd[0] == fam]
        assert any(not c.dr for c in b) and any(c.dr and c.bwd_drop_p for c in b) and any(c.dr and not c.bwd_drop_p for c in b), fam
        assert any(c.alias_dx for c in b) and any(c.rows % lc.BWD_ROWS for c in b) and any(c.rows == 8 for c in b), fam
    # the other entry points
    pg = [c for c in CASES if c.op == "pgrad"]
    assert {c.nblk for c in pg} == {1, 16, 17, 49, 64, 65, 131} and {c.cols for c in pg} == {8, 130, 512}
    assert all(c.rows == 8 * c.nblk - 3 and lc.ws_floats(c.rows, c.cols) == c.nblk * 2 * c.cols for c in pg)
    x32 = [c for c in CASES if c.op == "x32"]
    assert {c.cols for c in x32} == {8, 264, 512, 520, 1024} and {c.dtype for c in x32} == {"bf16", "f32"}
    assert {c.z for c in x32} == {None, "sep", "alias"} and {c.r for c in x32} == {True, False}
    assert any(c.lds[0] > c.cols for c in x32) and all(c.lds[1] > c.cols and c.lds[2] > c.cols for c in x32)
    ro = [c for c in CASES if c.op == "resout"]
    assert any(c.rows * (c.cols // 8) > lc.RESOUT_GRID_CAP for c in ro) and {c.r for c in ro} == {True, False}
    st = [c for c in CASES if c.op == "stats64"]
    assert {c.cols for c in st} == {64, 448, 512, 576, 1024} and {c.rows for c in st} == {1, 5}


def test_buffers_are_guarded_strided_and_exact_size():
    c = lc.BY_ID["wide-1024"]
    t = lc.make_tensors(c)
    ref = lc.reference(c, t)
    ldx, ldr, ldy = c.lds
    assert (ldx, ldr, ldy) == (1032, 1040, 1048)
    x = t.b["x"]
    assert x.whole[:lc.GUARD].isnan().all() and x.whole[-lc.GUARD:].isnan().all()
    rows = x.whole[lc.GUARD:lc.GUARD + c.rows * ldx].view(c.rows, ldx)
    assert rows[:, c.cols:].isnan().all() and rows[:, :c.cols].isfinite().all()
    assert (t.b["y"].whole == lc.SENTINEL).all()
    for name, n in (("z", c.rows * c.cols), ("mean", c.rows), ("rstd", c.rows), ("dgamma", c.cols), ("dbeta", c.cols),
                    ("ws", lc.ws_floats(c.rows, c.cols))):
        assert t.b[name].whole.numel() == n + 2 * lc.GUARD, name
    assert lc.ws_floats(c.rows, c.cols) == native.load_library().mit_layernorm_bwd_ws_floats(c.rows, c.cols)
    # inputs that give every term weight
    k = lc.const_row(c)
    z = ref["z"]
    assert (z[k] == 2.0).all() and ref["rstd"][k].item() == pytest.approx(c.eps ** -0.5, rel=1e-12)
    others = [i for i in range(c.rows) if i != k]
    sd = z[others].std(1)
    assert sd.min() >= 0.04 and sd.max() <= 5.0 and z[others].mean(1).abs().max() <= 8.6
    dy = t.v("dy").double()
    g = dy * t.row("gamma").double()
    assert (g.mean(1).abs() / g.abs().amax(1)).max() > 0.1  # mean(g) is O(1) of dx's terms


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_faultless_fake_passes(case):
    _run_fake(case)


@pytest.mark.parametrize("math", ["seq", "tree"])  # the two orders the bounds were measured under
@pytest.mark.parametrize("case", [c for c in CASES if not c.id.startswith("resout-past")], ids=lambda c: c.id)
def test_float32_fake_is_within_every_bound(case, math):
    """float32 math on the rounded inputs, outputs rounded on the store: on the bf16 cases the bf16 emulation"""
    _run_fake(case, math=math)


def test_every_fault_names_cases_that_exist():
    for f, ids in lc.FAULT_CASE.items():
        assert ids and all(i in lc.BY_ID for i in ids), f
    s1 = {lc.BY_ID[i].cols for i in lc.FAULT_CASE["no_s1"] if lc.BY_ID[i].dtype == "bf16"}
    assert s1 >= {768, 1024}  # ln_bwd_wide_kernel<2>: the widths at which a dropped mean(g) passed the older bound


@pytest.mark.parametrize("fault,cid", [(f, i) for f, ids in lc.FAULT_CASE.items() for i in ids])
def test_injected_fault_is_caught(fault, cid):
    case = lc.BY_ID[cid]
    t, ref = _tensors_and_ref(case)
    try:
        with pytest.raises(AssertionError):
            lc.run_case(case, t, lc.FakeOps("f64", fault), ref)
        with pytest.raises(AssertionError):  # ... and in the bf16 emulation / float32
            lc.run_case(case, t, lc.FakeOps("tree", fault), ref)
    finally:  # a run that stopped half-way may have left an aliased input overwritten
        del _cache[cid]


@pytest.mark.parametrize("rid,entry,change,frag", lc.REJECTIONS, ids=[r[0] for r in lc.REJECTIONS])
def test_rejections(rid, entry, change, frag):
    lib = native.load_library()
    rows, cols = 5, change.get("cols", 512)
    ld = change.get("ld", cols)
    n = rows * max(ld, 2056) + 64
    buf = {k: torch.zeros(n, dtype=torch.float32) for k in ("x", "r", "y", "z", "g", "b", "m", "s", "dg", "db", "ws")}
    p = {k: v.data_ptr() + (-v.data_ptr()) % 16 for k, v in buf.items()}
    ldx, ldy = change.get("ldx", ld), change.get("ldy", ld)
    if entry == "fwd":
        rc = lib.mit_layernorm_fwd(native.BF16, rows, cols, p["x"], ldx, None, ld, 0.0, None, 0, p["g"], p["b"], 1e-5,
                                   None, p["y"], ldy, None, None, None)
    elif entry == "bwd":
        rc = lib.mit_layernorm_bwd(native.BF16, rows, cols, p["x"], p["z"], p["m"], p["s"], p["g"], p["y"], None, 0.0,
                                   None, 0, p["dg"] if change.get("dgamma", True) else None,
                                   p["db"] if change.get("dbeta", True) else None, p["ws"], None)
    elif entry == "x32":
        y = p["x"] if change.get("y_is_x") else p["y"]
        rc = lib.mit_layernorm_fwd_x32(rows, cols, p["x"], ldx, p["r"], ld, p["z"] if change.get("z") else None, p["g"],
                                       p["b"], 1e-5, y, native.BF16, ldy, None)
    elif entry == "stats64":
        rc = lib.mit_row_stats64(rows, cols, p["x"], ld, p["y"], None)
    else:
        out = native.LnPlan()
        rc = lib.mit_layernorm_plan(native.BF16, rows, cols, p["x"], ld, None, ld, None, p["y"], ld, p["g"], p["b"],
                                    None, None, None, ctypes.byref(out))
    assert rc == 1, rid  # MIT_ERR_INVALID
    assert frag in lib.mit_last_error(), (rid, lib.mit_last_error())


def test_plan_rejects_nulls_and_reports_each_direction_alone():
    lib = native.load_library()
    assert lib.mit_layernorm_plan(native.BF16, 5, 512, None, 512, None, 512, None, None, 512, None, None, None, None,
                                  None, None) == 1
    assert b"null pointer" in lib.mit_last_error()
    out = native.LnPlan()
    assert lib.mit_layernorm_plan(native.BF16, 5, 512, None, 512, None, 512, None, None, 512, None, None, None, None,
                                  None, ctypes.byref(out)) == 1
    assert b"neither" in lib.mit_last_error()
    assert lib.mit_layernorm_plan(7, 5, 512, None, 512, None, 512, None, None, 512, None, None, None, None, None,
                                  ctypes.byref(out)) == 1
    assert b"bad dtype" in lib.mit_last_error()
    c = lc.BY_ID["wide-1024"]
    t, _ = _tensors_and_ref(c)
    with pytest.raises(native.NativeError, match="null pointer"):  # a forward without y
        native.layernorm_plan(native.BF16, c.rows, c.cols, x=t.v("x"), ldx=c.lds[0], gamma=t.row("gamma"), beta=t.row("beta"))
    with pytest.raises(native.NativeError, match="null pointer"):  # a backward without z
        native.layernorm_plan(native.BF16, c.rows, c.cols, dy=t.v("dy"), dx=t.v("dx"), gamma=t.row("gamma"))
    both = native.layernorm_plan(native.BF16, c.rows, c.cols, x=t.v("x"), ldx=c.lds[0], r=t.v("r"), ldr=c.lds[1], y=t.v("y"),
                                 ldy=c.lds[2], z=t.v("bz"), gamma=t.row("gamma"), beta=t.row("beta"), dy=t.v("dy"),
                                 dx=t.v("dx"), dr=t.v("dr"))
    assert (both.fwd, both.fwd_nv, both.bwd, both.bwd_nv) == (native.LN_WIDE, 2, native.LN_WIDE, 2)
