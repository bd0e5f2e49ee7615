"""The contract harness of csrc/misc.hip (tests/misc_contract.py) without a GPU:
  * its float64 reference equals F.cross_entropy and its autograd, F.embedding's backward, torch.optim.AdamW and
    clip_grad_norm_ in float64, F.conv2d (im2col) and a stable sort; its host mask follows csrc/common.h;
  * every case plans onto the kernel family it names (mit_cross_entropy_plan, mit_im2col_plan,
    mit_vit_assemble_plan, mit_embed_plan_keys_per_thread on the case's CPU buffers: same leading dimensions and
    alignment, nothing dereferenced), and the table reaches both cross-entropy kernels on both sides of 10240, both
    families of im2col and of assemble, all five key counts of the embedding plan, the 4-row and 16-row boundaries;
  * the harness catches a subtly wrong kernel: FakeOps, a torch implementation on the same guarded buffers, passes
    every case as it is, stays within every bound in float32 (on a bf16 case: the bf16 emulation) in both of its
    modes, and fails the named case(s) with each injected fault;
  * the rejected calls return MIT_ERR_INVALID with their message, and the queries -1 (argument checks come before
    any launch)."""
import pytest
import torch
import torch.nn.functional as F

import misc_contract as mc
import native

CASES = mc.CASES
_cache = {}


def _tensors_and_ref(case):
    """one set of buffers and one float64 reference per case, shared (run_case leaves the buffers as they were)"""
    if case.id not in _cache:
        t = mc.make_tensors(case)
        _cache[case.id] = (t, mc.reference(case, t))
    return _cache[case.id]


def _run_fake(case, math="f64", fault=None):
    t, ref = _tensors_and_ref(case)
    return mc.run_case(case, t, mc.FakeOps(math, fault), ref, twice=fault is None)


def _of(op):
    return [c for c in CASES if c.op == op]


# ------------------------------------------------------------------------------------------------
# the reference against torch
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", _of("ce"), ids=lambda c: c.id)
def test_reference_equals_cross_entropy_and_autograd(case):
    c = case
    t, ref = _tensors_and_ref(c)
    x = t.v("logits").double().clone().requires_grad_(True)
    tg = t.row("targets")
    per_row = F.cross_entropy(x, tg, ignore_index=mc.CE_IGNORE, reduction="none")
    torch.testing.assert_close(ref["loss"], per_row.detach(), rtol=1e-12, atol=1e-12)
    assert ref["sum"] == pytest.approx(c.loss0 + per_row.sum().item(), rel=1e-12)
    # the gradient of sum / count, count the global one (here: the local count + 3)
    count = t.row("count").double().item()
    assert count == float((tg != mc.CE_IGNORE).sum()) + 3
    (per_row.sum() / count).backward()
    torch.testing.assert_close(ref["grad"], x.grad, rtol=1e-10, atol=1e-18)
    assert (ref["grad"][tg == mc.CE_IGNORE] == 0).all()
    if c.rows >= 4:  # the inputs that give every term weight
        xd = x.detach()
        assert xd[0].argmax().item() == c.cols - 1 and (xd[1] == xd[1, 0]).all()
        assert xd[3].max().item() - xd[3].topk(2).values[1].item() >= 59
        if tg[1] != mc.CE_IGNORE:
            assert ref["loss"][1].item() == pytest.approx(torch.log(torch.tensor(float(c.cols), dtype=torch.float64)).item(), rel=1e-14)


@pytest.mark.parametrize("case", [c for c in _of("embbwd") if c.drop_p == 0], ids=lambda c: c.id)
def test_reference_equals_embedding_backward(case):
    c = case
    t, ref = _tensors_and_ref(c)
    tok = t.row("tokens")
    w = torch.zeros(mc.BWD_VOCAB, c.cols, dtype=torch.float64, requires_grad=True)
    out = F.embedding(tok, w, padding_idx=mc.PAD) * mc.f32r(c.cols ** 0.5)
    out.backward(t.v("dx").double())
    want = w.grad if c.planned else w.grad + t.v("dtable").double()
    torch.testing.assert_close(ref["grad"], want, rtol=1e-12, atol=1e-12)
    counts = torch.bincount(tok, minlength=mc.BWD_VOCAB).tolist()
    if c.layout == "runs":  # runs of exactly 1, 15, 16, 17 and 33 rows around the 16 rows in flight, PAD present
        assert counts == [mc.BWD_PADS, 1, 15, 16, 17, 33, 0, 0] and ref["present"].tolist() == [False] + [True] * 5 + [False] * 2
    else:
        assert counts[0] == c.B * c.T and not ref["present"].any()


@pytest.mark.parametrize("case", _of("embfwd")[:6], ids=lambda c: c.id)
def test_reference_equals_embedding_forward(case):
    c = case
    t, ref = _tensors_and_ref(c)
    tok = t.row("tokens").view(c.B, c.T)
    x = F.embedding(tok, t.v("table").double()) * mc.f32r(c.cols ** 0.5) + t.v("pe").double()[:c.T][None]
    m = ref["mask"].view(c.B, c.T, c.cols)
    torch.testing.assert_close(ref["out"].view(c.B, c.T, c.cols), x * m, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("case", _of("adamw") + _of("adamchain"), ids=lambda c: c.id)
def test_reference_equals_torch_adamw(case):
    c = case
    t, ref = _tensors_and_ref(c)
    p = t.row("p").double().clone().requires_grad_(True)
    g = t.row("g").double()
    opt = torch.optim.AdamW([p], lr=mc.f32r(c.lr), betas=(mc.B1, mc.B2), eps=mc.EPS, weight_decay=mc.f32r(c.wd))
    if c.op == "adamchain":
        for s, lr in enumerate(mc.CHAIN_LR, start=1):
            opt.param_groups[0]["lr"] = mc.f32r(lr)
            p.grad = g * s
            opt.step()
        assert mc.CHAIN_LR[1] != mc.CHAIN_LR[2]  # the lr changes at step 3
    else:
        st = opt.state[p]
        st["step"] = torch.tensor(float(c.step - 1))
        st["exp_avg"], st["exp_avg_sq"] = t.row("m").double().clone(), t.row("v").double().clone()
        p.grad = g * (c.coef if c.norm else 1.0)
        opt.step()
        torch.testing.assert_close(ref["m"], opt.state[p]["exp_avg"], rtol=1e-12, atol=1e-15)
        torch.testing.assert_close(ref["v"], opt.state[p]["exp_avg_sq"], rtol=1e-12, atol=1e-18)
    torch.testing.assert_close(ref["p"], p.detach(), rtol=1e-11, atol=1e-13)


@pytest.mark.parametrize("case", _of("gnorm"), ids=lambda c: c.id)
def test_reference_equals_clip_grad_norm(case):
    c = case
    t, ref = _tensors_and_ref(c)
    p = torch.zeros(c.cols, dtype=torch.float64, requires_grad=True)
    p.grad = t.row("grads").double().clone()
    mx = t.x["max_norm"]
    if mx > 0:
        total = torch.nn.utils.clip_grad_norm_([p], mx)
        assert ref["norm"] == pytest.approx(total.item(), rel=1e-13)
        want = t.row("grads").double() * ref["coef"]
        torch.testing.assert_close(p.grad, want, rtol=1e-12, atol=0)
    else:
        assert ref["coef"] == 1.0
    if c.gmode == "mixed":
        a = t.row("grads").abs()
        assert c.cols < 1000 or (a.min() < 1e-2 and a.max() > 1e2)
        side = {0.5: ref["coef"] < 0.51, 2.0: ref["coef"] == 1.0}.get(c.max_norm)
        assert side is None or side


@pytest.mark.parametrize("case", [c for c in _of("im2col") if not c.mis], ids=lambda c: c.id)
def test_reference_equals_conv2d_unfold(case):
    c = case
    t, ref = _tensors_and_ref(c)
    C, H, W, P, kpad = c.geom
    assert H != W and c.B == 2
    img = t.row("img").view(c.B, C, H, W)
    k = C * P * P
    y = F.conv2d(img, torch.eye(k).view(k, C, P, P), stride=P)           # [B, k, nph, npw]: the patch Conv2d
    want = y.flatten(2).transpose(1, 2).reshape(-1, k)                    # row b * np + p
    assert torch.equal(ref["out"][:, :k].float(), want.to(ref["out"].dtype).float())
    assert (mc._bits(ref["out"][:, k:]) == 0).all() and ref["out"].shape == (c.B * (H // P) * (W // P), kpad)


@pytest.mark.parametrize("case", _of("colsum")[::7], ids=lambda c: c.id)
def test_reference_colsum(case):
    c = case
    t, ref = _tensors_and_ref(c)
    s = t.v("dy").double()[:c.rows].sum(0) + (t.row("out").double() if c.accumulate else 0)
    torch.testing.assert_close(ref["out"], s, rtol=1e-13, atol=1e-13)


def test_host_mask_follows_the_documented_hash():
    """scalar Python integers, straight from csrc/common.h, against the vectorised torch form"""
    def lowbias32(x):
        x ^= x >> 16
        x = (x * 0x7feb352d) & mc.M32
        x ^= x >> 15
        x = (x * 0x846ca68b) & mc.M32
        return x ^ (x >> 16)
    for seed, site, p in ((None, 0, 0.1), (5, 7, 0.5), (2 ** 40 + 3, 7, 0.1)):
        key = (seed or 0) ^ ((0xD6E8FEB86659FD93 * (site + 1)) % 2 ** 64)
        k = (key & mc.M32) ^ (((key >> 32) * 0x9E3779B9) & mc.M32)
        thresh = int(mc.f32r(p) * 2 ** 32)
        want = [lowbias32(i ^ k) >= thresh for i in range(300)]
        got = mc.host_mask(300, p, seed, site)
        assert (got != 0).tolist() == want
        assert got.max().item() == (torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(p))).item()
    assert int(mc.f32r(0.5) * 2 ** 32) == 2 ** 31 and lowbias32(0) == 0


def test_cast_reference_is_torch_to_with_the_nan_image_pinned():
    src = mc.make_tensors(mc.BY_ID["cast-bf16-specials"]).row("src")
    ref, tt = mc.to_dtype(src, torch.bfloat16), src.to(torch.bfloat16)
    ok = ~src.isnan()
    assert ok.sum() == src.numel() - 1 and torch.equal(mc._bits(ref[ok]), mc._bits(tt[ok]))
    assert (mc._bits(ref[~ok]) == 0x7FC0).all() and tt[~ok].isnan().all()
    assert mc._bits(torch.tensor(float("nan")).to(torch.bfloat16)).item() == 0x7FC0  # torch's scalar path agrees
    assert ref[7].item() == 0 and mc._bits(ref)[7].item() == -32768 and ref[11].isinf() and ref[13].item() == 0


def test_stable_plan():
    tok = torch.tensor([3, 1, 3, 0, 1, 3])
    assert mc.stable_plan(tok).tolist() == [3, 1, 4, 0, 2, 5, 1, 2, 0, 3, 0, 0]
    for c in _of("embplan"):
        t, ref = _tensors_and_ref(c)
        tk = t.row("tokens")
        if c.cols > 2:
            assert tk[1] == 0 and tk[2] == mc.EMB_VOCAB - 1 and (tk[::17] == 7).all()  # smallest, largest id, a long run


# ------------------------------------------------------------------------------------------------
# the planned families
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in CASES if mc.expected_plan(c) is not None], ids=lambda c: c.id)
def test_case_plans_onto_its_family(case):
    t, _ = _tensors_and_ref(case)
    assert mc.planned(case, t, native) == mc.expected_plan(case)


def test_table_reaches_every_path():
    ce = _of("ce")
    rows_k = {c.cols: c for c in ce if c.plan == mc.CE_ROWS}
    block = [c for c in ce if c.plan == mc.CE_BLOCK]
    assert set(rows_k) == {8, 512, 520, 10240, 7, 509, 10233}
    assert {c.cols for c in block if c.dtype == "bf16" and c.row_loss and c.cols > mc.CE_ROWS_MAX_V} == {10241, 10248}
    assert {c.rows for c in ce} == {1, 4, 5, 9}  # around the 4 rows per block of ce_rows_bf16
    assert all(c.ld == mc.r8(c.cols) for c in rows_k.values() if c.cols % 8)
    by = lambda pred: any(pred(c) for c in block)
    assert by(lambda c: c.dtype == "f32" and c.row_loss) and by(lambda c: c.dtype == "f32" and not c.row_loss)
    assert by(lambda c: c.dtype == "bf16" and c.cols == 512 and not c.row_loss)
    assert by(lambda c: c.dtype == "bf16" and c.cols == 512 and c.misalign("logits") == 4)   # 8 B off
    assert by(lambda c: c.cols == 520 and c.ld == 523) and by(lambda c: c.cols == 300)
    for group in ([c for c in ce if c.plan == mc.CE_ROWS], block):
        assert {c.ignore for c in group} == {"third", "all", "none"} and {c.want_grad for c in group} == {True, False}
        assert any(c.loss0 == 3.5 for c in group) and any(c.cols % 8 for c in group)
        assert any((mc.ce_targets(c) == 0).any() for c in group) and any((mc.ce_targets(c) == c.cols - 1).any() for c in group)
        assert any(((mc.ce_targets(c) >= (c.cols - 1) // 8 * 8) & (mc.ce_targets(c) < c.cols - 1)).any() for c in group)
    assert {c.plan for c in _of("embplan")} == {1, 2, 4, 8, 16}
    assert [c.cols for c in _of("embplan")] == [1, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 16384]
    assert [c.cols for c in _of("embplan") if c.plan == 8] == [4097, 8192]  # the instance no other test launches
    im, asm = _of("im2col"), _of("assemble")
    for dt in ("bf16",):
        assert {c.plan for c in im if c.dtype == dt} == {mc.ELT_SCALAR, mc.ELT_VEC8}
        assert {c.plan for c in asm if c.dtype == dt} == {mc.ELT_SCALAR, mc.ELT_VEC8}
    assert any(c.plan == mc.ELT_SCALAR and c.mis for c in im) and any(c.geom[4] > c.geom[0] * c.geom[3] ** 2 for c in im)
    assert {c.geom for c in asm if not c.mis} == {(n, e) for n in (1, 6) for e in (8, 96, 100)}
    bw = [c for c in _of("embbwd") if c.planned]
    assert {c.cols for c in bw} == {8, 128, 520, 1024} and {c.dtype for c in bw} == {"bf16", "f32"}
    assert set(mc.BWD_RUNS) == {1, 15, 16, 17, 33} and {c.drop_p for c in bw} == {0.0, 0.1}
    assert {c.cols for c in _of("embbwd") if not c.planned} == {8, 130}
    assert any(c.B * c.T * c.cols > mc.GRID_CAP for c in _of("embfwd")) and {c.seed for c in _of("embfwd")} == {"none", "small", "big"}
    cs = _of("colsum")
    assert {c.rows for c in cs} == {0, 1, 127, 128, 129, 257} and {c.cols for c in cs} == {1, 256, 300}
    assert {c.ld - c.cols for c in cs} == {0, 8} and {c.accumulate for c in cs} == {False, True}
    assert [c.cols for c in _of("count")] == [1, 255, 16385, 40000] and 40000 > 64 * 256
    assert {c.cols for c in _of("gnorm") if c.gmode == "mixed" and c.max_norm > 0} == {1, 3, 4, 5, 1027, 262147}
    ad = _of("adamw")
    assert {c.cols for c in ad} == {1, 3, 4, 7, 4098} and {c.step for c in ad} == {1, 2, 1000}
    assert {(c.shadow, c.norm) for c in ad if c.cols == 7} == {(a, b) for a in (True, False) for b in (True, False)}
    assert {c.coef for c in ad} == {0.25, 1.0} and {c.wd for c in ad} == {0.0, 0.1}
    assert any(c.cols > mc.GRID_CAP for c in _of("cast")) and len(_of("mask")) == 12


def test_buffers_are_guarded_strided_and_exact_size():
    lib = native.load_library()
    c = mc.BY_ID["ce-rows-509"]
    t = mc.make_tensors(c)
    L = t.b["logits"]
    assert c.ld == 512 and L.whole[:mc.GUARD].isnan().all() and L.whole[-mc.GUARD:].isnan().all()
    rows = L.whole[mc.GUARD:mc.GUARD + c.rows * c.ld].view(c.rows, c.ld)
    assert rows[:, c.cols:].isnan().all() and rows[:, :c.cols].isfinite().all()
    assert t.b["row_loss"].whole.numel() == c.rows + 2 * mc.GUARD and (t.b["row_loss"].whole == mc.SENTINEL).all()
    c = mc.BY_ID["colsum-bf16-257x300-ld308"]
    t = mc.make_tensors(c)
    assert t.b["ws"].whole.numel() == lib.mit_colsum_ws_floats(257, 300) + 2 * mc.GUARD == 3 * 300 + 2 * mc.GUARD
    c = mc.BY_ID["gnorm-5-max2x"]
    assert mc.make_tensors(c).b["ws"].whole.numel() == lib.mit_grad_norm_ws_floats(5) + 2 * mc.GUARD
    c = mc.BY_ID["embbwd-plan-bf16-128-p0"]
    t = mc.make_tensors(c)
    assert t.b["plan"].whole.numel() == lib.mit_embed_plan_ints(88) + 2 * mc.GUARD
    assert t.b["dtable"].whole.numel() == mc.BWD_VOCAB * 128 + 2 * mc.GUARD and t.b["dx"].whole.numel() == 88 * 128 + 2 * mc.GUARD
    for c in _of("adamw")[:4]:
        t = mc.make_tensors(c)
        assert all(t.b[k].whole.numel() == c.cols + 2 * mc.GUARD for k in ("p", "g", "m", "v")) and (t.row("v") >= 0).all()


# ------------------------------------------------------------------------------------------------
# the harness against FakeOps
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_faultless_fake_passes(case):
    _run_fake(case)


@pytest.mark.parametrize("math", ["seq", "tree"])  # the two forms the bounds were measured under
@pytest.mark.parametrize("case", [c for c in CASES if not c.id.startswith(mc.SLOW_F32)], ids=lambda c: c.id)
def test_float32_fake_is_within_every_bound(case, math):
    """float32 math on the rounded inputs, outputs rounded on the store: on the bf16 cases the bf16 emulation"""
    _run_fake(case, math=math)


def test_every_fault_names_cases_that_exist():
    for f, ids in mc.FAULT_CASE.items():
        assert ids and all(i in mc.BY_ID for i in ids), f
    # launching embed_plan_kernel<4> where <8> is due leaves the upper half of the keys unsorted: only n in 4097..8192 sees it
    assert mc.FAULT_CASE["emb_plan_kpt_half"] == ["embplan-4097", "embplan-8192"]


@pytest.mark.parametrize("fault,cid", [(f, i) for f, ids in mc.FAULT_CASE.items() for i in ids])
def test_injected_fault_is_caught(fault, cid):
    case = mc.BY_ID[cid]
    t, ref = _tensors_and_ref(case)
    with pytest.raises(AssertionError):
        mc.run_case(case, t, mc.FakeOps("f64", fault), ref)
    with pytest.raises(AssertionError):  # ... and in the bf16 emulation / float32
        mc.run_case(case, t, mc.FakeOps("tree", fault), ref)


# ------------------------------------------------------------------------------------------------
# rejections: return codes only, nothing launched
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rid,entry,frag", mc.REJECTIONS, ids=[r[0] for r in mc.REJECTIONS])
def test_rejections(rid, entry, frag):
    lib = native.load_library()
    buf = {k: torch.zeros(4096, dtype=torch.float32) for k in "abcdefgh"}
    p = {k: v.data_ptr() + (-v.data_ptr()) % 16 for k, v in buf.items()}
    a, b, c_, d, e, f_, g, h = (p[k] for k in "abcdefgh")
    BF, F32 = native.BF16, native.F32
    query = None
    if entry == "gnorm":
        rc = lib.mit_grad_norm(a + 4, 8, 1.0, b, c_, None)
    elif entry.startswith("adamw-"):
        off = {k: (4 if entry == "adamw-" + k else 0) for k in ("p", "g", "m", "v")}
        sh = e + (2 if entry == "adamw-shadow" else 0)
        rc = lib.mit_adamw(8, a + off["p"], b + off["g"], c_ + off["m"], d + off["v"], sh, None, f_, g, 0.9, 0.999, 1e-8,
                           0.0, None)
    elif entry == "ce-ld":
        rc = lib.mit_cross_entropy(BF, 4, 512, a, 511, b, -100, c_, d, 1, e, None)
        query = lib.mit_cross_entropy_plan(BF, 4, 512, a, 511, e)
    elif entry == "ce-null":
        rc = lib.mit_cross_entropy(BF, 4, 512, None, 512, b, -100, c_, d, 1, e, None)
        query = lib.mit_cross_entropy_plan(BF, 4, 512, None, 512, e)
    elif entry == "im2col-H":
        rc = lib.mit_im2col(BF, 1, 1, 20, 16, 8, a, b, 64, None)
        query = lib.mit_im2col_plan(BF, 1, 1, 20, 16, 8, a, b, 64)
    elif entry == "im2col-kpad":
        rc = lib.mit_im2col(BF, 1, 1, 16, 16, 8, a, b, 56, None)
        query = lib.mit_im2col_plan(BF, 1, 1, 16, 16, 8, a, b, 56)
    elif entry == "assemble-null":
        rc = lib.mit_vit_assemble(BF, 1, 1, 8, a, None, c_, d, None)
        query = lib.mit_vit_assemble_plan(BF, 1, 1, 8, a, None, c_, d)
    elif entry == "embplan-n":
        rc = lib.mit_embed_plan(a, 16385, b, None)
        query = lib.mit_embed_plan_keys_per_thread(16385)
    elif entry == "embbwd-d":
        rc = lib.mit_embed_bwd(F32, 1, 4, 130, a, b, 1.0, 0.0, None, 0, 0, c_, d, None)
    elif entry == "colsum-ld":
        rc = lib.mit_colsum(F32, 4, 16, a, 15, b, 0, c_, None)
    assert rc == 1, rid  # MIT_ERR_INVALID
    assert frag in lib.mit_last_error(), (rid, lib.mit_last_error())
    assert query is None or query == -1


def test_queries_need_no_gpu_and_dereference_nothing():
    lib = native.load_library()
    # pointers that are never read: only their alignment matters
    assert lib.mit_cross_entropy_plan(native.BF16, 9, 10240, 4096, 10240, 4096) == native.CE_ROWS
    assert lib.mit_cross_entropy_plan(native.BF16, 9, 10241, 4096, 10248, 4096) == native.CE_BLOCK
    assert lib.mit_cross_entropy_plan(native.BF16, 9, 509, 4096, 512, 4096) == native.CE_ROWS
    assert lib.mit_cross_entropy_plan(native.BF16, 9, 509, 4096, 509, 4096) == native.CE_BLOCK
    assert lib.mit_cross_entropy_plan(native.BF16, 9, 512, 4096 + 8, 512, 4096) == native.CE_BLOCK
    assert lib.mit_cross_entropy_plan(native.BF16, 9, 512, 4096, 512, None) == native.CE_BLOCK
    assert lib.mit_cross_entropy_plan(native.F32, 9, 512, 4096, 512, 4096) == native.CE_BLOCK
    assert lib.mit_im2col_plan(native.BF16, 2, 3, 224, 224, 16, 4096, 4096, 768) == native.ELT_VEC8
    assert lib.mit_im2col_plan(native.BF16, 2, 3, 224, 224, 14, 4096, 4096, 592) == native.ELT_SCALAR
    assert lib.mit_vit_assemble_plan(native.BF16, 2, 196, 768, 4096, 4096, 4096, 4096) == native.ELT_VEC8
    assert lib.mit_vit_assemble_plan(native.BF16, 2, 196, 768, 4096, 4096 + 8, 4096, 4096) == native.ELT_SCALAR
    assert [lib.mit_embed_plan_keys_per_thread(n) for n in (-1, 0, 1, 1024, 1025, 4032, 4097, 8192, 8193, 16384, 16385)] == \
        [-1, 0, 1, 1, 2, 4, 8, 8, 16, 16, -1]
    assert [mc.kpt_of(n) for n in (0, 1, 1024, 1025, 4096, 4097, 8192, 8193, 16384)] == [0, 1, 1, 2, 4, 8, 8, 16, 16]
