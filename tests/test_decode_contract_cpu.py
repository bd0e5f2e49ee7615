"""tests/decode_contract.py without a GPU: its float64 references against torch (softmax attention with a
key-padding mask, torch.argmax with NaN, F.layer_norm on the merged statistics, F.linear with ReLU and a residual),
the fault-free FakeOps on every case in float64 and in both float32 orders within BOUND, every injected fault caught
on the cases FAULTS names, pack_key / argmax_of_keys against torch.argmax, and -- with the built library, still no
GPU -- the planned kernel of every case (mit_attention_decode_plan, mit_decode_gemm_plan), the planned LDS bytes
within a gfx950 workgroup's 160 KiB, and one rejected call per MIT_CHECK_ARG of mit_attention_decode and
mit_decode_gemm (synthetic aligned addresses: the queries dereference nothing)."""
import math

import pytest
import torch
import torch.nn.functional as F

import decode_contract as dc
import native

IDS = [c.id for c in dc.CASES]
OPS = {op: [c for c in dc.CASES if c.op == op] for op in {c.op for c in dc.CASES}}


# ------------------------------------------------------------------------------------------------
# the references against torch
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", OPS["attn"][::3], ids=[c.id for c in OPS["attn"][::3]])
def test_reference_attention_is_torch_softmax_attention(case):
    c = case
    if c.B <= 0:
        return
    t = dc.make_tensors(c)
    t.snapshot()
    ref, _ = dc.reference_attn(c, t)
    q, K, V, pad = dc.attn_windows(c, t)
    bias = None
    if pad is not None:
        bias = torch.zeros(pad.shape, dtype=torch.float64).masked_fill(pad, -math.inf)[:, None, None, :]
    o = F.scaled_dot_product_attention(q.double()[:, :, None, :], K.double().permute(0, 2, 1, 3),
                                       V.double().permute(0, 2, 1, 3), attn_mask=bias, scale=t.x["G"]["scale"])
    o = o[:, :, 0, :].reshape(ref.shape)
    # a row whose keys are all PAD: NaN in the reference (softmax of -inf only, as the header says), whatever
    # this torch's fused attention makes of it
    gone = pad.all(1) if pad is not None else torch.zeros(c.B, dtype=torch.bool)
    assert torch.isnan(ref[gone]).all() and not torch.isnan(ref[~gone]).any() and not torch.isnan(o[~gone]).any()
    assert bool(gone.any()) == (c.mask == "row_all")
    ok = ~torch.isnan(ref)
    assert torch.allclose(o[ok], ref[ok], rtol=1e-12, atol=1e-12)


def test_reference_argmax_is_torch_argmax():
    g = torch.Generator().manual_seed(0)
    rows = [torch.randn(37, generator=g) for _ in range(20)]
    for c in (dc.BY_ID["pick-V257-scalar-V%4-nan"], dc.BY_ID["pick-V4096-vec"], dc.BY_ID["pick-V5-scalar-V%4-inf"]):
        rows += list(dc.pick_rows(c, g)[0])
    for r in rows:
        assert dc.ref_argmax(r) == int(torch.argmax(r))
    assert dc.ref_argmax(torch.tensor([-1.0, -0.0, -2.0, 0.0])) == 1
    assert dc.ref_argmax(torch.tensor([-math.inf] * 4)) == 0
    assert dc.ref_argmax(torch.tensor([1.0, 9.0, math.nan, math.inf, math.nan])) == 2


@pytest.mark.parametrize("case", OPS["ln"], ids=[c.id for c in OPS["ln"]])
def test_reference_layernorm_is_layer_norm_of_the_merged_statistics(case):
    c = case
    t = dc.make_tensors(c)
    t.snapshot()
    ref, _ = dc.reference_ln(c, t)
    z = t.a["z"].bwin(0, c.M, c.W, t.x["ldz"]).double()
    want = F.layer_norm(z, (c.W,), t.a["gamma"].base[:c.W].double(), t.a["beta"].base[:c.W].double(), dc.f32r(c.eps))
    # the statistics are float32 roundings of the float64 ones: 2^-24 relative on the mean, amplified by mean / sd
    amp = 1 + float((z.mean(1).abs() / z.std(1).clamp_min(1e-3)).max())
    assert torch.allclose(ref, want, rtol=0, atol=4e-7 * amp * float(want.abs().max()))
    mean, var = dc.merge_stats(dc.host_stats(z), c.W)
    assert torch.allclose(mean, z.mean(1), rtol=1e-13, atol=1e-13)
    assert torch.allclose(var, z.var(1, unbiased=False), rtol=1e-11, atol=1e-13)


_LIN = [c for c in OPS["gemm"] if not c.a_ln and c.r_mode != 2 and c.M > 0][::4]


@pytest.mark.parametrize("case", _LIN, ids=[c.id for c in _LIN])
def test_reference_gemm_is_linear_relu_residual(case):
    c = case
    t = dc.make_tensors(c)
    t.snapshot()
    G = t.x["G"]
    v, _ = dc.reference_gemm(c, t)
    a = t.a["A"].bwin(0, c.M, c.K, G["lda"]).double()
    w = t.a["B"].bwin(0, c.N, c.K, G["ldb"]).double()
    want = F.linear(a, w, t.a["bias"].base[:c.N].double() if c.bias else None)
    if c.act == dc.ACT_RELU:
        want = F.relu(want)
    if c.r_mode == 1:
        want = want + t.a["r"].bwin(0, c.M, c.N, G["ldr"]).double()
    assert torch.allclose(v, want, rtol=1e-12, atol=1e-12)


def test_pack_key_and_argmax_of_keys_agree_with_torch_argmax():
    g = torch.Generator().manual_seed(1)
    v = torch.randn(64, 1088, generator=g)
    v[1] -= 50.0
    v[2, [5, 900]] = math.inf
    v[3, [70, 700]] = math.nan
    v[4] = -math.inf
    v[5] = 2.5
    v[6, 100] = -math.inf
    v[7] = -v[7].abs() - 1
    v[7, 40] = 0.0
    keys = dc.argmax_keys_of(v)
    want = torch.argmax(v, 1)
    assert torch.equal(dc.argmax_of_keys(keys), want)
    assert torch.equal(native.argmax_of_keys(keys.reshape(-1).contiguous(), 64), want)
    # the order of the keys is the order of the values, NaN on top; a smaller column wins among equal values
    x = torch.tensor([-math.inf, -3.0, -1e-30, -0.0, 0.0, 1e-30, 2.0, math.inf, math.nan])
    k = dc.pack_key(x, torch.zeros(9, dtype=torch.int64)) ^ torch.iinfo(torch.int64).min
    assert bool((k[1:] > k[:-1]).all())
    k2 = dc.pack_key(torch.tensor([1.0, 1.0]), torch.tensor([3, 4]))
    assert int(k2[0]) > int(k2[1])
    assert int(dc.pack_key(torch.tensor([1.0]), torch.tensor([7]))[0]) == (0xBF800000 - (1 << 32) << 32) | (0xFFFFFFFF - 7)


# ------------------------------------------------------------------------------------------------
# the fake: clean without faults, every fault caught
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", dc.CASES, ids=IDS)
def test_faultless_fake_passes(case):
    t = dc.make_tensors(case)
    dc.run_case(case, t, dc.FakeOps("f64"), twice=True, show=False)
    figs = dc.run_case(case, dc.make_tensors(case), dc.FakeOps("f64"), show=False)
    assert all(f < 0.51 for _, _, f in figs), figs   # float64 arithmetic: only the float32 rounding of the output is left


_FLOAT = [c for c in dc.CASES if c.op in ("attn", "gemm", "ln", "chain")]


@pytest.mark.parametrize("mode", ["seq", "tree"])
@pytest.mark.parametrize("case", _FLOAT, ids=[c.id for c in _FLOAT])
def test_float32_fake_is_within_every_bound(case, mode):
    dc.run_case(case, dc.make_tensors(case), dc.FakeOps(mode), show=False)


def test_bounds_come_from_the_float32_fake():
    """BOUND is 4 x the worst float32 figure; a host whose exp2 / rsqrt round differently moves that by a little"""
    worst = {}
    for c in _FLOAT:
        for mode in ("seq", "tree"):
            for kind, _, fig in dc.run_case(c, dc.make_tensors(c), dc.FakeOps(mode), show=False):
                worst[kind] = max(worst.get(kind, 0.0), fig)
    assert set(worst) == set(dc.BOUND)
    for kind, w in worst.items():
        assert 0.5 * dc.BOUND[kind] <= 4 * w <= 1.25 * dc.BOUND[kind], (kind, w)


def test_every_fault_names_cases_that_exist():
    for fault, ids in dc.FAULTS.items():
        assert ids, fault
        for i in ids:
            assert i in dc.BY_ID, (fault, i)


_FAULT_CASES = [(f, i) for f, ids in dc.FAULTS.items() for i in ids]


@pytest.mark.parametrize("fault,cid", _FAULT_CASES, ids=[f"{f}@{i}" for f, i in _FAULT_CASES])
def test_injected_fault_is_caught(fault, cid):
    c = dc.BY_ID[cid]
    with pytest.raises(AssertionError):
        dc.run_case(c, dc.make_tensors(c), dc.FakeOps("f64", faults=(fault,)), show=False)


def test_table_reaches_every_path():
    at = OPS["attn"]
    for fam in ("bh", "rows", "rows_nt"):
        for Dh in (16, 32, 64, 128):
            assert any(c.family == fam and c.Dh == Dh for c in at)
    assert any(c.family == "bh" and c.dtype == "bf16" and c.H == 8 and c.Dh == 16 for c in at)   # configs[0]
    assert not any(c.family == "bh" and c.dtype == "bf16" and c.H * c.Dh == 512 for c in at)
    assert any(c.family == "bh" and c.dtype == "f32" and c.H * c.Dh == 512 for c in at)
    lks = {c.Lk for c in at if c.family == "rows" and c.Dh == 64}
    assert {1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 192, 193, 197, 257} <= lks
    assert any(c.family == "rows_nt" and c.mask != "none" and not c.use_pos for c in at)
    pk = OPS["pick"]
    assert {c.V for c in pk} >= {1, 3, 4, 5, 255, 256, 257, 1024, 1028, 4096, 4100, 10000, 10001}
    assert any(dc.pick_is_vector(c) for c in pk)
    assert any(c.V % 4 and not dc.pick_is_vector(c) for c in pk)
    assert any(c.V % 4 == 0 and c.ld_pad == 1 for c in pk) and any(c.V % 4 == 0 and c.mis == 1 for c in pk)
    for c in pk:    # the labels follow the device-side predicate of greedy_pick_kernel
        assert ("-vec" in c.id) == dc.pick_is_vector(c) and ("-scalar" in c.id) != dc.pick_is_vector(c), c.id
    gm = OPS["gemm"]
    combos = {(c.a_ln, c.act, c.r_mode, c.c_f32, dc.expected_gemm_plan(c)[4]) for c in gm}
    for combo in [(False, 0, 0, False), (False, 1, 0, False), (False, 0, 1, False), (False, 0, 2, False)]:
        assert combo + (4,) in combos and combo + (8,) in combos
    for combo in [(True, 0, 0, False), (True, 1, 0, False), (True, 0, 0, True)]:
        assert combo + (8,) in combos
    assert {c.M for c in gm} >= {0, 1, 31, 32, 33, 63, 64, 65}
    assert {c.N for c in gm} >= {8, 56, 64, 72, 136, 1024, 1032}
    assert {c.K for c in gm if not c.a_ln} >= {8, 24, 64, 72, 192, 504, 512, 520, 576, 1024, 1088, 1536, 2048}
    assert any(c.cache and c.a_ln for c in gm) and {c.cache[0] for c in gm if c.cache} == {0, 8, 72, 64}
    assert {c.N for c in OPS["argmax"]} == {7, 509, 1001, 1024, 1088}
    for op in ("kvstore", "embed"):
        assert any(c.B * c.n > dc.GRID_CAP for c in OPS[op])


# ------------------------------------------------------------------------------------------------
# plans: the built library, no GPU
# ------------------------------------------------------------------------------------------------
_PLANNED = [c for c in dc.CASES if c.op in ("attn", "gemm", "argmax")]


@pytest.mark.parametrize("case", _PLANNED, ids=[c.id for c in _PLANNED])
def test_case_plans_onto_its_family(case):
    native.load_library()
    dc.check_plan(case, dc.make_tensors(case), native)


BASE = 0x7F0000000000   # synthetic addresses: 16-B aligned, never dereferenced


def _attn(**kw):
    a = dict(dtype=native.BF16, B=2, H=8, Dh=64, q=BASE, q_batch=1536, k=BASE + 0x10000, k_row=1024, k_batch=65536,
             v=BASE + 0x10400, v_row=1024, v_batch=65536, o=BASE + 0x900000, o_batch=512, Lk=9, pos=BASE + 0xA00000,
             key_tokens=None)
    a.update(kw)
    return native.attention_decode_plan(a["dtype"], a["B"], a["H"], a["Dh"], a["q"], a["q_batch"], a["k"], a["k_row"],
                                        a["k_batch"], a["v"], a["v_row"], a["v_batch"], a["o"], a["o_batch"],
                                        Lk=a["Lk"], pos=a["pos"], key_tokens=a["key_tokens"])


ATTN_REJECTIONS = [
    ("null-q", dict(q=None), b"null pointer"), ("null-k", dict(k=None), b"null pointer"),
    ("null-v", dict(v=None), b"null pointer"), ("null-o", dict(o=None), b"null pointer"),
    ("head-dim-48", dict(Dh=48), b"head_dim"), ("dtype-2", dict(dtype=2), b"bad dtype"),
    ("no-pos-no-lk", dict(pos=None, Lk=0), b"Lk > 0"),
    ("q-misaligned", dict(q=BASE + 8), b"16-B aligned"), ("k-misaligned", dict(k=BASE + 0x10002), b"16-B aligned"),
    ("v-misaligned", dict(v=BASE + 0x10404), b"16-B aligned"), ("o-misaligned", dict(o=BASE + 0x900008), b"16-B aligned"),
    ("q-batch-odd", dict(q_batch=1540), b"16-B aligned"), ("k-row-odd", dict(k_row=1028), b"16-B aligned"),
    ("k-batch-odd", dict(k_batch=65540), b"16-B aligned"), ("v-row-odd", dict(v_row=1026), b"16-B aligned"),
    ("v-batch-odd", dict(v_batch=65537), b"16-B aligned"), ("o-batch-odd", dict(o_batch=516), b"16-B aligned"),
]


def test_attention_plan_base_call_and_families():
    native.load_library()
    assert _attn() == dc.ATTN_ROWS
    assert _attn(pos=None) == dc.ATTN_ROWS_NT
    assert _attn(H=4) == dc.ATTN_BH and _attn(dtype=native.F32) == dc.ATTN_BH
    assert _attn(B=0) == dc.ATTN_ROWS          # planned, though nothing is launched
    assert _attn(q_batch=1536 + 4, dtype=native.F32) == dc.ATTN_BH   # 16 bytes of f32


@pytest.mark.parametrize("rid,change,frag", ATTN_REJECTIONS, ids=[r[0] for r in ATTN_REJECTIONS])
def test_attention_plan_rejections(rid, change, frag):
    lib = native.load_library()
    assert _attn(**change) == -1
    assert frag in lib.mit_last_error()


def _gemm(**kw):
    g = native.DecodeGemmArgs()
    base = dict(M=33, N=136, K=72, A=BASE, lda=80, B=BASE + 0x100000, ldb=80, bias=BASE + 0x200000, act=0, c_f32=0,
                C=BASE + 0x300000, ldc=144, r_mode=0, eps=1e-5)
    base.update(kw)
    for k, v in base.items():
        setattr(g, k, v)
    return g


_LN = dict(a_stats=BASE + 0x400008, a_gamma=BASE + 0x500000, a_beta=BASE + 0x600000)
_R2 = dict(r_mode=2, r=BASE + 0x700000, ldr=136, r_stats=BASE + 0x800008, r_gamma=BASE + 0x900000, r_beta=BASE + 0xA00000)
_KEYS = dict(C=None, argmax_keys=BASE + 0xB00008)
GEMM_REJECTIONS = [
    ("M-negative", dict(M=-1), b"bad extents"), ("N-zero", dict(N=0), b"bad extents"), ("K-zero", dict(K=0), b"bad extents"),
    ("null-A", dict(A=None), b"null operand"), ("null-B", dict(B=None), b"null operand"),
    ("no-output", dict(C=None), b"no output"),
    ("K-not-8", dict(K=76), b"multiples of 8"), ("N-not-8", dict(N=132), b"multiples of 8"),
    ("ldb-not-8", dict(ldb=84), b"multiples of 8"), ("lda-short", dict(lda=64), b"multiples of 8"),
    ("ldb-short", dict(ldb=64), b"multiples of 8"),
    ("act-gelu", dict(act=2), b"act 2 unsupported"), ("r-mode-3", dict(r_mode=3), b"bad r_mode"),
    ("ln-no-gamma", dict(_LN, a_gamma=None), b"LN operand needs"), ("ln-no-beta", dict(_LN, a_beta=None), b"LN operand needs"),
    ("ln-K-1032", dict(_LN, K=1032, lda=1032, ldb=1032), b"LN operand needs"),
    ("ln-lda-not-4", dict(_LN, lda=82), b"LN operand needs"),
    ("bf16-lda-not-8", dict(lda=84), b"lda % 8"),
    ("res-null", dict(r_mode=1), b"bad residual"), ("res-ldr-short", dict(r_mode=1, r=BASE + 0x700000, ldr=128), b"bad residual"),
    ("res-ldr-not-8", dict(r_mode=1, r=BASE + 0x700000, ldr=140), b"bad residual"),
    ("lnres-no-stats", dict(_R2, r_stats=None), b"LN residual needs"), ("lnres-no-gamma", dict(_R2, r_gamma=None), b"LN residual needs"),
    ("lnres-no-beta", dict(_R2, r_beta=None), b"LN residual needs"),
    ("lnres-N-1032", dict(_R2, N=1032, ldr=1032, ldc=1032), b"LN residual needs"),
    ("ldc-short", dict(ldc=128), b"bad ldc"), ("ldc-not-8", dict(ldc=140), b"bad ldc"),
    ("ldz-short", dict(z_out=BASE + 0xC00000, ldz=128), b"bad ldz"), ("ldz-not-8", dict(z_out=BASE + 0xC00000, ldz=140), b"bad ldz"),
    ("cache-no-pos", dict(cache=BASE + 0xD00000, c_row=136, c_batch=1360), b"cache needs pos"),
    ("cache-kv0-not-8", dict(cache=BASE + 0xD00000, pos=BASE + 0xE00000, c_row=136, c_batch=1360, kv_col0=4), b"cache needs pos"),
    ("cache-row-not-8", dict(cache=BASE + 0xD00000, pos=BASE + 0xE00000, c_row=132, c_batch=1360), b"cache needs pos"),
    ("cache-batch-not-8", dict(cache=BASE + 0xD00000, pos=BASE + 0xE00000, c_row=136, c_batch=1364), b"cache needs pos"),
    ("stats-without-z", dict(stats_out=BASE + 0xF00000), b"stats_out needs z_out"),
    ("B-span-2GiB", dict(N=1 << 20, ldb=1 << 10, K=1 << 10, lda=1 << 10, ldc=1 << 20), b">= 2 GiB"),
    ("A-span-2GiB", dict(M=1 << 21, lda=1 << 10, K=1 << 10, ldb=1 << 10), b">= 2 GiB"),
    ("A-misaligned", dict(A=BASE + 8), b"16-B aligned"), ("B-misaligned", dict(B=BASE + 0x100002), b"16-B aligned"),
    ("C-misaligned", dict(C=BASE + 0x300004), b"16-B aligned"), ("z-misaligned", dict(z_out=BASE + 0xC00008, ldz=136), b"16-B aligned"),
    ("r-misaligned", dict(r_mode=1, r=BASE + 0x700008, ldr=136), b"16-B aligned"),
    ("cache-misaligned", dict(cache=BASE + 0xD00008, pos=BASE + 0xE00000, c_row=136, c_batch=1360), b"16-B aligned"),
    ("a-gamma-misaligned", dict(_LN, a_gamma=BASE + 0x500004), b"16-B aligned"),
    ("a-beta-misaligned", dict(_LN, a_beta=BASE + 0x600004), b"16-B aligned"),
    ("r-gamma-misaligned", dict(_R2, r_gamma=BASE + 0x900004), b"16-B aligned"),
    ("r-beta-misaligned", dict(_R2, r_beta=BASE + 0xA00004), b"16-B aligned"),
    ("keys-with-ln", dict(_KEYS, **_LN), b"argmax_keys needs"), ("keys-with-relu", dict(_KEYS, act=1), b"argmax_keys needs"),
    ("keys-with-residual", dict(_KEYS, r_mode=1, r=BASE + 0x700000, ldr=136), b"argmax_keys needs"),
    ("keys-with-C", dict(argmax_keys=BASE + 0xB00008), b"argmax_keys needs"),
    ("keys-with-z", dict(_KEYS, z_out=BASE + 0xC00000, ldz=136), b"argmax_keys needs"),
    ("keys-with-cache", dict(_KEYS, cache=BASE + 0xD00000, pos=BASE + 0xE00000, c_row=136, c_batch=1360), b"argmax_keys needs"),
    ("keys-misaligned", dict(_KEYS, argmax_keys=BASE + 0xB00004), b"argmax_keys needs"),
    ("f32-C-without-ln", dict(c_f32=1), b"f32 C only"), ("f32-C-relu", dict(_LN, c_f32=1, act=1), b"f32 C only"),
    ("f32-C-residual", dict(_LN, c_f32=1, r_mode=1, r=BASE + 0x700000, ldr=136), b"f32 C only"),
    ("ln-with-residual", dict(_LN, r_mode=1, r=BASE + 0x700000, ldr=136), b"LN operand with a residual"),
    ("relu-with-residual", dict(act=1, r_mode=1, r=BASE + 0x700000, ldr=136), b"ReLU with a residual"),
]


def test_gemm_plan_base_calls():
    native.load_library()
    p = native.decode_gemm_plan(_gemm())
    assert dc.plan_tuple(p) == (0, 0, 0, 0, 4, 64, 3, 4 * 64 * 68 * 4)
    p = native.decode_gemm_plan(_gemm(**_LN))
    assert dc.plan_tuple(p) == (1, 0, 0, 0, 8, 32, 2 * 3, 8 * 32 * 68 * 4)
    p = native.decode_gemm_plan(_gemm(**_LN, K=1024, lda=1024, ldb=1024))
    assert p.lds_bytes == max(32 * (2048 + 16), 8 * 32 * 68 * 4) <= dc.LDS_LIMIT
    p = native.decode_gemm_plan(_gemm(**_R2))
    assert (p.r_mode, p.waves) == (2, 4)
    p = native.decode_gemm_plan(_gemm(**_KEYS, N=1001, K=2048, lda=2048, ldb=2048))
    assert dc.plan_tuple(p)[:6] == (0, 0, 3, 0, 4, 64) and p.grid == 16
    assert native.decode_gemm_plan(_gemm(**_KEYS, c_f32=1)).c_f32 == 0   # the argmax head has no C to widen
    assert native.decode_gemm_plan(_gemm(M=0)).grid == 0
    assert native.lib().mit_decode_gemm_plan(None, None) == -1


@pytest.mark.parametrize("rid,change,frag", GEMM_REJECTIONS, ids=[r[0] for r in GEMM_REJECTIONS])
def test_gemm_plan_rejections(rid, change, frag):
    lib = native.load_library()
    assert native.decode_gemm_plan(_gemm(**change)) is None
    assert frag in lib.mit_last_error(), lib.mit_last_error()
