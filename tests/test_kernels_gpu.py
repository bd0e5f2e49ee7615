"""Per-kernel numerics of libmit_hip.so against plain-PyTorch fp32 references (GPU only).

Tolerances: fp32 kernels ~1e-4 relative; bf16 kernels are compared with the SAME bf16-rounded
inputs fed to an fp32 reference, tolerance ~1e-2 of the output scale (bf16 output rounding).
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

N = None


@pytest.fixture(scope="module", autouse=True)
def _native():
    global N
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import native
    native.load_library()
    N = native
    torch.manual_seed(0)


def dev():
    return torch.device("cuda")


def _ref_mat(x, layout, rows, cols):
    """logical [rows, cols] operand from storage (K_CONTIG: stored [rows][cols]; MN: stored [cols][rows])."""
    return x.float() if layout == 0 else x.float().t()


def _close(got, ref, tol):
    # floor: a mathematically-zero reference (e.g. dQ when softmax is over one key) holds only noise
    scale = max(ref.abs().max().item(), 1e-3)
    err = (got.float() - ref).abs().max().item()
    assert err <= tol * scale, f"max err {err:.3e} vs scale {scale:.3e} (tol {tol})"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("al,bl", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("M,Nn,K", [(296, 200, 136), (128, 128, 64), (8, 8, 8), (256, 520, 1000), (72, 64, 124)])
def test_gemm_layouts(dtype, al, bl, M, Nn, K):
    if dtype == torch.bfloat16 and K % 8 and (al == 0 or bl == 0):
        pytest.skip("bf16 K-contiguous operands need K % 8 == 0 (host-checked)")
    A = torch.randn(M, K, device=dev()) if al == 0 else torch.randn(K, M, device=dev())
    B = torch.randn(Nn, K, device=dev()) if bl == 0 else torch.randn(K, Nn, device=dev())
    A, B = A.to(dtype), B.to(dtype)
    C = torch.empty(M, Nn, device=dev(), dtype=dtype)
    N.gemm(A, B, C, M, Nn, K, a_layout=al, b_layout=bl)
    Am = A.float() if al == 0 else A.float().t()
    Bm = B.float().t() if bl == 0 else B.float()
    ref = Am @ Bm
    _close(C, ref, 1e-2 if dtype == torch.bfloat16 else 1e-5)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_gemm_epilogues(dtype):
    M, Nn, K = 200, 136, 96
    x = torch.randn(M, K, device=dev()).to(dtype)
    w = torch.randn(Nn, K, device=dev()).to(dtype) / 10
    bias = torch.randn(Nn, device=dev())
    res = torch.randn(M, Nn, device=dev()).to(dtype)
    base = x.float() @ w.float().t()
    tol = 1e-2 if dtype == torch.bfloat16 else 1e-5
    for act, fn in [(N.ACT_RELU, F.relu), (N.ACT_GELU, F.gelu), (N.ACT_QUICK_GELU, lambda t: t * torch.sigmoid(1.702 * t))]:
        out = torch.empty(M, Nn, device=dev(), dtype=dtype)
        N.linear(x, w, out, bias=bias, act=act)
        _close(out, fn(base + bias), tol)
    out = torch.empty(M, Nn, device=dev(), dtype=dtype)
    N.linear(x, w, out, bias=bias, residual=res)
    _close(out, base + bias + res.float(), tol)
    # f32 output + accumulate + alpha
    acc = torch.randn(M, Nn, device=dev())
    ref = acc + 0.5 * base
    N.gemm(x, w, acc, M, Nn, K, alpha=0.5, accumulate=True)
    _close(acc, ref, tol)
    # aux mask (relu backward): out = base * (aux > 0) * 1.25
    aux = torch.randn(M, Nn, device=dev()).to(dtype)
    out = torch.empty(M, Nn, device=dev(), dtype=dtype)
    N.gemm(x, w, out, M, Nn, K, aux=aux, aux_scale=1.25)
    _close(out, base * (aux.float() > 0) * 1.25, tol)


def test_gemm_rejects_bad_shapes():
    A = torch.randn(300, 64, device=dev()).to(torch.bfloat16)
    B = torch.randn(64, 64, device=dev()).to(torch.bfloat16)
    C = torch.empty(300, 64, device=dev(), dtype=torch.bfloat16)
    with pytest.raises(N.NativeError, match="multiple"):
        N.gemm(A, B, C, 300, 64, 64, a_layout=N.MN_CONTIG, lda=300)  # M=300 not a multiple of 8


def test_dropout_mask_and_gemm_dropout():
    seed = torch.tensor([1234], dtype=torch.int64, device=dev())
    n = 1 << 20
    m = torch.empty(n, device=dev())
    N.dropout_mask(n, 0.1, seed, 7, m)
    keep = (m > 0).float().mean().item()
    assert abs(keep - 0.9) < 0.003
    assert torch.allclose(m[m > 0], torch.full_like(m[m > 0], 1 / 0.9))
    m2 = torch.empty(n, device=dev())
    N.dropout_mask(n, 0.1, seed, 8, m2)
    assert (m != m2).float().mean().item() > 0.1  # sites decorrelated
    # GEMM epilogue dropout == relu(xW^T+b) * mask(site, r*N+c)
    M, Nn, K = 64, 96, 32
    x = torch.randn(M, K, device=dev())
    w = torch.randn(Nn, K, device=dev())
    b = torch.randn(Nn, device=dev())
    out = torch.empty(M, Nn, device=dev())
    N.linear(x, w, out, bias=b, act=N.ACT_RELU, drop_p=0.1, seed=seed, site=3)
    mk = torch.empty(M * Nn, device=dev())
    N.dropout_mask(M * Nn, 0.1, seed, 3, mk)
    ref = F.relu(x @ w.t() + b) * mk.view(M, Nn)
    _close(out, ref, 1e-5)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("cols", [128, 192, 200, 130, 256, 512, 768, 1024])
def test_layernorm_fwd_bwd(dtype, cols):
    rows = 200
    x = torch.randn(rows, cols, device=dev()).to(dtype)
    r = torch.randn(rows, cols, device=dev()).to(dtype)
    g = 1 + 0.1 * torch.randn(cols, device=dev())
    bta = 0.1 * torch.randn(cols, device=dev())
    y = torch.empty_like(x)
    z = torch.empty_like(x)
    mean = torch.empty(rows, device=dev())
    rstd = torch.empty(rows, device=dev())
    N.layernorm_fwd(x, g, bta, 1e-5, y, r=r, z=z, mean=mean, rstd=rstd)
    zr = (x.float() + r.float()).requires_grad_(True)
    gr = g.clone().requires_grad_(True)
    br = bta.clone().requires_grad_(True)
    yr = F.layer_norm(zr, (cols,), gr, br, 1e-5)
    tol = 2e-2 if dtype == torch.bfloat16 else 1e-5
    _close(y, yr, tol)
    dy = torch.randn(rows, cols, device=dev()).to(dtype)
    yr.backward(dy.float())
    dx = torch.empty_like(x)
    dr = torch.empty_like(x)
    dg = torch.zeros(cols, device=dev())
    db = torch.zeros(cols, device=dev())
    ws = torch.empty(N.layernorm_bwd_ws_floats(rows, cols), device=dev())
    N.layernorm_bwd(dy, z, mean, rstd, g, dx, dg, db, ws, dr=dr)
    _close(dx, zr.grad, 3e-2 if dtype == torch.bfloat16 else 1e-4)
    _close(dr, zr.grad, 3e-2 if dtype == torch.bfloat16 else 1e-4)
    _close(dg, gr.grad, 2e-2 if dtype == torch.bfloat16 else 1e-4)
    _close(db, br.grad, 2e-2 if dtype == torch.bfloat16 else 1e-4)
    # deferred parameter reduction (partials left in ws, reduced later): identical results
    dx2, dg2, db2 = torch.empty_like(x), torch.zeros(cols, device=dev()), torch.zeros(cols, device=dev())
    ws2 = torch.empty_like(ws)
    N.layernorm_bwd(dy, z, mean, rstd, g, dx2, None, None, ws2)
    N.layernorm_param_grads(rows, cols, ws2, dg2, db2)
    assert torch.equal(dx2, dx) and torch.equal(dg2, dg) and torch.equal(db2, db)


@pytest.mark.parametrize("cols", [256, 768])
@pytest.mark.parametrize("rows", [1, 3, 201, 12608])
@pytest.mark.parametrize("res", [False, True])
def test_layernorm_fwd_two_rows_per_wave(cols, rows, res):
    """bf16 widths 256 / 768 run two rows per wave (ln_fwd_pair_kernel): odd row counts (the last
    wave's second row out of range), statistics, residual with dropout, z written."""
    x = torch.randn(rows, cols, device=dev()).to(torch.bfloat16)
    g = 1 + 0.1 * torch.randn(cols, device=dev())
    bta = 0.1 * torch.randn(cols, device=dev())
    y = torch.empty_like(x)
    mean, rstd = torch.empty(rows, device=dev()), torch.empty(rows, device=dev())
    zr = x.float()
    kw = {}
    if res:
        r = torch.randn(rows, cols, device=dev()).to(torch.bfloat16)
        seed = torch.tensor([11], dtype=torch.int64, device=dev())
        z = torch.empty_like(x)
        kw = dict(r=r, drop_p=0.1, seed=seed, site=5, z=z)
        mk = torch.empty(rows * cols, device=dev())
        N.dropout_mask(rows * cols, 0.1, seed, 5, mk)
        zr = zr + r.float() * mk.view(rows, cols)
    N.layernorm_fwd(x, g, bta, 1e-5, y, mean=mean, rstd=rstd, **kw)
    yr = F.layer_norm(zr, (cols,), g, bta, 1e-5)
    _close(y, yr, 2e-2)
    _close(mean, zr.mean(-1), 1e-5)
    _close(rstd, torch.rsqrt(zr.var(-1, unbiased=False) + 1e-5), 1e-4)
    if res:
        _close(kw["z"], zr, 1e-2)


def _attn_ref(q, k, v, causal, kpm, scale, drop=None):
    # q [B,H,Lq,D]
    s = (q @ k.transpose(-1, -2)) * scale
    Lq, Lk = s.shape[-2:]
    if causal:
        s = s + torch.triu(torch.full((Lq, Lk), float("-inf"), device=s.device), diagonal=1)
    if kpm is not None:
        s = s.masked_fill(kpm[:, None, None, :], float("-inf"))
    p = torch.softmax(s, -1)
    lse = torch.logsumexp(s, -1)
    if drop is not None:
        p = p * drop
    return p @ v, lse


_HD_CASES = [(64, k) for k in ["self_causal_pad", "cross", "bidir", "cross_s1", "self_drop", "self_long", "cross577",
                                "cross_drop", "bidir577", "bidir150", "cross230", "cross_drop40", "cross256", "cross_drop17",
                                "cross_q20", "cross_q20_drop"]]
# other head dims (generic kernels): configs[0]'s decoder is d128 / 8 heads = head_dim 16
_HD_CASES += [(hd, k) for hd in (16, 32, 128) for k in ["self_causal_pad", "cross", "self_drop", "cross_s1"]]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("D,kind", _HD_CASES)
def test_attention_fwd_bwd(dtype, D, kind):
    B, H = 3, 4
    if kind == "self_causal_pad" or kind == "self_drop":
        Lq = Lk = 63
    elif kind in ("cross", "cross_drop"):
        Lq, Lk = 63, 197
    elif kind == "bidir577":
        Lq = Lk = 577  # CLIP-L/14@336 encoder MHSA: 37 query tiles over 3 rounds of waves
    elif kind == "cross_s1":
        Lq, Lk = 31, 1
    elif kind == "self_long":
        Lq = Lk = 130  # several query and key tiles, causal tile skipping
    elif kind == "cross577":
        Lq, Lk = 63, 577  # CLIP-L/14@336 patch memory
    # the head-resident kernel's key tail (K/V staged to 16-row multiples): 2 / 3 tiles after full chunks,
    # 3 tiles and no full chunk (with dropout)
    elif kind == "bidir150":
        Lq = Lk = 150
    elif kind == "cross230":
        Lq, Lk = 63, 230
    elif kind == "cross_drop40":
        Lq, Lk = 63, 40
    # attn_fwd_head with whole 64-key chunks only (256 keys, no tail); 17 keys: no whole chunk, a 32-row tail, with dropout
    elif kind == "cross256":
        Lq, Lk = 50, 256
    elif kind == "cross_drop17":
        Lq, Lk = 63, 17
    # two query tiles (two waves), each sweeping 4 chunks + a 48-key tail (attn_fwd_head has no key split: a wave
    # owns its query tile's whole key range)
    elif kind in ("cross_q20", "cross_q20_drop"):
        Lq, Lk = 20, 300
    else:
        Lq = Lk = 197
    causal = kind.startswith("self")
    drop_p = 0.1 if kind in ("self_drop", "cross_drop", "cross_drop40", "cross_drop17", "cross_q20_drop") else 0.0
    q = torch.randn(B, Lq, H * D, device=dev()).to(dtype)
    kv = torch.randn(B, Lk, 2 * H * D, device=dev()).to(dtype)
    k, v = kv[..., :H * D], kv[..., H * D:]
    tok = None
    kpm = None
    if causal:
        tok = torch.randint(4, 100, (B, Lk), device=dev())
        tok[1, 40:] = 0
        tok[2, 10:] = 0
        kpm = tok == 0
    o = torch.empty(B, Lq, H * D, device=dev(), dtype=dtype)
    lse = torch.empty(B * H * Lq, device=dev())
    seed = torch.tensor([99], dtype=torch.int64, device=dev())
    args = N.attn_args(q, H * D, Lq * H * D, k, 2 * H * D, Lk * 2 * H * D, v, 2 * H * D, Lk * 2 * H * D, o, H * D,
                       Lq * H * D, lse=lse, key_tokens=tok, tok_batch=Lk, pad_idx=0, causal=causal,
                       scale=D ** -0.5, drop_p=drop_p, seed=seed, site=5)
    N.attention_fwd(N.dtype_code(q), B, H, Lq, Lk, args, Dh=D)
    qh = q.float().view(B, Lq, H, D).transpose(1, 2).requires_grad_(True)
    kh = k.float().reshape(B, Lk, H, D).transpose(1, 2).requires_grad_(True)
    vh = v.float().reshape(B, Lk, H, D).transpose(1, 2).requires_grad_(True)
    drop = None
    if drop_p > 0:
        mk = torch.empty(B * H * Lq * Lk, device=dev())
        N.dropout_mask(mk.numel(), drop_p, seed, 5, mk)
        drop = mk.view(B, H, Lq, Lk)
    oref, lref = _attn_ref(qh, kh, vh, causal, kpm, D ** -0.5, drop)
    tol = 2e-2 if dtype == torch.bfloat16 else 1e-4
    _close(o.view(B, Lq, H, D).transpose(1, 2), oref, tol)
    _close(lse.view(B, H, Lq), lref, 1e-3 if dtype == torch.bfloat16 else 1e-5)
    do = torch.randn(B, Lq, H * D, device=dev()).to(dtype)
    oref.backward(do.float().view(B, Lq, H, D).transpose(1, 2))
    dq = torch.empty_like(q)
    dkv = torch.empty_like(kv)
    delta = torch.empty(B * H * Lq, device=dev())
    grads = N.attn_grads(do, H * D, Lq * H * D, dq, H * D, Lq * H * D, dkv[..., :H * D], 2 * H * D, Lk * 2 * H * D,
                         dkv[..., H * D:], 2 * H * D, Lk * 2 * H * D, delta)
    N.attention_bwd(N.dtype_code(q), B, H, Lq, Lk, args, grads, Dh=D)
    gt = 4e-2 if dtype == torch.bfloat16 else 2e-4
    _close(dq.view(B, Lq, H, D).transpose(1, 2), qh.grad, gt)
    _close(dkv[..., :H * D].reshape(B, Lk, H, D).transpose(1, 2), kh.grad, gt)
    _close(dkv[..., H * D:].reshape(B, Lk, H, D).transpose(1, 2), vh.grad, gt)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_embed_ce_colsum(dtype):
    B, T, d, V = 4, 31, 128, 500
    tok = torch.randint(1, V, (B, T), device=dev())
    tok[1, 20:] = 0
    table = torch.randn(V, d, device=dev())
    pe = torch.randn(100, d, device=dev())
    out = torch.empty(B, T, d, device=dev(), dtype=dtype)
    N.embed_fwd(tok, table.to(dtype), math.sqrt(d), pe, out)
    ref = table.to(dtype).float()[tok] * math.sqrt(d) + pe[:T]
    _close(out, ref, 1e-2 if dtype == torch.bfloat16 else 1e-6)
    dx = torch.randn(B, T, d, device=dev()).to(dtype)
    dtab = torch.zeros(V, d, device=dev())
    N.embed_bwd(tok, dx, math.sqrt(d), dtab, 0)
    tr = table.clone().requires_grad_(True)
    (F.embedding(tok, tr, padding_idx=0) * math.sqrt(d)).backward(dx.float())
    _close(dtab, tr.grad, 1e-5)
    # deterministic (planned) path: same values, bit-identical on every repeat, also with repeated
    # tokens (a frequent word), dropout and d = 768
    for dd, p in ((d, 0.0), (768, 0.1)):
        tk = tok.clone()
        tk[0, ::3] = 7
        tk[2, 5:15] = 7
        dxx = torch.randn(B, T, dd, device=dev()).to(dtype)
        plan = torch.empty(N.embed_plan_ints(tk.numel()), dtype=torch.int32, device=dev())
        N.embed_plan(tk, plan)
        seed = torch.tensor([5], dtype=torch.int64, device=dev())
        outs = []
        for _ in range(3):
            dt = torch.zeros(V, dd, device=dev())
            N.embed_bwd(tk, dxx, 2.0, dt, 0, drop_p=p, seed=seed, site=4000, plan=plan)
            outs.append(dt)
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
        mk = torch.ones(B * T * dd, device=dev())
        if p > 0:
            N.dropout_mask(mk.numel(), p, seed, 4000, mk)
        tr = torch.zeros(V, dd, device=dev(), requires_grad=True)
        (F.embedding(tk, tr, padding_idx=0) * 2.0).backward(dxx.float() * mk.view(B, T, dd))
        _close(outs[0], tr.grad, 1e-5)
    # cross entropy with ignore
    rows = 300
    logits = torch.randn(rows, V, device=dev()).to(dtype)
    tgt = torch.randint(0, V, (rows,), device=dev())
    tgt[::7] = 0
    cnt = torch.zeros(1, device=dev())
    N.count_targets(tgt, 0, cnt)
    assert cnt.item() == (tgt != 0).sum().item()
    ls = torch.zeros(1, device=dev())
    lr = logits.float().clone().requires_grad_(True)
    ref = F.cross_entropy(lr, tgt, ignore_index=0)
    ref.backward()
    g = logits.clone()
    N.cross_entropy(g, tgt, 0, cnt, ls, True)
    mean = torch.empty(1, device=dev())
    N.scalar_div(ls, cnt, mean)
    assert abs(mean.item() - ref.item()) < 1e-4 * abs(ref.item()) + 1e-5
    assert abs(ls.item() / cnt.item() - ref.item()) < 1e-4 * abs(ref.item()) + 1e-5
    _close(g, lr.grad, 1e-2 if dtype == torch.bfloat16 else 1e-5)
    # colsum
    M, Nn = 1000, 300
    y = torch.randn(M, Nn, device=dev()).to(dtype)
    o = torch.empty(Nn, device=dev())
    ws = torch.empty(N.colsum_ws_floats(M, Nn), device=dev())
    N.colsum(y, M, Nn, o, ws)
    _close(o, y.float().sum(0), 1e-5)


def test_grad_norm_adamw_matches_torch():
    n = 100003
    p = torch.randn(n, device=dev())
    g = torch.randn(n, device=dev()) * 0.01
    m = torch.zeros(n, device=dev())
    v = torch.zeros(n, device=dev())
    sh = torch.empty(n, device=dev(), dtype=torch.bfloat16)
    ws = torch.empty(N.grad_norm_ws_floats(n), device=dev())
    norm = torch.empty(2, device=dev())
    lr = torch.tensor([1e-3], device=dev())
    step = torch.zeros(1, dtype=torch.int64, device=dev())
    pr = p.clone().requires_grad_(True)
    opt = torch.optim.AdamW([pr], lr=1e-3, betas=(0.9, 0.98), eps=1e-9, weight_decay=1e-5)
    for it in range(3):
        gg = g * (it + 1) * 100  # large -> clipping active
        pr.grad = gg.clone()
        tn = torch.nn.utils.clip_grad_norm_([pr], 5.0)
        opt.step()
        N.grad_norm(gg, 5.0, ws, norm)
        N.step_inc(step)
        N.adamw(p, gg, m, v, sh, norm, lr, step, 0.9, 0.98, 1e-9, 1e-5)
        assert abs(norm[0].item() - tn.item()) < 1e-4 * tn.item()
    torch.testing.assert_close(p, pr.detach(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(sh.float(), p, rtol=1e-2, atol=1e-2)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_im2col_patch_embed(dtype):
    B, C, Hh, P, E = 2, 3, 224, 16, 96
    img = torch.randn(B, C, Hh, Hh, device=dev())
    w = torch.randn(E, C, P, P, device=dev()) / 20
    b = torch.randn(E, device=dev())
    npch = (Hh // P) ** 2
    kpad = C * P * P
    cols = torch.empty(B * npch, kpad, device=dev(), dtype=dtype)
    N.im2col(img, cols, P, kpad)
    out = torch.empty(B * npch, E, device=dev(), dtype=dtype)
    wf = w.reshape(E, -1).to(dtype).contiguous()
    N.linear(cols, wf, out, bias=b)
    cls = torch.randn(E, device=dev())
    pos = torch.randn(npch + 1, E, device=dev())
    h = torch.empty(B, npch + 1, E, device=dev(), dtype=dtype)
    N.vit_assemble(out, cls, pos, h, B, npch, E)
    ref = F.conv2d(img.to(dtype).float(), w.to(dtype).float(), b, stride=P).flatten(2).transpose(1, 2)
    ref = torch.cat([cls.view(1, 1, E).expand(B, 1, E), ref], 1) + pos
    _close(h, ref, 2e-2 if dtype == torch.bfloat16 else 1e-4)


@pytest.mark.parametrize("V", [1000, 10000, 10240, 12000])
@pytest.mark.parametrize("want_grad", [True, False])
def test_cross_entropy_row_kernel(V, want_grad):
    """bf16 CE with the row_loss scratch: the register-resident one-wave-per-row kernel (V <= 10240)
    or the generic one (V = 12000), against torch F.cross_entropy(ignore_index=0) in fp32; the loss
    sum is row-ordered, so repeats are bit-identical."""
    rows = 1003
    g0 = torch.Generator().manual_seed(V)
    logits = (3 * torch.randn(rows, V, generator=g0)).to(dev(), torch.bfloat16)
    tgt = torch.randint(1, V, (rows,), generator=g0).to(dev())
    tgt[::5] = 0
    cnt = torch.zeros(1, device=dev())
    N.count_targets(tgt, 0, cnt)
    lr = logits.float().clone().requires_grad_(True)
    ref = F.cross_entropy(lr, tgt, ignore_index=0)
    ref.backward()
    outs = []
    for _ in range(2):
        g = logits.clone()
        ls = torch.zeros(1, device=dev())
        N.cross_entropy(g, tgt, 0, cnt, ls, want_grad, row_loss=torch.empty(rows, device=dev()))
        outs.append((g, ls))
    assert torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][0], outs[1][0])
    g, ls = outs[0]
    assert abs(ls.item() / cnt.item() - ref.item()) < 1e-4 * abs(ref.item()) + 1e-5
    if want_grad:
        _close(g, lr.grad, 1e-2)
        assert torch.count_nonzero(g[::5]).item() == 0  # ignored rows
    else:
        assert torch.equal(g, logits)


@pytest.mark.parametrize("R,kind", [(4032, "layer"), (520, "layer"), (3000, "tail"), (2048, "one")])
def test_gemm_grouped_weight_gradients_match_single_launches(R, kind):
    """mit_gemm_grouped (a decoder layer's six dW = dY^T X + bias row sums in one launch, split-K chosen
    for the group; the tiles dealt to the XCDs in per-problem runs) against float64 torch, and against
    the one-GEMM-per-problem launches. "tail": the cross-K/V + projection pair (split-K 2 on both);
    "one": a single problem with split-K 10."""
    dev = torch.device("cuda")
    d, F = 512, 2048
    g = torch.Generator().manual_seed(R)
    shapes = {"layer": [(d, F), (F, d), (d, d), (d, d), (d, d), (3 * d, d)],  # (M = out features, N = in)
              "tail": [(6 * d, d), (d, 768)], "one": [(d, 768)]}[kind]
    probs, refs = [], []
    for M, Nn in shapes:
        A = torch.randn(R, M, generator=g).to(dev, torch.bfloat16)
        B = torch.randn(R, Nn, generator=g).to(dev, torch.bfloat16)
        C = torch.full((M, Nn), float("nan"), device=dev)
        rs = torch.full((M,), float("nan"), device=dev)
        probs.append((A, B, C, M, Nn, R, M, Nn, rs))
        refs.append((A.double().cpu().t() @ B.double().cpu(), A.double().cpu().sum(0)))
    ws = torch.empty((N.gemm_grouped_ws_bytes(probs) + 255) // 4, device=dev)
    N.gemm_grouped(probs, ws)
    for (A, B, C, M, Nn, K, lda, ldb, rs), (rc, rr) in zip(probs, refs):
        assert (C.double().cpu() - rc).abs().max().item() < 1e-3 * rc.abs().max().item()
        assert (rs.double().cpu() - rr).abs().max().item() < 1e-3 * max(1.0, rr.abs().max().item())
        C1 = torch.empty_like(C)
        rs1 = torch.empty_like(rs)
        N.gemm(A, B, C1, M, Nn, K, a_layout=N.MN_CONTIG, b_layout=N.MN_CONTIG, lda=lda, ldb=ldb, rowsum=rs1,
               workspace=N.gemm_workspace(M, Nn, K, dev))
        assert torch.allclose(C, C1, rtol=1e-5, atol=1e-3) and torch.allclose(rs, rs1, rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize("M,Nn,K,layout", [(4032, 512, 2048, "nt"), (4032, 512, 1536, "nn"), (520, 512, 2048, "nn")])
def test_gemm_split_k_bias_residual(M, Nn, K, layout):
    """The decoder's long-K N = 512 GEMMs (fc2 forward: bias; the fc1 / self_in data gradients: a residual
    accumulated in place, output aliasing it) against float64 torch, with and without a split-K workspace
    (a bias / residual epilogue keeps them in one launch: DESIGN.md §4.1f)."""
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(K + M)
    A = torch.randn(M, K, generator=g).to(dev, torch.bfloat16)
    bl = N.K_CONTIG if layout == "nt" else N.MN_CONTIG
    B = (torch.randn(Nn, K, generator=g) if layout == "nt" else torch.randn(K, Nn, generator=g)).to(dev, torch.bfloat16)
    bias = torch.randn(Nn, generator=g).to(dev)
    R0 = torch.randn(M, Nn, generator=g).to(dev, torch.bfloat16)
    Bt = B.double().cpu() if layout == "nt" else B.double().cpu().t()
    ref = A.double().cpu() @ Bt.t() + bias.double().cpu() + R0.double().cpu()
    ws = N.gemm_workspace(M, Nn, K, dev)
    outs = []
    for w in (ws, None):
        C = R0.clone()  # residual aliases the output (dx += ...)
        N.gemm(A, B, C, M, Nn, K, b_layout=bl, bias=bias, residual=C, workspace=w)
        outs.append(C)
        assert (C.double().cpu() - ref).abs().max().item() < 2e-2 * ref.abs().max().item()
    assert ((outs[0].float() - outs[1].float()).norm() / outs[1].float().norm()).item() < 5e-3


def test_gemm_grouped_rejects_unsupported():
    dev = torch.device("cuda")
    A = torch.zeros(64, 64, device=dev, dtype=torch.bfloat16)
    C = torch.zeros(64, 64, device=dev, dtype=torch.bfloat16)  # bf16 output: not a weight gradient
    with pytest.raises(N.NativeError):
        N.gemm_grouped([(A, A, C, 64, 64, 64, 64, 64, None)], torch.empty(1024, device=dev))


def test_gemm_grouped_folds_layernorm_param_grads():
    """LayerNorm dgamma/dbeta jobs riding in the grouped launch equal mit_layernorm_param_grads bit for
    bit (same per-column summation order)."""
    dev = torch.device("cuda")
    R, d = 4032, 512
    g = torch.Generator().manual_seed(5)
    A = torch.randn(R, d, generator=g).to(dev, torch.bfloat16)
    B = torch.randn(R, d, generator=g).to(dev, torch.bfloat16)
    C = torch.empty(d, d, device=dev)
    jobs, want = [], []
    for k in range(3):
        z = torch.randn(R, d, generator=g).to(dev, torch.bfloat16)
        dy = torch.randn(R, d, generator=g).to(dev, torch.bfloat16)
        zf = z.float()
        mean = zf.mean(-1)
        rstd = torch.rsqrt(zf.var(-1, unbiased=False) + 1e-5)
        gamma = torch.randn(d, generator=g).to(dev)
        ws = torch.empty(N.layernorm_bwd_ws_floats(R, d), device=dev)
        dx = torch.empty_like(dy)
        N.layernorm_bwd(dy, z, mean, rstd, gamma, dx, None, None, ws)
        dg, db = torch.full((d,), float("nan"), device=dev), torch.full((d,), float("nan"), device=dev)
        rg, rb = torch.empty(d, device=dev), torch.empty(d, device=dev)
        N.layernorm_param_grads(R, d, ws, rg, rb)
        jobs.append((R, d, ws, dg, db))
        want.append((rg, rb))
    wsg = torch.empty((N.gemm_grouped_ws_bytes([(A, B, C, d, d, R, d, d, None)]) + 255) // 4, device=dev)
    N.gemm_grouped([(A, B, C, d, d, R, d, d, None)], wsg, ln_jobs=jobs)
    for (_, _, _, dg, db), (rg, rb) in zip(jobs, want):
        assert torch.equal(dg, rg) and torch.equal(db, rb)
    ref = A.double().cpu().t() @ B.double().cpu()
    assert (C.double().cpu() - ref).abs().max().item() < 1e-3 * ref.abs().max().item()


@pytest.mark.parametrize("n", [1, 5, 1023, 1024, 1500, 4032, 9000, 16384])
def test_embed_plan_matches_stable_sort(n):
    """mit_embed_plan (register / shuffle / LDS bitonic stages): slot k holds the k-th position in
    (token, position) order; plan[n + k] is the run length at a token's first slot, else 0."""
    g = torch.Generator().manual_seed(n)
    V = 50 if n > 64 else 7  # frequent repeats: long runs
    tk = torch.randint(0, V, (n,), generator=g)
    tk[:: max(1, n // 17)] = 3
    plan = torch.empty(N.embed_plan_ints(n), dtype=torch.int32, device=dev())
    N.embed_plan(tk.to(dev()), plan)
    p = plan.cpu()
    order = sorted(range(n), key=lambda i: (int(tk[i]), i))
    assert p[:n].tolist() == order
    runs = [0] * n
    k = 0
    while k < n:
        j = k
        while j < n and int(tk[order[j]]) == int(tk[order[k]]):
            j += 1
        runs[k] = j - k
        k = j
    assert p[n:].tolist() == runs


@pytest.mark.parametrize("kind", ["self_drop", "cross_drop", "cross_drop40", "cross_drop17"])
def test_attention_dropout_64bit_index_path(kind):
    """Dropout attentions whose mask index B*H*Lq*Lk reaches 2^32 run the 64-bit-index kernels (forward
    attn_fwd_simple, backward attn_bwd_dq/dkv_mfma): mit_attention_set_index_limit(1) sends these small
    calls down that path. The forward and the backward must rebuild the SAME mask (mix_u32's 64-bit index:
    high half rotated in, zero here) -- checked through outputs, lse and all three gradients against torch
    with the mask from mit_dropout_mask."""
    N.attention_set_index_limit(1.0)
    try:
        test_attention_fwd_bwd(torch.bfloat16, 64, kind)
    finally:
        N.attention_set_index_limit(0.0)
