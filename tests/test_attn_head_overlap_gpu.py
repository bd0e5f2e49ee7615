"""attn_fwd_head<DROP> with all of a thread's K/V chunk rows in flight at once and attn_bwd_head with the dropout
mask hashed into per-lane bits under the load wait (csrc/attention.hip), B = 2, H = 2, Dh = 64,
bf16.

Shapes: Lq in {1, 17, 63, 64} (one live row, a partial 16-row tile, the train step's Lq, a full tile) x Lk in
{16, 40, 150, 197, 230, 256} (no full 64-key chunk, tails of one / two / three 16-key tiles, the step's 197, two
key strips per wave and the LDS limit of the backward) x p in {0, 0.1, 0.5}; forward-only Lk = 577 (the configs[2]
memory: three staging round trips of eight chunk rows), Lq = 150 (more query tiles than waves, eight waves
staging), and Lk = 320 / 640 (two workgroups per CU at most / the whole LDS); one causal + PAD self-attention backward
(attn_bwd_head's other caller); one case on strided operands inside sentinel-filled buffers.

Checks: mit_attention_plan names the head kernels; O, lse, dQ, dK, dV against float32 torch on the same bf16
inputs with the mask rebuilt on the host from the documented hash (tests/misc_contract.py), at the bounds
test_kernels_gpu.py uses for these kernels (o 2e-2, lse 1e-3, grads 4e-2 of the output's scale); with Q = 0,
one-hot V and dO and p = 0.5 the kept keys per (b, h, i, j % 64) read off O equal the host mask's as integers and
the kept (i, j) pairs read off dV equal the host mask bit for bit; two launches are bitwise equal.

Index-limit case: below mit_attention_set_index_limit's limit the dispatch leaves the head kernels for the generic
forward and the dq / dkv MFMA pair (tests/attn_contract.py pins that), which round differently, so their outputs
cannot equal the head kernels' bit for bit. What is compared exactly is what the mask decides: the kept counts
and kept pairs of the Q = 0 probe from the two paths are equal, and the values agree within the bounds above."""
import pytest
import torch

import native as N
from misc_contract import host_mask

pytestmark = pytest.mark.gpu

B, H, D = 2, 2, 64
E = H * D
SEED, SITE = 1234567, 7
LQS, LKS, PS = (1, 17, 63, 64), (16, 40, 150, 197, 230, 256), (0.0, 0.1, 0.5)


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    N.load_library()
    try:
        yield
    finally:
        N.attention_set_index_limit(0.0)
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:  # a GPU fault poisons the process: launch nothing more on it
        pytest.exit(f"GPU error after an attention case, run ended: {e}", returncode=3)


def _close(got, ref, tol, what):
    scale = max(ref.abs().max().item(), 1e-3)
    err = (got.float() - ref).abs().max().item()
    print(f"{what}: max err {err:.3e} of scale {scale:.3e} (bound {tol})")
    assert err <= tol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e} (tol {tol})"


def _heads(x):  # [B, L, H*D] view -> [B, H, L, D]
    return x.float().reshape(x.shape[0], x.shape[1], H, D).transpose(1, 2)


class Run:
    """One attention problem on device buffers; pad > 0 puts every operand inside a larger sentinel-filled buffer"""
    SENT = 7.5

    def __init__(self, Lq, Lk, p, *, causal=False, q=None, kv=None, do=None, pad=0, gen=None):
        self.Lq, self.Lk, self.p, self.causal, self.pad = Lq, Lk, p, causal, pad
        g = gen or torch.Generator().manual_seed(Lq * 1000 + Lk)
        dev = "cuda"
        q = torch.randn(B, Lq, E, generator=g) if q is None else q
        kv = torch.randn(B, Lk, 2 * E, generator=g) if kv is None else kv
        do = torch.randn(B, Lq, E, generator=g) if do is None else do
        self.bufs = {}

        def window(name, L, W, src=None, dtype=torch.bfloat16):
            # rows of W elements at a row stride of W + 2 * pad, pad rows before / after each batch's L rows
            whole = torch.full((B, L + 2 * (pad > 0), W + 2 * pad), self.SENT, dtype=dtype, device=dev)
            view = whole[:, (pad > 0):(pad > 0) + L, pad:pad + W]
            if src is not None:
                view.copy_(src.to(dtype))
            self.bufs[name] = (whole, view)
            return view
        self.q, self.kv, self.do = window("q", Lq, E, q), window("kv", Lk, 2 * E, kv), window("do", Lq, E, do)
        self.o, self.dq, self.dkv = window("o", Lq, E), window("dq", Lq, E), window("dkv", Lk, 2 * E)
        self.lse = torch.full((B * H * Lq + 2,), self.SENT, device=dev)
        self.delta = torch.full((B * H * Lq + 2,), self.SENT, device=dev)
        self.tok = None
        if causal:
            self.tok = torch.randint(4, 100, (B, Lk), generator=g).to(dev)
            self.tok[1, Lk // 2:] = 0
        self.seed = torch.tensor([SEED], dtype=torch.int64, device=dev)
        st = lambda v: (v.stride(1), v.stride(0))  # noqa: E731
        self.a = N.attn_args(self.q, *st(self.q), self.kv, *st(self.kv), self.kv[..., E:], *st(self.kv), self.o, *st(self.o),
                             lse=self.lse[1:], key_tokens=self.tok, tok_batch=Lk, pad_idx=0, causal=causal, scale=D ** -0.5,
                             drop_p=p, seed=self.seed, site=SITE)
        self.g = N.attn_grads(self.do, *st(self.do), self.dq, *st(self.dq), self.dkv, *st(self.dkv), self.dkv[..., E:],
                              *st(self.dkv), self.delta[1:])

    def plan(self):
        return N.attention_plan(N.BF16, B, H, self.Lq, self.Lk, self.a, self.g)

    def fwd(self):
        N.attention_fwd(N.BF16, B, H, self.Lq, self.Lk, self.a)
        torch.cuda.synchronize()
        return self.o.clone(), self.lse[1:-1].clone()

    def bwd(self):
        N.attention_bwd(N.BF16, B, H, self.Lq, self.Lk, self.a, self.g)
        torch.cuda.synchronize()
        return self.dq.clone(), self.dkv.clone()

    def keep(self):
        """[B, H, Lq, Lk] float32 keep-multipliers of the documented hash, on the host"""
        if self.p == 0:
            return torch.ones(B, H, self.Lq, self.Lk)
        return host_mask(B * H * self.Lq * self.Lk, self.p, SEED, SITE).view(B, H, self.Lq, self.Lk)

    def reference(self):
        q, k, v = (_heads(x).cpu().requires_grad_(True) for x in (self.q, self.kv[..., :E], self.kv[..., E:]))
        s = (q @ k.transpose(-1, -2)) * D ** -0.5
        if self.causal:
            s = s + torch.triu(torch.full((self.Lq, self.Lk), float("-inf")), diagonal=1)
            s = s.masked_fill((self.tok.cpu() == 0)[:, None, None, :], float("-inf"))
        o = (torch.softmax(s, -1) * self.keep()) @ v
        o.backward(_heads(self.do).cpu())
        return o.detach(), torch.logsumexp(s, -1).detach(), q.grad, k.grad, v.grad

    def guards_intact(self, written):
        for name, (whole, view) in self.bufs.items():
            probe = whole.clone()
            if name in written:
                probe[:, (self.pad > 0):(self.pad > 0) + view.shape[1], self.pad:self.pad + view.shape[2]] = self.SENT
            else:
                continue
            assert bool((probe == self.SENT).all()), f"{name}: written outside its window"
        assert self.lse[0].item() == self.SENT and self.lse[-1].item() == self.SENT
        assert self.delta[0].item() == self.SENT and self.delta[-1].item() == self.SENT


def _check_values(r, fwd_only=False):
    o1, l1 = r.fwd()
    o2, l2 = r.fwd()
    assert torch.equal(o1.view(torch.int16), o2.view(torch.int16)) and torch.equal(l1, l2), "forward not deterministic"
    oref, lref, dqr, dkr, dvr = r.reference()
    tag = f"{r.Lq}x{r.Lk} p={r.p}"
    _close(_heads(o1).cpu(), oref, 2e-2, f"{tag} o")
    _close(l1.view(B, H, r.Lq).cpu(), lref, 1e-3, f"{tag} lse")
    if fwd_only:
        return
    dq1, dkv1 = r.bwd()
    dq2, dkv2 = r.bwd()
    assert torch.equal(dq1.view(torch.int16), dq2.view(torch.int16)), "dq not deterministic"
    assert torch.equal(dkv1.view(torch.int16), dkv2.view(torch.int16)), "dk / dv not deterministic"
    _close(_heads(dq1).cpu(), dqr, 4e-2, f"{tag} dq")
    _close(_heads(dkv1[..., :E]).cpu(), dkr, 4e-2, f"{tag} dk")
    _close(_heads(dkv1[..., E:]).cpu(), dvr, 4e-2, f"{tag} dv")


def _head_planned(r, bwd=True):
    p = r.plan()
    assert p.fwd == (N.ATTN_FWD_HEAD_DROP if r.p > 0 else N.ATTN_FWD_HEAD) or r.causal, f"forward family {p.fwd}"
    if bwd:
        assert p.bwd == N.ATTN_BWD_HEAD, f"backward family {p.bwd}"


@pytest.mark.parametrize("Lk", LKS)
@pytest.mark.parametrize("Lq", LQS)
def test_head_kernels_values_and_determinism(Lq, Lk):
    g = torch.Generator().manual_seed(Lq * 1000 + Lk)
    q, kv, do = torch.randn(B, Lq, E, generator=g), torch.randn(B, Lk, 2 * E, generator=g), torch.randn(B, Lq, E, generator=g)
    for p in PS:
        r = Run(Lq, Lk, p, q=q, kv=kv, do=do)
        _head_planned(r)
        _check_values(r)


@pytest.mark.parametrize("Lq,Lk", [(63, 577), (150, 197), (17, 320), (17, 640)])
def test_forward_staging_sizes(Lq, Lk):
    r = Run(Lq, Lk, 0.1)
    _head_planned(r, bwd=False)
    _check_values(r, fwd_only=True)


def test_self_attention_backward_causal_pad_dropout():
    r = Run(63, 63, 0.1, causal=True)
    p = r.plan()
    assert p.bwd == N.ATTN_BWD_HEAD
    _check_values(r)


def test_strided_operands_and_guard_bands():
    r = Run(63, 197, 0.1, pad=8)
    _head_planned(r)
    _check_values(r)
    r.guards_intact({"o", "dq", "dkv"})
    for name in ("q", "kv", "do"):  # inputs: not written at all
        whole, view = r.bufs[name]
        probe = whole.clone()
        probe[:, 1:1 + view.shape[1], 8:8 + view.shape[2]] = Run.SENT
        assert bool((probe == Run.SENT).all()), f"{name}: input written"


def _probe(Lq, Lk, bwd=True):
    """Q = 0 makes P uniform; V and dO one-hot (V[j, j % 64] = 1, dO[i, i] = 1) at p = 0.5 read the mask off:
    o[i, c] = 2 / Lk * (kept keys j of query i with j % 64 == c), at most 10 of them, so bf16 rounding (2^-8 of
    the value) stays under 0.04 of a count; dv[j, i] = bf16(2 * P_ij) if (i, j) is kept, else 0.
    Returns (the problem, kept keys per (b, h, i, j % 64), kept mask [B, H, Lq, Lk] from dv or None)"""
    eye = torch.eye(64)
    v = eye[torch.arange(Lk) % 64].repeat(1, H).expand(B, Lk, E)
    do = eye[torch.arange(Lq)].repeat(1, H).expand(B, Lq, E)
    r = Run(Lq, Lk, 0.5, q=torch.zeros(B, Lq, E), kv=torch.cat([torch.ones(B, Lk, E), v], -1), do=do)
    o, _ = r.fwd()
    counts = (_heads(o).cpu() * Lk / 2).round().long()
    kept = None
    if bwd:
        _, dkv = r.bwd()
        kept = (_heads(dkv[..., E:]).cpu() != 0).transpose(-1, -2)[:, :, :Lq]
    return r, counts, kept


def _host_counts(keep):
    Lk = keep.shape[-1]
    padded = torch.zeros(*keep.shape[:-1], (Lk + 63) // 64 * 64, dtype=torch.long)
    padded[..., :Lk] = keep
    return padded.view(*keep.shape[:-1], -1, 64).sum(-2)


@pytest.mark.parametrize("Lq,Lk", [(1, 16), (17, 40), (63, 197), (64, 230), (64, 256)])
def test_mask_bits_exact(Lq, Lk):
    r, counts, kept = _probe(Lq, Lk)
    _head_planned(r)
    keep = r.keep() > 0
    assert torch.equal(counts, _host_counts(keep)), "forward: kept keys differ from the host mask"
    assert torch.equal(kept, keep), "backward: kept (query, key) pairs differ from the host mask"


def test_mask_bits_exact_forward_577():
    r, counts, _ = _probe(63, 577, bwd=False)
    _head_planned(r, bwd=False)
    assert torch.equal(counts, _host_counts(r.keep() > 0))


def test_index_limit_path_keeps_the_same_mask():
    Lq, Lk = 63, 197
    r, counts, kept = _probe(Lq, Lk)
    _head_planned(r)
    try:
        N.attention_set_index_limit(1.0)
        p = r.plan()
        assert p.fwd == N.ATTN_GENERIC and p.bwd == N.ATTN_BWD_MFMA  # the 64-bit-index kernels, hash inline
        _, counts2, kept2 = _probe(Lq, Lk)
        assert torch.equal(counts, counts2) and torch.equal(kept, kept2)
        _check_values(Run(Lq, Lk, 0.1))
    finally:
        N.attention_set_index_limit(0.0)
