"""Micro-benchmark of mit_attention_bwd on the decoder's training shapes (bf16, dropout 0.1):
self-attention (63 x 63, causal + key-PAD mask, 8 heads) and cross-attention (63 queries x 197
patches). Run under rocprofv3 --kernel-trace --stats for the dQ / dKV kernel split.

--cold adds the "cold strided" mode: the cross-attention K/V and dK/dV are views into
[B*S, L*2*d] buffers laid out as decoder.py's kv_all / dkv (L = 6), a timed batch is one launch per layer, and a
pass over 512 MB of unrelated memory sits between batches. Hot and cold are both printed."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-image-transformer_amd"))
import torch  # noqa: E402

import native  # noqa: E402
from attn_bench import LAYERS, timed  # noqa: E402


def run(iters=20, cold=False):
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    B, H, T, S, d = 64, 8, 63, 197, 512
    seed = torch.tensor([123], device=dev)
    tok = torch.randint(4, 1000, (B, T), generator=g).to(dev)
    flush = torch.zeros(128 << 20, device=dev) if cold else None  # 512 MB, twice the 256 MB last-level cache
    for name, causal, Lk in (("self", True, T), ("cross", False, S)):
        nl = LAYERS if cold and not causal else 1
        ld = nl * 2 * d
        q = torch.randn(B, T, d, generator=g).to(dev, torch.bfloat16)
        kv = torch.randn(B * Lk, ld, generator=g).to(dev, torch.bfloat16)
        o = torch.empty(B, T, d, device=dev, dtype=torch.bfloat16)
        do = torch.randn(B, T, d, generator=g).to(dev, torch.bfloat16)
        dq = torch.empty_like(q)
        dkv = torch.empty_like(kv)
        delta = torch.empty(B * H * T, device=dev)
        calls = []
        for l in range(nl):
            lse = torch.empty(B * H * T, device=dev)
            kvl, dkvl = kv[:, l * 2 * d:], dkv[:, l * 2 * d:]
            a = native.attn_args(q, d, T * d, kvl, ld, Lk * ld, kvl[:, d:], ld, Lk * ld, o, d, T * d, lse=lse,
                                 key_tokens=tok if causal else None, tok_batch=T, causal=causal, scale=0.125, drop_p=0.1,
                                 seed=seed, site=3)
            native.attention_fwd(native.BF16, B, H, T, Lk, a)  # o is the last layer's: only delta reads it
            gr = native.attn_grads(do, d, T * d, dq, d, T * d, dkvl, ld, Lk * ld, dkvl[:, d:], ld, Lk * ld, delta)
            calls.append((a, gr))

        def fn(c=calls[nl // 2]):
            native.attention_bwd(native.BF16, B, H, T, Lk, *c)

        def batch():
            for c in calls:
                fn(c)
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t = timed(fn, iters) * 1e-6
        fl = 8.0 * B * H * T * Lk * 64  # dS/dP (2) + dQ, dK, dV (3) ... counted as 2x the forward's 4*Lq*Lk*d
        line = f"bwd {name:6s} B={B} H={H} Lq={T} Lk={Lk}  {t * 1e6:8.1f} us  {fl / t / 1e12:7.1f} TFLOP/s"
        if cold:
            line += f"  cold {timed(batch, iters, flush) / nl:8.1f} us"
        print(line, flush=True)


if __name__ == "__main__":
    native.load_library()
    run(cold="--cold" in sys.argv[1:])
