#!/usr/bin/env python3
"""Caption scoring against what a user had to do before it: time per call, the score kernel's own duration and
bandwidth, and the logits memory of both.

  python tools/score_bench.py [--reps 5] [--out profiles/score_bench.txt]
      configs[1]'s architecture (ViT-B/16, 197 patches + 6L d512 decoder, V = 10000) in bf16, B = 256 images, C = 1 and
      5 full-length candidates per image (T = 100 decoder positions, no PAD), in ONE process:
        score      ImageToTextModel.score_captions: the image encoded once, its cross-attention K/V computed once for
                   the C candidates, the head in chunks of decoder.default_head_rows rows reduced by mit_score_rows
        baseline   model.forward on the images repeated C times, in chunks of --chunk sequences (f32 logits
                   [chunk, T, V]), then torch.log_softmax and a gather on the device: the hand-rolled way
      Both end in a device synchronise and are timed by a host clock; they run interleaved, `reps` times after a warm-up
      round of every shape; medians with the spread. The two results are compared (worst per-caption difference per
      token). Peak memory: torch's peak allocation over a call minus what was allocated before it, and the logits
      buffers by shape.
      Then the parts of the scoring call on their own, device events around `n` repeats: the head GEMM chunks over all
      R = B*C*T rows, and mit_score_rows over the same rows, once on the ONE head buffer the call uses (32 MiB, re-read
      while it is still in the caches, as in the call) and once over a ring of buffers larger than the 256 MiB
      Infinity Cache (every launch reads from HBM). GB/s = rows * V * 2 bytes / kernel time: the bytes the kernel
      must read.
The two parts run as child processes, each under its own `timeout`; the parent never opens the GPU and stops at the
first part that fails. The parent starts --out afresh, the parts append to it."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-image-transformer_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

START, END, PAD = 1, 2, 0
B, T = 256, 100


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def sequences(vocab, C, seed=7):
    """[B, C, T + 1] START .. END sequences of full length: every one of the B*C*T positions is scored"""
    import torch
    g = torch.Generator().manual_seed(seed + C)
    seq = torch.randint(3, vocab, (B, C, T + 1), generator=g)
    seq[..., 0], seq[..., -1] = START, END
    return seq.cuda()


def baseline(m, images, seq, chunk):
    """per-caption log-probabilities [B, C] the hand-rolled way"""
    import torch
    b, c, L = seq.shape
    tok = seq[:, :, :-1].reshape(b * c, L - 1)
    tgt = seq[:, :, 1:].reshape(b * c, L - 1)
    per = max(1, chunk // c)
    out = []
    with torch.no_grad():
        for i in range(0, b, per):
            rows = slice(i * c, min(i + per, b) * c)
            logits = m.forward(images[i:i + per].repeat_interleave(c, 0), tok[rows])
            lp = torch.log_softmax(logits, -1).gather(-1, tgt[rows].unsqueeze(-1)).squeeze(-1)
            out.append((lp * (tgt[rows] != PAD)).sum(-1))
    return torch.cat(out).view(b, c)


def calls(args, emit):
    import torch
    from beam_bench import build_cfg1
    m = build_cfg1(args.vocab)
    dec = m.decoder
    g = torch.Generator().manual_seed(5)
    images = torch.randn(B, 3, 224, 224, generator=g).cuda()
    seqs = {c: sequences(args.vocab, c) for c in (1, 5)}
    runs = {}
    for c, seq in seqs.items():
        runs[f"score    C={c}"] = lambda seq=seq: m.score_captions(images, seq, START, END)
        runs[f"baseline C={c}"] = lambda seq=seq: baseline(m, images, seq, args.chunk)
    peak = {}
    for k, fn in runs.items():  # warm-up: every shape of the timed window; peak memory of one call
        fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peak[k] = torch.cuda.max_memory_allocated() - before
    t = {k: [] for k in runs}
    for _ in range(args.reps):
        for k, fn in runs.items():
            t[k].append(timed(fn))
    esz = 2
    emit(f"cfg1 architecture bf16, V = {args.vocab} (head row stride {dec.Vp}), B = {B} images, T = {T} positions per "
         f"candidate, memory mode patches (S = 197); medians of {args.reps} interleaved repeats, host clock around a call "
         f"that ends in a device synchronise; baseline in chunks of {args.chunk} sequences")
    med = {k: statistics.median(v) for k, v in t.items()}
    for k in runs:
        emit(f"  {k}: {1e3 * med[k]:9.1f} ms per call   (spread {1e3 * min(t[k]):.1f} .. {1e3 * max(t[k]):.1f} ms; peak "
             f"allocation over the call {peak[k] / 2 ** 20:8.1f} MiB)")
    for c, seq in seqs.items():
        R = B * c * T
        hr = dec.default_head_rows(R)
        per = max(1, args.chunk // c) * c
        emit(f"  C={c}: score / baseline = {med[f'score    C={c}'] / med[f'baseline C={c}']:.3f}; logits memory: score "
             f"{hr} x {dec.Vp} bf16 = {hr * dec.Vp * esz / 2 ** 20:.1f} MiB (head_rows {hr}, {-(-R // hr)} chunks), "
             f"baseline {per} x {T} x {dec.Vp} f32 = {per * T * dec.Vp * 4 / 2 ** 20:.1f} MiB and as much again for "
             f"log_softmax; all {R} rows at once would be {R * dec.Vp * 4 / 2 ** 30:.2f} GiB in f32")
        lp, n, _ = m.score_captions(images, seq, START, END)
        ref = baseline(m, images, seq, args.chunk)
        emit(f"        worst |score - baseline| per token over the {B * c} captions: "
             f"{float(((lp.double() - ref.double()).abs() / n).max()):.3e} (bf16 logits against f32 logits of the same GEMM)")


def parts(args, emit):
    import torch
    import native as N
    from beam_bench import build_cfg1
    m = build_cfg1(args.vocab)
    dec = m.decoder
    m.store.ensure_shadow(force=True)
    V, Vp, d, n = dec.V, dec.Vp, dec.d, args.n

    def event_time(fn):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return 1e-3 * e0.elapsed_time(e1) / n   # seconds per repeat

    g = torch.Generator().manual_seed(9)
    emit(f"parts of the scoring call on their own (device events around {n} repeats), R = B*C*T rows:")
    for c in (1, 5):
        R = B * c * T
        hr = dec.default_head_rows(R)
        x = (torch.randn(R, d, generator=g) * 0.5).to(torch.bfloat16).cuda()
        tgt = torch.randint(3, V, (R,), generator=g).cuda()
        tlp = torch.empty(R, dtype=torch.float32, device="cuda")
        rank = torch.empty(R, dtype=torch.int32, device="cuda")
        ring = [torch.empty(hr, Vp, dtype=torch.bfloat16, device="cuda") for _ in range(-(-(320 << 20) // (hr * Vp * 2)))]
        wo, bo = m.store.w("fc_out.weight"), m.store.p("fc_out.bias")
        chunks = [(r0, min(hr, R - r0)) for r0 in range(0, R, hr)]

        def head(bufs):
            for i, (r0, k) in enumerate(chunks):
                N.linear(x[r0:r0 + k], wo, bufs[i % len(bufs)], bias=bo)

        def score(bufs):
            for i, (r0, k) in enumerate(chunks):
                N.score_rows(bufs[i % len(bufs)], tgt[r0:r0 + k], PAD, tlp[r0:r0 + k], rank[r0:r0 + k], rows=k, V=V, ld=Vp)

        def both(bufs):
            for i, (r0, k) in enumerate(chunks):
                N.linear(x[r0:r0 + k], wo, bufs[i % len(bufs)], bias=bo)
                N.score_rows(bufs[i % len(bufs)], tgt[r0:r0 + k], PAD, tlp[r0:r0 + k], rank[r0:r0 + k], rows=k, V=V, ld=Vp)
        head(ring)      # every buffer holds real logits
        nbytes = R * V * 2
        t_head = event_time(lambda: head(ring[:1]))
        t_one = event_time(lambda: score(ring[:1]))
        t_ring = event_time(lambda: score(ring))
        t_both = event_time(lambda: both(ring[:1]))
        emit(f"  C={c}: R = {R}, head_rows {hr} ({len(chunks)} chunks; plan {N.score_rows_plan(N.BF16, hr, V, ring[0], Vp)}: "
             f"1 = the row in registers)")
        emit(f"        head GEMM chunks            {1e3 * t_head:8.3f} ms   ({2.0 * R * Vp * d / t_head / 1e12:.0f} TFLOP/s)")
        emit(f"        mit_score_rows, one buffer  {1e3 * t_one:8.3f} ms   ({nbytes / t_one / 1e9:.0f} GB/s of the "
             f"{nbytes / 1e9:.2f} GB it must read; the 32 MiB buffer stays in the caches)")
        emit(f"        mit_score_rows, {len(ring):2d}-buffer ring {1e3 * t_ring:6.3f} ms   ({nbytes / t_ring / 1e9:.0f} GB/s; "
             f"{len(ring) * hr * Vp * 2 / 2 ** 20:.0f} MiB of buffers: every launch reads from HBM)")
        emit(f"        head + score as the call interleaves them {1e3 * t_both:8.3f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=10, help="repeats inside a device-event window")
    ap.add_argument("--vocab", type=int, default=10000)
    ap.add_argument("--chunk", type=int, default=256, help="sequences per forward of the baseline")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_bench.txt"))
    ap.add_argument("--part", choices=["calls", "parts"], help="run one part in this process (the parent starts these)")
    ap.add_argument("--limit", type=int, default=420, help="seconds each part may take")
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if args.part is None:
        with open(args.out, "w") as f:
            f.write("# tools/score_bench.py on one MI355X (caption scoring: csrc/score.hip, decoder.run_score)\n")
        for part in ("calls", "parts"):
            rc = subprocess.call(["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__),
                                  "--part", part, "--reps", str(args.reps), "--n", str(args.n), "--vocab", str(args.vocab),
                                  "--chunk", str(args.chunk), "--out", args.out])
            if rc != 0:
                sys.exit(f"score_bench: part {part} ended with status {rc}; nothing further was started")
        return
    import torch
    if not torch.cuda.is_available():
        sys.exit("score_bench: needs the GPU (there is no CPU timing)")
    with open(args.out, "a") as f:
        def emit(s):
            print(s, flush=True)
            f.write(s + "\n")
            f.flush()
        (calls if args.part == "calls" else parts)(args, emit)


if __name__ == "__main__":
    main()
