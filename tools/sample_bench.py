#!/usr/bin/env python3
"""Sampled decode: what a token step costs next to the beam and greedy steps, and the pick kernel's own duration.

  python tools/sample_bench.py [--reps 5] [--out profiles/sample_bench.txt]
      configs[1]'s architecture (ViT-B/16, 197 patches + 6L d512 decoder, V = 10000) in bf16, max_len 100, an END that
      is never produced (every row runs all 99 token steps), in ONE process:
        sample-256x1 / sample-256x3   generate_sample_batch, B = 256 images, 1 / 3 samples each (T 0.7, top_k 50, top_p 0.9)
        beam-256x1 / beam-256x3       generate_beam_batch, B = 256, beam_size 1 / 3: the same body and f32 head, with
                                      the two-launch selection in place of the pick -- the yardstick
        greedy-256                    generate_batch, B = 256
      A call also runs the encoder and the cross-attention K/V and records its launch plan, so the step time is a
      DIFFERENCE: (call at max_len 100 - call at max_len 20) / 80, each call timed by a host clock around work that
      ends in a device synchronise. The configurations run interleaved, `reps` times after a warm-up round; medians
      are reported, with sample / beam at equal rows (the issue's yardstick: at most 1.10).
      Then the selection kernels alone on [R, 10000] f32 logits (device events around 200 launches): mit_sample_pick
      with each filter on and off, mit_beam_select at the same rows.
The two parts run as child processes, each under its own `timeout`; the parent never opens the GPU and stops at the
first part that fails. Both append to --out."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-image-transformer_amd"))

SAMPLING = dict(temperature=0.7, top_k=50, top_p=0.9)


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def steps(args, emit):
    import torch
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from beam_bench import build_cfg1
    m = build_cfg1(args.vocab)
    g = torch.Generator().manual_seed(5)
    images = torch.randn(256, 3, 224, 224, generator=g).cuda()
    never = args.vocab + 7
    long_, short = 100, 20
    runs = {
        "sample-256x1": lambda L: m.generate_sample_batch(images, 2, never, max_len=L, num_samples=1, seed=1, **SAMPLING),
        "sample-256x3": lambda L: m.generate_sample_batch(images, 2, never, max_len=L, num_samples=3, seed=1, **SAMPLING),
        "beam-256x1": lambda L: m.generate_beam_batch(images, 2, never, max_len=L, beam_size=1),
        "beam-256x3": lambda L: m.generate_beam_batch(images, 2, never, max_len=L, beam_size=3),
        "greedy-256": lambda L: m.generate_batch(images, 2, never, max_len=L),
    }
    for fn in runs.values():  # warm-up: every shape of the timed window
        fn(long_), fn(short)
    t = {k: {long_: [], short: []} for k in runs}
    for _ in range(args.reps):
        for L in (long_, short):
            for k, fn in runs.items():
                t[k][L].append(timed(lambda: fn(L)))
    step = {}
    emit(f"token step, cfg1 architecture bf16, V = {args.vocab}, max_len {long_}; medians of {args.reps} interleaved "
         f"repeats; step = (call at max_len {long_} - call at max_len {short}) / {long_ - short}; sampling at "
         f"T {SAMPLING['temperature']}, top_k {SAMPLING['top_k']}, top_p {SAMPLING['top_p']}")
    for k in runs:
        a, b = statistics.median(t[k][long_]), statistics.median(t[k][short])
        step[k] = 1e3 * (a - b) / (long_ - short)
        emit(f"  {k:12s} {step[k]:7.3f} ms per token step   (call: {1e3 * a:8.1f} ms at max_len {long_}, "
             f"{1e3 * b:7.1f} ms at {short}; spread of the long call {1e3 * min(t[k][long_]):.1f} .. "
             f"{1e3 * max(t[k][long_]):.1f} ms)")
    emit(f"  sample-256x1 / beam-256x1 = {step['sample-256x1'] / step['beam-256x1']:.3f}   "
         f"sample-256x3 / beam-256x3 = {step['sample-256x3'] / step['beam-256x3']:.3f}   (yardstick: <= 1.10)   "
         f"sample-256x1 / greedy-256 = {step['sample-256x1'] / step['greedy-256']:.3f}")


def kernels(args, emit):
    import torch
    import native as N
    N.load_library()
    V, n = args.vocab, 200
    Vp = (V + 7) // 8 * 8
    emit(f"selection kernels alone, [R, {V}] f32 logits (ld {Vp}), device events around {n} launches, us per launch")
    for R in (256, 768):
        g = torch.Generator().manual_seed(R)
        logits = (torch.randn(R, Vp, generator=g) * 3).cuda()
        ids = torch.zeros(R, n + 8, dtype=torch.int64, device="cuda")
        fin = torch.zeros(R, dtype=torch.int32, device="cuda")
        nf = torch.zeros(1, dtype=torch.int32, device="cuda")
        ticket = torch.zeros(1, dtype=torch.int32, device="cuda")
        lp = torch.zeros(R, dtype=torch.float32, device="cuda")
        length = torch.zeros(R, dtype=torch.int32, device="cuda")
        seed = torch.tensor([3], dtype=torch.int64, device="cuda")
        pos = torch.zeros(1, dtype=torch.int64, device="cuda")

        def event_time(fn):
            for _ in range(3):
                fn()
            pos.zero_()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            torch.cuda.synchronize()
            pos.zero_()
            return 1e3 * e0.elapsed_time(e1) / n
        row = [f"  R = {R:3d}:"]
        for name, T, k, p in (("pick T only", 0.7, 0, 1.0), ("top_k 50", 0.7, 50, 1.0), ("top_p 0.9", 0.7, 0, 0.9),
                              ("top_k 50 + top_p 0.9", 0.7, 50, 0.9)):
            us = event_time(lambda: N.sample_pick(logits, V, T, k, p, seed, 0, None, ids, pos, -1, 0, fin, nf, lp, length,
                                                  ticket))
            row.append(f"{name} {us:6.1f}")
        for K in (1, 3):
            B = R // K
            score = torch.zeros(B * K, dtype=torch.float32, device="cuda")
            anc = torch.zeros(B * K, n + 8, dtype=torch.int32, device="cuda")
            ws = torch.empty((N.beam_select_ws_bytes(B, K, V) + 7) // 8, dtype=torch.int64, device="cuda")
            us = event_time(lambda: N.beam_select(logits[:B * K], V, score, ids[:B * K], anc, pos, -1, 0, fin[:B * K],
                                                  length[:B * K], nf, ws, B, K))
            row.append(f"beam_select K={K} {us:6.1f}")
        emit("   ".join(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--vocab", type=int, default=10000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_bench.txt"))
    ap.add_argument("--part", choices=["steps", "kernels"], help="run one part in this process (the parent starts these)")
    ap.add_argument("--limit", type=int, default=420, help="seconds each part may take")
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if args.part is None:
        for part in ("steps", "kernels"):
            rc = subprocess.call(["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__),
                                  "--part", part, "--reps", str(args.reps), "--vocab", str(args.vocab), "--out", args.out])
            if rc != 0:
                sys.exit(f"sample_bench: part {part} ended with status {rc}; nothing further was started")
        return
    import torch
    if not torch.cuda.is_available():
        sys.exit("sample_bench: needs the GPU (there is no CPU timing)")
    with open(args.out, "a") as f:
        def emit(s):
            print(s, flush=True)
            f.write(s + "\n")
            f.flush()
        (steps if args.part == "steps" else kernels)(args, emit)


if __name__ == "__main__":
    main()
