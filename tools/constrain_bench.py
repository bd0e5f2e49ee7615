#!/usr/bin/env python3
"""Constrained decode: what the constraint launch costs per token step, what greedy decoding gives up with the head's
folded argmax, and the kernel's own duration.

  python tools/constrain_bench.py [--reps 5] [--out profiles/constrain_bench.txt]
      configs[1]'s architecture (ViT-B/16, 197 patches + 6L d512 decoder, V = 10000) in bf16, max_len 100, an END that
      is never produced (every row runs all 99 token steps), in ONE process:
        greedy-256 / beam-256x3 / sample-256    generate_batch, generate_beam_batch (beam_size 3), generate_sample_batch
                                                (T 0.7, top_k 50, top_p 0.9), B = 256 images, constraints OFF: the
                                                unconstrained code path, launch for launch
        ... +con                                the same with repetition_penalty 1.2, no_repeat_ngram_size 3,
                                                min_length 5, 4 suppressed ids and a 3-token prompt
      A call also runs the encoder and the cross-attention K/V and records its launch plan, so the step time is a
      DIFFERENCE: (call at max_len 100 - call at max_len 20) / 80, each call timed by a host clock around work that
      ends in a device synchronise. The configurations run interleaved, `reps` times after a warm-up round; medians
      are reported with the spread of the long call.
      Then mit_logits_constrain alone on [R, 10000] f32 logits (device events around 200 launches) at R = 256 and 768
      rows and positions p = 10 and 99, with the settings above (no forced step: the prompt is over) and on a forced
      step (the whole row is written).
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

SAMPLING = dict(temperature=0.7, top_k=50, top_p=0.9)
CONSTRAINTS = dict(repetition_penalty=1.2, no_repeat_ngram_size=3, min_length=5, suppress_tokens=(0, 1, 2, 3),
                   prompts=[11, 12, 13])


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
    base = {
        "greedy-256": lambda L, **c: m.generate_batch(images, 2, never, max_len=L, **c),
        "beam-256x3": lambda L, **c: m.generate_beam_batch(images, 2, never, max_len=L, beam_size=3, **c),
        "sample-256": lambda L, **c: m.generate_sample_batch(images, 2, never, max_len=L, seed=1, **SAMPLING, **c),
    }
    runs = {}
    for k, fn in base.items():
        runs[k] = fn
        runs[k + "+con"] = lambda L, fn=fn: fn(L, **CONSTRAINTS)
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
         f"T {SAMPLING['temperature']}, top_k {SAMPLING['top_k']}, top_p {SAMPLING['top_p']}; +con: repetition_penalty "
         f"{CONSTRAINTS['repetition_penalty']}, no_repeat_ngram_size {CONSTRAINTS['no_repeat_ngram_size']}, min_length "
         f"{CONSTRAINTS['min_length']}, {len(CONSTRAINTS['suppress_tokens'])} suppressed ids, a "
         f"{len(CONSTRAINTS['prompts'])}-token prompt")
    for k in runs:
        a, b = statistics.median(t[k][long_]), statistics.median(t[k][short])
        step[k] = 1e3 * (a - b) / (long_ - short)
        emit(f"  {k:15s} {step[k]:7.3f} ms per token step   (call: {1e3 * a:8.1f} ms at max_len {long_}, "
             f"{1e3 * b:7.1f} ms at {short}; spread of the long call {1e3 * min(t[k][long_]):.1f} .. "
             f"{1e3 * max(t[k][long_]):.1f} ms)")
    emit("  constraints on / off:   " + "   ".join(
        f"{k} {step[k + '+con'] / step[k]:.3f} (+{1e3 * (step[k + '+con'] - step[k]):.1f} us)" for k in base))


def kernels(args, emit):
    import torch
    import native as N
    N.load_library()
    V, n = args.vocab, 200
    Vp = (V + 7) // 8 * 8
    L = 100
    emit(f"mit_logits_constrain alone, [R, {V}] f32 logits (ld {Vp}), histories of 40 distinct tokens, device events "
         f"around {n} launches, us per launch")
    for R in (256, 768):
        g = torch.Generator().manual_seed(R)
        logits = (torch.randn(R, Vp, generator=g) * 3).cuda()
        tok = torch.randint(4, 44, (R, L), generator=g).cuda()
        fin = torch.zeros(R, dtype=torch.int32, device="cuda")
        sup = torch.tensor([0, 1, 2, 3], dtype=torch.int64, device="cuda")
        forced = torch.full((R, L), 7, dtype=torch.int64, device="cuda")
        pos = torch.zeros(1, dtype=torch.int64, device="cuda")

        def event_time(fn):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return 1e3 * e0.elapsed_time(e1) / n
        row = [f"  R = {R:3d}:"]
        for p in (10, 99):
            pos.fill_(p)
            torch.cuda.synchronize()
            kw = dict(finished=fin, repetition_penalty=1.2, no_repeat_ngram=3, min_length=5, end_id=5, suppress=sup)
            row.append(f"p = {p}: constraints {event_time(lambda: N.logits_constrain(logits, V, tok, pos, **kw)):6.1f}")
            row.append(f"forced step {event_time(lambda: N.logits_constrain(logits, V, tok, pos, forced=forced, **kw)):6.1f}")
        emit("   ".join(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--vocab", type=int, default=10000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "constrain_bench.txt"))
    ap.add_argument("--part", choices=["steps", "kernels"], help="run one part in this process (the parent starts these)")
    ap.add_argument("--limit", type=int, default=420, help="seconds each part may take")
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if args.part is None:
        with open(args.out, "w") as f:
            f.write("# tools/constrain_bench.py on one MI355X (constraints: csrc/constrain.hip, "
                    "decoder.DecodeConstraints)\n")
        for part in ("steps", "kernels"):
            rc = subprocess.call(["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__),
                                  "--part", part, "--reps", str(args.reps), "--vocab", str(args.vocab), "--out", args.out])
            if rc != 0:
                sys.exit(f"constrain_bench: part {part} ended with status {rc}; nothing further was started")
        return
    import torch
    if not torch.cuda.is_available():
        sys.exit("constrain_bench: needs the GPU (there is no CPU timing)")
    with open(args.out, "a") as f:
        def emit(s):
            print(s, flush=True)
            f.write(s + "\n")
            f.flush()
        (steps if args.part == "steps" else kernels)(args, emit)


if __name__ == "__main__":
    main()
