#!/usr/bin/env python3
"""Sampled / constrained rolling-batch captioning (generate_stream) against the static decoders, on one GPU.

  python tools/stream_bench.py [--reps 5] [--images 2048] [--out profiles/stream_bench.txt]
      tools/rolling_bench.py's set-up: configs[4]'s architecture (ViT-B/16, 197 patches + 6L d512 decoder, V = 10000,
      random weights) in bf16, `images` images resident on the device, slots = 256, END never produced, raggedness from
      the same SYNTHETIC caps (rolling_bench.synthetic_caps) -- no model was asked for its lengths.
        (a) ragged, captions/s, sampled at N = 1 and N = 5 samples per image (temperature 0.7, top_k 50, top_p 0.9):
            generate_stream(max_lens = caps) against the static way: generate_sample_batch on consecutive chunks of
            256 // N images (at most 256 rows) with max_len = max(cap in chunk), rows cut to their caps on the host.
            Token steps, slot occupancy, and at N = 5 the admit copies' share: N copies of an image's K/V per image,
            timed alone as 256-record mit_slot_admit_ex launches on a state of the same shape.
        (b) uniform, max_lens = None, 256 rows: the MARGINAL cost of a token step, (t(max_len 100) - t(max_len 52)) / 48,
            sampled stream against generate_sample_batch, and constrained greedy stream (repetition penalty 1.2,
            no-repeat 3-gram) against generate_batch with the same constraints; encoder and set-up cancel.
      Every figure: a warm-up of every shape first (where the stream's ids are compared with the static ones), then `reps`
      interleaved repeats (one of each variant per round), host clock around a call that ends in a device synchronise;
      medians with the spread.
The measurement runs in a child process under `timeout`; the parent never opens the GPU."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-image-transformer_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from rolling_bench import SLOTS, START, fmt, synthetic_caps, timed  # noqa: E402

SAMPLING = dict(temperature=0.7, top_k=50, top_p=0.9)
CONSTRAINTS = dict(repetition_penalty=1.2, no_repeat_ngram_size=3)


def bench(args, emit):
    import torch
    from beam_bench import build_cfg1
    m = build_cfg1(args.vocab)
    never = args.vocab + 7
    n = args.images
    images = torch.randn(n, 3, 224, 224, generator=torch.Generator().manual_seed(5)).cuda()
    caps = synthetic_caps(n)
    useful = sum(c - 1 for c in caps)
    emit(f"cfg4 architecture bf16, V = {args.vocab}, {n} images on the device, slots = {SLOTS}, END never produced; "
         f"SYNTHETIC caps (rolling_bench.synthetic_caps): mean {sum(caps) / n:.2f}, max {max(caps)}; sampling "
         f"{SAMPLING}; medians of {args.reps} interleaved repeats")

    def static(N):
        per = SLOTS // N
        out = []
        for lo in range(0, n, per):
            hi = min(lo + per, n)
            rows = m.generate_sample_batch(images[lo:hi], START, never, max_len=max(caps[lo:hi]), num_samples=N, seed=3,
                                           image_offset=lo, return_logprob=True, **SAMPLING)
            out.extend([ids[:c] for ids, _ in r] for r, c in zip(rows, caps[lo:hi]))
        return out

    def stream(N):
        got = m.generate_stream(images, START, never, max_len=100, slots=SLOTS, num_samples=N, seed=3, max_lens=caps,
                                return_logprob=True, **SAMPLING)
        return [[ids for ids, _ in r] for r in got]

    runs, sched = {}, {}
    for N in (1, 5):
        runs[f"static N={N}"] = lambda N=N: static(N)
        runs[f"stream N={N}"] = lambda N=N: stream(N)
    ref = {}
    for k, fn in runs.items():  # warm-up of every shape, and the results compared
        out = fn()
        torch.cuda.synchronize()
        if k.startswith("static"):
            ref[k.split()[1]] = out
        else:
            s = m.last_rolling_schedule
            sched[k] = (s.steps, s.polls, s.admits, s.chunks, out == ref[k.split()[1]])
    t = {k: [] for k in runs}
    for _ in range(args.reps):
        for k, fn in runs.items():
            t[k].append(timed(fn)[0])
    # the admit copies alone: 256-record launches on a state of the same shape (the pool holds whatever it holds)
    dec = m.decoder
    _, _, S, _, _ = m._encode_memory(images[:2])
    stt = dec.rolling_stream_begin(S, SLOTS, 100, START, never, pool=SLOTS, temperature=0.7)
    recs = [(s, s, 50, s, -1) for s in range(SLOTS)]
    dec.rolling_admit_ex(stt, recs)
    ta = []
    for _ in range(args.reps):
        ta.append(timed(lambda: [dec.rolling_admit_ex(stt, recs) for _ in range(8)])[0] / (8 * SLOTS))
    copy_us = 1e6 * statistics.median(ta)
    del stt
    for N in (1, 5):
        per = SLOTS // N
        st_steps = sum(max(caps[lo:lo + per]) - 1 for lo in range(0, n, per))
        ts, tr = statistics.median(t[f"static N={N}"]), statistics.median(t[f"stream N={N}"])
        steps, polls, admits, chunks, same = sched[f"stream N={N}"]
        emit(f"(a) N = {N}: static (generate_sample_batch per {per} images = {per * N} rows, max_len = chunk max): "
             f"{fmt(t[f'static N={N}'])}  {n * N / ts:8.0f} captions/s; {st_steps} token steps")
        emit(f"    N = {N}: stream: {fmt(t[f'stream N={N}'])}  {n * N / tr:8.0f} captions/s = {ts / tr:.2f}x static; "
             f"{steps} token steps ({st_steps / steps:.2f}x fewer), occupancy {N * useful / (steps * SLOTS):.3f}, "
             f"{polls} polls, {admits} admit launches, {chunks} encoder chunks; ids equal to static: {same}")
        emit(f"    N = {N}: admit copies: {n * N} of {copy_us:.2f} us each (timed alone, {SLOTS} per launch) = "
             f"{1e-3 * n * N * copy_us:.1f} ms = {100 * 1e-6 * n * N * copy_us / tr:.1f} % of the stream's time; an index "
             f"table would leave {n} copies ({100 * 1e-6 * n * copy_us / tr:.1f} %)")
    # (b) the marginal token step, uniform lengths, 256 rows
    one = images[:SLOTS]
    lens = (52, 100)
    ub = {}
    for L in lens:
        ub[("sampled static", L)] = lambda L=L: m.generate_sample_batch(one, START, never, max_len=L, seed=3, **SAMPLING)
        ub[("sampled stream", L)] = lambda L=L: m.generate_stream(one, START, never, max_len=L, slots=SLOTS, seed=3,
                                                                 **SAMPLING)
        ub[("constrained greedy static", L)] = lambda L=L: m.generate_batch(one, START, never, max_len=L, **CONSTRAINTS)
        ub[("constrained greedy stream", L)] = lambda L=L: m.generate_stream(one, START, never, max_len=L, slots=SLOTS,
                                                                            **CONSTRAINTS)
    same = {}
    for (who, L), fn in ub.items():
        same[(who, L)] = fn()
    torch.cuda.synchronize()
    tu = {k: [] for k in ub}
    for _ in range(args.reps):
        for k, fn in ub.items():
            tu[k].append(timed(fn)[0])
    dsteps = lens[1] - lens[0]
    emit(f"(b) uniform, {SLOTS} rows, END never, max_lens = None: marginal token step = (t(max_len {lens[1]}) - "
         f"t(max_len {lens[0]})) / {dsteps}, per repeat; constraints {CONSTRAINTS}")
    for who in ("sampled static", "sampled stream", "constrained greedy static", "constrained greedy stream"):
        perstep = [(b - a) / dsteps for a, b in zip(tu[(who, lens[0])], tu[(who, lens[1])])]
        eq = ""
        if who.endswith("stream"):
            eq = f"; ids equal to static: {same[(who, lens[1])] == same[(who.replace('stream', 'static'), lens[1])]}"
        emit(f"    {who:28s}: {fmt(perstep, 1e6, 'us')} per token step; whole call max_len {lens[1]}: "
             f"{fmt(tu[(who, lens[1])])}{eq}")
    emit("    (the stream's step runs 6 mit_kv_store_ragged launches that the scalar-position step folds into its in_proj "
         "GEMMs, and a poll every check_every steps, as the greedy rolling step does: profiles/rolling_bench.txt)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--images", type=int, default=2048)
    ap.add_argument("--vocab", type=int, default=10000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_bench.txt"))
    ap.add_argument("--child", action="store_true", help="measure in this process (the parent starts it)")
    ap.add_argument("--limit", type=int, default=540, help="seconds the measurement may take")
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if not args.child:
        with open(args.out, "w") as f:
            f.write("# tools/stream_bench.py on one MI355X (sampled / constrained rolling-batch captioning: "
                    "mit_logits_constrain_ragged, mit_sample_pick_ragged, mit_slot_admit_ex, model.generate_stream)\n")
        rc = subprocess.call(["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child",
                              "--reps", str(args.reps), "--images", str(args.images), "--vocab", str(args.vocab),
                              "--out", args.out])
        if rc != 0:
            sys.exit(f"stream_bench: the measurement ended with status {rc}")
        return
    import torch
    if not torch.cuda.is_available():
        sys.exit("stream_bench: needs the GPU (there is no CPU timing)")
    with open(args.out, "a") as f:
        def emit(s):
            print(s, flush=True)
            f.write(s + "\n")
            f.flush()
        bench(args, emit)


if __name__ == "__main__":
    main()
