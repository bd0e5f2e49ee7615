#!/usr/bin/env python3
"""Rolling-batch captioning against static batching, on one GPU.

  python tools/rolling_bench.py [--reps 5] [--images 2048] [--out profiles/rolling_bench.txt]
      configs[4]'s architecture (ViT-B/16, 197 patches + 6L d512 decoder, V = 10000, random weights) in bf16, `images`
      images resident on the device, slots = 256, END never produced, raggedness from max_lens. The length distribution is
      SYNTHETIC: caps = 1 + clip(rint(default_rng(0).lognormal(log(13), 0.4, images)), 5, 99) -- no model was asked.
        (a) ragged, captions/s: generate_rolling(max_lens = caps) against static batching, the parent commit's way:
            generate_batch on consecutive chunks of 256 with max_len = max(cap in chunk), rows cut to their caps on the
            host. Token steps run by each, the ideal ratio sum(chunk max - 1) * slots / sum(caps - 1), the slot
            occupancy (useful row-steps / row-steps run), the encoder's share (measured alone) and what is left for
            admit copies and polls.
        (c) (a) for check_every in 1, 2, 4, 8.
        (b) uniform, max_lens = None: the MARGINAL cost of a token step, (t(max_len 100) - t(max_len 52)) / 48 for 256
            images, rolling against generate_batch, so that the encoder and the set-up cancel.
      (b') `--trace static|rolling` runs that uniform call alone, to be traced from outside (one run each, kernel
            trace with statistics); `--trace-summary A.csv B.csv` appends the per-kernel difference to --out.
      Every figure: a warm-up of every shape first, then `reps` interleaved repeats (one of each variant per round), host
      clock around a call that ends in a device synchronise; medians with the spread.
The measurement runs in a child process under `timeout`; the parent never opens the GPU."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-image-transformer_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

START, SLOTS = 1, 256


def synthetic_caps(n):
    import numpy as np
    return (1 + np.clip(np.rint(np.random.default_rng(0).lognormal(np.log(13), 0.4, n)), 5, 99)).astype(int).tolist()


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def fmt(ts, scale=1e3, unit="ms"):
    return f"{scale * statistics.median(ts):9.2f} {unit} (spread {scale * min(ts):.2f} .. {scale * max(ts):.2f})"


def bench(args, emit):
    import torch
    from beam_bench import build_cfg1
    m = build_cfg1(args.vocab)
    never = args.vocab + 7
    n = args.images
    g = torch.Generator().manual_seed(5)
    images = torch.randn(n, 3, 224, 224, generator=g).cuda()
    caps = synthetic_caps(n)
    chunks = [(i, min(i + SLOTS, n)) for i in range(0, n, SLOTS)]

    def static():
        out = []
        for lo, hi in chunks:
            rows = m.generate_batch(images[lo:hi], START, never, max_len=max(caps[lo:hi]))
            out.extend(r[:c] for r, c in zip(rows, caps[lo:hi]))
        return out

    def rolling(ce):
        return m.generate_rolling(images, START, never, max_len=100, slots=SLOTS, check_every=ce, max_lens=caps)

    def encoder():
        for lo, hi in chunks:
            m._encode_memory(images[lo:hi])

    ces = (1, 2, 4, 8)
    runs = {"static": static, "encoder alone": encoder}
    runs.update({f"rolling check_every={ce}": (lambda ce=ce: rolling(ce)) for ce in ces})
    ref = None
    sched = {}
    for k, fn in runs.items():  # warm-up of every shape, and the results compared
        out = fn()
        torch.cuda.synchronize()
        if k == "static":
            ref = out
        elif k.startswith("rolling"):
            assert out == ref, f"{k}: ids differ from static batching"
            s = m.last_rolling_schedule
            sched[k] = (s.steps, s.polls, s.admits, s.chunks)
    t = {k: [] for k in runs}
    for _ in range(args.reps):
        for k, fn in runs.items():
            t[k].append(timed(fn)[0])
    useful = sum(c - 1 for c in caps)
    static_steps = sum(max(caps[lo:hi]) - 1 for lo, hi in chunks)
    emit(f"cfg4 architecture bf16, V = {args.vocab}, {n} images on the device, slots = {SLOTS}, END never produced; "
         f"SYNTHETIC caps = 1 + clip(rint(lognormal(log 13, 0.4)), 5, 99): mean {sum(caps) / n:.2f}, max {max(caps)}, "
         f"chunk maxima {[max(caps[lo:hi]) for lo, hi in chunks]}; medians of {args.reps} interleaved repeats")
    emit(f"(a) static batching (generate_batch per 256, max_len = chunk max): {fmt(t['static'])}  "
         f"{n / statistics.median(t['static']):8.0f} captions/s; {static_steps} token steps")
    emit(f"    encoder + projection alone, same chunks:                     {fmt(t['encoder alone'])}")
    ideal = static_steps * SLOTS / useful
    emit(f"    ideal step ratio sum(chunk max - 1) * slots / sum(caps - 1) = {ideal:.2f}x "
         f"({useful} useful row-steps = {useful / SLOTS:.1f} full steps)")
    enc = statistics.median(t["encoder alone"])
    for ce in ces:
        k = f"rolling check_every={ce}"
        steps, polls, admits, nchunks = sched[k]
        med = statistics.median(t[k])
        emit(f"(c) {k}: {fmt(t[k])}  {n / med:8.0f} captions/s = {statistics.median(t['static']) / med:.2f}x static; "
             f"{steps} token steps ({static_steps / steps:.2f}x fewer), occupancy {useful / (steps * SLOTS):.3f}, "
             f"{polls} polls, {admits} admit launches, {nchunks} encoder chunks; per step after the encoder "
             f"{1e6 * (med - enc) / steps:.0f} us")
    # (b) the marginal token step, uniform lengths
    one = images[:SLOTS]
    lens = (52, 100)
    ub = {}
    import rolling as R
    whos = ["static", f"rolling check_every={R.CHECK_EVERY_DEFAULT} (default)"] + \
        [f"rolling check_every={ce}" for ce in (1, 4, 8) if ce != R.CHECK_EVERY_DEFAULT]
    for L in lens:
        ub[("static", L)] = lambda L=L: m.generate_batch(one, START, never, max_len=L)
        for who in whos[1:]:
            ce = int(who.split("=")[1].split()[0])
            ub[(who, L)] = lambda L=L, ce=ce: m.generate_rolling(one, START, never, max_len=L, slots=SLOTS,
                                                                check_every=ce)
    for fn in ub.values():
        fn()
    torch.cuda.synchronize()
    tu = {k: [] for k in ub}
    for _ in range(args.reps):
        for k, fn in ub.items():
            tu[k].append(timed(fn)[0])
    dsteps = lens[1] - lens[0]
    emit(f"(b) uniform, {SLOTS} images, END never, max_lens = None: marginal token step = (t(max_len {lens[1]}) - "
         f"t(max_len {lens[0]})) / {dsteps}, per repeat")
    for who in whos:
        per = [(b - a) / dsteps for a, b in zip(tu[(who, lens[0])], tu[(who, lens[1])])]
        emit(f"    {who:36s}: {fmt(per, 1e6, 'us')} per token step; whole call max_len {lens[1]}: "
             f"{fmt(tu[(who, lens[1])])}")
    emit("    (the rolling step runs 6 mit_kv_store_ragged launches that the scalar-pos step folds into its in_proj GEMMs, "
         "and a poll every check_every steps; which launches the difference sits in: --trace / --trace-summary)")


TRACE_CALLS, TRACE_LEN = 4, 100


def trace(args):
    """The uniform call of (b), TRACE_CALLS times (the first warms up), for a kernel trace of this process."""
    import torch
    from beam_bench import build_cfg1
    m = build_cfg1(args.vocab)
    never = args.vocab + 7
    one = torch.randn(SLOTS, 3, 224, 224, generator=torch.Generator().manual_seed(5)).cuda()
    for _ in range(TRACE_CALLS):
        if args.trace == "static":
            m.generate_batch(one, START, never, max_len=TRACE_LEN)
        else:
            m.generate_rolling(one, START, never, max_len=TRACE_LEN, slots=SLOTS)
    torch.cuda.synchronize()


def trace_summary(args, emit):
    """Per-kernel device time per token step from the two kernel-stats tables (static, rolling) of --trace runs."""
    import csv

    def load(path):
        out = {}
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row.get("Name") or row.get("Kernel_Name") or row.get("KernelName")
                tot = float(row.get("TotalDurationNs") or row.get("Total_Duration_Ns") or 0)
                calls = int(float(row.get("Calls") or 0))
                short = name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
                a = out.setdefault(short[:70], [0, 0.0])
                a[0] += calls
                a[1] += tot
        return out
    st, ro = load(args.trace_summary[0]), load(args.trace_summary[1])
    steps = TRACE_CALLS * (TRACE_LEN - 1)
    emit(f"(b') kernel trace of the uniform call ({SLOTS} images, max_len {TRACE_LEN}, {TRACE_CALLS} calls = {steps} "
         f"token steps; each process traced on its own): device time per token step by kernel, us; encoder and "
         f"set-up kernels are in both and cancel in the difference")
    tot_s, tot_r = sum(v[1] for v in st.values()), sum(v[1] for v in ro.values())
    emit(f"    sum of kernel durations per token step: static {tot_s / steps / 1e3:.1f}, rolling {tot_r / steps / 1e3:.1f}, "
         f"difference {(tot_r - tot_s) / steps / 1e3:+.1f}")
    rows = []
    for k in set(st) | set(ro):
        a, b = st.get(k, [0, 0.0]), ro.get(k, [0, 0.0])
        rows.append(((b[1] - a[1]) / steps / 1e3, k, a, b))
    emit(f"    {'kernel':70s} {'static calls/step, us/step':>28s} {'rolling calls/step, us/step':>28s} {'diff us':>8s}")
    for d, k, a, b in sorted(rows, key=lambda r: -abs(r[0]))[:14]:
        emit(f"    {k:70s} {a[0] / steps:14.2f} {a[1] / steps / 1e3:13.2f} {b[0] / steps:14.2f} {b[1] / steps / 1e3:13.2f} "
             f"{d:+8.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--images", type=int, default=2048)
    ap.add_argument("--vocab", type=int, default=10000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rolling_bench.txt"))
    ap.add_argument("--child", action="store_true", help="measure in this process (the parent starts it)")
    ap.add_argument("--trace", choices=["static", "rolling"],
                    help="only run the uniform call of (b) in this process: the program of a kernel-trace run")
    ap.add_argument("--trace-summary", nargs=2, metavar=("STATIC_STATS_CSV", "ROLLING_STATS_CSV"),
                    help="append the per-kernel comparison of two kernel-stats tables to --out (no GPU)")
    ap.add_argument("--limit", type=int, default=540, help="seconds the measurement may take")
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if args.trace:
        return trace(args)
    if args.trace_summary:
        with open(args.out, "a") as f:
            def emit(s):
                print(s, flush=True)
                f.write(s + "\n")
            return trace_summary(args, emit)
    if not args.child:
        with open(args.out, "w") as f:
            f.write("# tools/rolling_bench.py on one MI355X (rolling-batch captioning: csrc/rolling.hip, the mit_*_ragged "
                    "entry points, model.generate_rolling)\n")
        rc = subprocess.call(["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child",
                              "--reps", str(args.reps), "--images", str(args.images), "--vocab", str(args.vocab),
                              "--out", args.out])
        if rc != 0:
            sys.exit(f"rolling_bench: the measurement ended with status {rc}")
        return
    import torch
    if not torch.cuda.is_available():
        sys.exit("rolling_bench: needs the GPU (there is no CPU timing)")
    with open(args.out, "a") as f:
        def emit(s):
            print(s, flush=True)
            f.write(s + "\n")
            f.flush()
        bench(args, emit)


if __name__ == "__main__":
    main()
