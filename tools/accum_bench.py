#!/usr/bin/env python3
"""What gradient accumulation costs: an optimizer step over k micro-batches against the same k train steps
without the accumulate launches, and mit_grad_accumulate's bandwidth beside adamw_kernel's.

  python tools/accum_bench.py [--k 4] [--steps 20] [--reps 5] [--out profiles/accum_bench.txt]
      configs[1] (ViT-B/16 patches + 6L d512 decoder, V = 10000) in bf16, dropout 0.1, B = 64, T = 64, in ONE process
      on ONE model (the same streams and buffers):
        accum     train_step_accum over k micro-batches + optimizer.step(5.0)
        baseline  k train_step calls + ONE optimizer.step(5.0): the unchanged code path, the same forwards,
                  backwards, encoder prefetches and optimizer work without the k accumulate launches (its gradient is
                  the last micro-batch's alone: a timing baseline, not a training recipe)
      Both are recorded once (native.record) after a warm-up and replayed, as bench.py replays its step; `steps`
      replays end in a device synchronise and are timed by a host clock; the two run interleaved, `reps` times;
      medians with the spread, and the difference per micro-batch.
      Then the kernels on their own, device events around `n` launches over the model's flat buffers (numel f32 each,
      two to five buffers: past the 256 MiB Infinity Cache): mit_grad_accumulate per mode (8 numel bytes FIRST, 12 numel
      ADD / LAST) and mit_adamw with the bf16 shadow (16 numel read + 14 numel written), GB/s = those bytes / time.
The measurement runs in a child process under `timeout`; the parent never opens the GPU."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-image-transformer_amd"))

B, T, VOCAB = 64, 64, 10000


def build():
    import torch
    import config
    import optim
    from model import ImageToTextModel
    config.MEMORY_MODE = "patches"
    config.ENCODER_MODEL_NAME = "google/vit-base-patch16-224-in21k"
    m = ImageToTextModel(VOCAB, 512, 8, 6, 2048, 100, 0.1, 0, memory_mode="patches", dtype=torch.bfloat16, seed=42)
    m.train()
    return m, optim.AdamW(m.store, lr=1e-4)


def micro_batches(k, image):
    import torch
    g = torch.Generator().manual_seed(1000)
    out = []
    for _ in range(k):
        cap = torch.randint(4, VOCAB, (B, T + 1), generator=g)
        cap[:, 0] = 2
        out.append((torch.randn(B, 3, image, image, generator=g).cuda(), cap[:, :-1].contiguous().cuda(),
                    cap[:, 1:].contiguous().cuda()))
    return out


def steps(args, emit):
    import torch
    import native
    k = args.k
    m, opt = build()
    mbs = micro_batches(k, m.encoder.image)

    def accum():
        m.train_step_accum(mbs, next_images=mbs[0][0])
        opt.step(5.0)

    def baseline():
        for i, (im, di, tg) in enumerate(mbs):
            m.train_step(im, di, tg, next_images=mbs[(i + 1) % k][0])
        opt.step(5.0)

    # ONE model for both, so they share streams, hardware queues and buffers. Either step leaves the encoder of
    # mbs[0] prefetched in the same arena (k is even), so the recorded programs replay in any order.
    progs = {}
    for name, fn in (("accum", accum), ("baseline", baseline)):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        progs[name] = native.record(fn)
        torch.cuda.synchronize()

    def timed(name):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            opt._sync_lr()
            progs[name].run()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps

    for name in progs:  # warm-up of the replays
        timed(name)
    t = {name: [] for name in progs}
    for _ in range(args.reps):
        for name in progs:
            t[name].append(timed(name))
    med = {n: statistics.median(v) for n, v in t.items()}
    emit(f"configs[1] bf16, dropout 0.1, B = {B}, T = {T}, k = {k} micro-batches per optimizer step; recorded once and "
         f"replayed ({progs['accum'].launches()} / {progs['baseline'].launches()} launches per step); {args.steps} steps "
         f"per window, host clock to a device synchronise, {args.reps} interleaved repeats, medians (spread)")
    for n in ("accum", "baseline"):
        emit(f"  {n:8s}: {1e3 * med[n]:8.3f} ms per optimizer step  ({1e3 * min(t[n]):.3f} .. {1e3 * max(t[n]):.3f} ms)  "
             f"= {1e3 * med[n] / k:.3f} ms per micro-batch")
    d = med["accum"] - med["baseline"]
    emit(f"  accum - baseline = {1e3 * d:+.3f} ms per optimizer step = {1e3 * d / k:+.3f} ms per micro-batch "
         f"({100 * d / med['baseline']:+.2f} % of the baseline step)")
    return m


def kernels(args, emit, m):
    import torch
    import native
    st = m.store
    n, reps = st.numel, args.n
    bufs = [torch.randn(n, dtype=torch.float32, device="cuda") * 1e-3 for _ in range(4)]
    bufs[3].abs_()  # second moment
    shadow = torch.empty(n, dtype=torch.bfloat16, device="cuda")
    lr = torch.full((1,), 1e-4, dtype=torch.float32, device="cuda")
    step = torch.ones(1, dtype=torch.int64, device="cuda")

    def event_time(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return 1e-3 * e0.elapsed_time(e1) / reps

    emit(f"kernels on their own over numel = {n} f32 ({4 * n / 1e6:.1f} MB a buffer), device events around {reps} "
         f"launches, {native.grad_accumulate_blocks(n)} blocks of 256 threads:")
    rates = {}
    for name, mode, nb in (("FIRST", native.ACC_FIRST, 8), ("ADD", native.ACC_ADD, 12), ("LAST", native.ACC_LAST, 12)):
        dt = event_time(lambda: native.grad_accumulate(bufs[0], bufs[1], mode))
        rates[name] = nb * n / dt
        emit(f"  mit_grad_accumulate {name:5s}: {1e6 * dt:8.1f} us   {nb * n / 1e6:7.1f} MB   {rates[name] / 1e9:7.0f} GB/s")
    dt = event_time(lambda: native.adamw(bufs[0], bufs[1], bufs[2], bufs[3], shadow, None, lr, step, 0.9, 0.98, 1e-9, 1e-5))
    ad = 30 * n / dt
    emit(f"  mit_adamw (bf16 shadow)  : {1e6 * dt:8.1f} us   {30 * n / 1e6:7.1f} MB   {ad / 1e9:7.0f} GB/s")
    worst = min(rates.values())
    emit(f"  slowest accumulate mode / adamw_kernel = {worst / ad:.2f} of its bytes/s"
         + ("" if worst >= 0.5 * ad else "  (UNDER HALF: see DESIGN.md)"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20, help="optimizer steps per timed window")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=50, help="launches inside a device-event window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accum_bench.txt"))
    ap.add_argument("--child", action="store_true", help="measure in this process (the parent starts it)")
    ap.add_argument("--limit", type=int, default=420, help="seconds the measurement may take")
    args = ap.parse_args()
    if args.k < 2 or args.k % 2:
        ap.error("--k must be even: ONE recorded step is replayed, and the encoder prefetch alternates between two "
                 "arenas per micro-batch")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if not args.child:
        with open(args.out, "w") as f:
            f.write("# tools/accum_bench.py on one MI355X (gradient accumulation: model.train_step_accum, "
                    "csrc/misc.hip grad_accumulate_kernel)\n")
        rc = subprocess.call(["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child",
                              "--k", str(args.k), "--steps", str(args.steps), "--reps", str(args.reps), "--n", str(args.n),
                              "--out", args.out])
        if rc != 0:
            sys.exit(f"accum_bench: the measurement ended with status {rc}")
        return
    import torch
    if not torch.cuda.is_available():
        sys.exit("accum_bench: needs the GPU (there is no CPU timing)")
    with open(args.out, "a") as f:
        def emit(s):
            print(s, flush=True)
            f.write(s + "\n")
            f.flush()
        kernels(args, emit, steps(args, emit))


if __name__ == "__main__":
    main()
