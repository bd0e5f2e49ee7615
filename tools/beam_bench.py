#!/usr/bin/env python3
"""Beam-search decode: what a token step costs next to the greedy step, and the bf16 noise floor its tests use.

  python tools/beam_bench.py [--reps 5] [--out profiles/beam_bench.txt]
      configs[1]'s architecture (ViT-B/16, 197 patches + 6L d512 decoder, V = 10000) in bf16, max_len 100, an END that
      is never produced (every row runs all 99 token steps):
        beam-256x3   generate_beam_batch, B = 256 images, beam_size 3 (768 rows)
        greedy-256   generate_batch, B = 256
        greedy-768   generate_batch, B = 768: the same GEMM and attention rows as beam-256x3, so beam / greedy-768
                     isolates the logits round trip, the selection and the ancestry gather
      A call also runs the encoder and the cross-attention K/V (256 images for the beam, 768 for greedy-768) and
      records its launch plan, so the step time is a DIFFERENCE: (call at max_len 100 - call at max_len 20) / 80,
      each call timed by a host clock around work that ends in a device synchronise. The three configurations run
      interleaved, `reps` times after a warm-up round; medians are reported.
  python tools/beam_bench.py --deviation
      Per fixture of tests/test_beam_gpu.py's bf16 test: the worst per-step deviation of the UNFUSED greedy decode
      (MIT_DECODE_FUSED=0, the step's f32 logits) from the model's teacher-forced full forward on the same ids,
      |log_softmax(decode)[token] - log_softmax(full)[token]|: BF16_STEP_DEV of that test.
Both append to --out."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-image-transformer_amd"))

import torch  # noqa: E402


def build_cfg1(vocab):
    import config
    from model import ImageToTextModel
    config.MEMORY_MODE = "patches"
    config.ENCODER_MODEL_NAME = "google/vit-base-patch16-224-in21k"
    m = ImageToTextModel(vocab, 512, 8, 6, 2048, 100, 0.1, 0, memory_mode="patches", dtype=torch.bfloat16, seed=42)
    m.eval()
    return m


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def bench(args, emit):
    m = build_cfg1(args.vocab)
    g = torch.Generator().manual_seed(5)
    images = torch.randn(768, 3, 224, 224, generator=g).cuda()
    never = args.vocab + 7
    long_, short = 100, 20
    runs = {
        "beam-256x3": lambda L: m.generate_beam_batch(images[:256], 2, never, max_len=L, beam_size=3),
        "greedy-256": lambda L: m.generate_batch(images[:256], 2, never, max_len=L),
        "greedy-768": lambda L: m.generate_batch(images, 2, never, max_len=L),
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
         f"repeats; step = (call at max_len {long_} - call at max_len {short}) / {long_ - short}")
    for k in runs:
        a, b = statistics.median(t[k][long_]), statistics.median(t[k][short])
        step[k] = 1e3 * (a - b) / (long_ - short)
        emit(f"  {k:11s} {step[k]:7.3f} ms per token step   (call: {1e3 * a:8.1f} ms at max_len {long_}, "
             f"{1e3 * b:7.1f} ms at {short}; spread of the long call {1e3 * min(t[k][long_]):.1f} .. "
             f"{1e3 * max(t[k][long_]):.1f} ms)")
    emit(f"  beam-256x3 / greedy-768 = {step['beam-256x3'] / step['greedy-768']:.3f}   "
         f"beam-256x3 / greedy-256 = {step['beam-256x3'] / step['greedy-256']:.3f}")


def deviation(args, emit):
    os.environ["MIT_DECODE_FUSED"] = "0"
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, ROOT)
    import test_beam_gpu as tb
    emit("bf16 unfused greedy decode (MIT_DECODE_FUSED=0) vs the teacher-forced full forward, worst per-step "
         "|log_softmax(decode)[token] - log_softmax(full)[token]|:")
    for name in tb.BF16_STEP_DEV:
        m, meta = tb._model(name, torch.bfloat16)
        imgs, L = tb._bf16_images(name, meta)
        imgs = imgs.cuda()
        B, V, dec = imgs.shape[0], m.decoder.V, m.decoder
        m.eval()
        with torch.no_grad():
            mem, mem_ld, S, _, _ = m._encode_memory(imgs.float())
            stt = dec.decode_begin(mem, mem_ld, S, B, L, 2, -1)
            assert not stt.fused
            got = []
            for p in range(L - 1):
                dec.decode_step(stt)
                lsm = torch.log_softmax(stt.logits[:, :V].float(), -1)
                got.append(lsm.gather(1, stt.ids[:, p + 1:p + 2]))
            got = torch.cat(got, 1)
            full = torch.log_softmax(m(imgs, stt.ids[:, :-1].contiguous()).float(), -1)
            want = full.gather(-1, stt.ids[:, 1:, None]).squeeze(-1)
        dev = (got - want).abs()
        emit(f"  {name:18s} B = {B:3d}, max_len {L}: worst {float(dev.max()):.3e}  (mean {float(dev.mean()):.2e})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--vocab", type=int, default=10000)
    ap.add_argument("--deviation", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beam_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("beam_bench: needs the GPU (there is no CPU timing)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        def emit(s):
            print(s, flush=True)
            f.write(s + "\n")
            f.flush()
        (deviation if args.deviation else bench)(args, emit)


if __name__ == "__main__":
    main()
