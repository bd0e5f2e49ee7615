"""Caption generation from a trained checkpoint (reference inference.py), batched on the MI355X path.

The reference captions one image per call: model.generate() greedy decode with a full-prefix
recompute per token (inference.py:84-91 -> model.py:171-242), then trims the ids at the first END,
drops a leading START (inference.py:98-115) and cleans the decoded text (inference.py:116-126).
Here the same ids come from ImageToTextModel.generate_batch (KV cache, one hipGraph-replayed token
step for the whole batch, decode.hip); postprocess_ids / clean_text restate the reference's
post-processing so a batch yields the reference's caption for every image.
"""
from __future__ import annotations

import argparse
import json
import os
from typing import Callable, List, Optional, Sequence

import torch

import config


def postprocess_ids(ids: Sequence[int], start_token_id: int, end_token_id: int) -> List[int]:
    """inference.py:98-113: keep the ids before the first END (all of them when there is none),
    then drop one leading START."""
    ids = list(ids)
    if end_token_id in ids:
        ids = ids[:ids.index(end_token_id)]
    if ids and ids[0] == start_token_id:
        ids = ids[1:]
    return ids


def clean_text(text: str, unk_token: str = config.UNK_TOKEN) -> str:
    """inference.py:120-126: remove every UNK token string, strip, collapse runs of whitespace."""
    return " ".join(text.replace(unk_token, "").strip().split())


def load_model(checkpoint_path: str, vocab_size: Optional[int] = None, device=None, dtype=None,
               memory_mode: Optional[str] = None):
    """inference.py:52-68: build ImageToTextModel with config's decoder geometry and load the weights.
    .safetensors (the reference's format) or a .pt written by train.save_checkpoint, read with
    torch.load(weights_only=True) — nothing in the file is executed."""
    from model import ImageToTextModel
    if not os.path.exists(checkpoint_path):
        raise FileNotFoundError(f"Checkpoint file not found: {checkpoint_path}")
    if checkpoint_path.endswith(".safetensors"):
        from safetensors.torch import load_file
        sd = load_file(checkpoint_path)
    else:
        ck = torch.load(checkpoint_path, map_location="cpu", weights_only=True)
        sd = ck.get("model_state_dict", ck)
    if vocab_size is None:
        vocab_size = sd["decoder.fc_out.weight"].shape[0] if "decoder.fc_out.weight" in sd else config.VOCAB_SIZE
    model = ImageToTextModel(vocab_size, config.DECODER_EMBED_DIM, config.DECODER_HEADS, config.DECODER_LAYERS,
                             config.DECODER_FF_DIM, config.MAX_SEQ_LEN, config.DECODER_DROPOUT, config.PAD_TOKEN_ID,
                             device=device, dtype=dtype, memory_mode=memory_mode)
    model.load_state_dict(sd)
    model.eval()
    return model


def generate_captions(model, images, decode: Optional[Callable[[List[int]], str]] = None,
                      start_token_id: int = config.START_TOKEN_ID, end_token_id: int = config.END_TOKEN_ID,
                      max_len: int = config.MAX_SEQ_LEN, batch_size: int = 256, beam_size: Optional[int] = None,
                      length_penalty: float = 0.0, temperature: Optional[float] = None, top_k: int = 0,
                      top_p: float = 1.0, seed: int = 0, repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0,
                      min_length: int = 0, suppress_tokens=(), prompts=None, kv_dtype: Optional[str] = None,
                      rolling_slots: Optional[int] = None, stream_slots: Optional[int] = None):
    """Captions for a list of PIL images / HWC arrays or a [B,3,H,W] pixel tensor, `batch_size` images
    per batched decode. Returns [(processed ids, text)] — text is None without a `decode` function
    (the BPE tokenizer, tokenizer.py, is a host-side library outside this path).
    beam_size: None decodes greedily (generate_batch); a number decodes with that many beams per image
    (generate_beam_batch, ranked by score / length**length_penalty) and post-processes the best beam alike.
    temperature: a number draws each caption from the model's distribution instead (generate_sample_batch with
    top_k / top_p / seed; one sample per image). Image i of `images` draws with (seed, i) whatever the
    batch_size, so the captions do not depend on how the images are batched.
    repetition_penalty / no_repeat_ngram_size / min_length / suppress_tokens / prompts: the decode constraints of
    generate_batch, generate_beam_batch and generate_sample_batch alike (defaults: off, and then not passed on).
    prompts is one token list for every image or one list per image of `images`; a prompt's tokens are part of the
    processed ids and so of the text.
    kv_dtype: "bf16" or "fp8", how the decode holds the cross-attention K/V (generate_batch); passed on only when
    given, as the constraints are.
    rolling_slots: a number decodes greedily with rolling batching (generate_rolling_iter: that many decode slots,
    a finished caption's slot handed to the next image; `batch_size` images per encoder chunk): the same
    (ids, text) list, sooner when the captions' lengths differ. It excludes beam_size, temperature and every decode
    constraint.
    stream_slots: a number decodes with rolling batching on that many slots whatever the request is -- greedy,
    sampled (temperature, top_k, top_p, seed; one sample per image) or constrained (every constraint above, prompts
    per image included) -- through generate_stream_iter; `batch_size` images per encoder chunk. The (ids, text) list
    is the one the batch_size path returns. It excludes beam_size and rolling_slots."""
    if stream_slots is not None:
        if beam_size is not None:
            raise ValueError("generate_captions: stream_slots decodes greedily or by sampling; it excludes beam_size "
                             "(the beams of an image interact)")
        if rolling_slots is not None:
            raise ValueError("generate_captions: choose rolling_slots or stream_slots, not both")
        if isinstance(images, torch.Tensor):
            pv = images if images.dim() == 4 else images.unsqueeze(0)
        else:
            pv = model.image_processor(images=list(images), return_tensors="pt")["pixel_values"]
        kw = dict(slots=stream_slots, encode_batch=batch_size, temperature=temperature, top_k=top_k, top_p=top_p,
                  seed=seed, repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size,
                  min_length=min_length, suppress_tokens=tuple(suppress_tokens or ()), prompts=prompts)
        if kv_dtype is not None:
            kw["kv_dtype"] = kv_dtype
        got = {i: ids for i, _, ids, _ in
               model.generate_stream_iter((pv[i:i + batch_size] for i in range(0, pv.shape[0], batch_size)),
                                          start_token_id, end_token_id, max_len=max_len, **kw)}
        out = []
        for i in range(pv.shape[0]):
            p = postprocess_ids(got[i], start_token_id, end_token_id)
            out.append((p, clean_text(decode(p)) if decode is not None else None))
        return out
    if rolling_slots is not None:
        if beam_size is not None or temperature is not None or repetition_penalty != 1.0 or no_repeat_ngram_size \
                or min_length or suppress_tokens or prompts:
            raise ValueError("generate_captions: rolling_slots is the greedy decode; it excludes beam_size, "
                             "temperature and the decode constraints")
        if isinstance(images, torch.Tensor):
            pv = images if images.dim() == 4 else images.unsqueeze(0)
        else:
            pv = model.image_processor(images=list(images), return_tensors="pt")["pixel_values"]
        kw = {} if kv_dtype is None else {"kv_dtype": kv_dtype}
        got = dict(model.generate_rolling_iter((pv[i:i + batch_size] for i in range(0, pv.shape[0], batch_size)),
                                               start_token_id, end_token_id, max_len=max_len, slots=rolling_slots,
                                               encode_batch=batch_size, **kw))
        out = []
        for i in range(pv.shape[0]):
            p = postprocess_ids(got[i], start_token_id, end_token_id)
            out.append((p, clean_text(decode(p)) if decode is not None else None))
        return out
    cons = {}
    if kv_dtype is not None:
        cons["kv_dtype"] = kv_dtype
    if repetition_penalty != 1.0:
        cons["repetition_penalty"] = repetition_penalty
    if no_repeat_ngram_size:
        cons["no_repeat_ngram_size"] = no_repeat_ngram_size
    if min_length:
        cons["min_length"] = min_length
    if suppress_tokens:
        cons["suppress_tokens"] = tuple(suppress_tokens)
    per_image = bool(prompts) and all(isinstance(p, (list, tuple)) for p in prompts)
    if temperature is not None and beam_size is not None:
        raise ValueError("generate_captions: choose beam search (beam_size) or sampling (temperature), not both")
    if isinstance(images, torch.Tensor):
        pv = images if images.dim() == 4 else images.unsqueeze(0)
    else:
        pv = model.image_processor(images=list(images), return_tensors="pt")["pixel_values"]
    # at most two batches on the device: the current one and the next, whose encoder runs beside this
    # batch's token steps (generate_batch next_images); the next iteration passes that very tensor object,
    # which generate_batch recognises as prefetched
    starts = list(range(0, pv.shape[0], batch_size))

    def dev(i):
        return pv[i:i + batch_size].to(model.device).float()
    out = []
    chunk = dev(starts[0]) if starts else None
    for j in range(len(starts)):
        nxt = dev(starts[j + 1]) if j + 1 < len(starts) else None
        if prompts:  # a list per image is cut with the images
            cons["prompts"] = list(prompts[starts[j]:starts[j] + batch_size]) if per_image else list(prompts)
        if temperature is not None:
            ids = model.generate_sample_batch(chunk, start_token_id, end_token_id, max_len=max_len,
                                              temperature=temperature, top_k=top_k, top_p=top_p, seed=seed,
                                              image_offset=starts[j], **cons)
        elif beam_size is None:
            ids = model.generate_batch(chunk, start_token_id, end_token_id, max_len=max_len, next_images=nxt, **cons)
        else:
            ids = model.generate_beam_batch(chunk, start_token_id, end_token_id, max_len=max_len,
                                            beam_size=beam_size, length_penalty=length_penalty, **cons)
        chunk = nxt
        for seq in ids:
            p = postprocess_ids(seq, start_token_id, end_token_id)
            out.append((p, clean_text(decode(p)) if decode is not None else None))
    return out


def rank_scores(logprobs: Sequence[float], tokens: Sequence[int], length_penalty: float = 0.0):
    """One image's candidates, best first: (candidate index, logprob, tokens, logprob / tokens**length_penalty),
    ordered by the last entry descending, ties to the lower index (model.rank_beams' rule)."""
    rows = [(c, float(lp), int(n), float(lp) / max(int(n), 1) ** length_penalty)
            for c, (lp, n) in enumerate(zip(logprobs, tokens))]
    return sorted(rows, key=lambda r: (-r[3], r[0]))


def score_captions(model, images, candidates, batch_size: int = 256, length_penalty: float = 0.0, *,
                   start_token_id: int = config.START_TOKEN_ID, end_token_id: int = config.END_TOKEN_ID):
    """Rank given candidate captions per image by the model's teacher-forced log-likelihood
    (ImageToTextModel.score_captions). images: PIL images / HWC arrays or a [B,3,H,W] pixel tensor, `batch_size`
    images per call, as generate_captions batches them. candidates: one flat list of candidate id lists scored
    against every image (zero-shot classification by prompt, retrieval), or one such list per image (re-ranking
    an image's own samples), or an int64 [B, C, L] tensor padded with PAD; a list or tensor per image is cut with
    the images. Returns per image rank_scores' list, best first. A candidate's score does not depend on which
    images share its batch."""
    if isinstance(images, torch.Tensor):
        pv = images if images.dim() == 4 else images.unsqueeze(0)
    else:
        pv = model.image_processor(images=list(images), return_tensors="pt")["pixel_values"]
    per_image = isinstance(candidates, torch.Tensor) or \
        any(len(c) > 0 and isinstance(c[0], (list, tuple)) for c in candidates)
    if per_image and len(candidates) != pv.shape[0]:
        raise ValueError(f"score_captions: {len(candidates)} candidate lists for {pv.shape[0]} images")
    out = []
    for i in range(0, pv.shape[0], batch_size):
        chunk = pv[i:i + batch_size].to(model.device).float()
        cand = candidates[i:i + batch_size] if per_image else candidates
        lp, n, _ = model.score_captions(chunk, cand, start_token_id, end_token_id)
        for lps, ns in zip(lp.tolist(), n.tolist()):
            out.append(rank_scores(lps, ns, length_penalty))
    return out


def generate_caption(image, model, decode=None) -> str:
    """inference.py:17-128 for one image (path, PIL image or pixel tensor) with a loaded model."""
    if isinstance(image, str):
        if not os.path.exists(image):
            raise FileNotFoundError(f"Image file not found: {image}")
        from PIL import Image
        image = Image.open(image).convert("RGB")
    ids, text = generate_captions(model, image if isinstance(image, torch.Tensor) else [image], decode)[0]
    return text if text is not None else " ".join(map(str, ids))


def _tokenizer_decode():
    """The trained BPE tokenizer's decode when its files exist (config.VOCAB_PATH / MERGES_PATH), else None."""
    vocab, merges = getattr(config, "VOCAB_PATH", None), getattr(config, "MERGES_PATH", None)
    if not vocab or not merges or not (os.path.exists(vocab) and os.path.exists(merges)):
        return None
    from tokenizers import ByteLevelBPETokenizer
    tok = ByteLevelBPETokenizer(vocab, merges)
    return lambda ids: tok.decode(ids, skip_special_tokens=False)


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Generate captions for images with a trained checkpoint.")
    ap.add_argument("--image_path", nargs="+", required=True, help="one or more image files")
    ap.add_argument("--checkpoint_path", required=True, help=".safetensors or .pt checkpoint")
    ap.add_argument("--batch_size", type=int, default=256)
    ap.add_argument("--beam_size", type=int, default=None, help="beam search with this many beams per image")
    ap.add_argument("--length_penalty", type=float, default=0.0,
                    help="beams are ranked by score / length**length_penalty")
    ap.add_argument("--temperature", type=float, default=None,
                    help="sample each caption at this temperature instead of decoding greedily")
    ap.add_argument("--top_k", type=int, default=0, help="sampling: keep the k most likely tokens (0: all)")
    ap.add_argument("--top_p", type=float, default=1.0, help="sampling: keep the smallest set of this mass (1: all)")
    ap.add_argument("--seed", type=int, default=0, help="sampling seed")
    ap.add_argument("--repetition_penalty", type=float, default=1.0,
                    help="divide (positive) / multiply (other) the logit of every token a caption already holds")
    ap.add_argument("--no_repeat_ngram_size", type=int, default=0, help="no n-gram of this size occurs twice (0: off)")
    ap.add_argument("--min_length", type=int, default=0, help="no END before this many generated tokens")
    ap.add_argument("--suppress_tokens", type=int, nargs="*", default=[], help="token ids that are never picked")
    ap.add_argument("--prompt_ids", type=int, nargs="*", default=[], help="token ids every caption starts with")
    ap.add_argument("--kv_dtype", choices=["bf16", "fp8"], default=None,
                    help="storage of the cross-attention K/V: fp8 halves its memory and the bytes a token step streams "
                         "(bf16 checkpoints; default: env MIT_DECODE_KV, else bf16)")
    ap.add_argument("--rolling_slots", type=int, default=None,
                    help="greedy decode with rolling batching on this many slots: a finished caption's slot goes to "
                         "the next image (excludes --beam_size, --temperature and the constraints)")
    ap.add_argument("--stream_slots", type=int, default=None,
                    help="rolling batching on this many slots for greedy, sampled (--temperature) and constrained "
                         "requests alike (excludes --beam_size and --rolling_slots)")
    ap.add_argument("--score_file", default=None,
                    help="score instead of generating: a JSON file holding one list of candidate id lists (scored "
                         "against every image) or one such list per image; prints each image's ranking")
    return ap


def load_score_file(path: str):
    """The candidates of --score_file: a JSON list of candidate id lists, or a list of such lists (one per image)."""
    with open(path) as f:
        cands = json.load(f)
    if not isinstance(cands, list) or not cands or not all(isinstance(c, list) for c in cands):
        raise ValueError(f"{path}: expected a JSON list of candidate id lists, or one such list per image")
    return cands


def decode_options(args) -> dict:
    """The parsed command line as generate_captions keyword arguments; a decode constraint is carried where the
    command line sets it (left at its default it is off, and generate_captions' own default says the same)."""
    o = dict(batch_size=args.batch_size, beam_size=args.beam_size, length_penalty=args.length_penalty,
             temperature=args.temperature, top_k=args.top_k, top_p=args.top_p, seed=args.seed)
    if args.repetition_penalty != 1.0:
        o["repetition_penalty"] = args.repetition_penalty
    if args.no_repeat_ngram_size:
        o["no_repeat_ngram_size"] = args.no_repeat_ngram_size
    if args.min_length:
        o["min_length"] = args.min_length
    if args.suppress_tokens:
        o["suppress_tokens"] = tuple(args.suppress_tokens)
    if args.prompt_ids:
        o["prompts"] = list(args.prompt_ids)
    if args.kv_dtype is not None:
        o["kv_dtype"] = args.kv_dtype
    if args.rolling_slots is not None:
        o["rolling_slots"] = args.rolling_slots
    if args.stream_slots is not None:
        o["stream_slots"] = args.stream_slots
    return o


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.temperature is not None and args.beam_size is not None:
        ap.error("--beam_size and --temperature exclude each other")
    if args.stream_slots is not None and (args.beam_size is not None or args.rolling_slots is not None):
        ap.error("--stream_slots excludes --beam_size and --rolling_slots")
    if args.score_file is not None and (args.temperature is not None or args.beam_size is not None):
        ap.error("--score_file scores given captions: it excludes --beam_size and --temperature")
    from PIL import Image
    model = load_model(args.checkpoint_path)
    for p in args.image_path:
        if not os.path.exists(p):
            raise FileNotFoundError(f"Image file not found: {p}")
    ims = [Image.open(p).convert("RGB") for p in args.image_path]
    if args.score_file is not None:
        ranked = score_captions(model, ims, load_score_file(args.score_file), batch_size=args.batch_size,
                                length_penalty=args.length_penalty)
        for p, rows in zip(args.image_path, ranked):
            print(f"{p}:")
            for c, lp, n, s in rows:
                print(f"  candidate {c}: logprob {lp:.4f} over {n} tokens, score {s:.4f}")
        return
    for p, (ids, text) in zip(args.image_path, generate_captions(model, ims, _tokenizer_decode(),
                                                                  **decode_options(args))):
        print(f"{p}: {text if text is not None else ids}")


if __name__ == "__main__":
    main()
