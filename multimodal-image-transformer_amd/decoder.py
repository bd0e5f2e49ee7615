"""Transformer decoder (reference decoder.py:75-193) with an explicit forward/backward on the
gfx950 kernels.

Semantics reproduced exactly (post-LN nn.TransformerDecoderLayer, torch/nn/modules/transformer.py
:1131-1199, built at decoder.py:112-120):
    x  = dropout(Emb[tok] * sqrt(d) + PE[t])                                  decoder.py:168-171
    x  = LN1(x + dropout(SelfAttn(x; causal + key-padding mask, attn dropout)))
    x  = LN2(x + dropout(CrossAttn(x, memory; attn dropout)))
    x  = LN3(x + dropout(W2 dropout(relu(W1 x + b1)) + b2))
    logits = x Wfc^T + bfc                                                   decoder.py:191
MHA uses a packed in_proj (q,k,v rows), scale 1/sqrt(head_dim) (torch/nn/functional.py:6435).

MI355X-specific layout decisions:
  * the cross-attention K/V projections of ALL layers only depend on the memory, so they are one
    GEMM  kv_all[B*S, L*2d] = memory @ W_kv_all^T  (N = 6144 at cfg1) in the forward, and one
    dW GEMM + one dX GEMM in the backward (the reference issues 2 x L smaller ones);
  * the masks are never materialised (computed in-kernel from tokens == PAD and j > i);
  * dropout masks are regenerated from (seed, site, index) in the backward, never stored;
  * weight gradients are written ONCE (no zero-fill + accumulate), straight into the flat f32
    gradient buffer (params.FlatParams) in backward-completion order.
"""
from __future__ import annotations

import math
import os
from typing import Callable, Dict, List, Optional, Tuple

import torch

import native
from params import FlatParams

EMB_SITE = 4000


def sinusoidal_pe(max_len: int, d: int) -> torch.Tensor:
    """The PositionalEncodingBatchFirst buffer (decoder.py:34-47), [max_len, d] f32."""
    pos = torch.arange(max_len).unsqueeze(1)
    div = torch.exp(torch.arange(0, d, 2) * (-math.log(10000.0) / d))
    pe = torch.zeros(max_len, d)
    pe[:, 0::2] = torch.sin(pos * div)
    pe[:, 1::2] = torch.cos(pos * div)
    return pe


def padded_vocab(V: int) -> int:
    """The vocabulary head is stored with Vp = round8(V) rows: the bf16 GEMMs need the contiguous
    extent of every operand (the fc_out weight gradient has M = V, lda = V) to be a multiple of 8,
    and the reference sizes V from the trained tokenizer (tokenizer.py:200-201, any size). The pad
    rows of fc_out are zero and stay zero (their gradient is exactly 0, so AdamW never moves them);
    the pad logit columns are 0 and never reach the caller, the loss or argmax."""
    return (V + 7) // 8 * 8


def decoder_entries(V: int, d: int, L: int, F: int, proj_in: Optional[int]) -> List[Tuple[str, Tuple[int, ...]]]:
    """Flat-buffer layout in backward-completion order (see params.py)."""
    Vp = padded_vocab(V)
    e = [("fc_out.weight", (Vp, d)), ("fc_out.bias", (Vp,))]
    for i in reversed(range(L)):
        p = f"layers.{i}."
        e += [(p + "linear2.weight", (d, F)), (p + "linear2.bias", (d,)), (p + "linear1.weight", (F, d)),
              (p + "linear1.bias", (F,)), (p + "norm3.weight", (d,)), (p + "norm3.bias", (d,)),
              (p + "cross_out.weight", (d, d)), (p + "cross_out.bias", (d,)), (p + "cross_q.weight", (d, d)),
              (p + "cross_q.bias", (d,)), (p + "norm2.weight", (d,)), (p + "norm2.bias", (d,)),
              (p + "self_out.weight", (d, d)), (p + "self_out.bias", (d,)), (p + "self_in.weight", (3 * d, d)),
              (p + "self_in.bias", (3 * d,)), (p + "norm1.weight", (d,)), (p + "norm1.bias", (d,))]
    e += [("cross_kv.weight", (L * 2 * d, d)), ("cross_kv.bias", (L * 2 * d,)), ("token_embedding.weight", (V, d))]
    if proj_in is not None:
        e += [("projection.weight", (d, proj_in)), ("projection.bias", (d,))]
    return e


def reference_to_flat(sd: Dict[str, torch.Tensor], L: int, d: int, prefix: str = "decoder.") -> Dict[str, torch.Tensor]:
    """Reference state_dict names (decoder.* / projection.*) -> flat entry names."""
    out = {}
    kv_w, kv_b = [None] * L, [None] * L
    for k, v in sd.items():
        if k.startswith("projection."):
            out[k] = v
            continue
        if not k.startswith(prefix):
            continue
        k = k[len(prefix):]
        if k in ("fc_out.weight", "fc_out.bias", "token_embedding.weight"):
            out[k] = v
        elif k.startswith("transformer_decoder.layers."):
            rest = k[len("transformer_decoder.layers."):]
            i, sub = rest.split(".", 1)
            i = int(i)
            p = f"layers.{i}."
            if sub == "self_attn.in_proj_weight":
                out[p + "self_in.weight"] = v
            elif sub == "self_attn.in_proj_bias":
                out[p + "self_in.bias"] = v
            elif sub.startswith("self_attn.out_proj."):
                out[p + "self_out." + sub.rsplit(".", 1)[1]] = v
            elif sub == "multihead_attn.in_proj_weight":
                out[p + "cross_q.weight"] = v[:d]
                kv_w[i] = v[d:]
            elif sub == "multihead_attn.in_proj_bias":
                out[p + "cross_q.bias"] = v[:d]
                kv_b[i] = v[d:]
            elif sub.startswith("multihead_attn.out_proj."):
                out[p + "cross_out." + sub.rsplit(".", 1)[1]] = v
            else:  # linear1/linear2/norm1-3
                out[p + sub] = v
    if all(x is not None for x in kv_w):
        out["cross_kv.weight"] = torch.cat(kv_w, 0)
    if all(x is not None for x in kv_b):
        out["cross_kv.bias"] = torch.cat(kv_b, 0)
    return out


def flat_to_reference(store: FlatParams, L: int, d: int, prefix: str = "decoder.") -> Dict[str, torch.Tensor]:
    """Inverse of reference_to_flat: the reference's state_dict keys (§8b), f32 copies."""
    sd = {}
    p = lambda n: store.p(n).detach().clone()  # noqa: E731
    kvw, kvb = store.p("cross_kv.weight"), store.p("cross_kv.bias")
    sd[prefix + "token_embedding.weight"] = p("token_embedding.weight")
    for i in range(L):
        r, q = f"{prefix}transformer_decoder.layers.{i}.", f"layers.{i}."
        sd[r + "self_attn.in_proj_weight"] = p(q + "self_in.weight")
        sd[r + "self_attn.in_proj_bias"] = p(q + "self_in.bias")
        sd[r + "self_attn.out_proj.weight"] = p(q + "self_out.weight")
        sd[r + "self_attn.out_proj.bias"] = p(q + "self_out.bias")
        sd[r + "multihead_attn.in_proj_weight"] = torch.cat([p(q + "cross_q.weight"), kvw[i * 2 * d:(i + 1) * 2 * d]], 0)
        sd[r + "multihead_attn.in_proj_bias"] = torch.cat([p(q + "cross_q.bias"), kvb[i * 2 * d:(i + 1) * 2 * d]], 0)
        sd[r + "multihead_attn.out_proj.weight"] = p(q + "cross_out.weight")
        sd[r + "multihead_attn.out_proj.bias"] = p(q + "cross_out.bias")
        for s in ("linear1", "linear2", "norm1", "norm2", "norm3"):
            sd[r + s + ".weight"] = p(q + s + ".weight")
            sd[r + s + ".bias"] = p(q + s + ".bias")
    V = getattr(store, "vocab", None)
    sd[prefix + "fc_out.weight"] = p("fc_out.weight")[:V]
    sd[prefix + "fc_out.bias"] = p("fc_out.bias")[:V]
    return sd


class _Acts:
    """Activation arena for one (B, T, S, train) shape; allocated once, reused every step."""

    def __init__(self, B, T, S, d, F, L, V, H, dt, dev, train: bool, proj_in: Optional[int] = None):
        R = B * T
        e = lambda *s: torch.empty(*s, dtype=dt, device=dev)  # noqa: E731
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)  # noqa: E731
        self.R = R
        self.x0 = e(R, d)
        self.y = e(R, d)
        self.kv = e(B * S, L * 2 * d)
        self.logits = e(R, padded_vocab(V))  # padded head columns: row stride Vp
        nl = L if train else 1  # eval keeps one set of per-layer buffers and reuses it
        self.qkv = [e(R, 3 * d) for _ in range(nl)]
        self.os = [e(R, d) for _ in range(nl)]
        self.oc = [e(R, d) for _ in range(nl)]
        self.qc = [e(R, d) for _ in range(nl)]
        self.h = [e(R, F) for _ in range(nl)]
        self.z = [[e(R, d) for _ in range(3)] for _ in range(nl)]
        self.st = [[(f(R), f(R)) for _ in range(3)] for _ in range(nl)]
        self.lse_s = [f(B * H * T) for _ in range(nl)]
        self.lse_c = [f(B * H * T) for _ in range(nl)]
        # per-layer normalised outputs x1, x2, x3 (x3 of layer l = input of layer l+1)
        self.xs = [[e(R, d) for _ in range(3)] for _ in range(L if train else 2)]
        self.count_loss = f(2)  # {non-PAD target count, CE loss sum}: one memset per step
        self.count = self.count_loss[0:1]
        self.loss_sum = self.count_loss[1:2]
        self.loss = f(1)
        self.row_loss = f(R)  # per-row CE losses (deterministic loss sum)
        # split-K scratch of the main stream: the d_model GEMMs (R x d outputs, 128 tiles at B = 64)
        # combine their K slices in-launch; weight-gradient / long-K GEMMs reduce in a second launch.
        # Zero-filled once: its first 4 KiB are tile counters the kernels leave at zero.
        E = proj_in or d
        Vp = padded_vocab(V)
        shapes = [(R, d, d), (R, d, F), (R, d, 3 * d), (R, d, Vp)]
        if train:
            shapes += [(Vp, d, R), (d, F, R), (F, d, R), (d, d, R), (3 * d, d, R), (L * 2 * d, d, B * S), (d, E, B * S),
                       (B * S, d, L * 2 * d)]
        need = max(native.gemm_workspace_bytes(m, n, k) for m, n, k in shapes)
        self.gemm_ws = torch.zeros(max(need, 4096) // 4 + 4, dtype=torch.float32, device=dev)
        if train:
            self.dx = e(R, d)
            self.dy = e(R, d)
            self.do = e(R, d)
            self.dq = e(R, d)
            self.dqkv = e(R, 3 * d)
            self.dh = e(R, F)
            self.dkv = e(B * S, L * 2 * d)
            self.dmem = e(B * S, d)
            self.delta = f(B * H * T)
            self.ln_ws = f(native.layernorm_bwd_ws_floats(R, d))
            # one column-partial buffer per LayerNorm: their dgamma/dbeta reductions run on the
            # side stream, off the dX chain (run_backward)
            self.ln_ws_side = [f(native.layernorm_bwd_ws_floats(R, d)) for _ in range(3 * L)]
            # deterministic embedding-gradient order (native.embed_plan of the step's tokens)
            self.emb_plan = torch.empty(native.embed_plan_ints(R), dtype=torch.int32, device=dev)
            # the weight-gradient GEMMs run on a side stream (_SideStream) with their own scratch
            self.gemm_ws_side = torch.zeros(max(need, 4096) // 4 + 4, dtype=torch.float32, device=dev)
            # grouped per-layer dW (TransformerDecoder.dw_grouped): the six dY operands of a layer in their own
            # buffers, two sets (layer parity) so layer l's grouped launch overlaps layer l-1's dX chain
            self.gdy = [[e(R, d) for _ in range(3)] for _ in range(2)]
            self.gdh = [e(R, F) for _ in range(2)]
            self.gdq = [e(R, d) for _ in range(2)]
            self.gdqkv = [e(R, 3 * d) for _ in range(2)]
            self.gws = None  # allocated on first use (native.gemm_grouped_ws_bytes)
            self.gws_tail = None  # the cross-K/V + projection pair
            self.gws_kv = None  # the cross-K/V weight gradient alone (TransformerDecoder.kv_dw_early)


SCORE_LOGITS_BYTES = 32 << 20  # budget of run_score's head buffer (head_rows x Vp logits in the model dtype)


class _ScoreActs:
    """Activation arena of run_score for one (B, C, T, S, head_rows) shape: forward-only buffers over the
    B * C * T candidate rows, the cross-attention K/V of the B images, ONE head chunk of logits, and the scores."""

    def __init__(self, B, C, T, S, d, F, L, Vp, H, dt, dev, head_rows):
        R = B * C * T
        e = lambda *s: torch.empty(*s, dtype=dt, device=dev)  # noqa: E731
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)  # noqa: E731
        i = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)  # noqa: E731
        self.R, self.head_rows = R, head_rows
        self.x0, self.y = e(R, d), e(R, d)
        self.kv = e(B * S, L * 2 * d)
        self.qkv, self.os, self.oc, self.qc, self.h = e(R, 3 * d), e(R, d), e(R, d), e(R, d), e(R, F)
        self.xs = [[e(R, d) for _ in range(3)] for _ in range(2)]
        self.lse = f(B * C * H * T)
        self.logits = e(head_rows, Vp)
        self.token_logprob, self.rank = f(R), i(R)
        self.seq_logprob, self.seq_tokens, self.seq_hits = f(B * C), i(B * C), i(B * C)


class _SideStream:
    """Second HIP stream for the backward's weight-gradient GEMMs (dW = dY^T X). Each layer's dW
    and dX GEMMs are independent; at d = 512 a decoder GEMM fills only 128-512 of the CUs' 512
    block slots, so running the dW chain beside the main dX -> LayerNorm -> attention chain fills
    the machine. Ordering: side waits for main before each dW (its dY is final); main waits for the
    side's last reader of a gradient buffer before overwriting it (guard); join() at the end. All
    edges are HIP events, so the step still captures into ONE hipGraph (as parallel branches)."""

    def __init__(self, device, priority: int = 0):
        self.stream = torch.cuda.Stream(device=device, priority=priority)
        self.ptr = self.stream.cuda_stream
        self.events = native.HipEvents(64)  # recorded on the main stream (side waits for main)
        self.plan_events = native.HipEvents(2)  # the embedding plan (side) -> embedding backward (main)
        self.side_events = native.HipEvents(128)  # recorded on the side stream only: a recycled slot
        self.pending = {}                         # re-recorded later on the SAME stream stays a safe wait

    def run(self, fn, reads=()):
        """fn issues native launches only (routed by native.on_stream, no torch stream switch)."""
        self.events.wait_stream(self.ptr, native.stream_ptr())
        with native.on_stream(self.ptr):
            fn()
        if reads:
            ev = self.side_events.record(self.ptr)
            for t in reads:
                self.pending[t.data_ptr()] = ev

    def guard(self, t):
        """Before the main stream writes t: wait for the side-stream GEMM still reading it."""
        ev = self.pending.pop(t.data_ptr(), None)
        if ev is not None:
            native.HipEvents.wait(native.stream_ptr(), ev)

    def under(self, fn):
        """Run fn (e.g. a DP gradient-bucket all-reduce) on the side stream after everything issued
        so far on both streams (a host step of a recorded program: native.host_call)."""
        self.events.wait_stream(self.ptr, native.stream_ptr())

        def call():
            with torch.cuda.stream(self.stream):
                fn()
        native.host_call(call)

    def join(self):
        """The caller's stream waits for everything issued on the side stream."""
        native.HipEvents.wait(native.stream_ptr(), self.side_events.record(self.ptr))
        self.pending.clear()


class DecodeConstraints:
    """What a token step may not pick (csrc/constrain.hip, mit_logits_constrain): edits of the step's f32 logits row
    between the vocabulary head and the pick, the same for greedy, beam and sampled decoding. The picks treat the
    edited row as the model's logits: beam scores and sample log-probabilities are log_softmax of the constrained row.

      repetition_penalty  t > 0 (1: off): every distinct token of a row's history, START included, has its logit
                          divided by t when positive, multiplied by t otherwise
      no_repeat_ngram     n >= 0 (0: off): a token that would complete an n-gram the row already holds is banned
      min_length          END is banned while fewer than min_length tokens have been generated
      suppress            token ids that are never picked
      prompts             None, one token list for every image, or one list per image (empty: no prompt): the
                          tokens that follow START, forced at no cost in score or log-probability

    All defaults: active() is False and every decode takes the unconstrained code path, launch for launch."""

    def __init__(self, repetition_penalty: float = 1.0, no_repeat_ngram: int = 0, min_length: int = 0,
                 suppress=(), prompts=None):
        self.repetition_penalty = float(repetition_penalty)
        self.no_repeat_ngram = int(no_repeat_ngram)
        self.min_length = int(min_length)
        self.suppress = tuple(int(t) for t in (suppress if suppress is not None else ()))
        if prompts is not None:
            prompts = list(prompts)
            per_image = len(prompts) > 0 and all(isinstance(p, (list, tuple)) for p in prompts)
            prompts = [[int(t) for t in p] for p in prompts] if per_image else [int(t) for t in prompts]
        self.prompts = prompts

    def per_image(self) -> bool:
        return bool(self.prompts) and isinstance(self.prompts[0], list)

    def has_prompts(self) -> bool:
        return bool(self.prompts) and (not self.per_image() or any(self.prompts))

    def active(self) -> bool:
        return (self.repetition_penalty != 1.0 or self.no_repeat_ngram != 0 or self.min_length != 0
                or bool(self.suppress) or self.has_prompts())

    def image_prompts(self, B: int) -> List[List[int]]:
        """One prompt (possibly empty) per image of a batch of B."""
        if not self.prompts:
            return [[] for _ in range(B)]
        if not self.per_image():
            return [list(self.prompts) for _ in range(B)]
        if len(self.prompts) != B:
            raise ValueError(f"prompts: {len(self.prompts)} lists for {B} images")
        return [list(p) for p in self.prompts]

    def rows(self, lo: int, hi: int) -> "DecodeConstraints":
        """The constraints of images lo .. hi - 1 (generate_batch's row groups)."""
        pr = self.prompts[lo:hi] if self.per_image() else self.prompts
        return DecodeConstraints(self.repetition_penalty, self.no_repeat_ngram, self.min_length, self.suppress, pr)

    def validate(self, V: int, max_len: int, end_id: int, B: int):
        """Host checks against a vocabulary of V, a decode of B images to max_len ids and its END."""
        t = self.repetition_penalty
        if not (t > 0 and math.isfinite(t)):
            raise ValueError(f"repetition_penalty {t} must be positive and finite")
        if self.no_repeat_ngram < 0 or self.min_length < 0:
            raise ValueError(f"no_repeat_ngram {self.no_repeat_ngram} and min_length {self.min_length} must be >= 0")
        for v in self.suppress:
            if not 0 <= v < V:
                raise ValueError(f"suppress: token {v} outside the vocabulary [0, {V})")
        for p in self.image_prompts(B):
            if 1 + len(p) > max_len:
                raise ValueError(f"prompt of {len(p)} tokens does not fit in max_len {max_len} after START")
            for v in p:
                if not 0 <= v < V:
                    raise ValueError(f"prompt: token {v} outside the vocabulary [0, {V})")
                if v == end_id:
                    raise ValueError(f"prompt: contains END ({end_id})")


KV_DTYPES = ("bf16", "fp8")


def resolve_kv_dtype(kv_dtype: Optional[str] = None, dtype: torch.dtype = torch.bfloat16) -> str:
    """The storage of a decode's cross-attention K/V: the argument, else env MIT_DECODE_KV, else "bf16" (which
    means the decoder's own dtype: the state as it always was). "fp8": OCP e4m3fn bytes with a power-of-two scale
    per (layer, image, head) for K and one for V (csrc/kv8.hip), half the bytes every token step streams and half
    the memory a batch's K/V holds; bf16 decoders only."""
    v = kv_dtype if kv_dtype is not None else os.environ.get("MIT_DECODE_KV") or "bf16"
    if v not in KV_DTYPES:
        raise ValueError(f"kv_dtype {v!r}: choose one of {KV_DTYPES}")
    if v == "fp8" and dtype != torch.bfloat16:
        raise ValueError(f"kv_dtype 'fp8' needs a bfloat16 decoder (this one is {dtype}): the quantiser reads bf16 "
                         f"K/V rows and the FP8 attention kernels take bf16 queries; float32 is the parity mode")
    return v


class DecodeState:
    """Device state of a batched greedy decode (TransformerDecoder.decode_begin / decode_step):
    token ids [B, max_len] (int64; column 0 = START), the device position, per-row finished flags
    and their count, the cross-attention K/V of all layers [L, B*S, 2d] (or, with kv_dtype "fp8", its e4m3 bytes
    kv8 and the scales kv_scale [L, images, 2H]: K heads, then V heads), per-layer self-attention
    caches [B, max_len, 2d] (K | V), and the B-row activations of one token step."""

    kv: Optional[torch.Tensor] = None        # [L, images*S, 2d] in the decoder's dtype; None with kv_dtype "fp8"
    kv8: Optional[torch.Tensor] = None       # fp8: uint8 [L, images*S, 2d] (K | V as kv)
    kv_scale: Optional[torch.Tensor] = None  # fp8: f32 [L, images, 2H]
    K = 0  # beam slots per image (BeamState); 0: greedy rows
    group = 1  # rows that share one cross-attention memory (SampleState: the samples of an image)
    cons: Optional[DecodeConstraints] = None  # active constraints (TransformerDecoder._constrain_begin), else None
    suppress: Optional[torch.Tensor] = None   # with cons: the suppressed ids on the device (int64), or None
    forced: Optional[torch.Tensor] = None     # with cons: int64 [rows, Lp + 1], column j + 1 = prompt token j, -1 = free
    row_pos: Optional[torch.Tensor] = None    # RollingState: int64 [rows], one position per row (then pos is None)

    def __init__(self, dec: "TransformerDecoder", B: int, S: int, max_len: int, start_id: int, end_id: int,
                 images: Optional[int] = None, kv_dtype: Optional[str] = None, shared_pos: bool = True):
        """B rows; images: how many memories the cross-attention K/V holds (default: one per row); kv_dtype:
        resolve_kv_dtype; shared_pos = False (RollingState): no pos / finished / n_finished are allocated, the
        subclass holds a position per row instead."""
        dev, dt = dec.device, dec.dtype
        d, F, L, V = dec.d, dec.F, dec.L, dec.V
        self.kv_dtype = resolve_kv_dtype(kv_dtype, dt)
        self.B, self.S, self.max_len, self.end_id = B, S, max_len, int(end_id)
        self.ids = torch.full((B, max_len), dec.pad_idx, dtype=torch.int64, device=dev)
        self.ids[:, 0] = int(start_id)
        self.pos = self.finished = self.n_finished = None
        if shared_pos:
            self.pos = torch.zeros(1, dtype=torch.int64, device=dev)
            self.finished = torch.zeros(B, dtype=torch.int32, device=dev)
            self.n_finished = torch.zeros(1, dtype=torch.int32, device=dev)
        # per layer contiguous [L][B*S][2d] (K | V): a decode attention block (b, h) then reads its S keys
        # at a 2 KiB stride instead of the training layout's L * 2d row (12 KiB at cfg1), which left the
        # S = 197 cross attention at ~2.6 TB/s on DRAM page misses
        n_img = B if images is None else images
        if self.kv_dtype == "fp8":  # no bf16 K/V is held: each layer's rows pass through one staging buffer
            self.kv8 = torch.empty(L, n_img * S, 2 * d, dtype=torch.uint8, device=dev)
            self.kv_scale = torch.empty(L, n_img, 2 * dec.H, dtype=torch.float32, device=dev)
        else:
            self.kv = torch.empty(L, n_img * S, 2 * d, dtype=dt, device=dev)
        self.cache = [torch.empty(B, max_len, 2 * d, dtype=dt, device=dev) for _ in range(L)]
        e = lambda n: torch.empty(B, n, dtype=dt, device=dev)  # noqa: E731
        self.x, self.x1, self.x2, self.y, self.o, self.q = e(d), e(d), e(d), e(d), e(d), e(d)
        self.qkv, self.h = e(3 * d), e(F)
        self.logits = torch.empty(B, padded_vocab(V), dtype=torch.float32, device=dev)  # f32: argmax on unrounded logits
        # bf16 step with the LayerNorms folded into the GEMMs (native.decode_gemm): the three pre-LN sums
        # of a layer in f32 and their per-64-column row statistics; the pick advances pos via `ticket`
        self.fused = dt == torch.bfloat16 and os.environ.get("MIT_DECODE_FUSED", "1") != "0"
        if self.fused:
            P = (d + 63) // 64
            self.z = [torch.empty(B, d, dtype=torch.float32, device=dev) for _ in range(3)]
            self.zst = [torch.empty(B, P, 2, dtype=torch.float32, device=dev) for _ in range(3)]
            self.ticket = torch.zeros(1, dtype=torch.int32, device=dev)
            # the head's packed argmax, ARGMAX_SLOTS per row (0 between steps)
            self.keys = torch.zeros(native.ARGMAX_SLOTS * B, dtype=torch.int64, device=dev)

    def token_lists(self) -> List[List[int]]:
        """Per row: START .. up to and including the first END (model.py:236-242), else max_len ids."""
        out = []
        for row in self.ids.cpu().tolist():
            if self.end_id in row[1:]:
                row = row[: row.index(self.end_id, 1) + 1]
            out.append(row)
        return out


class BeamState(DecodeState):
    """Device state of a beam search (TransformerDecoder.beam_begin / beam_step): a DecodeState of R = images * K
    rows (row b*K + k is slot k of image b) whose caches and ids are SLOT-ORDERED -- row r, position j holds what
    slot r wrote at step j -- plus per slot the cumulative log-probability `score`, `length` (generated tokens,
    END included) and the ancestor table `anc` (int32 [R, max_len]): anc[r, j] is the slot of the same image whose
    row holds position j of the beam now in slot r. The cross-attention K/V holds one memory per image."""

    def __init__(self, dec: "TransformerDecoder", images: int, K: int, S: int, max_len: int, start_id: int,
                 end_id: int, kv_dtype: Optional[str] = None):
        super().__init__(dec, images * K, S, max_len, start_id, end_id, images=images, kv_dtype=kv_dtype)
        dev = dec.device
        self.images, self.K = images, K
        self.score = torch.full((images, K), float("-inf"), dtype=torch.float32, device=dev)
        self.score[:, 0] = 0.0
        self.score = self.score.view(-1)
        self.length = torch.zeros(images * K, dtype=torch.int32, device=dev)
        self.anc = torch.zeros(images * K, max_len, dtype=torch.int32, device=dev)
        self.anc[:, 0] = torch.arange(K, dtype=torch.int32, device=dev).repeat(images)
        self.ws = torch.empty((native.beam_select_ws_bytes(images, K, dec.V) + 7) // 8, dtype=torch.int64, device=dev)

    def beam_ids(self) -> torch.Tensor:
        """int64 [images, K, max_len]: each slot's own ids, gathered through the ancestor table (one gather)."""
        B, K, T = self.images, self.K, self.max_len
        return self.ids.view(B, K, T).gather(1, self.anc.view(B, K, T).long())

    def token_lists(self) -> List[List[int]]:
        """Per row (image-major, slot-minor) as DecodeState.token_lists: START .. first END inclusive, else max_len."""
        out = []
        for row in self.beam_ids().view(self.B, self.max_len).cpu().tolist():
            if self.end_id in row[1:]:
                row = row[: row.index(self.end_id, 1) + 1]
            out.append(row)
        return out


class SampleState(DecodeState):
    """Device state of a sampled decode (TransformerDecoder.sample_begin / sample_step): a DecodeState of
    R = images * N rows (row b*N + n is sample n of image b), each with its own self-attention cache, plus per
    row the cumulative log-probability `logprob` (f32, at temperature 1 over the unfiltered vocabulary) and
    `length` (generated tokens, END included), the device seed, the global index `row0` of row 0 and the filter
    settings. The cross-attention K/V holds one memory per image, read by its N samples (group = N)."""

    def __init__(self, dec: "TransformerDecoder", images: int, N: int, S: int, max_len: int, start_id: int,
                 end_id: int, temperature: float, top_k: int, top_p: float, seed: int, row0: int,
                 kv_dtype: Optional[str] = None):
        super().__init__(dec, images * N, S, max_len, start_id, end_id, images=images, kv_dtype=kv_dtype)
        dev = dec.device
        self.images, self.group = images, N
        self.temperature, self.top_k, self.top_p, self.row0 = float(temperature), int(top_k), float(top_p), int(row0)
        self.logprob = torch.zeros(images * N, dtype=torch.float32, device=dev)
        self.length = torch.zeros(images * N, dtype=torch.int32, device=dev)
        s = int(seed) & 0xFFFFFFFFFFFFFFFF  # the kernels read a uint64
        self.seed = torch.tensor([s - (1 << 64) if s >= (1 << 63) else s], dtype=torch.int64, device=dev)
        if not hasattr(self, "ticket"):  # the fused state has one already
            self.ticket = torch.zeros(1, dtype=torch.int32, device=dev)


class _PoolView:
    """The cross-attention K/V tensors of `n` pool images from pool index `at`, under the names _cross_kv_begin
    writes through (kv / kv8 / kv_scale of a DecodeState)."""

    def __init__(self, stt: "RollingState", at: int, n: int):
        S = stt.S
        self.kv = stt.pool_kv[:, at * S:(at + n) * S] if stt.pool_kv is not None else None
        self.kv8 = stt.pool_kv8[:, at * S:(at + n) * S] if stt.pool_kv8 is not None else None
        self.kv_scale = stt.pool_scale[:, at:at + n] if stt.pool_scale is not None else None


class RollingState(DecodeState):
    """Device state of a rolling-batch greedy decode (TransformerDecoder.rolling_begin / rolling_fill / rolling_admit
    / rolling_step): a DecodeState of `slots` rows in which every row has its OWN position. In place of pos /
    finished / n_finished it holds row_pos (int64 [slots]), done (int32 [slots]), n_done (int32 [1]) -- three views
    of one buffer `poll_dev`, so that a poll is one device-to-host copy -- and limit (int64 [slots], the ids a row
    may hold). A pool of `pool` images' cross-attention K/V (pool_kv, or pool_kv8 + pool_scale with kv_dtype "fp8")
    feeds the slots: mit_slot_admit copies an image's rows into a slot and resets the slot. Every slot starts EMPTY:
    done = 1, n_done = slots, K/V (and scales) zero, ids[:, 0] = START, so stepping an empty slot is finite
    arithmetic whose results nobody reads. stream (a dict of _stream_init's arguments; None: nothing more is
    allocated) opts into the state of sampled / constrained rolling decode."""

    def __init__(self, dec: "TransformerDecoder", slots: int, S: int, max_len: int, start_id: int, end_id: int,
                 pool: Optional[int] = None, kv_dtype: Optional[str] = None, stream: Optional[dict] = None):
        # no shared position: pos / finished / n_finished stay None, so no scalar-pos launch can be given one
        super().__init__(dec, slots, S, max_len, start_id, end_id, kv_dtype=kv_dtype, shared_pos=False)
        dev = dec.device
        self.slots, self.pool, self.start_id = slots, slots if pool is None else int(pool), int(start_id)
        # [row_pos: 8 * slots | done: 4 * slots | n_done: 4 | pad] bytes
        nb = 12 * slots + 8
        self.poll_dev = torch.zeros(nb, dtype=torch.uint8, device=dev)
        self.row_pos = self.poll_dev[:8 * slots].view(torch.int64)
        self.done = self.poll_dev[8 * slots:12 * slots].view(torch.int32)
        self.n_done = self.poll_dev[12 * slots:12 * slots + 4].view(torch.int32)
        self.done.fill_(1)
        self.n_done.fill_(slots)
        self.poll_host = torch.zeros(nb, dtype=torch.uint8).pin_memory() if dev.type == "cuda" else \
            torch.zeros(nb, dtype=torch.uint8)
        self.limit = torch.ones(slots, dtype=torch.int64, device=dev)
        for c in self.cache:  # row 0 of an empty slot is read by the first steps before anything was admitted
            c.zero_()
        L, d = dec.L, dec.d
        if self.kv8 is not None:
            self.kv8.zero_()
            self.kv_scale.zero_()
            self.pool_kv, self.pool_kv8 = None, torch.empty(L, self.pool * S, 2 * d, dtype=torch.uint8, device=dev)
            self.pool_scale = torch.empty(L, self.pool, 2 * dec.H, dtype=torch.float32, device=dev)
        else:
            self.kv.zero_()
            self.pool_kv8, self.pool_scale = None, None
            self.pool_kv = torch.empty(L, self.pool * S, 2 * d, dtype=dec.dtype, device=dev)
        self.triples = torch.zeros(slots, 3, dtype=torch.int64, device=dev)
        self.triples_host = torch.zeros(slots, 3, dtype=torch.int64)
        self.triples_ev = None
        self.rows_idx = torch.zeros(slots, dtype=torch.int64, device=dev)       # slots whose ids a harvest takes
        self.rows_dev = torch.empty(slots, max_len, dtype=torch.int64, device=dev)
        self.rows_host = torch.empty(slots, max_len, dtype=torch.int64)
        if dev.type == "cuda":
            self.rows_host = self.rows_host.pin_memory()
        if dev.type == "cuda":
            self.triples_host = self.triples_host.pin_memory()
        self.stream = False
        if stream is not None:
            self._stream_init(dec, **stream)

    def _stream_init(self, dec, temperature=None, top_k=0, top_p=1.0, seed=0, constraints=None, prompt_table=None):
        """The opt-in state of sampled / constrained rolling decode (TransformerDecoder.rolling_stream_begin): per slot
        the global row id its random stream hangs on, the row of the prompt table its forced tokens come from (-1:
        none), the cumulative log-probability and the generated length -- all (re)set by mit_slot_admit_ex from
        records (slot, pool image, cap, row id, prompt index) -- plus the device seed, the filter settings, the
        prompt table (int64 [n, Lp + 1], DecodeState.forced's layout, one row per prompt) and the suppress list.
        A harvest takes the ids rows and the log-probabilities in one packed copy."""
        dev, slots = dec.device, self.slots
        self.stream = True
        self.temperature = None if temperature is None else float(temperature)
        self.top_k, self.top_p = int(top_k), float(top_p)
        self.row_id = torch.zeros(slots, dtype=torch.int64, device=dev)
        self.prompt_idx = torch.full((slots,), -1, dtype=torch.int64, device=dev)
        self.logprob = torch.zeros(slots, dtype=torch.float32, device=dev)
        self.length = torch.zeros(slots, dtype=torch.int32, device=dev)
        s = int(seed) & 0xFFFFFFFFFFFFFFFF  # the kernels read a uint64
        self.seed = torch.tensor([s - (1 << 64) if s >= (1 << 63) else s], dtype=torch.int64, device=dev)
        if constraints is not None and constraints.active():
            self.cons = constraints
            if constraints.suppress:
                self.suppress = torch.tensor(constraints.suppress, dtype=torch.int64, device=dev)
            if prompt_table is not None:
                self.forced = prompt_table.contiguous().to(dev)
        self.records = torch.zeros(slots, 5, dtype=torch.int64, device=dev)
        self.records_host = torch.zeros(slots, 5, dtype=torch.int64)
        self.pack_dev = torch.empty(slots, self.max_len + 1, dtype=torch.int64, device=dev)
        self.pack_host = torch.empty(slots, self.max_len + 1, dtype=torch.int64)
        if dev.type == "cuda":
            self.records_host = self.records_host.pin_memory()
            self.pack_host = self.pack_host.pin_memory()

    def harvest_ex(self, slot_list):
        """harvest for the opt-in state: (ids rows [n, max_len] on the host, the n log-probabilities), packed on the
        device (ids | the f32 bits of logprob) and taken in ONE stream-ordered copy, waited for before the admit
        launch that reuses the slots."""
        n, T = len(slot_list), self.max_len
        self.rows_idx[:n].copy_(torch.tensor(slot_list, dtype=torch.int64), non_blocking=True)
        idx = self.rows_idx[:n]
        self.pack_dev[:n, :T] = self.ids.index_select(0, idx)
        self.pack_dev[:n, T] = self.logprob.index_select(0, idx).view(torch.int32)
        self.pack_host[:n].copy_(self.pack_dev[:n], non_blocking=True)
        torch.cuda.current_stream().synchronize()
        lp = self.pack_host[:n, T].to(torch.int32).view(torch.float32).tolist()
        return self.pack_host[:n, :T], lp

    def harvest(self, slot_list):
        """The ids rows of the given slots, [len(slot_list), max_len] on the host (pinned): only those rows are
        gathered and copied, stream-ordered, and waited for -- before the admit launch that reuses the slots."""
        n = len(slot_list)
        self.rows_idx[:n].copy_(torch.tensor(slot_list, dtype=torch.int64), non_blocking=True)
        torch.index_select(self.ids, 0, self.rows_idx[:n], out=self.rows_dev[:n])
        self.rows_host[:n].copy_(self.rows_dev[:n], non_blocking=True)
        torch.cuda.current_stream().synchronize()
        return self.rows_host[:n]

    def snapshot(self):
        """(done flags, row_pos) of every slot as Python lists: one stream-ordered copy, then a wait for it."""
        self.poll_host.copy_(self.poll_dev, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        n = self.slots
        return (self.poll_host[8 * n:12 * n].view(torch.int32).tolist(), self.poll_host[:8 * n].view(torch.int64).tolist())


class TransformerDecoder:
    """Reference-surface decoder: same constructor arguments as decoder.py:84-85.

    Parameters live in a FlatParams store (shared with the model's projection when built by
    model.ImageToTextModel). ``forward(tgt_tokens, memory, memory_padding_mask=None)`` matches
    decoder.py:134-193 and returns f32 logits [B, T, V].
    """

    def __init__(self, vocab_size: int, embed_dim: int, num_heads: int, num_layers: int, ff_dim: int,
                 max_seq_len: int, dropout: float = 0.1, pad_idx: int = 0, *, store: Optional[FlatParams] = None,
                 device=None, dtype: Optional[torch.dtype] = None):
        native.require_gpu()
        self.V, self.d, self.H, self.L, self.F = vocab_size, embed_dim, num_heads, num_layers, ff_dim
        self.Vp = padded_vocab(vocab_size)
        if embed_dim % num_heads:
            raise ValueError(f"embed_dim {embed_dim} is not divisible by num_heads {num_heads}")
        self.hd = embed_dim // num_heads
        if self.hd not in (16, 32, 64, 128):
            raise ValueError(f"head_dim {self.hd} unsupported: the attention kernels take 16, 32, 64 or 128")
        self.max_seq_len, self.dropout, self.pad_idx = max_seq_len, dropout, pad_idx
        self.embed_dim = embed_dim
        self.device = device or torch.device("cuda")
        if store is None:
            dt = dtype or torch.bfloat16
            store = FlatParams(decoder_entries(vocab_size, embed_dim, num_layers, ff_dim, None), self.device, dt)
            store.vocab = vocab_size
            self._own_store = True
        else:
            self._own_store = False
        self.store = store
        self.dtype = store.compute_dtype
        self.pe = sinusoidal_pe(max_seq_len, embed_dim).to(self.device)
        self.training = True
        self._acts: Dict[tuple, _Acts] = {}
        # weight-gradient GEMMs on a second stream; in bf16 a decoder layer's six weight gradients go out
        # as ONE grouped launch (native.gemm_grouped; fp32 parity mode: one GEMM each, as they become
        # ready); the cross-K/V weight gradient (all layers' dY final once layer 0's cross-attention
        # backward ran) goes out right then, ahead of layer 0's grouped dW
        self.dw_side_stream = True
        self.dw_grouped = True
        self.kv_dw_early = True
        self._side = None
        self.side_priority = 0
        if self._own_store:
            self.init_weights(0)

    # --- weights -----------------------------------------------------------------------------
    def init_weights(self, seed: int = 0):
        """decoder.py:128-132: xavier_uniform_ on every >=2-D weight (embedding included, so the
        PAD row is not zero); MHA in/out-proj biases 0 (torch/nn/modules/activation.py:1241-1242);
        LayerNorm 1/0; Linear biases U(-1/sqrt(fan_in), 1/sqrt(fan_in)) (nn.Linear default)."""
        g = torch.Generator().manual_seed(seed)
        d, L = self.d, self.L
        for name, shape, _, _ in self.store.entries:
            if name.startswith("projection."):
                continue
            if name == "cross_kv.weight":
                # xavier on each layer's full in_proj [3d, d] (fan_out = 3d), restricted to the kv rows
                a = math.sqrt(6.0 / (3 * d + d))
                t = (torch.rand(*shape, generator=g) * 2 - 1) * a
            elif len(shape) == 2:
                rows, fi = shape
                if name == "fc_out.weight":
                    rows = self.V  # the pad rows of the head stay 0 (padded_vocab)
                fo = 3 * d if name.endswith("cross_q.weight") else rows
                a = math.sqrt(6.0 / (fo + fi))
                t = torch.zeros(shape)
                t[:rows] = (torch.rand(rows, fi, generator=g) * 2 - 1) * a
            elif "norm" in name:
                t = torch.ones(shape) if name.endswith("weight") else torch.zeros(shape)
            elif any(s in name for s in ("self_in.bias", "self_out.bias", "cross_q.bias", "cross_out.bias",
                                          "cross_kv.bias")):
                t = torch.zeros(shape)
            else:  # linear1/linear2/fc_out biases
                fan_in = {"linear1.bias": d, "linear2.bias": self.F, "fc_out.bias": d}[name.split(".", 2)[-1]
                                                                                        if name.startswith("layers.")
                                                                                        else name]
                b = 1 / math.sqrt(fan_in)
                n = self.V if name == "fc_out.bias" else shape[0]
                t = torch.zeros(shape)
                t[:n] = (torch.rand(n, generator=g) * 2 - 1) * b
            self.store.p(name).copy_(t)
        self.store.sync_shadow()

    def train(self, mode: bool = True):
        self.training = mode
        return self

    def eval(self):
        return self.train(False)

    def _side_stream(self) -> "_SideStream":
        if self._side is None:
            self._side = _SideStream(self.device, self.side_priority)
        return self._side

    # --- forward -----------------------------------------------------------------------------
    def acts(self, B, T, S, train) -> _Acts:
        key = (B, T, S, train)
        if key not in self._acts:
            pi = self.store.index.get("projection.weight")
            self._acts[key] = _Acts(B, T, S, self.d, self.F, self.L, self.V, self.H, self.dtype, self.device, train,
                                    proj_in=pi[0][1] if pi else None)
        return self._acts[key]

    def _p(self):
        return self.dropout if self.training else 0.0

    def run_forward(self, tokens: torch.Tensor, mem: torch.Tensor, mem_ld: int, S: int, A: _Acts,
                    seed: Optional[torch.Tensor], train: bool, logits_out: Optional[torch.Tensor] = None,
                    drop_p: Optional[float] = None, mem_keys: Optional[torch.Tensor] = None,
                    tick: Optional[Callable[[], None]] = None):
        """tokens int64 [B,T] (device); mem: memory rows [B*S, d] with row stride mem_ld.
        tick: called before each layer's launches (the train step issues other work there).
        train=True keeps every layer's activations for run_backward (A must be a train arena);
        drop_p defaults to the module's dropout in train mode and 0 otherwise.
        mem_keys: optional int64 [B, S], 0 where the memory key is padding (memory_padding_mask,
        decoder.py:134-186 -> memory_key_padding_mask of nn.TransformerDecoder), else 1."""
        B, T = tokens.shape
        d, H, L, V = self.d, self.H, self.L, self.V
        st = self.store
        p = drop_p if drop_p is not None else (self._p() if train else 0.0)
        w = st.w
        R = B * T
        ws = A.gemm_ws
        # fused cross-attention K/V projection of every layer (decoder-layer independent)
        native.gemm(mem, w("cross_kv.weight"), A.kv, B * S, L * 2 * d, d, lda=mem_ld, bias=st.p("cross_kv.bias"))
        native.embed_fwd(tokens, w("token_embedding.weight"), math.sqrt(d), self.pe, A.x0, drop_p=p, seed=seed,
                         site=EMB_SITE)
        xin = A.x0
        for l in range(L):
            if tick is not None:
                tick()
            j = l if train else 0
            xs = A.xs[l] if train else A.xs[l % 2]
            z, stt = A.z[j], A.st[j]
            pre = f"layers.{l}."
            base = 64 * l
            qkv = A.qkv[j]
            native.linear(xin, w(pre + "self_in.weight"), qkv, bias=st.p(pre + "self_in.bias"))
            sa = native.attn_args(qkv, 3 * d, T * 3 * d, qkv[:, d:], 3 * d, T * 3 * d, qkv[:, 2 * d:], 3 * d, T * 3 * d,
                                  A.os[j], d, T * d, lse=A.lse_s[j], key_tokens=tokens, tok_batch=T,
                                  pad_idx=self.pad_idx, causal=True, scale=1.0 / math.sqrt(self.hd), drop_p=p, seed=seed,
                                  site=base + 0)
            native.attention_fwd(native.dtype_code(qkv), B, H, T, T, sa, Dh=self.hd)
            native.linear(A.os[j], w(pre + "self_out.weight"), A.y, bias=st.p(pre + "self_out.bias"), workspace=ws)
            native.layernorm_fwd(xin, st.p(pre + "norm1.weight"), st.p(pre + "norm1.bias"), 1e-5, xs[0], r=A.y,
                                 drop_p=p, seed=seed, site=base + 1, z=z[0], mean=stt[0][0], rstd=stt[0][1])
            native.linear(xs[0], w(pre + "cross_q.weight"), A.qc[j], bias=st.p(pre + "cross_q.bias"), workspace=ws)
            kvl = A.kv[:, l * 2 * d:]
            ca = native.attn_args(A.qc[j], d, T * d, kvl, L * 2 * d, S * L * 2 * d, kvl[:, d:], L * 2 * d,
                                  S * L * 2 * d, A.oc[j], d, T * d, lse=A.lse_c[j], scale=1.0 / math.sqrt(self.hd), drop_p=p,
                                  seed=seed, site=base + 2, key_tokens=mem_keys, tok_batch=S, pad_idx=0)
            native.attention_fwd(native.dtype_code(qkv), B, H, T, S, ca, Dh=self.hd)
            native.linear(A.oc[j], w(pre + "cross_out.weight"), A.y, bias=st.p(pre + "cross_out.bias"), workspace=ws)
            native.layernorm_fwd(xs[0], st.p(pre + "norm2.weight"), st.p(pre + "norm2.bias"), 1e-5, xs[1], r=A.y,
                                 drop_p=p, seed=seed, site=base + 3, z=z[1], mean=stt[1][0], rstd=stt[1][1])
            native.linear(xs[1], w(pre + "linear1.weight"), A.h[j], bias=st.p(pre + "linear1.bias"),
                          act=native.ACT_RELU, drop_p=p, seed=seed, site=base + 4)
            native.linear(A.h[j], w(pre + "linear2.weight"), A.y, bias=st.p(pre + "linear2.bias"), workspace=ws)
            native.layernorm_fwd(xs[1], st.p(pre + "norm3.weight"), st.p(pre + "norm3.bias"), 1e-5, xs[2], r=A.y,
                                 drop_p=p, seed=seed, site=base + 5, z=z[2], mean=stt[2][0], rstd=stt[2][1])
            xin = xs[2]
        logits = A.logits if logits_out is None else logits_out
        native.linear(xin, w("fc_out.weight"), logits, bias=st.p("fc_out.bias"))
        return logits, xin

    # --- scoring -----------------------------------------------------------------------------
    def default_head_rows(self, R: int) -> int:
        """Rows per head chunk of run_score: as many as keep the head_rows x Vp logits buffer within
        SCORE_LOGITS_BYTES (32 MiB: 1536 rows of the bf16 V = 10000 head, a 6 x 40 grid of 256-tiles), a multiple
        of 256 where that is possible, and never more than the R rows there are."""
        n = max(1, SCORE_LOGITS_BYTES // (self.Vp * torch.empty(0, dtype=self.dtype).element_size()))
        if n >= 256:
            n -= n % 256
        return max(1, min(n, R))

    def score_acts(self, B, C, T, S, head_rows) -> _ScoreActs:
        key = ("score", B, C, T, S, head_rows)
        if key not in self._acts:
            self._acts[key] = _ScoreActs(B, C, T, S, self.d, self.F, self.L, self.Vp, self.H, self.dtype, self.device,
                                         head_rows)
        return self._acts[key]

    def run_score(self, tokens: torch.Tensor, targets: torch.Tensor, mem: torch.Tensor, mem_ld: int, S: int, *,
                  head_rows: Optional[int] = None) -> _ScoreActs:
        """Teacher-forced scores of C candidate captions per image: tokens / targets int64 [B, C, T] (device; the
        decoder inputs and the tokens they should predict, pad_idx = not scored); mem: memory rows [B*S, d] with
        row stride mem_ld. Forward only, no dropout, and nothing is kept for a backward.

        The image's cross-attention K/V is computed once for its C candidates (one GEMM over B*S rows); the
        self-attention runs over B*C sequences of T (causal + key-padding from tokens, as run_forward), the
        cross-attention as B batches of C*T queries over the image's S keys (q/o batch stride C*T*d), everything
        else row-wise over the B*C*T rows. The vocabulary head runs head_rows rows at a time (default:
        default_head_rows) into one logits buffer that native.score_rows reduces to a log-probability and a rank
        per row before the next chunk overwrites it, so logits for all rows never exist; native.score_sequences
        then sums per candidate. A chunk need not be a multiple of T. No GEMM takes a split-K workspace: a row's
        values do not depend on how many rows the call has.

        Returns the arena: seq_logprob f32 / seq_tokens / seq_hits int32 [B*C], token_logprob f32 / rank int32
        [B*C*T] (views the next call with the same shape overwrites)."""
        B, C, T = tokens.shape
        d, H, L, V = self.d, self.H, self.L, self.V
        st = self.store
        w = st.w
        R = B * C * T
        hr = self.default_head_rows(R) if head_rows is None else int(head_rows)
        if hr < 1:
            raise ValueError(f"head_rows must be positive, got {head_rows}")
        hr = min(hr, R)
        A = self.score_acts(B, C, T, S, hr)
        tok2 = tokens.view(B * C, T)
        tgt = targets.view(R)
        dt = native.dtype_code(A.x0)
        scale = 1.0 / math.sqrt(self.hd)
        native.gemm(mem, w("cross_kv.weight"), A.kv, B * S, L * 2 * d, d, lda=mem_ld, bias=st.p("cross_kv.bias"))
        native.embed_fwd(tok2, w("token_embedding.weight"), math.sqrt(d), self.pe, A.x0)
        xin = A.x0
        for l in range(L):
            xs = A.xs[l % 2]
            pre = f"layers.{l}."
            native.linear(xin, w(pre + "self_in.weight"), A.qkv, bias=st.p(pre + "self_in.bias"))
            sa = native.attn_args(A.qkv, 3 * d, T * 3 * d, A.qkv[:, d:], 3 * d, T * 3 * d, A.qkv[:, 2 * d:], 3 * d,
                                  T * 3 * d, A.os, d, T * d, lse=A.lse, key_tokens=tok2, tok_batch=T,
                                  pad_idx=self.pad_idx, causal=True, scale=scale)
            native.attention_fwd(dt, B * C, H, T, T, sa, Dh=self.hd)
            native.linear(A.os, w(pre + "self_out.weight"), A.y, bias=st.p(pre + "self_out.bias"))
            native.layernorm_fwd(xin, st.p(pre + "norm1.weight"), st.p(pre + "norm1.bias"), 1e-5, xs[0], r=A.y)
            native.linear(xs[0], w(pre + "cross_q.weight"), A.qc, bias=st.p(pre + "cross_q.bias"))
            kvl = A.kv[:, l * 2 * d:]
            ca = native.attn_args(A.qc, d, C * T * d, kvl, L * 2 * d, S * L * 2 * d, kvl[:, d:], L * 2 * d,
                                  S * L * 2 * d, A.oc, d, C * T * d, lse=A.lse, scale=scale)
            native.attention_fwd(dt, B, H, C * T, S, ca, Dh=self.hd)
            native.linear(A.oc, w(pre + "cross_out.weight"), A.y, bias=st.p(pre + "cross_out.bias"))
            native.layernorm_fwd(xs[0], st.p(pre + "norm2.weight"), st.p(pre + "norm2.bias"), 1e-5, xs[1], r=A.y)
            native.linear(xs[1], w(pre + "linear1.weight"), A.h, bias=st.p(pre + "linear1.bias"), act=native.ACT_RELU)
            native.linear(A.h, w(pre + "linear2.weight"), A.y, bias=st.p(pre + "linear2.bias"))
            native.layernorm_fwd(xs[1], st.p(pre + "norm3.weight"), st.p(pre + "norm3.bias"), 1e-5, xs[2], r=A.y)
            xin = xs[2]
        wo, bo = w("fc_out.weight"), st.p("fc_out.bias")
        for r0 in range(0, R, hr):
            n = min(hr, R - r0)
            native.linear(xin[r0:r0 + n], wo, A.logits, bias=bo)
            native.score_rows(A.logits, tgt[r0:r0 + n], self.pad_idx, A.token_logprob[r0:r0 + n], A.rank[r0:r0 + n],
                              rows=n, V=V, ld=self.Vp)
        native.score_sequences(A.token_logprob, A.rank, T, A.seq_logprob, A.seq_tokens, A.seq_hits, n_seq=B * C)
        return A

    def run_backward(self, tokens: torch.Tensor, mem: torch.Tensor, mem_ld: int, S: int, A: _Acts,
                     seed: Optional[torch.Tensor], dlogits: torch.Tensor,
                     proj_input: Optional[Tuple[torch.Tensor, int, int]] = None,
                     grads_ready: Optional[Callable[[str, str], None]] = None,
                     mem_keys: Optional[torch.Tensor] = None, tick: Optional[Callable[[], None]] = None):
        """Backward of run_forward(train=True) given dlogits [R, V] (compute dtype); tick as in run_forward.
        proj_input = (enc_rows, ld, E): encoder features feeding the projection (for dW_proj).
        grads_ready(first, last) is called as soon as the grads of a contiguous entry span are final."""
        B, T = tokens.shape
        d, H, L, V, F = self.d, self.H, self.L, self.V, self.F
        st, p = self.store, self._p()
        w, g = st.w, st.g
        R = B * T
        MN, K = native.MN_CONTIG, native.K_CONTIG
        x_last = A.xs[L - 1][2]
        ws = A.gemm_ws
        side = self._side_stream() if self.dw_side_stream else None
        # the embedding gradient's deterministic summation order depends on the tokens only: build it
        # on the side stream now, off the dX chain
        if side is None:
            native.embed_plan(tokens, A.emb_plan)
        else:
            # the embedding plan depends on the tokens only; the table gradient's zero fill (20 MB at
            # cfg1) rides with it, off the main stream's chain (the previous AdamW, its last reader, is
            # behind the side stream's wait on main)
            side.run(lambda: (native.embed_plan(tokens, A.emb_plan), native.zero(g("token_embedding.weight"))))
            plan_ev = side.plan_events.record(side.ptr)

        def dW(dy, x, wname, bname, M, N, K, lda, ldb):
            """weight grad dY^T X (TN GEMM) with the bias grad (row sums of dY^T) fused in, split-K;
            on the side stream when enabled."""
            if side is None:
                native.gemm(dy, x, g(wname), M, N, K, a_layout=MN, b_layout=MN, lda=lda, ldb=ldb, rowsum=g(bname),
                            workspace=ws)
                return
            side.run(lambda: native.gemm(dy, x, g(wname), M, N, K, a_layout=MN, b_layout=MN, lda=lda, ldb=ldb,
                                         rowsum=g(bname), workspace=A.gemm_ws_side), reads=(dy,))

        def guard(t):
            if side is not None:
                side.guard(t)

        def ln_bwd(l, k, dx, z, stt, dr, site, defer=False):
            """LayerNorm k (1..3) of layer l backward; dgamma/dbeta reduced on the side stream (defer: the
            reduction job is returned for the layer's grouped dW launch instead)."""
            gname, bname = f"layers.{l}.norm{k}.weight", f"layers.{l}.norm{k}.bias"
            if side is None:
                native.layernorm_bwd(dx, z, stt[0], stt[1], st.p(gname), dx, g(gname), g(bname), A.ln_ws, dr=dr,
                                     drop_p=p, seed=seed, site=site)
                return None
            ws_l = A.ln_ws_side[3 * l + k - 1]
            native.layernorm_bwd(dx, z, stt[0], stt[1], st.p(gname), dx, None, None, ws_l, dr=dr, drop_p=p, seed=seed,
                                 site=site)
            if defer:
                return (R, d, ws_l, g(gname), g(bname))
            side.run(lambda: native.layernorm_param_grads(R, d, ws_l, g(gname), g(bname)))
            return None

        def ready(first, last):
            if grads_ready is None:
                return
            if side is None:  # a host step of a recorded program (replayed in place)
                native.host_call(lambda: grads_ready(first, last))
            else:
                side.under(lambda: grads_ready(first, last))

        # fc_out
        Vp = self.Vp  # dlogits [R, Vp]: the pad columns hold exactly 0 (padded_vocab)
        dW(dlogits, x_last, "fc_out.weight", "fc_out.bias", Vp, d, R, Vp, d)
        native.gemm(dlogits, w("fc_out.weight"), A.dx, R, d, Vp, b_layout=MN, ldb=d, workspace=ws)
        ready("fc_out.weight", "fc_out.bias")
        ascale = 1.0 / (1.0 - p) if p > 0 else 1.0
        grouped = side is not None and self.dw_grouped and self.dtype == torch.bfloat16
        BS = B * S
        pair = grouped and proj_input is not None
        early = pair and self.kv_dw_early
        kv_prob = (A.dkv, mem, g("cross_kv.weight"), L * 2 * d, d, BS, L * 2 * d, mem_ld, g("cross_kv.bias"))

        def kv_early():
            if not early:
                return
            if A.gws_kv is None:
                A.gws_kv = torch.empty((native.gemm_grouped_ws_bytes([kv_prob]) + 255) // 4, dtype=torch.float32,
                                       device=self.device)
            side.run(lambda: native.gemm_grouped([kv_prob], A.gws_kv), reads=(A.dkv,))
            # its own DP bucket (12.6 MB at cfg1): all-reduced under the rest of the backward instead of with
            # the embedding / projection gradients after it (exposed communication)
            ready("cross_kv.weight", "cross_kv.bias")
        for l in reversed(range(L)):
            if tick is not None:
                tick()
            pre = f"layers.{l}."
            base = 64 * l
            xs, z, stt = A.xs[l], A.z[l], A.st[l]
            xin = A.x0 if l == 0 else A.xs[l - 1][2]
            if grouped:
                self._layer_backward_grouped(l, A, tokens, seed, p, xs, z, stt, xin, S, mem_keys, g, w, ln_bwd, guard,
                                             side, after_cross=kv_early if l == 0 else None)
                ready(pre + "linear2.weight", pre + "norm1.bias")
                continue
            # LN3 -> dz3 (dx, in place) and d(ffn_out) (dy)
            guard(A.dy)
            ln_bwd(l, 3, A.dx, z[2], stt[2], A.dy, base + 5)
            # FFN
            dW(A.dy, A.h[l], pre + "linear2.weight", pre + "linear2.bias", d, F, R, d, F)
            guard(A.dh)
            native.gemm(A.dy, w(pre + "linear2.weight"), A.dh, R, F, d, b_layout=MN, ldb=F, aux=A.h[l], ld_aux=F,
                        aux_scale=ascale)
            dW(A.dh, xs[1], pre + "linear1.weight", pre + "linear1.bias", F, d, R, F, d)
            native.gemm(A.dh, w(pre + "linear1.weight"), A.dx, R, d, F, b_layout=MN, ldb=d, residual=A.dx, ldr=d,
                        workspace=ws)
            # LN2
            guard(A.dy)
            ln_bwd(l, 2, A.dx, z[1], stt[1], A.dy, base + 3)
            # cross-attention block
            dW(A.dy, A.oc[l], pre + "cross_out.weight", pre + "cross_out.bias", d, d, R, d, d)
            native.gemm(A.dy, w(pre + "cross_out.weight"), A.do, R, d, d, b_layout=MN, ldb=d, workspace=ws)
            kvl, dkvl = A.kv[:, l * 2 * d:], A.dkv[:, l * 2 * d:]
            ca = native.attn_args(A.qc[l], d, T * d, kvl, L * 2 * d, S * L * 2 * d, kvl[:, d:], L * 2 * d,
                                  S * L * 2 * d, A.oc[l], d, T * d, lse=A.lse_c[l], scale=1.0 / math.sqrt(self.hd), drop_p=p,
                                  seed=seed, site=base + 2, key_tokens=mem_keys, tok_batch=S, pad_idx=0)
            cg = native.attn_grads(A.do, d, T * d, A.dq, d, T * d, dkvl, L * 2 * d, S * L * 2 * d, dkvl[:, d:],
                                   L * 2 * d, S * L * 2 * d, A.delta)
            guard(A.dq)
            native.attention_bwd(native.dtype_code(A.dq), B, H, T, S, ca, cg, Dh=self.hd)
            dW(A.dq, xs[0], pre + "cross_q.weight", pre + "cross_q.bias", d, d, R, d, d)
            native.gemm(A.dq, w(pre + "cross_q.weight"), A.dx, R, d, d, b_layout=MN, ldb=d, residual=A.dx, ldr=d,
                        workspace=ws)
            # LN1
            guard(A.dy)
            ln_bwd(l, 1, A.dx, z[0], stt[0], A.dy, base + 1)
            # self-attention block
            dW(A.dy, A.os[l], pre + "self_out.weight", pre + "self_out.bias", d, d, R, d, d)
            native.gemm(A.dy, w(pre + "self_out.weight"), A.do, R, d, d, b_layout=MN, ldb=d, workspace=ws)
            qkv = A.qkv[l]
            sa = native.attn_args(qkv, 3 * d, T * 3 * d, qkv[:, d:], 3 * d, T * 3 * d, qkv[:, 2 * d:], 3 * d, T * 3 * d,
                                  A.os[l], d, T * d, lse=A.lse_s[l], key_tokens=tokens, tok_batch=T,
                                  pad_idx=self.pad_idx, causal=True, scale=1.0 / math.sqrt(self.hd), drop_p=p, seed=seed,
                                  site=base + 0)
            sg = native.attn_grads(A.do, d, T * d, A.dqkv, 3 * d, T * 3 * d, A.dqkv[:, d:], 3 * d, T * 3 * d,
                                   A.dqkv[:, 2 * d:], 3 * d, T * 3 * d, A.delta)
            guard(A.dqkv)
            native.attention_bwd(native.dtype_code(A.dq), B, H, T, T, sa, sg, Dh=self.hd)
            dW(A.dqkv, xin, pre + "self_in.weight", pre + "self_in.bias", 3 * d, d, R, 3 * d, d)
            native.gemm(A.dqkv, w(pre + "self_in.weight"), A.dx, R, d, 3 * d, b_layout=MN, ldb=d, residual=A.dx,
                        ldr=d, workspace=ws)
            ready(pre + "linear2.weight", pre + "norm1.bias")
        # cross K/V of all layers
        if pair:
            # the memory gradient first, then the projection weight gradient -- with the cross-K/V one
            # as a group unless that went out early (kv_early) -- the step's last GEMMs
            enc_rows, enc_ld, E = proj_input
            native.gemm(A.dkv, w("cross_kv.weight"), A.dmem, BS, d, L * 2 * d, b_layout=MN, ldb=d, workspace=ws)
            tail = ([] if early else [kv_prob]) + [
                (A.dmem, enc_rows, g("projection.weight"), d, E, BS, d, enc_ld, g("projection.bias"))]
            if A.gws_tail is None:
                A.gws_tail = torch.empty((native.gemm_grouped_ws_bytes(tail) + 255) // 4, dtype=torch.float32,
                                         device=self.device)
            side.run(lambda: native.gemm_grouped(tail, A.gws_tail), reads=(A.dkv, A.dmem))
        else:
            dW(A.dkv, mem, "cross_kv.weight", "cross_kv.bias", L * 2 * d, d, BS, L * 2 * d, mem_ld)
        # embedding (scatter-add into a zeroed table gradient; PAD row gets nothing)
        ge = g("token_embedding.weight")
        if side is not None:
            native.HipEvents.wait(native.stream_ptr(), plan_ev)  # the plan and the zeroed table
        else:
            native.zero(ge)
        native.embed_bwd(tokens, A.dx, math.sqrt(d), ge, self.pad_idx, drop_p=p, seed=seed, site=EMB_SITE,
                         plan=A.emb_plan)
        last = "token_embedding.weight"
        if pair:
            last = "projection.bias"
        elif proj_input is not None:
            enc_rows, enc_ld, E = proj_input
            native.gemm(A.dkv, w("cross_kv.weight"), A.dmem, BS, d, L * 2 * d, b_layout=MN, ldb=d, workspace=ws)
            dW(A.dmem, enc_rows, "projection.weight", "projection.bias", d, E, BS, d, enc_ld)
            last = "projection.bias"
        ready("token_embedding.weight" if early else "cross_kv.weight", last)
        if side is not None:
            side.join()

    def _layer_backward_grouped(self, l, A, tokens, seed, p, xs, z, stt, xin, S, mem_keys, g, w, ln_bwd, guard, side,
                                after_cross=None):
        """One decoder layer of run_backward with its six weight gradients issued as ONE grouped launch
        (native.gemm_grouped) on the side stream after the layer's dX chain; the dY operands live in the
        layer-parity buffers A.gdy / gdh / gdq / gdqkv until that launch has read them."""
        B, T = tokens.shape
        d, H, L, F, R = self.d, self.H, self.L, self.F, A.R
        MN = native.MN_CONTIG
        pre = f"layers.{l}."
        base = 64 * l
        sp = l % 2
        dyF, dyC, dyS = A.gdy[sp]
        dh, dq, dqkv = A.gdh[sp], A.gdq[sp], A.gdqkv[sp]
        ascale = 1.0 / (1.0 - p) if p > 0 else 1.0
        ws = A.gemm_ws
        # LN3 -> dz3 (dx, in place) and d(ffn_out)
        guard(dyF)
        j3 = ln_bwd(l, 3, A.dx, z[2], stt[2], dyF, base + 5, defer=True)
        guard(dh)
        native.gemm(dyF, w(pre + "linear2.weight"), dh, R, F, d, b_layout=MN, ldb=F, aux=A.h[l], ld_aux=F,
                    aux_scale=ascale)
        native.gemm(dh, w(pre + "linear1.weight"), A.dx, R, d, F, b_layout=MN, ldb=d, residual=A.dx, ldr=d, workspace=ws)
        guard(dyC)
        j2 = ln_bwd(l, 2, A.dx, z[1], stt[1], dyC, base + 3, defer=True)
        native.gemm(dyC, w(pre + "cross_out.weight"), A.do, R, d, d, b_layout=MN, ldb=d, workspace=ws)
        kvl, dkvl = A.kv[:, l * 2 * d:], A.dkv[:, l * 2 * d:]
        ca = native.attn_args(A.qc[l], d, T * d, kvl, L * 2 * d, S * L * 2 * d, kvl[:, d:], L * 2 * d, S * L * 2 * d,
                              A.oc[l], d, T * d, lse=A.lse_c[l], scale=1.0 / math.sqrt(self.hd), drop_p=p, seed=seed,
                              site=base + 2, key_tokens=mem_keys, tok_batch=S, pad_idx=0)
        cg = native.attn_grads(A.do, d, T * d, dq, d, T * d, dkvl, L * 2 * d, S * L * 2 * d, dkvl[:, d:], L * 2 * d,
                               S * L * 2 * d, A.delta)
        guard(dq)
        native.attention_bwd(native.dtype_code(dq), B, H, T, S, ca, cg, Dh=self.hd)
        if after_cross is not None:
            after_cross()
        native.gemm(dq, w(pre + "cross_q.weight"), A.dx, R, d, d, b_layout=MN, ldb=d, residual=A.dx, ldr=d, workspace=ws)
        guard(dyS)
        j1 = ln_bwd(l, 1, A.dx, z[0], stt[0], dyS, base + 1, defer=True)
        native.gemm(dyS, w(pre + "self_out.weight"), A.do, R, d, d, b_layout=MN, ldb=d, workspace=ws)
        qkv = A.qkv[l]
        sa = native.attn_args(qkv, 3 * d, T * 3 * d, qkv[:, d:], 3 * d, T * 3 * d, qkv[:, 2 * d:], 3 * d, T * 3 * d,
                              A.os[l], d, T * d, lse=A.lse_s[l], key_tokens=tokens, tok_batch=T, pad_idx=self.pad_idx,
                              causal=True, scale=1.0 / math.sqrt(self.hd), drop_p=p, seed=seed, site=base + 0)
        sg = native.attn_grads(A.do, d, T * d, dqkv, 3 * d, T * 3 * d, dqkv[:, d:], 3 * d, T * 3 * d, dqkv[:, 2 * d:],
                               3 * d, T * 3 * d, A.delta)
        guard(dqkv)
        native.attention_bwd(native.dtype_code(dq), B, H, T, T, sa, sg, Dh=self.hd)
        native.gemm(dqkv, w(pre + "self_in.weight"), A.dx, R, d, 3 * d, b_layout=MN, ldb=d, residual=A.dx, ldr=d,
                    workspace=ws)
        probs = [(dyF, A.h[l], g(pre + "linear2.weight"), d, F, R, d, F, g(pre + "linear2.bias")),
                 (dh, xs[1], g(pre + "linear1.weight"), F, d, R, F, d, g(pre + "linear1.bias")),
                 (dyC, A.oc[l], g(pre + "cross_out.weight"), d, d, R, d, d, g(pre + "cross_out.bias")),
                 (dq, xs[0], g(pre + "cross_q.weight"), d, d, R, d, d, g(pre + "cross_q.bias")),
                 (dyS, A.os[l], g(pre + "self_out.weight"), d, d, R, d, d, g(pre + "self_out.bias")),
                 (dqkv, xin, g(pre + "self_in.weight"), 3 * d, d, R, 3 * d, d, g(pre + "self_in.bias"))]
        if A.gws is None:
            A.gws = torch.empty((native.gemm_grouped_ws_bytes(probs) + 255) // 4, dtype=torch.float32,
                                device=self.device)
        side.run(lambda: native.gemm_grouped(probs, A.gws, ln_jobs=(j3, j2, j1)), reads=(dyF, dh, dyC, dq, dyS, dqkv))

    # --- batched greedy decoding with a KV cache (config 5) ---------------------------------------
    def _constrain_begin(self, stt: "DecodeState", constraints: Optional[DecodeConstraints], images: int, rep: int):
        """Attach active constraints to a fresh state of images * rep rows (rep: the beams / samples of an image):
        validation on the host, the suppress list and the forced-token table on the device. Inactive or no
        constraints leave the state as it is, and its steps make no constraint launch."""
        if constraints is None or not constraints.active():
            return
        constraints.validate(self.V, stt.max_len, stt.end_id, images)
        stt.cons = constraints
        if constraints.suppress:
            stt.suppress = torch.tensor(constraints.suppress, dtype=torch.int64, device=self.device)
        if constraints.has_prompts():
            prompts = constraints.image_prompts(images)
            forced = torch.full((images, max(len(p) for p in prompts) + 1), -1, dtype=torch.int64)
            for b, p in enumerate(prompts):
                forced[b, 1:1 + len(p)] = torch.tensor(p, dtype=torch.int64)
            stt.forced = forced.repeat_interleave(rep, 0).contiguous().to(self.device)

    def _constrain(self, stt: "DecodeState"):
        """The step's constraint launch on stt.logits (between the head GEMM and the pick); a beam state's history
        goes through its ancestor table."""
        c = stt.cons
        native.logits_constrain(stt.logits, self.V, stt.ids, stt.pos, group=stt.K or 1, anc=stt.anc if stt.K else None,
                                finished=stt.finished, repetition_penalty=c.repetition_penalty,
                                no_repeat_ngram=c.no_repeat_ngram, min_length=c.min_length, end_id=stt.end_id,
                                suppress=stt.suppress, forced=stt.forced)

    def _cross_kv_begin(self, stt: "DecodeState", mem: torch.Tensor, mem_ld: int, S: int, B: int):
        """The cross-attention K | V of every layer for the B images of mem, once per decode (one GEMM per layer).
        An fp8 state gets each layer through one bf16 staging buffer [B*S, 2d], quantised from there (2H groups of
        head_dim columns per row: the K heads, then the V heads) and released when this returns."""
        d, L, st = self.d, self.L, self.store
        wkv, bkv = st.w("cross_kv.weight"), st.p("cross_kv.bias")
        fp8 = stt.kv8 is not None
        stage = torch.empty(B * S, 2 * d, dtype=self.dtype, device=self.device) if fp8 else None
        for l in range(L):
            native.gemm(mem, wkv[l * 2 * d:], stage if fp8 else stt.kv[l], B * S, 2 * d, d, lda=mem_ld,
                        bias=bkv[l * 2 * d:])
            if fp8:
                native.kv_quantize_fp8(stage, 2 * d, S * 2 * d, stt.kv8[l], 2 * d, S * 2 * d, stt.kv_scale[l], B, S,
                                       2 * self.H, Dh=self.hd)

    def decode_begin(self, mem: torch.Tensor, mem_ld: int, S: int, B: int, max_len: int, start_id: int,
                     end_id: int, constraints: Optional[DecodeConstraints] = None,
                     kv_dtype: Optional[str] = None) -> "DecodeState":
        """Set up a batched greedy decode over B images whose memory rows are mem [B*S, d] (row
        stride mem_ld): cross-attention K/V of every layer computed once (one fused GEMM), empty
        self-attention caches, ids[:, 0] = START, position 0 on the device. constraints: DecodeConstraints
        (inactive or None: the unconstrained step, launch for launch). kv_dtype: resolve_kv_dtype ("fp8": the
        cross-attention K/V as e4m3 bytes, quantised here once; unset, the state and every launch as before)."""
        if max_len > self.pe.shape[0]:
            raise ValueError(f"max_len {max_len} exceeds the positional table ({self.pe.shape[0]} = "
                             f"decoder_max_seq_len; the reference's PositionalEncoding would fail too)")
        stt = DecodeState(self, B, S, max_len, start_id, end_id, kv_dtype=kv_dtype)
        self._constrain_begin(stt, constraints, B, 1)
        self._cross_kv_begin(stt, mem, mem_ld, S, B)
        return stt

    def decode_step(self, stt: "DecodeState"):
        """One greedy token for every row: position p = stt.pos (device) -> ids[:, p+1]; p += 1.
        No host synchronisation: capturable into a hipGraph. With active constraints the head runs as the plain
        GEMM into f32 logits (as beam_step), the constraint launch edits them, and the pick is the argmax of the
        edited rows (greedy_pick_advance on the fused state; greedy_pick and step_inc otherwise)."""
        if stt.cons is not None:
            return self._decode_step_constrained(stt)
        if stt.fused:
            return self._decode_step_fused(stt)
        x = self._step_body(stt)
        st, w = self.store, self.store.w
        native.linear(x, w("fc_out.weight"), stt.logits, bias=st.p("fc_out.bias"))
        native.greedy_pick(stt.logits, stt.ids, stt.pos, stt.end_id, self.pad_idx, stt.finished, stt.n_finished,
                           V=self.V)
        native.step_inc(stt.pos)

    def _decode_step_constrained(self, stt: "DecodeState"):
        """decode_step with active constraints: the folded argmax of the fused head gives way to f32 logits in
        memory, which the constraint launch edits before the pick reads them."""
        x = self._step_body_fused(stt) if stt.fused else self._step_body(stt)
        st, w = self.store, self.store.w
        native.linear(x, w("fc_out.weight"), stt.logits, bias=st.p("fc_out.bias"))
        self._constrain(stt)
        if stt.fused:
            native.greedy_pick_advance(stt.logits, stt.ids, stt.pos, stt.end_id, self.pad_idx, stt.finished,
                                       stt.n_finished, stt.ticket, V=self.V)
        else:
            native.greedy_pick(stt.logits, stt.ids, stt.pos, stt.end_id, self.pad_idx, stt.finished, stt.n_finished,
                               V=self.V)
            native.step_inc(stt.pos)

    def _embed_step(self, stt: "DecodeState"):
        """stt.x = the embedding of every row's current token plus its position's encoding."""
        table = self.store.w("token_embedding.weight")
        if stt.row_pos is not None:
            native.embed_decode_ragged(stt.ids, stt.row_pos, table, math.sqrt(self.d), self.pe, stt.x)
        else:
            native.embed_decode(stt.ids, stt.pos, table, math.sqrt(self.d), self.pe, stt.x)

    def _attn_self(self, stt: "DecodeState", cache: torch.Tensor, scale: float):
        """The step's causal self-attention over the cache (query: stt.qkv's first d columns) -> stt.o; a beam
        state reads each key from its ancestor's row."""
        d, Tm = self.d, stt.max_len
        if stt.row_pos is not None:
            native.attention_decode_ragged(stt.qkv, 3 * d, cache, 2 * d, Tm * 2 * d, cache[:, :, d:], 2 * d, Tm * 2 * d,
                                           stt.o, d, stt.B, self.H, row_pos=stt.row_pos, key_tokens=stt.ids,
                                           tok_batch=Tm, pad_idx=self.pad_idx, scale=scale, Dh=self.hd)
        elif stt.K:
            native.attention_decode_beam(stt.qkv, 3 * d, cache, 2 * d, Tm * 2 * d, cache[:, :, d:], 2 * d, Tm * 2 * d,
                                         stt.o, d, stt.B, self.H, pos=stt.pos, group=stt.K, anc=stt.anc,
                                         key_tokens=stt.ids, tok_batch=Tm, pad_idx=self.pad_idx, scale=scale,
                                         Dh=self.hd)
        else:
            native.attention_decode(stt.qkv, 3 * d, cache, 2 * d, Tm * 2 * d, cache[:, :, d:], 2 * d, Tm * 2 * d, stt.o,
                                    d, stt.B, self.H, pos=stt.pos, key_tokens=stt.ids, tok_batch=Tm,
                                    pad_idx=self.pad_idx, scale=scale, Dh=self.hd)

    def _attn_cross(self, stt: "DecodeState", l: int, scale: float):
        """The step's cross-attention of stt.q over the image memory's K | V rows of layer l -> stt.o; the K beams
        (or the samples) of an image share its one K/V. An fp8 state goes to the FP8 kernels (csrc/kv8.hip)."""
        d, S = self.d, stt.S
        if stt.kv8 is not None:
            k8, sc, H = stt.kv8[l], stt.kv_scale[l], self.H
            native.attention_decode_fp8(stt.q, d, k8, 2 * d, S * 2 * d, k8[:, d:], 2 * d, S * 2 * d, sc, sc[:, H:], 2 * H,
                                        stt.o, d, stt.B, H, Lk=S, group=stt.K or stt.group, scale=scale, Dh=self.hd)
            return
        kvl = stt.kv[l]
        if stt.K or stt.group > 1:  # the slots (beam) or samples of an image read its one K/V
            native.attention_decode_beam(stt.q, d, kvl, 2 * d, S * 2 * d, kvl[:, d:], 2 * d, S * 2 * d, stt.o, d, stt.B,
                                         self.H, Lk=S, group=stt.K or stt.group, scale=scale, Dh=self.hd)
        else:
            native.attention_decode(stt.q, d, kvl, 2 * d, S * 2 * d, kvl[:, d:], 2 * d, S * 2 * d,
                                    stt.o, d, stt.B, self.H, Lk=S, scale=scale, Dh=self.hd)

    def _step_body(self, stt: "DecodeState") -> torch.Tensor:
        """One token step up to the vocabulary head's operand [B, d] (unfused: any dtype)."""
        d, L = self.d, self.L
        st, w = self.store, self.store.w
        B, Tm = stt.B, stt.max_len
        self._embed_step(stt)
        x = stt.x
        for l in range(L):
            pre = f"layers.{l}."
            cache = stt.cache[l]
            native.linear(x, w(pre + "self_in.weight"), stt.qkv, bias=st.p(pre + "self_in.bias"))
            if stt.row_pos is not None:
                native.kv_store_ragged(stt.qkv[:, d:], 3 * d, cache, 2 * d, Tm * 2 * d, B, 2 * d, stt.row_pos)
            else:
                native.kv_store(stt.qkv[:, d:], 3 * d, cache, 2 * d, Tm * 2 * d, B, 2 * d, stt.pos)
            self._attn_self(stt, cache, 1.0 / math.sqrt(self.hd))
            native.linear(stt.o, w(pre + "self_out.weight"), stt.y, bias=st.p(pre + "self_out.bias"))
            native.layernorm_fwd(x, st.p(pre + "norm1.weight"), st.p(pre + "norm1.bias"), 1e-5, stt.x1, r=stt.y)
            native.linear(stt.x1, w(pre + "cross_q.weight"), stt.q, bias=st.p(pre + "cross_q.bias"))
            self._attn_cross(stt, l, 1.0 / math.sqrt(self.hd))
            native.linear(stt.o, w(pre + "cross_out.weight"), stt.y, bias=st.p(pre + "cross_out.bias"))
            native.layernorm_fwd(stt.x1, st.p(pre + "norm2.weight"), st.p(pre + "norm2.bias"), 1e-5, stt.x2, r=stt.y)
            native.linear(stt.x2, w(pre + "linear1.weight"), stt.h, bias=st.p(pre + "linear1.bias"),
                          act=native.ACT_RELU)
            native.linear(stt.h, w(pre + "linear2.weight"), stt.y, bias=st.p(pre + "linear2.bias"))
            native.layernorm_fwd(stt.x2, st.p(pre + "norm3.weight"), st.p(pre + "norm3.bias"), 1e-5, x, r=stt.y)
        return x

    def _decode_step_fused(self, stt: "DecodeState"):
        """decode_step on bf16 with 8 GEMM/attention launches per layer (was 12): every post-LN residual
        block (transformer.py:1144-1153) is z = sublayer + LN_prev(z_prev) written in f32 by the
        GEMM that produces the sublayer output, and LN(z) is applied by its consumers (the next
        GEMM's operand staging / residual epilogue); the self-attention K|V row goes straight from the
        in_proj GEMM into the cache; the vocabulary head leaves each row's argmax as a packed atomic max
        (no logits in HBM) and the pick reads it and advances the position."""
        x = self._step_body_fused(stt)
        w, p, V = self.store.w, self.store.p, self.V
        # the head on the 128x128 GEMM with the argmax epilogue (mit_gemm argmax_keys): one round of 158 blocks,
        # ~10 us, against ~20 us for mit_decode_gemm's 628 split-K 64x64 blocks at one per CU
        # (per token step, 3 interleaved processes on one box: 667 -> 658 us, 383.7 k -> 389.0 k tokens/s)
        native.gemm(x, w("fc_out.weight")[:V], None, stt.B, V, self.d, bias=p("fc_out.bias")[:V], argmax_keys=stt.keys)
        native.greedy_pick_keys(stt.keys, stt.ids, stt.pos, stt.end_id, self.pad_idx, stt.finished, stt.n_finished)

    def _step_body_fused(self, stt: "DecodeState") -> torch.Tensor:
        """The fused bf16 token step up to the vocabulary head's operand: LN3 of the last layer in bf16 [B, d]."""
        d, L = self.d, self.L
        w, p = self.store.w, self.store.p
        Tm = stt.max_len
        z1, z2, z3 = stt.z
        s1, s2, s3 = stt.zst
        scale = 1.0 / math.sqrt(self.hd)
        self._embed_step(stt)
        for l in range(L):
            pre = f"layers.{l}."
            cache = stt.cache[l]
            if l == 0:
                a, a_ln = stt.x, None
            else:
                q3 = f"layers.{l - 1}.norm3."
                a, a_ln = z3, (s3, p(q3 + "weight"), p(q3 + "bias"))
            ln1 = (s1, p(pre + "norm1.weight"), p(pre + "norm1.bias"))
            ln2 = (s2, p(pre + "norm2.weight"), p(pre + "norm2.bias"))
            if stt.row_pos is not None:
                # per-row cache rows: the in_proj without its cache epilogue, then the K|V columns of stt.qkv (the
                # same bf16 values the epilogue would have stored) to cache row row_pos[b] of each row
                native.decode_gemm(a, w(pre + "self_in.weight"), out=stt.qkv, bias=p(pre + "self_in.bias"), a_ln=a_ln)
                native.kv_store_ragged(stt.qkv[:, d:], 3 * d, cache, 2 * d, Tm * 2 * d, stt.B, 2 * d, stt.row_pos)
            else:
                native.decode_gemm(a, w(pre + "self_in.weight"), out=stt.qkv, bias=p(pre + "self_in.bias"), a_ln=a_ln,
                                   cache=cache, c_row=2 * d, c_batch=Tm * 2 * d, kv_col0=d, pos=stt.pos)
            self._attn_self(stt, cache, scale)
            native.decode_gemm(stt.o, w(pre + "self_out.weight"), bias=p(pre + "self_out.bias"), residual=a, r_ln=a_ln,
                               z_out=z1, stats_out=s1)
            native.decode_gemm(z1, w(pre + "cross_q.weight"), out=stt.q, bias=p(pre + "cross_q.bias"), a_ln=ln1)
            self._attn_cross(stt, l, scale)
            native.decode_gemm(stt.o, w(pre + "cross_out.weight"), bias=p(pre + "cross_out.bias"), residual=z1,
                               r_ln=ln1, z_out=z2, stats_out=s2)
            native.decode_gemm(z2, w(pre + "linear1.weight"), out=stt.h, bias=p(pre + "linear1.bias"),
                               act=native.ACT_RELU, a_ln=ln2)
            native.decode_gemm(stt.h, w(pre + "linear2.weight"), bias=p(pre + "linear2.bias"), residual=z2, r_ln=ln2,
                               z_out=z3, stats_out=s3)
        q3 = f"layers.{L - 1}.norm3."
        native.decode_layernorm(z3, s3, p(q3 + "weight"), p(q3 + "bias"), stt.x)
        return stt.x

    # --- rolling-batch greedy decode: one position per row, slots refilled (csrc/rolling.hip) -----------
    def rolling_begin(self, S: int, slots: int, max_len: int, start_id: int, end_id: int, pool: Optional[int] = None,
                      kv_dtype: Optional[str] = None) -> "RollingState":
        """Allocate a rolling decode of `slots` rows over memories of S rows and a K/V pool of `pool` images (default
        `slots`). Every slot starts empty (RollingState); rolling_fill puts images into the pool, rolling_admit hands
        pool images to slots, rolling_step advances every slot that is not done by one token."""
        if max_len > self.pe.shape[0]:
            raise ValueError(f"max_len {max_len} exceeds the positional table ({self.pe.shape[0]} = "
                             f"decoder_max_seq_len; the reference's PositionalEncoding would fail too)")
        if slots < 1 or (pool is not None and pool < 1):
            raise ValueError(f"rolling decode needs slots >= 1 and pool >= 1 (got {slots}, {pool})")
        if max_len < 2:
            raise ValueError("rolling decode needs max_len >= 2 (a cap of 1 takes no slot)")
        return RollingState(self, slots, S, max_len, start_id, end_id, pool=pool, kv_dtype=kv_dtype)

    def rolling_fill(self, stt: "RollingState", mem: torch.Tensor, mem_ld: int, S: int, n: int, at: int = 0):
        """The cross-attention K/V of the n freshly encoded images of mem [n*S, d] (row stride mem_ld) into pool
        entries at .. at+n-1: _cross_kv_begin's GEMMs (and FP8 quantisation, whose scales are per (layer, image,
        head) and so do not depend on the other images of the chunk)."""
        if S != stt.S or n < 0 or at < 0 or at + n > stt.pool:
            raise ValueError(f"rolling_fill: {n} images of {S} rows at pool entry {at} do not fit a pool of {stt.pool} "
                             f"images of {stt.S} rows")
        if n:
            self._cross_kv_begin(_PoolView(stt, at, n), mem, mem_ld, S, n)

    def rolling_admit(self, stt: "RollingState", triples):
        """One mit_slot_admit launch for the (slot, pool entry, cap) triples: each slot gets the entry's K/V, START,
        position 0, done = 0 and limit = cap (2 <= cap <= max_len). The host must have taken a slot's ids before it
        is named here. No triples: no launch."""
        m = len(triples)
        if m == 0:
            return
        for s_, e_, c_ in triples:
            if not (0 <= s_ < stt.slots and 0 <= e_ < stt.pool and 2 <= c_ <= stt.max_len):
                raise ValueError(f"rolling_admit: bad triple (slot {s_}, pool entry {e_}, cap {c_})")
        if len({t[0] for t in triples}) != m:
            raise ValueError("rolling_admit: a slot is named twice")
        if stt.triples_ev is not None:  # the previous admission's copy out of the pinned triples has run
            stt.triples_ev.synchronize()
        stt.triples_host[:m] = torch.tensor(triples, dtype=torch.int64)
        stt.triples[:m].copy_(stt.triples_host[:m], non_blocking=True)
        if stt.triples_host.is_pinned():
            stt.triples_ev = torch.cuda.Event()
            stt.triples_ev.record()
        fp8 = stt.kv8 is not None
        native.slot_admit(stt.triples, m, stt.pool_kv8 if fp8 else stt.pool_kv, stt.kv8 if fp8 else stt.kv, stt.S,
                          stt.pool_scale, stt.kv_scale, stt.ids, stt.start_id, stt.row_pos, stt.done, stt.limit,
                          stt.n_done)

    def rolling_step(self, stt: "RollingState"):
        """One greedy token for every slot that is not done, each at its own position row_pos[b] -> ids[b, p + 1];
        a done (or empty) slot is frozen. The launch list does not depend on the state (admission is a separate
        launch), so one recording replays for every step. The fused bf16 step keeps the head's argmax epilogue."""
        if stt.fused:
            x = self._step_body_fused(stt)
            w, p, V = self.store.w, self.store.p, self.V
            native.gemm(x, w("fc_out.weight")[:V], None, stt.B, V, self.d, bias=p("fc_out.bias")[:V],
                        argmax_keys=stt.keys)
            native.greedy_pick_keys_ragged(stt.keys, stt.ids, stt.row_pos, stt.end_id, stt.limit, stt.done, stt.n_done)
            return
        x = self._step_body(stt)
        st, w = self.store, self.store.w
        native.linear(x, w("fc_out.weight"), stt.logits, bias=st.p("fc_out.bias"))
        native.greedy_pick_ragged(stt.logits, stt.ids, stt.row_pos, stt.end_id, stt.limit, stt.done, stt.n_done,
                                  V=self.V)

    # --- rolling-batch decode, sampled and constrained (mit_*_ragged of constrain.hip / sample.hip) ------
    def rolling_stream_begin(self, S: int, slots: int, max_len: int, start_id: int, end_id: int,
                             pool: Optional[int] = None, kv_dtype: Optional[str] = None,
                             temperature: Optional[float] = None, top_k: int = 0, top_p: float = 1.0, seed: int = 0,
                             constraints: Optional[DecodeConstraints] = None,
                             prompt_table: Optional[torch.Tensor] = None) -> "RollingState":
        """rolling_begin with the opt-in state of sampled / constrained decode (RollingState._stream_init).
        temperature None: greedy picks. constraints: the row-independent settings (penalty, n-gram, minimum length,
        suppress list); prompts come as prompt_table (int64 [n, Lp + 1], column j + 1 = prompt token j, -1 = free),
        which a slot's prompt_idx points into. Slots are admitted with rolling_admit_ex and stepped with
        rolling_stream_step."""
        if max_len > self.pe.shape[0]:
            raise ValueError(f"max_len {max_len} exceeds the positional table ({self.pe.shape[0]} = "
                             f"decoder_max_seq_len; the reference's PositionalEncoding would fail too)")
        if slots < 1 or (pool is not None and pool < 1):
            raise ValueError(f"rolling decode needs slots >= 1 and pool >= 1 (got {slots}, {pool})")
        if max_len < 2:
            raise ValueError("rolling decode needs max_len >= 2 (a cap of 1 takes no slot)")
        if temperature is not None and (not temperature > 0 or not top_p > 0 or top_k < 0):
            raise ValueError(f"sampling needs temperature > 0, top_p > 0 and top_k >= 0 (got {temperature}, {top_p}, "
                             f"{top_k})")
        return RollingState(self, slots, S, max_len, start_id, end_id, pool=pool, kv_dtype=kv_dtype,
                            stream=dict(temperature=temperature, top_k=top_k, top_p=top_p, seed=seed,
                                        constraints=constraints, prompt_table=prompt_table))

    def rolling_admit_ex(self, stt: "RollingState", records):
        """rolling_admit for the opt-in state: one mit_slot_admit_ex launch for the (slot, pool entry, cap, row id,
        prompt index) records, which also resets each slot's row id, prompt index, log-probability and length."""
        m = len(records)
        if m == 0:
            return
        n_prompts = stt.forced.shape[0] if stt.forced is not None else 0
        for s_, e_, c_, _r, pi in records:
            if not (0 <= s_ < stt.slots and 0 <= e_ < stt.pool and 2 <= c_ <= stt.max_len and pi < n_prompts):
                raise ValueError(f"rolling_admit_ex: bad record (slot {s_}, pool entry {e_}, cap {c_}, prompt {pi})")
        if len({t[0] for t in records}) != m:
            raise ValueError("rolling_admit_ex: a slot is named twice")
        if stt.triples_ev is not None:  # the previous admission's copy out of the pinned records has run
            stt.triples_ev.synchronize()
        stt.records_host[:m] = torch.tensor(records, dtype=torch.int64)
        stt.records[:m].copy_(stt.records_host[:m], non_blocking=True)
        if stt.records_host.is_pinned():
            stt.triples_ev = torch.cuda.Event()
            stt.triples_ev.record()
        fp8 = stt.kv8 is not None
        native.slot_admit_ex(stt.records, m, stt.pool_kv8 if fp8 else stt.pool_kv, stt.kv8 if fp8 else stt.kv, stt.S,
                             stt.pool_scale, stt.kv_scale, stt.ids, stt.start_id, stt.row_pos, stt.done, stt.limit,
                             stt.n_done, stt.row_id, stt.prompt_idx, stt.logprob, stt.length)

    def _rolling_logits(self, stt: "RollingState"):
        """The step's body and the head as a plain GEMM into f32 logits (as sample_step / _decode_step_constrained),
        then, with active constraints, their per-row launch."""
        x = self._step_body_fused(stt) if stt.fused else self._step_body(stt)
        st, w = self.store, self.store.w
        native.linear(x, w("fc_out.weight"), stt.logits, bias=st.p("fc_out.bias"))
        c = stt.cons
        if c is not None:
            native.logits_constrain_ragged(stt.logits, self.V, stt.ids, stt.row_pos, done=stt.done,
                                           repetition_penalty=c.repetition_penalty, no_repeat_ngram=c.no_repeat_ngram,
                                           min_length=c.min_length, end_id=stt.end_id, suppress=stt.suppress,
                                           forced=stt.forced, prompt_idx=stt.prompt_idx)

    def rolling_sample_step(self, stt: "RollingState"):
        """One sampled token for every slot that is not done, each at its own position and from its own random
        stream (seed, row_id[b], row_pos[b]); a done (or empty) slot is frozen. The launch list does not depend on
        the state, so one recording replays between admissions."""
        self._rolling_logits(stt)
        native.sample_pick_ragged(stt.logits, self.V, stt.temperature, stt.top_k, stt.top_p, stt.seed, stt.row_id, None,
                                  stt.ids, stt.row_pos, stt.end_id, stt.limit, stt.done, stt.n_done, stt.logprob,
                                  stt.length)

    def rolling_step_constrained(self, stt: "RollingState"):
        """rolling_step with active constraints: the folded argmax of the fused head gives way to f32 logits in
        memory, which the per-row constraint launch edits before the ragged pick reads them."""
        self._rolling_logits(stt)
        native.greedy_pick_ragged(stt.logits, stt.ids, stt.row_pos, stt.end_id, stt.limit, stt.done, stt.n_done,
                                  V=self.V)

    def rolling_stream_step(self, stt: "RollingState"):
        """The token step of an opt-in state: sampled when it has a temperature, else greedy -- constrained when
        constraints are active, else rolling_step itself."""
        if stt.temperature is not None:
            return self.rolling_sample_step(stt)
        if stt.cons is not None:
            return self.rolling_step_constrained(stt)
        return self.rolling_step(stt)

    # --- beam search on the same step (csrc/beam.hip) ---------------------------------------------------
    def beam_begin(self, mem: torch.Tensor, mem_ld: int, S: int, B: int, K: int, max_len: int, start_id: int,
                   end_id: int, constraints: Optional[DecodeConstraints] = None,
                   kv_dtype: Optional[str] = None) -> "BeamState":
        """Set up a beam search of K slots per image over B images (memory rows mem [B*S, d], row stride
        mem_ld): the cross-attention K/V of every layer computed once per IMAGE (its K beams share it), empty
        slot-ordered self-attention caches for the B*K rows, START in every slot, score 0 in slot 0 and -inf in
        the others, position 0 on the device. constraints: DecodeConstraints; an image's prompt is forced on its K
        beams, and scores are log_softmax of the constrained rows."""
        if max_len > self.pe.shape[0]:
            raise ValueError(f"max_len {max_len} exceeds the positional table ({self.pe.shape[0]} = "
                             f"decoder_max_seq_len; the reference's PositionalEncoding would fail too)")
        if not 1 <= K <= 8 or K > self.V:
            raise ValueError(f"beam_size {K} must be in 1..8 and at most the vocabulary ({self.V})")
        if max_len < 2:
            raise ValueError("beam search needs max_len >= 2")
        stt = BeamState(self, B, K, S, max_len, start_id, end_id, kv_dtype=kv_dtype)
        self._constrain_begin(stt, constraints, B, K)
        self._cross_kv_begin(stt, mem, mem_ld, S, B)
        return stt

    def beam_step(self, stt: "BeamState"):
        """One token for every beam: the greedy step's body with the ancestry-gathered attention, the head as a
        plain GEMM into f32 logits [B*K, padded_vocab], with active constraints their launch on those rows (each
        beam's history read through the ancestor table), then the selection (which advances the position).
        No host synchronisation: recordable and capturable like decode_step."""
        x = self._step_body_fused(stt) if stt.fused else self._step_body(stt)
        st, w = self.store, self.store.w
        native.linear(x, w("fc_out.weight"), stt.logits, bias=st.p("fc_out.bias"))
        if stt.cons is not None:
            self._constrain(stt)
        native.beam_select(stt.logits, self.V, stt.score, stt.ids, stt.anc, stt.pos, stt.end_id, self.pad_idx,
                           stt.finished, stt.length, stt.n_finished, stt.ws, stt.images, stt.K)

    # --- sampling on the same step (csrc/sample.hip) ------------------------------------------------------
    def sample_begin(self, mem: torch.Tensor, mem_ld: int, S: int, B: int, N: int, max_len: int, start_id: int,
                     end_id: int, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, seed: int = 0,
                     row0: int = 0, constraints: Optional[DecodeConstraints] = None,
                     kv_dtype: Optional[str] = None) -> "SampleState":
        """Set up a sampled decode of N samples per image over B images (memory rows mem [B*S, d], row stride
        mem_ld): the cross-attention K/V of every layer computed once per IMAGE, an empty self-attention cache per
        row, START in every row, log-probability 0, position 0 on the device. Row r draws with the uniform of
        (seed, row0 + r, position). constraints: DecodeConstraints; an image's prompt is forced on its N samples,
        and log-probabilities are log_softmax of the constrained rows."""
        if max_len > self.pe.shape[0]:
            raise ValueError(f"max_len {max_len} exceeds the positional table ({self.pe.shape[0]} = "
                             f"decoder_max_seq_len; the reference's PositionalEncoding would fail too)")
        if max_len < 2:
            raise ValueError("sampling needs max_len >= 2")
        if N < 1:
            raise ValueError(f"num_samples {N} must be at least 1")
        if not temperature > 0 or not top_p > 0 or top_k < 0:
            raise ValueError(f"sampling needs temperature > 0, top_p > 0 and top_k >= 0 (got {temperature}, {top_p}, "
                             f"{top_k})")
        stt = SampleState(self, B, N, S, max_len, start_id, end_id, temperature, top_k, top_p, seed, row0,
                          kv_dtype=kv_dtype)
        self._constrain_begin(stt, constraints, B, N)
        self._cross_kv_begin(stt, mem, mem_ld, S, B)
        return stt

    def sample_step(self, stt: "SampleState"):
        """One sampled token for every row: the greedy step's body (each row attends over its own cache, the N
        samples of an image over its one cross-attention K/V), the head as a plain GEMM into f32 logits
        [B*N, padded_vocab], with active constraints their launch on those rows, then the pick (which advances the
        position). No host synchronisation: recordable and capturable like decode_step."""
        x = self._step_body_fused(stt) if stt.fused else self._step_body(stt)
        st, w = self.store, self.store.w
        native.linear(x, w("fc_out.weight"), stt.logits, bias=st.p("fc_out.bias"))
        if stt.cons is not None:
            self._constrain(stt)
        native.sample_pick(stt.logits, self.V, stt.temperature, stt.top_k, stt.top_p, stt.seed, stt.row0, None, stt.ids,
                           stt.pos, stt.end_id, self.pad_idx, stt.finished, stt.n_finished, stt.logprob, stt.length,
                           stt.ticket)

    def forward_ops(self, tokens: torch.Tensor, mem: torch.Tensor, S: int, params: Dict[str, torch.Tensor],
                    seed: Optional[torch.Tensor], drop_p: float, mem_keys: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The forward of run_forward built from torch.ops.mit_hip operators (ops.py), so torch's autograd
        records it and ``loss.backward()`` runs each op's HIP backward (the reference loop, train.py:80-100).
        tokens int64 [B, T]; mem [B*S, d] memory rows (may require grad: the projection's output);
        params: the trainable f32 tensors by flat entry name (the model's nn.Parameters), whose compute-dtype
        shadows (store.w) the GEMMs read. Returns f32 logits [B, T, V]. Same kernels, dropout sites and
        seeds as run_forward: the same values."""
        import ops
        mh = ops.load()
        B, T = tokens.shape
        d, H, L = self.d, self.H, self.L
        st = self.store
        lp = (lambda n: st.w(n)) if st.shadow is not st.master else (lambda n: None)  # noqa: E731
        P = params
        sc = 1.0 / math.sqrt(self.hd)
        x = mh.embedding(tokens, P["token_embedding.weight"], self.pe, math.sqrt(d), drop_p, seed, EMB_SITE,
                         lp("token_embedding.weight"), self.pad_idx)
        kv = mh.linear(mem, P["cross_kv.weight"], P["cross_kv.bias"], weight_lp=lp("cross_kv.weight")).view(B, S, L * 2 * d)
        for l in range(L):
            q = f"layers.{l}."
            base = 64 * l

            def lin(t, n):
                return mh.linear(t, P[q + n + ".weight"], P[q + n + ".bias"], weight_lp=lp(q + n + ".weight"))

            def ln(t, r, k, site):
                return mh.layer_norm_train(t, P[q + f"norm{k}.weight"], P[q + f"norm{k}.bias"], 1e-5, r, drop_p, seed,
                                           site)[0]
            qkv = lin(x, "self_in")
            o = mh.attention_train(qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:], H, True, sc, tokens,
                                   self.pad_idx, drop_p, seed, base + 0)[0]
            x1 = ln(x, lin(o, "self_out"), 1, base + 1)
            kvl = kv[..., l * 2 * d:(l + 1) * 2 * d]
            oc = mh.attention_train(lin(x1, "cross_q"), kvl[..., :d], kvl[..., d:], H, False, sc, mem_keys, 0, drop_p,
                                    seed, base + 2)[0]
            x2 = ln(x1, lin(oc, "cross_out"), 2, base + 3)
            y = mh.ffn(x2, P[q + "linear1.weight"], P[q + "linear1.bias"], P[q + "linear2.weight"],
                       P[q + "linear2.bias"], drop_p, seed, base + 4, lp(q + "linear1.weight"),
                       lp(q + "linear2.weight"))[0]
            x = ln(x2, y, 3, base + 5)
        logits = mh.linear(x, P["fc_out.weight"], P["fc_out.bias"], out_f32=True, weight_lp=lp("fc_out.weight"))
        return logits if self.Vp == self.V else logits[..., :self.V]

    def forward(self, tgt_tokens: torch.Tensor, memory: torch.Tensor, memory_padding_mask=None) -> torch.Tensor:
        """decoder.py:134-193: f32 logits [B, T, V] (no autograd; training goes through the model's
        train step). memory_padding_mask: bool [B, S], True = padded memory position, masked out of
        the cross-attention (memory_key_padding_mask, decoder.py:179-186); a query whose memory is
        all padding gets NaN, like the reference."""
        tokens = tgt_tokens.to(self.device, torch.int64).contiguous()
        B, T = tokens.shape
        S = memory.shape[1]
        self.store.ensure_shadow(force=True)
        mem = memory.to(self.device, self.dtype).reshape(B * S, self.d).contiguous()
        keys = None
        if memory_padding_mask is not None:
            if tuple(memory_padding_mask.shape) != (B, S):
                raise ValueError(f"memory_padding_mask must be [B, S] = {(B, S)}, got {tuple(memory_padding_mask.shape)}")
            keys = (~memory_padding_mask.to(self.device, torch.bool)).to(torch.int64).contiguous()
        A = self.acts(B, T, S, False)
        out = torch.empty(B * T, self.Vp, dtype=torch.float32, device=self.device)
        self.run_forward(tokens, mem, self.d, S, A, None, False, logits_out=out, mem_keys=keys)
        return self.unpad_logits(out, B, T)

    __call__ = forward

    def unpad_logits(self, out: torch.Tensor, B: int, T: int) -> torch.Tensor:
        """[B*T, Vp] head output -> [B, T, V] (a copy only when V is not a multiple of 8)."""
        if self.Vp == self.V:
            return out.view(B, T, self.V)
        return out[:, :self.V].reshape(B, T, self.V)

    def flops_per_sequence(self, T: int, S: int) -> float:
        """Algorithmic forward FLOPs for one caption (SURVEY.md §8d convention)."""
        d, F, V, L = self.d, self.F, self.V, self.L
        layer = 2 * T * 3 * d * d + 2 * T * d * d + 4 * T * T * d + 2 * T * d * d + 2 * S * 2 * d * d + 4 * T * S * d \
            + 2 * T * d * d + 2 * T * 2 * d * F
        return L * layer + 2 * T * d * V
