"""ImageToTextModel: frozen vision encoder + projection + Transformer decoder (reference model.py:12-255).

Drop-in surface:
  * ``ImageToTextModel(decoder_vocab_size, decoder_embed_dim, decoder_heads, decoder_layers,
    decoder_ff_dim, decoder_max_seq_len, decoder_dropout, decoder_pad_idx)`` (model.py:14-16), the
    encoder chosen by config.ENCODER_MODEL_NAME;
  * ``forward(image_tensors f32[B,3,H,W], tgt_tokens i64[B,T]) -> f32[B,T,V]`` (model.py:116-169);
  * ``generate(image, start_token_id, end_token_id, max_len=100, method='greedy', beam_size=3)``
    (model.py:171-255);
  * ``state_dict()`` / ``load_state_dict()`` in the reference's key names.
Added for the MI355X path:
  * ``train_step(images, decoder_input_tokens, target_tokens, dist=None)``: the whole of
    train.py:75-93 (forward, CE(ignore PAD), backward) as one kernel sequence with no host sync,
    returning the loss as a device scalar; ``optim.AdamW.step(clip)`` finishes train.py:96-100.
  * ``memory_mode`` "cls" (reference: CLS token only, model.py:141) or "patches" (north star:
    cross-attention over the projected patch sequence).
"""
from __future__ import annotations

import math
import os
from collections import OrderedDict
from typing import Dict, Iterator, List, Optional, Tuple

import torch

import config
import data
import native
import rolling
from decoder import (DecodeConstraints, TransformerDecoder, decoder_entries, flat_to_reference, reference_to_flat,
                     resolve_kv_dtype)
from encoder import VisionEncoder, build_encoder
from params import FlatParams

def _dtype_from_config(dtype):
    if dtype is None:
        dtype = config.DTYPE
    if isinstance(dtype, torch.dtype):
        return dtype
    return {"bf16": torch.bfloat16, "bfloat16": torch.bfloat16, "fp32": torch.float32, "float32": torch.float32}[dtype]


# encoder chunks (VisionEncoder.forward_iter: patch embedding, layers, final LayerNorm) of the prefetched
# next batch issued before the decoder's first launch (train step); 0 / 1 / 2 / 4 / all measured within
# 0.3 % of each other
ENC_LEAD = 1

class GraphedStep:
    """A captured train step. step(images, decoder_input_tokens, target_tokens) copies a batch into
    the static buffers (skip by passing nothing) and replays; returns the loss device scalar. The
    learning rate is a device scalar the graph reads, refreshed from optimizer.param_groups before
    every replay (a scheduler's change takes effect like in the eager loop)."""

    def __init__(self, graph, images, dec_in, targets, loss, optimizer=None):
        self.graph, self.images, self.dec_in, self.targets, self.loss = graph, images, dec_in, targets, loss
        self.optimizer = optimizer

    def __call__(self, images=None, decoder_input_tokens=None, target_tokens=None):
        if images is not None:
            self.images.copy_(images, non_blocking=True)
            self.dec_in.copy_(decoder_input_tokens, non_blocking=True)
            self.targets.copy_(target_tokens, non_blocking=True)
        if self.optimizer is not None:
            self.optimizer._sync_lr()
        self.graph.replay()
        return self.loss


def rank_beams(ids: List[List[int]], scores: List[float], lengths: List[int], K: int, length_penalty: float = 0.0,
               return_all: bool = False):
    """Final ranking of a beam search (host): rows are image-major, slot-minor; per image the slots sorted by
    score / length**length_penalty, best first, ties to the lower slot. Returns per image the best ids, or with
    return_all the K (ids, score) pairs in rank order."""
    out = []
    for b in range(len(ids) // K):
        rows = range(b * K, (b + 1) * K)
        order = sorted(rows, key=lambda r: (-(scores[r] / max(lengths[r], 1) ** length_penalty), r))
        out.append([(ids[r], scores[r]) for r in order] if return_all else ids[order[0]])
    return out


class ImageToTextModel:
    def __init__(self, decoder_vocab_size: int, decoder_embed_dim: int, decoder_heads: int, decoder_layers: int,
                 decoder_ff_dim: int, decoder_max_seq_len: int, decoder_dropout: float, decoder_pad_idx: int, *,
                 encoder: Optional[VisionEncoder] = None, memory_mode: Optional[str] = None, dtype=None, device=None,
                 seed: Optional[int] = None):
        native.require_gpu()
        native.load_library()
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.dtype = _dtype_from_config(dtype)
        seed = config.RANDOM_SEED if seed is None else seed
        self.encoder = encoder if encoder is not None else build_encoder(device=self.device, dtype=self.dtype,
                                                                          seed=seed)
        if self.encoder.dtype != self.dtype:
            raise ValueError("encoder and model compute dtypes differ")
        self.memory_mode = memory_mode or config.MEMORY_MODE
        if self.memory_mode not in ("cls", "patches"):
            raise ValueError(f"memory_mode must be 'cls' or 'patches', got {self.memory_mode}")
        self.encoder.configure_for(self.memory_mode)  # residual-stream precision for this memory (encoder.py)
        self.encoder_output_dim = self.encoder.hidden_size
        self.decoder_embed_dim = decoder_embed_dim
        self.decoder_pad_idx = decoder_pad_idx
        E, d = self.encoder_output_dim, decoder_embed_dim
        self.has_projection = E != d  # model.py:97-102: Linear if dims differ, else Identity
        self.store = FlatParams(decoder_entries(decoder_vocab_size, d, decoder_layers, decoder_ff_dim,
                                                E if self.has_projection else None), self.device, self.dtype)
        self.store.vocab = decoder_vocab_size
        # what optim.AdamW needs to speak torch.optim.AdamW's state_dict in the reference's parameter
        # order (frozen encoder tensors first: model.py:48-66 registers the encoder before the rest)
        self.store.layout = dict(V=decoder_vocab_size, d=d, L=decoder_layers, F=decoder_ff_dim,
                                 proj_in=E if self.has_projection else None,
                                 n_encoder_params=self.encoder.num_reference_params())
        self.decoder = TransformerDecoder(decoder_vocab_size, d, decoder_heads, decoder_layers, decoder_ff_dim,
                                          decoder_max_seq_len, decoder_dropout, decoder_pad_idx, store=self.store,
                                          device=self.device)
        self.decoder.init_weights(seed + 1)
        if self.has_projection:
            g = torch.Generator().manual_seed(seed + 2)
            b = 1.0 / math.sqrt(E)  # nn.Linear default init bounds
            self.store.p("projection.weight").copy_((torch.rand(d, E, generator=g) * 2 - 1) * b)
            self.store.p("projection.bias").copy_((torch.rand(d, generator=g) * 2 - 1) * b)
            self.store.sync_shadow()
        # the processor the encoder was trained with (model.py:69-83 loads AutoImageProcessor for the
        # encoder's name): ViT = bilinear resize + mean/std 0.5; CLIP = shortest-edge bicubic resize,
        # centre crop, CLIP mean/std — bit-identical to the HF processors (tests/test_data_*.py)
        self.image_processor = data.ImagePreprocessor(self.encoder.kind, self.encoder.image, self.device)
        self.training = True
        # dropout RNG state: a device counter (graph-replay safe), distinct per DP rank
        self.seed_t = torch.tensor([seed * 1000003], dtype=torch.int64, device=self.device)
        self._mem: Dict[tuple, torch.Tensor] = {}
        self._enc_stream = None
        self._enc_slot = 0
        self._prefetched = None
        self._slot_free = None           # native.HipEvents(2): end of the backward of the step that read slot i
        self._slot_freed = [False, False]  # slot i's event recorded since the slot was last read
        self._step_terms = None          # train_step_accum: {count, loss sum, loss} of the accumulated step
        self._params: Optional["OrderedDict[str, torch.nn.Parameter]"] = None
        self._gen = 0  # bumped by every forward that writes the shared arenas (autograd staleness check)

    # --- nn.Module-like surface ----------------------------------------------------------------
    def train(self, mode: bool = True):
        self.training = mode
        self.decoder.train(mode)
        return self

    def eval(self):
        return self.train(False)

    def to(self, device):
        if torch.device(device).type != self.device.type:
            raise ValueError("ImageToTextModel lives on the GPU it was built on")
        return self

    def _param_table(self) -> "OrderedDict[str, torch.nn.Parameter]":
        """One nn.Parameter per trainable flat entry, ALIASING the f32 master buffer (same storage
        and version counter): torch.optim.AdamW / clip_grad_norm_ update and read the very memory
        the kernels use; .grad is a view of the flat gradient buffer once a backward ran."""
        if self._params is None:
            self._params = OrderedDict((n, torch.nn.Parameter(self.store.p(n), requires_grad=True))
                                       for n in self.store.names())
            for n, p in self._params.items():
                p._mit_store = self.store  # optim.AdamW(model.parameters()) finds the flat buffers
                p.register_post_accumulate_grad_hook(self._grad_to_flat(n))
        return self._params

    def _grad_to_flat(self, name):
        """After autograd accumulated a parameter's gradient (model(images, tokens) -> loss.backward()):
        make p.grad the view of the flat gradient buffer (one copy when autograd created a new tensor),
        so clip_grad_norm_, torch.optim.AdamW, the fused optim.AdamW and the DP buckets all see it."""
        st = self.store

        def hook(p):
            g = st.g(name)
            if p.grad is not None and p.grad.data_ptr() != g.data_ptr():
                g.copy_(p.grad)
                p.grad = g
        return hook

    def parameters(self, recurse: bool = True) -> Iterator[torch.nn.Parameter]:
        """The trainable parameters (projection + decoder; the encoder is frozen, model.py:87-90)
        in flat-buffer order. Padded entries (the vocabulary head, decoder.padded_vocab) include
        their zero pad rows, which get exactly-zero gradients."""
        return iter(self._param_table().values())

    def named_parameters(self, prefix: str = "", recurse: bool = True) -> Iterator[Tuple[str, torch.nn.Parameter]]:
        for n, p in self._param_table().items():
            yield prefix + n, p

    def zero_grad(self, set_to_none: bool = True):
        for p in self._param_table().values():
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    def num_trainable(self) -> int:
        return sum(n for _, _, _, n in self.store.entries)

    def set_rank_seed(self, rank: int, seed: Optional[int] = None):
        """Dropout streams differ per data-parallel rank."""
        seed = config.RANDOM_SEED if seed is None else seed
        self.seed_t.fill_(seed * 1000003 + rank * 7919 * 65537)

    # --- memory (encoder -> projection) ----------------------------------------------------------
    def _encoder_rows(self, images: torch.Tensor, slot: int = 0):
        """Frozen encoder -> (enc_rows, enc_ld, S): the rows that feed the projection."""
        self.encoder.configure_for(self.memory_mode)  # memory_mode may have changed since __init__ (cheap)
        B = images.shape[0]
        N, E = self.encoder.N, self.encoder.E
        if self.memory_mode == "cls":
            enc = self.encoder.forward(images, rows="cls", slot=slot)  # [B, E] view, row stride N*E
            return enc, N * E, 1
        enc = self.encoder.forward(images, rows="all", slot=slot)  # [B, N, E]
        return enc.reshape(B * N, E), E, N

    def _encoder_rows_iter(self, images: torch.Tensor, slot: int = 0):
        """_encoder_rows as a generator of launch chunks (VisionEncoder.forward_iter)."""
        self.encoder.configure_for(self.memory_mode)
        B = images.shape[0]
        N, E = self.encoder.N, self.encoder.E
        if self.memory_mode == "cls":
            enc = yield from self.encoder.forward_iter(images, rows="cls", slot=slot)
            return enc, N * E, 1
        if self.encoder.groups_for(B) == 2:  # CLIP-L towers at B = 64: two image groups on two streams
            enc = yield from self.encoder.forward_iter_groups(images, slot)
        else:
            enc = yield from self.encoder.forward_iter(images, rows="all", slot=slot)
        return enc.reshape(B * N, E), E, N

    def prefetch_encoder(self, images: torch.Tensor):
        """Start the frozen encoder's forward for the NEXT batch on a second stream; the next
        train_step(images) consumes it instead of recomputing. The encoder has no trainable state, so
        its output does not depend on the step in between: the result is identical, and its GEMMs
        fill the CUs the decoder's small kernels leave idle. Double-buffered arenas (slot 0/1)."""
        for _ in self.prefetch_encoder_iter(images):
            pass

    def prefetch_encoder_iter(self, images: torch.Tensor):
        """prefetch_encoder as a generator: each next() issues one launch chunk of the encoder forward
        (the patch embedding, one layer, the final LayerNorm) on the encoder stream. The train step
        interleaves the chunks with its decoder layers, so neither stream's launches wait behind the
        other's on the host (launches issue in program order, ~3.6 us each from a replayed plan)."""
        if self._enc_stream is None:
            self._enc_stream = torch.cuda.Stream(device=self.device)
            self._enc_events = native.HipEvents(8)
        slot = 1 - self._enc_slot
        images = images.to(self.device, non_blocking=True)
        enc = self._enc_stream.cuda_stream
        # the arena's previous reader (two steps back) is done: the encoder stream waits for the end of
        # that step's backward (its last read: the projection weight gradient; the encoder then runs
        # beside that step's HBM-bound clip + AdamW: +0.2 %), or for everything on main (the autograd
        # path records no slot event)
        if self._slot_freed[slot]:
            native.HipEvents.wait(enc, self._slot_free.pool[slot])
        else:
            self._enc_events.wait_stream(enc, native.stream_ptr())
        it = self._encoder_rows_iter(images, slot)
        while True:
            with torch.cuda.stream(self._enc_stream):  # (never left entered across a yield)
                try:
                    next(it)
                except StopIteration as e:
                    out = e.value
                    break
            yield
        ev = self._enc_events.record(enc)
        self._prefetched = (images, slot, out, ev)

    def _take_encoded(self, images: torch.Tensor):
        """The encoder rows for images: the prefetched ones when they are for these images (this stream
        waits for them), else computed here into the current arena."""
        pf, self._prefetched = self._prefetched, None
        if pf is not None and pf[0].data_ptr() == images.data_ptr() and pf[0].shape == images.shape:
            _, self._enc_slot, (enc_rows, enc_ld, S), ev = pf
            native.HipEvents.wait(native.stream_ptr(), ev)
            out = enc_rows, enc_ld, S
        else:
            out = self._encoder_rows(images, self._enc_slot)
        # the slot is being read again: a later prefetch into it must wait for this reader (re-armed by
        # _train_step once the step's readers are issued; every other caller leaves it unarmed, so the
        # prefetch waits for everything on the main stream)
        self._slot_freed[self._enc_slot] = False
        return out

    def _encode_memory(self, images: torch.Tensor, refresh: bool = True):
        """Returns (mem_rows, mem_ld, S, enc_rows, enc_ld): memory [B*S rows of d] and the
        encoder features that feed the projection (for its weight gradient). refresh: re-cast the
        bf16 weight shadow unconditionally (every path but the fused train step: params.ensure_shadow)."""
        B = images.shape[0]
        E, d = self.encoder.E, self.decoder_embed_dim
        self.store.ensure_shadow(force=refresh)
        self._gen += 1
        enc_rows, enc_ld, S = self._take_encoded(images)
        if not self.has_projection:
            return enc_rows, enc_ld, S, enc_rows, enc_ld
        key = (B, S)
        if key not in self._mem:
            self._mem[key] = torch.empty(B * S, d, dtype=self.dtype, device=self.device)
        mem = self._mem[key]
        native.gemm(enc_rows, self.store.w("projection.weight"), mem, B * S, d, E, lda=enc_ld,
                    bias=self.store.p("projection.bias"))
        return mem, d, S, enc_rows, enc_ld

    # --- forward (model.py:116-169) ------------------------------------------------------------
    def forward(self, image_tensors: torch.Tensor, tgt_tokens: torch.Tensor) -> torch.Tensor:
        """f32 logits [B, T, V]. With grad enabled and trainable parameters, the result carries an
        autograd node whose backward runs the HIP backward (the reference's loss.backward(),
        train.py:93); otherwise a forward-only launch sequence."""
        if torch.is_grad_enabled() and any(p.requires_grad for p in self._param_table().values()):
            return self._forward_ops(image_tensors, tgt_tokens)
        images = image_tensors.to(self.device)
        tokens = tgt_tokens.to(self.device, torch.int64).contiguous()
        B, T = tokens.shape
        mem, mem_ld, S, _, _ = self._encode_memory(images)
        A = self.decoder.acts(B, T, S, False)
        out = torch.empty(B * T, self.decoder.Vp, dtype=torch.float32, device=self.device)
        p = self.decoder.dropout if self.training else 0.0
        if p > 0:
            native.step_inc(self.seed_t)
        self.decoder.run_forward(tokens, mem, mem_ld, S, A, self.seed_t, False, logits_out=out, drop_p=p)
        return self.decoder.unpad_logits(out, B, T)

    __call__ = forward

    def _forward_ops(self, image_tensors, tgt_tokens):
        """model(images, tokens) under autograd (the reference loop, train.py:80-100): the frozen encoder
        runs as usual (no gradient), the projection and the decoder as torch.ops.mit_hip operators
        (ops.py, decoder.forward_ops) whose registered backward formulas run the HIP backward kernels.
        Parameter gradients land in the flat gradient buffer (see _param_table's hooks)."""
        import ops
        mh = ops.load()
        images = image_tensors.to(self.device)
        tokens = tgt_tokens.to(self.device, torch.int64).contiguous()
        B, T = tokens.shape
        self.store.ensure_shadow(force=True)
        self._gen += 1
        enc_rows, enc_ld, S = self._take_encoded(images)
        E = self.encoder_output_dim
        # the encoder arena is reused by the next forward: the projection's saved input is a copy
        enc = torch.as_strided(enc_rows, (B * S, E), (enc_ld, 1)).clone()
        P = self._param_table()
        p = self.decoder.dropout if self.training else 0.0
        seed = None
        if p > 0:
            native.step_inc(self.seed_t)
            seed = self.seed_t.clone()  # the backward regenerates this forward's masks whatever runs between
        if self.has_projection:
            st = self.store
            mem = mh.linear(enc, P["projection.weight"], P["projection.bias"],
                            weight_lp=st.w("projection.weight") if st.shadow is not st.master else None)
        else:
            mem = enc
        return self.decoder.forward_ops(tokens, mem, S, P, seed, p)

    # --- fused train step (train.py:75-93) -----------------------------------------------------
    def train_step(self, images: torch.Tensor, decoder_input_tokens: torch.Tensor, target_tokens: torch.Tensor,
                   dist=None, next_images: Optional[torch.Tensor] = None) -> torch.Tensor:
        """See _train_step. (Stream priorities for the step's own streams over the encoder prefetch
        measured neutral to -1.7 %, DESIGN.md §4.1c: all streams run at the default priority.)"""
        return self._train_step(images, decoder_input_tokens, target_tokens, dist, next_images)

    def _train_step(self, images: torch.Tensor, decoder_input_tokens: torch.Tensor, target_tokens: torch.Tensor,
                    dist=None, next_images: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Forward + CE(ignore PAD, mean over the GLOBAL non-PAD count) + backward into the flat
        gradient buffer. Returns the loss as a device scalar [1] (no host sync).
        next_images: the next batch's images, whose (frozen) encoder forward then runs on a second
        stream beside this step's decoder work (prefetch_encoder); results are unchanged."""
        targets = target_tokens.to(self.device, torch.int64, non_blocking=True).contiguous()

        def loss_terms(A):  # this step's own count, taken after the forward
            native.zero(A.count_loss)
            native.count_targets(targets, self.decoder_pad_idx, A.count)
            if dist is not None:
                dist.all_reduce_count(A.count)
            return A.count, A.loss_sum
        A = self._forward_backward(images, decoder_input_tokens, targets, loss_terms, next_images,
                                   dist.grads_ready if dist is not None else None)
        native.scalar_div(A.loss_sum, A.count, A.loss)
        if dist is not None:
            dist.finish_backward(A.loss)
        return A.loss

    def _forward_backward(self, images, decoder_input_tokens, targets, loss_terms, next_images, grads_ready):
        """One batch's forward, CE and backward into the flat gradient buffer (the body train_step and every
        micro-batch of train_step_accum share). loss_terms(A) -> (count, loss_sum), called between the
        forward and the CE: the device scalars the CE divides its gradient by and adds its loss to.
        Returns the activation arena."""
        images = images.to(self.device, non_blocking=True)
        tokens = decoder_input_tokens.to(self.device, torch.int64, non_blocking=True).contiguous()
        B, T = tokens.shape
        mem, mem_ld, S, enc_rows, enc_ld = self._encode_memory(images, refresh=False)
        pf = self.prefetch_encoder_iter(next_images) if next_images is not None else None

        def tick(n=1):
            nonlocal pf
            while pf is not None and n > 0:
                if next(pf, tick) is tick:  # exhausted: the prefetch is fully issued
                    pf = None
                n -= 1
        # the next batch's encoder: ENC_LEAD chunks now, then one per decoder layer (forward and backward),
        # the rest after the backward
        tick(ENC_LEAD)
        dec = self.decoder
        A = dec.acts(B, T, S, True)
        native.step_inc(self.seed_t)
        logits, _ = dec.run_forward(tokens, mem, mem_ld, S, A, self.seed_t, True, tick=tick)
        count, loss_sum = loss_terms(A)
        native.cross_entropy(logits, targets, self.decoder_pad_idx, count, loss_sum, True, row_loss=A.row_loss,
                             V=dec.V, ld=dec.Vp)
        proj = (enc_rows, enc_ld, self.encoder_output_dim) if self.has_projection else None
        dec.run_backward(tokens, mem, mem_ld, S, A, self.seed_t, logits, proj_input=proj,
                         grads_ready=grads_ready, tick=tick)
        tick(1 << 30)
        if self._enc_stream is not None:  # this step's last reader of its encoder slot is issued
            if self._slot_free is None:
                self._slot_free = native.HipEvents(2)
            self._slot_free.record_at(self._enc_slot, native.stream_ptr())
            self._slot_freed[self._enc_slot] = True
        return A

    def train_step_accum(self, micro_batches, dist=None, next_images: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One optimizer step's gradient over several micro-batches: a sequence of (images,
        decoder_input_tokens, target_tokens) whose B and T may differ. Equal to train_step on their
        concatenation: the non-PAD targets of ALL micro-batches are counted on the device before the first
        forward (all-reduced once under ``dist``), every micro-batch's CE divides by that one count, and the
        micro-batches' gradients are summed left to right into the flat gradient buffer (mit_grad_accumulate:
        FIRST / ADD / LAST through store.accum, one rounded f32 add each, bitwise reproducible), where
        optimizer.step, the DP all-reduce (once, after the last micro-batch: dist.finish_accumulated) and every
        reader of store.grad find it. Each micro-batch advances the dropout seed once; the frozen encoder of
        micro-batch i + 1 is prefetched beside micro-batch i, ``next_images`` (the next step's first
        micro-batch) beside the last. Returns the global mean loss as a device scalar [1]; no host sync, no
        torch kernel (recordable). One micro-batch is train_step itself, launch for launch."""
        mbs = list(micro_batches)
        if not mbs:
            raise ValueError("train_step_accum: no micro-batch")
        if len(mbs) == 1:
            return self._train_step(*mbs[0], dist=dist, next_images=next_images)
        pad = self.decoder_pad_idx
        targets = [tg.to(self.device, torch.int64, non_blocking=True).contiguous() for _, _, tg in mbs]
        if self._step_terms is None:  # {count, loss_sum, loss} of the step (an arena's own belong to one shape)
            self._step_terms = torch.empty(3, dtype=torch.float32, device=self.device)
        count, loss_sum, loss = self._step_terms[0:1], self._step_terms[1:2], self._step_terms[2:3]
        native.zero(self._step_terms[0:2])
        for tg in targets:
            native.count_targets(tg, pad, count)
        if dist is not None:
            dist.all_reduce_count(count)
        grad, acc = self.store.grad, self.store.ensure_accum()
        last = len(mbs) - 1
        for i, ((images, tokens, _), tg) in enumerate(zip(mbs, targets)):
            # without grads_ready: no bucket is final before the last accumulate
            self._forward_backward(images, tokens, tg, lambda A: (count, loss_sum),
                                   mbs[i + 1][0] if i < last else next_images, None)
            native.grad_accumulate(grad, acc, native.ACC_FIRST if i == 0 else native.ACC_LAST if i == last
                                   else native.ACC_ADD)
        native.scalar_div(loss_sum, count, loss)
        if dist is not None:
            dist.finish_accumulated(loss)
        return loss

    def make_graphed_step(self, optimizer, images, decoder_input_tokens, target_tokens, max_norm: float):
        """Capture train_step + optimizer.step(max_norm) (train.py:75-100, ~300 kernel launches) into
        ONE hipGraph over static input buffers. The two warm-up executions that size the arenas
        are undone (parameters, AdamW state and counters restored) before capture, so the graph
        starts from the same state the model had. Returns a GraphedStep (call it per batch)."""
        dev = self.device
        st_img = images.to(dev).clone()
        st_in = decoder_input_tokens.to(dev, torch.int64).clone()
        st_tg = target_tokens.to(dev, torch.int64).clone()
        store = self.store
        store.ensure_optimizer_state()
        saved = [t.clone() for t in (store.master, store.shadow, store.exp_avg, store.exp_avg_sq, optimizer.step_t,
                                     self.seed_t)]
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(2):
                self.train_step(st_img, st_in, st_tg)
                optimizer.step(max_norm)
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        for dst, src in zip((store.master, store.shadow, store.exp_avg, store.exp_avg_sq, optimizer.step_t,
                             self.seed_t), saved):
            dst.copy_(src)
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            loss = self.train_step(st_img, st_in, st_tg)
            optimizer.step(max_norm)
        return GraphedStep(graph, st_img, st_in, st_tg, loss, optimizer)

    @torch.no_grad()
    def eval_loss(self, images, decoder_input_tokens, target_tokens) -> torch.Tensor:
        """train.py:141-145 (forward + CE) without materialising f32 logits; device scalar."""
        images = images.to(self.device)
        tokens = decoder_input_tokens.to(self.device, torch.int64).contiguous()
        targets = target_tokens.to(self.device, torch.int64).contiguous()
        B, T = tokens.shape
        mem, mem_ld, S, _, _ = self._encode_memory(images)
        A = self.decoder.acts(B, T, S, False)
        logits, _ = self.decoder.run_forward(tokens, mem, mem_ld, S, A, self.seed_t, False, drop_p=0.0)
        native.zero(A.count)
        native.zero(A.loss_sum)
        native.count_targets(targets, self.decoder_pad_idx, A.count)
        native.cross_entropy(logits, targets, self.decoder_pad_idx, A.count, A.loss_sum, False, row_loss=A.row_loss,
                             V=self.decoder.V, ld=self.decoder.Vp)
        native.scalar_div(A.loss_sum, A.count, A.loss)
        return A.loss

    # --- scoring -------------------------------------------------------------------------------
    def _caption_sequences(self, captions, B: int, start_token_id: int, end_token_id: int) -> torch.Tensor:
        """The candidates of score_captions as one int64 [B, C, L] CPU tensor of START .. END sequences padded with
        pad_idx; every check of the candidates happens here, on the host, before anything is launched."""
        pad, V = self.decoder_pad_idx, self.decoder.V
        start, end = int(start_token_id), int(end_token_id)
        min_len = 0
        if isinstance(captions, torch.Tensor):
            if captions.dim() != 3 or captions.shape[0] != B:
                raise ValueError(f"score_captions: a caption tensor must be [B, C, L] with B = {B}, got "
                                 f"{tuple(captions.shape)}")
            min_len = captions.shape[2]
            cap = captions.to("cpu", torch.int64)
            if min_len >= 2 and min_len - 1 <= self.decoder.max_seq_len and 0 <= start < V and 0 <= end < V:
                # whole START .. END sequences (a tokenised validation set): checked without a Python loop
                n = (cap != pad).long().cumsum(-1).argmax(-1, keepdim=True)  # index of the last non-PAD id
                if bool(((cap >= 0) & (cap < V)).all()) and bool((cap[..., :1] == start).all()) and \
                        bool((cap.gather(-1, n) == end).all()) and cap.shape[1] > 0 and \
                        bool(((cap != pad) | (torch.arange(min_len) > n)).all()):
                    return cap.contiguous()
            per = cap.tolist()
            for img in per:  # a padded row holds its candidate up to the last non-PAD id
                for c in img:
                    while c and c[-1] == pad:
                        c.pop()
        else:
            captions = list(captions)
            if any(len(c) > 0 and isinstance(c[0], (list, tuple)) for c in captions):
                if len(captions) != B:
                    raise ValueError(f"score_captions: {len(captions)} candidate lists for {B} images")
                per = [list(img) for img in captions]
            else:  # one flat list of candidates for every image
                per = [captions] * B
        C = len(per[0]) if per else 0
        if C == 0 or any(len(img) != C for img in per):
            raise ValueError("score_captions: every image needs the same number (one at least) of candidates")
        seqs = []
        for b, img in enumerate(per):
            for c, cand in enumerate(img):
                ids = [int(t) for t in cand]
                if not ids:
                    raise ValueError(f"score_captions: candidate {c} of image {b} is empty")
                if min(ids) < 0 or max(ids) >= V:
                    raise ValueError(f"score_captions: candidate {c} of image {b} holds an id outside [0, {V})")
                if ids[0] != start:
                    ids = [start] + ids
                if ids[-1] != end:
                    ids = ids + [end]
                seqs.append(ids)
        if not (0 <= start < V and 0 <= end < V):
            raise ValueError(f"score_captions: START / END ids outside [0, {V})")
        L = max(min_len, max(len(s) for s in seqs))
        if L - 1 > self.decoder.max_seq_len:
            raise ValueError(f"score_captions: a sequence of {L} ids gives {L - 1} decoder positions, more than "
                             f"max_seq_len = {self.decoder.max_seq_len}")
        return torch.tensor([s + [pad] * (L - len(s)) for s in seqs], dtype=torch.int64).view(B, C, L)

    @torch.no_grad()
    def score_captions(self, images, captions, start_token_id: int, end_token_id: int, *, return_tokens: bool = False,
                       head_rows: Optional[int] = None):
        """Teacher-forced log-likelihoods of GIVEN captions, C candidates per image (the opposite question to
        generate_*: how likely is this caption for this image). captions: a list per image of C candidate id
        lists (ragged lengths; the same C for every image), or one flat list of candidates scored against every
        image, or an int64 tensor [B, C, L] padded with pad_idx. A candidate without a leading START or a trailing
        END gets them (what inference.postprocess_ids strips); the sequences are padded to a common length L, the
        decoder reads seq[:-1] and is scored on seq[1:] (train.py's split), PAD targets are not scored.

        The image is encoded once and its cross-attention K/V computed once for its C candidates; the vocabulary
        head runs in chunks of head_rows rows, each reduced on the device to a log-probability and a rank per row
        (csrc/score.hip), so logits [B, C, L - 1, V] never exist (decoder.run_score).

        Returns device tensors (logprob f32 [B, C] = sum over the scored positions of log p(target), tokens int32
        [B, C] = the scored positions, hits int32 [B, C] = the positions whose target is the argmax); with
        return_tokens also (token_logprob f32 [B, C, L - 1], rank int32 [B, C, L - 1]: 0 = the target is the
        argmax, rank < k = in the top k, -1 = PAD target). Empty candidates, ids outside [0, V), unequal candidate
        counts and sequences with more than max_seq_len positions raise ValueError before anything is launched."""
        n = images.shape[0] if isinstance(images, torch.Tensor) else len(images)
        seq = self._caption_sequences(captions, n, start_token_id, end_token_id)
        pv = images if isinstance(images, torch.Tensor) else \
            self.image_processor(images=images, return_tensors="pt")["pixel_values"]
        pv = pv.to(self.device).float()
        seq = seq.to(self.device)
        return self.score_tokens(pv, seq[:, :, :-1], seq[:, :, 1:], return_tokens=return_tokens, head_rows=head_rows)

    @torch.no_grad()
    def score_tokens(self, images: torch.Tensor, decoder_input_tokens: torch.Tensor, target_tokens: torch.Tensor, *,
                     return_tokens: bool = False, head_rows: Optional[int] = None):
        """score_captions on sequences that are already split and padded: pixel values [B, 3, H, W], decoder inputs
        and targets int64 [B, C, T] (or [B, T]: one candidate per image, a train / validation batch as it is),
        PAD targets not scored. Returns what score_captions returns, [B, C] (or [B])."""
        tokens = decoder_input_tokens.to(self.device, torch.int64)
        targets = target_tokens.to(self.device, torch.int64)
        flat = tokens.dim() == 2
        if flat:
            tokens, targets = tokens.unsqueeze(1), targets.unsqueeze(1)
        if tokens.dim() != 3 or tokens.shape != targets.shape or tokens.shape[0] != images.shape[0]:
            raise ValueError(f"score_tokens: tokens {tuple(tokens.shape)} / targets {tuple(targets.shape)} do not match "
                             f"{images.shape[0]} images")
        B, C, T = tokens.shape
        if T < 1 or T > self.decoder.max_seq_len:
            raise ValueError(f"score_tokens: {T} decoder positions outside 1 .. max_seq_len = {self.decoder.max_seq_len}")
        if head_rows is not None and int(head_rows) < 1:
            raise ValueError(f"score_tokens: head_rows must be positive, got {head_rows}")
        tokens, targets = tokens.contiguous(), targets.contiguous()
        mem, mem_ld, S, _, _ = self._encode_memory(images.to(self.device))
        A = self.decoder.run_score(tokens, targets, mem, mem_ld, S, head_rows=head_rows)
        shape = (B,) if flat else (B, C)
        out = (A.seq_logprob.view(shape).clone(), A.seq_tokens.view(shape).clone(), A.seq_hits.view(shape).clone())
        if return_tokens:
            out += (A.token_logprob.view(*shape, T).clone(), A.rank.view(*shape, T).clone())
        return out

    # --- generate (model.py:171-255) -----------------------------------------------------------
    @torch.no_grad()
    def generate(self, image, start_token_id, end_token_id, max_len=100, method="greedy", beam_size=3) -> List[int]:
        if method == "beam":
            print("Beam search not fully implemented in this example. Falling back to greedy.")
            method = "greedy"
        if method != "greedy":
            raise ValueError(f"Unsupported generation method: {method}. Choose 'greedy' or 'beam'.")
        self.eval()
        if isinstance(image, torch.Tensor):
            pv = image if image.dim() == 4 else image.unsqueeze(0)
        else:
            pv = self.image_processor(images=image, return_tensors="pt")["pixel_values"]
        pv = pv.to(self.device).float()
        mem, mem_ld, S, _, _ = self._encode_memory(pv)
        mem3 = mem.view(1, S, -1) if mem_ld == self.decoder_embed_dim else None
        if mem3 is None:  # identity projection + cls: gather the strided row
            mem3 = mem[:1].reshape(1, 1, -1).contiguous()
        ids = [int(start_token_id)]
        for _ in range(max_len - 1):
            logits = self.decoder.forward(torch.tensor([ids], device=self.device), mem3)
            nxt = int(torch.argmax(logits[0, -1]).item())
            ids.append(nxt)
            if nxt == end_token_id:
                break
        return ids

    @torch.no_grad()
    def generate_batch(self, images, start_token_id: int, end_token_id: int, max_len: int = 100,
                       use_graph: bool = True, check_every: int = 8, streams: Optional[int] = None,
                       next_images: Optional[torch.Tensor] = None, repetition_penalty: float = 1.0,
                       no_repeat_ngram_size: int = 0, min_length: int = 0, suppress_tokens=(),
                       prompts=None, kv_dtype: Optional[str] = None) -> List[List[int]]:
        """Greedy captions for a whole batch (BASELINE config 5): per image the same token list as
        generate() (model.py:171-242: START, argmax of the last position each step, stop after END,
        at most max_len ids), computed with cached self-attention K/V, the cross-attention K/V of
        the image memory computed once, and ONE hipGraph-captured step replayed per token. The host
        checks the finished count every `check_every` tokens (the only synchronisation).

        streams: the images are decoded as this many independent row groups, each with its own state,
        issued on its own HIP stream (default: env MIT_DECODE_STREAMS, else 1). Rows never interact in
        greedy decoding and every kernel computes a row the same way at any batch size, so the ids
        do not depend on the grouping. Measured at B = 256 (configs[4]): 2 / 3 / 4 groups take 1.12 /
        1.23 / 1.53x the one-group time -- the groups' kernels do overlap, but every kernel boundary
        costs the same whatever its size, so one group of full-width launches is fastest.

        next_images: the next call's images (pixel values on the device); their frozen encoder forward is
        issued on the encoder stream one launch chunk per token step, beside this call's latency-bound
        token steps, and the next call takes it (as train_step's next_images; the ids are unchanged).

        Constraints (decoder.DecodeConstraints, csrc/constrain.hip; the defaults switch them off and leave the
        decode launch for launch what it was): repetition_penalty (> 0; the logit of every token a row already
        holds is divided by it when positive, multiplied otherwise), no_repeat_ngram_size (no n-gram occurs twice
        in a row's ids), min_length (no END before that many generated tokens), suppress_tokens (ids never picked)
        and prompts (one token list per image, or one for all images: forced after START and part of the returned
        ids).
        With active constraints the head's folded argmax gives way to f32 logits, the constraint launch and the
        pick; a prompt list per image is split with the rows when streams > 1.

        kv_dtype: how the cross-attention K/V is held (decoder.resolve_kv_dtype: the argument, else env
        MIT_DECODE_KV, else "bf16", the decode as it always was). "fp8" (bf16 models) keeps it as e4m3 bytes with
        power-of-two scales per (layer, image, head): half the bytes a token step streams and half the memory a
        batch's K/V occupies; the ids are those of the bf16 decode on the dequantised K/V."""
        self.eval()
        pv = images if isinstance(images, torch.Tensor) else \
            self.image_processor(images=images, return_tensors="pt")["pixel_values"]
        pv = pv.to(self.device).float()
        B = pv.shape[0]
        mem, mem_ld, S, _, _ = self._encode_memory(pv)
        dec = self.decoder
        if streams is None:
            streams = int(os.environ.get("MIT_DECODE_STREAMS", "1"))
        G = max(1, min(int(streams), B))
        bounds = [B * i // G for i in range(G + 1)]
        cons = DecodeConstraints(repetition_penalty, no_repeat_ngram_size, min_length, suppress_tokens, prompts)
        if cons.active():  # the whole batch's prompt lists, before they are cut into row groups
            cons.validate(dec.V, max_len, int(end_token_id), B)
        states = [dec.decode_begin(mem[bounds[i] * S:bounds[i + 1] * S], mem_ld, S, bounds[i + 1] - bounds[i], max_len,
                                   start_token_id, end_token_id,
                                   constraints=cons.rows(bounds[i], bounds[i + 1]) if cons.active() else None,
                                   kv_dtype=kv_dtype)
                  for i in range(G)]
        steps = max_len - 1
        if steps > 0:
            for stt in states:
                dec.decode_step(stt)  # position 0 (eager: warms every kernel before capture)
            done = 1
            cur = torch.cuda.current_stream()
            side = [cur] + [torch.cuda.Stream(device=self.device) for _ in range(G - 1)]
            for s_ in side[1:]:
                s_.wait_stream(cur)

            def one_step():
                for stt, s_ in zip(states, side):
                    with torch.cuda.stream(s_):
                        dec.decode_step(stt)
            launch = os.environ.get("MIT_DECODE_LAUNCH", "plan") if use_graph else "eager"
            if launch == "graph" and steps > 1:
                # one hipGraph per group (ROCm launches a graph's nodes one by one from the host:
                # ~8.7 us each, so the groups' graphs hardly overlap)
                runs = []
                for stt in states:
                    graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph):
                        dec.decode_step(stt)
                    runs.append(graph.replay)

                def run():
                    for r, s_ in zip(runs, side):
                        with torch.cuda.stream(s_):
                            r()
            elif launch == "plan" and steps > 1:
                # the step's launches recorded once (a real step) and re-issued from C++ (mit_plan_run,
                # ~3.6 us per launch), every group on its own stream
                prog = native.record(one_step)
                done += 1
                run = prog.run
            else:
                run = one_step
            pf = self.prefetch_encoder_iter(next_images) if next_images is not None else None
            while done < steps:
                n = min(check_every, steps - done)
                for _ in range(n):
                    run()
                    # one encoder chunk per token step (one per 3 or 6 steps measured the same)
                    if pf is not None and next(pf, pf) is pf:
                        pf = None
                done += n
                if sum(int(stt.n_finished.item()) for stt in states) == B:
                    break
            for _ in pf or ():
                pass
            for s_ in side[1:]:
                cur.wait_stream(s_)
        out = []
        for stt in states:
            out.extend(stt.token_lists())
        return out

    # --- rolling-batch greedy captioning (decoder.RollingState, rolling.RollingScheduler) -----------------
    def generate_rolling_iter(self, batches, start_token_id: int, end_token_id: int, max_len: int = 100,
                              slots: int = 256, check_every: Optional[int] = None, max_lens=None,
                              kv_dtype: Optional[str] = None, use_graph: bool = True,
                              encode_batch: Optional[int] = None, pool: Optional[int] = None,
                              streams: Optional[int] = None, repetition_penalty: float = 1.0,
                              no_repeat_ngram_size: int = 0, min_length: int = 0, suppress_tokens=(), prompts=None):
        """Greedy captions of a stream of images with in-flight ("rolling") batching: `slots` decode rows are kept,
        every row at its own position; when a row's caption ends (END, or its cap) its slot is handed to the next
        image while the other rows go on, so a dataset costs about mean(length) token steps per `slots` images where
        generate_batch pays max(length). Yields (image index, ids) in COMPLETION order; the ids are exactly what
        generate_batch returns for that image (rows never interact in greedy decoding and every kernel computes a
        row the same way whatever its neighbours and positions are).

        batches: an iterable of pixel tensors [n_i, 3, H, W] (or one tensor); images are numbered in arrival order
        and encoded `encode_batch` at a time (default `slots`) into a K/V pool of `pool` images (default: one
        chunk; a multiple of encode_batch). max_lens: an optional per-image cap, 1 <= cap <= max_len, indexed by
        image number (a cap of 1 yields [START] and takes no slot). check_every: token steps between two polls of
        the device's done flags (default rolling.CHECK_EVERY_DEFAULT). kv_dtype: as generate_batch. use_graph /
        env MIT_DECODE_LAUNCH: the step is recorded once and replayed as a launch plan ("plan"; "graph" means the
        same here: the recorded plan is what replays between admissions), or issued eagerly ("eager",
        use_graph=False).

        Raises ValueError, before any launch, for decode constraints or prompts (the constraint kernel reads one
        shared position), streams > 1, slots < 1, caps outside [1, max_len] and max_len past the positional
        table."""
        dec = self.decoder
        if DecodeConstraints(repetition_penalty, no_repeat_ngram_size, min_length, suppress_tokens, prompts).active():
            raise ValueError("rolling decode does not take decode constraints or prompts (use generate_batch)")
        if streams is not None and int(streams) > 1:
            raise ValueError("rolling decode runs one row group (streams > 1 is generate_batch's)")
        if int(slots) < 1:
            raise ValueError(f"rolling decode needs slots >= 1 (got {slots})")
        if max_len < 1 or max_len > dec.pe.shape[0]:
            raise ValueError(f"max_len {max_len} must be in 1..{dec.pe.shape[0]} (the positional table, "
                             f"decoder_max_seq_len)")
        if max_lens is not None:
            max_lens = [int(c) for c in max_lens]
            bad = [(i, c) for i, c in enumerate(max_lens) if not 1 <= c <= max_len]
            if bad:
                raise ValueError(f"max_lens must lie in 1..{max_len}: image {bad[0][0]} has {bad[0][1]}")
        resolve_kv_dtype(kv_dtype, self.dtype)
        sch = rolling.RollingScheduler(int(slots), check_every, encode_batch, pool)
        self.last_rolling_schedule = sch  # its counters (steps, polls, admits, chunks) once the iterator is spent
        return self._rolling_run(sch, batches, int(start_token_id), int(end_token_id), int(max_len), max_lens, kv_dtype,
                                 use_graph)

    def generate_rolling(self, batches, start_token_id: int, end_token_id: int, max_len: int = 100, **kwargs):
        """generate_rolling_iter collected: the token lists in input order (what generate_batch returns for the
        concatenated images)."""
        got = dict(self.generate_rolling_iter(batches, start_token_id, end_token_id, max_len, **kwargs))
        return [got[i] for i in range(len(got))]

    @staticmethod
    def _rolling_chunks(batches, n: int):
        """The images of an iterable of pixel tensors (or one tensor) regrouped into tensors of exactly n images (the
        last one smaller)."""
        if isinstance(batches, torch.Tensor):
            batches = [batches]
        held, have = [], 0
        for b in batches:
            if b.dim() == 3:
                b = b.unsqueeze(0)
            while b.shape[0]:
                take = min(n - have, b.shape[0])
                held.append(b[:take])
                have += take
                b = b[take:]
                if have == n:
                    yield held[0] if len(held) == 1 else torch.cat([h.to(held[0].device) for h in held])
                    held, have = [], 0
        if have:
            yield held[0] if len(held) == 1 else torch.cat([h.to(held[0].device) for h in held])

    @torch.no_grad()
    def _rolling_run(self, sch, batches, start_id, end_id, max_len, max_lens, kv_dtype, use_graph):
        self.eval()
        dec = self.decoder
        source = self._rolling_chunks(batches, sch.encode_batch)
        stt, run = None, None
        launch = os.environ.get("MIT_DECODE_LAUNCH", "plan") if use_graph else "eager"
        while True:
            while True:  # chunks and admissions until no free slot is left that the source could fill
                while sch.wants_chunk():
                    pv = next(source, None)
                    if pv is None:
                        sch.close()
                        break
                    n, i0 = pv.shape[0], sch.next_image
                    if max_lens is not None and i0 + n > len(max_lens):
                        raise ValueError(f"max_lens holds {len(max_lens)} caps, the source at least {i0 + n} images")
                    caps = max_lens[i0:i0 + n] if max_lens is not None else [max_len] * n
                    at, trivial = sch.add_chunk(caps)
                    if len(trivial) < n:  # some image of the chunk needs a slot: encode it, K/V into the pool
                        mem, mem_ld, S, _, _ = self._encode_memory(pv.to(self.device).float())
                        if stt is None:
                            stt = dec.rolling_begin(S, sch.slots, max(max_len, 2), start_id, end_id, pool=sch.pool,
                                                    kv_dtype=kv_dtype)
                            dec.rolling_step(stt)  # every slot is empty: warms every kernel, moves nothing
                            if launch in ("plan", "graph"):
                                run = native.record(lambda: dec.rolling_step(stt)).run
                            else:
                                run = lambda: dec.rolling_step(stt)  # noqa: E731
                        dec.rolling_fill(stt, mem, mem_ld, S, n, at)
                    for i in trivial:
                        yield i, [start_id]
                triples = sch.admissions()
                if triples:  # launched before the next chunk may overwrite the pool region it reads
                    dec.rolling_admit(stt, triples)
                if not (triples and sch.wants_chunk()):
                    break
            if sch.finished():
                return
            for _ in range(sch.next_steps()):
                run()
            harvest = sch.poll(*stt.snapshot())
            if harvest:
                rows = stt.harvest([h[0] for h in harvest])  # the newly done rows only, before their slots are reused
                for r, (_, image, n_ids) in enumerate(harvest):
                    yield image, rows[r, :n_ids].tolist()

    # --- rolling-batch captioning, sampled and constrained (decoder.rolling_stream_begin / rolling_stream_step) ------
    def generate_stream_iter(self, batches, start_token_id: int, end_token_id: int, max_len: int = 100, *,
                             slots: int = 256, temperature: Optional[float] = None, top_k: int = 0, top_p: float = 1.0,
                             num_samples: int = 1, seed: int = 0, image_offset: int = 0,
                             repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0, min_length: int = 0,
                             suppress_tokens=(), prompts=None, max_lens=None, check_every: Optional[int] = None,
                             kv_dtype: Optional[str] = None, use_graph: bool = True,
                             encode_batch: Optional[int] = None, pool: Optional[int] = None,
                             streams: Optional[int] = None, beam_size: Optional[int] = None,
                             method: Optional[str] = None):
        """Captions of a stream of images with rolling batching (generate_rolling_iter's schedule: `slots` decode
        rows, each at its own position, a finished row's slot handed to the next work item) for greedy, SAMPLED and
        CONSTRAINED decoding. Yields (image, sample, ids, logprob) in COMPLETION order.

        temperature None: greedy (num_samples must be 1, logprob is None); the ids are generate_batch's for that
        image under the same constraints. temperature > 0: num_samples rows per image, drawn as
        generate_sample_batch draws them -- sample n of image i at position p uses the counter hash of (seed,
        (image_offset + i) * num_samples + n, p), whatever slot it sits in and whenever it was admitted -- so ids and
        logprob are generate_sample_batch's for the same seed, num_samples and global image index, bit for bit
        (while both run the same GEMM family). An image's samples share one pool entry of
        cross-attention K/V and each takes its own slot (one admit copy per sample).

        repetition_penalty, no_repeat_ngram_size, min_length, suppress_tokens, prompts: generate_batch's constraints
        (csrc/constrain.hip mit_logits_constrain_ragged: every row at its own position). prompts: one token list for
        all images, or one list per image indexed by image number (arrival order from 0, as max_lens); a slot reads
        its image's row of one prompt table. max_lens, check_every, kv_dtype, use_graph, encode_batch, pool: as
        generate_rolling_iter.

        Raises ValueError before any launch, from this call and not from the first next(): beams (beam_size or
        method "beam": the beams of an image interact), streams > 1, bad sampling parameters, greedy with
        num_samples != 1, bad constraint settings, caps outside [1, max_len], kv_dtype "fp8" on a float32 model.
        Per-image prompts and the number of caps are checked chunk by chunk, before that chunk's launches."""
        dec = self.decoder
        if (beam_size is not None and int(beam_size) > 1) or method == "beam":
            raise ValueError("stream decode does not run beam search: the beams of an image interact through the "
                             "selection and the ancestor table (use generate_beam_batch)")
        if method not in (None, "greedy", "sample"):
            raise ValueError(f"method {method!r}: stream decode is greedy (temperature None) or sampled")
        if streams is not None and int(streams) > 1:
            raise ValueError("stream decode runs one row group (streams > 1 is generate_batch's)")
        if int(slots) < 1:
            raise ValueError(f"stream decode needs slots >= 1 (got {slots})")
        N = int(num_samples)
        if N < 1:
            raise ValueError(f"num_samples {N} must be at least 1")
        if temperature is None:
            if N != 1:
                raise ValueError(f"greedy stream decode (temperature None) yields one caption per image, not {N}")
        elif not temperature > 0 or not top_p > 0 or top_k < 0:
            raise ValueError(f"sampling needs temperature > 0, top_p > 0 and top_k >= 0 (got {temperature}, {top_p}, "
                             f"{top_k})")
        if int(image_offset) < 0:
            raise ValueError(f"image_offset {image_offset} < 0")
        if max_len < 1 or max_len > dec.pe.shape[0]:
            raise ValueError(f"max_len {max_len} must be in 1..{dec.pe.shape[0]} (the positional table, "
                             f"decoder_max_seq_len)")
        if max_lens is not None:
            max_lens = [int(c) for c in max_lens]
            bad = [(i, c) for i, c in enumerate(max_lens) if not 1 <= c <= max_len]
            if bad:
                raise ValueError(f"max_lens must lie in 1..{max_len}: image {bad[0][0]} has {bad[0][1]}")
        cons = DecodeConstraints(repetition_penalty, no_repeat_ngram_size, min_length, suppress_tokens, prompts)
        # the settings every row shares (and a prompt for all images) now; a prompt list per image chunk by chunk
        DecodeConstraints(repetition_penalty, no_repeat_ngram_size, min_length, suppress_tokens,
                          None if cons.per_image() else cons.prompts).validate(dec.V, int(max_len), int(end_token_id), 1)
        resolve_kv_dtype(kv_dtype, self.dtype)
        sch = rolling.RollingScheduler(int(slots), check_every, encode_batch, pool, samples=N)
        self.last_rolling_schedule = sch
        return self._stream_run(sch, batches, int(start_token_id), int(end_token_id), int(max_len), max_lens, kv_dtype,
                                use_graph, cons, temperature, int(top_k), float(top_p), int(seed), int(image_offset))

    def generate_stream(self, batches, start_token_id: int, end_token_id: int, max_len: int = 100, *,
                        return_logprob: bool = False, **kwargs):
        """generate_stream_iter collected, in input order. Sampling (temperature given): generate_sample_batch's
        shapes for the concatenated images -- per image its ids when num_samples == 1 and return_logprob is False,
        else its num_samples (ids, logprob) pairs. Greedy: generate_batch's list of ids."""
        N = int(kwargs.get("num_samples", 1))
        sampled = kwargs.get("temperature") is not None
        got = {(i, n): (ids, lp) for i, n, ids, lp in
               self.generate_stream_iter(batches, start_token_id, end_token_id, max_len, **kwargs)}
        B = len(got) // N
        if not sampled or (N == 1 and not return_logprob):
            return [got[(i, 0)][0] for i in range(B)]
        return [[got[(i, n)] for n in range(N)] for i in range(B)]

    @torch.no_grad()
    def _stream_run(self, sch, batches, start_id, end_id, max_len, max_lens, kv_dtype, use_graph, cons, temperature,
                    top_k, top_p, seed, image_offset):
        self.eval()
        dec = self.decoder
        N = sch.samples
        source = self._rolling_chunks(batches, sch.encode_batch)
        stt, run = None, None
        launch = os.environ.get("MIT_DECODE_LAUNCH", "plan") if use_graph else "eager"
        per_image = cons.per_image() and cons.has_prompts()
        shared = cons.has_prompts() and not per_image
        table = None
        if cons.has_prompts():  # one table for the whole run: row i = image i's prompt (or row 0 = everybody's)
            rows = cons.prompts if per_image else [cons.prompts]
            table = torch.full((len(rows), max(len(p) for p in rows) + 1), -1, dtype=torch.int64)
            for b, p in enumerate(rows):
                table[b, 1:1 + len(p)] = torch.tensor(p, dtype=torch.int64)
        none_lp = None if temperature is None else 0.0
        while True:
            while True:  # chunks and admissions until no free slot is left that the source could fill
                while sch.wants_chunk():
                    pv = next(source, None)
                    if pv is None:
                        sch.close()
                        break
                    n, i0 = pv.shape[0], sch.next_image
                    if max_lens is not None and i0 + n > len(max_lens):
                        raise ValueError(f"max_lens holds {len(max_lens)} caps, the source at least {i0 + n} images")
                    if per_image:
                        if i0 + n > len(cons.prompts):
                            raise ValueError(f"prompts holds {len(cons.prompts)} lists, the source at least {i0 + n} "
                                             f"images")
                        DecodeConstraints(prompts=cons.prompts[i0:i0 + n]).validate(dec.V, max_len, end_id, n)
                    caps = max_lens[i0:i0 + n] if max_lens is not None else [max_len] * n
                    at, trivial = sch.add_chunk(caps)
                    if len(trivial) < n:  # some image of the chunk needs a slot: encode it, K/V into the pool
                        mem, mem_ld, S, _, _ = self._encode_memory(pv.to(self.device).float())
                        if stt is None:
                            stt = dec.rolling_stream_begin(S, sch.slots, max(max_len, 2), start_id, end_id,
                                                           pool=sch.pool, kv_dtype=kv_dtype, temperature=temperature,
                                                           top_k=top_k, top_p=top_p, seed=seed, constraints=cons,
                                                           prompt_table=table)
                            dec.rolling_stream_step(stt)  # every slot is empty: warms every kernel, moves nothing
                            if launch in ("plan", "graph"):
                                run = native.record(lambda: dec.rolling_stream_step(stt)).run
                            else:
                                run = lambda: dec.rolling_stream_step(stt)  # noqa: E731
                        dec.rolling_fill(stt, mem, mem_ld, S, n, at)
                    for i in trivial:
                        for k in range(N):
                            yield i, k, [start_id], none_lp
                records = [(s, entry, cap, image_offset * N + row, (row // N) if per_image else (0 if shared else -1))
                           for s, entry, cap, row in sch.admissions_ex()]
                if records:  # launched before the next chunk may overwrite the pool region it reads
                    dec.rolling_admit_ex(stt, records)
                if not (records and sch.wants_chunk()):
                    break
            if sch.finished():
                return
            for _ in range(sch.next_steps()):
                run()
            harvest = sch.poll(*stt.snapshot())
            if harvest:
                rows, lps = stt.harvest_ex([h[0] for h in harvest])  # before the slots are reused
                for r, (_, row, n_ids) in enumerate(harvest):
                    yield row // N, row % N, rows[r, :n_ids].tolist(), (None if temperature is None else lps[r])

    @torch.no_grad()
    def generate_beam_batch(self, images, start_token_id: int, end_token_id: int, max_len: int = 100,
                            beam_size: int = config.BEAM_SIZE, length_penalty: float = 0.0, return_all: bool = False,
                            use_graph: bool = True, check_every: int = 8, repetition_penalty: float = 1.0,
                            no_repeat_ngram_size: int = 0, min_length: int = 0, suppress_tokens=(), prompts=None,
                            kv_dtype: Optional[str] = None):
        """Beam-search captions for a whole batch: beam_size slots per image on the KV-cache step of
        generate_batch (decoder.beam_begin / beam_step). Per step a live beam offers its V continuations at
        score + log_softmax(logits), a finished beam itself once (padded); the beam_size best by (score, lower
        parent, lower token) go on; decoding stops when every beam of every image is finished, or at max_len.
        The selection, the KV-cache ancestry and every index stay on the device, so a step is recorded / captured
        and replayed as in generate_batch (same launch choices: use_graph, env MIT_DECODE_LAUNCH); the host reads
        the finished count every `check_every` tokens.

        Beams are ranked on the host by score / length**length_penalty (length: generated tokens, END included;
        0.0 ranks by the raw log-probability), ties to the lower slot. Returns per image the best beam's ids
        (START .. first END inclusive, else max_len ids), or with return_all its beam_size (ids, score) pairs,
        best first.

        repetition_penalty, no_repeat_ngram_size, min_length, suppress_tokens, prompts: the constraints of
        generate_batch (the defaults switch them off and leave the decode launch for launch what it was).
        A beam's constraints follow its own ids (its ancestry), scores are log_softmax of the constrained logits,
        and a prompt adds nothing to a score. kv_dtype: as generate_batch (the beams of an image read its one
        K/V, bf16 or fp8)."""
        self.eval()
        pv = images if isinstance(images, torch.Tensor) else \
            self.image_processor(images=images, return_tensors="pt")["pixel_values"]
        pv = pv.to(self.device).float()
        B, K = pv.shape[0], int(beam_size)
        mem, mem_ld, S, _, _ = self._encode_memory(pv)
        dec = self.decoder
        cons = DecodeConstraints(repetition_penalty, no_repeat_ngram_size, min_length, suppress_tokens, prompts)
        stt = dec.beam_begin(mem, mem_ld, S, B, K, max_len, start_token_id, end_token_id,
                             constraints=cons if cons.active() else None, kv_dtype=kv_dtype)
        steps = max_len - 1
        dec.beam_step(stt)  # position 0 (eager: warms every kernel before capture)
        done = 1
        launch = os.environ.get("MIT_DECODE_LAUNCH", "plan") if use_graph else "eager"
        if launch == "graph" and steps > 1:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                dec.beam_step(stt)
            run = graph.replay
        elif launch == "plan" and steps > 1:
            prog = native.record(lambda: dec.beam_step(stt))
            done += 1
            run = prog.run
        else:
            run = lambda: dec.beam_step(stt)  # noqa: E731
        while done < steps:
            n = min(check_every, steps - done)
            for _ in range(n):
                run()
            done += n
            if int(stt.n_finished.item()) == B * K:
                break
        return rank_beams(stt.token_lists(), stt.score.cpu().tolist(), stt.length.cpu().tolist(), K, length_penalty,
                          return_all)

    @torch.no_grad()
    def generate_beam(self, image, start_token_id: int, end_token_id: int, max_len: int = 100,
                      beam_size: int = config.BEAM_SIZE, length_penalty: float = 0.0, return_all: bool = False,
                      **constraints):
        """generate_beam_batch for one image (a PIL image / HWC array or a [3,H,W] / [1,3,H,W] pixel tensor);
        further keyword arguments: generate_beam_batch's constraints."""
        if isinstance(image, torch.Tensor):
            pv = image if image.dim() == 4 else image.unsqueeze(0)
        else:
            pv = self.image_processor(images=image, return_tensors="pt")["pixel_values"]
        return self.generate_beam_batch(pv, start_token_id, end_token_id, max_len=max_len, beam_size=beam_size,
                                        length_penalty=length_penalty, return_all=return_all, **constraints)[0]

    @torch.no_grad()
    def generate_sample_batch(self, images, start_token_id: int, end_token_id: int, max_len: int = 100,
                              temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, num_samples: int = 1,
                              seed: int = 0, image_offset: int = 0, return_logprob: bool = False,
                              use_graph: bool = True, check_every: int = 8, repetition_penalty: float = 1.0,
                              no_repeat_ngram_size: int = 0, min_length: int = 0, suppress_tokens=(), prompts=None,
                              kv_dtype: Optional[str] = None):
        """Sampled captions for a whole batch: num_samples rows per image on the KV-cache step of generate_batch
        (decoder.sample_begin / sample_step). Per step a live row draws its next token from softmax(logits /
        temperature) restricted to the top_k most likely tokens and, inside them, to the shortest prefix of mass
        top_p (0 / 1.0: filter off); a row stops after END, decoding when every row has, or at max_len. The draw
        of sample n of image b at position p is a counter hash of (seed, (image_offset + b) * num_samples + n, p):
        a caption depends on the seed and the image's global index, not on how the images were batched. The pick
        and every index stay on the device, so a step is recorded / captured and replayed as in generate_batch
        (same launch choices: use_graph, env MIT_DECODE_LAUNCH); the host reads the finished count every
        `check_every` tokens.

        Returns per image its ids (START .. first END inclusive, else max_len ids) when num_samples == 1 and
        return_logprob is False; else per image its num_samples (ids, logprob) pairs, logprob being the sum of
        log_softmax(logits)[token] (temperature 1, unfiltered) over the generated tokens, END included.

        repetition_penalty, no_repeat_ngram_size, min_length, suppress_tokens, prompts: the constraints of
        generate_batch (the defaults switch them off and leave the decode launch for launch what it was).
        The draw and the logprob are taken from the constrained logits; a prompt adds nothing to a logprob.
        kv_dtype: as generate_batch (the samples of an image read its one K/V, bf16 or fp8)."""
        self.eval()
        pv = images if isinstance(images, torch.Tensor) else \
            self.image_processor(images=images, return_tensors="pt")["pixel_values"]
        pv = pv.to(self.device).float()
        B, N = pv.shape[0], int(num_samples)
        mem, mem_ld, S, _, _ = self._encode_memory(pv)
        dec = self.decoder
        cons = DecodeConstraints(repetition_penalty, no_repeat_ngram_size, min_length, suppress_tokens, prompts)
        stt = dec.sample_begin(mem, mem_ld, S, B, N, max_len, start_token_id, end_token_id, temperature=temperature,
                               top_k=top_k, top_p=top_p, seed=seed, row0=int(image_offset) * N,
                               constraints=cons if cons.active() else None, kv_dtype=kv_dtype)
        steps = max_len - 1
        dec.sample_step(stt)  # position 0 (eager: warms every kernel before capture)
        done = 1
        launch = os.environ.get("MIT_DECODE_LAUNCH", "plan") if use_graph else "eager"
        if launch == "graph" and steps > 1:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                dec.sample_step(stt)
            run = graph.replay
        elif launch == "plan" and steps > 1:
            prog = native.record(lambda: dec.sample_step(stt))
            done += 1
            run = prog.run
        else:
            run = lambda: dec.sample_step(stt)  # noqa: E731
        while done < steps:
            n = min(check_every, steps - done)
            for _ in range(n):
                run()
            done += n
            if int(stt.n_finished.item()) == B * N:
                break
        ids = stt.token_lists()
        if N == 1 and not return_logprob:
            return ids
        lp = stt.logprob.cpu().tolist()
        return [[(ids[b * N + n], lp[b * N + n]) for n in range(N)] for b in range(B)]

    @torch.no_grad()
    def generate_sample(self, image, start_token_id: int, end_token_id: int, max_len: int = 100, **kwargs):
        """generate_sample_batch for one image (a PIL image / HWC array or a [3,H,W] / [1,3,H,W] pixel tensor);
        keyword arguments as generate_sample_batch."""
        if isinstance(image, torch.Tensor):
            pv = image if image.dim() == 4 else image.unsqueeze(0)
        else:
            pv = self.image_processor(images=image, return_tensors="pt")["pixel_values"]
        return self.generate_sample_batch(pv, start_token_id, end_token_id, max_len=max_len, **kwargs)[0]

    def sync_shadow(self):
        """Re-cast the bf16 weight shadow the kernels read from the f32 master. Needed only after
        editing weights out of band (through ``p.data``, which torch's version counter does not see)
        and before a fused ``train_step``; every other path refreshes the shadow itself
        (params.FlatParams.ensure_shadow)."""
        self.store.sync_shadow()

    # --- checkpoints (reference key names) --------------------------------------
    def state_dict(self) -> Dict[str, torch.Tensor]:
        sd = {}
        for k, v in self.encoder.hf_state_dict().items():
            sd["encoder." + k] = v
        if self.has_projection:
            sd["projection.weight"] = self.store.p("projection.weight").detach().clone()
            sd["projection.bias"] = self.store.p("projection.bias").detach().clone()
        sd.update(flat_to_reference(self.store, self.decoder.L, self.decoder_embed_dim))
        sd["decoder.positional_encoding.pe"] = self.decoder.pe.unsqueeze(0).clone()
        return sd

    def check_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True):
        """Raise (KeyError / ValueError) unless sd loads into this model: every trainable tensor
        present (strict) with the reference shape, encoder keys (if any) loadable. Touches nothing."""
        from optim import reference_trainable
        ref_shapes = dict(reference_trainable(self.store.layout))
        missing = [k for k in ref_shapes if k not in sd]
        if strict and missing:
            raise KeyError(f"missing keys: {missing[:6]}{'...' if len(missing) > 6 else ''}")
        bad = [(k, tuple(sd[k].shape), s) for k, s in ref_shapes.items() if k in sd and tuple(sd[k].shape) != s]
        if bad:
            raise ValueError("shape mismatch (checkpoint vs model): " +
                             ", ".join(f"{k} {a} vs {b}" for k, a, b in bad[:4]))
        enc = {k[len("encoder."):]: v for k, v in sd.items() if k.startswith("encoder.")}
        if enc:
            self.encoder.check_hf_state_dict(enc)

    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True):
        self.check_state_dict(sd, strict)
        enc = {k[len("encoder."):]: v for k, v in sd.items() if k.startswith("encoder.")}
        if enc:
            self.encoder.load_hf_state_dict(enc)
        flat = reference_to_flat(sd, self.decoder.L, self.decoder_embed_dim)
        names = set(self.store.names())
        with torch.no_grad():
            for k, v in flat.items():
                if k in names:
                    dst = self.store.p(k)
                    v = v.to(self.device, torch.float32)
                    if k.startswith("fc_out.") and v.shape[0] != dst.shape[0]:  # padded vocabulary head
                        if v.shape[0] != self.decoder.V:
                            raise ValueError(f"{k}: {tuple(v.shape)} does not match vocab {self.decoder.V}")
                        dst.zero_()
                        dst[:v.shape[0]].copy_(v)
                    else:
                        dst.copy_(v.reshape(dst.shape))
        self.store.sync_shadow()
        return self

    # --- accounting ----------------------------------------------------------------------------
    def flops_per_pair(self, T: int) -> float:
        """Algorithmic train FLOPs per image-caption pair: encoder fwd + 3 x decoder fwd
        (+ the projection, counted with the decoder as 3 x its forward)."""
        S = 1 if self.memory_mode == "cls" else self.encoder.N
        dec = self.decoder.flops_per_sequence(T, S)
        proj = 2 * S * self.encoder.E * self.decoder_embed_dim if self.has_projection else 0
        return self.encoder.flops_per_image() + 3 * (dec + proj)
