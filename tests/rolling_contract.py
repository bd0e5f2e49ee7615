"""The contract of rolling-batch captioning (csrc/decode.hip mit_*_ragged, csrc/rolling.hip mit_slot_admit,
decoder.RollingState, rolling.RollingScheduler, ImageToTextModel.generate_rolling_iter), in the manner of
tests/decode_contract.py: end-to-end inputs and their oracle, an independent simulation of the schedule, a scripted
driver that checks the scheduler's invariants, and the builders / references of the kernel cases.

End to end. Fixture tiny_vit_patches (procedural weights, V 512, d 192, 2 layers); images = cat([img, img.flip(-1),
img * 0.5, img.flip(-2), -img]) with img = FX.inputs(meta, 0)[0]: 20 images; START 2, END 69, max_len 24. With
oracle.ref_cpu (fp32, full-prefix recompute, END never produced, 23 steps) the first index of token 69 per image is
END_FIRST: nine distinct lengths, two images never end, and the smallest top-1 / top-2 logit margin over the 460
steps is 0.0033 > 2 TAU = 2e-3 (beam_contract.TAU, the project's fp32 logit bound), so the fp32 ids are pinned by
the oracle (tests/test_rolling_contract_cpu.py asserts both).

Schedule. `simulate` is a brute-force model of rolling batching written without the scheduler: time in token steps,
a poll every check_every steps, finished slots refilled at a poll from the images in order. `drive` runs a
RollingScheduler against scripted per-image lengths, playing the device (row_pos advances one per step until
length - 1, then done), and asserts: every image admitted exactly once, only into a slot seen empty or done, harvest
before reuse, complete output, pool entries never overwritten while waiting.
"""
import math

import torch

TAU2 = 2e-3                      # 2 x beam_contract.TAU
E2E_FIXTURE = "tiny_vit_patches"
START, END, NEVER, MAX_LEN = 2, 69, 10 ** 6, 24
END_FIRST = [5, 3, 3, 12, 13, 18, -1, 3, 4, 3, 3, 4, 10, 3, 13, 3, 5, 10, 11, -1]   # -1: END is never produced
SLOTS = (1, 3, 4, 20, 32)
ULP = 2.0 ** -23
L2E = 1.4426950408889634


def e2e_images(FX, fixture=E2E_FIXTURE):
    meta, _ = FX.load(fixture)
    img = FX.inputs(meta, 0)[0]
    return torch.cat([img, img.flip(-1), img * 0.5, img.flip(-2), -img]).contiguous()


_ORACLE = {}


def oracle(FX):
    """(ids [20][MAX_LEN] greedy with END never produced, smallest top-1 / top-2 margin over all steps), once."""
    from oracle import ref_cpu
    if "ids" not in _ORACLE:
        meta, _ = FX.load(E2E_FIXTURE)
        st = FX.state(meta)
        enc, dec = FX.enc_desc(meta), FX.dec_desc(meta)
        with torch.no_grad():
            mem = ref_cpu.memory_from_features(st, ref_cpu.encode(st, e2e_images(FX), enc), meta["mode"])
            toks = torch.full((mem.shape[0], 1), START, dtype=torch.int64)
            margin = math.inf
            for _ in range(MAX_LEN - 1):
                lg = ref_cpu.decoder_forward(st, toks, mem, heads=dec["heads"], layers=dec["layers"],
                                             max_len=dec["max_seq_len"])[:, -1].double()
                top = lg.topk(2, -1).values
                margin = min(margin, float((top[:, 0] - top[:, 1]).min()))
                toks = torch.cat([toks, lg.argmax(-1, keepdim=True)], 1)
        _ORACLE["ids"], _ORACLE["margin"] = toks.tolist(), margin
    return _ORACLE["ids"], _ORACLE["margin"]


def cut(ids, end, cap=None):
    """generate_batch's list of a full greedy row: START .. the first END inclusive, else every id; at most cap"""
    row = list(ids if cap is None else ids[:cap])
    if end in row[1:]:
        row = row[:row.index(end, 1) + 1]
    return row


def e2e_lengths():
    """ids per image for END = 69 and max_len 24"""
    return [MAX_LEN if e < 0 else e + 1 for e in END_FIRST]


# ------------------------------------------------------------------------------------------------
# the schedule
# ------------------------------------------------------------------------------------------------
def simulate(lengths, slots, check_every):
    """Brute force. lengths[i] >= 1 ids of image i (length - 1 token steps in a slot; 1: no slot). Returns (token
    steps run, completion order): every poll runs after exactly check_every steps while any slot is busy."""
    waiting = [i for i, n in enumerate(lengths) if n > 1]
    order = [i for i, n in enumerate(lengths) if n == 1]
    busy = {}                                    # slot -> [image, steps left]
    steps = 0
    while waiting or busy:
        for s in range(slots):
            if s not in busy and waiting:
                i = waiting.pop(0)
                busy[s] = [i, lengths[i] - 1]
        for _ in range(check_every):
            steps += 1
            for s in busy:
                busy[s][1] = max(0, busy[s][1] - 1)
        for s in sorted(busy):
            if busy[s][1] == 0:
                order.append(busy.pop(s)[0])
    return steps, order


def static_steps(lengths, slots, check_every, max_len):
    """Static batching on the same polling grid: consecutive chunks of `slots` images, each stepped until a poll
    (every check_every steps) sees its longest caption ended, at most max_len - 1 steps."""
    total = 0
    for i in range(0, len(lengths), slots):
        need = max(lengths[i:i + slots]) - 1
        total += min(-(-need // check_every) * check_every, max_len - 1)
    return total


def drive(sch, lengths, caps=None, batches=None, max_len=None):
    """Run the scheduler's protocol (rolling.py) against scripted lengths. caps: per-image cap handed to add_chunk
    (default: max_len, else the image's length); batches: how many images the source hands per chunk request (default:
    encode_batch). Returns dict(order, steps, polls, admits, chunks, admit_log)."""
    N = len(lengths)
    if caps is None:
        caps = [max_len if max_len is not None else n for n in lengths]
    assert all(1 <= min(n, c) for n, c in zip(lengths, caps))
    true_len = [min(n, c) for n, c in zip(lengths, caps)]
    dev_pos, dev_done = [0] * sch.slots, [1] * sch.slots          # the device: every slot starts empty = done
    dev_img = [None] * sch.slots
    pool = [None] * sch.pool                                      # image whose K/V an entry holds
    waiting_entry = {}                                            # image -> entry, from fill until admission
    seen_free = set(range(sch.slots))                             # slots the host has seen empty or done
    harvested, admitted, order, admit_log = set(), [], [], []
    src = 0
    guard = 0
    while True:
        guard += 1
        assert guard < 100000, "the schedule does not terminate"
        while True:
            while sch.wants_chunk():
                if src >= N:
                    sch.close()
                    break
                n = min(sch.encode_batch, N - src)
                at, trivial = sch.add_chunk(caps[src:src + n])
                assert at % sch.encode_batch == 0 and at + n <= sch.pool
                for j in range(n):
                    assert pool[at + j] not in waiting_entry, f"entry {at + j} overwritten before its image got a slot"
                    pool[at + j] = src + j
                    if caps[src + j] > 1:
                        waiting_entry[src + j] = at + j
                assert trivial == [src + j for j in range(n) if caps[src + j] == 1]
                order.extend(trivial)
                src += n
            triples = sch.admissions()
            assert len({t[0] for t in triples}) == len(triples)
            for s, entry, cap in triples:
                image = pool[entry]
                assert waiting_entry.pop(image) == entry and cap == caps[image] and cap >= 2
                assert s in seen_free, f"image {image} admitted into slot {s}, which was not seen done"
                assert dev_img[s] is None or dev_img[s] in harvested, f"slot {s} reused before its harvest"
                seen_free.discard(s)
                admitted.append(image)
                admit_log.append((image, s))
                dev_img[s], dev_pos[s], dev_done[s] = image, 0, 0
            if not (triples and sch.wants_chunk()):
                break
        if sch.finished():
            break
        n = sch.next_steps()
        assert n >= 1, "not finished, yet nothing to step"
        for _ in range(n):
            for s in range(sch.slots):
                if not dev_done[s]:
                    dev_pos[s] += 1
                    if dev_pos[s] + 1 == true_len[dev_img[s]]:
                        dev_done[s] = 1
        for s, image, n_ids in sch.poll(list(dev_done), list(dev_pos)):
            assert dev_img[s] == image and dev_done[s] and n_ids == true_len[image]
            assert image not in harvested
            harvested.add(image)
            seen_free.add(s)
            order.append(image)
    assert sorted(admitted) == [i for i in range(N) if caps[i] > 1], "every image is admitted exactly once"
    assert sorted(order) == list(range(N)), "output indices are complete, each once"
    assert src == N and not waiting_entry
    return dict(order=order, steps=sch.steps, polls=sch.polls, admits=sch.admits, chunks=sch.chunks,
                admit_log=admit_log)


# ------------------------------------------------------------------------------------------------
# kernel cases
# ------------------------------------------------------------------------------------------------
GUARD = 64


def guarded(shape, dtype, fill, device="cpu"):
    """(whole, view): `view` of `shape` in the middle of a flat buffer with GUARD elements of `fill` on either side"""
    n = 1
    for s in shape:
        n *= s
    whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=device)
    return whole, whole[GUARD:GUARD + n].view(*shape)


def bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


ROW_POS = [0, 6, 7, 32, 63, 98]
ATTN_CASES = [("bf16", 8, 64)] + [(dt, H, Dh) for dt in ("f32", "bf16")
                                  for H, Dh in ((3, 16), (3, 32), (3, 64), (1, 128))]   # (dtype, H, Dh); first: rows


def make_ragged_attn(dtype, H, Dh, row_pos=ROW_POS, max_len=100, pad_idx=0, seed=0):
    """The decoder's layout: q = the first W columns of qkv [B, 3W]; K | V the halves of cache [B, max_len, 2W];
    tokens [B, max_len]. Rows j <= row_pos[b] hold data, with PAD-masked keys inside the prefix (j = 1 and
    j = row_pos - 2 where they exist; never every key); K / V rows at j > row_pos[b] are NaN and their tokens PAD."""
    g = torch.Generator().manual_seed(seed)
    dt = {"bf16": torch.bfloat16, "f32": torch.float32}[dtype]
    B, W = len(row_pos), H * Dh
    qkv = torch.randn(B, 3 * W, generator=g).to(dt)
    cache = torch.full((B, max_len, 2 * W), float("nan"), dtype=dt)
    tok = torch.full((B, max_len), pad_idx, dtype=torch.int64)
    for b, p in enumerate(row_pos):
        cache[b, :p + 1] = torch.randn(p + 1, 2 * W, generator=g).to(dt)
        tok[b, :p + 1] = 7
        for j in (1, p - 2):
            if 0 < j < p:
                tok[b, j] = pad_idx
                cache[b, j] = 1e4 * (1 if j % 2 else -1)   # a masked key's row has weight exactly 0
    return dict(qkv=qkv, cache=cache, tok=tok, row_pos=torch.tensor(row_pos, dtype=torch.int64), B=B, H=H, Dh=Dh, W=W,
                max_len=max_len, pad_idx=pad_idx, scale=float(torch.tensor(Dh ** -0.5, dtype=torch.float32)))


def reference_attn(t):
    """(o [B, W] float64, unit [B, W]) by decode_contract's formulas, row by row over its own prefix"""
    B, H, Dh, W = t["B"], t["H"], t["Dh"], t["W"]
    o, unit = torch.zeros(B, W, dtype=torch.float64), torch.zeros(B, W, dtype=torch.float64)
    for b in range(B):
        Lk = int(t["row_pos"][b]) + 1
        q = t["qkv"][b, :W].double().view(H, Dh)
        K = t["cache"][b, :Lk, :W].double().view(Lk, H, Dh)
        V = t["cache"][b, :Lk, W:].double().view(Lk, H, Dh)
        pad = t["tok"][b, :Lk] == t["pad_idx"]
        s = torch.einsum("hd,jhd->hj", q, K) * t["scale"]
        A = torch.einsum("hd,jhd->hj", q.abs(), K.abs()) * t["scale"] * L2E
        s = s.masked_fill(pad[None], -math.inf)
        A = A.masked_fill(pad[None], 0.0)
        p = torch.softmax(s, -1)
        o[b] = torch.einsum("hj,jhd->hd", p, V).reshape(W)
        unit[b] = (ULP * (1 + A.max(-1).values)[:, None] * torch.einsum("hj,jhd->hd", p, V.abs())).reshape(W)
    return o, unit


def pick_rule(pick, pos, done, limit, end, ld_ids):
    """The one rule of the ragged picks for one row -> (write column or None, new pos, new done, counted)"""
    if done:
        return None, pos, done, 0
    lim = min(limit, ld_ids)
    col = pos + 1 if pos + 1 < lim else None
    npos = pos + 1 if col is not None else pos
    fin = pick == end or pos + 2 >= lim
    return col, npos, 1 if fin else 0, 1 if fin else 0


# rows of the pick cases: (logits row as a list of V = 8 floats, expected argmax, done, pos, limit); T = ld_ids = 6.
# The NaN / +-0 / first-maximum rows are those of decode_contract's pick cases.
NAN, INF = float("nan"), float("inf")
PICK_T, PICK_END = 6, 5
PICK_ROWS = [
    ([0, 1, 2, 3, 4, 9, 6, 7], 5, 0, 1, 6),            # picks END
    ([0, 9, 2, 3, 4, 5, 6, 7], 1, 0, 2, 4),            # reaches its limit (pos + 2 == limit)
    ([0, 1, 2, 3, 4, 9, 6, 7], 5, 0, 3, 5),            # END and the limit at once: counted once
    ([0, 1, 9, 3, 4, 5, 6, 7], 2, 1, 2, 6),            # frozen: nothing written, position unchanged
    ([0, 1, 2, 9, 4, 5, 6, 7], 3, 0, 4, 6),            # limit == ld_ids: the last column, none past the row
    ([0, 1, 2, 3, 9, 5, 6, 7], 4, 0, 0, 6),            # an ordinary row: goes on
    ([1, NAN, 9, NAN, 4, 5, 6, 7], 1, 0, 1, 6),        # NaN is the largest; the first NaN wins
    ([-1, -0.0, 0.0, -3, -4, -5, -6, -7], 1, 0, 1, 6),  # -0.0 and +0.0 are equal: the first of them
    ([3, 7, 7, 2, 7, 1, 0, -1], 1, 0, 1, 6),           # first maximum
    ([-INF] * 8, 0, 0, 1, 6),                          # a row of -inf only picks column 0
]
