"""The contract of sampled / constrained rolling-batch captioning (csrc/constrain.hip mit_logits_constrain_ragged,
csrc/sample.hip mit_sample_pick_ragged, csrc/rolling.hip mit_slot_admit_ex, decoder.RollingState's opt-in state,
rolling.RollingScheduler(samples=N), ImageToTextModel.generate_stream_iter), in the manner of rolling_contract.py:
the builders of the kernel cases, a scripted driver of the scheduler with several samples per image, and the GEMM
family query the end-to-end comparisons are made under.

A row's arithmetic does not depend on its neighbours, its slot or the other rows' positions, and its random stream
only on (seed, global row id, position): the kernel tests compare every live row BITWISE with the scalar-position
entry point launched on that row alone, and with the float references of constrain_contract / sample_contract that
pin those entry points.
"""
import ctypes

import numpy as np
import torch

import constrain_contract as cc
import rolling_contract as rc
import sample_contract as sc

NAN = float("nan")


# ------------------------------------------------------------------------------------------------
# the schedule with `samples` work items per image
# ------------------------------------------------------------------------------------------------
def flat(lengths):
    """item lengths in row-id order (image-major) from lengths[image][sample]"""
    return [n for per in lengths for n in per]


def drive_samples(sch, lengths, caps):
    """rolling_contract.drive for a RollingScheduler(samples=N): lengths[image][sample] ids per item, caps[image] >= 1.
    Plays the device and asserts: every (image, sample) admitted exactly once and only into a slot seen empty or
    done; an item's record names its image's pool entry, which still holds that image (a pool entry is not
    overwritten before ALL its samples got a slot); harvest before reuse; complete output. Returns dict(order [row
    ids], steps, admits, chunks)."""
    N, B = sch.samples, len(lengths)
    assert all(len(per) == N for per in lengths)
    true_len = {i * N + n: min(lengths[i][n], caps[i]) for i in range(B) for n in range(N)}
    dev_pos, dev_done, dev_item = [0] * sch.slots, [1] * sch.slots, [None] * sch.slots
    pool = [None] * sch.pool                     # image whose K/V an entry holds
    waiting = {}                                 # image -> samples of it still without a slot
    seen_free = set(range(sch.slots))
    harvested, admitted, order = set(), [], []
    src = guard = 0
    while True:
        guard += 1
        assert guard < 100000, "the schedule does not terminate"
        while True:
            while sch.wants_chunk():
                if src >= B:
                    sch.close()
                    break
                n = min(sch.encode_batch, B - src)
                at, trivial = sch.add_chunk(caps[src:src + n])
                assert at % sch.encode_batch == 0 and at + n <= sch.pool
                for j in range(n):
                    assert not waiting.get(pool[at + j]), \
                        f"entry {at + j} overwritten while samples of image {pool[at + j]} wait for a slot"
                    pool[at + j] = src + j
                    if caps[src + j] > 1:
                        waiting[src + j] = set(range(N))
                assert trivial == [src + j for j in range(n) if caps[src + j] == 1]
                order.extend(i * N + k for i in trivial for k in range(N))
                src += n
            recs = sch.admissions_ex()
            assert len({r[0] for r in recs}) == len(recs)
            for s, entry, cap, row in recs:
                image, k = divmod(row, N)
                assert pool[entry] == image, f"row {row}: entry {entry} holds image {pool[entry]}"
                assert k in waiting[image], f"row {row} admitted twice"
                waiting[image].discard(k)
                assert cap == caps[image] and cap >= 2
                assert s in seen_free, f"row {row} admitted into slot {s}, which was not seen done"
                assert dev_item[s] is None or dev_item[s] in harvested, f"slot {s} reused before its harvest"
                seen_free.discard(s)
                admitted.append(row)
                dev_item[s], dev_pos[s], dev_done[s] = row, 0, 0
            if not (recs and sch.wants_chunk()):
                break
        if sch.finished():
            break
        n = sch.next_steps()
        assert n >= 1, "not finished, yet nothing to step"
        for _ in range(n):
            for s in range(sch.slots):
                if not dev_done[s]:
                    dev_pos[s] += 1
                    if dev_pos[s] + 1 == true_len[dev_item[s]]:
                        dev_done[s] = 1
        for s, row, n_ids in sch.poll(list(dev_done), list(dev_pos)):
            assert dev_item[s] == row and dev_done[s] and n_ids == true_len[row]
            assert row not in harvested
            harvested.add(row)
            seen_free.add(s)
            order.append(row)
    assert sorted(admitted) == [i * N + k for i in range(B) if caps[i] > 1 for k in range(N)], \
        "every (image, sample) is admitted exactly once"
    assert sorted(order) == list(range(B * N)), "output items are complete, each once"
    assert src == B and not any(waiting.values())
    return dict(order=order, steps=sch.steps, admits=sch.admits, chunks=sch.chunks)


# ------------------------------------------------------------------------------------------------
# GEMM families: what the end-to-end comparisons assert first
# ------------------------------------------------------------------------------------------------
_P = 1 << 22          # a 16-B aligned address: the plan queries dereference nothing


def gemm_families(N, dec, M, fused):
    """The kernel family of every GEMM of one token step of decoder `dec` at M rows, through the library's plan
    queries (host only): the step's six GEMMs per layer -- mit_decode_gemm plans (a_mode, act, r_mode, c_f32, waves,
    block_rows) on the fused bf16 step, (tile, split-K) of mit_gemm otherwise -- and the f32 vocabulary head's (tile,
    split-K)."""
    d, F = dec.d, dec.F
    Vp = dec.store.w("fc_out.weight").shape[0]
    dt = N.BF16 if dec.dtype == torch.bfloat16 else N.F32

    def mit_gemm(n, k, act=0, out_f32=0):
        g = N.GemmArgs(dt, N.K_CONTIG, N.K_CONTIG, M, n, k, _P, k, _P, k, _P, n, 1.0, _P, act, None, n, None, n, 1.0,
                       0.0, None, 0, out_f32, 0, None, None, 0, None, None, 0, 0.0, None, 0, None)
        return N.gemm_plan(g)

    def decode_gemm(n, k, a_ln=False, act=0, r_mode=0, c=True):
        g = N.DecodeGemmArgs(M, n, k, _P, k, _P if a_ln else None, _P if a_ln else None, _P if a_ln else None, _P, k,
                             _P, act, 0, _P if c else None, n if c else 0, r_mode, _P if r_mode else None,
                             n if r_mode else 0, _P if r_mode == 2 else None, _P if r_mode == 2 else None,
                             _P if r_mode == 2 else None, 1e-5, None if c else _P, 0 if c else n, None if c else _P,
                             None, 0, 0, 0, None, None)
        p = N.decode_gemm_plan(g)
        assert p is not None, (n, k, a_ln, act, r_mode, c)
        return (p.a_mode, p.act, p.r_mode, p.c_f32, p.waves, p.block_rows)

    out = []
    if fused:
        for l in range(dec.L):
            out += [decode_gemm(3 * d, d, a_ln=l > 0), decode_gemm(d, d, r_mode=2 if l else 1, c=False),
                    decode_gemm(d, d, a_ln=True), decode_gemm(d, d, r_mode=2, c=False),
                    decode_gemm(F, d, a_ln=True, act=N.ACT_RELU), decode_gemm(d, F, r_mode=2, c=False)]
    else:
        out += [mit_gemm(3 * d, d), mit_gemm(d, d), mit_gemm(F, d, act=N.ACT_RELU), mit_gemm(d, F)]
    out.append(mit_gemm(Vp, d, out_f32=1))
    return out


class _Probe:
    def __init__(self, N):
        self.N, self.rows = N, []

    def before(self, *a):
        pass

    def after(self, g):
        self.rows.append((g.N, g.K, self.N.gemm_plan(g)))


def chunk_families(N, model, pixels):
    """The kernel family of every GEMM an encoder chunk of these images runs before the token steps: the encoder's
    and the projection's, read off the launches themselves (native.set_gemm_probe + the plan query), and the
    cross-attention K/V GEMM's. These go by the chunk's row count (images x memory rows) as the step's go by the
    slots: one image of 197 rows takes the register-streaming family (M <= 256), two or more the tile kernels."""
    probe = _Probe(N)
    N.set_gemm_probe(probe)
    try:
        _, _, S, _, _ = model._encode_memory(pixels.float())
        torch.cuda.synchronize()
    finally:
        N.set_gemm_probe(None)
    d, M = model.decoder.d, pixels.shape[0] * S
    dt = N.BF16 if model.dtype == torch.bfloat16 else N.F32
    g = N.GemmArgs(dt, N.K_CONTIG, N.K_CONTIG, M, 2 * d, d, _P, d, _P, d, _P, 2 * d, 1.0, _P, 0, None, 2 * d, None, 2 * d,
                   1.0, 0.0, None, 0, 0, 0, None, None, 0, None, None, 0, 0.0, None, 0, None)
    return probe.rows + [(2 * d, d, N.gemm_plan(g))]


# ------------------------------------------------------------------------------------------------
# mit_logits_constrain_ragged: one launch of seven rows
# ------------------------------------------------------------------------------------------------
CON_POS = [0, 1, 2, 5, 17, 255, 300]     # 300 > the block's 256 threads: the strided history loops run twice
CON_DONE = [0, 0, 0, 1, 1, 0, 0]         # row 3 is full of NaN
CON_LD_TOK, CON_LD_FORCED = 512, 8
CON_NGRAM, CON_THETA, CON_MINLEN = 3, 1.3, 3      # p + 1 < 3 (rows 0, 1), p + 1 == 3 (row 2), beyond (the others)
# rows of the prompt table: lengths 0, 1, ld_forced - 1, 3; the per-row indices include -1
CON_PROMPT_LEN = [0, 1, CON_LD_FORCED - 1, 3]
CON_PROMPT_IDX = [1, 2, -1, 3, 2, 0, 2]
# row 0 (p 0) forced by the prompt of length 1; row 1 (p 1) by the full-length prompt; row 2 has no prompt; row 5's
# prompt is empty; row 6 is past its prompt (p + 1 >= ld_forced): rows 2, 5, 6 get the free edits


def make_constrain(V, seed=0):
    """CPU tensors of the case: logits [7, ld] in a NaN-guarded buffer (ld padding NaN), histories from a small
    alphabet with out-of-range ids mixed in (constrain_contract.make_case's recipe), the prompt table, the suppress
    list, and per live row the expected float32 row."""
    g = torch.Generator().manual_seed(1000 + V + seed)
    R = len(CON_POS)
    ld = V + (0 if V in (512, 10000) else 3)
    mis = 1 if V == 509 else 0
    alpha = torch.randperm(V, generator=g)[:min(6, V)]
    pool = torch.cat([alpha, torch.tensor([V, V + 3, -5])])
    wts = torch.cat([torch.full((alpha.numel(),), 1.0), torch.full((3,), 0.25)])
    tok = torch.full((R, CON_LD_TOK), int(alpha[0]), dtype=torch.int64)      # past p: never read
    for r, p in enumerate(CON_POS):
        tok[r, :p + 1] = pool[torch.multinomial(wts, p + 1, replacement=True, generator=g)]
    end_id = int(alpha[1 % alpha.numel()])
    lg = torch.randn(R, V, generator=g) * 3.0
    for r in range(R):
        for k, a in enumerate(alpha.tolist()):
            lg[r, a] = cc.SPECIALS[(k + r) % len(cc.SPECIALS)]
    lg[3] = NAN
    suppress = [int(alpha[0]), end_id, V + 1, -3, int(alpha[-1]), (int(alpha[0]) + 1) % V]
    forced = torch.full((len(CON_PROMPT_LEN), CON_LD_FORCED), -1, dtype=torch.int64)
    for i, n in enumerate(CON_PROMPT_LEN):
        forced[i, 1:1 + n] = torch.randint(0, V, (n,), generator=g)
    forced[:, 0] = int(alpha[0])            # column 0 is START's: never applied
    want = []
    for r, p in enumerate(CON_POS):
        if CON_DONE[r]:
            want.append(None)
            continue
        pi = CON_PROMPT_IDX[r]
        f = int(forced[pi, p + 1]) if pi >= 0 and p + 1 < CON_LD_FORCED else -1
        want.append(cc.constrain_reference(lg[r].numpy(), tok[r, :p + 1].tolist(), CON_THETA, CON_NGRAM, CON_MINLEN,
                                           end_id, suppress, f))
    return dict(R=R, V=V, ld=ld, mis=mis, logits=lg, tok=tok, end_id=end_id, suppress=suppress, forced=forced,
                want=want)


# ------------------------------------------------------------------------------------------------
# mit_sample_pick_ragged: the state cases of rolling_contract.PICK_ROWS x the kernel's instantiations
# ------------------------------------------------------------------------------------------------
# (done, pos, limit) of rolling_contract.PICK_ROWS[:6] with T = ld_ids = 6 and END = 5; rows 0 and 2 draw END
PICK_STATES = [(r[2], r[3], r[4]) for r in rc.PICK_ROWS[:6]]
PICK_DRAWS_END = [True, False, True, False, False, False]
# weights in registers (1 and 10 chunks per thread), keys cached in LDS, keys re-read: sample_contract.PICK_CASES'
# geometry (509: odd, misaligned, scalar loads; the others 16-B loads, 12293 with a ragged last chunk)
PICK_V = (509, 10000, 12288, 12293)
PICK_ROW_ID = [0, 7, (1 << 20) + 3, 5, 123456, 2]
PICK_SEED = 0x1234_5678_9ABC_DEF0
PICK_T, PICK_K, PICK_P = 0.7, 50, 0.9


def make_sample_pick(V, hashed):
    """CPU tensors of the case: logits [6, ld] (row 3, frozen, NaN), the uniforms (supplied: the midpoint of a kept
    token's interval; hashed: sample_contract.uniform_reference of (seed, row id, position)), and per live row the
    float64 reference. Rows that draw END hold a logit so far above the others that END is the whole top-p prefix;
    the others hold -inf at END. The generator is advanced until every float margin of every live row is at least
    2 TAU_U, so a float32 kernel has no freedom in any pick."""
    R, END = len(PICK_STATES), rc.PICK_END
    ld = V + (0 if V % 4 == 0 else 3)
    mis = 1 if V == 509 else 0
    case = sc.PickCase("stream", 1, V, PICK_T, PICK_K, PICK_P)
    fin = torch.tensor([s[0] for s in PICK_STATES], dtype=torch.int32)
    for attempt in range(64):
        g = torch.Generator().manual_seed(7000 + V + 100 * attempt)
        lg = torch.randn(R, V, generator=g) * 5.0
        for r in range(R):
            lg[r, END] = float(lg[r].max()) + 40.0 if PICK_DRAWS_END[r] else float("-inf")
        top_p = sc._choose_top_p(case, lg[1:2], fin[1:2])    # from row 1: an ordinary distribution
        us, refs, ok = np.zeros(R, dtype=np.float32), [None] * R, True
        for r in range(R):
            if int(fin[r]):
                continue
            p = PICK_STATES[r][1]
            if hashed:
                u = float(sc.uniform_reference(PICK_SEED, PICK_ROW_ID[r], 1, p)[0])
            else:
                ref = sc.pick_reference(lg[r], PICK_T, PICK_K, top_p, 0.5)
                pr = np.where(ref["probs"] >= 5 * sc.TAU_U, ref["probs"], 0.0)
                j = int(torch.multinomial(torch.from_numpy(pr / pr.sum()), 1, generator=g))
                u = float(np.float32(ref["probs"][:j].sum() + ref["probs"][j] / 2))
            refs[r] = sc.pick_reference(lg[r], PICK_T, PICK_K, top_p, u)
            us[r] = u
            ok = ok and min(refs[r]["margin_u"], refs[r]["margin_p"]) >= 2 * sc.TAU_U
            ok = ok and (refs[r]["token"] == END) == PICK_DRAWS_END[r]
        if ok:
            break
    else:
        raise AssertionError(f"V {V}: no seed gives margins of at least {2 * sc.TAU_U}")
    lg = lg.clone()
    lg[fin != 0] = NAN
    return dict(R=R, V=V, ld=ld, mis=mis, logits=lg, us=torch.from_numpy(us), refs=refs, top_p=top_p, fin=fin)


def seed_tensor(seed, device):
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    return torch.tensor([s - (1 << 64) if s >= (1 << 63) else s], dtype=torch.int64, device=device)


def aligned_buffer(n=1 << 16):
    buf = ctypes.create_string_buffer(n + 64)
    return buf, ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
