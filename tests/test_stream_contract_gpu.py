"""The kernels of sampled / constrained rolling-batch decode on the GPU against tests/stream_contract.py:
mit_logits_constrain_ragged and mit_sample_pick_ragged bit-equal, row by row, to the scalar-position entry points run
on that row alone and exact against the float references that pin those; the ragged picks' one state rule; done /
frozen rows, ld padding and guard bands untouched; a second launch and a recorded replay bitwise equal;
mit_slot_admit_ex beside mit_slot_admit."""
import numpy as np
import pytest
import torch

import constrain_contract as cc
import native as N
import rolling_contract as rc
import sample_contract as sc
import stream_contract as st

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -77


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    N.load_library()
    yield
    torch.cuda.empty_cache()


def _same(a, b):
    return torch.equal(rc.bits(a.cpu()), rc.bits(b.cpu()))


def _guards(whole, fill):
    head, tail = whole[:rc.GUARD].cpu(), whole[-rc.GUARD:].cpu()
    if fill != fill:
        return bool(torch.isnan(head).all() and torch.isnan(tail).all())
    return bool((head == fill).all() and (tail == fill).all())


def _logits(t):
    """(whole, rows [R, ld]): the case's logits in a NaN-guarded device buffer, NaN ld padding, misaligned by t['mis']"""
    R, V, ld, mis = t["R"], t["V"], t["ld"], t["mis"]
    whole, flat = rc.guarded((R * ld + 4,), torch.float32, st.NAN, DEV)
    rows = flat[mis:mis + R * ld].view(R, ld)
    rows[:, :V] = t["logits"].to(DEV)
    return whole, rows


# ------------------------------------------------------------------------------------------------
# mit_logits_constrain_ragged
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", cc.CON_V)
def test_constrain_ragged(V):
    t = st.make_constrain(V)
    R, ld = t["R"], t["ld"]
    tok = t["tok"].to(DEV)
    row_pos = torch.tensor(st.CON_POS, dtype=torch.int64, device=DEV)
    done = torch.tensor(st.CON_DONE, dtype=torch.int32, device=DEV)
    sup = torch.tensor(t["suppress"], dtype=torch.int64, device=DEV)
    forced = t["forced"].to(DEV)
    pidx = torch.tensor(st.CON_PROMPT_IDX, dtype=torch.int64, device=DEV)
    kw = dict(repetition_penalty=st.CON_THETA, no_repeat_ngram=st.CON_NGRAM, min_length=st.CON_MINLEN,
              end_id=t["end_id"], suppress=sup)

    def launch(rows):
        N.logits_constrain_ragged(rows, V, tok, row_pos, done=done, forced=forced, prompt_idx=pidx, **kw)

    whole, rows = _logits(t)
    before = whole.clone()
    launch(rows)
    torch.cuda.synchronize()
    got = rows.cpu()
    b_rows = before[rc.GUARD:-rc.GUARD][t["mis"]:t["mis"] + R * ld].view(R, ld).cpu()
    assert _guards(whole, st.NAN), "a guard band was written"
    assert _same(whole[rc.GUARD:rc.GUARD + t["mis"]], before[rc.GUARD:rc.GUARD + t["mis"]])
    assert _same(got[:, V:], b_rows[:, V:]), "ld padding was written"
    for name, dev_t, cpu_t in (("tok", tok, t["tok"]), ("forced", forced, t["forced"])):
        assert _same(dev_t, cpu_t), f"{name} was written"
    assert row_pos.tolist() == st.CON_POS and done.tolist() == st.CON_DONE and pidx.tolist() == st.CON_PROMPT_IDX
    seen_forced = 0
    for r, p in enumerate(st.CON_POS):
        if st.CON_DONE[r]:
            assert _same(got[r], b_rows[r]), f"done row {r} was written"
            continue
        # the float32 restatement on the row's own history: bitwise
        w = t["want"][r]
        bad = np.nonzero(got[r, :V].numpy().view(np.uint32) != w.view(np.uint32))[0]
        assert bad.size == 0, f"V {V} row {r} (p {p}): {bad.size} column(s) differ from the reference; first {bad[0]}"
        if r in (0, 1):   # the forced steps: -inf everywhere, 0 at the prompt's token
            f = int(t["forced"][st.CON_PROMPT_IDX[r], p + 1])
            seen_forced += int(w[f] == 0.0 and np.isinf(np.delete(w, f)).all())
        # the row alone through the scalar-position entry point with *pos = p: the same bits
        _, one = _logits(dict(t, R=1, logits=t["logits"][r:r + 1]))
        pi = st.CON_PROMPT_IDX[r]
        N.logits_constrain(one, V, tok[r:r + 1], row_pos[r:r + 1], forced=forced[pi:pi + 1] if pi >= 0 else None,
                           repetition_penalty=st.CON_THETA, no_repeat_ngram=st.CON_NGRAM, min_length=st.CON_MINLEN,
                           end_id=t["end_id"], suppress=sup)
        torch.cuda.synchronize()
        assert _same(one[0], got[r]), f"V {V} row {r} (p {p}) differs from mit_logits_constrain on that row alone"
    assert seen_forced == 2, "rows 0 and 1 are forced steps"
    # a second launch and a recorded replay on the same inputs: bitwise equal
    _, rows2 = _logits(t)
    launch(rows2)
    torch.cuda.synchronize()
    assert _same(rows2, got)
    _, rows3 = _logits(t)
    prog = N.record(lambda: launch(rows3))
    assert prog.launches() == 1
    rows3.copy_(b_rows.to(DEV))
    prog.run()
    torch.cuda.synchronize()
    assert _same(rows3, got), "the recorded launch replays differently"


# ------------------------------------------------------------------------------------------------
# mit_sample_pick_ragged
# ------------------------------------------------------------------------------------------------
def _pick_state():
    rows = st.PICK_STATES
    M, T = len(rows), rc.PICK_T
    g = torch.Generator().manual_seed(5)
    iw, ids = rc.guarded((M, T), torch.int64, SENT, DEV)
    lw, logprob = rc.guarded((M,), torch.float32, float(SENT), DEV)
    logprob.copy_(-(torch.rand(M, generator=g) * 8.0))
    nw, length = rc.guarded((M,), torch.int32, SENT, DEV)
    length.copy_(torch.tensor([r[1] for r in rows], dtype=torch.int32))
    return dict(M=M, iw=iw, ids=ids, lw=lw, logprob=logprob, nw=nw, length=length,
                row_pos=torch.tensor([r[1] for r in rows], dtype=torch.int64, device=DEV),
                done=torch.tensor([r[0] for r in rows], dtype=torch.int32, device=DEV),
                limit=torch.tensor([r[2] for r in rows], dtype=torch.int64, device=DEV),
                n_done=torch.tensor([5], dtype=torch.int32, device=DEV))


@pytest.mark.parametrize("hashed", [False, True], ids=["uniforms", "hash"])
@pytest.mark.parametrize("V", st.PICK_V)
def test_sample_pick_ragged(V, hashed):
    t = st.make_sample_pick(V, hashed)
    R, T, END = t["R"], rc.PICK_T, rc.PICK_END
    seed = st.seed_tensor(st.PICK_SEED, DEV)
    row_id = torch.tensor(st.PICK_ROW_ID, dtype=torch.int64, device=DEV)
    us = None if hashed else t["us"].to(DEV)

    def launch(s, rows):
        N.sample_pick_ragged(rows, V, st.PICK_T, st.PICK_K, t["top_p"], seed, row_id, us, s["ids"], s["row_pos"], END,
                             s["limit"], s["done"], s["n_done"], s["logprob"], s["length"])

    whole, rows = _logits(t)
    before = whole.clone()
    s = _pick_state()
    lp0, len0 = s["logprob"].clone(), s["length"].clone()
    launch(s, rows)
    torch.cuda.synchronize()
    assert _same(whole, before), "the logits were written"
    # token and state: exact, by the one rule of the ragged picks and the float64 reference of the draw
    want_ids = torch.full((R, T), SENT, dtype=torch.int64)
    pos, dn, counted = [], [], 0
    for r, (d0, p, lim) in enumerate(st.PICK_STATES):
        pk = t["refs"][r]["token"] if t["refs"][r] is not None else 0
        col, npos, nd, c = rc.pick_rule(pk, p, d0, lim, END, T)
        if col is not None:
            want_ids[r, col] = pk
        pos.append(npos)
        dn.append(nd)
        counted += c
    assert torch.equal(s["ids"].cpu(), want_ids), (s["ids"].cpu().tolist(), want_ids.tolist())
    assert s["row_pos"].tolist() == pos and s["done"].tolist() == dn
    # END; the limit; both at once, counted once; limit == ld_ids
    assert int(s["n_done"]) == 5 + counted and counted == 4
    assert _guards(s["iw"], SENT) and _guards(s["lw"], float(SENT)) and _guards(s["nw"], SENT)
    live = [r for r in range(R) if not st.PICK_STATES[r][0]]
    assert s["length"].tolist() == [int(len0[r]) + (r in live) for r in range(R)]
    # every live row alone through mit_sample_pick with row0 = row_id[r] and *pos = p: token and logprob bitwise
    for r in range(R):
        if r not in live:
            assert _same(s["logprob"][r], lp0[r]), "a frozen row's logprob was written"
            continue
        p = st.PICK_STATES[r][1]
        _, one = _logits(dict(t, R=1, logits=t["logits"][r:r + 1]))
        ids1 = torch.full((1, T), SENT, dtype=torch.int64, device=DEV)
        pos1 = torch.tensor([p], dtype=torch.int64, device=DEV)
        fin1, nfin1 = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
        lp1, len1 = lp0[r:r + 1].clone(), len0[r:r + 1].clone()
        N.sample_pick(one, V, st.PICK_T, st.PICK_K, t["top_p"], seed, st.PICK_ROW_ID[r],
                      None if hashed else us[r:r + 1], ids1, pos1, END, 0, fin1, nfin1, lp1, len1,
                      torch.zeros(1, dtype=torch.int32, device=DEV))
        torch.cuda.synchronize()
        assert int(ids1[0, p + 1]) == int(s["ids"][r, p + 1]), f"V {V} row {r}: token differs from mit_sample_pick"
        assert _same(lp1[0], s["logprob"][r]), f"V {V} row {r}: logprob differs from mit_sample_pick bitwise"
    # a second launch from the same state: bitwise equal
    _, rows2 = _logits(t)
    s2 = _pick_state()
    launch(s2, rows2)
    torch.cuda.synchronize()
    for k in ("iw", "lw", "nw", "row_pos", "done", "n_done"):
        assert _same(s2[k], s[k]), k
    # stepped again: the rows now done are frozen, NaN or not
    ids_b, lp_b = s["ids"].clone(), s["logprob"].clone()
    launch(s, rows)
    torch.cuda.synchronize()
    for r in range(R):
        if dn[r]:
            assert torch.equal(s["ids"][r], ids_b[r]) and _same(s["logprob"][r], lp_b[r]) and \
                int(s["row_pos"][r]) == pos[r], f"frozen row {r} was written"


def test_sample_pick_ragged_is_recordable():
    """MIT_RECORD: the recorded launch replays on the positions and the state of the replay."""
    V, T = 16, 6
    logits = torch.randn(2, V, device=DEV)
    ids = torch.full((2, T), SENT, dtype=torch.int64, device=DEV)
    row_pos = torch.tensor([0, 2], dtype=torch.int64, device=DEV)
    done = torch.zeros(2, dtype=torch.int32, device=DEV)
    limit = torch.full((2,), T, dtype=torch.int64, device=DEV)
    n_done = torch.zeros(1, dtype=torch.int32, device=DEV)
    lp, ln = torch.zeros(2, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
    seed, rid = st.seed_tensor(3, DEV), torch.tensor([4, 9], dtype=torch.int64, device=DEV)
    prog = N.record(lambda: N.sample_pick_ragged(logits, V, 1.0, 0, 1.0, seed, rid, None, ids, row_pos, -1, limit, done,
                                                 n_done, lp, ln))
    assert prog.launches() == 1
    prog.run()
    torch.cuda.synchronize()
    assert row_pos.tolist() == [2, 4] and ln.tolist() == [2, 2] and done.tolist() == [0, 0]
    assert (ids[0, 1:3] != SENT).all() and (ids[1, 3:5] != SENT).all() and int((ids != SENT).sum()) == 4


# ------------------------------------------------------------------------------------------------
# mit_slot_admit_ex
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("m", [0, 4])
def test_slot_admit_ex(m, fp8):
    g = torch.Generator().manual_seed(11 + m)
    L, S, slots, pool, T, ns = 2, 3, 5, 4, 24, 4
    dt = torch.uint8 if fp8 else torch.bfloat16
    d2 = 32 if fp8 else 16                                   # row_bytes = 32
    src = torch.randint(0, 255, (L, pool * S, d2), generator=g).to(dt) if fp8 else \
        torch.randn(L, pool * S, d2, generator=g).to(dt)
    pool_kv = src.to(DEV)
    pool_scale = torch.randn(L, pool, ns, generator=g).to(DEV) if fp8 else None
    # (slot, pool image, cap, row id, prompt index); the third is out of range (pool image 4): nothing of it is written
    records = [(4, 0, 7, (1 << 33) + 5, 2), (0, 3, 24, 17, -1), (2, 4, 9, 99, 1), (3, 1, 2, 0, 0)][:m]
    valid = [r for r in records if r[1] < pool]

    def state():
        kw, kv = rc.guarded((L, slots * S, d2), dt, 7, DEV)
        sw = scale = None
        if fp8:
            sw, scale = rc.guarded((L, slots, ns), torch.float32, float(SENT), DEV)
        iw, ids = rc.guarded((slots, T), torch.int64, SENT, DEV)
        s = dict(kw=kw, kv=kv, sw=sw, scale=scale, iw=iw, ids=ids,
                 row_pos=torch.full((slots,), 9, dtype=torch.int64, device=DEV),
                 done=torch.ones(slots, dtype=torch.int32, device=DEV),
                 limit=torch.ones(slots, dtype=torch.int64, device=DEV),
                 n_done=torch.tensor([5], dtype=torch.int32, device=DEV))
        for name, dtp in (("row_id", torch.int64), ("prompt_idx", torch.int64), ("logprob", torch.float32),
                          ("length", torch.int32)):
            s[name + "_w"], s[name] = rc.guarded((slots,), dtp, SENT, DEV)
        return s

    a = state()
    rec = torch.tensor(records + [(1, 1, 3, 3, 3)] * (slots - m), dtype=torch.int64, device=DEV)   # rows >= m: not read
    N.slot_admit_ex(rec, m, pool_kv, a["kv"], S, pool_scale, a["scale"], a["ids"], 2, a["row_pos"], a["done"],
                    a["limit"], a["n_done"], a["row_id"], a["prompt_idx"], a["logprob"], a["length"])
    b = state()
    tr = rec[:, :3].contiguous()
    N.slot_admit(tr, m, pool_kv, b["kv"], S, pool_scale, b["scale"], b["ids"], 2, b["row_pos"], b["done"], b["limit"],
                 b["n_done"])
    torch.cuda.synchronize()
    # mit_slot_admit's results, unchanged and the same
    want_kv = torch.full((L, slots, S, d2), 7, dtype=dt)
    want_ids = torch.full((slots, T), SENT, dtype=torch.int64)
    want_pos, want_done, want_lim = [9] * slots, [1] * slots, [1] * slots
    want_scale = torch.full((L, slots, ns), float(SENT))
    want_new = {k: [SENT] * slots for k in ("row_id", "prompt_idx", "logprob", "length")}
    for s_, e, cap, rid, pi in valid:
        want_kv[:, s_] = src.view(L, pool, S, d2)[:, e]
        want_ids[s_, 0] = 2
        want_pos[s_], want_done[s_], want_lim[s_] = 0, 0, cap
        want_new["row_id"][s_], want_new["prompt_idx"][s_] = rid, pi
        want_new["logprob"][s_], want_new["length"][s_] = 0.0, 0
        if fp8:
            want_scale[:, s_] = pool_scale[:, e].cpu()
    for x, who in ((a, "mit_slot_admit_ex"), (b, "mit_slot_admit")):
        assert _same(x["kv"].view(L, slots, S, d2), want_kv), f"{who}: K/V copy"
        assert _guards(x["kw"], 7) and _guards(x["iw"], SENT)
        assert torch.equal(x["ids"].cpu(), want_ids), who
        assert x["row_pos"].tolist() == want_pos and x["done"].tolist() == want_done and \
            x["limit"].tolist() == want_lim, who
        assert int(x["n_done"]) == 5 - len(valid), f"{who}: an out-of-range record is not counted"
        if fp8:
            assert _same(x["scale"], want_scale) and _guards(x["sw"], float(SENT)), who
    assert _same(pool_kv, src)
    for k in want_new:
        assert a[k].tolist() == want_new[k], f"{k}: written for the named slots only"
        assert _guards(a[k + "_w"], SENT), k
        assert (b[k] == SENT).all(), f"mit_slot_admit wrote {k}"


def test_slot_admit_ex_is_recordable():
    L, S, d2, T = 2, 3, 8, 6
    pool_kv = torch.randn(L, 2 * S, d2, device=DEV).to(torch.bfloat16)
    kv = torch.zeros(L, 2 * S, d2, device=DEV, dtype=torch.bfloat16)
    ids = torch.full((2, T), SENT, dtype=torch.int64, device=DEV)
    row_pos = torch.full((2,), 4, dtype=torch.int64, device=DEV)
    done = torch.ones(2, dtype=torch.int32, device=DEV)
    limit = torch.ones(2, dtype=torch.int64, device=DEV)
    n_done = torch.tensor([2], dtype=torch.int32, device=DEV)
    rid, pidx = torch.zeros(2, dtype=torch.int64, device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV)
    lp, ln = torch.ones(2, device=DEV), torch.ones(2, dtype=torch.int32, device=DEV)
    rec = torch.tensor([[1, 0, 5, 40, -1]], dtype=torch.int64, device=DEV)
    prog = N.record(lambda: N.slot_admit_ex(rec, 1, pool_kv, kv, S, None, None, ids, 2, row_pos, done, limit, n_done,
                                            rid, pidx, lp, ln))
    assert prog.launches() == 1
    rec.copy_(torch.tensor([[0, 1, 7, 41, 3]]))
    prog.run()
    torch.cuda.synchronize()
    assert torch.equal(kv[:, :S], pool_kv[:, S:]) and torch.equal(kv[:, S:], pool_kv[:, :S])
    assert done.tolist() == [0, 0] and limit.tolist() == [7, 5] and int(n_done) == 0
    assert rid.tolist() == [41, 40] and pidx.tolist() == [3, -1] and lp.tolist() == [0.0, 0.0] and ln.tolist() == [0, 0]
