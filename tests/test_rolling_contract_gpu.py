"""The rolling-batch kernels on the GPU against tests/rolling_contract.py: mit_attention_decode_ragged (both kernel
families) bit-equal, row by row, to the scalar-pos entry point run on that row alone and within decode_contract's bound
of the float64 reference, with NaN K / V rows and PAD tokens past every row's prefix; mit_embed_decode_ragged and
mit_kv_store_ragged on sentinel-filled guarded buffers; the two ragged picks' one rule; mit_slot_admit."""
import pytest
import torch

import decode_contract as dc
import native as N
import rolling_contract as rc

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -77
_DT = {"bf16": torch.bfloat16, "f32": torch.float32}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    N.load_library()
    yield
    torch.cuda.empty_cache()


def _same(a, b):
    return torch.equal(rc.bits(a.cpu()), rc.bits(b.cpu()))


@pytest.mark.parametrize("dtype,H,Dh", rc.ATTN_CASES, ids=[f"{d}-H{h}-Dh{e}" for d, h, e in rc.ATTN_CASES])
def test_ragged_attention(dtype, H, Dh):
    t = rc.make_ragged_attn(dtype, H, Dh)
    B, W, Tm = t["B"], t["W"], t["max_len"]
    qkv, cache, tok, rp = (t[k].to(DEV) for k in ("qkv", "cache", "tok", "row_pos"))
    whole, o = rc.guarded((B, W), _DT[dtype], SENT, DEV)
    args = dict(key_tokens=tok, tok_batch=Tm, pad_idx=t["pad_idx"], scale=t["scale"], Dh=Dh)
    fam = N.attention_decode_ragged_plan(N.BF16 if dtype == "bf16" else N.F32, B, H, Dh, qkv.data_ptr(), 3 * W,
                                         cache.data_ptr(), 2 * W, Tm * 2 * W, cache[:, :, W:].data_ptr(), 2 * W,
                                         Tm * 2 * W, o.data_ptr(), W, row_pos=rp.data_ptr(), key_tokens=tok.data_ptr())
    assert fam == (N.DECODE_ATTN_ROWS if dtype == "bf16" and W == 512 else N.DECODE_ATTN_BH)
    N.attention_decode_ragged(qkv, 3 * W, cache, 2 * W, Tm * 2 * W, cache[:, :, W:], 2 * W, Tm * 2 * W, o, W, B, H,
                              row_pos=rp, **args)
    torch.cuda.synchronize()
    got = o.cpu()
    assert not torch.isnan(got.float()).any(), "a K / V row or token past a row's prefix was read"
    assert (whole[:rc.GUARD] == SENT).all() and (whole[-rc.GUARD:] == SENT).all()
    for name, dev_t in (("qkv", qkv), ("cache", cache), ("tok", tok), ("row_pos", rp)):
        assert _same(dev_t, t[name]), f"{name} was written"
    # row b alone through the scalar-pos entry point with *pos = row_pos[b]: the same bits
    for b in range(B):
        o1 = torch.full((1, W), SENT, dtype=_DT[dtype], device=DEV)
        cb = cache[b:b + 1]
        N.attention_decode(qkv[b:b + 1], 3 * W, cb, 2 * W, Tm * 2 * W, cb[:, :, W:], 2 * W, Tm * 2 * W, o1, W, 1, H,
                           pos=rp[b:b + 1], key_tokens=tok[b:b + 1], tok_batch=Tm, pad_idx=t["pad_idx"],
                           scale=t["scale"], Dh=Dh)
        assert _same(o1[0], got[b]), f"row {b} (row_pos {int(t['row_pos'][b])}) differs from the scalar-pos kernel"
    ref, unit = rc.reference_attn(t)
    figs = []
    dc.check_float("o", "attn", got, ref, unit, dtype == "bf16", figs)
    print(f"ragged attention {dtype} H{H} Dh{Dh}: {figs[0][2]:.3f} units (bound {dc.BOUND['attn']:.3f})")
    assert figs[0][2] <= dc.BOUND["attn"]


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_ragged_embed_and_kv_store(dtype):
    dt = _DT[dtype]
    g = torch.Generator().manual_seed(1)
    row_pos = rc.ROW_POS
    B, d, Tm, V = len(row_pos), 48, 100, 5
    rp = torch.tensor(row_pos, dtype=torch.int64, device=DEV)
    # embed: ids columns other than row_pos[b] name the NaN table row
    table = torch.randn(V, d, generator=g).to(dt)
    table[2] = float("nan")
    pe = torch.randn(Tm, d, generator=g)
    ids = torch.full((B, Tm), 2, dtype=torch.int64)
    for b, p in enumerate(row_pos):
        ids[b, p] = (0, 1, 3, 4)[b % 4]
    whole, out = rc.guarded((B, d), dt, SENT, DEV)
    tb, pd, idd = table.to(DEV), pe.to(DEV), ids.to(DEV)
    N.embed_decode_ragged(idd, rp, tb, 3.0, pd, out)
    torch.cuda.synchronize()
    assert (whole[:rc.GUARD] == SENT).all() and (whole[-rc.GUARD:] == SENT).all()
    for b, p in enumerate(row_pos):
        o1 = torch.empty(1, d, dtype=dt, device=DEV)
        N.embed_decode(idd[b:b + 1], rp[b:b + 1], tb, 3.0, pd, o1)
        assert _same(o1[0], out[b]), f"embed row {b}"
        ref = table[ids[b, p]].double() * 3.0 + pe[p].double()
        # float32 arithmetic (fused or not) on the two terms, then in bf16 the output rounding
        tol = 2.0 ** -22 * (table[ids[b, p]].double().abs() * 3.0 + pe[p].double().abs())
        if dtype == "bf16":
            tol = tol + 2.0 ** -8 * ref.abs()
        assert ((out[b].cpu().double() - ref).abs() <= tol).all(), f"embed row {b} against float64"
    # kv_store: only cache row row_pos[b] of row b changes, bitwise src's K | V columns
    W = 24
    src = torch.randn(B, 3 * W, generator=g).to(dt).to(DEV)
    cwhole, cache = rc.guarded((B, Tm, 2 * W), dt, SENT, DEV)
    N.kv_store_ragged(src[:, W:], 3 * W, cache, 2 * W, Tm * 2 * W, B, 2 * W, rp)
    torch.cuda.synchronize()
    want = torch.full((B, Tm, 2 * W), SENT, dtype=dt)
    for b, p in enumerate(row_pos):
        want[b, p] = src[b, W:].cpu()
    assert _same(cache, want)
    assert (cwhole[:rc.GUARD] == SENT).all() and (cwhole[-rc.GUARD:] == SENT).all()


def _pick_state(rows, reps=1):
    rows = rows * reps
    M, T = len(rows), rc.PICK_T
    iw, ids = rc.guarded((M, T), torch.int64, SENT, DEV)
    st = dict(M=M, iw=iw, ids=ids,
              row_pos=torch.tensor([r[3] for r in rows], dtype=torch.int64, device=DEV),
              done=torch.tensor([r[2] for r in rows], dtype=torch.int32, device=DEV),
              limit=torch.tensor([r[4] for r in rows], dtype=torch.int64, device=DEV),
              n_done=torch.tensor([5], dtype=torch.int32, device=DEV))
    return rows, st


def _check_picks(rows, st, picks, n0=5):
    T = rc.PICK_T
    want = torch.full((st["M"], T), SENT, dtype=torch.int64)
    pos, done, counted = [], [], 0
    for b, (r, pk) in enumerate(zip(rows, picks)):
        col, npos, nd, c = rc.pick_rule(pk, r[3], r[2], r[4], rc.PICK_END, T)
        if col is not None:
            want[b, col] = pk
        pos.append(npos)
        done.append(nd)
        counted += c
    assert torch.equal(st["ids"].cpu(), want), "ids: a pick is wrong or an untouched column was written"
    assert (st["iw"][:rc.GUARD] == SENT).all() and (st["iw"][-rc.GUARD:] == SENT).all()
    assert st["row_pos"].tolist() == pos and st["done"].tolist() == done
    assert int(st["n_done"]) == n0 + counted
    return want, pos, done, n0 + counted


def test_greedy_pick_ragged():
    rows, st = _pick_state(rc.PICK_ROWS)
    V, ld = 8, 12
    lw, logits = rc.guarded((st["M"], ld), torch.float32, float("nan"), DEV)   # pad columns V .. ld-1: NaN, never read
    logits[:, :V] = torch.tensor([r[0] for r in rows], dtype=torch.float32, device=DEV)
    before = logits.clone()
    N.greedy_pick_ragged(logits, st["ids"], st["row_pos"], rc.PICK_END, st["limit"], st["done"], st["n_done"], V=V)
    torch.cuda.synchronize()
    picks = [r[1] for r in rows]
    assert [dc.ref_argmax(torch.tensor(r[0], dtype=torch.float32)) for r in rows] == picks
    want, pos, done, n = _check_picks(rows, st, picks)
    assert _same(logits, before)
    # the 4-B path (ld % 4 != 0) picks the same; rows already done are now frozen
    rows2 = [(r[0], r[1], d, p, r[4]) for r, d, p in zip(rows, done, pos)]
    l2 = torch.full((st["M"], 9), float("nan"), device=DEV)
    l2[:, :V] = logits[:, :V]
    ids_before = st["ids"].clone()
    N.greedy_pick_ragged(l2, st["ids"], st["row_pos"], rc.PICK_END, st["limit"], st["done"], st["n_done"], V=V)
    torch.cuda.synchronize()
    for b, r in enumerate(rows2):
        col, npos, nd, c = rc.pick_rule(r[1], r[3], r[2], r[4], rc.PICK_END, rc.PICK_T)
        if r[2]:
            assert col is None and torch.equal(st["ids"][b], ids_before[b]), f"frozen row {b} was written"
        else:
            assert int(st["ids"][b, col]) == r[1] and int(st["row_pos"][b]) == npos
        n += c
    assert int(st["n_done"]) == n


@pytest.mark.parametrize("reps", [1, 103])   # 1030 rows: past the one block's 1024 threads
def test_greedy_pick_keys_ragged(reps):
    rows, st = _pick_state(rc.PICK_ROWS, reps)
    M = st["M"]
    v = torch.tensor([r[0] for r in rows], dtype=torch.float32)
    pk = dc.pack_key(v, torch.arange(8)[None, :].expand(M, 8))
    keys = torch.zeros(dc.ARGMAX_SLOTS, M, dtype=torch.int64)
    for c in range(8):                       # column c's key in slot (3 c) % SLOTS: the pick is the largest over slots
        keys[(3 * c) % dc.ARGMAX_SLOTS] = pk[:, c]
    picks = dc.argmax_of_keys(keys).tolist()
    kw, kd = rc.guarded((dc.ARGMAX_SLOTS * M,), torch.int64, SENT, DEV)
    kd.copy_(keys.view(-1))
    N.greedy_pick_keys_ragged(kd, st["ids"], st["row_pos"], rc.PICK_END, st["limit"], st["done"], st["n_done"])
    torch.cuda.synchronize()
    _check_picks(rows, st, picks)
    assert (kd == 0).all(), "the keys of every row, frozen ones included, are reset"
    assert (kw[:rc.GUARD] == SENT).all() and (kw[-rc.GUARD:] == SENT).all()


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("S", [1, 197])
@pytest.mark.parametrize("m", [0, 1, 3])
def test_slot_admit(m, S, fp8):
    g = torch.Generator().manual_seed(m + S)
    L, slots, pool, d2, T, ns = 2, 5, 4, 64, 24, 4
    dt = torch.uint8 if fp8 else torch.bfloat16
    src = torch.randint(0, 255, (L, pool * S, d2), generator=g).to(dt) if fp8 else \
        torch.randn(L, pool * S, d2, generator=g).to(dt)
    pool_kv = src.to(DEV)
    kw, kv = rc.guarded((L, slots * S, d2), dt, 7, DEV)
    pool_scale = scale = sw = None
    if fp8:
        pool_scale = torch.randn(L, pool, ns, generator=g).to(DEV)
        sw, scale = rc.guarded((L, slots, ns), torch.float32, SENT, DEV)
    iw, ids = rc.guarded((slots, T), torch.int64, SENT, DEV)
    row_pos = torch.full((slots,), 9, dtype=torch.int64, device=DEV)
    done = torch.ones(slots, dtype=torch.int32, device=DEV)
    limit = torch.ones(slots, dtype=torch.int64, device=DEV)
    n_done = torch.tensor([5], dtype=torch.int32, device=DEV)
    all_triples = [(4, 0, 7), (0, 3, 24), (2, 1, 2)][:m]
    tr = torch.tensor(all_triples + [(1, 1, 1)] * (slots - m), dtype=torch.int64, device=DEV)   # rows >= m: not read
    N.slot_admit(tr, m, pool_kv, kv, S, pool_scale, scale, ids, 2, row_pos, done, limit, n_done)
    torch.cuda.synchronize()
    want_kv = torch.full((L, slots, S, d2), 7, dtype=dt)
    want_ids = torch.full((slots, T), SENT, dtype=torch.int64)
    want_pos, want_done, want_lim = [9] * slots, [1] * slots, [1] * slots
    want_scale = torch.full((L, slots, ns), float(SENT))
    for s, e, cap in all_triples:
        want_kv[:, s] = src.view(L, pool, S, d2)[:, e]
        want_ids[s, 0] = 2
        want_pos[s], want_done[s], want_lim[s] = 0, 0, cap
        if fp8:
            want_scale[:, s] = pool_scale[:, e].cpu()
    assert _same(kv.view(L, slots, S, d2), want_kv), "named slots are the pool rows bit for bit, all others unchanged"
    assert (kw[:rc.GUARD] == 7).all() and (kw[-rc.GUARD:] == 7).all()
    assert torch.equal(ids.cpu(), want_ids) and (iw[:rc.GUARD] == SENT).all() and (iw[-rc.GUARD:] == SENT).all()
    assert row_pos.tolist() == want_pos and done.tolist() == want_done and limit.tolist() == want_lim
    assert int(n_done) == 5 - m
    assert _same(pool_kv, src)
    if fp8:
        assert _same(scale, want_scale) and (sw[:rc.GUARD] == SENT).all() and (sw[-rc.GUARD:] == SENT).all()


def test_ragged_store_and_admission_are_recordable():
    """MIT_RECORD: a recorded mit_kv_store_ragged replays on the positions of the replay, and a recorded
    mit_slot_admit replays on the triples the device holds at the replay. (The whole recorded step, with the ragged
    embed, attention and picks, is replayed by every plan-launch case of tests/test_rolling_gpu.py.)"""
    B, d = 3, 16
    rp = torch.tensor([0, 2, 1], dtype=torch.int64, device=DEV)
    src = torch.randn(B, d, device=DEV)
    cache = torch.zeros(B, 4, d, device=DEV)
    prog = N.record(lambda: N.kv_store_ragged(src, d, cache, d, 4 * d, B, d, rp))
    assert prog.launches() == 1
    cache.zero_()
    rp.copy_(torch.tensor([3, 0, 2]))
    prog.run()
    torch.cuda.synchronize()
    for b, p in enumerate((3, 0, 2)):
        assert torch.equal(cache[b, p], src[b]) and int((cache[b] != 0).any(-1).sum()) == 1
    # an admission: recorded with triple (1, 0, 5), replayed with (0, 1, 7) in the same device buffer
    L, S, d2, T = 2, 3, 8, 6
    pool_kv = torch.randn(L, 2 * S, d2, device=DEV).to(torch.bfloat16)
    kv = torch.zeros(L, 2 * S, d2, device=DEV, dtype=torch.bfloat16)
    ids = torch.full((2, T), SENT, dtype=torch.int64, device=DEV)
    row_pos = torch.full((2,), 4, dtype=torch.int64, device=DEV)
    done = torch.ones(2, dtype=torch.int32, device=DEV)
    limit = torch.ones(2, dtype=torch.int64, device=DEV)
    n_done = torch.tensor([2], dtype=torch.int32, device=DEV)
    tr = torch.tensor([[1, 0, 5]], dtype=torch.int64, device=DEV)
    prog = N.record(lambda: N.slot_admit(tr, 1, pool_kv, kv, S, None, None, ids, 2, row_pos, done, limit, n_done))
    assert prog.launches() == 1
    torch.cuda.synchronize()
    assert torch.equal(kv[:, S:], pool_kv[:, :S]) and done.tolist() == [1, 0] and int(n_done) == 1
    tr.copy_(torch.tensor([[0, 1, 7]]))
    prog.run()
    torch.cuda.synchronize()
    assert torch.equal(kv[:, :S], pool_kv[:, S:]) and torch.equal(kv[:, S:], pool_kv[:, :S])
    assert done.tolist() == [0, 0] and limit.tolist() == [7, 5] and row_pos.tolist() == [0, 0] and int(n_done) == 0
    assert ids[:, 0].tolist() == [2, 2] and (ids[:, 1:] == SENT).all()
