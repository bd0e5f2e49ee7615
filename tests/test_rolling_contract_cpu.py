"""Rolling-batch captioning without a GPU (tests/rolling_contract.py): the oracle precondition of the end-to-end GPU
test, the pure-Python scheduler against scripted lengths and the brute-force simulation, the ragged attention's plan
query against the scalar-pos one over decode_contract's argument table, and the argument rejections of every new entry
point (the library loads and validates without a GPU, as in tests/test_decode_contract_cpu.py)."""
import ctypes

import pytest
import torch

import decode_contract as dc
import fixtures as FX
import native as N
import rolling_contract as rc
from rolling import CHECK_EVERY_DEFAULT, RollingScheduler


def test_oracle_pins_the_end_to_end_ids():
    """The precondition of test_rolling_gpu's fp32 case: the oracle's greedy ids of the 20 images produce END = 69
    first at END_FIRST (nine distinct lengths, two images never), and every top-1 / top-2 margin exceeds 2 TAU."""
    ids, margin = rc.oracle(FX)
    assert len(ids) == 20 and all(len(r) == rc.MAX_LEN and r[0] == rc.START for r in ids)
    first = [r.index(rc.END, 1) if rc.END in r[1:] else -1 for r in ids]
    assert first == rc.END_FIRST
    assert len(set(rc.e2e_lengths())) == 9 and rc.END_FIRST.count(-1) == 2
    assert margin > rc.TAU2, margin
    assert [len(rc.cut(r, rc.END)) for r in ids] == rc.e2e_lengths()


LENGTHS = {
    "e2e": rc.e2e_lengths(),
    "equal": [7] * 11,
    "ones": [1] * 9,
    "few": [5, 2, 9],
    "none": [],
    "mixed-ones": [1, 4, 1, 1, 24, 2, 1, 3],
}


def test_scheduler_against_the_simulation():
    """Every (lengths, slots, check_every) of LENGTHS x SLOTS x {1, 3, 8}. drive() asserts the invariants (admitted exactly
    once, only into slots seen done, harvest before reuse, complete output, pool entries not overwritten); here: no more
    token steps than the brute-force simulation, the same completion order as it, and for slots >= N exactly static
    batching's steps."""
    for name in LENGTHS:
        for slots in rc.SLOTS:
            for check_every in (1, 3, 8):
                try:
                    _scheduler_case(LENGTHS[name], slots, check_every)
                except AssertionError as e:
                    raise AssertionError(f"lengths {name}, slots {slots}, check_every {check_every}: {e}") from e


def _scheduler_case(lengths, slots, check_every):
    sch = RollingScheduler(slots, check_every)
    out = rc.drive(sch, lengths, caps=[max(n, 1) if n == 1 else rc.MAX_LEN for n in lengths])
    steps, order = rc.simulate(lengths, slots, check_every)
    assert out["steps"] <= steps, (out["steps"], steps)
    slotted = [i for i, n in enumerate(lengths) if n > 1]   # cap-1 images complete as their chunk arrives
    assert [i for i in out["order"] if i in slotted] == [i for i in order if i in slotted]
    if slots >= len(lengths):
        assert out["steps"] == rc.static_steps(lengths, slots, check_every, rc.MAX_LEN) if lengths else out["steps"] == 0
    if not lengths:
        assert out["polls"] == 0 and out["admits"] == 0


def test_scheduler_pool_regions():
    """Encoder chunks smaller than the slots and pools of one or several regions: the same invariants, and never more
    steps than the simulation (a free slot never waits a poll for an image the source still has)."""
    lengths = rc.e2e_lengths()
    for encode_batch, pool in ((1, 1), (2, 4), (3, 3), (5, 10), (32, 32)):
        for slots in (1, 4, 7):
            sch = RollingScheduler(slots, 3, encode_batch, pool)
            out = rc.drive(sch, lengths, max_len=rc.MAX_LEN)
            assert out["steps"] <= rc.simulate(lengths, slots, 3)[0], (encode_batch, pool, slots)
            assert out["chunks"] == -(-len(lengths) // encode_batch)


def test_scheduler_caps():
    """Per-image caps: a cap of 1 takes no slot and completes at once; a cap below the length ends the row there; the
    last group of steps is no longer than the longest remaining cap."""
    lengths = [24] * 20
    caps = [(7 * i) % 19 + 1 for i in range(20)]
    assert 1 in caps
    sch = RollingScheduler(4, 3)
    out = rc.drive(sch, lengths, caps=caps)
    assert out["steps"] <= rc.simulate([min(a, b) for a, b in zip(lengths, caps)], 4, 3)[0]
    assert out["order"][0] == caps.index(1)
    one = RollingScheduler(32, 8)
    assert rc.drive(one, lengths, caps=caps)["steps"] == max(caps) - 1


def test_scheduler_rejects():
    for kw in (dict(slots=0), dict(slots=-3), dict(slots=4, check_every=0), dict(slots=4, encode_batch=0),
               dict(slots=4, encode_batch=3, pool=4), dict(slots=4, encode_batch=4, pool=2)):
        with pytest.raises(ValueError):
            RollingScheduler(**kw)
    sch = RollingScheduler(2)
    assert sch.check_every == CHECK_EVERY_DEFAULT and sch.pool == 2 and sch.encode_batch == 2
    with pytest.raises(ValueError):
        sch.add_chunk([3, 0])
    with pytest.raises(ValueError):
        sch.add_chunk([3, 3, 3])
    sch.add_chunk([3, 3])
    with pytest.raises(RuntimeError):
        sch.add_chunk([3])


def test_scheduler_module_needs_no_torch():
    import rolling
    src = open(rolling.__file__).read()
    assert "import torch" not in src and "import native" not in src


# ------------------------------------------------------------------------------------------------
# the C ABI without a GPU
# ------------------------------------------------------------------------------------------------
def test_ragged_plan_is_the_scalar_plan():
    """Over every attention case of decode_contract's table: its geometry, strides and Lk argument (attn_geom), a
    position and key tokens where the case has them. The queries dereference nothing, so the addresses are made up
    (16-B aligned bases plus the case's element offsets, as decode_contract.attn_plan_args forms them)."""
    cases = [c for c in dc.CASES if c.op == "attn"]
    assert len(cases) > 100
    for c in cases:
        G = dc.attn_geom(c)
        esz = 2 if c.dtype == "bf16" else 4
        q, kv, o, pos, tok = 1 << 20, 2 << 20, 3 << 20, (4 << 20) if c.use_pos else None, \
            (5 << 20) if c.mask != "none" else None
        args = (N.BF16 if c.dtype == "bf16" else N.F32, c.B, c.H, c.Dh, q + G["q_off"] * esz, G["q_batch"],
                kv + G["k_off"] * esz, G["row"], G["kv_batch"], kv + G["v_off"] * esz, G["row"], G["kv_batch"], o,
                G["o_batch"])
        want = N.attention_decode_plan(*args, Lk=G["lk_arg"], pos=pos, key_tokens=tok)
        got = N.attention_decode_ragged_plan(*args, Lk=G["lk_arg"], row_pos=pos, key_tokens=tok)
        assert got == want == dc.FAMILY[c.family], c.id


def test_ragged_plan_rejects_what_the_scalar_plan_rejects():
    buf = torch.zeros(4096, dtype=torch.float32)
    p = buf.data_ptr() + (-buf.data_ptr()) % 16
    good = dict(dtype=N.BF16, B=2, H=8, Dh=64, q=p, q_batch=512, k=p, k_row=1024, k_batch=8192, v=p, v_row=1024,
                v_batch=8192, o=p, o_batch=512)
    for kw in (dict(Dh=48), dict(dtype=5), dict(q=None), dict(q=p + 2), dict(k_row=1021), dict(o_batch=5)):
        a = dict(good, **kw)
        for fn, pk in ((N.attention_decode_plan, "pos"), (N.attention_decode_ragged_plan, "row_pos")):
            assert fn(*a.values(), Lk=0, **{pk: p}) == -1, (kw, fn.__name__)
    assert N.attention_decode_ragged_plan(*good.values(), Lk=0, row_pos=None) == -1   # neither a position nor Lk
    assert N.attention_decode_ragged_plan(*good.values(), Lk=0, row_pos=p) == N.DECODE_ATTN_ROWS


def _aligned(n=1 << 16):
    buf = ctypes.create_string_buffer(n + 64)
    return buf, ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16


def test_new_entry_points_reject_bad_arguments_without_launching():
    """Every new entry point returns MIT_ERR_INVALID (1) with a message for arguments its contract excludes; the
    checks run before any HIP call, so this needs no GPU."""
    lib = N.load_library()
    _keep, p = _aligned()

    def rejected(rc_, frag):
        assert rc_ == 1 and frag in lib.mit_last_error(), (rc_, lib.mit_last_error())
    att = [N.BF16, 2, 8, 64, p, 512, p, 1024, 8192, p, 1024, 8192, p, 512, 0, p, p, 100, 0, 0.125, None]
    for i, v, frag in ((4, None, b"null pointer"), (3, 48, b"head_dim"), (0, 9, b"bad dtype"), (15, None, b"position"),
                       (4, p + 2, b"aligned"), (7, 1021, b"aligned")):
        a = list(att)
        a[i] = v
        rejected(lib.mit_attention_decode_ragged(*a), frag)
    rejected(lib.mit_kv_store_ragged(N.BF16, 2, 8, p, 8, p, 8, 64, None, None), b"null pointer")
    rejected(lib.mit_kv_store_ragged(N.BF16, 2, 8, None, 8, p, 8, 64, p, None), b"null pointer")
    rejected(lib.mit_embed_decode_ragged(N.BF16, 2, 8, p, 6, None, p, 1.0, p, p, None), b"null pointer")
    rejected(lib.mit_embed_decode_ragged(N.BF16, 2, 8, p, 6, p, p, 1.0, None, p, None), b"null pointer")
    pick = [2, 8, p, 8, p, 6, p, 5, p, p, p, None]
    for i, v in ((2, None), (6, None), (8, None), (9, None), (10, None), (3, 7), (1, 0), (5, 0)):
        a = list(pick)
        a[i] = v
        rejected(lib.mit_greedy_pick_ragged(*a), b"bad arguments")
    keys = [2, p, p, 6, p, 5, p, p, p, None]
    for i, v, frag in ((1, None, b"bad arguments"), (4, None, b"bad arguments"), (6, None, b"bad arguments"),
                       (3, 0, b"bad arguments"), (0, 0, b"B = 0"), (0, 1 << 30, b"B =")):
        a = list(keys)
        a[i] = v
        rejected(lib.mit_greedy_pick_keys_ragged(*a), frag)
    adm = [2, p, 2, 197, 768, p, 4, p, 5, None, None, 0, p, 24, 2, p, p, p, p, None]
    for i, v, frag in ((0, -1, b"m = -1"), (1, None, b"null pointer"), (5, None, b"null pointer"),
                       (19 - 1, None, b"null pointer"), (2, 0, b"bad extents"), (3, 0, b"bad extents"),
                       (13, 0, b"bad extents"), (0, 6, b"exceeds the slots"), (4, 770, b"16-B aligned"),
                       (7, p + 8, b"16-B aligned"), (9, p, b"go together"), (10, p, b"go together")):
        a = list(adm)
        a[i] = v
        rejected(lib.mit_slot_admit(*a), frag)
    a = list(adm)
    a[9], a[10] = p, p
    rejected(lib.mit_slot_admit(*a), b"n_scale > 0")
    # m = 0 is a no-op whatever else is passed: nothing is launched, nothing is dereferenced
    a = list(adm)
    a[0] = 0
    a[1] = a[5] = a[7] = None
    assert lib.mit_slot_admit(*a) == 0
    for name in ("mit_attention_decode_ragged", "mit_attention_decode_ragged_plan", "mit_kv_store_ragged",
                 "mit_embed_decode_ragged", "mit_greedy_pick_ragged", "mit_greedy_pick_keys_ragged", "mit_slot_admit"):
        assert name in N.SIGNATURES and hasattr(N.load_library(), name)
