"""Beam search without a GPU: the C ABI's argument checks and host-only queries (mit_beam_select,
mit_beam_select_ws_bytes, mit_attention_decode_beam, mit_attention_decode_beam_plan), the float64 references of
tests/beam_contract.py against the pinned oracle's greedy decode, and the decision margins that let the GPU tests
compare every step of the end-to-end inputs exactly."""
import math

import pytest
import torch

import beam_contract as bc
import decode_contract as dc
import fixtures as FX
import native as N
from oracle import ref_cpu

BF16, F32 = N.BF16, N.F32


@pytest.fixture(scope="module")
def lib():
    return N.load_library()


def _err(lib):
    return (lib.mit_last_error() or b"").decode()


# ------------------------------------------------------------------------------------------------
# argument rejection: nothing is launched, no pointer dereferenced (the addresses are made up)
# ------------------------------------------------------------------------------------------------
def _select(lib, B=2, K=3, V=16, logits=0x1000, ld=16, score=0x2000, tok=0x3000, ld_tok=8, anc=0x4000, ld_anc=8,
            pos=0x5000, finished=0x6000, length=0x7000, n_finished=0x8000, ws=0x9000, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = max(lib.mit_beam_select_ws_bytes(B, min(max(K, 1), 8), V), 0)
    return lib.mit_beam_select(B, K, V, logits, ld, score, tok, ld_tok, anc, ld_anc, pos, 1, 0, finished, length,
                               n_finished, ws, ws_bytes, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(K=0), "outside 1..8"), (dict(K=9, V=64, ld=64), "outside 1..8"), (dict(K=-1), "outside 1..8"),
    (dict(K=4, V=3, ld=8), "must hold K"), (dict(V=16, ld=15), "ld 15 < V 16"),
    (dict(logits=None), "null"), (dict(score=None), "null"), (dict(tok=None), "null"), (dict(anc=None), "null"),
    (dict(pos=None), "null"), (dict(finished=None), "null"), (dict(length=None), "null"),
    (dict(n_finished=None), "null"), (dict(ws=None), "null"),
    (dict(ws_bytes=8), "workspace"), (dict(ws=0x9004), "aligned"), (dict(logits=0x1002), "aligned"),
    (dict(ld_tok=1), "two columns"), (dict(ld_anc=0), "two columns"),
])
def test_select_rejects(lib, kw, msg):
    assert _select(lib, **kw) == 1
    assert msg in _err(lib), _err(lib)


def test_select_ws_bytes(lib):
    assert lib.mit_beam_select_ws_bytes(2, 0, 16) == -1 and lib.mit_beam_select_ws_bytes(2, 9, 16) == -1
    assert lib.mit_beam_select_ws_bytes(-1, 3, 16) == -1
    sizes = {(B, K): lib.mit_beam_select_ws_bytes(B, K, 10000) for B in (0, 1, 256) for K in (1, 3, 8)}
    for (B, K), n in sizes.items():
        assert n >= 8 * B * K * K and n % 8 == 0     # the rows' K best (score, token) pairs
    assert sizes[(256, 3)] < 256 * 3 * 10000          # nothing of the vocabulary's size
    assert lib.mit_beam_select_ws_bytes(4, 3, 7) == lib.mit_beam_select_ws_bytes(4, 3, 10000)
    # one byte short is rejected, the exact size passes the check (B = 0 launches nothing: no GPU needed)
    assert _select(lib, B=0) == 0


def _attn(lib, fn="mit_attention_decode_beam_plan", dtype=F32, R=6, H=3, Dh=64, q=0x10000, q_batch=576, k=0x20000,
          k_row=384, k_batch=384 * 40, v=0x20300, v_row=384, v_batch=384 * 40, o=0x30000, o_batch=192, Lk=0,
          pos=0x40000, group=3, anc=0x50000, ld_anc=40, tok=0x60000):
    if fn.endswith("_plan"):
        return lib.mit_attention_decode_beam_plan(dtype, R, H, Dh, q, q_batch, k, k_row, k_batch, v, v_row, v_batch, o,
                                                  o_batch, Lk, pos, group, anc, ld_anc, tok)
    return lib.mit_attention_decode_beam(dtype, R, H, Dh, q, q_batch, k, k_row, k_batch, v, v_row, v_batch, o, o_batch,
                                         Lk, pos, group, anc, ld_anc, tok, 40, 0, 0.125, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(q=None), "null"), (dict(k=None), "null"), (dict(v=None), "null"), (dict(o=None), "null"),
    (dict(Dh=48), "head_dim"), (dict(dtype=7), "dtype"), (dict(pos=None, Lk=0), "position"),
    (dict(group=0), "group"), (dict(R=7), "whole groups"), (dict(ld_anc=0), "ancestor"), (dict(anc=0x50002), "ancestor"),
    (dict(q=0x10004), "16-B"), (dict(k_row=386), "16-B"), (dict(v_batch=384 * 40 + 2), "16-B"), (dict(o_batch=194), "16-B"),
    (dict(dtype=BF16, q_batch=580), "16-B"),
])
def test_attention_rejects(lib, kw, msg):
    assert _attn(lib, **kw) == -1
    assert msg in _err(lib), _err(lib)
    assert _attn(lib, fn="mit_attention_decode_beam", **kw) == 1      # the entry point: same decision, nothing launched


def test_attention_plan(lib):
    # gathered or shared K/V: the block-per-(row, head) family, whatever the shape
    assert _attn(lib) == dc.ATTN_BH
    assert _attn(lib, dtype=BF16, H=8, q_batch=1536, o_batch=512, k_row=1024, v_row=1024, k_batch=1024 * 40,
                 v_batch=1024 * 40) == dc.ATTN_BH
    assert _attn(lib, anc=None, pos=None, Lk=197, R=7) == dc.ATTN_BH          # shared cross K/V, ragged last image
    assert _attn(lib, Dh=16, H=12) == dc.ATTN_BH
    # group = 1 without a table IS mit_attention_decode: its plan, argument for argument
    for dtype, H, pos, Lk in [(F32, 3, 0x40000, 0), (BF16, 8, 0x40000, 0), (BF16, 8, None, 197), (BF16, 3, None, 5)]:
        a = dict(dtype=dtype, H=H, q_batch=H * 64 * 3, o_batch=H * 64, k_row=H * 128, v_row=H * 128,
                 k_batch=H * 128 * 40, v_batch=H * 128 * 40, pos=pos, Lk=Lk)
        want = lib.mit_attention_decode_plan(dtype, 6, H, 64, 0x10000, a["q_batch"], 0x20000, a["k_row"], a["k_batch"],
                                             0x20300, a["v_row"], a["v_batch"], 0x30000, a["o_batch"], Lk, pos, None)
        assert want >= 0 and _attn(lib, group=1, anc=None, **a) == want
    assert {dc.ATTN_ROWS, dc.ATTN_ROWS_NT} <= {
        _attn(lib, group=1, anc=None, dtype=BF16, H=8, q_batch=1536, o_batch=512, k_row=1024, v_row=1024,
              k_batch=1024 * 40, v_batch=1024 * 40, pos=p, Lk=7) for p in (0x40000, None)}


# ------------------------------------------------------------------------------------------------
# the references
# ------------------------------------------------------------------------------------------------
def test_select_cases_cover_the_shapes_with_clear_margins():
    seen = set()
    for c in bc.SEL_CASES:
        t = bc.make_select(c)      # asserts: every margin an exact tie or > TAU; the built parent maps come out
        m = t.x["ref"]["margin"]
        assert m == 0 or m > bc.TAU
        seen.add((c.V, c.K, c.B))
    assert {(V, K, B) for V in bc.SEL_V for K in bc.SEL_K for B in bc.SEL_B if K <= V} <= seen
    maps = {c.parents for c in bc.SEL_CASES if c.parents}
    assert maps == {(1, 2, 0), (1, 1, 0), (2, 2, 2)}


def test_select_score_bound_is_four_times_the_emulation():
    worst = max(f for f, _ in bc.emulation_figures().values())
    assert worst <= bc.BOUND_SCORE / 4 * 1.0005, f"float32 emulation figure {worst:.3f}: update BOUND_SCORE"
    assert worst >= bc.BOUND_SCORE / 4 * 0.9, f"BOUND_SCORE is looser than 4 x the emulation's {worst:.3f}"


def test_select_reference_by_hand():
    """K = 2, V = 3: slot 0 live (score -1), slot 1 finished (score -1.5)"""
    lg = torch.tensor([[0.0, math.log(2.0), math.log(5.0)], [float("nan")] * 3], dtype=torch.float64)
    tok = torch.tensor([[9, 4, -1], [9, 5, -1]])
    anc = torch.tensor([[0, 1, -1], [1, 0, -1]], dtype=torch.int32)
    r = bc.select_reference(lg, torch.tensor([-1.0, -1.5]), torch.tensor([0, 1]), torch.tensor([1, 1]), tok, anc, 1, 2,
                            end_id=2, pad_id=0)
    assert r["parent"].tolist() == [0, 1] and r["token"].tolist() == [2, 0]
    assert abs(float(r["score"][0]) - (-1.0 + math.log(5 / 8))) < 1e-12 and float(r["score"][1]) == -1.5
    assert r["finished"].tolist() == [1, 1] and r["length"].tolist() == [2, 1] and r["n_finished"] == 2
    assert r["anc"].tolist() == [[0, 1, 0], [1, 0, 1]] and r["tok"][:, 2].tolist() == [2, 0]
    assert abs(r["margin"] - min(-1.0 + math.log(5 / 8) + 1.5, -1.5 - (-1.0 + math.log(2 / 8)))) < 1e-12


@pytest.mark.parametrize("name", ["tiny_vit_cls", "tiny_vit_patches"])
def test_reference_with_one_beam_is_the_oracles_greedy(name):
    meta, T = FX.load(name)
    st = FX.state(meta)
    enc, dec = FX.enc_desc(meta), FX.dec_desc(meta)
    imgs = FX.inputs(meta, 0)[0][:2]
    for end in (69, 10 ** 6):
        for i in range(imgs.shape[0]):
            pv = imgs[i:i + 1]
            want = ref_cpu.greedy_generate(st, pv, enc, dec, 2, end, max_len=10, mode=meta["mode"])
            with torch.no_grad():
                mem = ref_cpu.memory_from_features(st, ref_cpu.encode(st, pv, enc), meta["mode"])
            got = bc.beam_search_reference(st, mem, dec, 2, end, 1, 10)
            assert got["ids"][0] == want
            assert got["length"][0] == len(want) - 1 and got["finished"][0] == int(want[-1] == end)


@pytest.mark.parametrize("K,end", bc.E2E_CASES)
def test_end_to_end_inputs_have_clear_margins(K, end):
    """No step of the reference decides by less than TAU on the inputs the GPU test compares step by step."""
    refs = bc.e2e_reference(FX, K, end)
    assert len(refs) == 4
    for i, r in enumerate(refs):
        worst = min((s["margin"], j) for j, s in enumerate(r["steps"]))
        print(f"K={K} END={end} image {i}: min margin {worst[0]:.2e} at step {worst[1]}, "
              f"{sum(r['finished'])} of {K} beams finished")
        assert worst[0] > bc.TAU, f"image {i}: margin {worst[0]:.2e} at step {worst[1]}"
    if end == 69:
        assert sum(sum(r["finished"]) for r in refs) >= 8      # END is produced: finished beams take part
    if end == -1:
        assert all(len(r["steps"]) == bc.E2E_MAX_LEN - 1 and not any(r["finished"]) for r in refs)


def test_rank_beams():
    import model
    ids = [[2, 5, 1], [2, 7, 7, 7], [2, 9, 1], [2, 3], [2, 4], [2, 6]]
    sc = [-2.0, -3.0, -2.0, -1.0, -0.5, -0.5]
    ln = [2, 3, 2, 1, 1, 1]
    assert model.rank_beams(ids, sc, ln, 3) == [[2, 5, 1], [2, 4]]                     # ties: the lower slot
    allb = model.rank_beams(ids, sc, ln, 3, return_all=True)
    assert [i for i, _ in allb[0]] == [ids[0], ids[2], ids[1]] and [s for _, s in allb[1]] == [-0.5, -0.5, -1.0]
    assert model.rank_beams(ids, sc, ln, 3, length_penalty=1.0)[0] == [2, 5, 1]        # -1, -1, -1: lower slot
    assert model.rank_beams(ids, sc, ln, 3, length_penalty=2.0)[0] == [2, 7, 7, 7]     # -0.5, -0.33, -0.5
    assert [bc.rank_slots(sc[:3], ln[:3], lp) for lp in (0.0, 2.0)] == [[0, 2, 1], [1, 0, 2]]
