"""Sampled / constrained rolling-batch captioning without a GPU (tests/stream_contract.py): RollingScheduler(samples=N)
against scripted lengths and the brute-force simulation, the argument rejections of the three new entry points (the
library loads and validates without a GPU), the references of the kernel cases, and the host surface over a stub
model: generate_captions(stream_slots=...) and the command line."""
import numpy as np
import pytest
import torch

import native as N
import rolling_contract as rc
import sample_contract as sc
import stream_contract as st
from rolling import RollingScheduler


# ------------------------------------------------------------------------------------------------
# the scheduler with several samples per image
# ------------------------------------------------------------------------------------------------
def _lengths(B, samples, seed):
    g = torch.Generator().manual_seed(seed)
    return [[int(x) for x in torch.randint(2, rc.MAX_LEN + 1, (samples,), generator=g)] for _ in range(B)]


@pytest.mark.parametrize("samples", [1, 2, 3, 5])
def test_scheduler_samples_against_the_simulation(samples):
    """drive_samples asserts the invariants (every (image, sample) admitted exactly once, only into a slot seen done,
    a pool entry not overwritten before all its samples got a slot, harvest before reuse, complete output); here: no
    more token steps than the brute-force simulation over the items in row-id order, and its completion order."""
    for B in (0, 1, 7, 20):
        lengths = _lengths(B, samples, 100 * samples + B)
        for slots in (1, 3, 4, 32):
            for check_every in (1, 3, 8):
                for encode_batch, pool in ((None, None), (2, 4), (3, 3)):
                    sch = RollingScheduler(slots, check_every, encode_batch, pool, samples=samples)
                    out = st.drive_samples(sch, lengths, [rc.MAX_LEN] * B)
                    steps, order = rc.simulate(st.flat(lengths), slots, check_every)
                    tag = (samples, B, slots, check_every, encode_batch, pool)
                    assert out["steps"] <= steps, tag
                    if encode_batch is None:   # the whole pool in one region: nothing ever waits for the encoder
                        assert out["order"] == order, tag
                    assert out["chunks"] == -(-B // sch.encode_batch), tag


def test_scheduler_samples_caps_and_row_ids():
    """Caps per IMAGE: a cap of 1 completes all the image's samples at once and takes no slot; records name the row id
    image * samples + n and the image's one pool entry."""
    samples, B = 3, 20
    caps = [(7 * i) % 19 + 1 for i in range(B)]
    lengths = [[rc.MAX_LEN] * samples for _ in range(B)]
    sch = RollingScheduler(4, 3, samples=samples)
    out = st.drive_samples(sch, lengths, caps)
    assert caps.index(1) == 0 and out["order"][:samples] == list(range(samples))
    assert out["steps"] <= rc.simulate([c for c in caps for _ in range(samples)], 4, 3)[0]
    sch = RollingScheduler(4, samples=2)
    at, trivial = sch.add_chunk([5, 1, 7])
    assert at == 0 and trivial == [1]
    assert sch.admissions_ex() == [(0, 0, 5, 0), (1, 0, 5, 1), (2, 2, 7, 4), (3, 2, 7, 5)]
    assert sch.region_left == [0] and sch.admissions() == []


def test_scheduler_samples_one_is_the_scheduler_as_it_was():
    lengths = rc.e2e_lengths()
    for slots in rc.SLOTS:
        a, b = RollingScheduler(slots, 3), RollingScheduler(slots, 3, samples=1)
        oa = rc.drive(a, lengths, max_len=rc.MAX_LEN)
        ob = rc.drive(b, lengths, max_len=rc.MAX_LEN)
        assert oa == ob
    with pytest.raises(ValueError):
        RollingScheduler(4, samples=0)


# ------------------------------------------------------------------------------------------------
# the C ABI without a GPU
# ------------------------------------------------------------------------------------------------
def test_new_entry_points_reject_bad_arguments_without_launching():
    """MIT_ERR_INVALID (1) with a message for what the contracts exclude; the checks run before any HIP call."""
    lib = N.load_library()
    _keep, p = st.aligned_buffer()

    def rejected(rc_, frag):
        assert rc_ == 1 and frag in lib.mit_last_error(), (rc_, lib.mit_last_error())
    # R, V, logits, ld, tok, ld_tok, row_pos, done, penalty, ngram, min_length, end, suppress, n_suppress, forced,
    # ld_forced, n_forced, prompt_idx, stream
    con = [2, 8, p, 8, p, 24, p, p, 1.2, 2, 0, 5, p, 1, p, 4, 3, p, None]
    for i, v, frag in ((2, None, b"null pointer"), (4, None, b"null pointer"), (6, None, b"null pointer"),
                       (8, 0.0, b"repetition_penalty"), (8, float("inf"), b"repetition_penalty"),
                       (9, -1, b"no_repeat_ngram"), (10, -1, b"min_length"), (13, -1, b"n_suppress"),
                       (12, None, b"null suppress"), (1, 0, b"vocabulary"), (3, 7, b"ld 7 < V"), (5, 0, b"ld_tok"),
                       (5, 4097, b"ld_tok"), (15, 0, b"prompt table"), (16, 0, b"prompt table"), (2, p + 2, b"aligned"),
                       (0, -1, b"bad row count")):
        a = list(con)
        a[i] = v
        rejected(lib.mit_logits_constrain_ragged(*a), frag)
    a = list(con)
    a[0] = 0                                      # no rows: nothing is launched
    assert lib.mit_logits_constrain_ragged(*a) == 0
    # R, V, logits, ld, temperature, top_k, top_p, seed, row_id, uniforms, ids, ld_ids, row_pos, end, limit, done,
    # n_done, logprob, length, stream
    pick = [2, 8, p, 8, 1.0, 0, 1.0, p, p, None, p, 6, p, 5, p, p, p, p, p, None]
    for i, v, frag in ((4, 0.0, b"temperature"), (6, 0.0, b"top_p"), (5, -1, b"top_k"), (1, 0, b"vocabulary"),
                       (3, 7, b"ld 7 < V"), (11, 1, b"two columns"), (2, None, b"null pointer"),
                       (10, None, b"null pointer"), (12, None, b"null pointer"), (14, None, b"null pointer"),
                       (15, None, b"null pointer"), (16, None, b"null pointer"), (8, None, b"neither uniforms nor row_id"),
                       (2, p + 2, b"aligned"), (0, -1, b"bad row count")):
        a = list(pick)
        a[i] = v
        rejected(lib.mit_sample_pick_ragged(*a), frag)
    a = list(pick)
    a[0] = 0
    assert lib.mit_sample_pick_ragged(*a) == 0
    adm = [2, p, 2, 3, 32, p, 4, p, 5, None, None, 0, p, 24, 2, p, p, p, p, p, p, p, p, None]
    for i, v, frag in ((0, -1, b"m = -1"), (1, None, b"null pointer"), (5, None, b"null pointer"),
                       (19, None, b"null pointer"), (20, None, b"null pointer"), (21, None, b"null pointer"),
                       (22, None, b"null pointer"), (2, 0, b"bad extents"), (13, 0, b"bad extents"),
                       (0, 6, b"exceeds the slots"), (4, 40, b"16-B aligned"), (7, p + 8, b"16-B aligned"),
                       (9, p, b"go together"), (10, p, b"go together")):
        a = list(adm)
        a[i] = v
        rejected(lib.mit_slot_admit_ex(*a), frag)
    a = list(adm)
    a[0] = 0
    a[1] = a[5] = a[7] = a[19] = None             # m = 0 is a no-op whatever else is passed
    assert lib.mit_slot_admit_ex(*a) == 0
    for name in ("mit_logits_constrain_ragged", "mit_sample_pick_ragged", "mit_slot_admit_ex"):
        assert name in N.SIGNATURES and hasattr(lib, name)
    assert N.ABI_VERSION == lib.mit_abi_version()


def test_kernel_case_builders():
    """The cases of tests/test_stream_contract_gpu.py hold what their docstrings promise (no GPU involved)."""
    t = st.make_constrain(509)
    assert [w is None for w in t["want"]] == [bool(d) for d in st.CON_DONE] and st.CON_DONE.count(1) == 2
    assert torch.isnan(t["logits"][3]).all() and not torch.isnan(t["logits"][4]).any()
    forced_rows = [r for r, w in enumerate(t["want"]) if w is not None and np.isinf(w).sum() == 508]
    assert forced_rows == [0, 1]
    assert -1 in st.CON_PROMPT_IDX and sorted(st.CON_PROMPT_LEN)[:2] == [0, 1] and st.CON_LD_FORCED - 1 in st.CON_PROMPT_LEN
    assert {p + 1 < st.CON_NGRAM for p in st.CON_POS} == {True, False} and st.CON_NGRAM - 1 in st.CON_POS
    assert max(st.CON_POS) > 256 and max(st.CON_POS) < st.CON_LD_TOK
    # the sampled pick: one V per instantiation of the kernel, the state rows of the ragged picks
    keys = [((v + 3) // 4) * 4 for v in st.PICK_V]
    assert keys[0] <= 1024 < keys[1] <= 10240 < keys[2] <= 12288 < keys[3]
    assert st.PICK_STATES == [(0, 1, 6), (0, 2, 4), (0, 3, 5), (1, 2, 6), (0, 4, 6), (0, 0, 6)]
    for hashed in (False, True):
        t = st.make_sample_pick(509, hashed)
        toks = [r["token"] if r is not None else None for r in t["refs"]]
        assert [k == rc.PICK_END for k in toks] == st.PICK_DRAWS_END and toks[3] is None
        assert all(min(r["margin_u"], r["margin_p"]) >= 2 * sc.TAU_U for r in t["refs"] if r is not None)
    assert len(set(st.PICK_ROW_ID)) == 6 and max(st.PICK_ROW_ID) > 1 << 20


# ------------------------------------------------------------------------------------------------
# generate_captions / command line over a stub model
# ------------------------------------------------------------------------------------------------
class _Stub:
    device = "cpu"

    def __init__(self):
        self.calls = []

    def generate_stream_iter(self, batches, start, end, **kw):
        chunks = [b.shape[0] for b in batches]
        self.calls.append(("stream", chunks, kw))
        n = sum(chunks)
        return iter([(i, 0, [start, 20 + i, end], None if kw["temperature"] is None else -1.5)
                     for i in reversed(range(n))])                      # completion order: any

    def generate_batch(self, chunk, start, end, **kw):
        self.calls.append(("greedy", chunk.shape[0], kw))
        return [[start, 7, end]] * chunk.shape[0]


def test_generate_captions_routes_stream_slots():
    import inference
    imgs = torch.zeros(5, 3, 4, 4)
    m = _Stub()
    prompts = [[4], [], [5, 6], [], [7]]
    out = inference.generate_captions(m, imgs, start_token_id=2, end_token_id=3, max_len=9, batch_size=2, stream_slots=3,
                                      temperature=0.7, top_k=5, top_p=0.9, seed=11, repetition_penalty=1.2,
                                      no_repeat_ngram_size=2, min_length=1, suppress_tokens=[8], prompts=prompts,
                                      kv_dtype="fp8")
    assert [p for p, _ in out] == [[20 + i] for i in range(5)]           # input order, START / END stripped
    (kind, chunks, kw), = m.calls
    assert kind == "stream" and chunks == [2, 2, 1]
    assert kw == dict(max_len=9, slots=3, encode_batch=2, temperature=0.7, top_k=5, top_p=0.9, seed=11,
                      repetition_penalty=1.2, no_repeat_ngram_size=2, min_length=1, suppress_tokens=(8,),
                      prompts=prompts, kv_dtype="fp8")
    m = _Stub()
    inference.generate_captions(m, imgs, start_token_id=2, end_token_id=3, max_len=9, stream_slots=4)
    (kind, chunks, kw), = m.calls
    assert kind == "stream" and kw["temperature"] is None and "kv_dtype" not in kw and kw["slots"] == 4
    for bad in (dict(beam_size=3), dict(rolling_slots=4)):
        with pytest.raises(ValueError, match="stream_slots"):
            inference.generate_captions(m, imgs, stream_slots=4, **bad)
    m = _Stub()
    inference.generate_captions(m, imgs, start_token_id=2, end_token_id=3, max_len=9)     # without it: as before
    assert m.calls[0][0] == "greedy"


def test_command_line_flags():
    import inference
    ap = inference.build_parser()
    base = ["--image_path", "a.png", "--checkpoint_path", "c.pt"]
    assert "stream_slots" not in inference.decode_options(ap.parse_args(base))
    o = inference.decode_options(ap.parse_args(base + ["--stream_slots", "16", "--temperature", "0.7", "--min_length",
                                                       "3", "--prompt_ids", "5", "6"]))
    assert o["stream_slots"] == 16 and o["temperature"] == 0.7 and o["min_length"] == 3 and o["prompts"] == [5, 6]
    assert "rolling_slots" not in o
    m = _Stub()
    inference.generate_captions(m, torch.zeros(2, 3, 4, 4), **o)            # the options are generate_captions keywords
    assert m.calls[0][0] == "stream" and m.calls[0][2]["slots"] == 16 and m.calls[0][2]["prompts"] == [5, 6]
    for flags in (["--beam_size", "3"], ["--rolling_slots", "4"]):
        with pytest.raises(SystemExit):
            inference.main(base + ["--stream_slots", "4"] + flags)


def test_stream_iter_rejects_before_anything_runs():
    """The call itself raises (it is not a generator function): checked on an object with no GPU state at all."""
    import model as M

    class _Dec:
        V = 100
        pe = torch.zeros(30, 4)

    class _Fake:
        decoder, dtype = _Dec(), torch.float32
    f = M.ImageToTextModel.generate_stream_iter
    for kw in (dict(beam_size=2), dict(method="beam"), dict(streams=2), dict(temperature=0.0), dict(num_samples=2),
               dict(temperature=1.0, num_samples=0), dict(temperature=1.0, top_p=0.0), dict(temperature=1.0, top_k=-2),
               dict(kv_dtype="fp8"), dict(slots=0), dict(max_lens=[0]), dict(max_len=31), dict(suppress_tokens=(100,)),
               dict(prompts=[3]), dict(repetition_penalty=-1.0)):
        with pytest.raises(ValueError):
            f(_Fake(), [], 2, 3, **{"max_len": 24, **kw})
