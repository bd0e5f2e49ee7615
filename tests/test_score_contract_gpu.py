"""Caption scoring on the GPU (csrc/score.hip) against tests/score_contract.py: every case through mit_score_rows and
mit_score_sequences (ranks, counts and the sequence sums exact, token_logprob within BOUND_LOGPROB, guards intact, a
second launch bitwise equal), the element-load path against the wide one, and one case recorded and replayed."""
import pytest
import torch

import native as N
import score_contract as sc

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    N.load_library()
    yield
    torch.cuda.empty_cache()


def _run(c, t):
    assert sc.launch_rows(N, c, t) == 0, N.lib().mit_last_error()
    assert sc.launch_sequences(N, c, t) == 0, N.lib().mit_last_error()
    torch.cuda.synchronize()


def _bits(t):
    return {k: a.bits().cpu().clone() for k, a in t.a.items()}


@pytest.mark.parametrize("cid", [c.id for c in sc.CASES])
def test_case(cid):
    """rank, the 0 / -1 of ignored rows, seq_tokens and seq_hits: exact. seq_logprob: bitwise the float32 sequential
    sum of the launch's own token_logprob. token_logprob within BOUND_LOGPROB = 75.3 units of u (|l_t| + |lse|).
    Guards (the logits with their NaN padding and NaN rows, the targets, the bands around every output): bitwise
    untouched. A second launch from restored buffers: bitwise the same."""
    c = sc.BY_ID[cid]
    assert N.score_rows_plan(sc._CODE[c.dtype], c.R, c.V, None, c.ld) == -1
    t = sc.make(c).to(DEV)
    assert N.lib().mit_score_rows_plan(sc._CODE[c.dtype], c.R, c.V, t.ptr("logits"), c.ld) == sc.plan_expected(c.dtype, c.V)
    t.snapshot()
    _run(c, t)
    fig = sc.check(c, t)
    print(f"{cid}: token_logprob figure {fig:.3f} (bound {sc.BOUND_LOGPROB:.2f})")
    assert fig <= sc.BOUND_LOGPROB, f"{cid}: token_logprob off by {fig:.2f} units (bound {sc.BOUND_LOGPROB:.2f})"
    first = _bits(t)
    t.restore()
    _run(c, t)
    for k, bits in _bits(t).items():
        assert torch.equal(bits, first[k]), f"{cid}: {k} differs between two launches"


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_element_loads_give_the_wide_loads_bits(dt):
    """the same rows behind a 16-B aligned base with ld = 512 and behind a base one element off with ld = 509:
    token_logprob and rank agree bit for bit"""
    out = []
    for cid in (f"{dt}-V509-T5-ld512", f"{dt}-V509-T5-mis1"):
        c = sc.BY_ID[cid]
        t = sc.make(c).to(DEV)
        assert (t.ptr("logits") % 16 == 0) == (c.mis == 0)
        _run(c, t)
        out.append((sc.read(t, "tlp", c.R).view(torch.int32), sc.read(t, "rank", c.R)))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


def test_more_rows_than_one_launch_takes():
    """R = 2^22 + 3 rows of V = 2 (mit_score_rows launches at most 2^22 rows at a time): every row against a
    vectorised float64 reference, ignored NaN rows on both sides of the seam included"""
    R, V = (1 << 22) + 3, 2
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(R, V, generator=g) * 3).to(torch.bfloat16)
    x[::11, 1] = x[::11, 0]                                              # exact ties
    tg = torch.randint(0, V, (R,), generator=g)
    ign = torch.zeros(R, dtype=torch.bool)
    ign[2::5] = True
    ign[(1 << 22) - 1], ign[(1 << 22) + 1] = True, True
    tg[ign] = -100
    x[ign] = float("nan")
    xd, td = x.to(DEV), tg.to(DEV)
    tlp = torch.full((R,), sc.SENT_F, dtype=torch.float32, device=DEV)
    rank = torch.full((R,), sc.SENT_I, dtype=torch.int32, device=DEV)
    N.score_rows(xd, td, -100, tlp, rank, V=V)
    torch.cuda.synchronize()
    x64, t = x.double(), tg.clamp(min=0)
    lt, lo = x64.gather(1, t[:, None])[:, 0], x64.gather(1, 1 - t[:, None])[:, 0]
    lse = torch.logsumexp(x64, 1)
    want_rank = ((lo > lt) | ((lo == lt) & (t == 1))).int()
    live = ~ign
    assert torch.equal(rank.cpu()[live], want_rank[live]) and (rank.cpu()[ign] == -1).all()
    assert (tlp.cpu()[ign] == 0).all()
    fig = ((tlp.cpu().double() - (lt - lse)).abs() / (sc.ULP * (lt.abs() + lse.abs())).clamp(min=sc.ULP))[live].max()
    print(f"R = {R}: token_logprob figure {float(fig):.3f}")
    assert fig <= sc.BOUND_LOGPROB


def test_record_and_replay():
    """both launches recorded by native.record; the replay fills cleared outputs with the same bits"""
    c = sc.BY_ID["bf16-V10000-T5-ld10048"]
    t = sc.make(c).to(DEV)
    t.snapshot()
    prog = N.record(lambda: (sc.launch_rows(N, c, t), sc.launch_sequences(N, c, t)))
    torch.cuda.synchronize()
    assert prog.launches() == 2
    fig = sc.check(c, t)
    assert fig <= sc.BOUND_LOGPROB
    first = _bits(t)
    t.restore()
    prog.run()
    torch.cuda.synchronize()
    sc.check(c, t)
    for k, bits in _bits(t).items():
        assert torch.equal(bits, first[k]), f"{k} differs between the recorded run and its replay"
