"""The contract of caption scoring (include/mit_hip.h, csrc/score.hip): mit_score_rows, mit_score_rows_plan and
mit_score_sequences -- the cases, a float64 reference of both entry points, and a float32 emulation of the kernel's
arithmetic that sets the tolerance. tests/test_score_contract_cpu.py runs the references against each other and the
argument checks without a GPU; tests/test_score_contract_gpu.py runs every case on the device.

Units. u = 2^-23. A row's token_logprob = l_t - lse is measured against float64 in u (|l_t| + |lse|): the two float32
quantities it is made of. BOUND_LOGPROB = 4 x the worst float32 emulation figure over all cases and both summation
orders (`python tests/score_contract.py` prints them), the BOUND convention of beam_contract / decode_contract.
Everything else is exact: rank (an integer count of integer compares on the inputs: it involves no float arithmetic,
and the cases keep every column that is not an exact tie with the target at least MARGIN away from it, so a kernel
that compared rounded quantities would still have no freedom), the 0 / -1 of ignored rows, seq_tokens, seq_hits, and
seq_logprob, which is the float32 sequential sum of the kernel's OWN token_logprob, bit for bit. Guards: the NaN ld
padding, the NaN rows of ignored targets, the logits themselves and the bands around every output are untouched.
"""
from dataclasses import dataclass, field

import numpy as np
import torch

import decode_contract as dc

ULP = 2.0 ** -23
NAN = float("nan")
NEG_INF = float("-inf")
MARGIN = 1e-3            # every column is an exact tie with the target or at least this far from it
F32, BF16 = 0, 1
SCORE_STREAM, SCORE_REGS = 0, 1
REGS_MAX_V = 10240       # bf16 rows up to here run the register-resident kernel
SENT_F, SENT_I = -12288.0, -77
_TORCH = {"bf16": torch.bfloat16, "f32": torch.float32}
_CODE = {"bf16": BF16, "f32": F32}
# 4 x the worst float32 emulation figure (measured: seq 18.836 (bf16-V33000-T1) / tree 0.613 (bf16-V7-T5-ld10))
BOUND_LOGPROB = 4 * 18.836


def plan_expected(dtype, V):
    return SCORE_REGS if dtype == "bf16" and V <= REGS_MAX_V else SCORE_STREAM


# ------------------------------------------------------------------------------------------------
# float64 references
# ------------------------------------------------------------------------------------------------
def rows_reference(logits, targets, ignore):
    """logits [R, V] (any float dtype; rows of ignored targets may be NaN), targets [R] int64. Returns a dict:
    logprob float64 [R] (0 where ignored), rank int [R] (-1 where ignored), lse, logit (float64; 0 where ignored)"""
    R, V = logits.shape
    out = dict(logprob=torch.zeros(R, dtype=torch.float64), rank=torch.full((R,), -1, dtype=torch.int32),
               lse=torch.zeros(R, dtype=torch.float64), logit=torch.zeros(R, dtype=torch.float64))
    col = torch.arange(V)
    for r in range(R):
        t = int(targets[r])
        if t == ignore:
            continue
        x = logits[r].double()
        out["lse"][r] = torch.logsumexp(x, 0)
        out["logit"][r] = x[t]
        out["logprob"][r] = x[t] - out["lse"][r]
        out["rank"][r] = int(((x > x[t]) | ((x == x[t]) & (col < t))).sum())     # -0.0 == +0.0 as floats
    return out


def logprob_unit(ref):
    unit = ULP * (ref["logit"].abs() + ref["lse"].abs())
    return torch.where(torch.isfinite(unit) & (unit > 0), unit, torch.full_like(unit, ULP))


def logprob_figure(got, ref):
    """worst |got - ref| of the scored rows in units of u (|l_t| + |lse|); ignored rows must hold exactly 0"""
    ign = ref["rank"] < 0
    assert torch.equal(got[ign].double(), torch.zeros(int(ign.sum()), dtype=torch.float64)), "an ignored row is not 0"
    if ign.all():
        return 0.0
    return float(((got.double() - ref["logprob"]).abs() / logprob_unit(ref))[~ign].max())


def rows_emulation(logits, targets, ignore, mode):
    """float32 token_logprob as a kernel computes it: m = the row maximum, s = sum exp(x - m) in the `mode` order
    ("seq": one element after the other, "tree": pairwise), lse = m + log s, x_t - lse"""
    R = logits.shape[0]
    out = torch.zeros(R, dtype=torch.float32)
    live = [r for r in range(R) if int(targets[r]) != ignore]
    if not live:
        return out
    x = logits[live].float()
    m = x.max(1).values
    s = dc.fsum(torch.exp(x - m[:, None]), 1, mode)
    lse = m + torch.log(s)
    out[live] = x[torch.arange(len(live)), targets[live]] - lse
    return out


def sequences_reference(token_logprob, rank, T, dtype=np.float32):
    """(seq_logprob, seq_tokens, seq_hits): the sum over each sequence's T rows in row order, accumulated in `dtype`
    from 0 (float32: the kernel's arithmetic, to be met bit for bit; float64: the reference value), the rows with
    rank >= 0 and the rows with rank == 0 (rank None: no counts)"""
    x = np.asarray(token_logprob, dtype=dtype).reshape(-1, T)
    acc = np.zeros(x.shape[0], dtype=dtype)
    for j in range(T):
        acc = (acc + x[:, j]).astype(dtype)
    if rank is None:
        return acc, None, None
    rk = np.asarray(rank).reshape(-1, T)
    return acc, (rk >= 0).sum(1).astype(np.int32), (rk == 0).sum(1).astype(np.int32)


# ------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------
@dataclass
class Case:
    id: str
    dtype: str
    V: int
    ld: int
    T: int
    n_seq: int
    mis: int = 0          # logits misalignment in elements: the element-load path
    rank: bool = True     # False: rank == NULL (and no sequence counts)
    ignore: int = -100
    x: dict = field(default_factory=dict)

    @property
    def R(self):
        return self.n_seq * self.T


def _cases():
    cs = []
    for dt in ("bf16", "f32"):
        def add(V, ld, T, n_seq, **kw):
            tag = "".join(f"-{k}{v}" for k, v in kw.items())
            cs.append(Case(f"{dt}-V{V}-T{T}" + (f"-ld{ld}" if ld != V else "") + tag, dt, V, ld, T, n_seq, **kw))
        add(1, 1, 1, 7)
        add(7, 10, 5, 3)                      # ld no multiple of the 16-B chunk: element loads
        add(64, 64, 5, 3)                     # ld == V, whole chunks
        add(64, 64, 5, 3, ignore=0)           # the model's ignore_index: PAD = 0
        add(509, 512, 5, 3)                   # wide loads, a chunk that straddles V, NaN padding
        add(509, 509, 5, 3, mis=1)            # the same rows off the 16-B alignment: the same bits
        add(509, 512, 5, 3, rank=False)
        add(10000, 10048, 5, 3)               # the decoder head
        add(REGS_MAX_V, REGS_MAX_V, 1, 7)     # the last row length of the register-resident kernel ...
        add(REGS_MAX_V + 1, REGS_MAX_V + 8, 1, 7)   # ... and the first past it
        add(33000, 33000, 1, 7)
    return cs


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
PATTERNS = ("first", "last", "ignored", "ties", "zeros", "neginf", "plain")


def make_rows(c):
    """(logits float32 [R, V] holding values exact in the case's dtype, NaN rows where ignored; targets int64 [R]).
    Row r follows PATTERNS[r % 7]: the target at column 0 / at column V - 1 / ignored with a NaN row / exact ties
    with the target on both sides of it / a +0.0 target among -0.0 and +0.0 columns / a quarter of the columns -inf /
    plain. The seed depends on (dtype, V, T) only: cases that differ in ld, alignment or rank share their rows."""
    g = torch.Generator().manual_seed(1000003 * c.V + 31 * c.T + (7 if c.dtype == "bf16" else 0))
    R, V = c.R, c.V
    x = (torch.randn(R, V, generator=g) * 3).to(_TORCH[c.dtype]).float()
    tg = torch.randint(0, V, (R,), generator=g)
    for r in range(R):
        pat = PATTERNS[r % len(PATTERNS)]
        if pat == "first":
            tg[r] = 0
        elif pat == "last":
            tg[r] = V - 1
        elif pat in ("ties", "zeros") and V >= 7:
            t = int(torch.randint(2, V - 2, (1,), generator=g))
            tg[r] = t
            if pat == "zeros":
                x[r, t] = 0.0
                x[r, t - 1] = -0.0
                x[r, t + 1] = -0.0
                x[r, 0] = 0.0
            lo = torch.randint(0, t, (2,), generator=g)
            hi = torch.randint(t + 1, V, (2,), generator=g)
            x[r, lo] = float(x[r, t])
            x[r, hi] = float(x[r, t])
        elif pat == "neginf" and V >= 7:
            kill = torch.rand(V, generator=g) < 0.25
            kill[int(tg[r])] = False
            x[r, kill] = NEG_INF
        # a column is an exact tie with the target or at least MARGIN from it (moved in whole dtype steps)
        t = int(tg[r])
        near = ((x[r] - x[r, t]).abs() < MARGIN) & (x[r] != x[r, t])
        x[r, near] = (x[r, near] - 0.5).to(_TORCH[c.dtype]).float()
    for r in range(R):
        if PATTERNS[r % len(PATTERNS)] == "ignored":
            tg[r] = c.ignore
            x[r] = NAN
    return x, tg


def make(c):
    """The case's guarded buffers (dc.Tensors on the CPU): logits with NaN ld padding and NaN bands, targets, the
    outputs filled with sentinels; t.x = the float64 reference of the rows and the geometry."""
    x, tg = make_rows(c)
    R, V, ld = c.R, c.V, c.ld
    t = dc.Tensors()
    lg = t.new("logits", (R - 1) * ld + V, _TORCH[c.dtype], NAN, margin=16, misalign=c.mis)
    lg.win(0, R, V, ld).copy_(x.to(_TORCH[c.dtype]))
    t.new("targets", R, torch.int64, SENT_I).win(0, 1, R, R).copy_(tg[None])
    t.new("tlp", R, torch.float32, SENT_F).allow(0, 1, R, R)
    t.new("seq_logprob", c.n_seq, torch.float32, SENT_F).allow(0, 1, c.n_seq, c.n_seq)
    if c.rank:
        t.new("rank", R, torch.int32, SENT_I).allow(0, 1, R, R)
        t.new("seq_tokens", c.n_seq, torch.int32, SENT_I).allow(0, 1, c.n_seq, c.n_seq)
        t.new("seq_hits", c.n_seq, torch.int32, SENT_I).allow(0, 1, c.n_seq, c.n_seq)
    t.x = dict(logits=x, targets=tg, ref=rows_reference(x, tg, c.ignore))
    return t


def launch_rows(N, c, t):
    return N.lib().mit_score_rows(_CODE[c.dtype], c.R, c.V, t.ptr("logits"), c.ld, t.ptr("targets"), c.ignore,
                                  t.ptr("tlp"), t.ptr("rank"), None)


def launch_sequences(N, c, t):
    return N.lib().mit_score_sequences(c.n_seq, c.T, t.ptr("tlp"), t.ptr("rank"), t.ptr("seq_logprob"),
                                       t.ptr("seq_tokens"), t.ptr("seq_hits"), None)


def read(t, name, n):
    a = t.a[name]
    return a.whole.detach().cpu()[a.off:a.off + n]


def check(c, t):
    """Both entry points ran on t: ranks, counts and the sequence sums exact, guards intact; returns the
    token_logprob figure (in units of u (|l_t| + |lse|))."""
    ref = t.x["ref"]
    for k, a in t.a.items():
        a.check(f"{c.id}: {k}")
    tlp = read(t, "tlp", c.R)
    rank = read(t, "rank", c.R) if c.rank else None
    if c.rank:
        assert torch.equal(rank, ref["rank"]), f"{c.id}: rank {rank.tolist()} != {ref['rank'].tolist()}"
    want, tokens, hits = sequences_reference(tlp.numpy(), None if rank is None else rank.numpy(), c.T)
    got = read(t, "seq_logprob", c.n_seq).numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{c.id}: seq_logprob {got} != {want}"
    if c.rank:
        assert np.array_equal(read(t, "seq_tokens", c.n_seq).numpy(), tokens), f"{c.id}: seq_tokens"
        assert np.array_equal(read(t, "seq_hits", c.n_seq).numpy(), hits), f"{c.id}: seq_hits"
    return logprob_figure(tlp, ref)


def emulation_figures(cases=None):
    """{mode: (worst figure, case id)} of the float32 emulation over the cases"""
    worst = {}
    for c in cases or CASES:
        x, tg = make_rows(c)
        ref = rows_reference(x, tg, c.ignore)
        for mode in ("seq", "tree"):
            f = logprob_figure(rows_emulation(x, tg, c.ignore, mode), ref)
            if f > worst.get(mode, (-1.0, ""))[0]:
                worst[mode] = (f, c.id)
    return worst


if __name__ == "__main__":
    for mode, (f, cid) in emulation_figures().items():
        print(f"{mode}: {f:.3f} ({cid})")
    print("BOUND_LOGPROB", BOUND_LOGPROB)
