"""Contract helpers of the sampling kernels (csrc/sample.hip) and of the sampled decode built on them.

  uniform_reference     the counter hash of include/mit_hip.h (mit_sample_uniform) restated in integer numpy
  pick_reference        float64 reference of one row of mit_sample_pick: the order, the top-k set K1, the top-p
                        prefix K2, the draw in ascending token order, lse -- with the row's three DECISION MARGINS in
                        probability mass: `margin_u` (distance of u from the nearest running-sum boundary, over Z2),
                        `margin_p` (distance of top_p from the kept prefix's mass and from the mass one token
                        shorter, over Z1), `margin_k` (the logit gap across the top-k boundary; 0 = an exact tie,
                        which the order resolves)
  pick_emulation        the same in float32 the way a kernel computes it (weights, sums in a "seq" or "blocked"
                        order), with the worst deviation of a running-sum fraction from float64
  oracle_trajectory     sampling over oracle.ref_cpu.decoder_forward, every step's reference recorded

TAU_U, the pick tolerance, is 4 x the worst float32-emulation deviation of a running-sum fraction (the draw's
cum / Z2 and the top-p prefix's cum / Z1) from float64 over all pick cases and both orders (`python
tests/sample_contract.py` prints them): the BOUND convention of beam_contract / decode_contract. It is measured
against the float64 reference, never against the kernel. Every pick case supplies its uniforms and is built so that
each float margin is at least 2 TAU_U (or an exact tie by construction): a float32 kernel then has no freedom in any
pick. temperature, top_p and u reach the kernel as float32, so the reference takes their float32 values.
"""
import math
import zlib
from dataclasses import dataclass, field

import numpy as np
import torch

import decode_contract as dc
from decode_contract import INT_SENT, NAN, ULP

SAMPLE_SITE = 9000
NEG_INF = float("-inf")
M32 = 0xFFFFFFFF
# 4 x the worst float32 emulation figure (measured: seq 2.56921e-05 (pick-V10000-R5-k10000-p0.9-T1.0) / blocked
# 9.62755e-07 (pick-V10000-R5-k0-p0.9-T1.0))
TAU_U = 4 * 2.5693e-5

PICK_V = (7, 509, 512, 10000)
PICK_R = (1, 5)
PICK_T = (0.7, 1.0, 1.5)
PICK_P = (1.0, 0.9, 0.3)


# ------------------------------------------------------------------------------------------------
# the uniform
# ------------------------------------------------------------------------------------------------
def _lowbias32(x):
    x = np.asarray(x, dtype=np.uint64) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & M32
    x ^= x >> np.uint64(16)
    return x


def hash_words(seed, row0, R, p):
    """uint32 [R] (as uint64): h of rows row0 .. row0 + R - 1 at position p for the uint64 seed (None: 0)"""
    key = ((0 if seed is None else int(seed)) ^ (0xD6E8FEB86659FD93 * (SAMPLE_SITE + 1))) & 0xFFFFFFFFFFFFFFFF
    a = int(_lowbias32((key & M32) + 0x9E3779B9))
    b = int(_lowbias32((key >> 32) ^ a))
    rows = (np.arange(R, dtype=np.uint64) + np.uint64(int(row0) & M32)) & M32
    return _lowbias32(_lowbias32(rows ^ np.uint64(a)) ^ np.uint64((int(p) & M32) ^ b))


def uniform_reference(seed, row0, R, p):
    """float32 [R]: u = (h >> 8) * 2^-24 in [0, 1), exactly what mit_sample_uniform writes"""
    return ((hash_words(seed, row0, R, p) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)


# ------------------------------------------------------------------------------------------------
# the pick: float64 reference
# ------------------------------------------------------------------------------------------------
def _order(l):
    """token indices by (logit descending, token ascending); -0.0 == +0.0"""
    return np.lexsort((np.arange(l.shape[0]), -l))


def pick_reference(logits, T, top_k, top_p, u):
    """One live row. logits: 1-D float tensor / array (no NaN), T / top_p / u: numbers (taken at float32). Returns a
    dict: token, K1, K2 (token arrays in the order), lse, probs (the K2 tokens' interval probabilities, ascending
    token order), tokens (K2 ascending), margin_u, margin_p, margin_k."""
    l = np.asarray(torch.as_tensor(logits).double() if not isinstance(logits, np.ndarray) else logits, dtype=np.float64)
    T, top_p, u = float(np.float32(T)), float(np.float32(top_p)), float(np.float32(u))
    V = l.shape[0]
    order = _order(l)
    k = top_k if 0 < top_k < V else V
    K1 = order[:k]
    m = l.max()
    w = np.exp((l - m) / T)
    margin_k = math.inf if k == V else float(l[order[k - 1]] - l[order[k]])
    cum1 = np.cumsum(w[K1])
    Z1 = cum1[-1]
    if top_p >= 1.0:
        n2, margin_p = k, math.inf
    else:
        n2 = min(int(np.searchsorted(cum1, top_p * Z1, side="left")) + 1, k)   # the first prefix with cum >= top_p Z1
        below = cum1[n2 - 2] if n2 >= 2 else 0.0
        margin_p = float(min(cum1[n2 - 1] - top_p * Z1, top_p * Z1 - below) / Z1)
    K2 = order[:n2]
    toks = np.sort(K2)
    cum2 = np.cumsum(w[toks])
    Z2 = cum2[-1]
    mark = u * Z2
    i = int(np.searchsorted(cum2, mark, side="right"))                         # the first running sum > mark
    i = min(i, toks.shape[0] - 1)
    bounds = np.concatenate([[0.0], cum2])
    d = np.abs(bounds - mark)
    if u == 0.0:
        d = d[bounds != 0.0]            # the exact tie with the empty prefix: the strict '>' decides
    lse = float(m + math.log(np.exp(l - m).sum()))
    return dict(token=int(toks[i]), K1=K1, K2=K2, tokens=toks, probs=np.diff(bounds) / Z2, lse=lse,
                margin_u=float(d.min() / Z2), margin_p=margin_p, margin_k=margin_k, Z1=float(Z1), Z2=float(Z2),
                frac_u=cum2 / Z2, frac_p=cum1[:n2] / Z1, logit=float(l[toks[i]]))


def _cumsum32(x, mode):
    """float32 running sums: "seq" one element after the other; "blocked" 64-element spans summed in sequence, the
    spans' totals scanned, each span's running sum started from its base (a block scan)"""
    x = x.astype(np.float32)
    if mode == "seq":
        return np.cumsum(x, dtype=np.float32)
    out = np.empty_like(x)
    base = np.float32(0)
    for s in range(0, x.shape[0], 64):
        seg = np.cumsum(x[s:s + 64], dtype=np.float32)
        out[s:s + 64] = base + seg
        base = np.float32(base + seg[-1])
    return out


def pick_emulation(logits, T, top_k, top_p, u, order="seq"):
    """pick_reference in float32: w = exp((l - m) / T) in float32, the sets from the integer order (exact), every
    sum in the `order` summation. Returns dict(token, n2, dev): dev = the worst |fraction32 - fraction64| over the
    draw's running sums / Z2 and the top-p prefix sums / Z1 (nan when the emulation's sets differ from float64's)."""
    ref = pick_reference(logits, T, top_k, top_p, u)
    l = np.asarray(torch.as_tensor(logits).float(), dtype=np.float32)
    T32, p32, u32 = np.float32(T), np.float32(top_p), np.float32(u)
    V = l.shape[0]
    ordr = _order(l.astype(np.float64))
    k = top_k if 0 < top_k < V else V
    K1 = ordr[:k]
    m = l.max()
    w = np.exp(((l - m) / T32).astype(np.float32)).astype(np.float32)
    cum1 = _cumsum32(w[K1], order)
    Z1 = cum1[-1]
    if p32 >= 1.0:
        n2 = k
    else:
        n2 = min(int(np.searchsorted(cum1, np.float32(p32 * Z1), side="left")) + 1, k)
    toks = np.sort(ordr[:n2])
    cum2 = _cumsum32(w[toks], order)
    Z2 = cum2[-1]
    i = min(int(np.searchsorted(cum2, np.float32(u32 * Z2), side="right")), toks.shape[0] - 1)
    dev = math.nan
    if n2 == ref["K2"].shape[0]:
        dev = float(np.abs(cum2.astype(np.float64) / float(Z2) - ref["frac_u"]).max())
        if p32 < 1.0:
            dev = max(dev, float(np.abs(cum1[:n2].astype(np.float64) / float(Z1) - ref["frac_p"]).max()))
    return dict(token=int(toks[i]), n2=n2, dev=dev)


# ------------------------------------------------------------------------------------------------
# the pick: cases
# ------------------------------------------------------------------------------------------------
@dataclass
class PickCase:
    id: str
    R: int
    V: int
    T: float = 1.0
    top_k: int = 0
    top_p: float = 1.0          # nominal: the case's top_p is a midpoint of two prefix masses near it (t.x["top_p"])
    kind: str = "mix"
    p: int = 5
    L: int = 12                 # ld_ids
    ld_pad: int = 3
    mis: int = 0                # logits misalignment (elements): 4-B loads
    end_id: int = 1
    pad_id: int = 0
    x: dict = field(default_factory=dict)


def _geometry(V):
    # 7: ld = 10 (scalar loads); 509: an odd vocabulary on a misaligned base (scalar loads); 512 / 10000: ld % 4 == 0
    # on an aligned base (16-B loads)
    return dict(ld_pad=0 if V in (512, 10000) else 3, mis=1 if V == 509 else 0)


def _pick_cases():
    cs = []
    i = 0
    for V in PICK_V:
        for R in PICK_R:
            for top_k in (0, 1, 3, 50, V):
                for top_p in PICK_P:
                    T = PICK_T[i % 3]
                    i += 1
                    cs.append(PickCase(f"pick-V{V}-R{R}-k{top_k}-p{top_p}-T{T}", R, V, T, top_k, top_p,
                                       p=5 if R == 1 else 9, **_geometry(V)))
    cs += [
        PickCase("pick-tie-V512-k3", 3, 512, 0.7, 3, 1.0, kind="tie", ld_pad=0),
        PickCase("pick-tie-V509-k3-p0.9", 3, 509, 1.0, 3, 0.9, kind="tie", mis=1),
        PickCase("pick-neginf-V509", 3, 509, 1.0, 0, 1.0, kind="neginf", mis=1),
        PickCase("pick-neginf-V512-k50-p0.9", 3, 512, 1.5, 50, 0.9, kind="neginf", ld_pad=0),
        PickCase("pick-u0-V512-k3", 3, 512, 1.0, 3, 1.0, kind="u0", ld_pad=0),
        PickCase("pick-u0-V7", 2, 7, 0.7, 0, 1.0, kind="u0"),
        PickCase("pick-end-V509-k50", 4, 509, 1.0, 50, 1.0, kind="end", mis=1),
        PickCase("pick-allfinished-V7", 3, 7, 1.0, 0, 1.0, kind="allfinished"),
        PickCase("pick-tail-V509-ld512", 3, 509, 0.7, 50, 0.9, ld_pad=3, mis=0),      # 16-B loads with a ragged last chunk
        PickCase("pick-lastcol-V512", 2, 512, 1.0, 3, 0.9, p=10, L=12, ld_pad=0),
        PickCase("pick-start-V10000", 5, 10000, 0.7, 50, 0.9, p=0, ld_pad=0),
        # 1024 / 10240 logits: the last sizes of the kernels that keep 1 / 10 chunks of weights per thread in registers
        PickCase("pick-V1024-k50-p0.9", 2, 1024, 1.0, 50, 0.9, ld_pad=0),
        PickCase("pick-V1025-k50-p0.9", 2, 1025, 0.7, 50, 0.9, ld_pad=3),
        PickCase("pick-V10240-k50-p0.3", 2, 10240, 1.0, 50, 0.3, ld_pad=0),
        PickCase("pick-V10241-k0-p0.9", 2, 10241, 0.7, 0, 0.9, ld_pad=3),
        # past the 12288 logits a block keeps in LDS: the row is re-read from memory
        PickCase("pick-V12293-k50-p0.9", 2, 12293, 0.7, 50, 0.9, ld_pad=3),
        PickCase("pick-V12292-k0-p0.3", 2, 12292, 1.0, 0, 0.3, ld_pad=0),
        PickCase("pick-V12288-k0-p1.0", 1, 12288, 1.5, 0, 1.0, ld_pad=0),
    ]
    return cs


PICK_CASES = _pick_cases()
PICK_BY_ID = {c.id: c for c in PICK_CASES}


def _pick_state(c, seed):
    """(logits [R, V] f32, finished [R]) on the CPU; logits peaked enough (randn * 5) that consecutive prefix masses
    near any top_p lie several TAU_U apart"""
    g = torch.Generator().manual_seed(seed)
    R, V = c.R, c.V
    lg = torch.randn(R, V, generator=g) * 5.0
    fin = torch.zeros(R, dtype=torch.int32)
    if c.kind == "mix" and R > 1:
        fin[torch.arange(R) % 5 == 3] = 1
    elif c.kind == "tie":
        # bitwise equal logits straddling the top-k boundary: 50 first, then 17, 210, 300, 400 by token
        for r in range(R):
            lg[r, 50] = 20.5
            lg[r, [400, 17, 300, 210]] = 20.0
    elif c.kind == "neginf":
        lg[:, torch.randperm(V, generator=g)[:V // 3]] = NEG_INF
        lg[0, 0] = NEG_INF
    elif c.kind == "allfinished":
        fin[:] = 1
    return lg, fin


def _choose_top_p(c, lg, fin):
    """the midpoint of two consecutive prefix masses of the first live row, nearest the nominal top_p"""
    if c.top_p >= 1.0:
        return 1.0
    live = [r for r in range(c.R) if not int(fin[r])]
    if not live:
        return c.top_p
    ref = pick_reference(lg[live[0]], c.T, c.top_k, 1.0, 0.5)
    l = lg[live[0]].double().numpy()
    w = np.exp((l - l.max()) / float(np.float32(c.T)))
    mass = np.concatenate([[0.0], np.cumsum(w[ref["K1"]])]) / ref["Z1"]
    mid = (mass[:-1] + mass[1:]) / 2
    return float(np.float32(mid[int(np.abs(mid - c.top_p).argmin())]))


def make_pick(c):
    """The case's guarded tensors (dc.Tensors on the CPU) with t.x = the float64 references and geometry. The seed is
    advanced until every float margin of every live row is at least 2 TAU_U (asserted); u is the midpoint of a kept
    token's interval (0 for the u0 kind)."""
    R, V, L, p = c.R, c.V, c.L, c.p
    assert p + 1 < L
    base = zlib.crc32(c.id.encode())
    for attempt in range(64):
        lg, fin = _pick_state(c, base + attempt)
        g = torch.Generator().manual_seed(base + 1000 + attempt)
        top_p = _choose_top_p(c, lg, fin)
        us, refs, ok = np.zeros(R, dtype=np.float32), [None] * R, True
        for r in range(R):
            if int(fin[r]):
                continue
            ref = pick_reference(lg[r], c.T, c.top_k, top_p, 0.5)
            if c.kind == "u0":
                u = 0.0
            else:
                # a kept token drawn with its probability among those whose interval is wide enough
                pr = np.where(ref["probs"] >= 5 * TAU_U, ref["probs"], 0.0)
                if pr.sum() == 0:
                    ok = False
                    break
                j = int(torch.multinomial(torch.from_numpy(pr / pr.sum()), 1, generator=g))
                lo = ref["probs"][:j].sum()
                u = float(np.float32(lo + ref["probs"][j] / 2))
            refs[r] = pick_reference(lg[r], c.T, c.top_k, top_p, u)
            us[r] = u
            ok = ok and min(refs[r]["margin_u"], refs[r]["margin_p"]) >= 2 * TAU_U
        if ok:
            break
    else:
        raise AssertionError(f"{c.id}: no seed gives margins of at least {2 * TAU_U}")
    end_id = c.end_id
    live = [r for r in range(R) if refs[r] is not None]
    if c.kind == "end":
        end_id = refs[live[0]]["token"]
    if c.kind == "tie":
        for r in live:
            assert refs[r]["margin_k"] == 0 and set(refs[r]["K1"].tolist()) == {50, 17, 210}, c.id
    lg = lg.clone()
    lg[fin != 0] = NAN                           # finished rows' logits are never read
    ld = V + c.ld_pad
    lp0 = -(torch.rand(R, generator=g) * 8.0)
    len0 = torch.full((R,), p, dtype=torch.int32)
    t = dc.Tensors()
    a = t.new("logits", R * ld, torch.float32, NAN, margin=ld + 8, misalign=c.mis)
    a.win(0, R, V, ld).copy_(lg)
    ids = torch.full((R, L), INT_SENT, dtype=torch.int64)
    ids[:, :p + 1] = torch.randint(2, V, (R, p + 1), generator=g)
    t.new("ids", R * L, torch.int64, INT_SENT, margin=L).win(0, R, L, L).copy_(ids)
    t.a["ids"].allow(p + 1, R, 1, L)
    t.new("uniforms", R, torch.float32, NAN, margin=8).base[:R] = torch.from_numpy(us)
    t.new("finished", R, torch.int32, INT_SENT, margin=8).base[:R] = fin
    t.new("logprob", R, torch.float32, NAN, margin=8).base[:R] = lp0
    t.new("length", R, torch.int32, INT_SENT, margin=8).base[:R] = len0
    for r in live:                               # nothing of a finished row but its ids column is written
        for name in ("finished", "logprob", "length"):
            t.a[name].allow(r, 1, 1, 1)
    t.new("pos", 1, torch.int64, INT_SENT, margin=8).base[0] = p
    t.a["pos"].allow(0, 1, 1, 1)
    t.new("n_finished", 1, torch.int32, INT_SENT, margin=8).base[0] = int(fin.sum())
    t.a["n_finished"].allow(0, 1, 1, 1)
    t.new("ticket", 1, torch.int32, INT_SENT, margin=8).base[0] = 0
    t.a["ticket"].allow(0, 1, 1, 1)
    token = torch.tensor([refs[r]["token"] if refs[r] else c.pad_id for r in range(R)])
    t.x.update(refs=refs, ld=ld, R=R, logits=lg, fin0=fin, lp0=lp0, len0=len0, top_p=top_p, end_id=end_id,
               token=token, us=us, ids0=ids)
    return t


def launch_pick(N, c, t, uniforms=True, seed_ptr=None, row0=0):
    """mit_sample_pick on the case's buffers through the raw C entry point (pointers into the guarded arrays)"""
    return N.lib().mit_sample_pick(c.R, c.V, t.ptr("logits"), t.x["ld"], c.T, c.top_k, t.x["top_p"], seed_ptr, row0,
                                   t.ptr("uniforms") if uniforms else None, t.ptr("ids"), c.L, t.ptr("pos"),
                                   t.x["end_id"], c.pad_id, t.ptr("finished"), t.ptr("n_finished"), t.ptr("logprob"),
                                   t.ptr("length"), t.ptr("ticket"), None)


def read(t, name, n):
    a = t.a[name]
    return a.whole.detach().cpu()[a.off:a.off + n]


def check_pick(c, t):
    """Exact state against the reference; returns the worst logprob figure in units of u (|logprob_in| + |logit| +
    |lse|)."""
    R, p, refs = c.R, c.p, t.x["refs"]
    ids = read(t, "ids", R * c.L).view(R, c.L)
    assert torch.equal(ids[:, p + 1], t.x["token"]), \
        f"{c.id}: tokens {ids[:, p + 1].tolist()} expected {t.x['token'].tolist()}"
    want = t.x["ids0"].clone()
    want[:, p + 1] = t.x["token"]
    assert torch.equal(ids, want), f"{c.id}: an ids column other than p + 1 changed"
    fin0 = t.x["fin0"]
    ends = torch.tensor([int(refs[r] is not None and refs[r]["token"] == t.x["end_id"]) for r in range(R)],
                        dtype=torch.int32)
    assert torch.equal(read(t, "finished", R), fin0 | ends), f"{c.id}: finished"
    assert torch.equal(read(t, "length", R), t.x["len0"] + (1 - fin0)), f"{c.id}: length"
    assert int(read(t, "n_finished", 1)) == int(fin0.sum()) + int(ends.sum()), f"{c.id}: n_finished is incremented"
    assert int(read(t, "pos", 1)) == p + 1, f"{c.id}: pos {int(read(t, 'pos', 1))}: it advances exactly once"
    assert int(read(t, "ticket", 1)) == 0, f"{c.id}: ticket left at {int(read(t, 'ticket', 1))}"
    for name, a in t.a.items():
        a.check(name)
    lp = read(t, "logprob", R).double()
    fig = 0.0
    for r in range(R):
        if refs[r] is None:
            continue
        lp0 = float(t.x["lp0"][r])
        want_lp = lp0 + refs[r]["logit"] - refs[r]["lse"]
        unit = ULP * (abs(lp0) + abs(refs[r]["logit"]) + abs(refs[r]["lse"]))
        fig = max(fig, abs(float(lp[r]) - want_lp) / unit)
    return fig


def emulation_figures(cases=None):
    """{order: (worst deviation of a running-sum fraction, case id)} of the float32 emulation over the pick cases;
    asserts that the emulation picks what float64 picks"""
    worst = {}
    for c in cases or PICK_CASES:
        t = make_pick(c)
        for order in ("seq", "blocked"):
            for r, ref in enumerate(t.x["refs"]):
                if ref is None:
                    continue
                em = pick_emulation(t.x["logits"][r], c.T, c.top_k, t.x["top_p"], t.x["us"][r], order)
                assert em["token"] == ref["token"] and em["n2"] == ref["K2"].shape[0], (c.id, r, order)
                if em["dev"] > worst.get(order, (-1.0, ""))[0]:
                    worst[order] = (em["dev"], c.id)
    return worst


# ------------------------------------------------------------------------------------------------
# the algorithm over the pinned oracle
# ------------------------------------------------------------------------------------------------
TAU = 1e-3                               # the project's fp32 logit bound
E2E_FIXTURE = "tiny_vit_patches"
E2E_START, E2E_END, E2E_MAX_LEN = 2, 69, 12
E2E_T, E2E_TOP_K = 0.5, 3
E2E_SEED = 0                             # committed by the seed search (`python tests/sample_contract.py --seeds`)


def undecided(ref, T):
    """True when a logit error of TAU could change the step's pick: a logit moving by TAU moves a probability mass
    by at most the factor exp(2 TAU / T)"""
    mass = TAU_U + math.exp(2 * TAU / T) - 1
    return ref["margin_u"] <= mass or ref["margin_k"] <= 2 * TAU or ref["margin_p"] <= mass


def e2e_images(FX):
    meta, _ = FX.load(E2E_FIXTURE)
    img = FX.inputs(meta, 0)[0]
    return torch.cat([img, img.flip(-1), img * 0.5])[:4].contiguous()


_E2E = {}


def e2e_memory(FX):
    from oracle import ref_cpu
    if "mem" not in _E2E:
        meta, _ = FX.load(E2E_FIXTURE)
        st = FX.state(meta)
        with torch.no_grad():
            mem = ref_cpu.memory_from_features(st, ref_cpu.encode(st, e2e_images(FX), FX.enc_desc(meta)), meta["mode"])
        _E2E["mem"] = (st, FX.dec_desc(meta), mem)
    return _E2E["mem"]


@torch.no_grad()
def oracle_steps(FX, ids, row, seed, n_steps=None):
    """The references of every step of ONE produced sequence (ids: START first, cut after END): a single
    teacher-forced oracle forward, then per position p the pick_reference of its logits at u(seed, row, p).
    Returns (references, float64 log_softmax of the logits [steps, V])."""
    from oracle import ref_cpu
    st, dec, mem = e2e_memory(FX)
    n = len(ids) - 1 if n_steps is None else n_steps
    toks = torch.tensor([ids[:n]])
    lg = ref_cpu.decoder_forward(st, toks, mem[row:row + 1], heads=dec["heads"], layers=dec["layers"],
                                 max_len=dec.get("max_seq_len", 100))[0]
    refs = [pick_reference(lg[p], E2E_T, E2E_TOP_K, 1.0, float(uniform_reference(seed, row, 1, p)[0]))
            for p in range(n)]
    return refs, torch.log_softmax(lg.double(), -1)


@torch.no_grad()
def oracle_trajectory(FX, seed, max_len=E2E_MAX_LEN):
    """The oracle's OWN sampled captions of the end-to-end images for `seed` (full-prefix recompute per token):
    [(ids, [step references])] per image, ids cut after END."""
    from oracle import ref_cpu
    st, dec, mem = e2e_memory(FX)
    out = []
    for row in range(mem.shape[0]):
        ids, refs = [E2E_START], []
        for p in range(max_len - 1):
            lg = ref_cpu.decoder_forward(st, torch.tensor([ids]), mem[row:row + 1], heads=dec["heads"],
                                         layers=dec["layers"], max_len=dec.get("max_seq_len", 100))[0, -1]
            ref = pick_reference(lg, E2E_T, E2E_TOP_K, 1.0, float(uniform_reference(seed, row, 1, p)[0]))
            refs.append(ref)
            ids.append(ref["token"])
            if ref["token"] == E2E_END:
                break
        out.append((ids, refs))
    return out


def undecided_share(traj):
    steps = [r for _, refs in traj for r in refs]
    return sum(undecided(r, E2E_T) for r in steps) / len(steps)


if __name__ == "__main__":
    import sys
    if "--seeds" in sys.argv:
        import os
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        import fixtures as FX
        for s in range(256):
            sh = undecided_share(oracle_trajectory(FX, s))
            print(f"seed {s}: {sh:.3f} of the oracle's own steps undecided", flush=True)
            if sh < 0.05:
                break
    else:
        for order, (f, cid) in emulation_figures().items():
            print(f"running-sum fraction, float32 emulation, {order}: worst {f:.5e} ({cid})")
