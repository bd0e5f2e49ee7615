"""Contract helpers of the beam-search kernels (csrc/beam.hip) and of the beam decode built on them.

  select_reference      float64 reference of mit_beam_select: the textbook step -- live slots offer their V
                        continuations at score + log_softmax(logits), finished slots themselves (padded), the K best
                        by (score descending, parent ascending, token ascending) go on -- with the state / tok / anc
                        update and the step's DECISION MARGIN: the smallest gap between consecutive candidates among
                        the best K + 1 (0 for an exact tie, which the (parent, token) order resolves)
  select_emulation      the same scores in float32 the way a kernel computes them (row maximum, sum of exp in a
                        "seq" or "tree" order, log, score + (logit - lse)), to size the float tolerance
  gathered_attention    float64 reference of mit_attention_decode_beam and its conditioning unit (decode_contract's)
  beam_search_reference the algorithm over oracle.ref_cpu.decoder_forward (full-prefix recompute per beam), every
                        step's state recorded

Units. u = 2^-23. A new slot's score is measured against float64 in u (|score_parent| + |logit| + |lse|): the three
float32 quantities the candidate is made of. BOUND_SCORE = 4 x the worst float32 emulation figure over all select
cases and both orders (`python tests/beam_contract.py` prints them), the BOUND convention of decode_contract /
ln_contract. Everything else of a selection is exact: tokens, parents, finished, length, n_finished, pos, anc, guards.

The select cases are built so that every float64 decision margin is either an exact tie by construction (bitwise
equal logits in a row; parents with bitwise equal scores and rows) or larger than TAU = 1e-3, the project's fp32
logit bound: a float32 kernel then has no freedom in any pick.
"""
import math
import zlib
from dataclasses import dataclass, field

import torch

import decode_contract as dc
from decode_contract import INT_SENT, NAN, ULP

TAU = 1e-3
NEG_INF = float("-inf")
# 4 x the worst float32 emulation figure (measured: seq 2.847 (sel-mix-V10000-K8-B5) / tree 0.228 (sel-mix-V509-K4-B1))
BOUND_SCORE = 4 * 2.847

SEL_V = (7, 509, 512, 10000)
SEL_K = (1, 3, 4, 8)
SEL_B = (1, 5)


# ------------------------------------------------------------------------------------------------
# mit_beam_select: float64 reference
# ------------------------------------------------------------------------------------------------
def select_reference(logits, score, finished, length, tok, anc, p, K, end_id, pad_id):
    """One selection step. logits [R, V] (rows of finished slots are ignored, may be NaN), score [R] float,
    finished / length [R] int, tok [R, T] int64, anc [R, T] int; p the position. Returns a dict: score (float64),
    finished, length, tok, anc (updated copies), parent [R] (slot within the image), token [R], n_finished,
    margin (float: the smallest gap between consecutive candidates among the best K + 1 over all images; 0 = tie),
    lse [R] (float64; nan for finished rows), src_logit [R] (the chosen logit; 0 for a finished parent)."""
    R, V = logits.shape
    B = R // K
    lg = logits.double()
    sc = score.double()
    out = dict(score=torch.empty(R, dtype=torch.float64), finished=finished.clone(), length=length.clone(),
               tok=tok.clone(), anc=anc.clone(), parent=torch.empty(R, dtype=torch.int64),
               token=torch.empty(R, dtype=torch.int64), lse=torch.full((R,), NAN, dtype=torch.float64),
               src_logit=torch.zeros(R, dtype=torch.float64))
    margin = math.inf
    for b in range(B):
        cands = []  # (score, parent, token, logit)
        for k in range(K):
            r = b * K + k
            if int(finished[r]):
                cands.append((float(sc[r]), k, int(pad_id), 0.0))
                continue
            lse = torch.logsumexp(lg[r], 0)
            out["lse"][r] = lse
            val = sc[r] + (lg[r] - lse)
            # the K + 1 best of the row are enough for the image's K + 1 best
            n = min(V, K + 1)
            top = torch.topk(val, n, sorted=True)
            # ties inside topk come in no promised order: collect every token at the n-th value or above
            idx = (val >= top.values[-1]).nonzero()[:, 0].tolist()
            cands.extend((float(val[v]), k, v, float(lg[r, v])) for v in idx)
        cands.sort(key=lambda c: (-c[0] if not math.isnan(c[0]) else -math.inf, c[1], c[2]))
        best = cands[:K + 1]
        for a, c in zip(best, best[1:]):
            gap = a[0] - c[0]
            if not math.isnan(gap) and not (math.isinf(a[0]) and math.isinf(c[0])):
                margin = min(margin, gap)
        for k, (s, par, token, lgt) in enumerate(cands[:K]):
            r, rp = b * K + k, b * K + par
            pf = int(finished[rp])
            out["score"][r] = s
            out["parent"][r], out["token"][r] = par, token
            out["finished"][r] = 1 if (pf or token == end_id) else 0
            out["length"][r] = int(length[rp]) + (0 if pf else 1)
            out["tok"][r, p + 1] = token
            out["anc"][r, :p + 1] = anc[rp, :p + 1]
            out["anc"][r, p + 1] = k
            out["src_logit"][r] = lgt
    out["parent_lse"] = torch.stack([torch.logsumexp(lg[(r // K) * K + int(out["parent"][r])], 0)
                                     if not int(finished[(r // K) * K + int(out["parent"][r])]) else
                                     torch.tensor(0.0, dtype=torch.float64) for r in range(R)])
    out["parent_score"] = torch.stack([sc[(r // K) * K + int(out["parent"][r])] for r in range(R)])
    out["n_finished"] = int(out["finished"].sum())
    out["margin"] = margin
    return out


def score_unit(ref):
    """u (|score_parent| + |logit| + |lse|) per new slot (-inf scores: unit 1, they are compared exactly)"""
    unit = ULP * (ref["parent_score"].abs() + ref["src_logit"].abs() + ref["parent_lse"].abs())
    return torch.where(torch.isfinite(unit) & (unit > 0), unit, torch.full_like(unit, ULP))


def select_emulation(logits, score, finished, ref, K, mode):
    """float32 scores of the reference's picks, computed as a kernel would: m = max, s = sum exp(x - m) in the
    `mode` order ("seq": one element after the other, "tree": pairwise), lse = m + log s, score + (logit - lse)"""
    R = logits.shape[0]
    out = torch.empty(R, dtype=torch.float32)
    lse = {}
    for r in range(R):
        rp = (r // K) * K + int(ref["parent"][r])
        if int(finished[rp]):
            out[r] = score[rp]
            continue
        if rp not in lse:
            x = logits[rp].float()
            m = x.max()
            lse[rp] = m + torch.log(dc.fsum(torch.exp(x - m), 0, mode))
        out[r] = score[rp].float() + (logits[rp, int(ref["token"][r])].float() - lse[rp])
    return out


def score_figure(got, ref):
    """worst |got - ref| in score units; -inf must match exactly"""
    r = ref["score"]
    inf = torch.isinf(r)
    assert torch.equal(got.double()[inf], r[inf]), "an infinite score differs"
    if inf.all():
        return 0.0
    return float(((got.double() - r).abs() / score_unit(ref))[~inf].max())


# ------------------------------------------------------------------------------------------------
# mit_beam_select: cases
# ------------------------------------------------------------------------------------------------
@dataclass
class SelCase:
    id: str
    B: int
    K: int
    V: int
    kind: str = "mix"
    p: int = 5
    T: int = 12          # ld_tok
    Ta: int = 14         # ld_anc
    ld_pad: int = 3
    mis: int = 0         # logits misalignment (elements): 4-B loads
    end_id: int = 1
    pad_id: int = 0
    parents: tuple = ()  # the parent map the case is built to produce (slot -> parent), image 0
    x: dict = field(default_factory=dict)


def _sel_cases():
    cs = []
    for V in SEL_V:
        for K in SEL_K:
            if K > V:
                continue
            for B in SEL_B:
                # 509: an odd vocabulary on a misaligned row (scalar loads); 512 / 10000: ld % 4 == 0 (16-B loads)
                cs.append(SelCase(f"sel-mix-V{V}-K{K}-B{B}", B, K, V, ld_pad=0 if V in (512, 10000) else 3,
                                  mis=1 if V == 509 else 0, p=5 if B == 1 else 9))
    cs += [
        SelCase("sel-dupmax-V512-K3", 2, 3, 512, kind="dupmax", ld_pad=0),
        SelCase("sel-twins-V509-K4", 2, 4, 509, kind="twins"),
        SelCase("sel-oneparent-V512-K4", 2, 4, 512, kind="oneparent", ld_pad=0),
        SelCase("sel-start-V509-K3", 3, 3, 509, kind="start", p=0),
        SelCase("sel-start-V10000-K8", 2, 8, 10000, kind="start", p=0, ld_pad=0),
        SelCase("sel-finished-V512-K4", 3, 4, 512, kind="finished", ld_pad=0),
        SelCase("sel-allfinished-V7-K3", 2, 3, 7, kind="allfinished"),
        SelCase("sel-end-V509-K3", 2, 3, 509, kind="end"),
        SelCase("sel-map120-V512-K3", 2, 3, 512, kind="map", parents=(1, 2, 0), ld_pad=0),
        SelCase("sel-map110-V509-K3", 2, 3, 509, kind="map", parents=(1, 1, 0)),
        SelCase("sel-map222-V7-K3", 2, 3, 7, kind="map", parents=(2, 2, 2)),
        SelCase("sel-lastcol-V512-K3", 2, 3, 512, kind="mix", p=10, T=12, Ta=12, ld_pad=0),
    ]
    return cs


SEL_CASES = _sel_cases()
SEL_BY_ID = {c.id: c for c in SEL_CASES}


def _sel_state(c, seed):
    """(logits [R, V] f32 with NaN rows where finished, score, finished, length) on the CPU"""
    g = torch.Generator().manual_seed(seed)
    B, K, V = c.B, c.K, c.V
    R = B * K
    lg = torch.randn(R, V, generator=g) * 3.0
    score = -(torch.rand(R, generator=g) * 8.0)
    fin = torch.zeros(R, dtype=torch.int32)
    length = torch.full((R,), c.p, dtype=torch.int32)
    kind = c.kind
    if kind == "mix" and K > 1:
        fin[torch.arange(R) % 5 == 3] = 1      # some finished parents, one of them with the image's best score
        if R > 3:
            score[3] = 0.25
        lg[:, c.end_id] += 4.0                 # END competitive in every row
    elif kind == "dupmax":
        # the row maximum twice (bitwise): the lower token first; a third equal value further on
        for r in range(R):
            lg[r, [400, 17, 300]] = 9.0
    elif kind == "twins":
        # parents 1 and 2 of every image: bitwise equal scores and rows -- the lower parent's candidate first
        for b in range(B):
            lg[b * K + 2] = lg[b * K + 1]
            score[b * K + 2] = score[b * K + 1] = -0.5
            score[b * K + 0] = score[b * K + 3] = -9.0
    elif kind == "oneparent":
        score[:] = -60.0
        score[1::K] = -1.0
    elif kind == "start":
        score[:] = NEG_INF
        score[0::K] = 0.0
        length[:] = 0
    elif kind == "finished":
        fin[:] = 1
        fin[0::K] = 0                           # one live parent per image, the others keep their place by score
        score[1::K] = -0.125
        fin[K + 1] = 0                          # image 1: two live parents
    elif kind == "allfinished":
        fin[:] = 1
    elif kind == "end":
        lg[:, c.end_id] = 12.0                  # END wins everywhere
    elif kind == "map":
        lg = torch.randn(R, V, generator=g) * 0.5
        m = c.parents
        score[:] = -40.0
        for b in range(B):
            rows = [b * K + k for k in range(K)]
            if m == (1, 2, 0):
                for r, s in zip(rows, (-3.0, -1.0, -2.0)):
                    score[r] = s
                    lg[r, 3 + r % 3] = 25.0
            elif m == (1, 1, 0):
                score[rows[1]], score[rows[0]] = -1.0, -4.0
                lg[rows[1], 5], lg[rows[1], 2] = 25.0, 24.5
                lg[rows[0], 6] = 25.0
            else:
                score[rows[2]] = -1.0
                lg[rows[2], 1], lg[rows[2], 4], lg[rows[2], 6] = 25.0, 24.5, 24.0
    lg[fin != 0] = NAN                          # finished rows' logits are never read
    length[fin != 0] -= 1
    return lg, score, fin, length


def make_select(c):
    """The case's guarded tensors (dc.Tensors on the CPU) with t.x = the float64 reference and geometry. The seed is
    advanced until every decision margin is an exact tie or > TAU (asserted)."""
    B, K, V = c.B, c.K, c.V
    R, T, Ta, p = B * K, c.T, c.Ta, c.p
    assert p + 1 < T and p + 1 < Ta
    base = zlib.crc32(c.id.encode())
    for attempt in range(64):
        lg, score, fin, length = _sel_state(c, base + attempt)
        g = torch.Generator().manual_seed(base + 1000 + attempt)
        tok = torch.full((R, T), INT_SENT, dtype=torch.int64)
        tok[:, :p + 1] = torch.randint(2, V, (R, p + 1), generator=g)
        anc = torch.full((R, Ta), INT_SENT, dtype=torch.int32)
        anc[:, :p + 1] = torch.randint(0, K, (R, p + 1), generator=g, dtype=torch.int32)
        ref = select_reference(lg, score, fin, length, tok, anc, p, K, c.end_id, c.pad_id)
        if ref["margin"] == 0 or ref["margin"] > TAU:
            break
    else:
        raise AssertionError(f"{c.id}: no seed gives margins that are ties or > {TAU}")
    assert ref["margin"] == 0 or ref["margin"] > TAU, (c.id, ref["margin"])
    if c.kind in ("dupmax", "twins"):
        assert ref["margin"] == 0, f"{c.id}: built to hold an exact tie"
    if c.parents:
        assert tuple(ref["parent"][:K].tolist()) == c.parents, (c.id, ref["parent"][:K].tolist())
    if c.kind == "oneparent":
        assert (ref["parent"] == 1).all()
    if c.kind == "start":
        assert (ref["parent"] == 0).all() and torch.isfinite(ref["score"]).all()
    ld = V + c.ld_pad
    t = dc.Tensors()
    a = t.new("logits", R * ld, torch.float32, NAN, margin=ld + 8, misalign=c.mis)
    a.win(0, R, V, ld).copy_(lg)
    t.new("score", R, torch.float32, NAN, margin=8).base[:R] = score
    t.a["score"].allow(0, 1, R, R)
    t.new("finished", R, torch.int32, INT_SENT, margin=8).base[:R] = fin
    t.a["finished"].allow(0, 1, R, R)
    t.new("length", R, torch.int32, INT_SENT, margin=8).base[:R] = length
    t.a["length"].allow(0, 1, R, R)
    t.new("tok", R * T, torch.int64, INT_SENT, margin=T).win(0, R, T, T).copy_(tok)
    t.a["tok"].allow(p + 1, R, 1, T)
    t.new("anc", R * Ta, torch.int32, INT_SENT, margin=Ta).win(0, R, Ta, Ta).copy_(anc)
    t.a["anc"].allow(0, R, p + 2, Ta)
    t.new("pos", 1, torch.int64, INT_SENT, margin=8).base[0] = p
    t.a["pos"].allow(0, 1, 1, 1)
    t.new("n_finished", 1, torch.int32, INT_SENT, margin=8).base[0] = 12345   # SET, not added to
    t.a["n_finished"].allow(0, 1, 1, 1)
    t.x.update(ref=ref, ld=ld, R=R, logits=lg, score0=score, fin0=fin)
    return t


def launch_select(N, c, t, ws):
    """mit_beam_select on the case's buffers through the raw C entry point (pointers into the guarded arrays)"""
    return N.lib().mit_beam_select(c.B, c.K, c.V, t.ptr("logits"), t.x["ld"], t.ptr("score"), t.ptr("tok"), c.T,
                                   t.ptr("anc"), c.Ta, t.ptr("pos"), c.end_id, c.pad_id, t.ptr("finished"),
                                   t.ptr("length"), t.ptr("n_finished"), ws.data_ptr(), ws.numel() * ws.element_size(),
                                   None)


def read(t, name, n):
    a = t.a[name]
    return a.whole.detach().cpu()[a.off:a.off + n]


def check_select(c, t):
    """Exact state against the reference; returns the score figure (in score units)."""
    ref, R, p = t.x["ref"], t.x["R"], c.p
    tok = read(t, "tok", R * c.T).view(R, c.T)
    anc = read(t, "anc", R * c.Ta).view(R, c.Ta)
    assert torch.equal(tok[:, p + 1], ref["token"]), \
        f"{c.id}: tokens {tok[:, p + 1].tolist()} expected {ref['token'].tolist()}"
    assert torch.equal(tok, ref["tok"]), f"{c.id}: a tok column other than p + 1 changed"
    assert torch.equal(anc[:, p + 1].long() % c.K, anc[:, p + 1].long()), f"{c.id}: ancestor outside [0, K)"
    assert torch.equal(anc, ref["anc"]), \
        f"{c.id}: ancestor table differs at {(anc != ref['anc']).nonzero()[:4].tolist()} (parents {ref['parent'].tolist()})"
    assert torch.equal(read(t, "finished", R), ref["finished"]), f"{c.id}: finished"
    assert torch.equal(read(t, "length", R), ref["length"]), f"{c.id}: length"
    assert int(read(t, "n_finished", 1)) == ref["n_finished"], \
        f"{c.id}: n_finished {int(read(t, 'n_finished', 1))} expected {ref['n_finished']} (set, not accumulated)"
    assert int(read(t, "pos", 1)) == p + 1, f"{c.id}: pos {int(read(t, 'pos', 1))}: it advances exactly once"
    for name, a in t.a.items():
        a.check(name)
    return score_figure(read(t, "score", R), ref)


def emulation_figures(cases=None):
    """{mode: (worst figure, case id)} of the float32 emulation over the select cases"""
    worst = {}
    for c in cases or SEL_CASES:
        t = make_select(c)
        for mode in ("seq", "tree"):
            em = select_emulation(t.x["logits"], t.x["score0"], t.x["fin0"], t.x["ref"], c.K, mode)
            f = score_figure(em, t.x["ref"])
            if f > worst.get(mode, (-1.0, ""))[0]:
                worst[mode] = (f, c.id)
    return worst


# ------------------------------------------------------------------------------------------------
# mit_attention_decode_beam: float64 reference
# ------------------------------------------------------------------------------------------------
def gather_index(R, Lk, group, anc):
    """[R, Lk] batch of key j for row r: through anc (int [R, >= Lk]) or r // group"""
    r = torch.arange(R)
    if anc is None:
        return (r // group)[:, None].expand(R, Lk)
    return ((r // group) * group)[:, None] + anc[:, :Lk].long()


def gathered_attention(q, k, v, Lk, group, anc, key_tokens, pad_idx, scale):
    """q [R, H, Dh]; k, v [NB, Lmax, H, Dh] (NB batches: R rows, or R / group images when anc is None); key_tokens
    [NB, Lmax] or None. Returns (o [R, H*Dh] float64, unit [R, H*Dh]) -- decode_contract's attn unit:
    u (1 + A) sum_j p_j |v_ji|. Only keys j < Lk and only the batches the index names are touched."""
    R = q.shape[0]
    idx = gather_index(R, Lk, group, anc)
    j = torch.arange(Lk)[None, :].expand(R, Lk)
    K = k[idx, j].double()          # [R, Lk, H, Dh]
    V = v[idx, j].double()
    qd = q.double()
    s = torch.einsum("bhd,bjhd->bhj", qd, K) * scale
    A = torch.einsum("bhd,bjhd->bhj", qd.abs(), K.abs()) * scale * dc.L2E
    if key_tokens is not None:
        pad = key_tokens[idx, j] == pad_idx
        s = s.masked_fill(pad[:, None, :], -math.inf)
        A = A.masked_fill(pad[:, None, :], 0.0)
    p = torch.softmax(s, -1)
    o = torch.einsum("bhj,bjhd->bhd", p, V)
    unit = ULP * (1 + A.max(-1).values)[..., None] * torch.einsum("bhj,bjhd->bhd", p.nan_to_num(0.0), V.abs())
    return o.reshape(R, -1), unit.reshape(R, -1)


# ------------------------------------------------------------------------------------------------
# the algorithm over the pinned oracle
# ------------------------------------------------------------------------------------------------
def rank_slots(scores, lengths, length_penalty=0.0):
    """slot order of the final ranking: score / length**length_penalty descending, ties to the lower slot"""
    return sorted(range(len(scores)), key=lambda k: (-(scores[k] / max(lengths[k], 1) ** length_penalty), k))


@torch.no_grad()
def beam_search_reference(params, memory, dec, start, end, K, max_len, pad=0):
    """Beam search of ONE image (memory [1, S, d]) over oracle.ref_cpu.decoder_forward, every live beam's prefix
    recomputed in full each step (float64 scores on the oracle's float32 logits). Returns a dict:
      steps: per step the state after it -- ids (K lists, START first), score [K], finished [K], length [K],
             parent [K], margin (the step's decision margin)
      ids: the final K id lists cut as DecodeState.token_lists cuts them; score, length: the final state;
      margin: the smallest step margin."""
    from oracle import ref_cpu
    ids = [[start] for _ in range(K)]
    score = [0.0] + [NEG_INF] * (K - 1)
    fin, length = [0] * K, [0] * K
    steps = []
    for p in range(max_len - 1):
        live = [k for k in range(K) if not fin[k]]
        if not live:
            break
        rows = {}
        if live:
            toks = torch.tensor([ids[k] for k in live])
            lg = ref_cpu.decoder_forward(params, toks, memory.expand(len(live), -1, -1), heads=dec["heads"],
                                         layers=dec["layers"], max_len=dec.get("max_seq_len", 100))[:, -1]
            rows = {k: lg[i] for i, k in enumerate(live)}
        V = next(iter(rows.values())).shape[0]
        logits = torch.full((K, V), NAN)
        for k, r in rows.items():
            logits[k] = r
        tok = torch.zeros(K, p + 2, dtype=torch.int64)
        anc = torch.zeros(K, p + 2, dtype=torch.int32)
        ref = select_reference(logits, torch.tensor(score, dtype=torch.float64), torch.tensor(fin), torch.tensor(length),
                               tok, anc, p, K, end, pad)
        par, tk = ref["parent"].tolist(), ref["token"].tolist()
        ids = [ids[par[k]] + [tk[k]] for k in range(K)]
        score, fin, length = ref["score"].tolist(), ref["finished"].tolist(), ref["length"].tolist()
        steps.append(dict(ids=[list(x) for x in ids], score=list(score), finished=list(fin), length=list(length),
                          parent=par, margin=ref["margin"]))
    out = []
    for row in ids:
        row = row + [pad] * (max_len - len(row))
        if end in row[1:]:
            row = row[: row.index(end, 1) + 1]
        out.append(row)
    return dict(steps=steps, ids=out, score=score, length=length, finished=fin,
                margin=min(s["margin"] for s in steps))


# the end-to-end inputs whose every decision margin is above TAU (tests/test_beam_contract_cpu.py checks it)
E2E_FIXTURE = "tiny_vit_patches"
E2E_START, E2E_MAX_LEN = 2, 16
E2E_CASES = [(3, 69), (3, 79), (3, -1), (4, 69), (4, 79), (4, -1)]   # (K, END; -1: never produced)


def e2e_images(FX):
    meta, _ = FX.load(E2E_FIXTURE)
    img = FX.inputs(meta, 0)[0]
    return torch.cat([img, img.flip(-1), img * 0.5])[:4].contiguous()


_E2E = {}


def e2e_reference(FX, K, end):
    """[per image beam_search_reference] for the end-to-end inputs, computed once per (K, end)"""
    from oracle import ref_cpu
    if (K, end) not in _E2E:
        meta, _ = FX.load(E2E_FIXTURE)
        st = FX.state(meta)
        enc, dec = FX.enc_desc(meta), FX.dec_desc(meta)
        if "mem" not in _E2E:
            with torch.no_grad():
                _E2E["mem"] = ref_cpu.memory_from_features(st, ref_cpu.encode(st, e2e_images(FX), enc), meta["mode"])
        mem = _E2E["mem"]
        _E2E[(K, end)] = [beam_search_reference(st, mem[i:i + 1], dec, E2E_START, end, K, E2E_MAX_LEN)
                          for i in range(mem.shape[0])]
    return _E2E[(K, end)]


if __name__ == "__main__":
    for mode, (f, cid) in emulation_figures().items():
        print(f"select score, float32 emulation, {mode}: worst {f:.3f} ({cid})")
