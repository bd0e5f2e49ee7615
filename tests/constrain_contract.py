"""Contract helpers of the logit-constraint kernel (csrc/constrain.hip, mit_logits_constrain) and of the constrained
decodes built on it.

  constrain_reference   one row of the header's contract restated in float32 numpy: repetition penalty, no-repeat
                        n-gram, minimum length, suppress list, forced token, in that order. Every changed value is one
                        float32 multiply, -inf or 0.0, so the restatement is BITWISE: no tolerance appears anywhere at
                        kernel level.
  CASES / make_case     guarded buffers (decode_contract.Tensors): NaN ld padding, NaN rows of finished rows,
                        sentinels around and inside every input the kernel must not write
  oracle_greedy         the constrained greedy decode over oracle.ref_cpu.decoder_forward, with the top-1 / top-2
                        margin of every free step after the constraints and the float64 log_softmax of every
                        constrained row at the picked token
"""
import zlib
from dataclasses import dataclass, field

import numpy as np
import torch

import decode_contract as dc
import sample_contract as sc
from decode_contract import INT_SENT, NAN

NEG_INF = np.float32("-inf")
TAU = sc.TAU                    # the project's fp32 logit bound


# ------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------
def constrain_reference(row, history, theta=1.0, n=0, min_length=0, end=-1, suppress=(), forced_token=-1):
    """row: float32 [V] (the ld padding cut off), history: the ids h[0 .. p], START included; forced_token: the
    forced table's entry for column p + 1 where it applies, else -1. Returns the edited float32 row."""
    out = np.array(row, dtype=np.float32, copy=True)
    V = out.shape[0]
    h = [int(t) for t in history]
    p = len(h) - 1
    if 0 <= int(forced_token) < V:                      # 5. overrides 1 to 4
        out[:] = NEG_INF
        out[int(forced_token)] = np.float32(0.0)
        return out
    th = np.float32(theta)
    if th != np.float32(1.0):                           # 1. each distinct token once, from its original value
        rinv = np.float32(1.0) / th
        for v in sorted(set(t for t in h if 0 <= t < V)):
            l = np.float32(row[v])
            out[v] = l * rinv if l > 0 else l * th
    if n > 0 and p + 1 >= n:                            # 2.
        g = h[p - n + 2:p + 1]
        for i in range(0, p - n + 2):
            if h[i:i + n - 1] == g and 0 <= h[i + n - 1] < V:
                out[h[i + n - 1]] = NEG_INF
    if p < min_length and 0 <= end < V:                 # 3.
        out[end] = NEG_INF
    for v in suppress:                                  # 4.
        if 0 <= int(v) < V:
            out[int(v)] = NEG_INF
    return out


# ------------------------------------------------------------------------------------------------
# kernel cases
# ------------------------------------------------------------------------------------------------
CON_V = (7, 509, 512, 10000)
CON_R = (1, 5)
CON_THETA = (1.0, 1.3, 0.8)
CON_N = (0, 1, 2, 3, 4)
SPECIALS = (0.0, -0.0, -2.5, 1.75, float("-inf"))      # values the history's tokens hold in a row


@dataclass
class ConCase:
    id: str
    R: int
    V: int
    p: int
    theta: float = 1.0
    n: int = 0
    min_length: int = 0
    sup: str = "none"           # none | overlap (history tokens, END, ids outside [0, V))
    forced: str = "none"        # none | free (-1 in column p + 1) | banned (a banned token) | beyond (p + 1 >= ld_forced)
    ld_tok: int = 0             # 0: p + 4
    group: int = 1              # > 1: a non-trivial ancestor table
    alphabet: int = 5           # distinct in-range tokens the histories are drawn from
    x: dict = field(default_factory=dict)


def _geometry(V):
    # 7: ld = 10; 509: an odd vocabulary on a misaligned base; 512 / 10000: ld == V on an aligned base
    return dict(ld_pad=0 if V in (512, 10000) else 3, mis=1 if V == 509 else 0)


def _cases():
    cs, i = [], 0
    for V in CON_V:
        for R in CON_R:
            for theta in CON_THETA:
                for n in CON_N:
                    ps = sorted({0, 1, max(n - 2, 0), max(n - 1, 0), 20})
                    p = ps[i % len(ps)]
                    ml = (0, p + 1, p)[i % 3]                       # off; p = min_length - 1 (banned); p = min_length
                    sup = ("none", "overlap")[(i // 2) % 2]
                    forced = ("none", "free", "banned", "beyond")[(i // 3) % 4]
                    if forced == "banned":
                        sup = "overlap"
                    cs.append(ConCase(f"con-V{V}-R{R}-t{theta}-n{n}-p{p}-ml{ml}-{sup}-{forced}", R, V, p, theta, n, ml,
                                      sup, forced))
                    i += 1
    for n in CON_N[1:]:     # both sides of p + 1 >= n, with everything else on
        for p in sorted({max(n - 2, 0), n - 1}):
            cs.append(ConCase(f"con-edge-n{n}-p{p}", 5, 509, p, 1.3, n, p + 1, "overlap", "none"))
    cs += [
        # more history than a workgroup has threads
        ConCase("con-long-p300-V10000", 5, 10000, 300, 1.3, 3, 301, "overlap", "free", ld_tok=512, alphabet=12),
        ConCase("con-long-p300-V509-n1", 2, 509, 300, 0.8, 1, 0, "none", "none", ld_tok=512, alphabet=40),
        ConCase("con-long-p299-V512-forced", 5, 512, 299, 1.3, 2, 0, "overlap", "banned", ld_tok=512, alphabet=12),
        # ancestry: a history that crosses slots
        ConCase("con-anc-g3-V509", 6, 509, 20, 1.3, 2, 21, "overlap", "none", group=3),
        ConCase("con-anc-g8-V10000", 16, 10000, 20, 0.8, 3, 0, "overlap", "free", group=8),
        ConCase("con-anc-g3-V7-p300", 3, 7, 300, 1.3, 4, 0, "none", "none", ld_tok=512, group=3),
        ConCase("con-anc-g8-V512-forced", 8, 512, 5, 1.3, 2, 6, "overlap", "banned", group=8),
        ConCase("con-allfinished-V7", 3, 7, 4, 1.3, 2, 5, "overlap", "banned"),
        ConCase("con-off-V509", 5, 509, 20, 1.0, 0, 0, "none", "none"),        # nothing to do: nothing written
    ]
    return cs


CASES = _cases()
BY_ID = {c.id: c for c in CASES}


def case_history(tok, anc, group, r, p):
    """h[0 .. p] of row r (numpy int64 [R, ld_tok], int32 [R, ld_anc] or None)"""
    if anc is None:
        return tok[r, :p + 1].tolist()
    g0 = (r // group) * group
    return [int(tok[g0 + int(anc[r, j]), j]) for j in range(p + 1)]


def make_case(c):
    """The case's guarded tensors on the CPU; t.x: the expected rows (float32 [R, V], None for finished rows) and
    geometry. Histories come from a small alphabet (duplicates and repeated n-grams abound) with ids >= V and < 0
    mixed in; the row holds SPECIALS at the alphabet's tokens."""
    R, V, p = c.R, c.V, c.p
    geo = _geometry(V)
    ld = V + geo["ld_pad"]
    ld_tok = c.ld_tok or p + 4
    g = torch.Generator().manual_seed(zlib.crc32(c.id.encode()))
    alpha = torch.randperm(V, generator=g)[:min(c.alphabet, V)]
    pool = torch.cat([alpha, torch.tensor([V, V + 3, -5])])            # out-of-range ids never index the row
    wts = torch.cat([torch.full((alpha.numel(),), 1.0), torch.full((3,), 0.25)])
    tok = torch.full((R, ld_tok), INT_SENT, dtype=torch.int64)
    tok[:, :p + 1] = pool[torch.multinomial(wts, R * (p + 1), replacement=True, generator=g)].view(R, p + 1)
    tok[:, p + 1:] = int(alpha[0])                                       # past p: never read (would ban / penalise)
    end_id = int(alpha[1 % alpha.numel()])
    lg = torch.randn(R, V, generator=g) * 3.0
    for r in range(R):
        for k, a in enumerate(alpha.tolist()):
            lg[r, a] = SPECIALS[(k + r) % len(SPECIALS)]
    fin = torch.zeros(R, dtype=torch.int32)
    if c.id.startswith("con-allfinished"):
        fin[:] = 1
    elif R >= 5:
        fin[3] = 1
    lg[fin != 0] = NAN
    anc = None
    if c.group > 1:
        anc = torch.randint(0, c.group, (R, ld_tok), generator=g, dtype=torch.int32)
        anc[:, p + 1:] = INT_SENT                                        # never read
    suppress = []
    if c.sup == "overlap":
        suppress = [int(alpha[0]), end_id, V + 1, -3, int(alpha[-1]), (int(alpha[0]) + 1) % V]
    ld_forced = 0
    forced = None
    if c.forced != "none":
        ld_forced = p + 1 if c.forced == "beyond" else p + 3
        forced = torch.randint(0, V, (R, ld_forced), generator=g)        # other columns: tokens that must not apply
        if c.forced == "free":
            forced[:, p + 1] = -1
            if R > 1:
                forced[1, p + 1] = V + 2                                 # outside [0, V): free as well
        elif c.forced == "banned":
            forced[:, p + 1] = suppress[0]
            if R > 2:
                forced[2, p + 1] = -1                                    # a free row among forced ones
    t = dc.Tensors()
    a = t.new("logits", R * ld, torch.float32, NAN, margin=ld + 8, misalign=geo["mis"])
    a.win(0, R, V, ld).copy_(lg)
    t.new("tok", R * ld_tok, torch.int64, INT_SENT, margin=ld_tok).win(0, R, ld_tok, ld_tok).copy_(tok)
    t.new("pos", 1, torch.int64, INT_SENT, margin=8).base[0] = p
    if R > 1 or c.id.startswith("con-allfinished"):                      # R == 1: finished is NULL (every row live)
        t.new("finished", R, torch.int32, INT_SENT, margin=8).base[:R] = fin
    if anc is not None:
        t.new("anc", R * ld_tok, torch.int32, INT_SENT, margin=ld_tok).win(0, R, ld_tok, ld_tok).copy_(anc)
    if suppress:
        t.new("suppress", len(suppress), torch.int64, INT_SENT, margin=8).base[:len(suppress)] = torch.tensor(suppress)
    if forced is not None:
        t.new("forced", R * ld_forced, torch.int64, INT_SENT, margin=ld_forced).win(0, R, ld_forced, ld_forced) \
            .copy_(forced)
    tok_n = tok.numpy()
    anc_n = anc.numpy() if anc is not None else None
    want, hist = [], []
    for r in range(R):
        if int(fin[r]):
            want.append(None)
            hist.append(None)
            continue
        h = case_history(tok_n, anc_n, c.group, r, p)
        f = int(forced[r, p + 1]) if forced is not None and p + 1 < ld_forced else -1
        want.append(constrain_reference(lg[r].numpy(), h, c.theta, c.n, c.min_length, end_id, suppress, f))
        hist.append(h)
        t.a["logits"].allow(r * ld, 1, V, ld)                            # a live row's V columns, nothing else
    t.x.update(ld=ld, ld_tok=ld_tok, ld_forced=ld_forced, end_id=end_id, n_suppress=len(suppress), want=want,
               hist=hist, fin=fin, logits=lg, suppress=suppress)
    return t


def gathered(c, t):
    """The ancestry case with every row's history gathered physically into tok and no table: the same rows"""
    g = dc.Tensors()
    g.a = dict(t.a)
    g.x = dict(t.x)
    R, p, ld_tok = c.R, c.p, t.x["ld_tok"]
    tok = torch.full((R, ld_tok), INT_SENT, dtype=torch.int64)
    for r in range(R):
        h = t.x["hist"][r]
        if h is not None:
            tok[r, :p + 1] = torch.tensor(h)
    a = dc.Arr(R * ld_tok, torch.int64, INT_SENT, margin=ld_tok)
    a.win(0, R, ld_tok, ld_tok).copy_(tok)
    g.a["tok"] = a
    del g.a["anc"]
    return g


def launch(N, c, t, use_anc=True):
    """mit_logits_constrain on the case's buffers through the raw C entry point"""
    anc = t.ptr("anc") if use_anc else None
    return N.lib().mit_logits_constrain(c.R, c.V, t.ptr("logits"), t.x["ld"], t.ptr("tok"), t.x["ld_tok"], t.ptr("pos"),
                                        c.group if anc else 1, anc, t.x["ld_tok"] if anc else 0, t.ptr("finished"),
                                        c.theta, c.n, c.min_length, t.x["end_id"], t.ptr("suppress"),
                                        t.x["n_suppress"], t.ptr("forced"), t.x["ld_forced"], None)


def check_case(c, t):
    """Live rows bitwise the reference's; everything else (ld padding, finished rows, every input) bitwise untouched"""
    R, V, ld = c.R, c.V, t.x["ld"]
    a = t.a["logits"]
    got = a.whole.detach().cpu()[a.off:a.off + R * ld].view(R, ld)[:, :V].numpy()
    for r in range(R):
        if t.x["want"][r] is None:
            continue
        w = t.x["want"][r]
        bad = np.nonzero(got[r].view(np.uint32) != w.view(np.uint32))[0]
        assert bad.size == 0, (f"{c.id}: row {r}: {bad.size} column(s) differ from the reference; first {int(bad[0])}: "
                               f"{got[r][bad[0]]!r} expected {w[bad[0]]!r} (was {t.x['logits'][r, int(bad[0])].item()!r})")
    for name, arr in t.a.items():
        arr.check(name)


# ------------------------------------------------------------------------------------------------
# the constrained greedy decode over the pinned oracle
# ------------------------------------------------------------------------------------------------
E2E_START, E2E_END, E2E_MAX_LEN = sc.E2E_START, sc.E2E_END, sc.E2E_MAX_LEN
# name -> generate_* keyword arguments (prompts are added by e2e_settings)
E2E_SETTINGS = {
    "off": dict(),
    "n2": dict(no_repeat_ngram_size=2),
    "theta1.3": dict(repetition_penalty=1.3),
    "minlen8": dict(min_length=8),
    "combined": dict(repetition_penalty=1.2, no_repeat_ngram_size=3, min_length=6, suppress_tokens=(0, 1, 2, 3)),
}


@torch.no_grad()
def oracle_greedy(FX, kw, prompts=None, max_len=E2E_MAX_LEN, rows=None):
    """Greedy decode of the end-to-end images over the CPU oracle with the constraints `kw` (generate_* keywords) and
    per-image `prompts` (lists, possibly empty). Returns per image dict(ids, margins, score): ids cut after END,
    margins = top-1 minus top-2 of every FREE step's constrained row, score = the float64 sum over the steps of
    log_softmax(constrained row)[token] (a forced step adds exactly 0)."""
    from oracle import ref_cpu
    st, dec, mem = sc.e2e_memory(FX)
    theta = kw.get("repetition_penalty", 1.0)
    n = kw.get("no_repeat_ngram_size", 0)
    ml = kw.get("min_length", 0)
    sup = kw.get("suppress_tokens", ())
    out = []
    for row in (range(mem.shape[0]) if rows is None else rows):
        pr = list(prompts[row]) if prompts else []
        ids, margins, score = [E2E_START], [], 0.0
        for p in range(max_len - 1):
            lg = ref_cpu.decoder_forward(st, torch.tensor([ids]), mem[row:row + 1], heads=dec["heads"],
                                         layers=dec["layers"], max_len=dec.get("max_seq_len", 100))[0, -1]
            f = pr[p] if p < len(pr) else -1
            c = constrain_reference(lg.float().numpy(), ids, theta, n, ml, E2E_END, sup, f)
            t = int(np.argmax(c))
            if f < 0:
                top = np.sort(c.astype(np.float64))[-2:]
                margins.append(float(top[1] - top[0]))
            score += float(torch.log_softmax(torch.from_numpy(c).double(), 0)[t])
            ids.append(t)
            if t == E2E_END:
                break
        out.append(dict(ids=ids, margins=margins, score=score))
    return out


_E2E = {}


def e2e_settings(FX):
    """{name: (keywords with prompts, oracle result per image)}. The combined setting gets per-image prompts: for
    image b the first two tokens (else the first one) after START of image (b + 1) % B's UNCONSTRAINED caption that
    are not END and for which every free step stays decided (margin > 2 TAU); an image whose candidates all fail
    decodes without a prompt."""
    if "s" in _E2E:
        return _E2E["s"]
    res = {}
    for name, kw in E2E_SETTINGS.items():
        if name != "combined":
            res[name] = (dict(kw), oracle_greedy(FX, kw))
    off = [r["ids"] for r in res["off"][1]]
    B = len(off)
    kw = E2E_SETTINGS["combined"]
    prompts, rows = [], []
    for b in range(B):
        src = [t for t in off[(b + 1) % B][1:] if t != E2E_END]
        best = None
        for cand in (src[:2], src[:1], []):
            if best is not None:
                continue
            r = oracle_greedy(FX, kw, {b: cand}, rows=[b])[0]
            if all(m > 2 * TAU for m in r["margins"]):
                best = (cand, r)
        assert best is not None, f"image {b}: the combined setting is undecided even without a prompt"
        prompts.append(best[0])
        rows.append(best[1])
    res["combined"] = (dict(kw, prompts=prompts), rows)
    _E2E["s"] = res
    return res
