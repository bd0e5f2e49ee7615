"""Gradient accumulation on the GPU: mit_grad_accumulate bit for bit against torch's f32 add, and
ImageToTextModel.train_step_accum against (i) the reference's single-process step at the whole batch
(tests/golden/dp2_tiny: B = 8, unequal PAD per half) for three splits of that batch, (ii) train_step itself
(one micro-batch; a batch padded to the longer T), (iii) itself (determinism, prefetch, record / replay),
then train_one_epoch(accum_steps=k) and the data-parallel step (two gloo ranks on the one GPU).
The reference tolerances are those tests/test_dist_gpu.py applies to the same quantities."""
import os

import pytest
import torch
import torch.multiprocessing as mp

import fixtures as FX
from gemm_contract import SENTINEL, Buf

pytestmark = pytest.mark.gpu

P = FX.P
I32 = torch.int32


# ------------------------------------------------------------------------------------------------
# the kernel
# ------------------------------------------------------------------------------------------------
def _grid_cap():
    import native
    return native.grad_accumulate_blocks(1 << 40)


def _big():
    """The sizes are 1, 3 (tail only), 4 (one vector), 1027 (two blocks, tail of 3), and this one: n % 4 == 3
    past a single trip of the grid-stride loop. The launch is capped at mit_grad_accumulate_blocks(huge) blocks
    of 256 threads x 4 floats (4096 blocks = 4 Mi floats = 16 MiB a buffer), so n = that + 4 * 1027 + 3 sends
    the first 1027 threads of the grid on a second trip, the rest on one, and leaves a 3-element tail."""
    big = _grid_cap() * 256 * 4 + 4 * 1027 + 3
    assert big % 4 == 3 and big // 4 > _grid_cap() * 256
    return big


def _values(n, seed):
    """Mixed magnitudes 1e-3 .. 1e3, both signs."""
    g = torch.Generator().manual_seed(seed)
    mag = torch.pow(10.0, torch.rand(n, generator=g) * 6 - 3)
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    return (mag * sign).float()


def _pair(n):
    """(grad, acc) values with a few NaN / inf: NaN + x, inf + x, -inf + x, inf + -inf (-> NaN), at vector and
    tail positions. No index holds a NaN in BOTH operands (which payload survives is not defined)."""
    grad, acc = _values(n, 11), _values(n, 12)
    nan, inf = float("nan"), float("inf")
    for i, (gv, av) in {1: (nan, None), 2: (None, inf), 3: (-inf, None), 5: (-inf, inf), 1024: (nan, None),
                        1025: (None, nan), n - 1: (None, -inf)}.items():
        if 0 < i < n:
            if gv is not None:
                grad[i] = gv
            if av is not None:
                acc[i] = av
    return grad, acc


def _same_f32(got, want, what):
    """Bit for bit, NaN at the same places (an f32 add defines that a NaN comes out, not which)."""
    gn, wn = torch.isnan(got), torch.isnan(want)
    assert torch.equal(gn, wn), f"{what}: NaN at different places"
    g, w = got.contiguous().view(I32), want.contiguous().view(I32)
    assert torch.equal(torch.where(gn, 0, g), torch.where(wn, 0, w)), f"{what}: differs bitwise"


def _bufs(n, grad, acc):
    G = Buf(1, n, n, torch.float32, SENTINEL, 0, "cuda", grad.view(1, n))
    A = Buf(1, n, n, torch.float32, SENTINEL, 0, "cuda", acc.view(1, n))
    G.snapshot()
    A.snapshot()
    return G, A


@pytest.mark.parametrize("n", [1, 3, 4, 1027, "past_one_trip"])
@pytest.mark.parametrize("mode", ["first", "add", "last"])
def test_grad_accumulate_bitwise(n, mode):
    import native
    n = _big() if n == "past_one_trip" else n
    grad, acc = _pair(n)
    G, A = _bufs(n, grad, acc)
    g0, a0 = G.view.reshape(-1).clone(), A.view.reshape(-1).clone()
    want = a0 + g0  # torch's f32 add on the same device
    native.grad_accumulate(G.view, A.view, {"first": native.ACC_FIRST, "add": native.ACC_ADD,
                                            "last": native.ACC_LAST}[mode], n=n)
    torch.cuda.synchronize()
    G.check_untouched("grad")
    A.check_untouched("acc")
    got_g, got_a = G.view.reshape(-1), A.view.reshape(-1)
    if mode == "first":
        G.check_unchanged("grad")
        assert torch.equal(got_a.view(I32), g0.view(I32)), "acc is not a bitwise copy of grad"
    elif mode == "add":
        G.check_unchanged("grad")
        _same_f32(got_a, want, "acc = acc0 + grad")
    else:
        A.check_unchanged("acc")
        _same_f32(got_g, want, "grad = acc + grad0")
    if n >= 4:
        assert torch.isnan(want).any() and torch.isinf(want).any()


def test_grad_accumulate_chain_is_left_to_right():
    import native
    n = 1027
    g0, g1, g2 = (_values(n, s).cuda() for s in (21, 22, 23))
    G, A = _bufs(n, g0.cpu(), torch.full((n,), float("nan")))  # acc needs no zero-fill: FIRST overwrites it
    native.grad_accumulate(G.view, A.view, native.ACC_FIRST, n=n)
    G.view.copy_(g1.view(1, n))
    native.grad_accumulate(G.view, A.view, native.ACC_ADD, n=n)
    G.view.copy_(g2.view(1, n))
    native.grad_accumulate(G.view, A.view, native.ACC_LAST, n=n)
    torch.cuda.synchronize()
    assert torch.equal(G.view.reshape(-1).view(I32), ((g0 + g1) + g2).view(I32))
    G.check_untouched("grad")
    A.check_untouched("acc")


# ------------------------------------------------------------------------------------------------
# the accumulated step
# ------------------------------------------------------------------------------------------------
def _dp2(step=0):
    meta, T = FX.load("dp2_tiny")
    imgs = P.make_images(meta["B"], meta["image_size"], meta["seed"] + 1 + 100 * step).cuda()
    cap = P.make_captions(meta["B"], meta["cap_len"], meta["dec"]["vocab"], meta["seed"] + 2 + 100 * step,
                          meta["lengths"])
    return meta, T, imgs, cap[:, :-1].contiguous().cuda(), cap[:, 1:].contiguous().cuda()


def _model(meta, dtype, dropout=0.0):
    import optim
    from model_util import build_model
    m, _ = build_model(meta, dtype, dropout=dropout)
    m.train()
    opt = optim.AdamW(m.store, lr=meta["lr"], betas=tuple(meta["betas"]), eps=meta["eps"],
                      weight_decay=meta["weight_decay"])
    return m, opt


def _micro(imgs, di, tg, bounds):
    return [(imgs[a:b], di[a:b], tg[a:b]) for a, b in bounds]


def _step(m, opt, meta, run):
    """run() -> loss, then optimizer.step: (loss, flat gradient before the step, [norm, coef], update by name)."""
    names = FX.trainable_names(meta)
    before = {k: v.clone() for k, v in m.state_dict().items() if k in names}
    loss = run()
    torch.cuda.synchronize()
    grad = m.store.grad.clone().cpu()
    opt.step(meta["clip"])
    torch.cuda.synchronize()
    after = m.state_dict()
    return loss.item(), grad, opt.norm_t.cpu().tolist(), {k: (after[k] - before[k]).cpu() for k in names}


def _check_reference(meta, T, loss, grad, norm, deltas):
    from test_dist_gpu import _check_against_reference
    total, coef = norm
    print(f"loss {loss:.7f} (reference {T['loss'].item():.7f}), norm {total:.6f} "
          f"(reference {T['grad_total_norm_preclip'].item():.6f})")
    assert abs(loss - T["loss"].item()) < 1e-4
    assert abs(total - T["grad_total_norm_preclip"].item()) < 1e-3 * total
    _check_against_reference(meta, T, grad.numpy(), coef, deltas)


SPLITS = {"halves": [(0, 4), (4, 8)], "four_of_2": [(0, 2), (2, 4), (4, 6), (6, 8)], "uneven_3_5": [(0, 3), (3, 8)]}


@pytest.mark.parametrize("split", sorted(SPLITS))
def test_accumulated_step_matches_reference_global_batch(split):
    """The uneven split passes only when every micro-batch's CE divides by the TOTAL non-PAD count."""
    meta, T, imgs, di, tg = _dp2()
    m, opt = _model(meta, torch.float32)
    mbs = _micro(imgs, di, tg, SPLITS[split])
    loss, grad, norm, deltas = _step(m, opt, meta, lambda: m.train_step_accum(mbs))
    assert m.store.accum is not None and m.store.accum.numel() == m.store.numel
    _check_reference(meta, T, loss, grad, norm, deltas)


def _state(m, opt):
    st = m.store
    return dict(grad=st.grad, master=st.master, exp_avg=st.exp_avg, exp_avg_sq=st.exp_avg_sq, seed=m.seed_t,
                step=opt.step_t)


def _assert_bitwise(a, b, keys=None):
    for k in keys or a:
        x, y = a[k], b[k]
        if x.dtype == torch.float32:
            x, y = x.view(I32), y.view(I32)
        assert torch.equal(x, y), k


def test_one_micro_batch_is_train_step():
    meta, T, imgs, di, tg = _dp2()
    (m1, o1), (m2, o2) = _model(meta, torch.bfloat16, 0.1), _model(meta, torch.bfloat16, 0.1)
    l1 = m1.train_step(imgs, di, tg).clone()
    o1.step(meta["clip"])
    l2 = m2.train_step_accum([(imgs, di, tg)]).clone()
    o2.step(meta["clip"])
    torch.cuda.synchronize()
    assert torch.equal(l1.view(I32), l2.view(I32))
    _assert_bitwise(_state(m1, o1), _state(m2, o2))
    assert m2.store.accum is None  # not allocated before a step over several micro-batches


def test_accumulated_step_is_deterministic_and_advances_the_seed_per_micro_batch():
    meta, T, imgs, di, tg = _dp2()
    bounds = [(0, 3), (3, 6), (6, 8)]
    out = []
    for _ in range(2):
        m, opt = _model(meta, torch.bfloat16, 0.1)
        seed0 = int(m.seed_t.item())
        loss = m.train_step_accum(_micro(imgs, di, tg, bounds)).clone()
        opt.step(meta["clip"])
        torch.cuda.synchronize()
        assert int(m.seed_t.item()) - seed0 == 3
        out.append((loss, _state(m, opt)))
    assert torch.equal(out[0][0].view(I32), out[1][0].view(I32))
    _assert_bitwise(out[0][1], out[1][1])


def test_micro_batches_draw_different_dropout_masks():
    """Two micro-batches holding the same data x: the total count doubles, so the step's gradient is
    g(x, mask 1) / 2 + g(x, mask 2) / 2. Had both drawn mask 1 it would equal train_step(x)'s gradient bit for
    bit (halving and x/2 + x/2 are exact); with dropout 0.1 at every site the two differ by far more than any
    rounding (asserted: over 1 % of the gradient's norm)."""
    meta, T, imgs, di, tg = _dp2()
    (m1, _), (m2, _) = _model(meta, torch.bfloat16, 0.1), _model(meta, torch.bfloat16, 0.1)
    m1.train_step(imgs, di, tg)
    m2.train_step_accum([(imgs, di, tg), (imgs, di, tg)])
    torch.cuda.synchronize()
    g1, g2 = m1.store.grad.double(), m2.store.grad.double()
    rel = ((g2 - g1).norm() / g1.norm()).item()
    print(f"relative difference {rel:.4f}")
    assert rel > 1e-2


def _as_fixture(meta, grad, coef, deltas):
    """A step's clipped gradient and update in the fixture's layout (grad1.full.* / delta1.full.*), so that
    FX.compare_stat checks another step against it exactly as it checks one against the reference."""
    from decoder import decoder_entries, flat_to_reference
    from params import FlatParams
    dec, enc = FX.dec_desc(meta), FX.enc_desc(meta)
    E = enc["hidden"]
    store = FlatParams(decoder_entries(dec["vocab"], dec["d"], dec["layers"], dec["ff"],
                                       E if E != dec["d"] else None), torch.device("cpu"), torch.float32)
    store.grad.copy_(grad)

    class GV:
        vocab = dec["vocab"]

        def p(self, n):
            return store.g(n)

    named = flat_to_reference(GV(), dec["layers"], dec["d"])
    if "projection.weight" in store.index:
        named["projection.weight"] = store.g("projection.weight")
        named["projection.bias"] = store.g("projection.bias")
    out = {}
    for k in FX.trainable_names(meta):
        out[f"grad1.full.{k}"] = (named[k] * coef).clone()
        if deltas is not None:
            out[f"delta1.full.{k}"] = deltas[k].clone()
    return out


def test_micro_batches_of_different_length_match_the_padded_batch():
    """Captions of 12 and 20 positions as two micro-batches against ONE train_step on the batch padded to
    T = 20 (PAD keys are masked, PAD targets ignored): the dp2_tiny tolerances, relative to that run."""
    meta, T, imgs, _, _ = _dp2()
    V = meta["dec"]["vocab"]
    ca = P.make_captions(4, 13, V, 501, [13, 9, 5, 11])
    cb = P.make_captions(4, 21, V, 502, [21, 14, 3, 17])
    full = torch.zeros(8, 21, dtype=torch.int64)
    full[:4, :13] = ca
    full[4:] = cb
    ca, cb, full = ca.cuda(), cb.cuda(), full.cuda()
    m1, o1 = _model(meta, torch.float32)
    ref = _step(m1, o1, meta, lambda: m1.train_step(imgs, full[:, :-1].contiguous(), full[:, 1:].contiguous()))
    m2, o2 = _model(meta, torch.float32)
    mbs = [(imgs[:4], ca[:, :-1].contiguous(), ca[:, 1:].contiguous()),
           (imgs[4:], cb[:, :-1].contiguous(), cb[:, 1:].contiguous())]
    got = _step(m2, o2, meta, lambda: m2.train_step_accum(mbs))
    print(f"loss {got[0]:.7f} vs {ref[0]:.7f}, norm {got[2][0]:.6f} vs {ref[2][0]:.6f}")
    assert abs(got[0] - ref[0]) < 1e-4
    assert abs(got[2][0] - ref[2][0]) < 1e-3 * ref[2][0]
    R = _as_fixture(meta, ref[1], ref[2][1], ref[3])
    G = _as_fixture(meta, got[1], got[2][1], None)
    for k in FX.trainable_names(meta):
        FX.compare_stat("grad1", k, G[f"grad1.full.{k}"], R, meta, rtol=2e-3, atol=2e-6, scale_tol=1e-3,
                        outlier_frac=2e-3)
        FX.compare_stat("delta1", k, got[3][k], R, meta, rtol=2e-3, atol=2e-6)


def test_prefetch_of_the_next_step_does_not_change_results():
    meta, T, imgs, di, tg = _dp2()
    _, _, imgs2, di2, tg2 = _dp2(step=1)
    steps = [_micro(imgs, di, tg, [(0, 4), (4, 8)]), _micro(imgs2, di2, tg2, [(0, 4), (4, 8)])]
    out = []
    for prefetch in (False, True):
        m, opt = _model(meta, torch.bfloat16, 0.1)
        losses = []
        for i, mbs in enumerate(steps):
            nxt = steps[i + 1][0][0] if prefetch and i + 1 < len(steps) else None
            losses.append(m.train_step_accum(mbs, next_images=nxt).clone())
            opt.step(meta["clip"])
        torch.cuda.synchronize()
        out.append((torch.cat(losses), _state(m, opt)))
    assert torch.equal(out[0][0].view(I32), out[1][0].view(I32))
    _assert_bitwise(out[0][1], out[1][1])


def test_recorded_accumulated_steps_replay_like_eager_ones():
    """tests/test_dist_gpu.py::_replay_worker without the process group: step 1 eager; steps 2-3 recorded by
    native.record (two micro-batches + optimizer.step each; the default guard rejects any torch kernel);
    replayed as steps 4-5 on new data copied into the same input tensors. A second model runs five eager
    steps on the same data. bf16, dropout 0.1: the replays must advance the dropout seed and the AdamW step
    as eager steps do."""
    import native
    meta = FX.load("dp2_tiny")[0]
    data = [_dp2(step=s)[2:] for s in range(5)]
    runs = {}
    for mode in ("eager", "replay"):
        m, opt = _model(meta, torch.bfloat16, 0.1)
        static = [t.clone() for t in data[0]]
        mbs = _micro(*static, [(0, 4), (4, 8)])
        held = {}

        def load(s):
            for dst, src in zip(static, data[s]):
                dst.copy_(src)

        def step():
            held["loss"] = m.train_step_accum(mbs)
            opt.step(meta["clip"])

        losses = []
        if mode == "eager":
            for s in range(5):
                load(s)
                step()
                losses.append(held["loss"].item())
        else:
            load(0)
            step()
            losses.append(held["loss"].item())
            progs = []
            for s in (1, 2):
                load(s)
                progs.append(native.record(step))
                losses.append(held["loss"].item())
            assert progs[0].launches() > 0
            for i, s in enumerate((3, 4)):
                load(s)
                opt._sync_lr()
                progs[i].run()
                losses.append(held["loss"].item())
        torch.cuda.synchronize()
        runs[mode] = (losses, {k: v.clone() for k, v in _state(m, opt).items() if k != "grad"})
    (le, se), (lr, sr) = runs["eager"], runs["replay"]
    assert le == lr, (le, lr)
    assert len(set(le)) == 5, le
    assert int(se["step"].item()) == 5
    _assert_bitwise(se, sr)


# ------------------------------------------------------------------------------------------------
# train_one_epoch
# ------------------------------------------------------------------------------------------------
def _loader(meta, n, B):
    out = []
    for s in range(n):
        imgs = P.make_images(B, meta["image_size"], meta["seed"] + 31 + s)
        cap = P.make_captions(B, meta["cap_len"], meta["dec"]["vocab"], meta["seed"] + 41 + s,
                              [meta["lengths"][(i + s) % len(meta["lengths"])] for i in range(B)])
        out.append({"images": imgs, "decoder_input_tokens": cap[:, :-1].contiguous(),
                    "target_tokens": cap[:, 1:].contiguous()})
    return out


def _halves(batches):
    out = []
    for b in batches:
        h = b["images"].shape[0] // 2
        out += [{k: v[:h] for k, v in b.items()}, {k: v[h:] for k, v in b.items()}]
    return out


def test_train_one_epoch_accumulates_half_batches_like_whole_ones():
    import train
    meta = FX.load("dp2_tiny")[0]
    names = FX.trainable_names(meta)
    whole = _loader(meta, 2, 8)
    runs = []
    for loader, k in ((whole, 1), (_halves(whole), 2)):
        m, opt = _model(meta, torch.float32)
        before = {n: v.clone() for n, v in m.state_dict().items() if n in names}
        grads, inner = [], opt.step

        def step(max_norm=0.0):
            grads.append(m.store.grad.clone().cpu())
            inner(max_norm)

        opt.step = step
        loss = train.train_one_epoch(m, loader, opt, None, "cuda", meta["clip"], None, 0, 0, None, accum_steps=k)
        after = m.state_dict()
        assert int(opt.step_t.item()) == 2 and len(grads) == 2
        runs.append((loss, {n: (after[n] - before[n]).cpu() for n in names}, grads, m))
    (l1, d1, g1, m1), (l2, d2, _, _) = runs
    print(f"epoch loss {l2:.7f} (accumulated) vs {l1:.7f}")
    assert abs(l1 - l2) <= 2e-3 * abs(l1), (l1, l2)
    # the update of two steps against the whole-batch run's, as delta1 is checked against the reference's:
    # elements whose gradient stayed under compare_stat's pinning floor in either step are not pinned
    floor = torch.minimum(g1[0].abs(), g1[1].abs())
    R = _as_fixture(meta, floor, 1.0, d1)
    for n in names:
        FX.compare_stat("delta1", n, d2[n], R, meta, rtol=2e-3, atol=2e-6)


def test_train_one_epoch_short_last_group_and_errors():
    import train
    meta = FX.load("dp2_tiny")[0]
    m, opt = _model(meta, torch.float32)
    loader = _loader(meta, 5, 2)
    train.train_one_epoch(m, loader, opt, None, "cuda", meta["clip"], None, 0, 0, None, accum_steps=2)
    assert int(opt.step_t.item()) == 3  # groups of 2, 2, 1
    with pytest.raises(ValueError):
        train.train_one_epoch(m, loader, opt, None, "cuda", meta["clip"], None, 0, 0, None, accum_steps=0)
    with pytest.raises(ValueError):  # a non-fused optimizer
        train.train_one_epoch(m, loader, torch.optim.AdamW(m.parameters(), lr=1e-4), None, "cuda", meta["clip"], None,
                              0, 0, None, accum_steps=2)
    with pytest.raises(ValueError):  # a criterion the fused step does not compute
        train.train_one_epoch(m, loader, opt, torch.nn.CrossEntropyLoss(ignore_index=0, label_smoothing=0.1), "cuda",
                              meta["clip"], None, 0, 0, None, accum_steps=2)
    assert int(opt.step_t.item()) == 3


# ------------------------------------------------------------------------------------------------
# data parallel
# ------------------------------------------------------------------------------------------------
def _dp_worker(rank, world, port, q):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (here, os.path.join(here, "..", "multimodal-image-transformer_amd"), os.path.join(here, "golden")):
        sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from dist import DataParallel
        meta, T, imgs, di, tg = _dp2()
        m, opt = _model(meta, torch.float32)
        dp = DataParallel(m, overlap=True)
        calls, inner = [], dp.all_reduce_grads

        def counted():
            calls.append(1)
            inner()

        dp.all_reduce_grads = counted
        half = meta["B"] // world
        lo = rank * half
        mbs = _micro(imgs, di, tg, [(lo, lo + 2), (lo + 2, lo + 4)])
        loss, grad, norm, deltas = _step(m, opt, meta, lambda: m.train_step_accum(mbs, dist=dp))
        if rank == 0:
            # numpy (pickled by value): the worker may exit before the parent reads the queue
            q.put((loss, grad.numpy(), norm, {k: v.numpy() for k, v in deltas.items()}, len(calls)))
    finally:
        dist.destroy_process_group()


def test_dp2_accumulated_step_matches_reference():
    """Two gloo ranks on cuda:0, each its half of dp2_tiny as two micro-batches of two rows: one count
    all-reduce, one all-reduce of the whole flat gradient after the last accumulate, one of the loss."""
    from test_dist_gpu import _free_port
    meta, T = FX.load("dp2_tiny")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    loss, grad, norm, deltas, n_reduces = q.get(timeout=240)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert n_reduces == 1
    _check_reference(meta, T, loss, torch.from_numpy(grad), norm, {k: torch.from_numpy(v) for k, v in deltas.items()})
