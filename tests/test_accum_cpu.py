"""Gradient accumulation without a GPU: mit_grad_accumulate's argument checks (they run before any launch),
the batch grouping of train_one_epoch, and the optimizer-step count train.main hands to its schedule."""
import ctypes

import pytest


def _lib():
    import native
    return native.load_library()


def _err(lib):
    return lib.mit_last_error() or b""


# an address that is never dereferenced: every call below is rejected, or returns, before a launch
A16 = 0x10000


def test_binding_loads_and_declares_the_entry_points_without_gpu():
    import native
    lib = _lib()
    for name in ("mit_grad_accumulate", "mit_grad_accumulate_blocks"):
        assert name in native.SIGNATURES and hasattr(lib, name)
    assert (native.ACC_FIRST, native.ACC_ADD, native.ACC_LAST) == (0, 1, 2)
    assert native.ABI_VERSION == lib.mit_abi_version()


@pytest.mark.parametrize("grad,acc,mode,what", [
    (None, A16, 0, b"null"),
    (A16, None, 1, b"null"),
    (A16 + 4, 2 * A16, 0, b"aligned"),
    (A16, 2 * A16 + 4, 2, b"aligned"),
    (A16, 2 * A16, -1, b"mode"),
    (A16, 2 * A16, 3, b"mode"),
])
def test_grad_accumulate_rejects_by_return_code(grad, acc, mode, what):
    lib = _lib()
    rc = lib.mit_grad_accumulate(1024, grad, acc, mode, None)
    assert rc == 1
    assert b"mit_grad_accumulate" in _err(lib) and what in _err(lib), _err(lib)


def test_grad_accumulate_rejects_negative_n_and_overlap():
    lib = _lib()
    assert lib.mit_grad_accumulate(-1, A16, 2 * A16, 0, None) == 1
    assert b"mit_grad_accumulate" in _err(lib)
    # 1024 floats from A16 and 1024 floats from A16 + 1024 bytes share bytes (only rejections run here: an
    # accepted n > 0 would launch)
    assert lib.mit_grad_accumulate(1024, A16, A16 + 1024, 1, None) == 1
    assert b"overlap" in _err(lib)
    assert lib.mit_grad_accumulate(1024, A16, A16, 2, None) == 1


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_grad_accumulate_n_zero_is_ok_without_a_launch(mode):
    assert _lib().mit_grad_accumulate(0, A16, 2 * A16, mode, None) == 0


def test_grad_accumulate_blocks_query():
    lib = _lib()
    assert lib.mit_grad_accumulate_blocks(0) == 0 and lib.mit_grad_accumulate_blocks(-5) == 0
    assert lib.mit_grad_accumulate_blocks(1) == 1
    assert lib.mit_grad_accumulate_blocks(1027) == 2  # 256 f32x4 + 3 tail elements: two blocks of 256 threads
    cap = lib.mit_grad_accumulate_blocks(1 << 40)
    assert cap == lib.mit_grad_accumulate_blocks(1 << 41) and cap >= 256  # capped: larger n loops grid-stride


def test_micro_groups():
    from train import micro_groups
    assert list(micro_groups(range(4), 1)) == [[0], [1], [2], [3]]
    assert [len(g) for g in micro_groups(range(7), 3)] == [3, 3, 1]
    assert list(micro_groups(range(7), 3)) == [[0, 1, 2], [3, 4, 5], [6]]
    assert list(micro_groups(iter(()), 2)) == []
    with pytest.raises(ValueError):
        micro_groups(range(3), 0)
    with pytest.raises(ValueError):
        micro_groups(range(3), -2)


def test_optimizer_steps_count_handed_to_the_schedule():
    """ceil(batches / k) * epochs: 5 batches by 2 are 3 optimizer steps an epoch."""
    import train
    assert train.optimizer_steps(5, 2, 3) == 9
    assert train.optimizer_steps(20, 1, 2) == 40
    assert train.optimizer_steps(4, 8, 1) == 1
    with pytest.raises(ValueError):
        train.optimizer_steps(5, 0, 1)


def test_main_hands_the_optimizer_step_count_to_linear_warmup(monkeypatch):
    """train.main builds its schedule before it touches any data: stop it there and read the total."""
    import config
    import train

    class Stop(Exception):
        pass

    seen = {}

    class Model:
        def __init__(self, *a, **k):
            pass

        def parameters(self):
            return []

    def warmup(opt, warm, total):
        seen["total"] = total
        raise Stop

    monkeypatch.setattr(train, "ImageToTextModel", Model)
    monkeypatch.setattr(train.optim, "AdamW", lambda *a, **k: object())
    monkeypatch.setattr(train, "LinearWarmup", warmup)
    monkeypatch.setattr(config, "WARMUP_STEPS", 2)
    import dist
    monkeypatch.setattr(dist, "init_from_env", lambda *a, **k: (0, 1))
    with pytest.raises(Stop):
        train.main(["--batches", "5", "--accum-steps", "2", "--epochs", "3"])
    assert seen["total"] == 9


def test_accum_steps_option():
    import config
    import train
    ap = train.build_parser()
    assert config.GRAD_ACCUM_STEPS == 1
    assert ap.parse_args([]).accum_steps == config.GRAD_ACCUM_STEPS
    assert ap.parse_args(["--accum-steps", "4"]).accum_steps == 4
    assert ap.parse_args(["--accum-steps", "4"]).batch_size == config.BATCH_SIZE
    with pytest.raises(ValueError):
        train.main(["--accum-steps", "0"])
