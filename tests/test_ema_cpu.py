"""Weight EMA -- what can be checked without a GPU: the float64 reference of tests/ema_ref.py is self-consistent, the new C
symbols and their host-side argument checks, the host-only argument handling of TrainEngine.set_ema / ema_weights, and
train.py's two flags."""
import ctypes
import functools
import sys

import numpy as np
import pytest

import ema_ref as R
from optim_host import cpu_optimizer
from vitpe import _lib


# ------------------------------------------------------------------------------------------ the reference
def test_equal_inputs_are_a_fixed_point_of_the_reference():
    p, e = R.ema_inputs(4099, seed=1)
    for d in (0.0, 0.5, 0.9, 0.9999):
        out = R.ema_ref(e, e, d)
        assert np.array_equal(out, e.astype(np.float64))
        assert np.all(R.ema_bound(e, e, out, d) == R.U * np.abs(e.astype(np.float64)))
    # d = 0 copies p, a decay next to 1 barely moves e; between them the result lies between e and p
    assert np.array_equal(R.ema_ref(p, e, 0.0), p.astype(np.float64))
    mid = R.ema_ref(p, e, 0.9)
    lo, hi = np.minimum(p, e).astype(np.float64), np.maximum(p, e).astype(np.float64)
    assert np.all((mid >= lo) & (mid <= hi))
    assert R.lerp_weight(0.9) == float(np.float32(1.0) - np.float32(0.9)) != 1.0 - 0.9


def test_inputs_stay_in_the_range_the_bound_needs():
    p, e = R.ema_inputs(R.SWEEP + 4099, seed=0)
    for x in (p, e):
        assert x.dtype == np.float32 and np.abs(x).min() >= 2.0 ** -10 and np.abs(x).max() <= 2.0 ** 4
    for n in R.SIZES + (R.SWEEP + 4099,):
        pm, em, kinds = R.with_marks(p[:n], e[:n])
        flat = [i for k in kinds.values() for i in k]
        assert len(flat) == len(set(flat)) == len(R.mark_indices(n))
        assert all(pm[i] == em[i] for i in kinds["equal"]) and all(em[i] == 0 for i in kinds["e_zero"])
        assert all(pm[i] == 0 for i in kinds["p_zero"])
        if n >= 3:
            assert all(len(k) >= 1 for k in kinds.values()) and n - 1 in flat and 0 in flat
    assert R.SWEEP in R.mark_indices(R.SWEEP + 4099) and 4 * ((R.SWEEP + 4099) // 4) in R.mark_indices(R.SWEEP + 4099)


@pytest.mark.parametrize("decay", [0.5, 0.9, 0.999, 0.9999])
def test_warmup_decay_is_monotone_and_reaches_the_decay(decay):
    ts = [1, 2, 3, 5, 10, 100, 1000, 10 ** 4, 10 ** 5, 10 ** 6]
    ds = [float(R.warmup_decay(decay, t)) for t in ts]
    assert all(a <= b for a, b in zip(ds, ds[1:]))
    assert ds[0] == float(np.float32(2.0) / np.float32(11.0)) and ds[-1] == float(np.float32(decay))
    assert all(0.0 < d <= float(np.float32(decay)) for d in ds)
    # the ramp crosses the decay where (1 + t) / (10 + t) = decay: t* = (10 decay - 1) / (1 - decay)
    t_star = (10 * decay - 1) / (1 - decay)
    assert t_star >= 8
    assert float(R.warmup_decay(decay, int(0.9 * t_star))) < float(np.float32(decay))
    assert float(R.warmup_decay(decay, int(1.1 * t_star) + 2)) == float(np.float32(decay))


# ------------------------------------------------------------------------------------------ the C boundary
def test_new_symbols_in_header_and_library():
    protos = _lib.parse_header()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("vitpe_ema_update", 6), ("vitpe_ema_swap", 5), ("vitpe_ema_blocks", 1)):
        assert name in protos and len(protos[name]) == nargs
        assert hasattr(handle, name)
    assert protos["vitpe_ema_update"][3] is ctypes.c_longlong and protos["vitpe_ema_update"][4] is ctypes.c_int
    assert protos["vitpe_ema_swap"][3] is ctypes.c_longlong
    h = _lib.lib()
    # the grid rule: one lane per 4 elements, 256 lanes per workgroup, capped at 256 x 8; a function of n alone
    for n, nb in ((0, 0), (-5, 0), (1, 1), (3, 1), (1024, 1), (1028, 2), (4099, 4), (R.SWEEP, R.GRID_CAP),
                  (R.SWEEP - 1024, R.GRID_CAP - 1), (R.SWEEP + 4099, R.GRID_CAP), (2 ** 33, R.GRID_CAP)):
        assert h.vitpe_ema_blocks(n) == nb, n
    # pure host argument checks: refused before anything touches a device (the non-null values are never dereferenced)
    fake = 4096
    assert h.vitpe_ema_update(fake, fake, None, 8, 0, None) == 1          # no hp
    assert h.vitpe_ema_update(None, None, None, 0, 0, None) == 1          # ... also at n == 0
    assert h.vitpe_ema_update(None, fake, fake, 8, 0, None) == 1          # no p
    assert h.vitpe_ema_update(fake, None, fake, 8, 1, None) == 1          # no e
    assert h.vitpe_ema_update(fake, fake, fake, -1, 0, None) == 1         # n < 0
    assert h.vitpe_ema_update(fake + 4, fake, fake, 8, 0, None) == 1      # p not 16-byte aligned
    assert h.vitpe_ema_update(fake, fake + 8, fake, 8, 1, None) == 1      # e not 16-byte aligned
    assert h.vitpe_ema_update(None, None, fake, 0, 0, None) == 0          # n == 0: nothing to launch
    assert h.vitpe_ema_swap(None, fake, None, 8, None) == 1
    assert h.vitpe_ema_swap(fake, None, None, 8, None) == 1
    assert h.vitpe_ema_swap(fake, fake, None, -1, None) == 1
    assert h.vitpe_ema_swap(fake + 4, fake, None, 8, None) == 1
    assert h.vitpe_ema_swap(fake, fake + 12, None, 8, None) == 1
    assert h.vitpe_ema_swap(fake, fake, fake + 2, 8, None) == 1           # the bf16 shadow as well
    assert h.vitpe_ema_swap(None, None, None, 0, None) == 0


# ------------------------------------------------------------------------------------------ TrainEngine, host side
class _HostEngine:
    """TrainEngine's methods over a StepOptimizer alone: what they do before they touch the model or a device.  The stand-in
    has `opt` and nothing else, so this only works for methods whose FIRST statement is their opt.guard / opt.needs_ema
    call -- which is what these tests assert; a method that read anything else of the engine first would fail here with
    an AttributeError, not pass."""

    def __init__(self, opt):
        self.opt = opt

    def __getattr__(self, name):
        from vitpe.engine import TrainEngine
        return functools.partial(getattr(TrainEngine, name), self)


def test_set_ema_argument_handling_without_a_device():
    from vitpe.optim import ema_value
    opt, dropped = cpu_optimizer()
    eng = _HostEngine(opt)
    for bad in (-0.1, 1.0, float("nan"), 1.5, float("inf"), -1e-9):
        with pytest.raises(_lib.VitpeError, match="set_ema"):
            eng.set_ema(bad)
        with pytest.raises(_lib.VitpeError, match="set_ema"):
            eng.set_ema(bad, warmup=True)
    assert opt.ema_decay is None and opt.flat_e is None and opt.ema_warmup is False
    # off -> off: nothing to allocate, nothing to drop, no device needed
    eng.set_ema(None)
    eng.set_ema(0)
    eng.set_ema(0.0, warmup=True)              # (a warm-up of nothing stays off)
    assert opt.ema_decay is None and opt.ema_warmup is False and dropped == []
    # the accepted values, as far as host logic goes
    assert ema_value(None) is None and ema_value(0) is None and ema_value(0.999) == 0.999
    assert ema_value(np.float32(0.5)) == 0.5
    # what needs the average refuses while it is off
    for call in (eng.reset_ema, eng.ema_state_dict, lambda: eng.load_ema_state_dict({})):
        with pytest.raises(_lib.VitpeError, match="EMA is off"):
            call()
    with pytest.raises(_lib.VitpeError, match="EMA is off"):
        with eng.ema_weights():
            pass


def test_training_calls_refuse_inside_the_swapped_state():
    opt, _ = cpu_optimizer()
    opt.ema_decay, opt.ema_swapped = 0.9, True          # as inside `with eng.ema_weights():`
    eng = _HostEngine(opt)
    for name, call in (("step", eng.step), ("step_indexed", lambda: eng.step_indexed(None)),
                       ("forward_backward", eng.forward_backward), ("capture", eng.capture),
                       ("set_ema", lambda: eng.set_ema(0.5)), ("reset_ema", eng.reset_ema)):
        with pytest.raises(_lib.VitpeError, match=name + ": not available inside ema_weights"):
            call()
    with pytest.raises(_lib.VitpeError, match="ema_weights: not available inside ema_weights"):
        with eng.ema_weights():
            pass


def test_train_py_model_ema_flags():
    sys.path.insert(0, _lib.REPO_ROOT)
    import train
    args = train.get_args([])
    assert args.model_ema == 0.0 and args.model_ema_warmup is False
    args = train.get_args(["--model_ema", "0.999", "--model_ema_warmup"])
    assert args.model_ema == 0.999 and args.model_ema_warmup is True
    for bad in (["--model_ema", "1.5"], ["--model_ema", "1.0"], ["--model_ema", "-0.1"], ["--model_ema", "nan"],
                ["--model_ema_warmup"]):
        with pytest.raises(SystemExit):
            train.get_args(bad)
