"""Gradient clipping by global norm -- what can be checked without a GPU: the float64 reference of tests/grad_clip_ref.py
against torch.nn.utils.clip_grad_norm_, that the kernel tests' inputs tell every wrong coefficient from the right one, the
new C symbols and their host-side argument checks, and the host-only behaviour of set_grad_clip / grad_norm (vitpe/optim.py)."""
import ctypes
import sys

import numpy as np
import pytest
import torch

import grad_clip_ref as R
from optim_host import cpu_optimizer
from vitpe import _lib


def _torch_clip(g, gs, max_norm, sizes):
    """clip_grad_norm_ on CPU, float64, over parameters of unequal size whose gradients are the pieces of g * gs."""
    full = torch.from_numpy(np.asarray(g, dtype=np.float64)) * gs
    assert sum(sizes) == full.numel()
    params = []
    for piece in torch.split(full, sizes):
        prm = torch.nn.Parameter(torch.zeros(piece.numel(), dtype=torch.float64))
        prm.grad = piece.clone()
        params.append(prm)
    norm = torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2.0, error_if_nonfinite=False)
    return float(norm), torch.cat([prm.grad for prm in params]).numpy()


@pytest.mark.parametrize("factor", [0.25, 1.0, 1e6])
def test_reference_agrees_with_torch_clip_grad_norm(factor):
    """max_norm below, equal to and far above the norm; the returned norm and the clipped gradients."""
    n, gs = 4099, 0.25
    g = R.with_marks(R.norm_inputs(n, seed=2), R.mark_groups(n)[1])
    norm0, _ = R.clip_ref(g, gs, 1.0)
    max_norm = factor * norm0
    norm, coef = R.clip_ref(g, gs, max_norm)
    t_norm, t_grad = _torch_clip(g, gs, max_norm, [1, 7, 4000, 64, 27])
    assert abs(norm - t_norm) <= 1e-14 * t_norm
    want = g.astype(np.float64) * gs * coef
    assert np.max(np.abs(want - t_grad)) <= 1e-14 * np.max(np.abs(t_grad))
    if factor < 1:
        assert abs(coef - factor) < 1e-3 and abs(np.linalg.norm(t_grad) - max_norm) < 1e-3 * max_norm
    elif factor == 1.0:
        assert 1 - 1e-3 < coef < 1.0          # the 1e-6 keeps it just under 1: torch scales here too
    else:
        assert coef == 1.0 and np.array_equal(t_grad, g.astype(np.float64) * gs)


# the factor at which each wrong variant must show on EVERY input of the kernel test (at the other one it may coincide
# with the right coefficient: without the clamp nothing changes while max_norm is below the norm, and so on)
SHOWS_AT = {"unscaled_norm": 0.5, "no_eps": 0.5, "no_clamp": 4.0, "squared_norm": 0.5}


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_kernel_test_inputs_tell_each_wrong_coefficient_from_the_right_one(variant):
    """On the inputs of test_grad_clip_gpu.py (gs = 0.25; every size, every run of marked elements; at 2^20 + 3 the bulk
    alone, the first two and the last run, the others differ from those only in which 4096-boundaries are marked) the
    wrong coefficient is at least 100 x the kernel test's tolerance away from the right one, relative."""
    assert R.GS == 0.25 and SHOWS_AT[variant] in R.FACTORS
    worst = np.inf
    for n in R.SIZES:
        base = R.norm_inputs(n)
        groups = R.mark_groups(n)
        if len(groups) > 6:
            groups = groups[:3] + groups[-1:]
        tol = max(R.norm_bound(n, mis) for mis in (0, 1))
        for marks in groups:
            g = R.with_marks(base, marks)
            norm, _ = R.clip_ref(g, R.GS, 1.0)
            max_norm = SHOWS_AT[variant] * norm
            _, right = R.clip_ref(g, R.GS, max_norm)
            _, wrong = R.clip_ref(g, R.GS, max_norm, variant=variant)
            worst = min(worst, abs(wrong - right) / right / tol)
    print(f"{variant}: smallest |wrong - right| / right = {worst:.1f} x the tolerance")
    assert worst >= 100.0


def test_marked_elements_carry_a_tenth_of_the_sum_each():
    for n in R.SIZES:
        base = R.norm_inputs(n)
        groups = R.mark_groups(n)
        assert groups[0] == [] and all(1 <= len(m) <= R.GROUP for m in groups[1:])
        flat = [i for m in groups for i in m]
        assert len(flat) == len(set(flat)) and n - 1 in flat and 0 in flat
        assert all(k in flat for k in range(0, n, 4096)) and all(i in flat for i in (1, 2, 3, 4) if i < n)
        for marks in (groups[1], groups[-1]):
            g = R.with_marks(base, marks).astype(np.float64)
            assert all(g[i] ** 2 >= 0.10 * np.sum(g * g) for i in marks)
    # the derived tolerance stays below the issue's ceiling at every size and alignment
    assert max(R.norm_bound(n, mis) for n in R.SIZES for mis in range(4)) <= 1e-5
    assert R.chain_length(2 ** 20 + 3, 0) == 4 + 11 and R.chain_length(1, 1) == 11


def test_new_symbols_in_header_and_library():
    protos = _lib.parse_header()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("vitpe_grad_clip", 6), ("vitpe_grad_clip_blocks", 1), ("vitpe_adamw_step", 9)):
        assert name in protos and len(protos[name]) == nargs
        assert hasattr(handle, name)
    assert protos["vitpe_grad_clip"][1] is ctypes.c_longlong and protos["vitpe_grad_clip"][4] is ctypes.c_int
    assert protos["vitpe_grad_clip_blocks"] == [ctypes.c_longlong]
    h = _lib.lib()
    # the grid rule: min(1024, ceil(n / 4096)), a function of n alone
    for n, nb in ((0, 0), (-5, 0), (1, 1), (4096, 1), (4097, 2), (2 ** 20 + 3, 257), (4096 * 1024, 1024), (10 ** 9, 1024),
                  (2 ** 33, 1024)):
        assert h.vitpe_grad_clip_blocks(n) == nb
    # pure host argument checks: refused before anything touches a device (the non-null values are never dereferenced)
    fake = 4096
    assert h.vitpe_grad_clip(None, 1, None, None, 1, None) == 1
    assert h.vitpe_grad_clip(None, 1, fake, fake, 1, None) == 1          # no gradient
    assert h.vitpe_grad_clip(fake, 1, None, fake, 1, None) == 1          # no hp
    assert h.vitpe_grad_clip(fake, 1, fake, None, 1, None) == 1          # no work buffer
    assert h.vitpe_grad_clip(fake, -1, fake, fake, 1, None) == 1         # n < 0
    assert h.vitpe_grad_clip(fake, 4097, fake, fake, 1, None) == 1       # the grid needs 2 partials
    assert h.vitpe_grad_clip(fake + 2, 8, fake, fake, 1, None) == 1      # not 4-byte aligned
    assert h.vitpe_grad_clip(None, 0, None, None, 0, None) == 1          # n == 0 still writes hp


def test_set_grad_clip_refuses_bad_values_and_grad_norm_needs_the_clip_on():
    opt, dropped = cpu_optimizer()
    for bad in (-1, -1e-9, float("nan"), float("inf"), float("-inf")):
        with pytest.raises(_lib.VitpeError, match="set_grad_clip"):
            opt.set_grad_clip(bad)
    assert opt.clip_max_norm is None
    with pytest.raises(_lib.VitpeError, match="clipping is off"):
        opt.grad_norm()
    # off -> off: nothing to allocate, nothing to drop, no device needed
    opt.set_grad_clip(None)
    opt.set_grad_clip(0)
    opt.set_grad_clip(0.0)
    assert opt.clip_max_norm is None and dropped == []
    with pytest.raises(_lib.VitpeError, match="clipping is off"):
        opt.grad_norm()


def test_train_py_clip_grad_flag():
    sys.path.insert(0, _lib.REPO_ROOT)
    import train
    assert train.get_args([]).clip_grad == 0.0
    assert train.get_args(["--clip_grad", "1.5"]).clip_grad == 1.5
    for bad in ("-1", "nan", "inf"):
        with pytest.raises(SystemExit):
            train.get_args(["--clip_grad", bad])
