"""The inputs and the reference of tests/ln_ref.py, checked without a GPU, producer by producer:

  * the variance condition: eps / 8 <= v <= 8 eps for >= 90 % of the rows every statistic is taken of, and a mean of the
    order of the standard deviation;
  * discrimination: the reference recomputed with the WRONG eps (the 1e-5 default where another value is passed, 0 where
    1e-5 is passed; eps2 / eps_next swapped for the block tail) moves rstd of EVERY row by >= 100x its gate (1e-4, both
    dtypes) and the fp32 normalised output by >= 100x the 1e-4 gate.  A bf16 normalised output is gated at 3e-2; 100x that
    is a change of 300 %, which a too-large eps cannot cause (it only shrinks the rows): there the condition is >= 10x the
    gate, and the statistics, gated at 1e-4 in bf16 as well, carry the 100x;
  * a plain fp32 torch restatement (for the bf16-only block tail: float64 with the kernel's bf16 rounding points) stays
    inside those gates, so the reference alone leaves a correct implementation inside them.
"""
import pytest
import torch

import ln_ref as R

DTS = ["f32", "bf16"]


def moved(wrong, right):
    return R.rel(wrong, right)


def rstd_moved(rows, eps, other):
    return float((R.stats(rows, other)[2] / R.stats(rows, eps)[2] - 1).abs().min())


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("eps", R.EPS_SWEEP)
@pytest.mark.parametrize("M,D", R.LAYERNORM_SHAPES)
def test_layernorm_inputs(dt, eps, M, D):
    x, g, b = R.layernorm_inputs(dt, M, D, eps)
    assert R.variance_condition(x, eps) >= 0.9 and R.mean_is_of_the_order_of_sigma(x)
    y = R.layer_norm(x, g, b, eps)
    assert moved(R.layer_norm(x, g, b, R.wrong_eps(eps)), y) >= (R.POWER * R.F32_TOL if dt == "f32" else R.POWER_BF16 * R.BF16_TOL)
    assert rstd_moved(x, eps, R.wrong_eps(eps)) >= R.POWER * R.STAT_TOL         # every single row
    assert R.rel(R.layer_norm(x, g, b, eps, torch.float32), y) < R.F32_TOL / 10
    xf = x.float()
    m32 = xf.mean(-1)
    r32 = 1.0 / torch.sqrt(((xf - m32[:, None]) ** 2).mean(-1) + eps)
    em, er = R.stat_errors(m32, r32, x, eps)
    assert em < R.STAT_TOL / 10 and er < R.STAT_TOL / 10


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("eps", R.EPS_SWEEP)
@pytest.mark.parametrize("M,N,K", R.LINEAR_SHAPES)
def test_linear_statistics_inputs(dt, eps, M, N, K):
    a, w, bias, resid = R.linear_inputs(dt, M, N, K, eps)
    c = R.linear_ref(a, w, bias, resid)
    for rows in (c, R.q(c.float(), dt)):                          # the exact rows and what a kernel stores of them
        assert R.variance_condition(rows, eps) >= 0.9 and R.mean_is_of_the_order_of_sigma(rows)
        assert rstd_moved(rows, eps, R.wrong_eps(eps)) >= R.POWER * R.STAT_TOL
    c32 = a @ w.t() + bias + resid
    assert R.rel(c32, c) < R.F32_TOL / 10


@pytest.mark.parametrize("M,HID,eps2,eps_next", R.TAIL2_CASES + [(B, HID, e, 100 * e) for B, HID, e in R.TAIL_CLS_CASES])
def test_block_tail_inputs(M, HID, eps2, eps_next):
    ins = R.tail2_inputs(M, HID, eps2, eps_next)
    assert eps_next > eps2
    ref = R.tail2_ref(ins, eps2, eps_next)
    kern = R.tail2_ref(ins, eps2, eps_next, stored=R.bf)          # float64 with the kernel's bf16 rounding points
    for t in (ref, kern):
        assert R.variance_condition(t["x_mid"], eps2) >= 0.9 and R.variance_condition(t["out"], eps_next) >= 0.9
        assert R.mean_is_of_the_order_of_sigma(t["x_mid"]) and R.mean_is_of_the_order_of_sigma(t["out"])
    # eps2 / eps_next swapped, and each replaced by what a kernel that ignores it would use
    for e2, en in ((eps_next, eps2), (R.wrong_eps(eps2), R.wrong_eps(eps_next))):
        assert float((R.stats(ref["x_mid"], e2)[2] / ref["rstd2"] - 1).abs().min()) >= R.POWER * R.STAT_TOL
        assert float((R.stats(ref["out"], en)[2] / ref["rstd_out"] - 1).abs().min()) >= R.POWER * R.STAT_TOL
        assert moved(R.tail2_ref(ins, e2, eps_next)["xn"], ref["xn"]) >= R.POWER_BF16 * R.BF16_TOL
    # what a correct bf16 kernel leaves: inside the gates of the normalised rows and of the two stored tensors
    for k in ("x_mid", "xn", "out"):
        assert R.rel(kern[k], ref[k]) < R.BF16_TOL / 2, k


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("eps", R.EPS_SWEEP)
@pytest.mark.parametrize("C,S,p,D,ape", R.PATCH_EMBED_CASES)
def test_patch_embed_inputs(dt, eps, C, S, p, D, ape):
    img, w, bias, cls, apet = R.patch_embed_inputs(dt, C, S, p, D, ape, eps)
    tok = R.patch_embed_ref(dt, img, w, bias, cls, apet, p)
    for rows in (tok, R.q(tok.float(), dt)):
        for part in (rows[:, :1], rows[:, 1:]):                   # the class-token row and the patch rows, separately
            assert R.variance_condition(part, eps) >= 0.9 and R.mean_is_of_the_order_of_sigma(part)
            assert rstd_moved(part, eps, R.wrong_eps(eps)) >= R.POWER * R.STAT_TOL
    tok32 = R.unfold(R.q(img, dt), p) @ w.t() + bias + (apet if apet is not None else 0)
    assert R.rel(tok32, tok[:, 1:]) < R.F32_TOL / 10
