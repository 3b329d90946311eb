"""The polynomial relative position bias at every degree 0-7, the part that needs no GPU: the reference of the GPU tests
(poly_degree_ref.py) is pinned to autograd through the oracle, every deliberately wrong variant of it is shown to lie far
outside the gate the GPU tests apply, and every case is on the route it names.

The degree refusals (PETables with degree -1 or 8) are in test_poly_degree_gpu.py: the host wrappers refuse a CPU tensor
before the library sees the degree, so pe_ok cannot be reached here the way test_attn_probs_cpu.py reaches the library."""
import pytest
import torch

import poly_degree_ref as R
from oracle import vit_oracle as O

F64 = torch.float64


@pytest.mark.parametrize("per_head", [False, True])
@pytest.mark.parametrize("degree", range(8))
def test_closed_form_gradient_is_autograd_through_the_oracle(degree, per_head):
    """g_k = sum dS d^k (and the forward, and dqkv) against autograd through oracle.polynomial_bias / attention_core"""
    B, G, H, hd = 2, 3, 2, 8
    N, D = G * G + 1, H * hd
    qkv = R.rnd(B, N, 3 * D, seed=degree + 1).to(F64).requires_grad_(True)
    dout = R.rnd(B, N, D, seed=degree + 20).to(F64)
    coeff = R.coeffs(degree, G, H, per_head, degree + 40).to(F64).requires_grad_(True)
    bias = O.polynomial_bias(coeff, N - 1, H, degree, not per_head)
    assert float((bias.detach() - R.bias_ref(coeff.detach(), H, G, per_head)).abs().max()) < 1e-14
    q, k, v = qkv.reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    out = O.attention_core(q, k, v, hd ** -0.5, None, bias).transpose(1, 2).reshape(B, N, D)
    dqkv, g = torch.autograd.grad(out, [qkv, coeff], dout)
    r = R.core_ref(qkv.detach(), dout, H, G, coeff.detach(), per_head)
    assert r.g.shape == coeff.shape
    assert float((r.out - out.detach()).abs().max()) < 1e-13
    assert float((r.dqkv - dqkv).abs().max()) < 1e-13
    assert float((r.g - g).abs().max()) <= 1e-12 * float(r.A.max())
    # the stand-alone bias backward's closed form, on the gradient autograd hands the bias
    # the stand-alone bias backward's closed form, on an arbitrary gradient of the materialised bias
    dbias = R.rnd(H, N, N, seed=degree + 60).to(F64)
    gb, ab = R.bias_bwd_ref(dbias, G, degree, per_head)
    lv = coeff.detach().clone().requires_grad_(True)
    (O.polynomial_bias(lv, N - 1, H, degree, not per_head) * dbias).sum().backward()
    assert float((gb - lv.grad).abs().max()) <= 1e-12 * float(ab.max())


@pytest.mark.parametrize("case", R.EXACT_CASES + R.FAR_CASES, ids=R.case_id)
def test_every_wrong_variant_is_far_outside_the_exact_gate(case):
    """For every exact case of the GPU file: each wrong variant differs from the reference in at least one component by at
    least 64 x 2^-23 E_k, four times the cap on the GPU gate; an fp32 evaluation of the same formulas stays inside it."""
    c = R.exact_case(*case)
    r = R.exact_ref(c)
    assert bool((r.E > 0).all())
    want = {"class_row", "class_col", "power_plus_one"} | ({"above_3_dropped"} if c.degree > 3 else set()) \
        | ({"heads_swapped"} if c.per_head and c.H > 1 else set()) | ({"stride_4"} if c.per_head and c.H > 1 and c.degree != 3 else set())
    assert set(r.wrong) == want
    worst = {name: float(((w - r.g).abs() / (R.EPS32 * r.E)).max()) for name, w in r.wrong.items()}
    print(f"{R.case_id(case)}: separation {worst}")
    assert min(worst.values()) >= R.SEPARATION, worst
    # the two class masks are what the small powers depend on most: a missing mask shows in EVERY power, the constant included
    for name in ("class_row", "class_col"):
        per_k = (r.wrong[name] - r.g).abs() / (R.EPS32 * r.E)
        assert float(per_k.min()) >= R.SEPARATION, (name, per_k)
    # the gate is reachable: dS and the sums formed in fp32 by torch
    P, q32 = r.probs.float(), c.qkv.float()
    v = q32.reshape(c.B, c.N, 3, c.H, c.hd).permute(2, 0, 3, 1, 4)[2]
    dP = c.dout.float().reshape(c.B, c.N, c.H, c.hd).transpose(1, 2) @ v.transpose(-2, -1)
    dS = P * (dP - (P * dP).sum(-1, keepdim=True))
    dS[:, :, 0, :] = 0
    dS[:, :, :, 0] = 0
    g32 = torch.einsum("bhij,kij->hk", dS.to(F64), R.powers(c.G, c.degree + 1))
    g32 = g32 if c.per_head else g32.sum(0)
    assert R.excess(g32, r.g, R.EPS32 * r.E) < 1.0


def test_every_case_is_on_the_route_it_names():
    for case in R.EXACT_CASES + R.FAR_CASES:
        assert R.pin(*case[:5])
    assert R.pin(*R.WIDE_GEOM) and R.pin(*R.FUSED64_GEOM)
    for wrong in [("core", "bf16", 17, 96, 2), ("fused", "bf16", 26, 64, 2), ("core_hd", "f32", 17, 64, 2),
                  ("fused64", "bf16", 65, 192, 6)]:
        with pytest.raises(AssertionError, match="left its route"):
            R.pin(*wrong)
    # both bf16 fused-backward instantiations and both sides of their degree switch are in the list
    degs = {c[5] for c in R.EXACT_CASES if c[0] == "fused" and c[1] == "bf16"}
    assert {0, 3} <= degs and {4, 7} <= degs
