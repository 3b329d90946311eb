"""The float64 head reference of tests/head_ref.py, checked without a GPU:

  * against torch.nn.functional autograd (layer_norm -> linear -> cross_entropy(reduction="sum") on the valid rows);
  * against the closed forms (equal head rows: CE = log Cn, arg-max = class 0, dlogits = (1 / Cn - onehot) grad_scale; a
    single class: loss 0, dlogits 0);
  * its inputs: the class rows' variance is within 8x of the eps passed, and a wrong eps (the 1e-5 default where another
    value is passed, 0 where 1e-5 is passed) moves logits and dx by >= 100x the GPU gate, so the GPU tests see eps;
  * a plain fp32 torch restatement of the same formulas stays inside every gate the GPU test applies (the reference alone
    leaves a correct fp32 implementation inside the gates, per image row as well);
  * the float64 class-row gradient rounded to bf16 satisfies the bf16 dx bound;
  * the case list launches every reachable instantiation of head_step_kernel in both dtypes;
  * a real vitpe.head.StepHead over CPU tensors: the control block set_valid writes, its defaults, refusals and caching.
"""
import math

import pytest
import torch

import head_ref as H

CASES = H.HEAD_STEP_CASES + [(dt, B, N, D, Cn, B, eps) for dt, B, N, D, Cn, eps in H.HEAD_FWD_BWD_CASES]
IDS = ["-".join(str(v) for v in c) for c in CASES]


def _case(c):
    dt, B, N, D, Cn, nv, eps = c
    ins = H.head_inputs(dt, B, N, D, Cn, eps)
    gs, ls, _ = H.scales(B, nv)
    return ins, H.head_ref(*ins, eps, nv, gs, ls), (gs, ls)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_reference_equals_torch_autograd(c):
    dt, B, N, D, Cn, nv, eps = c
    (x, g, b, wh, bh, labels), ref, (gs, ls) = _case(c)
    xr = x.double().requires_grad_(True)
    leaves = [t.double().requires_grad_(True) for t in (g, b, wh, bh)]
    y = torch.nn.functional.layer_norm(xr, (D,), leaves[0], leaves[1], eps)
    logits = torch.nn.functional.linear(y[:, 0], leaves[2], leaves[3])
    ce = torch.nn.functional.cross_entropy(logits[:nv], labels[:nv], reduction="sum") if nv else logits.sum() * 0
    (ce * gs).backward()                                   # d/dlogits = (softmax - onehot) grad_scale on the valid rows
    assert H.rel(ref["logits"], logits.detach()) < 1e-12
    assert abs(ref["loss"] - float(ce.detach()) * ls) <= 1e-12 * max(1.0, abs(ref["loss"]))
    assert ref["correct"] == int((logits[:nv].argmax(1) == labels[:nv]).sum()) if nv else ref["correct"] == 0
    assert float(xr.grad[:, 1:].abs().max()) == 0.0 if N > 1 else True
    for name, t in (("dx", xr.grad[:, 0]), ("dgamma", leaves[0].grad), ("dbeta", leaves[1].grad), ("dwh", leaves[2].grad),
                    ("dbh", leaves[3].grad)):
        assert H.rel(ref[name], t) < 1e-9, name
    assert float(ref["dlogits"][nv:].abs().max()) == 0.0 if nv < B else True


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_inputs_make_eps_decisive_and_fp32_is_inside_the_gates(c):
    dt, B, N, D, Cn, nv, eps = c
    (x, g, b, wh, bh, labels), ref, (gs, ls) = _case(c)
    assert H.variance_condition(x[:, 0], eps) >= 0.9
    m, s = x[:, 0].double().mean(1).abs(), x[:, 0].double().std(1, unbiased=False)
    assert bool(((m > 0.25 * s) & (m < 4 * s)).all())       # the mean is of the order of the standard deviation
    # the wrong eps
    wrong = H.head_ref(x, g, b, wh, bh, labels, 1e-5 if eps != 1e-5 else 0.0, nv, gs, ls)
    assert H.rel(wrong["logits"], ref["logits"]) >= 100 * H.TOL
    if nv > 0 and Cn > 1:
        assert H.rel(wrong["dx"], ref["dx"]) >= 100 * H.TOL
    # plain fp32
    f = H.head_ref(x, g, b, wh, bh, labels, eps, nv, gs, ls, dtype=torch.float32)
    assert H.rel(f["logits"], ref["logits"]) < H.TOL / 10 and H.row_rel(f["logits"], ref["logits"]) < H.TOL / 10
    assert H.rel(f["dlogits"], ref["dlogits"]) < H.TOL / 10 and H.row_rel(f["dlogits"], ref["dlogits"]) < H.TOL / 10
    assert H.loss_err(f["loss"], ref["loss"]) < H.LOSS_TOL / 10 and f["correct"] == ref["correct"]
    for name in ("dx", "dwh", "dbh", "dgamma", "dbeta"):
        assert H.rel(f[name], ref[name]) < H.TOL / 10, name
    # one rounding of the reference to bf16 is inside the bf16 bound of the class row (unit roundoff of bf16: 2^-8)
    assert H.dx_bf16_excess(ref["dx"].to(torch.bfloat16), ref["dx"]) <= 1.0


@pytest.mark.parametrize("Cn", [1, 2, 9, 17, 64])
@pytest.mark.parametrize("nv", [0, 3, 5])
def test_closed_forms(Cn, nv):
    B, D, eps = 5, 96, 1e-5
    x, g, b, wh, bh, labels = H.head_inputs("f32", B, 3, D, Cn, eps, seed=Cn)
    wh, bh = H.equal_rows_head(wh, bh)
    gs, ls, _ = H.scales(B, nv)
    ref = H.head_ref(x, g, b, wh, bh, labels, eps, nv, gs, ls)
    assert bool((ref["logits"] == ref["logits"][:, :1]).all())          # bit-identical logits per image
    assert abs(ref["loss"] - ls * nv * math.log(Cn)) < 1e-12
    assert ref["correct"] == int((labels[:nv] == 0).sum())
    onehot = torch.nn.functional.one_hot(labels, Cn).double()
    closed = (1.0 / Cn - onehot) * gs
    closed[nv:] = 0
    assert float((ref["dlogits"] - closed).abs().max()) < 1e-15
    if Cn == 1:
        assert ref["loss"] == 0.0 and float(ref["dlogits"].abs().max()) == 0.0 and float(ref["dx"].abs().max()) == 0.0


@pytest.mark.parametrize("B,Cn", H.CE_CASES)
def test_loss_reference_ties_and_shift(B, Cn):
    z, labels = H.tied_logits(B, Cn)
    assert bool(((z + 100).double() == z.double() + 100).all())         # the shift is exact in fp32
    ref = H.ce_ref(z, labels, B, H.f32(1.0 / B), H.f32(1.0 / B))
    loss = torch.nn.functional.cross_entropy(z.double(), labels, reduction="sum") * H.f32(1.0 / B)
    assert abs(ref["loss"] - float(loss)) < 1e-12 * max(1.0, abs(float(loss)))
    am = H.first_argmax(z)
    assert ref["correct"] == int((am == labels).sum())
    if Cn >= 2 and B >= 2:
        ties = (z == z.max(1, keepdim=True).values).sum(1)
        assert int((ties[0::4] == 2).all()) and bool((am[0::4] == labels[0::4]).all())       # tie after the label: correct
        assert int((ties[1::4] == 2).all()) and bool((am[1::4] < labels[1::4]).all())        # tie before the label: wrong
    sh = H.ce_ref(z + 100, labels, B, H.f32(1.0 / B), H.f32(1.0 / B))
    assert H.loss_err(sh["loss"], ref["loss"]) < 1e-12 and H.rel(sh["dlogits"], ref["dlogits"]) < 1e-12
    f = H.ce_ref(z + 100, labels, B, H.f32(1.0 / B), H.f32(1.0 / B), dtype=torch.float32)
    assert H.loss_err(f["loss"], ref["loss"]) < H.LOSS_TOL / 10 and H.row_rel(f["dlogits"], ref["dlogits"]) < H.TOL / 10


def test_case_list_reaches_every_instantiation():
    """vitpe_head_step accepts D <= 768 and Cn <= 64.  The weight leaves LDS when Cn D > 12288, which needs D > 192: with
    KD = 2 (D <= 128) and KD = 3 (D <= 192) the product is at most 64 * 192 = 12288, so (2, global) and (3, global) cannot be
    launched through the entry point; the other six (KD, WLDS) pairs must occur in both dtypes."""
    seen = {(H.head_step_instance(D, Cn), dt) for dt, _, _, D, Cn, _, _ in H.HEAD_STEP_CASES}
    reachable = {H.head_step_instance(D, Cn) for D in range(1, 769) for Cn in range(1, 65)}
    assert reachable == {(2, True), (3, True), (6, True), (12, True), (6, False), (12, False)}
    assert seen == {(inst, dt) for inst in reachable for dt in ("f32", "bf16")}
    vals = lambda i: {c[i] for c in H.HEAD_STEP_CASES}  # noqa: E731
    assert vals(1) == {1, 3, 5, 257} and vals(2) == {1, 17} and set(H.EPS_SWEEP) == vals(6)
    assert {(c[5] == 0, c[5] == 1, c[5] == c[1] - 1, c[5] == c[1]) for c in H.HEAD_STEP_CASES} >= {
        (True, False, False, False), (False, False, True, False), (False, False, False, True)}
    ragged_global = {c[0] for c in H.HEAD_STEP_CASES if not H.head_step_instance(c[3], c[4])[1] and 0 < c[5] < c[1]}
    assert ragged_global == {"f32", "bf16"}


def test_step_head_set_valid_writes_the_control_block_without_a_device():
    """StepHead over CPU tensors, world 2, batch 4: set_valid leaves float32 {world / n_global, 1 / n_global, n_valid, 0};
    the global count defaults to n_valid * world; counts outside the batch raise; an unchanged pair writes nothing."""
    from vitpe._lib import VitpeError
    from vitpe.head import StepHead
    B, N, D, Cn = 4, 3, 8, 5
    norm, lin = torch.nn.LayerNorm(D), torch.nn.Linear(D, Cn)
    grads = [torch.zeros_like(p) for p in (lin.weight, lin.bias, norm.weight, norm.bias)]
    dx = torch.ones(B, N, D)
    head = StepHead(norm, lin, grads, torch.zeros(B, N, D), dx, torch.zeros(B, dtype=torch.int64), torch.zeros(16),
                    torch.float32, N, True, world=2)
    f32 = lambda *v: torch.tensor(v, dtype=torch.float32)  # noqa: E731
    assert head.ctl.dtype == torch.float32 and head.valid == (B, 2 * B)
    assert torch.equal(head.ctl, f32(2 / 8, 1 / 8, 4, 0))          # the constructor's set_valid(B)
    assert not dx.any() and head.ticked is False                  # the zero rows of dx_out[L] are the head's to establish
    head.set_valid(3, 5)
    assert torch.equal(head.ctl, f32(2 / 5, 1 / 5, 3, 0))
    head.set_valid(3)
    assert head.valid == (3, 6) and torch.equal(head.ctl, f32(2 / 6, 1 / 6, 3, 0))
    head.set_valid(0, 1)                                           # a rank with an empty share of a global batch of 1
    assert torch.equal(head.ctl, f32(2.0, 1.0, 0, 0))
    for bad in ((B + 1, None), (-1, None), (-1, 4), (3, 2), (0, 0)):
        with pytest.raises(VitpeError):
            head.set_valid(*bad)
    assert head.valid == (0, 1) and torch.equal(head.ctl, f32(2.0, 1.0, 0, 0))   # a refused call changes nothing
    head.set_valid(3, 5)
    head.ctl.fill_(7.0)
    head.set_valid(3, 5)                                           # the pair it was last set for: no write
    assert torch.equal(head.ctl, torch.full((4,), 7.0))
    head.set_valid(3, 6)
    assert torch.equal(head.ctl, f32(2 / 6, 1 / 6, 3, 0))
