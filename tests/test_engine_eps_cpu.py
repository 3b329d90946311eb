"""The engine-level eps fixture of tests/engine_eps_ref.py, checked on the oracle without a GPU: the rows every LayerNorm
normalises have a variance within 8x of its eps, the oracle's optional `ln_eps` defaults to 1e-5 everywhere, and resetting
any SINGLE LayerNorm's eps to 1e-5 moves the logits or some gradient by >= 10x the gate the GPU test applies (1e-4 on
logits, 1e-3 on gradients) -- so the GPU test notices the engine handing a kernel the wrong module's eps."""
import pytest
import torch

import engine_eps_ref as E
from oracle import vit_oracle as O


@pytest.fixture(scope="module")
def fixture():
    cfg = O.VitConfig(pos_encoding=E.TAG, **E.GEOM)
    images, labels = E.batch(cfg, 4)
    params = E.calibrated_params(cfg, images)
    return cfg, params, images, labels, O.loss_and_grads(cfg, params, images, labels, E.LN_EPS)


def test_every_layernorm_sees_rows_of_variance_comparable_to_its_eps(fixture):
    cfg, params, images, _, _ = fixture
    assert len(set(E.LN_EPS.values())) == 5 and 1e-5 not in E.LN_EPS.values()
    for name, rows in E.stage_rows(cfg, params, images).items():
        assert E.variance_fraction(rows, E.LN_EPS[name]) >= 0.9, name


def test_ln_eps_defaults_to_the_reference_value(fixture):
    cfg, params, images, labels, _ = fixture
    a = O.loss_and_grads(cfg, params, images, labels)
    b = O.loss_and_grads(cfg, params, images, labels, {n: 1e-5 for n in E.LN_EPS})
    c = O.loss_and_grads(cfg, params, images, labels, {})
    for other in (b, c):
        assert torch.equal(a[0], other[0]) and torch.equal(a[1], other[1])
        assert all(torch.equal(a[2][n], other[2][n]) for n in a[2])


@pytest.mark.parametrize("name", list(E.LN_EPS))
def test_resetting_one_eps_is_visible_at_ten_times_the_gate(fixture, name):
    cfg, params, images, labels, ref = fixture
    wrong = O.loss_and_grads(cfg, params, images, labels, dict(E.LN_EPS, **{name: 1e-5}))
    assert E.worst_ratio(wrong, ref) >= 10
