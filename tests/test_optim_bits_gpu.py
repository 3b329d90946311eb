"""The optimizer-side kernels against tests/golden/optim_bits.json: after three seeded steps of lr_schedule, grad_clip,
adamw_step / adamw_step_groups and ema_update, and two ema_swap, every buffer holds the bits it held on the commit the
golden was recorded from (its "recorded_from"; the one before the kernels moved into csrc/optim.hip).  The cases and the
driver are tests/optim_bits.py; the golden is never regenerated from the code under test."""
import json

import pytest

import optim_bits as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden_bits():
    with open(O.GOLDEN_PATH) as f:
        return json.load(f)["cases"]


def test_golden_covers_every_case(golden_bits):
    assert set(golden_bits) == set(O.CASES)


@pytest.mark.parametrize("name", list(O.CASES))
def test_optimizer_bits_are_unchanged(golden_bits, name):
    assert O.run_case(name) == golden_bits[name], name
