"""The launch trace of every engine route against tests/golden/engine_trace.json: the same C-ABI calls, in the same order,
with the same scalar arguments and the same buffer aliasing as the commit the golden was recorded from (the one before
vitpe/engine.py was reorganised around Route; its hash is the golden's "recorded_from").  The recorder and the
configurations are tests/engine_trace.py; the golden is never regenerated from the code under test."""
import json

import pytest

import engine_trace as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden_trace():
    with open(E.GOLDEN_PATH) as f:
        return json.load(f)["configs"]


def test_golden_covers_every_configuration(golden_trace):
    assert set(golden_trace) == set(E.CONFIGS)


@pytest.mark.parametrize("name", list(E.CONFIGS))
def test_launch_trace_is_unchanged(golden_trace, name):
    """One small engine, one eager step, one evaluation forward, the split backward (and the probes' closures where the
    configuration has them): route flags, call names and the hash of the full trace all equal the golden's."""
    want = golden_trace[name]
    route, traces = E.trace_config(name)
    assert route == want["route"]
    assert set(traces) == set(want["sequences"])
    for seq, calls in traces.items():
        names, sha = E.digest(calls)
        assert " ".join(names) == want["sequences"][seq]["names"], (name, seq)
        assert sha == want["sequences"][seq]["sha256"], (name, seq, "same calls, other arguments or aliasing: "
                                                         "python tests/engine_trace.py --dump DIR on both commits and diff")
