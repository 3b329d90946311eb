"""Measured figures of the LayerNorm-eps and head/loss GPU tests: every test collects (check, measured, limit) triples,
appends them as one JSON line to profiles/ln_eps_head_parity.jsonl (the manner of _dump in test_bench_path_gpu.py; the
committed file holds a passing run) and only THEN asserts, so a failing run leaves its numbers behind.  A module's worst
figure per check is appended when the module finishes.  A module may name another file under profiles/
(Report(module, name): test_embed_gpu.py writes embed_parity.jsonl)."""
import json
import math
import os

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ln_eps_head_parity.jsonl"


def _append(line, name=None):
    """name: the file under profiles/ (None: NAME, the file of the LayerNorm-eps and head/loss modules)"""
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    with open(os.path.join(REPO, "profiles", name or NAME), "a") as f:
        f.write(json.dumps(line) + "\n")


def _num(v):
    v = float(v)
    return v if math.isfinite(v) else repr(v)


class Report:
    def __init__(self, module, name=None):
        self.module, self.worst, self.name = module, {}, name

    def case(self, test, case):
        return Case(self, test, case)

    def close(self):
        _append({"module": self.module, "worst": {k: {"measured": _num(v), "limit": _num(l), "at": at}
                                                  for k, (v, l, at) in sorted(self.worst.items())}}, self.name)


class Case:
    """lt / le / eq record one figure each; done() writes the line and raises if any of them missed."""

    def __init__(self, report, test, case):
        self.report, self.test, self.case_id = report, test, str(case)
        self.figures, self.bad = {}, []

    def _rec(self, key, value, limit, ok):
        value = float(value)
        self.figures[key] = max(self.figures.get(key, -math.inf), value) if not math.isnan(value) else value
        if not ok:
            self.bad.append((key, value, limit))
        w = self.report.worst.get(f"{self.test}:{key}")
        if w is None or not value <= w[0]:
            self.report.worst[f"{self.test}:{key}"] = (value, limit, self.case_id)

    def lt(self, key, value, limit):
        self._rec(key, value, limit, float(value) < limit)

    def le(self, key, value, limit):
        self._rec(key, value, limit, float(value) <= limit)

    def eq(self, key, got, want):
        """exact checks: the figure is |got - want| (a count of differing elements for tensors), the limit 0."""
        self._rec(key, abs(float(got) - float(want)), 0.0, float(got) == float(want))

    def done(self):
        _append({"module": self.report.module, "test": self.test, "case": self.case_id,
                 "figures": {k: _num(v) for k, v in self.figures.items()}, "missed": [list(map(str, b)) for b in self.bad]},
                self.report.name)
        assert not self.bad, f"{self.test}[{self.case_id}]: (check, measured, limit) missed: {self.bad}"
