#!/usr/bin/env python3
"""The engine's opt-in route for qkv bias / dropout / stochastic depth (TrainEngine(extras=True)), timed with HIP events:

kernels: vitpe_branch_drop_fwd / _bwd (both sites, p = 0.1) against the two launches they replace (vitpe_dropout_* into an
         intermediate, then vitpe_drop_path_*), bf16, on [512 * 65, 192] and [64 * 197, 768]; medians of 5 repeats of 50
         launches, rotating over enough buffer sets that no launch finds its operands in the last-level cache (256 MB).
         Bytes are the algorithmic ones: 2 n (backward) / 3 n (forward with residual) elements for the fused pass,
         4 n / 5 n for the pair.
steps:   CIFAR geometry (32 / 4, d 192, 6 heads, depth 6, B 512, bf16, rope-axial): the captured extras step with all four
         options at 0.1, one module-path step of the same model (forward, CE, backward, torch.optim.AdamW, eager), the
         extras step with no option active and the default engine's step; medians of 3 repeats.
Prints one JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "vit-rpe-rope_amd"))
from vitpe import kernels as K  # noqa: E402


def timeit(fn, iters=50, warm=5, reps=5):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters * 1e3)  # us
    return statistics.median(out)


class Rotor:
    """fn(set) over a ring of operand sets"""

    def __init__(self, sets, fn):
        self.sets, self.fn, self.i = sets, fn, 0

    def __call__(self):
        self.fn(self.sets[self.i])
        self.i = (self.i + 1) % len(self.sets)


def kernels(p=0.1):
    T, dev = torch.bfloat16, "cuda"
    rng = K.new_rng_pairs(2, dev)
    for B, N, D in ((512, 65, 192), (64, 197, 768)):
        n = B * N * D
        nsets = max(2, -(-(512 << 20) // (4 * n * 2)))
        sets = [tuple(torch.randn(B, N, D, device=dev).to(T) for _ in range(4)) for _ in range(nsets)]   # x, resid, tmp, y
        fused_f = timeit(Rotor(sets, lambda s: K.branch_drop_fwd(s[0], rng[0], p, rng[1], p, resid=s[1], out=s[3])))
        pair_f = timeit(Rotor(sets, lambda s: (K.dropout_fwd(s[0], rng[0], p, out=s[2]),
                                               K.drop_path_fwd(s[2], rng[1], p, resid=s[1], out=s[3]))))
        fused_b = timeit(Rotor(sets, lambda s: K.branch_drop_bwd(s[0], rng[0], p, rng[1], p, out=s[3])))
        pair_b = timeit(Rotor(sets, lambda s: (K.dropout_bwd(s[0], rng[0], p, out=s[2]),
                                               K.drop_path_bwd(s[2], rng[1], p, out=s[3]))))
        tbs = lambda elems, us: round(elems * 2 / us / 1e6, 2)  # noqa: E731
        print(json.dumps({"kernel": "branch_drop", "shape": [B * N, D], "elements": n, "p": p, "buffer_sets": nsets,
                          "fwd_us": round(fused_f, 2), "fwd_bytes": 3 * n * 2, "fwd_TBps": tbs(3 * n, fused_f),
                          "fwd_two_launches_us": round(pair_f, 2), "fwd_two_launches_bytes": 5 * n * 2,
                          "fwd_two_launches_TBps": tbs(5 * n, pair_f),
                          "bwd_us": round(fused_b, 2), "bwd_bytes": 2 * n * 2, "bwd_TBps": tbs(2 * n, fused_b),
                          "bwd_two_launches_us": round(pair_b, 2), "bwd_two_launches_bytes": 4 * n * 2,
                          "bwd_two_launches_TBps": tbs(4 * n, pair_b)}), flush=True)
        del sets


def steps(B=512, p=0.1):
    from models.vit import VisionTransformer
    from vitpe.engine import TrainEngine
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    images = torch.randn(B, 3, 32, 32, device=dev, generator=g)
    labels = torch.randint(0, 10, (B,), device=dev, generator=g)
    opts = dict(qkv_bias=True, drop_rate=p, attn_drop_rate=p, drop_path_rate=p)

    def model(**kw):
        torch.manual_seed(0)
        return VisionTransformer(pos_encoding="rope-axial", **kw).to(dev)

    def engine_step(extras, **kw):
        eng = TrainEngine(model(**kw), B, compute_dtype=torch.bfloat16, use_graph=True, extras=extras)
        eng.images.copy_(images); eng.labels.copy_(labels)
        us = timeit(eng.step, iters=50, warm=10, reps=3)
        loss = eng.read_metrics()[0] / eng.steps_done
        assert loss == loss, "non-finite loss"
        return us

    def module_step():
        m = model(**opts).set_compute_dtype(torch.bfloat16).train()
        opt = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=0.01)

        def one():
            opt.zero_grad(set_to_none=True)
            torch.nn.functional.cross_entropy(m(images), labels).backward()
            opt.step()
        return timeit(one, iters=20, warm=5, reps=3)

    res = {"geometry": "32/4 d192 H6 depth6 B%d bf16 rope-axial" % B, "p": p}
    res["extras_all_options_captured_step_us"] = round(engine_step(True, **opts), 1)
    res["module_path_eager_step_us"] = round(module_step(), 1)
    res["extras_no_option_captured_step_us"] = round(engine_step(True), 1)
    res["default_engine_captured_step_us"] = round(engine_step(False), 1)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["kernels", "steps", "all"], default="all")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    if a.part in ("kernels", "all"):
        kernels()
    if a.part in ("steps", "all"):
        steps()
