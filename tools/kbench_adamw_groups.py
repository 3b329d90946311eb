#!/usr/bin/env python3
"""Cost of AdamW with parameter groups (vitpe_adamw_step_groups) and of the per-step LR schedule, timed with HIP events:

kernels: on flat buffers of the two model sizes -- the default CIFAR model (32 / 4, d 192, depth 6) and ViT-B/16
         (bench.py --config imnet: 224 / 16, d 768, depth 12): `adamw` = vitpe_adamw_step as the engine launches it (bf16
         flat copy, zero_grad, the step counter ticked by the head kernel: 34 B / element -- p, g, m, v in and out, the
         bf16 copy out), `groups` =
         vitpe_adamw_step_groups on the same operands with 4 groups (the (lr, wd) scales of the kernel test, spans of
         1 / 2 / 33 / 5 granules repeating: + 1 B per 8 elements), `groups1` = the same with every scale 1 (what the map
         costs without divergent rates), `sched` = vitpe_lr_schedule alone; rotating over a ring of operand sets (4 / 2
         sets) so that no set is served from the caches more than the step's own would be; medians of 5 repeats of 200
         (CIFAR) / 20 (ViT-B) launches, the variants alternating inside every repeat.  `*_GBps` are the achieved bytes/s,
         `*_spread` the (max - min) / median of the five repeats.  Expectation, not a gate: `groups` is no slower than
         `adamw` beyond `adamw_spread`.
steps:   the engine's captured step, groups + schedule off against on (vit_param_groups(model, True, 0.75), a 1000-step
         schedule), ONE engine switched back and forth (the step is re-captured at every switch; two engines differ by more
         than the update costs): 512 images at the CIFAR geometry and 64 at ViT-B/16, bf16, rope-axial; medians of 5
         repeats of 100 / 20 steps.
Prints one JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "vit-rpe-rope_amd"))
from vitpe import ddp  # noqa: E402
from vitpe import kernels as K  # noqa: E402

GEOM = {"cifar": dict(img_size=32, patch_size=4, embed_dim=192, depth=6, num_heads=6),
        "vit_b16": dict(img_size=224, patch_size=16, embed_dim=768, depth=12, num_heads=12)}
ADAMW_BYTES, GROUPS_BYTES = 34, 34 + 1 / 8   # per element
GROUPS4 = [(1.0, 1.0), (1.0, 0.0), (0.5, 1.0), (0.0, 0.0)]
SPANS4 = (1, 2, 33, 5)


def model(name):
    from models.vit import VisionTransformer
    torch.manual_seed(0)
    return VisionTransformer(pos_encoding="rope-axial", **GEOM[name])


def alternate(fns, iters, warm=5, reps=5):
    """{name: (median, min, max) us per call}; every repeat times each variant once, in turn."""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[k].append(e0.elapsed_time(e1) / iters * 1e3)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in out.items()}


def report(measure, res, **extra):
    row = dict(measure=measure, **extra)
    for k, (med, lo, hi) in res.items():
        row[k + "_us"], row[k + "_min_us"], row[k + "_max_us"] = round(med, 2), round(lo, 2), round(hi, 2)
    print(json.dumps(row), flush=True)
    return row


class Rotor:
    def __init__(self, sets, fn):
        self.sets, self.fn, self.i = sets, fn, 0

    def __call__(self):
        self.fn(self.sets[self.i])
        self.i = (self.i + 1) % len(self.sets)


def kernels(name, ring, iters):
    n = ddp.flat_layout([p.numel() for p in model(name).parameters()], 8)[1]
    g = torch.Generator(device="cuda").manual_seed(0)
    period = np.repeat(np.arange(4, dtype=np.uint8), SPANS4)
    gid_np = np.tile(period, n // 8 // period.size + 1)[:n // 8]
    sets = []
    for _ in range(ring):
        f = dict(dtype=torch.float32, device="cuda")
        hp = torch.zeros(16, **f)
        hp[:5] = torch.tensor([1e-3, 0.9, 0.999, 1e-8, 0.05], **f)
        hp[5:9] = torch.tensor([1.0, 0.1, 0.001, 1.0], **f)      # as after the head kernel's tick of step 1
        sets.append(dict(p=torch.randn(n, generator=g, **f) * 0.02, g=torch.randn(n, generator=g, **f) * 1e-3,
                         m=torch.zeros(n, **f), v=torch.zeros(n, **f), s=torch.zeros(n, dtype=torch.bfloat16, device="cuda"),
                         hp=hp, gid=torch.from_numpy(gid_np).cuda(), gtab=torch.tensor(GROUPS4, **f),
                         ones=torch.ones(4, 2, **f),
                         sched=torch.tensor([1e-3, 1e-5, 5.0, 1000.0, 1e-3, 0.0, 0.0, 0.0], **f)))

    def adamw(s):
        K.adamw_step(s["p"], s["g"], s["m"], s["v"], s["hp"], shadow_bf16=s["s"], zero_grad=True, ticked=True)

    def groups(s):
        K.adamw_step_groups(s["p"], s["g"], s["m"], s["v"], s["hp"], s["gid"], s["gtab"], shadow_bf16=s["s"], zero_grad=True,
                            ticked=True)

    def groups1(s):
        K.adamw_step_groups(s["p"], s["g"], s["m"], s["v"], s["hp"], s["gid"], s["ones"], shadow_bf16=s["s"], zero_grad=True,
                            ticked=True)

    def sched(s):
        K.lr_schedule(s["hp"], s["sched"], ticked=True)

    res = alternate({"adamw": Rotor(sets, adamw), "groups": Rotor(sets, groups), "groups1": Rotor(sets, groups1),
                     "sched": Rotor(sets, sched)}, iters)
    gbps = lambda key, per: round(per * n / res[key][0] / 1e3, 1)  # noqa: E731
    spread = lambda key: round((res[key][2] - res[key][1]) / res[key][0], 4)  # noqa: E731
    report("optimizer kernels", res, model=name, n_flat=n, workgroups=K.adamw_groups_blocks(n), ring=ring,
           adamw_GBps=gbps("adamw", ADAMW_BYTES), groups_GBps=gbps("groups", GROUPS_BYTES),
           adamw_spread=spread("adamw"), groups_spread=spread("groups"),
           groups_over_adamw=round(res["groups"][0] / res["adamw"][0], 4))


def steps(name, B, iters, reps=5):
    """ONE engine, groups + schedule switched off and on in turn (each switch re-captures the step): the same buffers at
    the same addresses in both states -- two engines of this geometry differ by more than the update costs."""
    from vitpe.engine import TrainEngine
    from vitpe.optim import vit_param_groups
    g = torch.Generator(device="cuda").manual_seed(1)
    S = GEOM[name]["img_size"]
    images = torch.randn(B, 3, S, S, generator=g, device="cuda")
    labels = torch.randint(0, 10, (B,), generator=g, device="cuda")
    eng = TrainEngine(model(name).cuda(), B, compute_dtype=torch.bfloat16, use_graph=True)
    eng.step(images, labels)
    groups = vit_param_groups(eng.model, True, 0.75)
    out = {"off": [], "on": []}
    for _ in range(reps):
        for key in ("off", "on"):
            eng.set_param_groups(groups if key == "on" else None)
            eng.set_lr_schedule(1e-3 if key == "on" else None, 1000, warmup_steps=5, min_lr=1e-5)
            for _ in range(5):
                eng.step()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                eng.step()
            e1.record()
            torch.cuda.synchronize()
            out[key].append(e0.elapsed_time(e1) / iters * 1e3)
    res = {k: (statistics.median(v), min(v), max(v)) for k, v in out.items()}
    report("TrainEngine.step", res, model=name, B=B, dtype="bf16", n_groups=len(groups) + 1,
           added_us=round(res["on"][0] - res["off"][0], 2), on_over_off=round(res["on"][0] / res["off"][0], 4),
           off_spread=round((res["off"][2] - res["off"][1]) / res["off"][0], 4))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip_steps", action="store_true")
    ap.add_argument("--skip_vit_b16", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    kernels("cifar", 4, 200)
    if not a.skip_vit_b16:
        kernels("vit_b16", 2, 20)
    if not a.skip_steps:
        steps("cifar", 512, 100)
        if not a.skip_vit_b16:
            steps("vit_b16", 64, 20)
