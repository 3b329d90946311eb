#!/usr/bin/env python3
"""Cost of the weight EMA (vitpe_ema_update behind vitpe_adamw_step), timed with HIP events:

kernels: on flat buffers of the two model sizes -- the default CIFAR model (32 / 4, d 192, depth 6) and ViT-B/16
         (bench.py --config imnet: 224 / 16, d 768, depth 12): `ema` = vitpe_ema_update alone (12 B / element: p and e in,
         e out), `adamw` = vitpe_adamw_step alone as the engine launches it (bf16 flat copy, zero_grad, the step counter
         ticked by the head kernel: 34 B / element -- p, g, m, v in and out, the bf16 copy out), `adamw+ema` = the two in
         the step's order; rotating over a ring of operand sets (4 / 2 sets) so that no set is served from the caches
         more than the step's own would be; medians of 5 repeats of 200 (CIFAR) / 20 (ViT-B) launches, the variants
         alternating inside every repeat.  `ema_GBps` / `adamw_GBps` are the achieved bytes/s at those byte counts,
         `*_spread` the (max - min) / median of the five repeats: the EMA kernel has the same access pattern and fewer
         streams, so it is expected to stream no slower than AdamW less that spread (an expectation, not a gate).
         `swap` = vitpe_ema_swap with the bf16 copy (18 B / element), what entering or leaving ema_weights() costs on top
         of the shadow refresh.
steps:   the engine's captured step, EMA off against on (decay 0.999), ONE engine switched back and forth (the step is
         re-captured at every switch; two engines differ by more than the update costs): 512 images at the CIFAR geometry
         and 64 at ViT-B/16, bf16, rope-axial; medians of 5 repeats of 100 / 20 steps.
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
from vitpe import ddp  # noqa: E402
from vitpe import kernels as K  # noqa: E402

GEOM = {"cifar": dict(img_size=32, patch_size=4, embed_dim=192, depth=6, num_heads=6),
        "vit_b16": dict(img_size=224, patch_size=16, embed_dim=768, depth=12, num_heads=12)}
EMA_BYTES, ADAMW_BYTES, SWAP_BYTES = 12, 34, 18   # per element


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
    sets = []
    for _ in range(ring):
        f = dict(dtype=torch.float32, device="cuda")
        hp = torch.zeros(16, **f)
        hp[:5] = torch.tensor([1e-3, 0.9, 0.999, 1e-8, 0.05], **f)
        hp[5:9] = torch.tensor([1.0, 0.1, 0.001, 1.0], **f)      # as after the head kernel's tick of step 1
        hp[13] = 0.999
        p = torch.randn(n, generator=g, **f) * 0.02
        sets.append(dict(p=p, e=p.clone(), g=torch.randn(n, generator=g, **f) * 1e-3, m=torch.zeros(n, **f),
                         v=torch.zeros(n, **f), s=torch.zeros(n, dtype=torch.bfloat16, device="cuda"), hp=hp))

    def adamw(s):
        K.adamw_step(s["p"], s["g"], s["m"], s["v"], s["hp"], shadow_bf16=s["s"], zero_grad=True, ticked=True)

    def ema(s):
        K.ema_update(s["p"], s["e"], s["hp"])

    def both(s):
        adamw(s)
        ema(s)

    def swap(s):
        K.ema_swap(s["p"], s["e"], shadow_bf16=s["s"])

    res = alternate({"adamw": Rotor(sets, adamw), "ema": Rotor(sets, ema), "adamw+ema": Rotor(sets, both),
                     "swap": Rotor(sets, swap)}, iters)
    gbps = lambda key, per: round(per * n / res[key][0] / 1e3, 1)  # noqa: E731
    spread = lambda key: round((res[key][2] - res[key][1]) / res[key][0], 4)  # noqa: E731
    report("optimizer kernels", res, model=name, n_flat=n, workgroups=K.ema_blocks(n), ring=ring,
           ema_GBps=gbps("ema", EMA_BYTES), adamw_GBps=gbps("adamw", ADAMW_BYTES), swap_GBps=gbps("swap", SWAP_BYTES),
           ema_spread=spread("ema"), adamw_spread=spread("adamw"),
           added_us=round(res["adamw+ema"][0] - res["adamw"][0], 2))


def steps(name, B, iters, reps=5):
    """ONE engine, the average switched off and on in turn (each switch re-captures the step): the same buffers at the
    same addresses in both states -- two engines of this geometry differ by more than the update costs."""
    from vitpe.engine import TrainEngine
    g = torch.Generator(device="cuda").manual_seed(1)
    S = GEOM[name]["img_size"]
    images = torch.randn(B, 3, S, S, generator=g, device="cuda")
    labels = torch.randint(0, 10, (B,), generator=g, device="cuda")
    eng = TrainEngine(model(name).cuda(), B, compute_dtype=torch.bfloat16, use_graph=True)
    eng.step(images, labels)
    out = {"off": [], "on": []}
    for _ in range(reps):
        for key, decay in (("off", None), ("on", 0.999)):
            eng.set_ema(decay)
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
    report("TrainEngine.step", res, model=name, B=B, dtype="bf16", added_us=round(res["on"][0] - res["off"][0], 2),
           on_over_off=round(res["on"][0] / res["off"][0], 4),
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
