#!/usr/bin/env python3
"""Cost of gradient clipping by global norm (vitpe_grad_clip + vitpe_adamw_step reading hp[9]), timed with HIP events:

kernels: on flat buffers of the two model sizes -- the default CIFAR model (32 / 4, d 192, depth 6) and ViT-B/16
         (bench.py --config imnet: 224 / 16, d 768, depth 12) -- the optimizer as the engine launches it (bf16 flat copy,
         zero_grad, the step counter ticked by the head kernel):  `adamw` = vitpe_adamw_step alone, `clip` = vitpe_grad_clip
         alone, `clip+adamw` = the two together; rotating over a ring of operand sets (4 / 2 sets) so that no set is
         served from the caches more than the step's own would be; medians of 5 repeats of 200 (CIFAR) / 20 (ViT-B)
         launches, the three variants alternating inside every repeat.  --parent_lib PATH times vitpe_adamw_step of ANOTHER
         build of libvitpe.so (the parent commit's) in the same process as `parent_adamw`.  The gradient is zero after the
         first launch (zero_grad): the kernels' time does not depend on the values.
steps:   the engine's captured step, clipping off against on (max_norm 1.0), two engines on the same batch, alternating:
         512 images at the CIFAR geometry and 64 at ViT-B/16, bf16, rope-axial; medians of 5 repeats of 100 / 20 steps.
Prints one JSON line per measurement."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "vit-rpe-rope_amd"))
from vitpe import _lib as L  # noqa: E402
from vitpe import ddp  # noqa: E402
from vitpe import kernels as K  # noqa: E402

GEOM = {"cifar": dict(img_size=32, patch_size=4, embed_dim=192, depth=6, num_heads=6),
        "vit_b16": dict(img_size=224, patch_size=16, embed_dim=768, depth=12, num_heads=12)}


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


def kernels(name, ring, iters, parent):
    n = ddp.flat_layout([p.numel() for p in model(name).parameters()], 8)[1]
    g = torch.Generator(device="cuda").manual_seed(0)
    sets = []
    for _ in range(ring):
        f = dict(dtype=torch.float32, device="cuda")
        hp = torch.zeros(16, **f)
        hp[:5] = torch.tensor([1e-3, 0.9, 0.999, 1e-8, 0.05], **f)
        hp[5:9] = torch.tensor([1.0, 0.1, 0.001, 1.0], **f)      # as after the head kernel's tick of step 1
        hp[12] = 1.0
        sets.append(dict(p=torch.randn(n, generator=g, **f) * 0.02, g=torch.randn(n, generator=g, **f) * 1e-3,
                         m=torch.zeros(n, **f), v=torch.zeros(n, **f), s=torch.zeros(n, dtype=torch.bfloat16, device="cuda"),
                         hp=hp, partial=torch.zeros(K.grad_clip_blocks(n), **f)))

    def adamw(s, clipped=False):
        K.adamw_step(s["p"], s["g"], s["m"], s["v"], s["hp"], shadow_bf16=s["s"], zero_grad=True, ticked=True, clipped=clipped)

    def clip(s):
        K.grad_clip(s["g"], s["hp"], s["partial"])

    def both(s):
        clip(s)
        adamw(s, clipped=True)

    fns = {"adamw": Rotor(sets, adamw), "clip": Rotor(sets, clip), "clip+adamw": Rotor(sets, both)}
    if parent is not None:
        def parent_adamw(s):
            L.check(parent.vitpe_adamw_step(s["p"].data_ptr(), s["g"].data_ptr(), s["m"].data_ptr(), s["v"].data_ptr(),
                                            s["s"].data_ptr(), s["hp"].data_ptr(), n, 3, L.stream_ptr()), "parent vitpe_adamw_step")
        fns["parent_adamw"] = Rotor(sets, parent_adamw)
    res = alternate(fns, iters)
    report("optimizer kernels", res, model=name, n_flat=n, workgroups=K.grad_clip_blocks(n), ring=ring,
           clip_read_GBps=round(4 * n / res["clip"][0] / 1e3, 1), added_us=round(res["clip+adamw"][0] - res["adamw"][0], 2))


def steps(name, B, iters):
    from vitpe.engine import TrainEngine
    g = torch.Generator(device="cuda").manual_seed(1)
    S = GEOM[name]["img_size"]
    images = torch.randn(B, 3, S, S, generator=g, device="cuda")
    labels = torch.randint(0, 10, (B,), generator=g, device="cuda")
    engines = {}
    for key, max_norm in (("off", None), ("on", 1.0)):
        eng = TrainEngine(model(name).cuda(), B, compute_dtype=torch.bfloat16, use_graph=True)
        eng.set_grad_clip(max_norm)
        eng.step(images, labels)
        engines[key] = eng
    res = alternate({k: e.step for k, e in engines.items()}, iters)
    report("TrainEngine.step", res, model=name, B=B, dtype="bf16", added_us=round(res["on"][0] - res["off"][0], 2),
           on_over_off=round(res["on"][0] / res["off"][0], 4), last_norm=round(engines["on"].grad_norm(), 4))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent_lib", default=None, help="libvitpe.so of the parent commit: its vitpe_adamw_step is timed too")
    ap.add_argument("--skip_steps", action="store_true")
    ap.add_argument("--skip_vit_b16", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    parent = None
    if a.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(a.parent_lib))
        parent.vitpe_adamw_step.argtypes = L.parse_header()["vitpe_adamw_step"]
        parent.vitpe_adamw_step.restype = ctypes.c_int
    kernels("cifar", 4, 200, parent)
    if not a.skip_vit_b16:
        kernels("vit_b16", 2, 20, parent)
    if not a.skip_steps:
        steps("cifar", 512, 100)
        if not a.skip_vit_b16:
            steps("vit_b16", 64, 20)
