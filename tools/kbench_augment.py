#!/usr/bin/env python3
"""Cost of the augmentation stream (RandomCrop(S, padding=4) + RandomHorizontalFlip inside the gather kernels), timed with HIP
events, augmentation off against on in the same process:

kernels: vitpe_patch_embed from the resident uint8 dataset at B = 512 / CIFAR (3 x 32 x 32, patch 4, d 192, bf16, with the
         patch-matrix and LayerNorm-statistics outputs the engine asks for) over a 50000-record set, and vitpe_unfold_u8 at
         the 224 / 16 geometry (B = 64, bf16) over a 512-record set; random sample indices, rotating over 8 index batches;
         medians of 5 repeats of 200 launches.
steps:   the engine's captured 512-image step (32 / 4, d 192, 6 heads, depth 6, bf16, rope-axial) on step_indexed;
         medians of 5 repeats of 100 steps.
--off_only measures only the unaugmented entry points (it then also runs on a tree from before the augmentation, for the
"off against the parent commit" comparison).  Prints one JSON line per measurement."""
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

PAD, HFLIP = 4, True


def timeit(fn, iters=200, warm=10, reps=5):
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
    return statistics.median(out), min(out), max(out)


class Rotor:
    """fn(set) over a ring of operand sets"""

    def __init__(self, sets, fn):
        self.sets, self.fn, self.i = sets, fn, 0

    def __call__(self):
        self.fn(self.sets[self.i])
        self.i = (self.i + 1) % len(self.sets)


def report(name, off, on, **extra):
    row = dict(measure=name, **extra, off_us=round(off[0], 2), off_min_us=round(off[1], 2), off_max_us=round(off[2], 2))
    if on is not None:
        row.update(on_us=round(on[0], 2), on_min_us=round(on[1], 2), on_max_us=round(on[2], 2), on_over_off=round(on[0] / off[0], 3))
    print(json.dumps(row), flush=True)


def dataset(n, C, S, g):
    data = torch.randint(0, 256, (n, C, S, S), dtype=torch.uint8, device="cuda", generator=g)
    mean = torch.tensor((0.4914, 0.4822, 0.4465)[:C], device="cuda")
    std = torch.tensor((0.2023, 0.1994, 0.2010)[:C], device="cuda")
    return data, mean, std


def kernels(off_only):
    T, dev = torch.bfloat16, "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    aug = None if off_only else dict(rng=K.new_rng_pairs(1, dev), crop_pad=PAD, hflip=HFLIP)
    # fused patch embed, CIFAR
    B, C, S, p, D = 512, 3, 32, 4, 192
    P, Kp = (S // p) ** 2, C * p * p
    data, mean, std = dataset(50000, C, S, g)
    idx = [torch.randint(0, 50000, (B,), device=dev, generator=g) for _ in range(8)]
    w = (torch.randn(D, Kp, device=dev, generator=g) * 0.2).to(T)
    bias, cls = torch.randn(D, device=dev, generator=g), torch.randn(D, device=dev, generator=g)
    tok, pat = torch.empty(B, P + 1, D, dtype=T, device=dev), torch.empty(B * P, Kp, dtype=T, device=dev)
    st = (torch.empty(B * (P + 1), device=dev), torch.empty(B * (P + 1), device=dev))

    def embed(i, **kw):
        K.patch_embed(w, bias, cls, None, p, T, data=data, index=i, mean=mean, std=std, out=tok, patches_out=pat, stats=st, **kw)

    off = timeit(Rotor(idx, embed))
    on = None if off_only else timeit(Rotor(idx, lambda i: embed(i, **aug)))
    report("vitpe_patch_embed[u8]", off, on, B=B, C=C, S=S, p=p, D=D, dtype="bf16")
    del data
    # unfold at 224 / 16
    B, C, S, p = 64, 3, 224, 16
    data, mean, std = dataset(512, C, S, g)
    idx = [torch.randint(0, 512, (B,), device=dev, generator=g) for _ in range(8)]
    pat = torch.empty(B * (S // p) ** 2, C * p * p, dtype=T, device=dev)

    def unf(i, **kw):
        K.unfold_u8(data, i, mean, std, p, T, out=pat, **kw)

    off = timeit(Rotor(idx, unf))
    on = None if off_only else timeit(Rotor(idx, lambda i: unf(i, **aug)))
    report("vitpe_unfold_u8", off, on, B=B, C=C, S=S, p=p, dtype="bf16",
           off_GBps=round((B * C * S * S * 3) / off[0] / 1e3, 1))     # 1 byte in, one bf16 out per pixel


def steps(off_only):
    from models.vit import VisionTransformer
    from vitpe.data import ResidentDataset
    from vitpe.engine import TrainEngine
    B, n = 512, 50000
    g = torch.Generator(device="cuda").manual_seed(1)
    data, _, _ = dataset(n, 3, 32, g)
    labels = torch.randint(0, 10, (n,), device="cuda", generator=g)
    ds = ResidentDataset(data, labels, (0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010), "cuda")
    idx = [torch.randint(0, n, (B,), device="cuda", generator=g) for _ in range(8)]
    torch.manual_seed(0)
    model = VisionTransformer(img_size=32, patch_size=4, embed_dim=192, depth=6, num_heads=6, pos_encoding="rope-axial").cuda()
    eng = TrainEngine(model, B, compute_dtype=torch.bfloat16, use_graph=True)
    eng.attach_dataset(ds)
    off = timeit(Rotor(idx, eng.step_indexed), iters=100)
    on = None
    if not off_only:
        eng.set_augment(PAD, HFLIP)
        on = timeit(Rotor(idx, eng.step_indexed), iters=100)
    report("TrainEngine.step_indexed", off, on, B=B, depth=6, dtype="bf16")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--off_only", action="store_true")
    ap.add_argument("--skip_steps", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    kernels(a.off_only)
    if not a.skip_steps:
        steps(a.off_only)
