#!/usr/bin/env python3
"""Cost of the erasing stream (RandomErasing inside vitpe_unfold_u8's gather), timed with HIP events; medians of 5 repeats of
200 launches, random sample indices rotating over 8 index batches, prob 0.25:

images:  data.augment_batch's launch -- vitpe_unfold_u8 with p = S and the fp32 img_out -- at B = 512 / CIFAR (3 x 32 x 32)
         over a 50000-record set;
patches: vitpe_unfold_u8 at the 224 / 16 geometry (B = 64, bf16) over a 512-record set;
each as  off / crop 4 + flip / crop 4 + flip + erasing in each fill mode / erasing alone.
Prints one JSON line per measurement; --out FILE appends them there as well."""
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

PAD, HFLIP, PROB = 4, True, 0.25
MODES = ("const", "rand", "pixel")
OUT = None


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


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
    return dict(us=round(statistics.median(out), 2), min_us=round(min(out), 2), max_us=round(max(out), 2))


class Rotor:
    """fn(set) over a ring of operand sets"""

    def __init__(self, sets, fn):
        self.sets, self.fn, self.i = sets, fn, 0

    def __call__(self):
        self.fn(self.sets[self.i])
        self.i = (self.i + 1) % len(self.sets)


def variants(rng):
    aug = dict(rng=rng, crop_pad=PAD, hflip=HFLIP)
    out = [("off", {}), ("crop+flip", aug)]
    out += [(f"crop+flip+erase[{m}]", dict(aug, erase_prob=PROB, erase_mode=m)) for m in MODES]
    out += [(f"erase[{m}] alone", dict(rng=rng, erase_prob=PROB, erase_mode=m)) for m in MODES]
    return out


def measure(name, n, B, C, S, p, T, with_img):
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    data = torch.randint(0, 256, (n, C, S, S), dtype=torch.uint8, device=dev, generator=g)
    mean = torch.tensor((0.4914, 0.4822, 0.4465)[:C], device=dev)
    std = torch.tensor((0.2023, 0.1994, 0.2010)[:C], device=dev)
    idx = [torch.randint(0, n, (B,), device=dev, generator=g) for _ in range(8)]
    pat = torch.empty(B * (S // p) ** 2, C * p * p, dtype=T, device=dev)
    img = torch.empty(B, C, S, S, device=dev) if with_img else None
    base = None
    for variant, kw in variants(K.new_rng_pairs(1, dev)):
        t = timeit(Rotor(idx, lambda i: K.unfold_u8(data, i, mean, std, p, T, out=pat, img_out=img, **kw)))
        base = base or t["us"]
        emit(dict(measure=name, variant=variant, B=B, C=C, S=S, p=p, dtype=str(T).split(".")[-1], **t,
                  over_off=round(t["us"] / base, 3)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="append the JSON lines to this file")
    a = ap.parse_args()
    OUT = a.out
    assert torch.cuda.is_available(), "needs the MI355X"
    measure("augment_batch images (vitpe_unfold_u8, p = S, img_out)", 50000, 512, 3, 32, 32, torch.float32, True)
    measure("vitpe_unfold_u8 patches", 512, 64, 3, 224, 16, torch.bfloat16, False)
