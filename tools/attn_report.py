#!/usr/bin/env python3
"""Attention statistics of a model as a table: per layer and head the mean attention distance (pixels), the mean row
entropy (nats), the attention mass on the class token and the class row's entropy, averaged over batches --
VisionTransformer.attention_stats, no [N, N] map stored -- and the mean attention-rollout map.  The plot-free counterpart
of the reference's attention visualizers: run it once per --pos_encoding and compare the JSON files.

  tools/attn_report.py --pos_encoding rope-axial --checkpoint checkpoints/cifar10_rope-axial_best.pth --out report.json

--checkpoint: a state_dict as train.py saves it (none: the freshly initialised model).  Batches are synthetic
(seeded standard-normal images) unless --images names a .pt file holding a float tensor [M, C, S, S]."""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "vit-rpe-rope_amd"))
from vitpe import kernels as K  # noqa: E402

SLOTS = {"distance_px": K.STAT_DISTANCE, "entropy": K.STAT_ENTROPY, "cls_mass": K.STAT_CLS_MASS,
         "cls_entropy": K.STAT_CLS_ENTROPY}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pos_encoding", default="rope-axial")
    ap.add_argument("--img_size", type=int, default=32)
    ap.add_argument("--patch_size", type=int, default=4)
    ap.add_argument("--in_chans", type=int, default=3)
    ap.add_argument("--num_classes", type=int, default=10)
    ap.add_argument("--embed_dim", type=int, default=192)
    ap.add_argument("--depth", type=int, default=6)
    ap.add_argument("--num_heads", type=int, default=6)
    ap.add_argument("--checkpoint")
    ap.add_argument("--images", help=".pt file with a float tensor [M, C, S, S]; default: synthetic batches")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--bf16", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", help="write the JSON table here (default: print it)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    from models.vit import VisionTransformer
    torch.manual_seed(a.seed)
    model = VisionTransformer(img_size=a.img_size, patch_size=a.patch_size, in_chans=a.in_chans, num_classes=a.num_classes,
                              embed_dim=a.embed_dim, depth=a.depth, num_heads=a.num_heads, pos_encoding=a.pos_encoding)
    if a.checkpoint:
        model.load_state_dict(torch.load(a.checkpoint, map_location="cpu"))
    model = model.cuda().eval()
    if a.bf16:
        model.set_compute_dtype(torch.bfloat16)
    if a.images:
        data = torch.load(a.images, map_location="cpu").float()
        chunks = [data[i:i + a.batch] for i in range(0, len(data), a.batch)]
    else:
        g = torch.Generator().manual_seed(a.seed)
        chunks = [torch.randn(a.batch, a.in_chans, a.img_size, a.img_size, generator=g) for _ in range(a.batches)]
    total, rollout, n = None, None, 0
    for x in chunks:
        x = x.cuda()
        s = torch.stack([v.double().sum(0) for _, v in sorted(model.attention_stats(x).items())])   # [L, H, 4]
        r = model.attention_rollout(x).double().sum(0)                                               # [N]
        total, rollout, n = (s, r, len(x)) if total is None else (total + s, rollout + r, n + len(x))
    mean, G = (total / n).cpu(), a.img_size // a.patch_size
    report = {"pos_encoding": a.pos_encoding, "checkpoint": a.checkpoint, "images": n, "layers": a.depth, "heads": a.num_heads,
              "grid": G, "patch_size": a.patch_size,
              "per_layer": {name: [round(float(v), 6) for v in mean[..., k].mean(1)] for name, k in SLOTS.items()},
              "per_head": {name: [[round(float(v), 6) for v in row] for row in mean[..., k]] for name, k in SLOTS.items()},
              "rollout_cls": round(float(rollout[0] / n), 6),
              "rollout_map": [[round(float(v), 6) for v in row] for row in (rollout[1:] / n).view(G, G).cpu()]}
    text = json.dumps(report, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)


if __name__ == "__main__":
    main()
