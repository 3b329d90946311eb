#!/usr/bin/env python3
"""Cost of the attention probabilities: vitpe_attention_core_probs (full [B,H,N,N] and cls_only [B,H,N]) against
vitpe_attention_core_fwd of the same build on the same qkv, bf16, rope-axial and none, HIP-event timed, at
  B 512 / N 65 / hd 32 / H 6   (52 MB of probabilities)   and   B 64 / N 197 / hd 64 / H 12   (119 MB).
The kernel is a store stream behind a forward-like prologue, so the figure next to the time is the achieved write bandwidth
4 B H N^2 bytes / time; `fill_us` / `fill_TBps` is torch's fill_ of the same buffers on the same box (tools/membw.py's write
figure) to hold it against.  The outputs rotate over enough buffers (> 256 MB) that no launch finds its lines in the cache.
Prints one JSON line per measurement; --out FILE also writes them there."""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "vit-rpe-rope_amd"))
from vitpe import kernels as K  # noqa: E402


def timeit(fn, iters=40, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3  # us


def measure(B, G, hd, H):
    N, T, dev = G * G + 1, torch.bfloat16, "cuda"
    D = H * hd
    g = torch.Generator(device=dev).manual_seed(0)
    qkv = (torch.randn(B, N, 3 * D, device=dev, generator=g) * 0.5).to(T)
    out = torch.empty(B, N, D, device=dev, dtype=T)
    nbytes = 4 * B * H * N * N
    nbuf = max(2, -(-300_000_000 // nbytes))
    probs = [torch.empty(B, H, N, N, device=dev) for _ in range(nbuf)]
    rows = torch.empty(B, H, N, device=dev)
    k = [0]

    def nxt():
        k[0] += 1
        return probs[k[0] % nbuf]

    fill = timeit(lambda: nxt().fill_(0.5))
    for mode in ("rope-axial", "none"):
        pe = K.PETables(mode, G)
        if mode == "rope-axial":
            inv = 1.0 / (100.0 ** (torch.arange(0, hd // 4, dtype=torch.float) / (hd // 4)))
            pe.cos, pe.sin = K.rope_axial_tables(inv.to(dev), G)
        fwd = timeit(lambda: K.attention_core_fwd(qkv, H, pe, out=out))
        full = timeit(lambda: K.attention_core_probs(qkv, H, pe, out=nxt()))
        cls = timeit(lambda: K.attention_core_probs(qkv, H, pe, cls_only=True, out=rows))
        yield {"kernel": "attention_core_probs", "mode": mode, "B": B, "N": N, "H": H, "hd": hd, "dtype": "bf16",
               "probs_MB": round(nbytes / 1e6, 1), "buffers": nbuf, "core_fwd_us": round(fwd, 2), "probs_us": round(full, 2),
               "probs_write_TBps": round(nbytes / full / 1e6, 3), "cls_only_us": round(cls, 2), "fill_us": round(fill, 2),
               "fill_TBps": round(nbytes / fill / 1e6, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    lines = []
    for geom in ((512, 8, 32, 6), (64, 14, 64, 12)):
        for rec in measure(*geom):
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
