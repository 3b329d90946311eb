#!/usr/bin/env python3
"""Cost of attention-probability dropout: vitpe_attention_core_fwd_drop / _bwd_drop at p = 0.1 against vitpe_attention_core_fwd /
_bwd, bf16, at N = 65 / hd 32 (B = 512, d = 192) and N = 197 / hd 64 (B = 64, d = 768), rope-axial and none, HIP-event timed
(medians of 5 repeats of 50 launches).  Also the elementwise dropout kernel on the [B N, d] activation.  Prints one JSON
line per measurement."""
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


def main(p=0.1):
    assert torch.cuda.is_available(), "needs the MI355X"
    T, dev = torch.bfloat16, "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    rng = K.new_rng_pairs(1, dev)[0]
    for B, G, hd, D in ((512, 8, 32, 192), (64, 14, 64, 768)):
        N, H = G * G + 1, D // hd
        qkv = (torch.randn(B, N, 3 * D, device=dev, generator=g) * 0.5).to(T)
        dout = (torch.randn(B, N, D, device=dev, generator=g) * 0.5).to(T)
        out, dqkv = torch.empty(B, N, D, device=dev, dtype=T), torch.empty(B, N, 3 * D, device=dev, dtype=T)
        for mode in ("rope-axial", "none"):
            pe = K.PETables(mode, G)
            if mode == "rope-axial":
                inv = 1.0 / (100.0 ** (torch.arange(0, hd // 4, dtype=torch.float) / (hd // 4)))
                pe.cos, pe.sin = K.rope_axial_tables(inv.to(dev), G)
            fwd = timeit(lambda: K.attention_core_fwd(qkv, H, pe, out=out))
            bwd = timeit(lambda: K.attention_core_bwd(qkv, dout, H, pe, out=dqkv))
            fwd_d = timeit(lambda: K.attention_core_fwd_drop(qkv, H, pe, rng, p, out=out))
            bwd_d = timeit(lambda: K.attention_core_bwd_drop(qkv, dout, H, pe, rng, p, out=dqkv))
            print(json.dumps({"kernel": "attention_core", "mode": mode, "B": B, "N": N, "d": D, "H": H, "hd": hd, "p": p,
                              "fwd_us": round(fwd, 2), "fwd_drop_us": round(fwd_d, 2), "fwd_ratio": round(fwd_d / fwd, 3),
                              "bwd_us": round(bwd, 2), "bwd_drop_us": round(bwd_d, 2), "bwd_ratio": round(bwd_d / bwd, 3)}),
                  flush=True)
        us = timeit(lambda: K.dropout_fwd(dout, rng, p, resid=dout, out=out))
        print(json.dumps({"kernel": "dropout_fwd+resid", "elements": dout.numel(), "us": round(us, 2),
                          "GBps": round(3 * dout.numel() * 2 / us / 1e3, 1)}), flush=True)


if __name__ == "__main__":
    main()
