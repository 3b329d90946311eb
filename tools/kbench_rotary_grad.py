#!/usr/bin/env python3
"""The attention-core backward with and without the gradients w.r.t. caller rotary tables (vitpe_attention_core_bwd vs
vitpe_attention_core_bwd_tables, bf16), HIP-event timed: B = 512 / N = 65 / hd 32 (d = 192, H = 6) and B = 64 / N = 197 /
hd 64 (d = 768, H = 12), with 2-D (rope-axial) and 3-D (rope-mixed) tables.  The table variant includes its slab
reduction and the workspace from the caching allocator.  Prints one JSON line per measurement."""
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "vit-rpe-rope_amd"))
from vitpe import kernels as K  # noqa: E402
from kbench_heads import timeit  # noqa: E402


def main():
    assert torch.cuda.is_available(), "needs the MI355X"
    dev, T = "cuda", torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(0)
    for B, G, D, H in ((512, 8, 192, 6), (64, 14, 768, 12)):
        N, hd = G * G + 1, D // H
        qkv = (torch.randn(B, N, 3 * D, device=dev, generator=g) * 0.5).to(T)
        dout = (torch.randn(B, N, D, device=dev, generator=g) * 0.5).to(T)
        dqkv = torch.empty_like(qkv)
        for mode, shape in (("rope-axial", (N - 1, hd // 2)), ("rope-mixed", (H, N - 1, hd // 2))):
            pe = K.PETables(mode, G, cos=torch.rand(shape, device=dev, generator=g),
                            sin=torch.rand(shape, device=dev, generator=g))
            dfr = torch.zeros(2, H, hd // 2, device=dev)
            dc, ds = torch.zeros(shape, device=dev), torch.zeros(shape, device=dev)
            plain = timeit(lambda: K.attention_core_bwd(qkv, dout, H, pe, None, None, dfr, out=dqkv))
            tabs = timeit(lambda: K.attention_core_bwd(qkv, dout, H, pe, out=dqkv, dcos=dc, dsin=ds))
            print(json.dumps({"kernel": "attention_core_bwd", "mode": mode, "B": B, "N": N, "d": D, "H": H, "hd": hd,
                              "plain_us": round(plain, 2), "tables_us": round(tabs, 2),
                              "ratio": round(tabs / plain, 3)}), flush=True)


if __name__ == "__main__":
    main()
