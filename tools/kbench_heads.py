#!/usr/bin/env python3
"""Attention core by head dimension: vitpe_attention_core_fwd / _bwd at B = 512, N = 65 (rope-axial and none, bf16) for hd 24, 32,
48, 96 at d = 192 (H = 192 / hd) and hd 128 at d = 384 (H = 3), HIP-event timed; then the captured bf16 train step of a
depth-6 d = 192 model at H = 4, 6 and 8 (img/s).  H = 6 runs the fused CIFAR kernels, H = 4 / 8 the qkv Linear + core.
Prints one JSON line per measurement."""
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "vit-rpe-rope_amd"))
from vitpe import kernels as K  # noqa: E402


def timeit(fn, iters=50, warm=5):
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


def core_times(B=512, G=8):
    N, T, dev = G * G + 1, torch.bfloat16, "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    for hd, D in ((24, 192), (32, 192), (48, 192), (96, 192), (128, 384)):
        H = D // hd
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
            print(json.dumps({"kernel": "attention_core", "mode": mode, "B": B, "N": N, "d": D, "H": H, "hd": hd,
                              "fwd_us": round(fwd, 2), "bwd_us": round(bwd, 2)}), flush=True)


def step_rate(H, B=512, steps=40, warm=10):
    from vitpe.engine import TrainEngine
    from vitpe.vit import VisionTransformer
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = VisionTransformer(in_chans=3, num_classes=10, pos_encoding="rope-axial", rope_theta=100.0, img_size=32,
                              patch_size=4, embed_dim=192, depth=6, num_heads=H).to(dev)
    eng = TrainEngine(model, B, compute_dtype=torch.bfloat16, use_graph=True)
    g = torch.Generator(device=dev).manual_seed(1234)
    eng.images.copy_(torch.randn(B, 3, 32, 32, generator=g, device=dev))
    eng.labels.copy_(torch.randint(0, 10, (B,), generator=g, device=dev))
    for _ in range(warm):
        eng.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    print(json.dumps({"step": "bf16 captured", "d": 192, "depth": 6, "H": H, "hd": 192 // H, "B": B,
                      "fused_attention": bool(eng.attn_fused), "ms_per_step": round(dt * 1e3, 3),
                      "img_per_s": round(B / dt)}), flush=True)


def main():
    assert torch.cuda.is_available(), "needs the MI355X"
    core_times()
    for H in (6, 4, 8):
        step_rate(H)


if __name__ == "__main__":
    main()
