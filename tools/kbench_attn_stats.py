#!/usr/bin/env python3
"""Cost of the attention statistics (vitpe_attention_core_stats), timed with HIP events.  bf16, modes rope-axial and none, at
  B 512 / H 6 / N 65 / hd 32   (52 MB of probabilities a layer)   and   B 64 / H 12 / N 197 / hd 64   (119 MB)
against two yardsticks on the same qkv:
  probs          vitpe_attention_core_probs alone, which does the same arithmetic up to the row sum and stores 4 N^2 bytes
                 per (image, head) where the statistics kernel stores 4 (4 + N);
  probs + torch  attention_core_probs followed by the torch reductions that give the same four numbers (and, for colsum,
                 the weights-times-map product) -- how a user gets them without the kernel.
All arms are timed INTERLEAVED: rounds of one window each, the median and the spread (min, max) over the rounds.  The
probability buffers rotate over more than 300 MB so that no launch finds its lines in the cache.  The results of the kernel
and of the torch reductions are compared once at the timed size (max |d| / max |ref| per slot).

rollout: VisionTransformer.attention_rollout against the same rollout built from attention_maps (head mean, then the row
vector times the [N, N] mean map per layer), on the default CIFAR model (B 512) and a ViT-B/16 geometry (B 64), bf16.
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

OUT = None
SLOTS = ("distance", "entropy", "cls_mass", "cls_entropy")


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3   # us


def interleaved(fns, iters, rounds=7, warm=5):
    """{name: fn} -> {name: dict(us median, min_us, max_us)} over `rounds` alternating windows"""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(window(fn, iters))
    return {k: dict(us=round(statistics.median(v), 2), min_us=round(min(v), 2), max_us=round(max(v), 2)) for k, v in t.items()}


def grid_distances(G, dev):
    t = torch.arange(G * G, device=dev)
    y, x = (t // G).float(), (t % G).float()
    return ((y[:, None] - y[None, :]) ** 2 + (x[:, None] - x[None, :]) ** 2).sqrt()


def torch_stats(p, d, unit):
    """the four numbers of kernels.attention_core_stats from the stored probabilities p [B,H,N,N], in torch on the device"""
    P = p.shape[-1] - 1
    row_ent = -torch.xlogy(p, p).sum(-1)
    return torch.stack([unit / P * (p[..., 1:, 1:] * d).sum((-1, -2)), row_ent.mean(-1), p[..., 1:, 0].sum(-1) / P,
                        row_ent[..., 0]], dim=-1)


def measure_kernel(B, G, hd, H, iters):
    N, T, dev = G * G + 1, torch.bfloat16, "cuda"
    gen = torch.Generator(device=dev).manual_seed(0)
    qkv = (torch.randn(B, N, 3 * H * hd, device=dev, generator=gen) * 0.5).to(T)
    w = torch.rand(B, N, device=dev, generator=gen)
    d, unit = grid_distances(G, dev), 4.0
    nbytes = 4 * B * H * N * N
    nbuf = max(2, -(-300_000_000 // nbytes))
    probs = [torch.empty(B, H, N, N, device=dev) for _ in range(nbuf)]
    outs = (torch.empty(B, H, 4, device=dev), torch.empty(B, H, N, device=dev))
    k = [0]

    def nxt():
        k[0] += 1
        return probs[k[0] % nbuf]

    for mode in ("rope-axial", "none"):
        pe = K.PETables(mode, G)
        if mode == "rope-axial":
            inv = 1.0 / (100.0 ** (torch.arange(0, hd // 4, dtype=torch.float) / (hd // 4)))
            pe.cos, pe.sin = K.rope_axial_tables(inv.to(dev), G)
        p0 = K.attention_core_probs(qkv, H, pe, out=probs[0])
        ref_s, ref_c = torch_stats(p0.double(), d.double(), unit), torch.einsum("bi,bhij->bhj", w.double(), p0.double())
        got_s, got_c = K.attention_core_stats(qkv, H, pe, unit=unit, weights=w)
        err = {n: float((got_s[..., i].double() - ref_s[..., i]).abs().max() / ref_s[..., i].abs().max()) for i, n in enumerate(SLOTS)}
        err["colsum"] = float((got_c.double() - ref_c).abs().max() / ref_c.abs().max())
        del ref_s, ref_c
        t = interleaved({
            "stats": lambda: K.attention_core_stats(qkv, H, pe, unit=unit, out=(outs[0], None)),
            "stats_colsum": lambda: K.attention_core_stats(qkv, H, pe, unit=unit, weights=w, out=outs),
            "probs": lambda: K.attention_core_probs(qkv, H, pe, out=nxt()),
            "probs_torch_stats": lambda: torch_stats(K.attention_core_probs(qkv, H, pe, out=nxt()), d, unit),
            "probs_torch_colsum": lambda: torch.einsum("bi,bhij->bhj", w, K.attention_core_probs(qkv, H, pe, out=nxt())),
        }, iters)
        emit(dict(measure="vitpe_attention_core_stats", mode=mode, B=B, N=N, H=H, hd=hd, dtype="bfloat16", iters=iters,
                  probs_MB=round(nbytes / 1e6, 1), stats_bytes=4 * B * H * (4 + N), buffers=nbuf, **t,
                  stats_over_probs=round(t["stats"]["us"] / t["probs"]["us"], 3),
                  stats_colsum_over_probs=round(t["stats_colsum"]["us"] / t["probs"]["us"], 3),
                  stats_over_probs_torch=round(t["stats"]["us"] / t["probs_torch_stats"]["us"], 3),
                  colsum_over_probs_torch=round(t["stats_colsum"]["us"] / t["probs_torch_colsum"]["us"], 3),
                  rel_err_vs_float64_of_probs=err))


def rollout_from_maps(m, x, residual=0.5):
    maps = m.attention_maps(x)
    B, _, N, _ = maps[0].shape
    v = torch.zeros(B, N, device=x.device)
    v[:, 0] = 1.0
    for l in reversed(range(len(maps))):
        v = (1.0 - residual) * torch.einsum("bi,bij->bj", v, maps[l].mean(1)) + residual * v
    return v


def measure_rollout(name, B, iters, **model_args):
    from models.vit import VisionTransformer
    dev = "cuda"
    torch.manual_seed(0)
    m = VisionTransformer(**model_args).to(dev).set_compute_dtype(torch.bfloat16).eval()
    S = model_args.get("img_size", 32)
    x = torch.randn(B, 3, S, S, device=dev)
    a, b = m.attention_rollout(x), rollout_from_maps(m, x)
    err = float((a - b).abs().max() / b.abs().max())
    with torch.no_grad():
        t = interleaved({"attention_rollout": lambda: m.attention_rollout(x), "rollout_from_maps": lambda: rollout_from_maps(m, x),
                         "eval_forward": lambda: m(x)}, iters)
    emit(dict(measure="VisionTransformer.attention_rollout vs the rollout from attention_maps", model=name, B=B,
              N=int(a.shape[1]), layers=len(m.blocks), heads=m.num_heads, dtype="bfloat16", iters=iters, **t,
              ratio=round(t["attention_rollout"]["us"] / t["rollout_from_maps"]["us"], 3), rel_err_between_the_two=err))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="append the JSON lines to this file")
    a = ap.parse_args()
    OUT = a.out
    assert torch.cuda.is_available(), "needs the MI355X"
    measure_kernel(512, 8, 32, 6, iters=100)
    measure_kernel(64, 14, 64, 12, iters=100)
    measure_rollout("default CIFAR", 512, iters=10)
    measure_rollout("ViT-B/16", 64, iters=5, img_size=224, patch_size=16, embed_dim=768, depth=12, num_heads=12,
                    num_classes=1000, pos_encoding="rope-axial")
