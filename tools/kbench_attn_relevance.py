#!/usr/bin/env python3
"""Cost of the gradient-weighted attention relevance (vitpe_attention_core_relevance), timed with HIP events.  bf16, modes
rope-axial and none, at
  B 512 / H 6 / N 65 / hd 32   (52 MB of probabilities a layer)   and   B 64 / H 12 / N 197 / hd 64   (119 MB)
against two yardsticks on the same qkv / dout / weights:
  stats_colsum   vitpe_attention_core_stats with weights, the kernel it extends (same arithmetic up to the row sum, no V
                 tile, no second MFMA pass) -- recorded, not gated;
  probs + torch  attention_core_probs, then G = einsum(dO, V) as a second [B,H,N,N] tensor, the product, the clamp and the
                 weights-times-map einsum in torch on the device -- how a user gets the same colsum without the kernel.
All arms are timed INTERLEAVED: rounds of one window each, the median and the spread (min, max) over the rounds.  The
probability buffers rotate over more than 300 MB so that no launch finds its lines in the cache.  The two results are
compared once at the timed size (max |d| / max sum_i |w_i| |G_ij A_ij|).

model: VisionTransformer.attention_relevance against the same relevance from attention_maps (the stored [B,H,N,N]
probabilities) + autograd hooks on the attention modules (their input, and the gradient at their output), and against
saliency (one forward + backward on the same path), on the default CIFAR model (B 512) and a ViT-B/16 geometry (B 64), bf16.
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


def torch_relevance(p, qkv, dout, w, H, clamp=True):
    """colsum [B,H,N] from the stored probabilities p [B,H,N,N]: G as a second [B,H,N,N] tensor, all in torch on the device"""
    B, N, D3 = qkv.shape
    hd = D3 // 3 // H
    v = qkv.view(B, N, 3, H, hd)[:, :, 2]
    g = torch.einsum("bihd,bjhd->bhij", dout.view(B, N, H, hd), v).float()
    t = g * p
    if clamp:
        t = t.clamp_(min=0.0)
    return torch.einsum("bi,bhij->bhj", w, t)


def measure_kernel(B, G, hd, H, iters):
    N, T, dev = G * G + 1, torch.bfloat16, "cuda"
    gen = torch.Generator(device=dev).manual_seed(0)
    qkv = (torch.randn(B, N, 3 * H * hd, device=dev, generator=gen) * 0.5).to(T)
    dout = (torch.randn(B, N, H * hd, device=dev, generator=gen) * 0.5).to(T)
    w = torch.rand(B, N, device=dev, generator=gen)
    nbytes = 4 * B * H * N * N
    nbuf = max(2, -(-300_000_000 // nbytes))
    probs = [torch.empty(B, H, N, N, device=dev) for _ in range(nbuf)]
    out = torch.empty(B, H, N, device=dev)
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
        v = qkv.view(B, N, 3, H, hd)[:, :, 2].double()
        g0 = torch.einsum("bihd,bjhd->bhij", dout.view(B, N, H, hd).double(), v)
        t0 = g0 * p0.double()
        ref, mag = torch.einsum("bi,bhij->bhj", w.double(), t0.clamp(min=0.0)), torch.einsum("bi,bhij->bhj", w.double(), t0.abs())
        del g0, t0, v
        got = K.attention_core_relevance(qkv, dout, H, pe, w)
        err = float((got.double() - ref).abs().max() / mag.max())
        err_torch = float((torch_relevance(p0, qkv, dout, w, H).double() - ref).abs().max() / mag.max())
        del ref, mag
        t = interleaved({
            "relevance": lambda: K.attention_core_relevance(qkv, dout, H, pe, w, out=out),
            "relevance_signed": lambda: K.attention_core_relevance(qkv, dout, H, pe, w, clamp=False, out=out),
            "stats_colsum": lambda: K.attention_core_stats(qkv, H, pe, weights=w, out=outs),
            "probs": lambda: K.attention_core_probs(qkv, H, pe, out=nxt()),
            "probs_torch_relevance": lambda: torch_relevance(K.attention_core_probs(qkv, H, pe, out=nxt()), qkv, dout, w, H),
        }, iters)
        emit(dict(measure="vitpe_attention_core_relevance", mode=mode, B=B, N=N, H=H, hd=hd, dtype="bfloat16", iters=iters,
                  probs_MB=round(nbytes / 1e6, 1), colsum_bytes=4 * B * H * N, buffers=nbuf, **t,
                  relevance_over_stats_colsum=round(t["relevance"]["us"] / t["stats_colsum"]["us"], 3),
                  relevance_over_probs=round(t["relevance"]["us"] / t["probs"]["us"], 3),
                  relevance_over_probs_torch=round(t["relevance"]["us"] / t["probs_torch_relevance"]["us"], 3),
                  err_vs_float64_of_probs=err, err_of_the_torch_route=err_torch))


def relevance_from_maps(m, x, clamp=True):
    """the relevance of attention_relevance(x) the stored-maps way: attention_maps for the probabilities, forward hooks on
    the attention modules for their inputs, full backward hooks for the gradient at their outputs, the rest in torch"""
    maps = m.attention_maps(x)
    ins, douts, hooks = {}, {}, []
    for l, blk in enumerate(m.blocks):
        hooks.append(blk.attn.register_forward_hook(lambda mod, args, out, l=l: ins.__setitem__(l, args[0].detach())))
        hooks.append(blk.attn.register_full_backward_hook(lambda mod, gi, go, l=l: douts.__setitem__(l, go[0].detach())))
    try:
        with torch.no_grad():
            tok = m._embed(x)
        with torch.enable_grad():
            tok = tok.requires_grad_(True)
            P = (x.shape[-1] // m.patch_size) ** 2
            logits = m._head(m._blocks(tok, P))
            picked = logits.gather(1, logits.detach().argmax(dim=1).view(-1, 1)).sum()
            torch.autograd.grad(picked, inputs=[tok])
    finally:
        for h in hooks:
            h.remove()
    with torch.no_grad():
        B, N, C = ins[0].shape
        H = m.num_heads
        v = torch.zeros(B, N, device=x.device)
        v[:, 0] = 1.0
        for l in reversed(range(len(m.blocks))):
            a = m.blocks[l].attn
            qkv = torch.nn.functional.linear(ins[l], a.qkv.weight.to(ins[l].dtype),
                                             None if a.qkv.bias is None else a.qkv.bias.to(ins[l].dtype))
            do = douts[l] @ a.proj.weight.to(douts[l].dtype)
            g = torch.einsum("bihd,bjhd->bhij", do.view(B, N, H, C // H), qkv.view(B, N, 3, H, C // H)[:, :, 2]).float()
            t = g * maps[l]
            if clamp:
                t = t.clamp_(min=0.0)
            v = v + torch.einsum("bi,bij->bj", v, t.mean(1))
        return v


def measure_model(name, B, iters, **model_args):
    from vitpe.vit import VisionTransformer
    dev = "cuda"
    torch.manual_seed(0)
    m = VisionTransformer(**model_args).to(dev).set_compute_dtype(torch.bfloat16).eval()
    S = model_args.get("img_size", 32)
    x = torch.randn(B, 3, S, S, device=dev)
    a, b = m.attention_relevance(x), relevance_from_maps(m, x)
    e_cls = torch.zeros_like(b)
    e_cls[:, 0] = 1.0
    err = float((a - b).abs().max() / (b - e_cls).abs().max())
    t = interleaved({"attention_relevance": lambda: m.attention_relevance(x), "relevance_from_maps": lambda: relevance_from_maps(m, x),
                     "saliency": lambda: m.saliency(x)}, iters, rounds=5, warm=2)
    with torch.no_grad():
        t.update(interleaved({"eval_forward": lambda: m(x)}, iters, rounds=5, warm=2))
    emit(dict(measure="VisionTransformer.attention_relevance vs the relevance from attention_maps + hooks", model=name, B=B,
              N=int(a.shape[1]), layers=len(m.blocks), heads=m.num_heads, dtype="bfloat16", iters=iters, **t,
              ratio_to_maps=round(t["attention_relevance"]["us"] / t["relevance_from_maps"]["us"], 3),
              ratio_to_saliency=round(t["attention_relevance"]["us"] / t["saliency"]["us"], 3),
              err_between_the_two_without_identity=err))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="append the JSON lines to this file")
    ap.add_argument("--only", choices=["kernel", "model"], help="one half of the measurements")
    a = ap.parse_args()
    OUT = a.out
    assert torch.cuda.is_available(), "needs the MI355X"
    if a.only != "model":
        measure_kernel(512, 8, 32, 6, iters=100)
        measure_kernel(64, 14, 64, 12, iters=100)
    if a.only != "kernel":
        measure_model("default CIFAR", 512, iters=10)
        measure_model("ViT-B/16", 64, iters=5, img_size=224, patch_size=16, embed_dim=768, depth=12, num_heads=12,
                      num_classes=1000, pos_encoding="rope-axial")
