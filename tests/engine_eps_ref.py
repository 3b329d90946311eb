"""A depth-2 model of the default CIFAR geometry whose five LayerNorms carry five different eps values, with the weights that
write the residual stream (patch_embed, cls_token, attn.proj, mlp.fc2) shrunk so that the rows every LayerNorm normalises
have a variance within 8x of that LayerNorm's eps.  With nn.LayerNorm's 1e-5 everywhere and residual rows of variance ~1,
the engine could hand any kernel any module's eps unnoticed; here resetting ANY single eps to 1e-5 moves the logits or a
gradient by >= 10x the gate (tests/test_engine_eps_cpu.py asserts it on the oracle, which takes the values as `ln_eps`).
Shared by that file and tests/test_engine_eps_gpu.py.  No GPU and no vitpe import here."""
import torch
import torch.nn.functional as F

from oracle import vit_oracle as O

# in forward order; none of them is the 1e-5 default, and they grow with the residual stream (x + branch contains x)
LN_EPS = {"blocks.0.norm1": 1e-6, "blocks.0.norm2": 4e-6, "blocks.1.norm1": 4e-5, "blocks.1.norm2": 2e-4, "norm": 1e-3}
TAG = "rope-mixed"
GEOM = dict(depth=2)


def bf16_(params):
    for k, v in params.items():
        if v.is_floating_point():
            params[k] = v.to(torch.bfloat16).to(torch.float32)
    return params


def _row_var(x):
    return x.double().var(-1, unbiased=False)


def _scale(params, names, s):
    for n in names:
        params[n] = (params[n] * s).to(torch.bfloat16).to(torch.float32)


def stage_rows(cfg, params, images, ln_eps=LN_EPS):
    """{LayerNorm module name: the rows [B, N, D] it normalises} of the oracle's forward pass."""
    rows = {}
    x = O.patch_embed(cfg, params, images)
    freqs_cis, bias = O.pe_tables(cfg, params)
    d = cfg.embed_dim
    for i in range(cfg.depth):
        pre = f"blocks.{i}."
        rows[pre + "norm1"] = x
        xn = F.layer_norm(x, (d,), params[pre + "norm1.weight"], params[pre + "norm1.bias"], ln_eps[pre + "norm1"])
        a = O.fused_attention(xn, params[pre + "attn.qkv.weight"], cfg.num_heads, freqs_cis, bias)
        x = x + F.linear(a, params[pre + "attn.proj.weight"], params[pre + "attn.proj.bias"])
        rows[pre + "norm2"] = x
        xn = F.layer_norm(x, (d,), params[pre + "norm2.weight"], params[pre + "norm2.bias"], ln_eps[pre + "norm2"])
        x = x + O.mlp(xn, params[pre + "mlp.fc1.weight"], params[pre + "mlp.fc1.bias"], params[pre + "mlp.fc2.weight"],
                      params[pre + "mlp.fc2.bias"])
    rows["norm"] = x
    return rows


def calibrated_params(cfg, images, ln_eps=LN_EPS):
    """The oracle's closed-form parameters (bf16-representable) with each writer of the residual stream scaled once, in
    forward order, so that the median row variance at the next LayerNorm equals that LayerNorm's eps."""
    params = bf16_(O.closed_form_params(cfg))
    order = list(ln_eps)                               # forward order
    writers = [["patch_embed.weight", "patch_embed.bias"]]
    for i in range(cfg.depth):
        writers += [[f"blocks.{i}.attn.proj.weight", f"blocks.{i}.attn.proj.bias"],
                    [f"blocks.{i}.mlp.fc2.weight", f"blocks.{i}.mlp.fc2.bias"]]
    for name, ws in zip(order, writers):
        for _ in range(2):                             # (x + branch is not linear in the branch's scale: one refinement)
            v = _row_var(stage_rows(cfg, params, images, ln_eps)[name][:, 1:] if name == order[0] else
                         stage_rows(cfg, params, images, ln_eps)[name])
            _scale(params, ws, float((ln_eps[name] / v.median()).sqrt()))
        if name == order[0]:                           # the class-token row is cls_token alone
            v = _row_var(params["cls_token"].reshape(1, -1))
            _scale(params, ["cls_token"], float((ln_eps[name] / v).sqrt()))
    return params


def variance_fraction(rows, eps):
    v = _row_var(rows).reshape(-1)
    return float(((v >= eps / 8) & (v <= 8 * eps)).double().mean())


def batch(cfg, B, seed=11):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, cfg.in_chans, cfg.img_size, cfg.img_size, generator=g),
            torch.randint(0, cfg.num_classes, (B,), generator=g))


def worst_ratio(got, ref, logit_gate=1e-4, grad_gate=1e-3):
    """max over (logits, every gradient) of rel error / its gate, for (logits, loss, grads) triples of the oracle"""
    from conftest import rel_err
    r = rel_err(got[0], ref[0]) / logit_gate
    for n, g in ref[2].items():
        if g is not None and float(g.abs().max()) > 0:
            r = max(r, rel_err(got[2][n], g) / grad_gate)
    return r
