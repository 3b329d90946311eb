"""float64 references of the gradient-weighted attention relevance (vitpe_attention_core_relevance; Chefer, Gur & Wolf,
"Generic Attention-model Explainability", ICCV 2021: R <- R + A~ R).

For one block and head, with A the softmax the reference calls `attn` (models/vit.py:71-84), V the head's value rows of the
qkv projection and dO the gradient of a scalar w.r.t. the merged-head output in front of proj:
  G = dO_h V_h^T                              the gradient w.r.t. A with V held fixed (ref_grad_attn)
  colsum_j = sum_i w_i f(G_ij A_ij)           f = max(0, .) with clamp, the identity without (ref_relevance)
  A~ = mean_h f(G . A),  R = (I + A~_{L-1}) ... (I + A~_start),  result = R's class row (ref_relevance_rollout)
ref_model_relevance restates the reference's forward with the oracle's own helpers and reads A.grad after logit.backward().

The error measure of the tests: max|got - ref| / max(colsum_abs), colsum_abs_j = sum_i |w_i| |G_ij A_ij| -- the suite's
rel_err where every term is non-negative, and bounded under cancellation where they are signed."""
import torch
import torch.nn.functional as F

from oracle import vit_oracle as O


def ref_grad_attn(qkv, dout, H):
    """qkv [B, N, 3D], dout [B, N, D] -> float64 G [B, H, N, N], G[b, h, i, j] = dout[b, i, h-th head] . v[b, j, h-th head]"""
    B, N, D3 = qkv.shape
    D = D3 // 3
    v = qkv.double().reshape(B, N, 3, H, D // H).permute(2, 0, 3, 1, 4)[2]          # [B, H, N, hd]
    do = dout.double().reshape(B, N, H, D // H).permute(0, 2, 1, 3)                # [B, H, N, hd]
    return do @ v.transpose(-2, -1)


def ref_relevance(p, G, w, clamp):
    """p, G [B, H, N, N], w [B, N] -> float64 (colsum, colsum_abs), both [B, H, N]"""
    t = G.double() * p.double()
    f = t.clamp(min=0.0) if clamp else t
    return (torch.einsum("bi,bhij->bhj", w.double(), f), torch.einsum("bi,bhij->bhj", w.double().abs(), t.abs()))


def err_measure(got, ref, ref_abs):
    """max|got - ref| / max(colsum_abs)"""
    return float((got.detach().cpu().double() - ref.double()).abs().max() / ref_abs.double().abs().max())


def ref_relevance_rollout(abars):
    """abars: the layers' A~ [B, N, N], bottom block of the product first -> float64 [B, N]: the class token's row of
    (I + A~_last) ... (I + A~_first), propagated as a row vector from the top block down: v <- v + v A~_l."""
    B, N, _ = abars[0].shape
    v = torch.zeros(B, N, dtype=torch.float64)
    v[:, 0] = 1.0
    for a in reversed(abars):
        v = v + torch.einsum("bi,bij->bj", v, a.double())
    return v


def model_forward(cfg, params, images, retain=False):
    """O.forward restated with the oracle's own helpers and an explicit softmax -> (logits, [attn [B, H, N, N] per block]);
    retain: every attn keeps its .grad after a backward"""
    x = O.patch_embed(cfg, params, images)
    freqs_cis, bias = O.pe_tables(cfg, params)
    d, H, hd = cfg.embed_dim, cfg.num_heads, cfg.head_dim
    attns = []
    for i in range(cfg.depth):
        pre = f"blocks.{i}."
        xn = F.layer_norm(x, (d,), params[pre + "norm1.weight"], params[pre + "norm1.bias"], 1e-5)
        B, N, _ = xn.shape
        q, k, v = F.linear(xn, params[pre + "attn.qkv.weight"], params.get(pre + "attn.qkv.bias")) \
            .reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
        if freqs_cis is not None:
            cos, sin = freqs_cis
            q_p, k_p = O.apply_rotary_emb(q[:, :, 1:], k[:, :, 1:], O.reshape_for_broadcast(cos, q[:, :, 1:]),
                                          O.reshape_for_broadcast(sin, q[:, :, 1:]))
            q, k = torch.cat([q[:, :, :1], q_p], dim=2), torch.cat([k[:, :, :1], k_p], dim=2)
        s = (q @ k.transpose(-2, -1)) * hd ** -0.5
        if bias is not None:
            s = s + bias
        attn = s.softmax(dim=-1)
        if retain:
            attn.retain_grad()
        attns.append(attn)
        a = (attn @ v).transpose(1, 2).reshape(B, N, d)
        x = x + F.linear(a, params[pre + "attn.proj.weight"], params[pre + "attn.proj.bias"])
        xn = F.layer_norm(x, (d,), params[pre + "norm2.weight"], params[pre + "norm2.bias"], 1e-5)
        x = x + O.mlp(xn, params[pre + "mlp.fc1.weight"], params[pre + "mlp.fc1.bias"], params[pre + "mlp.fc2.weight"],
                      params[pre + "mlp.fc2.bias"])
    x = F.layer_norm(x, (d,), params["norm.weight"], params["norm.bias"], 1e-5)
    return F.linear(x[:, 0], params["head.weight"], params["head.bias"]), attns


def ref_model_relevance(cfg, params, images, target=None, start=0, clamp=True):
    """-> (relevance float64 [B, N], logits float64 [B, classes], the target used [B], scale float64 [B, N]).  params:
    {state_dict key: tensor} (used in float64); target None: the arg-max class.  scale: the same propagation with
    mean_h |G . A| in place of mean_h f(G . A), minus e_cls -- the model-level counterpart of colsum_abs (what the terms
    of the result add up to in magnitude, without the identity's 1, which would hide every patch entry)."""
    params = {k: v.detach().double().requires_grad_(True) if v.is_floating_point() else v for k, v in params.items()}
    logits, attns = model_forward(cfg, params, images.double(), retain=True)
    if target is None:
        target = logits.detach().argmax(dim=1)
    logits.gather(1, target.view(-1, 1)).sum().backward()
    abars, mags = [], []
    for a in attns[start:]:
        t = a.grad * a.detach()
        abars.append((t.clamp(min=0.0) if clamp else t).mean(dim=1))
        mags.append(t.abs().mean(dim=1))
    scale = ref_relevance_rollout(mags)
    scale[:, 0] -= 1.0
    return ref_relevance_rollout(abars), logits.detach(), target, scale
