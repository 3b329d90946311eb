"""torch.library custom ops over the HIP kernels: `torch.ops.vitpe.*`.

Forward ops return the tensors their backward needs; backward is registered with
`register_autograd` and is hand-written on the same kernels (the reference relies on
autograd over ATen ops; here the gradients are explicit).  Parameters arrive as the fp32
masters; the compute type of the GEMMs follows the activation dtype (float32 = exact-fp32
MFMA parity mode, bfloat16 = throughput mode) and weight shadows are produced on the fly.
Parameter gradients are returned in fp32.

Each hand-written backward is a custom op of its own (`vitpe::<op>_backward`, with a fake like the forward ops): the
function handed to `register_autograd` has to be traceable, and one that hands data pointers to the library is not --
under torch.compile / AOT autograd it would be run on fake tensors.  A custom op cannot return None, so a gradient that
does not exist (no qkv bias, no PE parameter, constant tables) leaves a backward op as an empty tensor; `_opt` turns it
back into None.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch
from torch import Tensor

from . import _lib as L
from . import kernels as K

MODES = ["none", "absolute", "relative", "polynomial", "rope-axial", "rope-mixed"]


def _opt(t: Tensor) -> Optional[Tensor]:
    return None if t.numel() == 0 else t


def _zeros(t: Tensor) -> Tensor:
    return torch.zeros(t.shape, dtype=t.dtype, device=t.device)


def _shadow(w: Tensor, dtype) -> Tensor:
    return w.contiguous() if dtype == torch.float32 else K.cast(w.contiguous(), dtype)


def _shadow_t(w: Tensor, dtype) -> Tensor:
    return K.transpose_cast(w.contiguous(), dtype)


def _pe_tables(mode: int, grid: int, pe_param: Optional[Tensor], inv_freq: Optional[Tensor], degree: int,
               per_head: bool, cos: Optional[Tensor] = None, sin: Optional[Tensor] = None) -> K.PETables:
    name = MODES[mode]
    t = K.PETables(name, grid, degree=degree, coeff_per_head=per_head)
    if cos is not None:   # the caller's own (cos, sin) tables (reference vit.py:51-64 rotates with what it is handed)
        t.cos, t.sin = cos.float().contiguous(), sin.float().contiguous()
        return t
    if name == "relative":
        t.table = pe_param.contiguous()
    elif name == "polynomial":
        t.coeff = pe_param.contiguous()
    elif name == "rope-axial":
        t.cos, t.sin = K.rope_axial_tables(inv_freq.contiguous(), grid)
    elif name == "rope-mixed":
        t.cos, t.sin = K.rope_mixed_tables(pe_param.contiguous(), grid)
    return t


# ---- layer_norm ---------------------------------------------------------------------------
@torch.library.custom_op("vitpe::layer_norm", mutates_args=())
def layer_norm(x: Tensor, weight: Tensor, bias: Tensor, eps: float) -> Tuple[Tensor, Tensor, Tensor]:
    y, mean, rstd = K.layernorm_fwd(x.contiguous(), weight, bias, eps)
    return y, mean, rstd


# The fakes answer with what the real ops return: freshly allocated CONTIGUOUS tensors whatever the strides of the inputs
# (every op works on x.contiguous(); torch.empty_like of a transposed input would keep its strides).
@layer_norm.register_fake
def layer_norm_fake(x, weight, bias, eps):
    m = x.numel() // x.shape[-1]
    return x.new_empty(x.shape), x.new_empty(m, dtype=torch.float32), x.new_empty(m, dtype=torch.float32)


def _ln_setup(ctx, inputs, output):
    x, weight, _, _ = inputs
    _, mean, rstd = output
    ctx.save_for_backward(x, weight, mean, rstd)


@torch.library.custom_op("vitpe::layer_norm_backward", mutates_args=())
def layer_norm_backward(dy: Tensor, x: Tensor, weight: Tensor, mean: Tensor, rstd: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """-> (dx, dweight, dbias)"""
    dg, db = _zeros(weight), _zeros(weight)
    dx = K.layernorm_bwd(dy.contiguous(), x.contiguous(), mean, rstd, weight, dg, db)
    return dx, dg, db


@layer_norm_backward.register_fake
def layer_norm_backward_fake(dy, x, weight, mean, rstd):
    return x.new_empty(x.shape), weight.new_empty(weight.shape), weight.new_empty(weight.shape)


def _ln_backward(ctx, dy, _dm, _dr):
    x, weight, mean, rstd = ctx.saved_tensors
    dx, dg, db = torch.ops.vitpe.layer_norm_backward(dy, x, weight, mean, rstd)
    return dx, dg, db, None


layer_norm.register_autograd(_ln_backward, setup_context=_ln_setup)


# ---- attention: y = [resid +] proj(fused_attention(xn)) ----------------------------------------
def _fused_ok(xn: Tensor, num_heads: int) -> bool:
    B, N, D = xn.shape
    return bool(L.lib().vitpe_fused_attention_supported(L.dtype_code(xn.dtype), N, D, D // num_heads))


def _attention_forward(op: str, one_kernel: bool, xn, wqkv, bqkv, wproj, bproj, resid, num_heads, mode, grid, pe_param,
                       inv_freq, degree, per_head, cos, sin, tables_grad, attn_p, proj_p, rng):
    """-> (y, a, qkv), the forward of both attention ops (`op`: the name their errors carry).  one_kernel: the routes
    that fuse the qkv projection into the attention kernel are allowed (they have no bias input, no dropout and no table
    gradients); otherwise, and where none of them fits: qkv Linear (panel GEMM) + the per-(image, head) attention core."""
    dt = xn.dtype
    B, N, D = xn.shape
    t = _pe_tables(mode, grid, pe_param, inv_freq, degree, per_head, cos, sin)
    if tables_grad and attn_p > 0.0:
        raise NotImplementedError(f"{op}: gradients of caller rotary tables together with attn_drop > 0")
    if tables_grad and (cos is None or MODES[mode] not in ("rope-axial", "rope-mixed")):
        raise L.VitpeError(f"{op}: tables_grad needs caller (cos, sin) tables in a rope mode")
    if (attn_p > 0.0 or proj_p > 0.0) and (rng is None or tuple(rng.shape) != (2, 2)):
        raise L.VitpeError(f"{op}: dropout needs rng, a [2, 2] int64 device tensor")
    one_kernel = one_kernel and not tables_grad   # (the backward with table gradients is the core's: it reads qkv)
    if one_kernel and _fused_ok(xn, num_heads):
        if K.fused_attention_wide_supported(dt, N, D, D // num_heads):
            a = K.fused_attention_fwd_wide(xn.contiguous(), K.pack_qkv_weights_wide(wqkv.contiguous(), dt, num_heads), num_heads, t)
        else:
            a = K.fused_attention_fwd(xn.contiguous(), K.pack_qkv_weights(wqkv.contiguous(), dt, num_heads), num_heads, t)
        qkv = xn.new_empty(0)
    elif one_kernel and K.attention_fused64_supported(dt, N, num_heads, D // num_heads):
        # ViT-B/16 geometry: projection + PE + core in one kernel; the raw projection is its side output (the core
        # backward reads it)
        qkv = xn.new_empty((B, N, 3 * D))
        a = K.attention_fused64_fwd(xn.contiguous(), K.pack_weight_frags(wqkv.contiguous().float(), dt, 64, 0), num_heads, t,
                                    qkv_out=qkv)
    else:
        qkv = K.linear(xn.contiguous().view(B * N, D), _shadow(wqkv, dt), bqkv, epi=L.EPI_BIAS).view(B, N, 3 * D)
        if attn_p > 0.0:
            a = K.attention_core_fwd_drop(qkv, num_heads, t, rng[0], attn_p)
        else:
            a = K.attention_core_fwd(qkv, num_heads, t)
    r2 = None if resid is None else resid.contiguous().view(B * N, D)
    if proj_p > 0.0:
        y = K.linear(a.view(B * N, D), _shadow(wproj, dt), bproj, epi=L.EPI_BIAS)
        y = K.dropout_fwd(y, rng[1], proj_p, resid=r2)
    elif r2 is None:
        y = K.linear(a.view(B * N, D), _shadow(wproj, dt), bproj, epi=L.EPI_BIAS)
    else:
        y = K.linear(a.view(B * N, D), _shadow(wproj, dt), bproj, epi=L.EPI_BIAS_RESID, resid=r2)
    return y.view(B, N, D), a, qkv


def _attention_setup(ctx, output, one_kernel, xn, wqkv, bqkv, wproj, resid, num_heads, mode, grid, pe_param, inv_freq, degree,
                     per_head, cos, sin, tables_grad, attn_p, proj_p, rng):
    _, a, qkv = output
    ctx.save_for_backward(xn, wqkv, wproj, a, qkv, pe_param, inv_freq, cos, sin, rng)
    ctx.meta = (one_kernel, num_heads, mode, grid, degree, per_head, resid is not None, tables_grad, bqkv is not None, attn_p,
                proj_p)


@torch.library.custom_op("vitpe::attention_backward", mutates_args=())
def attention_backward(dy: Tensor, xn: Tensor, wqkv: Tensor, wproj: Tensor, a: Tensor, qkv: Tensor, pe_param: Optional[Tensor],
                       inv_freq: Optional[Tensor], cos: Optional[Tensor], sin: Optional[Tensor], rng: Optional[Tensor],
                       one_kernel: bool, num_heads: int, mode: int, grid: int, degree: int, per_head: bool, tables_grad: bool,
                       has_bqkv: bool, attn_p: float, proj_p: float
                       ) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """-> (dxn, dwqkv, dbqkv, dwproj, dbproj, dpe, dcos, dsin), the backward of both attention ops on what their forward
    saved; the gradients that do not exist are empty tensors."""
    dt = xn.dtype
    B, N, D = xn.shape
    dy2 = dy.contiguous().view(B * N, D)
    if proj_p > 0.0:   # d(proj output) = dy . m / (1 - p), the proj site's mask regenerated; the residual takes dy itself
        dy2 = K.dropout_bwd(dy2, rng[1], proj_p)
    # proj: da = dy Wproj ; dWproj = dy^T a ; dbproj = colsum(dy)
    da = K.linear(dy2, _shadow_t(wproj, dt), None, epi=L.EPI_BIAS)
    dwproj = _zeros(wproj)
    dbproj = torch.zeros(D, dtype=torch.float32, device=dy.device)
    K.gemm_tn(dy2, a.view(B * N, D), dwproj, dbproj)
    # attention backward -> dqkv (+ PE parameter grads)
    t = _pe_tables(mode, grid, pe_param, inv_freq, degree, per_head, cos, sin)
    dpe = _zeros(pe_param) if pe_param is not None else None
    name = MODES[mode]
    pe_grads = dict(dtable=dpe if name == "relative" else None, dcoeff=dpe if name == "polynomial" else None,
                    dfreqs=dpe if name == "rope-mixed" else None)
    if cos is not None and name == "rope-mixed":   # caller-supplied tables are constants: the kernel's frequency gradient is discarded
        pe_grads["dfreqs"] = torch.zeros(2, num_heads, D // num_heads // 2, dtype=torch.float32, device=xn.device)
        dpe = None
    dcos = dsin = None
    if attn_p > 0.0:   # the attention-probability mask regenerated inside the core
        dqkv = K.attention_core_bwd_drop(qkv, da.view(B, N, D), num_heads, t, rng[0], attn_p, **pe_grads)
    elif tables_grad:   # gradients w.r.t. the caller's tables (vitpe_attention_core_bwd_tables), fp32 like t.cos / t.sin
        dcos, dsin = torch.zeros_like(t.cos), torch.zeros_like(t.sin)
        dqkv = K.attention_core_bwd(qkv, da.view(B, N, D), num_heads, t, dcos=dcos, dsin=dsin)
        dcos, dsin = dcos.view(cos.shape).to(cos.dtype), dsin.view(sin.shape).to(sin.dtype)
    elif one_kernel and qkv.numel() == 0:   # the forward was the kernel that keeps qkv on the chip
        dqkv = K.fused_attention_bwd(xn.contiguous(), K.pack_qkv_weights(wqkv.contiguous(), dt, num_heads),
                                     da.view(B, N, D), num_heads, t, **pe_grads)
    else:
        dqkv = K.attention_core_bwd(qkv, da.view(B, N, D), num_heads, t, **pe_grads)
    dq2 = dqkv.view(B * N, 3 * D)
    dxn = K.linear(dq2, _shadow_t(wqkv, dt), None, epi=L.EPI_BIAS).view(B, N, D)
    dwqkv = _zeros(wqkv)
    dbqkv = torch.zeros(3 * D, dtype=torch.float32, device=dy.device) if has_bqkv else None   # gemm_tn's dbias: colsum(dqkv)
    K.gemm_tn(dq2, xn.contiguous().view(B * N, D), dwqkv, dbqkv)
    dbqkv, dpe, dcos, dsin = (xn.new_empty(0) if g is None else g for g in (dbqkv, dpe, dcos, dsin))   # (one tensor each)
    return dxn, dwqkv, dbqkv, dwproj, dbproj, dpe, dcos, dsin


@attention_backward.register_fake
def attention_backward_fake(dy, xn, wqkv, wproj, a, qkv, pe_param, inv_freq, cos, sin, rng, one_kernel, num_heads, mode, grid,
                            degree, per_head, tables_grad, has_bqkv, attn_p, proj_p):
    D = xn.shape[-1]
    f32 = dict(dtype=torch.float32)
    no_dpe = pe_param is None or (cos is not None and MODES[mode] == "rope-mixed")
    tabs = tables_grad and attn_p == 0.0
    return (xn.new_empty(xn.shape), wqkv.new_empty(wqkv.shape), xn.new_empty(3 * D, **f32) if has_bqkv else xn.new_empty(0),
            wproj.new_empty(wproj.shape), xn.new_empty(D, **f32), xn.new_empty(0) if no_dpe else pe_param.new_empty(pe_param.shape),
            cos.new_empty(cos.shape) if tabs else xn.new_empty(0), sin.new_empty(sin.shape) if tabs else xn.new_empty(0))


def _attention_backward(ctx, dy):
    """-> (dxn, dwqkv, dbqkv, dwproj, dbproj, dresid, dpe, dcos, dsin), the backward of both attention ops."""
    xn, wqkv, wproj, a, qkv, pe_param, inv_freq, cos, sin, rng = ctx.saved_tensors
    one_kernel, num_heads, mode, grid, degree, per_head, has_resid, tables_grad, has_bqkv, attn_p, proj_p = ctx.meta
    dxn, dwqkv, dbqkv, dwproj, dbproj, dpe, dcos, dsin = torch.ops.vitpe.attention_backward(
        dy, xn, wqkv, wproj, a, qkv, pe_param, inv_freq, cos, sin, rng, one_kernel, num_heads, mode, grid, degree, per_head,
        tables_grad, has_bqkv, attn_p, proj_p)
    return dxn, dwqkv, _opt(dbqkv), dwproj, dbproj, dy if has_resid else None, _opt(dpe), _opt(dcos), _opt(dsin)


@torch.library.custom_op("vitpe::attention", mutates_args=())
def attention(xn: Tensor, wqkv: Tensor, wproj: Tensor, bproj: Tensor, resid: Optional[Tensor], num_heads: int,
              mode: int, grid: int, pe_param: Optional[Tensor], inv_freq: Optional[Tensor], degree: int,
              per_head: bool, cos: Optional[Tensor] = None, sin: Optional[Tensor] = None,
              tables_grad: bool = False) -> Tuple[Tensor, Tensor, Tensor]:
    """-> (y, a, qkv).  CIFAR geometry: one fused kernel (qkv never leaves the chip, `qkv` is empty; bf16 at N = 65,
    d = 192, hd = 32: the 32x32-tile kernel); bf16 at hd = 64, N = 197: projection + core in one kernel, `qkv` its side output;
    other geometries: qkv Linear (panel GEMM) + the per-(image, head) attention core.  cos / sin: caller-supplied rotary tables ([P, hd/2] or [H, P, hd/2]) used instead of the module's own.
    tables_grad: the caller's tables require grad -- the qkv Linear + core route at every geometry (the fused kernels
    return no table gradients), so that the backward has `qkv` and runs the core backward with table gradients."""
    return _attention_forward("vitpe::attention", True, xn, wqkv, None, wproj, bproj, resid, num_heads, mode, grid, pe_param,
                              inv_freq, degree, per_head, cos, sin, tables_grad, 0.0, 0.0, None)


@attention.register_fake
def attention_fake(xn, wqkv, wproj, bproj, resid, num_heads, mode, grid, pe_param, inv_freq, degree, per_head, cos=None,
                   sin=None, tables_grad=False):
    """The branch of _attention_forward on the concrete shape (the route is a function of dtype, N, D and the head
    dimension, so a trace specialises on them): `qkv` is empty where the kernel that keeps it on the chip runs (_fused_ok
    and no table gradients), [B, N, 3D] on the hd-64 one-kernel route and on the qkv Linear + core route.  The backward
    dispatches on qkv.numel() == 0."""
    B, N, D = (int(s) for s in xn.shape)
    on_chip = not tables_grad and bool(L.lib().vitpe_fused_attention_supported(L.dtype_code(xn.dtype), N, D, D // num_heads))
    return xn.new_empty((B, N, D)), xn.new_empty((B, N, D)), xn.new_empty(0) if on_chip else xn.new_empty((B, N, 3 * D))


def _attn_setup(ctx, inputs, output):
    xn, wqkv, wproj, bproj, resid, num_heads, mode, grid, pe_param, inv_freq, degree, per_head, cos, sin, tables_grad = inputs
    _attention_setup(ctx, output, True, xn, wqkv, None, wproj, resid, num_heads, mode, grid, pe_param, inv_freq, degree,
                     per_head, cos, sin, tables_grad, 0.0, 0.0, None)


def _attn_backward(ctx, dy, _da, _dqkv):
    dxn, dwqkv, _, dwproj, dbproj, dresid, dpe, dcos, dsin = _attention_backward(ctx, dy)
    return (dxn, dwqkv, dwproj, dbproj, dresid, None, None, None, dpe, None, None, None, dcos, dsin, None)


attention.register_autograd(_attn_backward, setup_context=_attn_setup)


# ---- attention with a qkv bias and / or dropout (reference vit.py:28-38: qkv_bias, attn_drop, proj_drop) -------------------
@torch.library.custom_op("vitpe::attention_drop", mutates_args=())
def attention_drop(xn: Tensor, wqkv: Tensor, bqkv: Optional[Tensor], wproj: Tensor, bproj: Tensor, resid: Optional[Tensor],
                   num_heads: int, mode: int, grid: int, pe_param: Optional[Tensor], inv_freq: Optional[Tensor], degree: int,
                   per_head: bool, cos: Optional[Tensor], sin: Optional[Tensor], tables_grad: bool, attn_p: float,
                   proj_p: float, rng: Optional[Tensor]) -> Tuple[Tensor, Tensor, Tensor]:
    """-> (y, a, qkv): vitpe::attention on the qkv Linear (bias epilogue, the real bias) + attention core route at every
    geometry -- the one-kernel fused paths have no bias input and no dropout.  attn_p > 0: the dropout core (softmax ->
    dropout -> @ v inside the kernel); proj_p > 0: the elementwise dropout kernel behind the proj Linear, residual fused.
    rng: [2, 2] int64 device tensor, the (seed, offset) pairs of the attention-probability site (row 0) and the proj site
    (row 1); the backward regenerates both masks from it.  tables_grad together with attn_p > 0 is refused."""
    return _attention_forward("vitpe::attention_drop", False, xn, wqkv, bqkv, wproj, bproj, resid, num_heads, mode, grid,
                              pe_param, inv_freq, degree, per_head, cos, sin, tables_grad, attn_p, proj_p, rng)


@attention_drop.register_fake
def attention_drop_fake(xn, wqkv, bqkv, wproj, bproj, resid, num_heads, mode, grid, pe_param, inv_freq, degree, per_head, cos,
                        sin, tables_grad, attn_p, proj_p, rng):
    B, N, D = xn.shape
    return xn.new_empty((B, N, D)), xn.new_empty((B, N, D)), xn.new_empty((B, N, 3 * D))


def _attn_drop_setup(ctx, inputs, output):
    (xn, wqkv, bqkv, wproj, bproj, resid, num_heads, mode, grid, pe_param, inv_freq, degree, per_head, cos, sin, tables_grad,
     attn_p, proj_p, rng) = inputs
    _attention_setup(ctx, output, False, xn, wqkv, bqkv, wproj, resid, num_heads, mode, grid, pe_param, inv_freq, degree,
                     per_head, cos, sin, tables_grad, attn_p, proj_p, rng)


def _attn_drop_backward(ctx, dy, _da, _dqkv):
    dxn, dwqkv, dbqkv, dwproj, dbproj, dresid, dpe, dcos, dsin = _attention_backward(ctx, dy)
    return (dxn, dwqkv, dbqkv, dwproj, dbproj, dresid, None, None, None, dpe, None, None, None, dcos, dsin,
            None, None, None, None)


attention_drop.register_autograd(_attn_drop_backward, setup_context=_attn_drop_setup)


# ---- attention probabilities (reference vit.py:71-84: `attn` after softmax, before attn_drop) -------------------------------
@torch.library.custom_op("vitpe::attention_probs", mutates_args=())
def attention_probs(qkv: Tensor, num_heads: int, mode: int, grid: int, pe_param: Optional[Tensor], inv_freq: Optional[Tensor],
                    degree: int, per_head: bool, cos: Optional[Tensor] = None, sin: Optional[Tensor] = None,
                    cls_only: bool = False) -> Tensor:
    """qkv [B,N,3D] (the qkv Linear's output) -> softmax(QK^T hd^-0.5 [+ bias]) fp32 [B,H,N,N]; cls_only: the class token's
    row, [B,H,N].  PE arguments as vitpe::attention.  For analysis: no autograd is registered, the result is a constant."""
    t = _pe_tables(mode, grid, pe_param, inv_freq, degree, per_head, cos, sin)
    return K.attention_core_probs(qkv.contiguous(), num_heads, t, cls_only=cls_only)


@attention_probs.register_fake
def attention_probs_fake(qkv, num_heads, mode, grid, pe_param, inv_freq, degree, per_head, cos=None, sin=None, cls_only=False):
    B, N, _ = qkv.shape
    shape = (B, num_heads, N) if cls_only else (B, num_heads, N, N)
    return qkv.new_empty(shape, dtype=torch.float32)


# ---- mlp: y = [resid +] fc2(gelu(fc1(xn)))  (timm Mlp, reference vit.py:118,124) ----------------
@torch.library.custom_op("vitpe::mlp", mutates_args=())
def mlp(xn: Tensor, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor, resid: Optional[Tensor], p: float = 0.0,
        rng: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """p > 0 (timm Mlp's drop, drop1 behind the activation and drop2 behind fc2): fc1 + GELU -> dropout -> fc2 + bias ->
    dropout [+ resid]; rng [2, 2] int64: the pairs of drop1 (row 0) and drop2 (row 1).  The returned h is then the
    dropped activation (what fc2 read)."""
    dt = xn.dtype
    shp = xn.shape
    D = shp[-1]
    x2 = xn.contiguous().view(-1, D)
    h, u = K.linear(x2, _shadow(w1, dt), b1, epi=L.EPI_BIAS_GELU)
    if p > 0.0:
        if rng is None or tuple(rng.shape) != (2, 2):
            raise L.VitpeError("vitpe::mlp: dropout needs rng, a [2, 2] int64 device tensor")
        h = K.dropout_fwd(h, rng[0], p)
        y = K.linear(h, _shadow(w2, dt), b2, epi=L.EPI_BIAS)
        y = K.dropout_fwd(y, rng[1], p, resid=None if resid is None else resid.contiguous().view(-1, D))
        return y.view(shp), h, u
    if resid is None:
        y = K.linear(h, _shadow(w2, dt), b2, epi=L.EPI_BIAS)
    else:
        y = K.linear(h, _shadow(w2, dt), b2, epi=L.EPI_BIAS_RESID, resid=resid.contiguous().view(-1, D))
    return y.view(shp), h, u


@mlp.register_fake
def mlp_fake(xn, w1, b1, w2, b2, resid, p=0.0, rng=None):
    m = xn.numel() // xn.shape[-1]
    return xn.new_empty(xn.shape), xn.new_empty(m, w1.shape[0]), xn.new_empty(m, w1.shape[0])


def _mlp_setup(ctx, inputs, output):
    xn, w1, b1, w2, b2, resid, p, rng = inputs
    _, h, u = output
    ctx.save_for_backward(xn, w1, w2, h, u, rng)
    ctx.has_resid = resid is not None
    ctx.p = p


@torch.library.custom_op("vitpe::mlp_backward", mutates_args=())
def mlp_backward(dy: Tensor, xn: Tensor, w1: Tensor, w2: Tensor, h: Tensor, u: Tensor, rng: Optional[Tensor], p: float
                 ) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """-> (dxn, dw1, db1, dw2, db2)"""
    dt = xn.dtype
    D = xn.shape[-1]
    dy2 = dy.contiguous().view(-1, D)
    x2 = xn.contiguous().view(-1, D)
    if p > 0.0:
        dy2 = K.dropout_bwd(dy2, rng[1], p)
    du = K.linear(dy2, _shadow_t(w2, dt), None, epi=L.EPI_GELU_BWD, u=u)
    if p > 0.0:   # (dy W2) . m1 / (1-p) . gelu'(u): the two elementwise factors commute
        du = K.dropout_bwd(du, rng[0], p)
    dw2, db2 = _zeros(w2), torch.zeros(w2.shape[0], dtype=torch.float32, device=dy.device)
    K.gemm_tn(dy2, h, dw2, db2)
    dxn = K.linear(du, _shadow_t(w1, dt), None, epi=L.EPI_BIAS).view(xn.shape)
    dw1, db1 = _zeros(w1), torch.zeros(w1.shape[0], dtype=torch.float32, device=dy.device)
    K.gemm_tn(du, x2, dw1, db1)
    return dxn, dw1, db1, dw2, db2


@mlp_backward.register_fake
def mlp_backward_fake(dy, xn, w1, w2, h, u, rng, p):
    f32 = dict(dtype=torch.float32)
    return (xn.new_empty(xn.shape), w1.new_empty(w1.shape), xn.new_empty(w1.shape[0], **f32), w2.new_empty(w2.shape),
            xn.new_empty(w2.shape[0], **f32))


def _mlp_backward(ctx, dy, _dh, _du):
    xn, w1, w2, h, u, rng = ctx.saved_tensors
    dxn, dw1, db1, dw2, db2 = torch.ops.vitpe.mlp_backward(dy, xn, w1, w2, h, u, rng, ctx.p)
    return dxn, dw1, db1, dw2, db2, dy if ctx.has_resid else None, None, None


mlp.register_autograd(_mlp_backward, setup_context=_mlp_setup)


# ---- dropout / drop_path: y = [resid +] x . mask / (1 - p) ------------------------------------------
# (torch.nn.Dropout and timm's DropPath(scale_by_keep=True) -- the latter third-party, parity unpinned -- on the
#  project's own Philox stream; rng: int64 [2] device tensor (seed, offset), saved for the backward, which regenerates the
#  mask)
@torch.library.custom_op("vitpe::dropout", mutates_args=())
def dropout(x: Tensor, resid: Optional[Tensor], p: float, rng: Tensor) -> Tensor:
    return K.dropout_fwd(x.contiguous(), rng, p, resid=None if resid is None else resid.contiguous())


@dropout.register_fake
def dropout_fake(x, resid, p, rng):
    return x.new_empty(x.shape)


def _drop_setup(ctx, inputs, output):
    x, resid, p, rng = inputs
    ctx.save_for_backward(rng)
    ctx.p, ctx.has_resid = p, resid is not None


@torch.library.custom_op("vitpe::dropout_backward", mutates_args=())
def dropout_backward(dy: Tensor, rng: Tensor, p: float) -> Tensor:
    return K.dropout_bwd(dy.contiguous(), rng, p)


@dropout_backward.register_fake
def dropout_backward_fake(dy, rng, p):
    return dy.new_empty(dy.shape)


def _dropout_backward(ctx, dy):
    (rng,) = ctx.saved_tensors
    return torch.ops.vitpe.dropout_backward(dy, rng, ctx.p), (dy if ctx.has_resid else None), None, None


dropout.register_autograd(_dropout_backward, setup_context=_drop_setup)


@torch.library.custom_op("vitpe::drop_path", mutates_args=())
def drop_path(x: Tensor, resid: Optional[Tensor], p: float, rng: Tensor) -> Tensor:
    return K.drop_path_fwd(x.contiguous(), rng, p, resid=None if resid is None else resid.contiguous())


@drop_path.register_fake
def drop_path_fake(x, resid, p, rng):
    return x.new_empty(x.shape)


@torch.library.custom_op("vitpe::drop_path_backward", mutates_args=())
def drop_path_backward(dy: Tensor, rng: Tensor, p: float) -> Tensor:
    return K.drop_path_bwd(dy.contiguous(), rng, p)


@drop_path_backward.register_fake
def drop_path_backward_fake(dy, rng, p):
    return dy.new_empty(dy.shape)


def _drop_path_backward(ctx, dy):
    (rng,) = ctx.saved_tensors
    return torch.ops.vitpe.drop_path_backward(dy, rng, ctx.p), (dy if ctx.has_resid else None), None, None


drop_path.register_autograd(_drop_path_backward, setup_context=_drop_setup)


# ---- patch_embed: images -> tokens (unfold + GEMM + cls + APE), reference vit.py:245-258 ---------
@torch.library.custom_op("vitpe::patch_embed", mutates_args=())
def patch_embed(images: Tensor, weight: Tensor, bias: Tensor, cls_token: Tensor, ape: Optional[Tensor],
                patch: int, bf16: bool) -> Tuple[Tensor, Tensor]:
    dt = torch.bfloat16 if bf16 else torch.float32
    B, C, S, _ = images.shape
    g = S // patch
    P = g * g
    D = weight.shape[0]
    patches = K.unfold(images.contiguous().float(), patch, dt)
    w = _shadow(weight.reshape(D, -1), dt)
    ape_rows = ape[0, :P].contiguous() if ape is not None else None
    tok = K.patch_embed_gemm(patches, w, bias, cls_token.reshape(-1).contiguous(), ape_rows, B, P)
    return tok, patches


@patch_embed.register_fake
def patch_embed_fake(images, weight, bias, cls_token, ape, patch, bf16):
    dt = torch.bfloat16 if bf16 else torch.float32
    B, C, S, _ = images.shape
    P = (S // patch) ** 2
    return (images.new_empty((B, P + 1, weight.shape[0]), dtype=dt),
            images.new_empty((B * P, C * patch * patch), dtype=dt))


def _pe_setup(ctx, inputs, output):
    images, weight, bias, cls_token, ape, patch, bf16 = inputs
    _, patches = output
    ctx.save_for_backward(patches)
    ctx.shapes = (weight.shape, cls_token.shape, None if ape is None else ape.shape)


@torch.library.custom_op("vitpe::patch_embed_backward", mutates_args=())
def patch_embed_backward(dtok: Tensor, patches: Tensor, ape_len: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """-> (dweight [D, C p p], dbias [D], dcls [D], dape [1, ape_len, D]); ape_len 0: no APE table, dape is empty"""
    dev = dtok.device
    B, Ntok, D = dtok.shape
    dcls = torch.zeros(D, dtype=torch.float32, device=dev)
    dape = torch.zeros((1, ape_len, D), dtype=torch.float32, device=dev) if ape_len > 0 else None
    dape_rows = dape[0, :Ntok - 1] if dape is not None else None  # contiguous leading rows of [1,max_len,D]
    dpatch = K.embed_bwd(dtok.contiguous(), dcls, dape_rows)
    dw = torch.zeros((D, patches.shape[1]), dtype=torch.float32, device=dev)
    db = torch.zeros(D, dtype=torch.float32, device=dev)
    K.gemm_tn(dpatch, patches, dw, db)
    return dw, db, dcls, dape if dape is not None else dcls.new_empty(0)


@patch_embed_backward.register_fake
def patch_embed_backward_fake(dtok, patches, ape_len):
    D = dtok.shape[-1]
    f32 = dict(dtype=torch.float32)
    return (dtok.new_empty((D, patches.shape[1]), **f32), dtok.new_empty(D, **f32), dtok.new_empty(D, **f32),
            dtok.new_empty((1, ape_len, D), **f32) if ape_len > 0 else dtok.new_empty(0, **f32))


def _pe_backward(ctx, dtok, _dp):
    (patches,) = ctx.saved_tensors
    wshape, cshape, ashape = ctx.shapes
    dw, db, dcls, dape = torch.ops.vitpe.patch_embed_backward(dtok, patches, 0 if ashape is None else ashape[1])
    return None, dw.view(wshape), db, dcls.view(cshape), None if ashape is None else dape.view(ashape), None, None


patch_embed.register_autograd(_pe_backward, setup_context=_pe_setup)


# ---- head: logits = Linear(LayerNorm(x)[:, 0]), reference vit.py:284-285 ------------------------
@torch.library.custom_op("vitpe::head", mutates_args=())
def head(x: Tensor, gamma: Tensor, beta: Tensor, wh: Tensor, bh: Tensor, eps: float) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    logits, ws = K.head_fwd(x.contiguous(), gamma, beta, wh.contiguous(), bh, eps, save=True)
    return logits, ws[0], ws[1], ws[2]


@head.register_fake
def head_fake(x, gamma, beta, wh, bh, eps):
    B, _, D = x.shape
    f = dict(dtype=torch.float32)
    return x.new_empty((B, wh.shape[0]), **f), x.new_empty((B, D), **f), x.new_empty((B, D), **f), x.new_empty((B,), **f)


def _head_setup(ctx, inputs, output):
    x, gamma, beta, wh, bh, eps = inputs
    _, xhat, yn, rstd = output
    ctx.save_for_backward(gamma, wh, xhat, yn, rstd)
    ctx.xmeta = (x.dtype, x.shape[1])


@torch.library.custom_op("vitpe::head_backward", mutates_args=())
def head_backward(dlogits: Tensor, gamma: Tensor, wh: Tensor, xhat: Tensor, yn: Tensor, rstd: Tensor, bf16: bool, ntok: int
                  ) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """-> (dx [B, ntok, D] in the type of x, dgamma, dbeta, dwh, dbh)"""
    dtype = torch.bfloat16 if bf16 else torch.float32
    dwh, dbh = _zeros(wh), torch.zeros(wh.shape[0], dtype=torch.float32, device=wh.device)
    dg, db = _zeros(gamma), _zeros(gamma)
    dx = K.head_bwd(dlogits.contiguous().float(), wh.contiguous(), gamma, (xhat, yn, rstd), dtype, ntok, dwh, dbh, dg, db)
    return dx, dg, db, dwh, dbh


@head_backward.register_fake
def head_backward_fake(dlogits, gamma, wh, xhat, yn, rstd, bf16, ntok):
    B, D = xhat.shape
    return (xhat.new_empty((B, ntok, D), dtype=torch.bfloat16 if bf16 else torch.float32), gamma.new_empty(gamma.shape),
            gamma.new_empty(gamma.shape), wh.new_empty(wh.shape), wh.new_empty(wh.shape[0], dtype=torch.float32))


def _head_backward(ctx, dlogits, *_):
    gamma, wh, xhat, yn, rstd = ctx.saved_tensors
    dtype, ntok = ctx.xmeta
    dx, dg, db, dwh, dbh = torch.ops.vitpe.head_backward(dlogits, gamma, wh, xhat, yn, rstd, dtype == torch.bfloat16, ntok)
    return dx, dg, db, dwh, dbh, None


head.register_autograd(_head_backward, setup_context=_head_setup)


# ---- cross entropy (mean), reference train.py:113,194 --------------------------------------------
@torch.library.custom_op("vitpe::cross_entropy", mutates_args=())
def cross_entropy(logits: Tensor, labels: Tensor) -> Tuple[Tensor, Tensor]:
    out2, dlog = K.cross_entropy(logits.contiguous().float(), labels.contiguous())
    return out2[0].clone(), dlog


@cross_entropy.register_fake
def cross_entropy_fake(logits, labels):
    return logits.new_empty((), dtype=torch.float32), logits.new_empty(logits.shape, dtype=torch.float32)


def _ce_setup(ctx, inputs, output):
    ctx.save_for_backward(output[1])


def _ce_backward(ctx, dloss, _):
    (dlog,) = ctx.saved_tensors
    return dlog * dloss, None


cross_entropy.register_autograd(_ce_backward, setup_context=_ce_setup)
