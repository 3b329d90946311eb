"""Tensor-level wrappers over the C ABI (include/vitpe.h).

Each function validates device / dtype / shape, allocates outputs with torch (PyTorch owns all
device memory), and enqueues the HIP kernel on torch's current stream.  No arithmetic happens
in Python; there is no fallback path.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional, Tuple

import torch

from . import _lib as L
from ._lib import check, dtype_code, lib, ptr, require_device, stream_ptr

SPLITS_TARGET_WGS = 512  # workgroups a weight-gradient launch should expose


def _f32(t, name):
    if t is not None and t.dtype != torch.float32:
        raise L.VitpeError(f"{name} must be float32")


# ---- GEMMs --------------------------------------------------------------------------------
def gemm_nt(a, w, bias=None, epi=L.EPI_BIAS, resid=None, u=None, out=None):
    """epi(A[M,K] W[N,K]^T) -> C[M,N]; EPI_BIAS_GELU returns (C, U)."""
    require_device(a, w, bias, resid, u, out)
    M, K = a.shape
    N = w.shape[0]
    assert w.shape[1] == K and a.dtype == w.dtype
    _f32(bias, "bias")
    c = out if out is not None else torch.empty((M, N), dtype=a.dtype, device=a.device)
    if epi == L.EPI_BIAS_GELU and u is None:
        u = torch.empty((M, N), dtype=a.dtype, device=a.device)
    check(lib().vitpe_gemm_nt(dtype_code(a.dtype), epi, ptr(a), ptr(w), ptr(c), ptr(bias), ptr(resid), ptr(u),
                              None, None, M, N, K, 0, 0, stream_ptr()), "vitpe_gemm_nt")
    return (c, u) if epi == L.EPI_BIAS_GELU else c


def linear(a, w, bias=None, epi=L.EPI_BIAS, resid=None, u=None, out=None, stats=None, eps=1e-5):
    """Second-generation linear (vitpe_linear): epi(A[M,K] W[N,K]^T); `stats=(mean, rstd)` (N == 192)
    additionally receives the LayerNorm statistics of the output rows.  EPI_BIAS_GELU returns (C, U)."""
    require_device(a, w, bias, resid, u, out)
    M, K = a.shape
    N = w.shape[0]
    assert w.shape[1] == K and a.dtype == w.dtype
    _f32(bias, "bias")
    c = out if out is not None else torch.empty((M, N), dtype=a.dtype, device=a.device)
    if epi == L.EPI_BIAS_GELU and u is None:
        u = torch.empty((M, N), dtype=a.dtype, device=a.device)
    mean, rstd = stats if stats is not None else (None, None)
    require_device(mean, rstd)
    check(lib().vitpe_linear(dtype_code(a.dtype), epi, ptr(a), ptr(w), ptr(c), ptr(bias), ptr(resid), ptr(u),
                             ptr(mean), ptr(rstd), eps, M, N, K, stream_ptr()), "vitpe_linear")
    return (c, u) if epi == L.EPI_BIAS_GELU else c


def linear_ln(x, gamma, beta, mean, rstd, w, bias=None, epi=L.EPI_BIAS, u=None, out=None, xn_out=None):
    """epi(LayerNorm(x) W^T) with the LayerNorm applied while staging x (row statistics given)."""
    require_device(x, gamma, beta, mean, rstd, w, bias, u, out, xn_out)
    M, K = x.shape
    N = w.shape[0]
    c = out if out is not None else torch.empty((M, N), dtype=x.dtype, device=x.device)
    if epi == L.EPI_BIAS_GELU and u is None:
        u = torch.empty((M, N), dtype=x.dtype, device=x.device)
    check(lib().vitpe_linear_ln(dtype_code(x.dtype), epi, ptr(x), ptr(gamma), ptr(beta), ptr(mean), ptr(rstd),
                                ptr(xn_out), ptr(w), ptr(c), ptr(bias), ptr(u), M, N, K, stream_ptr()), "vitpe_linear_ln")
    return (c, u) if epi == L.EPI_BIAS_GELU else c


def linear_lnbwd(dy, wt, x, mean, rstd, gamma, dres, dgamma, dbeta, out=None):
    """dx = dres + LayerNorm'(dy wt^T) (LayerNorm input rows x); dgamma/dbeta accumulated."""
    require_device(dy, wt, x, mean, rstd, gamma, dres, dgamma, dbeta, out)
    M, K = dy.shape
    assert wt.shape == (192, K) and x.shape[-1] == 192
    dx = out if out is not None else torch.empty((M, 192), dtype=dy.dtype, device=dy.device)
    check(lib().vitpe_linear_lnbwd(dtype_code(dy.dtype), ptr(dy), ptr(wt), ptr(dx), ptr(x), ptr(mean), ptr(rstd),
                                   ptr(gamma), ptr(dres), ptr(dgamma), ptr(dbeta), M, K, stream_ptr()),
          "vitpe_linear_lnbwd")
    return dx


def linear_lnbwd2(dy, wt_pk, x, mean, rstd, gamma, dres, dgamma, dbeta, out=None):
    """linear_lnbwd on the wave-per-tile mapping; wt_pk = pack_weight_frags(weight^T [192,K], dtype, 64, 0)."""
    require_device(dy, wt_pk, x, mean, rstd, gamma, dres, dgamma, dbeta, out)
    M, K = dy.shape
    assert wt_pk.numel() == 192 * K and x.shape[-1] == 192 and dy.dtype == wt_pk.dtype == x.dtype == dres.dtype
    _f32(gamma, "gamma"), _f32(dgamma, "dgamma"), _f32(dbeta, "dbeta"), _f32(mean, "mean"), _f32(rstd, "rstd")
    dx = out if out is not None else torch.empty((M, 192), dtype=dy.dtype, device=dy.device)
    check(lib().vitpe_linear_lnbwd2(dtype_code(dy.dtype), ptr(dy), ptr(wt_pk), ptr(dx), ptr(x), ptr(mean), ptr(rstd),
                                    ptr(gamma), ptr(dres), ptr(dgamma), ptr(dbeta), M, K, stream_ptr()),
          "vitpe_linear_lnbwd2")
    return dx


def patch_embed_gemm(patches, w, bias, cls, ape, B, P, out=None):
    """tokens[B,P+1,N] from unfolded patches [B*P,K] (vit.py:248-258)."""
    require_device(patches, w, bias, cls, ape, out)
    M, K = patches.shape
    N = w.shape[0]
    assert M == B * P
    _f32(bias, "bias"), _f32(cls, "cls"), _f32(ape, "ape")
    c = out if out is not None else torch.empty((B, P + 1, N), dtype=patches.dtype, device=patches.device)
    check(lib().vitpe_gemm_nt(dtype_code(patches.dtype), L.EPI_PATCH, ptr(patches), ptr(w), ptr(c), ptr(bias), None,
                              None, ptr(ape), ptr(cls), M, N, K, P, P + 1, stream_ptr()), "vitpe_gemm_nt(patch)")
    return c


def wgrad_splits(M, N, K):
    """token slices for a single vitpe_gemm_tn launch: enough (n, k) tiles x slices to cover the CUs"""
    tiles = ((N + 127) // 128) * ((K + 127) // 128 if (K % 128 == 0 or K > 192) else (K + 63) // 64)
    return max(1, min(64, SPLITS_TARGET_WGS // max(tiles, 1), (M + 255) // 256))


def gemm_tn(dy, x, dw, dbias=None, splits=None):
    """dW[N,K] += dY[M,N]^T X[M,K]; dbias[N] += colsum(dY)."""
    require_device(dy, x, dw, dbias)
    M, N = dy.shape
    K = x.shape[1]
    assert x.shape[0] == M and dw.numel() == N * K and dy.dtype == x.dtype
    _f32(dw, "dw"), _f32(dbias, "dbias")
    if splits is None:
        splits = wgrad_splits(M, N, K)
    check(lib().vitpe_gemm_tn(dtype_code(dy.dtype), ptr(dy), ptr(x), ptr(dw), ptr(dbias), M, N, K, splits,
                              stream_ptr()), "vitpe_gemm_tn")


def pack_weight_frags(w, dtype, kchunk, phi, out=None):
    """Fragment-major packed copy of the fp32 weight w [R, C] (include/vitpe.h: vitpe_pack_weight_frags)."""
    require_device(w, out)
    _f32(w, "w")
    R, C = w.shape
    out = out if out is not None else torch.empty((R, C), dtype=dtype, device=w.device)
    assert out.dtype == dtype and out.numel() == R * C
    check(lib().vitpe_pack_weight_frags(dtype_code(dtype), ptr(w), ptr(out), R, C, int(kchunk), int(bool(phi)), stream_ptr()),
          "vitpe_pack_weight_frags")
    return out


def block_tail2_supported(dtype, D, HID) -> bool:
    return bool(lib().vitpe_block_tail2_supported(dtype_code(dtype), int(D), int(HID)))


def block_tail2_fwd(attn_out, x_in, wp_pk, bp, gamma, beta, w1_pk, b1, w2_pk, b2, x_mid=None, mean2=None, rstd2=None,
                    xn_out=None, gp=None, h=None, out=None, stats=None, eps2=1e-5, eps_next=1e-5, save=True):
    """The block tail -- x_mid = x_in + attn_out Wp^T + bp; out = x_mid + fc2(gelu(fc1(LN2(x_mid)))) -- in one kernel on
    packed weights (pack_weight_frags: wp kchunk 192 natural, w1 kchunk 192 phi, w2 kchunk 32
    phi).  What it keeps of the hidden layer for backward is gp = gelu'(u) and h = gelu(u) (save=True), or nothing.
    Returns (out, x_mid, mean2, rstd2, gp, h)."""
    require_device(attn_out, x_in, wp_pk, bp, gamma, beta, w1_pk, b1, w2_pk, b2, x_mid, mean2, rstd2, xn_out, gp, h, out)
    M, D = attn_out.shape
    HID = b1.numel()
    assert x_in.shape == (M, D) and wp_pk.numel() == D * D and w1_pk.numel() == HID * D and w2_pk.numel() == D * HID
    assert attn_out.dtype == x_in.dtype == wp_pk.dtype == w1_pk.dtype == w2_pk.dtype
    for t_, n_ in ((bp, "bp"), (gamma, "gamma"), (beta, "beta"), (b1, "b1"), (b2, "b2")):
        _f32(t_, n_)
    dt, dev = attn_out.dtype, attn_out.device
    x_mid = x_mid if x_mid is not None else torch.empty((M, D), dtype=dt, device=dev)
    mean2 = mean2 if mean2 is not None else torch.empty(M, dtype=torch.float32, device=dev)
    rstd2 = rstd2 if rstd2 is not None else torch.empty(M, dtype=torch.float32, device=dev)
    if save:
        gp = gp if gp is not None else torch.empty((M, HID), dtype=torch.float16, device=dev)   # gelu'(u) is kept as IEEE half
        h = h if h is not None else torch.empty((M, HID), dtype=dt, device=dev)
        assert gp.shape == h.shape == (M, HID) and h.dtype == dt and gp.dtype == torch.float16
    else:
        gp = h = None
    out = out if out is not None else torch.empty((M, D), dtype=dt, device=dev)
    mo, ro = stats if stats is not None else (None, None)
    require_device(mo, ro)
    check(lib().vitpe_block_tail2_fwd(dtype_code(dt), ptr(attn_out), ptr(x_in), ptr(wp_pk), ptr(bp), ptr(gamma), ptr(beta),
                                      ptr(x_mid), ptr(mean2), ptr(rstd2), ptr(xn_out), ptr(w1_pk), ptr(b1), ptr(w2_pk),
                                      ptr(b2), ptr(gp), ptr(h), ptr(out), ptr(mo), ptr(ro), float(eps2), float(eps_next),
                                      M, D, HID, stream_ptr()), "vitpe_block_tail2_fwd")
    return out, x_mid, mean2, rstd2, gp, h


def block_tail2_bwd(dy, gp, w2t_pk, w1t_pk, x_mid, mean2, rstd2, gamma, dgamma, dbeta, wpt_pk, du=None, out=None, da=None):
    """Backward of block_tail2_fwd w.r.t. its inputs on packed TRANSPOSED weights (pack_weight_frags of fc2.weight^T
    (192, phi), fc1.weight^T (32, phi), proj.weight^T (192, phi)) -> (dx_mid, du, da); dgamma / dbeta accumulated."""
    require_device(dy, gp, w2t_pk, w1t_pk, x_mid, mean2, rstd2, gamma, dgamma, dbeta, wpt_pk, du, out, da)
    M, D = dy.shape
    HID = gp.shape[1]
    assert gp.shape == (M, HID) and x_mid.shape == (M, D) and w2t_pk.numel() == HID * D and w1t_pk.numel() == HID * D
    assert wpt_pk.numel() == D * D and dy.dtype == w2t_pk.dtype == w1t_pk.dtype == x_mid.dtype == wpt_pk.dtype
    assert gp.dtype == torch.float16   # (block_tail2_fwd keeps gelu'(u) as IEEE half)
    _f32(gamma, "gamma"), _f32(dgamma, "dgamma"), _f32(dbeta, "dbeta"), _f32(mean2, "mean2"), _f32(rstd2, "rstd2")
    du = du if du is not None else torch.empty(gp.shape, dtype=dy.dtype, device=dy.device)
    out = out if out is not None else torch.empty_like(dy)
    da = da if da is not None else torch.empty_like(dy)
    check(lib().vitpe_block_tail2_bwd(dtype_code(dy.dtype), ptr(dy), ptr(gp), ptr(w2t_pk), ptr(w1t_pk), ptr(x_mid), ptr(mean2),
                                      ptr(rstd2), ptr(gamma), ptr(du), ptr(out), ptr(dgamma), ptr(dbeta), ptr(wpt_pk), ptr(da),
                                      M, D, HID, stream_ptr()), "vitpe_block_tail2_bwd")
    return out, du, da


def block_tail2_bwd_pre(dqkv, wqt_pk, x1, mean1, rstd1, gamma1, dres1, dgamma1, dbeta1, dy_out, gp, w2t_pk, w1t_pk, x_mid,
                        mean2, rstd2, gamma, dgamma, dbeta, wpt_pk, du=None, out=None, da=None):
    """block_tail2_bwd preceded in the same kernel by the upper block's linear_lnbwd2: dy_out = dres1 + LN1'(dqkv Wqkv) is
    written and feeds the MLP backward from registers (wqt_pk = pack_weight_frags(qkv.weight^T, 64, 0))."""
    require_device(dqkv, wqt_pk, x1, mean1, rstd1, gamma1, dres1, dgamma1, dbeta1, dy_out, gp, w2t_pk, w1t_pk, x_mid, mean2,
                   rstd2, gamma, dgamma, dbeta, wpt_pk, du, out, da)
    M, K1 = dqkv.shape
    D, HID = dy_out.shape[1], gp.shape[1]
    assert dy_out.shape == (M, D) and gp.shape == (M, HID) and x_mid.shape == (M, D) and wqt_pk.numel() == D * K1
    assert dqkv.dtype == wqt_pk.dtype == dy_out.dtype == w2t_pk.dtype == w1t_pk.dtype == x_mid.dtype == wpt_pk.dtype
    assert gp.dtype == torch.float16
    for t_, n_ in ((gamma, "gamma"), (dgamma, "dgamma"), (dbeta, "dbeta"), (gamma1, "gamma1"), (dgamma1, "dgamma1"),
                   (dbeta1, "dbeta1"), (mean1, "mean1"), (rstd1, "rstd1"), (mean2, "mean2"), (rstd2, "rstd2")):
        _f32(t_, n_)
    du = du if du is not None else torch.empty(gp.shape, dtype=dy_out.dtype, device=dy_out.device)
    out = out if out is not None else torch.empty_like(dy_out)
    da = da if da is not None else torch.empty_like(dy_out)
    check(lib().vitpe_block_tail2_bwd_pre(dtype_code(dqkv.dtype), ptr(dqkv), ptr(wqt_pk), ptr(x1), ptr(mean1), ptr(rstd1),
                                          ptr(gamma1), ptr(dres1), ptr(dgamma1), ptr(dbeta1), K1, ptr(dy_out), ptr(gp),
                                          ptr(w2t_pk), ptr(w1t_pk), ptr(x_mid), ptr(mean2), ptr(rstd2), ptr(gamma), ptr(du),
                                          ptr(out), ptr(dgamma), ptr(dbeta), ptr(wpt_pk), ptr(da), M, D, HID, stream_ptr()),
          "vitpe_block_tail2_bwd_pre")
    return out, du, da


def tail_cls_fwd(attn_out, x_in, wp_pk, bp, gamma, beta, w1_pk, b1, w2_pk, b2, B, row_step, x_mid, mean2, rstd2, out,
                 xn_out=None, gp=None, h=None, eps2=1e-5):
    """block_tail2_fwd on the B rows r * row_step of the full-layout buffers (include/vitpe.h: vitpe_tail_cls_fwd), in place:
    every other row of x_mid / mean2 / rstd2 / xn_out / gp / h / out keeps what it held.  gp and h: both (training) or
    neither (evaluation)."""
    require_device(attn_out, x_in, wp_pk, bp, gamma, beta, w1_pk, b1, w2_pk, b2, x_mid, mean2, rstd2, xn_out, gp, h, out)
    M, D = attn_out.shape
    HID = b1.numel()
    assert row_step >= 1 and (B == 0 or (B - 1) * row_step < M)
    assert x_in.shape == x_mid.shape == out.shape == (M, D) and mean2.numel() == M and rstd2.numel() == M
    assert wp_pk.numel() == D * D and w1_pk.numel() == HID * D and w2_pk.numel() == D * HID
    assert attn_out.dtype == x_in.dtype == wp_pk.dtype == w1_pk.dtype == w2_pk.dtype == x_mid.dtype == out.dtype
    assert xn_out is None or (xn_out.shape == (M, D) and xn_out.dtype == attn_out.dtype)
    assert (gp is None) == (h is None)
    if gp is not None:
        assert gp.shape == h.shape == (M, HID) and h.dtype == attn_out.dtype and gp.dtype == torch.float16
    for t_, n_ in ((bp, "bp"), (gamma, "gamma"), (beta, "beta"), (b1, "b1"), (b2, "b2"), (mean2, "mean2"), (rstd2, "rstd2")):
        _f32(t_, n_)
    check(lib().vitpe_tail_cls_fwd(dtype_code(attn_out.dtype), ptr(attn_out), ptr(x_in), ptr(wp_pk), ptr(bp), ptr(gamma),
                                   ptr(beta), ptr(x_mid), ptr(mean2), ptr(rstd2), ptr(xn_out), ptr(w1_pk), ptr(b1),
                                   ptr(w2_pk), ptr(b2), ptr(gp), ptr(h), ptr(out), float(eps2), int(B), int(row_step), D, HID,
                                   stream_ptr()), "vitpe_tail_cls_fwd")


def tail_cls_bwd(dy, gp, w2t_pk, w1t_pk, x_mid, mean2, rstd2, gamma, dgamma, dbeta, wpt_pk, B, row_step, du, out, da):
    """block_tail2_bwd on the B rows r * row_step of the full-layout buffers (vitpe_tail_cls_bwd), in place: every other row
    of du / out (= d x_mid) / da keeps what it held; dgamma / dbeta accumulated."""
    require_device(dy, gp, w2t_pk, w1t_pk, x_mid, mean2, rstd2, gamma, dgamma, dbeta, wpt_pk, du, out, da)
    M, D = dy.shape
    HID = gp.shape[1]
    assert row_step >= 1 and (B == 0 or (B - 1) * row_step < M)
    assert gp.shape == du.shape == (M, HID) and x_mid.shape == out.shape == da.shape == (M, D)
    assert mean2.numel() == M and rstd2.numel() == M and w2t_pk.numel() == HID * D and w1t_pk.numel() == HID * D
    assert wpt_pk.numel() == D * D
    assert dy.dtype == w2t_pk.dtype == w1t_pk.dtype == x_mid.dtype == wpt_pk.dtype == du.dtype == out.dtype == da.dtype
    assert gp.dtype == torch.float16
    _f32(gamma, "gamma"), _f32(dgamma, "dgamma"), _f32(dbeta, "dbeta"), _f32(mean2, "mean2"), _f32(rstd2, "rstd2")
    check(lib().vitpe_tail_cls_bwd(dtype_code(dy.dtype), ptr(dy), ptr(gp), ptr(w2t_pk), ptr(w1t_pk), ptr(x_mid), ptr(mean2),
                                   ptr(rstd2), ptr(gamma), ptr(du), ptr(out), ptr(dgamma), ptr(dbeta), ptr(wpt_pk), ptr(da),
                                   int(B), int(row_step), D, HID, stream_ptr()), "vitpe_tail_cls_bwd")


class _WgradProblem(ctypes.Structure):   # include/vitpe.h: vitpe_wgrad_problem
    _fields_ = [("dY", ctypes.c_void_p), ("X", ctypes.c_void_p), ("dW", ctypes.c_void_p), ("dbias", ctypes.c_void_p),
                ("M", ctypes.c_int), ("N", ctypes.c_int), ("K", ctypes.c_int), ("x_op", ctypes.c_int),
                ("x_mean", ctypes.c_void_p), ("x_rstd", ctypes.c_void_p), ("x_gamma", ctypes.c_void_p),
                ("x_beta", ctypes.c_void_p)]


class WgradGroup:
    """A fixed list of weight-gradient problems (dY [M,N], X [M,K], dW [N,K] fp32, dbias [N] fp32 | None[, ln[, row_step]]),
    launched together by one vitpe_wgrad_group call.  The tensors are referenced, not copied.  The optional fifth
    element ln = (mean [M], rstd [M], gamma [K], beta [K]) makes the operand LayerNorm(X), recomputed inside the kernel
    from the raw rows X (the normalised tensor is never stored).  The optional sixth element row_step > 1 contracts over
    rows 0, row_step, 2 row_step, ... of dY, X and the statistics only (ceil(M / row_step) logical rows)."""

    MAX = 28

    def __init__(self, problems):
        problems = [tuple(p) + (None,) * (6 - len(p)) for p in problems]
        if not 0 < len(problems) <= self.MAX:
            raise L.VitpeError(f"WgradGroup takes 1..{self.MAX} problems, got {len(problems)}")
        # (what the kernel contracts over: the strided views of a row-step problem)
        self.keep = [(p[0][::p[5]], p[1][::p[5]]) + p[2:4] if p[5] else p[:4] for p in problems]
        self._full = [p[:2] for p in problems]
        self._ln = [p[4] for p in problems]
        self.dtype = problems[0][0].dtype
        self.arr = (_WgradProblem * len(problems))()
        self.steps = (ctypes.c_int * len(problems))(*[int(p[5] or 1) for p in problems])
        self.strided = any(st != 1 for st in self.steps)
        for i, (dy, x, dw, db, ln, rs) in enumerate(problems):
            require_device(dy, x, dw, db)
            rs = int(rs or 1)
            Mfull, N = dy.shape
            K = x.shape[1]
            assert rs >= 1 and x.shape[0] == Mfull and dw.numel() == N * K and dy.dtype == x.dtype == self.dtype
            assert dy.is_contiguous() and x.is_contiguous() and dw.is_contiguous()
            M = -(-Mfull // rs)
            _f32(dw, "dw"), _f32(db, "dbias")
            if ln is None:
                self.arr[i] = _WgradProblem(ptr(dy), ptr(x), ptr(dw), ptr(db), M, N, K, 0, None, None, None, None)
            else:
                mean, rstd, gamma, beta = ln
                require_device(mean, rstd, gamma, beta)
                for t_, n_ in ((mean, "mean"), (rstd, "rstd"), (gamma, "gamma"), (beta, "beta")):
                    _f32(t_, n_)
                assert mean.numel() == Mfull and rstd.numel() == Mfull and gamma.numel() == K and beta.numel() == K
                self.arr[i] = _WgradProblem(ptr(dy), ptr(x), ptr(dw), ptr(db), M, N, K, 1, ptr(mean), ptr(rstd), ptr(gamma),
                                            ptr(beta))

    def launch(self):
        if self.strided:
            check(lib().vitpe_wgrad_group_rows(dtype_code(self.dtype), ctypes.addressof(self.arr), ctypes.addressof(self.steps),
                                               len(self.arr), stream_ptr()), "vitpe_wgrad_group_rows")
            return
        check(lib().vitpe_wgrad_group(dtype_code(self.dtype), ctypes.addressof(self.arr), len(self.arr), stream_ptr()),
              "vitpe_wgrad_group")


def wgrad_group(problems):
    WgradGroup(problems).launch()


# ---- LayerNorm ------------------------------------------------------------------------------
def layernorm_fwd(x, gamma, beta, eps=1e-5, out=None, mean=None, rstd=None, stats_only=False):
    require_device(x, gamma, beta, out)
    D = x.shape[-1]
    M = x.numel() // D
    _f32(gamma, "gamma"), _f32(beta, "beta")
    y = None if stats_only else (out if out is not None else torch.empty_like(x))
    mean = mean if mean is not None else torch.empty(M, dtype=torch.float32, device=x.device)
    rstd = rstd if rstd is not None else torch.empty(M, dtype=torch.float32, device=x.device)
    check(lib().vitpe_layernorm_fwd(dtype_code(x.dtype), ptr(x), ptr(gamma), ptr(beta), ptr(y), ptr(mean), ptr(rstd),
                                    M, D, eps, stream_ptr()), "vitpe_layernorm_fwd")
    return y, mean, rstd


def layernorm_bwd_workspace(M, D, device):
    return torch.empty(lib().vitpe_layernorm_bwd_blocks(M) * 2 * D, dtype=torch.float32, device=device)


def layernorm_bwd(dy, x, mean, rstd, gamma, dgamma, dbeta, dres=None, out=None, workspace=None):
    """dx = dres + LN'(dy); dgamma/dbeta accumulated."""
    require_device(dy, x, mean, rstd, gamma, dgamma, dbeta, dres, out, workspace)
    D = x.shape[-1]
    M = x.numel() // D
    dx = out if out is not None else torch.empty_like(x)
    ws = workspace if workspace is not None else layernorm_bwd_workspace(M, D, x.device)
    check(lib().vitpe_layernorm_bwd(dtype_code(x.dtype), ptr(dy), ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(dres),
                                    ptr(dx), ptr(dgamma), ptr(dbeta), ptr(ws), M, D, stream_ptr()),
          "vitpe_layernorm_bwd")
    return dx


# ---- fused attention ------------------------------------------------------------------------
class PETables:
    """Device-side positional-encoding operands of the fused attention kernels."""

    def __init__(self, mode: str, grid: int, cos=None, sin=None, table=None, coeff=None, degree=0,
                 coeff_per_head=False):
        self.mode, self.grid = mode, grid
        self.cos, self.sin, self.table, self.coeff = cos, sin, table, coeff
        self.degree, self.coeff_per_head = degree, coeff_per_head

    @property
    def code(self):
        return L.PE_CODES[self.mode]


def _pe_tail(pe: PETables):
    """The positional-encoding operands of every attention entry point, in the C ABI's order."""
    return (pe.code, ptr(pe.cos), ptr(pe.sin), ptr(pe.table), ptr(pe.coeff), pe.grid, pe.degree, int(pe.coeff_per_head))


def _ln_variant(name, ln):
    """(entry-point name, LayerNorm operands) of a fused attention call: ln=(gamma, beta, mean, rstd) selects the _ln entry."""
    if ln is None:
        return name, ()
    require_device(*ln)
    return name + "_ln", tuple(ptr(t) for t in ln)


def fused_attention_supported(dtype, N, D, HD) -> bool:
    return bool(lib().vitpe_fused_attention_supported(dtype_code(dtype), N, D, HD))


def pack_qkv_weights(wqkv_f32, dtype, num_heads, out=None):
    """fp32 master [3D,D] -> fragment-major packed T copy consumed by the fused attention kernels."""
    require_device(wqkv_f32, out)
    _f32(wqkv_f32, "wqkv")
    D = wqkv_f32.shape[1]
    o = out if out is not None else torch.empty((3 * D, D), dtype=dtype, device=wqkv_f32.device)
    check(lib().vitpe_pack_qkv_weights(dtype_code(dtype), ptr(wqkv_f32), ptr(o), D, D // num_heads, stream_ptr()),
          "vitpe_pack_qkv_weights")
    return o


def fused_attention_fwd(xn, wqkv, num_heads, pe: PETables, out=None, ln=None, xn_out=None):
    """wqkv: PACKED weights (pack_qkv_weights).  ln=(gamma, beta, mean, rstd): `xn` holds the RAW tokens and
    the LayerNorm is applied while staging them (xn_out then receives LayerNorm(x))."""
    require_device(xn, wqkv, pe.cos, pe.sin, pe.table, pe.coeff, out, xn_out)
    B, N, D = xn.shape
    HD = D // num_heads
    assert wqkv.numel() == 3 * D * D and wqkv.dtype == xn.dtype
    o = out if out is not None else torch.empty_like(xn)
    name, lnp = _ln_variant("vitpe_fused_attention_fwd", ln)
    if ln is not None:
        lnp += (ptr(xn_out),)
    check(getattr(lib(), name)(dtype_code(xn.dtype), ptr(xn), *lnp, ptr(wqkv), ptr(o), B, N, D, HD, *_pe_tail(pe),
                               stream_ptr()), name)
    return o


def fused_attention_wide_supported(dtype, N, D, HD) -> bool:
    return bool(lib().vitpe_fused_attention_wide_supported(dtype_code(dtype), N, D, HD))


def pack_qkv_weights_wide(wqkv_f32, dtype, num_heads, out=None):
    """fp32 master [3D,D] -> the wide pack of the 32x32-tile forward kernel (include/vitpe.h: 3 D D elements, q rows
    pre-multiplied by hd^-0.5 log2 e)."""
    require_device(wqkv_f32, out)
    _f32(wqkv_f32, "wqkv")
    D = wqkv_f32.shape[1]
    n = lib().vitpe_qkv_wide_pack_elems(D)
    o = out if out is not None else torch.empty(n, dtype=dtype, device=wqkv_f32.device)
    assert o.numel() == n and o.dtype == dtype
    check(lib().vitpe_pack_qkv_weights_wide(dtype_code(dtype), ptr(wqkv_f32), ptr(o), D, D // num_heads, stream_ptr()),
          "vitpe_pack_qkv_weights_wide")
    return o


def fused_attention_fwd_wide(xn, wqkv_wide, num_heads, pe: PETables, out=None, ln=None, xn_out=None):
    """fused_attention_fwd on the 32x32-tile kernel (bf16, N = 65, D = 192, hd = 32); wqkv_wide = pack_qkv_weights_wide."""
    require_device(xn, wqkv_wide, pe.cos, pe.sin, pe.table, pe.coeff, out, xn_out)
    B, N, D = xn.shape
    HD = D // num_heads
    assert wqkv_wide.numel() == 3 * D * D and wqkv_wide.dtype == xn.dtype
    o = out if out is not None else torch.empty_like(xn)
    g = ln if ln is not None else (None, None, None, None)
    if ln is not None:
        require_device(*ln)
    check(lib().vitpe_fused_attention_fwd_wide(dtype_code(xn.dtype), ptr(xn), ptr(g[0]), ptr(g[1]), ptr(g[2]), ptr(g[3]),
                                               ptr(xn_out), ptr(wqkv_wide), ptr(o), B, N, D, HD, *_pe_tail(pe),
                                               stream_ptr()), "vitpe_fused_attention_fwd_wide")
    return o


def fused_attention_bwd(xn, wqkv, dout, num_heads, pe: PETables, dtable=None, dcoeff=None, dfreqs=None, out=None, ln=None):
    """-> dqkv [B,N,3D]; PE-parameter gradients accumulated into dtable/dcoeff/dfreqs.  ln=(gamma, beta, mean, rstd):
    `xn` holds the RAW tokens and the LayerNorm is recomputed while staging them (nothing normalised was stored)."""
    require_device(xn, wqkv, dout, dtable, dcoeff, dfreqs, out)
    B, N, D = xn.shape
    HD = D // num_heads
    dqkv = out if out is not None else torch.empty((B, N, 3 * D), dtype=xn.dtype, device=xn.device)
    name, lnp = _ln_variant("vitpe_fused_attention_bwd", ln)
    check(getattr(lib(), name)(dtype_code(xn.dtype), ptr(xn), *lnp, ptr(wqkv), ptr(dout), ptr(dqkv), B, N, D, HD,
                               *_pe_tail(pe), ptr(dtable), ptr(dcoeff), ptr(dfreqs), stream_ptr()), name)
    return dqkv


def attention_core_supported(dtype, N, HD):
    return bool(lib().vitpe_attention_core_supported(dtype_code(dtype), N, HD))


def attention_core_fwd(qkv, num_heads, pe: PETables, out=None):
    """qkv [B,N,3D] (output of the qkv Linear) -> merged heads [B,N,D]; one workgroup per (image, head)."""
    require_device(qkv, out)
    B, N, D3 = qkv.shape
    D = D3 // 3
    HD = D // num_heads
    o = out if out is not None else torch.empty((B, N, D), dtype=qkv.dtype, device=qkv.device)
    check(lib().vitpe_attention_core_fwd(dtype_code(qkv.dtype), ptr(qkv), ptr(o), B, N, num_heads, HD, *_pe_tail(pe),
                                         stream_ptr()), "vitpe_attention_core_fwd")
    return o


def attention_core_probs(qkv, num_heads, pe: PETables, cls_only=False, out=None):
    """qkv [B,N,3D] (output of the qkv Linear) -> the attention probabilities softmax(QK^T hd^-0.5 [+ bias]) in fp32:
    [B,H,N,N], or with cls_only the class token's row alone, [B,H,N] (bitwise row 0 of the full result).  The tensor the
    reference calls `attn` between softmax and attn_drop (vit.py:71-84), from the same operands as attention_core_fwd; never
    dropped out, no gradient."""
    require_device(qkv, out, pe.cos, pe.sin, pe.table, pe.coeff)
    B, N, D3 = qkv.shape
    HD = D3 // 3 // num_heads
    shape = (B, num_heads, N) if cls_only else (B, num_heads, N, N)
    o = out if out is not None else torch.empty(shape, dtype=torch.float32, device=qkv.device)
    if tuple(o.shape) != shape or o.dtype != torch.float32:
        raise L.VitpeError(f"attention_core_probs: out must be float32 {shape}")
    check(lib().vitpe_attention_core_probs(dtype_code(qkv.dtype), ptr(qkv), ptr(o), int(bool(cls_only)), B, N, num_heads, HD,
                                           *_pe_tail(pe), stream_ptr()), "vitpe_attention_core_probs")
    return o


# slots of attention_core_stats' [B,H,4] result (include/vitpe.h: VITPE_STAT_*)
STAT_DISTANCE, STAT_ENTROPY, STAT_CLS_MASS, STAT_CLS_ENTROPY = range(4)


def attention_core_stats(qkv, num_heads, pe: PETables, unit=1.0, weights=None, out=None):
    """qkv [B,N,3D] (output of the qkv Linear) -> (stats, colsum): statistics of the attention probabilities
    softmax(QK^T hd^-0.5 [+ bias]) reduced inside the kernel, the [N,N] maps never stored (vitpe_attention_core_stats).
    stats fp32 [B,H,4]: STAT_DISTANCE (mean attention distance over patch queries and keys on the pe.grid-wide raster, in
    units of `unit`), STAT_ENTROPY (mean row entropy, nats), STAT_CLS_MASS (mean attention of the patch queries on the class
    token), STAT_CLS_ENTROPY (entropy of the class row).  weights fp32 [B,N]: colsum fp32 [B,H,N] = sum_i weights[b,i] p_ij is
    returned as well (None otherwise); the stats are bitwise the same either way.  out: (stats, colsum_or_None) to write
    into.  Same operands, supported shapes and refusals as attention_core_fwd; no gradient."""
    o_stats, o_col = out if out is not None else (None, None)
    B, N, D3 = qkv.shape
    HD = D3 // 3 // num_heads
    # the argument checks come first and look at shapes and dtypes only: they raise before any device is touched
    if int(pe.grid) < 1:
        raise L.VitpeError(f"attention_core_stats: grid must be >= 1 (the token raster of the distance), got {pe.grid}")
    if weights is None and o_col is not None:
        raise L.VitpeError("attention_core_stats: a colsum output needs weights")
    if weights is not None and (weights.dtype != torch.float32 or tuple(weights.shape) != (B, N)
                                or not weights.is_contiguous()):
        raise L.VitpeError(f"attention_core_stats: weights must be float32, contiguous, {(B, N)}")
    require_device(qkv, weights, o_stats, o_col, pe.cos, pe.sin, pe.table, pe.coeff)
    if o_stats is None:
        o_stats = torch.empty((B, num_heads, 4), dtype=torch.float32, device=qkv.device)
    if weights is not None and o_col is None:
        o_col = torch.empty((B, num_heads, N), dtype=torch.float32, device=qkv.device)
    if tuple(o_stats.shape) != (B, num_heads, 4) or o_stats.dtype != torch.float32:
        raise L.VitpeError(f"attention_core_stats: stats out must be float32 {(B, num_heads, 4)}")
    if o_col is not None and (tuple(o_col.shape) != (B, num_heads, N) or o_col.dtype != torch.float32):
        raise L.VitpeError(f"attention_core_stats: colsum out must be float32 {(B, num_heads, N)}")
    check(lib().vitpe_attention_core_stats(dtype_code(qkv.dtype), ptr(qkv), ptr(o_stats), ptr(weights), ptr(o_col), float(unit),
                                           B, N, num_heads, HD, *_pe_tail(pe), stream_ptr()), "vitpe_attention_core_stats")
    return o_stats, o_col


def attention_core_relevance(qkv, dout, num_heads, pe: PETables, weights, clamp=True, out=None):
    """One propagation step of the gradient-weighted attention relevance (Chefer, Gur & Wolf, ICCV 2021), reduced inside
    the kernel (vitpe_attention_core_relevance): qkv [B,N,3D] (output of the qkv Linear), dout [B,N,D] (the gradient of a
    scalar w.r.t. the core's merged-head output, the tensor in front of proj; same dtype as qkv), weights fp32 [B,N]
    -> colsum fp32 [B,H,N] = sum_i weights[b,i] f(G_ij A_ij), with A the attention probabilities
    (attention_core_probs), G = dout_h V_h^T their gradient with V held fixed, f = max(0, .) under clamp (Chefer's rule) and
    the identity without.  Neither [N,N] tensor is stored; fixed summation order (two calls give the same bits).  out: the
    colsum to write into.  The operands of attention_core_fwd; refused beyond its refusals: the geometries whose K~ and V
    tiles do not fit the LDS together ("Attention relevance").  No gradient."""
    # the argument checks come first and look at shapes and dtypes only: they raise before any device is touched
    if qkv.dim() != 3 or qkv.shape[-1] % (3 * num_heads) != 0:
        raise L.VitpeError(f"attention_core_relevance: qkv must be [B, N, 3 * H * hd], got {tuple(qkv.shape)}")
    B, N, D3 = qkv.shape
    D = D3 // 3
    HD = D // num_heads
    if qkv.dtype not in (torch.float32, torch.bfloat16) or not qkv.is_contiguous():
        raise L.VitpeError("attention_core_relevance: qkv must be float32 or bfloat16, contiguous")
    if dout is None or tuple(dout.shape) != (B, N, D) or dout.dtype != qkv.dtype or not dout.is_contiguous():
        raise L.VitpeError(f"attention_core_relevance: dout must be {qkv.dtype}, contiguous, {(B, N, D)}")
    if weights is None:
        raise L.VitpeError("attention_core_relevance: weights are required")
    if weights.dtype != torch.float32 or tuple(weights.shape) != (B, N) or not weights.is_contiguous():
        raise L.VitpeError(f"attention_core_relevance: weights must be float32, contiguous, {(B, N)}")
    if out is not None and (tuple(out.shape) != (B, num_heads, N) or out.dtype != torch.float32 or not out.is_contiguous()):
        raise L.VitpeError(f"attention_core_relevance: colsum out must be float32, contiguous, {(B, num_heads, N)}")
    require_device(qkv, dout, weights, out, pe.cos, pe.sin, pe.table, pe.coeff)
    o = out if out is not None else torch.empty((B, num_heads, N), dtype=torch.float32, device=qkv.device)
    check(lib().vitpe_attention_core_relevance(dtype_code(qkv.dtype), ptr(qkv), ptr(dout), ptr(weights), ptr(o),
                                               int(bool(clamp)), B, N, num_heads, HD, *_pe_tail(pe), stream_ptr()),
          "vitpe_attention_core_relevance")
    return o


def attention_fused64_supported(dtype, N, num_heads, HD) -> bool:
    return bool(lib().vitpe_attention_fused64_supported(dtype_code(dtype), int(N), int(num_heads), int(HD)))


def attention_fused64_fwd(xn, wqkv_pk, num_heads, pe: PETables, qkv_out=None, out=None):
    """qkv projection + PE + attention core in one kernel at hd = 64 (ViT-B/16 geometry): xn [B,N,D] layer-normed tokens,
    wqkv_pk = pack_weight_frags(qkv.weight [3D,D], dtype, 64, 0); qkv_out (optional) [B,N,3D] gets the raw projection
    for attention_core_bwd.  -> merged heads [B,N,D]."""
    require_device(xn, wqkv_pk, qkv_out, out, pe.cos, pe.sin, pe.table, pe.coeff)
    B, N, D = xn.shape
    HD = D // num_heads
    assert wqkv_pk.numel() == 3 * D * D and wqkv_pk.dtype == xn.dtype
    if qkv_out is not None:
        assert qkv_out.shape == (B, N, 3 * D) and qkv_out.dtype == xn.dtype and qkv_out.is_contiguous()
    o = out if out is not None else torch.empty_like(xn)
    check(lib().vitpe_attention_fused64_fwd(dtype_code(xn.dtype), ptr(xn), ptr(wqkv_pk), ptr(qkv_out), ptr(o), B, N, num_heads,
                                            HD, *_pe_tail(pe), stream_ptr()), "vitpe_attention_fused64_fwd")
    return o


def attention_core_bwd(qkv, dout, num_heads, pe: PETables, dtable=None, dcoeff=None, dfreqs=None, out=None,
                       dcos=None, dsin=None):
    """-> dqkv [B,N,3D]; PE-parameter gradients accumulated into dtable/dcoeff/dfreqs.  dcos / dsin (both or neither,
    fp32, the shape of pe.cos / pe.sin): the gradients w.r.t. the caller's rotary tables are accumulated into them
    (vitpe_attention_core_bwd_tables; dfreqs is then not touched)."""
    require_device(qkv, dout, dtable, dcoeff, dfreqs, out, dcos, dsin)
    B, N, D3 = qkv.shape
    HD = D3 // 3 // num_heads
    dqkv = out if out is not None else torch.empty_like(qkv)
    if dcos is None and dsin is None:
        check(lib().vitpe_attention_core_bwd(dtype_code(qkv.dtype), ptr(qkv), ptr(dout), ptr(dqkv), B, N, num_heads, HD,
                                             *_pe_tail(pe), ptr(dtable), ptr(dcoeff), ptr(dfreqs),
                                             stream_ptr()), "vitpe_attention_core_bwd")
        return dqkv
    if dcos is None or dsin is None or pe.cos is None or dcos.shape != pe.cos.shape or dsin.shape != pe.sin.shape:
        raise L.VitpeError("attention_core_bwd: dcos and dsin must both be given, shaped like the rotary tables")
    _f32(dcos, "dcos"), _f32(dsin, "dsin")
    ws = torch.empty(4 * B * num_heads * (N - 1) * (HD // 2), dtype=torch.float32, device=qkv.device)
    check(lib().vitpe_attention_core_bwd_tables(dtype_code(qkv.dtype), ptr(qkv), ptr(dout), ptr(dqkv), B, N, num_heads, HD,
                                                *_pe_tail(pe), None, None, None, ptr(dcos), ptr(dsin), ptr(ws),
                                                stream_ptr()),
          "vitpe_attention_core_bwd_tables")
    return dqkv


# ---- dropout (csrc/dropout.hip, csrc/philox.h; DESIGN.md "Dropout streams") -----------------------------------------
SITE_ELEMENT, SITE_SAMPLE, SITE_ATTENTION = 0, 1, 2


def new_rng_pairs(n, device):
    """n (seed, offset) pairs [n, 2] int64 drawn from torch's device generator -- no host sync; torch.manual_seed
    therefore reproduces them.  The kernels read a pair as two unsigned 64-bit words."""
    return torch.empty((n, 2), dtype=torch.int64, device=device).random_()


def _check_rng(rng):
    require_device(rng)
    if rng.dtype != torch.int64 or rng.numel() != 2:
        raise L.VitpeError("rng must be a contiguous int64 device tensor of two words (seed, offset)")


def dropout_mask(rng, p, n=None, attn_shape=None):
    """uint8 keep mask of a site (tests only): n elements (elementwise / per-sample sites) or attn_shape = (B, H, N)
    -> [B, H, N, N]."""
    _check_rng(rng)
    if attn_shape is not None:
        B, H, N = attn_shape
        m = torch.empty((B, H, N, N), dtype=torch.uint8, device=rng.device)
        check(lib().vitpe_dropout_mask(SITE_ATTENTION, ptr(rng), ptr(m), 0, B, H, N, float(p), stream_ptr()),
              "vitpe_dropout_mask")
        return m
    m = torch.empty(n, dtype=torch.uint8, device=rng.device)
    check(lib().vitpe_dropout_mask(SITE_ELEMENT, ptr(rng), ptr(m), n, 0, 0, 0, float(p), stream_ptr()), "vitpe_dropout_mask")
    return m


def dropout_fwd(x, rng, p, resid=None, out=None):
    """y = [resid +] x . m / (1 - p); the mask is a function of (rng, element index, p) and is not stored."""
    require_device(x, resid, out)
    _check_rng(rng)
    y = out if out is not None else torch.empty_like(x)
    assert resid is None or (resid.shape == x.shape and resid.dtype == x.dtype)
    check(lib().vitpe_dropout_fwd(dtype_code(x.dtype), ptr(x), ptr(resid), ptr(y), x.numel(), ptr(rng), float(p),
                                  stream_ptr()), "vitpe_dropout_fwd")
    return y


def dropout_bwd(dy, rng, p, out=None):
    require_device(dy, out)
    _check_rng(rng)
    dx = out if out is not None else torch.empty_like(dy)
    check(lib().vitpe_dropout_bwd(dtype_code(dy.dtype), ptr(dy), ptr(dx), dy.numel(), ptr(rng), float(p), stream_ptr()),
          "vitpe_dropout_bwd")
    return dx


def drop_path_fwd(x, rng, p, resid=None, out=None):
    """y = [resid +] x * m_b / (1 - p), one decision per sample (leading dimension)."""
    require_device(x, resid, out)
    _check_rng(rng)
    y = out if out is not None else torch.empty_like(x)
    assert resid is None or (resid.shape == x.shape and resid.dtype == x.dtype)
    B = x.shape[0]
    check(lib().vitpe_drop_path_fwd(dtype_code(x.dtype), ptr(x), ptr(resid), ptr(y), B, x.numel() // max(B, 1), ptr(rng),
                                    float(p), stream_ptr()), "vitpe_drop_path_fwd")
    return y


def drop_path_bwd(dy, rng, p, out=None):
    require_device(dy, out)
    _check_rng(rng)
    dx = out if out is not None else torch.empty_like(dy)
    B = dy.shape[0]
    check(lib().vitpe_drop_path_bwd(dtype_code(dy.dtype), ptr(dy), ptr(dx), B, dy.numel() // max(B, 1), ptr(rng), float(p),
                                    stream_ptr()), "vitpe_drop_path_bwd")
    return dx


def _branch_drop_args(x, rng_elem, rng_path):
    if rng_elem is None and rng_path is None:
        raise L.VitpeError("branch_drop: at least one of rng_elem / rng_path must be given")
    for rng in (rng_elem, rng_path):
        if rng is not None:
            _check_rng(rng)
    B = x.shape[0]
    return B, x.numel() // max(B, 1)


def branch_drop_fwd(x, rng_elem, p_elem, rng_path, p_path, resid=None, out=None):
    """y = [resid +] (x . m_e / (1 - p_elem)) * m_b / (1 - p_path) in one pass: dropout_fwd followed by drop_path_fwd, bit
    for bit.  rng_elem / rng_path None leaves that site out; the samples are the leading dimension."""
    require_device(x, resid, out)
    B, per = _branch_drop_args(x, rng_elem, rng_path)
    y = out if out is not None else torch.empty_like(x)
    assert resid is None or (resid.shape == x.shape and resid.dtype == x.dtype)
    assert y.dtype == x.dtype and y.numel() == x.numel()
    check(lib().vitpe_branch_drop_fwd(dtype_code(x.dtype), ptr(x), ptr(resid), ptr(y), B, per, ptr(rng_elem), float(p_elem),
                                      ptr(rng_path), float(p_path), stream_ptr()), "vitpe_branch_drop_fwd")
    return y


def branch_drop_bwd(dy, rng_elem, p_elem, rng_path, p_path, out=None):
    """dx = dy . m_e / (1 - p_elem) * m_b / (1 - p_path) with the forward's pairs (dropout_bwd, then drop_path_bwd)."""
    require_device(dy, out)
    B, per = _branch_drop_args(dy, rng_elem, rng_path)
    dx = out if out is not None else torch.empty_like(dy)
    assert dx.dtype == dy.dtype and dx.numel() == dy.numel()
    check(lib().vitpe_branch_drop_bwd(dtype_code(dy.dtype), ptr(dy), ptr(dx), B, per, ptr(rng_elem), float(p_elem),
                                      ptr(rng_path), float(p_path), stream_ptr()), "vitpe_branch_drop_bwd")
    return dx


def rng_advance(table, inc=1):
    """offset += inc (mod 2^64) in every (seed, offset) row of `table` [n, 2] int64, on the device (no host sync)."""
    require_device(table)
    if table.dtype != torch.int64 or table.dim() != 2 or table.shape[1] != 2:
        raise L.VitpeError("rng_advance: table must be a contiguous [n, 2] int64 device tensor")
    check(lib().vitpe_rng_advance(ptr(table), table.shape[0], int(inc) & 0xFFFFFFFFFFFFFFFF, stream_ptr()),
          "vitpe_rng_advance")
    return table


def attention_core_fwd_drop(qkv, num_heads, pe: PETables, rng, p, out=None):
    """attention_core_fwd with attention-probability dropout (softmax -> dropout -> @ v) inside the kernel."""
    require_device(qkv, out)
    _check_rng(rng)
    B, N, D3 = qkv.shape
    D = D3 // 3
    HD = D // num_heads
    o = out if out is not None else torch.empty((B, N, D), dtype=qkv.dtype, device=qkv.device)
    check(lib().vitpe_attention_core_fwd_drop(dtype_code(qkv.dtype), ptr(qkv), ptr(o), B, N, num_heads, HD,
                                              *_pe_tail(pe), ptr(rng), float(p), stream_ptr()),
          "vitpe_attention_core_fwd_drop")
    return o


def attention_core_bwd_drop(qkv, dout, num_heads, pe: PETables, rng, p, dtable=None, dcoeff=None, dfreqs=None, out=None):
    """attention_core_bwd of attention_core_fwd_drop: the mask is regenerated from the same rng pair."""
    require_device(qkv, dout, dtable, dcoeff, dfreqs, out)
    _check_rng(rng)
    B, N, D3 = qkv.shape
    HD = D3 // 3 // num_heads
    dqkv = out if out is not None else torch.empty_like(qkv)
    check(lib().vitpe_attention_core_bwd_drop(dtype_code(qkv.dtype), ptr(qkv), ptr(dout), ptr(dqkv), B, N, num_heads, HD,
                                              *_pe_tail(pe), ptr(dtable), ptr(dcoeff), ptr(dfreqs),
                                              ptr(rng), float(p), stream_ptr()), "vitpe_attention_core_bwd_drop")
    return dqkv


# ---- patch embed ----------------------------------------------------------------------------
def unfold(images, patch, dtype, out=None):
    require_device(images, out)
    _f32(images, "images")
    B, C, S, _ = images.shape
    g = S // patch
    o = out if out is not None else torch.empty((B * g * g, C * patch * patch), dtype=dtype, device=images.device)
    check(lib().vitpe_unfold(dtype_code(dtype), ptr(images), ptr(o), B, C, S, patch, stream_ptr()), "vitpe_unfold")
    return o


def _check_augment(rng, crop_pad, S, what):
    """Arguments of the augmentation stream ("Augmentation stream"), checked before anything touches a device."""
    if not isinstance(rng, torch.Tensor) or rng.dtype != torch.int64 or rng.numel() != 2:
        raise L.VitpeError(f"{what}: rng must be a contiguous int64 device tensor of two words (seed, offset)")
    if int(crop_pad) < 0 or (S is not None and int(crop_pad) > int(S)):
        raise L.VitpeError(f"{what}: crop_pad must be in 0..S (the image size{'' if S is None else f', {int(S)}'}), got {crop_pad}")
    require_device(rng)


def augment_params(rng, B, crop_pad=0, hflip=False):
    """int32 [B, 3] = (oy, ox, flip) of batch slots 0..B-1 for the pair `rng` (tests only: the product kernels make the
    same draw in registers)."""
    _check_augment(rng, crop_pad, None, "augment_params")
    out = torch.empty((B, 3), dtype=torch.int32, device=rng.device)
    check(lib().vitpe_augment_params(ptr(rng), ptr(out), B, int(crop_pad), int(bool(hflip)), stream_ptr()),
          "vitpe_augment_params")
    return out


ERASE_MODES = {"const": 0, "rand": 1, "pixel": 2}     # timm's names: fill 0 / one normal per channel / one per pixel and channel
ERASE_SCALE, ERASE_RATIO = (0.02, 0.33), (0.3, 3.3)   # torchvision's defaults


def _check_erase(prob, mode, scale, ratio, C, what):
    """Arguments of the erasing stream ("Erasing stream"), checked before anything touches a device.
    -> the C entries' tail (erase_thr, erase_mode, smin, smax, lmin, lmax)."""
    try:
        prob, (smin, smax), (rmin, rmax) = float(prob), (float(v) for v in scale), (float(v) for v in ratio)
    except (TypeError, ValueError):
        raise L.VitpeError(f"{what}: erase_prob must be a number, erase_scale and erase_ratio pairs of numbers") from None
    if not 0.0 <= prob <= 1.0:
        raise L.VitpeError(f"{what}: erase_prob must be in [0, 1], got {prob}")
    if mode not in ERASE_MODES:
        raise L.VitpeError(f"{what}: erase_mode must be one of {sorted(ERASE_MODES)}, got {mode!r}")
    if not 0.0 < smin <= smax <= 1.0:
        raise L.VitpeError(f"{what}: erase_scale must satisfy 0 < min <= max <= 1, got {(smin, smax)}")
    if not (0.0 < rmin <= rmax and math.isfinite(rmax)):
        raise L.VitpeError(f"{what}: erase_ratio must satisfy 0 < min <= max, got {(rmin, rmax)}")
    if mode != "const" and C is not None and int(C) > 4:
        raise L.VitpeError(f"{what}: erase_mode {mode!r} draws at most 4 channels per call, the images have {int(C)}")
    thr = int(math.floor(ctypes.c_float(prob).value * 4294967296.0))     # floor((double)(float)prob 2^32)
    return thr, ERASE_MODES[mode], smin, smax, math.log(rmin), math.log(rmax)


def _erase_tail(rng, prob, mode, scale, ratio, C, what):
    """None when every erasing argument is at its default (the caller then takes the entry it took before the erasing stream
    existed), else the checked tail of the _erase entries."""
    if prob == 0. and mode == "const" and tuple(scale) == ERASE_SCALE and tuple(ratio) == ERASE_RATIO:
        return None
    tail = _check_erase(prob, mode, scale, ratio, C, what)
    if rng is None and tail[0] != 0:
        raise L.VitpeError(f"{what}: erase_prob > 0 needs rng, the (seed, offset) pair of the augmentation site")
    return tail if rng is not None else None


def erase_params(rng, B, S, prob, scale=ERASE_SCALE, ratio=ERASE_RATIO, host=False):
    """int32 [B, 5] = (on, i, j, h, w) of batch slots 0..B-1: the erasing stream's draws for the pair `rng` and image size S
    (tests only: the product kernels make the same draws in registers).  host=True: the same function compiled for the CPU;
    rng is then a pair of Python ints or a CPU int64 tensor of two words, the result a CPU tensor, no device is touched."""
    thr, _, smin, smax, lmin, lmax = _check_erase(prob, "const", scale, ratio, None, "erase_params")
    if int(S) < 1 or int(B) < 0:
        raise L.VitpeError(f"erase_params: B >= 0 and S >= 1 required, got B = {B}, S = {S}")
    if host:
        words = [int(v) & 0xFFFFFFFFFFFFFFFF for v in (rng.reshape(-1).tolist() if isinstance(rng, torch.Tensor) else rng)]
        if len(words) != 2:
            raise L.VitpeError("erase_params: rng must hold two words (seed, offset)")
        pair = (ctypes.c_ulonglong * 2)(*words)
        out = torch.zeros((int(B), 5), dtype=torch.int32)
        check(lib().vitpe_erase_params_host(ctypes.cast(pair, ctypes.c_void_p), out.data_ptr(), int(B), int(S), thr, smin, smax,
                                            lmin, lmax), "vitpe_erase_params_host")
        return out
    _check_augment(rng, 0, None, "erase_params")
    out = torch.empty((int(B), 5), dtype=torch.int32, device=rng.device)
    check(lib().vitpe_erase_params(ptr(rng), ptr(out), int(B), int(S), thr, smin, smax, lmin, lmax, stream_ptr()),
          "vitpe_erase_params")
    return out


def unfold_u8(data, index, mean, std, patch, dtype, out=None, img_out=None, rng=None, crop_pad=0, hflip=False,
              erase_prob=0., erase_mode="const", erase_scale=ERASE_SCALE, erase_ratio=ERASE_RATIO):
    """Resident uint8 dataset [Ndata,C,S,S] + sample indices [B] int64 (None: the first rows) -> normalised
    patch matrix [B*P, C*p*p] (ToTensor + Normalize + unfold in one pass); img_out optionally gets the fp32 images.
    rng (a (seed, offset) pair): RandomCrop(S, padding=crop_pad) + RandomHorizontalFlip (if hflip) per batch slot, on the
    augmentation stream, inside the same kernel; crop_pad / hflip are ignored without it.
    erase_prob > 0 (needs rng): RandomErasing(erase_prob, erase_scale, erase_ratio) with timm's fill mode erase_mode on top,
    on the erasing stream of the same pair."""
    erase = _erase_tail(rng, erase_prob, erase_mode, erase_scale, erase_ratio, data.shape[1], "unfold_u8")
    if rng is not None:
        _check_augment(rng, crop_pad, data.shape[2], "unfold_u8")
    require_device(data, index, mean, std, out, img_out)
    if data.dtype != torch.uint8 or (index is not None and index.dtype != torch.int64):
        raise L.VitpeError("unfold_u8: data must be uint8 and index int64")
    _f32(mean, "mean"), _f32(std, "std"), _f32(img_out, "img_out")
    _, C, S, _ = data.shape
    B = index.shape[0] if index is not None else data.shape[0]
    g = S // patch
    o = out if out is not None else torch.empty((B * g * g, C * patch * patch), dtype=dtype, device=data.device)
    if erase is not None:
        check(lib().vitpe_unfold_u8_erase(dtype_code(dtype), ptr(data), ptr(index), ptr(mean), ptr(std), ptr(o), ptr(img_out), B,
                                          C, S, patch, ptr(rng), int(crop_pad), int(bool(hflip)), *erase, stream_ptr()),
              "vitpe_unfold_u8_erase")
        return o
    if rng is not None:
        check(lib().vitpe_unfold_u8_aug(dtype_code(dtype), ptr(data), ptr(index), ptr(mean), ptr(std), ptr(o), ptr(img_out), B,
                                        C, S, patch, ptr(rng), int(crop_pad), int(bool(hflip)), stream_ptr()),
              "vitpe_unfold_u8_aug")
        return o
    check(lib().vitpe_unfold_u8(dtype_code(dtype), ptr(data), ptr(index), ptr(mean), ptr(std), ptr(o), ptr(img_out), B, C, S,
                                patch, stream_ptr()), "vitpe_unfold_u8")
    return o


def resize_coeffs(size_in: int, size_out: int):
    """Coefficient tables of one pass of PIL's 8-bit bilinear resample from length size_in to size_out (host only):
    -> (bounds int32 [out,2] = (first source index, tap count), kk int32 [out,ksize] = round(weight * 2^22))."""
    size_in, size_out = int(size_in), int(size_out)
    if size_in < 1 or size_out < 1:
        raise L.VitpeError(f"resize_coeffs: sizes must be positive (got {size_in} -> {size_out})")
    ksize = 2 * -(-max(size_in, size_out) // size_out) + 1      # 2 ceil(max(in / out, 1)) + 1
    bounds = torch.zeros((size_out, 2), dtype=torch.int32)
    kk = torch.zeros((size_out, ksize), dtype=torch.int32)
    got = lib().vitpe_resize_coeffs(size_in, size_out, bounds.data_ptr(), kk.data_ptr(), ksize)
    if got != ksize:
        raise L.VitpeError(f"vitpe_resize_coeffs({size_in}, {size_out}) returned {got}, expected ksize {ksize}")
    return bounds, kk


def resize_u8_supported(S0: int, S: int) -> bool:
    return bool(lib().vitpe_resize_u8_supported(int(S0), int(S)))


def resize_u8(images_u8, S: int, out=None):
    """transforms.Resize(S) on a device uint8 tensor [N,C,S0,S0] -> [N,C,S,S]: PIL's Image.resize((S, S), BILINEAR),
    bit for bit (S == S0: a copy).  `out` (optional) is a contiguous uint8 device tensor of at least N*C*S*S elements."""
    require_device(images_u8, out)
    S = int(S)
    if images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.shape[2] != images_u8.shape[3]:
        raise L.VitpeError("resize_u8: images must be uint8 [N,C,S0,S0] (square)")
    N, C, S0, _ = images_u8.shape
    if not resize_u8_supported(S0, S):
        raise L.VitpeError(f"resize_u8: {S0} -> {S} is not supported (source 8..64, target 4..512)")
    if out is None:
        out = torch.empty((N, C, S, S), dtype=torch.uint8, device=images_u8.device)
    elif out.dtype != torch.uint8 or out.numel() < N * C * S * S:
        raise L.VitpeError("resize_u8: out must be uint8 with at least N*C*S*S elements")
    bounds = kk = None
    ksize = 0
    if S != S0:
        bounds, kk = (t.to(images_u8.device) for t in resize_coeffs(S0, S))     # square: both passes share the tables
        ksize = kk.shape[1]
    check(lib().vitpe_resize_u8(ptr(images_u8), ptr(out), N * C, S0, S, ptr(bounds), ptr(kk), ptr(bounds), ptr(kk), ksize,
                                stream_ptr()), "vitpe_resize_u8")
    return out


def patch_embed_supported(dtype, C, S, p, D) -> bool:
    return bool(lib().vitpe_patch_embed_supported(dtype_code(dtype), C, S, p, D))


def patch_embed(w, bias, cls, ape, patch, dtype, images=None, data=None, index=None, mean=None, std=None, out=None,
                patches_out=None, stats=None, eps=1e-5, rng=None, crop_pad=0, hflip=False):
    """Fused unfold + patch-embed GEMM + bias + APE + class token (+ LayerNorm statistics of the token rows).
    images [B,C,S,S] fp32, or data (uint8 dataset) + index [B] int64 + mean/std [C].  w [D, C*p*p] in `dtype`.
    rng (data path only): the augmentation stream, as unfold_u8."""
    if rng is not None:
        if images is not None or data is None:
            raise L.VitpeError("patch_embed: rng (augmentation) needs the uint8 `data` path; augment fp32 images with "
                               "data.augment_batch first")
        _check_augment(rng, crop_pad, data.shape[2], "patch_embed")
    require_device(w, bias, cls, ape, images, data, index, mean, std, out, patches_out)
    src = images if images is not None else data
    C, S = src.shape[1], src.shape[2]
    B = images.shape[0] if images is not None else (index.shape[0] if index is not None else data.shape[0])
    D = w.shape[0]
    P = (S // patch) ** 2
    assert w.dtype == dtype and w.shape[1] == C * patch * patch
    _f32(bias, "bias"), _f32(cls, "cls"), _f32(ape, "ape"), _f32(images, "images")
    o = out if out is not None else torch.empty((B, P + 1, D), dtype=dtype, device=w.device)
    mo, ro = stats if stats is not None else (None, None)
    require_device(mo, ro)
    if rng is not None:
        check(lib().vitpe_patch_embed_aug(dtype_code(dtype), ptr(images), ptr(data), ptr(index), ptr(mean), ptr(std), ptr(w),
                                          ptr(bias), ptr(cls), ptr(ape), ptr(o), ptr(patches_out), ptr(mo), ptr(ro), B, C, S,
                                          patch, D, float(eps), ptr(rng), int(crop_pad), int(bool(hflip)), stream_ptr()),
              "vitpe_patch_embed_aug")
        return o
    check(lib().vitpe_patch_embed(dtype_code(dtype), ptr(images), ptr(data), ptr(index), ptr(mean), ptr(std), ptr(w), ptr(bias),
                                  ptr(cls), ptr(ape), ptr(o), ptr(patches_out), ptr(mo), ptr(ro), B, C, S, patch, D, float(eps),
                                  stream_ptr()), "vitpe_patch_embed")
    return o


def embed_bwd(dtok, dcls, dape, out=None):
    require_device(dtok, dcls, dape, out)
    B, Ntok, D = dtok.shape
    dpatch = out if out is not None else torch.empty((B * (Ntok - 1), D), dtype=dtok.dtype, device=dtok.device)
    check(lib().vitpe_embed_bwd(dtype_code(dtok.dtype), ptr(dtok), ptr(dcls), ptr(dape), ptr(dpatch), B, Ntok, D,
                                stream_ptr()), "vitpe_embed_bwd")
    return dpatch


def patch_embed_dgrad(dtok, w, C, S, p, out=None):
    """Image gradient of the patch embed (vitpe_patch_embed_dgrad): dtok [B, P+1, D] and the flattened Conv2d weight
    w [D, C p p], both of the compute type -> fp32 [B, C, S, S], fully overwritten."""
    require_device(dtok, w, out)
    if dtok.dim() != 3 or w.dim() != 2 or dtok.dtype != w.dtype:
        raise L.VitpeError("patch_embed_dgrad: dtok [B, P+1, D] and w [D, C p p] of one compute type")
    B, Ntok, D = dtok.shape
    C, S, p = int(C), int(S), int(p)
    if p < 1 or S < p or S % p != 0 or Ntok != (S // p) ** 2 + 1 or tuple(w.shape) != (D, C * p * p):
        raise L.VitpeError(f"patch_embed_dgrad: dtok {tuple(dtok.shape)} / w {tuple(w.shape)} do not belong to "
                           f"C={C}, S={S}, p={p}")
    _f32(out, "out")
    o = out if out is not None else torch.empty((B, C, S, S), dtype=torch.float32, device=dtok.device)
    if tuple(o.shape) != (B, C, S, S):
        raise L.VitpeError("patch_embed_dgrad: out must be [B, C, S, S]")
    check(lib().vitpe_patch_embed_dgrad(dtype_code(dtok.dtype), ptr(dtok), ptr(w), ptr(o), B, C, S, p, D, stream_ptr()),
          "vitpe_patch_embed_dgrad")
    return o


# ---- PE tables ------------------------------------------------------------------------------
def relative_position_index(L_, device):
    out = torch.empty((L_, L_), dtype=torch.int64, device=device)
    require_device(out)
    check(lib().vitpe_relative_position_index(ptr(out), L_, stream_ptr()), "vitpe_relative_position_index")
    return out


def l1_distance_matrix(G, device):
    out = torch.empty((G * G, G * G), dtype=torch.int64, device=device)
    require_device(out)
    check(lib().vitpe_l1_distance_matrix(ptr(out), G, stream_ptr()), "vitpe_l1_distance_matrix")
    return out


def rope_axial_tables(inv_freq, grid):
    require_device(inv_freq)
    half = inv_freq.numel() * 2
    cos = torch.empty((grid * grid, half), dtype=torch.float32, device=inv_freq.device)
    sin = torch.empty_like(cos)
    check(lib().vitpe_rope_axial_tables(ptr(inv_freq), ptr(cos), ptr(sin), grid, half, stream_ptr()),
          "vitpe_rope_axial_tables")
    return cos, sin


def rope_mixed_tables(freqs, grid, cos=None, sin=None):
    require_device(freqs, cos, sin)
    _, H, half = freqs.shape
    if cos is None:
        cos = torch.empty((H, grid * grid, half), dtype=torch.float32, device=freqs.device)
        sin = torch.empty_like(cos)
    check(lib().vitpe_rope_mixed_tables(ptr(freqs), ptr(cos), ptr(sin), H, grid, half, stream_ptr()),
          "vitpe_rope_mixed_tables")
    return cos, sin


def relative_bias(table, L_):
    require_device(table)
    H = table.shape[0]
    out = torch.empty((H, L_, L_), dtype=torch.float32, device=table.device)
    check(lib().vitpe_relative_bias(ptr(table), ptr(out), H, L_, stream_ptr()), "vitpe_relative_bias")
    return out


def polynomial_bias(coeff, H, grid, degree, per_head):
    require_device(coeff)
    L_ = grid * grid + 1
    out = torch.empty((H, L_, L_), dtype=torch.float32, device=coeff.device)
    check(lib().vitpe_polynomial_bias(ptr(coeff), ptr(out), H, grid, degree, int(per_head), stream_ptr()),
          "vitpe_polynomial_bias")
    return out


def relative_bias_bwd(dbias, L_):
    require_device(dbias)
    _f32(dbias, "dbias")
    H = dbias.shape[0]
    out = torch.empty((H, 2 * L_ - 1), dtype=torch.float32, device=dbias.device)
    check(lib().vitpe_relative_bias_bwd(ptr(dbias), ptr(out), H, L_, stream_ptr()), "vitpe_relative_bias_bwd")
    return out


def polynomial_bias_bwd(dbias, H, grid, degree, per_head):
    require_device(dbias)
    _f32(dbias, "dbias")
    out = torch.empty((H, degree + 1) if per_head else (degree + 1,), dtype=torch.float32, device=dbias.device)
    check(lib().vitpe_polynomial_bias_bwd(ptr(dbias), ptr(out), H, grid, degree, int(per_head), stream_ptr()),
          "vitpe_polynomial_bias_bwd")
    return out


def rope_mixed_tables_bwd(freqs, dcos, dsin, grid):
    require_device(freqs, dcos, dsin)
    _f32(dcos, "dcos"), _f32(dsin, "dsin")
    _, H, half = freqs.shape
    out = torch.empty_like(freqs)
    check(lib().vitpe_rope_mixed_tables_bwd(ptr(freqs), ptr(dcos), ptr(dsin), ptr(out), H, grid, half, stream_ptr()),
          "vitpe_rope_mixed_tables_bwd")
    return out


def apply_rotary(x, cos, sin):
    """rope_utils.py:18-37 on one tensor x [B,H,P,HD] fp32."""
    require_device(x, cos, sin)
    _f32(x, "x")
    B, H, P, HD = x.shape
    per_head = cos.dim() == 3
    y = torch.empty_like(x)
    check(lib().vitpe_apply_rotary(ptr(x), ptr(y), ptr(cos), ptr(sin), B, H, P, HD, int(per_head), stream_ptr()),
          "vitpe_apply_rotary")
    return y


def apply_rotary_bwd(dy, x, cos, sin, dcos=None, dsin=None, want_dx=True):
    """Backward of apply_rotary: -> dx [B,H,P,HD] fp32 (None unless want_dx); the gradients w.r.t. cos / sin ([P,HD/2] or
    [H,P,HD/2]) are ACCUMULATED into dcos / dsin when given (summed over the batch, and the heads for a 2-D table, in a
    fixed order).  x is only read for the table gradients."""
    require_device(dy, x, cos, sin, dcos, dsin)
    _f32(dy, "dy"), _f32(x, "x"), _f32(dcos, "dcos"), _f32(dsin, "dsin")
    B, H, P, HD = dy.shape
    per_head = cos.dim() == 3
    for t in (dcos, dsin):
        if t is not None and t.shape != cos.shape:
            raise L.VitpeError("apply_rotary_bwd: dcos / dsin must be shaped like cos / sin")
    dx = torch.empty_like(dy) if want_dx else None
    ws = None
    if dcos is not None or dsin is not None:
        R = B if per_head else B * H
        ws = torch.empty(2 * min(R, 64) * (H if per_head else 1) * P * (HD // 2), dtype=torch.float32, device=dy.device)
    check(lib().vitpe_apply_rotary_bwd(ptr(dy), ptr(x), ptr(cos), ptr(sin), ptr(dx), ptr(dcos), ptr(dsin), ptr(ws), B, H, P,
                                       HD, int(per_head), stream_ptr()), "vitpe_apply_rotary_bwd")
    return dx


# ---- head + loss ----------------------------------------------------------------------------
def head_fwd(x, gamma, beta, wh, bh, eps=1e-5, save=False, logits=None, ws=None):
    """logits [B,C] = Linear(LayerNorm(x[:,0])) ; ws = (xhat, yn, rstd) when save."""
    require_device(x, gamma, beta, wh, bh, logits)
    B, Ntok, D = x.shape
    Cn = wh.shape[0]
    lg = logits if logits is not None else torch.empty((B, Cn), dtype=torch.float32, device=x.device)
    if save and ws is None:
        ws = (torch.empty((B, D), dtype=torch.float32, device=x.device),
              torch.empty((B, D), dtype=torch.float32, device=x.device),
              torch.empty((B,), dtype=torch.float32, device=x.device))
    w0, w1, w2 = ws if ws is not None else (None, None, None)
    check(lib().vitpe_head_fwd(dtype_code(x.dtype), ptr(x), ptr(gamma), ptr(beta), ptr(wh), ptr(bh), ptr(lg), ptr(w0),
                               ptr(w1), ptr(w2), B, Ntok, D, Cn, eps, stream_ptr()), "vitpe_head_fwd")
    return lg, ws


def cross_entropy(logits, labels, grad_scale=None, dlogits=None, out2=None, want_grad=True):
    """-> (out2 = [mean loss, #correct], dlogits)."""
    require_device(logits, labels, dlogits, out2)
    B, Cn = logits.shape
    assert labels.dtype == torch.int64
    if want_grad and dlogits is None:
        dlogits = torch.empty_like(logits)
    o = out2 if out2 is not None else torch.empty(2, dtype=torch.float32, device=logits.device)
    gs = (1.0 / B) if grad_scale is None else grad_scale
    check(lib().vitpe_cross_entropy(ptr(logits), ptr(labels), ptr(dlogits), ptr(o), B, Cn, gs, stream_ptr()),
          "vitpe_cross_entropy")
    return o, dlogits


def cross_entropy_ctl(logits, labels, ctl, dlogits=None, out2=None, metric_acc=None):
    """cross_entropy with {grad_scale, loss_scale, n_valid} read from the device tensor `ctl` (float32[>=3]): rows
    >= n_valid are padding (dlogits 0, not counted); out2 = [loss_scale * sum of losses, #correct]; metric_acc += out2."""
    require_device(logits, labels, ctl, dlogits, out2, metric_acc)
    B, Cn = logits.shape
    assert labels.dtype == torch.int64 and ctl.dtype == torch.float32 and ctl.numel() >= 3
    _f32(dlogits, "dlogits"), _f32(out2, "out2"), _f32(metric_acc, "metric_acc")
    o = out2 if out2 is not None else torch.empty(2, dtype=torch.float32, device=logits.device)
    check(lib().vitpe_cross_entropy_ctl(ptr(logits), ptr(labels), ptr(dlogits), ptr(o), ptr(metric_acc), ptr(ctl), B, Cn,
                                        stream_ptr()), "vitpe_cross_entropy_ctl")
    return o, dlogits


def head_bwd(dlogits, wh, gamma, ws, dtype, Ntok, dwh, dbh, dgamma, dbeta, dx=None, ws_dyn=None):
    require_device(dlogits, wh, gamma, dwh, dbh, dgamma, dbeta, dx, ws_dyn)
    B, Cn = dlogits.shape
    D = wh.shape[1]
    if dx is None:
        dx = torch.empty((B, Ntok, D), dtype=dtype, device=dlogits.device)
    if ws_dyn is None:
        ws_dyn = torch.empty((B, D), dtype=torch.float32, device=dlogits.device)
    check(lib().vitpe_head_bwd(dtype_code(dtype), ptr(dlogits), ptr(wh), ptr(gamma), ptr(ws[0]), ptr(ws[1]),
                               ptr(ws[2]), ptr(ws_dyn), ptr(dx), ptr(dwh), ptr(dbh), ptr(dgamma), ptr(dbeta), B, Ntok,
                               D, Cn, stream_ptr()), "vitpe_head_bwd")
    return dx


def head_step(x, gamma, beta, wh, bh, labels, logits, dlogits, ws, ws_dyn, dx, out2, metric_acc, per_image, ctl, dwh, dbh,
              dgamma, dbeta, eps=1e-5, hp_tick=None):
    """The train step's head in one launch pair: final LayerNorm of the class row + logits + cross-entropy (device-side
    scalars `ctl`, as cross_entropy_ctl) + dlogits + the class row of dx (rows 1.. of dx are NOT touched: the caller
    keeps them zero) + parameter gradients (accumulated).  ws = (xhat, yn, rstd) work buffers; per_image [B,2] fp32."""
    require_device(x, gamma, beta, wh, bh, labels, logits, dlogits, ws[0], ws[1], ws_dyn, dx, out2, metric_acc, per_image, ctl,
                   dwh, dbh, dgamma, dbeta, hp_tick)
    B, Ntok, D = x.shape
    Cn = wh.shape[0]
    assert labels.dtype == torch.int64 and per_image.numel() >= 2 * B and ctl.numel() >= 3
    check(lib().vitpe_head_step(dtype_code(x.dtype), ptr(x), ptr(gamma), ptr(beta), ptr(wh), ptr(bh), ptr(labels), ptr(logits),
                                ptr(dlogits), ptr(ws[0]), ptr(ws[1]), ptr(ws_dyn), ptr(dx), ptr(out2), ptr(metric_acc),
                                ptr(per_image), ptr(ctl), ptr(dwh), ptr(dbh), ptr(dgamma), ptr(dbeta), B, Ntok, D, Cn, float(eps),
                                ptr(hp_tick), stream_ptr()), "vitpe_head_step")


# ---- optimizer / shadows --------------------------------------------------------------------
def adamw_step(p, g, m, v, hp, shadow_bf16=None, zero_grad=True, ticked=False, clipped=False):
    """ticked: the step counter / bias corrections in hp were already advanced (head_step hp_tick).
    clipped: scale the gradient by hp[9] (what grad_clip left there) instead of hp[8]."""
    require_device(p, g, m, v, hp, shadow_bf16)
    check(lib().vitpe_adamw_step(ptr(p), ptr(g), ptr(m), ptr(v), ptr(shadow_bf16), ptr(hp), p.numel(),
                                 int(bool(zero_grad)) | (2 if ticked else 0) | (4 if clipped else 0),
                                 stream_ptr()), "vitpe_adamw_step")


def adamw_groups_blocks(n: int) -> int:
    """Workgroups adamw_step_groups launches for n elements (the grid cap shows at n >= 2048 * 256 * 8)."""
    return lib().vitpe_adamw_groups_blocks(int(n))


def adamw_step_groups(p, g, m, v, hp, gid, gtab, shadow_bf16=None, zero_grad=True, ticked=False, clipped=False):
    """adamw_step with parameter groups: granule i / 8 of the flat buffers belongs to group gid[i / 8] (uint8, one byte per
    8 elements), which trains at lr = hp[0] * gtab[k, 0] and weight decay hp[4] * gtab[k, 1] (gtab: fp32 [n_groups, 2]);
    everything else as adamw_step, whose result it equals bit for bit when every scale is 1 (include/vitpe.h)."""
    require_device(p, g, m, v, hp, gid, gtab, shadow_bf16)
    for t, name in ((p, "p"), (g, "g"), (m, "m"), (v, "v"), (hp, "hp"), (gtab, "gtab")):
        if t is None:
            raise L.VitpeError(f"adamw_step_groups: {name} is missing")
        _f32(t, name)
    n = p.numel()
    if gid is None or gid.dtype != torch.uint8:
        raise L.VitpeError("adamw_step_groups: gid must be a uint8 tensor, one byte per 8-element granule")
    if hp.numel() < 16 or g.numel() != n or m.numel() != n or v.numel() != n:
        raise L.VitpeError("adamw_step_groups: hp must hold 16 floats and g, m, v as many elements as p")
    if gtab.numel() < 2 or gtab.numel() % 2 or gtab.numel() > 512:
        raise L.VitpeError(f"adamw_step_groups: gtab must hold 1..256 (lr, weight decay) scale pairs, got {gtab.numel()} floats")
    if gid.numel() < (n + 7) // 8:
        raise L.VitpeError(f"adamw_step_groups: gid holds {gid.numel()} granules, {n} elements need {(n + 7) // 8}")
    if shadow_bf16 is not None and (shadow_bf16.dtype != torch.bfloat16 or shadow_bf16.numel() != n):
        raise L.VitpeError("adamw_step_groups: shadow_bf16 (bf16) must hold as many elements as p")
    check(lib().vitpe_adamw_step_groups(ptr(p), ptr(g), ptr(m), ptr(v), ptr(shadow_bf16), ptr(hp), n,
                                        int(bool(zero_grad)) | (2 if ticked else 0) | (4 if clipped else 0),
                                        ptr(gid), gid.numel(), ptr(gtab), gtab.numel() // 2, stream_ptr()),
          "vitpe_adamw_step_groups")


def lr_schedule(hp, sched, ticked=False):
    """hp[0] = sched[6] = the linear warm-up + cosine learning rate of step k = hp[5] - sched[5] (- 1 when `ticked`: the
    head already advanced the counter), one lane on the device; sched: the 8-float block of include/vitpe.h."""
    require_device(hp, sched)
    if hp is None or sched is None:
        raise L.VitpeError("lr_schedule: hp and sched are required")
    _f32(hp, "hp"); _f32(sched, "sched")
    if hp.numel() < 16 or sched.numel() < 8:
        raise L.VitpeError("lr_schedule: hp must hold 16 floats and sched 8")
    check(lib().vitpe_lr_schedule(ptr(hp), ptr(sched), int(bool(ticked)), stream_ptr()), "vitpe_lr_schedule")


def grad_clip_blocks(n: int) -> int:
    """Floats of the work buffer grad_clip needs for a gradient of n elements."""
    return lib().vitpe_grad_clip_blocks(int(n))


def grad_clip(g, hp, partial):
    """clip_grad_norm_ on the flat fp32 gradient g (a 1-d view at any element offset), on the device: hp[10] =
    hp[8] * ||g||, hp[11] = min(1, hp[12] / (hp[10] + 1e-6)), hp[9] = hp[8] * hp[11] (include/vitpe.h); g is left as it
    is -- adamw_step(clipped=True) applies hp[9].  partial: fp32 work buffer of >= grad_clip_blocks(g.numel()) floats."""
    require_device(g, hp, partial)
    _f32(g, "g"); _f32(hp, "hp"); _f32(partial, "partial")
    if hp.numel() < 16:
        raise L.VitpeError(f"grad_clip: hp must hold 16 floats, got {hp.numel()}")
    check(lib().vitpe_grad_clip(ptr(g), g.numel(), ptr(hp), ptr(partial), partial.numel(), stream_ptr()), "vitpe_grad_clip")


def ema_blocks(n: int) -> int:
    """Workgroups ema_update / ema_swap launch for n elements (the grid cap shows at n >= 2048 * 256 * 4)."""
    return lib().vitpe_ema_blocks(int(n))


def ema_update(p, e, hp, warmup=False):
    """e += (1 - d_t) * (p - e) on the flat fp32 buffers, one launch: d_t = hp[13], or with warmup
    min(hp[13], (1 + t) / (10 + t)) at t = hp[5] - hp[14]; d_t is left in hp[15] (include/vitpe.h).  p is only read."""
    require_device(p, e, hp)
    _f32(p, "p"); _f32(e, "e"); _f32(hp, "hp")
    if hp is None or hp.numel() < 16 or e.numel() != p.numel():
        raise L.VitpeError("ema_update: hp must hold 16 floats and e as many elements as p")
    check(lib().vitpe_ema_update(ptr(p), ptr(e), ptr(hp), p.numel(), int(bool(warmup)), stream_ptr()), "vitpe_ema_update")


def ema_swap(p, e, shadow_bf16=None):
    """p <-> e in place; shadow_bf16 (optional) = bf16 of the new p, as cast() rounds.  Twice restores every bit."""
    require_device(p, e, shadow_bf16)
    _f32(p, "p"); _f32(e, "e")
    if e.numel() != p.numel() or (shadow_bf16 is not None and (shadow_bf16.dtype != torch.bfloat16 or
                                                               shadow_bf16.numel() != p.numel())):
        raise L.VitpeError("ema_swap: e (fp32) and shadow_bf16 (bf16) must hold as many elements as p")
    check(lib().vitpe_ema_swap(ptr(p), ptr(e), ptr(shadow_bf16), p.numel(), stream_ptr()), "vitpe_ema_swap")


def cast(src, dtype, out=None):
    require_device(src, out)
    _f32(src, "src")
    o = out if out is not None else torch.empty(src.shape, dtype=dtype, device=src.device)
    check(lib().vitpe_cast(dtype_code(dtype), ptr(src), ptr(o), src.numel(), stream_ptr()), "vitpe_cast")
    return o


def transpose_cast(src, dtype, out=None):
    """[R,C] fp32 -> [C,R] T."""
    require_device(src, out)
    _f32(src, "src")
    R, C = src.shape
    o = out if out is not None else torch.empty((C, R), dtype=dtype, device=src.device)
    check(lib().vitpe_transpose_cast(dtype_code(dtype), ptr(src), ptr(o), R, C, stream_ptr()), "vitpe_transpose_cast")
    return o


def refresh_shadows(flat, dst_base, desc, ndesc, total_tiles, tile_map=None):
    require_device(flat, dst_base, desc, tile_map)
    assert tile_map is None or (tile_map.dtype == torch.int16 and tile_map.numel() == total_tiles)
    check(lib().vitpe_refresh_shadows(dtype_code(dst_base.dtype), ptr(flat), ptr(dst_base), ptr(desc), ndesc, total_tiles,
                                      ptr(tile_map), stream_ptr()), "vitpe_refresh_shadows")


def selftest_mma(a, bt, brow):
    require_device(a, bt, brow)
    c_row = torch.empty((16, 16), dtype=torch.float32, device=a.device)
    c_tr = torch.empty((16, 16), dtype=torch.float32, device=a.device)
    check(L.debug_lib().vitpe_selftest_mma(dtype_code(a.dtype), ptr(a), ptr(bt), ptr(brow), ptr(c_row), ptr(c_tr),
                                   stream_ptr()), "vitpe_selftest_mma")
    return c_row, c_tr
