"""Attention probabilities (vitpe_attention_core_probs), the part that needs no GPU: the yardstick of the GPU tests is pinned
to the oracle, the library exports the entry point, the host wrapper refuses CPU tensors and the op's fake implementation
returns the right shapes.

ref_probs is ref_attention (attn_tokens.py) up to `s.softmax(-1)`: the reference's `attn` between softmax and attn_drop
(models/vit.py:71-84), on a projection qkv [B, N, 3D]."""
import ctypes

import pytest
import torch

from attn_tokens import attn_case, q
from conftest import rel_err
from oracle import vit_oracle as O
from test_kernels_gpu import ATTN_MODES, oracle_attn


def ref_probs(qkv, H, mode, pe):
    """softmax(QK^T hd^-0.5 [+ bias]) [B, H, N, N] of a projection qkv [B, N, 3D] (any float dtype), rotation and bias from
    the oracle's table functions.  pe: the leaves of the positional encoding (table / coeff / inv_freq / freqs)."""
    B, N, D3 = qkv.shape
    D = D3 // 3
    hd = D // H
    qq, kk, _ = qkv.reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    if mode.startswith("rope"):
        if mode == "rope-axial":
            cos, sin = O.rope_axial_tables(N - 1, pe["inv_freq"])
        else:
            cos, sin = O.rope_mixed_tables(N - 1, pe["freqs"])
        cos, sin = cos.to(qkv.dtype), sin.to(qkv.dtype)
        cos, sin = (cos[None, None], sin[None, None]) if cos.dim() == 2 else (cos[None], sin[None])
        h2 = hd // 2

        def rot(t):
            t1, t2 = t[:, :, 1:, :h2], t[:, :, 1:, h2:]
            return torch.cat([t[:, :, :1], torch.cat([t1 * cos - t2 * sin, t1 * sin + t2 * cos], dim=-1)], dim=2)
        qq, kk = rot(qq), rot(kk)
    s = (qq @ kk.transpose(-2, -1)) * hd ** -0.5
    if mode == "relative":
        idx = torch.arange(N)[:, None] - torch.arange(N)[None, :] + N - 1
        s = s + pe["table"].to(qkv.dtype)[:, idx]
    elif mode.startswith("polynomial"):
        s = s + O.polynomial_bias(pe["coeff"], N - 1, H, 3, mode == "polynomial").to(qkv.dtype)
    return s.softmax(dim=-1)


def probs_times_v(p, qkv, H):
    """probs [B, H, N, N] @ v of the projection, heads merged -> [B, N, D]"""
    B, N, D3 = qkv.shape
    D = D3 // 3
    v = qkv.reshape(B, N, 3, H, D // H).permute(2, 0, 3, 1, 4)[2]
    return (p.to(v.dtype) @ v).transpose(1, 2).reshape(B, N, D)


@pytest.mark.parametrize("mode", ATTN_MODES)
def test_ref_probs_times_v_is_the_oracle_attention_core(mode):
    D, H, B = 64, 2, 2
    N, hd, G, xn, wqkv, dout, pe = attn_case(mode, D, H, B, seed=60, G=5)
    assert N == 26
    ref, _, _ = oracle_attn(mode, xn, wqkv, dout, pe, H, "f32")
    qkv = torch.nn.functional.linear(q(xn, "f32"), q(wqkv, "f32"))
    p = ref_probs(qkv, H, mode, pe)
    assert p.shape == (B, H, N, N)
    assert rel_err(probs_times_v(p, qkv, H), ref) < 1e-6


def test_library_exports_the_entry_point_and_the_header_declares_it():
    from vitpe import _lib
    protos = _lib.parse_header()
    assert "vitpe_attention_core_probs" in protos
    args = protos["vitpe_attention_core_probs"]
    # (dtype, qkv, probs, cls_only, B, N, H, HD, mode, cos, sin, table, coeff, grid, degree, coeff_per_head, stream)
    assert len(args) == 17 and args[1] is ctypes.c_void_p and args[2] is ctypes.c_void_p and args[3] is ctypes.c_int
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "vitpe_attention_core_probs")


def test_host_wrapper_refuses_a_cpu_tensor():
    from vitpe import kernels as K
    from vitpe._lib import VitpeError
    with pytest.raises(VitpeError, match="no CPU fallback"):
        K.attention_core_probs(torch.zeros(1, 17, 3 * 64), 2, K.PETables("none", 4))
    with pytest.raises(VitpeError, match="no CPU fallback"):
        K.attention_core_probs(torch.zeros(1, 17, 3 * 64), 2, K.PETables("none", 4), cls_only=True)


@pytest.mark.parametrize("cls_only", [False, True])
def test_op_fake_implementation_returns_the_shape(cls_only):
    from vitpe import ops  # noqa: F401  (registers torch.ops.vitpe.*)
    B, N, H, hd = 3, 26, 2, 32
    qkv = torch.empty(B, N, 3 * H * hd, device="meta", dtype=torch.bfloat16)
    out = torch.ops.vitpe.attention_probs(qkv, H, 0, 5, None, None, 0, False, None, None, cls_only)
    assert out.device.type == "meta" and out.dtype == torch.float32
    assert tuple(out.shape) == ((B, H, N) if cls_only else (B, H, N, N))
    assert not out.requires_grad
