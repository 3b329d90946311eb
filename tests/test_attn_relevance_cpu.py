"""Gradient-weighted attention relevance (vitpe_attention_core_relevance), the part that needs no GPU: the float64 references
of the GPU tests (attn_relevance_ref.py) are pinned to autograd, to the row identity and to the explicit matrix product,
the restated forward to the oracle's; the header declares the entry point and the library exports it; the host wrapper
checks its arguments before it looks for a device; the wrapper and the module methods refuse CPU tensors."""
import ctypes

import pytest
import torch

from attn_relevance_ref import (err_measure, model_forward, ref_grad_attn, ref_model_relevance, ref_relevance,
                                ref_relevance_rollout)
from oracle import vit_oracle as O


def _operands(B=2, H=3, N=10, hd=8, seed=1):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, N, 3 * H * hd, generator=g, dtype=torch.float64)
    dout = torch.randn(B, N, H * hd, generator=g, dtype=torch.float64)
    p = torch.randn(B, H, N, N, generator=g, dtype=torch.float64).softmax(-1)
    return qkv, dout, p


# ------------------------------------------------------------------------------------------ the references
def test_ref_grad_attn_is_autograds_gradient_of_the_attention_output():
    """G = d (sum dO . (A V)) / dA with V held fixed"""
    qkv, dout, p = _operands()
    B, N, D3 = qkv.shape
    H, D = 3, D3 // 3
    a = p.clone().requires_grad_(True)
    v = qkv.reshape(B, N, 3, H, D // H).permute(2, 0, 3, 1, 4)[2]
    o = (a @ v).transpose(1, 2).reshape(B, N, D)
    (dout * o).sum().backward()
    G = ref_grad_attn(qkv, dout, H)
    assert tuple(G.shape) == (B, H, N, N) and G.dtype == torch.float64
    assert float((G - a.grad).abs().max()) < 1e-12
    assert float((G - G.transpose(-1, -2)).abs().max()) > 0.1   # (asymmetric: a transposed G is not the same thing)


def test_row_identity_sum_j_G_A_is_dO_dot_O():
    qkv, dout, p = _operands(seed=2)
    B, N, D3 = qkv.shape
    H, D = 3, D3 // 3
    v = qkv.reshape(B, N, 3, H, D // H).permute(2, 0, 3, 1, 4)[2]
    o = p @ v                                                        # [B, H, N, hd]
    do = dout.reshape(B, N, H, D // H).permute(0, 2, 1, 3)
    G = ref_grad_attn(qkv, dout, H)
    assert float(((G * p).sum(-1) - (do * o).sum(-1)).abs().max()) < 1e-12
    # ref_relevance with weights e_i, unclamped, summed over the keys is that row's value
    for i in (0, N - 1):
        w = torch.zeros(B, N, dtype=torch.float64)
        w[:, i] = 1.0
        c, ca = ref_relevance(p, G, w, clamp=False)
        assert float((c.sum(-1) - (do * o).sum(-1)[..., i]).abs().max()) < 1e-12
        assert float((ca - (G * p).abs()[:, :, i]).abs().max()) < 1e-12


def test_ref_relevance_clamps_per_head_and_entry():
    qkv, dout, p = _operands(seed=3)
    G = ref_grad_attn(qkv, dout, 3)
    w = torch.randn(2, 10, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    c1, a1 = ref_relevance(p, G, w, clamp=True)
    c0, a0 = ref_relevance(p, G, w, clamp=False)
    want1 = torch.stack([torch.stack([w[b] @ (G[b, h] * p[b, h]).clamp(min=0) for h in range(3)]) for b in range(2)])
    want0 = torch.stack([torch.stack([w[b] @ (G[b, h] * p[b, h]) for h in range(3)]) for b in range(2)])
    assert float((c1 - want1).abs().max()) < 1e-12 and float((c0 - want0).abs().max()) < 1e-12
    assert torch.equal(a0, a1) and bool((a0 >= c0.abs() - 1e-12).all()) and bool((a0 >= c1.abs() - 1e-12).all())
    assert err_measure(c0, c0, a0) == 0.0


def test_ref_relevance_rollout_is_the_explicit_products_class_row():
    N = 4
    a0 = torch.tensor([[0.0, 0.5, 0.0, 0.0], [0.25, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0, 0.0], [2.0, 0.0, 0.0, 0.5]],
                      dtype=torch.float64)
    a1 = torch.tensor([[0.5, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 0.0], [0.0, 0.25, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0]],
                      dtype=torch.float64)
    maps = [torch.stack([a0, a1.t()]), torch.stack([a1, a0.t()])]    # [B = 2, N, N] per layer, bottom first
    eye = torch.eye(N, dtype=torch.float64)
    R = (eye + maps[1]) @ (eye + maps[0])
    r = ref_relevance_rollout(maps)
    assert float((r - R[:, 0]).abs().max()) < 1e-12
    # image 0 by hand: e_cls (I + a1) = [1.5, 0, 1, 0]; times (I + a0) = [1.5, 0.75, 1, 0]
    assert float((r[0] - torch.tensor([1.5, 0.75, 1.0, 0.0], dtype=torch.float64)).abs().max()) < 1e-12
    assert float((ref_relevance_rollout(maps[1:]) - (eye + maps[1])[:, 0]).abs().max()) < 1e-12
    # the order matters: the product the other way round is another vector
    assert float((r - ((eye + maps[0]) @ (eye + maps[1]))[:, 0]).abs().max()) > 0.1


def tiny_cfg(mode):
    return O.VitConfig(img_size=16, patch_size=4, embed_dim=64, depth=2, num_heads=2, pos_encoding=mode)


@pytest.mark.parametrize("mode", ["none", "relative", "polynomial", "rope-axial", "rope-mixed"])
def test_ref_model_forward_is_the_oracles(mode):
    cfg = tiny_cfg(mode)
    params = {k: v.double() for k, v in O.closed_form_params(cfg).items()}
    images = O.closed_form_batch(cfg, 2)[0].double()
    want = O.forward(cfg, params, images)
    logits, attns = model_forward(cfg, params, images)
    assert float((logits - want).abs().max()) < 1e-12
    assert len(attns) == 2 and tuple(attns[0].shape) == (2, 2, 17, 17)
    r, lg, t, scale = ref_model_relevance(cfg, params, images)
    assert float((lg - want).abs().max()) < 1e-12 and torch.equal(t, want.argmax(1))
    assert tuple(r.shape) == (2, 17) and r.dtype == torch.float64 and bool((r[:, 0] >= 1.0).all()) and bool((r >= 0).all())
    e_cls = torch.zeros(2, 17, dtype=torch.float64)
    e_cls[:, 0] = 1.0
    assert bool((scale >= r - e_cls - 1e-15).all()) and float(scale.max()) > 0.0   # |.| bounds the clamped terms
    r1 = ref_model_relevance(cfg, params, images, target=torch.tensor([3, 0]), start=1, clamp=False)[0]
    assert float((r1 - r).abs().max()) > 0.0


# ------------------------------------------------------------------------------------------ header, library
def test_library_exports_the_entry_point_and_the_header_declares_it():
    from vitpe import _lib
    protos = _lib.parse_header()
    assert "vitpe_attention_core_relevance" in protos
    args = protos["vitpe_attention_core_relevance"]
    # (dtype, qkv, dout, weights, colsum, clamp, B, N, H, HD, mode, cos, sin, table, coeff, grid, degree, coeff_per_head, stream)
    assert len(args) == 19
    assert args[0] is ctypes.c_int and all(a is ctypes.c_void_p for a in args[1:5])
    assert all(a is ctypes.c_int for a in args[5:11]) and all(a is ctypes.c_void_p for a in args[11:15])
    assert all(a is ctypes.c_int for a in args[15:18]) and args[18] is ctypes.c_void_p
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "vitpe_attention_core_relevance")
    assert ctypes.CDLL(_lib.LIB_PATH).vitpe_abi_version() == 5   # entries are only added


# ------------------------------------------------------------------------------------------ refusals without a device
def test_host_wrapper_refuses_a_cpu_tensor():
    from vitpe import kernels as K
    from vitpe._lib import VitpeError
    with pytest.raises(VitpeError, match="no CPU fallback"):
        K.attention_core_relevance(torch.zeros(1, 17, 3 * 64), torch.zeros(1, 17, 64), 2, K.PETables("none", 4), torch.zeros(1, 17))
    with pytest.raises(VitpeError, match="no CPU fallback"):
        K.attention_core_relevance(torch.zeros(1, 17, 3 * 64), torch.zeros(1, 17, 64), 2, K.PETables("none", 4), torch.zeros(1, 17),
                                   clamp=False, out=torch.zeros(1, 2, 17))


def test_argument_checks_come_before_any_device():
    """on CPU tensors the shape / dtype errors are raised, not the device refusal that a valid call would get"""
    from vitpe import kernels as K
    from vitpe._lib import VitpeError
    qkv, dout, w, pe = torch.zeros(2, 17, 3 * 64), torch.zeros(2, 17, 64), torch.zeros(2, 17), K.PETables("none", 4)
    with pytest.raises(VitpeError, match="weights are required"):
        K.attention_core_relevance(qkv, dout, 2, pe, None)
    with pytest.raises(VitpeError, match="weights must be float32"):
        K.attention_core_relevance(qkv, dout, 2, pe, torch.zeros(2, 16))
    with pytest.raises(VitpeError, match="weights must be float32"):
        K.attention_core_relevance(qkv, dout, 2, pe, torch.zeros(2, 17, dtype=torch.float64))
    with pytest.raises(VitpeError, match="weights must be float32"):
        K.attention_core_relevance(qkv, dout, 2, pe, torch.zeros(17, 2).t())   # not contiguous
    with pytest.raises(VitpeError, match="dout must be"):
        K.attention_core_relevance(qkv, torch.zeros(2, 17, 3 * 64), 2, pe, w)
    with pytest.raises(VitpeError, match="dout must be"):
        K.attention_core_relevance(qkv, dout.bfloat16(), 2, pe, w)
    with pytest.raises(VitpeError, match="dout must be"):
        K.attention_core_relevance(qkv, torch.zeros(2, 64, 17).transpose(1, 2), 2, pe, w)   # not contiguous
    with pytest.raises(VitpeError, match="qkv must be"):
        K.attention_core_relevance(torch.zeros(2, 17, 3 * 64 + 1), dout, 2, pe, w)
    with pytest.raises(VitpeError, match="qkv must be"):
        K.attention_core_relevance(qkv.double(), dout.double(), 2, pe, w)
    with pytest.raises(VitpeError, match="colsum out must be"):
        K.attention_core_relevance(qkv, dout, 2, pe, w, out=torch.zeros(2, 2, 16))


def test_module_methods_refuse_a_cpu_tensor():
    from vitpe._lib import VitpeError
    from vitpe.vit import Attention, Block, VisionTransformer
    x = torch.zeros(1, 17, 64)
    with pytest.raises(VitpeError, match="no CPU fallback"):
        Attention(64, num_heads=2).attention_relevance(x, x)
    with pytest.raises(VitpeError, match="no CPU fallback"):
        Block(64, 2).attention_relevance(x, x, weights=torch.zeros(1, 17))
    model = VisionTransformer(img_size=16, patch_size=4, embed_dim=64, depth=2, num_heads=2, pos_encoding="relative")
    with pytest.raises(VitpeError, match="no CPU fallback"):
        model.attention_relevance(torch.zeros(1, 3, 16, 16))
    assert model.training


def test_model_method_argument_errors_are_value_errors():
    from vitpe.vit import VisionTransformer
    model = VisionTransformer(img_size=16, patch_size=4, embed_dim=64, depth=2, num_heads=2, pos_encoding="none")
    x = torch.zeros(2, 3, 16, 16)
    for start in (-1, 2):
        with pytest.raises(ValueError, match="start_layer"):
            model.attention_relevance(x, start_layer=start)
    for target in (torch.zeros(3, dtype=torch.int64), torch.zeros(2, dtype=torch.int32), torch.zeros(2, 1, dtype=torch.int64),
                   [0, 1]):
        with pytest.raises(ValueError, match="target"):
            model.attention_relevance(x, target=target)
    assert model.training and all(m.training for m in model.modules())
