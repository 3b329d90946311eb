"""Attention statistics (vitpe_attention_core_stats), the part that needs no GPU: the float64 references of the GPU tests
(attn_stats_ref.py) are pinned to closed forms, the header declares the entry point and its slots and the library exports
it, the host wrapper checks its arguments before it looks for a device, and the wrapper and the module methods refuse CPU
tensors."""
import ctypes
import math
import re

import pytest
import torch

from attn_stats_ref import (CLS_ENTROPY, CLS_MASS, DISTANCE, ENTROPY, grid_distances, ref_colsum, ref_rollout, ref_stats,
                            rollout_matrix, shifted_identity)


# ------------------------------------------------------------------------------------------ the references
@pytest.mark.parametrize("N,G", [(26, 5), (65, 8), (18, 4)])   # (18, 4): a ragged raster
def test_uniform_attention_closed_forms(N, G):
    P, unit = N - 1, 4.0
    p = torch.full((2, 3, N, N), 1.0 / N, dtype=torch.float64)
    s = ref_stats(p, G, unit)
    assert tuple(s.shape) == (2, 3, 4) and s.dtype == torch.float64
    dsum = sum(math.hypot((i // G) - (j // G), (i % G) - (j % G)) for i in range(P) for j in range(P))
    assert torch.allclose(s[..., DISTANCE], torch.tensor(unit * dsum / (P * N), dtype=torch.float64), rtol=1e-12)
    assert torch.allclose(s[..., ENTROPY], torch.tensor(math.log(N), dtype=torch.float64), rtol=1e-12)
    assert torch.allclose(s[..., CLS_MASS], torch.tensor(1.0 / N, dtype=torch.float64), rtol=1e-12)
    assert torch.allclose(s[..., CLS_ENTROPY], torch.tensor(math.log(N), dtype=torch.float64), rtol=1e-12)


def test_shifted_identity_gives_the_neighbour_distance():
    """N = 26 on a 5 x 5 grid, unit 1.  Key i + 1: of the patch queries 1 .. 24, twenty step one column to the right and
    four (tokens 5, 10, 15, 20) wrap to the start of the next row, sqrt(1 + 4^2) away; query 25 keeps itself.  Key i + 5:
    queries 1 .. 20 step one row down.  Key i - 1: query 1 lands on the class token, which has no distance but is the
    whole class mass."""
    N, G, P = 26, 5, 25
    right = ref_stats(shifted_identity(N, 1)[None, None], G)[0, 0]
    assert right[DISTANCE].item() == pytest.approx((20 + 4 * math.sqrt(17.0)) / P, rel=1e-12)
    assert right[ENTROPY].item() == 0.0 and right[CLS_MASS].item() == 0.0 and right[CLS_ENTROPY].item() == 0.0
    down = ref_stats(shifted_identity(N, G)[None, None], G, unit=4.0)[0, 0]
    assert down[DISTANCE].item() == pytest.approx(4.0 * 20 / P, rel=1e-12)
    left = ref_stats(shifted_identity(N, -1)[None, None], G)[0, 0]
    assert left[DISTANCE].item() == pytest.approx((20 + 4 * math.sqrt(17.0)) / P, rel=1e-12)   # queries 2 .. 25; 1 -> class token
    assert left[CLS_MASS].item() == pytest.approx(1.0 / P, rel=1e-12)
    # a transposed coordinate map would swap the two: one token on is one COLUMN on
    d = grid_distances(N, G)
    assert d[0, 1].item() == 1.0 and d[0, G].item() == 1.0 and d[0, G - 1].item() == G - 1 and d[G - 1, G].item() == math.sqrt(17.0)


def test_ref_colsum_and_rollout_are_the_explicit_products():
    g = torch.Generator().manual_seed(3)
    B, H, N, L = 2, 3, 10, 4
    maps = [torch.rand(B, H, N, N, generator=g, dtype=torch.float64).softmax(-1) for _ in range(L)]
    w = torch.rand(B, N, generator=g, dtype=torch.float64)
    want = torch.stack([torch.stack([w[b] @ maps[0][b, h] for h in range(H)]) for b in range(B)])
    assert float((ref_colsum(maps[0], w) - want).abs().max()) < 1e-12
    for start, residual in ((0, 0.5), (1, 0.5), (0, 0.0), (2, 0.9)):
        m = torch.eye(N, dtype=torch.float64).expand(B, N, N)
        for a in maps[start:]:                                  # A^_{L-1} ... A^_{start}
            m = rollout_matrix(a, residual) @ m
        r = ref_rollout(maps, start, residual)
        assert float((r - m[:, 0]).abs().max()) < 1e-12
        assert float((r.sum(-1) - 1.0).abs().max()) < 1e-12


# ------------------------------------------------------------------------------------------ header, library, constants
def test_library_exports_the_entry_point_and_the_header_declares_it():
    from vitpe import _lib
    protos = _lib.parse_header()
    assert "vitpe_attention_core_stats" in protos
    args = protos["vitpe_attention_core_stats"]
    # (dtype, qkv, stats, weights, colsum, unit, B, N, H, HD, mode, cos, sin, table, coeff, grid, degree, coeff_per_head, stream)
    assert len(args) == 19
    assert args[0] is ctypes.c_int and all(a is ctypes.c_void_p for a in args[1:5]) and args[5] is ctypes.c_float
    assert all(a is ctypes.c_int for a in args[6:11]) and args[18] is ctypes.c_void_p
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "vitpe_attention_core_stats")
    assert ctypes.CDLL(_lib.LIB_PATH).vitpe_abi_version() == 5   # entries are only added


def test_slot_names_agree_in_the_header_and_in_kernels():
    from vitpe import _lib
    from vitpe import kernels as K
    slots = dict(re.findall(r"#define\s+VITPE_STAT_(\w+)\s+(\d+)", open(_lib.HEADER_PATH).read()))
    assert sorted(slots) == ["CLS_ENTROPY", "CLS_MASS", "DISTANCE", "ENTROPY"]
    for name, value in slots.items():
        assert getattr(K, "STAT_" + name) == int(value), name
    assert (K.STAT_DISTANCE, K.STAT_ENTROPY, K.STAT_CLS_MASS, K.STAT_CLS_ENTROPY) == (DISTANCE, ENTROPY, CLS_MASS, CLS_ENTROPY)


# ------------------------------------------------------------------------------------------ refusals without a device
def test_host_wrapper_refuses_a_cpu_tensor():
    from vitpe import kernels as K
    from vitpe._lib import VitpeError
    with pytest.raises(VitpeError, match="no CPU fallback"):
        K.attention_core_stats(torch.zeros(1, 17, 3 * 64), 2, K.PETables("none", 4))
    with pytest.raises(VitpeError, match="no CPU fallback"):
        K.attention_core_stats(torch.zeros(1, 17, 3 * 64), 2, K.PETables("none", 4), unit=4.0, weights=torch.zeros(1, 17))


def test_argument_checks_come_before_any_device():
    """on CPU tensors the shape / dtype / grid errors are raised, not the device refusal that a valid call would get"""
    from vitpe import kernels as K
    from vitpe._lib import VitpeError
    qkv = torch.zeros(2, 17, 3 * 64)
    with pytest.raises(VitpeError, match="grid must be >= 1"):
        K.attention_core_stats(qkv, 2, K.PETables("none", 0))
    with pytest.raises(VitpeError, match="weights must be float32"):
        K.attention_core_stats(qkv, 2, K.PETables("none", 4), weights=torch.zeros(2, 16))
    with pytest.raises(VitpeError, match="weights must be float32"):
        K.attention_core_stats(qkv, 2, K.PETables("none", 4), weights=torch.zeros(2, 17, dtype=torch.float64))
    with pytest.raises(VitpeError, match="weights must be float32"):
        K.attention_core_stats(qkv, 2, K.PETables("none", 4), weights=torch.zeros(17, 2).t())   # not contiguous
    with pytest.raises(VitpeError, match="colsum output needs weights"):
        K.attention_core_stats(qkv, 2, K.PETables("none", 4), out=(torch.zeros(2, 2, 4), torch.zeros(2, 2, 17)))


def test_module_methods_refuse_a_cpu_tensor():
    from vitpe._lib import VitpeError
    from vitpe.vit import Attention, Block, VisionTransformer
    x = torch.zeros(1, 17, 64)
    with pytest.raises(VitpeError, match="no CPU fallback"):
        Attention(64, num_heads=2).attention_stats(x)
    with pytest.raises(VitpeError, match="no CPU fallback"):
        Block(64, 2).attention_stats(x, weights=torch.zeros(1, 17))
    model = VisionTransformer(img_size=16, patch_size=4, embed_dim=64, depth=2, num_heads=2, pos_encoding="relative")
    with pytest.raises(VitpeError, match="no CPU fallback"):
        model.attention_stats(torch.zeros(1, 3, 16, 16))
    with pytest.raises(VitpeError, match="no CPU fallback"):
        model.attention_rollout(torch.zeros(1, 3, 16, 16))
    assert model.training
