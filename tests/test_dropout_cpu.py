"""Dropout, stochastic depth and qkv bias -- what can be checked without a GPU: the host build of the Philox generator
against a numpy restatement and the published known answers, the statistics of the documented stream, and the Python
surface (constructors, state_dict keys, the TrainEngine / train.py refusals)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dropout_stream as S  # noqa: E402

from vitpe import _lib  # noqa: E402


def _philox(key, ctr):
    k, c, o = (ctypes.c_uint * 2)(*key), (ctypes.c_uint * 4)(*ctr), (ctypes.c_uint * 4)()
    vp = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
    assert _lib.lib().vitpe_philox4x32_10(vp(k), vp(c), vp(o)) == 0
    return [int(v) for v in o]


# Random123's known-answer vectors for philox4x32-10 (kat_vectors of the Random123 distribution): counter, key -> output
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    assert tuple(_philox(key, ctr)) == want
    assert tuple(int(v) for v in S.philox4x32_10(key, ctr)) == want


def test_philox_matches_numpy_restatement():
    g = np.random.default_rng(20240611)
    keys = g.integers(0, 2 ** 32, size=(3000, 2), dtype=np.uint64)
    ctrs = g.integers(0, 2 ** 32, size=(3000, 4), dtype=np.uint64)
    want = S.philox4x32_10(keys, ctrs)
    for k, c, w in zip(keys, ctrs, want):
        assert _philox([int(v) for v in k], [int(v) for v in c]) == [int(v) for v in w]


def test_null_pointers_are_invalid_value():
    assert _lib.lib().vitpe_philox4x32_10(None, None, None) == 1


@pytest.mark.parametrize("p,rng", [(0.1, (0x1234567890ABCDEF, 7)), (0.5, (42, 0xFEDCBA9876543210))])
def test_stream_keeps_one_minus_p(p, rng):
    """n = 2^20 decisions keep n (1 - p) within 5 sigma of the binomial (a condition on the definition itself)."""
    n = 1 << 20
    kept = int(S.mask_elements(rng, n, p).sum())
    sigma = (n * p * (1 - p)) ** 0.5
    assert abs(kept - n * (1 - p)) <= 5 * sigma, (kept, n * (1 - p), sigma)


def test_stream_is_a_function_of_the_element_only():
    """The same element gives the same decision whatever else is asked for with it (no dependence on batch shape)."""
    rng, p = (99, 3), 0.3
    full = S.mask_elements(rng, 1000, p)
    idx = np.array([999, 5, 4, 123], dtype=np.uint64)
    assert np.array_equal(S.keep(rng, idx, p), full[idx.astype(np.int64)])
    a = S.mask_attention(rng, 2, 3, 17, p)
    assert a.shape == (2, 3, 17, 17)
    assert not np.array_equal(a, S.mask_attention((99, 4), 2, 3, 17, p))      # another offset: another mask
    assert np.array_equal(a[:1], S.mask_attention(rng, 1, 3, 17, p))         # leading images do not depend on B


def test_numpy_masks_reproduce_the_fixture(golden):
    """dropout.npz (tools/make_golden.py gen_dropout) stores the pairs and the packed bits of every mask the reference's
    arithmetic was run under: the restated stream gives them back bit for bit.  The generator took those bits from this same
    restatement (dropout_stream.py), so this test pins the restatement against DRIFT, not against an error in it: that it is
    right rests on the Random123 known-answer vectors above and on the device masks, produced from the HIP source, matching
    it bit for bit (test_dropout_gpu.py::test_masks_are_the_documented_stream)."""
    g = golden("dropout")
    for tag, N, B in (("rope-axial", 17, 3), ("relative", 17, 3), ("rope-axial", 65, 2), ("relative", 65, 2)):
        key = f"attn/{tag}/n{N}"
        pairs = [tuple(int(v) for v in r) for r in g[f"{key}/pairs"]]
        assert np.array_equal(np.packbits(S.mask_attention(pairs[0], B, 3, N, 0.1)), g[f"{key}/mask_attn"])
        assert np.array_equal(np.packbits(S.mask_elements(pairs[1], B * N * 96, 0.2)), g[f"{key}/mask_proj"])
    pairs = [tuple(int(v) for v in r) for r in g["block/pairs"]]
    B, N = 4, 17
    assert np.array_equal(np.packbits(S.mask_attention(pairs[0], B, 3, N, 0.15)), g["block/mask_attn"])
    for k, name, n in ((1, "proj", B * N * 96), (2, "drop1", B * N * 384), (3, "drop2", B * N * 96)):
        assert np.array_equal(np.packbits(S.mask_elements(pairs[k], n, 0.1)), g[f"block/mask_{name}"])
    for k, name in ((4, "path_attn"), (5, "path_mlp")):
        assert np.array_equal(np.packbits(S.mask_elements(pairs[k], B, 0.3)), g[f"block/mask_{name}"])


def test_threshold_and_scale():
    assert int(S.threshold(0.0)) == 0 and int(S.threshold(0.5)) == 1 << 31
    assert int(S.threshold(np.nextafter(np.float32(1), np.float32(0)))) < 2 ** 32
    assert S.scale(0.5) == np.float32(2.0)


def test_constructors_accept_the_arguments():
    from models.vit import Attention, Block, Mlp, VisionTransformer
    a = Attention(96, num_heads=3, qkv_bias=True, attn_drop=0.1, proj_drop=0.2)
    assert a.qkv.bias is not None and a.qkv.bias.shape == (288,)
    assert (a.attn_drop_p, a.proj_drop_p) == (0.1, 0.2)
    m = Mlp(96, 384, drop=0.1)
    assert m.drop == 0.1
    b = Block(96, 3, qkv_bias=True, drop=0.1, attn_drop=0.2, drop_path=0.3)
    assert b.drop_path_p == 0.3 and b.attn.attn_drop_p == 0.2 and b.attn.proj_drop_p == 0.1 and b.mlp.drop == 0.1
    v = VisionTransformer(img_size=32, patch_size=8, embed_dim=96, depth=4, num_heads=3, pos_encoding="rope-axial",
                          qkv_bias=True, drop_rate=0.1, attn_drop_rate=0.1, drop_path_rate=0.3)
    rates = [blk.drop_path_p for blk in v.blocks]
    assert rates[0] == 0.0 and rates[-1] == pytest.approx(0.3) and rates == sorted(rates)
    assert rates[1] == pytest.approx(0.1)                     # linear in the depth
    for name, bad in (("attn_drop", -0.1), ("proj_drop", 1.0)):
        with pytest.raises(ValueError):
            Attention(96, 3, **{name: bad})
    with pytest.raises(NotImplementedError):
        Block(96, 3, norm_layer=nn.BatchNorm1d)              # still refused
    with pytest.raises(TypeError):
        VisionTransformer(32, 8, 3, 10, 96, 2, 3, 4., "none", 100.0, 3, True, True)   # the extras are keyword-only


def test_state_dict_keys_with_qkv_bias():
    from models.vit import VisionTransformer
    plain = VisionTransformer(img_size=32, patch_size=8, embed_dim=96, depth=2, num_heads=3, pos_encoding="relative")
    v = VisionTransformer(img_size=32, patch_size=8, embed_dim=96, depth=2, num_heads=3, pos_encoding="relative",
                          qkv_bias=True, drop_rate=0.1, attn_drop_rate=0.1, drop_path_rate=0.1)
    extra = set(v.state_dict()) - set(plain.state_dict())
    assert extra == {"blocks.0.attn.qkv.bias", "blocks.1.attn.qkv.bias"}        # dropout adds no state
    assert set(plain.state_dict()) <= set(v.state_dict())
    for i in range(2):
        assert torch.count_nonzero(v.state_dict()[f"blocks.{i}.attn.qkv.bias"]) == 0   # _init_weights: zero


def test_train_engine_refuses_before_touching_a_device():
    from models.vit import VisionTransformer
    from vitpe.engine import TrainEngine, engine_unsupported
    v = VisionTransformer(img_size=32, patch_size=4, embed_dim=192, depth=2, num_heads=6, pos_encoding="rope-mixed",
                          qkv_bias=True, attn_drop_rate=0.1, drop_path_rate=0.2)
    assert engine_unsupported(v) == ["attn_drop", "drop_path", "qkv_bias"]
    with pytest.raises(NotImplementedError) as e:
        TrainEngine(v, 8)
    for name in ("qkv_bias", "attn_drop", "drop_path"):
        assert name in str(e.value)
    plain = VisionTransformer(img_size=32, patch_size=4, embed_dim=192, depth=2, num_heads=6)
    assert engine_unsupported(plain) == []


def test_train_py_parses_and_refuses_the_flags():
    sys.path.insert(0, _lib.REPO_ROOT)
    import train
    args = train.get_args(["--qkv_bias", "--drop", "0.1", "--attn_drop", "0.05", "--drop_path", "0.2"])
    assert args.qkv_bias is True and (args.drop, args.attn_drop, args.drop_path) == (0.1, 0.05, 0.2)
    msg = train.engine_refusal(args)
    for flag in ("--qkv_bias", "--drop", "--attn_drop", "--drop_path"):
        assert flag in msg
    with pytest.raises(SystemExit) as e:
        train.main(["--drop_path", "0.2"])
    assert "--drop_path" in str(e.value)
    off = train.get_args([])
    assert off.qkv_bias is False and (off.drop, off.attn_drop, off.drop_path) == (0.0, 0.0, 0.0)
    assert train.engine_refusal(off) is None
    with pytest.raises(SystemExit):
        train.get_args(["--drop", "1.0"])
