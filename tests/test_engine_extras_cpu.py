"""The opt-in engine route for qkv bias / dropout / stochastic depth -- what can be checked without a GPU: the train.py flag,
the two refusals (with and without the opt-in), the site-table constants, the rank shift of the offsets and the new C
symbols."""
import ctypes
import sys

import pytest
import torch

from vitpe import _lib

FLAGS = ["--qkv_bias", "--drop", "0.1", "--attn_drop", "0.05", "--drop_path", "0.2"]


def _train():
    sys.path.insert(0, _lib.REPO_ROOT)
    import train
    return train


def test_train_py_flag_lifts_the_refusal():
    train = _train()
    args = train.get_args(FLAGS + ["--engine_extras"])
    assert args.engine_extras is True and args.qkv_bias is True and (args.drop, args.attn_drop, args.drop_path) == (0.1, 0.05, 0.2)
    assert train.engine_refusal(args) is None
    off = train.get_args(FLAGS)
    assert off.engine_extras is False
    msg = train.engine_refusal(off)
    for flag in ("--qkv_bias", "--drop", "--attn_drop", "--drop_path", "--engine_extras"):
        assert flag in msg
    assert train.engine_refusal(train.get_args(["--engine_extras"])) is None
    assert train.engine_refusal(train.get_args([])) is None


def _model(**kw):
    from models.vit import VisionTransformer
    return VisionTransformer(img_size=32, patch_size=8, embed_dim=96, depth=2, num_heads=3, pos_encoding="rope-mixed", **kw)


def test_engine_keyword_moves_the_refusal_to_the_device_check():
    from vitpe.engine import TrainEngine
    v = _model(qkv_bias=True, drop_rate=0.1, attn_drop_rate=0.1, drop_path_rate=0.2)
    with pytest.raises(_lib.VitpeError, match="HIP device"):       # options accepted: what stops it is the CPU model
        TrainEngine(v, 8, extras=True)
    with pytest.raises(NotImplementedError) as e:
        TrainEngine(v, 8)
    for name in ("qkv_bias", "attn_drop", "drop", "drop_path", "extras=True"):
        assert name in str(e.value)
    with pytest.raises(NotImplementedError):
        TrainEngine(v, 8, extras=False)
    with pytest.raises(_lib.VitpeError, match="HIP device"):       # a plain model is accepted on the route as well
        TrainEngine(_model(), 8, extras=True)


def test_rank_shift_of_the_offsets():
    from vitpe.engine import shift_rng_offsets
    g = torch.Generator().manual_seed(3)
    t = torch.randint(-2 ** 62, 2 ** 62, (12, 2), generator=g, dtype=torch.int64)
    t[0, 1] = -1                                                  # 2^64 - 1: the shift wraps
    out = {r: shift_rng_offsets(t, r) for r in (0, 1, 7)}
    assert torch.equal(out[0], t) and out[0] is not t
    u64 = lambda v: int(v) & (2 ** 64 - 1)  # noqa: E731
    for r, o in out.items():
        assert torch.equal(o[:, 0], t[:, 0])                      # seeds alone
        for i in range(12):
            assert u64(o[i, 1]) == (u64(t[i, 1]) + (r << 48)) % 2 ** 64
    for a, b in ((0, 1), (0, 7), (1, 7)):
        assert not (out[a][:, 1] == out[b][:, 1]).any()
    big = shift_rng_offsets(t, 40000)                             # rank << 48 above 2^63
    assert u64(big[3, 1]) == (u64(t[3, 1]) + (40000 << 48)) % 2 ** 64


def test_site_constants():
    from vitpe import engine as E
    sites = [E.SITE_ATTN, E.SITE_PROJ, E.SITE_MLP1, E.SITE_MLP2, E.SITE_PATH_A, E.SITE_PATH_M]
    assert sites == [0, 1, 2, 3, 4, 5] and E.SITES_PER_LAYER == 6
    rows = [E.site_row(l, k) for l in range(3) for k in sites]
    assert rows == list(range(18))
    assert E.site_row(2, E.SITE_MLP2) == 6 * 2 + 3


def test_new_symbols_in_header_and_library():
    protos = _lib.parse_header()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("vitpe_branch_drop_fwd", 11), ("vitpe_branch_drop_bwd", 10), ("vitpe_rng_advance", 4)):
        assert name in protos and len(protos[name]) == nargs
        assert hasattr(handle, name)
    assert protos["vitpe_rng_advance"][2] is ctypes.c_ulonglong
    # pure host argument checks: refused before anything touches a device
    h = _lib.lib()
    assert h.vitpe_branch_drop_fwd(0, None, None, None, 4, 16, None, 0.1, None, 0.1, None) == 1
    assert h.vitpe_rng_advance(None, 0, 1, None) == 0 and h.vitpe_rng_advance(None, 1, 1, None) == 1
