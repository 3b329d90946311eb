"""transforms.Resize on the host side: the coefficient tables of vitpe_resize_coeffs against the fixture's PIL-independent
tables (tests/golden/resize.npz, tools/make_golden.py --only resize), the fixture against itself and, where PIL imports,
against PIL directly; train.py accepts the geometries that need a resize.  Needs the built library, no GPU."""
import ctypes
import sys

import numpy as np
import pytest

from conftest import REPO

CASES = [("mnist", 28, S) for S in (14, 16, 32, 64, 224)] + [("cifar", 32, S) for S in (16, 24, 48, 64, 224)]


def apply_pass(planes, bounds, kk):
    """One pass of PIL's 8-bit resample along the last axis: clip((2^21 + sum_x in[xmin + x] * k[x]) >> 22, 0, 255)."""
    bounds, kk = np.asarray(bounds), np.asarray(kk).astype(np.int64)
    idx = np.minimum(bounds[:, :1] + np.arange(kk.shape[1])[None], planes.shape[-1] - 1)   # taps past n weigh 0
    acc = (planes[..., idx].astype(np.int64) * kk).sum(-1) + (1 << 21)
    return np.clip(acc >> 22, 0, 255).astype(np.uint8)


def apply_resize(x, bounds, kk):
    """[N,C,S0,S0] -> [N,C,S,S]: horizontal pass to a uint8 intermediate, then the vertical pass."""
    mid = apply_pass(x, bounds, kk)
    return apply_pass(mid.transpose(0, 1, 3, 2), bounds, kk).transpose(0, 1, 3, 2)


@pytest.mark.parametrize("name,S0,S", CASES)
def test_resize_coeffs_equal_the_fixture(golden, name, S0, S):
    from vitpe import kernels as K
    g = golden("resize")
    bounds, kk = K.resize_coeffs(S0, S)
    assert bounds.dtype == kk.dtype and bounds.numpy().dtype == np.int32
    assert np.array_equal(bounds.numpy(), g[f"{name}/{S}/bounds"])
    assert np.array_equal(kk.numpy(), g[f"{name}/{S}/kk"])
    assert kk.shape[1] == (3 if S >= S0 else 2 * -(-S0 // S) + 1)
    # every output's weights sum to 2^22 up to the rounding of each tap
    assert int(np.abs(kk.numpy().astype(np.int64).sum(1) - (1 << 22)).max()) <= kk.shape[1]


def test_resize_coeffs_refuses_a_small_ksize_cap():
    from vitpe import _lib
    h = _lib.lib()
    for S0, S, ksize in ((32, 64, 3), (28, 14, 5), (64, 4, 33)):
        bounds = np.full((S, 2), -7, dtype=np.int32)
        kk = np.full((S, ksize), -7, dtype=np.int32)
        args = (S0, S, bounds.ctypes.data_as(ctypes.c_void_p), kk.ctypes.data_as(ctypes.c_void_p))
        assert h.vitpe_resize_coeffs(*args, ksize - 1) < 0
        assert (bounds == -7).all() and (kk == -7).all()          # refused: nothing written
        assert h.vitpe_resize_coeffs(*args, ksize) == ksize
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds.sum(1) <= S0).all()
    assert h.vitpe_resize_coeffs(0, 8, None, None, 3) < 0


def test_resize_support_range():
    from vitpe import kernels as K
    assert all(K.resize_u8_supported(a, b) for a in (8, 28, 32, 64) for b in (4, 16, 224, 512))
    assert not any(K.resize_u8_supported(a, b) for a, b in ((128, 64), (32, 1024), (4, 32), (32, 2), (0, 0)))


@pytest.mark.parametrize("name,S0,S", CASES)
def test_fixture_outputs_follow_from_its_coefficients(golden, name, S0, S):
    g = golden("resize")
    x, y = g[f"{name}/{S}/x"], g[f"{name}/{S}/y"]
    assert x.dtype == np.uint8 and y.dtype == np.uint8
    assert x.shape == (2 if S == 224 else 4, 3 if name == "cifar" else 1, S0, S0) and y.shape == x.shape[:2] + (S, S)
    assert np.array_equal(apply_resize(x, g[f"{name}/{S}/bounds"], g[f"{name}/{S}/kk"]), y)


@pytest.mark.parametrize("name,S0,S", CASES)
def test_fixture_and_library_coefficients_against_pil(golden, name, S0, S):
    Image = pytest.importorskip("PIL.Image")
    from vitpe import kernels as K
    g = golden("resize")
    x, y = g[f"{name}/{S}/x"], g[f"{name}/{S}/y"]
    pil = np.zeros_like(y)
    for i in range(x.shape[0]):
        if x.shape[1] == 1:
            pil[i, 0] = np.asarray(Image.fromarray(x[i, 0], "L").resize((S, S), Image.BILINEAR))
        else:
            hwc = np.ascontiguousarray(x[i].transpose(1, 2, 0))
            pil[i] = np.asarray(Image.fromarray(hwc, "RGB").resize((S, S), Image.BILINEAR)).transpose(2, 0, 1)
    assert np.array_equal(pil, y)
    bounds, kk = K.resize_coeffs(S0, S)
    assert np.array_equal(apply_resize(x, bounds.numpy(), kk.numpy()), pil)


def test_train_py_accepts_the_resize_geometries():
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    import train as T
    for dataset in ("cifar10", "mnist"):
        for geom in (["--img_size", "64"], ["--img_size", "64", "--patch_size", "8"],
                     ["--img_size", "224", "--patch_size", "16"], ["--img_size", "48"],
                     ["--img_size", "16", "--patch_size", "4"],
                     ["--img_size", "224", "--patch_size", "16", "--embed_dim", "768", "--num_heads", "12"]):
            args = T.get_args(["--dataset", dataset] + geom)
            assert args.img_size == int(geom[1]) and not args.synthetic
