"""Random crop + horizontal flip on the resident dataset -- what can be checked without a GPU: the numpy restatement of the
augmentation stream against the host build of the Philox generator, the distribution of the documented draws, the
argument checks that run before anything touches a device, the CLI flags and the rank shift of the engine's pair."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_ref as A  # noqa: E402

from vitpe import _lib  # noqa: E402
from vitpe._lib import VitpeError  # noqa: E402


def _philox(key, ctr):
    k, c, o = (ctypes.c_uint * 2)(*key), (ctypes.c_uint * 4)(*ctr), (ctypes.c_uint * 4)()
    vp = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
    assert _lib.lib().vitpe_philox4x32_10(vp(k), vp(c), vp(o)) == 0
    return [int(v) for v in o]


@pytest.mark.parametrize("rng", [(0xFEDCBA9876543210, (1 << 32) + 5), (0x8000000000000001, 0xC000000000000007), (3, 0)])
@pytest.mark.parametrize("pad,hflip", [(0, False), (1, True), (4, True), (4, False), (32, True)])
def test_params_match_the_host_philox(rng, pad, hflip):
    """One Philox call per slot: key = the seed's halves, counter = (b, 0, the offset's halves); seeds and offsets with bits
    set above bit 31."""
    seed, off = rng
    B = 41
    got = A.params(rng, B, pad, hflip)
    assert got.shape == (B, 3)
    for b in range(B):
        w = _philox([seed & 0xFFFFFFFF, seed >> 32], [b, 0, off & 0xFFFFFFFF, off >> 32])
        want = [(w[0] * (2 * pad + 1)) >> 32, (w[1] * (2 * pad + 1)) >> 32, (w[2] >> 31) if hflip else 0]
        assert [int(v) for v in got[b]] == want
    assert got[:, :2].min() >= 0 and got[:, :2].max() <= 2 * pad


def test_distribution_of_the_draws():
    """pad = 4 over 4096 slots of one fixed pair: every offset 0..8 occurs in oy and in ox, and the flip share is within
    0.5 +- 0.05 (6 sigma of the binomial: sigma = sqrt(0.25 / 4096) = 0.0078)."""
    prm = A.params((0x1234567890ABCDEF, (1 << 40) + 17), 4096, 4, True)
    assert set(prm[:, 0].tolist()) == set(range(9))
    assert set(prm[:, 1].tolist()) == set(range(9))
    assert abs(prm[:, 2].mean() - 0.5) <= 0.05, prm[:, 2].mean()
    assert not np.array_equal(prm[:, 0], prm[:, 1])
    assert A.params((0x1234567890ABCDEF, (1 << 40) + 17), 4096, 4, False)[:, 2].sum() == 0


def test_reference_images_pad_with_the_zero_byte():
    """The restatement itself: pad = 0 without a flip is ToTensor + Normalize; a slot whose window lies in the padding reads
    (0 - mean) / std; a flip mirrors the columns."""
    g = np.random.default_rng(3)
    data = g.integers(0, 256, size=(4, 1, 8, 8), dtype=np.uint8)
    mean, std = (0.1307,), (0.3081,)
    plain = ((data.astype(np.float32) / np.float32(255)) - np.float32(mean[0])) / np.float32(std[0])
    assert np.array_equal(A.images(data, None, mean, std, (5, 6), 0, False), plain)
    rng = (77, 1 << 33)
    prm = A.params(rng, 4, 8, True)
    img = A.images(data, [2, 2, 0, 1], mean, std, rng, 8, True)
    zero = (np.float32(0) - np.float32(mean[0])) / np.float32(std[0])
    for b, rec in enumerate([2, 2, 0, 1]):
        oy, ox, flip = (int(v) for v in prm[b])
        for y, x in ((0, 0), (7, 7), (3, 5)):
            sy, sx = y + oy - 8, (7 - x if flip else x) + ox - 8
            want = plain[rec, 0, sy, sx] if 0 <= sy < 8 and 0 <= sx < 8 else zero
            assert img[b, 0, y, x] == want
    assert np.array_equal(A.unfold(plain, 4)[1, :4], plain[0, 0, 0, 4:8])     # patch (0, 1), row ky = 0


def _cpu_dataset(S=8):
    from vitpe.data import ResidentDataset
    return ResidentDataset(torch.zeros(4, 1, S, S, dtype=torch.uint8), torch.zeros(4, dtype=torch.int64), (0.5,), (0.5,), "cpu")


@pytest.mark.parametrize("rng,pad,word", [(torch.zeros(2, dtype=torch.int64), 0, "device"),          # a CPU pair
                                          (torch.zeros(2, dtype=torch.int32), 0, "int64"),           # wrong dtype
                                          (torch.zeros(3, dtype=torch.int64), 0, "two words"),
                                          (torch.zeros(2, dtype=torch.int64), 9, "crop_pad"),        # > S = 8
                                          (torch.zeros(2, dtype=torch.int64), -1, "crop_pad")])
def test_argument_checks_come_before_the_device(rng, pad, word):
    from vitpe import data as D
    from vitpe import kernels as K
    ds = _cpu_dataset()
    w = torch.zeros(16, 16)
    calls = (lambda: K.unfold_u8(ds.images, None, ds.mean, ds.std, 4, torch.float32, rng=rng, crop_pad=pad, hflip=True),
             lambda: K.patch_embed(w, w[0], w[0], None, 4, torch.float32, data=ds.images, mean=ds.mean, std=ds.std, rng=rng,
                                   crop_pad=pad),
             lambda: D.augment_batch(ds, None, rng, crop_pad=pad, hflip=True))
    for call in calls:
        with pytest.raises(VitpeError) as e:
            call()
        assert word in str(e.value), str(e.value)


def test_patch_embed_refuses_rng_with_fp32_images():
    from vitpe import kernels as K
    w = torch.zeros(16, 16)
    with pytest.raises(VitpeError) as e:
        K.patch_embed(w, w[0], w[0], None, 4, torch.float32, images=torch.zeros(1, 1, 8, 8), rng=torch.zeros(2, dtype=torch.int64))
    assert "augment_batch" in str(e.value)


def test_train_py_parses_and_refuses_the_flags():
    sys.path.insert(0, _lib.REPO_ROOT)
    import train
    args = train.get_args(["--random_crop", "4", "--hflip"])
    assert args.random_crop == 4 and args.hflip is True
    assert train.augment_refusal(args) is None
    off = train.get_args([])
    assert off.random_crop == 0 and off.hflip is False and train.augment_refusal(off) is None
    for flags in (["--random_crop", "4"], ["--hflip"], ["--random_crop", "4", "--hflip"]):
        with pytest.raises(SystemExit) as e:
            train.main(flags + ["--synthetic"])
        for f in flags:
            if f.startswith("--"):
                assert f in str(e.value)
        assert "--synthetic" in str(e.value)
    with pytest.raises(SystemExit):
        train.get_args(["--random_crop", "33"])            # > --img_size
    with pytest.raises(SystemExit):
        train.get_args(["--random_crop", "-1"])


def test_rank_shift_of_the_engine_pair():
    """Ranks that drew the same pair (same torch seed) differ by rank << 48 on the offset only."""
    from vitpe.engine import new_augment_rng
    pairs = []
    for rank in (0, 1, 5, 0xFFFF):
        torch.manual_seed(1234)
        pairs.append(new_augment_rng("cpu", rank))
    base = pairs[0]
    assert base.shape == (1, 2) and base.dtype == torch.int64
    for rank, pr in zip((1, 5, 0xFFFF), pairs[1:]):
        assert int(pr[0, 0]) == int(base[0, 0])
        assert (int(pr[0, 1]) - int(base[0, 1])) % (1 << 64) == (rank << 48) % (1 << 64)
