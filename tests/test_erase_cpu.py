"""RandomErasing in the embed gather -- what can be checked without a GPU: the host build of the erasing stream's draws
(vitpe_erase_params_host, the VITPE_HD function the kernels run) against the float64 restatement in erase_ref.py, the
distribution of the draws, the untouched crop/flip stream and the argument checks that run before anything touches a
device.  The reference's borderline slots (erase_ref.py: a side length within 1e-3 of a rounding boundary) are
left out of the exact comparisons, and every test says how many there are."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_ref as A  # noqa: E402
import dropout_stream as DS  # noqa: E402
import erase_ref as E  # noqa: E402

from vitpe import _lib  # noqa: E402
from vitpe._lib import VitpeError  # noqa: E402

SEED = 0xFEDCBA9876543210
OFFSET = (1 << 32) + 5
RNG = (SEED, OFFSET)
RETRY_SCALE = (0.3, 0.95)


@pytest.fixture(scope="module")
def K():
    from vitpe import kernels
    return kernels


def _host(K, B, S, prob, scale=E.SCALE, ratio=E.RATIO, rng=RNG):
    got = K.erase_params(rng, B, S, prob, scale, ratio, host=True)
    assert got.dtype == torch.int32 and tuple(got.shape) == (B, 5) and not got.is_cuda
    return got.numpy().astype(np.int64)


def _inside(prm, S):
    on = prm[:, 0] == 1
    i, j, h, w = (prm[on, k] for k in range(1, 5))
    assert (i >= 0).all() and (j >= 0).all() and (h < S).all() and (w < S).all()
    assert (i + h <= S).all() and (j + w <= S).all()
    assert (prm[~on] == 0).all()


def test_host_draws_equal_the_reference_at_32(K):
    """B = 4096, S = 32, prob 0.5, default scale and ratio: 11 borderline slots (0.27 %), at most 1 % allowed; exact on the
    others; the erased share within 6 sigma of prob (sigma = sqrt(0.25 / 4096) = 0.0078)."""
    B, S, prob = 4096, 32, 0.5
    want, border, attempts = E.params(RNG, B, S, prob)
    got = _host(K, B, S, prob)
    print(f"borderline slots: {int(border.sum())} of {B}")
    assert border.sum() <= 0.01 * B
    assert np.array_equal(got[~border], want[~border])
    _inside(got, S)
    assert abs(got[:, 0].mean() - prob) <= 6 * np.sqrt(prob * (1 - prob) / B), got[:, 0].mean()
    assert set(np.unique(attempts).tolist()) >= {-1, 0}
    # the same pair through a CPU tensor of two int64 words
    signed = [v - (1 << 64) if v >= (1 << 63) else v for v in RNG]
    assert np.array_equal(K.erase_params(torch.tensor(signed), 64, S, prob, host=True).numpy(), got[:64])


def test_host_draws_retry_up_to_ten_times(K):
    """S = 16, scale (0.3, 0.95), B = 512, every slot switched on: the reference accepts at every attempt index 0..9 and four
    slots exhaust all ten attempts (nothing erased, torchvision's behaviour)."""
    B, S = 512, 16
    want, border, attempts = E.params(RNG, B, S, 1.0, RETRY_SCALE)
    assert set(attempts.tolist()) == set(range(E.ATTEMPTS + 1)) and (attempts == E.ATTEMPTS).sum() == 4
    assert (want[attempts == E.ATTEMPTS] == 0).all()
    print(f"borderline slots: {int(border.sum())} of {B}")
    assert border.sum() <= 0.01 * B
    got = _host(K, B, S, 1.0, RETRY_SCALE)
    assert np.array_equal(got[~border], want[~border])
    _inside(got, S)
    assert got[:, 0].sum() == B - 4 or border.any()


@pytest.mark.parametrize("S", [32, 16, 8])
def test_prob_zero_erases_none_and_one_erases_all(K, S):
    B = 256
    assert (_host(K, B, S, 0.0) == 0).all()
    allon = _host(K, B, S, 1.0)
    want, border, _ = E.params(RNG, B, S, 1.0)
    assert (want[:, 0] == 1).all() and border.sum() <= 0.01 * B      # (default scale: no slot runs out of attempts)
    assert np.array_equal(allon[~border], want[~border]) and (allon[:, 0] == 1).all()
    _inside(allon, S)
    # the switch is the documented threshold on w3 of the crop/flip call
    w3 = DS.words(RNG, np.uint64(4) * np.arange(B, dtype=np.uint64) + np.uint64(3)).astype(np.uint64)
    for prob in (0.25, 0.5, 0.999):
        assert np.array_equal(_host(K, B, S, prob)[:, 0] == 1, w3 < np.uint64(E.threshold(prob)))


def test_the_switch_is_the_fourth_word_of_the_crop_flip_call():
    """The crop and flip draws of augment_ref.params read words 0..2 of the call (b, 0); the switch reads word 3 of the same
    call, the attempts and fills other calls: erasing cannot move a crop or a flip."""
    B = 64
    first = E.calls(RNG, np.arange(B, dtype=np.uint64), np.zeros(B, dtype=np.uint64)).astype(np.uint64)
    prm = A.params(RNG, B, 4, True)
    assert np.array_equal(prm[:, 0], (first[:, 0] * np.uint64(9)) >> np.uint64(32))
    assert np.array_equal(prm[:, 1], (first[:, 1] * np.uint64(9)) >> np.uint64(32))
    assert np.array_equal(prm[:, 2], first[:, 2] >> np.uint64(31))
    on = E.params(RNG, B, 32, 0.5)[0][:, 0]
    assert np.array_equal(on == 1, first[:, 3] < np.uint64(1 << 31))
    # and the reference images outside the rectangles are augment_ref's, bit for bit
    data = np.random.default_rng(1).integers(0, 256, size=(6, 3, 32, 32), dtype=np.uint8)
    stats = ((0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010))
    base = A.images(data, None, *stats, RNG, 4, True)
    for mode in ("const", "rand", "pixel"):
        img, mask, prm, _ = E.images(data, None, *stats, RNG, 4, True, 0.5, mode)
        m = np.broadcast_to(mask[:, None], img.shape)
        assert prm[:, 0].min() == 0 and prm[:, 0].max() == 1
        assert np.array_equal(img[~m].astype(np.float32).view(np.uint32), base[~m].view(np.uint32))
        assert np.isfinite(img).all()
        if mode == "const":
            assert (img[m] == 0).all()


def test_reference_normals_look_normal():
    """Box-Muller on the documented uniforms: 4 x 16384 values with mean 0 +- 6 / sqrt(n) and variance 1 +- 6 sqrt(2 / n)."""
    n = 16384
    z = E.normals(E.calls(RNG, np.arange(n, dtype=np.uint64), np.full(n, 11, dtype=np.uint64)))
    assert z.shape == (n, 4) and np.isfinite(z).all()
    assert abs(z.mean()) <= 6 / np.sqrt(4 * n) and abs(z.var() - 1) <= 6 * np.sqrt(2 / (4 * n))
    u = E.uniform(np.array([0, 0xFFFFFFFF], dtype=np.uint32))
    assert 0 < u[0] < u[1] < 1 and u[0] == np.float32(u[0]) and u[1] == np.float32(u[1])      # exact in fp32, inside (0, 1)


def _cpu_dataset(C=1, S=8):
    from vitpe.data import ResidentDataset
    return ResidentDataset(torch.zeros(4, C, S, S, dtype=torch.uint8), torch.zeros(4, dtype=torch.int64), (0.5,) * C,
                           (0.5,) * C, "cpu")


BAD = [(dict(erase_prob=-0.1), "erase_prob"), (dict(erase_prob=1.5), "erase_prob"), (dict(erase_prob=float("nan")), "erase_prob"),
       (dict(erase_prob=0.5, erase_mode="noise"), "erase_mode"),
       (dict(erase_prob=0.5, erase_scale=(0.0, 0.3)), "erase_scale"), (dict(erase_prob=0.5, erase_scale=(0.4, 0.3)), "erase_scale"),
       (dict(erase_prob=0.5, erase_scale=(0.4, 1.1)), "erase_scale"),
       (dict(erase_prob=0.5, erase_ratio=(0.0, 3.3)), "erase_ratio"), (dict(erase_prob=0.5, erase_ratio=(3.3, 0.3)), "erase_ratio"),
       (dict(erase_prob=0.0, erase_ratio=(-1.0, 0.3)), "erase_ratio")]       # checked even where the switch is off


@pytest.mark.parametrize("kw,word", BAD)
def test_argument_checks_come_before_the_device(K, kw, word):
    """Every tensor here lives on the CPU: a call that reached the device check would fail with another message."""
    from vitpe import data as D
    ds = _cpu_dataset()
    rng = torch.zeros(2, dtype=torch.int64)
    calls = (lambda: K.unfold_u8(ds.images, None, ds.mean, ds.std, 4, torch.float32, rng=rng, **kw),
             lambda: D.augment_batch(ds, None, rng, **kw))
    for call in calls:
        with pytest.raises(VitpeError) as e:
            call()
        assert word in str(e.value), str(e.value)
    prob, scale, ratio = kw.get("erase_prob", 0.5), kw.get("erase_scale", E.SCALE), kw.get("erase_ratio", E.RATIO)
    if "erase_mode" not in kw:
        with pytest.raises(VitpeError) as e:
            K.erase_params(rng, 4, 8, prob, scale, ratio)
        assert word in str(e.value)


def test_more_argument_checks(K):
    ds5 = _cpu_dataset(C=5)
    rng = torch.zeros(2, dtype=torch.int64)
    for mode in ("rand", "pixel"):                  # one call gives four normals: C <= 4
        with pytest.raises(VitpeError) as e:
            K.unfold_u8(ds5.images, None, ds5.mean, ds5.std, 4, torch.float32, rng=rng, erase_prob=0.5, erase_mode=mode)
        assert "4 channels" in str(e.value)
    ds = _cpu_dataset()
    with pytest.raises(VitpeError) as e:            # erasing needs the pair
        K.unfold_u8(ds.images, None, ds.mean, ds.std, 4, torch.float32, erase_prob=0.5)
    assert "needs rng" in str(e.value)
    with pytest.raises(VitpeError) as e:            # valid erasing arguments: the next stop is the device check
        K.unfold_u8(ds.images, None, ds.mean, ds.std, 4, torch.float32, rng=rng, erase_prob=0.5)
    assert "device" in str(e.value)
    lib = _lib.lib()                                # the C entry's own checks (host entry: nothing to launch)
    pair = torch.tensor([1, 2], dtype=torch.int64)
    out = torch.zeros(4, 5, dtype=torch.int32)
    ok = (pair.data_ptr(), out.data_ptr(), 4, 8, 1 << 31, 0.02, 0.33, -1.0, 1.0)
    assert lib.vitpe_erase_params_host(*ok) == 0
    for k, v in ((4, (1 << 32) + 1), (5, 0.0), (5, 0.5), (6, 1.5), (7, 2.0), (7, float("nan")), (8, float("inf")), (3, 0)):
        bad = list(ok)
        bad[k] = v
        assert lib.vitpe_erase_params_host(*bad) == 1, (k, v)
    assert lib.vitpe_abi_version() == 5
