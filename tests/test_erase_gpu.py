"""RandomErasing in the uint8 gather ("Erasing stream"): the draws, vitpe_unfold_u8_erase in every fill mode and
data.augment_batch against the float64 restatement in erase_ref.py.  `const` mode and everything outside a rectangle is
bit-exact; the normals of `rand` and `pixel` are within 1e-4 absolute of float64 (fp32 sqrt(-2 ln u) cos(2 pi u) with
rad <= 5.8 errs below 1e-5; a wrong word, pixel or channel is off by O(1)).  The fixed cases have no borderline slot
(erase_ref.py) and assert it, so no slot is left out silently."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_ref as A  # noqa: E402
import erase_ref as E  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 0xFEDCBA9876543210                    # the pair of test_augment_gpu.py
OFFSET = (1 << 32) + 5
RNG = (SEED, OFFSET)
STATS = {1: ((0.1307,), (0.3081,)), 3: ((0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010))}
INDEX = [3, 0, 3, 6, 1]                      # B = 5, record 3 twice
INDEX8 = [3, 0, 3, 6, 1, 2, 5, 4]
GEOMS = [(3, 32, 4), (1, 28, 4), (3, 16, 8), (1, 28, 7), (1, 8, 4)]     # (C, S, p)
RETRY_SCALE = (0.3, 0.95)
TOL = 1e-4


@pytest.fixture(scope="module")
def K():
    from vitpe import kernels
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return kernels


def signed(v):
    return v - (1 << 64) if v >= (1 << 63) else v


def pair(seed=SEED, offset=OFFSET):
    return torch.tensor([signed(seed), signed(offset)], dtype=torch.int64, device="cuda")


def words(rng):
    return tuple(int(v) & 0xFFFFFFFFFFFFFFFF for v in rng.reshape(-1).tolist())


_DATA = {}


def dataset(C, S, n=7):
    if (C, S, n) not in _DATA:
        x = np.random.default_rng(100 * C + S).integers(0, 256, size=(n, C, S, S), dtype=np.uint8)
        mean, std = STATS[C]
        _DATA[(C, S, n)] = (x, torch.from_numpy(x).cuda(), torch.tensor(mean, device="cuda"), torch.tensor(std, device="cuda"))
    return _DATA[(C, S, n)]


_REF = {}


def ref(C, S, pad, hflip, index, prob, mode="const", scale=E.SCALE, rng=RNG, n=7):
    """(img float64, mask, prm, borderline) of erase_ref.images, computed once per case; never modified."""
    key = (C, S, pad, hflip, tuple(index), prob, mode, scale, rng, n)
    if key not in _REF:
        _REF[key] = E.images(dataset(C, S, n)[0], index, *STATS[C], rng, pad, hflip, prob, mode, scale)
    return _REF[key]


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


# ---- 1. the draws -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [E.SCALE, RETRY_SCALE])
@pytest.mark.parametrize("S", [32, 16])
def test_device_draws_equal_the_host_entry_and_the_reference(K, S, scale):
    B = 37
    for prob in (0.5, 1.0):
        got = K.erase_params(pair(), B, S, prob, scale)
        assert got.dtype == torch.int32 and tuple(got.shape) == (B, 5) and got.is_cuda
        host = K.erase_params(RNG, B, S, prob, scale, host=True)
        assert torch.equal(got.cpu(), host)                                            # all slots
        want, border, _ = E.params(RNG, B, S, prob, scale)
        print(f"S {S} scale {scale} prob {prob}: {int(border.sum())} borderline of {B}")
        assert border.sum() <= 1
        assert np.array_equal(got.cpu().numpy().astype(np.int64)[~border], want[~border])
    assert (K.erase_params(pair(), B, S, 0.0, scale) == 0).all()


# ---- 2. vitpe_unfold_u8_erase, const -----------------------------------------------------------------------------------------
def _unfold_const(K, C, S, p, pad, hflip, index, scale):
    x, xd, mean, std = dataset(C, S)
    B = len(index)
    want64, mask, prm, border = ref(C, S, pad, hflip, index, 1.0, "const", scale)
    assert not border.any()
    want_img = want64.astype(np.float32)
    want = A.unfold(want_img, p)
    idx = torch.tensor(index, device="cuda")
    kw = dict(rng=pair(), crop_pad=pad, hflip=hflip, erase_prob=1.0, erase_scale=scale)
    img = torch.full((B, C, S, S), float("nan"), device="cuda")
    got = K.unfold_u8(xd, idx, mean, std, p, torch.float32, img_out=img, **kw)
    assert tuple(got.shape) == want.shape
    assert np.array_equal(bits(img), want_img.view(np.uint32))
    assert np.array_equal(bits(got), want.view(np.uint32))
    got16 = K.unfold_u8(xd, idx, mean, std, p, torch.bfloat16, **kw)
    assert torch.equal(got16.cpu(), torch.from_numpy(want).to(torch.bfloat16))
    return want_img, mask, prm


@pytest.mark.parametrize("pad,hflip", [(0, False), (2, True)])
@pytest.mark.parametrize("C,S,p", GEOMS)
def test_unfold_u8_const_equals_the_reference(K, C, S, p, pad, hflip):
    want_img, mask, prm = _unfold_const(K, C, S, p, pad, hflip, INDEX, E.SCALE)
    assert (prm[:, 0] == 1).all() and mask.any() and not mask.all()
    assert (want_img[np.broadcast_to(mask[:, None], want_img.shape)] == 0).all()
    assert not np.array_equal(prm[0], prm[2])                     # the same record in two slots: two rectangles
    base = A.images(dataset(C, S)[0], INDEX, *STATS[C], RNG, pad, hflip)
    assert not np.array_equal(want_img, base)                      # the erasing changed something


@pytest.mark.parametrize("C,S,p", [(3, 32, 4), (3, 16, 8)])
def test_unfold_u8_const_with_retries(K, C, S, p):
    """scale (0.3, 0.95): most first attempts do not fit; the reference's first 8 slots need up to 5 attempts."""
    attempts = E.params(RNG, len(INDEX8), S, 1.0, RETRY_SCALE)[2]
    assert attempts.max() == 4 and (attempts >= 1).sum() >= 3
    _unfold_const(K, C, S, p, 2, True, INDEX8, RETRY_SCALE)


# ---- 3. vitpe_unfold_u8_erase, rand and pixel ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["rand", "pixel"])
@pytest.mark.parametrize("C,S,p,pad,hflip", [(3, 32, 4, 4, True), (1, 28, 7, 0, False), (3, 16, 8, 2, True)])
def test_unfold_u8_rand_and_pixel(K, C, S, p, pad, hflip, mode):
    x, xd, mean, std = dataset(C, S)
    B = len(INDEX)
    want64, mask, prm, border = ref(C, S, pad, hflip, INDEX, 1.0, mode)
    assert not border.any() and (prm[:, 0] == 1).all()
    m = np.broadcast_to(mask[:, None], want64.shape)
    idx = torch.tensor(INDEX, device="cuda")
    kw = dict(rng=pair(), crop_pad=pad, hflip=hflip, erase_prob=1.0, erase_mode=mode)
    img = torch.full((B, C, S, S), float("nan"), device="cuda")
    got = K.unfold_u8(xd, idx, mean, std, p, torch.float32, img_out=img, **kw)
    img_h, got_h = img.cpu().numpy(), got.cpu().numpy()
    assert np.array_equal(img_h[~m].view(np.uint32), want64[~m].astype(np.float32).view(np.uint32))     # outside: bit-exact
    err = np.abs(img_h.astype(np.float64) - want64)[m].max()
    print(f"{mode} C {C} S {S}: max |kernel - float64| inside the rectangles = {err:.3e}")
    assert err <= TOL
    assert np.array_equal(got_h.view(np.uint32), A.unfold(img_h, p).view(np.uint32))                  # patch matrix == image
    got16 = K.unfold_u8(xd, idx, mean, std, p, torch.bfloat16, **kw)
    assert torch.equal(got16.cpu(), got.cpu().to(torch.bfloat16))
    for b in range(B):
        _, i, j, h, w = (int(v) for v in prm[b])
        rect = img_h[b, :, i:i + h, j:j + w].reshape(C, -1)
        assert rect.shape[1] > 1
        const = (rect == rect[:, :1]).all()
        assert const if mode == "rand" else not const
        if C > 1:
            assert not np.array_equal(rect[0], rect[1])               # the channels draw their own values


# ---- 4. data.augment_batch ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["const", "rand", "pixel"])
@pytest.mark.parametrize("C,S,pad,hflip", [(3, 32, 4, True), (1, 28, 2, True), (1, 16, 0, False)])
def test_augment_batch_returns_the_erased_images(K, C, S, pad, hflip, mode):
    """The module path's images (one patch per image, p = S).  prob 0.5: slots 0 and 4 of the five are erased, 1..3 are not;
    (1, 16) has crop and flip off: erasing alone."""
    from vitpe.data import ResidentDataset, augment_batch
    x = dataset(C, S)[0]
    idx = torch.tensor(INDEX, device="cuda")
    want64, mask, prm, border = ref(C, S, pad, hflip, INDEX, 0.5, mode)
    assert not border.any() and prm[:, 0].tolist() == [1, 0, 0, 0, 1]
    ds = ResidentDataset(torch.from_numpy(x), torch.arange(x.shape[0]), *STATS[C], "cuda")
    images = augment_batch(ds, idx, pair(), crop_pad=pad, hflip=hflip, erase_prob=0.5, erase_mode=mode)
    assert images.dtype == torch.float32 and tuple(images.shape) == (len(INDEX), C, S, S)
    m = np.broadcast_to(mask[:, None], want64.shape)
    assert np.abs(images.cpu().numpy().astype(np.float64) - want64)[m].max() <= TOL
    assert np.array_equal(bits(images)[~m], want64[~m].astype(np.float32).view(np.uint32))
    assert torch.isfinite(images).all()
    plain = augment_batch(ds, idx, pair(), crop_pad=pad, hflip=hflip)
    assert not torch.equal(plain[0], images[0]) and torch.equal(plain[1:4], images[1:4])       # erased / untouched slots


# ---- 5. identity and the C entry's checks ---------------------------------------------------------------------------------------
TAIL = (1 << 31, 0, 0.02, 0.33, math.log(0.3), math.log(3.3))            # erase_thr, erase_mode, smin, smax, lmin, lmax
BAD_TAILS = [((1 << 32) + 1, 0, 0.02, 0.33, -1.0, 1.0), (1 << 31, 3, 0.02, 0.33, -1.0, 1.0), (1 << 31, -1, 0.02, 0.33, -1.0, 1.0),
             (1 << 31, 0, 0.0, 0.33, -1.0, 1.0), (1 << 31, 0, 0.5, 0.33, -1.0, 1.0), (1 << 31, 0, 0.02, 1.5, -1.0, 1.0),
             (1 << 31, 0, 0.02, 0.33, 1.0, -1.0), (1 << 31, 0, 0.02, 0.33, float("nan"), 1.0)]


@pytest.mark.parametrize("C,S,p", [(3, 32, 4), (3, 16, 8), (1, 16, 8)])
def test_switched_off_nothing_changes(K, C, S, p):
    from vitpe import _lib as L
    x, xd, mean, std = dataset(C, S)
    B, dt, pad = len(INDEX), torch.bfloat16, 2
    idx = torch.tensor(INDEX, device="cuda")
    lib, sp = L.lib(), L.stream_ptr()
    rng = pair()
    off = (0,) + TAIL[1:]
    imgs = [torch.empty(B, C, S, S, device="cuda") for _ in range(5)]
    plain = K.unfold_u8(xd, idx, mean, std, p, dt, img_out=imgs[0])
    aug = K.unfold_u8(xd, idx, mean, std, p, dt, img_out=imgs[1], rng=rng, crop_pad=pad, hflip=True)
    assert not torch.equal(aug, plain)
    py0 = K.unfold_u8(xd, idx, mean, std, p, dt, img_out=imgs[2], rng=rng, crop_pad=pad, hflip=True, erase_prob=0.,
                      erase_mode="rand")                                                     # the _erase entry with thr = 0
    c0, cnull = torch.empty_like(plain), torch.empty_like(plain)
    head = (L.BF16, xd.data_ptr(), idx.data_ptr(), mean.data_ptr(), std.data_ptr())
    assert lib.vitpe_unfold_u8_erase(*head, c0.data_ptr(), imgs[3].data_ptr(), B, C, S, p, rng.data_ptr(), pad, 1, *off, sp) == 0
    assert lib.vitpe_unfold_u8_erase(*head, cnull.data_ptr(), imgs[4].data_ptr(), B, C, S, p, None, pad, 1, *TAIL, sp) == 0
    assert torch.equal(py0, aug) and torch.equal(c0, aug) and torch.equal(imgs[2], imgs[1]) and torch.equal(imgs[3], imgs[1])
    assert torch.equal(cnull, plain) and torch.equal(imgs[4], imgs[0])
    untouched = torch.full_like(plain, 7.0)
    for bad in BAD_TAILS:
        assert lib.vitpe_unfold_u8_erase(*head, untouched.data_ptr(), None, B, C, S, p, rng.data_ptr(), pad, 1, *bad, sp) == 1, bad
    assert lib.vitpe_unfold_u8_erase(*head, untouched.data_ptr(), None, B, C, S, p, rng.data_ptr(), S + 1, 1, *TAIL, sp) == 1
    assert (untouched == 7.0).all()                                                          # nothing was launched
    torch.cuda.synchronize()
