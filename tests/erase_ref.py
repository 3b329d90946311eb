"""numpy / float64 restatement of the erasing stream ("Erasing stream"), shared by test_erase_cpu.py and
test_erase_gpu.py.  Written from the contract, not from the HIP source.  RandomErasing(p, scale, ratio) after Normalize, on the
output pixel coordinates (after crop and flip), on the augmentation site's pair rng = (seed, offset).  Every draw is a
Philox4x32-10 call (dropout_stream.py) with

    key = (lo32 seed, hi32 seed), counter = (c0, c1, lo32 offset, hi32 offset) -> w0, w1, w2, w3
    u(w) = ((w >> 9) + 0.5) 2^-23

    switch     (c0, c1) = (b, 0), the crop/flip call: slot b is erased iff w3 < floor(float32(prob) 2^32)
    attempt a  (c0, c1) = (b, a + 1), a = 0..9:
                   area = S S (smin + u(w0) (smax - smin)),  r = exp(lmin + u(w1) (lmax - lmin))
                   h = rint(sqrt(area r)),  w = rint(sqrt(area / r)),  accepted iff h < S and w < S, then
                   i = mulhi32(w2, S - h + 1),  j = mulhi32(w3, S - w + 1);   no accepted attempt: nothing is erased
               smin, smax are float32 values, lmin = float32(log(rmin)), lmax = float32(log(rmax))
    fill of output pixel (c, y, x), i <= y < i + h, j <= x < j + w:
        const  0
        rand   normal(c) of the call (c0, c1) = (b, 11)
        pixel  normal(c) of the call (c0, c1) = (lo32 e, 0x80000000 | hi32 e),  e = (b S + y) S + x
        normal(c), k = c >> 1:  sqrt(-2 ln u(w[2k])) * (sin if c & 1 else cos)(float32(6.2831853) u(w[2k+1]))

The kernels evaluate the rectangle chain in float32, this file in float64: a slot is BORDERLINE when some attempt it makes has
sqrt(area r) or sqrt(area / r) within 1e-3 of a half-integer (float32's relative error near 1e-6 on values up to
1.8 S = 58 at S <= 32 is at most 6e-5 absolute: more than 10x margin).  Borderline slots are left out of exact comparisons.
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_ref as A  # noqa: E402
import dropout_stream as S  # noqa: E402

SCALE, RATIO = (0.02, 0.33), (0.3, 3.3)
ATTEMPTS = 10
BORDER = 1e-3
TWO_PI = float(np.float32(6.2831853))


def threshold(prob):
    return int(math.floor(float(np.float32(prob)) * 4294967296.0))


def calls(rng, c0, c1):
    """c0, c1: equal-shaped unsigned integer arrays -> uint32 [..., 4], one Philox call each for the pair rng."""
    seed, off = (int(v) & 0xFFFFFFFFFFFFFFFF for v in rng)
    c0, c1 = np.broadcast_arrays(np.asarray(c0, dtype=np.uint64), np.asarray(c1, dtype=np.uint64))
    ctr = np.stack([c0, c1, np.full_like(c0, off & 0xFFFFFFFF), np.full_like(c0, off >> 32)], axis=-1)
    key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64), c0.shape + (2,))
    return S.philox4x32_10(key, ctr)


def uniform(w):
    return ((np.asarray(w, dtype=np.uint64) >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def params(rng, B, Sz, prob, scale=SCALE, ratio=RATIO):
    """-> (prm int64 [B, 5] = (on, i, j, h, w), borderline bool [B], attempts int64 [B]): attempts = the index of the accepted
    attempt, ATTEMPTS where all ten were refused (on = 0), -1 where the switch is off."""
    b = np.arange(B, dtype=np.uint64)
    switch = calls(rng, b, np.zeros_like(b))[:, 3].astype(np.uint64) < np.uint64(threshold(prob))
    smin, smax = (float(np.float32(v)) for v in scale)
    lmin, lmax = (float(np.float32(math.log(v))) for v in ratio)
    prm = np.zeros((B, 5), dtype=np.int64)
    border = np.zeros(B, dtype=bool)
    attempts = np.full(B, -1, dtype=np.int64)
    for s in np.nonzero(switch)[0]:
        attempts[s] = ATTEMPTS
        for a in range(ATTEMPTS):
            w = calls(rng, np.uint64(s), np.uint64(a + 1))
            area = Sz * Sz * (smin + uniform(w[0]) * (smax - smin))
            r = math.exp(lmin + uniform(w[1]) * (lmax - lmin))
            fh, fw = math.sqrt(area * r), math.sqrt(area / r)
            if min(abs(fh - math.floor(fh) - 0.5), abs(fw - math.floor(fw) - 0.5)) < BORDER:
                border[s] = True
            h, wd = int(np.rint(fh)), int(np.rint(fw))
            if h < Sz and wd < Sz:
                i = (int(w[2]) * (Sz - h + 1)) >> 32
                j = (int(w[3]) * (Sz - wd + 1)) >> 32
                prm[s] = (1, i, j, h, wd)
                attempts[s] = a
                break
    return prm, border, attempts


def normals(w):
    """uint32 [..., 4] -> float64 [..., 4]: the normal of channel c = 0..3 of each call."""
    u = uniform(w)
    out = np.empty(u.shape, dtype=np.float64)
    for c in range(4):
        k = c >> 1
        rad = np.sqrt(-2.0 * np.log(u[..., 2 * k]))
        ang = TWO_PI * u[..., 2 * k + 1]
        out[..., c] = rad * (np.sin(ang) if c & 1 else np.cos(ang))
    return out


def fill(rng, b, Sz, C, prm_b, mode):
    """float64 [C, h, w]: the values of slot b's rectangle."""
    _, i, j, h, wd = (int(v) for v in prm_b)
    if mode == "const":
        return np.zeros((C, h, wd))
    assert C <= 4
    if mode == "rand":
        z = normals(calls(rng, np.uint64(b), np.uint64(11)))[:C]
        return np.broadcast_to(z.reshape(C, 1, 1), (C, h, wd)).copy()
    assert mode == "pixel"
    y, x = np.meshgrid(np.arange(i, i + h, dtype=np.uint64), np.arange(j, j + wd, dtype=np.uint64), indexing="ij")
    e = (np.uint64(b) * np.uint64(Sz) + y) * np.uint64(Sz) + x
    z = normals(calls(rng, e & S.MASK32, np.uint64(0x80000000) | (e >> S.S32)))       # [h, w, 4]
    return np.ascontiguousarray(z[..., :C].transpose(2, 0, 1))


def images(data_u8, index, mean, std, rng, pad, hflip, prob, mode="const", scale=SCALE, ratio=RATIO):
    """-> (img float64 [B,C,S,S], mask bool [B,S,S] (the rectangles), prm, borderline).  Outside the rectangles img holds the
    float32 values of augment_ref.images exactly; inside, the float64 fill."""
    base = A.images(data_u8, index, mean, std, rng, pad, hflip)
    B, C, Sz, _ = base.shape
    prm, border, _ = params(rng, B, Sz, prob, scale, ratio)
    img = base.astype(np.float64)
    mask = np.zeros((B, Sz, Sz), dtype=bool)
    for b in range(B):
        on, i, j, h, wd = (int(v) for v in prm[b])
        if on:
            mask[b, i:i + h, j:j + wd] = True
            img[b, :, i:i + h, j:j + wd] = fill(rng, b, Sz, C, prm[b], mode)
    return img, mask, prm, border
