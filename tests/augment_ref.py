"""numpy restatement of the augmentation stream ("Augmentation stream"), shared by test_augment_cpu.py and
test_augment_gpu.py.  Written from the contract, not from the HIP source.  For the pair rng = (seed, offset), crop padding
`pad` and the flag `hflip`, batch slot b makes one Philox4x32-10 call (dropout_stream.py)

    key = (lo32 seed, hi32 seed), counter = (lo32 b, hi32 b, lo32 offset, hi32 offset) -> w0, w1, w2, w3
    (the words of the logical elements 4b, 4b+1, 4b+2 of a dropout site with the same pair)
    oy = mulhi32(w0, 2 pad + 1), ox = mulhi32(w1, 2 pad + 1), flip = hflip and (w2 >> 31)

and output pixel (c, y, x) of slot b is the source byte u = data[index[b], c, y + oy - pad, (S-1-x if flip else x) + ox - pad],
or u = 0 outside the image, then v = ((float32)u / 255 - mean[c]) / std[c] in float32, in that order.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dropout_stream as S  # noqa: E402


def params(rng, B, pad, hflip):
    """-> int64 [B, 3] = (oy, ox, flip) of slots 0..B-1."""
    b = np.arange(B, dtype=np.uint64)
    w = np.stack([S.words(rng, np.uint64(4) * b + np.uint64(k)) for k in range(3)], axis=-1).astype(np.uint64)
    span = np.uint64(2 * int(pad) + 1)
    oy = (w[:, 0] * span) >> np.uint64(32)
    ox = (w[:, 1] * span) >> np.uint64(32)
    flip = (w[:, 2] >> np.uint64(31)) if hflip else np.zeros(B, dtype=np.uint64)
    return np.stack([oy, ox, flip], axis=-1).astype(np.int64)


def images(data_u8, index, mean, std, rng, pad, hflip):
    """data_u8 uint8 [N,C,S,S], index int [B] or None (the first records) -> float32 [B,C,S,S]."""
    data_u8 = np.asarray(data_u8)
    index = np.arange(data_u8.shape[0]) if index is None else np.asarray(index)
    B, (_, C, Sz, _) = len(index), data_u8.shape
    prm = params(rng, B, pad, hflip)
    padded = np.zeros((C, Sz + 2 * pad, Sz + 2 * pad), dtype=np.uint8)
    out = np.empty((B, C, Sz, Sz), dtype=np.float32)
    mean = np.asarray(mean, dtype=np.float32).reshape(C, 1, 1)
    std = np.asarray(std, dtype=np.float32).reshape(C, 1, 1)
    for b in range(B):
        oy, ox, flip = (int(v) for v in prm[b])
        padded[:] = 0
        padded[:, pad:pad + Sz, pad:pad + Sz] = data_u8[index[b]]
        win = padded[:, oy:oy + Sz, ox:ox + Sz]            # source (y + oy - pad, xs + ox - pad) of the unpadded image
        if flip:
            win = win[:, :, ::-1]                          # xs = S - 1 - x
        out[b] = (win.astype(np.float32) / np.float32(255.0) - mean) / std
    return out


def unfold(img, p):
    """float32 [B,C,S,S] -> [B * (S/p)^2, C p^2], row = b P + gy G + gx, column = c p^2 + ky p + kx."""
    B, C, Sz, _ = img.shape
    G = Sz // p
    x = img.reshape(B, C, G, p, G, p).transpose(0, 2, 4, 1, 3, 5)      # b, gy, gx, c, ky, kx
    return np.ascontiguousarray(x).reshape(B * G * G, C * p * p)


def patches(data_u8, index, mean, std, rng, pad, hflip, p):
    return unfold(images(data_u8, index, mean, std, rng, pad, hflip), p)
