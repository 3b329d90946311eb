"""numpy restatement of the dropout streams ("Dropout streams"), shared by test_dropout_cpu.py and
test_dropout_gpu.py.  Written from the definition, not from the HIP source: Philox4x32-10 as published (Salmon et al.,
SC'11), and for a site with the pair (seed, offset) and the logical element e

    key = (lo32 seed, hi32 seed), counter = (lo32(e >> 2), hi32(e >> 2), lo32 offset, hi32 offset), word = e & 3
    keep(e) = word >= floor(p * 2^32);  kept values are multiplied by 1 / (1 - p)  (float32 arithmetic)
"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK32 = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(key, ctr):
    """key [..., 2], ctr [..., 4] (any unsigned integer arrays) -> uint32 [..., 4]."""
    key = np.asarray(key).astype(np.uint64)
    ctr = np.asarray(ctr).astype(np.uint64)
    k0, k1 = key[..., 0] & MASK32, key[..., 1] & MASK32
    c0, c1, c2, c3 = (ctr[..., i] & MASK32 for i in range(4))
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                      # 32 x 32 -> 64 bit products (no overflow in uint64)
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & MASK32, (p0 >> S32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def threshold(p):
    return np.uint32(int(np.floor(float(np.float32(p)) * 4294967296.0)))


def scale(p):
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def words(rng, e):
    """The 32-bit word of every logical element index in e (uint64 array) for the pair rng = (seed, offset)."""
    seed, off = (int(v) & 0xFFFFFFFFFFFFFFFF for v in rng)
    e = np.asarray(e, dtype=np.uint64)
    q = e >> np.uint64(2)
    uq, inv = np.unique(q, return_inverse=True)
    ctr = np.stack([uq & MASK32, uq >> S32, np.full_like(uq, off & 0xFFFFFFFF), np.full_like(uq, off >> 32)], axis=-1)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    w = philox4x32_10(np.broadcast_to(key, (len(uq), 2)), ctr)
    return w[inv.reshape(e.shape), (e & np.uint64(3)).astype(np.int64)]


def keep(rng, e, p):
    return words(rng, e) >= threshold(p)


def mask_elements(rng, n, p):
    """Elementwise site (and the per-sample site with n = B): e = index."""
    return keep(rng, np.arange(n, dtype=np.uint64), p)


def mask_attention(rng, B, H, N, p):
    """Attention-probability site -> bool [B, H, N, N]: e = ((b H + h) N + i) NP + j, NP = N rounded up to 4."""
    NP = (N + 3) // 4 * 4
    rows = np.arange(B * H * N, dtype=np.uint64).reshape(B, H, N, 1)
    return keep(rng, rows * np.uint64(NP) + np.arange(N, dtype=np.uint64), p)
