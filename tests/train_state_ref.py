"""Plain numpy / float64 restatements of what a training step leaves behind: the AdamW update (adamw_kernel in
csrc/optim.hip) and the seven destination layouts of refresh_shadows_kernel (kinds 0-6, include/vitpe.h).  Shared by
tests/test_train_state_cpu.py (the references are right, the inputs discriminate) and tests/test_train_state_gpu.py
(the kernels against them).  No GPU and no vitpe import here."""
import math

import numpy as np

U = 2.0 ** -24   # unit roundoff of fp32: one rounding to nearest moves a value by at most U relative

# the record layout of vitpe_refresh_shadows (include/vitpe.h; the dtype engine._build_flat fills)
REC_DTYPE = np.dtype([("src", "<i8"), ("dst", "<i8"), ("dst2", "<i8"), ("R", "<i4"), ("C", "<i4"), ("tile0", "<i4"),
                      ("kind", "<i4"), ("HD", "<i4"), ("kind2", "<i4"), ("HD2", "<i4"), ("pad", "<i4")])


# ------------------------------------------------------------------------------------------ AdamW
def adamw_ref(p, g, m, v, hp, bc1, bc2, variant=None):
    """One AdamW step in float64 on the fp32 device values as they are, in adamw_kernel's order of operations: the gradient
    is scaled first (hp[8]), the decay is decoupled (p * (1 - lr * wd)), denom = sqrt(v) / sqrt(bc2) + eps.  hp[0..4] and
    hp[8] are widened from fp32; the bias corrections bc1 / bc2 are arguments (the device forms them from fp32 betas).
    Returns (p, m, v, delta), delta = the update term p lost.

    variant: one of the WRONG updates the input set of adamw_inputs() must tell from the right one
    ("eps_in_bc", "l2_decay", "no_bc2", "scale_late"); None = the right one."""
    assert variant in (None, "eps_in_bc", "l2_decay", "no_bc2", "scale_late")
    f = lambda a: np.asarray(a, dtype=np.float64)   # noqa: E731
    p, g, m, v = f(p), f(g), f(m), f(v)
    hp = np.asarray(hp, dtype=np.float32).astype(np.float64)
    lr, b1, b2, eps, wd, gs = hp[0], hp[1], hp[2], hp[3], hp[4], hp[8]
    bc1, bc2 = float(bc1), float(bc2)
    gi = g if variant == "scale_late" else g * gs
    if variant == "l2_decay":
        gi = gi + wd * p
        pd = p
    else:
        pd = p * (1.0 - lr * wd)
    m = b1 * m + (1.0 - b1) * gi
    v = b2 * v + (1.0 - b2) * gi * gi
    if variant == "eps_in_bc":
        denom = (np.sqrt(v) + eps) / math.sqrt(bc2)
    elif variant == "no_bc2":
        denom = np.sqrt(v) + eps
    else:
        denom = np.sqrt(v) / math.sqrt(bc2) + eps
    delta = (lr / bc1) * (m * gs if variant == "scale_late" else m) / denom
    return pd - delta, m, v, delta


def adamw_bounds(p0, p_ref, m_ref, v_ref, delta_ref):
    """Per-element fp32 error bounds of adamw_kernel against adamw_ref started from the same fp32 state (U = 2^-24), for
    inputs whose moments do not cancel (g keeps its sign from step to step) and whose (1 - b2) g^2 is a normal number.

    Count of the roundings (every fp32 operation: <= U relative; -ffp-contract=on fuses a multiply into the following
    add, which only removes one; 1 - b1 and 1 - b2 are exact for betas in [0.5, 1]):
      m = b1 m + (1 - b1) (g gs):  g gs 1, (1 - b1) gi 1, b1 m 1 (the other summand), the sum 1: the longer chain is 3
          -> 3U |m_ref|; the issue's 4U is kept.
      v = b2 v + (1 - b2) gi gi:   gi enters twice 2, two products 2, the sum 1 (b2 v: 1 + 1 = 2 is the shorter chain)
          -> 5U |v_ref|; the issue's 6U is kept.
      p = p0 (1 - lr wd) - delta:  lr wd 1 (worth 5e-5 U of p0), 1 - x 1, the product 1, and the final subtraction 1 on
          |p0| + |delta| -> 3.0001 U |p0| + U |delta| + the error of delta;
      delta = (lr / bc1) m / (sqrt(v) (1 / sqrt(bc2)) + eps): numerator lr / bc1 1, m 3, product 1 = 5; denominator
          v 5 / 2 = 2.5, sqrt 1, sqrt(bc2) 1 and its reciprocal 1, product 1, + eps 1 = 7.5; the division 1: 13.5
          -> p: 3.0001 U |p0| + 14.5 U |delta_ref|; the issue's 4U |p0| + 16U |delta_ref| is kept (it is the larger)."""
    bp = 4 * U * np.abs(p0) + 16 * U * np.abs(delta_ref)
    return bp, 4 * U * np.abs(m_ref), 6 * U * np.abs(v_ref)


ADAMW_HP = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.05, gs=0.25)


def adamw_hp(**over):
    """The 16-float hp block of vitpe_adamw_step (include/vitpe.h) with the test's hyper-parameters, as fp32."""
    h = dict(ADAMW_HP, **over)
    hp = np.zeros(16, dtype=np.float32)
    hp[:5] = [h["lr"], h["b1"], h["b2"], h["eps"], h["wd"]]
    hp[8] = h["gs"]
    return hp


def adamw_inputs(n, seed=0):
    """(p0, g) fp32 [n]: |g| log-spaced over 1e-15 .. 1 in a seeded random order with both signs and exact zeros (every
    17th element), p0 drawn from {0, +-1e-3, +-1}.  |g| >= 1e-15 keeps (1 - b2) (g gs)^2 a normal fp32 number
    (6e-35 at gs = 0.25); the small |g| put eps in charge of the denominator, the zeros of p0 leave the update term alone
    in p, p0 = +-1 makes the decay term visible."""
    rng = np.random.default_rng(seed)
    expo = np.linspace(-14.999, 0.0, n)[rng.permutation(n)]
    g = (10.0 ** expo) * rng.choice([-1.0, 1.0], size=n)
    g[::17] = 0.0
    p0 = rng.choice(np.array([0.0, 1e-3, -1e-3, 1.0, -1.0]), size=n)
    g = g.astype(np.float32)
    assert float(np.abs(g[g != 0]).min()) >= 1e-15
    return p0.astype(np.float32), g


# ------------------------------------------------------------------------------------------ weight copies
def _frag_index(R, C, kchunk, phi):
    """vitpe_pack_weight_frags of a [R, C] matrix (include/vitpe.h): 1-KB fragments (64 lanes x 8 elements) at fragment
    index ((kc * R/16 + nt) * kchunk/32 + ks); lane 16 g + cc, element e holds W[16 nt + cc][kchunk kc + 32 ks + k],
    k = 8 g + e (phi 0) or (e < 4 ? 4 g + e : 16 + 4 g + e - 4) (phi 1).  Returns (row, col) per destination element."""
    assert R % 16 == 0 and kchunk % 32 == 0 and C % kchunk == 0
    ksc, ntr = kchunk // 32, R // 16
    idx = np.arange(R * C)
    e, lane, blk = idx & 7, (idx >> 3) & 63, idx >> 9
    ks, nt, kc = blk % ksc, (blk // ksc) % ntr, blk // ksc // ntr
    cc, g = lane & 15, lane >> 4
    k = np.where(e < 4, 4 * g + e, 16 + 4 * g + e - 4) if phi else 8 * g + e
    return 16 * nt + cc, kchunk * kc + 32 * ks + k


def shadow_index(kind, R, C, hd):
    """Flat source index (into the row-major fp32 [R, C] master) of every destination element of shadow `kind`."""
    src = np.arange(R * C).reshape(R, C)
    if kind == 0:      # dst[c][r] = src[r][c]
        return src.T.reshape(-1).copy()
    if kind == 1:      # vitpe_pack_qkv_weights: block (head, {q,k,v}, 16-row tile nt, 32-deep chunk ks), lane 16 g + c, e
        D = C
        assert R == 3 * D and D % hd == 0 and hd % 16 == 0 and D % 32 == 0
        H = D // hd    # rows: mat, h, nt, c ; columns: ks, g, e  ->  h, mat, nt, ks, g, c, e
        return src.reshape(3, H, hd // 16, 16, D // 32, 4, 8).transpose(1, 0, 2, 4, 5, 3, 6).reshape(-1).copy()
    if kind in (2, 3):
        r, c = _frag_index(R, C, hd, kind & 1)
        return r * C + c
    if kind in (4, 5):  # the same packs of the TRANSPOSE [C, R]: its element (r', c') is src[c'][r']
        r, c = _frag_index(C, R, hd, kind & 1)
        return c * C + r
    if kind == 6:      # vitpe_pack_qkv_weights_wide: block ((h * 3 + mat) * D/16 + s), lane r + 32 hh, element j
        D = C
        assert R == 3 * D and hd == 32 and D % 32 == 0
        H = D // 32    # rows: mat, h, r ; columns: s, hh, j  ->  h, mat, s, hh, r, j
        return src.reshape(3, H, 32, D // 16, 2, 8).transpose(1, 0, 3, 4, 2, 5).reshape(-1).copy()
    raise ValueError(f"shadow kind {kind}")


def wide_qscale(hd):
    """The q-row factor of the wide pack, hd^-0.5 log2(e), as the fp32 number tests/test_kernels_gpu.py
    (test_wide_qkv_pack_layout) multiplies by."""
    return np.float32(math.log2(math.e) / math.sqrt(hd))


def shadow_ref(kind, w, hd, qscale=None):
    """Destination array (flat fp32) of shadow `kind` of the fp32 master w [R, C]: an index gather of w; kind 6 multiplies
    the q rows (the first C of the 3 C) by hd^-0.5 log2(e) in fp32 (qscale overrides the factor)."""
    w = np.ascontiguousarray(np.asarray(w, dtype=np.float32))
    R, C = w.shape
    idx = shadow_index(kind, R, C, hd)
    out = w.reshape(-1)[idx]
    if kind == 6:
        qs = wide_qscale(hd) if qscale is None else np.float32(qscale)
        out = np.where(idx // C < C, out * qs, out).astype(np.float32)
    return out


# The descriptor list of the stand-alone vitpe_refresh_shadows test: the smallest that reaches every branch of the kernel
# (a ragged transposed copy, every kind as first and kinds 0 / 2 / 4 / 5 as second shadow, the ViT-B pair 0 + 2 at chunk 64).
SHADOW_CASES = [   # (R, C, kind, HD, kind2, HD2)
    (50, 70, 0, 0, -1, 0),
    (192, 64, 1, 32, 4, 64),
    (192, 64, 6, 32, -1, 0),
    (64, 128, 2, 64, 5, 32),
    (96, 32, 3, 32, 0, 0),
    (192, 64, 0, 0, 2, 64),
]


def shadow_layout(cases=SHADOW_CASES, align=8, gap=24):
    """Source / destination offsets for `cases`: every span starts on a multiple of `align` elements, `gap` unused
    elements in front of every span (and after the last).  Returns (records [REC_DTYPE], tile_map int16, n_src, n_dst,
    spans) with spans = [(case index, kind, HD, dst offset, R, C)], one per shadow written."""
    up = lambda x: (x + align - 1) // align * align   # noqa: E731
    rec = np.zeros(len(cases), dtype=REC_DTYPE)
    spans, src, dst, tile0 = [], 0, 0, 0
    for i, (R, C, kind, hd, kind2, hd2) in enumerate(cases):
        src = up(src + gap)
        s0, src = src, src + R * C
        dst = up(dst + gap)
        d1, dst = dst, dst + R * C
        spans.append((i, kind, hd, d1, R, C))
        d2 = 0
        if kind2 >= 0:
            dst = up(dst + gap)
            d2, dst = dst, dst + R * C
            spans.append((i, kind2, hd2, d2, R, C))
        rec[i] = (s0, d1, d2, R, C, tile0, kind, hd, kind2, hd2, 0)
        tile0 += ((R + 31) // 32) * ((C + 31) // 32)
    tmap = np.zeros(tile0, dtype=np.int16)
    for i in range(len(cases)):
        tmap[rec["tile0"][i]:] = i
    return rec, tmap, up(src + gap), up(dst + gap), spans
