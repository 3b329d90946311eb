"""Case lists, input builders and the float64 reference for the tests of csrc/embed.hip: the fused patch embedding
(vitpe_patch_embed / vitpe_patch_embed_aug) and the stand-alone unfold kernels.  Shared by tests/test_embed_cpu.py (the
lists reach every code path, the reference equals the oracle and a float64 conv2d, seeded index bugs are visible above
the gates) and tests/test_embed_gpu.py (the kernels against the reference).  No GPU and no vitpe import here.

The reference:  tokens[b, 0] = cls,  tokens[b, 1 + n] = X[b P + n] W^T + bias (+ ape[n])  in float64, with X the patch
matrix THE KERNEL SEES (rounded to the compute type) and W rounded likewise.  X from fp32 images is a reshape / permute;
X from the resident uint8 dataset is augment_ref.images + augment_ref.unfold (the bit-level restatement of the gather,
ToTensor, Normalize, crop and flip) -- nothing of it is restated a second time here.

Gates of the GPU test (none of them comes from a measured result):
  patch matrix   bit-equal to X
  class row      bit-equal to cls rounded to the compute type
  patch rows     per element, with A = sum_k |x_k| |w_dk| + |bias_d| + |ape_nd|  (abs_terms):
                   fp32   |d| <= (K + 4) 2^-23 A
                   bf16   |d| <= 2^-8 |ref| + (K + 4) 2^-23 A
                 twice the standard forward bound (K + 2) 2^-24 A of a K-term fp32 dot product plus two additions in any
                 order, plus half a bf16 ulp for the one rounding on store; bf16 in addition: the stored value is the
                 rounding of SOME value within the fp32 bound of the reference (outside_rounding_interval)
  integer case   pixels in [-3, 3], w in {-1, 0, 1}, bias / ape in [-8, 8], cls in [-100, 100]: every partial sum is an
                 integer of magnitude <= 64 * 3 + 8 + 8 = 208, exact in fp32 accumulation and in bf16 storage, so tokens
                 are bit-equal in both types
  statistics     ln_ref.stat_errors against the float64 statistics of the rows the kernel stored, ln_ref.STAT_TOL
"""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_ref as A  # noqa: E402
from head_ref import DT  # noqa: E402

# the kernel's limits (csrc/embed.hip: EMB_KP, EMB_MP, EMB_DMAX) and the grid caps of the unfold launches
KP, MP, DMAX = 64, 64, 256
UNFOLD_CAP, UNFOLD8_CAP = 8192 * 256, 16384 * 256

STATS = {1: ((0.1307,), (0.3081,)), 3: ((0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010))}
SEED = 0xC0FFEE1234567891                    # high bits set
OFFSET = (1 << 33) + 11                      # bits above bit 31
INDEX = [3, 0, 3, 6, 1, 5, 2, 2]             # B = 8 batch slots over 7 records, records 3 and 2 twice
NREC = 7
B_IMG = 3                                    # batch of the fp32-image cases
DEFAULT_PAD = 2                              # crop padding of the "u8aug" source of a FUSED_CASES entry
EPS = 1e-5
BOTH, F32 = ("f32", "bf16"), ("f32",)

# (C, S, p, D, dtypes)
FUSED_CASES = [
    (1, 32, 8, 64, BOTH),     # generic branch, K = 64 (no K padding), P = 16: waves 1-3 own no tile
    (1, 64, 8, 256, BOTH),    # generic, P = 64, D at its maximum
    (1, 56, 8, 128, BOTH),    # generic, P = 49: ragged last tile
    (1, 16, 2, 96, F32),      # K = 4
    (3, 16, 2, 192, F32),     # K = 12, three channels on the generic branch
    (3, 10, 2, 48, F32),      # P = 25
    (1, 24, 6, 80, F32),      # K = 36: a 4-element tail in the second 32-wide step, D / 16 = 5
    (3, 32, 4, 16, BOTH),     # D at its minimum
    (3, 32, 4, 256, BOTH),    # D at its maximum
    (1, 20, 4, 240, BOTH),    # P = 25, K = 16
    (3, 8, 4, 32, BOTH),      # P = 4: one live wave, twelve dead rows in its tile
    (3, 32, 4, 192, BOTH),    # the CIFAR geometry (already in the suite)
    (1, 28, 4, 64, BOTH),     # MNIST's native size (already in the suite)
    (1, 24, 4, 112, BOTH),    # P = 36: three live waves, D / 16 = 7
    (1, 12, 4, 144, BOTH),    # P = 9, D / 16 = 9
    (1, 16, 8, 160, BOTH),    # generic, P = 4, D / 16 = 10
    (3, 12, 4, 176, BOTH),    # K = 48, D / 16 = 11
    (1, 32, 8, 208, BOTH),    # generic, D / 16 = 13
    (1, 16, 4, 224, BOTH),    # D / 16 = 14
]
# (C, S, p, D, pad, dtypes): the augmentation stream, on the generic branch but for the last
AUG_CASES = [
    (1, 32, 8, 64, 3, BOTH),
    (1, 56, 8, 128, 4, BOTH),
    (3, 16, 2, 192, 2, F32),
    (1, 16, 2, 96, 16, F32),   # pad == S: windows wholly in the padding
    (3, 32, 4, 256, 4, BOTH),  # p = 4 (the aligned-dword row) at the widest D
]
# (dtype, C, S, p, D, the one condition of the support predicate that fails)
REFUSED = [
    ("f32", 1, 28, 7, 64, "K % chunk"), ("bf16", 1, 28, 7, 64, "K % chunk"),       # K = 49
    ("f32", 3, 32, 8, 256, "K > 64"), ("bf16", 3, 32, 8, 256, "K > 64"),           # K = 192
    ("bf16", 3, 16, 2, 192, "K % chunk"),                                          # K = 12: no multiple of 8
    ("f32", 3, 36, 4, 192, "P > 64"), ("bf16", 3, 36, 4, 192, "P > 64"),           # P = 81
    ("f32", 3, 32, 4, 8, "D < 16"), ("bf16", 3, 32, 4, 24, "D % 16"), ("f32", 3, 32, 4, 272, "D > 256"),
    ("bf16", 3, 32, 4, 8, "D < 16"), ("f32", 3, 32, 4, 24, "D % 16"), ("bf16", 3, 32, 4, 272, "D > 256"),
    ("f32", 3, 30, 4, 192, "S % p"), ("bf16", 1, 28, 8, 64, "S % p"),
]
# vitpe_unfold / vitpe_unfold_u8[_aug]: (C, S, p), every one in both dtypes
UNFOLD_CASES = [(3, 32, 8), (1, 48, 24), (3, 224, 16), (1, 28, 7), (3, 16, 2)]
UNFOLD_B = 2                                 # fp32 images; the uint8 forms gather the slots of INDEX
UNFOLD_PAD = 3
# the smallest launches that enter the grid-stride loops: (kernel, dtype, C, S, p, B)
ABOVE_CAP = [("unfold", "f32", 3, 64, 2, 352), ("unfold_u8", "f32", 3, 64, 2, 352), ("unfold8", "bf16", 1, 8, 8, 524800)]


# ---- which code a case runs ----------------------------------------------------------------------------------------------
def geometry(C, S, p):
    G = S // p
    return G, G * G, C * p * p


def refusals(dt, C, S, p, D):
    """Every condition of vitpe_patch_embed_supported that the case fails (empty: the fused kernel takes it)."""
    if C < 1 or p < 1 or S < p or S % p != 0:
        return ("S % p",)
    _, P, K = geometry(C, S, p)
    chunk = 8 if dt == "bf16" else 4             # elements of a 16-byte chunk
    conds = (("K > 64", K > KP), ("K % chunk", K % chunk != 0), ("P > 64", P > MP), ("D < 16", D < 16), ("D > 256", D > DMAX),
             ("D % 16", D >= 16 and D % 16 != 0))     # (below 16 no width is a multiple of 16: one condition, "D < 16")
    return tuple(name for name, failed in conds if failed)


def branch(dt, C, S, p, D, source, aug=False):
    """(fused or the refusal, gather branch, source, KS = 32-wide K steps, K padded, P % 16, live waves, D / 16)"""
    assert source in ("img", "u8") and not (aug and source == "img")
    why = refusals(dt, C, S, p, D)
    _, P, K = geometry(C, S, p)
    return ("fused" if not why else why[0], "p4" if p == 4 else "generic", "u8aug" if aug else source, (K + 31) // 32, K < KP,
            P % 16, min(4, (P + 15) // 16), D // 16)


def unfold_launch(kernel, dt, C, S, p, B):
    """(threads the launch needs at one item per thread, the cap of its grid) as vitpe_unfold / launch_unfold_u8 compute
    them; the route: bf16 with p % 8 == 0 takes unfold8_kernel (one thread per 8 pixels), everything else one thread per
    patch row."""
    _, P, _ = geometry(C, S, p)
    total = B * P * C * p
    if kernel == "unfold8":
        assert dt == "bf16" and p % 8 == 0
        return total * (p // 8), UNFOLD8_CAP
    assert kernel == "unfold_u8" or not (dt == "bf16" and p % 8 == 0)
    return total, UNFOLD_CAP


for _c in ABOVE_CAP:
    _need, _cap = unfold_launch(*_c)
    assert _cap < _need <= _cap + _cap // 16, (_c, _need, _cap)      # above the cap, and by little


# ---- patch matrices --------------------------------------------------------------------------------------------------------
def q(t, dt):
    """the values the kernel sees: rounded to `dt`, as fp32"""
    return t.to(DT[dt]).float()


def unfold_img(img, p):
    """fp32 [B,C,S,S] -> [B P, C p^2]: row = b P + gy G + gx, column = c p^2 + ky p + kx"""
    B, C, S, _ = img.shape
    G = S // p
    return img.reshape(B, C, G, p, G, p).permute(0, 2, 4, 1, 3, 5).reshape(B * G * G, C * p * p).contiguous()


_DATA = {}


def dataset(C, S, n=NREC):
    """n random uint8 records [n,C,S,S], made once per geometry (numpy, never written to)"""
    if (C, S, n) not in _DATA:
        x = np.random.default_rng(1000 * C + S).integers(0, 256, size=(n, C, S, S), dtype=np.uint8)
        x.setflags(write=False)
        _DATA[(C, S, n)] = x
    return _DATA[(C, S, n)]


def u8_images(C, S, index=INDEX, pad=None, hflip=True, rng=(SEED, OFFSET), data=None):
    """fp32 [B,C,S,S] the gather leaves: pad None = no augmentation stream (the plain uint8 path)"""
    data = dataset(C, S) if data is None else data
    if pad is None:
        return torch.from_numpy(A.images(data, index, *STATS[C], (0, 0), 0, False))
    return torch.from_numpy(A.images(data, index, *STATS[C], rng, pad, hflip))


def u8_patches(C, S, p, **kw):
    return torch.from_numpy(A.unfold(u8_images(C, S, **kw).numpy(), p))


def draws(pad, B=len(INDEX), hflip=True, rng=(SEED, OFFSET)):
    return A.params(rng, B, pad, hflip)


def draws_cover(prm, pad):
    """a flipped and an unflipped slot, and a window that crosses each of the four borders"""
    oy, ox, fl = prm[:, 0], prm[:, 1], prm[:, 2]
    return bool(fl.min() == 0 and fl.max() == 1 and (oy < pad).any() and (oy > pad).any() and (ox < pad).any()
                and (ox > pad).any())


# ---- the reference ---------------------------------------------------------------------------------------------------------
def tokens_ref(dt, patches, w, bias, cls, ape):
    """float64 [B, P + 1, D] from the patch matrix [B, P, K] (rounded to `dt` here, as the kernel's is) and w rounded to
    `dt`; the class row is cls, which the position embedding skips; ape [P, D] or None"""
    B, P, _ = patches.shape
    D = w.shape[0]
    tok = q(patches, dt).double() @ q(w, dt).double().t() + bias.double()
    if ape is not None:
        tok = tok + ape.double()
    return torch.cat([cls.double().expand(B, 1, D), tok], 1)


def abs_terms(dt, patches, w, bias, ape):
    """float64 [B, P, D]: A = sum_k |x_k| |w_dk| + |bias_d| + |ape_nd| of every patch-row element"""
    a = q(patches, dt).double().abs() @ q(w, dt).double().abs().t() + bias.double().abs()
    return a + ape.double().abs() if ape is not None else a


def token_bound(dt, ref_rows, A_, K):
    """per-element gate of the patch rows (module docstring)"""
    b = (K + 4) * 2.0 ** -23 * A_
    return b + 2.0 ** -8 * ref_rows.abs() if dt == "bf16" else b


def excess(got_rows, ref_rows, bound):
    """worst |d| / bound over the elements (<= 1 passes); an element with bound 0 must be exact"""
    d = (got_rows.double() - ref_rows).abs()
    r = torch.where(bound > 0, d / bound.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, math.inf), torch.zeros_like(d)))
    return float(r.max())


def outside_rounding_interval(got_rows, ref_rows, bound32):
    """bf16 only: the number of stored elements that are NOT the bf16 rounding of any value within the fp32 bound of the
    reference.  Rounding is monotone, so a correct kernel stores RNE(ref - bound32) <= got <= RNE(ref + bound32); the ends
    are moved out by one fp32 ulp so that this function's own float64 -> fp32 -> bf16 conversion cannot cut the interval.
    Sharper than the 2^-8 |ref| term for elements far below the top of their binade."""
    inf = torch.tensor(math.inf)
    lo = torch.nextafter((ref_rows - bound32).float(), -inf).to(torch.bfloat16).double()
    hi = torch.nextafter((ref_rows + bound32).float(), inf).to(torch.bfloat16).double()
    g = got_rows.double()
    return int(((g < lo) | (g > hi)).sum())


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _seed(C, S, p, D):
    return ((C * 131 + S) * 131 + p) * 131 + D


def int_inputs(C, S, p, D, B=B_IMG):
    """The exact case.  w in {-1, 0, 1} with no two equal rows where 3^K >= D allows it (K = 4: no two equal (row, bias)
    pairs) and no two equal columns, so that a swapped or shifted operand index cannot cancel; bias, ape in [-8, 8], cls in
    [-100, 100], pixels in [-3, 3]."""
    _, P, K = geometry(C, S, p)
    g = _gen(_seed(C, S, p, D))
    img = torch.randint(-3, 4, (B, C, S, S), generator=g).float()
    nd = min(K, 8)                                            # the first nd columns carry a distinct base-3 code per row
    codes = torch.randperm(3 ** nd, generator=g)
    w = torch.randint(-1, 2, (D, K), generator=g)
    code = codes[torch.arange(D) % codes.numel()]
    for j in range(nd):
        w[:, j] = (code // 3 ** j) % 3 - 1
    bias = torch.randint(-8, 9, (D,), generator=g)
    for d in range(codes.numel(), D):                         # a repeated code (K = 4, D > 81) gets another bias
        bias[d] = (bias[d - codes.numel()] + 8 + 1) % 17 - 8
    ape = torch.randint(-8, 9, (P, D), generator=g).float()
    cls = torch.randint(-100, 101, (D,), generator=g).float()
    return img, w.float(), bias.float(), cls, ape


def real_inputs(dt, C, S, p, D, B=B_IMG):
    """images uniform in [-2, 2] (the range of normalised pixels), w ~ 0.3 N(0, 1) rounded to `dt`, bias, cls, ape ~ N(0, 1)"""
    _, P, K = geometry(C, S, p)
    g = _gen(_seed(C, S, p, D) + 1)
    img = torch.rand(B, C, S, S, generator=g) * 4 - 2
    w = q(torch.randn(D, K, generator=g) * 0.3, dt)
    bias, cls = torch.randn(D, generator=g), torch.randn(D, generator=g)
    ape = torch.randn(P, D, generator=g)
    return img, w, bias, cls, ape


# ---- seeded index bugs (test_embed_cpu.py: the inputs see them) --------------------------------------------------------------
def mutant_patches(img, p, bug):
    """the patch matrix a gather with one wrong index expression would build from fp32 images [B,C,S,S]"""
    B, C, S, _ = img.shape
    G = S // p
    x = img.reshape(B, C, G, p, G, p).permute(0, 2, 4, 1, 3, 5)         # b, gy, gx, c, ky, kx
    if bug == "kx_ky_swapped":
        return x.transpose(4, 5).reshape(B * G * G, C * p * p).contiguous()
    if bug == "channel_stride_p":                                         # k0 = ch p + ky p: channels overwrite each other
        out = torch.zeros(B * G * G, C * p * p)
        rows = x.reshape(B * G * G, C, p, p)
        for c in range(C):
            for ky in range(p):
                out[:, c * p + ky * p:c * p + ky * p + p] = rows[:, c, ky]
        return out
    if bug == "row_from_neighbour_patch":                                 # row ky = p - 1 comes from patch n + 1
        rows = x.reshape(B, G * G, C, p, p).clone()
        rows[:, :, :, p - 1] = torch.roll(rows, -1, 1)[:, :, :, p - 1]
        return rows.reshape(B * G * G, C * p * p)
    raise ValueError(bug)


def flip_without_crop_offset(C, S, pad, index=INDEX, rng=(SEED, OFFSET)):
    """fp32 images of a gather that forgets `+ ox - pad` in the flipped branch (sx = S - 1 - x)"""
    data, prm = dataset(C, S), draws(pad, len(index), True, rng)
    out = u8_images(C, S, index=index, pad=pad, rng=rng).clone()
    mean = np.asarray(STATS[C][0], np.float32).reshape(C, 1, 1)
    std = np.asarray(STATS[C][1], np.float32).reshape(C, 1, 1)
    for b, (oy, ox, fl) in enumerate(prm):
        if fl:
            padded = np.zeros((C, S + 2 * pad, S + 2 * pad), np.uint8)
            padded[:, pad:pad + S, pad:pad + S] = data[index[b]]
            win = padded[:, oy:oy + S, pad:pad + S][:, :, ::-1]
            out[b] = torch.from_numpy((win.astype(np.float32) / np.float32(255.0) - mean) / std)
    return out
