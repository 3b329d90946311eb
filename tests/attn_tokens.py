"""Attention inputs at every token count the kernels accept, not only N = G^2 + 1.

The attention kernels work on 16-token tiles and are compiled for MT = 2, 4, 5, 10, 13, 17 tiles, so the support queries
accept whole ranges of N (17-32, 49-64, 65-80, 145-160, 193-208, 257-272).  This module builds the cases the token-count
tests (test_token_counts_cpu.py, test_token_counts_gpu.py) share:

  * token_case   -- attn_case (test_kernels_gpu.py) with N given instead of derived from a grid;
  * masked_case  -- inputs on which a wrong decision about the last tile is an order-one error under the suite's
                    rel_err = max|a - b| / max|b| (on random inputs one admitted padding key is a ~1/N dilution, far
                    below the bf16 gate);
  * ref_attention -- a plain torch restatement of oracle.vit_oracle.attention_core on a [B, N, 3D] projection, with the
                    masking defects the CPU test simulates;
  * guarded_input / guarded_output / row checks for the GPU tests.

How masked_case works (q, k, v = x W^T per head, all values below exactly representable in bf16):
  * x[..., 0] = 1 and, in every head, the q row of feature F0 has the single weight +c and the k row the single weight
    -c: every real logit is shifted by -c^2 hd^-0.5 (about -17), identically for all keys, so it cancels in the softmax;
    a zero padding key stays at logit 0 and takes the whole row if it is admitted;
  * x[..., 1] marks the query rows {0, N - 1} ({N - 1} in relative mode), x[..., 2] marks row N - 1: feature F1 of q and k
    gets the weight d on those columns, which makes key N - 1 the dominant key (+d^2 hd^-0.5, about +25 ... +37) of those
    queries; every v feature is offset by +2 at every token but N - 1, where it is offset by -2: a key mask that stops
    one short replaces those output rows, an admitted zero row pulls every other output row from about 2 to 0;
  * relative mode: table[:, 0] (pair i = 0, j = N - 1) = 48 makes key N - 1 the dominant key of query 0 through the table
    alone, table[:, 2N - 2] (pair i = N - 1, j = 0) = 64 makes key 0 beat key N - 1 for query N - 1: a table index that is
    off by one in either direction moves row 0 or row N - 1;
  * rope modes: F0 = 0 and F1 = hd / 4 are left unrotated (their frequencies are set to zero), so that the shifts stay
    the same for every key.
"""
import math

import numpy as np
import torch

from conftest import rel_err
from oracle import vit_oracle as O
from test_kernels_gpu import DT, attn_case, q, rnd, tol  # noqa: F401  (re-exported for the two test files)

# tile count -> the new token counts: first, middle(s), last but one, full (17, 50, 65, 145, 197, 257 are covered elsewhere)
TOKEN_COUNTS = {2: (18, 24, 26, 31, 32), 4: (49, 56, 63, 64), 5: (66, 72, 79, 80), 10: (146, 152, 159, 160),
                13: (193, 198, 200, 207, 208), 17: (258, 264, 271, 272)}
ALL_COUNTS = tuple(n for mt in sorted(TOKEN_COUNTS) for n in TOKEN_COUNTS[mt])
MIDDLE_AND_FULL = {2: (24, 32), 4: (56, 64), 5: (72, 80), 10: (152, 160), 13: (200, 208), 17: (264, 272)}
ANY_N_MODES = ("none", "relative")
TABLE_LO, TABLE_HI = 48.0, 64.0


def is_square(n):
    return math.isqrt(n) ** 2 == n


def token_case(mode, N, D, H, B, seed=0):
    """attn_case with N given: (N, hd, G, xn, wqkv, dout, pe).  none / relative at any N; the grid modes need N - 1 square."""
    G = math.isqrt(N - 1)
    if mode not in ANY_N_MODES:
        assert is_square(N - 1), (mode, N)
        return attn_case(mode, D, H, B, seed=seed, G=G)
    hd = D // H
    xn = rnd(B, N, D, seed=seed + 1)
    wqkv = rnd(3 * D, D, seed=seed + 2, scale=0.3)
    dout = rnd(B, N, D, seed=seed + 3)
    pe = {"table": rnd(H, 2 * N - 1, seed=seed + 4, scale=0.5)} if mode == "relative" else {}
    return N, hd, G, xn, wqkv, dout, pe


def mask_consts(hd):
    """(c, d, F0, F1): c^2 hd^-0.5 ~ 17 (integers are exact in bf16), d^2 hd^-0.5 in 25 ... 37."""
    c = math.ceil(math.sqrt(16.0 * math.sqrt(hd)))
    d = 12 if hd <= 32 else 16
    return float(c), float(d), 0, hd // 4


def masked_case(mode, N, D, H, B, seed=0):
    """The mask-sensitive case in (x, W) form, same tuple as token_case; the qkv-buffer kernels take core_qkv(xn, wqkv)."""
    N, hd, G, xn, wqkv, dout, pe = token_case(mode, N, D, H, B, seed=seed)
    c, d, F0, F1 = mask_consts(hd)
    xn, wqkv, dout = xn.clone(), wqkv.clone(), dout.clone()
    if mode == "relative":                      # an index off by one moves rows 0 / N - 1 only: they weigh 4 x in d qkv
        dout[:, [0, N - 1]] *= 4.0
    xn[..., 0] = 1.0
    xn[..., 1:3] = 0.0
    xn[:, N - 1, 1:3] = 1.0
    if mode != "relative":
        xn[:, 0, 1] = 1.0
    wqkv[:, 0:3] = 0.0
    wqkv[2 * D:, 0] = 2.0                       # every v feature: +2 at every token, -2 at token N - 1
    wqkv[2 * D:, 2] = -4.0
    for h in range(H):
        for mat, f, col, val in ((0, F0, 0, c), (1, F0, 0, -c), (0, F1, 1, d), (1, F1, 2, d)):
            wqkv[mat * D + h * hd + f] = 0.0
            wqkv[mat * D + h * hd + f, col] = val
    if mode == "relative":
        pe["table"] = pe["table"].clone()
        pe["table"][:, 0] = TABLE_LO
        pe["table"][:, 2 * N - 2] = TABLE_HI
    elif mode == "rope-axial":
        pe["inv_freq"] = pe["inv_freq"].clone()
        pe["inv_freq"][0] = 0.0                 # pairs 0 (x phase) and hd / 4 (y phase) are not rotated
    elif mode == "rope-mixed":
        pe["freqs"] = pe["freqs"].clone()
        pe["freqs"][:, :, [F0, F1]] = 0.0
    return N, hd, G, xn, wqkv, dout, pe


def masked_layernorm(D, seed=0):
    """(gamma, beta) that keep the logit shift of masked_case through a LayerNorm: column 0 of LayerNorm(x) is exactly 1,
    columns 1 and 2 exactly 0 (the dominant-key part of the construction does not pass a LayerNorm)."""
    gamma, beta = 1 + 0.1 * rnd(D, seed=seed + 5), 0.1 * rnd(D, seed=seed + 6)
    gamma[0:3] = 0.0
    beta[0], beta[1], beta[2] = 1.0, 0.0, 0.0
    return gamma, beta


# ------------------------------------------------------------------------------------------ reference with defects
DEFECTS = ("pad_key", "drop_last_key", "index+1", "index-1")


def ref_attention(qkv, H, mode, pe, defect=None):
    """O.attention_core restated on a projection qkv [B, N, 3D] (any float dtype) -> merged heads [B, N, D].
    pe: the leaves of the positional encoding (table / coeff / inv_freq / freqs), differentiable.
    defect: None, or one of DEFECTS --
      pad_key        one zero key / value row past N admitted to the softmax, its bias read at the clamped table index
                     (the additive bias of the other modes is zero there, a zero key stays zero under rotation);
      drop_last_key  key N - 1 masked out;
      index+1 / -1   the relative-table index shifted by one before the clamp."""
    B, N, D3 = qkv.shape
    D = D3 // 3
    hd = D // H
    qq, kk, vv = qkv.reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    if mode.startswith("rope"):
        if mode == "rope-axial":
            cos, sin = O.rope_axial_tables(N - 1, pe["inv_freq"])
        else:
            cos, sin = O.rope_mixed_tables(N - 1, pe["freqs"])
        cos, sin = cos.to(qkv.dtype), sin.to(qkv.dtype)
        cos, sin = (cos[None, None], sin[None, None]) if cos.dim() == 2 else (cos[None], sin[None])
        h2 = hd // 2

        def rot(t):
            t1, t2 = t[:, :, 1:, :h2], t[:, :, 1:, h2:]
            return torch.cat([t[:, :, :1], torch.cat([t1 * cos - t2 * sin, t1 * sin + t2 * cos], dim=-1)], dim=2)
        qq, kk = rot(qq), rot(kk)
    nk = N + 1 if defect == "pad_key" else N
    if defect == "pad_key":
        kk = torch.cat([kk, torch.zeros_like(kk[:, :, :1])], dim=2)
        vv = torch.cat([vv, torch.zeros_like(vv[:, :, :1])], dim=2)
    s = (qq @ kk.transpose(-2, -1)) * hd ** -0.5
    if mode == "relative":
        idx = torch.arange(N)[:, None] - torch.arange(nk)[None, :] + N - 1
        idx = idx + {"index+1": 1, "index-1": -1}.get(defect, 0)
        s = s + pe["table"].to(qkv.dtype)[:, idx.clamp(0, 2 * N - 2)]
    elif mode.startswith("polynomial"):
        bias = O.polynomial_bias(pe["coeff"], N - 1, H, 3, mode == "polynomial").to(qkv.dtype)
        if defect == "pad_key":
            bias = torch.cat([bias, torch.zeros_like(bias[:, :, :1])], dim=2)
        s = s + bias
    if defect == "drop_last_key":
        s = torch.cat([s[..., :N - 1], torch.full_like(s[..., :1], float("-inf"))], dim=-1)
    o = s.softmax(dim=-1) @ vv
    return o.transpose(1, 2).reshape(B, N, D)


def ref_fwd_bwd(mode, xn, wqkv, dout, pe, H, dt="f32", defect=None, dtype=torch.float32, round_qkv=False):
    """oracle_attn (test_kernels_gpu.py) through ref_attention: (out, dqkv, PE-leaf gradients).  dt: the operand
    rounding of the kernel's inputs; dtype: the arithmetic; round_qkv: q / k / v rounded to bf16 after the projection."""
    leaves = {k: v.clone().to(dtype if k != "inv_freq" else v.dtype).requires_grad_(k != "inv_freq") for k, v in pe.items()}
    qkv = torch.nn.functional.linear(q(xn, dt).to(dtype), q(wqkv, dt).to(dtype))
    if round_qkv:
        qkv = qkv.bfloat16().to(dtype)
    qkv = qkv.detach().requires_grad_(True)
    out = ref_attention(qkv, H, mode, leaves, defect)
    out.backward(q(dout, dt).to(dtype))
    return out.detach(), qkv.grad, {k: v.grad for k, v in leaves.items() if v.requires_grad}


# ------------------------------------------------------------------------------------------ geometry lists
def core_geoms():
    """(mode, N, hd) of the attention-core cases: every new N x {none, relative} at hd 32 / 64, all six head dimensions at
    a middle and the full count of every tile count, N = 26 in the four grid modes."""
    g = [(m, n, hd) for n in ALL_COUNTS for m in ANY_N_MODES for hd in (32, 64)]
    g += [(m, n, hd) for mt in sorted(MIDDLE_AND_FULL) for n in MIDDLE_AND_FULL[mt] for m in ANY_N_MODES
          for hd in (24, 48, 96, 128)]
    g += [(m, 26, hd) for m in ("polynomial", "polynomial_perhead", "rope-axial", "rope-mixed") for hd in (32, 64)]
    return g


FUSED_GEOMS = [(m, n, D) for n in TOKEN_COUNTS[5] for m in ANY_N_MODES for D in (192, 96)]          # hd 32
FUSED64_GEOMS = [(m, n) for n in TOKEN_COUNTS[13] for m in ANY_N_MODES]                             # D 128, H 2
WIDE_MODES = ("none", "relative", "polynomial", "polynomial_perhead", "rope-axial", "rope-mixed")   # N 65, D 192, H 6


def masked_geoms():
    """every (mode, N, D, H) a GPU test runs masked_case on"""
    g = {(m, n, 2 * hd, 2) for m, n, hd in core_geoms()}
    g |= {(m, n, D, D // 32) for m, n, D in FUSED_GEOMS}
    g |= {(m, n, 128, 2) for m, n in FUSED64_GEOMS}
    g |= {(m, 65, 192, 6) for m in WIDE_MODES}
    return sorted(g)


# ------------------------------------------------------------------------------------------ GPU-side helpers
def guarded_input(t, rows=16):
    """t [..., R, C] on the device, followed in the same allocation by `rows` rows of NaN: a read past the last image's
    rows that is not zeroed turns that image's result non-finite."""
    t = t.contiguous()
    n, c = t.numel(), t.shape[-1]
    buf = torch.full((n + rows * c,), float("nan"), device=t.device, dtype=t.dtype)
    buf[:n] = t.reshape(-1)
    return buf[:n].view(t.shape)


class Guarded:
    """a NaN-prefilled output of `shape` followed by `rows` rows of NaN guard"""

    def __init__(self, shape, dtype, rows=16):
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + rows * shape[-1],), float("nan"), device="cuda", dtype=dtype)
        self.t = self.buf[:self.n].view(*shape)

    def check(self, what=""):
        assert torch.isnan(self.buf[self.n:]).all(), f"{what}: written past the end"
        assert torch.isfinite(self.t).all(), f"{what}: a row was not written, or is not finite"
        return self.t.clone()


def edge_rows(N):
    mt = (N + 15) // 16
    return sorted({r for r in (0, 1, 15, 16, 16 * (mt - 1) - 1, 16 * (mt - 1), N - 2, N - 1) if 0 <= r < N})


def worst_row_err(a, b, N):
    """max over the edge rows of rel_err restricted to that token row (all images)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return max(rel_err(a[:, r], b[:, r]) for r in edge_rows(N))
