"""float64 references of the attention statistics (vitpe_attention_core_stats) and of attention rollout, on probabilities
p [B, H, N, N] such as ref_probs (test_attn_probs_cpu.py) returns for a float64 projection.

Token t >= 1 sits at (y, x) = ((t - 1) // G, (t - 1) % G) for every N (the raster may be ragged).  Slots of the result, in
the order of include/vitpe.h (VITPE_STAT_*):
  0 distance     unit / P . sum_{i>=1} sum_{j>=1} p_ij sqrt((y_i - y_j)^2 + (x_i - x_j)^2)      (P = N - 1, not renormalised)
  1 entropy      1 / N . sum_i (- sum_j p_ij ln p_ij)                                            (nats, 0 ln 0 = 0)
  2 class mass   1 / P . sum_{i>=1} p_i0
  3 class entropy  - sum_j p_0j ln p_0j
"""
import torch

DISTANCE, ENTROPY, CLS_MASS, CLS_ENTROPY = range(4)
SLOTS = ("distance", "entropy", "cls_mass", "cls_entropy")


def grid_distances(N, G):
    """[P, P] float64: Euclidean distance of patch tokens 1 .. N - 1 on the G-wide raster"""
    t = torch.arange(N - 1)
    y, x = (t // G).double(), (t % G).double()
    return ((y[:, None] - y[None, :]) ** 2 + (x[:, None] - x[None, :]) ** 2).sqrt()


def ref_stats(p, G, unit=1.0):
    """p [B, H, N, N] -> float64 [B, H, 4]"""
    p = p.double()
    N = p.shape[-1]
    P = N - 1
    dist = unit / P * (p[..., 1:, 1:] * grid_distances(N, G)).sum((-1, -2))
    row_ent = -torch.xlogy(p, p).sum(-1)                     # [B, H, N]; xlogy(0, 0) = 0
    return torch.stack([dist, row_ent.mean(-1), p[..., 1:, 0].sum(-1) / P, row_ent[..., 0]], dim=-1)


def ref_colsum(p, w):
    """p [B, H, N, N], w [B, N] -> float64 [B, H, N]: sum_i w[b, i] p[b, h, i, j]"""
    return torch.einsum("bi,bhij->bhj", w.double(), p.double())


def rollout_matrix(a, residual):
    """A^ = (1 - residual) mean_h A + residual I of one layer's maps a [B, H, N, N] -> float64 [B, N, N]"""
    a = a.double().mean(1)
    return (1.0 - residual) * a + residual * torch.eye(a.shape[-1], dtype=torch.float64)


def ref_rollout(maps, start=0, residual=0.5):
    """maps: the layers' probabilities [B, H, N, N], bottom block first -> float64 [B, N]: the class token's row of
    A^_{L-1} ... A^_{start}, propagated as a row vector from the top block down."""
    B, _, N, _ = maps[0].shape
    v = torch.zeros(B, N, dtype=torch.float64)
    v[:, 0] = 1.0
    for a in reversed(maps[start:]):
        v = torch.einsum("bi,bij->bj", v, rollout_matrix(a, residual))
    return v


def shifted_identity(N, delta):
    """[N, N] float64: row i puts all its mass on key i + delta where that key exists, on itself otherwise"""
    p = torch.zeros(N, N, dtype=torch.float64)
    for i in range(N):
        j = i + delta
        p[i, j if 0 <= j < N else i] = 1.0
    return p
