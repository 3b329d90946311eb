"""Float64 restatement of the classifier head and its loss (csrc/head.hip: head_fwd_kernel, ce_kernel, head_step_kernel,
head_bwd_rows_kernel, head_bwd_params_kernel), the input builders and the case lists.  Shared by
tests/test_head_loss_cpu.py (the reference against torch.nn.functional autograd and against closed forms; a plain fp32
restatement inside the gates) and tests/test_head_loss_gpu.py (the kernels against it).  No GPU and no vitpe import here.

    xhat   = (x[:, 0] - mean) / sqrt(var + eps)            (biased variance of the class row)
    logits = (xhat gamma + beta) Wh^T + bh
    loss   = loss_scale * sum_{b < n_valid} CE_b           CE_b = logsumexp(logits_b) - logits_b[label_b]
    correct= #{b < n_valid : first index of max(logits_b) == label_b}
    dlogits= (softmax(logits_b) - onehot(label_b)) * grad_scale  for b < n_valid, 0 for the padded rows
and the gradients of  sum(dlogits . logits)  w.r.t. the class row, Wh, bh, gamma and beta.

Gates (the project's: tests/test_kernels_gpu.py F32_TOL, test_head_ce_fwd_bwd):
    logits, dlogits, every fp32 gradient tensor    max|a - b| / max|b| < 1e-4, and the same per image row
    loss                                           |a - b| < 1e-5 max(1, |b|)
    correct count, padded dlogits rows             exact
    class row of dx, fp32                          max|a - b| / max|b| < 1e-4
    class row of dx, bf16                          |a - b| <= 2^-8 |b| + 1e-4 max|b| per element: the kernel computes the row in
                                                   fp32 (the 1e-4 term) and rounds it once to bf16 (8 significant bits:
                                                   at most 2^-8 of the value, reached only next to a power of two)
"""
import math

import numpy as np
import torch

TOL = 1e-4          # F32_TOL of tests/test_kernels_gpu.py
LOSS_TOL = 1e-5     # test_head_ce_fwd_bwd
WORLD = 4           # grad_scale = WORLD / n_global, loss_scale = 1 / n_global: what a 4-rank run puts into ctl
EPS_SWEEP = (1e-6, 1e-5, 1e-3)
DT = {"f32": torch.float32, "bf16": torch.bfloat16}

# head_step: (dtype, B, N, D, Cn, n_valid, eps).  KD = registers per lane (2: D <= 128, 3: <= 192, 6: <= 384, 12: <= 768);
# the head weight is staged in LDS when Cn D <= 12288 (WLDS), read from global memory otherwise.
HEAD_STEP_CASES = [
    # KD 2, WLDS
    ("f32", 1, 1, 64, 3, 1, 1e-6), ("bf16", 3, 17, 64, 3, 2, 1e-5),
    ("f32", 5, 17, 96, 9, 0, 1e-3), ("bf16", 257, 1, 96, 9, 256, 1e-6),
    ("f32", 3, 17, 128, 8, 3, 1e-5), ("bf16", 5, 1, 128, 8, 1, 1e-3),
    # KD 3, WLDS
    ("f32", 257, 17, 160, 10, 257, 1e-6), ("bf16", 3, 17, 160, 10, 0, 1e-5),
    ("f32", 5, 17, 192, 64, 4, 1e-3), ("bf16", 5, 17, 192, 64, 5, 1e-6),
    # KD 6, WLDS
    ("f32", 3, 1, 288, 16, 1, 1e-5), ("bf16", 257, 17, 288, 16, 256, 1e-3),
    ("f32", 5, 17, 384, 17, 5, 1e-6), ("bf16", 1, 17, 384, 17, 1, 1e-5),
    # KD 12, WLDS (Cn D <= 12288)
    ("f32", 3, 17, 576, 10, 2, 1e-3), ("bf16", 5, 17, 576, 10, 4, 1e-6),
    ("f32", 5, 1, 768, 16, 1, 1e-5), ("bf16", 3, 17, 768, 16, 3, 1e-3),
    # KD 12, weight from global memory
    ("f32", 5, 17, 768, 17, 4, 1e-6), ("bf16", 5, 17, 768, 17, 4, 1e-5),
    # KD 6, weight from global memory
    ("f32", 257, 17, 384, 64, 256, 1e-3), ("bf16", 3, 1, 384, 64, 2, 1e-6),
    ("f32", 3, 17, 200, 62, 2, 1e-5), ("bf16", 5, 17, 200, 62, 5, 1e-3),
    # a single class
    ("f32", 5, 17, 192, 1, 4, 1e-6), ("bf16", 3, 17, 192, 1, 3, 1e-5), ("f32", 1, 1, 768, 1, 0, 1e-3),
]

# head_fwd + cross_entropy + head_bwd: (dtype, B, N, D, Cn, eps)
HEAD_FWD_BWD_CASES = [
    ("f32", 4100, 2, 64, 3, 1e-6), ("bf16", 4100, 2, 64, 3, 1e-3),     # more than 1024 workgroups of 4 images: grid stride
    ("f32", 6, 1, 192, 10, 1e-5), ("bf16", 6, 1, 192, 10, 1e-6),       # a single token
    ("bf16", 6, 3, 100, 5, 1e-3),                                      # D % 8 != 0: the scalar zero fill of rows 1..
    ("f32", 8, 2, 1024, 1000, 1e-6), ("bf16", 8, 2, 1024, 1000, 1e-5),
]

# cross_entropy: (B, Cn); the largest B only at Cn <= 10
CE_CASES = [(1, 1), (1, 1000), (255, 2), (256, 10), (257, 100), (600, 1000), (600, 10), (600, 1), (4100, 1), (4100, 2),
            (4100, 10)]


def head_step_instance(D, Cn):
    """(KD, WLDS) of head_step_kernel that vitpe_head_step launches for this head (csrc/head.hip: head_step_launch)."""
    kd = (D + 63) // 64
    return (2 if kd <= 2 else 3 if kd == 3 else 6 if kd <= 6 else 12), Cn * D <= 16 * 768


def f32(v):
    """The fp32 value of a scalar the device reads from a float32 tensor, as a Python float."""
    return float(np.float32(v))


def scales(B, n_valid):
    """(grad_scale, loss_scale, n_global) as fp32 values: this rank holds n_valid of the n_global images of the step."""
    n_global = n_valid + WORLD * B - B
    return f32(WORLD / n_global), f32(1.0 / n_global), n_global


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def small_variance_rows(M, D, eps, seed):
    """[M, D] fp32 rows whose variance is comparable to eps (eps / 4 .. 4 eps before rounding) and whose mean is of the
    order of their standard deviation (0.5 .. 1.5 sigma, either sign)."""
    g = _gen(seed)
    sigma = math.sqrt(eps) * 2.0 ** (torch.rand(M, 1, generator=g, dtype=torch.float64) * 2 - 1)
    z = torch.randn(M, D, generator=g, dtype=torch.float64)
    z = (z - z.mean(1, keepdim=True)) / z.std(1, unbiased=False, keepdim=True)
    sign = torch.where(torch.rand(M, 1, generator=g) < 0.5, -1.0, 1.0).double()
    mean = sign * sigma * (0.5 + torch.rand(M, 1, generator=g, dtype=torch.float64))
    return (mean + sigma * z).float()


def variance_condition(rows, eps):
    """Fraction of the rows (float64 statistics of the values given) whose variance v has eps / 8 <= v <= 8 eps."""
    v = rows.double().var(-1, unbiased=False).reshape(-1)
    return float(((v >= eps / 8) & (v <= 8 * eps)).double().mean())


def head_inputs(dt, B, N, D, Cn, eps, seed=0):
    """x [B, N, D] (fp32 values exactly representable in `dt`), gamma, beta, Wh, bh (fp32), labels (int64).  The class rows
    have small variance (small_variance_rows); the other tokens are of order one.  Labels hit class 0 and class Cn - 1."""
    g = _gen(1000 + seed)
    x = torch.rand(B, N, D, generator=g) * 2 - 1
    x[:, 0] = small_variance_rows(B, D, eps, 2000 + seed)
    x = x.to(DT[dt]).float()
    gamma = 1 + 0.2 * (torch.rand(D, generator=g) * 2 - 1)
    beta = 0.2 * (torch.rand(D, generator=g) * 2 - 1)
    wh = 0.3 * (torch.rand(Cn, D, generator=g) * 2 - 1)
    bh = 0.5 * (torch.rand(Cn, generator=g) * 2 - 1)
    bh = bh + 0.25 * torch.sign(bh)                       # no logit row sits next to zero by construction
    labels = torch.randint(0, Cn, (B,), generator=g)
    labels[-1] = Cn - 1
    if B > 1:
        labels[0] = 0
    return x, gamma, beta, wh, bh, labels


def first_argmax(z):
    """First index of the maximum of every row (torch.max / the kernels' semantics), written out."""
    m = z.max(1, keepdim=True).values
    idx = torch.arange(z.shape[1]).expand_as(z)
    return torch.where(z == m, idx, torch.full_like(idx, z.shape[1])).min(1).values


def ce_ref(logits, labels, n_valid, grad_scale, loss_scale, dtype=torch.float64):
    """-> dict(loss, correct, dlogits) of the loss kernel's contract on given logits."""
    z = logits.to(dtype)
    B, Cn = z.shape
    valid = torch.arange(B) < n_valid
    m = z.max(1, keepdim=True).values
    e = torch.exp(z - m)
    se = e.sum(1, keepdim=True)
    ce = (m + torch.log(se)).squeeze(1) - z.gather(1, labels[:, None]).squeeze(1)
    onehot = torch.zeros_like(z).scatter_(1, labels[:, None], 1.0)
    dlogits = torch.where(valid[:, None], (e / se - onehot) * grad_scale, torch.zeros_like(z))
    return dict(loss=float((ce * valid).sum() * loss_scale), dlogits=dlogits,
                correct=int(((first_argmax(z) == labels) & valid).sum()))


def head_ref(x, gamma, beta, wh, bh, labels, eps, n_valid, grad_scale, loss_scale, dtype=torch.float64):
    """The whole head in `dtype` (float64: the reference; float32: the plain restatement the CPU test holds against it).
    x: [B, N, D] or the class rows [B, D].  -> dict of tensors / numbers (see the module docstring)."""
    xc = (x[:, 0] if x.dim() == 3 else x).to(dtype)
    gamma, beta, wh, bh = (t.to(dtype) for t in (gamma, beta, wh, bh))
    mean = xc.mean(1, keepdim=True)
    var = ((xc - mean) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = (xc - mean) * rstd
    yn = xhat * gamma + beta
    logits = yn @ wh.t() + bh
    out = ce_ref(logits, labels, n_valid, grad_scale, loss_scale, dtype)
    dl = out["dlogits"]
    dyn = dl @ wh
    gy = dyn * gamma
    out.update(logits=logits, rstd=rstd.squeeze(1), mean=mean.squeeze(1), var=var.squeeze(1),
               dx=rstd * (gy - gy.mean(1, keepdim=True) - xhat * (gy * xhat).mean(1, keepdim=True)),
               dwh=dl.t() @ yn, dbh=dl.sum(0), dgamma=(dyn * xhat).sum(0), dbeta=dyn.sum(0))
    return out


def equal_rows_head(wh, bh):
    """The closed-form head: every row of Wh equal to its first, every bh equal: all logits of an image are the same
    number, so CE_b = log(Cn), the arg-max is class 0 and dlogits = (1 / Cn - onehot) grad_scale."""
    return wh[:1].expand_as(wh).contiguous(), bh[:1].expand_as(bh).contiguous()


# ---- error figures ----------------------------------------------------------------------------------------------------
def rel(a, b):
    """max|a - b| / max|b|; 0 when both are identically zero, inf when only the reference is."""
    a, b = a.double(), b.double()
    if a.numel() == 0:
        return 0.0
    num, den = float((a - b).abs().max()), float(b.abs().max())
    return num / den if den > 0 else (0.0 if num == 0 else math.inf)


def row_rel(a, b):
    """The worst per-row rel: a wrong image must not hide behind a larger one."""
    a, b = a.double(), b.double()
    num, den = (a - b).abs().max(1).values, b.abs().max(1).values
    r = torch.where(den > 0, num / den.clamp_min(1e-300), torch.where(num == 0, 0.0, math.inf).double())
    return float(r.max()) if r.numel() else 0.0


def loss_err(a, b):
    """|a - b| / max(1, |b|): gate LOSS_TOL."""
    return abs(float(a) - float(b)) / max(1.0, abs(float(b)))


def dx_bf16_excess(got, ref):
    """max over elements of |got - ref| / (2^-8 |ref| + 1e-4 max|ref|): the bf16 class-row bound holds iff <= 1 (0 for an
    identically zero reference that is met exactly)."""
    got, ref = got.double(), ref.double()
    bound = 2.0 ** -8 * ref.abs() + TOL * ref.abs().max()
    d = (got - ref).abs()
    if float(bound.max()) == 0.0:
        return 0.0 if float(d.max()) == 0.0 else math.inf
    return float((d / bound.clamp_min(1e-300)).max())


def tied_logits(B, Cn, seed=0):
    """Logits on the grid 2^-10 in (-3, 3) (so that z + 100 is exact in fp32; the gaps stay below 5, so no softmax row
    saturates: softmax - onehot of a saturated row cancels in fp32 and its per-row error says nothing about the kernel) and
    labels, with exact ties at the row maximum
    (needs Cn >= 2): rows 0, 4, .. tie the label with a LATER class (first index wins: correct), rows 1, 5, .. tie an
    EARLIER class with the label (the earlier one wins: wrong), rows 2, 6, .. tie two other classes around the label when
    there is room, rows 3, 7, .. are left alone."""
    g = _gen(3000 + seed)
    z = torch.round(torch.randn(B, Cn, generator=g).clamp(-2.5, 2.5) * 0.8 * 1024) / 1024
    labels = torch.randint(0, Cn, (B,), generator=g)
    if Cn >= 2:
        for b in range(B):
            kind, top = b % 4, float(z[b].max()) + 0.5
            y = int(labels[b])
            if kind == 0:
                y = min(y, Cn - 2)
                labels[b] = y
                z[b, y] = z[b, Cn - 1 if b % 8 == 0 else y + 1] = top
            elif kind == 1:
                y = max(y, 1)
                labels[b] = y
                z[b, y] = z[b, 0 if b % 8 == 1 else y - 1] = top
            elif kind == 2 and Cn >= 3:
                y = min(max(y, 1), Cn - 2)
                labels[b] = y
                z[b, y - 1] = z[b, y + 1] = top
    return z, labels
