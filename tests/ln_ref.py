"""Input builders and the float64 reference for the tests of LayerNorm's eps and row statistics.  Every entry point that
forms rstd = 1 / sqrt(var + eps) is driven with rows whose variance v is COMPARABLE to the eps passed (eps / 8 <= v <= 8 eps
for >= 90 % of the rows, asserted on the reference) and whose mean is of the order of their standard deviation, with
non-default eps values: at the suite's usual variance of 0.3 .. 1.3 a missing, misplaced or swapped eps moves every output
by ~1e-5, below the fp32 gate.  Shared by tests/test_ln_eps_cpu.py (the inputs discriminate: the wrong eps moves the
outputs by >= 100x the gate; a plain fp32 / bf16-rounding restatement stays inside the gates) and tests/test_ln_eps_gpu.py
(the kernels against the reference).  No GPU and no vitpe import here.

Statistics: every producer documents that it takes mean / rstd "of the values as stored" (two-pass, after rounding to the
tensor's type), so their reference is the float64 statistics of the rows the kernel itself stored, read back.  Gate, both
dtypes:  |mean - ref| <= 1e-4 max|row|  and  |rstd / ref - 1| <= 1e-4  per row; a two-pass fp32 reduction over D <= 1024
elements is bounded by (D + 4) 2^-24 < 6.2e-5.  Normalised outputs: the project's F32_TOL / BF16_TOL (test_kernels_gpu.py)
against the float64 chain from the (rounded) inputs.
"""
import math

import torch

from head_ref import DT, EPS_SWEEP, rel, small_variance_rows, variance_condition  # noqa: F401  (re-exported)

F32_TOL, BF16_TOL, STAT_TOL = 1e-4, 3e-2, 1e-4
POWER = 100          # the wrong eps must move an affected output by at least POWER x its gate ...
POWER_BF16 = 10      # ... except a bf16 normalised output (gate 3e-2: 100x would be a change of 300 %; test_ln_eps_cpu.py)

LAYERNORM_SHAPES = [(67, 96), (33, 768), (5, 1024)]
LINEAR_SHAPES = [(397, 192, 192), (130, 192, 96)]                   # N = 192: the statistics epilogue
TAIL2_CASES = [(13, 128, 1e-6, 1e-4), (265, 768, 1e-5, 1e-3)]       # (M, HID, eps2, eps_next), D = 192, bf16
TAIL_CLS_CASES = [(1, 128, 1e-6), (17, 128, 1e-3)]                  # (B, HID, eps2): the smallest hidden size of its shape test
PATCH_EMBED_CASES = [(1, 28, 4, 64, True), (3, 32, 4, 192, False)]  # (C, S, p, D, ape)


def tol(dt):
    return F32_TOL if dt == "f32" else BF16_TOL


def wrong_eps(eps):
    """What a kernel that ignores its argument would use: the 1e-5 default, or 0 where 1e-5 itself is passed."""
    return 1e-5 if eps != 1e-5 else 0.0


def q(t, dt):
    """the values the kernel sees: rounded to `dt`, as fp32"""
    return t.to(DT[dt]).float()


def _u(g, *shape):
    return torch.rand(*shape, generator=g) * 2 - 1


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def stats(rows, eps):
    """float64 (mean, var, rstd) of the rows given"""
    r = rows.double()
    mean = r.mean(-1)
    var = ((r - mean[..., None]) ** 2).mean(-1)
    return mean, var, 1.0 / torch.sqrt(var + eps)


def layer_norm(rows, gamma, beta, eps, dtype=torch.float64):
    r = rows.to(dtype)
    mean = r.mean(-1, keepdim=True)
    var = ((r - mean) ** 2).mean(-1, keepdim=True)
    return (r - mean) / torch.sqrt(var + eps) * gamma.to(dtype) + beta.to(dtype)


def stat_errors(mean, rstd, rows, eps):
    """(max over rows of |mean - ref| / max|row|, max |rstd / ref - 1|) against the float64 statistics of `rows`: gate
    STAT_TOL each."""
    m, _, r = stats(rows, eps)
    rowmax = rows.double().abs().amax(-1).clamp_min(1e-300)
    return (float(((mean.double().reshape(m.shape) - m).abs() / rowmax).max()),
            float((rstd.double().reshape(r.shape) / r - 1).abs().max()))


def mean_is_of_the_order_of_sigma(rows, frac=0.9):
    m, v, _ = stats(rows, 0.0)
    s = v.sqrt()
    return float(((m.abs() > 0.2 * s) & (m.abs() < 5 * s)).double().mean()) >= frac


# ---- vitpe_layernorm_fwd -----------------------------------------------------------------------------------------------
def layernorm_inputs(dt, M, D, eps, seed=0):
    g = _gen(10 + seed)
    return q(small_variance_rows(M, D, eps, 20 + seed), dt), 1 + 0.2 * _u(g, D), 0.2 * _u(g, D)


# ---- vitpe_linear with the statistics epilogue: C = A W^T + bias + R -----------------------------------------------------
def linear_inputs(dt, M, N, K, eps, seed=0):
    """W is scaled so that A W^T has a standard deviation of sqrt(eps / 2); the residual rows add eps / 2 and the mean."""
    g = _gen(30 + seed)
    a, w0 = q(_u(g, M, K), dt), _u(g, N, K)
    raw = a.double() @ w0.double().t()
    w = q(w0 * (math.sqrt(eps / 2) / float(raw.std())), dt)
    bias = 0.3 * math.sqrt(eps) * _u(g, N)
    resid = q(small_variance_rows(M, N, eps / 2, 40 + seed), dt)
    return a, w, bias, resid


def linear_ref(a, w, bias, resid):
    return a.double() @ w.double().t() + bias.double() + resid.double()


# ---- vitpe_block_tail2_fwd / vitpe_tail_cls_fwd (bf16, D = 192) -----------------------------------------------------------
TAIL_D = 192


def bf(t):
    return t.to(torch.bfloat16).to(t.dtype)


def tail2_inputs(M, HID, eps2, eps_next, seed=0):
    """x_mid = x_in + attn_out Wp^T + bp gets variance ~ eps2; out = x_mid + fc2(gelu(fc1(LN2 x_mid))) contains x_mid, so
    eps_next > eps2 and W2 / b2 are scaled for a variance ~ eps_next.  All tensors hold bf16-representable values except
    the fp32 biases and the LayerNorm weight."""
    D, g = TAIL_D, _gen(50 + seed)
    a_, x_in = bf(_u(g, M, D)), bf(small_variance_rows(M, D, eps2 / 2, 60 + seed))
    wp0 = _u(g, D, D)
    wp = bf(wp0 * (math.sqrt(eps2 / 2) / float((a_.double() @ wp0.double().t()).std())))
    bp = 0.3 * math.sqrt(eps2) * _u(g, D)
    gam, bet = 1 + 0.2 * _u(g, D), 0.2 * _u(g, D)
    w1, b1 = bf(0.08 * _u(g, HID, D)), 0.1 * _u(g, HID)
    w20 = _u(g, D, HID)
    ins = dict(a=a_, x_in=x_in, wp=wp, bp=bp, gamma=gam, beta=bet, w1=w1, b1=b1, w2=w20, b2=torch.zeros(D))
    h = tail2_ref(ins, eps2, eps_next)["h"]
    ins["w2"] = bf(w20 * (math.sqrt(eps_next) / float((h @ w20.double().t()).std(1).median())))
    ins["b2"] = math.sqrt(eps_next) * (0.8 + 0.3 * _u(g, D))
    return ins


def tail2_ref(ins, eps2, eps_next, dtype=torch.float64, stored=None):
    """The block tail in `dtype`.  stored: a rounding applied where the kernel stores or re-reads a tensor in bf16 (x_mid, the
    normalised rows that feed fc1, the hidden activation, out) -- None for the float64 reference, `bf` for the restatement
    that shows what a correct bf16 kernel leaves.  Statistics are those of the (stored) rows."""
    st = stored or (lambda t: t)
    c = {k: v.to(dtype) for k, v in ins.items()}
    x_mid = st(c["x_in"] + c["a"] @ c["wp"].t() + c["bp"])
    xn = st(layer_norm(x_mid, c["gamma"], c["beta"], eps2, dtype))
    h = st(torch.nn.functional.gelu(xn @ c["w1"].t() + c["b1"]))
    out = st(x_mid + h @ c["w2"].t() + c["b2"])
    m2, _, r2 = stats(x_mid, eps2)
    mo, _, ro = stats(out, eps_next)
    return dict(x_mid=x_mid, xn=xn, h=h, out=out, mean2=m2, rstd2=r2, mean_out=mo, rstd_out=ro)


# ---- vitpe_patch_embed -----------------------------------------------------------------------------------------------------
def patch_embed_inputs(dt, C, S, p, D, ape, eps, B=3, seed=0):
    """Class-token row: cls itself (the absolute position embedding skips it), variance ~ eps.  Patch rows: W scaled so that
    patches W^T has variance eps / 2, the bias carries the mean and the rest of the variance."""
    g = _gen(70 + seed)
    P, Kk = (S // p) ** 2, C * p * p
    img = _u(g, B, C, S, S)
    w0 = _u(g, D, Kk)
    raw = unfold(q(img, dt), p).double() @ w0.double().t()
    w = q(w0 * (math.sqrt(eps / 2) / float(raw.std())), dt)
    bias = small_variance_rows(1, D, eps / 4, 80 + seed)[0]
    cls = small_variance_rows(1, D, eps, 90 + seed)[0]
    apet = 0.5 * math.sqrt(eps) * _u(g, P, D) if ape else None
    return img, w, bias, cls, apet


def unfold(img, p):
    """[B, C, S, S] -> [B, P, C p p]: the patch matrix of a stride-p convolution (channel, row, column order)"""
    return torch.nn.functional.unfold(img, p, stride=p).transpose(1, 2).contiguous()


def patch_embed_ref(dt, img, w, bias, cls, apet, p):
    """float64 tokens [B, P + 1, D]; the patches are rounded to `dt` as the kernel's patch matrix is."""
    tok = unfold(q(img, dt), p).double() @ w.double().t() + bias.double()
    if apet is not None:
        tok = tok + apet.double()
    B, D = img.shape[0], w.shape[0]
    return torch.cat([cls.double().expand(B, 1, D), tok], 1)
