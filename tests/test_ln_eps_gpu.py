"""LayerNorm's eps and the row statistics of every entry point that forms rstd = 1 / sqrt(var + eps), through the C ABI,
on rows whose variance is comparable to the eps passed and with non-default, mutually different eps values (the inputs,
the float64 reference and why they make eps visible: tests/ln_ref.py; that they do: tests/test_ln_eps_cpu.py).  The head's
two entry points get the same sweep in tests/test_head_loss_gpu.py.

Tolerances:
  mean / rstd   |mean - ref| <= 1e-4 max|row|, |rstd / ref - 1| <= 1e-4 per row, both dtypes, against the float64 statistics
                of the rows the kernel itself stored (read back): every producer documents statistics "of the values as
                stored", two-pass; a two-pass fp32 reduction over D <= 1024 elements is bounded by (D + 4) 2^-24 < 6.2e-5.
                This isolates the statistics from GEMM rounding.
  y, xn_out     the project's gates (test_kernels_gpu.py: F32_TOL 1e-4, BF16_TOL 3e-2, rel = max|a - b| / max|b|) against the
                float64 chain from the rounded inputs; the stored tensors x_mid / out / tokens / C at the same gates.
  bit-identity  vitpe_patch_embed_aug with rng = NULL against vitpe_patch_embed; block_tail2_fwd with save on against off.
"""
import pytest
import torch

import ln_ref as R
from parity_report import Report

pytestmark = pytest.mark.gpu
DT = R.DT
bf16 = torch.bfloat16


@pytest.fixture(scope="module")
def K():
    from vitpe import kernels
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return kernels


@pytest.fixture(scope="module")
def report():
    r = Report("test_ln_eps_gpu")
    yield r
    r.close()


def dev(t, dtype=None):
    t = t.cuda()
    return t.to(dtype).contiguous() if dtype is not None else t.contiguous()


def empty(*s):
    return torch.full(s, float("nan"), device="cuda")


def stat_figures(r, tag, mean, rstd, rows, eps):
    em, er = R.stat_errors(mean.cpu(), rstd.cpu(), rows.float().cpu(), eps)
    r.le(tag + "mean", em, R.STAT_TOL)
    r.le(tag + "rstd", er, R.STAT_TOL)


def bits_differ(a, b):
    v = torch.int16 if a.element_size() == 2 else torch.int32
    return int((a.contiguous().view(v) != b.contiguous().view(v)).sum())


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("eps", R.EPS_SWEEP)
@pytest.mark.parametrize("M,D", R.LAYERNORM_SHAPES)
def test_layernorm_fwd_eps_and_statistics(K, report, dt, eps, M, D):
    x, g, b = R.layernorm_inputs(dt, M, D, eps)
    assert R.variance_condition(x, eps) >= 0.9
    y, mean, rstd = K.layernorm_fwd(dev(x, DT[dt]), dev(g), dev(b), eps=eps)
    r = report.case("layernorm_fwd", f"{dt}-{eps}-{M}-{D}")
    r.lt(f"y_{dt}", R.rel(y.float().cpu(), R.layer_norm(x, g, b, eps)), R.tol(dt))
    stat_figures(r, "", mean, rstd, x, eps)
    _, m2, r2 = K.layernorm_fwd(dev(x, DT[dt]), dev(g), dev(b), eps=eps, stats_only=True)
    r.eq("stats_only_differs", bits_differ(m2, mean) + bits_differ(r2, rstd), 0)
    r.done()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("eps", R.EPS_SWEEP)
@pytest.mark.parametrize("M,N,K_", R.LINEAR_SHAPES)
def test_linear_statistics_epilogue_eps(K, report, dt, eps, M, N, K_):
    from vitpe import _lib as L
    a, w, bias, resid = R.linear_inputs(dt, M, N, K_, eps)
    mean, rstd = empty(M), empty(M)
    c = K.linear(dev(a, DT[dt]), dev(w, DT[dt]), dev(bias), epi=L.EPI_BIAS_RESID, resid=dev(resid, DT[dt]),
                 stats=(mean, rstd), eps=eps)
    r = report.case("linear_stats", f"{dt}-{eps}-{M}-{N}-{K_}")
    assert R.variance_condition(c.float().cpu(), eps) >= 0.9
    r.lt(f"c_{dt}", R.rel(c.float().cpu(), R.linear_ref(a, w, bias, resid)), R.tol(dt))
    stat_figures(r, "", mean, rstd, c, eps)
    r.done()


def tail_operands(K, ins):
    pk = (K.pack_weight_frags(dev(ins["wp"]), bf16, 192, 0), K.pack_weight_frags(dev(ins["w1"]), bf16, 192, 1),
          K.pack_weight_frags(dev(ins["w2"]), bf16, 32, 1))
    return pk[0], dev(ins["bp"]), dev(ins["gamma"]), dev(ins["beta"]), pk[1], dev(ins["b1"]), pk[2], dev(ins["b2"])


@pytest.mark.parametrize("M,HID,eps2,eps_next", R.TAIL2_CASES)
def test_block_tail2_fwd_two_eps(K, report, M, HID, eps2, eps_next):
    D = R.TAIL_D
    assert K.block_tail2_supported(bf16, D, HID)
    ins = R.tail2_inputs(M, HID, eps2, eps_next)
    ref = R.tail2_ref(ins, eps2, eps_next)
    ops = tail_operands(K, ins)
    r = report.case("block_tail2_fwd", f"{M}-{HID}-{eps2}-{eps_next}")
    got = {}
    for save in (True, False):
        mo, ro = empty(M), empty(M)
        xn = torch.empty(M, D, device="cuda", dtype=bf16)
        out, x_mid, m2, r2, gp, h = K.block_tail2_fwd(dev(ins["a"], bf16), dev(ins["x_in"], bf16), *ops, xn_out=xn,
                                                     stats=(mo, ro), eps2=eps2, eps_next=eps_next, save=save)
        torch.cuda.synchronize()
        assert (h is not None) == save
        got[save] = dict(out=out, x_mid=x_mid, mean2=m2, rstd2=r2, xn=xn, mean_out=mo, rstd_out=ro)
    g = got[True]
    assert R.variance_condition(g["x_mid"].float().cpu(), eps2) >= 0.9
    assert R.variance_condition(g["out"].float().cpu(), eps_next) >= 0.9
    for k in ("x_mid", "xn", "out"):
        r.lt(k, R.rel(g[k].float().cpu(), ref[k]), R.BF16_TOL)
    stat_figures(r, "ln2_", g["mean2"], g["rstd2"], g["x_mid"], eps2)
    stat_figures(r, "next_", g["mean_out"], g["rstd_out"], g["out"], eps_next)
    r.eq("save_off_differs", sum(bits_differ(got[False][k], g[k]) for k in g), 0)
    r.done()


@pytest.mark.parametrize("B,HID,eps2", R.TAIL_CLS_CASES)
def test_tail_cls_fwd_eps(K, report, B, HID, eps2):
    from test_cls_rows_gpu import N, full, noise, others_untouched
    D, M = R.TAIL_D, B * N
    ins = R.tail2_inputs(B, HID, eps2, 100 * eps2)
    ref = R.tail2_ref(ins, eps2, 100 * eps2)
    o = dict(x_mid=noise((M, D), 1), m2=noise((M,), 2, torch.float32), r2=noise((M,), 3, torch.float32), xn=noise((M, D), 4),
             gp=noise((M, HID), 5, torch.float16), h=noise((M, HID), 6), out=noise((M, D), 7))
    before = {k: v.clone() for k, v in o.items()}
    K.tail_cls_fwd(full(ins["a"], B), full(ins["x_in"], B), *tail_operands(K, ins), B, N, o["x_mid"], o["m2"], o["r2"], o["out"],
                   xn_out=o["xn"], gp=o["gp"], h=o["h"], eps2=eps2)
    torch.cuda.synchronize()
    r = report.case("tail_cls_fwd", f"{B}-{HID}-{eps2}")
    for k in o:
        assert others_untouched(o[k], before[k]), k
    x_mid, xn, out = (o[k][::N].float().cpu() for k in ("x_mid", "xn", "out"))
    assert R.variance_condition(x_mid, eps2) >= 0.9
    for k, v in (("x_mid", x_mid), ("xn", xn), ("out", out)):
        r.lt(k, R.rel(v, ref[k]), R.BF16_TOL)
    stat_figures(r, "ln2_", o["m2"][::N], o["r2"][::N], x_mid, eps2)
    r.done()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("eps", R.EPS_SWEEP)
@pytest.mark.parametrize("C,S,p,D,ape", R.PATCH_EMBED_CASES)
def test_patch_embed_statistics_eps(K, report, dt, eps, C, S, p, D, ape):
    from vitpe._lib import check, dtype_code, lib, ptr, stream_ptr
    assert K.patch_embed_supported(DT[dt], C, S, p, D)
    img, w, bias, cls, apet = R.patch_embed_inputs(dt, C, S, p, D, ape, eps)
    B, P = img.shape[0], (S // p) ** 2
    ref = R.patch_embed_ref(dt, img, w, bias, cls, apet, p)
    wd, bd, cd, ad, imd = dev(w, DT[dt]), dev(bias), dev(cls), (dev(apet) if ape else None), dev(img)
    mean, rstd = empty(B * (P + 1)), empty(B * (P + 1))
    tok = K.patch_embed(wd, bd, cd, ad, p, DT[dt], images=imd, stats=(mean, rstd), eps=eps)
    r = report.case("patch_embed", f"{dt}-{eps}-{C}-{S}-{p}-{D}-{ape}")
    t = tok.float().cpu()
    mean, rstd = mean.view(B, P + 1), rstd.view(B, P + 1)
    for tag, sl in (("cls_", slice(0, 1)), ("patch_", slice(1, None))):      # the class-token row and the patch rows
        assert R.variance_condition(t[:, sl], eps) >= 0.9
        r.lt(f"{tag}tokens_{dt}", R.rel(t[:, sl], ref[:, sl]), R.tol(dt))
        stat_figures(r, tag, mean[:, sl], rstd[:, sl], t[:, sl], eps)
    # the augmentation entry point without an rng pair is the same kernel: bit-identical
    m2, r2 = empty(B * (P + 1)), empty(B * (P + 1))
    tok2 = torch.empty_like(tok)
    check(lib().vitpe_patch_embed_aug(dtype_code(DT[dt]), ptr(imd), None, None, None, None, ptr(wd), ptr(bd), ptr(cd), ptr(ad),
                                      ptr(tok2), None, ptr(m2), ptr(r2), B, C, S, p, D, float(eps), None, 0, 0, stream_ptr()),
          "vitpe_patch_embed_aug")
    torch.cuda.synchronize()
    r.eq("aug_without_rng_differs", bits_differ(tok2, tok) + bits_differ(m2.view(B, P + 1), mean)
         + bits_differ(r2.view(B, P + 1), rstd), 0)
    r.done()
