"""The classifier head, the loss and embed_bwd (csrc/head.hip, csrc/embed.hip) through the C ABI against the float64 reference of
tests/head_ref.py, at the shapes where the kernels take another path:

  vitpe_head_step          every (KD, WLDS) instantiation a valid (D <= 768, Cn <= 64) reaches, in both dtypes (case list and
                           its coverage: head_ref.HEAD_STEP_CASES, test_head_loss_cpu.py); class-group boundaries Cn = 1, 3, 8,
                           9, 16, 17, 62, 64; the masked tail D % 64 != 0 at KD = 2, 3, 6; B = 1, 3, 5, 257 (a workgroup with
                           dead waves, several 32-image chunks of head_bwd_params_kernel, more than 256 per-image rows);
                           n_valid = 0, 1, B - 1, B with grad_scale != loss_scale; N = 1 and 17; the eps sweep on class rows
                           whose variance is within 8x of eps; the refusals Cn = 65 and D = 832
  vitpe_cross_entropy[_ctl] B up to 4100 (one workgroup, rows t, t + 256, ..), Cn = 1 .. 1000, ties at the maximum before and
                           after the label, logits shifted by +100, n_valid = 0, 1, 256, B, the evaluation form
  vitpe_head_fwd / _bwd    the grid-stride loop (B = 4100), N = 1, the scalar zero fill (bf16, D = 100), D = 1024 x 1000 classes
  vitpe_embed_bwd          B = 1, 16, 17, 50 (batch chunks of 16), both dtypes, dape given and NULL, accumulation

Tolerances (head_ref.py; all the project's own): logits / dlogits / fp32 gradients rel < 1e-4, per tensor AND per image row;
loss |d| < 1e-5 max(1, |ref|); counts, padded dlogits rows, untouched and zero-filled dx rows exact; class row of dx 1e-4 in
fp32 and |d| <= 2^-8 |ref| + 1e-4 max|ref| per element in bf16; rstd of the head |rstd / ref - 1| <= 1e-4; embed_bwd sums
1e-5 (test_embed_bwd), dpatch bit-exact.  The references are float64 on the values the kernel sees (bf16-rounded x).
"""
import math

import pytest
import torch

import head_ref as H
from parity_report import Report

pytestmark = pytest.mark.gpu
DT = H.DT


@pytest.fixture(scope="module")
def K():
    from vitpe import kernels
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return kernels


@pytest.fixture(scope="module")
def report():
    r = Report("test_head_loss_gpu")
    yield r
    r.close()


def z(*s):
    return torch.zeros(*s, device="cuda")


def ids(cases):
    return ["-".join(str(v) for v in c) for c in cases]


def ndiff(a, b):
    """number of elements of a that differ from b (a tensor or a number)"""
    return int((a != b).sum())


def run_head_step(K, dt, x, g, b, wh, bh, labels, eps, ctl, calls=2):
    """-> the buffers after `calls` launches on the same inputs, and a snapshot of the accumulated ones after the first."""
    B, N, D = x.shape
    Cn = wh.shape[0]
    o = dict(logits=z(B, Cn) + 7, dlogits=z(B, Cn) + 7, dx=torch.full((B, N, D), 7.0, device="cuda").to(DT[dt]),
             out2=z(2), macc=z(2), dwh=z(Cn, D), dbh=z(Cn), dgamma=z(D), dbeta=z(D))
    ws, dyn, per_image = (z(B, D), z(B, D)), z(B, D), z(2 * B)
    dev = [t.cuda() for t in (g, b, wh, bh, labels)]
    xd = x.cuda().to(DT[dt])
    first = None
    for _ in range(calls):
        K.head_step(xd, dev[0], dev[1], dev[2], dev[3], dev[4], o["logits"], o["dlogits"], ws, dyn, o["dx"], o["out2"],
                    o["macc"], per_image, ctl, o["dwh"], o["dbh"], o["dgamma"], o["dbeta"], eps=eps)
        if first is None:
            first = {k: o[k].clone() for k in ("dwh", "dbh", "dgamma", "dbeta", "macc")}
    torch.cuda.synchronize()
    return {k: v.float().cpu() for k, v in o.items()}, {k: v.cpu() for k, v in first.items()}


@pytest.mark.parametrize("c", H.HEAD_STEP_CASES, ids=ids(H.HEAD_STEP_CASES))
def test_head_step_against_float64(K, report, c):
    dt, B, N, D, Cn, nv, eps = c
    x, g, b, wh, bh, labels = H.head_inputs(dt, B, N, D, Cn, eps)
    gs, ls, _ = H.scales(B, nv)
    ref = H.head_ref(x, g, b, wh, bh, labels, eps, nv, gs, ls)
    ctl = torch.tensor([gs, ls, float(nv), 0.0], device="cuda")
    got, first = run_head_step(K, dt, x, g, b, wh, bh, labels, eps, ctl)
    r = report.case("head_step", "-".join(str(v) for v in c))
    r.lt("logits", H.rel(got["logits"], ref["logits"]), H.TOL)
    r.lt("logits_row", H.row_rel(got["logits"], ref["logits"]), H.TOL)
    r.lt("dlogits", H.rel(got["dlogits"], ref["dlogits"]), H.TOL)
    r.lt("dlogits_row", H.row_rel(got["dlogits"], ref["dlogits"]), H.TOL)
    r.eq("dlogits_padded_nonzero", ndiff(got["dlogits"][nv:], 0.0), 0)
    r.lt("loss", H.loss_err(got["out2"][0], ref["loss"]), H.LOSS_TOL)
    r.eq("correct", got["out2"][1], ref["correct"])
    if dt == "f32":
        r.lt("dx_f32", H.rel(got["dx"][:, 0], ref["dx"]), H.TOL)
    else:
        r.le("dx_bf16_excess", H.dx_bf16_excess(got["dx"][:, 0], ref["dx"]), 1.0)
    r.eq("dx_rows_1_touched", ndiff(got["dx"][:, 1:], 7.0), 0)
    # the second call: parameter gradients and metric_acc hold exactly twice one call's (one 32-image chunk: one atomic add
    # per element and call, g + g is exact; several chunks arrive in any order, so those are only gated against 2 x ref)
    for k in ("dwh", "dbh", "dgamma", "dbeta"):
        r.lt(k + "_twice", H.rel(got[k], 2 * ref[k]), H.TOL)
        r.lt(k + "_once", H.rel(first[k], ref[k]), H.TOL)
        if B <= 32:
            r.eq(k + "_doubling", ndiff(got[k], 2 * first[k]), 0)
    r.eq("metric_acc_first", ndiff(first["macc"], got["out2"]), 0)
    r.eq("metric_acc_twice", ndiff(got["macc"], 2 * got["out2"]), 0)
    r.done()


@pytest.mark.parametrize("dt,B,N,D,Cn,nv", [("f32", 5, 17, 96, 9, 4), ("bf16", 5, 17, 768, 17, 4), ("f32", 3, 1, 192, 64, 3),
                                            ("bf16", 5, 17, 384, 1, 5)])
def test_head_step_closed_forms(K, report, dt, B, N, D, Cn, nv):
    """Equal head rows: every logit of an image bit-identical, CE = log Cn, arg-max = class 0, dlogits = (1 / Cn - onehot)
    grad_scale.  A single class: loss 0, dlogits 0."""
    eps = 1e-5
    x, g, b, wh, bh, labels = H.head_inputs(dt, B, N, D, Cn, eps, seed=3)
    wh, bh = H.equal_rows_head(wh, bh)
    gs, ls, _ = H.scales(B, nv)
    ctl = torch.tensor([gs, ls, float(nv), 0.0], device="cuda")
    got, _ = run_head_step(K, dt, x, g, b, wh, bh, labels, eps, ctl, calls=1)
    closed = (1.0 / Cn - torch.nn.functional.one_hot(labels, Cn).double()) * gs
    closed[nv:] = 0
    r = report.case("head_step_closed", f"{dt}-{B}-{N}-{D}-{Cn}-{nv}")
    r.eq("logits_differ_within_image", ndiff(got["logits"], got["logits"][:, :1]), 0)
    r.lt("loss", H.loss_err(got["out2"][0], ls * nv * math.log(Cn)), H.LOSS_TOL)
    r.eq("correct", got["out2"][1], int((labels[:nv] == 0).sum()))
    r.lt("dlogits_row", H.row_rel(got["dlogits"], closed), H.TOL)
    if Cn == 1:
        r.eq("loss_single_class", got["out2"][0], 0.0)
        r.eq("dlogits_single_class_nonzero", ndiff(got["dlogits"], 0.0), 0)
    r.done()


def test_head_step_refuses_what_it_cannot_run(K):
    from vitpe._lib import VitpeError
    for D, Cn in ((192, 65), (832, 10)):
        x, g, b, wh, bh, labels = H.head_inputs("f32", 3, 2, D, Cn, 1e-5)
        ctl = torch.tensor([1.0, 1.0, 3.0, 0.0], device="cuda")
        with pytest.raises(VitpeError):
            run_head_step(K, "f32", x, g, b, wh, bh, labels, 1e-5, ctl, calls=1)


# ---- cross_entropy / cross_entropy_ctl -----------------------------------------------------------------------------------
def _ce_figures(r, tag, out2, dl, ref, nv):
    r.lt(tag + "loss", H.loss_err(out2[0], ref["loss"]), H.LOSS_TOL)
    r.eq(tag + "correct", out2[1], ref["correct"])
    if dl is not None:
        dl = dl.cpu()
        r.lt(tag + "dlogits", H.rel(dl, ref["dlogits"]), H.TOL)
        r.lt(tag + "dlogits_row", H.row_rel(dl, ref["dlogits"]), H.TOL)
        r.eq(tag + "dlogits_padded_nonzero", ndiff(dl[nv:], 0.0), 0)


@pytest.mark.parametrize("B,Cn", H.CE_CASES)
def test_cross_entropy_ties_shift_and_batch(K, report, B, Cn):
    zl, labels = H.tied_logits(B, Cn)
    ref = H.ce_ref(zl, labels, B, H.f32(1.0 / B), H.f32(1.0 / B))
    r = report.case("cross_entropy", f"{B}-{Cn}")
    for tag, shift in (("", 0.0), ("shift100_", 100.0)):      # the shift is exact in fp32: the same reference holds
        out2, dl = K.cross_entropy((zl + shift).cuda(), labels.cuda())
        _ce_figures(r, tag, out2.cpu(), dl, ref, B)
    # closed form: all logits of a row equal -> CE = log Cn, first index wins, dlogits = (1 / Cn - onehot) / B
    flat = zl[:, :1].expand(B, Cn).contiguous()
    out2, dl = K.cross_entropy(flat.cuda(), labels.cuda())
    closed = (1.0 / Cn - torch.nn.functional.one_hot(labels, Cn).double()) * H.f32(1.0 / B)
    r.lt("closed_loss", H.loss_err(out2[0].cpu(), math.log(Cn)), H.LOSS_TOL)
    r.eq("closed_correct", out2[1].cpu(), int((labels == 0).sum()))
    r.lt("closed_dlogits_row", H.row_rel(dl.cpu(), closed), H.TOL)
    r.done()


@pytest.mark.parametrize("Cn", [10, 1000])
@pytest.mark.parametrize("nv", [0, 1, 256, 600])
def test_cross_entropy_ctl_ragged_and_evaluation_form(K, report, nv, Cn):
    B = 600
    zl, labels = H.tied_logits(B, Cn, seed=1)
    gs, ls, _ = H.scales(B, nv)
    ref = H.ce_ref(zl, labels, nv, gs, ls)
    ctl = torch.tensor([gs, ls, float(nv), 0.0], device="cuda")
    r = report.case("cross_entropy_ctl", f"{B}-{Cn}-{nv}")
    out2, dl = K.cross_entropy_ctl(zl.cuda(), labels.cuda(), ctl, dlogits=z(B, Cn) + 7)
    _ce_figures(r, "", out2.cpu(), dl, ref, nv)
    # the evaluation form: no dlogits, metric_acc accumulates
    macc = z(2)
    for rep in range(2):
        o2, none = K.cross_entropy_ctl(zl.cuda(), labels.cuda(), ctl, dlogits=None, metric_acc=macc)
        assert none is None
        r.eq(f"eval_out2_{rep}", ndiff(o2.cpu(), out2.cpu()), 0)
        r.eq(f"eval_metric_acc_{rep}", ndiff(macc.cpu(), (rep + 1) * out2.cpu()), 0)
    r.done()


# ---- head_fwd + cross_entropy + head_bwd -----------------------------------------------------------------------------------
@pytest.mark.parametrize("c", H.HEAD_FWD_BWD_CASES, ids=ids(H.HEAD_FWD_BWD_CASES))
def test_head_fwd_bwd_against_float64(K, report, c):
    dt, B, N, D, Cn, eps = c
    x, g, b, wh, bh, labels = H.head_inputs(dt, B, N, D, Cn, eps)
    s = H.f32(1.0 / B)
    ref = H.head_ref(x, g, b, wh, bh, labels, eps, B, s, s)
    xd, gd, bd, whd, bhd = x.cuda().to(DT[dt]), g.cuda(), b.cuda(), wh.cuda(), bh.cuda()
    r = report.case("head_fwd_bwd", "-".join(str(v) for v in c))
    lg0, none = K.head_fwd(xd, gd, bd, whd, bhd, eps=eps, save=False)
    assert none is None
    lg, ws = K.head_fwd(xd, gd, bd, whd, bhd, eps=eps, save=True)
    r.eq("logits_save_on_off_differ", ndiff(lg0, lg), 0)
    r.lt("logits", H.rel(lg.cpu(), ref["logits"]), H.TOL)
    r.lt("logits_row", H.row_rel(lg.cpu(), ref["logits"]), H.TOL)
    r.le("rstd", float((ws[2].cpu().double() / ref["rstd"] - 1).abs().max()), 1e-4)
    out2, dl = K.cross_entropy(lg, labels.cuda())
    _ce_figures(r, "", out2.cpu(), dl, ref, B)
    grads = dict(dwh=z(Cn, D), dbh=z(Cn), dgamma=z(D), dbeta=z(D))
    dx = torch.full((B, N, D), 7.0, device="cuda").to(DT[dt])
    K.head_bwd(dl, whd, gd, ws, DT[dt], N, grads["dwh"], grads["dbh"], grads["dgamma"], grads["dbeta"], dx=dx)
    dx = dx.float().cpu()
    if dt == "f32":
        r.lt("dx_f32", H.rel(dx[:, 0], ref["dx"]), H.TOL)
    else:
        r.le("dx_bf16_excess", H.dx_bf16_excess(dx[:, 0], ref["dx"]), 1.0)
    r.eq("dx_rows_1_nonzero", ndiff(dx[:, 1:], 0.0), 0)
    for k, v in grads.items():
        r.lt(k, H.rel(v.cpu(), ref[k]), H.TOL)
    r.done()


# ---- embed_bwd ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("Ntok,D", [(17, 96), (65, 192)])
def test_embed_bwd_batch_chunks_accumulation_and_null_dape(K, report, dt, Ntok, D):
    """dcls += sum_b dtok[b, 0], dape += sum_b dtok[b, 1:] over batch chunks of 16 (fp32 atomics), dpatch = the patch rows
    repacked, bit for bit; dape == NULL (no absolute position embedding) leaves out that sum only."""
    r = report.case("embed_bwd", f"{dt}-{Ntok}-{D}")
    for B in (1, 16, 17, 50):
        g = torch.Generator().manual_seed(B)
        dtok = (torch.rand(B, Ntok, D, generator=g) * 2 - 1).to(DT[dt])
        cls0, ape0 = torch.rand(D, generator=g) + 0.5, torch.rand(Ntok - 1, D, generator=g) + 0.5
        for with_ape in (True, False):
            dcls, dape = cls0.cuda(), (ape0.cuda() if with_ape else None)
            dpatch = K.embed_bwd(dtok.cuda(), dcls, dape)
            r.lt("dcls", H.rel(dcls.cpu(), cls0.double() + dtok[:, 0].double().sum(0)), 1e-5)
            if with_ape:
                r.lt("dape", H.rel(dape.cpu(), ape0.double() + dtok[:, 1:].double().sum(0)), 1e-5)
            r.eq("dpatch_differs", ndiff(dpatch.cpu().float(), dtok[:, 1:].reshape(-1, D).float()), 0)
    r.done()
