"""Class-row tail kernels (csrc/tail_cls.hip) at the hidden sizes and batches where their batched weight streams take
another path.  The kernels load weight fragments ahead of use: hidden tiles two register sets deep, the k loops over the
hidden layer in batches of 8 chunks with a remainder path.

HID (all pass vitpe_block_tail2_supported):
  128   8 hidden tiles for 12 waves (four waves have none), 4 k-chunks: less than one batch
  320   20 tiles (waves with two and with one), 10 k-chunks: one batch and a remainder of 2
  1536  96 tiles, 48 k-chunks: the maximum, the LDS extent
B: 1 (a single row in a clamped tile), 17 (ragged), 33 (a third workgroup of one row).

The method, helpers and tolerances are those of test_cls_rows_gpu.py (restated next to each assert): N = 65, D = 192, bf16;
every non-class row of every input holds the sentinel 1e4 and every non-class row of every output must come back
bit-identical; class rows against fp32 math on the rounded operands and against the full-row kernels on the gathered rows.
Both kernels, the forward in its training and evaluation forms, and two launches on the same inputs: bit-equal except
dgamma / dbeta (fp32 atomics across workgroups).
"""
import pytest
import torch

from conftest import rel_err
from test_cls_rows_gpu import D, N, full, noise, others_untouched
from test_kernels_gpu import BF16_TOL, K, dev, q, rnd  # noqa: F401  (K: the kernels fixture)

pytestmark = pytest.mark.gpu

HIDS = [128, 320, 1536]
BATCHES = [1, 17, 33]
bf = torch.bfloat16


def bits_equal(a, b):
    return torch.equal(a.view(torch.int16 if a.element_size() == 2 else torch.int32),
                       b.view(torch.int16 if b.element_size() == 2 else torch.int32))


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("HID", HIDS)
def test_tail_cls_forward_hidden_sizes(K, HID, B):
    assert K.block_tail2_supported(bf, D, HID)
    M = B * N
    a_, x_in = rnd(B, D, seed=21), rnd(B, D, seed=22)
    wp, bp = rnd(D, D, seed=23, scale=0.07), 0.1 * rnd(D, seed=24)
    g, b = 1 + 0.1 * rnd(D, seed=25), 0.1 * rnd(D, seed=26)
    w1, b1 = rnd(HID, D, seed=27, scale=0.08), 0.1 * rnd(HID, seed=28)
    w2, b2 = rnd(D, HID, seed=29, scale=0.05), 0.1 * rnd(D, seed=30)
    wp_pk, w1_pk, w2_pk = (K.pack_weight_frags(dev(wp), bf, 192, 0), K.pack_weight_frags(dev(w1), bf, 192, 1),
                           K.pack_weight_frags(dev(w2), bf, 32, 1))
    ins = (full(a_, B), full(x_in, B), wp_pk, dev(bp), dev(g), dev(b), w1_pk, dev(b1), w2_pk, dev(b2), B, N)
    before = dict(x_mid=noise((M, D), 1), m2=noise((M,), 2, torch.float32), r2=noise((M,), 3, torch.float32), xn=noise((M, D), 4),
                  gp=noise((M, HID), 5, torch.float16), h=noise((M, HID), 6), out=noise((M, D), 7))

    def launch(train):
        o = {k: v.clone() for k, v in before.items()}
        K.tail_cls_fwd(*ins, o["x_mid"], o["m2"], o["r2"], o["out"],
                       **(dict(xn_out=o["xn"], gp=o["gp"], h=o["h"]) if train else {}))
        torch.cuda.synchronize()
        return o

    outs = launch(True)
    for k in outs:
        assert others_untouched(outs[k], before[k]), k
    x_mid, m2, r2, xn_out, gp, h, out = (outs[k][::N].float().cpu() for k in ("x_mid", "m2", "r2", "xn", "gp", "h", "out"))
    # fp32 math on the rounded operands, stage by stage from the kernel's own (rounded) intermediates
    xm = q(a_, "bf16") @ q(wp, "bf16").t() + bp + q(x_in, "bf16")
    assert rel_err(x_mid, xm) < BF16_TOL                                                    # 3e-2
    assert rel_err(m2, x_mid.mean(1)) < 1e-5
    assert rel_err(r2, (x_mid.var(1, unbiased=False) + 1e-5).rsqrt()) < 1e-5
    xn = torch.nn.functional.layer_norm(x_mid, (D,), g, b)
    assert rel_err(xn_out, xn) < BF16_TOL                                                   # 3e-2
    u_ref = (xn_out @ q(w1, "bf16").t() + b1).requires_grad_(True)
    h_ref = torch.nn.functional.gelu(u_ref)
    assert rel_err(h, h_ref.detach()) < 6e-3
    gp_ref, = torch.autograd.grad(h_ref.sum(), u_ref)
    assert rel_err(gp, gp_ref) < 1.2e-3       # gelu'(u) kept as IEEE half (round toward zero)
    ref = x_mid + q(h_ref.detach(), "bf16") @ q(w2, "bf16").t() + b2
    assert rel_err(out, ref) < BF16_TOL                                                     # 3e-2
    # the full-row kernel on the gathered rows: same arithmetic and rounding points
    o2, xm2, m22, r22, gp2, h2 = K.block_tail2_fwd(dev(a_, bf), dev(x_in, bf), wp_pk, dev(bp), dev(g), dev(b), w1_pk, dev(b1),
                                                  w2_pk, dev(b2))
    assert rel_err(x_mid, xm2.float().cpu()) < 4e-3 and rel_err(out, o2.float().cpu()) < 8e-3
    assert rel_err(h, h2.float().cpu()) < 8e-3 and rel_err(gp, gp2.float().cpu()) < 1.2e-3
    # evaluation form: the same rows, nothing of the hidden layer (nor the normalised rows) written
    ev = launch(False)
    for k in ("x_mid", "m2", "r2", "out"):
        assert bits_equal(ev[k], outs[k]), k
    for k in ("h", "gp", "xn"):
        assert bits_equal(ev[k], before[k]), k
    # a second launch on the same inputs: every output bit-equal
    again = launch(True)
    for k in outs:
        assert bits_equal(again[k], outs[k]), k


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("HID", HIDS)
def test_tail_cls_backward_hidden_sizes(K, HID, B):
    M = B * N
    x, g = rnd(B, D, seed=41), 1 + 0.1 * rnd(D, seed=42)
    dy, gp = rnd(B, D, seed=43), 0.5 + 0.6 * rnd(B, HID, seed=44)
    w2, w1, wp = rnd(D, HID, seed=45, scale=0.05), rnd(HID, D, seed=46, scale=0.08), rnd(D, D, seed=47, scale=0.07)
    xd = dev(x, bf)
    _, mean, rstd = K.layernorm_fwd(xd, dev(g), torch.zeros(D, device="cuda"))
    w2t_pk = K.pack_weight_frags(dev(w2.t().contiguous()), bf, 192, 1)
    w1t_pk = K.pack_weight_frags(dev(w1.t().contiguous()), bf, 32, 1)
    wpt_pk = K.pack_weight_frags(dev(wp.t().contiguous()), bf, 192, 1)
    gph = q(gp, "bf16").to(torch.float16)       # (exact: the values were rounded to 8 mantissa bits)
    ins = (full(dy, B), full(q(gp, "bf16"), B, dtype=torch.float16), w2t_pk, w1t_pk, full(x, B),
           full(mean.cpu(), B, dtype=torch.float32), full(rstd.cpu(), B, dtype=torch.float32), dev(g))
    before = dict(du=noise((M, HID), 11), dx=noise((M, D), 12), da=noise((M, D), 13))

    def launch():
        o = {k: v.clone() for k, v in before.items()}
        dg2, db2 = torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")
        K.tail_cls_bwd(*ins, dg2, db2, wpt_pk, B, N, du=o["du"], out=o["dx"], da=o["da"])
        torch.cuda.synchronize()
        return o, dg2.cpu(), db2.cpu()

    outs, dg2, db2 = launch()
    for k in outs:
        assert others_untouched(outs[k], before[k]), k
    du2, dx2, da2 = (outs[k][::N].float().cpu() for k in ("du", "dx", "da"))
    # fp32 math on the rounded operands (the checks and tolerances of test_tail_cls_backward_class_rows_only)
    dyq, gpq, xq = q(dy, "bf16"), q(gp, "bf16"), q(x, "bf16")
    assert rel_err(du2, (dyq @ q(w2, "bf16")) * gpq) < 6e-3
    dxn = du2 @ q(w1, "bf16")
    mu, rs = mean.cpu()[:, None], rstd.cpu()[:, None]
    xhat = (xq - mu) * rs
    gy = dxn * g
    dx_ref = dyq + rs * (gy - gy.mean(1, keepdim=True) - xhat * (gy * xhat).mean(1, keepdim=True))
    assert rel_err(dx2, dx_ref) < 6e-3
    assert rel_err(dg2, (dxn * xhat).sum(0)) < 2e-3 and rel_err(db2, dxn.sum(0)) < 2e-3
    assert rel_err(da2, dx2 @ q(wp, "bf16")) < 6e-3
    # the full-row kernel on the gathered rows: same arithmetic and rounding points, so the bounds above hold between the
    # two as well (6e-3 on the bf16 tensors, 2e-3 on the fp32 column sums)
    dgf, dbf = torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")
    dxf, duf, daf = K.block_tail2_bwd(dev(dy, bf), dev(gph), w2t_pk, w1t_pk, xd, mean, rstd, dev(g), dgf, dbf, wpt_pk)
    torch.cuda.synchronize()
    assert rel_err(du2, duf.float().cpu()) < 6e-3 and rel_err(dx2, dxf.float().cpu()) < 6e-3
    assert rel_err(da2, daf.float().cpu()) < 6e-3
    assert rel_err(dg2, dgf.cpu()) < 2e-3 and rel_err(db2, dbf.cpu()) < 2e-3
    # a second launch on the same inputs: bit-equal, except the atomically summed dgamma / dbeta (2e-3)
    again, dg3, db3 = launch()
    for k in outs:
        assert bits_equal(again[k], outs[k]), k
    assert rel_err(dg3, dg2) < 2e-3 and rel_err(db3, db2) < 2e-3
