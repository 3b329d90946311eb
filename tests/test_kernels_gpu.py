"""GPU parity tests, kernel by kernel, through the C ABI (ctypes) against the CPU oracle.

Tolerances (written here, per the parity contract):
  * integer tables: bit-exact;
  * fp32 mode (exact-fp32 MFMA): 1e-4 relative (north-star gate; typically ~1e-6);
  * bf16 mode: 3e-2 relative against the fp32 oracle (bf16 has 8 significant bits).
"rel" = max|a-b| / max|b| (conftest.rel_err).
"""
import math

import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import vit_oracle as O

pytestmark = pytest.mark.gpu

F32_TOL = 1e-4
BF16_TOL = 3e-2
DT = {"f32": torch.float32, "bf16": torch.bfloat16}


def tol(dt):
    return F32_TOL if dt == "f32" else BF16_TOL


@pytest.fixture(scope="module")
def K():
    from vitpe import kernels
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return kernels


def dev(t, dtype=None):
    t = t.cuda()
    return t.to(dtype).contiguous() if dtype is not None else t.contiguous()


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def q(t, dt):
    """the values the kernel actually sees (bf16-rounded inputs for bf16 mode)"""
    return t.detach().to(DT[dt]).float().clone()


# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_selftest_mma_operand_maps(K, dt):
    # asymmetric integer data: exact in both types; catches swapped row/col maps
    g = torch.Generator().manual_seed(1)
    A = torch.randint(-4, 5, (16, 32), generator=g).float()
    B = torch.randint(-4, 5, (32, 16), generator=g).float() + torch.arange(16).float()[None, :] * 0.0
    B[:, 3] += 2.0
    ref = A @ B
    c_row, c_tr = K.selftest_mma(dev(A, DT[dt]), dev(B.t().contiguous(), DT[dt]), dev(B, DT[dt]))
    assert torch.equal(c_row.cpu(), ref), "row-fragment MMA map wrong"
    assert torch.equal(c_tr.cpu(), ref), "transposed-LDS-read fragment map wrong"


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("M,N,K_", [(195, 96, 96), (260, 192, 192), (130, 576, 192), (65, 192, 768), (128, 96, 48), (64, 192, 16)])
def test_gemm_nt_bias(K, dt, M, N, K_):
    a, w, b = rnd(M, K_, seed=1), rnd(N, K_, seed=2, scale=0.2), rnd(N, seed=3)
    ref = q(a, dt) @ q(w, dt).t() + b
    out = K.gemm_nt(dev(a, DT[dt]), dev(w, DT[dt]), dev(b), epi=0)
    assert rel_err(out.float().cpu(), ref) < tol(dt)
    out = K.gemm_nt(dev(a, DT[dt]), dev(w, DT[dt]), None, epi=0)
    assert rel_err(out.float().cpu(), ref - b) < tol(dt)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_gemm_nt_gelu_resid_gelubwd(K, dt):
    M, N, K_ = 195, 384, 96
    a, w, b = rnd(M, K_, seed=1), rnd(N, K_, seed=2, scale=0.3), rnd(N, seed=3)
    u_ref = q(a, dt) @ q(w, dt).t() + b
    h, u = K.gemm_nt(dev(a, DT[dt]), dev(w, DT[dt]), dev(b), epi=1)
    assert rel_err(u.float().cpu(), u_ref) < tol(dt)
    assert rel_err(h.float().cpu(), torch.nn.functional.gelu(u_ref)) < tol(dt)
    r = rnd(M, N, seed=4)
    out = K.gemm_nt(dev(a, DT[dt]), dev(w, DT[dt]), dev(b), epi=2, resid=dev(r, DT[dt]))
    assert rel_err(out.float().cpu(), u_ref + q(r, dt)) < tol(dt)
    # gelu backward epilogue: (A W^T) * gelu'(U)
    uu = rnd(M, N, seed=5, scale=3.0)
    ug = q(uu, dt).requires_grad_(True)
    torch.nn.functional.gelu(ug).sum().backward()
    out = K.gemm_nt(dev(a, DT[dt]), dev(w, DT[dt]), None, epi=4, u=dev(uu, DT[dt]))
    assert rel_err(out.float().cpu(), (u_ref - b) * ug.grad) < tol(dt)


@pytest.mark.parametrize("mt", [0, 4, 5, 6])
@pytest.mark.parametrize("M,N,K_", [(4200, 1024, 192), (2049, 2304, 64), (5000, 1024, 640), (4200, 3072, 128), (2100, 2048, 64)])
def test_gemm_big_tile_kernel_all_epilogues(K, mt, M, N, K_):
    """csrc/gemm2d.hip (bf16, many rows x wide weights: vitpe_gemm_nt hands these shapes to it) at every tile height, ragged
    last row tile, one / three / ten K steps, against fp32 math on the bf16-rounded operands.  N = 3072 / 2048: the wide outputs,
    whose tiles are walked in supertile order."""
    from vitpe import _lib as L
    assert L.debug_lib().vitpe_debug_set_gemm2d_mt(mt) == 0
    try:
        dt = "bf16"
        a, w, b = rnd(M, K_, seed=1), rnd(N, K_, seed=2, scale=0.2), rnd(N, seed=3)
        ref = q(a, dt) @ q(w, dt).t() + b
        A, W = dev(a, DT[dt]), dev(w, DT[dt])
        assert rel_err(K.gemm_nt(A, W, dev(b), epi=0).float().cpu(), ref) < tol(dt)
        assert rel_err(K.linear(A, W, None, epi=0).float().cpu(), ref - b) < tol(dt)
        r = rnd(M, N, seed=4)
        out = K.gemm_nt(A, W, dev(b), epi=2, resid=dev(r, DT[dt]))
        assert rel_err(out.float().cpu(), ref + q(r, dt)) < tol(dt)
        h, u = K.gemm_nt(A, W, dev(b), epi=1)
        assert rel_err(u.float().cpu(), ref) < tol(dt)
        assert rel_err(h.float().cpu(), torch.nn.functional.gelu(ref)) < tol(dt)
        uu = rnd(M, N, seed=5, scale=3.0)
        ug = q(uu, dt).requires_grad_(True)
        torch.nn.functional.gelu(ug).sum().backward()
        out = K.gemm_nt(A, W, None, epi=4, u=dev(uu, DT[dt]))
        assert rel_err(out.float().cpu(), (ref - b) * ug.grad) < tol(dt)
        # row-exact check on a few rows (a tile permutation or a missing row would pass a max-norm test on random data
        # only by luck; this pins rows at both ends of the ragged last tile)
        o = K.gemm_nt(A, W, dev(b), epi=0).float().cpu()
        for row in (0, 1, 127, 128, M - 2, M - 1):
            assert rel_err(o[row], ref[row]) < tol(dt)
    finally:
        L.debug_lib().vitpe_debug_set_gemm2d_mt(0)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("M,N,K_", [(397, 192, 192), (1300, 768, 192), (650, 192, 768), (260, 192, 576), (33, 384, 96), (130, 192, 96)])
def test_linear_panel_kernel_all_epilogues(K, dt, M, N, K_):
    a, w, b = rnd(M, K_, seed=1), rnd(N, K_, seed=2, scale=0.2), rnd(N, seed=3)
    ref = q(a, dt) @ q(w, dt).t() + b
    A, W = dev(a, DT[dt]), dev(w, DT[dt])
    out = K.linear(A, W, dev(b), epi=0)
    assert rel_err(out.float().cpu(), ref) < tol(dt)
    assert rel_err(K.linear(A, W, None, epi=0).float().cpu(), ref - b) < tol(dt)
    r = rnd(M, N, seed=4)
    out = K.linear(A, W, dev(b), epi=2, resid=dev(r, DT[dt]))
    assert rel_err(out.float().cpu(), ref + q(r, dt)) < tol(dt)
    h, u = K.linear(A, W, dev(b), epi=1)
    assert rel_err(u.float().cpu(), ref) < tol(dt)
    assert rel_err(h.float().cpu(), torch.nn.functional.gelu(ref)) < tol(dt)
    uu = rnd(M, N, seed=5, scale=3.0)
    ug = q(uu, dt).requires_grad_(True)
    torch.nn.functional.gelu(ug).sum().backward()
    out = K.linear(A, W, None, epi=4, u=dev(uu, DT[dt]))
    assert rel_err(out.float().cpu(), (ref - b) * ug.grad) < tol(dt)
    if N == 192:  # fused LayerNorm statistics of the output rows
        mean = torch.empty(M, device="cuda")
        rstd = torch.empty(M, device="cuda")
        out = K.linear(A, W, dev(b), epi=2, resid=dev(r, DT[dt]), stats=(mean, rstd))
        o = out.float().cpu()
        assert rel_err(mean.cpu(), o.mean(-1)) < 1e-4
        assert rel_err(rstd.cpu(), 1.0 / torch.sqrt(o.var(-1, unbiased=False) + 1e-5)) < 1e-4


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_layernorm_fused_into_linear_and_attention(K, dt):
    """LN prologue of vitpe_linear_ln, LN-backward epilogue of vitpe_linear_lnbwd, LN inside the attention staging."""
    M, D, hid = 397, 192, 768
    x, g, b = rnd(M, D, seed=1, scale=2.0) + 0.3, 1 + 0.1 * rnd(D, seed=2), 0.1 * rnd(D, seed=3)
    w1, b1 = rnd(hid, D, seed=4, scale=0.2), rnd(hid, seed=5)
    xq = q(x, dt)
    xn_ref = torch.nn.functional.layer_norm(xq, (D,), g, b, 1e-5)
    X = dev(x, DT[dt])
    mean, rstd = torch.empty(M, device="cuda"), torch.empty(M, device="cuda")
    K.layernorm_fwd(X, dev(g), dev(b), mean=mean, rstd=rstd, stats_only=True)
    assert rel_err(mean.cpu(), xq.mean(-1)) < 1e-5
    xn_out = torch.empty_like(X)
    h, u = K.linear_ln(X, dev(g), dev(b), mean, rstd, dev(w1, DT[dt]), dev(b1), epi=1, xn_out=xn_out)
    assert rel_err(xn_out.float().cpu(), xn_ref) < tol(dt)
    u_ref = q(xn_ref, dt) @ q(w1, dt).t() + b1
    assert rel_err(u.float().cpu(), u_ref) < tol(dt)
    assert rel_err(h.float().cpu(), torch.nn.functional.gelu(u_ref)) < tol(dt)
    # backward: dx = dres + LN'(dy @ wt^T)
    Kd = 576
    dy, wt, dres = rnd(M, Kd, seed=6), rnd(D, Kd, seed=7, scale=0.2), rnd(M, D, seed=8)
    xr = xq.clone().requires_grad_(True)
    gr, br = g.clone().requires_grad_(True), b.clone().requires_grad_(True)
    yr = torch.nn.functional.layer_norm(xr, (D,), gr, br, 1e-5)
    dxn = q(q(dy, dt) @ q(wt, dt).t(), dt)
    yr.backward(dxn)
    dgam, dbet = torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")
    dx = K.linear_lnbwd(dev(dy, DT[dt]), dev(wt, DT[dt]), X, mean, rstd, dev(g), dev(dres, DT[dt]), dgam, dbet)
    assert rel_err(dx.float().cpu(), xr.grad + q(dres, dt)) < tol(dt)
    assert rel_err(dgam.cpu(), gr.grad) < tol(dt)
    assert rel_err(dbet.cpu(), br.grad) < tol(dt)
    # attention with LN in the staging == attention on pre-normalised tokens
    B, N, H = 3, 65, 6
    xa = rnd(B, N, D, seed=9, scale=2.0)
    wq = K.pack_qkv_weights(dev(rnd(3 * D, D, seed=10, scale=0.3)), DT[dt], H)
    t = device_pe(K, "rope-axial", {"inv_freq": O.rope_axial_inv_freq(32, 100.0)}, H, 8)
    Xa = dev(xa, DT[dt])
    xn, m_, r_ = K.layernorm_fwd(Xa, dev(g), dev(b))
    ref = K.fused_attention_fwd(xn, wq, H, t)
    xn2 = torch.empty_like(Xa)
    out = K.fused_attention_fwd(Xa, wq, H, t, ln=(dev(g), dev(b), m_, r_), xn_out=xn2)
    assert torch.equal(xn2, xn)
    assert rel_err(out.float().cpu(), ref.float().cpu()) < 1e-6


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("M,N,K_,splits", [(195, 96, 96, 1), (650, 576, 192, 4), (333, 192, 768, 3), (260, 192, 48, 2), (200, 96, 384, 5)])
def test_gemm_tn_wgrad(K, dt, M, N, K_, splits):
    dy, x = rnd(M, N, seed=1), rnd(M, K_, seed=2)
    ref_w = q(dy, dt).t() @ q(x, dt)
    ref_b = q(dy, dt).sum(0)
    dw = torch.zeros(N, K_, device="cuda")
    db = torch.zeros(N, device="cuda")
    K.gemm_tn(dev(dy, DT[dt]), dev(x, DT[dt]), dw, db, splits=splits)
    assert rel_err(dw.cpu(), ref_w) < tol(dt)
    assert rel_err(db.cpu(), ref_b) < tol(dt)
    K.gemm_tn(dev(dy, DT[dt]), dev(x, DT[dt]), dw, None, splits=splits)  # accumulates
    assert rel_err(dw.cpu(), 2 * ref_w) < tol(dt)


def _frag_pack_ref(w, kchunk, phi):
    """numpy restatement of vitpe_pack_weight_frags (include/vitpe.h)."""
    import numpy as np
    R, C = w.shape
    ksc, ntr = kchunk // 32, R // 16
    out = np.empty(R * C, dtype=np.float32)
    idx = np.arange(R * C)
    e, l, blk = idx & 7, (idx >> 3) & 63, idx >> 9
    ks, nt, kc = blk % ksc, (blk // ksc) % ntr, blk // ksc // ntr
    cc, g = l & 15, l >> 4
    k = np.where(e < 4, 4 * g + e, 16 + 4 * g + e - 4) if phi else 8 * g + e
    out[:] = w.numpy()[16 * nt + cc, kchunk * kc + 32 * ks + k]
    return torch.from_numpy(out).view(R, C)


@pytest.mark.parametrize("shape,kchunk,phi", [((192, 192), 192, 0), ((768, 192), 192, 1), ((192, 768), 32, 1), ((32, 64), 32, 1)])
def test_pack_weight_frags_layout(K, shape, kchunk, phi):
    w = rnd(*shape, seed=7)
    for dt in (torch.bfloat16, torch.float32):
        got = K.pack_weight_frags(dev(w), dt, kchunk, phi).float().cpu()
        assert torch.equal(got, _frag_pack_ref(w, kchunk, phi).to(dt).float())


@pytest.mark.parametrize("M,HID,save", [(650, 768, True), (130 * 2 + 5, 768, False), (33280, 768, True), (13, 128, True),
                                        (144 * 3, 1536, True), (16 * 2048 + 16 * 40 + 3, 768, True)])
def test_block_tail2_forward_equals_the_per_linear_path(K, M, HID, save):
    """The wave-per-token-tile block tail (hidden activation in registers, packed weights by LDS-DMA) against the
    three panel-GEMM launches on the same operands, and against fp32 math on the rounded operands."""
    D, bf = 192, torch.bfloat16
    assert K.block_tail2_supported(bf, D, HID)
    a_, x_in = rnd(M, D, seed=21), rnd(M, D, seed=22)
    wp, bp = rnd(D, D, seed=23, scale=0.07), 0.1 * rnd(D, seed=24)
    g, b = 1 + 0.1 * rnd(D, seed=25), 0.1 * rnd(D, seed=26)
    w1, b1 = rnd(HID, D, seed=27, scale=0.08), 0.1 * rnd(HID, seed=28)
    w2, b2 = rnd(D, HID, seed=29, scale=0.05), 0.1 * rnd(D, seed=30)
    mo, ro = torch.empty(M, device="cuda"), torch.empty(M, device="cuda")
    xn_out = torch.empty(M, D, device="cuda", dtype=bf)
    wp_pk = K.pack_weight_frags(dev(wp), bf, 192, 0)
    w1_pk = K.pack_weight_frags(dev(w1), bf, 192, 1)
    w2_pk = K.pack_weight_frags(dev(w2), bf, 32, 1)
    out, x_mid, m2, r2, gp, h = K.block_tail2_fwd(dev(a_, bf), dev(x_in, bf), wp_pk, dev(bp), dev(g), dev(b), w1_pk, dev(b1),
                                                 w2_pk, dev(b2), xn_out=xn_out, stats=(mo, ro), save=save)
    assert (h is not None) == save and (gp is not None) == save
    # the per-Linear launches it replaces (vitpe_linear with row statistics, vitpe_linear_ln, vitpe_linear): same operands,
    # other summation orders and one more rounding of the hidden activation
    if HID % 192 == 0:   # (vitpe_linear_ln: output widths in units of 192)
        from vitpe import _lib as L
        m21, r21 = torch.empty(M, device="cuda"), torch.empty(M, device="cuda")
        mo1, ro1 = torch.empty(M, device="cuda"), torch.empty(M, device="cuda")
        x_mid1 = K.linear(dev(a_, bf), dev(wp, bf), dev(bp), epi=L.EPI_BIAS_RESID, resid=dev(x_in, bf), stats=(m21, r21))
        xn1 = torch.empty_like(xn_out)
        h1, _ = K.linear_ln(x_mid1, dev(g), dev(b), m21, r21, dev(w1, bf), dev(b1), epi=L.EPI_BIAS_GELU, xn_out=xn1)
        out1 = K.linear(h1, dev(w2, bf), dev(b2), epi=L.EPI_BIAS_RESID, resid=x_mid1, stats=(mo1, ro1))
        assert rel_err(x_mid.float().cpu(), x_mid1.float().cpu()) < 4e-3      # different summation order, then one rounding
        assert rel_err(m2.cpu(), m21.cpu()) < 1e-3 and rel_err(r2.cpu(), r21.cpu()) < 1e-3
        assert rel_err(xn_out.float().cpu(), xn1.float().cpu()) < 8e-3
        assert rel_err(out.float().cpu(), out1.float().cpu()) < 8e-3
        assert rel_err(mo.cpu(), mo1.cpu()) < 2e-3 and rel_err(ro.cpu(), ro1.cpu()) < 2e-3
        if save:
            assert rel_err(h.float().cpu(), h1.float().cpu()) < 8e-3
    # fp32 math on the rounded operands, stage by stage from the kernel's own (rounded) intermediates
    xm = q(a_, "bf16") @ q(wp, "bf16").t() + bp + q(x_in, "bf16")
    assert rel_err(x_mid.float().cpu(), xm) < BF16_TOL
    xmq = x_mid.float().cpu()
    assert rel_err(m2.cpu(), xmq.mean(1)) < 1e-5
    assert rel_err(r2.cpu(), (xmq.var(1, unbiased=False) + 1e-5).rsqrt()) < 1e-5
    xn = torch.nn.functional.layer_norm(xmq, (D,), g, b)
    assert rel_err(xn_out.float().cpu(), xn) < BF16_TOL
    xnq = xn_out.float().cpu()
    u_ref = (xnq @ q(w1, "bf16").t() + b1).requires_grad_(True)
    h_ref = torch.nn.functional.gelu(u_ref)
    if save:
        assert rel_err(h.float().cpu(), h_ref.detach()) < 6e-3
        gp_ref, = torch.autograd.grad(h_ref.sum(), u_ref)
        assert gp.dtype == torch.float16 and rel_err(gp.float().cpu(), gp_ref) < 1.2e-3   # gelu'(u) kept as IEEE half (round toward zero)
    ref = xmq + q(h_ref.detach(), "bf16") @ q(w2, "bf16").t() + b2
    assert rel_err(out.float().cpu(), ref) < BF16_TOL
    o = out.float().cpu()
    assert rel_err(mo.cpu(), o.mean(1)) < 1e-4
    assert rel_err(ro.cpu(), (o.var(1, unbiased=False) + 1e-5).rsqrt()) < 1e-4


def test_block_tail2_unsupported_shapes_are_errors(K):
    bf = torch.bfloat16
    assert not K.block_tail2_supported(bf, 256, 768) and not K.block_tail2_supported(torch.float32, 192, 768)
    assert not K.block_tail2_supported(bf, 192, 100) and not K.block_tail2_supported(bf, 192, 3072)
    assert not K.block_tail2_supported(bf, 192, 64)


@pytest.mark.parametrize("M,HID", [(650, 768), (130 * 2 + 5, 768), (33280, 768), (13, 128), (16 * 2048 + 16 * 40 + 3, 768)])
def test_block_tail2_backward_on_saved_derivative(K, M, HID):
    """The wave-per-token-tile backward (packed transposed weights, gelu'(u) as saved by the forward): du / dx_mid / da /
    dgamma / dbeta against fp32 math on the rounded operands."""
    D, bf = 192, torch.bfloat16
    x, g = rnd(M, D, seed=41), 1 + 0.1 * rnd(D, seed=42)
    dy, gp = rnd(M, D, seed=43), 0.5 + 0.6 * rnd(M, HID, seed=44)
    w2, w1, wp = rnd(D, HID, seed=45, scale=0.05), rnd(HID, D, seed=46, scale=0.08), rnd(D, D, seed=47, scale=0.07)
    xd = dev(x, bf)
    _, mean, rstd = K.layernorm_fwd(xd, dev(g), torch.zeros(D, device="cuda"))
    w2t_pk = K.pack_weight_frags(dev(w2.t().contiguous()), bf, 192, 1)
    w1t_pk = K.pack_weight_frags(dev(w1.t().contiguous()), bf, 32, 1)
    wpt_pk = K.pack_weight_frags(dev(wp.t().contiguous()), bf, 192, 1)
    dg2, db2 = torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")
    dx2, du2, da2 = K.block_tail2_bwd(dev(dy, bf), dev(q(gp, "bf16"), torch.float16), w2t_pk, w1t_pk, xd, mean, rstd, dev(g), dg2, db2, wpt_pk)
    # fp32 math on the rounded operands, stage by stage from the kernel's own (rounded) intermediates
    dyq, gpq, xq = q(dy, "bf16"), q(gp, "bf16"), q(x, "bf16")
    du_ref = (dyq @ q(w2, "bf16")) * gpq
    assert rel_err(du2.float().cpu(), du_ref) < 6e-3
    dxn = du2.float().cpu() @ q(w1, "bf16")                      # [M, D]
    mu, rs = mean.cpu()[:, None], rstd.cpu()[:, None]
    xhat = (xq - mu) * rs
    gy = dxn * g
    dx_ref = dyq + rs * (gy - gy.mean(1, keepdim=True) - xhat * (gy * xhat).mean(1, keepdim=True))
    assert rel_err(dx2.float().cpu(), dx_ref) < 6e-3
    assert rel_err(dg2.cpu(), (dxn * xhat).sum(0)) < 2e-3 and rel_err(db2.cpu(), dxn.sum(0)) < 2e-3
    assert rel_err(da2.float().cpu(), dx2.float().cpu() @ q(wp, "bf16")) < 6e-3


@pytest.mark.parametrize("M,Kd", [(650, 576), (33280, 576), (13, 192), (16 * 2048 + 16 * 40 + 3, 384)])
def test_linear_lnbwd2_equals_the_panel_kernel(K, M, Kd):
    """dx = dres + LayerNorm'(dY W) on the wave-per-tile mapping (packed W^T) against vitpe_linear_lnbwd and fp32 math."""
    D, bf = 192, torch.bfloat16
    x, g = rnd(M, D, seed=51), 1 + 0.1 * rnd(D, seed=52)
    dy, dres = rnd(M, Kd, seed=53), rnd(M, D, seed=54)
    w = rnd(Kd, D, seed=55, scale=0.06)                       # the Linear's weight [K, 192]
    xd = dev(x, bf)
    _, mean, rstd = K.layernorm_fwd(xd, dev(g), torch.zeros(D, device="cuda"))
    dg2, db2 = torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")
    dx2 = K.linear_lnbwd2(dev(dy, bf), K.pack_weight_frags(dev(w.t().contiguous()), bf, 64, 0), xd, mean, rstd, dev(g),
                          dev(dres, bf), dg2, db2)
    dg1, db1 = torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")
    dx1 = K.linear_lnbwd(dev(dy, bf), dev(w.t().contiguous(), bf), xd, mean, rstd, dev(g), dev(dres, bf), dg1, db1)
    assert rel_err(dx2.float().cpu(), dx1.float().cpu()) < 8e-3
    assert rel_err(dg2.cpu(), dg1.cpu()) < 5e-3 and rel_err(db2.cpu(), db1.cpu()) < 5e-3
    dxn = q(dy, "bf16") @ q(w, "bf16")
    mu, rs = mean.cpu()[:, None], rstd.cpu()[:, None]
    xhat = (q(x, "bf16") - mu) * rs
    gy = dxn * g
    ref = q(dres, "bf16") + rs * (gy - gy.mean(1, keepdim=True) - xhat * (gy * xhat).mean(1, keepdim=True))
    assert rel_err(dx2.float().cpu(), ref) < 6e-3
    assert rel_err(dg2.cpu(), (dxn * xhat).sum(0)) < 2e-3 and rel_err(db2.cpu(), dxn.sum(0)) < 2e-3


@pytest.mark.parametrize("M,HID,K1", [(650, 768, 576), (33280, 768, 576), (13, 128, 192), (16 * 300 + 5, 768, 384), (100, 256, 320), (40, 128, 64)])
def test_block_tail2_backward_with_fused_qkv_gradient_prologue(K, M, HID, K1):
    """vitpe_block_tail2_bwd_pre == vitpe_linear_lnbwd2 (the upper block's qkv data gradient + LayerNorm1 backward + residual)
    followed by vitpe_block_tail2_bwd on its output: same dy, du, dx_mid, da and both pairs of LayerNorm gradients."""
    D, bf = 192, torch.bfloat16
    dq, wq = rnd(M, K1, seed=61), rnd(K1, D, seed=62, scale=0.06)
    x1, g1, dres1 = rnd(M, D, seed=63), 1 + 0.1 * rnd(D, seed=64), rnd(M, D, seed=65)
    xm, g2 = rnd(M, D, seed=66), 1 + 0.1 * rnd(D, seed=67)
    gp = 0.5 + 0.6 * rnd(M, HID, seed=68)
    w2, w1, wp = rnd(D, HID, seed=69, scale=0.05), rnd(HID, D, seed=70, scale=0.08), rnd(D, D, seed=71, scale=0.07)
    x1d, xmd = dev(x1, bf), dev(xm, bf)
    _, m1, r1 = K.layernorm_fwd(x1d, dev(g1), torch.zeros(D, device="cuda"))
    _, m2, r2 = K.layernorm_fwd(xmd, dev(g2), torch.zeros(D, device="cuda"))
    wqt_pk = K.pack_weight_frags(dev(wq.t().contiguous()), bf, 64, 0)
    w2t_pk = K.pack_weight_frags(dev(w2.t().contiguous()), bf, 192, 1)
    w1t_pk = K.pack_weight_frags(dev(w1.t().contiguous()), bf, 32, 1)
    wpt_pk = K.pack_weight_frags(dev(wp.t().contiguous()), bf, 192, 1)
    z = lambda: torch.zeros(D, device="cuda")  # noqa: E731
    # the two launches
    dg1a, db1a, dg2a, db2a = z(), z(), z(), z()
    if K1 % 192 == 0:
        dy_a = K.linear_lnbwd2(dev(dq, bf), wqt_pk, x1d, m1, r1, dev(g1), dev(dres1, bf), dg1a, db1a)
    else:   # widths the stand-alone kernel does not take (it streams 192-wide slabs): the generic pair of launches
        dxn = K.linear(dev(dq, bf), dev(wq.t().contiguous(), bf), None)
        dy_a = K.layernorm_bwd(dxn, x1d, m1, r1, dev(g1), dg1a, db1a, dres=dev(dres1, bf))
    dx_a, du_a, da_a = K.block_tail2_bwd(dy_a, dev(gp, torch.float16), w2t_pk, w1t_pk, xmd, m2, r2, dev(g2), dg2a, db2a, wpt_pk)
    # the fused launch
    dg1b, db1b, dg2b, db2b = z(), z(), z(), z()
    dy_b = torch.empty(M, D, device="cuda", dtype=bf)
    dx_b, du_b, da_b = K.block_tail2_bwd_pre(dev(dq, bf), wqt_pk, x1d, m1, r1, dev(g1), dev(dres1, bf), dg1b, db1b, dy_b,
                                             dev(gp, torch.float16), w2t_pk, w1t_pk, xmd, m2, r2, dev(g2), dg2b, db2b, wpt_pk)
    if K1 % 192 == 0:
        assert torch.equal(dy_b.cpu(), dy_a.cpu())
        assert torch.equal(du_b.cpu(), du_a.cpu()) and torch.equal(dx_b.cpu(), dx_a.cpu()) and torch.equal(da_b.cpu(), da_a.cpu())
        tol = 1e-5                                          # fp32 atomics in a different order
    else:                                                   # the generic pair rounds dxn to bf16 between its launches
        for u_, v_ in ((dy_b, dy_a), (du_b, du_a), (dx_b, dx_a), (da_b, da_a)):
            assert rel_err(u_.float().cpu(), v_.float().cpu()) < 1.5e-2
        tol = 4e-3
    for u_, v_ in ((dg1b, dg1a), (db1b, db1a), (dg2b, dg2a), (db2b, db2a)):
        assert rel_err(u_.cpu(), v_.cpu()) < tol


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_wgrad_group_many_problems_one_launch(K, dt):
    """Ragged problem list (block edges, M not a multiple of the stage, with / without bias, repeated
    launches accumulate): every problem against dY^T X on the values the kernel sees."""
    shapes = [(650, 576, 192, True), (650, 192, 192, True), (333, 768, 192, True), (333, 192, 768, True),
              (195, 96, 96, False), (260, 192, 48, True), (70, 200, 392, True), (1, 8, 8, True)]
    probs, refs = [], []
    for i, (M, N, K_, bias) in enumerate(shapes):
        dy, x = rnd(M, N, seed=10 + i), rnd(M, K_, seed=40 + i)
        dw = torch.zeros(N, K_, device="cuda")
        db = torch.zeros(N, device="cuda") if bias else None
        probs.append((dev(dy, DT[dt]), dev(x, DT[dt]), dw, db))
        refs.append((q(dy, dt).t() @ q(x, dt), q(dy, dt).sum(0)))
    grp = K.WgradGroup(probs)
    grp.launch()
    for (dy, x, dw, db), (rw, rb) in zip(probs, refs):
        assert rel_err(dw.cpu(), rw) < tol(dt), tuple(dw.shape)
        if db is not None:
            assert rel_err(db.cpu(), rb) < tol(dt), tuple(dw.shape)
    grp.launch()   # accumulates
    for (dy, x, dw, db), (rw, rb) in zip(probs, refs):
        assert rel_err(dw.cpu(), 2 * rw) < tol(dt)


@pytest.mark.parametrize("M", [64, 640, 65 * 64])
def test_wgrad_group_full_blocks_and_stages(K, M):
    """bf16 with every M a multiple of 64 and every N, K a multiple of 192 (the shapes of the bench path): work runs crossing
    block and problem boundaries, one- and two-stage problems, bias on and off, accumulation over launches; per-row check on
    one problem."""
    shapes = [(M, 576, 192, True), (M, 192, 192, True), (2 * M, 768, 192, True), (M, 192, 768, False), (64, 192, 384, True),
              (128, 384, 192, True)]
    probs, refs = [], []
    for i, (M_, N, K_, bias) in enumerate(shapes):
        dy, x = rnd(M_, N, seed=110 + i), rnd(M_, K_, seed=140 + i)
        dw = torch.zeros(N, K_, device="cuda")
        db = torch.zeros(N, device="cuda") if bias else None
        probs.append((dev(dy, torch.bfloat16), dev(x, torch.bfloat16), dw, db))
        refs.append((q(dy, "bf16").t() @ q(x, "bf16"), q(dy, "bf16").sum(0)))
    grp = K.WgradGroup(probs)
    grp.launch()
    for (dy, x, dw, db), (rw, rb) in zip(probs, refs):
        assert rel_err(dw.cpu(), rw) < BF16_TOL, tuple(dw.shape)
        if db is not None:
            assert rel_err(db.cpu(), rb) < BF16_TOL, tuple(dw.shape)
    d0, r0 = probs[0][2].cpu(), refs[0][0]
    for row in (0, 47, 48, 191, 192, 575):     # wave-tile and block edges: a misplaced tile shows in its own rows
        assert rel_err(d0[row], r0[row]) < BF16_TOL, row
    grp.launch()   # accumulates
    for (dy, x, dw, db), (rw, rb) in zip(probs, refs):
        assert rel_err(dw.cpu(), 2 * rw) < BF16_TOL


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_wgrad_group_window_mode_many_blocks(K, dt):
    """A list of more than two chip-fulls of 192 x 192 blocks (the ViT-B/16 weight gradients: 1 152 per launch) is run in
    windows of whole blocks, the last partial window in row ranges: every problem against dY^T X, ragged edges included."""
    shapes = [(192, 960, 960, True)] * 10 + [(200, 960, 904, False)] * 8 + [(64, 1152, 768, True)] * 4 + [(330, 200, 392, True)] * 2
    probs, refs = [], []
    for i, (M, N, K_, bias) in enumerate(shapes):
        dy, x = rnd(M, N, seed=210 + i), rnd(M, K_, seed=250 + i)
        dw = torch.zeros(N, K_, device="cuda")
        db = torch.zeros(N, device="cuda") if bias else None
        probs.append((dev(dy, DT[dt]), dev(x, DT[dt]), dw, db))
        refs.append((q(dy, dt).t() @ q(x, dt), q(dy, dt).sum(0)))
    assert sum(-(-N // 192) * -(-K_ // 192) for _, N, K_, _ in shapes) >= 2 * 256
    grp = K.WgradGroup(probs)
    grp.launch()
    for (dy, x, dw, db), (rw, rb) in zip(probs, refs):
        assert rel_err(dw.cpu(), rw) < tol(dt), tuple(dw.shape)
        if db is not None:
            assert rel_err(db.cpu(), rb) < tol(dt), tuple(dw.shape)
    for row in (0, 191, 192, 959):
        assert rel_err(probs[0][2][row].cpu(), refs[0][0][row]) < tol(dt), row
    grp.launch()   # accumulates
    for (dy, x, dw, db), (rw, rb) in zip(probs, refs):
        assert rel_err(dw.cpu(), 2 * rw) < tol(dt)


@pytest.mark.parametrize("case", ["one problem", "few blocks", "table", "windows", "ragged rows"])
def test_wgrad_group_wide_blocks(K, case):
    """Lists whose every problem has N % 192 == 0 and K % 384 == 0 (bf16, plain X) run on the 192 x 384-block kernel
    (LDS-DMA staging, 96 x 96 wave tiles): stream-K, table, window placements; bias on / off; a partial last stage (rows
    past M are zeroed in LDS); two launches accumulate (checked as 2 x); every problem against dY^T X with per-row checks."""
    shapes = {"one problem": [(640, 192, 384, True)],
              "few blocks": [(64 * 9, 384, 768, True), (64 * 9, 192, 384, False), (64 * 5, 768, 768, True)],
              "table": [(64 * 40, 768, 768, True), (64 * 40, 2304, 768, False), (64 * 40, 768, 3072, True), (64 * 40, 3072, 768, True)],
              "windows": [(64 * 6, 2304, 768, False), (64 * 6, 768, 768, True), (64 * 6, 3072, 768, True), (64 * 6, 768, 3072, True)] * 6,
              "ragged rows": [(64 * 3 + 17, 384, 768, True), (1, 192, 384, True), (130, 576, 384, False)]}[case]
    probs, refs = [], []
    for i, (M, N, K_, bias) in enumerate(shapes):
        dy, x = rnd(M, N, seed=310 + i), rnd(M, K_, seed=350 + i)
        dw = torch.zeros(N, K_, device="cuda")
        db = torch.zeros(N, device="cuda") if bias else None
        probs.append((dev(dy, torch.bfloat16), dev(x, torch.bfloat16), dw, db))
        refs.append((q(dy, "bf16").t() @ q(x, "bf16"), q(dy, "bf16").sum(0)))
    if case == "windows":
        assert sum((N // 192) * (K_ // 384) for _, N, K_, _ in shapes) >= 2 * 256
    from vitpe import _lib as L
    grp = K.WgradGroup(probs)
    assert L.debug_lib().vitpe_debug_set_wgrad_wide(1) == 0      # (the default)
    grp.launch()
    grp.launch()   # accumulates
    snap = [(dw.clone(), None if db is None else db.clone()) for _, _, dw, db in probs]
    for (dy, x, dw, db), (rw, rb) in zip(probs, refs):
        dw *= 0.5
        if db is not None:
            db *= 0.5
    for (dy, x, dw, db), (rw, rb) in zip(probs, refs):
        assert rel_err(dw.cpu(), rw) < tol("bf16"), tuple(dw.shape)
        worst = max(rel_err(dw[r_].cpu(), rw[r_]) for r_ in (0, 95, 96, dw.shape[0] - 1))
        assert worst < 2 * tol("bf16"), (tuple(dw.shape), worst)
        assert rel_err(dw[:, -97:].cpu(), rw[:, -97:]) < 2 * tol("bf16")
        if db is not None:
            assert rel_err(db.cpu(), rb) < tol("bf16"), tuple(dw.shape)
    # the same list on the 192 x 192 kernel (debug switch): same sums up to the order of the fp32 atomics
    try:
        L.debug_lib().vitpe_debug_set_wgrad_wide(0)
        for _, _, dw, db in probs:
            dw.zero_()
            if db is not None:
                db.zero_()
        grp.launch()
        grp.launch()
    finally:
        L.debug_lib().vitpe_debug_set_wgrad_wide(1)
    for (dy, x, dw, db), (dw_w, db_w) in zip(probs, snap):
        assert rel_err(dw.cpu(), dw_w.cpu()) < 1e-4
        if db is not None:
            assert rel_err(db.cpu(), db_w.cpu()) < 1e-4


def test_wgrad_group_range_major_windows_model_sized_list(K):
    """A list the size of the CIFAR model's (24 nn.Linear problems, 72 blocks of 192 x 192) with enough rows for seven row
    ranges per block: 504 (range, block) pairs dealt range-major over two rounds of the chip, a partial flush per pair."""
    M = 64 * 29 + 17
    probs, refs = [], []
    for i, (N, K_) in enumerate([(576, 192), (192, 192), (768, 192), (192, 768)] * 6):
        dy, x = rnd(M, N, seed=310 + i), rnd(M, K_, seed=350 + i)
        dw, db = torch.zeros(N, K_, device="cuda"), torch.zeros(N, device="cuda")
        probs.append((dev(dy, torch.bfloat16), dev(x, torch.bfloat16), dw, db))
        refs.append((q(dy, "bf16").t() @ q(x, "bf16"), q(dy, "bf16").sum(0)))
    K.wgrad_group(probs)
    for (dy, x, dw, db), (rw, rb) in zip(probs, refs):
        assert rel_err(dw.cpu(), rw) < BF16_TOL and rel_err(db.cpu(), rb) < BF16_TOL, tuple(dw.shape)
    for row in (0, 191, 192, 575):
        assert rel_err(probs[0][2][row].cpu(), refs[0][0][row]) < BF16_TOL, row


def test_wgrad_group_large_balanced_run(K):
    """bench-like sizes (many stages per block, work runs crossing block and problem boundaries)"""
    M = 65 * 96
    probs, refs = [], []
    for i, (N, K_) in enumerate([(576, 192), (192, 192), (768, 192), (192, 768)] * 2):
        dy, x = rnd(M, N, seed=70 + i), rnd(M, K_, seed=90 + i)
        dw, db = torch.zeros(N, K_, device="cuda"), torch.zeros(N, device="cuda")
        probs.append((dev(dy, torch.bfloat16), dev(x, torch.bfloat16), dw, db))
        refs.append((q(dy, "bf16").t() @ q(x, "bf16"), q(dy, "bf16").sum(0)))
    K.wgrad_group(probs)
    for (dy, x, dw, db), (rw, rb) in zip(probs, refs):
        assert rel_err(dw.cpu(), rw) < 1e-4     # bf16 products are exact in fp32; only the summation order differs
        assert rel_err(db.cpu(), rb) < 1e-4


@pytest.mark.parametrize("M", [65 * 64, 65 * 64 + 7])
def test_wgrad_group_whole_model_list(K, M):
    """A whole-model problem list (6 x {fc2, fc1, proj, qkv} + patch embed), the shape of the engine's launch: big
    enough for the XCD-co-located (block, token-range) table; ragged last stage when M % 64 != 0."""
    D, hid = 192, 768
    probs, refs = [], []
    shapes = [(D, hid, True), (hid, D, True), (D, D, True), (3 * D, D, False)] * 6 + [(D, 48, True)]
    for i, (N, K_, bias) in enumerate(shapes):
        dy, x = rnd(M, N, seed=200 + i), rnd(M, K_, seed=300 + i)
        dw = torch.zeros(N, K_, device="cuda")
        db = torch.zeros(N, device="cuda") if bias else None
        probs.append((dev(dy, torch.bfloat16), dev(x, torch.bfloat16), dw, db))
        refs.append((q(dy, "bf16").t() @ q(x, "bf16"), q(dy, "bf16").sum(0)))
    grp = K.WgradGroup(probs)
    grp.launch()
    for (dy, x, dw, db), (rw, rb) in zip(probs, refs):
        assert rel_err(dw.cpu(), rw) < 1e-4, tuple(dw.shape)
        if db is not None:
            assert rel_err(db.cpu(), rb) < 1e-4, tuple(dw.shape)
    grp.launch()   # accumulates
    for (dy, x, dw, db), (rw, rb) in zip(probs, refs):
        assert rel_err(dw.cpu(), 2 * rw) < 1e-4


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_wgrad_group_layernorm_operand_is_recomputed_in_the_kernel(K, dt):
    """x_op = LayerNorm: the X operand is the RAW rows plus their statistics and the affine parameters; the kernel's
    dW must equal dY^T LayerNorm(X) (oracle: torch layer_norm in fp32 on the values the kernel sees), next to plain
    problems in the same launch.  Shapes of the engine's fc1 and qkv problems, M ragged."""
    probs, refs = [], []
    for i, (M, N, K_, bias, ln) in enumerate([(650, 768, 192, True, True), (650, 576, 192, False, True),
                                             (333, 192, 768, True, False), (199, 384, 192, True, True)]):
        dy, x = rnd(M, N, seed=500 + i), rnd(M, K_, seed=540 + i) * 2 + 0.3
        gam, bet = rnd(K_, seed=560 + i) + 1.5, rnd(K_, seed=580 + i)
        dw = torch.zeros(N, K_, device="cuda")
        db = torch.zeros(N, device="cuda") if bias else None
        xq = q(x, dt)
        if ln:
            _, mean, rstd = K.layernorm_fwd(dev(x, DT[dt]).view(1, M, K_), dev(gam), dev(bet), stats_only=True)
            xn = torch.nn.functional.layer_norm(xq, (K_,), gam, bet, 1e-5)
            probs.append((dev(dy, DT[dt]), dev(x, DT[dt]), dw, db, (mean, rstd, dev(gam), dev(bet))))
            refs.append((q(dy, dt).t() @ xn, q(dy, dt).sum(0)))
        else:
            probs.append((dev(dy, DT[dt]), dev(x, DT[dt]), dw, db))
            refs.append((q(dy, dt).t() @ xq, q(dy, dt).sum(0)))
    grp = K.WgradGroup(probs)
    grp.launch()
    for prob, (rw, rb) in zip(probs, refs):
        dw, db = prob[2], prob[3]
        assert rel_err(dw.cpu(), rw) < (2e-4 if dt == "f32" else 1e-2), tuple(dw.shape)   # bf16: xhat rounded to bf16 once
        if db is not None:
            assert rel_err(db.cpu(), rb) < tol(dt)


def test_wgrad_group_rejects_bad_lists(K):
    from vitpe._lib import VitpeError
    with pytest.raises(VitpeError):
        K.WgradGroup([])
    dy, x = torch.zeros(8, 8, device="cuda"), torch.zeros(8, 8, device="cuda")
    with pytest.raises(VitpeError):
        K.WgradGroup([(dy, x, torch.zeros(8, 8, device="cuda"), None)] * (K.WgradGroup.MAX + 1))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("M,D", [(195, 192), (67, 96), (33, 768), (4500, 768), (5, 1024), (300, 1024)])
def test_layernorm_fwd_bwd(K, dt, M, D):
    x, g, b = rnd(M, D, seed=1, scale=2.0) + 0.3, 1 + 0.1 * rnd(D, seed=2), 0.1 * rnd(D, seed=3)
    dy, dres = rnd(M, D, seed=4), rnd(M, D, seed=5)
    xr = q(x, dt).requires_grad_(True)
    gr, br = g.clone().requires_grad_(True), b.clone().requires_grad_(True)
    yr = torch.nn.functional.layer_norm(xr, (D,), gr, br, 1e-5)
    yr.backward(q(dy, dt))
    y, mean, rstd = K.layernorm_fwd(dev(x, DT[dt]), dev(g), dev(b))
    assert rel_err(y.float().cpu(), yr.detach()) < tol(dt)
    assert rel_err(mean.cpu(), x.to(DT[dt]).float().mean(-1)) < 1e-5
    assert rel_err(rstd.cpu(), (q(x, dt).double().var(-1, unbiased=False) + 1e-5).rsqrt()) < 1e-5
    dgam = torch.zeros(D, device="cuda")
    dbet = torch.zeros(D, device="cuda")
    dx = K.layernorm_bwd(dev(dy, DT[dt]), dev(x, DT[dt]), mean, rstd, dev(g), dgam, dbet, dres=dev(dres, DT[dt]))
    assert rel_err(dx.float().cpu(), xr.grad + q(dres, dt)) < tol(dt)
    assert rel_err(dgam.cpu(), gr.grad) < tol(dt)
    assert rel_err(dbet.cpu(), br.grad) < tol(dt)


# ------------------------------------------------------------------------------------------
ATTN_MODES = ["none", "relative", "polynomial", "polynomial_perhead", "rope-axial", "rope-mixed"]


def attn_case(mode, D, H, B, seed=0, G=8):
    """inputs + oracle outputs for the attention ops (default N=65: 32x32 images, patch 4)."""
    N, hd = G * G + 1, D // H
    xn = rnd(B, N, D, seed=seed + 1)
    wqkv = rnd(3 * D, D, seed=seed + 2, scale=0.3)
    dout = rnd(B, N, D, seed=seed + 3)
    pe = {}
    if mode == "relative":
        pe["table"] = rnd(H, 2 * N - 1, seed=seed + 4, scale=0.5)
    elif mode.startswith("polynomial"):
        shp = (4,) if mode == "polynomial" else (H, 4)
        pe["coeff"] = rnd(*shp, seed=seed + 5, scale=0.4) * torch.tensor([1.0, 1 / 8, 1 / 64, 1 / 512])
    elif mode == "rope-axial":
        pe["inv_freq"] = O.rope_axial_inv_freq(hd, 100.0)
    elif mode == "rope-mixed":
        pe["freqs"] = rnd(2, H, hd // 2, seed=seed + 6, scale=0.7)
    return N, hd, G, xn, wqkv, dout, pe


def oracle_attn(mode, xn, wqkv, dout, pe, H, dt):
    N = xn.shape[1]
    xn_, w_ = q(xn, dt), q(wqkv, dt)
    leaves = {k: v.clone().requires_grad_(k != "inv_freq") for k, v in pe.items()}
    freqs_cis = bias = None
    if mode == "relative":
        bias = O.relative_bias(leaves["table"], N)
    elif mode.startswith("polynomial"):
        bias = O.polynomial_bias(leaves["coeff"], N - 1, H, 3, mode == "polynomial")
    elif mode == "rope-axial":
        freqs_cis = O.rope_axial_tables(N - 1, leaves["inv_freq"])
    elif mode == "rope-mixed":
        freqs_cis = O.rope_mixed_tables(N - 1, leaves["freqs"])
    B, _, D = xn.shape
    hd = D // H
    qkv = torch.nn.functional.linear(xn_, w_).requires_grad_(True)
    qkv_h = qkv.reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    o = O.attention_core(qkv_h[0], qkv_h[1], qkv_h[2], hd ** -0.5, freqs_cis, bias)
    out = o.transpose(1, 2).reshape(B, N, D)
    out.backward(q(dout, dt))
    grads = {k: v.grad for k, v in leaves.items() if v.requires_grad}
    return out.detach(), qkv.grad, grads


def device_pe(K, mode, pe, H, G):
    from vitpe.kernels import PETables
    m = "polynomial" if mode.startswith("polynomial") else mode
    t = PETables(m, G)
    if mode == "relative":
        t.table = dev(pe["table"])
    elif mode.startswith("polynomial"):
        t.coeff, t.degree, t.coeff_per_head = dev(pe["coeff"]), 3, mode != "polynomial"
    elif mode == "rope-axial":
        t.cos, t.sin = K.rope_axial_tables(dev(pe["inv_freq"]), G)
    elif mode == "rope-mixed":
        t.cos, t.sin = K.rope_mixed_tables(dev(pe["freqs"]), G)
    return t


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("mode", ATTN_MODES)
@pytest.mark.parametrize("D,H,B", [(192, 6, 3), (96, 3, 2)])
def test_fused_attention_fwd(K, dt, mode, D, H, B):
    N, hd, G, xn, wqkv, dout, pe = attn_case(mode, D, H, B)
    ref, _, _ = oracle_attn(mode, xn, wqkv, dout, pe, H, dt)
    t = device_pe(K, mode, pe, H, G)
    out = K.fused_attention_fwd(dev(xn, DT[dt]), K.pack_qkv_weights(dev(wqkv), DT[dt], H), H, t)
    assert rel_err(out.float().cpu(), ref) < tol(dt)


def test_wide_qkv_pack_layout(K):
    """vitpe_pack_qkv_weights_wide against its definition (include/vitpe.h): block ((h * 3 + mat) * 12 + s) x 64 lanes x 8,
    lane (r, hh), element j <- W[mat D + 32 h + r][16 s + 8 hh + j], q rows x hd^-0.5 log2(e)."""
    D, H = 192, 6
    W = rnd(3 * D, D, seed=77, scale=0.3)
    got = K.pack_qkv_weights_wide(dev(W), torch.bfloat16, H).float().cpu().view(H, 3, D // 16, 2, 32, 8)   # [h][mat][s][hh][r][j]
    Wv = W.view(3, H, 32, D // 16, 2, 8).permute(1, 0, 3, 4, 2, 5).clone()                                    # same index order
    Wv[:, 0] *= math.log2(math.e) / math.sqrt(32)
    assert torch.equal(got, Wv.bfloat16().float())


@pytest.mark.parametrize("ln", [False, True])
@pytest.mark.parametrize("mode", ATTN_MODES)
@pytest.mark.parametrize("B", [3, 512])
def test_fused_attention_fwd_wide(K, mode, B, ln):
    """The 32x32-tile forward (csrc/attn32.hip; bf16, N = 65, d = 192) against the oracle: an odd batch (idle second image
    slot of the last workgroup) and the batch the benchmark is quoted on; with the LayerNorm fused into the staging, the
    normalised side output must equal the stand-alone LayerNorm kernel's."""
    D, H = 192, 6
    N, hd, G, x, wqkv, dout, pe = attn_case(mode, D, H, B, seed=31)
    assert K.fused_attention_wide_supported(torch.bfloat16, N, D, hd)
    t = device_pe(K, mode, pe, H, G)
    w = K.pack_qkv_weights_wide(dev(wqkv), torch.bfloat16, H)
    if ln:
        xr = dev(x * 1.7 + 0.4, torch.bfloat16)
        gam, bet = dev(1 + 0.1 * rnd(D, seed=5)), dev(0.1 * rnd(D, seed=6))
        xn, mean, rstd = K.layernorm_fwd(xr, gam, bet)
        xo = torch.empty_like(xr)
        out = K.fused_attention_fwd_wide(xr, w, H, t, ln=(gam, bet, mean, rstd), xn_out=xo)
        assert rel_err(xo.float().cpu(), xn.float().cpu()) < 1e-2   # (one bf16 ulp: the two kernels order the LayerNorm arithmetic differently)
        ref, _, _ = oracle_attn(mode, xo.float().cpu(), wqkv, dout, pe, H, "bf16")
    else:
        out = K.fused_attention_fwd_wide(dev(x, torch.bfloat16), w, H, t)
        ref, _, _ = oracle_attn(mode, x, wqkv, dout, pe, H, "bf16")
    assert torch.isfinite(out.float()).all()
    assert rel_err(out.float().cpu(), ref) < BF16_TOL


@pytest.mark.parametrize("mode", ["rope-axial", "polynomial"])
@pytest.mark.parametrize("B", [511, 512])
def test_fused_attention_at_the_benchmark_batch(K, mode, B):
    """Forward (16x16-tile kernel) and backward at the batch the metric is quoted on and one image less (the odd batch
    exercises the idle second image slot of the last two-image workgroup): a chip-full of workgroups against the oracle."""
    D, H = 192, 6
    N, hd, G, xn, wqkv, dout, pe = attn_case(mode, D, H, B, seed=41)
    ref, dqkv_ref, g_ref = oracle_attn(mode, xn, wqkv, dout, pe, H, "bf16")
    t = device_pe(K, mode, pe, H, G)
    w = K.pack_qkv_weights(dev(wqkv), torch.bfloat16, H)
    out = K.fused_attention_fwd(dev(xn, torch.bfloat16), w, H, t)
    assert rel_err(out.float().cpu(), ref) < BF16_TOL
    dcoef = torch.zeros_like(dev(pe["coeff"])) if mode == "polynomial" else None
    dqkv = K.fused_attention_bwd(dev(xn, torch.bfloat16), w, dev(dout, torch.bfloat16), H, t, None, dcoef, None)
    assert rel_err(dqkv.float().cpu(), dqkv_ref) < BF16_TOL
    if mode == "polynomial":
        assert rel_err(dcoef.cpu(), g_ref["coeff"]) < BF16_TOL


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("mode", ATTN_MODES)
@pytest.mark.parametrize("D,H,B", [(192, 6, 3), (96, 3, 2)])
def test_fused_attention_bwd(K, dt, mode, D, H, B):
    N, hd, G, xn, wqkv, dout, pe = attn_case(mode, D, H, B, seed=10)
    _, dqkv_ref, g_ref = oracle_attn(mode, xn, wqkv, dout, pe, H, dt)
    t = device_pe(K, mode, pe, H, G)
    dtab = torch.zeros(H, 2 * N - 1, device="cuda") if mode == "relative" else None
    dcoef = torch.zeros_like(dev(pe["coeff"])) if mode.startswith("polynomial") else None
    dfr = torch.zeros(2, H, hd // 2, device="cuda") if mode == "rope-mixed" else None
    dqkv = K.fused_attention_bwd(dev(xn, DT[dt]), K.pack_qkv_weights(dev(wqkv), DT[dt], H), dev(dout, DT[dt]), H, t,
                                 dtab, dcoef, dfr)
    assert rel_err(dqkv.float().cpu(), dqkv_ref) < tol(dt)
    if mode == "relative":
        assert rel_err(dtab.cpu(), g_ref["table"]) < tol(dt)
    if mode.startswith("polynomial"):
        assert rel_err(dcoef.cpu(), g_ref["coeff"]) < tol(dt)
    if mode == "rope-mixed":
        assert rel_err(dfr.cpu(), g_ref["freqs"]) < max(tol(dt), 2e-4)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("mode", ["rope-axial", "relative"])
def test_fused_attention_bwd_with_layernorm_recomputed(K, dt, mode):
    """vitpe_fused_attention_bwd_ln (raw tokens + statistics) against vitpe_fused_attention_bwd on the normalised
    tokens the forward would have stored: same d_qkv."""
    D, H, B = 192, 6, 3
    N, hd, G, x, wqkv, dout, pe = attn_case(mode, D, H, B, seed=21)
    x = x * 1.7 + 0.4
    gam, bet = dev(rnd(D, seed=5) + 1.2), dev(rnd(D, seed=6))
    t = device_pe(K, mode, pe, H, G)
    xd = dev(x, DT[dt])
    xn, mean, rstd = K.layernorm_fwd(xd, gam, bet)
    w = K.pack_qkv_weights(dev(wqkv), DT[dt], H)
    mk = lambda: (torch.zeros(H, 2 * N - 1, device="cuda") if mode == "relative" else None)  # noqa: E731
    d0, d1 = mk(), mk()
    a = K.fused_attention_bwd(xn, w, dev(dout, DT[dt]), H, t, d0)
    b_ = K.fused_attention_bwd(xd, w, dev(dout, DT[dt]), H, t, d1, ln=(gam, bet, mean, rstd))
    assert rel_err(b_.float().cpu(), a.float().cpu()) < (1e-5 if dt == "f32" else 2e-2)
    if mode == "relative":
        assert rel_err(d1.cpu(), d0.cpu()) < (1e-5 if dt == "f32" else 2e-2)


# attention core on a qkv buffer: CIFAR geometry (N=65, hd=32) and the ImageNet-shaped one of
# BASELINE config 5 (N=197, hd=64; d reduced to 2 heads x 64 so that the oracle stays fast -- the
# kernel's work is per (image, head) and independent of the number of heads)
CORE_SHAPES = [(192, 6, 2, 8), (128, 2, 2, 14), (768, 12, 1, 14)]


def core_qkv(xn, wqkv, dt):
    return torch.nn.functional.linear(q(xn, dt), q(wqkv, dt))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("mode", ATTN_MODES)
@pytest.mark.parametrize("D,H,B,G", CORE_SHAPES)
def test_attention_core_fwd(K, dt, mode, D, H, B, G):
    N, hd, G, xn, wqkv, dout, pe = attn_case(mode, D, H, B, seed=20, G=G)
    wqkv = wqkv * (0.3 if D > 200 else 1.0)
    ref, _, _ = oracle_attn(mode, xn, wqkv, dout, pe, H, dt)
    t = device_pe(K, mode, pe, H, G)
    out = K.attention_core_fwd(dev(core_qkv(xn, wqkv, dt), DT[dt]), H, t)
    # bf16: the oracle keeps qkv in fp32, the device buffer is rounded to bf16 first
    assert rel_err(out.float().cpu(), ref) < tol(dt)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("mode", ATTN_MODES)
@pytest.mark.parametrize("D,H,B,G", CORE_SHAPES)
def test_attention_core_bwd(K, dt, mode, D, H, B, G):
    N, hd, G, xn, wqkv, dout, pe = attn_case(mode, D, H, B, seed=30, G=G)
    wqkv = wqkv * (0.3 if D > 200 else 1.0)
    _, dqkv_ref, g_ref = oracle_attn(mode, xn, wqkv, dout, pe, H, dt)
    t = device_pe(K, mode, pe, H, G)
    dtab = torch.zeros(H, 2 * N - 1, device="cuda") if mode == "relative" else None
    dcoef = torch.zeros_like(dev(pe["coeff"])) if mode.startswith("polynomial") else None
    dfr = torch.zeros(2, H, hd // 2, device="cuda") if mode == "rope-mixed" else None
    dqkv = K.attention_core_bwd(dev(core_qkv(xn, wqkv, dt), DT[dt]), dev(dout, DT[dt]), H, t, dtab, dcoef, dfr)
    assert rel_err(dqkv.float().cpu(), dqkv_ref) < tol(dt)
    if mode == "relative":
        assert rel_err(dtab.cpu(), g_ref["table"]) < tol(dt)
    if mode.startswith("polynomial"):
        assert rel_err(dcoef.cpu(), g_ref["coeff"]) < tol(dt)
    if mode == "rope-mixed":
        assert rel_err(dfr.cpu(), g_ref["freqs"]) < max(tol(dt), 2e-4)


def test_attention_core_matches_fused_kernel(K):
    """Same geometry through both paths (bf16): the two kernels share the tile math."""
    mode, D, H, B = "rope-axial", 192, 6, 4
    N, hd, G, xn, wqkv, dout, pe = attn_case(mode, D, H, B, seed=40)
    t = device_pe(K, mode, pe, H, G)
    xb, wb = dev(xn, torch.bfloat16), dev(wqkv, torch.bfloat16)
    fused = K.fused_attention_fwd(xb, K.pack_qkv_weights(dev(wqkv), torch.bfloat16, H), H, t)
    core = K.attention_core_fwd(K.linear(xb.reshape(B * N, D), wb).reshape(B, N, 3 * D), H, t)
    assert rel_err(core.float().cpu(), fused.float().cpu()) < 2e-2


@pytest.mark.parametrize("mode", ATTN_MODES)
@pytest.mark.parametrize("D,H,B", [(128, 2, 3), (768, 12, 2)])
def test_attention_fused64_fwd(K, mode, D, H, B):
    """The one-kernel forward at the ViT-B/16 geometry (N = 197, hd = 64: qkv projection + PE + core per (image, head))
    against the oracle, against the two launches it replaces (vitpe_linear + vitpe_attention_core_fwd) on the same operands,
    and its raw-projection side output against the Linear's."""
    G, bf = 14, torch.bfloat16
    N, hd, G, xn, wqkv, dout, pe = attn_case(mode, D, H, B, seed=50, G=G)
    wqkv = wqkv * (0.3 if D > 200 else 1.0)
    assert N == 197 and hd == 64 and K.attention_fused64_supported(bf, N, H, hd)
    ref, _, _ = oracle_attn(mode, xn, wqkv, dout, pe, H, "bf16")
    t = device_pe(K, mode, pe, H, G)
    xb = dev(xn, bf)
    qkv_out = torch.full((B, N, 3 * D), float("nan"), device="cuda", dtype=bf)
    out = K.attention_fused64_fwd(xb, K.pack_weight_frags(dev(wqkv), bf, 64, 0), H, t, qkv_out=qkv_out)
    assert rel_err(out.float().cpu(), ref) < tol("bf16")
    qkv2 = K.linear(xb.reshape(B * N, D), dev(wqkv, bf)).reshape(B, N, 3 * D)
    assert rel_err(qkv_out.float().cpu(), qkv2.float().cpu()) < 8e-3          # other summation order, then one rounding
    out2 = K.attention_core_fwd(qkv2, H, t)
    assert rel_err(out.float().cpu(), out2.float().cpu()) < 1.5e-2
    out3 = K.attention_fused64_fwd(xb, K.pack_weight_frags(dev(wqkv), bf, 64, 0), H, t)      # inference: no side output
    assert torch.equal(out3.cpu(), out.cpu())


def test_attention_fused64_unsupported_shapes(K):
    bf = torch.bfloat16
    assert K.attention_fused64_supported(bf, 197, 12, 64) and K.attention_fused64_supported(bf, 208, 2, 64)
    assert not K.attention_fused64_supported(bf, 65, 6, 32) and not K.attention_fused64_supported(torch.float32, 197, 12, 64)
    assert not K.attention_fused64_supported(bf, 209, 12, 64) and not K.attention_fused64_supported(bf, 192, 12, 64)


def test_attention_core_unsupported_shape_is_an_error(K):
    from vitpe._lib import VitpeError
    from vitpe.kernels import PETables
    assert K.attention_core_supported(torch.bfloat16, 17, 32) and K.attention_core_supported(torch.float32, 257, 64)
    assert not K.attention_core_supported(torch.bfloat16, 65, 16) and not K.attention_core_supported(torch.bfloat16, 101, 32)
    with pytest.raises(VitpeError):   # head dimension 16 (e.g. --num_heads 12 at d = 192) has no instantiation
        K.attention_core_fwd(torch.zeros(1, 17, 3 * 32, device="cuda"), 2, PETables("none", 4))
    with pytest.raises(VitpeError):   # 101 tokens (7 tiles): not in the compiled set
        K.attention_core_fwd(torch.zeros(1, 101, 3 * 64, device="cuda"), 2, PETables("none", 10))


def test_pack_qkv_weights_layout(K):
    D, H, hd = 96, 3, 32
    w = rnd(3 * D, D, seed=3)
    pk = K.pack_qkv_weights(dev(w), torch.float32, H).cpu().reshape(H, 3, hd // 16, D // 32, 4, 16, 8)  # h,mat,nt,ks,g,c,e
    ref = w.reshape(3, H, hd // 16, 16, D // 32, 4, 8).permute(1, 0, 2, 4, 5, 3, 6)  # mat,h,nt,c,ks,g,e -> h,mat,nt,ks,g,c,e
    assert torch.equal(pk, ref)


def test_fused_attention_unsupported_shape_is_an_error(K):
    from vitpe._lib import VitpeError
    from vitpe.kernels import PETables
    xn = torch.zeros(1, 17, 64, device="cuda")
    w = torch.zeros(192, 64, device="cuda")
    with pytest.raises(VitpeError):
        K.fused_attention_fwd(xn, w, 2, PETables("none", 4))


# ------------------------------------------------------------------------------------------
def test_integer_tables_bit_exact(K, golden):
    g = golden("tables")
    for N in (65, 197):
        idx = K.relative_position_index(N, "cuda").cpu().numpy()
        assert idx.dtype == np.int64 and np.array_equal(idx, g[f"rel_index_{N}"])
        assert np.array_equal(idx, O.relative_position_index(N))
    for G in (8, 14):
        l1 = K.l1_distance_matrix(G, "cuda").cpu().numpy()
        assert l1.dtype == np.int64 and np.array_equal(l1, g[f"l1_{G}"])


def test_pe_float_tables_vs_golden(K, golden):
    g = golden("tables")
    for hd, P, G in ((32, 64, 8), (64, 196, 14)):
        cos, sin = K.rope_axial_tables(dev(torch.from_numpy(g[f"axial_inv_freq_hd{hd}"])), G)
        assert rel_err(cos.cpu(), g[f"axial_cos_hd{hd}_P{P}"]) < 1e-5
        assert rel_err(sin.cpu(), g[f"axial_sin_hd{hd}_P{P}"]) < 1e-5
    for H, hd, P, G in ((6, 32, 64, 8), (3, 32, 64, 8), (12, 64, 196, 14)):
        fr = O.closed_form_tensor("pos_embed.freqs", (2, H, hd // 2))
        cos, sin = K.rope_mixed_tables(dev(fr), G)
        assert rel_err(cos.cpu(), g[f"mixed_cos_H{H}_hd{hd}_P{P}"]) < 1e-5
        assert rel_err(sin.cpu(), g[f"mixed_sin_H{H}_hd{hd}_P{P}"]) < 1e-5
    tab = O.closed_form_tensor("pos_embed.relative_position_bias_table", (6, 129))
    assert np.array_equal(K.relative_bias(dev(tab), 65).cpu().numpy(), g["rel_bias_H6_N65"])
    c = O.closed_form_tensor("pos_embed.coefficients", (4,))
    assert rel_err(K.polynomial_bias(dev(c), 6, 8, 3, False).cpu(), g["poly_bias_H6_N65_shared"]) < 1e-5
    c = O.closed_form_tensor("pos_embed.coefficients", (6, 4))
    assert rel_err(K.polynomial_bias(dev(c), 6, 8, 3, True).cpu(), g["poly_bias_H6_N65_perhead"]) < 1e-5


def test_apply_rotary_vs_golden(K, golden):
    g = golden("rotary")
    qq = O.closed_form_tensor("rotary.q", (2, 6, 64, 32)) * 20
    kk = O.closed_form_tensor("rotary.k", (2, 6, 64, 32)) * 20
    cos, sin = K.rope_axial_tables(dev(O.rope_axial_inv_freq(32, 100.0)), 8)
    assert rel_err(K.apply_rotary(dev(qq), cos, sin).cpu(), g["axial_q"]) < 1e-5
    assert rel_err(K.apply_rotary(dev(kk), cos, sin).cpu(), g["axial_k"]) < 1e-5
    cos, sin = K.rope_mixed_tables(dev(O.closed_form_tensor("pos_embed.freqs", (2, 6, 16))), 8)
    assert rel_err(K.apply_rotary(dev(qq), cos, sin).cpu(), g["mixed_q"]) < 1e-5
    assert rel_err(K.apply_rotary(dev(kk), cos, sin).cpu(), g["mixed_k"]) < 1e-5


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("C,S,p", [(3, 32, 4), (1, 32, 4), (3, 224, 16)])
def test_unfold_and_patch_embed(K, dt, C, S, p):
    B, D = 3, 96
    cfg = O.VitConfig(img_size=S, patch_size=p, in_chans=C, embed_dim=D, depth=1, num_heads=3, pos_encoding="absolute")
    params = O.closed_form_params(cfg)
    img, _ = O.closed_form_batch(cfg, B)
    P = cfg.num_patches
    patches = K.unfold(dev(img), p, DT[dt])
    g = S // p
    ref_p = img.reshape(B, C, g, p, g, p).permute(0, 2, 4, 1, 3, 5).reshape(B * P, C * p * p)
    assert torch.equal(patches.float().cpu(), q(ref_p, dt))
    pq = {k: v for k, v in params.items()}
    pq["patch_embed.weight"] = q(params["patch_embed.weight"], dt)
    ref = O.patch_embed(cfg, pq, q(img, dt))
    w = dev(params["patch_embed.weight"].reshape(D, -1), DT[dt])
    ape = dev(params["pos_embed.pos_embed"][0, :P])
    tok = K.patch_embed_gemm(patches, w, dev(params["patch_embed.bias"]), dev(params["cls_token"].reshape(-1)), ape, B, P)
    assert rel_err(tok.float().cpu(), ref) < tol(dt)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_head_ce_fwd_bwd(K, dt):
    B, Ntok, D, Cn = 37, 65, 192, 10
    x = rnd(B, Ntok, D, seed=1, scale=2.0)
    g, b = 1 + 0.1 * rnd(D, seed=2), 0.1 * rnd(D, seed=3)
    wh, bh = rnd(Cn, D, seed=4, scale=0.3), rnd(Cn, seed=5, scale=0.1)
    labels = torch.randint(0, Cn, (B,), generator=torch.Generator().manual_seed(6))
    xr = q(x, dt).requires_grad_(True)
    leaves = [t.clone().requires_grad_(True) for t in (g, b, wh, bh)]
    y = torch.nn.functional.layer_norm(xr, (D,), leaves[0], leaves[1], 1e-5)
    logits_ref = torch.nn.functional.linear(y[:, 0], leaves[2], leaves[3])
    loss_ref = torch.nn.functional.cross_entropy(logits_ref, labels)
    loss_ref.backward()
    logits, ws = K.head_fwd(dev(x, DT[dt]), dev(g), dev(b), dev(wh), dev(bh), save=True)
    assert rel_err(logits.cpu(), logits_ref.detach()) < 1e-4
    out2, dlog = K.cross_entropy(logits, dev(labels))
    assert abs(float(out2[0]) - float(loss_ref)) < 1e-5
    assert int(out2[1]) == int((logits_ref.argmax(1) == labels).sum())
    grads = [torch.zeros_like(dev(t)) for t in (wh, bh, g, b)]
    dx = K.head_bwd(dlog, dev(wh), dev(g), ws, DT[dt], Ntok, grads[0], grads[1], grads[2], grads[3])
    assert rel_err(dx.float().cpu(), xr.grad) < tol(dt)
    assert rel_err(grads[0].cpu(), leaves[2].grad) < 1e-4
    assert rel_err(grads[1].cpu(), leaves[3].grad) < 1e-4
    assert rel_err(grads[2].cpu(), leaves[0].grad) < 1e-4
    assert rel_err(grads[3].cpu(), leaves[1].grad) < 1e-4


def test_adamw_matches_oracle(K):
    n = 10007
    p0, g0 = rnd(n, seed=1), rnd(n, seed=2, scale=0.1)
    params, st = {"w": p0.clone()}, O.AdamWState()
    p = dev(p0.clone())
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    hp = torch.zeros(16, device="cuda")
    hp[:5] = torch.tensor([1e-3, 0.9, 0.999, 1e-8, 0.01])
    hp[8] = 1.0
    shadow = torch.empty(n, dtype=torch.bfloat16, device="cuda")
    for step in range(3):
        gs = g0 * (step + 1)
        O.adamw_update(params, {"w": gs}, st)
        g = dev(gs.clone())
        K.adamw_step(p, g, m, v, hp, shadow_bf16=shadow, zero_grad=True)
        assert float(g.abs().max()) == 0.0
    assert rel_err(p.cpu(), params["w"]) < 1e-6
    assert torch.equal(shadow.cpu(), p.cpu().to(torch.bfloat16))
    assert float(hp[5]) == 3.0


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_transpose_cast(K, dt):
    src = rnd(576, 192, seed=1)
    out = K.transpose_cast(dev(src), DT[dt])
    assert torch.equal(out.float().cpu(), q(src, dt).t())
    assert torch.equal(K.cast(dev(src), DT[dt]).float().cpu(), q(src, dt))


def test_embed_bwd(K):
    B, Ntok, D = 5, 65, 96
    dtok = rnd(B, Ntok, D, seed=1)
    dcls = torch.zeros(D, device="cuda")
    dape = torch.zeros(Ntok - 1, D, device="cuda")
    dpatch = K.embed_bwd(dev(dtok), dcls, dape)
    assert rel_err(dcls.cpu(), dtok[:, 0].sum(0)) < 1e-5
    assert rel_err(dape.cpu(), dtok[:, 1:].sum(0)) < 1e-5
    assert torch.equal(dpatch.cpu(), dtok[:, 1:].reshape(-1, D))


# ---- resident uint8 input ---------------------------------------------------------------
@pytest.mark.parametrize("C,S,p,name", [(3, 32, 4, "cifar10"), (1, 32, 4, "mnist"), (3, 224, 16, "cifar10")])
def test_unfold_u8_gather_normalise_unfold(K, C, S, p, name):
    """vitpe_unfold_u8 == DataLoader gather + ToTensor + Normalize (oracle restatement of train.py:69-82)
    + the fp32 unfold; fp32 output bit-exact (same operations in the same order), bf16 = its rounding."""
    g = torch.Generator().manual_seed(S + C)
    data = torch.randint(0, 256, (37, C, S, S), generator=g, dtype=torch.uint8)
    idx = torch.randperm(37, generator=g)[:9]
    mean, std = O.DATASET_STATS[name]
    ref_img = O.normalize_u8(data[idx], mean, std)
    ref_patches = K.unfold(ref_img.cuda(), p, torch.float32).cpu()
    md, sd = torch.tensor(mean).cuda(), torch.tensor(std).cuda()
    img_out = torch.empty(9, C, S, S, device="cuda")
    got = K.unfold_u8(data.cuda(), idx.cuda(), md, sd, p, torch.float32, img_out=img_out)
    assert torch.equal(img_out.cpu(), ref_img)
    assert torch.equal(got.cpu(), ref_patches)
    got16 = K.unfold_u8(data.cuda(), idx.cuda(), md, sd, p, torch.bfloat16)
    assert torch.equal(got16.cpu(), ref_patches.to(torch.bfloat16))
    first = K.unfold_u8(data.cuda(), None, md, sd, p, torch.float32)        # NULL index: records in order
    assert torch.equal(first.cpu(), K.unfold(O.normalize_u8(data, mean, std).cuda(), p, torch.float32).cpu())
    from vitpe._lib import VitpeError
    with pytest.raises(VitpeError):
        K.unfold_u8(data.float().cuda(), idx.cuda(), md, sd, p, torch.float32)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("B,N,D,Cn,nvalid", [(37, 65, 192, 10, 37), (37, 65, 192, 10, 20), (5, 17, 96, 3, 5), (9, 65, 192, 64, 4),
                                             (6, 197, 768, 10, 6), (6, 65, 384, 10, 6)])
def test_head_step_equals_the_three_kernels(K, dt, B, N, D, Cn, nvalid):
    """vitpe_head_step (the train step's head, one launch pair) == vitpe_head_fwd + vitpe_cross_entropy_ctl + vitpe_head_bwd,
    with the ragged-batch scalars (rows >= n_valid masked) and across replays (the scratch re-arms).  The fused kernel
    writes only the class rows of dx: the other rows keep what the caller put there (zeros in the engine)."""
    x = dev(rnd(B, N, D, seed=1), DT[dt])
    g, b = dev(1 + 0.1 * rnd(D, seed=2)), dev(0.1 * rnd(D, seed=3))
    wh, bh = dev(rnd(Cn, D, seed=4, scale=0.2)), dev(0.1 * rnd(Cn, seed=5))
    labels = torch.randint(0, Cn, (B,), generator=torch.Generator().manual_seed(6)).cuda()
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    ctl = torch.tensor([1.0 / nvalid, 1.0 / nvalid, float(nvalid), 0.0], device="cuda")
    lg, ws = K.head_fwd(x, g, b, wh, bh, save=True)
    out2, dlog = K.cross_entropy_ctl(lg, labels, ctl, dlogits=z(B, Cn))
    gw, gb, gg, gbt = z(Cn, D), z(Cn), z(D), z(D)
    dx = K.head_bwd(dlog, wh, g, ws, DT[dt], N, gw, gb, gg, gbt)
    lg2, dlog2, dx2 = z(B, Cn), z(B, Cn), torch.full((B, N, D), 7.0, device="cuda").to(DT[dt])
    ws2, dyn2 = (z(B, D), z(B, D), z(B)), z(B, D)
    o2, macc, scratch = z(2), z(2), z(2 * B)
    gw2, gb2, gg2, gbt2 = z(Cn, D), z(Cn), z(D), z(D)
    hp = torch.zeros(16, device="cuda")
    hp[:5] = torch.tensor([1e-3, 0.9, 0.999, 1e-8, 0.05])
    for rep in range(2):
        K.head_step(x, g, b, wh, bh, labels, lg2, dlog2, ws2, dyn2, dx2, o2, macc, scratch, ctl, gw2, gb2, gg2, gbt2,
                    hp_tick=(hp if rep == 1 else None))
    # hp_tick: the launch advanced the optimizer's step counter and bias corrections exactly once (second call only)
    assert float(hp[5]) == 1.0 and abs(float(hp[6]) - 0.1) < 1e-6 and abs(float(hp[7]) - 1e-3) < 1e-7
    p_, g_, m_, v_ = z(64) + 1.0, z(64) + 0.5, z(64), z(64)
    K.adamw_step(p_, g_, m_, v_, hp, zero_grad=True, ticked=True)        # uses the corrections above, does not tick again
    assert float(hp[5]) == 1.0 and float(g_.abs().max()) == 0.0
    pr, gr, mr, vr, hpr = z(64) + 1.0, z(64) + 0.5, z(64), z(64), hp.clone()
    hpr[5:8] = 0.0
    K.adamw_step(pr, gr, mr, vr, hpr)                                     # the stand-alone form ticks itself
    assert float(hpr[5]) == 1.0 and torch.equal(p_.cpu(), pr.cpu()) and torch.equal(m_.cpu(), mr.cpu())
    assert rel_err(lg2.cpu(), lg.cpu()) < 1e-5 and rel_err(dlog2.cpu(), dlog.cpu()) < 1e-5
    assert float(dlog2[nvalid:].abs().max()) == 0.0 if nvalid < B else True
    assert rel_err(dx2[:, 0].float().cpu(), dx[:, 0].float().cpu()) < (1e-5 if dt == "f32" else 1e-2)
    assert float((dx2[:, 1:].float() - 7.0).abs().max()) == 0.0           # rows 1.. untouched
    assert abs(float(o2[0]) - float(out2[0])) < 1e-5 and float(o2[1]) == float(out2[1])
    assert abs(float(macc[0]) - 2 * float(out2[0])) < 2e-5 and float(macc[1]) == 2 * float(out2[1])
    for a2, a1 in ((gw2, gw), (gb2, gb), (gg2, gg), (gbt2, gbt)):
        assert rel_err(a2.cpu(), 2 * a1.cpu()) < 1e-5                    # accumulated twice


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("C,S,p,D,ape", [(3, 32, 4, 192, False), (3, 32, 4, 192, True), (1, 32, 4, 96, False), (1, 28, 4, 64, True),
                                         (1, 32, 8, 256, False)])
def test_fused_patch_embed_equals_unfold_gemm_layernorm(K, dt, C, S, p, D, ape):
    """vitpe_patch_embed == vitpe_unfold + vitpe_gemm_nt(EPI_PATCH) + vitpe_layernorm_fwd statistics, from fp32 images and
    from the resident uint8 dataset; the patch matrix it leaves behind is bit-identical to the unfold kernels'."""
    B, G = 5, S // p
    P, Kk = G * G, C * p * p
    assert K.patch_embed_supported(DT[dt], C, S, p, D)
    img = dev(rnd(B, C, S, S, seed=1))
    w = dev(rnd(D, Kk, seed=2, scale=0.3), DT[dt])
    bias, cls = dev(0.1 * rnd(D, seed=3)), dev(0.2 * rnd(D, seed=4))
    apet = dev(0.1 * rnd(P, D, seed=5)) if ape else None
    gam, bet = torch.ones(D, device="cuda"), torch.zeros(D, device="cuda")
    patches = K.unfold(img, p, DT[dt])
    ref = K.patch_embed_gemm(patches, w, bias, cls, apet, B, P)
    _, m_ref, r_ref = K.layernorm_fwd(ref, gam, bet, stats_only=True)
    mean, rstd = torch.empty(B * (P + 1), device="cuda"), torch.empty(B * (P + 1), device="cuda")
    pout = torch.empty_like(patches)
    out = K.patch_embed(w, bias, cls, apet, p, DT[dt], images=img, patches_out=pout, stats=(mean, rstd))
    assert torch.equal(pout, patches)
    assert rel_err(out.float().cpu(), ref.float().cpu()) < (1e-5 if dt == "f32" else 1e-2)
    assert rel_err(mean.cpu(), m_ref.cpu()) < (1e-5 if dt == "f32" else 2e-2) and rel_err(rstd.cpu(), r_ref.cpu()) < (1e-5 if dt == "f32" else 2e-2)
    # uint8 dataset path
    g = torch.Generator().manual_seed(7)
    data = torch.randint(0, 256, (11, C, S, S), generator=g, dtype=torch.uint8).cuda()
    idx = torch.tensor([3, 0, 10, 7, 7], dtype=torch.int64).cuda()
    mu, sd = dev(torch.tensor([0.4914, 0.4822, 0.4465][:C])), dev(torch.tensor([0.2023, 0.1994, 0.2010][:C]))
    p8 = K.unfold_u8(data, idx, mu, sd, p, DT[dt])
    ref8 = K.patch_embed_gemm(p8, w, bias, cls, apet, B, P)
    pout8 = torch.empty_like(p8)
    out8 = K.patch_embed(w, bias, cls, apet, p, DT[dt], data=data, index=idx, mean=mu, std=sd, patches_out=pout8)
    assert torch.equal(pout8, p8)
    assert rel_err(out8.float().cpu(), ref8.float().cpu()) < (1e-5 if dt == "f32" else 1e-2)
