"""Dropout, attention-probability dropout, stochastic depth and qkv bias on the device.

The keep masks are rebuilt in numpy from the documented stream (dropout_stream.py) and the (seed, offset) pairs; the
arithmetic they are applied to is restated here in torch on the CPU (autograd), on the oracle's own pieces.  Tolerances are
the suite's: kernels 1e-4 (fp32) / 3e-2 (bf16), frequency gradients max(tol, 2e-4) (test_kernels_gpu.py); modules 1e-4 on
outputs and 1e-3 on gradients in fp32 (test_model_gpu.py).
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dropout_stream as S  # noqa: E402

from conftest import rel_err  # noqa: E402
from oracle import vit_oracle as O  # noqa: E402
from test_head_dims_gpu import guarded  # noqa: E402
from test_kernels_gpu import DT, attn_case, core_qkv, dev, device_pe, q, rnd, tol  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = ["none", "relative", "polynomial", "rope-axial", "rope-mixed"]


@pytest.fixture(scope="module")
def K():
    from vitpe import kernels
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return kernels


def pair(seed, offset):
    """(device tensor, python tuple) of one (seed, offset) pair"""
    t = torch.tensor([seed, offset], dtype=torch.int64, device="cuda")
    return t, (seed, offset)


def as_pair(t):
    return tuple(int(v) for v in t.cpu())


# ---- masks ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("N", [17, 65, 197])
def test_masks_are_the_documented_stream(K, N, p):
    rng, pr = pair(0x0123456789ABCDEF, 0x0FEDCBA987654321 + N)
    n = 3 * N * 40 + 3                                   # (not a multiple of 4: the last call is partly used)
    assert np.array_equal(K.dropout_mask(rng, p, n=n).cpu().numpy().astype(bool), S.mask_elements(pr, n, p))
    assert np.array_equal(K.dropout_mask(rng, p, n=N).cpu().numpy().astype(bool), S.mask_elements(pr, N, p))   # per sample
    B, H = 2, 3
    got = K.dropout_mask(rng, p, attn_shape=(B, H, N)).cpu().numpy().astype(bool)
    assert np.array_equal(got, S.mask_attention(pr, B, H, N, p))


# ---- elementwise dropout and drop path ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("n", [4096, 4099, 7])
def test_dropout_fwd_bwd(K, dt, n):
    p = 0.25
    rng, pr = pair(77, 1234567)
    x, r, dy = rnd(n, seed=1), rnd(n, seed=2), rnd(n, seed=3)
    m = torch.from_numpy(S.mask_elements(pr, n, p)).float() * float(S.scale(p))
    ybuf, y = guarded((n,), DT[dt])
    K.dropout_fwd(dev(x, DT[dt]), rng, p, resid=dev(r, DT[dt]), out=y)
    dbuf, dx = guarded((n,), DT[dt])
    K.dropout_bwd(dev(dy, DT[dt]), rng, p, out=dx)
    torch.cuda.synchronize()
    assert torch.isnan(ybuf[n:]).all() and torch.isnan(dbuf[n:]).all()
    assert torch.isfinite(y).all() and torch.isfinite(dx).all()
    assert rel_err(y.float().cpu(), q(r, dt) + q(x, dt) * m) < tol(dt)
    assert rel_err(dx.float().cpu(), q(dy, dt) * m) < tol(dt)
    assert torch.equal(dx.float().cpu() == 0, (m == 0) | (q(dy, dt) == 0))
    y2 = K.dropout_fwd(dev(x, DT[dt]), rng, p)           # no residual; an unaligned view takes the scalar path
    assert rel_err(y2.float().cpu(), q(x, dt) * m) < tol(dt)
    if n > 8:
        xu = dev(torch.cat([torch.zeros(1), x]), DT[dt])[1:]
        yu = torch.empty(n + 1, device="cuda", dtype=DT[dt])[1:]
        K.dropout_fwd(xu, rng, p, out=yu)
        assert torch.equal(yu, y2)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_drop_path_fwd_bwd(K, dt):
    B, per, p = 7, 17 * 96, 0.4
    rng, pr = pair(5, 6)
    x, r, dy = rnd(B, 17, 96, seed=4), rnd(B, 17, 96, seed=5), rnd(B, 17, 96, seed=6)
    mb = S.mask_elements(pr, B, p)
    assert 0 < mb.sum() < B                                # (the fixed pair drops some samples and keeps some)
    m = (torch.from_numpy(mb).float() * float(S.scale(p)))[:, None, None]
    ybuf, y = guarded((B, 17, 96), DT[dt])
    K.drop_path_fwd(dev(x, DT[dt]), rng, p, resid=dev(r, DT[dt]), out=y)
    dx = K.drop_path_bwd(dev(dy, DT[dt]), rng, p)
    torch.cuda.synchronize()
    assert torch.isnan(ybuf[B * per:]).all() and torch.isfinite(y).all()
    assert rel_err(y.float().cpu(), q(r, dt) + q(x, dt) * m) < tol(dt)
    assert rel_err(dx.float().cpu(), q(dy, dt) * m) < tol(dt)


def test_drop_path_many_samples(K):
    """more samples than one grid dimension's 65535: every sample still gets its own decision"""
    B, per, p = 70001, 8, 0.5
    rng, pr = pair(21, 22)
    x = torch.ones(B, per, device="cuda")
    ybuf, y = guarded((B, per), torch.float32)
    K.drop_path_fwd(x, rng, p, out=y)
    torch.cuda.synchronize()
    m = torch.from_numpy(S.mask_elements(pr, B, p)).float() * float(S.scale(p))
    assert torch.isnan(ybuf[B * per:]).all()
    assert torch.equal(y.cpu(), m[:, None].expand(B, per))


def test_dropout_op_autograd_is_zero_where_the_mask_is(K):
    """forward and backward use the same mask: d sum(y) / dx is 1 / (1 - p) where y kept x and exactly 0 elsewhere"""
    from vitpe import ops  # noqa: F401  (registers torch.ops.vitpe.*)
    p = 0.3
    rng, pr = pair(11, 12)
    x = rnd(5, 65, 96, seed=7).cuda().requires_grad_(True)
    y = torch.ops.vitpe.dropout(x, None, p, rng)
    y.sum().backward()
    m = torch.from_numpy(S.mask_elements(pr, x.numel(), p)).view(x.shape)
    assert torch.equal(x.grad.cpu() != 0, m)
    assert torch.equal((y.detach().cpu() != 0) | (x.detach().cpu() == 0), m | (x.detach().cpu() == 0))
    assert torch.allclose(x.grad.cpu()[m], torch.tensor(float(S.scale(p))))


# ---- the attention core with dropout --------------------------------------------------------------------------------------
def masked_core(qh, kh, vh, scale, freqs_cis, bias, keep, rs):
    """oracle/vit_oracle.attention_core with the reference's attn_drop (vit.py:84-88) applied as a given mask"""
    if freqs_cis is not None:
        cos, sin = freqs_cis
        q_cls, q_p = qh[:, :, :1], qh[:, :, 1:]
        k_cls, k_p = kh[:, :, :1], kh[:, :, 1:]
        cos, sin = O.reshape_for_broadcast(cos, q_p), O.reshape_for_broadcast(sin, q_p)
        q_p, k_p = O.apply_rotary_emb(q_p, k_p, cos, sin)
        qh, kh = torch.cat([q_cls, q_p], dim=2), torch.cat([k_cls, k_p], dim=2)
    attn = (qh @ kh.transpose(-2, -1)) * scale
    if bias is not None:
        attn = attn + bias
    attn = attn.softmax(dim=-1)
    attn = attn * keep * rs
    return attn @ vh


def pe_terms(mode, pe, N, H):
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
    return leaves, freqs_cis, bias


def run_drop_core(K, mode, D, H, B, G, dt, p, seed):
    N, hd, G, xn, wqkv, dout, pe = attn_case(mode, D, H, B, seed=seed, G=G)
    wqkv = wqkv * (0.3 if D > 200 else 0.6 if hd > 64 else 1.0)      # (the spread of the existing core cases)
    rng, pr = pair(1000 + seed, 17 * seed + N)
    keep = torch.from_numpy(S.mask_attention(pr, B, H, N, p)).float()
    leaves, freqs_cis, bias = pe_terms(mode, pe, N, H)
    qkv_ref = core_qkv(xn, wqkv, dt).requires_grad_(True)
    qkv_h = qkv_ref.reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    ref = masked_core(qkv_h[0], qkv_h[1], qkv_h[2], hd ** -0.5, freqs_cis, bias, keep, float(S.scale(p)))
    ref = ref.transpose(1, 2).reshape(B, N, D)
    ref.backward(q(dout, dt))
    t = device_pe(K, mode, pe, H, G)
    qkv = dev(qkv_ref.detach(), DT[dt])
    obuf, out = guarded((B, N, D), DT[dt])
    K.attention_core_fwd_drop(qkv, H, t, rng, p, out=out)
    dtab = torch.zeros(H, 2 * N - 1, device="cuda") if mode == "relative" else None
    dcoef = torch.zeros_like(dev(pe["coeff"])) if mode.startswith("polynomial") else None
    dfr = torch.zeros(2, H, hd // 2, device="cuda") if mode == "rope-mixed" else None
    gbuf, dqkv = guarded((B, N, 3 * D), DT[dt])
    K.attention_core_bwd_drop(qkv, dev(dout, DT[dt]), H, t, rng, p, dtab, dcoef, dfr, out=dqkv)
    torch.cuda.synchronize()
    assert torch.isnan(obuf[B * N * D:]).all() and torch.isnan(gbuf[B * N * 3 * D:]).all()
    assert torch.isfinite(out).all() and torch.isfinite(dqkv).all()
    errs = dict(out=rel_err(out.float().cpu(), ref.detach()), dqkv=rel_err(dqkv.float().cpu(), qkv_ref.grad))
    if mode == "relative":
        errs["table"] = rel_err(dtab.cpu(), leaves["table"].grad)
    if mode.startswith("polynomial"):
        errs["coeff"] = rel_err(dcoef.cpu(), leaves["coeff"].grad)
    print(f"drop core {mode} D{D} H{H} N{N} {dt} p{p}:", {k: f"{v:.2e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v < tol(dt), (k, v)
    if mode == "rope-mixed":
        e = rel_err(dfr.cpu(), leaves["freqs"].grad)
        print(f"  freqs {e:.2e}")
        assert e < max(tol(dt), 2e-4)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("D,H", [(96, 3), (128, 2)])
def test_dropout_core_n65(K, dt, mode, D, H):
    run_drop_core(K, mode, D, H, 2, 8, dt, 0.1, seed=40)


@pytest.mark.parametrize("dt,mode,hd,H,D", [("f32", "rope-mixed", 24, 8, 192), ("bf16", "relative", 48, 4, 192),
                                            ("bf16", "rope-axial", 96, 2, 192), ("bf16", "polynomial", 128, 3, 384)])
def test_dropout_core_other_head_dims(K, dt, mode, hd, H, D):
    assert D == hd * H
    run_drop_core(K, mode, D, H, 2, 8, dt, 0.2, seed=50)


@pytest.mark.parametrize("mode", ["relative", "rope-mixed"])
@pytest.mark.parametrize("G", [4, 14, 16])
def test_dropout_core_token_counts_bf16(K, mode, G):
    """N = 17 / 197 / 257 (2, 13 and 17 token tiles) at hd 64"""
    run_drop_core(K, mode, 128, 2, 1 if G > 4 else 3, G, "bf16", 0.1, seed=60 + G)


@pytest.mark.parametrize("G", [14, 16])
def test_dropout_core_token_counts_hd32_f32(K, G):
    run_drop_core(K, "none", 96, 3, 1, G, "f32", 0.5, seed=70 + G)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("mode", MODES)
def test_p0_through_the_new_entry_is_the_existing_kernel(K, dt, mode):
    N, hd, G, xn, wqkv, dout, pe = attn_case(mode, 128, 2, 2, seed=45, G=8)
    t = device_pe(K, mode, pe, 2, G)
    qkv, do = dev(core_qkv(xn, wqkv, dt), DT[dt]), dev(dout, DT[dt])
    rng, _ = pair(1, 2)
    assert torch.equal(K.attention_core_fwd_drop(qkv, 2, t, rng, 0.0), K.attention_core_fwd(qkv, 2, t))

    def grads():
        return dict(dtable=torch.zeros(2, 2 * N - 1, device="cuda") if mode == "relative" else None,
                    dcoeff=torch.zeros_like(dev(pe["coeff"])) if mode == "polynomial" else None,
                    dfreqs=torch.zeros(2, 2, hd // 2, device="cuda") if mode == "rope-mixed" else None)
    assert torch.equal(K.attention_core_bwd_drop(qkv, do, 2, t, rng, 0.0, **grads()), K.attention_core_bwd(qkv, do, 2, t, **grads()))


def test_bad_arguments_launch_nothing(K):
    from vitpe import _lib as L
    from vitpe.kernels import PETables
    h = L.lib()
    rng, _ = pair(1, 2)
    x = torch.full((64,), float("nan"), device="cuda")
    y = torch.full((64,), float("nan"), device="cuda")
    st = L.stream_ptr()
    for p in (-0.1, 1.0, 1.5, float("nan")):
        assert h.vitpe_dropout_fwd(0, x.data_ptr(), None, y.data_ptr(), 64, rng.data_ptr(), p, st) == 1
        assert h.vitpe_dropout_bwd(0, x.data_ptr(), y.data_ptr(), 64, rng.data_ptr(), p, st) == 1
        assert h.vitpe_drop_path_fwd(0, x.data_ptr(), None, y.data_ptr(), 4, 16, rng.data_ptr(), p, st) == 1
        assert h.vitpe_dropout_mask(0, rng.data_ptr(), y.data_ptr(), 64, 0, 0, 0, p, st) == 1
    assert h.vitpe_dropout_fwd(0, x.data_ptr(), None, y.data_ptr(), 64, None, 0.1, st) == 1
    assert h.vitpe_drop_path_bwd(0, x.data_ptr(), y.data_ptr(), 4, 16, None, 0.1, st) == 1
    assert h.vitpe_dropout_mask(3, rng.data_ptr(), y.data_ptr(), 64, 1, 1, 8, 0.1, st) == 1     # unknown site
    qkv = torch.zeros(1, 17, 3 * 64, device="cuda")
    out = torch.full((1, 17, 64), float("nan"), device="cuda")
    args = (0, qkv.data_ptr(), out.data_ptr(), 1, 17, 2, 32, 0, None, None, None, None, 4, 0, 0)
    assert h.vitpe_attention_core_fwd_drop(*args, None, 0.1, st) == 1
    assert h.vitpe_attention_core_fwd_drop(*args, rng.data_ptr(), 1.0, st) == 1
    assert h.vitpe_attention_core_fwd_drop(*args, rng.data_ptr(), -0.5, st) == 1
    dout = torch.zeros(1, 17, 64, device="cuda")
    dqkv = torch.full((1, 17, 3 * 64), float("nan"), device="cuda")
    bargs = (0, qkv.data_ptr(), dout.data_ptr(), dqkv.data_ptr(), 1, 17, 2, 32, 0, None, None, None, None, 4, 0, 0,
             None, None, None)
    assert h.vitpe_attention_core_bwd_drop(*bargs, None, 0.1, st) == 1
    for p in (-0.5, 1.0, float("nan")):
        assert h.vitpe_attention_core_bwd_drop(*bargs, rng.data_ptr(), p, st) == 1
    assert h.vitpe_dropout_bwd(0, x.data_ptr(), y.data_ptr(), 64, None, 0.1, st) == 1
    assert h.vitpe_drop_path_fwd(0, x.data_ptr(), None, y.data_ptr(), 4, 16, None, 0.1, st) == 1
    torch.cuda.synchronize()
    assert torch.isnan(y).all() and torch.isnan(out).all() and torch.isnan(dqkv).all()
    with pytest.raises(L.VitpeError):
        K.attention_core_fwd_drop(qkv, 2, PETables("none", 4), rng, 1.0)


# ---- modules ----------------------------------------------------------------------------------------------------------------
def ref_attention(attn, x, mode, pe_mod, rng_pairs, attn_p, proj_p):
    """reference vit.py:47-92 in torch on the CPU with the masks of the given pairs; -> (y, leaves)"""
    B, N, D = x.shape
    H, hd = attn.num_heads, attn.head_dim
    P = {n: p.detach().cpu().clone().requires_grad_(True) for n, p in attn.named_parameters() if "pos_encoding" not in n}
    freqs_cis = bias = None
    if mode == "relative":
        P["table"] = pe_mod.relative_position_bias_table.detach().cpu().clone().requires_grad_(True)
        bias = O.relative_bias(P["table"], N)
    elif mode == "rope-axial":
        freqs_cis = O.rope_axial_tables(N - 1, O.rope_axial_inv_freq(hd, 100.0))
    qkv = F.linear(x, P["qkv.weight"], P.get("qkv.bias")).reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    keep = torch.ones(B, H, N, N)
    if attn_p > 0:
        keep = torch.from_numpy(S.mask_attention(rng_pairs[0], B, H, N, attn_p)).float()
    o = masked_core(qkv[0], qkv[1], qkv[2], hd ** -0.5, freqs_cis, bias, keep, float(S.scale(attn_p)))
    y = F.linear(o.transpose(1, 2).reshape(B, N, D), P["proj.weight"], P["proj.bias"])
    if proj_p > 0:
        y = y * torch.from_numpy(S.mask_elements(rng_pairs[1], y.numel(), proj_p)).view(y.shape).float() * float(S.scale(proj_p))
    return y, P


def make_attention(mode, N, qkv_bias=True, attn_drop=0.1, proj_drop=0.2, seed=3):
    from models.vit import Attention
    from vitpe.positional_encoding import RelativePositionalEncoding, RoPEAxial
    torch.manual_seed(seed)
    attn = Attention(96, num_heads=3, qkv_bias=qkv_bias, attn_drop=attn_drop, proj_drop=proj_drop)
    pe_mod = None
    with torch.no_grad():
        for p in attn.parameters():
            p.copy_(torch.randn_like(p) * (0.2 if p.dim() > 1 else 0.1))
    if mode == "relative":
        pe_mod = RelativePositionalEncoding(N - 1, 3)
        with torch.no_grad():
            pe_mod.relative_position_bias_table.copy_(torch.randn_like(pe_mod.relative_position_bias_table) * 0.3)
    elif mode == "rope-axial":
        pe_mod = RoPEAxial(dim=32, theta=100.0)
    if pe_mod is not None:
        attn.set_pos_encoding(pe_mod)
    return attn.cuda(), pe_mod


@pytest.mark.parametrize("mode", ["rope-axial", "relative"])
@pytest.mark.parametrize("N", [17, 65])
def test_attention_module_with_bias_and_dropout(K, mode, N):
    """Attention(d 96, H 3, qkv_bias, attn_drop, proj_drop) in fp32: output 1e-4, gradients 1e-3 against the restatement,
    with the masks rebuilt from the pairs the module saved (last_rng)"""
    B = 3
    attn, pe_mod = make_attention(mode, N)
    attn.train()
    x = rnd(B, N, 96, seed=9)
    dy = rnd(B, N, 96, seed=10)
    xd = x.cuda().requires_grad_(True)
    torch.manual_seed(123)
    y = attn(xd, freqs_cis=(N - 1,) if mode == "rope-axial" else None)
    y.backward(dy.cuda())
    pairs = [as_pair(r) for r in attn.last_rng]
    assert pairs[0] != pairs[1]
    xr = x.clone().requires_grad_(True)
    yr, P = ref_attention(attn, xr, mode, pe_mod, pairs, 0.1, 0.2)
    yr.backward(dy)
    assert rel_err(y.detach().cpu(), yr.detach()) < 1e-4
    assert rel_err(xd.grad.cpu(), xr.grad) < 1e-3
    for n, p in attn.named_parameters():
        if "pos_encoding" in n:
            continue
        assert rel_err(p.grad.cpu(), P[n].grad) < 1e-3, n
    if mode == "relative":
        assert rel_err(pe_mod.relative_position_bias_table.grad.cpu(), P["table"].grad) < 1e-3
    # reproducibility: the same torch seed gives the same pairs, outputs and gradients; another seed another mask
    g1 = {n: p.grad.clone() for n, p in attn.named_parameters()}
    attn.zero_grad()
    xd2 = x.cuda().requires_grad_(True)
    torch.manual_seed(123)
    y2 = attn(xd2, freqs_cis=(N - 1,) if mode == "rope-axial" else None)
    y2.backward(dy.cuda())
    assert torch.equal(y2, y) and torch.equal(xd2.grad, xd.grad)
    for n, p in attn.named_parameters():   # (weight and table gradients are accumulated with float atomics: not bitwise)
        assert rel_err(p.grad.cpu(), g1[n].cpu()) < 1e-5, n
    torch.manual_seed(124)
    attn(xd2, freqs_cis=(N - 1,) if mode == "rope-axial" else None)
    other = [as_pair(r) for r in attn.last_rng]
    assert other != pairs
    assert not np.array_equal(S.mask_attention(other[0], B, 3, N, 0.1), S.mask_attention(pairs[0], B, 3, N, 0.1))


def test_qkv_bias_alone_runs_without_dropout_kernels(K):
    attn, _ = make_attention("none", 65, qkv_bias=True, attn_drop=0., proj_drop=0.)
    attn.train()
    x, dy = rnd(2, 65, 96, seed=11), rnd(2, 65, 96, seed=12)
    xd = x.cuda().requires_grad_(True)
    y = attn(xd)
    y.backward(dy.cuda())
    assert attn.last_rng is None                          # nothing was drawn
    xr = x.clone().requires_grad_(True)
    yr, P = ref_attention(attn, xr, "none", None, None, 0., 0.)
    yr.backward(dy)
    assert rel_err(y.detach().cpu(), yr.detach()) < 1e-4
    assert rel_err(attn.qkv.bias.grad.cpu(), P["qkv.bias"].grad) < 1e-3
    assert rel_err(attn.qkv.weight.grad.cpu(), P["qkv.weight"].grad) < 1e-3
    assert rel_err(xd.grad.cpu(), xr.grad) < 1e-3


def test_table_gradients_with_attn_drop_are_refused(K):
    attn, _ = make_attention("rope-axial", 17, qkv_bias=False, attn_drop=0.1, proj_drop=0.)   # (only a rotary module reads tables)
    attn.train()
    cos = torch.rand(16, 16, device="cuda").requires_grad_(True)
    sin = torch.rand(16, 16, device="cuda").requires_grad_(True)
    x = rnd(2, 17, 96, seed=13).cuda()
    with pytest.raises(NotImplementedError, match="attn_drop"):
        attn(x, freqs_cis=(cos, sin))
    attn(x, freqs_cis=(cos.detach(), sin.detach()))      # constant tables: fine
    attn.eval()
    attn(x, freqs_cis=(cos, sin))                         # eval: no dropout, the table-gradient route as before


# ---- against the reference's own numbers (tests/golden/dropout.npz, tools/make_golden.py gen_dropout) ----------------------
def feed_pairs(monkeypatch, K, chunks):
    """the next len(chunks) calls of kernels.new_rng_pairs return the fixture's pairs instead of drawing new ones"""
    queue = [torch.tensor(c, dtype=torch.int64, device="cuda") for c in chunks]
    monkeypatch.setattr(K, "new_rng_pairs", lambda n, device: queue.pop(0))


def check_grads(g, key, named):
    for k in g.files:
        if k.startswith(f"{key}/grad/"):
            name = k[len(f"{key}/grad/"):]
            assert rel_err(named[name].grad.cpu().numpy(), g[k]) < 1e-3, name
        elif k.startswith(f"{key}/grad_rows"):
            step, name = k[len(f"{key}/grad_rows"):].split("/", 1)
            assert rel_err(named[name].grad.cpu().numpy()[::int(step)], g[k]) < 1e-3, name


@pytest.mark.parametrize("tag,N,B", [("rope-axial", 17, 3), ("relative", 17, 3), ("rope-axial", 65, 2), ("relative", 65, 2)])
def test_attention_vs_reference_golden(K, golden, monkeypatch, tag, N, B):
    """Attention(d 96, H 3, qkv_bias=True, attn_drop 0.1, proj_drop 0.2), fp32, against the reference's Attention run
    under the same masks: output 1e-4, gradients 1e-3 (the model-level gates of test_model_gpu.py)"""
    from models.vit import Attention
    from vitpe.positional_encoding import RelativePositionalEncoding, RoPEAxial
    g = golden("dropout")
    key = f"attn/{tag}/n{N}"
    CF = O.closed_form_tensor
    att = Attention(96, num_heads=3, qkv_bias=True, attn_drop=0.1, proj_drop=0.2)
    pem = RelativePositionalEncoding(N - 1, 3) if tag == "relative" else RoPEAxial(dim=32, theta=100.0)
    att.set_pos_encoding(pem)
    with torch.no_grad():
        for n, p in att.named_parameters():
            p.copy_(CF(("pos_embed." + n[len("pos_encoding."):]) if n.startswith("pos_encoding.") else "attn." + n, tuple(p.shape)))
    att = att.cuda().train()
    feed_pairs(monkeypatch, K, [g[f"{key}/pairs"].tolist()])
    x = (CF("attn.x", (B, N, 96)) * 20).cuda().requires_grad_(True)
    y = att(x, freqs_cis=(N - 1,) if tag == "rope-axial" else None)
    y.backward((CF("attn.dy", (B, N, 96)) * 20).cuda())
    assert [as_pair(r) for r in att.last_rng] == [tuple(r) for r in g[f"{key}/pairs"].tolist()]
    assert rel_err(y.detach().cpu(), g[f"{key}/y"]) < 1e-4
    assert rel_err(x.grad.cpu(), g[f"{key}/dx"]) < 1e-3
    check_grads(g, key, dict(att.named_parameters()))


def test_block_vs_reference_golden(K, golden, monkeypatch):
    """Block(d 96, H 3, qkv_bias, drop 0.1, attn_drop 0.15, drop_path 0.3) at N = 17, B = 4 against the reference's Block
    with its Dropout / DropPath modules replaced by the same masks (timm's Mlp drop order and DropPath are third-party:
    restated, parity unpinned)"""
    from models.vit import Block
    g = golden("dropout")
    CF = O.closed_form_tensor
    blk = Block(96, 3, qkv_bias=True, drop=0.1, attn_drop=0.15, drop_path=0.3)
    with torch.no_grad():
        for n, p in blk.named_parameters():
            p.copy_(CF("blk." + n, tuple(p.shape)))
    blk = blk.cuda().train()
    pairs = g["block/pairs"].tolist()   # attention, proj, drop1, drop2, path (attention), path (MLP)
    feed_pairs(monkeypatch, K, [pairs[4:6], pairs[0:2], pairs[2:4]])   # drawn in this order: Block, Attention, Mlp
    x = (CF("blk.x", (4, 17, 96)) * 20).cuda().requires_grad_(True)
    y = blk(x)
    y.backward((CF("blk.dy", (4, 17, 96)) * 20).cuda())
    assert rel_err(y.detach().cpu(), g["block/y"]) < 1e-4
    assert rel_err(x.grad.cpu(), g["block/dx"]) < 1e-3
    check_grads(g, "block", dict(blk.named_parameters()))


def ref_block(blk, x, pairs, rates):
    """reference vit.py:120-125 with timm's Mlp drop1 / drop2 and DropPath(scale_by_keep=True) restated (third-party:
    parity unpinned) on the masks of the given pairs"""
    drop, attn_p, dpath = rates
    B, N, D = x.shape
    P = {n: p.detach().cpu().clone().requires_grad_(True) for n, p in blk.named_parameters()}
    sub = {n[len("attn."):]: p for n, p in P.items() if n.startswith("attn.")}
    H, hd = blk.attn.num_heads, blk.attn.head_dim
    n1 = F.layer_norm(x, (D,), P["norm1.weight"], P["norm1.bias"], 1e-5)
    qkv = F.linear(n1, sub["qkv.weight"], sub["qkv.bias"]).reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    keep = torch.from_numpy(S.mask_attention(pairs["attn"][0], B, H, N, attn_p)).float()
    o = masked_core(qkv[0], qkv[1], qkv[2], hd ** -0.5, None, None, keep, float(S.scale(attn_p)))
    a = F.linear(o.transpose(1, 2).reshape(B, N, D), sub["proj.weight"], sub["proj.bias"])
    el = lambda t, pr, p: t * torch.from_numpy(S.mask_elements(pr, t.numel(), p)).view(t.shape).float() * float(S.scale(p))  # noqa: E731
    sm = lambda pr: (torch.from_numpy(S.mask_elements(pr, B, dpath)).float() * float(S.scale(dpath)))[:, None, None]  # noqa: E731
    x = x + sm(pairs["block"][0]) * el(a, pairs["attn"][1], drop)
    n2 = F.layer_norm(x, (D,), P["norm2.weight"], P["norm2.bias"], 1e-5)
    h = el(F.gelu(F.linear(n2, P["mlp.fc1.weight"], P["mlp.fc1.bias"])), pairs["mlp"][0], drop)
    m = el(F.linear(h, P["mlp.fc2.weight"], P["mlp.fc2.bias"]), pairs["mlp"][1], drop)
    return x + sm(pairs["block"][1]) * m, P


def test_block_with_all_four_rates(K):
    from models.vit import Block
    rates = (0.1, 0.15, 0.3)
    torch.manual_seed(5)
    blk = Block(96, 3, qkv_bias=True, drop=rates[0], attn_drop=rates[1], drop_path=rates[2])
    with torch.no_grad():
        for n, p in blk.named_parameters():
            p.copy_(torch.randn_like(p) * (0.15 if p.dim() > 1 else 0.1) + (1.0 if n.endswith("norm1.weight") or n.endswith("norm2.weight") else 0.0))
    blk = blk.cuda().train()
    B, N = 4, 17
    x, dy = rnd(B, N, 96, seed=14), rnd(B, N, 96, seed=15)
    xd = x.cuda().requires_grad_(True)
    torch.manual_seed(2)
    y = blk(xd)
    y.backward(dy.cuda())
    pairs = dict(attn=[as_pair(r) for r in blk.attn.last_rng], mlp=[as_pair(r) for r in blk.mlp.last_rng],
                 block=[as_pair(r) for r in blk.last_rng])
    allp = pairs["attn"] + pairs["mlp"] + pairs["block"]
    assert len(set(allp)) == 6                            # every site of the layer drew its own pair
    xr = x.clone().requires_grad_(True)
    yr, P = ref_block(blk, xr, pairs, rates)
    yr.backward(dy)
    assert rel_err(y.detach().cpu(), yr.detach()) < 1e-4
    assert rel_err(xd.grad.cpu(), xr.grad) < 1e-3
    for n, p in blk.named_parameters():
        assert rel_err(p.grad.cpu(), P[n].grad) < 1e-3, n


def test_eval_and_zero_rates_equal_a_plain_module(K):
    from models.vit import Attention, Block, VisionTransformer
    x = rnd(2, 65, 96, seed=16).cuda()
    torch.manual_seed(0)
    plain = Block(96, 3).cuda()
    for kw in (dict(drop=0.2, attn_drop=0.1, drop_path=0.3), dict(drop=0., attn_drop=0., drop_path=0.)):
        blk = Block(96, 3, **kw).cuda()
        blk.load_state_dict(plain.state_dict())
        blk.eval() if kw["drop"] else blk.train()
        assert torch.equal(blk(x), plain(x))
        assert blk.last_rng is None and blk.attn.last_rng is None and blk.mlp.last_rng is None
    a0, a1 = Attention(96, 3).cuda(), Attention(96, 3, attn_drop=0.5, proj_drop=0.5).cuda()
    a1.load_state_dict(a0.state_dict())
    a1.train()(x)
    assert a1.last_rng is not None
    assert torch.equal(a1.eval()(x), a0(x))
    assert a1.last_rng is None                            # a forward that draws nothing leaves no stale pairs behind
    torch.manual_seed(1)
    v0 = VisionTransformer(img_size=32, patch_size=8, embed_dim=96, depth=2, num_heads=3, pos_encoding="rope-mixed").cuda()
    v1 = VisionTransformer(img_size=32, patch_size=8, embed_dim=96, depth=2, num_heads=3, pos_encoding="rope-mixed",
                           drop_rate=0.1, attn_drop_rate=0.1, drop_path_rate=0.2).cuda()
    v1.load_state_dict(v0.state_dict())
    img = rnd(3, 3, 32, 32, seed=17).cuda()
    assert torch.equal(v1.eval()(img), v0.eval()(img))


def test_model_trains_with_every_option_and_layers_differ(K):
    """VisionTransformer with all extras: a training forward / backward is finite, reproducible under torch.manual_seed, and
    two layers of one forward use different pairs"""
    from models.vit import VisionTransformer
    torch.manual_seed(3)
    v = VisionTransformer(img_size=32, patch_size=8, embed_dim=96, depth=3, num_heads=3, pos_encoding="rope-mixed",
                          qkv_bias=True, drop_rate=0.1, attn_drop_rate=0.1, drop_path_rate=0.2).cuda().train()
    img = rnd(4, 3, 32, 32, seed=18).cuda()
    lab = torch.tensor([1, 2, 3, 4], device="cuda")
    outs = []
    for _ in range(2):
        v.zero_grad()
        torch.manual_seed(77)
        logits = v(img)
        torch.nn.functional.cross_entropy(logits, lab).backward()
        outs.append((logits.detach().clone(), {n: p.grad.clone() for n, p in v.named_parameters()}))
    assert torch.isfinite(outs[0][0]).all() and all(torch.isfinite(g).all() for g in outs[0][1].values())
    assert torch.equal(outs[0][0], outs[1][0])
    for n in outs[0][1]:                    # (parameter gradients are accumulated with float atomics: not bitwise)
        assert rel_err(outs[0][1][n].cpu(), outs[1][1][n].cpu()) < 1e-5, n
    assert v.blocks[0].last_rng is None                   # first block: drop-path rate 0
    seen = [as_pair(r) for b in v.blocks for r in b.attn.last_rng] + [as_pair(r) for b in v.blocks for r in b.mlp.last_rng]
    assert len(set(seen)) == len(seen)
    assert torch.count_nonzero(v.blocks[0].attn.qkv.bias.grad) > 0
