"""Gradients w.r.t. caller-supplied rotary tables: the stand-alone apply_rotary_emb (vitpe_apply_rotary_bwd), the attention
core backward with table gradients (vitpe_attention_core_bwd_tables) through the C ABI, and the drop-in Attention with
differentiable (cos, sin), against the reference's own numbers (golden/rotary_grad.npz, tools/make_golden.py --only
rotary_grad) and the CPU oracle under autograd.  cos and sin are independent inputs (the tables used here do not satisfy
cos^2 + sin^2 = 1).

Tolerances are those of the existing suite: kernels and the fp32 drop-in module 1e-4, bf16 3e-2 (test_kernels_gpu.py);
the stand-alone rotation is elementwise fp32 plus fixed-order sums over at most 24 rows: 1e-5.  bf16 dq / dk come back in
bf16: one rounding of the fp32 result, at most 2^-8 of an element, so 4e-3 against the oracle's fp32 gradient.
"""
import pytest
import torch

from conftest import rel_err
from oracle import vit_oracle as O
from test_kernels_gpu import DT, attn_case, core_qkv, dev, q, rnd, tol

pytestmark = pytest.mark.gpu

CF = O.closed_form_tensor
RG_TOK, RG_POS = slice(0, None, 8), slice(0, None, 8)
RG_ROWS = {96: slice(1, None, 8), 192: slice(1, None, 16)}


@pytest.fixture(scope="module")
def K():
    from vitpe import kernels
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return kernels


def fixture_tables(kind, shape):
    """the (angle, cos, sin) recipe of tools/make_golden.py rotary_grad_tables, as cuda leaves"""
    if kind == "angle":
        ang = (CF("rg.angle", shape) * 40).cuda().requires_grad_(True)
        return ang, ang.cos(), ang.sin()
    cos = (0.8 + CF("rg.cos", shape) * 6).cuda().requires_grad_(True)
    sin = (CF("rg.sin", shape) * 12).cuda().requires_grad_(True)
    return None, cos, sin


# ---- 2. drop-in Attention vs the reference's own gradients -----------------------------------------------------------
@pytest.mark.parametrize("kind", ["angle", "free"])
@pytest.mark.parametrize("D,H", [(96, 3), (192, 8)])
def test_dropin_attention_table_grads_vs_reference(golden, D, H, kind):
    """fp32 drop-in Attention with differentiable (cos, sin): a learned-angle 2-D table on a RoPEAxial module, independent
    3-D cos / sin leaves on a RoPEMixed one.  The RoPEMixed module's own frequencies get no gradient: the tables are the
    caller's, not rebuilt from `freqs`."""
    from models.positional_encoding import RoPEAxial, RoPEMixed
    from models.vit import Attention
    g = golden("rotary_grad")
    hd, N, P = D // H, 65, 64
    att = Attention(D, num_heads=H)
    att.set_pos_encoding(RoPEAxial(hd, 100.0) if kind == "angle" else RoPEMixed(hd, H, 100.0))
    with torch.no_grad():
        att.qkv.weight.copy_(CF("attn.qkv.weight", (3 * D, D)))
        att.proj.weight.copy_(CF("attn.proj.weight", (D, D)))
        att.proj.bias.copy_(CF("attn.proj.bias", (D,)))
    att = att.cuda()
    x = (CF("rg.x", (2, N, D)) * 20).cuda().requires_grad_(True)
    dy = (CF("rg.dy", (2, N, D)) * 20).cuda()
    ang, cos, sin = fixture_tables(kind, (P, hd // 2) if kind == "angle" else (H, P, hd // 2))
    if ang is not None:
        cos.retain_grad(), sin.retain_grad()
    y = att(x, freqs_cis=(cos, sin))
    y.backward(dy)
    key = f"d{D}/{kind}"
    rows = RG_ROWS[D]
    assert rel_err(y.detach()[:, RG_TOK].cpu(), g[f"{key}/y"]) < 1e-4
    assert rel_err(x.grad[:, RG_TOK].cpu(), g[f"{key}/dx"]) < 1e-4
    assert rel_err(att.qkv.weight.grad[rows].cpu(), g[f"{key}/dwqkv"]) < 1e-4
    assert rel_err(att.proj.weight.grad[rows].cpu(), g[f"{key}/dwproj"]) < 1e-4
    assert rel_err(att.proj.bias.grad.cpu(), g[f"{key}/dbproj"]) < 1e-4
    assert cos.grad.shape == cos.shape and sin.grad.shape == sin.shape
    assert rel_err(cos.grad.cpu(), g[f"{key}/dcos"]) < 1e-4
    assert rel_err(sin.grad.cpu(), g[f"{key}/dsin"]) < 1e-4
    if ang is not None:
        assert rel_err(ang.grad.cpu(), g[f"{key}/dangle"]) < 1e-4
    else:
        assert att.pos_encoding.freqs.grad is None


def test_dropin_attention_own_mixed_tables_keep_the_frequency_path():
    """RoPEMixed.get_freqs_cis of the module's own `freqs`: still rebuilt in the kernel (the gradient reaches `freqs`),
    and the same result as the same tables taken as the caller's own through the new path (autograd then carries d cos /
    d sin into `freqs` through the table builder)."""
    from models.positional_encoding import RoPEMixed
    from models.vit import Attention
    D, H, N = 96, 3, 65
    outs, grads = [], []
    for detach_path in (False, True):
        att = Attention(D, num_heads=H)
        pe = RoPEMixed(D // H, H, 100.0)
        att.set_pos_encoding(pe)
        with torch.no_grad():
            att.qkv.weight.copy_(CF("attn.qkv.weight", (3 * D, D)))
            att.proj.weight.copy_(CF("attn.proj.weight", (D, D)))
            att.proj.bias.copy_(CF("attn.proj.bias", (D,)))
            pe.freqs.copy_(CF("pos_embed.freqs", tuple(pe.freqs.shape)))
        att = att.cuda()
        x = (CF("rg.x", (2, N, D)) * 20).cuda()
        cos, sin = pe.get_freqs_cis(N - 1, x.device)
        if detach_path:   # same values, not provably the module's own: the table-gradient route
            cos, sin = cos * 1.0, sin * 1.0
        y = att(x, freqs_cis=(cos, sin))
        y.backward(torch.ones_like(y))
        outs.append(y.detach().cpu())
        grads.append(pe.freqs.grad.detach().cpu())
    assert rel_err(outs[1], outs[0]) < 1e-4
    assert rel_err(grads[1], grads[0]) < 2e-4   # (frequency gradients: max(tol, 2e-4) as in test_kernels_gpu.py)


# ---- 3. apply_rotary_emb under autograd --------------------------------------------------------------------------------
COMBOS = [("q",), ("cos", "sin"), ("sin",), ("q", "k", "cos", "sin")]


def rotary_case(shape_tag, dt):
    q0 = CF("rotary.q", (2, 6, 64, 32)) * 20
    k0 = CF("rotary.k", (2, 6, 64, 32)) * 20
    shape = (1, 1, 64, 16) if shape_tag == "shared" else (1, 6, 64, 16)
    c0, s0 = 0.8 + CF("rg.cos", shape) * 6, CF("rg.sin", shape) * 12
    dq_up, dk_up = CF("rg.dq", (2, 6, 64, 32)) * 20, CF("rg.dk", (2, 6, 64, 32)) * 20
    if dt == "bf16":   # (the upstream gradient of a bf16 output is bf16: the oracle gets the same values)
        dq_up, dk_up = q(dq_up, dt), q(dk_up, dt)
    return q0.to(DT[dt]), k0.to(DT[dt]), c0, s0, dq_up, dk_up


@pytest.mark.parametrize("needs", COMBOS, ids=["-".join(c) for c in COMBOS])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("shape_tag", ["shared", "per_head"])
def test_apply_rotary_emb_gradients(golden, shape_tag, dt, needs):
    from models.rope_utils import apply_rotary_emb
    g = golden("rotary_grad")
    q0, k0, c0, s0, dq_up, dk_up = rotary_case(shape_tag, dt)
    ins = {"q": q0.cuda(), "k": k0.cuda(), "cos": c0.cuda(), "sin": s0.cuda()}
    for n in needs:
        ins[n].requires_grad_(True)
    qr, kr = apply_rotary_emb(ins["q"], ins["k"], ins["cos"], ins["sin"])
    assert qr.grad_fn is not None and qr.dtype == q0.dtype and kr.dtype == k0.dtype
    ((qr.float() * dq_up.cuda()).sum() + (kr.float() * dk_up.cuda()).sum()).backward()
    # oracle: the reference's arithmetic under autograd on the values the kernel sees (fp32 of the bf16 inputs)
    ref = {"q": q0.float(), "k": k0.float(), "cos": c0.clone(), "sin": s0.clone()}
    for n in ref:
        ref[n].requires_grad_(True)
    oq, ok = O.apply_rotary_emb(ref["q"], ref["k"], ref["cos"], ref["sin"])
    ((oq * dq_up).sum() + (ok * dk_up).sum()).backward()
    for n in ("q", "k", "cos", "sin"):
        if n not in needs:
            assert ins[n].grad is None, n
            continue
        got = ins[n].grad
        assert got.shape == ins[n].shape and got.dtype == ins[n].dtype, n
        t = 1e-5 if (dt == "f32" or n in ("cos", "sin")) else 4e-3
        assert rel_err(got.float().cpu(), ref[n].grad) < t, n
        if dt == "f32":   # and the reference's own numbers
            fx = g[f"rot/{shape_tag}/d{n}"]
            assert rel_err((got[:, :, RG_POS] if n in ("q", "k") else got).cpu(), fx) < 1e-5, n


def test_apply_rotary_emb_unreshaped_tables_and_forward_bits():
    """[P, D/2] / [H, P, D/2] tables (not reshaped for broadcast) get gradients in that shape; the forward values are
    the plain kernel's, bit for bit."""
    from models.rope_utils import apply_rotary_emb
    from vitpe import kernels as Kn
    q0 = (CF("rotary.q", (2, 6, 64, 32)) * 20).cuda()
    k0 = (CF("rotary.k", (2, 6, 64, 32)) * 20).cuda()
    for shape in ((64, 16), (6, 64, 16)):
        c = (0.8 + CF("rg.cos", shape) * 6).cuda().requires_grad_(True)
        s = (CF("rg.sin", shape) * 12).cuda().requires_grad_(True)
        qr, kr = apply_rotary_emb(q0, k0, c, s)
        assert torch.equal(qr.detach(), Kn.apply_rotary(q0, c.detach(), s.detach()))
        (qr.sum() + 2 * kr.sum()).backward()
        rc, rs = c.detach().cpu().requires_grad_(True), s.detach().cpu().requires_grad_(True)
        bshape = (1,) * (4 - len(shape)) + shape
        oq, ok = O.apply_rotary_emb(q0.cpu(), k0.cpu(), rc.view(bshape), rs.view(bshape))
        (oq.sum() + 2 * ok.sum()).backward()
        assert c.grad.shape == shape and s.grad.shape == shape
        assert rel_err(c.grad.cpu(), rc.grad) < 1e-5 and rel_err(s.grad.cpu(), rs.grad) < 1e-5


def test_apply_rotary_bwd_is_bit_reproducible(K):
    x = rnd(4, 6, 64, 32, seed=3).cuda()
    dy = rnd(4, 6, 64, 32, seed=4).cuda()
    c, s = rnd(64, 16, seed=5).cuda(), rnd(64, 16, seed=6).cuda()
    res = []
    for _ in range(2):
        dc, ds = torch.zeros_like(c), torch.zeros_like(s)
        dx = K.apply_rotary_bwd(dy, x, c, s, dc, ds)
        res.append((dx, dc, ds))
    for a, b in zip(*res):
        assert torch.equal(a, b)


# ---- 4. the core backward with table gradients through the C ABI -------------------------------------------------------
def oracle_tables(xn, wqkv, dout, cos, sin, H, dt):
    """O.attention_core + autograd with cos / sin leaves: out, dqkv, dcos, dsin"""
    B, N, D = xn.shape
    hd = D // H
    cl, sl = cos.clone().requires_grad_(True), sin.clone().requires_grad_(True)
    qkv = torch.nn.functional.linear(q(xn, dt), q(wqkv, dt)).requires_grad_(True)
    qkv_h = qkv.reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    o = O.attention_core(qkv_h[0], qkv_h[1], qkv_h[2], hd ** -0.5, (cl, sl))
    out = o.transpose(1, 2).reshape(B, N, D)
    out.backward(q(dout, dt))
    return out.detach(), qkv.grad, cl.grad, sl.grad


def run_core_tables(K, hd, H, G, dt, tdim, B=2, seed=200):
    from vitpe.kernels import PETables
    D = hd * H
    N, _, G, xn, wqkv, dout, _ = attn_case("none", D, H, B, seed=seed, G=G)
    wqkv = wqkv * (0.3 if D > 200 else 0.6 if hd > 64 else 1.0)   # (as test_head_dims_gpu.py)
    P = N - 1
    shape = (P, hd // 2) if tdim == 2 else (H, P, hd // 2)
    cos = 0.8 + rnd(*shape, seed=seed + 7, scale=0.3)
    sin = rnd(*shape, seed=seed + 8, scale=0.6)
    ref, dqkv_ref, dcos_ref, dsin_ref = oracle_tables(xn, wqkv, dout, cos, sin, H, dt)
    t = PETables("rope-axial" if tdim == 2 else "rope-mixed", G, cos=dev(cos), sin=dev(sin))
    qkv = dev(core_qkv(xn, wqkv, dt), DT[dt])
    do = dev(dout, DT[dt])
    assert rel_err(K.attention_core_fwd(qkv, H, t).float().cpu(), ref) < tol(dt)
    dfr = torch.zeros(2, H, hd // 2, device="cuda") if tdim == 3 else None
    plain = K.attention_core_bwd(qkv, do, H, t, None, None, dfr)
    res = []
    for _ in range(2):
        dc, ds = torch.zeros_like(t.cos), torch.zeros_like(t.sin)
        dqkv = K.attention_core_bwd(qkv, do, H, t, dcos=dc, dsin=ds)
        res.append((dqkv, dc, ds))
    dqkv, dc, ds = res[0]
    assert torch.equal(dqkv, plain), "dqkv differs from vitpe_attention_core_bwd"
    assert rel_err(dqkv.float().cpu(), dqkv_ref) < tol(dt)
    assert rel_err(dc.cpu(), dcos_ref) < tol(dt)
    assert rel_err(ds.cpu(), dsin_ref) < tol(dt)
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a, b), "two runs differ"


@pytest.mark.parametrize("tdim", [2, 3])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("hd,H", [(24, 8), (32, 6), (48, 4), (64, 3), (96, 2), (128, 3)])
def test_attention_core_table_grads_n65(K, hd, H, dt, tdim):
    run_core_tables(K, hd, H, 8, dt, tdim)


@pytest.mark.parametrize("tdim", [2, 3])
def test_attention_core_table_grads_n197_bf16(K, tdim):
    run_core_tables(K, 64, 3, 14, "bf16", tdim, B=2, seed=210)


@pytest.mark.parametrize("tdim", [2, 3])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_attention_core_table_grads_n257(K, dt, tdim):
    run_core_tables(K, 32, 4, 16, dt, tdim, B=1, seed=220)


# ---- 5. bf16 drop-in Attention at the fused geometries: routed through the core ----------------------------------------
@pytest.mark.parametrize("tdim", [2, 3])
@pytest.mark.parametrize("D,H,G", [(192, 6, 8), (768, 12, 14)])
def test_dropin_bf16_attention_fused_geometries_route_table_grads(D, H, G, tdim):
    """d = 192 / H = 6 (the wide fused kernel) and d = 768 / H = 12 / N = 197 (the fused hd-64 kernel) return no table
    gradients themselves: differentiable tables take the qkv Linear + core route.  Against the oracle at 3e-2.  Inputs are
    those of the kernel suite (attn_case, uniform random): with the closed-form sinusoid weights the output projection
    sums structured, cancelling terms, and its relative error is no longer the attention's."""
    from models.positional_encoding import RoPEAxial, RoPEMixed
    from models.vit import Attention
    hd, B = D // H, 2
    N, _, G, x0, wq, dy0, _ = attn_case("none", D, H, B, seed=240, G=G)
    wq = wq * (0.3 if D > 200 else 1.0)
    wp, bp = rnd(D, D, seed=245, scale=0.3), rnd(D, seed=246, scale=0.1)
    att = Attention(D, num_heads=H)
    att.set_pos_encoding(RoPEAxial(hd, 100.0) if tdim == 2 else RoPEMixed(hd, H, 100.0))
    with torch.no_grad():
        att.qkv.weight.copy_(wq), att.proj.weight.copy_(wp), att.proj.bias.copy_(bp)
    att = att.cuda()
    xb, dy = x0.to(torch.bfloat16), dy0.to(torch.bfloat16)
    shape = (N - 1, hd // 2) if tdim == 2 else (H, N - 1, hd // 2)
    c0, s0 = 0.8 + rnd(*shape, seed=31, scale=0.3), rnd(*shape, seed=32, scale=0.6)
    x = xb.cuda().requires_grad_(True)
    cos, sin = c0.cuda().requires_grad_(True), s0.cuda().requires_grad_(True)
    y = att(x, freqs_cis=(cos, sin))
    y.backward(dy.cuda())
    # oracle on the bf16-rounded operands, in fp32
    xo = xb.float().requires_grad_(True)
    wqo, wpo, bpo = q(wq, "bf16").requires_grad_(True), q(wp, "bf16").requires_grad_(True), bp.clone().requires_grad_(True)
    co, so = c0.clone().requires_grad_(True), s0.clone().requires_grad_(True)
    a = O.fused_attention(xo, wqo, H, freqs_cis=(co, so))
    yo = torch.nn.functional.linear(a, wpo, bpo)
    yo.backward(dy.float())
    assert rel_err(y.detach().float().cpu(), yo.detach()) < 3e-2
    assert rel_err(x.grad.float().cpu(), xo.grad) < 3e-2
    assert rel_err(att.qkv.weight.grad.cpu(), wqo.grad) < 3e-2
    assert rel_err(att.proj.weight.grad.cpu(), wpo.grad) < 3e-2
    assert rel_err(cos.grad.cpu(), co.grad) < 3e-2
    assert rel_err(sin.grad.cpu(), so.grad) < 3e-2
