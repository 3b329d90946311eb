"""Attention kernels at every token count the support queries accept (17-32, 49-64, 65-80, 145-160, 193-208, 257-272), not
only at N = G^2 + 1: per tile count the first, a middle, the last-but-one and the full count (attn_tokens.TOKEN_COUNTS), on
the suite's random inputs and on attn_tokens.masked_case, whose sensitivity to a wrong last-tile decision is proved on the
CPU (test_token_counts_cpu.py).

Gates are the project's: tol(dt) = 1e-4 fp32 / 3e-2 bf16 under rel_err against the CPU oracle, max(tol, 2e-4) for
frequency gradients, 8e-3 / 1.5e-2 for the fused64 kernel against Linear + core, 1e-5 / 2e-2 for a LayerNorm-fused call
against the plain call; per-row checks on the rows next to a tile edge at 2 x tol(dt) (as test_wgrad_group_wide_blocks).
Every input whose rows past N could be read is followed by a NaN guard, every output starts as NaN and is followed by one;
out, dqkv and qkv_out (no atomics) must be bit-identical over three launches.

VITPE_TOKEN_REPORT=<file>: the worst figure per kernel family, dtype and input kind is written there as JSON at exit.
"""
import atexit
import json
import os

import pytest
import torch

from attn_tokens import (ALL_COUNTS, ANY_N_MODES, FUSED64_GEOMS, FUSED_GEOMS, MIDDLE_AND_FULL, WIDE_MODES, Guarded,
                         guarded_input, masked_case, masked_layernorm, token_case, worst_row_err)
from conftest import rel_err
from oracle import vit_oracle as O
from test_kernels_gpu import ATTN_MODES, DT, core_qkv, dev, device_pe, oracle_attn, rnd, tol

pytestmark = pytest.mark.gpu

BUILDERS = {"random": token_case, "masked": masked_case}
WORST = {}


def note(family, dt, kind, what, value):
    key = f"{family}/{dt}/{kind}/{what}"
    WORST[key] = max(WORST.get(key, 0.0), float(value))
    return value


@atexit.register
def _report():
    path = os.environ.get("VITPE_TOKEN_REPORT")
    if path and WORST:
        with open(path, "w") as f:
            json.dump(WORST, f, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def K():
    from vitpe import kernels
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return kernels


def pe_grads(mode, pe, H, N, hd):
    dtab = torch.zeros(H, 2 * N - 1, device="cuda") if mode == "relative" else None
    dcoef = torch.zeros_like(dev(pe["coeff"])) if mode.startswith("polynomial") else None
    dfr = torch.zeros(2, H, hd // 2, device="cuda") if mode == "rope-mixed" else None
    return dtab, dcoef, dfr


def check_pe_grads(fam, dt, kind, mode, got, g_ref):
    dtab, dcoef, dfr = got
    if mode == "relative":
        assert note(fam, dt, kind, "dtable", rel_err(dtab.cpu(), g_ref["table"])) < tol(dt)
    if mode.startswith("polynomial"):
        assert note(fam, dt, kind, "dcoeff", rel_err(dcoef.cpu(), g_ref["coeff"])) < tol(dt)
    if mode == "rope-mixed":
        assert note(fam, dt, kind, "dfreqs", rel_err(dfr.cpu(), g_ref["freqs"])) < max(tol(dt), 2e-4)


def check_against(fam, dt, kind, what, got, ref, N):
    got = got.float().cpu()
    assert note(fam, dt, kind, what, rel_err(got, ref)) < tol(dt), (what, N)
    assert note(fam, dt, kind, what + " edge rows", worst_row_err(got, ref, N)) < 2 * tol(dt), (what, N)


# ------------------------------------------------------------------------------------------ attention core
def run_core(K, kind, mode, N, hd, dt, H=2, B=2):
    """B = 2: the padding rows of image 0 are the first rows of image 1; those of image 1 are the NaN guard."""
    D = hd * H
    _, _, G, xn, wqkv, dout, pe = BUILDERS[kind](mode, N, D, H, B, seed=N + hd)
    if kind == "random":
        wqkv = wqkv * (0.3 if D > 200 else 0.6 if hd > 64 else 1.0)      # the logit spread of the existing core cases
    ref, dqkv_ref, g_ref = oracle_attn(mode, xn, wqkv, dout, pe, H, dt)
    t = device_pe(K, mode, pe, H, G)
    qkv = guarded_input(dev(core_qkv(xn, wqkv, dt), DT[dt]))
    do = guarded_input(dev(dout, DT[dt]))
    outs, dqkvs = [], []
    for _ in range(3):
        o, g = Guarded((B, N, D), DT[dt]), Guarded((B, N, 3 * D), DT[dt])
        K.attention_core_fwd(qkv, H, t, out=o.t)
        grads = pe_grads(mode, pe, H, N, hd)
        K.attention_core_bwd(qkv, do, H, t, *grads, out=g.t)
        torch.cuda.synchronize()
        outs.append(o.check("out"))
        dqkvs.append(g.check("dqkv"))
    check_against("core", dt, kind, "out", outs[0], ref, N)
    check_against("core", dt, kind, "dqkv", dqkvs[0], dqkv_ref, N)
    check_pe_grads("core", dt, kind, mode, grads, g_ref)
    for i in (1, 2):
        assert torch.equal(outs[i], outs[0]) and torch.equal(dqkvs[i], dqkvs[0]), "launches differ"


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("mode", ANY_N_MODES)
@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("N", ALL_COUNTS)
def test_attention_core_every_new_token_count(K, N, hd, mode, dt):
    assert K.attention_core_supported(DT[dt], N, hd)
    for kind in BUILDERS:
        run_core(K, kind, mode, N, hd, dt)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("mode", ANY_N_MODES)
@pytest.mark.parametrize("hd", [24, 48, 96, 128])
@pytest.mark.parametrize("N", [n for mt in sorted(MIDDLE_AND_FULL) for n in MIDDLE_AND_FULL[mt]])
def test_attention_core_other_head_dims_middle_and_full(K, N, hd, mode, dt):
    """hd 24 / 48: padded feature columns and padded rows in the same tile.  The support query decides which (dtype, hd,
    tile count) exist (the two backward LDS tiles do not fit everywhere); what it refuses is refused by the call."""
    from vitpe._lib import VitpeError
    if not K.attention_core_supported(DT[dt], N, hd):
        with pytest.raises(VitpeError):
            K.attention_core_fwd(torch.zeros(1, N, 3 * hd, device="cuda", dtype=DT[dt]), 1, K.PETables("none", 0))
        return
    for kind in BUILDERS:
        run_core(K, kind, mode, N, hd, dt)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("mode", ATTN_MODES)
@pytest.mark.parametrize("hd", [32, 64])
def test_attention_core_26_tokens_all_modes(K, hd, mode, dt):
    """N = 26 (5 x 5 grid, --img_size 20 --patch_size 4): the one new count the grid modes can have; ten live rows in the
    last of two tiles"""
    for kind in BUILDERS:
        run_core(K, kind, mode, 26, hd, dt)


@pytest.mark.parametrize("tdim", [2, 3])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("hd,H", [(32, 6), (64, 3)])
def test_attention_core_table_grads_26_tokens(K, hd, H, dt, tdim):
    from test_rotary_grad_gpu import run_core_tables
    run_core_tables(K, hd, H, 5, dt, tdim, seed=230)


# ------------------------------------------------------------------------------------------ fused 16x16-tile kernels
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("mode,N,D", FUSED_GEOMS)
def test_fused_attention_66_to_80_tokens(K, mode, N, D, B, dt):
    """vitpe_fused_attention_fwd / _bwd and their LayerNorm-fused variants; B odd: idle second image slot"""
    H = D // 32
    assert K.fused_attention_supported(DT[dt], N, D, 32)
    lntol = 1e-5 if dt == "f32" else 2e-2
    for kind in BUILDERS:
        _, hd, G, xn, wqkv, dout, pe = BUILDERS[kind](mode, N, D, H, B, seed=N + B)
        ref, dqkv_ref, g_ref = oracle_attn(mode, xn, wqkv, dout, pe, H, dt)
        t = device_pe(K, mode, pe, H, G)
        w = K.pack_qkv_weights(dev(wqkv), DT[dt], H)
        x, do = guarded_input(dev(xn, DT[dt])), guarded_input(dev(dout, DT[dt]))
        outs, dqkvs = [], []
        for _ in range(3):
            o, g = Guarded((B, N, D), DT[dt]), Guarded((B, N, 3 * D), DT[dt])
            K.fused_attention_fwd(x, w, H, t, out=o.t)
            grads = pe_grads(mode, pe, H, N, hd)
            K.fused_attention_bwd(x, w, do, H, t, *grads, out=g.t)
            torch.cuda.synchronize()
            outs.append(o.check("out"))
            dqkvs.append(g.check("dqkv"))
        check_against("fused", dt, kind, "out", outs[0], ref, N)
        check_against("fused", dt, kind, "dqkv", dqkvs[0], dqkv_ref, N)
        check_pe_grads("fused", dt, kind, mode, grads, g_ref)
        for i in (1, 2):
            assert torch.equal(outs[i], outs[0]) and torch.equal(dqkvs[i], dqkvs[0]), "launches differ"
        # LayerNorm in the staging: raw tokens + statistics against the plain call on layernorm_fwd's output
        gam, bet = masked_layernorm(D, seed=N) if kind == "masked" else (1 + 0.1 * rnd(D, seed=5), 0.1 * rnd(D, seed=6))
        gam, bet = dev(gam), dev(bet)
        xr = guarded_input(dev(rnd(B, N, D, seed=N + 9) * 1.7 + 0.4, DT[dt]))
        xln, mean, rstd = K.layernorm_fwd(xr, gam, bet)
        if kind == "masked":
            assert (xln[..., 0] == 1).all() and (xln[..., 1:3] == 0).all()
        ref_ln, _, _ = oracle_attn(mode, xln.float().cpu(), wqkv, dout, pe, H, dt)
        o, xo, g = Guarded((B, N, D), DT[dt]), Guarded((B, N, D), DT[dt]), Guarded((B, N, 3 * D), DT[dt])
        plain = K.fused_attention_fwd(xln, w, H, t)
        K.fused_attention_fwd(xr, w, H, t, out=o.t, ln=(gam, bet, mean, rstd), xn_out=xo.t)
        d0, d1 = pe_grads(mode, pe, H, N, hd), pe_grads(mode, pe, H, N, hd)
        plain_b = K.fused_attention_bwd(xln, w, do, H, t, *d0)
        K.fused_attention_bwd(xr, w, do, H, t, *d1, out=g.t, ln=(gam, bet, mean, rstd))
        torch.cuda.synchronize()
        out_ln, xn_out, dqkv_ln = o.check("out (ln)"), xo.check("xn_out"), g.check("dqkv (ln)")
        assert note("fused_ln", dt, kind, "xn_out vs layernorm_fwd", rel_err(xn_out.float().cpu(), xln.float().cpu())) < lntol
        assert note("fused_ln", dt, kind, "out vs plain", rel_err(out_ln.float().cpu(), plain.float().cpu())) < lntol
        assert note("fused_ln", dt, kind, "dqkv vs plain", rel_err(dqkv_ln.float().cpu(), plain_b.float().cpu())) < lntol
        assert note("fused_ln", dt, kind, "out", rel_err(out_ln.float().cpu(), ref_ln)) < tol(dt)
        if mode == "relative":
            assert note("fused_ln", dt, kind, "dtable vs plain", rel_err(d1[0].cpu(), d0[0].cpu())) < lntol


# ------------------------------------------------------------------------------------------ fused64 forward
@pytest.mark.parametrize("kind", list(BUILDERS))
@pytest.mark.parametrize("mode,N", FUSED64_GEOMS)
def test_attention_fused64_193_to_208_tokens(K, mode, N, kind):
    """The one-kernel forward at hd 64: rows past N of the last token tile read and WRITE their clamped row (N - 1) of x /
    qkv_out, so qkv_out is NaN-prefilled, guarded and compared bit for bit over three launches."""
    D, H, B, bf = 128, 2, 3, torch.bfloat16
    assert K.attention_fused64_supported(bf, N, H, 64)
    _, hd, G, xn, wqkv, dout, pe = BUILDERS[kind](mode, N, D, H, B, seed=N)
    ref, _, _ = oracle_attn(mode, xn, wqkv, dout, pe, H, "bf16")
    t = device_pe(K, mode, pe, H, G)
    xb = guarded_input(dev(xn, bf))
    wp = K.pack_weight_frags(dev(wqkv), bf, 64, 0)
    outs, qkvs = [], []
    for _ in range(3):
        o, s = Guarded((B, N, D), bf), Guarded((B, N, 3 * D), bf)
        K.attention_fused64_fwd(xb, wp, H, t, qkv_out=s.t, out=o.t)
        torch.cuda.synchronize()
        outs.append(o.check("out"))
        qkvs.append(s.check("qkv_out"))
    for i in (1, 2):
        assert torch.equal(outs[i], outs[0]) and torch.equal(qkvs[i], qkvs[0]), "launches differ"
    check_against("fused64", "bf16", kind, "out", outs[0], ref, N)
    qkv2 = K.linear(xb.reshape(B * N, D), dev(wqkv, bf)).reshape(B, N, 3 * D)
    assert note("fused64", "bf16", kind, "qkv_out vs linear", rel_err(qkvs[0].float().cpu(), qkv2.float().cpu())) < 8e-3
    assert note("fused64", "bf16", kind, "qkv_out vs linear edge rows",
                worst_row_err(qkvs[0].float().cpu(), qkv2.float().cpu(), N)) < 2 * 8e-3
    out2 = K.attention_core_fwd(qkv2, H, t)
    assert note("fused64", "bf16", kind, "out vs linear + core", rel_err(outs[0].float().cpu(), out2.float().cpu())) < 1.5e-2
    o = Guarded((B, N, D), bf)
    K.attention_fused64_fwd(xb, wp, H, t, out=o.t)              # inference: no side output
    assert torch.equal(o.check("out, no side output"), outs[0])


# ------------------------------------------------------------------------------------------ wide kernel (N = 65)
def run_wide(K, mode, B, ln):
    """three launches of the 32x32-tile forward on masked_case -> (outputs, oracle)"""
    D, H, N, bf = 192, 6, 65, torch.bfloat16
    _, hd, G, xn, wqkv, dout, pe = masked_case(mode, N, D, H, B, seed=31)
    assert K.fused_attention_wide_supported(bf, N, D, hd)
    t = device_pe(K, mode, pe, H, G)
    w = K.pack_qkv_weights_wide(dev(wqkv), bf, H)
    outs = []
    for _ in range(3):
        o = Guarded((B, N, D), bf)
        if ln:
            gam, bet = masked_layernorm(D, seed=31)
            gam, bet = dev(gam), dev(bet)
            xr = guarded_input(dev(rnd(B, N, D, seed=40) * 1.7 + 0.4, bf))
            xln, mean, rstd = K.layernorm_fwd(xr, gam, bet)
            xo = Guarded((B, N, D), bf)
            K.fused_attention_fwd_wide(xr, w, H, t, out=o.t, ln=(gam, bet, mean, rstd), xn_out=xo.t)
            torch.cuda.synchronize()
            xn_out = xo.check("xn_out")
            assert (xn_out[..., 0] == 1).all() and (xn_out[..., 1:3] == 0).all()
            assert rel_err(xn_out.float().cpu(), xln.float().cpu()) < 1e-2      # one bf16 ulp, as test_fused_attention_fwd_wide
            ref, _, _ = oracle_attn(mode, xn_out.float().cpu(), wqkv, dout, pe, H, "bf16")
        else:
            K.fused_attention_fwd_wide(guarded_input(dev(xn, bf)), w, H, t, out=o.t)
            torch.cuda.synchronize()
            ref, _, _ = oracle_attn(mode, xn, wqkv, dout, pe, H, "bf16")
        outs.append(o.check("out"))
    return outs, ref


@pytest.mark.parametrize("ln", [False, True])
@pytest.mark.parametrize("B", [3, 4])
@pytest.mark.parametrize("mode", WIDE_MODES)
def test_fused_attention_wide_on_masked_inputs(K, mode, B, ln):
    """The 32x32-tile forward the benchmark runs (bf16, N = 65: one live row in the third 32-row tile) on the mask-sensitive
    input; B = 3: idle second image slot."""
    outs, ref = run_wide(K, mode, B, ln)
    for o in outs:
        check_against("wide_ln" if ln else "wide", "bf16", "masked", "out", o, ref, 65)


@pytest.mark.parametrize("ln", [False, True])
@pytest.mark.parametrize("B", [3, 4])
@pytest.mark.parametrize("mode", WIDE_MODES)
def test_fused_attention_wide_launches_are_bit_identical(K, mode, B, ln):
    """The kernel has no atomics on its output: three launches on the same operands must agree bit for bit.  (They did
    not in the modes none, rope-axial and rope-mixed while the row maximum was taken by an inline-asm v_max3_f32 on MFMA
    results, in front of which the compiler inserts no MFMA -> VALU wait states: csrc/attn32.hip, max3.)"""
    outs, _ = run_wide(K, mode, B, ln)
    for i in (1, 2):
        assert torch.equal(outs[i], outs[0]), "launches differ"


# ------------------------------------------------------------------------------------------ drop-in Attention
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("resid", [False, True])
@pytest.mark.parametrize("rel", [False, True])
@pytest.mark.parametrize("N,D,H", [(26, 64, 2), (72, 192, 6), (80, 96, 3), (198, 128, 2), (208, 128, 2), (152, 64, 2)])
def test_dropin_attention_at_token_counts_off_the_grid(N, D, H, rel, resid, dt):
    """models.vit.Attention under autograd with no positional encoding and with RelativePositionalEncoding(N - 1, H): y, dx
    and every parameter gradient against a float64 torch restatement on the operands the kernels see; tolerances of
    test_model_gpu.py (fp32: 1e-4 outputs, 1e-3 gradients; bf16: 3e-2).  Also runs vitpe_linear / vitpe_gemm_tn at
    M = B N that is a multiple of nothing."""
    from models import positional_encoding as pe
    from models.vit import Attention
    B, hd, dtype = 3, D // H, DT[dt]
    otol, gtol = (1e-4, 1e-3) if dt == "f32" else (3e-2, 3e-2)
    att = Attention(D, num_heads=H)
    pos = pe.RelativePositionalEncoding(N - 1, num_heads=H) if rel else None
    if rel:
        att.set_pos_encoding(pos)
    gen = torch.Generator().manual_seed(N)
    with torch.no_grad():
        att.qkv.weight.copy_(torch.randn(3 * D, D, generator=gen) * 1.3 / D ** 0.5)     # q, k, v of spread 1.3
        att.proj.weight.copy_(torch.randn(D, D, generator=gen) * 0.1)
        att.proj.bias.copy_(torch.randn(D, generator=gen) * 0.1)
        if rel:
            pos.relative_position_bias_table.copy_(torch.randn(pos.relative_position_bias_table.shape, generator=gen) * 0.5)
    att.cuda()
    x, dy, r = (torch.randn(B, N, D, generator=gen) for _ in range(3))
    xd = x.cuda().to(dtype).requires_grad_(True)
    rd = r.cuda().to(dtype).requires_grad_(True) if resid else None
    y = att(xd, resid=rd)
    y.backward(dy.cuda().to(dtype))
    rq = lambda v: v.to(dtype).double()  # noqa: E731
    xr, wq, wp = (rq(v).requires_grad_(True) for v in (x, att.qkv.weight.detach().cpu(), att.proj.weight.detach().cpu()))
    bp = att.proj.bias.detach().cpu().double().requires_grad_(True)
    qkv = (xr @ wq.t()).reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    tab = pos.relative_position_bias_table.detach().cpu().double().requires_grad_(True) if rel else None
    o = O.attention_core(qkv[0], qkv[1], qkv[2], hd ** -0.5, None, O.relative_bias(tab, N) if rel else None)
    ref = o.transpose(1, 2).reshape(B, N, D) @ wp.t() + bp
    if resid:
        ref = ref + rq(r)
    ref.backward(rq(dy))
    fam = "dropin rel" if rel else "dropin none"
    assert note(fam, dt, "random", "y", rel_err(y.detach().float().cpu(), ref.detach())) < otol
    assert note(fam, dt, "random", "dx", rel_err(xd.grad.float().cpu(), xr.grad)) < gtol
    assert note(fam, dt, "random", "dwqkv", rel_err(att.qkv.weight.grad.cpu(), wq.grad)) < gtol
    assert note(fam, dt, "random", "dwproj", rel_err(att.proj.weight.grad.cpu(), wp.grad)) < gtol
    assert note(fam, dt, "random", "dbproj", rel_err(att.proj.bias.grad.cpu(), bp.grad)) < gtol
    if rel:
        assert note(fam, dt, "random", "dtable", rel_err(pos.relative_position_bias_table.grad.cpu(), tab.grad)) < gtol
    if resid:
        assert torch.equal(rd.grad, dy.cuda().to(dtype))


# ------------------------------------------------------------------------------------------ engine at 26 tokens
@pytest.mark.parametrize("tag", ["rope-mixed", "relative"])
def test_engine_at_26_tokens(tag):
    """--img_size 20 --patch_size 4 (N = 26, hd 32), in the style of test_engine_runs_the_other_geometries_the_cli_accepts:
    fp32 logits, loss and every gradient against the oracle, then three captured bf16 steps stay finite."""
    from test_bench_path_gpu import build
    from vitpe.engine import TrainEngine
    geom = dict(depth=1, img_size=20, embed_dim=64, num_heads=2)
    cfg, model = build(tag, {}, geom)
    assert cfg.seq_len == 26
    params = {n: p.detach().cpu().clone() for n, p in model.named_parameters()}
    B = 3
    images, labels = O.closed_form_batch(cfg, B, salt=7)
    ref_logits, ref_loss, ref_grads = O.loss_and_grads(cfg, params, images, labels)
    eng = TrainEngine(model, B, compute_dtype=torch.float32, use_graph=False)
    assert not eng.attn_fused
    eng._load_batch(images.cuda(), labels.cuda())
    eng.forward_backward()
    assert rel_err(eng.logits.cpu(), ref_logits) < 1e-4
    assert abs(float(eng.out2[0]) - float(ref_loss)) < 1e-4
    for n, p in model.named_parameters():
        assert rel_err(p.grad.cpu(), ref_grads[n]) < 1e-3, n
    cfg, model = build(tag, {}, geom, seeded=True)
    eb = TrainEngine(model, B, compute_dtype=torch.bfloat16, use_graph=True)
    for _ in range(3):
        eb.step(images.cuda(), labels.cuda())
    torch.cuda.synchronize()
    assert torch.isfinite(eb.flat_p).all()
