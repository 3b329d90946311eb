"""The polynomial relative position bias at every degree 0-7 on the GPU, entry point by entry point against the float64
reference of poly_degree_ref.py.  The public `degree` selects code that the implementations do not share: the Horner
table of stage_poly (every attention kernel), the two polynomial instantiations of the bf16 fused backward (PDEG = 3 for
degrees 0-3, PDEG = 7 above), the run-time `k <= degree` loops of the fp32 fused backward and of the core backward, the
flush of degree + 1 floats per head group, and the stand-alone bias kernels of pe.hip.

Gates:
  a. polynomial_bias / polynomial_bias_bwd: every power against its own scale sum |dbias| d^k, by (terms + 4) 2^-23 (the
     manner of test_embed_dgrad_gpu.py; terms = the summands of the component);
  b. forward outputs: the project's 1e-4 (fp32) / 3e-2 (bf16) under rel_err = max|a - b| / max|b| (one scale per output);
  c. backward on exact inputs (poly_degree_ref.exact_case): every component k of every head on its own,
     |got - ref| <= C_EXACT 2^-23 E_k.  C_EXACT is four times the worst ratio the kernels were measured at against the
     float64 reference (profiles/poly_degree_parity.jsonl, check "exact:c_ratio"), rounded up to a power of two, and may
     not exceed 16.  test_poly_degree_cpu.py shows every wrong variant of the reference at 64 or more;
  d. backward on random inputs: d_qkv under the gates of (b), the coefficient gradient per component against
     sum |dS| d^k with the same 1e-4 / 3e-2 factors.  This gate is loose (it is there for the fused-LayerNorm
     instantiations); (c) carries the precision;
  e. in (c) and (d) the gradient buffer is prefilled and must be added to, and eight sentinel floats behind the
     degree + 1 (H (degree + 1)) live ones, in the same allocation, must be bit-unchanged;
  g. degrees -1 and 8 are refused by every attention entry point (each reaches pe_ok of csrc/attn_common.h before it
     launches anything: fused_fwd / fused_bwd of attn.hip, vitpe_fused_attention_fwd_wide, core_entry,
     vitpe_attention_core_stats and vitpe_attention_fused64_fwd) and leave their outputs untouched.

Figures are recorded first (profiles/poly_degree_parity.jsonl through parity_report.py) and asserted afterwards.
"""
import math

import pytest
import torch

import poly_degree_ref as R
from conftest import rel_err
from parity_report import Report

pytestmark = pytest.mark.gpu

DT = R.DT
TOL = {"f32": 1e-4, "bf16": 3e-2}
C_EXACT = 2.0           # (c): worst measured ratio 0.32 to 0.42 over three runs (attn_core_bwd_kernel at hd 48; the flush is
                        # atomic, its order varies): 0.42 x 4 = 1.69 -> 2
assert C_EXACT <= R.C_CAP
N_SENTINEL = 8
PH = [False, True]


@pytest.fixture(scope="module")
def K():
    from vitpe import kernels
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return kernels


@pytest.fixture(scope="module")
def report():
    r = Report("test_poly_degree_gpu", "poly_degree_parity.jsonl")
    yield r
    r.close()


def dev(t, dtype=None):
    t = t.cuda()
    return t.to(dtype).contiguous() if dtype is not None else t.contiguous()


def tables(K, c, coeff=None, degree=None):
    return K.PETables("polynomial", c.G, coeff=dev(c.coeff if coeff is None else coeff), degree=c.degree if degree is None else degree,
                      coeff_per_head=c.per_head)


def ph_id(p):
    return "perhead" if p else "shared"


def pow2_near(x):
    """a power of two of the size of x / 4 (exact in fp32), 1 for x = 0"""
    x = float(x)
    return 2.0 ** (math.floor(math.log2(x)) - 2) if x > 0 else 1.0


class GradBuffer:
    """The coefficient-gradient operand of a backward: the live floats prefilled with known values of the size of a quarter
    of their scale, alternating in sign, and N_SENTINEL floats behind them in the same allocation."""

    def __init__(self, scale):
        self.shape = tuple(scale.shape)
        n = scale.numel()
        self.fill = torch.tensor([(-1.0) ** i * pow2_near(s) for i, s in enumerate(scale.reshape(-1).tolist())], dtype=torch.float32)
        self.sentinel = torch.tensor([12345.0 + 3 * i for i in range(N_SENTINEL)], dtype=torch.float32)
        self.buf = torch.cat([self.fill, self.sentinel]).cuda()
        self.live = self.buf[:n].view(self.shape)
        assert self.live.data_ptr() == self.buf.data_ptr() and self.live.is_contiguous()

    def added(self):
        """what the kernel added to the live floats, float64 (the prefill is exact in fp32)"""
        return self.buf[:self.fill.numel()].cpu().to(R.F64).reshape(self.shape) - self.fill.to(R.F64).reshape(self.shape)

    def sentinels_moved(self):
        got = self.buf[self.fill.numel():].cpu()
        return int((got.view(torch.int32) != self.sentinel.view(torch.int32)).sum())


def check_grad(case, got_buf, ref_g, scale, factor, key):
    """every component on its own, against its own scale; the buffer contract (e)"""
    # (a kernel that overwrote the prefill instead of adding to it is off by the prefill, about a quarter of the scale)
    case.le(key, R.excess(got_buf.added(), ref_g, factor * scale), 1.0)
    case.eq("sentinels_moved", got_buf.sentinels_moved(), 0)


# ------------------------------------------------------------------------------------------ a. the stand-alone bias kernels
@pytest.mark.parametrize("per_head", PH, ids=ph_id)
@pytest.mark.parametrize("degree", range(8))
def test_polynomial_bias_and_its_backward(K, report, degree, per_head):
    """poly_bias_kernel / poly_bias_bwd_kernel (pe.hip): G = 2 gives 16 pairs for the 256 threads of a power's workgroup"""
    for G in (2, 4, 8, 14):
        for H in (1, 3):
            c = report.case("bias", f"d{degree}-{ph_id(per_head)}-G{G}-H{H}")
            N = G * G + 1
            coeff = R.coeffs(degree, G, H, per_head, 900 + 10 * degree + G + H)
            got = K.polynomial_bias(dev(coeff), H, G, degree, per_head).cpu()
            ref = R.bias_ref(coeff.to(R.F64), H, G, per_head)
            mag = R.bias_ref(coeff.to(R.F64).abs(), H, G, per_head)            # sum_k |c_k| d^k
            c.le("fwd", R.excess(got, ref, (degree + 1 + 4) * R.EPS32 * mag), 1.0)
            c.eq("fwd_class_row_col", int((got[:, 0, :] != 0).sum() + (got[:, :, 0] != 0).sum()), 0)
            dbias = R.rnd(H, N, N, seed=degree * 100 + G * 7 + H)               # class row and column not zero: they are masked
            gg = K.polynomial_bias_bwd(dev(dbias), H, G, degree, per_head).cpu()
            g, a = R.bias_bwd_ref(dbias.to(R.F64), G, degree, per_head)
            assert gg.shape == g.shape
            terms = (G * G) ** 2 * (1 if per_head else H)
            c.le("bwd", R.excess(gg, g, (terms + 4) * R.EPS32 * a), 1.0)
            c.done()


# ------------------------------------------------------------------------------------------ b. forward
def ln_operands(K, c):
    """raw tokens, LayerNorm parameters and statistics of a fused-LayerNorm run, and the normalised tokens the stand-alone
    LayerNorm kernel gives (what the reference is computed on, as test_fused_attention_fwd_wide does)"""
    xr = dev(c.xn * 1.7 + 0.4, DT[c.dt])
    gam, bet = dev(1 + 0.1 * R.rnd(c.D, seed=5)), dev(0.1 * R.rnd(c.D, seed=6))
    xn, mean, rstd = K.layernorm_fwd(xr, gam, bet)
    return xr, (gam, bet, mean, rstd), xn


def ref_on(c, xn_dev):
    """core_ref of a random case on the normalised tokens a device LayerNorm produced"""
    qd = lambda t: t.to(DT[c.dt]).to(R.F64)   # noqa: E731
    qkv = xn_dev.cpu().to(R.F64) @ qd(c.wqkv).t()
    return R.core_ref(qkv, qd(c.dout), c.H, c.G, c.coeff.to(R.F64), c.per_head)


@pytest.mark.parametrize("per_head", PH, ids=ph_id)
@pytest.mark.parametrize("degree", R.FWD_DEGREES)
@pytest.mark.parametrize("ln", [False, True], ids=["plain", "ln"])
@pytest.mark.parametrize("geom", R.FUSED_GEOMS, ids=R.case_id)
def test_fused_attention_fwd(K, report, geom, ln, degree, per_head):
    c = R.random_case(*geom, degree, per_head)
    w = K.pack_qkv_weights(dev(c.wqkv), DT[c.dt], c.H)
    t = tables(K, c)
    if ln:
        xr, lnp, xn = ln_operands(K, c)
        xo = torch.empty_like(xr)
        out = K.fused_attention_fwd(xr, w, c.H, t, ln=lnp, xn_out=xo)
        ref = ref_on(c, xo)      # (the kernel's own normalised tokens, as test_kernels_gpu.py)
    else:
        out = K.fused_attention_fwd(dev(c.xn, DT[c.dt]), w, c.H, t)
        ref = R.random_ref(c, core=False)
    rc = report.case("fwd_fused", f"{R.case_id(geom)}-{'ln' if ln else 'plain'}-d{degree}-{ph_id(per_head)}")
    rc.lt("out", rel_err(out.float().cpu(), ref.out.float()), TOL[c.dt])
    rc.done()


@pytest.mark.parametrize("per_head", PH, ids=ph_id)
@pytest.mark.parametrize("degree", R.FWD_DEGREES)
@pytest.mark.parametrize("ln", [False, True], ids=["plain", "ln"])
def test_fused_attention_fwd_wide(K, report, ln, degree, per_head):
    c = R.random_case(*R.WIDE_GEOM, degree, per_head)
    w = K.pack_qkv_weights_wide(dev(c.wqkv), torch.bfloat16, c.H)
    t = tables(K, c)
    if ln:
        xr, lnp, xn = ln_operands(K, c)
        xo = torch.empty_like(xr)
        out = K.fused_attention_fwd_wide(xr, w, c.H, t, ln=lnp, xn_out=xo)
        ref = ref_on(c, xo)      # (the wide kernel's own normalised tokens, as test_kernels_gpu.py)
    else:
        out = K.fused_attention_fwd_wide(dev(c.xn, torch.bfloat16), w, c.H, t)
        ref = R.random_ref(c, core=False)
    rc = report.case("fwd_wide", f"{'ln' if ln else 'plain'}-d{degree}-{ph_id(per_head)}")
    rc.lt("out", rel_err(out.float().cpu(), ref.out.float()), TOL["bf16"])
    rc.done()


@pytest.mark.parametrize("per_head", PH, ids=ph_id)
@pytest.mark.parametrize("degree", R.FWD_DEGREES)
def test_attention_fused64_fwd(K, report, degree, per_head):
    c = R.random_case(*R.FUSED64_GEOM, degree, per_head)
    bf = torch.bfloat16
    out = K.attention_fused64_fwd(dev(c.xn, bf), K.pack_weight_frags(dev(c.wqkv), bf, 64, 0), c.H, tables(K, c))
    rc = report.case("fwd_fused64", f"d{degree}-{ph_id(per_head)}")
    rc.lt("out", rel_err(out.float().cpu(), R.random_ref(c, core=False).out.float()), TOL["bf16"])
    rc.done()


def stats_of(ref, G, unit):
    from attn_stats_ref import ref_stats
    return ref_stats(ref.probs, G, unit)


CORE_FWD_CASES = [g + (d, ph) for g in R.CORE_GEOMS for d in R.FWD_DEGREES for ph in PH] + R.FAR_CASES


@pytest.mark.parametrize("case", CORE_FWD_CASES, ids=R.case_id)
def test_attention_core_fwd_probs_and_stats(K, report, case):
    """the three forward readers of the bias-by-distance table on one projection; the last two cases reach 30 of its 32
    entries (G = 16)"""
    c = R.random_case(*case)
    ref = R.random_ref(c, core=True)
    qkv, t = dev(c.qkv, DT[c.dt]), tables(K, c)
    rc = report.case("fwd_core", R.case_id(case))
    rc.lt("out", rel_err(K.attention_core_fwd(qkv, c.H, t).float().cpu(), ref.out.float()), TOL[c.dt])
    probs = K.attention_core_probs(qkv, c.H, t)
    rc.lt("probs", rel_err(probs.cpu(), ref.probs.float()), TOL[c.dt])
    rc.lt("probs_cls", rel_err(K.attention_core_probs(qkv, c.H, t, cls_only=True).cpu(), ref.probs[:, :, 0].float()), TOL[c.dt])
    stats, _ = K.attention_core_stats(qkv, c.H, t, unit=4.0)
    want = stats_of(ref, c.G, 4.0)
    for i, name in enumerate(("distance", "entropy", "cls_mass", "cls_entropy")):
        rc.lt("stat_" + name, rel_err(stats[..., i].cpu(), want[..., i].float()), TOL[c.dt])
    rc.done()


# ------------------------------------------------------------------------------------------ c. backward, exact inputs
def run_bwd(K, c, buf, ln=None, xn=None, drop=False):
    """the backward entry point of a case's kernel -> d_qkv; the coefficient gradient is accumulated into buf.live"""
    dt, t = DT[c.dt], tables(K, c)
    if c.kernel == "fused":
        w = K.pack_qkv_weights(dev(c.wqkv), dt, c.H)
        return K.fused_attention_bwd(dev(c.xn, dt) if xn is None else xn, w, dev(c.dout, dt), c.H, t, None, buf.live, None, ln=ln)
    if drop:
        rng = K.new_rng_pairs(1, "cuda")[0]
        return K.attention_core_bwd_drop(dev(c.qkv, dt), dev(c.dout, dt), c.H, t, rng, 0.0, None, buf.live, None)
    return K.attention_core_bwd(dev(c.qkv, dt), dev(c.dout, dt), c.H, t, None, buf.live, None)


def instantiation(c):
    if c.kernel == "fused":
        return "attn_bwd_kernel" if c.dt == "f32" else f"attn_bwd_reg_kernel<PDEG={3 if c.degree <= 3 else 7}>"
    return f"attn_core_bwd_kernel<hd={c.hd}>"


@pytest.mark.parametrize("case", R.EXACT_CASES + R.FAR_CASES, ids=R.case_id)
def test_backward_on_exact_inputs_every_power_on_its_own(K, report, case):
    c = R.exact_case(*case)
    ref = R.exact_ref(c)
    buf = GradBuffer(ref.E)
    dqkv = run_bwd(K, c, buf)
    rc = report.case("exact", f"{R.case_id(case)}:{instantiation(c)}")
    got = buf.added()
    ratio = (got - ref.g).abs() / (R.EPS32 * ref.E)
    rc.le("c_ratio", float(ratio.max()), C_EXACT)
    rc.le("c_ratio_k0", float(ratio.reshape(-1, c.degree + 1)[:, 0].max()), C_EXACT)
    rc.eq("sentinels_moved", buf.sentinels_moved(), 0)
    rc.lt("dqkv", rel_err(dqkv.float().cpu(), ref.dqkv.float()), TOL[c.dt])
    rc.done()


# ------------------------------------------------------------------------------------------ d. backward, random inputs
RANDOM_BWD = ([(g, v, d, ph) for g in R.FUSED_GEOMS for v in ("plain", "ln") for d in R.RANDOM_DEGREES for ph in PH]
              + [(g, v, d, ph) for g in R.CORE_GEOMS for v in ("plain", "drop0") for d in R.RANDOM_DEGREES for ph in PH])


@pytest.mark.parametrize("geom,variant,degree,per_head", RANDOM_BWD,
                         ids=[f"{R.case_id(g)}-{v}-d{d}-{ph_id(p)}" for g, v, d, p in RANDOM_BWD])
def test_backward_on_random_inputs(K, report, geom, variant, degree, per_head):
    c = R.random_case(*geom, degree, per_head)
    if variant == "ln":
        xr, lnp, xn = ln_operands(K, c)
        ref = ref_on(c, xn)
        buf = GradBuffer(ref.A)
        dqkv = run_bwd(K, c, buf, ln=lnp, xn=xr)
    else:
        ref = R.random_ref(c, core=c.kernel != "fused")
        buf = GradBuffer(ref.A)
        dqkv = run_bwd(K, c, buf, drop=variant == "drop0")
    rc = report.case("random", f"{R.case_id(geom)}-{variant}-d{degree}-{ph_id(per_head)}")
    rc.lt("dqkv", rel_err(dqkv.float().cpu(), ref.dqkv.float()), TOL[c.dt])
    check_grad(rc, buf, ref.g, ref.A, TOL[c.dt], "dcoeff_per_power")
    rc.done()


# ------------------------------------------------------------------------------------------ f. above the kernels
@pytest.mark.parametrize("mode", ["polynomial", "polynomial_perhead"])
@pytest.mark.parametrize("route", ["b", "d16"])
def test_attention_op_at_degree_5(route, mode):
    """torch.ops.vitpe.attention on the wide32 / fused-backward route and on the core route: y and every gradient, with
    the runner and the gates of test_ops_gpu.py"""
    import ops_ref
    import test_ops_gpu as T
    import vitpe.ops  # noqa: F401
    c = ops_ref.attn_case(route, mode, True, degree=5)
    assert c.pe["coeff"].shape[-1] == 6 and ops_ref.op_pe_args(c)[4] == 5
    T.check_attention(T.AttnRun(c), T.attn_key(c, "attention_degree5"), f"{mode} degree 5")


COEFF = "pos_embed.coefficients"


def per_power_summands(cfg, params, images, labels, ref_grads):
    """The size of the summands of every component of d coefficients before they cancel over the batch: the oracle's
    gradient of each image on its own (the loss is a batch mean, so their mean IS the batch gradient: checked per
    component), scale = the mean of their magnitudes.  Same shape as the coefficients: every power of every head has its
    own scale, where _summand_scale of test_bench_path_gpu.py has one for the whole vector."""
    from oracle import vit_oracle as O
    parts = torch.stack([O.loss_and_grads(cfg, params, images[i:i + 1], labels[i:i + 1])[2][COEFF].to(R.F64)
                         for i in range(images.shape[0])])
    scale = parts.abs().mean(0)
    assert bool(((parts.mean(0) - ref_grads[COEFF].to(R.F64)).abs() <= 1e-3 * scale + 1e-5 * scale.max()).all())   # (fp32 oracle)
    return scale


def per_power_excess(got, ref, scale, factor):
    """worst over the components of |got - ref| / (factor max(|ref|, scale))"""
    ref = ref.to(R.F64)
    return R.excess(got.cpu(), ref, factor * torch.maximum(ref.abs(), scale))


@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("degree,shared", [(1, True), (5, False)], ids=["d1-shared", "d5-perhead"])
def test_dropin_model_vs_oracle(report, degree, shared, depth):
    """VisionTransformer(pos_encoding="polynomial", poly_degree=d) in fp32 through autograd, gates of test_model_gpu.py
    (logits and loss 1e-4, gradients 1e-3 max-norm); the coefficients per power against that power's summand scale.
    With ONE block the logits do not depend on the coefficients at all: the head reads the class token, whose row of the
    bias is zero, and no later block mixes the patch rows into it.  The oracle's coefficient gradient is then exactly
    zero and the kernels' must be too (a scale of 0 admits no error); two blocks give every power a gradient."""
    import test_model_gpu as M
    from oracle import vit_oracle as O
    extra = {"pos_encoding": "polynomial", "poly_degree": degree, "poly_shared_heads": shared}
    cfg, model = M.build("polynomial", extra, dict(embed_dim=96, depth=depth, num_heads=3))
    assert tuple(model.pos_embed.coefficients.shape) == ((degree + 1,) if shared else (3, degree + 1))
    images, labels = O.closed_form_batch(cfg, 4)
    logits = model(images.cuda())
    loss = torch.nn.CrossEntropyLoss()(logits, labels.cuda())
    loss.backward()
    params = O.closed_form_params(cfg)
    ref_logits, ref_loss, ref_grads = O.loss_and_grads(cfg, params, images, labels)
    rc = report.case("dropin", f"d{degree}-{ph_id(not shared)}-depth{depth}")
    rc.lt("logits", rel_err(logits.detach().cpu(), ref_logits), 1e-4)
    rc.lt("loss", abs(float(loss) - float(ref_loss)), 1e-4)
    for name, p_ in model.named_parameters():
        if name != COEFF:
            rc.lt("grad", rel_err(p_.grad.cpu(), ref_grads[name]), 1e-3)
    scale = per_power_summands(cfg, params, images, labels, ref_grads)
    assert bool((scale == 0).all() if depth == 1 else (scale > 0).all())
    rc.le("coeff_per_power", per_power_excess(model.pos_embed.coefficients.grad, ref_grads[COEFF], scale, 1e-3), 1.0)
    rc.done()


@pytest.mark.parametrize("degree,shared", [(0, True), (7, False)], ids=["d0-shared", "d7-perhead"])
def test_bf16_captured_step_at_degrees_0_and_7(report, degree, shared):
    """One captured bf16 TrainEngine step at B = 16 with the helpers and gates of test_bench_path_gpu.py: coefficient
    tensors of 1 and 8 H floats in the flat parameter, AdamW and shadow layouts.  The coefficients are compared per power
    against that power's summand scale (5e-2, the file's gradient gate), not with one max-norm over the vector."""
    import test_bench_path_gpu as P
    from oracle import vit_oracle as O
    from vitpe.engine import TrainEngine
    B = 16
    extra = {"pos_encoding": "polynomial", "poly_degree": degree, "poly_shared_heads": shared}
    cfg, model = P.build("polynomial", extra, {}, seeded=True)
    assert model.pos_embed.coefficients.numel() == (1 if shared else 8 * cfg.num_heads)
    # the reference's initialisation gives every power the same std 0.02: at degree 7 the bias reaches 0.02 x 14^7, the
    # softmax is one-hot and the coefficient gradient vanishes.  Power k is scaled by 14^-k instead, as everywhere here.
    with torch.no_grad():
        model.pos_embed.coefficients.copy_(R.coeffs(degree, 8, cfg.num_heads, not shared, 4242).reshape(model.pos_embed.coefficients.shape))
    P.bf16_round_(model)
    params ={n: p.detach().cpu().clone() for n, p in model.named_parameters()}
    g = torch.Generator().manual_seed(11)
    images, labels = torch.randn(B, 3, 32, 32, generator=g), torch.randint(0, 10, (B,), generator=g)
    ref_logits, ref_loss, ref_grads = O.loss_and_grads(cfg, params, images, labels)
    eng = TrainEngine(model, B, compute_dtype=torch.bfloat16, use_graph=True)
    assert eng.attn_fused and eng.fuse_ln and eng.fuse_ln_bwd and eng.tail2 and eng.group_wgrad
    grads = P.graph_step_gradients(eng, images.cuda(), labels.cuda())
    assert eng.graph_fb is not None
    scale = per_power_summands(cfg, params, images, labels, ref_grads)
    assert bool((scale > 0).all()), "a component without gradient checks nothing"
    fig = {}
    bad = P.compare_all("step", model, grads, ref_grads, fig, summand_scale={COEFF: float(scale.max())})
    rc = report.case("captured_step", f"d{degree}-{ph_id(not shared)}")
    rc.le("logits", rel_err(eng.logits.cpu(), ref_logits), 5e-2)
    rc.le("loss", abs(float(eng.out2[0]) - float(ref_loss)), 2e-2)
    rc.le("grad_rel", fig["step"]["rel"], 5e-2)
    rc.le("grad_cos_deficit", 1.0 - fig["step"]["cos"], 1e-3)
    rc.le("grad_row", fig["step"]["row"], 0.01)
    rc.le("coeff_per_power", per_power_excess(grads[COEFF], ref_grads[COEFF], scale, 5e-2), 1.0)
    rc.done()
    assert not bad, bad


# ------------------------------------------------------------------------------------------ g. refusals
@pytest.mark.parametrize("degree", [-1, 8])
def test_degrees_outside_0_to_7_are_refused_everywhere(K, degree):
    """every attention entry point raises before it launches anything: outputs and gradient buffers keep their bytes"""
    from vitpe._lib import VitpeError
    bf = torch.bfloat16
    coeff = torch.full((6, 9), 0.25)                      # enough floats for any reading of the degree

    def pe(G, per_head=False):
        return K.PETables("polynomial", G, coeff=dev(coeff), degree=degree, coeff_per_head=per_head)

    def guard(*shape, dtype=torch.float32):
        return torch.full(shape, 7.0, device="cuda", dtype=dtype)

    def refused(call, *outs):
        with pytest.raises(VitpeError):
            call()
        torch.cuda.synchronize()
        for o in outs:
            assert bool((o == 7.0).all()), "a refused call wrote its output"

    for dt, D, H in (("f32", 96, 3), ("bf16", 192, 6)):
        x, w, o, dq, dc = guard(3, 65, D, dtype=DT[dt]), guard(3 * D, D, dtype=DT[dt]), guard(3, 65, D, dtype=DT[dt]), \
            guard(3, 65, 3 * D, dtype=DT[dt]), guard(H, 9)
        gam, stat = guard(D), guard(3 * 65)
        for per_head in PH:
            refused(lambda: K.fused_attention_fwd(x, w, H, pe(8, per_head), out=o), o)
            refused(lambda: K.fused_attention_fwd(x, w, H, pe(8, per_head), out=o, ln=(gam, gam, stat, stat), xn_out=dq[..., :D].contiguous()), o)
            refused(lambda: K.fused_attention_bwd(x, w, x, H, pe(8, per_head), None, dc, None, out=dq), dq, dc)
            refused(lambda: K.fused_attention_bwd(x, w, x, H, pe(8, per_head), None, dc, None, out=dq, ln=(gam, gam, stat, stat)), dq, dc)
    x, w, o = guard(3, 65, 192, dtype=bf), guard(3 * 192 * 192, dtype=bf), guard(3, 65, 192, dtype=bf)
    refused(lambda: K.fused_attention_fwd_wide(x, w, 6, pe(8), out=o), o)
    x, w, o = guard(3, 197, 128, dtype=bf), guard(3 * 128 * 128, dtype=bf), guard(3, 197, 128, dtype=bf)
    qo = guard(3, 197, 3 * 128, dtype=bf)
    refused(lambda: K.attention_fused64_fwd(x, w, 2, pe(14), qkv_out=qo, out=o), o, qo)
    rng = K.new_rng_pairs(1, "cuda")[0]
    for dt, hd in (("f32", 32), ("bf16", 64), ("bf16", 48)):
        D = 2 * hd
        qkv, do, o, dq, dc = guard(3, 17, 3 * D, dtype=DT[dt]), guard(3, 17, D, dtype=DT[dt]), guard(3, 17, D, dtype=DT[dt]), \
            guard(3, 17, 3 * D, dtype=DT[dt]), guard(2, 9)
        pr, prc, st = guard(3, 2, 17, 17), guard(3, 2, 17), guard(3, 2, 4)
        refused(lambda: K.attention_core_fwd(qkv, 2, pe(4), out=o), o)
        refused(lambda: K.attention_core_fwd_drop(qkv, 2, pe(4), rng, 0.1, out=o), o)
        refused(lambda: K.attention_core_probs(qkv, 2, pe(4), out=pr), pr)
        refused(lambda: K.attention_core_probs(qkv, 2, pe(4), cls_only=True, out=prc), prc)
        refused(lambda: K.attention_core_stats(qkv, 2, pe(4), out=(st, None)), st)
        refused(lambda: K.attention_core_bwd(qkv, do, 2, pe(4, True), None, dc, None, out=dq), dq, dc)
        refused(lambda: K.attention_core_bwd_drop(qkv, do, 2, pe(4, True), rng, 0.1, None, dc, None, out=dq), dq, dc)
