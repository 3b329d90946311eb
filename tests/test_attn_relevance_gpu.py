"""Gradient-weighted attention relevance on the GPU: vitpe_attention_core_relevance through kernels.attention_core_relevance,
Attention / Block.attention_relevance and VisionTransformer.attention_relevance, against the float64 references of
attn_relevance_ref.py (pinned to autograd and to the explicit products in test_attn_relevance_cpu.py) on ref_probs
(test_attn_probs_cpu.py).

Operands are rounded as the statistics tests round them: x and W to the compute type, the projection rounded to bf16 in
bf16 mode, dout to the compute type; the device buffers hold exactly the values the float64 reference sees.  The error
measure throughout is max|got - ref| / max(colsum_abs), colsum_abs_j = sum_i |w_i| |G_ij A_ij| (attn_relevance_ref.py); the
gate is the suite's tol(dt) (1e-4 / 3e-2) unless a test says otherwise.  B = 2, H = 2 throughout, both clamp values unless
stated.  The measured figures go to profiles/attn_relevance_parity.jsonl before anything is asserted."""
import functools
import math

import pytest
import torch

from attn_relevance_ref import err_measure, ref_grad_attn, ref_model_relevance, ref_relevance
from attn_tokens import DT, Guarded, edge_rows, guarded_input, masked_case, q, tol, token_case
from oracle import vit_oracle as O
from parity_report import Report
from test_attn_probs_cpu import ref_probs
from test_attn_stats_gpu import PARITY as STATS_PARITY, shift_case
from test_kernels_gpu import K, dev, device_pe, rnd  # noqa: F401  (K: the kernels fixture)

pytestmark = pytest.mark.gpu

B, H = 2, 2
CLAMPS = (True, False)


@pytest.fixture(scope="module")
def report():
    r = Report("test_attn_relevance_gpu", "attn_relevance_parity.jsonl")
    yield r
    r.close()


@functools.lru_cache(maxsize=None)
def case(mode, N, hd, dt, masked=False):
    """(G, qkv [B, N, 3D] and dout [B, N, D] fp32 on the CPU holding the values the kernel reads, pe leaves, signed weights
    [B, N], and in float64 the probabilities, their gradient and {clamp: (colsum, colsum_abs)}) -- built once"""
    mk = masked_case if masked else token_case
    N, hd, G, xn, wqkv, dout, pe = mk(mode, N, H * hd, H, B, seed=90)
    qkv = torch.nn.functional.linear(q(xn, dt), q(wqkv, dt))
    if dt == "bf16":
        qkv = qkv.bfloat16().float()
    dout = q(dout, dt)
    p = ref_probs(qkv.double(), H, mode, pe)
    g = ref_grad_attn(qkv, dout, H)
    w = rnd(B, N, seed=91)
    return G, qkv, dout, pe, w, p, g, {c: ref_relevance(p, g, w, c) for c in CLAMPS}


def run(K, mode, N, hd, dt, clamp, masked=False, out=None, guard=False):
    G, qkv, dout, pe, w = case(mode, N, hd, dt, masked)[:5]
    qd, dd, wd = dev(qkv, DT[dt]), dev(dout, DT[dt]), dev(w)
    if guard:
        qd, dd, wd = guarded_input(qd), guarded_input(dd), guarded_input(wd)
    return K.attention_core_relevance(qd, dd, H, device_pe(K, mode, pe, H, G), wd, clamp=clamp, out=out)


def gate(c, got, refs, limit, suffix=""):
    """records the error measure of one result against `limit` in the Case c"""
    ref, ref_abs = refs
    c.lt("colsum" + suffix, err_measure(got, ref, ref_abs), limit)


# ------------------------------------------------------------------------------------------ 1. parity against float64
# the statistics tests' list (one case each at 10, 13 and 17 tiles: one, two and three rounds of query-tile jobs per wave,
# i.e. the slab is stored, then added to), and the remaining head dimensions
PARITY = list(STATS_PARITY) + [("none", 26, 48), ("none", 26, 96), ("none", 26, 128)]


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("mode,N,hd", PARITY)
def test_colsum_matches_the_float64_reference(K, report, mode, N, hd, dt):
    refs = case(mode, N, hd, dt)[7]
    c = report.case("parity", f"{mode}-N{N}-hd{hd}-{dt}")
    for clamp in CLAMPS:
        got = run(K, mode, N, hd, dt, clamp)
        assert got.dtype == torch.float32 and tuple(got.shape) == (B, H, N) and not got.requires_grad
        gate(c, got, refs[clamp], tol(dt), suffix="" if clamp else "_signed")
    print(f"{mode} N={N} hd={hd} {dt}: " + " ".join(f"{k} {v:.2e}" for k, v in c.figures.items()))
    c.done()


# ------------------------------------------------------------------------------------------ 2. exact inputs
def small_ints(n, mul, mod, off):
    return ((torch.arange(n) * mul) % mod - off).float()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("N", [18, 26, 65])
def test_uniform_rows_closed_form(K, report, N, dt):
    """q = k = 0: every row is uniform over its N keys.  Every V row of head h is u_h, dO_i = c_i u', c_i integers of both
    signs: G_ij = c_i (u_h . u'), colsum_j = (u_h . u') / N . sum_i w_i f(c_i) where u_h . u' > 0 -- the same for every key
    j.  No operand is rounded in either type.  A clamp on the wrong side, a missing 1 / N (or 1 / (N + padding)) and a
    padding query or key that was admitted each change it by an order-one factor.  Gate 1e-5."""
    hd = 32
    u = torch.stack([small_ints(hd, 3, 5, 2), 2.0 * small_ints(hd, 2, 7, 3)])        # [H, hd]
    up = torch.stack([small_ints(hd, 1, 3, 1), small_ints(hd, 5, 4, 1)])            # [H, hd]
    dots = (u.double() * up.double()).sum(-1)
    assert bool((dots != 0).all()) and float(dots[0]) != float(dots[1])
    cq = small_ints(N, 7, 9, 4)                                                     # [N], -4 .. 4
    assert bool((cq > 0).any()) and bool((cq < 0).any())
    qkv = torch.zeros(B, N, 3, H, hd)
    qkv[:, :, 2] = u
    dout = (cq[None, :, None, None] * up[None, None]).expand(B, N, H, hd).reshape(B, N, H * hd)
    w = rnd(B, N, seed=92)
    from vitpe.kernels import PETables
    c = report.case("uniform", f"N{N}-{dt}")
    for clamp in CLAMPS:
        got = K.attention_core_relevance(dev(qkv.reshape(B, N, 3 * H * hd), DT[dt]), dev(dout, DT[dt]), H,
                                         PETables("none", math.isqrt(N - 1)), dev(w), clamp=clamp)
        t = cq.double()[None, None, :] * dots[None, :, None] / N                    # [1, H, N]: G_ij A_ij, any j
        f = t.clamp(min=0.0) if clamp else t
        want = (w.double()[:, None, :] * f).sum(-1, keepdim=True).expand(B, H, N)
        mag = (w.double().abs()[:, None, :] * t.abs()).sum(-1, keepdim=True).expand(B, H, N)
        assert bool(torch.isfinite(got).all())
        gate(c, got, (want, mag), 1e-5, suffix="" if clamp else "_signed")
    c.done()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("N", [26, 65])   # 26: ten padding keys; 65: five tiles, one real token in the last
@pytest.mark.parametrize("shift", ["+1", "-1", "+G", "-G"])
def test_shifted_identities_with_asymmetric_gradients(K, report, shift, N, dt):
    """shift_case (test_attn_stats_gpu.py): row i puts its mass on key i + delta.  V_j and dO_i are small integers with
    dO_i . V_j depending asymmetrically on (i, j): colsum_j is w_{j - delta} f(G_{j - delta, j}) to within N e^-30, so a
    transposed G or a key or query index that is off by one is an order-one error.  No operand is rounded.  Gate 1e-5."""
    hd, G = 32, math.isqrt(N - 1)
    delta = {"+1": 1, "-1": -1, "+G": G, "-G": -G}[shift]
    table, p = shift_case(N, delta)
    f = torch.arange(hd)
    v = ((3 * torch.arange(N)[:, None] + f[None, :]) % 7 - 3).float()               # [N, hd]
    do = ((5 * torch.arange(N)[:, None] + 2 * f[None, :]) % 5 - 2).float()          # [N, hd]
    qkv = torch.zeros(B, N, 3, H, hd)
    qkv[:, :, 2, 0], qkv[:, :, 2, 1] = v, -v.flip(-1)
    qkv[1, :, 2] *= 2.0
    dout = torch.stack([do, do.flip(-1)], dim=1)[None].expand(B, N, H, hd).reshape(B, N, H * hd).contiguous()
    qkv = qkv.reshape(B, N, 3 * H * hd)
    g = ref_grad_attn(qkv, dout, H)
    assert float((g - g.transpose(-1, -2)).abs().max()) >= 1.0
    w = rnd(B, N, seed=93)
    from vitpe.kernels import PETables
    c = report.case("shifted", f"{shift}-N{N}-{dt}")
    for clamp in CLAMPS:
        got = K.attention_core_relevance(dev(qkv, DT[dt]), dev(dout, DT[dt]), H, PETables("relative", G, table=dev(table)),
                                         dev(w), clamp=clamp)
        gate(c, got, ref_relevance(p, g, w, clamp), 1e-5, suffix="" if clamp else "_signed")
    c.done()


# ------------------------------------------------------------------------------------------ 3. the forward kernel
@pytest.mark.parametrize("mode", ["none", "relative", "rope-mixed"])
def test_row_sums_agree_with_the_forward_kernel(K, report, mode):
    """fp32, N = 65, hd = 32, unclamped, weights = e_i: sum_j colsum_j = sum_j G_ij A_ij = dO_i . O_i, with O from
    attention_core_fwd on the same buffer.  Gate (N + 8) 2^-24 relative to sum_j |G_ij A_ij|: the linear worst case of an
    fp32 sum of N terms with a few roundings each."""
    N, hd, dt = 65, 32, "f32"
    G, qkv, dout, pe, _, p, g, _ = case(mode, N, hd, dt)
    bound = (N + 8) * 2.0 ** -24
    t, qd, dd = device_pe(K, mode, pe, H, G), dev(qkv, DT[dt]), dev(dout, DT[dt])
    o = K.attention_core_fwd(qd, H, t).cpu().double().reshape(B, N, H, hd)
    rowdot = (dout.double().reshape(B, N, H, hd) * o).sum(-1).permute(0, 2, 1)      # [B, H, N]: dO_i . O_i
    mag = (g * p).abs().sum(-1)                                                     # [B, H, N]: sum_j |G_ij A_ij|
    c = report.case("vs_forward_kernel", mode)
    for i in edge_rows(N):
        w = torch.zeros(B, N)
        w[:, i] = 1.0
        got = K.attention_core_relevance(qd, dd, H, t, dev(w), clamp=False).cpu().double().sum(-1)
        c.lt(f"row{i}", float(((got - rowdot[..., i]).abs() / mag[..., i]).max()), bound)
    c.done()


# ------------------------------------------------------------------------------------------ 4. token-count edges
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("mode", ["none", "relative"])
@pytest.mark.parametrize("N", [18, 31, 32, 49, 64, 66, 80])
def test_token_count_edges(K, report, mode, N, dt):
    """masked_case: a wrongly admitted or dropped key, or a table index off by one, is an order-one change of rows 0 and
    N - 1, whose mass sits on one key."""
    refs = case(mode, N, 32, dt, True)[7]
    c = report.case("edges", f"{mode}-N{N}-{dt}")
    for clamp in CLAMPS:
        gate(c, run(K, mode, N, 32, dt, clamp, masked=True), refs[clamp], tol(dt), suffix="" if clamp else "_signed")
    c.done()


# ------------------------------------------------------------------------------------------ 5. bounds
@pytest.mark.parametrize("mode,N", [("rope-mixed", 26), ("rope-mixed", 65), ("relative", 32)])
def test_nothing_is_written_or_read_out_of_bounds(K, report, mode, N):
    dt = "bf16"
    refs = case(mode, N, 32, dt)[7]
    c = report.case("bounds", f"{mode}-N{N}")
    for clamp in CLAMPS:
        o = Guarded((B, H, N), torch.float32)
        run(K, mode, N, 32, dt, clamp, out=o.t, guard=True)
        torch.cuda.synchronize()
        gate(c, o.check(f"colsum {mode} N={N}"), refs[clamp], tol(dt), suffix="" if clamp else "_signed")
    c.done()


# ------------------------------------------------------------------------------------------ 6. reproducibility
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("mode,N,hd", [("none", 26, 32), ("relative", 65, 32), ("rope-axial", 197, 64), ("rope-axial", 257, 32)])
def test_two_launches_give_the_same_bits(K, mode, N, hd, dt):
    for clamp in CLAMPS:
        assert torch.equal(run(K, mode, N, hd, dt, clamp), run(K, mode, N, hd, dt, clamp))


# ------------------------------------------------------------------------------------------ 7. modules and model
def model_err(got, ref, scale):
    return float((got.cpu().double() - ref).abs().max() / scale.abs().max())


@pytest.mark.parametrize("mode", ["rope-mixed", "relative"])
def test_model_attention_relevance(K, report, mode):
    from vitpe.vit import VisionTransformer
    torch.manual_seed(7)
    model = VisionTransformer(img_size=16, patch_size=4, embed_dim=64, depth=2, num_heads=H, pos_encoding=mode).cuda()
    cfg = O.VitConfig(img_size=16, patch_size=4, embed_dim=64, depth=2, num_heads=H, pos_encoding=mode)
    N = 17
    if mode == "relative":
        with torch.no_grad():
            model.pos_embed.relative_position_bias_table.copy_(rnd(H, 2 * N - 1, seed=86, scale=0.5))
    params = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    x = rnd(B, 3, 16, 16, seed=87)
    xd = x.cuda()
    x0 = xd.clone()
    tgt = torch.tensor([3, 8])
    model.eval()
    with torch.no_grad():
        before = model(xd)
    inner = model._relevance_pass(xd)[0].detach()
    assert torch.equal(inner, before), "the internal pass is not the forward's own sequence"
    model.train()
    state = torch.cuda.get_rng_state()
    got = {"default": model.attention_relevance(xd), "target": model.attention_relevance(xd, target=tgt.cuda()),
           "start1": model.attention_relevance(xd, start_layer=1), "signed": model.attention_relevance(xd, clamp=False)}
    assert torch.equal(torch.cuda.get_rng_state(), state), "attention_relevance consumed CUDA RNG"
    assert model.training and all(mod.training for mod in model.modules())
    assert all(prm.grad is None for prm in model.parameters())
    assert torch.equal(xd, x0) and not xd.requires_grad
    want = {"default": ref_model_relevance(cfg, params, x), "target": ref_model_relevance(cfg, params, x, target=tgt),
            "start1": ref_model_relevance(cfg, params, x, start=1), "signed": ref_model_relevance(cfg, params, x, clamp=False)}
    c = report.case("model", mode)
    c.lt("logits", float((before.cpu().double() - want["default"][1]).abs().max() / want["default"][1].abs().max()), tol("f32"))
    c.eq("argmax_target", int((before.argmax(1).cpu() != want["default"][2]).sum()), 0)
    for name, r in got.items():
        assert tuple(r.shape) == (B, N) and r.dtype == torch.float32 and not r.requires_grad and r.grad_fn is None
        ref, _, _, scale = want[name]
        c.lt(name, model_err(r, ref, scale), tol("f32"))
    c.done()
    with pytest.raises(ValueError):
        model.attention_relevance(xd, start_layer=2)
    with pytest.raises(ValueError):
        model.attention_relevance(xd, target=torch.zeros(B + 1, dtype=torch.int64, device="cuda"))
    assert model.training and all(mod.training for mod in model.modules())   # restored on an exception as well
    model.eval()
    with torch.no_grad():
        after = model(xd)
    assert torch.equal(before, after)


def test_attention_module_relevance_ignores_dropout_and_mode(K, report):
    from vitpe.positional_encoding import RelativePositionalEncoding
    from vitpe.vit import Attention, Block
    N = 26
    pe = RelativePositionalEncoding(N - 1, H)
    with torch.no_grad():
        pe.relative_position_bias_table.copy_(rnd(H, 2 * N - 1, seed=83, scale=0.5))
    torch.manual_seed(5)
    m = Attention(64, num_heads=H, qkv_bias=True, attn_drop=0.5)
    with torch.no_grad():
        m.qkv.weight.copy_(rnd(192, 64, seed=81, scale=0.3))
        m.qkv.bias.copy_(rnd(192, seed=82, scale=0.5))
        m.proj.weight.copy_(rnd(64, 64, seed=85, scale=0.3))
        m.proj.bias.copy_(rnd(64, seed=89, scale=0.5))
    m.set_pos_encoding(pe)
    m = m.cuda()
    x, dy, w = rnd(B, N, 64, seed=84), rnd(B, N, 64, seed=94), rnd(B, N, seed=88)
    qkv = torch.nn.functional.linear(x, m.qkv.weight.detach().cpu(), m.qkv.bias.detach().cpu())
    dout = dy.double() @ m.proj.weight.detach().cpu().double()                      # dO = dy W_proj: the bias plays no part
    p = ref_probs(qkv.double(), H, "relative", {"table": pe.relative_position_bias_table.detach().cpu()})
    g = ref_grad_attn(qkv, dout, H)
    xd, dyd, wd = x.cuda(), dy.cuda(), w.cuda()
    c = report.case("attention_module", "relative-N26")
    for clamp in CLAMPS:
        m.train()
        state = torch.cuda.get_rng_state()
        r_train = m.attention_relevance(xd, dyd, weights=wd, clamp=clamp)
        assert torch.equal(torch.cuda.get_rng_state(), state), "attention_relevance consumed CUDA RNG"
        assert m.training and m.last_rng is None
        m.eval()
        r_eval = m.attention_relevance(xd, dyd, weights=wd, clamp=clamp)
        assert torch.equal(r_train, r_eval) and not r_eval.requires_grad
        assert tuple(r_eval.shape) == (B, H, N) and r_eval.dtype == torch.float32
        gate(c, r_eval, ref_relevance(p, g, w, clamp), tol("f32"), suffix="" if clamp else "_signed")
    e_cls = torch.zeros(B, N)
    e_cls[:, 0] = 1.0
    gate(c, m.attention_relevance(xd, dyd), ref_relevance(p, g, e_cls, True), tol("f32"), suffix="_default_weights")
    assert all(prm.grad is None for prm in m.parameters())
    # Block.attention_relevance: the same on norm1(x)
    blk = Block(64, H, qkv_bias=True, attn_drop=0.5).cuda().train()
    with torch.no_grad():
        n1 = torch.nn.functional.layer_norm(xd, (64,), blk.norm1.weight, blk.norm1.bias, blk.norm1.eps)
    rb = blk.attention_relevance(xd, dyd, weights=wd)
    ra = blk.attn.attention_relevance(n1, dyd, weights=wd)
    c.lt("block_vs_attention", float((rb - ra).abs().max() / ra.abs().max()), tol("f32"))
    c.done()
    assert blk.training


# ------------------------------------------------------------------------------------------ 8. refusals
def test_unsupported_shapes_and_arguments_are_errors(K):
    from vitpe._lib import VitpeError
    from vitpe.kernels import PETables

    def z(*shape, dtype=torch.float32):
        return torch.zeros(*shape, device="cuda", dtype=dtype)
    with pytest.raises(VitpeError):   # 101 tokens (7 tiles): not in the compiled set
        K.attention_core_relevance(z(1, 101, 3 * 64), z(1, 101, 64), 2, PETables("none", 10), z(1, 101))
    with pytest.raises(VitpeError):   # head dimension 40 has no instantiation
        K.attention_core_relevance(z(1, 17, 3 * 80), z(1, 17, 80), 2, PETables("none", 4), z(1, 17))
    with pytest.raises(VitpeError):   # no weights
        K.attention_core_relevance(z(2, 17, 3 * 64), z(2, 17, 64), 2, PETables("none", 4), None)
    with pytest.raises(VitpeError):   # weights of the wrong shape
        K.attention_core_relevance(z(2, 17, 3 * 64), z(2, 17, 64), 2, PETables("none", 4), z(2, 16))
    with pytest.raises(VitpeError):   # weights of the wrong dtype
        K.attention_core_relevance(z(2, 17, 3 * 64), z(2, 17, 64), 2, PETables("none", 4), z(2, 17, dtype=torch.bfloat16))
    with pytest.raises(VitpeError):   # dout of the wrong shape
        K.attention_core_relevance(z(2, 17, 3 * 64), z(2, 17, 3 * 64), 2, PETables("none", 4), z(2, 17))
    with pytest.raises(VitpeError):   # dout of the wrong dtype
        K.attention_core_relevance(z(2, 17, 3 * 64), z(2, 17, 64, dtype=torch.bfloat16), 2, PETables("none", 4), z(2, 17))
    # a refused geometry leaves the output as it was: fp32, hd 128 at 10 tiles (K~ and V do not fit the LDS together)
    out = torch.full((1, 1, 146), 7.0, device="cuda")
    with pytest.raises(VitpeError):
        K.attention_core_relevance(z(1, 146, 3 * 128), z(1, 146, 128), 1, PETables("none", 12), z(1, 146), out=out)
    assert bool((out == 7.0).all())
