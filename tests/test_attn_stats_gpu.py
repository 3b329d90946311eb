"""Attention statistics on the GPU: vitpe_attention_core_stats through kernels.attention_core_stats, Attention / Block
.attention_stats and VisionTransformer.attention_stats / attention_rollout, against the float64 references of
attn_stats_ref.py (pinned to closed forms in test_attn_stats_cpu.py) on ref_probs (test_attn_probs_cpu.py).

Operands are rounded as the probability tests round them: x and W to the compute type, the projection rounded to bf16 in
bf16 mode; the device buffer holds exactly the values the float64 reference sees.  Every slot of stats [B, H, 4] and colsum
are compared separately under the suite's rel_err = max|a - b| / max|b| and tol(dt) (1e-4 / 3e-2).  B = 2, H = 2, unit = 4
throughout.  The measured figures go to profiles/attn_stats_parity.jsonl before anything is asserted."""
import functools
import math

import pytest
import torch

from attn_stats_ref import CLS_ENTROPY, SLOTS, ref_colsum, ref_rollout, ref_stats
from attn_tokens import DT, Guarded, guarded_input, masked_case, q, rel_err, tol, token_case
from parity_report import Report
from test_attn_probs_cpu import ref_probs
from test_kernels_gpu import ATTN_MODES, K, dev, device_pe, rnd  # noqa: F401  (K: the kernels fixture)

pytestmark = pytest.mark.gpu

B, H, UNIT = 2, 2, 4.0


@pytest.fixture(scope="module")
def report():
    r = Report("test_attn_stats_gpu", "attn_stats_parity.jsonl")
    yield r
    r.close()


@functools.lru_cache(maxsize=None)
def case(mode, N, hd, dt, masked=False):
    """(G, qkv [B, N, 3D] fp32 on the CPU holding the values the kernel reads, pe leaves, weights [B, N], and in float64
    ref_stats, ref_colsum and the probabilities themselves) -- built once"""
    mk = masked_case if masked else token_case
    N, hd, G, xn, wqkv, _, pe = mk(mode, N, H * hd, H, B, seed=70)
    qkv = torch.nn.functional.linear(q(xn, dt), q(wqkv, dt))
    if dt == "bf16":
        qkv = qkv.bfloat16().float()
    p = ref_probs(qkv.double(), H, mode, pe)
    w = rnd(B, N, seed=71)
    return G, qkv, pe, w, ref_stats(p, G, UNIT), ref_colsum(p, w), p


def run(K, mode, N, hd, dt, masked=False, weights=True, out=None, guard=False):
    """-> (stats, colsum) on the device for case(...), with its weights or without"""
    G, qkv, pe, w = case(mode, N, hd, dt, masked)[:4]
    qd, wd = dev(qkv, DT[dt]), dev(w) if weights else None
    if guard:
        qd, wd = guarded_input(qd), guarded_input(wd)
    return K.attention_core_stats(qd, H, device_pe(K, mode, pe, H, G), unit=UNIT, weights=wd, out=out)


def slot_errs(stats, ref):
    return {name: rel_err(stats[..., k].cpu(), ref[..., k]) for k, name in enumerate(SLOTS)}


def gate(c, stats, colsum, rs, rc, limit, suffix=""):
    """records every slot's and colsum's rel_err against `limit` in the Case c"""
    for name, e in slot_errs(stats, rs).items():
        c.lt(name + suffix, e, limit)
    if colsum is not None:
        c.lt("colsum" + suffix, rel_err(colsum.cpu(), rc), limit)


# ------------------------------------------------------------------------------------------ 1. parity against float64
# the probability tests' list, and one case each at 10, 13 and 17 tiles (ten, seven and six waves: one, two and three
# rounds of query-tile jobs per wave, i.e. the colsum slab is stored, then added to)
PARITY = [(m, n, hd) for n, hd in ((26, 32), (26, 64), (65, 32), (65, 64), (17, 24), (50, 24)) for m in ATTN_MODES]
PARITY += [("rope-axial", 197, 64), ("relative", 145, 32), ("rope-axial", 257, 32)]


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("mode,N,hd", PARITY)
def test_stats_match_the_float64_reference(K, report, mode, N, hd, dt):
    rs, rc = case(mode, N, hd, dt)[4:6]
    s0, c0 = run(K, mode, N, hd, dt, weights=False)
    s1, c1 = run(K, mode, N, hd, dt)
    assert c0 is None
    assert s0.dtype == torch.float32 and tuple(s0.shape) == (B, H, 4) and not s0.requires_grad
    assert c1.dtype == torch.float32 and tuple(c1.shape) == (B, H, N) and not c1.requires_grad
    c = report.case("parity", f"{mode}-N{N}-hd{hd}-{dt}")
    gate(c, s0, None, rs, rc, tol(dt))
    gate(c, s1, c1, rs, rc, tol(dt))
    print(f"{mode} N={N} hd={hd} {dt}: " + " ".join(f"{k} {v:.2e}" for k, v in c.figures.items()))
    c.done()


# ------------------------------------------------------------------------------------------ 2. geometry on exact inputs
def shift_case(N, delta):
    """qkv = 0 and a relative table that is 30 at the offset of key i + delta (index i - j + N - 1 = N - 1 - delta), 0
    elsewhere: row i is a shifted identity to within N e^-30 where key i + delta exists, uniform where it does not.  No
    operand is rounded in either type.  -> (table, float64 probabilities)"""
    table = torch.zeros(H, 2 * N - 1)
    table[:, N - 1 - delta] = 30.0
    return table, ref_probs(torch.zeros(B, N, 3 * H * 32, dtype=torch.float64), H, "relative", {"table": table})


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("N", [26, 65])   # 26: 4-byte rows, ten padding keys; 65: five tiles
@pytest.mark.parametrize("shift", ["+1", "-1", "+G", "-G", "key0"])
def test_token_to_coordinate_map_on_shifted_identities(K, report, shift, N, dt):
    """A transposed or off-by-one token-to-coordinate map moves the distance of +-1 (one column; sqrt(1 + (G-1)^2) at a row
    end) and +-G (one row) by an order-one factor; near-uniform random attention does not see it.  key0 = offset
    -(N - 1): query N - 1 alone finds its key, the class token.

    Gate 1e-5 relative per slot.  The class row's entropy (slot 3) is compared absolutely against 1e-5 ln N: where the
    class row selects a key (+1, +G) its entropy is about 30 N e^-30 = 1e-10, of which the part ln(1 + N e^-30) is lost when
    the fp32 row sum rounds to 1 -- no fp32 kernel holds that value to 1e-5 of itself; ln N is the entropy's scale, and the
    reference value wherever the class row is uniform."""
    G = math.isqrt(N - 1)
    delta = {"+1": 1, "-1": -1, "+G": G, "-G": -G, "key0": -(N - 1)}[shift]
    table, p = shift_case(N, delta)
    from vitpe.kernels import PETables
    t = PETables("relative", G, table=dev(table))
    stats, _ = K.attention_core_stats(torch.zeros(B, N, 3 * H * 32, device="cuda", dtype=DT[dt]), H, t, unit=UNIT)
    rs = ref_stats(p, G, UNIT)
    c = report.case("geometry", f"{shift}-N{N}-{dt}")
    for name, e in list(slot_errs(stats, rs).items())[:CLS_ENTROPY]:
        c.lt(name, e, 1e-5)
    c.lt("cls_entropy_abs", float((stats[..., CLS_ENTROPY].cpu().double() - rs[..., CLS_ENTROPY]).abs().max()),
         1e-5 * math.log(N))
    c.done()


# ------------------------------------------------------------------------------------------ 3. uniform rows
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("N", [18, 26, 65])   # 18: a ragged raster (G = 4)
def test_uniform_rows_closed_forms(K, report, N, dt):
    """qkv = 0 without bias: every row is uniform over its N keys.  A padding key that reached the entropy's 0 . (-inf)
    would turn it NaN; one that was admitted would make it ln(N + 1)."""
    from vitpe.kernels import PETables
    G, P = math.isqrt(N - 1), N - 1
    stats, colsum = K.attention_core_stats(torch.zeros(B, N, 3 * H * 32, device="cuda", dtype=DT[dt]), H, PETables("none", G),
                                           unit=UNIT, weights=torch.ones(B, N, device="cuda"))
    dsum = sum(math.hypot((i // G) - (j // G), (i % G) - (j % G)) for i in range(P) for j in range(P))
    want = torch.tensor([UNIT * dsum / (P * N), math.log(N), 1.0 / N, math.log(N)], dtype=torch.float64).expand(B, H, 4)
    assert bool(torch.isfinite(stats).all())
    c = report.case("uniform", f"N{N}-{dt}")
    gate(c, stats, colsum, want, torch.ones(B, H, N, dtype=torch.float64), 1e-5)
    c.done()


# ------------------------------------------------------------------------------------------ 4. token-count edges
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("mode", ["none", "relative"])
@pytest.mark.parametrize("N", [18, 31, 32, 49, 64, 66, 80])
def test_token_count_edges(K, report, mode, N, dt):
    """masked_case: a wrongly admitted or dropped key, or a table index off by one, is an order-one change of rows 0 and
    N - 1.  One key dominates the class row there, so its entropy (slot 3) is about 0 in the reference and is compared
    absolutely, against tol(dt) ln N."""
    rs, rc = case(mode, N, 32, dt, True)[4:6]
    stats, colsum = run(K, mode, N, 32, dt, masked=True)
    c = report.case("edges", f"{mode}-N{N}-{dt}")
    for name, e in list(slot_errs(stats, rs).items())[:CLS_ENTROPY]:
        c.lt(name, e, tol(dt))
    c.lt("colsum", rel_err(colsum.cpu(), rc), tol(dt))
    c.lt("cls_entropy_abs", float((stats[..., CLS_ENTROPY].cpu().double() - rs[..., CLS_ENTROPY]).abs().max()),
         tol(dt) * math.log(N))
    c.done()


# ------------------------------------------------------------------------------------------ 5. bounds
@pytest.mark.parametrize("mode,N", [("rope-mixed", 26), ("rope-mixed", 65), ("relative", 32)])
def test_nothing_is_written_or_read_out_of_bounds(K, report, mode, N):
    dt = "bf16"
    rs, rc = case(mode, N, 32, dt)[4:6]
    o_stats, o_col = Guarded((B, H, 4), torch.float32), Guarded((B, H, N), torch.float32)
    run(K, mode, N, 32, dt, out=(o_stats.t, o_col.t), guard=True)
    torch.cuda.synchronize()
    c = report.case("bounds", f"{mode}-N{N}")
    gate(c, o_stats.check(f"stats {mode} N={N}"), o_col.check(f"colsum {mode} N={N}"), rs, rc, tol(dt))
    c.done()


# ------------------------------------------------------------------------------------------ 6. the probabilities kernel
@pytest.mark.parametrize("mode", ["none", "relative", "rope-mixed"])
def test_agrees_with_the_reduced_probabilities_kernel(K, report, mode):
    """fp32, N = 65: the float64 reduction of attention_core_probs' own output.  Both kernels form the same p = e / l; every
    slot and every colsum entry is a sum of at most N^2 non-negative fp32 terms (weights in [0, 1) here), each with a
    few roundings of its own: (N^2 + 8) 2^-24 is the linear worst case of fp32 accumulation, 2.5e-4."""
    N, hd, dt = 65, 32, "f32"
    G, qkv, pe, _ = case(mode, N, hd, dt)[:4]
    bound = (N * N + 8) * 2.0 ** -24
    assert bound < 1e-3
    t, qd = device_pe(K, mode, pe, H, G), dev(qkv, DT[dt])
    w = rnd(B, N, seed=72).abs()
    p = K.attention_core_probs(qd, H, t).cpu()
    stats, colsum = K.attention_core_stats(qd, H, t, unit=UNIT, weights=dev(w))
    c = report.case("vs_probs_kernel", mode)
    gate(c, stats, colsum, ref_stats(p, G, UNIT), ref_colsum(p, w), bound)
    c.done()


# ------------------------------------------------------------------------------------------ 7. reproducibility
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("mode,N,hd", [("none", 26, 32), ("relative", 65, 32), ("rope-axial", 197, 64), ("rope-axial", 257, 32)])
def test_two_launches_give_the_same_bits(K, mode, N, hd, dt):
    s1, c1 = run(K, mode, N, hd, dt)
    s2, c2 = run(K, mode, N, hd, dt)
    s0, _ = run(K, mode, N, hd, dt, weights=False)
    assert torch.equal(s1, s2) and torch.equal(c1, c2)
    assert torch.equal(s0, s1), "the stats depend on whether colsum is written"


# ------------------------------------------------------------------------------------------ 8. modules and model
@pytest.mark.parametrize("mode", ["rope-mixed", "relative"])
def test_model_attention_stats_and_rollout(K, report, mode):
    from vitpe.vit import VisionTransformer
    torch.manual_seed(7)
    model = VisionTransformer(img_size=16, patch_size=4, embed_dim=64, depth=2, num_heads=H, pos_encoding=mode).cuda()
    N, G = 17, 4
    if mode == "relative":
        with torch.no_grad():
            model.pos_embed.relative_position_bias_table.copy_(rnd(H, 2 * N - 1, seed=86, scale=0.5))
    x = rnd(B, 3, 16, 16, seed=87).cuda()
    model.eval()
    with torch.no_grad():
        before = model(x)
    maps = {l: m.cpu() for l, m in model.attention_maps(x).items()}
    model.train()
    state = torch.cuda.get_rng_state()
    stats = model.attention_stats(x)
    roll = model.attention_rollout(x)
    roll1 = model.attention_rollout(x, start_layer=1)
    roll0 = model.attention_rollout(x, residual=0.0)
    assert torch.equal(torch.cuda.get_rng_state(), state), "the analysis methods consumed CUDA RNG"
    assert model.training and all(mod.training for mod in model.modules())
    assert sorted(stats) == [0, 1]
    assert all(tuple(v.shape) == (B, H, 4) and v.dtype == torch.float32 and not v.requires_grad for v in stats.values())
    assert sorted(model.attention_stats(x, layers=[1])) == [1]
    bound = (N * N + 8) * 2.0 ** -24
    c = report.case("model", mode)
    for l in (0, 1):
        gate(c, stats[l], None, ref_stats(maps[l], G, 4.0), None, bound, suffix=f"@{l}")
    both = [maps[0], maps[1]]
    for name, r, ref in (("rollout", roll, ref_rollout(both)), ("rollout_start1", roll1, ref_rollout(both, start=1)),
                         ("rollout_residual0", roll0, ref_rollout(both, residual=0.0))):
        assert tuple(r.shape) == (B, N) and r.dtype == torch.float32 and not r.requires_grad
        c.lt(name, rel_err(r.cpu(), ref), tol("f32"))
        c.lt(name + "_sum", float((r.double().sum(-1) - 1.0).abs().max()), 1e-5)
    c.done()
    with pytest.raises(ValueError):
        model.attention_rollout(x, start_layer=2)
    assert model.training and all(mod.training for mod in model.modules())   # restored on an exception as well
    model.eval()
    with torch.no_grad():
        after = model(x)
    assert torch.equal(before, after)


def test_attention_module_stats_ignore_dropout_and_mode(K, report):
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
    m.set_pos_encoding(pe)
    m = m.cuda()
    x = rnd(B, N, 64, seed=84)
    w = rnd(B, N, seed=88)
    qkv = torch.nn.functional.linear(x, m.qkv.weight.detach().cpu(), m.qkv.bias.detach().cpu())
    p = ref_probs(qkv.double(), H, "relative", {"table": pe.relative_position_bias_table.detach().cpu()})
    xd, wd = x.cuda(), w.cuda()
    m.train()
    state = torch.cuda.get_rng_state()
    s_train, c_train = m.attention_stats(xd, weights=wd, unit=UNIT)
    assert torch.equal(torch.cuda.get_rng_state(), state), "attention_stats consumed CUDA RNG"
    assert m.training and m.last_rng is None
    m.eval()
    s_eval, c_eval = m.attention_stats(xd, weights=wd, unit=UNIT)
    assert torch.equal(s_train, s_eval) and torch.equal(c_train, c_eval)
    assert not s_eval.requires_grad and not c_eval.requires_grad
    assert m.attention_stats(xd)[1] is None
    c = report.case("attention_module", "relative-N26")
    gate(c, s_eval, c_eval, ref_stats(p, 5, UNIT), ref_colsum(p, w), tol("f32"))
    c.done()
    # Block.attention_stats: the same on norm1(x)
    blk = Block(64, H, qkv_bias=True, attn_drop=0.5).cuda().train()
    with torch.no_grad():
        n1 = torch.nn.functional.layer_norm(xd, (64,), blk.norm1.weight, blk.norm1.bias, blk.norm1.eps)
    sb, cb = blk.attention_stats(xd, weights=wd, unit=UNIT)
    sa, ca = blk.attn.attention_stats(n1, weights=wd, unit=UNIT)
    assert rel_err(sb.cpu(), sa.cpu()) < tol("f32") and rel_err(cb.cpu(), ca.cpu()) < tol("f32")
    assert blk.training


# ------------------------------------------------------------------------------------------ 9. refusals
def test_unsupported_shapes_and_arguments_are_errors(K):
    from vitpe._lib import VitpeError
    from vitpe.kernels import PETables

    def z(*shape, dtype=torch.float32):
        return torch.zeros(*shape, device="cuda", dtype=dtype)
    with pytest.raises(VitpeError):   # 101 tokens (7 tiles): not in the compiled set
        K.attention_core_stats(z(1, 101, 3 * 64), 2, PETables("none", 10))
    with pytest.raises(VitpeError):   # head dimension 40 has no instantiation
        K.attention_core_stats(z(1, 17, 3 * 80), 2, PETables("none", 4))
    with pytest.raises(VitpeError):   # weights of the wrong shape
        K.attention_core_stats(z(2, 17, 3 * 64), 2, PETables("none", 4), weights=z(2, 16))
    with pytest.raises(VitpeError):   # weights of the wrong dtype
        K.attention_core_stats(z(2, 17, 3 * 64), 2, PETables("none", 4), weights=z(2, 17, dtype=torch.bfloat16))
    with pytest.raises(VitpeError):   # colsum without weights
        K.attention_core_stats(z(2, 17, 3 * 64), 2, PETables("none", 4), out=(z(2, 2, 4), z(2, 2, 17)))
