"""Attention probabilities on the GPU: vitpe_attention_core_probs through kernels.attention_core_probs, the op, Attention /
Block.attention_probs and VisionTransformer.attention_maps, against ref_probs (test_attn_probs_cpu.py: ref_attention up to
the softmax, pinned there to the oracle).

Operands are rounded as the kernel's are (ref_fwd_bwd's convention): x and W to the compute type, the projection rounded to
bf16 in bf16 mode; the device buffer holds exactly the values the reference sees.  The gate is the suite's tol(dt) under
rel_err = max|a - b| / max|b|.  B = 2, H = 2 throughout."""
import functools

import pytest
import torch

from attn_tokens import DT, Guarded, edge_rows, guarded_input, masked_case, q, rel_err, tol, token_case
from test_attn_probs_cpu import probs_times_v, ref_probs
from test_kernels_gpu import ATTN_MODES, K, dev, device_pe, rnd  # noqa: F401  (K: the kernels fixture)

pytestmark = pytest.mark.gpu

B, H = 2, 2


@functools.lru_cache(maxsize=None)
def case(mode, N, hd, dt, masked=False):
    """(G, qkv [B, N, 3D] fp32 on the CPU holding the values the kernel reads, pe leaves, ref_probs of them) -- built once"""
    mk = masked_case if masked else token_case
    N, hd, G, xn, wqkv, _, pe = mk(mode, N, H * hd, H, B, seed=70)
    qkv = torch.nn.functional.linear(q(xn, dt), q(wqkv, dt))
    if dt == "bf16":
        qkv = qkv.bfloat16().float()
    return G, qkv, pe, ref_probs(qkv, H, mode, pe)


def run(K, mode, N, hd, dt, masked=False, **kw):
    G, qkv, pe, ref = case(mode, N, hd, dt, masked)
    return K.attention_core_probs(dev(qkv, DT[dt]), H, device_pe(K, mode, pe, H, G), **kw), ref


# ------------------------------------------------------------------------------------------ 1. parity
# N = 26: two tiles, odd row stride (4-byte stores); N = 65: five tiles; hd 24 on the padded tiles at N = 17 (one
# 16-byte-unaligned tile pair) and N = 50 (four tiles, row stride a multiple of 2 only); N = 197, hd 64: 13 tiles
PARITY = [(m, n, hd) for n, hd in ((26, 32), (26, 64), (65, 32), (65, 64), (17, 24), (50, 24)) for m in ATTN_MODES]
PARITY += [("rope-axial", 197, 64)]


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("mode,N,hd", PARITY)
def test_probs_match_the_reference(K, mode, N, hd, dt):
    p, ref = run(K, mode, N, hd, dt)
    assert p.dtype == torch.float32 and tuple(p.shape) == (B, H, N, N) and not p.requires_grad
    err = rel_err(p.cpu(), ref)
    print(f"{mode} N={N} hd={hd} {dt}: rel_err {err:.3e}")
    assert err < tol(dt)


# ------------------------------------------------------------------------------------------ 2. every token count's edge
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("mode", ["none", "relative"])
@pytest.mark.parametrize("N", [18, 31, 32, 49, 64, 66, 80])   # 32, 64, 80: 16-byte stores; the others: 4-byte stores
def test_edge_rows_pick_the_reference_key(K, mode, N, dt):
    """masked_case: one wrongly admitted or dropped key, or a table index off by one, is an order-one change of rows 0 and
    N - 1, and an admitted padding key takes every row.  For each edge row the arg-max key and its probability match.
    Two keys whose reference probabilities differ by less than the gate tol(dt) of the row's maximum are not ordered at the
    kernel's precision (bf16 rounds the rotated, scaled q and k to 8 bits: a logit moves by up to ~2^-8 |logit|): there
    either of the two is the arg-max."""
    p, ref = run(K, mode, N, 32, dt, masked=True)
    p = p.cpu()
    for r in edge_rows(N):
        pk, pr = p[:, :, r], ref[:, :, r]                       # [B, H, N]
        jk, jr = pk.argmax(-1), pr.argmax(-1)
        top = pr.max(-1).values
        tie = (top - pr.gather(-1, jk[..., None])[..., 0]) < tol(dt) * top
        assert bool(((jk == jr) | tie).all()), (r, jk.tolist(), jr.tolist())
        err = float(((pk.max(-1).values - top).abs() / top).max())
        assert err < tol(dt), (r, err)
    for r in ((0, N - 1) if mode == "none" else (N - 1,)):      # the constructed rows: one dominant key, no tie clause
        want = N - 1 if mode == "none" else 0
        assert bool((p[:, :, r].argmax(-1) == want).all()) and bool((ref[:, :, r].argmax(-1) == want).all()), r
    if mode == "relative":
        assert bool((p[:, :, 0].argmax(-1) == N - 1).all())


# ------------------------------------------------------------------------------------------ 3. bounds
@pytest.mark.parametrize("cls_only", [False, True])
@pytest.mark.parametrize("mode,N", [("rope-mixed", 26), ("rope-mixed", 65), ("relative", 32)])
def test_nothing_is_written_or_read_out_of_bounds(K, mode, N, cls_only):
    dt = "bf16"
    G, qkv, pe, ref = case(mode, N, 32, dt)
    out = Guarded((B, H, N) if cls_only else (B, H, N, N), torch.float32)
    K.attention_core_probs(guarded_input(dev(qkv, DT[dt])), H, device_pe(K, mode, pe, H, G), cls_only=cls_only, out=out.t)
    torch.cuda.synchronize()
    p = out.check(f"{mode} N={N} cls_only={cls_only}").cpu()
    assert rel_err(p, ref[:, :, 0] if cls_only else ref) < tol(dt)


# ------------------------------------------------------------------------------------------ 4. rows are distributions
@pytest.mark.parametrize("mode", ["none", "relative", "rope-mixed"])
def test_rows_are_distributions(K, mode):
    """fp32, N = 65.  A stored entry is p_j * (1 / l), l the fp32 sum of the p_j: one v_rcp_f32 (1 ulp) and one rounding of
    the product per entry, N roundings in the running sum of l -- the row sum is off 1 by at most (N + 2) 2^-24 = 4.0e-6 at
    N = 65.  Gate: 1e-5.  (The sum here is taken in fp64 and adds nothing.)"""
    N = 65
    p, _ = run(K, mode, N, 32, "f32")
    assert (N + 2) * 2.0 ** -24 < 1e-5
    assert bool((p >= 0).all())
    dev_ = float((p.double().sum(-1) - 1.0).abs().max())
    print(f"{mode}: max |row sum - 1| = {dev_:.3e}")
    assert dev_ < 1e-5


# ------------------------------------------------------------------------------------------ 5. the forward that ships
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("mode,N,hd", [("rope-axial", 65, 32), ("relative", 65, 32), ("rope-axial", 197, 64),
                                       ("relative", 197, 64)])
def test_probs_times_v_is_the_core_forward(K, mode, N, hd, dt):
    G, qkv, pe, _ = case(mode, N, hd, dt)
    t = device_pe(K, mode, pe, H, G)
    qd = dev(qkv, DT[dt])
    out = K.attention_core_fwd(qd, H, t)
    pv = probs_times_v(K.attention_core_probs(qd, H, t), qd.float(), H)
    assert rel_err(pv.cpu(), out.float().cpu()) < tol(dt)


# ------------------------------------------------------------------------------------------ 6. cls_only
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("mode", ATTN_MODES)
def test_cls_only_is_row_zero_bit_for_bit(K, mode, dt):
    full, _ = run(K, mode, 26, 32, dt)
    row, _ = run(K, mode, 26, 32, dt, cls_only=True)
    assert tuple(row.shape) == (B, H, 26)
    assert torch.equal(row, full[:, :, 0, :])


# ------------------------------------------------------------------------------------------ 7. modules
def _attention(pe_module=None):
    from vitpe.vit import Attention
    torch.manual_seed(5)
    m = Attention(64, num_heads=H, qkv_bias=True, attn_drop=0.5)
    with torch.no_grad():
        m.qkv.weight.copy_(rnd(192, 64, seed=81, scale=0.3))
        m.qkv.bias.copy_(rnd(192, seed=82, scale=0.5))
    if pe_module is not None:
        m.set_pos_encoding(pe_module)
    return m.cuda()


def test_attention_module_probs_ignore_dropout_and_mode(K):
    from vitpe.positional_encoding import RelativePositionalEncoding
    N = 26
    pe = RelativePositionalEncoding(N - 1, H)
    with torch.no_grad():
        pe.relative_position_bias_table.copy_(rnd(H, 2 * N - 1, seed=83, scale=0.5))
    m = _attention(pe)
    x = rnd(B, N, 64, seed=84)
    qkv = torch.nn.functional.linear(x, m.qkv.weight.detach().cpu(), m.qkv.bias.detach().cpu())
    ref = ref_probs(qkv, H, "relative", {"table": pe.relative_position_bias_table.detach().cpu()})
    xd = x.cuda()
    m.train()
    state = torch.cuda.get_rng_state()
    p_train = m.attention_probs(xd)
    assert torch.equal(torch.cuda.get_rng_state(), state), "attention_probs consumed CUDA RNG"
    assert m.training and m.last_rng is None
    m.eval()
    p_eval = m.attention_probs(xd)
    assert torch.equal(p_train, p_eval)
    assert tuple(p_eval.shape) == (B, H, N, N) and not p_eval.requires_grad
    assert rel_err(p_eval.cpu(), ref) < tol("f32")
    assert torch.equal(m.attention_probs(xd, cls_only=True), p_eval[:, :, 0])


def test_attention_module_probs_with_caller_tables(K):
    from oracle import vit_oracle as O
    from vitpe.positional_encoding import RoPEAxial
    N, hd = 26, 32
    m = _attention(RoPEAxial(hd, 10.0)).train()   # (a rotary module, the only kind that reads caller tables, vit.py:51; not its own theta)
    x = rnd(B, N, 64, seed=85)
    inv_freq = O.rope_axial_inv_freq(hd, 100.0)
    cos, sin = O.rope_axial_tables(N - 1, inv_freq)
    qkv = torch.nn.functional.linear(x, m.qkv.weight.detach().cpu(), m.qkv.bias.detach().cpu())
    ref = ref_probs(qkv, H, "rope-axial", {"inv_freq": inv_freq})
    p = m.attention_probs(x.cuda(), freqs_cis=(cos.cuda(), sin.cuda()))
    assert rel_err(p.cpu(), ref) < tol("f32")
    # without tables the module does not rotate (reference vit.py:51): a different result
    assert rel_err(m.attention_probs(x.cuda()).cpu(), ref) > 10 * tol("f32")


# ------------------------------------------------------------------------------------------ 8. model
@pytest.mark.parametrize("mode", ["rope-mixed", "relative"])
def test_model_attention_maps(K, mode):
    from vitpe.vit import VisionTransformer
    torch.manual_seed(7)
    model = VisionTransformer(img_size=16, patch_size=4, embed_dim=64, depth=2, num_heads=H, pos_encoding=mode).cuda()
    N = 17
    if mode == "relative":
        with torch.no_grad():
            model.pos_embed.relative_position_bias_table.copy_(rnd(H, 2 * N - 1, seed=86, scale=0.5))
    x = rnd(B, 3, 16, 16, seed=87).cuda()
    seen = []
    hook = model.blocks[0].register_forward_hook(lambda mod, args, out: seen.append(out.detach().float().cpu()))
    model.eval()
    with torch.no_grad():
        before = model(x)
    hook.remove()
    model.train()
    state = torch.cuda.get_rng_state()
    maps = model.attention_maps(x)
    assert torch.equal(torch.cuda.get_rng_state(), state)
    assert model.training and all(mod.training for mod in model.modules())
    assert sorted(maps) == [0, 1] and all(tuple(v.shape) == (B, H, N, N) and not v.requires_grad for v in maps.values())
    blk = model.blocks[1]
    n1 = torch.nn.functional.layer_norm(seen[0], (64,), blk.norm1.weight.detach().cpu(), blk.norm1.bias.detach().cpu(),
                                        blk.norm1.eps)
    qkv = torch.nn.functional.linear(n1, blk.attn.qkv.weight.detach().cpu())
    leaves = {"freqs": model.pos_embed.freqs.detach().cpu()} if mode == "rope-mixed" else \
        {"table": model.pos_embed.relative_position_bias_table.detach().cpu()}
    assert rel_err(maps[1].cpu(), ref_probs(qkv, H, mode, leaves)) < tol("f32")
    only = model.attention_maps(x, layers=[1], cls_only=True)
    assert sorted(only) == [1] and torch.equal(only[1], maps[1][:, :, 0])
    model.eval()
    with torch.no_grad():
        after = model(x)
    assert torch.equal(before, after)


# ------------------------------------------------------------------------------------------ 9. refusals
def test_unsupported_shapes_are_errors(K):
    from vitpe._lib import VitpeError
    from vitpe.kernels import PETables
    with pytest.raises(VitpeError):   # 101 tokens (7 tiles): not in the compiled set
        K.attention_core_probs(torch.zeros(1, 101, 3 * 64, device="cuda"), 2, PETables("none", 10))
    with pytest.raises(VitpeError):   # head dimension 40 has no instantiation
        K.attention_core_probs(torch.zeros(1, 17, 3 * 80, device="cuda"), 2, PETables("none", 4), cls_only=True)
