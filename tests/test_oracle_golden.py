"""Pin the CPU oracle to vectors produced by the reference itself
(tools/make_golden.py imported /root/reference in the build container).

Integer tables: bit-exact.  Floating point: the oracle restates the same fp32
op sequence, tolerance 2e-6 relative (summation-order noise only).
"""
import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import vit_oracle as O

FTOL = 2e-6
MODES = [("none", {}), ("absolute", {}), ("relative", {}), ("polynomial", {}),
         ("polynomial_perhead", {"pos_encoding": "polynomial", "poly_shared_heads": False}),
         ("rope-axial", {}), ("rope-mixed", {})]


def cfg_for(tag, extra, **geom):
    kw = dict(pos_encoding=extra.get("pos_encoding", tag))
    kw.update({k: v for k, v in extra.items() if k != "pos_encoding"})
    kw.update(geom)
    return O.VitConfig(**kw)


def test_relative_index_bit_exact(golden):
    g = golden("tables")
    for N in (65, 197):
        idx = O.relative_position_index(N)
        assert idx.dtype == np.int64
        assert np.array_equal(idx, g[f"rel_index_{N}"])
    assert O.relative_position_index(65).min() == 0 and O.relative_position_index(65).max() == 128


def test_l1_matrix_bit_exact(golden):
    g = golden("tables")
    for grid in (8, 14):
        l1 = O.l1_distance_matrix(grid)
        assert l1.dtype == np.int64
        assert np.array_equal(l1, g[f"l1_{grid}"])
    assert O.l1_distance_matrix(8).max() == 14


def test_rope_axial_tables(golden):
    g = golden("tables")
    for hd, P in ((32, 64), (64, 196)):
        inv = O.rope_axial_inv_freq(hd, 100.0)
        assert np.array_equal(inv.numpy(), g[f"axial_inv_freq_hd{hd}"])
        cos, sin = O.rope_axial_tables(P, inv)
        assert np.array_equal(cos.numpy(), g[f"axial_cos_hd{hd}_P{P}"])
        assert np.array_equal(sin.numpy(), g[f"axial_sin_hd{hd}_P{P}"])


def test_rope_mixed_tables_scramble(golden):
    g = golden("tables")
    for H, hd, P in ((6, 32, 64), (3, 32, 64), (12, 64, 196)):
        freqs = O.closed_form_tensor("pos_embed.freqs", (2, H, hd // 2))
        cos, sin = O.rope_mixed_tables(P, freqs)
        assert rel_err(cos.numpy(), g[f"mixed_cos_H{H}_hd{hd}_P{P}"]) < FTOL
        assert rel_err(sin.numpy(), g[f"mixed_sin_H{H}_hd{hd}_P{P}"]) < FTOL
    # the reference's output is a non-contiguous view with strides (hd/2, H*hd/2, 1)
    assert list(g["mixed_stride_H6_hd32_P64"]) == [16, 96, 1]
    # the scramble really is a scramble: a clean per-head phase would differ
    freqs = O.closed_form_tensor("pos_embed.freqs", (2, 6, 16))
    t_x, t_y = O._t_xy(8)
    clean = torch.cos(t_x[None, :, None] * freqs[0][:, None, :] + t_y[None, :, None] * freqs[1][:, None, :])
    assert rel_err(clean.numpy(), g["mixed_cos_H6_hd32_P64"]) > 1e-2


def test_rope_mixed_init(golden):
    g = golden("tables")
    f = O.rope_mixed_init_freqs(32, 6, 100.0, torch.from_numpy(g["mixed_init_angles"]))
    assert rel_err(f.numpy(), g["mixed_init_freqs"]) < FTOL


def test_bias_tables(golden):
    g = golden("tables")
    tab = O.closed_form_tensor("pos_embed.relative_position_bias_table", (6, 129))
    assert np.array_equal(O.relative_bias(tab, 65).numpy(), g["rel_bias_H6_N65"])
    c = O.closed_form_tensor("pos_embed.coefficients", (4,))
    assert rel_err(O.polynomial_bias(c, 64, 6, 3, True).numpy(), g["poly_bias_H6_N65_shared"]) < FTOL
    c = O.closed_form_tensor("pos_embed.coefficients", (6, 4))
    assert rel_err(O.polynomial_bias(c, 64, 6, 3, False).numpy(), g["poly_bias_H6_N65_perhead"]) < FTOL


def test_apply_rotary(golden):
    g = golden("rotary")
    q = O.closed_form_tensor("rotary.q", (2, 6, 64, 32)) * 20
    k = O.closed_form_tensor("rotary.k", (2, 6, 64, 32)) * 20
    cos, sin = O.rope_axial_tables(64, O.rope_axial_inv_freq(32, 100.0))
    qr, kr = O.apply_rotary_emb(q, k, O.reshape_for_broadcast(cos, q), O.reshape_for_broadcast(sin, q))
    assert np.array_equal(qr.numpy(), g["axial_q"]) and np.array_equal(kr.numpy(), g["axial_k"])
    cos, sin = O.rope_mixed_tables(64, O.closed_form_tensor("pos_embed.freqs", (2, 6, 16)))
    qr, kr = O.apply_rotary_emb(q, k, O.reshape_for_broadcast(cos, q), O.reshape_for_broadcast(sin, q))
    assert rel_err(qr.numpy(), g["mixed_q"]) < FTOL and rel_err(kr.numpy(), g["mixed_k"]) < FTOL
    assert int(g["bad_shape_raises"]) == 1
    with pytest.raises(ValueError):
        O.reshape_for_broadcast(torch.zeros(4), q)


ATTN_TAGS = ["none", "relative", "polynomial", "polynomial_perhead", "rope-axial", "rope-mixed"]


def oracle_attention_case(tag):
    """Re-run the fixture's Attention case on the oracle (dim 96, H 3, B 2, N 65)."""
    D, H, B, N = 96, 3, 2, 65
    hd = D // H
    wqkv = O.closed_form_tensor("attn.qkv.weight", (3 * D, D)).requires_grad_(True)
    wproj = O.closed_form_tensor("attn.proj.weight", (D, D)).requires_grad_(True)
    bproj = O.closed_form_tensor("attn.proj.bias", (D,)).requires_grad_(True)
    x = (O.closed_form_tensor("attn.x", (B, N, D)) * 20).requires_grad_(True)
    dy = O.closed_form_tensor("attn.dy", (B, N, D)) * 20
    pe = {}
    freqs_cis = bias = None
    if tag == "relative":
        pe["relative_position_bias_table"] = O.closed_form_tensor(
            "pos_embed.relative_position_bias_table", (H, 2 * N - 1)).requires_grad_(True)
        bias = O.relative_bias(pe["relative_position_bias_table"], N)
    elif tag.startswith("polynomial"):
        shared = tag == "polynomial"
        pe["coefficients"] = O.closed_form_tensor(
            "pos_embed.coefficients", (4,) if shared else (H, 4)).requires_grad_(True)
        bias = O.polynomial_bias(pe["coefficients"], N - 1, H, 3, shared)
    elif tag == "rope-axial":
        freqs_cis = O.rope_axial_tables(N - 1, O.rope_axial_inv_freq(hd, 100.0))
    elif tag == "rope-mixed":
        pe["freqs"] = O.closed_form_tensor("pos_embed.freqs", (2, H, hd // 2)).requires_grad_(True)
        freqs_cis = O.rope_mixed_tables(N - 1, pe["freqs"])
    a = O.fused_attention(x, wqkv, H, freqs_cis, bias)
    y = torch.nn.functional.linear(a, wproj, bproj)
    y.backward(dy)
    res = {"y": y, "dx": x.grad, "dwqkv": wqkv.grad, "dwproj": wproj.grad, "dbproj": bproj.grad}
    for k, v in pe.items():
        res["dpe." + k] = v.grad
    return {k: v.detach().numpy() for k, v in res.items()}


@pytest.mark.parametrize("tag", ATTN_TAGS)
def test_attention_module(golden, tag):
    g = golden("attention")
    res = oracle_attention_case(tag)
    keys = [k.split("/", 1)[1] for k in g.files if k.startswith(tag + "/")]
    assert sorted(keys) == sorted(res.keys())
    for k in keys:
        assert rel_err(res[k], g[f"{tag}/{k}"]) < 5e-6, k


@pytest.mark.parametrize("tag", ["none_tables", "relative_tables", "polynomial_tables", "rope-axial_none"])
def test_attention_module_ignores_what_its_encoding_does_not_use(golden, tag):
    """golden/attention_tables.npz: the reference's Attention handed constant (cos, sin) tables under pos_encoding None,
    relative and polynomial -- nothing is rotated, the bias is still added (vit.py:51, 73-81) -- and RoPEAxial handed
    freqs_cis=None -- plain attention.  The oracle under that rule reproduces y; rotating with the tables does not."""
    g = golden("attention_tables")
    D, H, B, N = 64, 2, 2, 17
    CF = O.closed_form_tensor
    wqkv, wproj, bproj = CF("attn.qkv.weight", (3 * D, D)), CF("attn.proj.weight", (D, D)), CF("attn.proj.bias", (D,))
    x = CF("attn.x", (B, N, D)) * 20
    bias = None
    if tag == "relative_tables":
        bias = O.relative_bias(CF("pos_embed.relative_position_bias_table", (H, 2 * N - 1)), N)
    elif tag == "polynomial_tables":
        bias = O.polynomial_bias(CF("pos_embed.coefficients", (4,)), N - 1, H, 3, True)
    y = torch.nn.functional.linear(O.fused_attention(x, wqkv, H, None, bias), wproj, bproj)
    assert rel_err(y.numpy(), g[f"{tag}/y"]) < FTOL
    tabs = (torch.from_numpy(g["cos"]), torch.from_numpy(g["sin"]))
    rotated = torch.nn.functional.linear(O.fused_attention(x, wqkv, H, tabs, bias), wproj, bproj)
    assert rel_err(rotated.numpy(), g[f"{tag}/y"]) > 1e3 * FTOL


@pytest.mark.parametrize("tag,extra", MODES)
def test_small_model_logits_loss_grads(golden, tag, extra):
    g = golden("model")
    cfg = cfg_for(tag, extra, embed_dim=96, depth=2, num_heads=3)
    params = O.closed_form_params(cfg)
    images, labels = O.closed_form_batch(cfg, 4)
    logits, loss, grads = O.loss_and_grads(cfg, params, images, labels)
    assert rel_err(logits.numpy(), g[f"small/{tag}/logits"]) < 5e-6
    assert abs(float(loss) - float(g[f"small/{tag}/loss"])) < 5e-6
    n_learn = sum(int(np.prod(s)) for s in O.param_shapes(cfg).values())
    assert n_learn == int(g[f"small/{tag}/n_params"])
    for key in [k for k in g.files if k.startswith(f"small/{tag}/grad/")]:
        name = key.split("/grad/")[1]
        ref = g[key]
        mine = grads[name].numpy()
        if name == "pos_embed.pos_embed":
            assert float(np.abs(mine[:, cfg.num_patches:]).max()) == 0.0
            mine = mine[:, :ref.shape[1]]
        assert rel_err(mine, ref) < 1e-4, name  # fp32 reduction-order noise; north-star gate


@pytest.mark.parametrize("tag,extra", MODES)
def test_small_model_adamw_trajectory(golden, tag, extra):
    g = golden("model")
    cfg = cfg_for(tag, extra, embed_dim=96, depth=2, num_heads=3)
    params = O.closed_form_params(cfg)
    images, labels = O.closed_form_batch(cfg, 4)
    st = O.AdamWState()
    losses = [float(O.train_step(cfg, params, st, images, labels)[1]) for _ in range(5)]
    ref = g[f"small/{tag}/adamw_losses"]
    # Steps 1-2 are tight.  From step 3 on Adam's m/sqrt(v) turns gradients whose
    # magnitude is fp32 noise (~1e-11, e.g. 7-10 % of qkv.weight) into +-lr
    # updates whose SIGN is noise, so any two fp32 implementations (the oracle's
    # adamw_update agrees with torch.optim.AdamW to 1e-7) drift apart chaotically.
    assert np.allclose(losses[:2], ref[:2], rtol=1e-5, atol=2e-6)
    assert np.allclose(losses, ref, rtol=1e-2)
    assert rel_err(params["head.bias"].numpy(), g[f"small/{tag}/adamw_final_head_bias"]) < 2e-2


@pytest.mark.parametrize("tag,extra", MODES)
def test_full_model_logits(golden, tag, extra):
    g = golden("model")
    cfg = cfg_for(tag, extra)
    params = O.closed_form_params(cfg)
    images, labels = O.closed_form_batch(cfg, 4)
    with torch.no_grad():
        logits = O.forward(cfg, params, images)
        feats = O.forward_features(cfg, params, images)
    assert rel_err(logits.numpy(), g[f"full/{tag}/logits"]) < 1e-5
    assert rel_err(feats[:, 0].numpy(), g[f"full/{tag}/features_cls"]) < 1e-5
    assert abs(float(O.loss_fn(logits, labels)) - float(g[f"full/{tag}/loss"])) < 1e-5
    assert sum(int(np.prod(s)) for s in O.param_shapes(cfg).values()) == int(g[f"full/{tag}/n_params"])


def test_mnist_and_imnet_shapes(golden):
    g = golden("model")
    cfg = O.VitConfig(in_chans=1, pos_encoding="none")
    params = O.closed_form_params(cfg)
    images, labels = O.closed_form_batch(cfg, 4)
    logits, loss, grads = O.loss_and_grads(cfg, params, images, labels)
    assert rel_err(logits.numpy(), g["mnist/none/logits"]) < 1e-5
    assert rel_err(grads["patch_embed.weight"].numpy(), g["mnist/none/grad/patch_embed.weight"]) < 5e-5
    cfg = O.VitConfig(img_size=224, patch_size=16, embed_dim=768, depth=1, num_heads=12,
                      pos_encoding="rope-axial")
    params = O.closed_form_params(cfg)
    images, labels = O.closed_form_batch(cfg, 2)
    with torch.no_grad():
        logits = O.forward(cfg, params, images)
    assert rel_err(logits.numpy(), g["imnet1/rope-axial/logits"]) < 2e-5


def test_bad_mode_message(golden):
    msg = str(golden("model")["bad_mode_message"])
    with pytest.raises(ValueError) as e:
        O.VitConfig(pos_encoding="bogus")
    assert str(e.value) == msg == "Unknown positional encoding type: bogus"
