#!/usr/bin/env python3
"""Generate tests/golden/*.npz by importing the reference in the BUILD container.

Runs only where /root/reference exists (never on the GPU box).  The reference
source is imported from where it lies; nothing of it is copied.  Only data
(inputs are closed-form, so mostly *outputs*) is written to tests/golden/.

timm is absent from this image: models/vit.py:9-10 imports
`timm.models.vision_transformer.{PatchEmbed, Mlp}` and
`timm.models.layers.DropPath`.  Only `Mlp` is exercised (vit.py:118).  A local
stand-in restating timm's published Mlp (fc1 -> act -> fc2, biases on) is put
in sys.modules so the reference's own Attention / Block / VisionTransformer
code runs unmodified.  Consequently everything except the Mlp arithmetic is
pinned by the reference itself; the Mlp boundary is "parity unpinned".

Usage:  python tools/make_golden.py            (writes tests/golden/)
        python tools/make_golden.py --only resize     (resize.npz alone, from PIL; also heads, rotary_grad, dropout,
                                                       attention_tables)
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
OUT = os.path.join(REPO, "tests", "golden")
sys.path.insert(0, REPO)

from oracle import vit_oracle as O  # noqa: E402  (closed-form fills only)


def _install_timm_standin():
    class Mlp(nn.Module):
        def __init__(self, in_features, hidden_features=None, out_features=None,
                     act_layer=nn.GELU, drop=0.0):
            super().__init__()
            out_features = out_features or in_features
            hidden_features = hidden_features or in_features
            self.fc1 = nn.Linear(in_features, hidden_features)
            self.act = act_layer()
            self.fc2 = nn.Linear(hidden_features, out_features)

        def forward(self, x):
            return self.fc2(self.act(self.fc1(x)))

    class _Unused(nn.Module):
        def __init__(self, *a, **k):
            raise RuntimeError("stand-in: not exercised by the reference path")

    timm = types.ModuleType("timm")
    tm = types.ModuleType("timm.models")
    tv = types.ModuleType("timm.models.vision_transformer")
    tl = types.ModuleType("timm.models.layers")
    tv.Mlp, tv.PatchEmbed, tl.DropPath = Mlp, _Unused, _Unused
    timm.models, tm.vision_transformer, tm.layers = tm, tv, tl
    sys.modules.update({"timm": timm, "timm.models": tm,
                        "timm.models.vision_transformer": tv, "timm.models.layers": tl})


def load_reference():
    """Import /root/reference/models as package `refmodels` (avoids clashing
    with this repo's own drop-in `models` package)."""
    _install_timm_standin()
    pkg = types.ModuleType("refmodels")
    pkg.__path__ = [os.path.join(REF, "models")]
    sys.modules["refmodels"] = pkg
    mods = {}
    for name in ("positional_encoding", "rope_utils", "vit"):
        spec = importlib.util.spec_from_file_location(
            f"refmodels.{name}", os.path.join(REF, "models", f"{name}.py"))
        m = importlib.util.module_from_spec(spec)
        sys.modules[f"refmodels.{name}"] = m
        spec.loader.exec_module(m)
        mods[name] = m
    return mods


def fill_closed_form(model, cfg):
    with torch.no_grad():
        for name, p in model.named_parameters():
            p.copy_(O.closed_form_tensor(name, tuple(p.shape), cfg))


def np_(t):
    return t.detach().cpu().numpy()


MODES = [
    ("none", {}),
    ("absolute", {}),
    ("relative", {}),
    ("polynomial", {}),
    ("polynomial_perhead", {"pos_encoding": "polynomial", "poly_shared_heads": False}),
    ("rope-axial", {}),
    ("rope-mixed", {}),
]


def mode_cfg(tag, extra, **geom):
    kw = dict(pos_encoding=extra.get("pos_encoding", tag))
    kw.update({k: v for k, v in extra.items() if k != "pos_encoding"})
    kw.update(geom)
    return O.VitConfig(**kw)


def build_ref_model(ref, cfg):
    m = ref["vit"].VisionTransformer(
        img_size=cfg.img_size, patch_size=cfg.patch_size, in_chans=cfg.in_chans,
        num_classes=cfg.num_classes, embed_dim=cfg.embed_dim, depth=cfg.depth,
        num_heads=cfg.num_heads, mlp_ratio=cfg.mlp_ratio, pos_encoding=cfg.pos_encoding,
        rope_theta=cfg.rope_theta, poly_degree=cfg.poly_degree,
        poly_shared_heads=cfg.poly_shared_heads)
    names = [n for n, _ in m.named_parameters()]
    assert names == list(O.param_shapes(cfg).keys()), (names, list(O.param_shapes(cfg).keys()))
    fill_closed_form(m, cfg)
    return m


def gen_tables(ref):
    pe = ref["positional_encoding"]
    out = {}
    for N in (65, 197):
        r = pe.RelativePositionalEncoding(N - 1, num_heads=2)
        out[f"rel_index_{N}"] = np_(r.relative_position_index).astype(np.int64)
    for g in (8, 14):
        # degree-1 polynomial with coefficients [0,1] exposes the L1 matrix itself
        p = pe.PolynomialRPE(g * g, degree=1, num_heads=1, shared_across_heads=True)
        with torch.no_grad():
            p.coefficients.copy_(torch.tensor([0.0, 1.0]))
        b = p.get_bias()[0, 1:, 1:]
        out[f"l1_{g}"] = np_(b).round().astype(np.int64)
        assert np.array_equal(out[f"l1_{g}"].astype(np.float32), np_(b))
    for hd, P in ((32, 64), (64, 196)):
        a = pe.RoPEAxial(dim=hd, theta=100.0)
        cos, sin = a.get_freqs_cis(P, torch.device("cpu"))
        out[f"axial_inv_freq_hd{hd}"] = np_(a.inv_freq)
        out[f"axial_cos_hd{hd}_P{P}"] = np_(cos)
        out[f"axial_sin_hd{hd}_P{P}"] = np_(sin)
    for H, hd, P in ((6, 32, 64), (3, 32, 64), (12, 64, 196)):
        mx = pe.RoPEMixed(dim=hd, num_heads=H, theta=100.0)
        with torch.no_grad():
            mx.freqs.copy_(O.closed_form_tensor("pos_embed.freqs", (2, H, hd // 2)))
        cos, sin = mx.get_freqs_cis(P, torch.device("cpu"))
        out[f"mixed_cos_H{H}_hd{hd}_P{P}"] = np.ascontiguousarray(np_(cos))
        out[f"mixed_sin_H{H}_hd{hd}_P{P}"] = np.ascontiguousarray(np_(sin))
        out[f"mixed_stride_H{H}_hd{hd}_P{P}"] = np.array(cos.stride(), dtype=np.int64)
    # mixed init formula (positional_encoding.py:266-290) with a known RNG stream
    torch.manual_seed(1234)
    mx = pe.RoPEMixed(dim=32, num_heads=6, theta=100.0)
    torch.manual_seed(1234)
    ang = torch.cat([torch.rand(1) * 2 * torch.pi for _ in range(6)])
    out["mixed_init_angles"] = np_(ang)
    out["mixed_init_freqs"] = np_(mx.freqs)
    # bias tables from closed-form parameters
    r = pe.RelativePositionalEncoding(64, num_heads=6)
    with torch.no_grad():
        r.relative_position_bias_table.copy_(
            O.closed_form_tensor("pos_embed.relative_position_bias_table", (6, 129)))
    out["rel_bias_H6_N65"] = np_(r.get_bias())
    for shared in (True, False):
        p = pe.PolynomialRPE(64, degree=3, num_heads=6, shared_across_heads=shared)
        shp = (4,) if shared else (6, 4)
        with torch.no_grad():
            p.coefficients.copy_(O.closed_form_tensor("pos_embed.coefficients", shp))
        out[f"poly_bias_H6_N65_{'shared' if shared else 'perhead'}"] = np_(p.get_bias())
    np.savez_compressed(os.path.join(OUT, "tables.npz"), **out)
    print("tables.npz", {k: v.shape for k, v in out.items()})


def gen_rotary(ref):
    ru, pe = ref["rope_utils"], ref["positional_encoding"]
    q = O.closed_form_tensor("rotary.q", (2, 6, 64, 32)) * 20
    k = O.closed_form_tensor("rotary.k", (2, 6, 64, 32)) * 20
    out = {}
    a = pe.RoPEAxial(dim=32, theta=100.0)
    cos, sin = a.get_freqs_cis(64, torch.device("cpu"))
    qr, kr = ru.apply_rotary_emb(q, k, ru.reshape_for_broadcast(cos, q),
                                 ru.reshape_for_broadcast(sin, q))
    out["axial_q"], out["axial_k"] = np_(qr), np_(kr)
    mx = pe.RoPEMixed(dim=32, num_heads=6, theta=100.0)
    with torch.no_grad():
        mx.freqs.copy_(O.closed_form_tensor("pos_embed.freqs", (2, 6, 16)))
    cos, sin = mx.get_freqs_cis(64, torch.device("cpu"))
    qr, kr = ru.apply_rotary_emb(q, k, ru.reshape_for_broadcast(cos, q),
                                 ru.reshape_for_broadcast(sin, q))
    out["mixed_q"], out["mixed_k"] = np_(qr), np_(kr)
    try:
        ru.reshape_for_broadcast(torch.zeros(4), q)
        out["bad_shape_raises"] = np.array(0)
    except ValueError:
        out["bad_shape_raises"] = np.array(1)
    np.savez_compressed(os.path.join(OUT, "rotary.npz"), **out)
    print("rotary.npz", {k: v.shape for k, v in out.items()})


ATTN_DIM, ATTN_H, ATTN_B, ATTN_N = 96, 3, 2, 65


def gen_attention(ref):
    """Single reference Attention module (vit.py:14-98): y, dx, dW, dPE."""
    vit, pe = ref["vit"], ref["positional_encoding"]
    out = {}
    for tag in ("none", "relative", "polynomial", "polynomial_perhead", "rope-axial", "rope-mixed"):
        torch.manual_seed(0)
        att = vit.Attention(ATTN_DIM, num_heads=ATTN_H)
        hd = ATTN_DIM // ATTN_H
        pem, freqs_cis = None, None
        if tag == "relative":
            pem = pe.RelativePositionalEncoding(ATTN_N - 1, ATTN_H)
        elif tag.startswith("polynomial"):
            pem = pe.PolynomialRPE(ATTN_N - 1, 3, ATTN_H, shared_across_heads=(tag == "polynomial"))
        elif tag == "rope-axial":
            pem = pe.RoPEAxial(hd, 100.0)
        elif tag == "rope-mixed":
            pem = pe.RoPEMixed(hd, ATTN_H, 100.0)
        elif tag == "none":
            pem = pe.NoPositionalEncoding()
        att.set_pos_encoding(pem)
        with torch.no_grad():
            att.qkv.weight.copy_(O.closed_form_tensor("attn.qkv.weight", (3 * ATTN_DIM, ATTN_DIM)))
            att.proj.weight.copy_(O.closed_form_tensor("attn.proj.weight", (ATTN_DIM, ATTN_DIM)))
            att.proj.bias.copy_(O.closed_form_tensor("attn.proj.bias", (ATTN_DIM,)))
            for n, p in pem.named_parameters():
                p.copy_(O.closed_form_tensor("pos_embed." + n, tuple(p.shape)))
        x = (O.closed_form_tensor("attn.x", (ATTN_B, ATTN_N, ATTN_DIM)) * 20).requires_grad_(True)
        dy = O.closed_form_tensor("attn.dy", (ATTN_B, ATTN_N, ATTN_DIM)) * 20
        if tag.startswith("rope"):
            freqs_cis = pem.get_freqs_cis(ATTN_N - 1, torch.device("cpu"))
        y = att(x, freqs_cis=freqs_cis)
        y.backward(dy)
        out[f"{tag}/y"] = np_(y)
        out[f"{tag}/dx"] = np_(x.grad)
        out[f"{tag}/dwqkv"] = np_(att.qkv.weight.grad)
        out[f"{tag}/dwproj"] = np_(att.proj.weight.grad)
        out[f"{tag}/dbproj"] = np_(att.proj.bias.grad)
        for n, p in pem.named_parameters():
            out[f"{tag}/dpe.{n}"] = np_(p.grad)
    np.savez_compressed(os.path.join(OUT, "attention.npz"), **out)
    print("attention.npz", {k: v.shape for k, v in out.items()})


TAB_DIM, TAB_H, TAB_B, TAB_N = 64, 2, 2, 17


def gen_attention_tables(ref):
    """The reference Attention.forward handed what its pos_encoding does not use (vit.py:51, 73-81): pos_encoding None,
    RelativePositionalEncoding and PolynomialRPE each handed constant (cos, sin) tables -- never rotated, the bias still
    added -- and RoPEAxial handed freqs_cis=None -- plain attention.  y alone, closed-form tensors as gen_attention."""
    vit, pe = ref["vit"], ref["positional_encoding"]
    D, H, B, N = TAB_DIM, TAB_H, TAB_B, TAB_N
    hd = D // H
    ang = torch.linspace(0.0, 2.5, (N - 1) * (hd // 2)).reshape(N - 1, hd // 2) ** 1.3   # angles up to 2.5 rad: no module's own
    cos, sin = torch.cos(ang), torch.sin(ang)
    out = {"cos": np_(cos), "sin": np_(sin)}
    for tag in ("none_tables", "relative_tables", "polynomial_tables", "rope-axial_none"):
        torch.manual_seed(0)
        att = vit.Attention(D, num_heads=H)
        pem = {"none_tables": None, "relative_tables": pe.RelativePositionalEncoding(N - 1, H),
               "polynomial_tables": pe.PolynomialRPE(N - 1, 3, H, shared_across_heads=True),
               "rope-axial_none": pe.RoPEAxial(hd, 100.0)}[tag]
        att.set_pos_encoding(pem)
        with torch.no_grad():
            att.qkv.weight.copy_(O.closed_form_tensor("attn.qkv.weight", (3 * D, D)))
            att.proj.weight.copy_(O.closed_form_tensor("attn.proj.weight", (D, D)))
            att.proj.bias.copy_(O.closed_form_tensor("attn.proj.bias", (D,)))
            for n, p in (pem.named_parameters() if pem is not None else ()):
                p.copy_(O.closed_form_tensor("pos_embed." + n, tuple(p.shape)))
            x = O.closed_form_tensor("attn.x", (B, N, D)) * 20
            out[f"{tag}/y"] = np_(att(x, freqs_cis=None if tag == "rope-axial_none" else (cos, sin)))
    np.savez_compressed(os.path.join(OUT, "attention_tables.npz"), **out)
    print("attention_tables.npz", {k: v.shape for k, v in out.items()})


SMALL = dict(embed_dim=96, depth=2, num_heads=3)
GRAD_KEYS_SMALL = ["patch_embed.weight", "patch_embed.bias", "cls_token", "blocks.0.attn.qkv.weight",
                   "blocks.0.norm1.weight", "blocks.0.norm1.bias", "blocks.0.attn.proj.bias",
                   "blocks.1.mlp.fc1.bias", "blocks.1.mlp.fc2.weight", "blocks.1.norm2.weight",
                   "norm.weight", "norm.bias", "head.weight", "head.bias"]


def gen_model(ref):
    out = {}
    for tag, extra in MODES:
        # reduced geometry: logits, loss, selected grads, 5-step AdamW trajectory
        cfg = mode_cfg(tag, extra, **SMALL)
        model = build_ref_model(ref, cfg)
        images, labels = O.closed_form_batch(cfg, 4)
        logits = model(images)
        loss = nn.CrossEntropyLoss()(logits, labels)
        loss.backward()
        out[f"small/{tag}/logits"] = np_(logits)
        out[f"small/{tag}/loss"] = np_(loss)
        grads = dict(model.named_parameters())
        for k in GRAD_KEYS_SMALL:
            out[f"small/{tag}/grad/{k}"] = np_(grads[k].grad)
        for k, p in grads.items():
            if k.startswith("pos_embed."):
                g = p.grad
                if k == "pos_embed.pos_embed":
                    g = g[:, :cfg.num_patches + 2]  # rows beyond N-1 are exactly zero
                    assert float(p.grad[:, cfg.num_patches:].abs().max()) == 0.0
                out[f"small/{tag}/grad/{k}"] = np_(g)
        out[f"small/{tag}/n_params"] = np.array(sum(p.numel() for p in model.parameters()))
        out[f"small/{tag}/state_keys"] = np.array(sorted(model.state_dict().keys()))
        # AdamW trajectory (train.py:111-116,195): same batch, 5 steps
        model = build_ref_model(ref, cfg)
        opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=0.01)
        traj = []
        for _ in range(5):
            opt.zero_grad()
            l = nn.CrossEntropyLoss()(model(images), labels)
            l.backward()
            opt.step()
            traj.append(float(l))
        out[f"small/{tag}/adamw_losses"] = np.array(traj, dtype=np.float64)
        out[f"small/{tag}/adamw_final_head_bias"] = np_(model.head.bias)
        # full CIFAR geometry: logits + loss + counts
        cfg = mode_cfg(tag, extra)
        model = build_ref_model(ref, cfg)
        images, labels = O.closed_form_batch(cfg, 4)
        with torch.no_grad():
            logits = model(images)
            feats = model.forward_features(images)
        out[f"full/{tag}/logits"] = np_(logits)
        out[f"full/{tag}/loss"] = np_(nn.CrossEntropyLoss()(logits, labels))
        out[f"full/{tag}/features_cls"] = np_(feats[:, 0])
        out[f"full/{tag}/n_params"] = np.array(sum(p.numel() for p in model.parameters()))
        out[f"full/{tag}/n_state_keys"] = np.array(len(model.state_dict()))
        out[f"full/{tag}/state_keys"] = np.array(sorted(model.state_dict().keys()))
        print(tag, "params", int(out[f"full/{tag}/n_params"]), "keys", int(out[f"full/{tag}/n_state_keys"]))
    # MNIST-shaped (BASELINE config 1): in_chans=1, none
    cfg = O.VitConfig(in_chans=1, pos_encoding="none")
    model = build_ref_model(ref, cfg)
    images, labels = O.closed_form_batch(cfg, 4)
    logits = model(images)
    loss = nn.CrossEntropyLoss()(logits, labels)
    loss.backward()
    out["mnist/none/logits"], out["mnist/none/loss"] = np_(logits), np_(loss)
    out["mnist/none/grad/patch_embed.weight"] = np_(model.patch_embed.weight.grad)
    # ImageNet-scale geometry, one block (BASELINE config 5 shape class)
    cfg = O.VitConfig(img_size=224, patch_size=16, embed_dim=768, depth=1, num_heads=12,
                      pos_encoding="rope-axial")
    model = build_ref_model(ref, cfg)
    images, labels = O.closed_form_batch(cfg, 2)
    with torch.no_grad():
        logits = model(images)
    out["imnet1/rope-axial/logits"] = np_(logits)
    out["imnet1/rope-axial/loss"] = np_(nn.CrossEntropyLoss()(logits, labels))
    # error behaviour (vit.py:195-196)
    try:
        ref["vit"].VisionTransformer(pos_encoding="bogus")
        out["bad_mode_message"] = np.array("")
    except ValueError as e:
        out["bad_mode_message"] = np.array(str(e))
    np.savez_compressed(os.path.join(OUT, "model.npz"), **out)
    print("model.npz", len(out), "arrays")


# head dimensions 24 / 48 (d = 192 at H = 8 / 4) and 128 (d = 384, H = 3): (tag, extra, embed_dim, num_heads)
HEADS_MODELS = [(tag, extra, 192, H) for H in (8, 4) for tag, extra in
                (("rope-mixed", {}), ("relative", {}),
                 ("polynomial_perhead", {"pos_encoding": "polynomial", "poly_shared_heads": False}))] + \
               [("rope-axial", {}, 384, 3)]
HEADS_QKV_ROWS = slice(3, None, 16)   # rows of the qkv-weight gradient kept: every head of q, k and v has some


def gen_heads(ref):
    """Depth-1 models at the head counts of HEADS_MODELS (B = 2, closed-form weights): logits, loss, the gradients of the
    positional parameters and a row sample of the gradient of blocks.0.attn.qkv.weight (tests/test_head_dims_gpu.py)."""
    out = {}
    for tag, extra, D, H in HEADS_MODELS:
        cfg = mode_cfg(tag, extra, embed_dim=D, depth=1, num_heads=H)
        model = build_ref_model(ref, cfg)
        images, labels = O.closed_form_batch(cfg, 2)
        logits = model(images)
        loss = nn.CrossEntropyLoss()(logits, labels)
        loss.backward()
        key = f"d{D}_h{H}/{tag}"
        out[f"{key}/logits"], out[f"{key}/loss"] = np_(logits), np_(loss)
        for k, p in model.named_parameters():
            if k.startswith("pos_embed."):
                out[f"{key}/grad/{k}"] = np_(p.grad)
        g = model.blocks[0].attn.qkv.weight.grad
        rows = np.arange(g.shape[0])[HEADS_QKV_ROWS]
        out[f"{key}/qkv_rows"] = rows.astype(np.int64)
        out[f"{key}/grad_rows/blocks.0.attn.qkv.weight"] = np_(g[torch.from_numpy(rows)])
    np.savez_compressed(os.path.join(OUT, "heads.npz"), **out)
    print("heads.npz", {k: v.shape for k, v in out.items()})


# gradients w.r.t. caller-supplied rotary tables (tests/test_rotary_grad_gpu.py): Attention at (d, H), N = 65, B = 2, and
# apply_rotary_emb on [2, 6, 64, 32].  Closed-form inputs (regenerated by the test), the outputs sampled to keep the file
# small: tokens RG_TOK of y / dx, rows RG_ROWS[d] of the weight gradients, positions RG_POS of dq / dk.
RG_GEOMS, RG_B, RG_N = ((96, 3), (192, 8)), 2, 65
RG_TOK, RG_ROWS, RG_POS = slice(0, None, 8), {96: slice(1, None, 8), 192: slice(1, None, 16)}, slice(0, None, 8)


def rotary_grad_tables(kind, shape):
    """(cos, sin) leaves of the rotary_grad cases: "angle" -> (angle, cos(angle), sin(angle)), a learned-angle table;
    "free" -> independent cos / sin with cos^2 + sin^2 != 1"""
    if kind == "angle":
        ang = (O.closed_form_tensor("rg.angle", shape) * 40).requires_grad_(True)
        return ang, ang.cos(), ang.sin()
    cos = (0.8 + O.closed_form_tensor("rg.cos", shape) * 6).requires_grad_(True)
    sin = (O.closed_form_tensor("rg.sin", shape) * 12).requires_grad_(True)
    return None, cos, sin


def gen_rotary_grad(ref):
    vit, pe, ru = ref["vit"], ref["positional_encoding"], ref["rope_utils"]
    out = {"tok": np.arange(RG_N)[RG_TOK], "pos": np.arange(64)[RG_POS]}
    for D, H in RG_GEOMS:
        hd, P = D // H, RG_N - 1
        out[f"d{D}/rows"] = np.arange(3 * D)[RG_ROWS[D]]
        for kind, shape in (("angle", (P, hd // 2)), ("free", (H, P, hd // 2))):
            att = vit.Attention(D, num_heads=H)
            att.set_pos_encoding(pe.RoPEAxial(hd, 100.0) if kind == "angle" else pe.RoPEMixed(hd, H, 100.0))
            with torch.no_grad():
                att.qkv.weight.copy_(O.closed_form_tensor("attn.qkv.weight", (3 * D, D)))
                att.proj.weight.copy_(O.closed_form_tensor("attn.proj.weight", (D, D)))
                att.proj.bias.copy_(O.closed_form_tensor("attn.proj.bias", (D,)))
            x = (O.closed_form_tensor("rg.x", (RG_B, RG_N, D)) * 20).requires_grad_(True)
            dy = O.closed_form_tensor("rg.dy", (RG_B, RG_N, D)) * 20
            ang, cos, sin = rotary_grad_tables(kind, shape)
            if ang is not None:
                cos.retain_grad(), sin.retain_grad()
            y = att(x, freqs_cis=(cos, sin))
            y.backward(dy)
            key = f"d{D}/{kind}"
            out[f"{key}/y"], out[f"{key}/dx"] = np_(y[:, RG_TOK]), np_(x.grad[:, RG_TOK])
            out[f"{key}/dwqkv"] = np_(att.qkv.weight.grad[RG_ROWS[D]])
            out[f"{key}/dwproj"] = np_(att.proj.weight.grad[RG_ROWS[D]])
            out[f"{key}/dbproj"] = np_(att.proj.bias.grad)
            out[f"{key}/dcos"], out[f"{key}/dsin"] = np_(cos.grad), np_(sin.grad)
            if ang is not None:
                out[f"{key}/dangle"] = np_(ang.grad)
    q = (O.closed_form_tensor("rotary.q", (2, 6, 64, 32)) * 20).requires_grad_(True)
    k = (O.closed_form_tensor("rotary.k", (2, 6, 64, 32)) * 20).requires_grad_(True)
    dq_up = O.closed_form_tensor("rg.dq", (2, 6, 64, 32)) * 20
    dk_up = O.closed_form_tensor("rg.dk", (2, 6, 64, 32)) * 20
    for tag, shape in (("shared", (1, 1, 64, 16)), ("per_head", (1, 6, 64, 16))):
        q.grad = k.grad = None
        _, cos, sin = rotary_grad_tables("free", shape)
        qr, kr = ru.apply_rotary_emb(q, k, cos, sin)
        ((qr * dq_up).sum() + (kr * dk_up).sum()).backward()
        out[f"rot/{tag}/dq"], out[f"rot/{tag}/dk"] = np_(q.grad[:, :, RG_POS]), np_(k.grad[:, :, RG_POS])
        out[f"rot/{tag}/dcos"], out[f"rot/{tag}/dsin"] = np_(cos.grad), np_(sin.grad)
    np.savez_compressed(os.path.join(OUT, "rotary_grad.npz"), **out)
    print("rotary_grad.npz", {k: v.shape for k, v in out.items()})


# --------------------------------------------------------------------------- resize.npz
# transforms.Resize(S) of reference train.py:70,79 on the square PIL images of datasets.MNIST (mode L) and
# datasets.CIFAR10 (mode RGB) is, by torchvision's documented behaviour, img.resize((S, S), Image.BILINEAR) (PIL always
# antialiases).  torchvision is not installed in the build container, so that mapping is taken from its documentation
# and could not be confirmed by running it; what the fixture pins is PIL's resize itself.
RESIZE_CASES = {"mnist": (1, 28, (14, 16, 32, 64, 224)), "cifar": (3, 32, (16, 24, 48, 64, 224))}


def resize_pass_coeffs(size_in, size_out):
    """PIL's 8-bit bilinear coefficients of one pass, restated independently of PIL (Python floats are IEEE doubles,
    one operation per expression): -> (bounds int32 [out,2], kk int32 [out,ksize])."""
    import math
    scale = size_in / size_out
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((size_out, 2), dtype=np.int32)
    kk = np.zeros((size_out, ksize), dtype=np.int32)
    for xx in range(size_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), size_in) - xmin
        w = []
        for x in range(n):
            t = abs((x + xmin - center + 0.5) / fs)
            w.append(1.0 - t if t < 1.0 else 0.0)
        ww = 0.0
        for v in w:
            ww += v
        for x in range(n):
            kk[xx, x] = int(w[x] / ww * float(1 << 22) + 0.5)
        bounds[xx] = (xmin, n)
    return bounds, kk


def resize_apply(planes, bounds, kk):
    """One pass along the last axis by the integer formula: clip((2^21 + sum in[xmin + x] * k[x]) >> 22)."""
    idx = np.minimum(bounds[:, :1] + np.arange(kk.shape[1])[None], planes.shape[-1] - 1)   # taps past n weigh 0
    acc = (planes[..., idx].astype(np.int64) * kk.astype(np.int64)).sum(-1) + (1 << 21)
    return np.clip(acc >> 22, 0, 255).astype(np.uint8)


def resize_inputs(rng, n, C, S0):
    """n images [n,C,S0,S0] uint8: random bytes, a 0/255 checkerboard (clip and rounding half-way points), a smooth
    ramp, random again."""
    x = rng.integers(0, 256, (n, C, S0, S0), dtype=np.uint8)
    yy, xx = np.mgrid[0:S0, 0:S0]
    if n > 1:
        for c in range(C):
            x[1, c] = (((yy + xx + c) % 2) * 255).astype(np.uint8)
    if n > 2:
        for c in range(C):
            x[2, c] = ((yy * (c + 1) + xx * (3 - c)) * 255 // ((S0 - 1) * 4)).astype(np.uint8)
    return x


def gen_resize():
    from PIL import Image
    rng = np.random.default_rng(20261016)
    out = {}
    for name, (C, S0, sizes) in RESIZE_CASES.items():
        for S in sizes:
            n = 2 if S == 224 else 4
            x = resize_inputs(rng, n, C, S0)
            y = np.zeros((n, C, S, S), dtype=np.uint8)
            for i in range(n):
                if C == 1:
                    y[i, 0] = np.asarray(Image.fromarray(x[i, 0], "L").resize((S, S), Image.BILINEAR))
                else:
                    hwc = np.ascontiguousarray(x[i].transpose(1, 2, 0))
                    y[i] = np.asarray(Image.fromarray(hwc, "RGB").resize((S, S), Image.BILINEAR)).transpose(2, 0, 1)
            bounds, kk = resize_pass_coeffs(S0, S)
            mid = resize_apply(x, bounds, kk)                                        # horizontal -> [n,C,S0,S]
            mine = resize_apply(mid.transpose(0, 1, 3, 2), bounds, kk).transpose(0, 1, 3, 2)   # vertical
            assert np.array_equal(mine, y), f"{name} {S0}->{S}: the restated coefficients do not reproduce PIL"
            key = f"{name}/{S}"
            out[f"{key}/x"], out[f"{key}/y"], out[f"{key}/bounds"], out[f"{key}/kk"] = x, y, bounds, kk
    np.savez_compressed(os.path.join(OUT, "resize.npz"), **out)
    print("resize.npz", {k: v.shape for k, v in out.items() if k.endswith("/y")})


# ---- dropout.npz: the reference's own Attention / Block arithmetic under GIVEN dropout masks ------------------------------
# The masks are the project's documented stream (DESIGN.md "Dropout streams", restated in tests/dropout_stream.py) for fixed
# (seed, offset) pairs; the reference's nn.Dropout modules, the timm stand-in's drop and DropPath are replaced by modules
# that multiply with those masks, everything else is the reference's vit.py.  Inputs and weights are closed-form (not
# stored); stored: the pairs, the packed mask bits, outputs and gradients (large weight gradients as a row sample).
DROP_DIM, DROP_H = 96, 3
DROP_ATTN_CASES = [("rope-axial", 17, 3), ("relative", 17, 3), ("rope-axial", 65, 2), ("relative", 65, 2)]
DROP_ATTN_P, DROP_PROJ_P = 0.1, 0.2
DROP_BLOCK = dict(N=17, B=4, drop=0.1, attn_drop=0.15, drop_path=0.3)


class _MaskMul(nn.Module):
    """x * mask_k on the k-th call (masks already carry 1 / (1 - p))"""

    def __init__(self, *masks):
        super().__init__()
        self.masks, self.calls = masks, 0

    def forward(self, x):
        m = self.masks[self.calls % len(self.masks)]
        self.calls += 1
        return x * m


def _drop_pairs(tag, n):
    """n fixed (seed, offset) pairs below 2^63 (torch int64), derived from the case tag"""
    import hashlib
    h = hashlib.sha256(tag.encode()).digest()
    while len(h) < 16 * n:
        h += hashlib.sha256(h).digest()
    v = np.frombuffer(h[:16 * n], dtype="<u8").reshape(n, 2) >> np.uint64(1)
    return [(int(a), int(b)) for a, b in v]


def gen_dropout(ref):
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import dropout_stream as S
    vit, pe = ref["vit"], ref["positional_encoding"]
    out = {}
    CF = O.closed_form_tensor
    f32 = lambda m, p: torch.from_numpy(m.astype(np.float32) * S.scale(p))  # noqa: E731
    for tag, N, B in DROP_ATTN_CASES:
        key = f"attn/{tag}/n{N}"
        pairs = _drop_pairs(key, 2)
        att = vit.Attention(DROP_DIM, num_heads=DROP_H, qkv_bias=True, attn_drop=DROP_ATTN_P, proj_drop=DROP_PROJ_P)
        hd = DROP_DIM // DROP_H
        pem = pe.RelativePositionalEncoding(N - 1, DROP_H) if tag == "relative" else pe.RoPEAxial(hd, 100.0)
        att.set_pos_encoding(pem)
        with torch.no_grad():
            for n, p in att.named_parameters():
                if not n.startswith("pos_encoding."):
                    p.copy_(CF("attn." + n, tuple(p.shape)))
            for n, p in pem.named_parameters():
                p.copy_(CF("pos_embed." + n, tuple(p.shape)))
        ma = S.mask_attention(pairs[0], B, DROP_H, N, DROP_ATTN_P)
        mp = S.mask_elements(pairs[1], B * N * DROP_DIM, DROP_PROJ_P).reshape(B, N, DROP_DIM)
        att.attn_drop, att.proj_drop = _MaskMul(f32(ma, DROP_ATTN_P)), _MaskMul(f32(mp, DROP_PROJ_P))
        x = (CF("attn.x", (B, N, DROP_DIM)) * 20).requires_grad_(True)
        dy = CF("attn.dy", (B, N, DROP_DIM)) * 20
        freqs_cis = pem.get_freqs_cis(N - 1, torch.device("cpu")) if tag == "rope-axial" else None
        y = att(x, freqs_cis=freqs_cis)
        y.backward(dy)
        out[f"{key}/pairs"] = np.array(pairs, dtype=np.int64)
        out[f"{key}/mask_attn"], out[f"{key}/mask_proj"] = np.packbits(ma), np.packbits(mp)
        out[f"{key}/y"], out[f"{key}/dx"] = np_(y), np_(x.grad)
        out[f"{key}/grad_rows4/qkv.weight"] = np_(att.qkv.weight.grad)[::4]
        for n in ("qkv.bias", "proj.weight", "proj.bias"):
            out[f"{key}/grad/{n}"] = np_(dict(att.named_parameters())[n].grad)
        for n, p in pem.named_parameters():
            out[f"{key}/grad/pos_encoding.{n}"] = np_(p.grad)
    c = DROP_BLOCK
    N, B = c["N"], c["B"]
    pairs = _drop_pairs("block", 6)      # attention probabilities, proj, drop1, drop2, drop-path (attention), drop-path (MLP)
    blk = vit.Block(DROP_DIM, DROP_H, qkv_bias=True, drop=c["drop"], attn_drop=c["attn_drop"], drop_path=0.)
    blk.set_pos_encoding(pe.NoPositionalEncoding())
    with torch.no_grad():
        for n, p in blk.named_parameters():
            p.copy_(CF("blk." + n, tuple(p.shape)))
    hid = blk.mlp.fc1.weight.shape[0]
    ma = S.mask_attention(pairs[0], B, DROP_H, N, c["attn_drop"])
    mp = S.mask_elements(pairs[1], B * N * DROP_DIM, c["drop"]).reshape(B, N, DROP_DIM)
    m1 = S.mask_elements(pairs[2], B * N * hid, c["drop"]).reshape(B, N, hid)
    m2 = S.mask_elements(pairs[3], B * N * DROP_DIM, c["drop"]).reshape(B, N, DROP_DIM)
    da, dm = (S.mask_elements(pairs[k], B, c["drop_path"]).reshape(B, 1, 1) for k in (4, 5))
    blk.attn.attn_drop, blk.attn.proj_drop = _MaskMul(f32(ma, c["attn_drop"])), _MaskMul(f32(mp, c["drop"]))
    # timm's Mlp: fc1 -> act -> drop1 -> fc2 -> drop2; timm's DropPath(scale_by_keep=True): x * keep_b / (1 - p) -- both
    # third-party, restated (parity unpinned); the Block applies ONE DropPath module to both branches (vit.py:115,122,124)
    d1, d2 = _MaskMul(f32(m1, c["drop"])), _MaskMul(f32(m2, c["drop"]))
    mlp = blk.mlp
    mlp.forward = lambda t: d2(mlp.fc2(d1(mlp.act(mlp.fc1(t)))))
    blk.drop_path = _MaskMul(f32(da, c["drop_path"]), f32(dm, c["drop_path"]))
    x = (CF("blk.x", (B, N, DROP_DIM)) * 20).requires_grad_(True)
    dy = CF("blk.dy", (B, N, DROP_DIM)) * 20
    y = blk(x)
    y.backward(dy)
    out["block/pairs"] = np.array(pairs, dtype=np.int64)
    for n, m in (("attn", ma), ("proj", mp), ("drop1", m1), ("drop2", m2), ("path_attn", da), ("path_mlp", dm)):
        out[f"block/mask_{n}"] = np.packbits(m)
    out["block/y"], out["block/dx"] = np_(y), np_(x.grad)
    rows = {"attn.qkv.weight": 4, "mlp.fc1.weight": 8, "mlp.fc2.weight": 4}
    for n, p in blk.named_parameters():
        if n in rows:
            out[f"block/grad_rows{rows[n]}/{n}"] = np_(p.grad)[::rows[n]]
        else:
            out[f"block/grad/{n}"] = np_(p.grad)
    np.savez_compressed(os.path.join(OUT, "dropout.npz"), **out)
    print("dropout.npz", {k: v.shape for k, v in out.items()})


def main():
    if sys.argv[1:] == ["--only", "resize"]:   # PIL only: the reference's modules are not needed; the others stay as they are
        os.makedirs(OUT, exist_ok=True)
        gen_resize()
        print("resize.npz", os.path.getsize(os.path.join(OUT, "resize.npz")), "bytes")
        return
    assert os.path.isdir(REF), "reference not present: this script runs in the build container only"
    os.makedirs(OUT, exist_ok=True)
    torch.set_num_threads(8)
    ref = load_reference()
    if sys.argv[1:] == ["--only", "heads"]:   # leaves the other fixtures byte-identical
        gen_heads(ref)
        print("heads.npz", os.path.getsize(os.path.join(OUT, "heads.npz")), "bytes")
        return
    if sys.argv[1:] == ["--only", "dropout"]:
        gen_dropout(ref)
        print("dropout.npz", os.path.getsize(os.path.join(OUT, "dropout.npz")), "bytes")
        return
    if sys.argv[1:] == ["--only", "rotary_grad"]:
        gen_rotary_grad(ref)
        print("rotary_grad.npz", os.path.getsize(os.path.join(OUT, "rotary_grad.npz")), "bytes")
        return
    if sys.argv[1:] == ["--only", "attention_tables"]:
        gen_attention_tables(ref)
        print("attention_tables.npz", os.path.getsize(os.path.join(OUT, "attention_tables.npz")), "bytes")
        return
    gen_tables(ref)
    gen_rotary(ref)
    gen_attention(ref)
    gen_attention_tables(ref)
    gen_model(ref)
    gen_heads(ref)
    gen_rotary_grad(ref)
    gen_dropout(ref)
    gen_resize()
    for f in sorted(os.listdir(OUT)):
        print(f, os.path.getsize(os.path.join(OUT, f)), "bytes")


if __name__ == "__main__":
    main()
