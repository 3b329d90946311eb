"""The torch.ops.vitpe.* layer, the parts that need no GPU: every fake (meta) implementation against what the real op is
specified to return on the route its shape takes, the schemas, and the float64 references of ops_ref.py themselves -- that
they are right (against the oracle and torch.nn.functional) and that each defect the GPU tests are aimed at would miss
the gate those tests use by a wide margin."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ops_ref as R
from conftest import rel_err
from oracle import vit_oracle as O

F32, BF16 = torch.float32, torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    import vitpe.ops
    return vitpe.ops


def meta(*shape, dtype=F32):
    return torch.empty(*shape, dtype=dtype, device="meta")


def transposed(B, N, D, dtype):
    """a non-contiguous [B, N, D]: a [N, B, D] tensor transposed"""
    t = meta(N, B, D, dtype=dtype).transpose(0, 1)
    assert tuple(t.shape) == (B, N, D) and not t.is_contiguous()
    return t


def check(outs, spec, what):
    """each output: the shape and dtype of the spec, freshly allocated and contiguous (the real ops' outputs are)"""
    outs = outs if isinstance(outs, (tuple, list)) else (outs,)
    assert len(outs) == len(spec), what
    for i, (o, (shape, dtype)) in enumerate(zip(outs, spec)):
        assert tuple(o.shape) == tuple(shape), f"{what}: output {i} has shape {tuple(o.shape)}, the real op returns {tuple(shape)}"
        assert o.dtype == dtype, f"{what}: output {i} is {o.dtype}, the real op returns {dtype}"
        assert o.is_contiguous(), f"{what}: output {i} has strides {o.stride()}, the real op returns a contiguous tensor"
        assert o.device.type == "meta"


def attn_meta_args(c, x, tables_grad=False):
    dt = R.DT[c.dt]
    B, N, D, H = c.B, c.N, c.D, c.H
    pe_param = None if c.pe_param is None else meta(*c.pe_param.shape)
    inv_freq = meta(c.hd // 4) if "inv_freq" in c.pe else None
    cos = None if c.cos is None else meta(*c.cos.shape)
    mode, grid, _, _, degree, per_head, _, _ = R.op_pe_args(c)
    resid = None if c.resid is None else meta(B, N, D, dtype=dt)
    return x, resid, (H, mode, grid, pe_param, inv_freq, degree, per_head, cos, cos, tables_grad)


# ---- fakes against the route -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("contig", [True, False], ids=["contiguous", "transposed"])
@pytest.mark.parametrize("route,mode,resid", R.ATTN_CASES)
def test_attention_fake_returns_the_route_s_saved_tensors(ops, route, mode, resid, contig):
    """vitpe::attention on meta tensors: y and a are [B, N, D] and `qkv` is what the route of this geometry saves -- empty
    on the routes that keep it on the chip (a, b), [B, N, 3D] on the hd-64 one-kernel route (c) and on Linear + core (d, e).
    The expected shape comes from the library's host predicates, not from the fake."""
    c = R.attn_case(route, mode, resid)
    dt = R.DT[c.dt]
    B, N, D = c.B, c.N, c.D
    x = meta(B, N, D, dtype=dt) if contig else transposed(B, N, D, dt)
    x, res, tail = attn_meta_args(c, x)
    out = torch.ops.vitpe.attention(x, meta(3 * D, D), meta(D, D), meta(D), res, *tail)
    got_route = R.route_of(c.dt, N, D, c.H)
    spec = [((B, N, D), dt), ((B, N, D), dt), (R.qkv_shape(got_route, B, N, D), dt)]
    check(out, spec, f"vitpe::attention route {route} ({got_route})")
    check(ops.attention_fake(x, meta(3 * D, D), meta(D, D), meta(D), res, *tail), spec, "attention_fake called directly")
    # the drop op: Linear + core at every geometry
    out = torch.ops.vitpe.attention_drop(x, meta(3 * D, D), meta(3 * D), meta(D, D), meta(D), res, *tail, 0.0, 0.0, None)
    check(out, spec[:2] + [((B, N, 3 * D), dt)], f"vitpe::attention_drop route {route}")


@pytest.mark.parametrize("route,tables,resid", R.TABLE_CASES)
@pytest.mark.parametrize("tables_grad", [False, True])
def test_attention_fake_with_caller_tables(ops, route, tables, resid, tables_grad):
    """constant caller tables keep the route of the geometry; tables that require grad take Linear + core everywhere"""
    c = R.attn_case(route, "none", resid, tables)
    dt = R.DT[c.dt]
    B, N, D = c.B, c.N, c.D
    x, res, tail = attn_meta_args(c, meta(B, N, D, dtype=dt), tables_grad)
    out = torch.ops.vitpe.attention(x, meta(3 * D, D), meta(D, D), meta(D), res, *tail)
    r = R.route_of(c.dt, N, D, c.H, tables_grad=tables_grad)
    assert r == ("core" if tables_grad else c.want_route)
    check(out, [((B, N, D), dt), ((B, N, D), dt), (R.qkv_shape(r, B, N, D), dt)], f"vitpe::attention tables {route}")


def test_case_lists_sit_on_their_routes():
    """every listed geometry reaches the route it is listed under (attn_case asserts it; here for the whole list, and
    that the list covers every route)"""
    seen = {R.attn_case(r, m, res).want_route for r, m, res in R.ATTN_CASES}
    assert seen == {"fused16", "wide32", "fused64", "core"}
    for r, m in R.DROP_CASES:   # a qkv bias leaves the fused kernels
        assert R.attn_case(r, m, True, None, True).want_route == "core"
    from vitpe import _lib
    assert _lib.lib().vitpe_fused_attention_supported(_lib.BF16, 65, 192, 32) == 1   # (what route b would otherwise take)


@pytest.mark.parametrize("contig", [True, False], ids=["contiguous", "transposed"])
@pytest.mark.parametrize("shape,dt", R.LN_CASES)
def test_layer_norm_and_dropout_fakes(ops, shape, dt, contig):
    B, N, D = shape
    x = meta(B, N, D, dtype=R.DT[dt]) if contig else transposed(B, N, D, R.DT[dt])
    check(torch.ops.vitpe.layer_norm(x, meta(D), meta(D), 1e-5), [(shape, R.DT[dt]), ((B * N,), F32), ((B * N,), F32)], "vitpe::layer_norm")
    rng = meta(2, dtype=torch.int64)
    for name in ("dropout", "drop_path"):
        for res in (None, x):
            check(getattr(torch.ops.vitpe, name)(x, res, 0.25, rng), [(shape, R.DT[dt])], "vitpe::" + name)


@pytest.mark.parametrize("contig", [True, False], ids=["contiguous", "transposed"])
@pytest.mark.parametrize("shape,hid,dt,resid", R.MLP_CASES)
def test_mlp_fake(ops, shape, hid, dt, resid, contig):
    B, N, D = shape
    t = R.DT[dt]
    x = meta(B, N, D, dtype=t) if contig else transposed(B, N, D, t)
    out = torch.ops.vitpe.mlp(x, meta(hid, D), meta(hid), meta(D, hid), meta(D), x if resid else None)
    check(out, [(shape, t), ((B * N, hid), t), ((B * N, hid), t)], "vitpe::mlp")
    out = torch.ops.vitpe.mlp(x, meta(hid, D), meta(hid), meta(D, hid), meta(D), None, 0.1, meta(2, 2, dtype=torch.int64))
    check(out, [(shape, t), ((B * N, hid), t), ((B * N, hid), t)], "vitpe::mlp, p > 0")


@pytest.mark.parametrize("contig", [True, False], ids=["contiguous", "transposed"])
@pytest.mark.parametrize("B,N,D,C,dt", R.HEAD_CASES)
def test_head_and_cross_entropy_fakes(ops, B, N, D, C, dt, contig):
    x = meta(B, N, D, dtype=R.DT[dt]) if contig else transposed(B, N, D, R.DT[dt])
    out = torch.ops.vitpe.head(x, meta(D), meta(D), meta(C, D), meta(C), 1e-5)
    check(out, [((B, C), F32), ((B, D), F32), ((B, D), F32), ((B,), F32)], "vitpe::head")
    logits = meta(5, 10) if contig else meta(10, 5).t()
    check(torch.ops.vitpe.cross_entropy(logits, meta(5, dtype=torch.int64)), [((), F32), ((5, 10), F32)], "vitpe::cross_entropy")


@pytest.mark.parametrize("contig", [True, False], ids=["contiguous", "channels_last"])
@pytest.mark.parametrize("ape,dt", R.EMBED_CASES)
def test_patch_embed_fake(ops, ape, dt, contig):
    g = R.EMBED_GEOM
    B, C, S, p, D = g["B"], g["C"], g["S"], g["p"], g["D"]
    P = (S // p) ** 2
    images = meta(B, C, S, S) if contig else meta(B, S, S, C).permute(0, 3, 1, 2)
    out = torch.ops.vitpe.patch_embed(images, meta(D, C, p, p), meta(D), meta(1, 1, D), meta(1, g["max_len"], D) if ape else None,
                                      p, dt == "bf16")
    check(out, [((B, P + 1, D), R.DT[dt]), ((B * P, C * p * p), R.DT[dt])], "vitpe::patch_embed")


@pytest.mark.parametrize("contig", [True, False], ids=["contiguous", "transposed"])
@pytest.mark.parametrize("cls_only", [False, True])
def test_attention_probs_fake(ops, cls_only, contig):
    B, N, D, H = 3, 26, 64, 2
    qkv = meta(B, N, 3 * D, dtype=BF16) if contig else transposed(B, N, 3 * D, BF16)
    out = torch.ops.vitpe.attention_probs(qkv, H, 0, 5, None, None, 0, False, None, None, cls_only)
    check(out, [((B, H, N) if cls_only else (B, H, N, N), F32)], "vitpe::attention_probs")


# ---- the fakes of the backward ops: every gradient in the shape and type of what it is the gradient of ------------------------
@pytest.mark.parametrize("route,mode", [("a", "relative"), ("b", "polynomial_perhead"), ("c", "rope-mixed"), ("d16", "none"),
                                        ("e", "polynomial")])
@pytest.mark.parametrize("has_bqkv", [False, True])
def test_attention_backward_fake(ops, route, mode, has_bqkv):
    c = R.attn_case(route, mode, True)
    dt = R.DT[c.dt]
    B, N, D = c.B, c.N, c.D
    x, _, (H, m, grid, pe_param, inv_freq, degree, per_head, _, _, _) = attn_meta_args(c, transposed(B, N, D, dt))
    qkv = meta(*R.qkv_shape(c.want_route, B, N, D), dtype=dt)
    out = torch.ops.vitpe.attention_backward(transposed(B, N, D, dt), x, meta(3 * D, D), meta(D, D), meta(B, N, D, dtype=dt), qkv,
                                             pe_param, inv_freq, None, None, None, True, H, m, grid, degree, per_head, False,
                                             has_bqkv, 0.0, 0.0)
    none = ((0,), dt)
    check(out, [((B, N, D), dt), ((3 * D, D), F32), ((3 * D,), F32) if has_bqkv else none, ((D, D), F32), ((D,), F32),
                (tuple(pe_param.shape), F32) if pe_param is not None else none, none, none], "vitpe::attention_backward")
    # caller tables that require grad: d cos / d sin in their shape, no parameter gradient
    cos = meta(H, N - 1, c.hd // 2)
    out = torch.ops.vitpe.attention_backward(meta(B, N, D, dtype=dt), x, meta(3 * D, D), meta(D, D), meta(B, N, D, dtype=dt),
                                             meta(B, N, 3 * D, dtype=dt), None, None, cos, cos, None, True, H, 5, grid, 0, False,
                                             True, False, 0.0, 0.0)
    check(out[5:], [none, (tuple(cos.shape), F32), (tuple(cos.shape), F32)], "vitpe::attention_backward, tables_grad")


def test_other_backward_fakes(ops):
    B, N, D, HID, C = 3, 26, 64, 256, 10
    for dt in (F32, BF16):
        x, dy = transposed(B, N, D, dt), transposed(B, N, D, dt)
        check(torch.ops.vitpe.layer_norm_backward(dy, x, meta(D), meta(B * N), meta(B * N)),
              [((B, N, D), dt), ((D,), F32), ((D,), F32)], "vitpe::layer_norm_backward")
        check(torch.ops.vitpe.mlp_backward(dy, x, meta(HID, D), meta(D, HID), meta(B * N, HID, dtype=dt), meta(B * N, HID, dtype=dt), None, 0.0),
              [((B, N, D), dt), ((HID, D), F32), ((HID,), F32), ((D, HID), F32), ((D,), F32)], "vitpe::mlp_backward")
        for name in ("dropout_backward", "drop_path_backward"):
            check(getattr(torch.ops.vitpe, name)(dy, meta(2, dtype=torch.int64), 0.25), [((B, N, D), dt)], "vitpe::" + name)
        for ape_len in (0, 40):
            check(torch.ops.vitpe.patch_embed_backward(dy, meta(B * (N - 1), 48, dtype=dt), ape_len),
                  [((D, 48), F32), ((D,), F32), ((D,), F32), ((1, ape_len, D) if ape_len else (0,), F32)], "vitpe::patch_embed_backward")
        check(torch.ops.vitpe.head_backward(meta(B, C), meta(D), meta(C, D), meta(B, D), meta(B, D), meta(B), dt == BF16, N),
              [((B, N, D), dt), ((D,), F32), ((D,), F32), ((C, D), F32), ((C,), F32)], "vitpe::head_backward")


def test_forward_and_backward_trace_on_fake_tensors(ops):
    """What torch.compile / AOT autograd does to an op: run its forward AND the function registered as its backward on
    fake tensors.  A backward that hands data pointers to the library cannot be run that way, so each one is an op of its
    own; the traced graph holds the forward ops and their backward ops."""
    from torch.fx.experimental.proxy_tensor import make_fx

    def m(*shape, dtype=F32, rg=True):
        return torch.empty(*shape, dtype=dtype, device="meta", requires_grad=rg)

    B, N, D, H, HID, C = 3, 26, 64, 2, 256, 10

    def step(rng, images, wpe, bpe, cls, ape, g1, b1, wqkv, bqkv, wproj, bproj, table, w1, c1, w2, c2, gh, bh, wh, ch, labels):
        v = torch.ops.vitpe
        x = v.patch_embed(images, wpe, bpe, cls, ape, 4, False)[0]
        n1 = v.layer_norm(x, g1, b1, 1e-5)[0]
        x = v.attention(n1, wqkv, wproj, bproj, x, H, 2, 5, table, None, 0, False)[0]
        x = v.attention_drop(n1, wqkv, bqkv, wproj, bproj, x, H, 2, 5, table, None, 0, False, None, None, False, 0.1, 0.1, rng)[0]
        x = v.drop_path(v.dropout(v.mlp(x, w1, c1, w2, c2, None, 0.1, rng)[0], None, 0.1, rng[0]), x, 0.1, rng[1])
        loss = v.cross_entropy(v.head(x, gh, bh, wh, ch, 1e-5)[0], labels)[0]
        params = (wpe, bpe, cls, ape, g1, b1, wqkv, bqkv, wproj, bproj, table, w1, c1, w2, c2, gh, bh, wh, ch)
        return torch.autograd.grad(0.37 * loss, params)

    args = (torch.empty(2, 2, dtype=torch.int64, device="meta"), m(B, 3, 20, 20, rg=False), m(D, 3, 4, 4), m(D), m(1, 1, D), m(1, 40, D), m(D), m(D), m(3 * D, D), m(3 * D), m(D, D), m(D),
            m(H, 2 * N - 1), m(HID, D), m(HID), m(D, HID), m(D), m(D), m(D), m(C, D), m(C),
            torch.empty(B, dtype=torch.int64, device="meta"))
    gm = make_fx(step, tracing_mode="fake")(*args)
    seen = {str(n.target).split(".")[1] for n in gm.graph.nodes if n.op == "call_function" and str(n.target).startswith("vitpe.")}
    assert seen == set(SCHEMAS) - {"attention_probs"}, sorted(set(SCHEMAS) - seen)
    for g, a in zip(gm(*args), args[2:]):
        assert g.shape == a.shape and g.dtype == F32


# ---- schemas ------------------------------------------------------------------------------------------------------------
SCHEMAS = {
    "layer_norm": "vitpe::layer_norm(Tensor x, Tensor weight, Tensor bias, float eps) -> (Tensor, Tensor, Tensor)",
    "attention": "vitpe::attention(Tensor xn, Tensor wqkv, Tensor wproj, Tensor bproj, Tensor? resid, SymInt num_heads, SymInt mode, "
                 "SymInt grid, Tensor? pe_param, Tensor? inv_freq, SymInt degree, bool per_head, Tensor? cos=None, Tensor? sin=None, "
                 "bool tables_grad=False) -> (Tensor, Tensor, Tensor)",
    "attention_drop": "vitpe::attention_drop(Tensor xn, Tensor wqkv, Tensor? bqkv, Tensor wproj, Tensor bproj, Tensor? resid, "
                      "SymInt num_heads, SymInt mode, SymInt grid, Tensor? pe_param, Tensor? inv_freq, SymInt degree, bool per_head, "
                      "Tensor? cos, Tensor? sin, bool tables_grad, float attn_p, float proj_p, Tensor? rng) -> (Tensor, Tensor, Tensor)",
    "attention_probs": "vitpe::attention_probs(Tensor qkv, SymInt num_heads, SymInt mode, SymInt grid, Tensor? pe_param, "
                       "Tensor? inv_freq, SymInt degree, bool per_head, Tensor? cos=None, Tensor? sin=None, bool cls_only=False) -> Tensor",
    "mlp": "vitpe::mlp(Tensor xn, Tensor w1, Tensor b1, Tensor w2, Tensor b2, Tensor? resid, float p=0., Tensor? rng=None) "
           "-> (Tensor, Tensor, Tensor)",
    "dropout": "vitpe::dropout(Tensor x, Tensor? resid, float p, Tensor rng) -> Tensor",
    "drop_path": "vitpe::drop_path(Tensor x, Tensor? resid, float p, Tensor rng) -> Tensor",
    "patch_embed": "vitpe::patch_embed(Tensor images, Tensor weight, Tensor bias, Tensor cls_token, Tensor? ape, SymInt patch, "
                   "bool bf16) -> (Tensor, Tensor)",
    "head": "vitpe::head(Tensor x, Tensor gamma, Tensor beta, Tensor wh, Tensor bh, float eps) -> (Tensor, Tensor, Tensor, Tensor)",
    "cross_entropy": "vitpe::cross_entropy(Tensor logits, Tensor labels) -> (Tensor, Tensor)",
    # the hand-written backwards, ops of their own so that the functions registered with autograd stay traceable
    "layer_norm_backward": "vitpe::layer_norm_backward(Tensor dy, Tensor x, Tensor weight, Tensor mean, Tensor rstd) "
                           "-> (Tensor, Tensor, Tensor)",
    "attention_backward": "vitpe::attention_backward(Tensor dy, Tensor xn, Tensor wqkv, Tensor wproj, Tensor a, Tensor qkv, "
                          "Tensor? pe_param, Tensor? inv_freq, Tensor? cos, Tensor? sin, Tensor? rng, bool one_kernel, "
                          "SymInt num_heads, SymInt mode, SymInt grid, SymInt degree, bool per_head, bool tables_grad, "
                          "bool has_bqkv, float attn_p, float proj_p) "
                          "-> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)",
    "mlp_backward": "vitpe::mlp_backward(Tensor dy, Tensor xn, Tensor w1, Tensor w2, Tensor h, Tensor u, Tensor? rng, float p) "
                    "-> (Tensor, Tensor, Tensor, Tensor, Tensor)",
    "dropout_backward": "vitpe::dropout_backward(Tensor dy, Tensor rng, float p) -> Tensor",
    "drop_path_backward": "vitpe::drop_path_backward(Tensor dy, Tensor rng, float p) -> Tensor",
    "patch_embed_backward": "vitpe::patch_embed_backward(Tensor dtok, Tensor patches, SymInt ape_len) "
                            "-> (Tensor, Tensor, Tensor, Tensor)",
    "head_backward": "vitpe::head_backward(Tensor dlogits, Tensor gamma, Tensor wh, Tensor xhat, Tensor yn, Tensor rstd, "
                     "bool bf16, SymInt ntok) -> (Tensor, Tensor, Tensor, Tensor, Tensor)",
}


def test_schemas_pinned(ops):
    import os
    import re
    src = open(os.path.splitext(ops.__file__)[0] + ".py").read()
    assert sorted(re.findall(r'custom_op\("vitpe::(\w+)"', src)) == sorted(SCHEMAS), "an op was added or removed: pin its schema here"
    for name, want in SCHEMAS.items():
        assert str(getattr(torch.ops.vitpe, name).default._schema) == want, name
        assert callable(getattr(ops, name + "_fake")), f"the fake of vitpe::{name} has a name of its own"


# ---- the references are right -------------------------------------------------------------------------------------------
def test_attention_reference_equals_the_oracle():
    """ops_ref's attention on a shared case: to 1e-12 against O.attention_core composed by hand in float64 (the same
    arithmetic, restated once more), and to fp32 accuracy against oracle_attn of test_kernels_gpu.py (the fp32 oracle the
    kernel tests use) on the attention output and d qkv."""
    from test_kernels_gpu import oracle_attn
    for mode in R.ATTN_MODES:
        c = R.attn_case("a", mode, True)
        y, g = R.attention_ref(c)
        lv, pe = R.attention_operands64(c)
        fc, bias = R.pe_operands64(c.mode, c.N, c.H, pe)
        B, N, D, H, hd = c.B, c.N, c.D, c.H, c.hd
        qkv = (lv["xn"] @ lv["wqkv"].t()).reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
        a = O.attention_core(qkv[0], qkv[1], qkv[2], hd ** -0.5, fc, bias).transpose(1, 2).reshape(B, N, D)
        y2 = lv["resid"] + a @ lv["wproj"].t() + lv["bproj"]
        assert rel_err(y2.detach(), y) < 1e-12, mode
        # against the fp32 oracle: identity projection, so that y is the attention output and dy the gradient it receives
        eye = torch.eye(D, dtype=R.F64)
        fc, bias = R.pe_operands64(c.mode, c.N, c.H, {k: v.detach() for k, v in pe.items()})
        xl = R.leaf(R.q64(c.xn, c.dt))
        qkv_l = (xl @ R.q64(c.wqkv, c.dt).t()).detach().requires_grad_(True)
        qh = qkv_l.reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
        out = O.attention_core(qh[0], qh[1], qh[2], hd ** -0.5, fc, bias).transpose(1, 2).reshape(B, N, D) @ eye
        out.backward(R.q64(c.dy, c.dt))
        ref_out, ref_dqkv, _ = oracle_attn(mode, c.xn, c.wqkv, c.dy, c.pe, H, c.dt)
        assert rel_err(ref_out, out.detach()) < 5e-6 and rel_err(ref_dqkv, qkv_l.grad) < 5e-6, mode


def test_plain_references_equal_torch_functional():
    c = R.mlp_case((2, 26, 64), 256, "f32", True)
    x, w1, b1, w2, b2, res = (R.f64(t) for t in (c.xn, c.w1, c.b1, c.w2, c.b2, c.resid))
    y, h, u = R.mlp(x, w1, b1, w2, b2, res)
    want = res + F.linear(F.gelu(F.linear(x, w1, b1)), w2, b2)
    assert rel_err(y, want) < 1e-12 and rel_err(y, res + O.mlp(x, w1, b1, w2, b2)) < 1e-12
    assert rel_err(h, F.gelu(u)) < 1e-12 and rel_err(u, F.linear(x, w1, b1).reshape(-1, 256)) < 1e-12
    c = R.ln_case((2, 26, 64), "f32")
    assert rel_err(R.layer_norm_y(R.f64(c.x), R.f64(c.weight), R.f64(c.bias), c.eps),
                   F.layer_norm(R.f64(c.x), (64,), R.f64(c.weight), R.f64(c.bias), c.eps)) < 1e-12
    c = R.head_case(3, 26, 64, 10, "f32")
    want = F.linear(F.layer_norm(R.f64(c.x), (64,), R.f64(c.gamma), R.f64(c.beta), c.eps)[:, 0], R.f64(c.wh), R.f64(c.bh))
    assert rel_err(R.head(R.f64(c.x), R.f64(c.gamma), R.f64(c.beta), R.f64(c.wh), R.f64(c.bh), c.eps), want) < 1e-12
    c = R.ce_case()
    loss, dlog = R.cross_entropy_ref(c)
    lg = R.leaf(R.f64(c.logits))
    (R.CE_UPSTREAM * F.cross_entropy(lg, c.labels)).backward()
    assert abs(float(loss) - float(F.cross_entropy(lg.detach(), c.labels))) < 1e-12 and rel_err(dlog, lg.grad) < 1e-12
    c = R.embed_case(True, "f32")
    tok, patches = R.patch_embed(R.f64(c.images), R.f64(c.weight), R.f64(c.bias), R.f64(c.cls_token), R.f64(c.ape), c.patch)
    conv = F.conv2d(R.f64(c.images), R.f64(c.weight), R.f64(c.bias), stride=c.patch).flatten(2).transpose(1, 2)
    assert rel_err(tok[:, 1:], conv + R.f64(c.ape)[:, :c.N - 1]) < 1e-12 and rel_err(tok[:, 0], R.f64(c.cls_token)[0].expand(3, -1)) < 1e-12
    assert rel_err(patches @ R.f64(c.weight).reshape(64, -1).t() + R.f64(c.bias), conv.reshape(-1, 64)) < 1e-12


# ---- ... and sensitive: each defect the GPU tests are aimed at misses their gate by at least 10 x ---------------------------
def miss(defect, ref, gate, what):
    ratio = rel_err(defect, ref) / gate
    assert ratio >= 10.0, f"{what}: the defect is only {ratio:.1f} x the gate {gate:g}; the GPU test could not see it"
    return ratio


@pytest.mark.parametrize("dt,D,H,N", R.RULE_GEOMS)
@pytest.mark.parametrize("enc", R.RULE_ENCODINGS)
def test_rule_defects_miss_the_gate(dt, D, H, N, enc):
    """rotating with the caller's tables under a non-RoPE encoding; dropping the bias when tables are handed to a
    relative / polynomial module"""
    t = R.rule_module_tensors(dt, D, H, N, enc)
    y, g = R.rule_ref(t)
    yr, gr = R.rule_ref(t, rotate=True)
    miss(yr, y, R.OUT_TOL[dt], f"rotated under {enc}: y")
    for k in ("xn", "wqkv", "wproj"):
        miss(gr[k], g[k], R.GRAD_TOL[dt], f"rotated under {enc}: d{k}")
    if t.pe:
        yb, gb = R.rule_ref(t, with_bias=False)
        miss(yb, y, R.OUT_TOL[dt], f"bias dropped under {enc}: y")
        miss(gb["pe"], g["pe"], R.GRAD_TOL[dt], f"bias dropped under {enc}: d pe")


@pytest.mark.parametrize("route,tables,resid", R.TABLE_CASES)
def test_not_rotating_misses_the_gate(route, tables, resid):
    """not rotating under a RoPE encoding that was handed tables"""
    c = R.attn_case(route, "none", resid, tables)
    y, g = R.attention_ref(c)
    lv, _ = R.attention_operands64(c)
    y0 = R.attention_y(lv["xn"], lv["wqkv"], None, lv["wproj"], lv["bproj"], lv["resid"], c.H)
    g0 = R.backward(y0, R.q64(c.dy, c.dt), lv)
    miss(y0.detach(), y, R.OUT_TOL[c.dt], f"route {route}, {tables} tables not applied: y")
    for k in ("xn", "wqkv", "wproj"):
        miss(g0[k], g[k], R.GRAD_TOL[c.dt], f"route {route}, {tables} tables not applied: d{k}")


def test_dropped_dresid_and_ignored_upstream_factor_miss_the_gate():
    for route in R.ROUTES:
        c = R.attn_case(route, "none", True)
        _, g = R.attention_ref(c)
        miss(torch.zeros_like(g["resid"]), g["resid"], R.GRAD_TOL[c.dt], f"attention route {route}: dresid dropped")
    for key in R.MLP_CASES:
        if key[3]:
            _, g = R.mlp_ref(R.mlp_case(*key))
            miss(torch.zeros_like(g["resid"]), g["resid"], R.GRAD_TOL[key[2]], "mlp: dresid dropped")
    c = R.ce_case()
    _, d = R.cross_entropy_ref(c)
    _, d1 = R.cross_entropy_ref(c, upstream=1.0)
    miss(d1, d, R.GRAD_TOL["f32"], "cross_entropy: upstream factor ignored")


def test_attention_tables_fixture(golden):
    """golden/attention_tables.npz is small and holds the four reference outputs and the tables they were handed"""
    import os
    from conftest import GOLDEN
    assert os.path.getsize(os.path.join(GOLDEN, "attention_tables.npz")) < 100 * 1024
    g = golden("attention_tables")
    assert sorted(g.files) == sorted(["cos", "sin"] + [t + "/y" for t in list(R.GOLDEN_TAGS.values()) + ["rope-axial_none"]])
    cos, sin = R.caller_tables(16, 32)
    assert np.array_equal(g["cos"], cos.numpy()) and np.array_equal(g["sin"], sin.numpy())
    assert float(np.abs(np.arctan2(g["sin"], g["cos"])).max()) > 2.0   # order-one angles
