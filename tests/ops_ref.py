"""Float64 references and case lists of the torch.ops.vitpe.* tests (test_ops_cpu.py, test_ops_gpu.py).

Every reference is a plain torch restatement of one op in float64 with autograd-derived gradients, computed on the
operands the kernels see: in bf16 mode the activations, the upstream gradient and the GEMM weights (the shadows the ops
cast on the fly) are rounded to bf16 first, as q() / oracle_attn do in test_kernels_gpu.py; biases, LayerNorm and head
parameters and positional-encoding leaves stay the fp32 masters the kernels read.  The attention arithmetic is the
oracle's (oracle.vit_oracle: attention_core, relative_bias, polynomial_bias, rope_*_tables), not restated.

Case lists: the smallest shapes that still reach each route of the ops ("What the op tests pin").  route_of()
derives the route of a geometry from the library's pure host predicates, the same calls vitpe/ops.py branches on, and
every attention case asserts that it still lies on the route it is listed under.
"""
import functools
import math
import types

import torch
import torch.nn.functional as F

from oracle import vit_oracle as O

F64 = torch.float64
DT = {"f32": torch.float32, "bf16": torch.bfloat16}

# the project's gates (test_model_gpu.py, test_kernels_gpu.py): rel_err = max|a - b| / max|b|
OUT_TOL = {"f32": 1e-4, "bf16": 3e-2}     # forward outputs (and the saved h / u of the mlp)
GRAD_TOL = {"f32": 1e-3, "bf16": 3e-2}    # gradients
FREQ_FLOOR = 2e-4                         # frequency gradients: max(tol, 2e-4)

ATTN_MODES = ["none", "relative", "polynomial", "polynomial_perhead", "rope-axial", "rope-mixed"]
OP_MODE = {"none": 0, "absolute": 1, "relative": 2, "polynomial": 3, "polynomial_perhead": 3, "rope-axial": 4, "rope-mixed": 5}


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def q64(t, dt):
    """the values a kernel sees of an operand it reads in the compute type, in float64"""
    return None if t is None else t.detach().to(DT[dt]).to(F64)


def f64(t):
    return None if t is None else t.detach().to(F64)


def leaf(t):
    return None if t is None else t.clone().requires_grad_(True)


def backward(out, dy, leaves):
    """-> {name: d sum(out . dy) / d leaf} for the leaves that are tensors"""
    names = [k for k, v in leaves.items() if v is not None]
    gs = torch.autograd.grad(out, [leaves[k] for k in names], dy, allow_unused=True)
    return {k: (torch.zeros_like(leaves[k]) if g is None else g) for k, g in zip(names, gs)}


# ---- routes of vitpe::attention -----------------------------------------------------------------------------------------
B_ATTN = 3   # odd: the idle second image slot of the last two-image workgroup
ROUTES = {   # name: (dtype, N, D, H, route)
    "a": ("f32", 65, 96, 3, "fused16"),       # the kernel that keeps qkv on the chip, 16x16 tiles
    "b": ("bf16", 65, 192, 6, "wide32"),      # the same route, 32x32-tile forward kernel
    "c": ("bf16", 197, 128, 2, "fused64"),    # projection + PE + core in one kernel, qkv its side output
    "d32": ("f32", 26, 64, 2, "core"),        # qkv Linear + attention core
    "d16": ("bf16", 26, 64, 2, "core"),
    "e": ("f32", 197, 128, 2, "core"),
}


def route_of(dt, N, D, H, one_kernel=True, tables_grad=False):
    """The branch _attention_forward takes, from the library's host predicates alone (no device needed)."""
    from vitpe import _lib as L
    h, code, hd = L.lib(), L.dtype_code(DT[dt]), D // H
    if one_kernel and not tables_grad and h.vitpe_fused_attention_supported(code, N, D, hd):
        return "wide32" if h.vitpe_fused_attention_wide_supported(code, N, D, hd) else "fused16"
    if one_kernel and not tables_grad and h.vitpe_attention_fused64_supported(code, N, H, hd):
        return "fused64"
    assert h.vitpe_attention_core_supported(code, N, hd), (dt, N, D, H)
    return "core"


def qkv_shape(route, B, N, D):
    """what the real op returns as `qkv` (the backward dispatches on its numel)"""
    return (0,) if route in ("fused16", "wide32") else (B, N, 3 * D)


def caller_tables(P, hd, H=None):
    """constant rotary tables that are not any module's own (angles up to 2.5 rad, as
    test_attention_uses_the_callers_rotary_tables): [P, hd/2], or [H, P, hd/2] with H"""
    ang = torch.linspace(0.0, 2.5, P * (hd // 2)).reshape(P, hd // 2) ** 1.3
    if H is not None:
        ang = torch.stack([ang * (1 + 0.1 * h) for h in range(H)])
    return torch.cos(ang), torch.sin(ang)


def pe_leaves(mode, N, H, hd, seed, gain=1.0, degree=3):
    """the positional-encoding operands of a mode (as attn_case in test_kernels_gpu.py); gain: a factor on the bias
    parameters; degree: of the polynomial modes (coefficient k scaled by 8^-k)"""
    pe = {}
    if mode == "relative":
        pe["table"] = rnd(H, 2 * N - 1, seed=seed + 4, scale=0.5 * gain)
    elif mode.startswith("polynomial"):
        shp = (degree + 1,) if mode == "polynomial" else (H, degree + 1)
        pe["coeff"] = rnd(*shp, seed=seed + 5, scale=0.4 * gain) * torch.tensor([1.0 / 8 ** k for k in range(degree + 1)])
    elif mode == "rope-axial":
        pe["inv_freq"] = O.rope_axial_inv_freq(hd, 100.0)
    elif mode == "rope-mixed":
        pe["freqs"] = rnd(2, H, hd // 2, seed=seed + 6, scale=0.7)
    return pe


@functools.lru_cache(maxsize=None)
def attn_case(route, mode, resid, tables=None, qkv_bias=False, one_kernel=True, degree=3):
    """One attention case: fp32 CPU operands and the geometry.  tables: None | "shared" ([P, hd/2]) | "per_head"
    ([H, P, hd/2]) constant caller tables (the mode is then the rotary one of that rank, without parameters).  degree: of
    the polynomial modes."""
    dt, N, D, H, want = ROUTES[route]
    hd, B = D // H, B_ATTN
    if tables is not None:
        mode = "rope-axial" if tables == "shared" else "rope-mixed"
    seed = 1000 * (sorted(ROUTES).index(route) + 1) + 10 * ATTN_MODES.index(mode)
    c = types.SimpleNamespace(route=route, dt=dt, N=N, D=D, H=H, hd=hd, B=B, grid=int(math.isqrt(N - 1)), mode=mode,
                              tables=tables, one_kernel=one_kernel and not qkv_bias, degree=degree)
    assert c.grid * c.grid == N - 1
    c.want_route = want if c.one_kernel else "core"
    got = route_of(dt, N, D, H, one_kernel=c.one_kernel)
    assert got == c.want_route, f"case {route} ({dt}, N {N}, D {D}, H {H}) left its route: {c.want_route} -> {got}"
    c.xn = rnd(B, N, D, seed=seed + 1)
    c.wqkv = rnd(3 * D, D, seed=seed + 2, scale=0.3)
    c.bqkv = rnd(3 * D, seed=seed + 7, scale=0.5) if qkv_bias else None
    c.wproj = rnd(D, D, seed=seed + 8, scale=0.15)
    c.bproj = rnd(D, seed=seed + 9, scale=0.3)
    c.resid = rnd(B, N, D, seed=seed + 10, scale=0.3) if resid else None   # (small: y stays sensitive to the attention term)
    c.dy = rnd(B, N, D, seed=seed + 3)
    c.pe = {} if tables is not None else pe_leaves(mode, N, H, hd, seed, degree=degree)
    c.cos, c.sin = (None, None) if tables is None else caller_tables(N - 1, hd, H if tables == "per_head" else None)
    c.pe_param = c.pe.get("table", c.pe.get("coeff", c.pe.get("freqs")))
    c.key = (route, mode, resid, tables, qkv_bias, one_kernel, degree)
    return c


def op_pe_args(c, pe_param=None, cos=None, sin=None):
    """(mode, grid, pe_param, inv_freq, degree, per_head, cos, sin) of the attention ops for a case; the tensor arguments
    default to the case's CPU ones (pass device copies)"""
    poly = c.mode.startswith("polynomial")
    return (OP_MODE[c.mode], c.grid, pe_param, c.pe.get("inv_freq"), c.degree if poly else 0, c.mode == "polynomial_perhead", cos, sin)


def pe_operands64(mode, N, H, pe, cos=None, sin=None, degree=3):
    """(freqs_cis, bias) of the oracle's attention core in float64; pe: {name: float64 leaf}.  The axial tables are
    built in fp32 like the device's (they are fp32 operands of the kernels, not leaves).  degree: of the polynomial modes."""
    if cos is not None:
        return (f64(cos), f64(sin)), None
    if mode == "relative":
        return None, O.relative_bias(pe["table"], N)
    if mode.startswith("polynomial"):
        return None, O.polynomial_bias(pe["coeff"], N - 1, H, degree, mode == "polynomial")
    if mode == "rope-axial":
        cos, sin = O.rope_axial_tables(N - 1, pe["inv_freq"].float())
        return (f64(cos), f64(sin)), None
    if mode == "rope-mixed":
        return O.rope_mixed_tables(N - 1, pe["freqs"]), None
    return None, None


def attention_y(xn, wqkv, bqkv, wproj, bproj, resid, H, freqs_cis=None, bias=None):
    """y = [resid +] proj(attention(qkv(xn)))  (reference vit.py:43-94), any float type"""
    B, N, D = xn.shape
    hd = D // H
    qkv = F.linear(xn, wqkv, bqkv).reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    o = O.attention_core(qkv[0], qkv[1], qkv[2], hd ** -0.5, freqs_cis, bias).transpose(1, 2).reshape(B, N, D)
    y = F.linear(o, wproj, bproj)
    return y if resid is None else resid + y


def attention_operands64(c):
    """the float64 leaves of a case, rounded as the kernels see them"""
    lv = dict(xn=leaf(q64(c.xn, c.dt)), wqkv=leaf(q64(c.wqkv, c.dt)), bqkv=leaf(f64(c.bqkv)), wproj=leaf(q64(c.wproj, c.dt)),
              bproj=leaf(f64(c.bproj)), resid=leaf(q64(c.resid, c.dt)))
    pe = {k: (leaf(f64(v)) if k != "inv_freq" else v) for k, v in c.pe.items()}
    return lv, pe


@functools.lru_cache(maxsize=None)
def _attention_ref(key):
    c = attn_case(*key)
    lv, pe = attention_operands64(c)
    freqs_cis, bias = pe_operands64(c.mode, c.N, c.H, pe, c.cos, c.sin, c.degree)
    y = attention_y(lv["xn"], lv["wqkv"], lv["bqkv"], lv["wproj"], lv["bproj"], lv["resid"], c.H, freqs_cis, bias)
    leaves = dict(lv)
    if c.pe_param is not None:
        leaves["pe"] = [v for k, v in pe.items() if k != "inv_freq"][0]
    return y.detach(), backward(y, q64(c.dy, c.dt), leaves)


def attention_ref(c):
    """-> (y, {xn, wqkv, [bqkv], wproj, bproj, [resid], [pe]: gradient}) in float64; computed once per case"""
    return _attention_ref(c.key)


ATTN_CASES = [(r, m, res) for r in ROUTES for m in ATTN_MODES for res in (False, True)]
TABLE_CASES = [(r, t, res) for r in ("b", "d32", "d16") for t in ("shared", "per_head") for res in (False, True)]
DROP_CASES = [("d32", "relative"), ("d16", "rope-mixed"), ("b", "none"), ("b", "polynomial_perhead")]   # + a qkv bias, p = 0


# ---- layer_norm ---------------------------------------------------------------------------------------------------------
LN_CASES = [((2, 26, 64), dt) for dt in DT] + [((3, 65, 192), dt) for dt in DT]
LN_EPS = 1e-5


@functools.lru_cache(maxsize=None)
def ln_case(shape, dt):
    D = shape[-1]
    return types.SimpleNamespace(dt=dt, shape=shape, x=rnd(*shape, seed=11, scale=2.0) + 0.3, weight=1 + 0.1 * rnd(D, seed=12),
                                 bias=0.1 * rnd(D, seed=13), dy=rnd(*shape, seed=14), eps=LN_EPS, key=(shape, dt))


def layer_norm_y(x, weight, bias, eps):
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * weight + bias


@functools.lru_cache(maxsize=None)
def _layer_norm_ref(key):
    c = ln_case(*key)
    lv = dict(x=leaf(q64(c.x, c.dt)), weight=leaf(f64(c.weight)), bias=leaf(f64(c.bias)))
    y = layer_norm_y(lv["x"], lv["weight"], lv["bias"], c.eps)
    x = lv["x"].detach()
    mean = x.mean(-1).reshape(-1)
    rstd = (1.0 / torch.sqrt(((x - x.mean(-1, keepdim=True)) ** 2).mean(-1) + c.eps)).reshape(-1)
    return dict(y=y.detach(), mean=mean, rstd=rstd), backward(y, q64(c.dy, c.dt), lv)


def layer_norm_ref(c):
    return _layer_norm_ref(c.key)


# ---- mlp ----------------------------------------------------------------------------------------------------------------
MLP_CASES = [(shape, hid, dt, res) for shape, hid in (((2, 26, 64), 256), ((3, 65, 192), 768)) for dt in DT for res in (False, True)]


@functools.lru_cache(maxsize=None)
def mlp_case(shape, hid, dt, resid):
    D = shape[-1]
    return types.SimpleNamespace(dt=dt, shape=shape, hid=hid, xn=rnd(*shape, seed=21), w1=rnd(hid, D, seed=22, scale=0.2),
                                 b1=rnd(hid, seed=23, scale=0.5), w2=rnd(D, hid, seed=24, scale=0.1), b2=rnd(D, seed=25, scale=0.3),
                                 resid=rnd(*shape, seed=26) if resid else None, dy=rnd(*shape, seed=27),
                                 key=(shape, hid, dt, resid))


def gelu_erf(u):
    return 0.5 * u * (1.0 + torch.erf(u / math.sqrt(2.0)))


def mlp(xn, w1, b1, w2, b2, resid=None):
    """-> (y, h, u): u = fc1(xn), h = GELU_erf(u), y = [resid +] fc2(h)   (timm Mlp, reference vit.py:118,124)"""
    u = xn.reshape(-1, xn.shape[-1]) @ w1.t() + b1
    h = gelu_erf(u)
    y = (h @ w2.t() + b2).reshape(xn.shape)
    return (y if resid is None else resid + y), h, u


@functools.lru_cache(maxsize=None)
def _mlp_ref(key):
    c = mlp_case(*key)
    lv = dict(xn=leaf(q64(c.xn, c.dt)), w1=leaf(q64(c.w1, c.dt)), b1=leaf(f64(c.b1)), w2=leaf(q64(c.w2, c.dt)),
              b2=leaf(f64(c.b2)), resid=leaf(q64(c.resid, c.dt)))
    y, h, u = mlp(**lv)
    return dict(y=y.detach(), h=h.detach(), u=u.detach()), backward(y, q64(c.dy, c.dt), lv)


def mlp_ref(c):
    return _mlp_ref(c.key)


# ---- head ---------------------------------------------------------------------------------------------------------------
HEAD_CASES = [(3, 26, 64, 10, dt) for dt in DT]


@functools.lru_cache(maxsize=None)
def head_case(B, N, D, C, dt):
    return types.SimpleNamespace(dt=dt, x=rnd(B, N, D, seed=31, scale=2.0) + 0.3, gamma=1 + 0.1 * rnd(D, seed=32),
                                 beta=0.1 * rnd(D, seed=33), wh=rnd(C, D, seed=34, scale=0.2), bh=rnd(C, seed=35, scale=0.3),
                                 dlogits=rnd(B, C, seed=36), eps=LN_EPS, key=(B, N, D, C, dt))


def head(x, gamma, beta, wh, bh, eps):
    """logits = Linear(LayerNorm(x)[:, 0])   (reference vit.py:284-285)"""
    return layer_norm_y(x, gamma, beta, eps)[:, 0] @ wh.t() + bh


@functools.lru_cache(maxsize=None)
def _head_ref(key):
    c = head_case(*key)
    lv = dict(x=leaf(q64(c.x, c.dt)), gamma=leaf(f64(c.gamma)), beta=leaf(f64(c.beta)), wh=leaf(f64(c.wh)), bh=leaf(f64(c.bh)))
    logits = head(**lv, eps=c.eps)
    return logits.detach(), backward(logits, f64(c.dlogits), lv)


def head_ref(c):
    return _head_ref(c.key)


# ---- cross_entropy ------------------------------------------------------------------------------------------------------
CE_UPSTREAM = 0.37   # the loss is backpropagated through a factor that is not 1: the backward is dlog * dloss


@functools.lru_cache(maxsize=None)
def ce_case(B=5, C=10):
    g = torch.Generator().manual_seed(41)
    return types.SimpleNamespace(logits=rnd(B, C, seed=42, scale=3.0), labels=torch.randint(0, C, (B,), generator=g))


def cross_entropy_ref(c, upstream=CE_UPSTREAM):
    """-> (mean loss, d (upstream * loss) / d logits)   (reference train.py:113,194)"""
    lg = leaf(f64(c.logits))
    loss = -(torch.log_softmax(lg, -1)[torch.arange(len(c.labels)), c.labels]).mean()
    return loss.detach(), torch.autograd.grad(upstream * loss, lg)[0]


# ---- patch_embed --------------------------------------------------------------------------------------------------------
EMBED_CASES = [(ape, dt) for ape in (False, True) for dt in DT]
EMBED_GEOM = dict(B=3, C=3, S=20, p=4, D=64, max_len=40)   # N 26; the APE table is longer than the token count


@functools.lru_cache(maxsize=None)
def embed_case(ape, dt):
    g = EMBED_GEOM
    B, C, S, p, D = g["B"], g["C"], g["S"], g["p"], g["D"]
    N = (S // p) ** 2 + 1
    return types.SimpleNamespace(dt=dt, patch=p, images=rnd(B, C, S, S, seed=51), weight=rnd(D, C, p, p, seed=52, scale=0.2),
                                 bias=rnd(D, seed=53, scale=0.3), cls_token=rnd(1, 1, D, seed=54, scale=0.5),
                                 ape=rnd(1, g["max_len"], D, seed=55, scale=0.5) if ape else None, dtok=rnd(B, N, D, seed=56),
                                 N=N, key=(ape, dt))


def patch_embed(images, weight, bias, cls_token, ape, patch):
    """-> (tokens [B, N, D], patch matrix [B P, C p p]): Conv2d(k = s = p) as unfold + GEMM, class token prepended, the
    APE table added to the patch rows (reference vit.py:245-258, positional_encoding.py:39) -- the oracle's patch_embed"""
    B, C, S, _ = images.shape
    cfg = O.VitConfig(img_size=S, patch_size=patch, in_chans=C, embed_dim=weight.shape[0],
                      pos_encoding="absolute" if ape is not None else "none")
    params = {"patch_embed.weight": weight, "patch_embed.bias": bias, "cls_token": cls_token, "pos_embed.pos_embed": ape}
    g = S // patch
    patches = images.reshape(B, C, g, patch, g, patch).permute(0, 2, 4, 1, 3, 5).reshape(B * g * g, C * patch * patch)
    return O.patch_embed(cfg, params, images), patches


@functools.lru_cache(maxsize=None)
def _patch_embed_ref(key):
    c = embed_case(*key)
    lv = dict(weight=leaf(q64(c.weight, c.dt)), bias=leaf(f64(c.bias)), cls_token=leaf(f64(c.cls_token)), ape=leaf(f64(c.ape)))
    tok, patches = patch_embed(q64(c.images, c.dt), lv["weight"], lv["bias"], lv["cls_token"], lv["ape"], c.patch)
    return dict(tok=tok.detach(), patches=patches), backward(tok, q64(c.dtok, c.dt), lv)


def patch_embed_ref(c):
    return _patch_embed_ref(c.key)


# ---- the caller-table rule, module level (reference vit.py:51, 73-81) ----------------------------------------------------
RULE_GEOMS = [("f32", 64, 2, 17), ("bf16", 192, 6, 65)]   # (dtype, D, H, N)
RULE_B = 2
RULE_ENCODINGS = ["None", "absolute", "relative", "polynomial", "polynomial_perhead"]   # handed (cos, sin): never rotated
GOLDEN_TAGS = {"None": "none_tables", "relative": "relative_tables", "polynomial": "polynomial_tables"}   # + "rope-axial_none"


def rule_module_tensors(dt, D, H, N, enc):
    """random weights of a stand-alone Attention and its encoding's parameter (the closed-form sin() fills cancel in the
    projection, which bf16 cannot follow), the input, the upstream gradient and constant caller tables"""
    hd, B = D // H, RULE_B
    seed = 7000 + D
    t = types.SimpleNamespace(dt=dt, D=D, H=H, N=N, hd=hd, B=B, enc=enc)
    t.x, t.dy = rnd(B, N, D, seed=seed + 1), rnd(B, N, D, seed=seed + 3)
    t.wqkv, t.wproj, t.bproj = rnd(3 * D, D, seed=seed + 2, scale=0.3), rnd(D, D, seed=seed + 8, scale=0.15), rnd(D, seed=seed + 9, scale=0.3)
    mode = {"None": "none", "absolute": "none"}.get(enc, enc)
    t.mode = mode
    t.pe = pe_leaves(mode, N, H, hd, seed, gain=4.0)   # a bias of a few units: leaving it out is an order-one error
    t.cos, t.sin = caller_tables(N - 1, hd)
    return t


def rule_ref(t, rotate=False, with_bias=True):
    """-> (y, {x, wqkv, wproj, bproj, [pe]}) of the module under the rule: unrotated, the module's bias added.  rotate /
    with_bias = False restate the two ways of getting it wrong (test_ops_cpu.py measures how far off they are)."""
    lv = dict(xn=leaf(q64(t.x, t.dt)), wqkv=leaf(q64(t.wqkv, t.dt)), wproj=leaf(q64(t.wproj, t.dt)), bproj=leaf(f64(t.bproj)))
    pe = {k: (leaf(f64(v)) if k != "inv_freq" else v) for k, v in t.pe.items()}
    freqs_cis, bias = pe_operands64(t.mode, t.N, t.H, pe)
    if rotate:
        freqs_cis = (f64(t.cos), f64(t.sin))
    if not with_bias:
        bias = None
    y = attention_y(lv["xn"], lv["wqkv"], None, lv["wproj"], lv["bproj"], None, t.H, freqs_cis, bias)
    leaves = dict(lv)
    for k, v in pe.items():
        if k != "inv_freq":
            leaves["pe"] = v
    return y.detach(), backward(y, q64(t.dy, t.dt), leaves)


def golden_attention_inputs(D=64, H=2, N=17, B=2):
    """the closed-form tensors of golden/attention_tables.npz (tools/make_golden.py, gen_attention_tables)"""
    CF = O.closed_form_tensor
    return dict(wqkv=CF("attn.qkv.weight", (3 * D, D)), wproj=CF("attn.proj.weight", (D, D)), bproj=CF("attn.proj.bias", (D,)),
                x=CF("attn.x", (B, N, D)) * 20,
                table=CF("pos_embed.relative_position_bias_table", (H, 2 * N - 1)), coeff=CF("pos_embed.coefficients", (4,)))
