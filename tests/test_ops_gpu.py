"""torch.ops.vitpe.* and the Attention / Mlp / Block modules over them, op by op against the float64 references of
ops_ref.py (computed on the operands the kernels see), at geometries the model goldens do not use.

Gates are the project's, none is new (ops_ref.OUT_TOL / GRAD_TOL): fp32 1e-4 on outputs and 1e-3 on gradients
(test_model_gpu.py), bf16 3e-2, all under rel_err = max|a - b| / max|b|; frequency gradients max(tol, 2e-4)
(test_kernels_gpu.py); the saved h / u of the mlp as outputs.  Bit-equality is asked of what a backward must leave alone
(inputs, saved side outputs), never of weight gradients: gemm_tn and the attention backward accumulate with atomics.

VITPE_OPS_REPORT=<file>: the worst figure per op / dtype / route is written there as JSON lines at exit
(profiles/ops_parity.jsonl holds a passing MI355X run).
"""
import atexit
import json
import os

import pytest
import torch

import ops_ref as R
from conftest import rel_err

pytestmark = pytest.mark.gpu

DT = R.DT
WORST = {}


def note(key, value, gate):
    value = float(value)
    w = WORST.get(key)
    if w is None or not value <= w[0]:
        WORST[key] = (value, gate)
    return value


@atexit.register
def _report():
    path = os.environ.get("VITPE_OPS_REPORT")
    if path and WORST:
        with open(path, "w") as f:
            for k in sorted(WORST):
                f.write(json.dumps({"check": k, "worst": WORST[k][0], "gate": WORST[k][1]}) + "\n")


def close(got, ref, gate, key, what=""):
    """record the figure, print it, then assert it"""
    if got is None:
        raise AssertionError(f"{key} {what}: no gradient came back (None)")
    e = note(key, rel_err(got.detach().float().cpu(), ref), gate)
    print(f"{key} {what}: {e:.3e} (gate {gate:g})")
    assert e < gate, f"{key} {what}: rel_err {e:.3e} >= {gate:g}"


@pytest.fixture(scope="module", autouse=True)
def _device():
    import vitpe.ops  # noqa: F401
    assert torch.cuda.is_available(), "these tests need the MI355X"


def dev(t, dtype=torch.float32, rg=False, transposed=False):
    """a device copy; transposed: the same values as a non-contiguous view (a [N, B, D] tensor transposed to [B, N, D])"""
    if t is None:
        return None
    d = t.cuda().to(dtype).contiguous()
    if transposed:
        d = d.transpose(0, 1).contiguous().transpose(0, 1)
        assert not d.is_contiguous()
    return d.requires_grad_(rg)


def run_backward(y, dy, transposed=False):
    """backpropagate sum(y . dy); transposed: through (y.transpose(0, 1) * w).sum(), which hands the op a non-contiguous dy"""
    if transposed:
        (y.transpose(0, 1) * dy.transpose(0, 1).contiguous()).sum().backward(retain_graph=True)
    else:
        y.backward(dy, retain_graph=True)


ALL = ("x", "w", "pe", "resid")


# ---- attention -----------------------------------------------------------------------------------------------------------
class AttnRun:
    """one forward + backward of vitpe::attention / attention_drop on a case"""

    def __init__(self, c, req=ALL, x_t=False, dy_t=False, backward=True):
        dt = DT[c.dt]
        self.c = c
        T = self.T = {}
        T["xn"] = dev(c.xn, dt, "x" in req, transposed=x_t)
        for k in ("wqkv", "bqkv", "wproj", "bproj"):
            T[k] = dev(getattr(c, k), rg="w" in req)
        T["resid"] = dev(c.resid, dt, "resid" in req)
        T["pe"] = dev(c.pe_param, rg="pe" in req)
        self.inv_freq, self.cos, self.sin = dev(c.pe.get("inv_freq")), dev(c.cos), dev(c.sin)
        self.dy = dev(c.dy, dt)
        mode, grid, _, _, degree, per_head, _, _ = R.op_pe_args(c)
        tail = (c.H, mode, grid, T["pe"], self.inv_freq, degree, per_head, self.cos, self.sin, False)
        if c.one_kernel:
            self.y, self.a, self.qkv = torch.ops.vitpe.attention(T["xn"], T["wqkv"], T["wproj"], T["bproj"], T["resid"], *tail)
        else:
            self.y, self.a, self.qkv = torch.ops.vitpe.attention_drop(T["xn"], T["wqkv"], T["bqkv"], T["wproj"], T["bproj"],
                                                                      T["resid"], *tail, 0.0, 0.0, None)
        self.dy_t = dy_t
        if backward:
            self.backward()

    def backward(self):
        run_backward(self.y, self.dy, self.dy_t)

    def tensors(self):
        """everything a backward must leave alone: the inputs and the saved side outputs"""
        t = {k: v for k, v in self.T.items() if v is not None}
        t.update(a=self.a, qkv=self.qkv, dy=self.dy, y=self.y)
        for k in ("inv_freq", "cos", "sin"):
            if getattr(self, k) is not None:
                t[k] = getattr(self, k)
        return t

    def grads(self):
        return {k: v.grad for k, v in self.T.items() if v is not None}

    def zero(self):
        for v in self.T.values():
            if v is not None:
                v.grad = None


def attn_key(c, op="attention"):
    return f"{op}/{c.dt}/{c.route}:{c.want_route}"


def grad_gate(c, k):
    g = R.GRAD_TOL[c.dt]
    return max(g, R.FREQ_FLOOR) if (k == "pe" and c.mode == "rope-mixed") else g


def check_attention(run, key, what, grads=True):
    c = run.c
    y, g = R.attention_ref(c)
    assert run.y.is_contiguous() and run.a.is_contiguous() and run.y.dtype == DT[c.dt]
    assert tuple(run.qkv.shape) == R.qkv_shape(c.want_route, c.B, c.N, c.D), "the route's saved qkv"
    close(run.y, y, R.OUT_TOL[c.dt], key + "/y", what)
    if grads:
        got = run.grads()
        assert sorted(got) == sorted(g)
        for k in sorted(g):
            close(got[k], g[k], grad_gate(c, k), f"{key}/d{k}", what)


@pytest.mark.parametrize("route,mode,resid", R.ATTN_CASES)
def test_attention_parity(route, mode, resid):
    """y and every gradient (x, both weights, the proj bias, the residual, the PE parameter) on each route and mode"""
    c = R.attn_case(route, mode, resid)
    check_attention(AttnRun(c), attn_key(c), f"{mode} resid={resid}")


@pytest.mark.parametrize("route,tables,resid", R.TABLE_CASES)
def test_attention_parity_with_constant_caller_tables(route, tables, resid):
    c = R.attn_case(route, "none", resid, tables)
    check_attention(AttnRun(c), attn_key(c) + "/tables", f"{tables} resid={resid}")


@pytest.mark.parametrize("route,mode", R.DROP_CASES)
def test_attention_drop_parity_with_a_qkv_bias(route, mode):
    """vitpe::attention_drop at p = 0 with a non-zero qkv bias: the bias epilogue and d bqkv; at N 65 / D 192 bf16 the
    bias takes the op off the fused kernels onto Linear + core"""
    c = R.attn_case(route, mode, True, None, True)
    run = AttnRun(c)
    assert run.grads()["bqkv"] is not None
    check_attention(run, attn_key(c, "attention_drop"), mode)


@pytest.mark.parametrize("x_t,dy_t", [(True, False), (False, True), (True, True)], ids=["x", "dy", "x+dy"])
@pytest.mark.parametrize("route", list(R.ROUTES))
def test_attention_non_contiguous_operands(route, x_t, dy_t):
    c = R.attn_case(route, "relative", True)
    check_attention(AttnRun(c, x_t=x_t, dy_t=dy_t), attn_key(c) + "/strided", f"x_t={x_t} dy_t={dy_t}")


_FULL = {}


def full_run(c):
    """the all-enabled run of a case, once"""
    if c.key not in _FULL:
        _FULL[c.key] = {k: (None if v is None else v.detach().float().cpu()) for k, v in AttnRun(c).grads().items()}
    return _FULL[c.key]


OWNER = {"xn": "x", "wqkv": "w", "bqkv": "w", "wproj": "w", "bproj": "w", "resid": "resid", "pe": "pe"}


@pytest.mark.parametrize("req", ALL)
@pytest.mark.parametrize("route", ["b", "c", "d32", "d16"])
def test_attention_partial_requires_grad(route, req):
    """fine-tuning with frozen parts: the enabled inputs get the gradients of the all-enabled run, the others none"""
    c = R.attn_case(route, "relative", True)
    full = full_run(c)
    got = AttnRun(c, req=(req,)).grads()
    for k, v in got.items():
        if OWNER[k] == req:
            close(v, full[k], grad_gate(c, k), f"{attn_key(c)}/partial/d{k}", f"only {req}")
        else:
            assert v is None, f"{k} does not require grad but received one"


def unchanged(before, run_tensors, what):
    for k, v in run_tensors.items():
        assert torch.equal(before[k], v), f"{what}: the backward changed `{k}`"


def twice(run, gate_of, key):
    """backward leaves inputs and saved tensors bit-equal; a second backward(retain_graph=True) reproduces the first"""
    before = {k: v.detach().clone() for k, v in run.tensors().items()}
    run.backward()
    unchanged(before, run.tensors(), key)
    first = {k: v.detach().clone() for k, v in run.grads().items() if v is not None}
    assert first
    run.zero()
    run.backward()
    unchanged(before, run.tensors(), key + " (second backward)")
    for k, v in first.items():
        close(run.grads()[k], v.float().cpu(), gate_of(k), f"{key}/again/d{k}")


@pytest.mark.parametrize("route,mode", [("a", "relative"), ("b", "polynomial_perhead"), ("c", "rope-mixed"), ("d32", "rope-axial"),
                                        ("d16", "relative"), ("e", "polynomial")])
def test_attention_backward_leaves_things_alone(route, mode):
    c = R.attn_case(route, mode, True)
    twice(AttnRun(c, backward=False), lambda k: grad_gate(c, k), attn_key(c))


# ---- mlp -----------------------------------------------------------------------------------------------------------------
class MlpRun:
    def __init__(self, c, req=ALL, x_t=False, dy_t=False, backward=True):
        dt = DT[c.dt]
        self.c, self.dy_t = c, dy_t
        T = self.T = {"xn": dev(c.xn, dt, "x" in req, transposed=x_t), "resid": dev(c.resid, dt, "resid" in req)}
        for k in ("w1", "b1", "w2", "b2"):
            T[k] = dev(getattr(c, k), rg="w" in req)
        self.dy = dev(c.dy, dt)
        self.y, self.h, self.u = torch.ops.vitpe.mlp(T["xn"], T["w1"], T["b1"], T["w2"], T["b2"], T["resid"])
        if backward:
            self.backward()

    def backward(self):
        run_backward(self.y, self.dy, self.dy_t)

    def tensors(self):
        t = {k: v for k, v in self.T.items() if v is not None}
        t.update(h=self.h, u=self.u, y=self.y, dy=self.dy)
        return t

    grads, zero = AttnRun.grads, AttnRun.zero


def check_mlp(run, what):
    c = run.c
    o, g = R.mlp_ref(c)
    key = f"mlp/{c.dt}/D{c.shape[-1]}"
    for k, v in (("y", run.y), ("h", run.h), ("u", run.u)):
        assert v.is_contiguous()
        close(v, o[k], R.OUT_TOL[c.dt], f"{key}/{k}", what)
    got = run.grads()
    assert sorted(got) == sorted(g)
    for k in sorted(g):
        close(got[k], g[k], R.GRAD_TOL[c.dt], f"{key}/d{k}", what)


@pytest.mark.parametrize("shape,hid,dt,resid", R.MLP_CASES)
def test_mlp_parity(shape, hid, dt, resid):
    check_mlp(MlpRun(R.mlp_case(shape, hid, dt, resid)), f"resid={resid}")


@pytest.mark.parametrize("x_t,dy_t", [(True, False), (False, True)], ids=["x", "dy"])
@pytest.mark.parametrize("dt", list(DT))
def test_mlp_non_contiguous_operands(dt, x_t, dy_t):
    check_mlp(MlpRun(R.mlp_case((3, 65, 192), 768, dt, True), x_t=x_t, dy_t=dy_t), f"x_t={x_t} dy_t={dy_t}")


@pytest.mark.parametrize("req", ["x", "w", "resid"])
@pytest.mark.parametrize("dt", list(DT))
def test_mlp_partial_requires_grad(dt, req):
    c = R.mlp_case((2, 26, 64), 256, dt, True)
    full = MlpRun(c).grads()
    for k, v in MlpRun(c, req=(req,)).grads().items():
        if {"xn": "x", "resid": "resid"}.get(k, "w") == req:
            close(v, full[k].float().cpu(), R.GRAD_TOL[dt], f"mlp/{dt}/partial/d{k}", f"only {req}")
        else:
            assert v is None, f"{k} does not require grad but received one"


@pytest.mark.parametrize("dt", list(DT))
def test_mlp_backward_leaves_things_alone(dt):
    twice(MlpRun(R.mlp_case((3, 65, 192), 768, dt, True), backward=False), lambda k: R.GRAD_TOL[dt], f"mlp/{dt}")


# ---- layer_norm ------------------------------------------------------------------------------------------------------------
class LnRun:
    def __init__(self, c, x_t=False, dy_t=False, backward=True):
        dt = DT[c.dt]
        self.c, self.dy_t = c, dy_t
        self.T = {"x": dev(c.x, dt, True, transposed=x_t), "weight": dev(c.weight, rg=True), "bias": dev(c.bias, rg=True)}
        self.dy = dev(c.dy, dt)
        self.y, self.mean, self.rstd = torch.ops.vitpe.layer_norm(self.T["x"], self.T["weight"], self.T["bias"], c.eps)
        if backward:
            self.backward()

    def backward(self):
        run_backward(self.y, self.dy, self.dy_t)

    def tensors(self):
        return dict(self.T, mean=self.mean, rstd=self.rstd, y=self.y, dy=self.dy)

    grads, zero = AttnRun.grads, AttnRun.zero


@pytest.mark.parametrize("x_t,dy_t", [(False, False), (True, False), (False, True)], ids=["contiguous", "x", "dy"])
@pytest.mark.parametrize("shape,dt", R.LN_CASES)
def test_layer_norm_parity(shape, dt, x_t, dy_t):
    c = R.ln_case(shape, dt)
    run = LnRun(c, x_t, dy_t)
    o, g = R.layer_norm_ref(c)
    key = f"layer_norm/{dt}/D{shape[-1]}"
    assert run.y.is_contiguous()
    close(run.y, o["y"], R.OUT_TOL[dt], key + "/y")
    close(run.mean, o["mean"], R.OUT_TOL["f32"], key + "/mean")   # (the statistics are fp32 in both modes)
    close(run.rstd, o["rstd"], R.OUT_TOL["f32"], key + "/rstd")
    for k in sorted(g):
        close(run.grads()[k], g[k], R.GRAD_TOL[dt], f"{key}/d{k}")


@pytest.mark.parametrize("dt", list(DT))
def test_layer_norm_backward_leaves_things_alone(dt):
    twice(LnRun(R.ln_case((3, 65, 192), dt), backward=False), lambda k: R.GRAD_TOL[dt], f"layer_norm/{dt}")


# ---- head, cross_entropy -----------------------------------------------------------------------------------------------------
class HeadRun:
    def __init__(self, c, req=ALL, x_t=False, backward=True):
        self.c = c
        T = self.T = {"x": dev(c.x, DT[c.dt], "x" in req, transposed=x_t)}
        for k in ("gamma", "beta", "wh", "bh"):
            T[k] = dev(getattr(c, k), rg="w" in req)
        self.dy = dev(c.dlogits)
        self.logits, *self.ws = torch.ops.vitpe.head(T["x"], T["gamma"], T["beta"], T["wh"], T["bh"], c.eps)
        if backward:
            self.backward()

    def backward(self):
        self.logits.backward(self.dy, retain_graph=True)

    def tensors(self):
        return dict(self.T, logits=self.logits, xhat=self.ws[0], yn=self.ws[1], rstd=self.ws[2], dy=self.dy)

    grads, zero = AttnRun.grads, AttnRun.zero


@pytest.mark.parametrize("x_t", [False, True], ids=["contiguous", "x"])
@pytest.mark.parametrize("B,N,D,C,dt", R.HEAD_CASES)
def test_head_parity(B, N, D, C, dt, x_t):
    c = R.head_case(B, N, D, C, dt)
    run = HeadRun(c, x_t=x_t)
    logits, g = R.head_ref(c)
    close(run.logits, logits, R.OUT_TOL[dt], f"head/{dt}/logits")
    got = run.grads()
    assert got["x"].dtype == DT[dt] and float(got["x"][:, 1:].abs().max()) == 0.0   # only the class row feeds the head
    for k in sorted(g):
        close(got[k], g[k], R.GRAD_TOL[dt], f"head/{dt}/d{k}")


@pytest.mark.parametrize("req", ["x", "w"])
@pytest.mark.parametrize("B,N,D,C,dt", R.HEAD_CASES)
def test_head_partial_requires_grad(B, N, D, C, dt, req):
    c = R.head_case(B, N, D, C, dt)
    full = HeadRun(c).grads()
    for k, v in HeadRun(c, req=(req,)).grads().items():
        if ("x" if k == "x" else "w") == req:
            close(v, full[k].float().cpu(), R.GRAD_TOL[dt], f"head/{dt}/partial/d{k}", f"only {req}")
        else:
            assert v is None, f"{k} does not require grad but received one"


@pytest.mark.parametrize("B,N,D,C,dt", R.HEAD_CASES)
def test_head_backward_leaves_things_alone(B, N, D, C, dt):
    twice(HeadRun(R.head_case(B, N, D, C, dt), backward=False), lambda k: R.GRAD_TOL[dt], f"head/{dt}")


@pytest.mark.parametrize("t", [False, True], ids=["contiguous", "transposed"])
def test_cross_entropy_through_an_upstream_factor(t):
    """the backward is dlog * dloss: 0.37 * loss is backpropagated, so an ignored upstream factor is a 170 % error"""
    c = R.ce_case()
    loss_ref, d_ref = R.cross_entropy_ref(c)
    logits = (c.logits.t().contiguous().cuda().t() if t else c.logits.cuda()).requires_grad_(True)
    assert logits.is_contiguous() != t
    labels = c.labels.cuda()
    loss, dlog = torch.ops.vitpe.cross_entropy(logits, labels)
    saved = dlog.clone()
    close(loss, loss_ref, R.OUT_TOL["f32"], "cross_entropy/f32/loss")
    for again in (False, True):
        logits.grad = None
        (R.CE_UPSTREAM * loss).backward(retain_graph=True)
        close(logits.grad, d_ref, R.GRAD_TOL["f32"], "cross_entropy/f32/dlogits", f"again={again}")
        assert torch.equal(dlog, saved) and torch.equal(logits.detach().cpu(), c.logits) and torch.equal(labels.cpu(), c.labels)


# ---- patch_embed -----------------------------------------------------------------------------------------------------------
class EmbedRun:
    def __init__(self, c, channels_last=False, backward=True):
        self.c = c
        im = c.images.cuda()
        self.images = im.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2) if channels_last else im
        self.T = {k: dev(getattr(c, k), rg=True) for k in ("weight", "bias", "cls_token", "ape")}
        T = self.T
        self.dy = dev(c.dtok, DT[c.dt])
        self.tok, self.patches = torch.ops.vitpe.patch_embed(self.images, T["weight"], T["bias"], T["cls_token"], T["ape"],
                                                             c.patch, c.dt == "bf16")
        if backward:
            self.backward()

    def backward(self):
        self.tok.backward(self.dy, retain_graph=True)

    def tensors(self):
        t = {k: v for k, v in self.T.items() if v is not None}
        t.update(images=self.images, tok=self.tok, patches=self.patches, dy=self.dy)
        return t

    grads, zero = AttnRun.grads, AttnRun.zero


@pytest.mark.parametrize("channels_last", [False, True], ids=["contiguous", "channels_last"])
@pytest.mark.parametrize("ape,dt", R.EMBED_CASES)
def test_patch_embed_parity(ape, dt, channels_last):
    c = R.embed_case(ape, dt)
    run = EmbedRun(c, channels_last)
    o, g = R.patch_embed_ref(c)
    key = f"patch_embed/{dt}/{'ape' if ape else 'plain'}"
    assert run.tok.dtype == DT[dt] and run.patches.dtype == DT[dt]
    close(run.tok, o["tok"], R.OUT_TOL[dt], key + "/tokens")
    assert torch.equal(run.patches.float().cpu().double(), o["patches"]), "the patch matrix is a gather: exact"
    got = {k: v for k, v in run.grads().items()}
    assert sorted(got) == sorted(g)
    for k in sorted(g):
        assert got[k].shape == getattr(c, k).shape
        close(got[k], g[k], R.GRAD_TOL[dt], f"{key}/d{k}")
    if ape:   # the rows of the table past the token count receive exactly nothing
        assert float(got["ape"][0, c.N - 1:].abs().max()) == 0.0


@pytest.mark.parametrize("dt", list(DT))
def test_patch_embed_backward_leaves_things_alone(dt):
    twice(EmbedRun(R.embed_case(True, dt), backward=False), lambda k: R.GRAD_TOL[dt], f"patch_embed/{dt}")


def test_images_that_require_grad_are_refused():
    """vitpe::patch_embed returns no gradient for `images` (the reference never differentiates them): the model says so
    instead of leaving images.grad None"""
    from models.vit import VisionTransformer
    m = VisionTransformer(img_size=20, patch_size=4, embed_dim=64, depth=1, num_heads=2, pos_encoding="none").cuda()
    x = torch.randn(2, 3, 20, 20, device="cuda")
    assert m(x).shape == (2, 10)
    with pytest.raises(NotImplementedError, match="images"):
        m(x.clone().requires_grad_(True))
    with torch.no_grad():   # nothing is differentiated: nothing to refuse
        assert m(x.clone().requires_grad_(True)).shape == (2, 10)


# ---- torch.library.opcheck ---------------------------------------------------------------------------------------------------
OPCHECK = ("test_schema", "test_autograd_registration", "test_faketensor", "test_aot_dispatch_static")
# static, not dynamic: the route is a function of the concrete shape and the fakes specialise on it.  atol / rtol: the fp32
# gradient gate -- eager and compiled weight gradients differ by the order of their atomics
OPTOL = dict(atol=R.GRAD_TOL["f32"], rtol=R.GRAD_TOL["f32"])


def opcheck(op, args, utils=OPCHECK):
    res = torch.library.opcheck(op, args, test_utils=utils, **OPTOL)
    assert all(v == "SUCCESS" for v in res.values()), res


def rng_pairs(n):
    from vitpe import kernels as K
    return K.new_rng_pairs(n, torch.device("cuda"))


@pytest.mark.parametrize("route,mode", [("a", "relative"), ("b", "rope-mixed"), ("c", "polynomial"), ("d32", "rope-axial"),
                                        ("e", "none")])
def test_opcheck_attention(route, mode):
    c = R.attn_case(route, mode, True)
    r = AttnRun(c, backward=False)
    T = r.T
    mode_, grid, _, _, degree, per_head, _, _ = R.op_pe_args(c)
    opcheck(torch.ops.vitpe.attention, (T["xn"], T["wqkv"], T["wproj"], T["bproj"], T["resid"], c.H, mode_, grid, T["pe"],
                                        r.inv_freq, degree, per_head, None, None, False))


@pytest.mark.parametrize("route,mode,attn_p,proj_p", [("d32", "relative", 0.0, 0.0), ("b", "rope-mixed", 0.2, 0.1)])
def test_opcheck_attention_drop(route, mode, attn_p, proj_p):
    c = R.attn_case(route, mode, True, None, True)
    r = AttnRun(c, backward=False)
    T = r.T
    mode_, grid, _, _, degree, per_head, _, _ = R.op_pe_args(c)
    rng = rng_pairs(2) if attn_p > 0 else None
    opcheck(torch.ops.vitpe.attention_drop, (T["xn"], T["wqkv"], T["bqkv"], T["wproj"], T["bproj"], T["resid"], c.H, mode_, grid,
                                             T["pe"], r.inv_freq, degree, per_head, None, None, False, attn_p, proj_p, rng))


def test_opcheck_attention_with_differentiable_tables():
    c = R.attn_case("a", "none", False, "per_head")   # (tables that require grad: Linear + core, also at this geometry)
    r = AttnRun(c, backward=False)
    T = r.T
    cos, sin = r.cos.clone().requires_grad_(True), r.sin.clone().requires_grad_(True)
    opcheck(torch.ops.vitpe.attention, (T["xn"], T["wqkv"], T["wproj"], T["bproj"], None, c.H, 5, c.grid, None, None, 0, False,
                                        cos, sin, True))


@pytest.mark.parametrize("cls_only", [False, True])
def test_opcheck_attention_probs(cls_only):
    c = R.attn_case("d16", "relative", False)
    qkv = dev(R.rnd(c.B, c.N, 3 * c.D, seed=3), DT[c.dt])
    opcheck(torch.ops.vitpe.attention_probs, (qkv, c.H, 2, c.grid, dev(c.pe_param), None, 0, False, None, None, cls_only),
            utils=("test_schema", "test_faketensor", "test_aot_dispatch_static"))   # (no autograd is registered: a constant)


@pytest.mark.parametrize("dt,p", [("f32", 0.0), ("bf16", 0.0), ("f32", 0.25)])
def test_opcheck_mlp(dt, p):
    r = MlpRun(R.mlp_case((2, 26, 64), 256, dt, True), backward=False)
    T = r.T
    opcheck(torch.ops.vitpe.mlp, (T["xn"], T["w1"], T["b1"], T["w2"], T["b2"], T["resid"], p, rng_pairs(2) if p > 0 else None))


@pytest.mark.parametrize("dt", list(DT))
def test_opcheck_layer_norm_head_cross_entropy(dt):
    r = LnRun(R.ln_case((2, 26, 64), dt), backward=False)
    opcheck(torch.ops.vitpe.layer_norm, (r.T["x"], r.T["weight"], r.T["bias"], 1e-5))
    h = HeadRun(R.head_case(3, 26, 64, 10, dt), backward=False)
    opcheck(torch.ops.vitpe.head, (h.T["x"], h.T["gamma"], h.T["beta"], h.T["wh"], h.T["bh"], 1e-5))
    c = R.ce_case()
    opcheck(torch.ops.vitpe.cross_entropy, (c.logits.cuda().requires_grad_(True), c.labels.cuda()))


@pytest.mark.parametrize("name", ["dropout", "drop_path"])
@pytest.mark.parametrize("dt", list(DT))
def test_opcheck_dropout_and_drop_path(name, dt):
    c = R.ln_case((2, 26, 64), dt)
    x, res = dev(c.x, DT[dt], True), dev(c.dy, DT[dt], True)
    for resid in (None, res):
        opcheck(getattr(torch.ops.vitpe, name), (x, resid, 0.25, rng_pairs(1)[0]))


@pytest.mark.parametrize("ape,dt", [(True, "f32"), (False, "bf16")])
def test_opcheck_patch_embed(ape, dt):
    r = EmbedRun(R.embed_case(ape, dt), backward=False)
    T = r.T
    opcheck(torch.ops.vitpe.patch_embed, (r.images, T["weight"], T["bias"], T["cls_token"], T["ape"], r.c.patch, dt == "bf16"))


# ---- the caller-table rule, module level (reference vit.py:51, 73-81) ------------------------------------------------------
def rule_module(t, enc):
    from models.vit import Attention
    from models import positional_encoding as pe
    att = Attention(t.D, num_heads=t.H)
    P = t.N - 1
    pos = {"None": lambda: None, "absolute": lambda: pe.AbsolutePositionalEncoding(t.D, max_len=P + 7),
           "relative": lambda: pe.RelativePositionalEncoding(P, num_heads=t.H),
           "polynomial": lambda: pe.PolynomialRPE(P, 3, t.H, shared_across_heads=True),
           "polynomial_perhead": lambda: pe.PolynomialRPE(P, 3, t.H, shared_across_heads=False),
           "rope-axial": lambda: pe.RoPEAxial(t.hd, 100.0), "rope-mixed": lambda: pe.RoPEMixed(t.hd, t.H, 100.0)}[enc]()
    att.set_pos_encoding(pos)
    with torch.no_grad():
        att.qkv.weight.copy_(t.wqkv), att.proj.weight.copy_(t.wproj), att.proj.bias.copy_(t.bproj)
        if enc == "relative":
            pos.relative_position_bias_table.copy_(t.pe["table"])
        elif enc.startswith("polynomial"):
            pos.coefficients.copy_(t.pe["coeff"])
    att.cuda()
    param = {"relative": lambda: pos.relative_position_bias_table, "polynomial": lambda: pos.coefficients,
             "polynomial_perhead": lambda: pos.coefficients}.get(enc, lambda: None)()
    return att, param


def check_rule(att, param, t, y_ref, g_ref, freqs_cis, key):
    dt = t.dt
    x = dev(t.x, DT[dt], True)
    y = att(x, freqs_cis=freqs_cis)
    close(y, y_ref, R.OUT_TOL[dt], key + "/y")
    y.backward(dev(t.dy, DT[dt]))
    got = {"xn": x.grad, "wqkv": att.qkv.weight.grad, "wproj": att.proj.weight.grad, "bproj": att.proj.bias.grad}
    if param is not None:
        got["pe"] = param.grad
    for k in sorted(got):
        close(got[k], g_ref[k], R.GRAD_TOL[dt], f"{key}/d{k}")


@pytest.mark.parametrize("enc", R.RULE_ENCODINGS)
@pytest.mark.parametrize("dt,D,H,N", R.RULE_GEOMS)
def test_caller_tables_under_an_encoding_that_is_not_rotary(dt, D, H, N, enc):
    """Attention handed (cos, sin) under pos_encoding None / absolute / relative / polynomial: the reference never looks at
    them (vit.py:51) and still adds the bias (vit.py:73-81) -- y, dx, dWqkv, dWproj, dbproj and the bias parameter's
    gradient equal the UNROTATED float64 reference with the bias added; a mis-shaped table is not looked at either."""
    t = R.rule_module_tensors(dt, D, H, N, enc)
    att, param = rule_module(t, enc)
    y_ref, g_ref = R.rule_ref(t)
    key = f"rule/{dt}/{enc}"
    cos, sin = t.cos.cuda(), t.sin.cuda()
    check_rule(att, param, t, y_ref, g_ref, (cos, sin), key)
    with torch.no_grad():
        x = dev(t.x, DT[dt])
        y0 = att(x, freqs_cis=None)
        assert torch.equal(att(x, freqs_cis=(cos, sin)), y0), "the tables changed the output"
        assert torch.equal(att(x, freqs_cis=(cos[:, :-1], sin[:, :-1])), y0), "a table the reference never reads was shape-checked"
        assert torch.equal(att(x, freqs_cis=(N - 1,)), y0)
        # attention_probs follows the same rule
        p = att.attention_probs(x, freqs_cis=(cos, sin))
        assert torch.equal(p, att.attention_probs(x, freqs_cis=None))
        qkv = R.q64(t.x, dt) @ R.q64(t.wqkv, dt).t()
        qh = qkv.reshape(t.B, N, 3, H, t.hd).permute(2, 0, 3, 1, 4)
        _, bias = R.pe_operands64(t.mode, N, H, {k: R.f64(v) for k, v in t.pe.items()})
        s = (qh[0] @ qh[1].transpose(-2, -1)) * t.hd ** -0.5
        p_ref = (s if bias is None else s + bias).softmax(-1)
        close(p, p_ref, R.OUT_TOL[dt], key + "/probs")


@pytest.mark.parametrize("enc", ["rope-axial", "rope-mixed"])
@pytest.mark.parametrize("dt,D,H,N", R.RULE_GEOMS)
def test_rotary_module_without_freqs_cis_is_plain_attention(dt, D, H, N, enc):
    t = R.rule_module_tensors(dt, D, H, N, "None")
    att, _ = rule_module(t, enc)
    y_ref, g_ref = R.rule_ref(t)
    check_rule(att, None, t, y_ref, g_ref, None, f"rule/{dt}/{enc}:no-tables")
    # ... and handed tables it rotates with them (the other half of the rule)
    y_rot, g_rot = R.rule_ref(t, rotate=True)
    att.zero_grad()
    check_rule(att, None, t, y_rot, g_rot, (t.cos.cuda(), t.sin.cuda()), f"rule/{dt}/{enc}:tables")
    with torch.no_grad():
        x = dev(t.x, DT[dt])
        assert torch.equal(att.attention_probs(x, freqs_cis=None), rule_module(t, "None")[0].attention_probs(x))


@pytest.mark.parametrize("enc", ["None", "relative", "polynomial", "rope-axial"])
def test_caller_table_rule_against_the_reference_s_own_numbers(golden, enc):
    """fp32 y of the module on the closed-form tensors against golden/attention_tables.npz, written by the reference's own
    Attention.forward"""
    g = golden("attention_tables")
    D, H, N, B = 64, 2, 17, 2
    gi = R.golden_attention_inputs(D, H, N, B)
    t = R.rule_module_tensors("f32", D, H, N, enc if enc != "rope-axial" else "None")
    t.wqkv, t.wproj, t.bproj = gi["wqkv"], gi["wproj"], gi["bproj"]
    t.pe = {"relative": {"table": gi["table"]}, "polynomial": {"coeff": gi["coeff"]}}.get(enc, {})
    att, _ = rule_module(t, enc)
    cos, sin = torch.from_numpy(g["cos"]).cuda(), torch.from_numpy(g["sin"]).cuda()
    with torch.no_grad():
        y = att(gi["x"].cuda(), freqs_cis=None if enc == "rope-axial" else (cos, sin))
    tag = "rope-axial_none" if enc == "rope-axial" else R.GOLDEN_TAGS[enc]
    close(y, g[tag + "/y"], R.OUT_TOL["f32"], f"rule/golden/{tag}")


def test_block_with_caller_tables_on_a_relative_block():
    """Block(x, freqs_cis=(cos, sin)) on a relative block used to raise; it is the block without the tables"""
    from models.vit import Block
    from models import positional_encoding as pe
    D, H, N = 64, 2, 17
    torch.manual_seed(3)
    blk = Block(D, H)
    pos = pe.RelativePositionalEncoding(N - 1, num_heads=H)
    blk.set_pos_encoding(pos)
    blk.cuda()
    x = torch.randn(2, N, D, device="cuda")
    cos, sin = (v.cuda() for v in R.caller_tables(N - 1, D // H))
    with torch.no_grad():
        y = blk(x, freqs_cis=(cos, sin))
        assert torch.equal(y, blk(x)) and torch.isfinite(y).all()
        assert torch.equal(blk.attention_probs(x, freqs_cis=(cos, sin)), blk.attention_probs(x))
