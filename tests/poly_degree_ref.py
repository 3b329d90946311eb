"""Float64 reference of the polynomial relative position bias at every degree 0-7 (test_poly_degree_cpu.py,
test_poly_degree_gpu.py), with the coefficient gradient per head and per power and the scale each power is gated against.

The bias of patch pair (i, j) is sum_k c_k d_ij^k of the L1 grid distance d (reference positional_encoding.py:127-171), the
class token's row and column stay zero.  Its coefficient gradient is g_k = sum dS_ij d_ij^k over patch pairs: component k
scales like (grid distance)^k, so one max-norm over the vector checks the top power only.  Here every power is compared on
its own, against
    E_k = sum_{i,j >= 1} P_ij (|dP_ij| + sum_m P_im |dP_im|) d_ij^k,
the size of the terms that fp32 rounding of P, dP and the row dot product acts on (dS = P (dP - sum_m P_im dP_im) is formed
in fp32 in every backward kernel), and -- for random inputs -- against A_k = sum |dS_ij| d_ij^k.

Exact inputs (exact_case): a zero query projection makes the logits the bias alone; V and dO are small integers that bf16
holds exactly, the class token's rows of both weighted by CLS_WEIGHT.  dP is then an exact integer in both compute types
and the bf16 kernels' coefficient gradient carries fp32 error only, so E_k gates them as sharply as the fp32 ones.  The
fused kernels take xn and wqkv: xn is integer and the value projection has three +-1 entries per row.

wrong_variants restates the ways a kernel could be subtly wrong (class row / column not masked -- with the class token's
packed coordinate (0, 0), as the kernels have it --, power k + 1 for k, heads swapped, powers above 3 dropped, a per-head
stride of 4); test_poly_degree_cpu.py shows that every one of them is far outside the gate on every exact case.

Every case is pinned to its kernel by the library's host predicates (pin), as ops_ref.route_of does: a case that leaves its
route fails when the case list is built, at collection.
"""
import functools
import types

import torch

F64 = torch.float64
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
EPS32 = 2.0 ** -23
MAXDEG = 7
CLS_WEIGHT = 8          # factor on the class token's rows of V and dO in the exact cases
SEPARATION = 64.0       # every wrong variant is at least this many 2^-23 E_k away in some component
C_CAP = 16.0            # the exact gate's factor may not exceed this
B_ODD = 3               # odd: the idle second image slot of the last two-image workgroup


# ---- geometry ---------------------------------------------------------------------------------------------------------------
def token_distance(G):
    """[N, N] float64 L1 grid distance between tokens, the class token at the packed coordinate (0, 0) of the kernels (its
    row and column are masked, not its distance)"""
    t = torch.arange(G * G)
    x = torch.cat([torch.zeros(1, dtype=torch.long), t % G])
    y = torch.cat([torch.zeros(1, dtype=torch.long), t // G])
    return ((x[:, None] - x[None, :]).abs() + (y[:, None] - y[None, :]).abs()).to(F64)


def powers(G, n):
    """[n, N, N]: d^0 .. d^(n-1)  (0^0 = 1, as the reference's l1.pow(0))"""
    d = token_distance(G)
    return torch.stack([d.pow(k) for k in range(n)])


def coeffs(degree, G, H, per_head, seed):
    """fp32 coefficients, power k scaled by (2 (G - 1))^-k (the largest distance): the bias stays O(1) at every degree"""
    g = torch.Generator().manual_seed(seed)
    shape = (H, degree + 1) if per_head else (degree + 1,)
    c = (torch.rand(*shape, generator=g) * 2 - 1) * 0.5
    return (c * torch.tensor([float(2 * (G - 1)) ** -k for k in range(degree + 1)])).float()


# ---- routes -----------------------------------------------------------------------------------------------------------------
KERNELS = ("fused", "wide", "fused64", "core", "core_hd")


def pin(kernel, dt, N, D, H):
    """assert that (dt, N, D, H) runs on `kernel`, from the library's host predicates alone (no device needed):
    fused = the 16x16-tile kernels of attn.hip, wide = the 32x32-tile forward, fused64 = the one-kernel forward at hd 64,
    core = the attention core at its own head dimensions 32 / 64, core_hd = the per-head-dimension builds (attn_core_hd)"""
    from vitpe import _lib as L
    h, code, hd = L.lib(), L.dtype_code(DT[dt]), D // H
    assert D % H == 0 and kernel in KERNELS
    fused = bool(h.vitpe_fused_attention_supported(code, N, D, hd))
    wide = bool(h.vitpe_fused_attention_wide_supported(code, N, D, hd))
    f64_ = bool(h.vitpe_attention_fused64_supported(code, N, H, hd))
    core = bool(h.vitpe_attention_core_supported(code, N, hd))
    on = {"fused": fused, "wide": wide and fused, "fused64": f64_ and not fused, "core": core and hd in (32, 64),
          "core_hd": core and hd not in (32, 64)}[kernel]
    assert on, f"case ({kernel}, {dt}, N {N}, D {D}, H {H}) left its route: fused {fused} wide {wide} fused64 {f64_} core {core}"
    return True


# ---- the reference ------------------------------------------------------------------------------------------------------------
def _per_power(w, pw):
    """sum_b,i,j w[b,h,i,j] pw[k,i,j] -> [H, K]"""
    return torch.einsum("bhij,kij->hk", w, pw)


def core_ref(qkv, dout, H, G, coeff, per_head):
    """The attention core with the polynomial bias in float64, forward and backward, on a projection qkv [B, N, 3D] and the
    upstream gradient dout [B, N, D] (float64, as the kernels see them); coeff float64 [degree + 1] or [H, degree + 1].
    -> namespace: out [B,N,D], dqkv [B,N,3D], probs [B,H,N,N], g / E / A ([degree + 1] shared, [H, degree + 1] per head:
    the coefficient gradient, the exact-input scale and the summand scale sum |dS| d^k) and wrong {name: gradient}."""
    B, N, D3 = qkv.shape
    D = D3 // 3
    hd = D // H
    deg = coeff.shape[-1] - 1
    assert N == G * G + 1 and coeff.dtype == F64 and 0 <= deg <= MAXDEG
    q, k, v = qkv.reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    dO = dout.reshape(B, N, H, hd).transpose(1, 2)
    pw = powers(G, deg + 2)
    cf = coeff if per_head else coeff[None].expand(H, -1)
    patch = torch.ones(N, N, dtype=F64)
    patch[0, :] = 0
    patch[:, 0] = 0
    bias = torch.einsum("hk,kij->hij", cf, pw[:deg + 1]) * patch
    scale = hd ** -0.5
    P = (q @ k.transpose(-2, -1) * scale + bias).softmax(-1)
    out = (P @ v).transpose(1, 2).reshape(B, N, D)
    dP = dO @ v.transpose(-2, -1)
    dS = P * (dP - (P * dP).sum(-1, keepdim=True))
    dq, dk, dv = dS @ k * scale, dS.transpose(-2, -1) @ q * scale, P.transpose(-2, -1) @ dO
    dqkv = torch.stack([dq, dk, dv]).permute(1, 3, 0, 2, 4).reshape(B, N, 3 * D)

    def fold(t):   # [H, K] -> the layout of the coefficient tensor
        return t if per_head else t.sum(0)

    r = types.SimpleNamespace(out=out, dqkv=dqkv, probs=P, degree=deg, per_head=per_head)
    g_h = _per_power(dS * patch, pw[:deg + 1])
    r.g = fold(g_h)
    r.E = fold(_per_power(P * (dP.abs() + (P * dP.abs()).sum(-1, keepdim=True)) * patch, pw[:deg + 1]))
    r.A = fold(_per_power(dS.abs() * patch, pw[:deg + 1]))
    row = patch.clone()
    row[0, 1:] = 1         # the class row counted
    col = patch.clone()
    col[1:, 0] = 1         # the class column counted
    w = {"class_row": fold(_per_power(dS * row, pw[:deg + 1])),
         "class_col": fold(_per_power(dS * col, pw[:deg + 1])),
         "power_plus_one": fold(_per_power(dS * patch, pw[1:deg + 2]))}
    if deg > 3:
        hi = g_h.clone()
        hi[:, 4:] = 0
        w["above_3_dropped"] = fold(hi)
    if per_head and H > 1:
        w["heads_swapped"] = g_h.roll(1, 0)
        if deg != 3:   # head h flushed at 4 h instead of (degree + 1) h, inside the H (degree + 1) live floats
            flat = torch.zeros(H * (deg + 1), dtype=F64)
            for h in range(H):
                for kk in range(deg + 1):
                    if 4 * h + kk < flat.numel():
                        flat[4 * h + kk] += g_h[h, kk]
            w["stride_4"] = flat.reshape(H, deg + 1)
    r.wrong = w
    return r


def bias_ref(coeff, H, G, per_head):
    """[H, N, N] float64: the materialised bias (the oracle's polynomial_bias restated on token_distance)"""
    deg = coeff.shape[-1] - 1
    N = G * G + 1
    cf = coeff if per_head else coeff[None].expand(H, -1)
    patch = torch.ones(N, N, dtype=F64)
    patch[0, :] = 0
    patch[:, 0] = 0
    return torch.einsum("hk,kij->hij", cf.to(F64), powers(G, deg + 1)) * patch


def bias_bwd_ref(dbias, G, degree, per_head):
    """-> (g, A): d coeff and sum |dbias| d^k per power of a gradient dbias [H, N, N] (float64) of the materialised bias"""
    pw = powers(G, degree + 1)
    pw[:, 0, :] = 0
    pw[:, :, 0] = 0
    g = torch.einsum("hij,kij->hk", dbias, pw)
    a = torch.einsum("hij,kij->hk", dbias.abs(), pw)
    return (g, a) if per_head else (g.sum(0), a.sum(0))


# ---- cases ------------------------------------------------------------------------------------------------------------------
def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _sparse_pm1(g, rows, cols, n=3):
    """[rows, cols] with n entries of +-1 per row"""
    w = torch.zeros(rows, cols)
    for r in range(rows):
        idx = torch.randperm(cols, generator=g)[:n]
        w[r, idx] = torch.randint(0, 2, (n,), generator=g).float() * 2 - 1
    return w


def _seed(kernel, dt, N, D, H, degree, per_head):
    return ((((KERNELS.index(kernel) * 7 + (dt == "bf16")) * 263 + N) * 1031 + D) * 17 + H) * 16 + 2 * degree + per_head


@functools.lru_cache(maxsize=None)
def exact_case(kernel, dt, N, D, H, degree, per_head, B=B_ODD):
    """Exact inputs (module docstring).  kernel "fused": xn [B,N,D] and wqkv [3D,D] (qkv = xn wqkv^T is exact); the core
    kernels: the projection qkv [B,N,3D] itself.  fp32 CPU tensors whose values bf16 holds exactly."""
    pin(kernel, dt, N, D, H)
    G = int(round((N - 1) ** 0.5))
    assert G * G == N - 1
    g = torch.Generator().manual_seed(_seed(kernel, dt, N, D, H, degree, per_head))
    c = types.SimpleNamespace(kernel=kernel, dt=dt, N=N, D=D, H=H, hd=D // H, G=G, B=B, degree=degree, per_head=per_head,
                              key=(kernel, dt, N, D, H, degree, per_head, B))
    c.coeff = coeffs(degree, G, H, per_head, 77 + _seed(kernel, dt, N, D, H, degree, per_head))
    c.dout = _ints(g, -4, 4, B, N, D)
    c.dout[:, 0] *= CLS_WEIGHT
    if kernel == "fused":
        c.xn = _ints(g, -2, 2, B, N, D)
        c.xn[:, 0] *= CLS_WEIGHT
        c.wqkv = torch.cat([torch.zeros(D, D), _sparse_pm1(g, D, D), _sparse_pm1(g, D, D)])   # q rows zero
        c.qkv = c.xn @ c.wqkv.t()
    else:
        c.qkv = torch.cat([torch.zeros(B, N, D), _ints(g, -2, 2, B, N, D), _ints(g, -4, 4, B, N, D)], dim=-1)
        c.qkv[:, 0, 2 * D:] *= CLS_WEIGHT
    for t in (c.dout, c.qkv):   # bf16 holds every operand exactly, and dP = dO V^T stays an exact fp32 integer
        assert torch.equal(t.bfloat16().float(), t)
    assert c.hd * float(c.dout.abs().max()) * float(c.qkv[..., 2 * D:].abs().max()) < 2 ** 24
    return c


@functools.lru_cache(maxsize=None)
def _exact_ref(key):
    c = exact_case(*key)
    return core_ref(c.qkv.to(F64), c.dout.to(F64), c.H, c.G, c.coeff.to(F64), c.per_head)


def exact_ref(c):
    """core_ref of an exact case, computed once"""
    return _exact_ref(c.key)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


@functools.lru_cache(maxsize=None)
def random_case(kernel, dt, N, D, H, degree, per_head, B=B_ODD):
    """Random inputs in the manner of attn_case (test_kernels_gpu.py): xn, wqkv, dout fp32; the projection the core kernels
    read is the compute-type rounding of xn wqkv^T on the rounded operands."""
    pin(kernel, dt, N, D, H)
    G = int(round((N - 1) ** 0.5))
    assert G * G == N - 1
    s = 100000 + _seed(kernel, dt, N, D, H, degree, per_head)
    c = types.SimpleNamespace(kernel=kernel, dt=dt, N=N, D=D, H=H, hd=D // H, G=G, B=B, degree=degree, per_head=per_head,
                              key=(kernel, dt, N, D, H, degree, per_head, B))
    c.xn, c.wqkv, c.dout = rnd(B, N, D, seed=s + 1), rnd(3 * D, D, seed=s + 2, scale=0.3), rnd(B, N, D, seed=s + 3)
    c.coeff = coeffs(degree, G, H, per_head, s + 5)
    qd = lambda t: t.to(DT[dt]).to(F64)   # noqa: E731
    c.qkv64 = qd(c.xn) @ qd(c.wqkv).t()
    c.qkv = c.qkv64.float()               # what the core kernels get (rounded once more to the compute type by the test)
    return c


@functools.lru_cache(maxsize=None)
def _random_ref(key, core):
    c = random_case(*key)
    qkv = c.qkv.to(DT[c.dt]).to(F64) if core else c.qkv64
    return core_ref(qkv, c.dout.to(DT[c.dt]).to(F64), c.H, c.G, c.coeff.to(F64), c.per_head)


def random_ref(c, core):
    """core_ref of a random case; core: on the projection rounded to the compute type (the core kernels' operand),
    otherwise on the unrounded product (the fused kernels project on the chip)"""
    return _random_ref(c.key, bool(core))


def excess(got, ref, bound):
    """worst |got - ref| / bound over the components (<= 1 passes); a component with bound 0 must be exact"""
    d = (got.to(F64) - ref).abs()
    r = torch.where(bound > 0, d / bound.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, float("inf")), torch.zeros_like(d)))
    return float(r.max())


# ---- the case lists of the GPU file (test_poly_degree_cpu.py checks separation and routes on the same lists) ------------------
# (kernel, dt, N, D, H): the smallest shapes at which each kernel runs its real tiling
FUSED_GEOMS = [("fused", "f32", 65, 96, 3), ("fused", "bf16", 65, 192, 6),
               ("fused", "bf16", 65, 96, 3), ("fused", "f32", 65, 192, 6)]   # (the other two widths the kernels are built for)
CORE_GEOMS = [(k, dt, N, hd * 2, 2) for dt in ("f32", "bf16")
              for k, N, hd in (("core", 17, 32), ("core", 26, 32), ("core", 17, 64), ("core", 26, 64), ("core_hd", 17, 48))]
FAR_GEOMS = [("core", dt, 257, 32, 1) for dt in ("f32", "bf16")]       # G 16: distances up to 30 of the 32 table entries
WIDE_GEOM = ("wide", "bf16", 65, 192, 6)
FUSED64_GEOM = ("fused64", "bf16", 197, 128, 2)
FUSED_EXACT_DEGREES = (0, 1, 2, 3, 4, 5, 7)    # bf16: 0-3 on the PDEG = 3 instantiation, 4-7 on PDEG = 7
CORE_EXACT_DEGREES = (0, 3, 7)
EXACT_CASES = ([g + (d, ph) for g in FUSED_GEOMS for d in FUSED_EXACT_DEGREES for ph in (False, True)]
               + [g + (d, ph) for g in CORE_GEOMS for d in CORE_EXACT_DEGREES for ph in (False, True)])
FAR_CASES = [g + (7, False, 1) for g in FAR_GEOMS]                      # B = 1, degree 7
RANDOM_DEGREES = (0, 2, 5, 7)
FWD_DEGREES = (0, 1, 2, 3, 4, 7)
for _c in EXACT_CASES + FAR_CASES + [WIDE_GEOM + (0, False), FUSED64_GEOM + (0, False)]:
    pin(*_c[:5])


def case_id(c):
    return "-".join(str(x) for x in c)
