"""The block-tail backward moves its activation rows as whole 128-byte lines: two token lanes share a line and exchange
16-byte pieces.  These tests use the smallest shapes at which that exchange or the row clamp can go wrong.

Exact part: the transposed weights are signed selection matrices (one +-1 per row) and every activation is a small
integer or one of {0.5, 1, -1, 0.25}, so every product and sum is exact in bf16 / fp32 and the outputs are compared with
`==` against float64.  Every (row, 16-byte piece) of gelu'(u) and of d_qkv spells its own index, so a swapped piece or
row cannot pass.  The LayerNorms are made exact as well: statistics mean = 0, rstd = 1 on an all-zero input row give
xhat = 0; norm2 gets gamma = 0 (dx_mid = dy), the upper norm1 gets gamma = 1 and a product whose rows sum to zero
(features n and n + 96 select the same d_qkv column with opposite signs), so dy_out = dres1 + d_qkv Wqkv exactly.

Random part: the same shapes against float64 math on the rounded operands with the bounds of the three block-tail
backward tests in test_kernels_gpu.py (6e-3 on du / dx / da / dy, 2e-3 on dgamma / dbeta).

Every output has a guard row after row M - 1 that must keep its sentinel value."""
import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

D, BF = 192, torch.bfloat16
MS = [1, 2, 15, 16, 17, 31, 33, 16 * 9 + 1]      # the last: a ninth tile in the only workgroup
HIDS = [128, 192, 768]
K1S = [64, 192, 320, 576]                        # one k chunk, an odd number of chunks, the real width
GUARD = -512.0


@pytest.fixture(scope="module")
def K():
    from vitpe import kernels
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return kernels


def dev(t, dtype=torch.float32):
    return t.to(dtype).cuda().contiguous()


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def q(t):
    return t.to(BF).double()


def guarded(M, W):
    buf = torch.full((M + 1, W), GUARD, device="cuda", dtype=BF)
    return buf, buf[:M]


def guard_kept(*bufs):
    return all(bool((b[-1] == GUARD).all()) for b in bufs)


def selection(rows, cols, shift, step):
    """[rows, cols], one +-1 per row"""
    w = torch.zeros(rows, cols, dtype=torch.float64)
    r = torch.arange(rows)
    w[r, (step * r + shift) % cols] = torch.where(r % 3 == 0, -1.0, 1.0).double()
    return w


def zero_sum_selection(K1, shift):
    """[192, K1]: rows n and n + 96 select column (n + 96 shift) % K1 with opposite signs"""
    w = torch.zeros(D, K1, dtype=torch.float64)
    n = torch.arange(96)
    col = (n + 96 * shift) % K1
    w[n, col] = 1.0
    w[n + 96, col] = -1.0
    return w


def coded(M, W, values):
    """[M, W]: the 8 elements of the 16-byte piece p of row m spell m W / 8 + p in base len(values)"""
    b = len(values)
    idx = torch.arange(M)[:, None] * (W // 8) + torch.arange(W // 8)[None, :]
    assert int(idx.max()) < b ** 8
    digits = torch.stack([(idx // b ** e) % b for e in range(8)], dim=-1)
    return torch.tensor(values, dtype=torch.float64)[digits].reshape(M, W)


def small_ints(M, W, a, b):
    """nonzero integers in [-3, 3]"""
    v = (a * torch.arange(M)[:, None] + b * torch.arange(W)[None, :]) % 6
    return torch.tensor([1.0, 2.0, 3.0, -1.0, -2.0, -3.0], dtype=torch.float64)[v]


GP_VALUES = [0.5, 1.0, -1.0, 0.25]


class ExactMlp:
    """operands of the MLP half shared by the exact tests of one (M, HID)"""

    def __init__(self, K, M, HID):
        self.gp = coded(M, HID, GP_VALUES)
        self.w2t = selection(HID, D, 3, 5)       # fc2.weight^T
        self.w1t = selection(D, HID, 1, 7)       # fc1.weight^T
        self.wpt = selection(D, D, 2, 11)        # attn.proj.weight^T
        self.pk = (K.pack_weight_frags(dev(self.w2t), BF, 192, 1), K.pack_weight_frags(dev(self.w1t), BF, 32, 1))
        self.wpt_pk = K.pack_weight_frags(dev(self.wpt), BF, 192, 1)
        self.gp_d = dev(self.gp, torch.float16)
        self.xmid = torch.zeros(M, D, device="cuda", dtype=BF)
        self.mean, self.rstd = torch.zeros(M, device="cuda"), torch.ones(M, device="cuda")
        self.gamma0 = torch.zeros(D, device="cuda")

    def check(self, dy, dx, du, da, dg, db, what):
        du_ref = (dy @ self.w2t.t()) * self.gp
        assert torch.equal(du.double().cpu(), du_ref), what
        assert torch.equal(dx.double().cpu(), dy), what
        assert torch.equal(da.double().cpu(), dy @ self.wpt.t()), what
        assert torch.equal(db.double().cpu(), (du_ref @ self.w1t.t()).sum(0)), what       # rows past M masked
        assert not dg.any(), what


@pytest.mark.parametrize("M", MS)
def test_du_lines_exact(K, M):
    for HID in HIDS:
        e = ExactMlp(K, M, HID)
        dy = small_ints(M, D, 3, 5)
        dg, db = torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")
        (dub, du), (dxb, dx), (dab, da) = guarded(M, HID), guarded(M, D), guarded(M, D)
        K.block_tail2_bwd(dev(dy, BF), e.gp_d, e.pk[0], e.pk[1], e.xmid, e.mean, e.rstd, e.gamma0, dg, db, e.wpt_pk,
                          du=du, out=dx, da=da)
        e.check(dy, dx, du, da, dg, db, f"M={M} HID={HID}")
        assert guard_kept(dub, dxb, dab), f"M={M} HID={HID}"


@pytest.mark.parametrize("M", MS)
def test_dqkv_lines_exact(K, M):
    for i, K1 in enumerate(K1S):
        HID = HIDS[i % len(HIDS)]
        e = ExactMlp(K, M, HID)
        dq, dres1 = coded(M, K1, [-2.0, -1.0, 0.0, 1.0, 2.0]), small_ints(M, D, 5, 1)
        x1, gamma1 = torch.zeros(M, D, device="cuda", dtype=BF), torch.ones(D, device="cuda")
        for shift in range((K1 + 95) // 96):              # every d_qkv column is selected by some launch
            what = f"M={M} HID={HID} K1={K1} shift={shift}"
            wqt = zero_sum_selection(K1, shift)
            wqt_pk = K.pack_weight_frags(dev(wqt), BF, 64, 0)
            dxn = dq @ wqt.t()
            dy_ref = dres1 + dxn
            z = lambda: torch.zeros(D, device="cuda")  # noqa: E731
            dg1, db1, dg2, db2 = z(), z(), z(), z()
            (dyb, dyo), (dub, du), (dxb, dx), (dab, da) = guarded(M, D), guarded(M, HID), guarded(M, D), guarded(M, D)
            K.block_tail2_bwd_pre(dev(dq, BF), wqt_pk, x1, e.mean, e.rstd, gamma1, dev(dres1, BF), dg1, db1, dyo, e.gp_d,
                                  e.pk[0], e.pk[1], e.xmid, e.mean, e.rstd, e.gamma0, dg2, db2, e.wpt_pk, du=du, out=dx, da=da)
            assert torch.equal(dyo.double().cpu(), dy_ref), what
            assert torch.equal(db1.double().cpu(), dxn.sum(0)) and not dg1.any(), what
            e.check(dy_ref, dx, du, da, dg2, db2, what)
            assert guard_kept(dyb, dub, dxb, dab), what
            if K1 % 192 == 0:
                dg3, db3 = z(), z()
                ob, o = guarded(M, D)
                K.linear_lnbwd2(dev(dq, BF), wqt_pk, x1, e.mean, e.rstd, gamma1, dev(dres1, BF), dg3, db3, out=o)
                assert torch.equal(o.double().cpu(), dy_ref), what
                assert torch.equal(db3.double().cpu(), dxn.sum(0)) and not dg3.any(), what
                assert guard_kept(ob), what


def ln_backward_ref(dxn, x, mean, rstd, g, res):
    mu, rs = mean.double().cpu()[:, None], rstd.double().cpu()[:, None]
    xhat = (x - mu) * rs
    gy = dxn * g
    dx = res + rs * (gy - gy.mean(1, keepdim=True) - xhat * (gy * xhat).mean(1, keepdim=True))
    return dx, (dxn * xhat).sum(0), dxn.sum(0)


class RandomMlp:
    def __init__(self, K, M, HID):
        self.xm, self.g2 = rnd(M, D, seed=66), (1 + 0.1 * rnd(D, seed=67)).double()
        self.gp = q(0.5 + 0.6 * rnd(M, HID, seed=68))                  # bf16 values: exact as IEEE half
        self.w2, self.w1, self.wp = rnd(D, HID, seed=69, scale=0.05), rnd(HID, D, seed=70, scale=0.08), rnd(D, D, seed=71, scale=0.07)
        self.xmd = dev(self.xm, BF)
        _, self.m2, self.r2 = K.layernorm_fwd(self.xmd, dev(self.g2), torch.zeros(D, device="cuda"))
        self.w2t_pk = K.pack_weight_frags(dev(self.w2.t()), BF, 192, 1)
        self.w1t_pk = K.pack_weight_frags(dev(self.w1.t()), BF, 32, 1)
        self.wpt_pk = K.pack_weight_frags(dev(self.wp.t()), BF, 192, 1)
        self.gp_d = dev(self.gp, torch.float16)

    def check(self, dy, dx, du, da, dg, db, what):
        """stage by stage from the kernel's own (rounded) intermediates; dy = the rounded values the MLP half saw"""
        assert rel_err(du.double().cpu(), (dy @ q(self.w2)) * self.gp) < 6e-3, what
        dxn = du.double().cpu() @ q(self.w1)
        dx_ref, dg_ref, db_ref = ln_backward_ref(dxn, q(self.xm), self.m2, self.r2, self.g2, dy)
        assert rel_err(dx.double().cpu(), dx_ref) < 6e-3, what
        assert rel_err(dg.cpu(), dg_ref) < 2e-3 and rel_err(db.cpu(), db_ref) < 2e-3, what
        assert rel_err(da.double().cpu(), dx.double().cpu() @ q(self.wp)) < 6e-3, what


@pytest.mark.parametrize("M", MS)
def test_du_lines_random(K, M):
    for HID in HIDS:
        r = RandomMlp(K, M, HID)
        dy = rnd(M, D, seed=43)
        dg, db = torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")
        (dub, du), (dxb, dx), (dab, da) = guarded(M, HID), guarded(M, D), guarded(M, D)
        K.block_tail2_bwd(dev(dy, BF), r.gp_d, r.w2t_pk, r.w1t_pk, r.xmd, r.m2, r.r2, dev(r.g2), dg, db, r.wpt_pk,
                          du=du, out=dx, da=da)
        r.check(q(dy), dx, du, da, dg, db, f"M={M} HID={HID}")
        assert guard_kept(dub, dxb, dab), f"M={M} HID={HID}"


@pytest.mark.parametrize("M", MS)
def test_dqkv_lines_random(K, M):
    for i, K1 in enumerate(K1S):
        HID = HIDS[i % len(HIDS)]
        what = f"M={M} HID={HID} K1={K1}"
        r = RandomMlp(K, M, HID)
        dq, wq = rnd(M, K1, seed=61), rnd(K1, D, seed=62, scale=0.06)
        x1, g1, dres1 = rnd(M, D, seed=63), (1 + 0.1 * rnd(D, seed=64)).double(), rnd(M, D, seed=65)
        x1d = dev(x1, BF)
        _, m1, r1 = K.layernorm_fwd(x1d, dev(g1), torch.zeros(D, device="cuda"))
        wqt_pk = K.pack_weight_frags(dev(wq.t()), BF, 64, 0)
        z = lambda: torch.zeros(D, device="cuda")  # noqa: E731
        dg1, db1, dg2, db2 = z(), z(), z(), z()
        (dyb, dyo), (dub, du), (dxb, dx), (dab, da) = guarded(M, D), guarded(M, HID), guarded(M, D), guarded(M, D)
        K.block_tail2_bwd_pre(dev(dq, BF), wqt_pk, x1d, m1, r1, dev(g1), dev(dres1, BF), dg1, db1, dyo, r.gp_d, r.w2t_pk,
                              r.w1t_pk, r.xmd, r.m2, r.r2, dev(r.g2), dg2, db2, r.wpt_pk, du=du, out=dx, da=da)
        dy_ref, dg1_ref, db1_ref = ln_backward_ref(q(dq) @ q(wq), q(x1), m1, r1, g1, q(dres1))
        assert rel_err(dyo.double().cpu(), dy_ref) < 6e-3, what
        assert rel_err(dg1.cpu(), dg1_ref) < 2e-3 and rel_err(db1.cpu(), db1_ref) < 2e-3, what
        r.check(dyo.double().cpu(), dx, du, da, dg2, db2, what)
        assert guard_kept(dyb, dub, dxb, dab), what
        if K1 % 192 == 0:
            # the two launches the fused one replaces: the same values
            dg1a, db1a, dg2a, db2a = z(), z(), z(), z()
            (dyab, dya), (duab, dua), (dxab, dxa), (daab, daa) = guarded(M, D), guarded(M, HID), guarded(M, D), guarded(M, D)
            K.linear_lnbwd2(dev(dq, BF), wqt_pk, x1d, m1, r1, dev(g1), dev(dres1, BF), dg1a, db1a, out=dya)
            K.block_tail2_bwd(dya, r.gp_d, r.w2t_pk, r.w1t_pk, r.xmd, r.m2, r.r2, dev(r.g2), dg2a, db2a, r.wpt_pk,
                              du=dua, out=dxa, da=daa)
            assert torch.equal(dyo, dya) and torch.equal(du, dua) and torch.equal(dx, dxa) and torch.equal(da, daa), what
            assert guard_kept(dyab, duab, dxab, daab), what
