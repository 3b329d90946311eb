"""Class-row mode of the top block ("Top block on the class-token rows"): the block tail, its backward and
three weight gradients on the class-token rows only, in place on the full-layout [batch x tokens, .] buffers (csrc/tail_cls.hip, row-step problems of csrc/wgrad.hip).

Kernel tests: N = 65 tokens, D = 192, HID = 768, bf16, B in {3 (a partial 16-row tile), 17 (ragged), 32 (two whole tiles)};
every NON-class row of every input holds a large finite sentinel (a read of it shows in the result) and every non-class row
of every output must come back bit-identical.  Tolerances are those of the full-row kernels' tests in test_kernels_gpu.py
(restated next to each assert).  Engine tests: one captured step with the mode on and one with VITPE_CLS_ROWS=0, each in a
fresh child process, against the fp32 oracle under the gates of test_bench_path_gpu.py.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, rel_err
from test_kernels_gpu import BF16_TOL, K, dev, q, rnd  # noqa: F401  (K: the kernels fixture)

pytestmark = pytest.mark.gpu

N, D, HID = 65, 192, 768
SENTINEL = 1e4
BATCHES = [3, 17, 32]
bf = torch.bfloat16


def full(rows, B, fill=SENTINEL, dtype=bf):
    """[B * N, C] device tensor: class row b * N = rows[b], every other row = fill."""
    C = rows.shape[1] if rows.dim() == 2 else None
    t = torch.full((B * N,) + ((C,) if C else ()), fill, dtype=torch.float32)
    t[::N] = rows
    return t.cuda().to(dtype).contiguous()


def noise(shape, seed, dtype=bf):
    """what an output buffer holds before the launch"""
    return (rnd(*shape, seed=seed) * 3).cuda().to(dtype).contiguous()


def others_untouched(after, before):
    mask = torch.ones(after.shape[0], dtype=torch.bool, device=after.device)
    mask[::N] = False
    a, b = after[mask], before[mask]
    if a.dtype == torch.float16 or a.dtype == bf:
        return torch.equal(a.view(torch.int16), b.view(torch.int16))
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("B", BATCHES)
def test_tail_cls_forward_class_rows_only(K, B):
    M = B * N
    a_, x_in = rnd(B, D, seed=21), rnd(B, D, seed=22)
    wp, bp = rnd(D, D, seed=23, scale=0.07), 0.1 * rnd(D, seed=24)
    g, b = 1 + 0.1 * rnd(D, seed=25), 0.1 * rnd(D, seed=26)
    w1, b1 = rnd(HID, D, seed=27, scale=0.08), 0.1 * rnd(HID, seed=28)
    w2, b2 = rnd(D, HID, seed=29, scale=0.05), 0.1 * rnd(D, seed=30)
    wp_pk, w1_pk, w2_pk = K.pack_weight_frags(dev(wp), bf, 192, 0), K.pack_weight_frags(dev(w1), bf, 192, 1), K.pack_weight_frags(dev(w2), bf, 32, 1)
    outs = dict(x_mid=noise((M, D), 1), m2=noise((M,), 2, torch.float32), r2=noise((M,), 3, torch.float32), xn=noise((M, D), 4),
                gp=noise((M, HID), 5, torch.float16), h=noise((M, HID), 6), out=noise((M, D), 7))
    before = {k: v.clone() for k, v in outs.items()}
    K.tail_cls_fwd(full(a_, B), full(x_in, B), wp_pk, dev(bp), dev(g), dev(b), w1_pk, dev(b1), w2_pk, dev(b2), B, N,
                   outs["x_mid"], outs["m2"], outs["r2"], outs["out"], xn_out=outs["xn"], gp=outs["gp"], h=outs["h"])
    torch.cuda.synchronize()
    for k in outs:
        assert others_untouched(outs[k], before[k]), k
    x_mid, m2, r2, xn_out, gp, h, out = (outs[k][::N].float().cpu() for k in ("x_mid", "m2", "r2", "xn", "gp", "h", "out"))
    # fp32 math on the rounded operands, stage by stage from the kernel's own (rounded) intermediates: the checks and
    # tolerances of test_block_tail2_forward_equals_the_per_linear_path
    xm = q(a_, "bf16") @ q(wp, "bf16").t() + bp + q(x_in, "bf16")
    assert rel_err(x_mid, xm) < BF16_TOL
    assert rel_err(m2, x_mid.mean(1)) < 1e-5
    assert rel_err(r2, (x_mid.var(1, unbiased=False) + 1e-5).rsqrt()) < 1e-5
    xn = torch.nn.functional.layer_norm(x_mid, (D,), g, b)
    assert rel_err(xn_out, xn) < BF16_TOL
    u_ref = (xn_out @ q(w1, "bf16").t() + b1).requires_grad_(True)
    h_ref = torch.nn.functional.gelu(u_ref)
    assert rel_err(h, h_ref.detach()) < 6e-3
    gp_ref, = torch.autograd.grad(h_ref.sum(), u_ref)
    assert rel_err(gp, gp_ref) < 1.2e-3       # gelu'(u) kept as IEEE half (round toward zero)
    ref = x_mid + q(h_ref.detach(), "bf16") @ q(w2, "bf16").t() + b2
    assert rel_err(out, ref) < BF16_TOL
    # ... and the full-row kernel on the gathered rows: same arithmetic and rounding points
    o2, xm2, m22, r22, gp2, h2 = K.block_tail2_fwd(dev(a_, bf), dev(x_in, bf), wp_pk, dev(bp), dev(g), dev(b), w1_pk, dev(b1),
                                                  w2_pk, dev(b2))
    assert rel_err(x_mid, xm2.float().cpu()) < 4e-3 and rel_err(out, o2.float().cpu()) < 8e-3     # (its per-Linear comparison's bounds)
    assert rel_err(h, h2.float().cpu()) < 8e-3 and rel_err(gp, gp2.float().cpu()) < 1.2e-3
    # evaluation form: nothing of the hidden layer is written
    ev = {k: before[k].clone() for k in outs}
    K.tail_cls_fwd(full(a_, B), full(x_in, B), wp_pk, dev(bp), dev(g), dev(b), w1_pk, dev(b1), w2_pk, dev(b2), B, N,
                   ev["x_mid"], ev["m2"], ev["r2"], ev["out"])
    torch.cuda.synchronize()
    assert torch.equal(ev["out"], outs["out"]) and torch.equal(ev["h"], before["h"]) and torch.equal(ev["gp"], before["gp"])


@pytest.mark.parametrize("B", BATCHES)
def test_tail_cls_backward_class_rows_only(K, B):
    M = B * N
    x, g = rnd(B, D, seed=41), 1 + 0.1 * rnd(D, seed=42)
    dy, gp = rnd(B, D, seed=43), 0.5 + 0.6 * rnd(B, HID, seed=44)
    w2, w1, wp = rnd(D, HID, seed=45, scale=0.05), rnd(HID, D, seed=46, scale=0.08), rnd(D, D, seed=47, scale=0.07)
    xd = dev(x, bf)
    _, mean, rstd = K.layernorm_fwd(xd, dev(g), torch.zeros(D, device="cuda"))
    w2t_pk = K.pack_weight_frags(dev(w2.t().contiguous()), bf, 192, 1)
    w1t_pk = K.pack_weight_frags(dev(w1.t().contiguous()), bf, 32, 1)
    wpt_pk = K.pack_weight_frags(dev(wp.t().contiguous()), bf, 192, 1)
    dg2, db2 = torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")
    outs = dict(du=noise((M, HID), 11), dx=noise((M, D), 12), da=noise((M, D), 13))
    before = {k: v.clone() for k, v in outs.items()}
    K.tail_cls_bwd(full(dy, B), full(q(gp, "bf16"), B, dtype=torch.float16), w2t_pk, w1t_pk, full(x, B),
                   full(mean.cpu(), B, dtype=torch.float32), full(rstd.cpu(), B, dtype=torch.float32), dev(g), dg2, db2, wpt_pk,
                   B, N, du=outs["du"], out=outs["dx"], da=outs["da"])
    torch.cuda.synchronize()
    for k in outs:
        assert others_untouched(outs[k], before[k]), k
    du2, dx2, da2 = (outs[k][::N].float().cpu() for k in ("du", "dx", "da"))
    # the checks and tolerances of test_block_tail2_backward_on_saved_derivative
    dyq, gpq, xq = q(dy, "bf16"), q(gp, "bf16"), q(x, "bf16")
    assert rel_err(du2, (dyq @ q(w2, "bf16")) * gpq) < 6e-3
    dxn = du2 @ q(w1, "bf16")
    mu, rs = mean.cpu()[:, None], rstd.cpu()[:, None]
    xhat = (xq - mu) * rs
    gy = dxn * g
    dx_ref = dyq + rs * (gy - gy.mean(1, keepdim=True) - xhat * (gy * xhat).mean(1, keepdim=True))
    assert rel_err(dx2, dx_ref) < 6e-3
    assert rel_err(dg2.cpu(), (dxn * xhat).sum(0)) < 2e-3 and rel_err(db2.cpu(), dxn.sum(0)) < 2e-3
    assert rel_err(da2, dx2 @ q(wp, "bf16")) < 6e-3


@pytest.mark.parametrize("ln", [False, True])
@pytest.mark.parametrize("B", [17, 130])
def test_wgrad_group_row_step_problems(K, B, ln):
    """One ordinary problem and three row_step = N problems (the top block's fc2 / fc1 / proj shapes) in one launch against
    gemm_tn on the gathered rows; B = 130: two 64-row stages and a partial one.  Non-class rows of the strided operands hold
    the sentinel.  Plain problems: 1e-4 (bf16 products are exact in fp32, only the summation order differs:
    test_wgrad_group_whole_model_list); LayerNorm operand: 1e-2 (xhat rounded to bf16 once:
    test_wgrad_group_layernorm_operand_is_recomputed_in_the_kernel)."""
    M = B * N
    dq, xq_ = dev(rnd(M, 3 * D, seed=600), bf), dev(rnd(M, D, seed=601), bf)
    probs = [(dq, xq_, torch.zeros(3 * D, D, device="cuda"), None)]
    refs = [(dq, xq_, None)]
    gam, bet = rnd(D, seed=630) + 1.5, rnd(D, seed=631)
    for i, (Nn, Kk, bias, use_ln) in enumerate([(D, HID, True, False), (HID, D, True, ln), (D, D, True, False)]):
        dyr, xr = rnd(B, Nn, seed=610 + i), rnd(B, Kk, seed=620 + i) * 2 + 0.3
        dw, db = torch.zeros(Nn, Kk, device="cuda"), torch.zeros(Nn, device="cuda")
        lnop = None
        xg = dev(xr, bf)
        if use_ln:
            _, mean, rstd = K.layernorm_fwd(xg.view(1, B, Kk), dev(gam), dev(bet), stats_only=True)
            lnop = (full(mean.cpu(), B, dtype=torch.float32), full(rstd.cpu(), B, dtype=torch.float32), dev(gam), dev(bet))
            xg = dev(torch.nn.functional.layer_norm(xg.float().cpu(), (Kk,), gam, bet, 1e-5), bf)
        probs.append((full(dyr, B), full(xr, B), dw, db, lnop, N))
        refs.append((dev(dyr, bf), xg, use_ln))
    grp = K.WgradGroup(probs)
    grp.launch()
    torch.cuda.synchronize()
    for prob, (dyg, xg, use_ln) in zip(probs, refs):
        dw, db = prob[2], prob[3]
        rw = torch.zeros_like(dw)
        rb = torch.zeros_like(db) if db is not None else None
        K.gemm_tn(dyg, xg, rw, rb)
        assert rel_err(dw.cpu(), rw.cpu()) < (1e-2 if use_ln else 1e-4), (tuple(dw.shape), use_ln)
        if db is not None:
            assert rel_err(db.cpu(), rb.cpu()) < 1e-4, tuple(dw.shape)


def test_wgrad_group_short_slots_behind_a_placed_list(K):
    """The engine's whole-model list at B = 130: 21 long problems (6 x qkv, 5 x {fc2, fc1, proj}: 64 blocks of 133 stages,
    enough for the table / range-major placements -- NOT stream-K, whose runs cover short problems by themselves) and the top
    block's three row_step = N problems of THREE stages each (130 rows), which run as short slots behind the placed work:
    the slot -> (problem, block, stage range) lookup with slots of two stages and a last slot of one.  Every problem at
    1e-4 against fp32 math on the values the kernel sees (as test_wgrad_group_whole_model_list), launched twice."""
    B = 130
    M = B * N
    shapes = [(D, HID, True), (HID, D, True), (D, D, True), (3 * D, D, False)]
    probs, refs = [], []
    for l in range(6):
        for j, (Nn, Kk, bias) in enumerate(shapes):
            i = 4 * l + j
            dw = torch.zeros(Nn, Kk, device="cuda")
            db = torch.zeros(Nn, device="cuda") if bias else None
            if l == 0 and j < 3:    # the top block comes first in the engine's list
                dyr, xr = rnd(B, Nn, seed=700 + i), rnd(B, Kk, seed=740 + i)
                probs.append((full(dyr, B), full(xr, B), dw, db, None, N))
            else:
                dyr, xr = rnd(M, Nn, seed=700 + i), rnd(M, Kk, seed=740 + i)
                probs.append((dev(dyr, bf), dev(xr, bf), dw, db))
            refs.append((q(dyr, "bf16").t() @ q(xr, "bf16"), q(dyr, "bf16").sum(0)))
    grp = K.WgradGroup(probs)
    for rep_ in (1, 2):     # accumulates
        grp.launch()
        torch.cuda.synchronize()
        for prob, (rw, rb) in zip(probs, refs):
            dw, db = prob[2], prob[3]
            assert rel_err(dw.cpu(), rep_ * rw) < 1e-4, (tuple(dw.shape), len(prob))
            if db is not None:
                assert rel_err(db.cpu(), rep_ * rb) < 1e-4, (tuple(dw.shape), len(prob))


# ---------------------------------------------------------------------------------------------------------------------------
# engine: a fresh child process per run (the switch is read when the engine is built)
def _child(tag, out_path, probes):
    """One captured step from the seeded weights and batch of test_bench_path_gpu (B = 16); probes: step -> every
    kernel_probes() closure once -> gradients zeroed -> a second step from the SAME state is what gets reported."""
    import test_bench_path_gpu as BP
    from vitpe.engine import TrainEngine
    B = 16
    cfg, model = BP.build(tag, {}, {}, seeded=True)
    g = torch.Generator().manual_seed(11)
    images, labels = torch.randn(B, 3, 32, 32, generator=g).cuda(), torch.randint(0, 10, (B,), generator=g).cuda()
    eng = TrainEngine(model, B, compute_dtype=bf, use_graph=True)
    assert eng.cls_rows == (os.environ.get("VITPE_CLS_ROWS", "1") == "1")
    res = {}
    if probes:
        state = [t.clone() for t in (eng.flat_p, eng.flat_m, eng.flat_v, eng.hp)]
        eng.step(images, labels)
        for pr in eng.kernel_probes():
            for fn in pr["fns"]:
                fn()
        torch.cuda.synchronize()
        for t, c in zip((eng.flat_p, eng.flat_m, eng.flat_v, eng.hp), state):
            t.copy_(c)
        eng.flat_g.zero_()
        eng.refresh_shadows()
    eng.step(images, labels)
    torch.cuda.synchronize()
    if eng.cls_rows:
        top = eng.Lyr - 1
        for name, t in (("du", eng.du_l[top]), ("dx_mid", eng.dx_mid[top]), ("da", eng.da_top)):
            t2 = t.view(B, eng.N, -1)
            res["nonzero_" + name] = np.array(int((t2[:, 1:] != 0).sum()))
            res["class_" + name] = np.array(float(t2[:, 0].float().abs().max()))
    beta1, beta2 = float(eng.hp[1]), float(eng.hp[2])
    for n, p in eng.model.named_parameters():
        o = eng._off[id(p)]
        res["g:" + n] = (eng.flat_m[o:o + p.numel()] / (1.0 - beta1)).view(p.shape).cpu().numpy()
        res["v:" + n] = (eng.flat_v[o:o + p.numel()] / (1.0 - beta2)).view(p.shape).cpu().numpy()
    res["logits"], res["loss"] = eng.logits.cpu().numpy(), np.array(float(eng.out2[0]))
    # evaluation (test 6): eager forward at a ragged batch of 17 through an engine of its own
    cfg2, model2 = BP.build(tag, {}, {}, seeded=True)
    e2 = TrainEngine(model2, 32, compute_dtype=bf, use_graph=False)
    g2 = torch.Generator().manual_seed(12)
    res["eval_logits"] = e2.forward_only(torch.randn(17, 3, 32, 32, generator=g2).cuda()).float().cpu().numpy()
    np.savez(out_path, **res)


def _run_child(tag, tmp_path, cls_rows, probes=False):
    out = os.path.join(str(tmp_path), f"{tag}_{cls_rows}_{int(probes)}.npz")
    env = dict(os.environ, VITPE_CLS_ROWS=cls_rows)
    subprocess.run([sys.executable, os.path.abspath(__file__), "child", tag, out, str(int(probes))], check=True, env=env,
                   cwd=os.path.join(REPO, "tests"), timeout=300)
    return np.load(out)


_ORACLE = {}


def _oracle(tag):
    if tag not in _ORACLE:
        import test_bench_path_gpu as BP
        from oracle import vit_oracle as O
        cfg, model = BP.build(tag, {}, {}, seeded=True)
        params = {n: p.detach().cpu().clone() for n, p in model.named_parameters()}
        if tag == "rope-axial":
            params["pos_embed.inv_freq"] = model.pos_embed.inv_freq.cpu()
        g = torch.Generator().manual_seed(11)
        images, labels = torch.randn(16, 3, 32, 32, generator=g), torch.randint(0, 10, (16,), generator=g)
        _ORACLE[tag] = (model, *O.loss_and_grads(cfg, params, images, labels))
    return _ORACLE[tag]


def _gate(tag, run, key):
    """the per-tensor gates test_bench_path_gpu.py applies to the default path; returns (violations, per-tensor max-norm error)"""
    import test_bench_path_gpu as BP
    model, ref_logits, ref_loss, ref_grads = _oracle(tag)
    grads = {n: torch.from_numpy(run["g:" + n]) for n, _ in model.named_parameters()}
    report = {}
    bad = BP.compare_all(key, model, grads, ref_grads, report)
    errs = {}
    for n, _ in model.named_parameters():
        mine, ref = run["g:" + n], ref_grads[n].numpy()
        if n == "pos_embed.pos_embed":
            mine = mine[:, :ref.shape[1]]
        if float(np.abs(ref).max()) > 0.0:
            errs[n] = rel_err(mine, ref)
            # second moment after the first step = g^2: the same max-norm gate on |g|
            v = np.sqrt(run["v:" + n])
            if n == "pos_embed.pos_embed":
                v = v[:, :ref.shape[1]]
            if rel_err(v, np.abs(ref)) > 5e-2:
                bad.append((n, "v", rel_err(v, np.abs(ref))))
    if rel_err(run["logits"], ref_logits) > 5e-2:
        bad.append(("logits", "rel", rel_err(run["logits"], ref_logits)))
    if abs(float(run["loss"]) - float(ref_loss)) > 2e-2:
        bad.append(("loss", "abs", abs(float(run["loss"]) - float(ref_loss))))
    BP._dump(report, "cls_rows_parity.jsonl")
    return bad, errs


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    cache = {}

    def get(tag, cls_rows, probes=False):
        k = (tag, cls_rows, probes)
        if k not in cache:
            cache[k] = _run_child(tag, tmp_path_factory.mktemp("cls"), cls_rows, probes)
        return cache[k]
    return get


@pytest.mark.parametrize("tag", ["rope-axial", "polynomial"])
def test_engine_step_equals_the_full_row_path(runs, tag):
    on, off = runs(tag, "1"), runs(tag, "0")
    bad_on, err_on = _gate(tag, on, tag + "/cls_rows")
    bad_off, err_off = _gate(tag, off, tag + "/full_rows")
    print(json.dumps({n: (err_on[n], err_off[n]) for n in err_on}))
    assert not bad_on, bad_on
    # the two paths differ in fp32 summation order only: no tensor's error against the oracle grows by more than that
    # (on the gradients g = m / (1 - beta1) only, on purpose: after one step v = (1 - beta2) g^2 carries the same information,
    #  and it has its own 5e-2 gate in _gate)
    worse = [(n, err_on[n], err_off[n]) for n in err_on if err_on[n] > 1.5 * err_off[n]]
    assert not worse, worse
    # logits and loss: within the step's run-to-run spread (bench.py: about 1 % of the logits' maximum)
    assert np.abs(on["logits"] - off["logits"]).max() <= 1e-2 * np.abs(off["logits"]).max()
    assert abs(float(on["loss"]) - float(off["loss"])) <= 1e-2 * abs(float(off["loss"]))


def test_zero_invariant_survives_the_kernel_probes(runs):
    """step -> every kernel_probes() closure once -> step: the non-class rows of du_l[L-1], dx_mid[L-1] and the top block's
    d(attention output) buffer are exactly zero afterwards, and that step's gradients pass the gates."""
    tag = "rope-axial"
    run = runs(tag, "1", True)
    for name in ("du", "dx_mid", "da"):
        assert int(run["nonzero_" + name]) == 0, name
        assert float(run["class_" + name]) > 0.0, name       # (the class rows were written)
    bad, _ = _gate(tag, run, tag + "/cls_rows_after_probes")
    assert not bad, bad


def test_evaluation_forward_equals_the_full_row_path(runs):
    """forward_only at a ragged batch (17 images in an engine of 32): bf16 logits gate of test_model_gpu.py (5e-2)"""
    on, off = runs("rope-axial", "1"), runs("rope-axial", "0")
    assert on["eval_logits"].shape == (17, 10)
    assert rel_err(on["eval_logits"], off["eval_logits"]) < 5e-2


if __name__ == "__main__" and len(sys.argv) == 5 and sys.argv[1] == "child":
    for p_ in (REPO, os.path.join(REPO, "vit-rpe-rope_amd"), os.path.join(REPO, "tests")):
        if p_ not in sys.path:
            sys.path.insert(0, p_)
    _child(sys.argv[2], sys.argv[3], sys.argv[4] == "1")
