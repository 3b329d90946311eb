"""TrainEngine(extras=True): qkv bias, dropout, attention dropout and stochastic depth on the engine's per-Linear route, the
site table that feeds its kernels, and the two kernels the route adds (vitpe_branch_drop_*, vitpe_rng_advance).

Yardstick of the engine: the module path (VisionTransformer.train() under torch autograd), which test_dropout_gpu.py pins to
the reference's golden block.  Both sides get the same masks: the module model runs first, the pairs it drew (last_rng of
every block) are written into a table in the documented order and copied into the engine.  Gates: fp32 logits / loss 1e-4,
gradients 1e-3 per tensor (test_model_gpu.py); bf16 per tensor rel <= 5e-2 and cosine >= 0.999 (test_bench_path_gpu.py).
"""
import copy
import csv

import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import vit_oracle as O

pytestmark = pytest.mark.gpu

SMALL = dict(img_size=32, patch_size=8, embed_dim=96, num_heads=3, depth=3)     # N = 17: two token tiles
WIDE = dict(img_size=32, patch_size=4, embed_dim=192, num_heads=6, depth=2)     # N = 65: the fused kernels' geometry
RATES = dict(qkv_bias=True, drop_rate=0.1, attn_drop_rate=0.15, drop_path_rate=0.3)
MODES = ["none", "absolute", "relative", "polynomial", "rope-axial", "rope-mixed"]
DT = {"f32": torch.float32, "bf16": torch.bfloat16}


@pytest.fixture(scope="module")
def K():
    from vitpe import kernels
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return kernels


def pair(seed, offset):
    return torch.tensor([seed, offset], dtype=torch.int64, device="cuda")


def cosine(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(a @ b / max(np.linalg.norm(a) * np.linalg.norm(b), 1e-300))


# ---- vitpe_branch_drop_* against the two kernels it replaces -----------------------------------------------------------------
def _offset_by_one(t):
    """the same values in storage that starts one element off the allocation's alignment (scalar path)"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    return v


@pytest.mark.parametrize("unaligned", [False, True])
@pytest.mark.parametrize("sites", ["elem", "path", "both"])
@pytest.mark.parametrize("B", [5, 1])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_branch_drop_equals_the_two_kernels(K, dt, B, sites, unaligned):
    per, p_e, p_p = 17 * 96, 0.25, 0.4
    g = torch.Generator().manual_seed(11 + B)
    x, r, dy = (torch.randn(B, 17, 96, generator=g).cuda().to(DT[dt]) for _ in range(3))
    # (pairs whose per-sample stream keeps some samples and drops some at B = 5; B = 1: one kept, one dropped below)
    rng_e = pair(77, 1234567) if sites != "path" else None
    for rng_p in ([pair(5, 6), pair(5, 7), pair(5, 8)] if sites != "elem" else [None]):
        for resid in (r, None):
            t = x
            if rng_e is not None:
                t = K.dropout_fwd(t, rng_e, p_e, resid=resid if rng_p is None else None)
            if rng_p is not None:
                t = K.drop_path_fwd(t, rng_p, p_p, resid=resid)
            args = [x, resid]
            if unaligned:
                args = [_offset_by_one(x), None if resid is None else _offset_by_one(resid)]
                out = torch.full((x.numel() + 2,), float("nan"), dtype=DT[dt], device="cuda")
                got = K.branch_drop_fwd(args[0], rng_e, p_e, rng_p, p_p, resid=args[1], out=out[1:-1].view(x.shape))
                assert torch.isnan(out[0]) and torch.isnan(out[-1])
            else:
                got = K.branch_drop_fwd(x, rng_e, p_e, rng_p, p_p, resid=resid)
            assert torch.isfinite(got).all() and torch.equal(got, t), (sites, resid is None)
        want = dy
        if rng_e is not None:
            want = K.dropout_bwd(want, rng_e, p_e)
        if rng_p is not None:
            want = K.drop_path_bwd(want, rng_p, p_p)
        src = _offset_by_one(dy) if unaligned else dy
        assert torch.equal(K.branch_drop_bwd(src, rng_e, p_e, rng_p, p_p), want), sites


def test_branch_drop_masks_both_ways(K):
    """the fixed pairs of the test above really drop and keep: samples and elements (else equality would show nothing)"""
    x = torch.ones(5, 17, 96, device="cuda")
    y = K.branch_drop_fwd(x, pair(77, 1234567), 0.25, pair(5, 6), 0.4)
    kept = (y != 0).flatten(1).any(1)
    assert 0 < int(kept.sum()) < 5
    frac = float((y[kept] != 0).float().mean())
    assert 0.6 < frac < 0.9
    assert torch.allclose(y[y != 0], torch.tensor(1 / 0.75 / 0.6, device="cuda"), rtol=1e-6)
    ones = {float(K.branch_drop_fwd(x[:1], None, 0., pair(5, s), 0.4).flatten()[0]) != 0 for s in (6, 7, 8)}
    assert ones == {True, False}                          # B = 1 above sees a kept and a dropped sample


def test_branch_drop_bad_arguments_launch_nothing(K):
    from vitpe import _lib as L
    h = L.lib()
    rng = pair(1, 2)
    x = torch.full((64,), float("nan"), device="cuda")
    y = torch.full((64,), float("nan"), device="cuda")
    st = L.stream_ptr()
    xp, yp, rp = x.data_ptr(), y.data_ptr(), rng.data_ptr()
    assert h.vitpe_branch_drop_fwd(0, xp, None, yp, 4, 16, None, 0.1, None, 0.1, st) == 1        # both sites null
    assert h.vitpe_branch_drop_bwd(0, xp, yp, 4, 16, None, 0.1, None, 0.1, st) == 1
    assert h.vitpe_branch_drop_fwd(0, xp, None, yp, 4, 15, rp, 0.1, rp, 0.1, st) == 1            # per % 4 != 0
    assert h.vitpe_branch_drop_bwd(0, xp, yp, 4, 14, rp, 0.1, None, 0.0, st) == 1
    for p in (-0.1, 1.0, float("nan")):
        assert h.vitpe_branch_drop_fwd(0, xp, None, yp, 4, 16, rp, p, None, 0.0, st) == 1
        assert h.vitpe_branch_drop_fwd(0, xp, None, yp, 4, 16, None, 0.0, rp, p, st) == 1
    assert h.vitpe_branch_drop_fwd(2, xp, None, yp, 4, 16, rp, 0.1, rp, 0.1, st) == 1            # unknown dtype
    assert h.vitpe_branch_drop_fwd(0, None, None, yp, 4, 16, rp, 0.1, rp, 0.1, st) == 1
    assert h.vitpe_rng_advance(None, 3, 1, st) == 1
    assert h.vitpe_rng_advance(rp, -1, 1, st) == 1
    torch.cuda.synchronize()
    assert torch.isnan(y).all() and rng.tolist() == [1, 2]
    with pytest.raises(L.VitpeError):
        K.branch_drop_fwd(x.view(4, 16), None, 0.1, None, 0.1)


# ---- vitpe_rng_advance --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 300])
def test_rng_advance(K, n):
    g = torch.Generator().manual_seed(n)
    t = torch.randint(-2 ** 62, 2 ** 62, (n, 2), generator=g, dtype=torch.int64)
    t[0, 1] = -1                                          # 2^64 - 1 as the kernels read it: wraps
    d = t.cuda()
    inc = 5
    K.rng_advance(d, inc)
    got = d.cpu()
    assert torch.equal(got[:, 0], t[:, 0])
    assert int(got[0, 1]) == inc - 1
    assert torch.equal(got[1:, 1], t[1:, 1] + inc)
    K.rng_advance(d, 2 ** 64 - inc)                       # the full uint64 range of inc: back where it started
    assert torch.equal(d.cpu(), t)


def test_rng_advance_of_nothing(K):
    from vitpe import _lib as L
    K.rng_advance(torch.empty((0, 2), dtype=torch.int64, device="cuda"))
    d = torch.tensor([[3, 4]], dtype=torch.int64, device="cuda")
    assert L.lib().vitpe_rng_advance(d.data_ptr(), 0, 9, L.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert d.tolist() == [[3, 4]]


# ---- engine against the module path ---------------------------------------------------------------------------------------
def make_model(pos, geom, opts, seed=0):
    from models.vit import VisionTransformer
    torch.manual_seed(seed)
    model = VisionTransformer(pos_encoding=pos, **geom, **opts)
    with torch.no_grad():   # (the init leaves biases, the class token and some PE parameters at zero: move everything)
        for p in model.parameters():
            p.add_(torch.randn_like(p) * 0.02)
    return model


def batch(model, B, salt):
    g = torch.Generator().manual_seed(100 + salt)
    C = model.patch_embed.weight.shape[1]
    S = int(round(model.num_patches ** 0.5)) * model.patch_size
    return torch.randn(B, C, S, S, generator=g).cuda(), torch.randint(0, model.num_classes, (B,), generator=g).cuda()


def module_path(model, images, labels, dtype):
    """forward, CE, backward of the module model -> (logits, loss, {name: grad}, site table [6 depth, 2] on the device)"""
    from vitpe.engine import SITES_PER_LAYER, SITE_ATTN, SITE_MLP1, SITE_PATH_A, SITE_PROJ, SITE_MLP2, SITE_PATH_M
    ref = copy.deepcopy(model).cuda().set_compute_dtype(dtype).train()
    logits = ref(images)
    loss = torch.nn.functional.cross_entropy(logits.float(), labels)
    loss.backward()
    table = torch.zeros(SITES_PER_LAYER * len(ref.blocks), 2, dtype=torch.int64, device="cuda")
    for l, blk in enumerate(ref.blocks):
        for src, sites in ((blk.attn.last_rng, (SITE_ATTN, SITE_PROJ)), (blk.mlp.last_rng, (SITE_MLP1, SITE_MLP2)),
                           (blk.last_rng, (SITE_PATH_A, SITE_PATH_M))):
            if src is not None:
                for row, site in zip(src, sites):
                    table[SITES_PER_LAYER * l + site] = row
    grads = {n: p.grad.detach().float().cpu() for n, p in ref.named_parameters()}
    return logits.detach().float().cpu(), float(loss.detach()), grads, table


def engine_on(model, images, labels, dtype, table=None, use_graph=False, **kw):
    from vitpe.engine import TrainEngine
    eng = TrainEngine(copy.deepcopy(model).cuda(), images.shape[0], compute_dtype=dtype, use_graph=use_graph, extras=True, **kw)
    if table is not None:
        eng.set_rng_table(table)
    eng.images.copy_(images); eng.labels.copy_(labels)
    return eng


def check_fp32(eng, logits, loss, grads):
    assert rel_err(eng.logits.cpu(), logits) < 1e-4
    assert abs(float(eng.out2[0]) - loss) < 1e-4
    for n, p in eng.model.named_parameters():
        ref = grads[n]
        if float(ref.abs().max()) == 0.0:
            assert float(p.grad.abs().max()) == 0.0, n
            continue
        assert rel_err(p.grad.cpu(), ref) < 1e-3, n


@pytest.mark.parametrize("pos", MODES)
def test_engine_fp32_matches_the_module_path(K, pos):
    model = make_model(pos, SMALL, RATES, seed=1)
    images, labels = batch(model, 6, 1)
    torch.manual_seed(7)
    logits, loss, grads, table = module_path(model, images, labels, torch.float32)
    assert int((table != 0).any(1).sum()) == 6 * 3 - 2      # every site drew a pair but block 0's two drop-path sites
    eng = engine_on(model, images, labels, torch.float32, table)
    eng.forward_backward()
    check_fp32(eng, logits, loss, grads)
    assert "blocks.0.attn.qkv.bias" in grads and all(n in grads for n, _ in eng.model.named_parameters())
    assert int(torch.count_nonzero(eng.model.blocks[0].attn.qkv.bias.grad)) > 0
    # the masks matter: another table gives other logits
    eng.set_rng_table(table + 1)
    eng.forward_backward()
    assert rel_err(eng.logits.cpu(), logits) > 1e-3


DROP_KERNELS = ["dropout_fwd", "dropout_bwd", "drop_path_fwd", "drop_path_bwd", "branch_drop_fwd", "branch_drop_bwd",
                "attention_core_fwd_drop", "attention_core_bwd_drop"]


def spy(monkeypatch, K):
    calls = {}
    for name in DROP_KERNELS:
        def wrap(*a, _f=getattr(K, name), _n=name, **kw):
            calls[_n] = calls.get(_n, 0) + 1
            return _f(*a, **kw)
        monkeypatch.setattr(K, name, wrap)
    return calls


@pytest.mark.parametrize("opt", ["qkv_bias", "drop_rate", "attn_drop_rate", "drop_path_rate"])
def test_each_option_alone(K, monkeypatch, opt):
    opts = {opt: True if opt == "qkv_bias" else RATES[opt]}
    model = make_model("rope-mixed", SMALL, opts, seed=2)
    images, labels = batch(model, 6, 2)
    torch.manual_seed(8)
    logits, loss, grads, table = module_path(model, images, labels, torch.float32)
    eng = engine_on(model, images, labels, torch.float32, table)
    calls = spy(monkeypatch, K)
    eng.forward_backward()
    check_fp32(eng, logits, loss, grads)
    L = 3
    want = {"qkv_bias": {},
            "drop_rate": dict(dropout_fwd=L, dropout_bwd=L, branch_drop_fwd=2 * L, branch_drop_bwd=2 * L),
            "attn_drop_rate": dict(attention_core_fwd_drop=L, attention_core_bwd_drop=L),
            "drop_path_rate": dict(branch_drop_fwd=2 * (L - 1), branch_drop_bwd=2 * (L - 1))}[opt]   # block 0: rate 0
    assert calls == want
    if opt == "qkv_bias":
        assert int(torch.count_nonzero(eng.model.blocks[0].attn.qkv.bias.grad)) > 0


@pytest.mark.parametrize("pos", ["rope-axial", "relative"])
def test_wide_geometry_bf16_all_options(K, pos):
    model = make_model(pos, WIDE, RATES, seed=3)
    images, labels = batch(model, 3, 3)
    assert K.fused_attention_supported(torch.bfloat16, 65, 192, 32)     # what the default engine would take here
    torch.manual_seed(9)
    logits, loss, grads, table = module_path(model, images, labels, torch.bfloat16)
    eng = engine_on(model, images, labels, torch.bfloat16, table)
    assert eng.attn_fused is False and not (eng.fuse_ln or eng.tail2 or eng.cls_rows or eng.attn_fused64)
    eng.forward_backward()
    worst = dict(rel=0.0, cos=1.0)
    r = rel_err(eng.logits.cpu(), logits)
    print(f"extras bf16 {pos}: logits rel {r:.2e}")
    assert r <= 5e-2
    bad = []
    for n, p in eng.model.named_parameters():
        mine, ref = p.grad.cpu().numpy(), grads[n].numpy()
        if float(np.abs(ref).max()) == 0.0:
            assert float(np.abs(mine).max()) == 0.0, n
            continue
        r, c = rel_err(mine, ref), cosine(mine, ref)
        worst = dict(rel=max(worst["rel"], r), cos=min(worst["cos"], c))
        if r > 5e-2 or c < 0.999:
            bad.append((n, r, c))
    print(f"extras bf16 {pos}: worst gradient rel {worst['rel']:.2e} cos {worst['cos']:.6f}")
    assert not bad, bad


def test_captured_step_advances_the_table_and_eval_is_clean(K):
    """3 steps, eager and captured, from one initial table: same losses, offsets + 3, seeds untouched, nothing left by the
    capture warm-up; the calls that are no step leave the table alone; evaluation = the module model in eval mode."""
    model = make_model("rope-axial", SMALL, RATES, seed=4)
    images, labels = batch(model, 6, 4)
    torch.manual_seed(10)
    table0 = K.new_rng_pairs(6 * 3, "cuda")
    table0[0, 1] = -2                                       # (an offset that wraps during the steps)
    losses, engines = {}, {}
    for use_graph in (False, True):
        eng = engine_on(model, images, labels, torch.float32, table0, use_graph=use_graph, lr=1e-3)
        assert torch.equal(eng.rng_table, table0)
        before = K.dropout_mask(eng.rng_table[1], 0.1, n=6 * 17 * 96).clone()
        ls = []
        for _ in range(3):
            eng.step()
            ls.append(eng.read_metrics()[0])
        losses[use_graph], engines[use_graph] = ls, eng
        t = eng.rng_table.cpu()
        assert torch.equal(t[:, 0], table0[:, 0].cpu())
        assert torch.equal(t[:, 1], table0[:, 1].cpu() + 3) and int(t[0, 1]) == 1
        assert not torch.equal(K.dropout_mask(eng.rng_table[1], 0.1, n=6 * 17 * 96), before)
    assert all(np.isfinite(losses[True])) and np.allclose(losses[True], losses[False], rtol=5e-3), losses
    for eng in engines.values():
        t = eng.rng_table.clone()
        eng.forward_backward()
        eng.flat_g.zero_()
        a = eng.forward_only(images).clone()
        eng.eval_loss(6, torch.zeros(2, device="cuda"))
        b = eng.forward_only(images)
        assert torch.equal(eng.rng_table, t)
        assert torch.equal(a, b)                              # no dropout in an evaluation forward
        ref = copy.deepcopy(model).cuda().eval()
        ref.load_state_dict(eng.model.state_dict())
        with torch.no_grad():
            want = ref(images)
        assert rel_err(a.cpu(), want.cpu()) < 1e-4
    with pytest.raises(NotImplementedError, match="extras"):
        engines[True].kernel_probes()


def test_extras_on_a_plain_model_matches_the_oracle(K):
    """the forced per-Linear route at the fused kernels' geometry, no option active: the comparator of the default route.
    The table exists and advances by one per step (the advance is the route's, not a site's)."""
    from models.vit import VisionTransformer
    kw = dict(pos_encoding="rope-mixed", depth=2)
    cfg = O.VitConfig(**kw)
    model = VisionTransformer(**kw)
    with torch.no_grad():
        for n, p in model.named_parameters():
            p.copy_(O.closed_form_tensor(n, tuple(p.shape), cfg))
    params = {n: p.detach().clone() for n, p in model.named_parameters()}
    images, labels = O.closed_form_batch(cfg, 5, salt=2)
    ref_logits, ref_loss, ref_grads = O.loss_and_grads(cfg, params, images, labels)
    eng = engine_on(model, images.cuda(), labels.cuda(), torch.float32)
    assert not (eng.attn_fused or eng.attn_wide or eng.fuse_ln or eng.fuse_ln_bwd or eng.tail2 or eng.lnbwd2
                or eng.fuse_lnbwd or eng.cls_rows or eng.attn_fused64) and len(eng.qkv_l) == 2
    eng.forward_backward()
    assert rel_err(eng.logits.cpu(), ref_logits) < 1e-4
    for n, p in eng.model.named_parameters():
        assert rel_err(p.grad.cpu(), ref_grads[n]) < 1e-3, n
    t = eng.rng_table.clone()
    assert tuple(t.shape) == (12, 2)
    eng.flat_g.zero_()
    eng.step()
    assert torch.equal(eng.rng_table[:, 1], t[:, 1] + 1) and torch.equal(eng.rng_table[:, 0], t[:, 0])


def test_train_py_with_engine_extras(tmp_path):
    import train as T
    T.main(["--engine_extras", "--qkv_bias", "--drop", "0.1", "--attn_drop", "0.1", "--drop_path", "0.1", "--synthetic",
            "--epochs", "1", "--steps_per_epoch", "3", "--batch_size", "32",
            "--log_dir", str(tmp_path / "logs"), "--ckpt_dir", str(tmp_path / "ckpt")])
    logs = list((tmp_path / "logs").glob("mnist_absolute_*.csv"))
    assert len(logs) == 1
    rows = list(csv.DictReader(open(logs[0])))
    assert len(rows) == 1
    assert np.isfinite(float(rows[0]["train_loss"])) and np.isfinite(float(rows[0]["test_loss"]))
    sd = torch.load(tmp_path / "ckpt" / "mnist_absolute_best.pth", map_location="cpu")
    assert "blocks.0.attn.qkv.bias" in sd and "rng_table" not in sd
