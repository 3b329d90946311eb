"""The attention core at head dimensions 24, 48, 96 and 128 (d = 192 at H = 8 / 4 / 2, d = 384 at H = 3 ...): kernel parity
through the C ABI against the CPU oracle, column ownership of the padded heads (24 / 48 run on 32- / 64-wide tiles), the
support query, the TrainEngine and the drop-in model against the oracle and the reference's own numbers (golden/heads.npz),
and train.py at the head counts this opens.

Tolerances are the ones of the existing suite: kernels 1e-4 (fp32) / 3e-2 (bf16), frequency gradients max(tol, 2e-4)
(test_kernels_gpu.py); engine and drop-in model 1e-4 on logits and loss, 1e-3 on gradients (test_bench_path_gpu.py,
test_model_gpu.py).
"""
import csv

import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import vit_oracle as O
from test_kernels_gpu import ATTN_MODES, DT, attn_case, core_qkv, dev, device_pe, oracle_attn, tol

pytestmark = pytest.mark.gpu

NEW_HDS = (24, 48, 96, 128)
# (head dimension, heads, model width) at N = 65
HD_GEOMS = [(24, 8, 192), (48, 4, 192), (96, 2, 192), (128, 3, 384)]
# token counts of the compiled tile counts MT = 2, 4, 5, 10, 13, 17
TOKENS = (17, 50, 65, 145, 197, 257)
# (dtype, head dimension) -> tile counts whose two backward LDS tiles do not fit 160 KB
REFUSED_MT = {("bf16", 128): {17}, ("f32", 96): {13, 17}, ("f32", 128): {10, 13, 17}}


@pytest.fixture(scope="module")
def K():
    from vitpe import kernels
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return kernels


def run_core(K, mode, D, H, B, G, dt, seed):
    """attention_core_fwd / _bwd against O.attention_core + autograd: output, dqkv and the PE-parameter gradients."""
    N, hd, G, xn, wqkv, dout, pe = attn_case(mode, D, H, B, seed=seed, G=G)
    # logit spread grows with the width of the projection and with sqrt(hd): hd 96 at d = 192 is brought back to the
    # spread of the existing core cases (d 128 / hd 64), as d > 200 is by test_kernels_gpu.py.  Unscaled, the bf16
    # per-head polynomial-coefficient gradient at N = 197 (sums of dS x distance^k over 197^2 pairs) lands at 3.5e-2 of
    # the oracle; the same kernel in fp32 meets 1e-4 unscaled (test_attention_core_hd96_n145_f32).
    wqkv = wqkv * (0.3 if D > 200 else 0.6 if hd > 64 else 1.0)
    ref, dqkv_ref, g_ref = oracle_attn(mode, xn, wqkv, dout, pe, H, dt)
    t = device_pe(K, mode, pe, H, G)
    qkv = dev(core_qkv(xn, wqkv, dt), DT[dt])
    out = K.attention_core_fwd(qkv, H, t)
    assert rel_err(out.float().cpu(), ref) < tol(dt)
    dtab = torch.zeros(H, 2 * N - 1, device="cuda") if mode == "relative" else None
    dcoef = torch.zeros_like(dev(pe["coeff"])) if mode.startswith("polynomial") else None
    dfr = torch.zeros(2, H, hd // 2, device="cuda") if mode == "rope-mixed" else None
    dqkv = K.attention_core_bwd(qkv, dev(dout, DT[dt]), H, t, dtab, dcoef, dfr)
    assert rel_err(dqkv.float().cpu(), dqkv_ref) < tol(dt)
    if mode == "relative":
        assert rel_err(dtab.cpu(), g_ref["table"]) < tol(dt)
    if mode.startswith("polynomial"):
        assert rel_err(dcoef.cpu(), g_ref["coeff"]) < tol(dt)
    if mode == "rope-mixed":
        assert rel_err(dfr.cpu(), g_ref["freqs"]) < max(tol(dt), 2e-4)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("mode", ATTN_MODES)
@pytest.mark.parametrize("hd,H,D", HD_GEOMS)
def test_attention_core_new_head_dims_n65(K, dt, mode, hd, H, D):
    assert D == hd * H
    run_core(K, mode, D, H, 2, 8, dt, seed=60)


@pytest.mark.parametrize("mode", ATTN_MODES)
@pytest.mark.parametrize("hd,H", [(24, 8), (48, 4), (96, 2)])
def test_attention_core_new_head_dims_n197_bf16(K, mode, hd, H):
    run_core(K, mode, hd * H, H, 1, 14, "bf16", seed=70)


@pytest.mark.parametrize("mode", ATTN_MODES)
def test_attention_core_hd96_n145_f32(K, mode):
    """fp32 hd 96 runs up to 10 tiles (its two backward tiles do not fit at 13): the largest token count it has, at the
    exact-fp32 tolerance, with the unscaled projection"""
    N, hd, G, xn, wqkv, dout, pe = attn_case(mode, 192, 2, 1, seed=75, G=12)
    assert N == 145 and hd == 96
    ref, dqkv_ref, g_ref = oracle_attn(mode, xn, wqkv, dout, pe, 2, "f32")
    t = device_pe(K, mode, pe, 2, G)
    qkv = dev(core_qkv(xn, wqkv, "f32"), torch.float32)
    assert rel_err(K.attention_core_fwd(qkv, 2, t).cpu(), ref) < tol("f32")
    dtab = torch.zeros(2, 2 * N - 1, device="cuda") if mode == "relative" else None
    dcoef = torch.zeros_like(dev(pe["coeff"])) if mode.startswith("polynomial") else None
    dfr = torch.zeros(2, 2, hd // 2, device="cuda") if mode == "rope-mixed" else None
    dqkv = K.attention_core_bwd(qkv, dev(dout), 2, t, dtab, dcoef, dfr)
    assert rel_err(dqkv.cpu(), dqkv_ref) < tol("f32")
    if mode == "relative":
        assert rel_err(dtab.cpu(), g_ref["table"]) < tol("f32")
    if mode.startswith("polynomial"):
        assert rel_err(dcoef.cpu(), g_ref["coeff"]) < tol("f32")
    if mode == "rope-mixed":
        assert rel_err(dfr.cpu(), g_ref["freqs"]) < 2e-4


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("hd,H", [(24, 8), (48, 4), (96, 2), (128, 3)])
def test_attention_core_new_head_dims_n17(K, dt, hd, H):
    run_core(K, "rope-mixed", hd * H, H, 2, 4, dt, seed=80)


def guarded(shape, dtype, guard=64):
    """a NaN-filled buffer: the tensor of `shape` followed by `guard` NaN elements"""
    n = int(np.prod(shape))
    buf = torch.full((n + guard,), float("nan"), device="cuda", dtype=dtype)
    return buf, buf[:n].view(*shape)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("mode", ["none", "relative", "rope-axial", "rope-mixed"])
@pytest.mark.parametrize("hd,H", [(24, 4), (48, 3)])
def test_padded_heads_write_only_their_own_columns(K, dt, mode, hd, H):
    """hd 24 / 48 run on 32- / 64-wide tiles: a store of a padded feature would land in the next head's columns (or past
    the end of the row).  Every head gets its own scale, the outputs start as NaN and end in a NaN guard: a write into a
    neighbour breaks parity, a missing write leaves a NaN, a write past the end clears the guard.  Three launches
    give bit-identical results."""
    B, G = 2, 8
    D = hd * H
    N, _, G, xn, wqkv, dout, pe = attn_case(mode, D, H, B, seed=90, G=G)
    # head h of q, k and v scaled by 1 + h / 2 (the rows of wqkv that produce it), and of the output gradient likewise
    head_scale = (1.0 + 0.5 * torch.arange(H, dtype=torch.float32)).repeat_interleave(hd)
    wqkv = wqkv * head_scale.repeat(3)[:, None] * 0.7
    dout = dout * head_scale
    ref, dqkv_ref, _ = oracle_attn(mode, xn, wqkv, dout, pe, H, dt)
    t = device_pe(K, mode, pe, H, G)
    qkv = dev(core_qkv(xn, wqkv, dt), DT[dt])
    do = dev(dout, DT[dt])
    outs, dqkvs = [], []
    for _ in range(3):
        obuf, out = guarded((B, N, D), DT[dt])
        gbuf, dqkv = guarded((B, N, 3 * D), DT[dt])
        K.attention_core_fwd(qkv, H, t, out=out)
        dtab = torch.zeros(H, 2 * N - 1, device="cuda") if mode == "relative" else None
        dfr = torch.zeros(2, H, hd // 2, device="cuda") if mode == "rope-mixed" else None
        K.attention_core_bwd(qkv, do, H, t, dtab, None, dfr, out=dqkv)
        torch.cuda.synchronize()
        assert torch.isnan(obuf[B * N * D:]).all() and torch.isnan(gbuf[B * N * 3 * D:]).all()
        assert torch.isfinite(out).all() and torch.isfinite(dqkv).all()
        outs.append(out.cpu())
        dqkvs.append(dqkv.cpu())
    assert rel_err(outs[0].float(), ref) < tol(dt)
    assert rel_err(dqkvs[0].float(), dqkv_ref) < tol(dt)
    for h in range(H):   # per head as well: a small head must not hide in a large one's error budget
        cols = slice(h * hd, (h + 1) * hd)
        assert rel_err(outs[0].float()[..., cols], ref[..., cols]) < tol(dt), h
    for i in (1, 2):
        assert torch.equal(outs[i], outs[0]) and torch.equal(dqkvs[i], dqkvs[0])


def test_support_query_covers_the_new_head_dims(K):
    from vitpe._lib import VitpeError
    from vitpe.kernels import PETables
    for dt in ("f32", "bf16"):
        for hd in NEW_HDS:
            for n in TOKENS:
                mt = (n + 15) // 16
                want = mt not in REFUSED_MT.get((dt, hd), set())
                assert K.attention_core_supported(DT[dt], n, hd) == want, (dt, hd, n)
        for hd in (16, 12, 40, 8, 256):
            assert not K.attention_core_supported(DT[dt], 65, hd), (dt, hd)
        for hd in NEW_HDS:
            assert not K.attention_core_supported(DT[dt], 101, hd), (dt, hd)
    with pytest.raises(VitpeError):   # 101 tokens (7 tiles) at hd 24
        K.attention_core_fwd(torch.zeros(1, 101, 3 * 48, device="cuda"), 2, PETables("none", 10))
    with pytest.raises(VitpeError):   # hd 40
        K.attention_core_fwd(torch.zeros(1, 65, 3 * 80, device="cuda"), 2, PETables("none", 8))
    with pytest.raises(VitpeError):   # fp32 hd 128 at 197 tokens: the backward tiles do not fit
        K.attention_core_fwd(torch.zeros(1, 197, 3 * 256, device="cuda"), 2, PETables("none", 14))


@pytest.mark.parametrize("heads", [8, 4])
@pytest.mark.parametrize("tag", ["rope-mixed", "relative"])
def test_engine_at_the_new_head_counts(heads, tag):
    """TrainEngine at d = 192, H = 8 (hd 24) / 4 (hd 48): the unfused path (qkv Linear + attention core); fp32 logits,
    loss and every gradient against the oracle, then three captured bf16 steps stay finite."""
    from test_bench_path_gpu import build
    from vitpe.engine import TrainEngine
    geom = dict(depth=1, embed_dim=192, num_heads=heads)
    cfg, model = build(tag, {}, geom)
    params = {n: p.detach().cpu().clone() for n, p in model.named_parameters()}
    B = 3
    images, labels = O.closed_form_batch(cfg, B, salt=7)
    ref_logits, ref_loss, ref_grads = O.loss_and_grads(cfg, params, images, labels)
    eng = TrainEngine(model, B, compute_dtype=torch.float32, use_graph=False)
    assert not eng.attn_fused
    eng._load_batch(images.cuda(), labels.cuda())
    eng.forward_backward()
    assert rel_err(eng.logits.cpu(), ref_logits) < 1e-4
    assert abs(float(eng.out2[0]) - float(ref_loss)) < 1e-4
    for n, p in model.named_parameters():
        assert rel_err(p.grad.cpu(), ref_grads[n]) < 1e-3, n
    cfg, model = build(tag, {}, geom, seeded=True)
    eb = TrainEngine(model, B, compute_dtype=torch.bfloat16, use_graph=True)
    for _ in range(3):
        eb.step(images.cuda(), labels.cuda())
    torch.cuda.synchronize()
    assert torch.isfinite(eb.flat_p).all()


HEADS_MODELS = [("rope-mixed", {}, 192, 8), ("relative", {}, 192, 8),
                ("polynomial_perhead", {"pos_encoding": "polynomial", "poly_shared_heads": False}, 192, 8),
                ("rope-mixed", {}, 192, 4), ("relative", {}, 192, 4),
                ("polynomial_perhead", {"pos_encoding": "polynomial", "poly_shared_heads": False}, 192, 4),
                ("rope-axial", {}, 384, 3)]


@pytest.mark.parametrize("tag,extra,D,H", HEADS_MODELS)
def test_dropin_model_vs_reference_golden_at_new_head_dims(golden, tag, extra, D, H):
    """models.vit.VisionTransformer (depth 1, fp32) against the reference's own logits, loss and the gradients of the
    positional parameters and of blocks.0.attn.qkv.weight (tools/make_golden.py gen_heads)."""
    from models.vit import VisionTransformer
    g = golden("heads")
    key = f"d{D}_h{H}/{tag}"
    kw = dict(pos_encoding=extra.get("pos_encoding", tag), embed_dim=D, depth=1, num_heads=H)
    kw.update({k: v for k, v in extra.items() if k != "pos_encoding"})
    cfg = O.VitConfig(**kw)
    model = VisionTransformer(**kw)
    with torch.no_grad():
        for n, p in model.named_parameters():
            p.copy_(O.closed_form_tensor(n, tuple(p.shape), cfg))
    model = model.cuda().set_compute_dtype(torch.float32)
    images, labels = O.closed_form_batch(cfg, 2)
    logits = model(images.cuda())
    loss = torch.nn.CrossEntropyLoss()(logits, labels.cuda())
    loss.backward()
    assert rel_err(logits.detach().cpu(), g[f"{key}/logits"]) < 1e-4
    assert abs(float(loss) - float(g[f"{key}/loss"])) < 1e-4
    grads = dict(model.named_parameters())
    names = [k.split("/grad/")[1] for k in g.files if k.startswith(f"{key}/grad/")]
    assert len(names) == (tag != "rope-axial")   # the positional parameters (rope-axial has none)
    for name in names:
        assert rel_err(grads[name].grad.cpu().numpy(), g[f"{key}/grad/{name}"]) < 1e-3, name
    # the qkv-weight gradient: a row sample that holds rows of every head of q, k and v (tools/make_golden.py)
    rows = g[f"{key}/qkv_rows"]
    assert set((rows % D) // (D // H)) == set(range(H))
    dw = grads["blocks.0.attn.qkv.weight"].grad.cpu().numpy()[rows]
    assert rel_err(dw, g[f"{key}/grad_rows/blocks.0.attn.qkv.weight"]) < 1e-3


def test_train_py_accepts_and_runs_the_new_head_counts(tmp_path):
    """get_args() accepts --num_heads 8 / 4 / 2 at d = 192 and --embed_dim 384 --num_heads 3; a synthetic run of two short
    epochs at --num_heads 8 writes its CSV."""
    import train as T
    for ok in (["--num_heads", "8"], ["--num_heads", "4"], ["--num_heads", "2"], ["--embed_dim", "384", "--num_heads", "3"]):
        T.get_args(ok)
    with pytest.raises(SystemExit):
        T.get_args(["--num_heads", "12"])
    T.main(["--dataset", "cifar10", "--pos_encoding", "rope-mixed", "--batch_size", "16", "--epochs", "2", "--synthetic",
            "--steps_per_epoch", "3", "--depth", "2", "--num_heads", "8",
            "--log_dir", str(tmp_path / "logs"), "--ckpt_dir", str(tmp_path / "ckpt")])
    logs = list((tmp_path / "logs").glob("cifar10_rope-mixed_*.csv"))
    assert len(logs) == 1
    with open(logs[0]) as f:
        rows = list(csv.reader(f))
    assert rows[0][0] == "epoch" and [r[0] for r in rows[1:]] == ["1", "2"]
    assert all(np.isfinite(float(v)) for r in rows[1:] for v in r[1:])
