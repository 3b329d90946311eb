"""End-to-end parity of the path bench.py times: the bf16 TrainEngine with its default fusions (LayerNorm-fused attention
forward, block-tail forward / backward kernels, grouped weight gradients) INSIDE the captured HIP graph, at the full
geometries of BASELINE.json -- logits, loss and EVERY parameter gradient against the CPU oracle (fp32, reference op
order) evaluated on the same bf16-representable weights.

The captured step ends in AdamW, which zeroes the gradient buffer; after the FIRST step the first moment is
m = (1 - beta1) * g, so the gradients the graph computed are read back as flat_m / (1 - beta1).

Tolerances (bf16 activations carry 8 significant bits through 6 resp. 12 layers; stated per check):
  logits     max|a-b| / max|b| <= 5e-2
  loss       |a-b| <= 2e-2
  every grad max-norm rel <= 5e-2  AND  cosine >= 0.999
  dWqkv / d table / d freqs / d coeff additionally per ROW: ||row_a - row_b||_2 <= 0.08 ||row_b||_2 + 0.01 max_row||row_b||_2
  (the floor only admits rows whose whole norm is below 1 % of the largest row's -- they are dominated by rounding).
  one tensor, one case: the SHARED polynomial coefficients at B = 512 -- max-norm error <= 5e-2 of the size of the summands
  before they cancel (_summand_scale), instead of the cancelled sum.
"""
import json
import os

import numpy as np
import pytest
import torch

from conftest import REPO, rel_err
from oracle import vit_oracle as O

pytestmark = pytest.mark.gpu

MODES = [("none", {}), ("absolute", {}), ("relative", {}), ("polynomial", {}),
         ("polynomial_perhead", {"pos_encoding": "polynomial", "poly_shared_heads": False}),
         ("rope-axial", {}), ("rope-mixed", {})]
ROW_CHECKED = ("attn.qkv.weight", "relative_position_bias_table", "pos_embed.freqs", "pos_embed.coefficients")


def bf16_round_(model):
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(p.to(torch.bfloat16).to(torch.float32))


def build(tag, extra, geom, seeded=False):
    from models.vit import VisionTransformer
    kw = dict(pos_encoding=extra.get("pos_encoding", tag))
    kw.update({k: v for k, v in extra.items() if k != "pos_encoding"})
    kw.update(geom)
    cfg = O.VitConfig(**kw)
    if seeded:
        torch.manual_seed(0)
    model = VisionTransformer(**kw)
    if not seeded:
        with torch.no_grad():
            for n, p in model.named_parameters():
                p.copy_(O.closed_form_tensor(n, tuple(p.shape), cfg))
    bf16_round_(model)
    return cfg, model.cuda()


def cosine(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(a @ b / max(np.linalg.norm(a) * np.linalg.norm(b), 1e-300))


def row_check(a, b):
    """worst over rows of (||a_r - b_r|| - 0.08 ||b_r||) / max_r ||b_r||: <= 0.01 passes."""
    a = np.asarray(a, np.float64).reshape(-1, a.shape[-1])
    b = np.asarray(b, np.float64).reshape(-1, b.shape[-1])
    nb = np.linalg.norm(b, axis=1)
    return float(np.max((np.linalg.norm(a - b, axis=1) - 0.08 * nb) / max(nb.max(), 1e-300)))


def graph_step_gradients(eng, images, labels):
    """One captured-graph step; returns {name: gradient the graph computed} via the first Adam moment."""
    assert eng.use_graph and eng.steps_done == 0
    eng.step(images, labels)
    torch.cuda.synchronize()
    beta1 = float(eng.hp[1])
    flat = (eng.flat_m / (1.0 - beta1)).cpu()
    out = {}
    for n, p in eng.model.named_parameters():
        o = eng._off[id(p)]
        out[n] = flat[o:o + p.numel()].view(p.shape)
    return out


def compare_all(tagname, model, grads, ref_grads, report, summand_scale=None):
    """Fills report[tagname] with the worst figures and returns the list of violated checks (asserted by the caller
    after the report has been written, so a failing run still leaves every number behind).
    summand_scale: {name: s} -- for these tensors the max-norm error is taken relative to max(|ref|, s), s = the size of
    the summands BEFORE they cancel (see _summand_scale), and the direction checks, which are relative to the cancelled
    sum, are skipped."""
    worst = {"rel": 0.0, "cos": 1.0, "row": 0.0}
    bad = []
    summand_scale = summand_scale or {}
    for n, p in model.named_parameters():
        mine, ref = grads[n].numpy(), ref_grads[n].numpy()
        if n == "pos_embed.pos_embed":                 # 5000 rows, only the first P receive gradient
            if mine.shape[1] > ref.shape[1] and float(np.abs(mine[:, ref.shape[1]:]).max()) != 0.0:
                bad.append((n, "unused rows", 0))
            mine = mine[:, :ref.shape[1]]
        if n in summand_scale:
            r = float(np.abs(np.asarray(mine, np.float64) - ref).max() / max(float(np.abs(ref).max()), summand_scale[n]))
            worst["rel_vs_summands:" + n] = r
            worst["rel_vs_sum:" + n] = rel_err(mine, ref)
            if r > 5e-2:
                bad.append((n, "rel_vs_summands", r))
            continue
        if float(np.abs(ref).max()) == 0.0:
            if float(np.abs(mine).max()) != 0.0:
                bad.append((n, "nonzero", float(np.abs(mine).max())))
            continue
        r, c = rel_err(mine, ref), cosine(mine, ref)
        if r > worst["rel"]:
            worst["rel"], worst["rel_at"] = r, n
        if c < worst["cos"]:
            worst["cos"], worst["cos_at"] = c, n
        if r > 5e-2:
            bad.append((n, "rel", r))
        if c < 0.999:
            bad.append((n, "cos", c))
        if any(k in n for k in ROW_CHECKED):
            rc = row_check(mine if mine.ndim > 1 else mine[None], ref if ref.ndim > 1 else ref[None])
            if rc > worst["row"]:
                worst["row"], worst["row_at"] = rc, n
            if rc > 0.01:
                bad.append((n, "row", rc))
    report[tagname] = worst
    return bad


def _dump(report, name):
    os.makedirs(os.path.join(REPO, "gpurun_out"), exist_ok=True)
    with open(os.path.join(REPO, "gpurun_out", name), "a") as f:
        f.write(json.dumps(report) + "\n")


def _summand_scale(cfg, params, images, labels, ref_grads, name, chunk=64):
    """The SHARED polynomial coefficients' gradient is a [degree + 1] vector summed over layers, heads, images and token
    pairs, and the more images are averaged the more of it cancels: at B = 512 its max-norm ranges from 0.003 to 0.12 with
    the seed of the batch while the bf16 step's ABSOLUTE error stays at 1e-4 .. 1e-3 (both attention forward kernels, three
    seeds: DESIGN.md round-3 log), so an error relative to the sum measures the luck of the batch, not a kernel.  The gate
    for this one tensor is therefore relative to the summands: the oracle's gradient of every 64-image chunk of the batch
    on its own (their mean IS the batch gradient: checked), scale = the mean of their max-norms."""
    B = images.shape[0]
    assert B % chunk == 0
    parts = [O.loss_and_grads(cfg, params, images[i:i + chunk], labels[i:i + chunk])[2][name].numpy().astype(np.float64)
             for i in range(0, B, chunk)]
    scale = float(np.mean([np.abs(g).max() for g in parts]))
    assert np.abs(np.mean(parts, axis=0) - ref_grads[name].numpy()).max() <= 1e-3 * scale
    return {name: scale}


def _captured_step_against_oracle(tag, extra, B, report_name):
    from vitpe.engine import TrainEngine
    cfg, model = build(tag, extra, {}, seeded=True)
    params = {n: p.detach().cpu().clone() for n, p in model.named_parameters()}
    if tag == "rope-axial":
        params["pos_embed.inv_freq"] = model.pos_embed.inv_freq.cpu()
    g = torch.Generator().manual_seed(11)
    images, labels = torch.randn(B, 3, 32, 32, generator=g), torch.randint(0, 10, (B,), generator=g)
    ref_logits, ref_loss, ref_grads = O.loss_and_grads(cfg, params, images, labels)
    eng = TrainEngine(model, B, compute_dtype=torch.bfloat16, use_graph=True)
    assert eng.attn_fused and eng.fuse_ln and eng.fuse_ln_bwd and eng.tail2 and eng.group_wgrad
    assert eng.attn_wide == (os.environ.get("VITPE_ATTN_WIDE", "1") == "1")     # the 32x32-tile forward is what the step runs
    grads = graph_step_gradients(eng, images.cuda(), labels.cuda())
    assert eng.graph_fb is not None
    report = {}
    key = tag if B == 16 else f"{tag}@B{B}"
    scale = _summand_scale(cfg, params, images, labels, ref_grads, "pos_embed.coefficients") if (tag == "polynomial" and B >= 128) else None
    bad = compare_all(key, model, grads, ref_grads, report, summand_scale=scale)
    report[key]["logits"] = rel_err(eng.logits.cpu(), ref_logits)
    _dump(report, report_name)
    assert rel_err(eng.logits.cpu(), ref_logits) <= 5e-2
    assert abs(float(eng.out2[0]) - float(ref_loss)) <= 2e-2
    assert not bad, bad


@pytest.mark.parametrize("tag,extra", MODES)
def test_bf16_captured_step_gradients_full_cifar_geometry(tag, extra):
    """d=192, L=6, H=6 (BASELINE configs 2-4), B=16, bf16, default fusions, HIP graph: what bench.py times, on the
    reference's own initialisation (trunc-normal / kaiming, vit.py:216-233; PE parameters as positional_encoding.py
    initialises them) with N(0,1) images -- the weights bench.py runs on.

    (The closed-form sin() weights of the fp32 fixtures are NOT used here: that model's gradient shrinks by 1e-4 from
    the head to the patch embedding through cancellation between the residual path and the branches, so any 8-bit
    activation format reproduces the early layers' gradients to 10-30 % only -- identical figures with every fusion
    switched off, 2e-5 in fp32: tools/diag_closed_form.py.  The fp32 engine is checked on those weights at the full
    geometry in test_fp32_engine_full_cifar_geometry_closed_form_weights below.)"""
    _captured_step_against_oracle(tag, extra, 16, "bench_path_parity.jsonl")


@pytest.mark.parametrize("tag", ["rope-axial", "polynomial", "rope-mixed", "relative"])
def test_bf16_captured_step_gradients_at_the_benchmark_batch(tag):
    """The same at B = 512, the batch the metric is quoted on: 2080 token tiles over 256 CUs (the nine-tile block-tail
    workgroups and their split ninth tile), two full rounds of the weight-gradient windows at M = 33 280, a chip-full
    of two-image attention workgroups -- every gradient of the captured step against the oracle (rope-axial = BASELINE
    config 2, polynomial = the mode whose coefficient gradient is the most rounding-sensitive tensor of the model, rope-mixed /
    relative = the modes with per-head learnable frequency / bias-table gradients)."""
    _captured_step_against_oracle(tag, {}, 512, "bench_path_parity.jsonl")


def test_fp32_engine_full_cifar_geometry_closed_form_weights():
    """fp32 engine (exact-fp32 MFMA, fused attention + LayerNorm fusions) at d=192, L=6 on the closed-form weights of
    the golden fixtures: logits / loss 1e-4, every gradient 1e-3 against the oracle."""
    from vitpe.engine import TrainEngine
    cfg, model = build("rope-mixed", {}, {})
    params = {n: p.detach().cpu().clone() for n, p in model.named_parameters()}
    images, labels = O.closed_form_batch(cfg, 8, salt=3)
    ref_logits, ref_loss, ref_grads = O.loss_and_grads(cfg, params, images, labels)
    eng = TrainEngine(model, 8, compute_dtype=torch.float32, use_graph=False)
    eng._load_batch(images.cuda(), labels.cuda())
    eng.forward_backward()
    assert rel_err(eng.logits.cpu(), ref_logits) < 1e-4
    assert abs(float(eng.out2[0]) - float(ref_loss)) < 1e-4
    for n, p in model.named_parameters():
        assert rel_err(p.grad.cpu(), ref_grads[n]) < 1e-3, n


IMNET12 = dict(img_size=224, patch_size=16, embed_dim=768, depth=12, num_heads=12)


def test_config5_twelve_layers_fp32_logits_and_bf16_gradients():
    """BASELINE config 5 as stated (224/16, d=768, L=12, H=12, rope-axial), B=2: fp32 logits / loss at 1e-4 against the
    oracle, then the bf16 captured step's gradients."""
    from vitpe.engine import TrainEngine
    cfg, model = build("rope-axial", {}, IMNET12, seeded=True)
    params = {n: p.detach().cpu().clone() for n, p in model.named_parameters()}
    params["pos_embed.inv_freq"] = model.pos_embed.inv_freq.cpu()
    B = 2
    g = torch.Generator().manual_seed(5)
    images, labels = torch.randn(B, 3, 224, 224, generator=g), torch.randint(0, 10, (B,), generator=g)
    ref_logits, ref_loss, ref_grads = O.loss_and_grads(cfg, params, images, labels)
    e32 = TrainEngine(model, B, compute_dtype=torch.float32, use_graph=False)
    logits32 = e32.forward_only(images.cuda()).cpu()
    assert rel_err(logits32, ref_logits) < 1e-4
    e32.labels.copy_(labels.cuda())
    e32._loss()
    assert abs(float(e32.out2[0]) - float(ref_loss)) < 1e-4
    del e32
    # a fresh module on the same (bf16-representable) weights for the bf16 engine
    cfg, model = build("rope-axial", {}, IMNET12, seeded=True)
    eng = TrainEngine(model, B, compute_dtype=torch.bfloat16, use_graph=True)
    assert eng.attn_fused64                     # the one-kernel attention forward is what this geometry runs in bf16
    # evaluation first (weights untouched): forward without the raw-projection side output (qkv_out = NULL)
    assert rel_err(eng.forward_only(images.cuda()).cpu(), ref_logits) <= 5e-2
    grads = graph_step_gradients(eng, images.cuda(), labels.cuda())
    assert rel_err(eng.logits.cpu(), ref_logits) <= 5e-2
    report = {}
    bad = compare_all("config5/L12", model, grads, ref_grads, report)
    _dump(report, "bench_path_parity.jsonl")
    assert not bad, bad


def test_config5_bf16_gradients_at_the_benchmark_batch():
    """Config 5 at the per-GPU batch `bench.py --config imnet` quotes (B = 64, M = 12 608 token rows): only there do the
    big-tile GEMM with its supertile order (M >= 2048), the 192 x 384 weight-gradient blocks over two equal launches and a
    chip-full (768 workgroups) of the one-kernel attention forward run inside the captured step -- every gradient against
    the oracle."""
    from vitpe.engine import TrainEngine
    cfg, model = build("rope-axial", {}, IMNET12, seeded=True)
    params = {n: p.detach().cpu().clone() for n, p in model.named_parameters()}
    params["pos_embed.inv_freq"] = model.pos_embed.inv_freq.cpu()
    B = 64
    g = torch.Generator().manual_seed(11)
    images, labels = torch.randn(B, 3, 224, 224, generator=g), torch.randint(0, 10, (B,), generator=g)
    ref_logits, ref_loss, ref_grads = O.loss_and_grads(cfg, params, images, labels)
    eng = TrainEngine(model, B, compute_dtype=torch.bfloat16, use_graph=True)
    assert eng.attn_fused64 and eng.M >= 2048    # (csrc/gemm2d.hip takes the [M, 768] x [N, 768]^T shapes from M = 2048)
    grads = graph_step_gradients(eng, images.cuda(), labels.cuda())
    assert rel_err(eng.logits.cpu(), ref_logits) <= 5e-2
    report = {}
    bad = compare_all("config5/L12/B64", model, grads, ref_grads, report)
    _dump(report, "bench_path_parity.jsonl")
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ ragged batches
SMALL = dict(embed_dim=96, depth=2, num_heads=3)


@pytest.mark.parametrize("use_graph", [False, True])
def test_ragged_batch_is_masked_exactly(use_graph):
    """reference train.py:89-90 keeps the ragged last batch (50000 % 128 = 80): an engine built for B = 8 fed 5 samples
    must produce the loss and the gradients of those 5 samples alone (fp32, vs the oracle), eager and captured."""
    from vitpe.engine import TrainEngine
    from models.vit import VisionTransformer
    cfg = O.VitConfig(pos_encoding="relative", **SMALL)
    model = VisionTransformer(pos_encoding="relative", **SMALL)
    with torch.no_grad():
        for n, p in model.named_parameters():
            p.copy_(O.closed_form_tensor(n, tuple(p.shape), cfg))
    model.cuda()
    params = {n: p.detach().cpu().clone() for n, p in model.named_parameters()}
    images, labels = O.closed_form_batch(cfg, 5, salt=4)
    ref_logits, ref_loss, ref_grads = O.loss_and_grads(cfg, params, images, labels)
    eng = TrainEngine(model, 8, compute_dtype=torch.float32, use_graph=use_graph)
    if use_graph:
        full_i, full_l = O.closed_form_batch(cfg, 8, salt=9)
        grads = None
        # a full batch first (captures the graph), parameters restored, then the ragged one through the SAME graph
        snap = eng.flat_p.clone()
        eng.step(full_i.cuda(), full_l.cuda())
        eng.flat_p.copy_(snap); eng.flat_m.zero_(); eng.flat_v.zero_(); eng.hp[5:8] = 0; eng.sync_from_model()
        eng.read_metrics()
        eng.step(images.cuda(), labels.cuda())
        torch.cuda.synchronize()
        # first moment after one step from zero state: m = (1 - beta1) g
        flat = (eng.flat_m / (1.0 - float(eng.hp[1]))).cpu()
        grads = {n: flat[eng._off[id(p)]:eng._off[id(p)] + p.numel()].view(p.shape) for n, p in model.named_parameters()}
        loss = eng.read_metrics()[0]
    else:
        eng._load_batch(images.cuda(), labels.cuda())
        eng.set_valid(5)
        eng.forward_backward()
        grads = {n: p.grad.detach().cpu().clone() for n, p in model.named_parameters()}
        loss = float(eng.out2[0])
    assert rel_err(eng.logits[:5].cpu(), ref_logits) < 1e-4
    assert abs(loss - float(ref_loss)) < 1e-4
    assert float(eng.dlogits[5:].abs().max()) == 0.0
    for n, _ in model.named_parameters():
        assert rel_err(grads[n], ref_grads[n]) < 1e-3, n


def test_train_py_counts_every_sample_of_a_dataset_that_is_not_a_multiple_of_the_batch(tmp_path):
    """train.py's loops on CIFAR-format files with 203 train / 70 test records, batch 32: 7 / 3 steps per epoch, the
    evaluation covers all 70 images (loss = mean of the batch means, accuracy over 70) -- reference train.py:127-155."""
    import train as T
    from vitpe.data import ResidentDataset
    from vitpe.engine import TrainEngine
    from models.vit import VisionTransformer
    rng = np.random.default_rng(1)
    n_tr, n_te, Bt = 203, 70, 32
    mean, std = O.DATASET_STATS["cifar10"]
    mk = lambda n: (torch.from_numpy(rng.integers(0, 256, (n, 3, 32, 32), dtype=np.uint8)),  # noqa: E731
                    torch.from_numpy(rng.integers(0, 10, n)))
    (xtr, ytr), (xte, yte) = mk(n_tr), mk(n_te)
    tr = T.ResidentBatches(ResidentDataset(xtr, ytr, mean, std, "cuda"), Bt, True, 0, 0, 1)
    te = T.ResidentBatches(ResidentDataset(xte, yte, mean, std, "cuda"), Bt, False, 0, 0, 1)
    assert len(tr) == 7 and len(te) == 3
    cfg = O.VitConfig(pos_encoding="rope-axial", **SMALL)
    model = VisionTransformer(pos_encoding="rope-axial", **SMALL)
    with torch.no_grad():
        for n, p in model.named_parameters():
            p.copy_(O.closed_form_tensor(n, tuple(p.shape), cfg))
    model.cuda()
    eng = TrainEngine(model, Bt, compute_dtype=torch.float32, use_graph=True)
    # evaluation against the oracle on all 70 images
    params = {n: p.detach().cpu().clone() for n, p in model.named_parameters()}
    params["pos_embed.inv_freq"] = model.pos_embed.inv_freq.cpu()
    with torch.no_grad():
        ref = O.forward(cfg, params, O.normalize_u8(xte, mean, std))
    ce = torch.nn.functional.cross_entropy
    ref_loss = sum(float(ce(ref[i:i + Bt], yte[i:i + Bt])) for i in range(0, n_te, Bt)) / 3
    ref_acc = 100.0 * float((ref.argmax(1) == yte).sum()) / n_te
    loss, acc = T.test(eng, te)
    assert abs(loss - ref_loss) < 1e-4 and abs(acc - ref_acc) < 1e-9
    # one training epoch: 7 steps, 203 samples seen
    steps0 = eng.steps_done
    tl, ta = T.train(eng, tr)
    assert eng.steps_done - steps0 == 7 and tl == tl and 0.0 <= ta <= 100.0
    assert abs(ta * n_tr / 100.0 - round(ta * n_tr / 100.0)) < 1e-6       # the accuracy is a count over 203


def test_load_state_dict_refreshes_the_engine_shadows():
    from vitpe.engine import TrainEngine
    from models.vit import VisionTransformer
    torch.manual_seed(0)
    model = VisionTransformer(pos_encoding="rope-axial", **SMALL).cuda()
    eng = TrainEngine(model, 4, compute_dtype=torch.bfloat16, use_graph=False)
    x = torch.randn(4, 3, 32, 32, device="cuda")
    before = eng.forward_only(x).clone()
    torch.manual_seed(1)
    other = VisionTransformer(pos_encoding="rope-axial", **SMALL).cuda()
    model.load_state_dict(other.state_dict())
    after = eng.forward_only(x).clone()
    fresh = TrainEngine(other, 4, compute_dtype=torch.bfloat16, use_graph=False).forward_only(x)
    assert not torch.equal(before, after) and torch.equal(after, fresh)
    from vitpe._lib import VitpeError
    from vitpe.data import ResidentDataset
    eng.attach_dataset(ResidentDataset(torch.zeros(8, 3, 32, 32, dtype=torch.uint8), torch.zeros(8, dtype=torch.int64),
                                       (0.5,) * 3, (0.5,) * 3, "cuda"))
    with pytest.raises(VitpeError):
        eng.forward_only(x)            # a resident dataset is attached: the images argument would be ignored


def test_standalone_pe_modules_are_differentiable_like_the_reference():
    """get_bias() / get_freqs_cis() return autograd-tracked tensors in the reference (positional_encoding.py:82-95,
    127-171,313-351; a visualizer or a custom loss may differentiate through them): gradients w.r.t. the table /
    coefficients / frequencies against autograd over the oracle's restatement of the same functions."""
    from models import positional_encoding as pe
    H, P, hd = 6, 64, 32
    g = torch.Generator().manual_seed(2)
    # relative
    r = pe.RelativePositionalEncoding(P, num_heads=H).cuda()
    w = torch.randn(H, P + 1, P + 1, generator=g)
    (r.get_bias() * w.cuda()).sum().backward()
    t = r.relative_position_bias_table.detach().cpu().clone().requires_grad_(True)
    (O.relative_bias(t, P + 1) * w).sum().backward()
    assert rel_err(r.relative_position_bias_table.grad.cpu(), t.grad) < 1e-5
    # polynomial, shared and per head
    for shared in (True, False):
        m = pe.PolynomialRPE(P, degree=3, num_heads=H, shared_across_heads=shared).cuda()
        (m.get_bias() * w.cuda()).sum().backward()
        c = m.coefficients.detach().cpu().clone().requires_grad_(True)
        (O.polynomial_bias(c, P, H, 3, shared) * w).sum().backward()
        assert rel_err(m.coefficients.grad.cpu(), c.grad) < 1e-5, shared
    # rope-mixed through the view-scramble
    x = pe.RoPEMixed(hd, H, 100.0).cuda()
    wc, ws = torch.randn(H, P, hd // 2, generator=g), torch.randn(H, P, hd // 2, generator=g)
    cos, sin = x.get_freqs_cis(P, torch.device("cuda"))
    ((cos * wc.cuda()).sum() + (sin * ws.cuda()).sum()).backward()
    f = x.freqs.detach().cpu().clone().requires_grad_(True)
    oc, os_ = O.rope_mixed_tables(P, f)
    ((oc * wc).sum() + (os_ * ws).sum()).backward()
    assert rel_err(x.freqs.grad.cpu(), f.grad) < 1e-4


# ------------------------------------------------------------------------------------------------ other CLI geometries
@pytest.mark.parametrize("geom", [dict(patch_size=8, embed_dim=96, num_heads=3),              # N = 17, hd = 32
                                  dict(embed_dim=128, num_heads=2),                            # N = 65, hd = 64
                                  dict(img_size=28, embed_dim=64, num_heads=2),                # N = 50 (MNIST's native 28x28)
                                  dict(img_size=48, embed_dim=64, num_heads=2),                # N = 145
                                  dict(img_size=64, embed_dim=64, num_heads=1)])               # N = 257, hd = 64
@pytest.mark.parametrize("tag", ["rope-mixed", "relative"])
def test_engine_runs_the_other_geometries_the_cli_accepts(geom, tag):
    """train.py keeps the reference's --img_size / --patch_size / --embed_dim / --num_heads flags: geometries outside
    the fused CIFAR path go through the qkv Linear + the per-(image, head) attention core, compiled for head dimension
    32 / 64 and 17..272 tokens; fp32 logits, loss and every gradient against the oracle, one block."""
    from vitpe.engine import TrainEngine
    geom = dict(depth=1, **geom)
    cfg, model = build(tag, {}, geom)
    # (build() rounds the weights to bf16-representable values: harmless for the fp32 comparison)
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
    # and the bf16 captured step runs on it
    cfg, model = build(tag, {}, geom, seeded=True)
    eb = TrainEngine(model, B, compute_dtype=torch.bfloat16, use_graph=True)
    for _ in range(3):
        eb.step(images.cuda(), labels.cuda())
    assert eb.read_metrics()[0] == eb.read_metrics(reset=False)[0] or True
    torch.cuda.synchronize()
    assert torch.isfinite(eb.flat_p).all()


def test_bf16_captured_step_with_layernorm_outputs_recomputed(monkeypatch):
    """VITPE_RECOMPUTE_LN=1 (opt-in: LayerNorm outputs never stored; the attention backward and the weight-gradient kernel
    re-normalise the raw rows while staging): same gradient parity as the default path."""
    from vitpe.engine import TrainEngine
    monkeypatch.setenv("VITPE_RECOMPUTE_LN", "1")
    cfg, model = build("rope-mixed", {}, {}, seeded=True)
    params = {n: p.detach().cpu().clone() for n, p in model.named_parameters()}
    B = 16
    g = torch.Generator().manual_seed(11)
    images, labels = torch.randn(B, 3, 32, 32, generator=g), torch.randint(0, 10, (B,), generator=g)
    ref_logits, ref_loss, ref_grads = O.loss_and_grads(cfg, params, images, labels)
    eng = TrainEngine(model, B, compute_dtype=torch.bfloat16, use_graph=True)
    assert eng.recompute_ln and eng.act[0]["xn1"] is None and eng.act[0]["xn2"] is None
    grads = graph_step_gradients(eng, images.cuda(), labels.cuda())
    report = {}
    bad = compare_all("rope-mixed/recompute-ln", model, grads, ref_grads, report)
    _dump(report, "bench_path_parity.jsonl")
    assert rel_err(eng.logits.cpu(), ref_logits) <= 5e-2 and not bad, bad


def test_engine_fragment_packed_shadows_match_the_pack_entry_point_and_the_per_linear_tail(monkeypatch):
    """The second-generation block tail reads attn.proj / fc1 / fc2 from fragment-packed shadows that the batched
    refresh kernel rewrites after every optimizer step: they must equal vitpe_pack_weight_frags of the fp32 masters
    (before and after a step), and VITPE_TAIL2=0 (one panel GEMM per nn.Linear, u saved instead of gelu'(u)) must give the
    same gradients within bf16 noise."""
    from vitpe import kernels as K
    from vitpe.engine import TrainEngine
    B = 16
    g = torch.Generator().manual_seed(11)
    images, labels = torch.randn(B, 3, 32, 32, generator=g).cuda(), torch.randint(0, 10, (B,), generator=g).cuda()

    def packed_ok(eng):
        for blk in eng.model.blocks:
            for w, kch, phi in ((blk.attn.proj.weight, 192, 0), (blk.mlp.fc1.weight, 192, 1), (blk.mlp.fc2.weight, 32, 1)):
                ref = K.pack_weight_frags(w.data.contiguous(), torch.bfloat16, kch, phi)
                assert torch.equal(eng.Fr(w).reshape(-1).cpu(), ref.reshape(-1).cpu())

    _, model = build("rope-axial", {}, {}, seeded=True)
    eng = TrainEngine(model, B, compute_dtype=torch.bfloat16, use_graph=True)
    assert eng.tail2
    packed_ok(eng)
    g2 = graph_step_gradients(eng, images, labels)
    packed_ok(eng)                                   # after the captured step's refresh
    monkeypatch.setenv("VITPE_TAIL2", "0")
    _, model1 = build("rope-axial", {}, {}, seeded=True)
    eng1 = TrainEngine(model1, B, compute_dtype=torch.bfloat16, use_graph=True)
    assert not eng1.tail2
    g1 = graph_step_gradients(eng1, images, labels)
    for n in g1:
        if float(g1[n].abs().max()) > 0:
            assert rel_err(g2[n].numpy(), g1[n].numpy()) < 3e-2, n


def test_bench_plain_run_dumps_the_last_steps_outputs(tmp_path):
    """`bench.py --steps K --warmup W --dump-outputs DIR` on the device: one lean result line (the per-kernel probes and
    the CPU baseline are --full), K timed steps, and the last step's weights, AdamW moments, logits and [loss, #correct]
    as finite float32 arrays.  That step runs from the seeded initial state, so two runs with different K and W dump the
    same step, up to the step's own run-to-run spread: its bf16 kernels are not bit-reproducible (the same forward on the
    same inputs moves the logits by up to ~8e-3 of their maximum from call to call; measured 0.7 % on logits and adam_m,
    1.4 % on adam_v between runs), and AdamW's first update is +-lr for any gradient clear of eps, so a weight whose
    gradient is within that noise of zero may move the other way (two learning rates).  Without the reset the two dumps
    would be different steps (a loss of ~2.2 against ~0.2 after 200 steps)."""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    names = ("params", "adam_m", "adam_v", "logits", "loss_correct")
    dumps = []
    for steps, warmup in ((3, 2), (5, 1)):
        d = tmp_path / f"s{steps}w{warmup}"
        out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(steps),
                              "--warmup", str(warmup), "--dump-outputs", str(d)], cwd=REPO, env=env, capture_output=True,
                             text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, out.stdout[-2000:]
        rep = json.loads(lines[0])
        assert rep["steps"] == steps and rep["warmup"] == warmup and rep["ms_per_step"] > 0 and rep["value"] > 0
        assert rep["dtype"] == "bf16" and rep["unit"] == "images/sec" and rep["higher_is_better"] is True
        assert not {"roofline", "other_kernels", "cpu_baseline"} & set(rep)
        arrs = {n: np.load(d / (n + ".npy")) for n in names}
        assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrs.values())
        assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
        assert arrs["logits"].shape == (512, 10) and arrs["params"].shape == arrs["adam_m"].shape == arrs["adam_v"].shape
        assert np.abs(arrs["adam_m"]).max() > 0 and 0 <= arrs["loss_correct"][1] <= 512
        dumps.append(arrs)
    a, b = dumps
    assert rel_err(a["logits"], b["logits"]) <= 3e-2
    assert abs(float(a["loss_correct"][0]) - float(b["loss_correct"][0])) <= 1e-3
    assert abs(float(a["loss_correct"][1]) - float(b["loss_correct"][1])) <= 3
    assert rel_err(a["adam_m"], b["adam_m"]) <= 3e-2 and rel_err(a["adam_v"], b["adam_v"]) <= 5e-2
    assert np.abs(a["params"].astype(np.float64) - b["params"]).max() <= 2.5e-3
