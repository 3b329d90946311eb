"""csrc/embed.hip through the C ABI against tests/embed_ref.py (case lists, gates and their derivation: that module's
docstring; their coverage of the kernel's paths and their power against a wrong index: test_embed_cpu.py).

  vitpe_patch_embed[_aug]   every (gather branch, source, K-step count, K padding, P % 16, live waves, D / 16) the support
                            predicate admits: the exact integer case (tokens and patch matrix bit-equal in both dtypes),
                            real-valued inputs from fp32 images, the uint8 dataset and the uint8 dataset with the
                            augmentation stream (patch matrix and class row bit-equal, patch rows within the forward
                            bound per element, statistics of the stored rows to 1e-4), every output NaN-filled before the
                            launch and followed by a 64-element NaN guard; index NULL, repeated indices, patches / stats
                            NULL, three launches; the refusals
  vitpe_unfold, _u8, _u8_aug  p = 2, 7, 8, 16, 24 in both dtypes, and the three smallest launches that exceed the grid cap
                            (a thread walks several images, the augmented form redraws when the image changes), bit-exact
  TrainEngine               the MNIST geometries of the generic gather branch (C = 1, p = 8) and the fp32-only CIFAR one
                            (p = 2): fp32 against the oracle, fused against unfused, bf16 captured steps, and the patch
                            matrix a captured augmented step leaves

Measured, MI355X (profiles/embed_parity.jsonl holds every figure; DESIGN.md, "What the patch-embed tests pin"): worst
|d| / bound of the patch rows 0.20 in fp32 (K = 4; 0.04 at K >= 36: the fp32 MFMA chain meets the plain fp32 bound) and
0.995 in bf16, all of it the half-ulp term (no element outside its rounding interval); statistics 3.3e-8 / 5.4e-7 (gate
1e-4); everything gated exactly is exact.  No figure needed a wider gate.
"""
import numpy as np
import pytest
import torch

import augment_ref as A
import embed_ref as E
import ln_ref as LN
from conftest import rel_err
from oracle import vit_oracle as O
from parity_report import Report
from test_head_dims_gpu import guarded

pytestmark = pytest.mark.gpu
DT = E.DT
NOT_SUPPORTED = 801          # hipErrorNotSupported

CASES_DT = [(C, S, p, D, dt) for C, S, p, D, dts in E.FUSED_CASES for dt in dts]
AUG_DT = [(C, S, p, D, pad, dt) for C, S, p, D, pad, dts in E.AUG_CASES for dt in dts]
UNFOLD_DT = [(C, S, p, dt) for C, S, p in E.UNFOLD_CASES for dt in E.BOTH]


def ids(cases):
    return ["-".join(str(v) for v in c) for c in cases]


@pytest.fixture(scope="module")
def K():
    from vitpe import kernels
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return kernels


@pytest.fixture(scope="module")
def report():
    r = Report("test_embed_gpu", "embed_parity.jsonl")
    yield r
    r.close()


def signed(v):
    return v - (1 << 64) if v >= (1 << 63) else v


def pair(seed=E.SEED, offset=E.OFFSET):
    return torch.tensor([signed(seed), signed(offset)], dtype=torch.int64, device="cuda")


def words(rng):
    return tuple(int(v) & 0xFFFFFFFFFFFFFFFF for v in rng.reshape(-1).tolist())


def bits(t):
    """the bit patterns of a float32 / bfloat16 tensor (host)"""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def nbits(got, want):
    """number of elements of `got` whose bits differ from `want` (cast to got's type first: want holds representable values)"""
    return int((bits(got) != bits(want.to(got.dtype))).sum())


def u8_source(C, S, index=E.INDEX, pad=None, data=None):
    """keyword arguments of K.patch_embed / positional ones of K.unfold_u8 for the uint8 dataset of the geometry"""
    x = E.dataset(C, S) if data is None else data
    src = dict(data=torch.tensor(x).cuda(), index=None if index is None else torch.tensor(index, device="cuda"),
               mean=torch.tensor(E.STATS[C][0], device="cuda"), std=torch.tensor(E.STATS[C][1], device="cuda"))
    if pad is not None:
        src.update(rng=pair(), crop_pad=pad, hflip=True)
    return src


def run_embed(K, dt, C, S, p, w, bias, cls, ape, src, B, patches=True, stats=True):
    """One launch into NaN-filled, NaN-guarded outputs -> host copies, the NaNs left inside and the guard elements lost."""
    _, P, Kk = E.geometry(C, S, p)
    T, D = DT[dt], w.shape[0]
    bufs = {"tok": guarded((B, P + 1, D), T)}
    if patches:
        bufs["pat"] = guarded((B * P, Kk), T)
    if stats:
        bufs["mean"], bufs["rstd"] = guarded((B * (P + 1),), torch.float32), guarded((B * (P + 1),), torch.float32)
    v = {k: b[1] for k, b in bufs.items()}
    K.patch_embed(w.cuda().to(T), bias.cuda(), cls.cuda(), None if ape is None else ape.cuda(), p, T, out=v["tok"],
                  patches_out=v.get("pat"), stats=(v["mean"], v["rstd"]) if stats else None, eps=E.EPS, **src)
    torch.cuda.synchronize()
    out = {k: t.cpu() for k, t in v.items()}
    out["nan_inside"] = sum(int(torch.isnan(t.float()).sum()) for t in out.values())
    out["guard_lost"] = sum(int((~torch.isnan(buf[view.numel():].float())).sum()) for buf, view in bufs.values())
    return out


def check_rows(r, tag, dt, got, x, w, bias, cls, ape, stats=True):
    """the figures of one launch against the float64 reference of patch matrix x [B, P, K]"""
    B, P, Kk = x.shape
    ref = E.tokens_ref(dt, x, w, bias, cls, ape)
    terms = E.abs_terms(dt, x, w, bias, ape)
    bound = E.token_bound(dt, ref[:, 1:], terms, Kk)
    tok = got["tok"].float()
    r.eq(tag + "nan_inside", got["nan_inside"], 0)
    r.eq(tag + "guard_lost", got["guard_lost"], 0)
    if "pat" in got:
        r.eq(tag + "patches_bits", nbits(got["pat"], x.reshape(B * P, Kk)), 0)
    r.eq(tag + "class_row_bits", nbits(got["tok"][:, 0], cls.expand(B, -1)), 0)
    r.le(f"{tag}patch_rows_excess_{dt}", E.excess(tok[:, 1:], ref[:, 1:], bound), 1.0)
    if dt == "bf16":
        r.eq(tag + "outside_rounding_interval",
             E.outside_rounding_interval(tok[:, 1:], ref[:, 1:], E.token_bound("f32", ref[:, 1:], terms, Kk)), 0)
    if stats:
        mean, rstd = got["mean"].reshape(B, P + 1), got["rstd"].reshape(B, P + 1)
        for name, sl in (("class", slice(0, 1)), ("patch", slice(1, None))):
            em, er = LN.stat_errors(mean[:, sl], rstd[:, sl], tok[:, sl], E.EPS)
            r.le(f"{tag}{name}_mean", em, LN.STAT_TOL)
            r.le(f"{tag}{name}_rstd", er, LN.STAT_TOL)


# ---- 1. the exact case -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES_DT, ids=ids(CASES_DT))
def test_integer_inputs_give_bit_equal_tokens(K, report, c):
    """Small integers: no rounding anywhere, so tokens and patch matrix equal the reference bit for bit in both dtypes; the
    weights have no two equal rows or columns (test_embed_cpu.py), so a wrong operand index cannot cancel."""
    C, S, p, D, dt = c
    assert K.patch_embed_supported(DT[dt], C, S, p, D)
    _, P, Kk = E.geometry(C, S, p)
    img, w, bias, cls, ape = E.int_inputs(C, S, p, D)
    x = E.unfold_img(img, p)
    r = report.case("integer", "-".join(str(v) for v in c))
    for tag, a in (("ape_", ape), ("noape_", None)):
        got = run_embed(K, dt, C, S, p, w, bias, cls, a, dict(images=img.cuda()), img.shape[0])
        ref = E.tokens_ref(dt, x.reshape(-1, P, Kk), w, bias, cls, a)
        r.eq(tag + "tokens_bits", nbits(got["tok"], ref.float()), 0)
        r.eq(tag + "patches_bits", nbits(got["pat"], x), 0)
        r.eq(tag + "nan_inside", got["nan_inside"], 0)
        r.eq(tag + "guard_lost", got["guard_lost"], 0)
        tok = got["tok"].float()
        em, er = LN.stat_errors(got["mean"].reshape(-1, P + 1), got["rstd"].reshape(-1, P + 1), tok, E.EPS)
        r.le(tag + "mean", em, LN.STAT_TOL)
        r.le(tag + "rstd", er, LN.STAT_TOL)
    r.done()


# ---- 2. real values, the three sources -------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES_DT, ids=ids(CASES_DT))
def test_real_inputs_from_the_three_sources(K, report, c):
    C, S, p, D, dt = c
    assert K.patch_embed_supported(DT[dt], C, S, p, D)
    _, P, Kk = E.geometry(C, S, p)
    img, w, bias, cls, ape = E.real_inputs(dt, C, S, p, D)
    sources = (("img_", dict(images=img.cuda()), E.unfold_img(img, p)),
               ("u8_", u8_source(C, S), E.u8_patches(C, S, p)),
               ("u8aug_", u8_source(C, S, pad=E.DEFAULT_PAD), E.u8_patches(C, S, p, pad=E.DEFAULT_PAD)))
    r = report.case("real", "-".join(str(v) for v in c))
    for tag, src, x in sources:
        x = x.reshape(-1, P, Kk)
        for a in (ape, None):
            got = run_embed(K, dt, C, S, p, w, bias, cls, a, src, x.shape[0])
            check_rows(r, tag, dt, got, x, w, bias, cls, a)
    r.done()


# ---- 3. behaviour ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", E.BOTH)
@pytest.mark.parametrize("C,S,p,D", [(1, 32, 8, 64), (1, 56, 8, 128), (3, 32, 4, 192)])
def test_null_arguments_repeated_indices_and_repeated_launches(K, report, C, S, p, D, dt):
    _, P, Kk = E.geometry(C, S, p)
    _, w, bias, cls, ape = E.real_inputs(dt, C, S, p, D)
    r = report.case("behaviour", f"{C}-{S}-{p}-{D}-{dt}")
    keys = ("tok", "pat", "mean", "rstd")

    def same(tag, a, b, which=keys):
        for k in which:
            r.eq(f"{tag}_{k}_bits", int((bits(a[k]) != bits(b[k])).sum()), 0)

    # index == NULL is index == arange
    listed = run_embed(K, dt, C, S, p, w, bias, cls, ape, u8_source(C, S, index=list(range(E.NREC))), E.NREC)
    null = run_embed(K, dt, C, S, p, w, bias, cls, ape, u8_source(C, S, index=None), E.NREC)
    same("index_null", null, listed)
    x = E.u8_patches(C, S, p, index=None).reshape(-1, P, Kk)
    check_rows(r, "index_null_", dt, null, x, w, bias, cls, ape)
    # the same record in two slots (INDEX[0] == INDEX[2]): equal rows without the stream, two draws with it
    B = len(E.INDEX)
    plain = run_embed(K, dt, C, S, p, w, bias, cls, ape, u8_source(C, S), B)
    r.eq("repeat_tok_bits", int((bits(plain["tok"][0]) != bits(plain["tok"][2])).sum()), 0)
    r.eq("repeat_pat_bits", int((bits(plain["pat"][:P]) != bits(plain["pat"][2 * P:3 * P])).sum()), 0)
    drawn = run_embed(K, dt, C, S, p, w, bias, cls, ape, u8_source(C, S, pad=E.DEFAULT_PAD), B)
    assert not torch.equal(drawn["pat"][:P], drawn["pat"][2 * P:3 * P]) and not torch.equal(drawn["tok"][0], drawn["tok"][2])
    # patches == NULL, stats == NULL: the tokens do not change
    for tag, kw in (("no_patches", dict(patches=False)), ("no_stats", dict(stats=False)), ("neither", dict(patches=False, stats=False))):
        got = run_embed(K, dt, C, S, p, w, bias, cls, ape, u8_source(C, S, pad=E.DEFAULT_PAD), B, **kw)
        same(tag, got, drawn, which=[k for k in keys if k in got])
        r.eq(tag + "_nan_inside", got["nan_inside"], 0)
        r.eq(tag + "_guard_lost", got["guard_lost"], 0)
    # three launches
    for rep in range(2):
        same(f"launch{rep + 2}", run_embed(K, dt, C, S, p, w, bias, cls, ape, u8_source(C, S, pad=E.DEFAULT_PAD), B), drawn)
    r.done()


@pytest.mark.parametrize("dt", E.BOTH)
def test_null_patches_and_stats_from_fp32_images(K, report, dt):
    """the NULL patches / NULL stats combination on the fp32-image path, both gather branches"""
    r = report.case("null_outputs_img", dt)
    for C, S, p, D in ((1, 32, 8, 64), (3, 32, 4, 256)):
        _, P, Kk = E.geometry(C, S, p)
        img, w, bias, cls, ape = E.real_inputs(dt, C, S, p, D)
        full = run_embed(K, dt, C, S, p, w, bias, cls, ape, dict(images=img.cuda()), img.shape[0])
        bare = run_embed(K, dt, C, S, p, w, bias, cls, ape, dict(images=img.cuda()), img.shape[0], patches=False, stats=False)
        r.eq(f"p{p}_tok_bits", int((bits(full["tok"]) != bits(bare["tok"])).sum()), 0)
        check_rows(r, f"p{p}_", dt, bare, E.unfold_img(img, p).reshape(-1, P, Kk), w, bias, cls, ape, stats=False)
    r.done()


# ---- 4. the augmentation stream on the generic branch ----------------------------------------------------------------------
@pytest.mark.parametrize("c", AUG_DT, ids=ids(AUG_DT))
def test_fused_embed_with_rng_on_every_gather_form(K, report, c):
    """The patch matrix is augment_ref's bit for bit; the tokens are those of the same kernel run on the augmented fp32
    images (data.augment_batch), bit for bit, and within the bound of the float64 reference."""
    from vitpe.data import ResidentDataset, augment_batch
    C, S, p, D, pad, dt = c
    assert K.patch_embed_supported(DT[dt], C, S, p, D)
    _, P, Kk = E.geometry(C, S, p)
    _, w, bias, cls, ape = E.real_inputs(dt, C, S, p, D)
    B = len(E.INDEX)
    x = E.u8_patches(C, S, p, pad=pad).reshape(B, P, Kk)
    r = report.case("aug", "-".join(str(v) for v in c))
    got = run_embed(K, dt, C, S, p, w, bias, cls, ape, u8_source(C, S, pad=pad), B)
    check_rows(r, "", dt, got, x, w, bias, cls, ape)
    data = torch.tensor(E.dataset(C, S))
    ds = ResidentDataset(data, torch.arange(data.shape[0]), *E.STATS[C], "cuda")
    images = augment_batch(ds, torch.tensor(E.INDEX, device="cuda"), pair(), crop_pad=pad, hflip=True)
    r.eq("augment_batch_bits", nbits(images, E.u8_images(C, S, pad=pad)), 0)
    again = run_embed(K, dt, C, S, p, w, bias, cls, ape, dict(images=images), B)
    for k in ("tok", "pat", "mean", "rstd"):
        r.eq(f"from_images_{k}_bits", int((bits(again[k]) != bits(got[k])).sum()), 0)
    r.done()


# ---- 5. the refusals -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", E.REFUSED, ids=ids(E.REFUSED))
def test_refused_geometries_return_not_supported_and_write_nothing(K, c):
    from vitpe import _lib as L
    dt, C, S, p, D, _ = c
    T = DT[dt]
    assert not K.patch_embed_supported(T, C, S, p, D)
    B, G = 2, S // p
    P, Kk = G * G, C * p * p
    lib, sp = L.lib(), L.stream_ptr()
    w = torch.zeros(D, Kk, device="cuda", dtype=T)
    bias, cls = torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")
    img = torch.zeros(B, C, S, S, device="cuda")
    src = u8_source(C, S, index=[1, 0])
    rng = pair()
    outs = [torch.full((n,), float("nan"), device="cuda", dtype=t)
            for n, t in ((B * (P + 1) * D, T), (B * P * Kk, T), (B * (P + 1), torch.float32), (B * (P + 1), torch.float32))]
    tail = [w.data_ptr(), bias.data_ptr(), cls.data_ptr(), None] + [o.data_ptr() for o in outs] + [B, C, S, p, D, E.EPS]
    u8 = [None, src["data"].data_ptr(), src["index"].data_ptr(), src["mean"].data_ptr(), src["std"].data_ptr()]
    assert lib.vitpe_patch_embed(L.dtype_code(T), img.data_ptr(), None, None, None, None, *tail, sp) == NOT_SUPPORTED
    assert lib.vitpe_patch_embed(L.dtype_code(T), *u8, *tail, sp) == NOT_SUPPORTED
    assert lib.vitpe_patch_embed_aug(L.dtype_code(T), *u8, *tail, rng.data_ptr(), 2, 1, sp) == NOT_SUPPORTED
    with pytest.raises(L.VitpeError):
        K.patch_embed(w, bias, cls, None, p, T, images=img, out=outs[0].view(B, P + 1, D))
    torch.cuda.synchronize()
    for o in outs:
        assert bool(torch.isnan(o.float()).all())


# ---- 6. the stand-alone unfold kernels -------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", UNFOLD_DT, ids=ids(UNFOLD_DT))
def test_unfold_kernels_are_the_reshape(K, report, c):
    C, S, p, dt = c
    T = DT[dt]
    _, P, Kk = E.geometry(C, S, p)
    r = report.case("unfold", "-".join(str(v) for v in c))
    img = torch.rand(E.UNFOLD_B, C, S, S, generator=torch.Generator().manual_seed(S + p)) * 4 - 2
    buf, out = guarded((E.UNFOLD_B * P, Kk), T)
    K.unfold(img.cuda(), p, T, out=out)
    r.eq("unfold_bits", nbits(out, E.unfold_img(img, p)), 0)
    r.eq("unfold_guard_lost", int((~torch.isnan(buf[out.numel():].float())).sum()), 0)
    B = len(E.INDEX)
    for tag, pad in (("u8_", None), ("u8aug_", E.UNFOLD_PAD)):
        src = u8_source(C, S, pad=pad)
        buf, out = guarded((B * P, Kk), T)
        ibuf, iout = guarded((B, C, S, S), torch.float32)
        K.unfold_u8(src.pop("data"), src.pop("index"), src.pop("mean"), src.pop("std"), p, T, out=out, img_out=iout, **src)
        want = E.u8_images(C, S, pad=pad)
        r.eq(tag + "patches_bits", nbits(out, E.unfold_img(want, p)), 0)
        r.eq(tag + "images_bits", nbits(iout, want), 0)
        r.eq(tag + "guard_lost", int((~torch.isnan(buf[out.numel():].float())).sum())
             + int((~torch.isnan(ibuf[iout.numel():])).sum()), 0)
    r.done()


def test_unfold_above_the_grid_cap_fp32(K, report):
    """2 162 688 patch rows on 2 097 152 threads: the first 65 536 threads move a second row, of another image"""
    _, dt, C, S, p, B = E.ABOVE_CAP[0]
    _, P, Kk = E.geometry(C, S, p)
    img = torch.rand(B, C, S, S, generator=torch.Generator().manual_seed(1))
    buf, out = guarded((B * P, Kk), DT[dt])
    K.unfold(img.cuda(), p, DT[dt], out=out)
    r = report.case("unfold_above_cap", "unfold-f32")
    r.eq("bits", nbits(out, E.unfold_img(img, p)), 0)
    r.eq("guard_lost", int((~torch.isnan(buf[out.numel():])).sum()), 0)
    r.done()


def test_unfold8_above_the_grid_cap_bf16(K, report):
    """4 198 400 eight-pixel pieces on 4 194 304 threads (p = 8: one piece per patch row)"""
    _, dt, C, S, p, B = E.ABOVE_CAP[2]
    _, P, Kk = E.geometry(C, S, p)
    img = torch.rand(B, C, S, S, generator=torch.Generator().manual_seed(2)) * 4 - 2
    buf, out = guarded((B * P, Kk), DT[dt])
    K.unfold(img.cuda(), p, DT[dt], out=out)
    r = report.case("unfold_above_cap", "unfold8-bf16")
    r.eq("bits", nbits(out, E.unfold_img(img, p)), 0)
    r.eq("guard_lost", int((~torch.isnan(buf[out.numel():].float())).sum()), 0)
    r.done()


def test_unfold_u8_above_the_grid_cap_plain_and_with_rng(K, report):
    """The uint8 gather above the cap: a thread's second row belongs to another image, so the augmented form must draw
    again (aug_b).  Every image is compared in full (the first, the last and all between), every draw against the stream."""
    _, dt, C, S, p, B = E.ABOVE_CAP[1]
    _, P, Kk = E.geometry(C, S, p)
    g = np.random.default_rng(3)
    data = g.integers(0, 256, size=(B, C, S, S), dtype=np.uint8)
    index = g.integers(0, B, size=B).tolist()
    pad = E.UNFOLD_PAD
    r = report.case("unfold_above_cap", "unfold_u8-f32")
    for tag, pd in (("plain_", None), ("rng_", pad)):
        src = u8_source(C, S, index=index, pad=pd, data=data)
        buf, out = guarded((B * P, Kk), DT[dt])
        ibuf, iout = guarded((B, C, S, S), torch.float32)
        K.unfold_u8(src.pop("data"), src.pop("index"), src.pop("mean"), src.pop("std"), p, DT[dt], out=out, img_out=iout, **src)
        want = E.u8_images(C, S, index=index, pad=pd, data=data)
        per_image = (bits(iout) != bits(want)).reshape(B, -1).sum(1)
        r.eq(tag + "images_wrong", int((per_image != 0).sum()), 0)
        r.eq(tag + "patches_bits", nbits(out, E.unfold_img(want, p)), 0)
        r.eq(tag + "guard_lost", int((~torch.isnan(buf[out.numel():])).sum()) + int((~torch.isnan(ibuf[iout.numel():])).sum()), 0)
    prm = K.augment_params(pair(), B, pad, True).cpu().numpy().astype(np.int64)
    r.eq("draws_wrong", int((prm != E.draws(pad, B)).any(1).sum()), 0)
    r.done()


# ---- 7. TrainEngine --------------------------------------------------------------------------------------------------------
MNIST_P8 = dict(in_chans=1, img_size=32, patch_size=8, embed_dim=64, num_heads=2, depth=1)     # K = 64, P = 16, N = 17
CIFAR_P2 = dict(img_size=16, patch_size=2, embed_dim=96, num_heads=3, depth=1)                 # K = 12, P = 64, N = 65


@pytest.mark.parametrize("tag", ["absolute", "rope-mixed"])
@pytest.mark.parametrize("geom,bf16_fused", [(MNIST_P8, True), (CIFAR_P2, False)], ids=["mnist_p8", "cifar_p2"])
def test_engine_on_the_generic_gather_branch(geom, bf16_fused, tag, monkeypatch, report):
    """train.py --dataset mnist --img_size 32 --patch_size 8 and (fp32) --dataset cifar10 --img_size 16 --patch_size 2 run
    the fused embed's p != 4 gather: fp32 logits, loss and every gradient against the oracle (the gates of
    test_engine_runs_the_other_geometries_the_cli_accepts), the unfused route within 1e-5 of the fused one, three captured
    bf16 steps.  K = 12 is no multiple of a bf16 chunk: neither the fused kernel nor the patch GEMM takes it in bf16, so
    that engine is only asked for its route."""
    from test_bench_path_gpu import build
    from vitpe.engine import TrainEngine
    cfg, model = build(tag, {}, geom)
    params = {n: p.detach().cpu().clone() for n, p in model.named_parameters()}
    B = 3
    images, labels = O.closed_form_batch(cfg, B, salt=7)
    ref_logits, ref_loss, ref_grads = O.loss_and_grads(cfg, params, images, labels)
    eng = TrainEngine(model, B, compute_dtype=torch.float32, use_graph=False)
    assert eng.fuse_embed
    eng._load_batch(images.cuda(), labels.cuda())
    eng.forward_backward()
    r = report.case("engine", f"{geom['img_size']}-{geom['patch_size']}-{tag}")
    r.lt("logits", rel_err(eng.logits.cpu(), ref_logits), 1e-4)
    r.lt("loss", abs(float(eng.out2[0]) - float(ref_loss)), 1e-4)
    for n, p in model.named_parameters():
        r.lt("grad:" + n, rel_err(p.grad.cpu(), ref_grads[n]), 1e-3)
    fused_logits = eng.logits.cpu().clone()
    # bf16: the captured step
    _, mb = build(tag, {}, geom, seeded=True)
    eb = TrainEngine(mb, B, compute_dtype=torch.bfloat16, use_graph=bf16_fused)
    assert eb.fuse_embed == bf16_fused
    if bf16_fused:
        for _ in range(3):
            eb.step(images.cuda(), labels.cuda())
        torch.cuda.synchronize()
        r.eq("bf16_nonfinite", int((~torch.isfinite(eb.flat_p)).sum()), 0)
    # the same fp32 engine on unfold + patch GEMM + LayerNorm statistics
    monkeypatch.setenv("VITPE_FUSE_EMBED", "0")
    _, m2 = build(tag, {}, geom)
    e2 = TrainEngine(m2, B, compute_dtype=torch.float32, use_graph=False)
    assert not e2.fuse_embed
    e2._load_batch(images.cuda(), labels.cuda())
    e2.forward_backward()
    r.lt("logits_fused_vs_unfused", rel_err(fused_logits, e2.logits.cpu()), 1e-5)
    r.done()


@pytest.mark.parametrize("dt", E.BOTH)
def test_engine_captured_step_crops_the_mnist_dataset_on_the_generic_branch(dt):
    """A resident MNIST-shaped uint8 dataset, set_augment(3, True): the patch matrix a captured step leaves is
    augment_ref.patches of the pair the step consumed, bit for bit, on two consecutive steps."""
    from test_bench_path_gpu import build
    from vitpe.data import ResidentDataset
    from vitpe.engine import TrainEngine
    B, pad, n = 8, 3, 32
    _, model = build("rope-mixed", {}, MNIST_P8, seeded=True)
    eng = TrainEngine(model, B, compute_dtype=DT[dt], use_graph=True)
    assert eng.fuse_embed
    x = E.dataset(1, 32, n)
    labels = torch.from_numpy(np.random.default_rng(5).integers(0, 10, n))
    eng.attach_dataset(ResidentDataset(torch.tensor(x), labels, *E.STATS[1], "cuda"))
    eng.set_augment(pad, True, rng=pair())
    idx = [5, 9, 31, 0, 9, 17, 2, 30]
    idx_d = torch.tensor(idx, device="cuda")
    seen = []
    for step in range(2):
        before = words(eng.aug_rng)
        assert before == (E.SEED, E.OFFSET + step)
        eng.step_indexed(idx_d)
        torch.cuda.synchronize()
        want = torch.from_numpy(A.patches(x, idx, *E.STATS[1], before, pad, True, 8)).to(DT[dt])
        assert torch.equal(bits(eng.patches), bits(want)), step
        seen.append(eng.patches.cpu().clone())
    assert not torch.equal(seen[0], seen[1]) and eng.graph_fb is not None
    assert torch.isfinite(eng.flat_p).all()
