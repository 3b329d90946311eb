"""Random crop + horizontal flip on the resident uint8 dataset ("Augmentation stream"): the draws, the two gather
kernels, the engine's training steps and the CLI against the numpy restatement in augment_ref.py.  The contract is
bit-level, so every comparison is exact: no tolerance appears anywhere."""
import csv
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_ref as A  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 0xFEDCBA9876543210                    # high bits set
OFFSET = (1 << 32) + 5                       # bits above bit 31
STATS = {1: ((0.1307,), (0.3081,)), 3: ((0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010))}
INDEX = [3, 0, 3, 6, 1]                      # B = 5, record 3 twice
GEOMS = [(3, 32, 4, 4), (1, 28, 4, 2), (3, 16, 8, 3), (1, 28, 7, 1), (1, 8, 4, 8)]     # (C, S, p, pad)


@pytest.fixture(scope="module")
def K():
    from vitpe import kernels
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return kernels


def signed(v):
    return v - (1 << 64) if v >= (1 << 63) else v


def pair(seed=SEED, offset=OFFSET):
    return torch.tensor([signed(seed), signed(offset)], dtype=torch.int64, device="cuda")


def words(rng):
    return tuple(int(v) & 0xFFFFFFFFFFFFFFFF for v in rng.reshape(-1).tolist())


_DATA = {}


def dataset(C, S, n=7):
    """n random uint8 records [n,C,S,S] (host array, device tensor, mean, std on the device), made once per geometry."""
    if (C, S, n) not in _DATA:
        x = np.random.default_rng(100 * C + S).integers(0, 256, size=(n, C, S, S), dtype=np.uint8)
        mean, std = STATS[C]
        _DATA[(C, S, n)] = (x, torch.from_numpy(x).cuda(), torch.tensor(mean, device="cuda"), torch.tensor(std, device="cuda"))
    return _DATA[(C, S, n)]


_REF = {}


def ref_images(C, S, pad, hflip, index):
    key = (C, S, pad, hflip, None if index is None else tuple(index))
    if key not in _REF:
        x = dataset(C, S)[0]
        _REF[key] = A.images(x, index, *STATS[C], (SEED, OFFSET), pad, hflip)
    return _REF[key]


# ---- 1. the draws -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hflip", [True, False])
@pytest.mark.parametrize("pad", [0, 1, 4])
def test_augment_params_are_the_documented_stream(K, pad, hflip):
    got = K.augment_params(pair(), 37, pad, hflip)
    assert got.dtype == torch.int32 and tuple(got.shape) == (37, 3)
    assert np.array_equal(got.cpu().numpy().astype(np.int64), A.params((SEED, OFFSET), 37, pad, hflip))


# ---- 2. vitpe_unfold_u8_aug -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_index", [True, False])
@pytest.mark.parametrize("C,S,p,pad", GEOMS)
def test_unfold_u8_with_rng_equals_the_reference(K, C, S, p, pad, use_index):
    x, xd, mean, std = dataset(C, S)
    index = INDEX if use_index else None
    idx = torch.tensor(INDEX, device="cuda") if use_index else None
    B = len(INDEX) if use_index else x.shape[0]
    want_img = ref_images(C, S, pad, True, index)
    want = A.unfold(want_img, p)
    prm = A.params((SEED, OFFSET), B, pad, True)
    assert prm[:, 2].min() == 0 and prm[:, 2].max() == 1          # the case has flipped and unflipped slots
    img = torch.full((B, C, S, S), float("nan"), device="cuda")
    got = K.unfold_u8(xd, idx, mean, std, p, torch.float32, img_out=img, rng=pair(), crop_pad=pad, hflip=True)
    assert tuple(got.shape) == want.shape
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert np.array_equal(img.cpu().numpy().view(np.uint32), want_img.view(np.uint32))
    got16 = K.unfold_u8(xd, idx, mean, std, p, torch.bfloat16, rng=pair(), crop_pad=pad, hflip=True)
    assert torch.equal(got16.cpu(), torch.from_numpy(want).to(torch.bfloat16))
    if use_index:      # the same record in two slots gets two independent draws
        assert not np.array_equal(prm[0], prm[2]) and not np.array_equal(want_img[0], want_img[2])
    if pad == S:       # windows that lie wholly in the padding are legal: every pixel is (0 - mean) / std
        outside = [b for b in range(B) if prm[b, 0] == 0 or prm[b, 0] == 2 * pad or prm[b, 1] == 0 or prm[b, 1] == 2 * pad]
        zero = (np.float32(0) - np.float32(STATS[C][0][0])) / np.float32(STATS[C][1][0])
        assert use_index or outside                                # (slot 6 of the seven has ox = 0)
        for b in outside:
            assert (want_img[b] == zero).all()


def test_augment_batch_returns_the_augmented_images(K):
    from vitpe.data import ResidentDataset, augment_batch
    C, S, pad = 3, 32, 4
    x = dataset(C, S)[0]
    ds = ResidentDataset(torch.from_numpy(x), torch.arange(x.shape[0]), *STATS[C], "cuda")
    got = augment_batch(ds, torch.tensor(INDEX, device="cuda"), pair(), crop_pad=pad, hflip=True)
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(INDEX), C, S, S)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), ref_images(C, S, pad, True, INDEX).view(np.uint32))


# ---- 3. vitpe_patch_embed_aug -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C,S,p,D,pad", [(3, 32, 4, 192, 4), (1, 28, 4, 96, 2)])
def test_fused_embed_with_rng(K, C, S, p, D, pad, dt):
    from vitpe.data import ResidentDataset, augment_batch
    x, xd, mean, std = dataset(C, S)
    B, P, Kp = len(INDEX), (S // p) ** 2, C * p * p
    assert K.patch_embed_supported(dt, C, S, p, D)
    g = torch.Generator().manual_seed(S)
    w = (torch.randn(D, Kp, generator=g) * 0.2).cuda().to(dt)
    bias, cls = torch.randn(D, generator=g).cuda(), torch.randn(D, generator=g).cuda()
    ape = torch.randn(P, D, generator=g).cuda()
    idx = torch.tensor(INDEX, device="cuda")

    def run(**src):
        tok = torch.empty(B, P + 1, D, dtype=dt, device="cuda")
        pat = torch.empty(B * P, Kp, dtype=dt, device="cuda")
        st = (torch.empty(B * (P + 1), device="cuda"), torch.empty(B * (P + 1), device="cuda"))
        K.patch_embed(w, bias, cls, ape, p, dt, out=tok, patches_out=pat, stats=st, **src)
        return tok, pat, st

    tok, pat, st = run(data=xd, index=idx, mean=mean, std=std, rng=pair(), crop_pad=pad, hflip=True)
    want = torch.from_numpy(A.unfold(ref_images(C, S, pad, True, INDEX), p)).to(dt)
    assert torch.equal(pat.cpu(), want)
    ds = ResidentDataset(torch.from_numpy(x), torch.arange(x.shape[0]), *STATS[C], "cuda")
    tok2, pat2, st2 = run(images=augment_batch(ds, idx, pair(), crop_pad=pad, hflip=True))
    assert torch.equal(pat2, pat) and torch.equal(tok2, tok)
    assert torch.equal(st2[0], st[0]) and torch.equal(st2[1], st[1])
    assert torch.isfinite(tok.float()).all() and torch.isfinite(st[1]).all()


# ---- 4. unaugmented identity ------------------------------------------------------------------------------------------------
# whether the fused kernel has the geometry: K = 192 is outside it (that case keeps only its unfold half), K = 64 at p = 8 is
# its generic gather branch
NO_CROP_FUSED = {(3, 32, 4, 192): True, (3, 16, 8, 96): False, (1, 16, 8, 96): True}


@pytest.mark.parametrize("C,S,p,D", list(NO_CROP_FUSED))
def test_without_crop_and_flip_nothing_changes(K, C, S, p, D):
    from vitpe import _lib as L
    x, xd, mean, std = dataset(C, S)
    B, P, Kp, dt = len(INDEX), (S // p) ** 2, C * p * p, torch.bfloat16
    idx = torch.tensor(INDEX, device="cuda")
    lib, sp = L.lib(), L.stream_ptr()
    # unfold_u8: no rng / rng with pad = 0 and no flip / the _aug entry with rng = NULL
    img0, img1, img2 = (torch.empty(B, C, S, S, device="cuda") for _ in range(3))
    plain = K.unfold_u8(xd, idx, mean, std, p, dt, img_out=img0)
    off = K.unfold_u8(xd, idx, mean, std, p, dt, img_out=img1, rng=pair(), crop_pad=0, hflip=False)
    null = torch.empty_like(plain)
    assert lib.vitpe_unfold_u8_aug(L.BF16, xd.data_ptr(), idx.data_ptr(), mean.data_ptr(), std.data_ptr(), null.data_ptr(),
                                   img2.data_ptr(), B, C, S, p, None, 4, 1, sp) == 0
    assert torch.equal(off, plain) and torch.equal(null, plain) and torch.equal(img1, img0) and torch.equal(img2, img0)
    assert np.array_equal(img0.cpu().numpy(), A.images(x, INDEX, *STATS[C], (1, 2), 0, False))
    # patch_embed (where the fused kernel has the geometry)
    assert K.patch_embed_supported(dt, C, S, p, D) == NO_CROP_FUSED[(C, S, p, D)]
    if NO_CROP_FUSED[(C, S, p, D)]:
        g = torch.Generator().manual_seed(1)
        w = (torch.randn(D, Kp, generator=g) * 0.2).cuda().to(dt)
        bias, cls = torch.randn(D, generator=g).cuda(), torch.randn(D, generator=g).cuda()
        src = dict(data=xd, index=idx, mean=mean, std=std)
        outs = []
        for extra in ({}, dict(rng=pair(), crop_pad=0, hflip=False)):
            pat = torch.empty(B * P, Kp, dtype=dt, device="cuda")
            outs.append((K.patch_embed(w, bias, cls, None, p, dt, patches_out=pat, **src, **extra), pat))
        tok, pat = torch.empty_like(outs[0][0]), torch.empty_like(outs[0][1])
        args = [L.BF16, None, xd.data_ptr(), idx.data_ptr(), mean.data_ptr(), std.data_ptr(), w.data_ptr(), bias.data_ptr(),
                cls.data_ptr(), None, tok.data_ptr(), pat.data_ptr(), None, None, B, C, S, p, D, 1e-5]
        assert lib.vitpe_patch_embed_aug(*args, None, 4, 1, sp) == 0
        outs.append((tok, pat))
        for t, q in outs[1:]:
            assert torch.equal(t, outs[0][0]) and torch.equal(q, outs[0][1])
        # fp32 images together with a pair: invalid, nothing is launched
        img = torch.zeros(B, C, S, S, device="cuda")
        args[1], args[2] = img.data_ptr(), None
        rng = pair()
        assert lib.vitpe_patch_embed_aug(*args, rng.data_ptr(), 4, 1, sp) == 1
        args[1], args[2] = None, xd.data_ptr()
        assert lib.vitpe_patch_embed_aug(*args, rng.data_ptr(), S + 1, 1, sp) == 1      # pad > S
        assert lib.vitpe_patch_embed_aug(*args, rng.data_ptr(), -1, 1, sp) == 1
        with pytest.raises(L.VitpeError):
            K.patch_embed(w, bias, cls, None, p, dt, images=img, rng=rng, crop_pad=4)
    rng = pair()
    assert lib.vitpe_unfold_u8_aug(L.BF16, xd.data_ptr(), idx.data_ptr(), mean.data_ptr(), std.data_ptr(), null.data_ptr(),
                                   None, B, C, S, p, rng.data_ptr(), S + 1, 1, sp) == 1
    torch.cuda.synchronize()


# ---- 5. / 6. TrainEngine ----------------------------------------------------------------------------------------------------
def _engine(extras, B, depth=2, patch=4, n=32, dt=torch.bfloat16):
    from models.vit import VisionTransformer
    from vitpe.data import ResidentDataset
    from vitpe.engine import TrainEngine
    torch.manual_seed(0)
    model = VisionTransformer(img_size=32, patch_size=patch, embed_dim=192, depth=depth, num_heads=6,
                              pos_encoding="rope-axial").cuda()
    eng = TrainEngine(model, B, compute_dtype=dt, use_graph=True, extras=extras)
    x = dataset(3, 32, n)[0]
    labels = torch.from_numpy(np.random.default_rng(5).integers(0, 10, n))
    ds = ResidentDataset(torch.from_numpy(x), labels, *STATS[3], "cuda")
    return eng, ds, x


def _ref_patches(x, idx, rng_words, pad, hflip, p, dt=torch.bfloat16):
    return torch.from_numpy(A.patches(x, idx, *STATS[3], rng_words, pad, hflip, p)).to(dt)


@pytest.mark.parametrize("extras", [False, True])
def test_engine_steps_crop_and_flip_anew_every_step(extras):
    from vitpe._lib import VitpeError
    B, pad = 8, 4
    eng, ds, x = _engine(extras, B)
    assert eng.fuse_embed
    table0 = eng.rng_table.clone() if extras else None
    eng.attach_dataset(ds)
    eng.set_augment(pad, True)
    assert tuple(eng.aug_rng.shape) == (1, 2) and eng.aug_rng.dtype == torch.int64 and eng.aug_rng.is_cuda
    if extras:
        assert tuple(eng.rng_table.shape) == tuple(table0.shape)             # the site table keeps its shape
    idx = [5, 9, 31, 0, 9, 17, 2, 30]
    idx_d = torch.tensor(idx, device="cuda")
    seen = []
    for step in range(2):                                                    # (the first one captures the graph)
        before = words(eng.aug_rng)
        eng.step_indexed(idx_d)
        torch.cuda.synchronize()
        after = words(eng.aug_rng)
        assert after[0] == before[0] and after[1] == (before[1] + 1) % (1 << 64)
        assert torch.equal(eng.patches.cpu(), _ref_patches(x, idx, before, pad, True, 4)), step
        seen.append(eng.patches.cpu().clone())
    assert not torch.equal(seen[0], seen[1])
    assert eng.graph_fb is not None
    # evaluation never augments: the unaugmented patch matrix, and the logits of an engine that never had it set
    plain = _ref_patches(x, idx, (0, 0), 0, False, 4)
    stream = words(eng.aug_rng)
    logits = eng.forward_indexed(idx_d).clone()
    assert torch.equal(eng.patches.cpu(), plain) and words(eng.aug_rng) == stream
    other, _, _ = _engine(extras, B)
    other.attach_dataset(ds)
    other.flat_p.copy_(eng.flat_p)
    other.refresh_shadows()
    assert torch.equal(other.forward_indexed(idx_d), logits) and torch.isfinite(logits).all()
    # a caller's pair is copied in as it is
    eng.set_augment(pad, True, rng=pair())
    assert words(eng.aug_rng) == (SEED, OFFSET) and eng.graph_fb is None
    eng.step_indexed(idx_d)
    torch.cuda.synchronize()
    assert torch.equal(eng.patches.cpu(), _ref_patches(x, idx, (SEED, OFFSET), pad, True, 4))
    assert words(eng.aug_rng) == (SEED, OFFSET + 1)
    # no dataset, augmentation on: refused, not trained without the crop
    eng.attach_dataset(None)
    with pytest.raises(VitpeError) as e:
        eng.step(torch.zeros(B, 3, 32, 32, device="cuda"), torch.zeros(B, dtype=torch.int64, device="cuda"))
    assert "attach_dataset" in str(e.value) and "augment_batch" in str(e.value)
    eng.attach_dataset(ds)
    # the defaults switch it off again
    eng.set_augment()
    assert eng.aug_rng is None and eng.graph_fb is None
    for _ in range(2):
        eng.step_indexed(idx_d)
        torch.cuda.synchronize()
        assert torch.equal(eng.patches.cpu(), plain)
    assert "aug_rng" not in eng.model.state_dict()
    with pytest.raises(VitpeError):
        eng.set_augment(33, False)


def test_engine_unfold_route_crops_too():
    """img 32 / patch 2: 257 tokens, outside the fused embed -- vitpe_unfold_u8_aug + the patch GEMM.  fp32: the patch
    GEMM's bf16 operands need K = C p^2 = 12 to be a multiple of 8."""
    B, pad = 2, 4
    eng, ds, x = _engine(False, B, depth=1, patch=2, dt=torch.float32)
    assert not eng.fuse_embed and eng.N == 257
    eng.attach_dataset(ds)
    eng.set_augment(pad, True, rng=pair())
    idx = [7, 7]
    eng.step_indexed(torch.tensor(idx, device="cuda"))
    torch.cuda.synchronize()
    assert torch.equal(eng.patches.cpu(), _ref_patches(x, idx, (SEED, OFFSET), pad, True, 2, torch.float32))
    assert words(eng.aug_rng) == (SEED, OFFSET + 1)
    assert torch.isfinite(eng.logits.float()).all()


# ---- 7. the CLI -------------------------------------------------------------------------------------------------------------
def test_train_py_with_random_crop_and_hflip(tmp_path):
    import train as T
    g = np.random.default_rng(0)
    root = tmp_path / "data" / "cifar-10-batches-bin"
    root.mkdir(parents=True)
    for name, n in [(f"data_batch_{i}.bin", 16) for i in range(1, 6)] + [("test_batch.bin", 32)]:
        rec = np.zeros((n, 3073), dtype=np.uint8)
        rec[:, 0] = g.integers(0, 10, n)
        rec[:, 1:] = g.integers(0, 256, (n, 3072))
        rec.tofile(root / name)
    T.main(["--dataset", "cifar10", "--pos_encoding", "rope-axial", "--data_dir", str(tmp_path / "data"), "--log_dir",
            str(tmp_path / "logs"), "--ckpt_dir", str(tmp_path / "ckpt"), "--epochs", "1", "--batch_size", "16", "--depth", "2",
            "--random_crop", "4", "--hflip"])
    logs = list((tmp_path / "logs").glob("cifar10_rope-axial_*.csv"))
    rows = list(csv.reader(logs[0].read_text().strip().splitlines()))
    assert len(rows) == 2 and rows[0][:3] == ["epoch", "train_loss", "train_acc"]
    assert all(math.isfinite(float(v)) for v in rows[1]) and float(rows[1][1]) > 0.0
