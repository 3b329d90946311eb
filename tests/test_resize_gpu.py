"""transforms.Resize on the device (vitpe_resize_u8) against PIL's output recorded in tests/golden/resize.npz.  The
reference's transform is integer arithmetic, so every comparison is byte for byte: a differing byte is a bug."""
import math
import struct

import numpy as np
import pytest
import torch

from oracle import vit_oracle as O

pytestmark = pytest.mark.gpu

CASES = [("mnist", 28, S) for S in (14, 16, 32, 64, 224)] + [("cifar", 32, S) for S in (16, 24, 48, 64, 224)]
SENTINEL = 0xA5


def fixture(golden, name, S):
    g = golden("resize")
    return torch.from_numpy(g[f"{name}/{S}/x"]), torch.from_numpy(g[f"{name}/{S}/y"])


@pytest.mark.parametrize("name,S0,S", CASES)
def test_resize_u8_equals_pil_byte_for_byte(golden, name, S0, S):
    from vitpe import kernels as K
    x, y = fixture(golden, name, S)
    out = K.resize_u8(x.cuda(), S)
    assert out.dtype == torch.uint8 and out.shape == y.shape
    assert torch.equal(out.cpu(), y)


@pytest.mark.parametrize("name,S0", [("mnist", 28), ("cifar", 32)])
def test_resize_u8_to_the_same_size_is_the_identity(golden, name, S0):
    from vitpe import kernels as K
    x, _ = fixture(golden, name, 64)
    xd = x.cuda()
    out = K.resize_u8(xd, S0)
    assert out.data_ptr() != xd.data_ptr() and torch.equal(out.cpu(), x)


@pytest.mark.parametrize("name,S0,S", [("mnist", 28, 14), ("mnist", 28, 224), ("cifar", 32, 24), ("cifar", 32, 64)])
def test_resize_u8_writes_only_its_output_and_repeats(golden, name, S0, S):
    from vitpe import kernels as K
    x, y = fixture(golden, name, S)
    xd = x.cuda()
    tail = 4096
    bufs = []
    for _ in range(2):
        buf = torch.full((y.numel() + tail,), SENTINEL, dtype=torch.uint8, device="cuda")
        K.resize_u8(xd, S, out=buf)
        bufs.append(buf.cpu())
    assert torch.equal(bufs[0][:y.numel()].view(y.shape), y)
    assert bool((bufs[0][y.numel():] == SENTINEL).all())
    assert torch.equal(bufs[0], bufs[1])
    assert torch.equal(xd.cpu(), x)                      # the source is read only


def test_resize_u8_odd_target_and_odd_source(golden):
    """Sizes off the packed-store path (S % 4 != 0, odd S0) against a numpy application of the library's own tables."""
    from test_resize_cpu import apply_resize
    from vitpe import kernels as K
    g = torch.Generator().manual_seed(11)
    for S0, S in ((32, 30), (28, 45), (27, 64), (9, 5), (64, 4), (8, 511), (64, 512), (33, 33)):
        x = torch.randint(0, 256, (3, 2, S0, S0), generator=g, dtype=torch.uint8)
        x[1] = ((torch.arange(S0)[:, None] + torch.arange(S0)[None]) % 2 * 255).to(torch.uint8)
        bounds, kk = K.resize_coeffs(S0, S)
        want = x.numpy() if S == S0 else apply_resize(x.numpy(), bounds.numpy(), kk.numpy())
        buf = torch.full((want.size + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
        K.resize_u8(x.cuda(), S, out=buf)
        buf = buf.cpu()
        assert np.array_equal(buf[:want.size].view(3, 2, S, S).numpy(), want), (S0, S)
        assert bool((buf[want.size:] == SENTINEL).all()), (S0, S)


def test_resize_u8_many_planes(golden):
    """40 000 CIFAR-shaped images (120 000 planes, 0.49 GB out): the grid walk and the 64-bit plane offsets."""
    from vitpe import kernels as K
    x, y = fixture(golden, "cifar", 64)
    reps = 10000
    big = x.cuda().repeat(reps, 1, 1, 1)
    out = K.resize_u8(big, 64)
    assert out.shape == (4 * reps, 3, 64, 64)
    assert bool((out.view(reps, 4, 3, 64, 64) == y.cuda()).all())


def test_resize_u8_refuses_what_it_does_not_cover():
    from vitpe import kernels as K
    from vitpe._lib import VitpeError
    ok = torch.zeros((2, 3, 32, 32), dtype=torch.uint8, device="cuda")
    for bad, S in ((torch.zeros((1, 1, 128, 128), dtype=torch.uint8, device="cuda"), 64), (ok, 1024), (ok, 2),
                   (torch.zeros((2, 3, 32, 28), dtype=torch.uint8, device="cuda"), 64),
                   (torch.zeros((2, 3, 32, 32), dtype=torch.float32, device="cuda"), 64),
                   (torch.zeros((2, 3, 32, 32), dtype=torch.uint8), 64),
                   (torch.zeros((3, 32, 32), dtype=torch.uint8, device="cuda"), 64)):
        with pytest.raises(VitpeError):
            K.resize_u8(bad, S)
    with pytest.raises(VitpeError):                       # too small a destination
        K.resize_u8(ok, 64, out=torch.zeros(2 * 3 * 64 * 64 - 1, dtype=torch.uint8, device="cuda"))


# ---- dataset files -----------------------------------------------------------------------------------------------------
def write_cifar(root, images, labels, train):
    """CIFAR-10 binary version: 1 label byte + 3072 channel-planar pixel bytes per record; the train split is cut over
    the five batch files."""
    root.mkdir(parents=True, exist_ok=True)
    rec = np.concatenate([np.asarray(labels, dtype=np.uint8)[:, None], np.asarray(images).reshape(len(labels), 3072)], 1)
    if train:
        cuts = np.linspace(0, len(labels), 6).astype(int)
        for i in range(5):
            rec[cuts[i]:cuts[i + 1]].tofile(root / f"data_batch_{i + 1}.bin")
    else:
        rec.tofile(root / "test_batch.bin")


def write_mnist(root, images, labels, train):
    root.mkdir(parents=True, exist_ok=True)
    pre = "train" if train else "t10k"
    n = len(labels)
    with open(root / f"{pre}-images-idx3-ubyte", "wb") as f:
        f.write(struct.pack(">IIII", 0x00000803, n, 28, 28))
        f.write(np.asarray(images, dtype=np.uint8).reshape(n, 28, 28).tobytes())
    with open(root / f"{pre}-labels-idx1-ubyte", "wb") as f:
        f.write(struct.pack(">II", 0x00000801, n))
        f.write(np.asarray(labels, dtype=np.uint8).tobytes())


@pytest.mark.parametrize("name,S0,S", CASES)
def test_resident_dataset_from_files_holds_the_pil_output(golden, tmp_path, name, S0, S):
    from vitpe.data import ResidentDataset
    x, y = fixture(golden, name, S)
    reps = 3                                              # 6 or 12 records: every CIFAR batch file gets at least one
    xs, ys = x.repeat(reps, 1, 1, 1), y.repeat(reps, 1, 1, 1)
    labels = np.arange(xs.shape[0]) % 10
    dataset = "cifar10" if name == "cifar" else "mnist"
    for train in (True, False):
        (write_cifar if name == "cifar" else write_mnist)(tmp_path, xs.numpy(), labels, train)
        ds = ResidentDataset.from_files(dataset, str(tmp_path), train, "cuda", S)
        assert ds.images.dtype == torch.uint8 and ds.images.is_cuda and len(ds) == xs.shape[0]
        assert torch.equal(ds.images.cpu(), ys)
        assert ds.labels.dtype == torch.int64 and ds.labels.cpu().tolist() == labels.tolist()
        assert ds.mean.cpu().tolist() == torch.tensor(O.DATASET_STATS[dataset][0]).tolist()
        assert ds.std.cpu().tolist() == torch.tensor(O.DATASET_STATS[dataset][1]).tolist()


def test_resident_dataset_resized(golden):
    from vitpe.data import ResidentDataset
    x, y = fixture(golden, "cifar", 48)
    mean, std = O.DATASET_STATS["cifar10"]
    ds = ResidentDataset(x, torch.arange(4), mean, std, "cuda")
    assert ds.resized(32) is ds
    big = ds.resized(48)
    assert torch.equal(big.images.cpu(), y) and torch.equal(big.labels, ds.labels)
    assert torch.equal(big.mean, ds.mean) and torch.equal(big.std, ds.std)
    assert torch.equal(ds.images.cpu(), x)


# ---- train.py end to end -----------------------------------------------------------------------------------------------
def synthetic_files(tmp_path, dataset, n_train, n_test):
    rng = np.random.default_rng(0)
    if dataset == "cifar10":
        root, shape, write = tmp_path / "data" / "cifar-10-batches-bin", (3, 32, 32), write_cifar
    else:
        root, shape, write = tmp_path / "data" / "MNIST" / "raw", (1, 28, 28), write_mnist
    for n, train in ((n_train, True), (n_test, False)):
        write(root, rng.integers(0, 256, (n,) + shape, dtype=np.uint8), rng.integers(0, 10, n), train)


@pytest.mark.parametrize("dataset,flags", [
    ("cifar10", ["--img_size", "64", "--patch_size", "8", "--batch_size", "32", "--embed_dim", "96", "--depth", "2",
                 "--num_heads", "3"]),
    ("cifar10", ["--img_size", "224", "--patch_size", "16", "--embed_dim", "768", "--num_heads", "12", "--depth", "1",
                 "--batch_size", "8"]),
    ("mnist", ["--img_size", "32", "--batch_size", "32", "--embed_dim", "96", "--depth", "2", "--num_heads", "3"]),
], ids=["cifar10-64-p8", "cifar10-224-p16", "mnist-32"])
def test_train_py_runs_on_resized_datasets(tmp_path, dataset, flags):
    """train.py with an --img_size away from the records' own size: two short epochs on files in the dataset's format
    (synthetic content), CSV log and checkpoint written, every logged loss finite."""
    import train as T
    synthetic_files(tmp_path, dataset, 80, 24)
    T.main(["--dataset", dataset, "--pos_encoding", "rope-axial", "--epochs", "2", "--data_dir", str(tmp_path / "data"),
            "--log_dir", str(tmp_path / "logs"), "--ckpt_dir", str(tmp_path / "ckpt")] + flags)
    assert (tmp_path / "ckpt" / f"{dataset}_rope-axial_best.pth").exists()
    logs = list((tmp_path / "logs").glob(f"{dataset}_rope-axial_*.csv"))
    rows = logs[0].read_text().strip().splitlines()
    assert rows[0] == "epoch,train_loss,train_acc,test_loss,test_acc,best_acc" and len(rows) == 3
    for row in rows[1:]:
        _, train_loss, _, test_loss, _, _ = row.split(",")
        assert math.isfinite(float(train_loss)) and math.isfinite(float(test_loss)) and float(train_loss) > 0


# ---- engine parity -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dataset,S,patch", [("cifar", "cifar10", 64, 8), ("mnist", "mnist", 32, 4),
                                                  ("cifar", "cifar10", 16, 4)])
def test_engine_on_the_resized_dataset_equals_engine_on_pil_images(golden, name, dataset, S, patch):
    """A TrainEngine stepping on indices into the device-resized resident dataset computes the same logits, bit for bit
    in fp32, as one fed the fixture's PIL output normalised on the host."""
    from models.vit import VisionTransformer
    from vitpe.data import ResidentDataset
    from vitpe.engine import TrainEngine
    x, y = fixture(golden, name, S)
    B = x.shape[0]
    labels = torch.arange(B) % 10
    mean, std = O.DATASET_STATS[dataset]
    ds = ResidentDataset(x, labels, mean, std, "cuda").resized(S)
    kw = dict(img_size=S, patch_size=patch, in_chans=x.shape[1], embed_dim=96, depth=2, num_heads=3,
              pos_encoding="rope-axial")
    cfg = O.VitConfig(**kw)
    engines = []
    for resident in (True, False):
        model = VisionTransformer(**kw)
        with torch.no_grad():
            for n, p in model.named_parameters():
                p.copy_(O.closed_form_tensor(n, tuple(p.shape), cfg))
        eng = TrainEngine(model.cuda().set_compute_dtype(torch.float32), B, compute_dtype=torch.float32, use_graph=False)
        if resident:
            eng.attach_dataset(ds)
        engines.append(eng)
    idx = torch.tensor([2, 0, 3, 1][:B] if B == 4 else [1, 0])
    engines[0].step_indexed(idx.cuda())
    engines[1].step(O.normalize_u8(y[idx], mean, std).cuda(), labels[idx].cuda())
    torch.cuda.synchronize()
    assert torch.equal(engines[0].labels.cpu(), engines[1].labels.cpu())
    assert bool(torch.isfinite(engines[0].logits).all())
    assert torch.equal(engines[0].logits.cpu(), engines[1].logits.cpu())
