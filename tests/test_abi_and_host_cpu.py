"""CPU-only checks: the C-ABI library loads and exports every symbol include/vitpe.h declares,
and the host-side mirror of the reference interface (no compute calls without a GPU)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO


def test_library_exports_every_declared_symbol():
    from vitpe import _lib
    protos = _lib.parse_header()
    assert len(protos) >= 25
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in protos:
        assert hasattr(handle, name), f"{name} declared in include/vitpe.h but not exported"
    # and nothing vitpe_* is exported without a declaration
    out = os.popen(f"nm -D --defined-only {_lib.LIB_PATH}").read()
    exported = set(re.findall(r"\bT (vitpe_\w+)", out))
    debug = set(_lib.parse_header(_lib.DEBUG_HEADER_PATH))      # self-tests / census: include/vitpe_debug.h, not the product ABI
    assert debug and all("debug" in n or "selftest" in n for n in debug) and not (debug & set(protos))
    assert not any("debug" in n or "selftest" in n for n in protos)
    assert exported == set(protos) | debug, exported ^ (set(protos) | debug)
    assert _lib.lib().vitpe_abi_version() == 5


def test_pure_host_entry_points():
    from vitpe import _lib
    h = _lib.lib()
    assert h.vitpe_fused_attention_supported(_lib.BF16, 65, 192, 32) == 1
    assert h.vitpe_fused_attention_supported(_lib.F32, 65, 96, 32) == 1
    assert h.vitpe_fused_attention_supported(_lib.BF16, 197, 768, 64) == 0
    assert h.vitpe_layernorm_bwd_blocks(33280) == 256 and h.vitpe_layernorm_bwd_blocks(5) == 2


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from vitpe import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(_lib.VitpeError, match="no CPU fallback"):
        _lib.lib()


def test_product_package_never_imports_the_oracle():
    pkg = os.path.join(REPO, "vit-rpe-rope_amd", "vitpe")
    for f in os.listdir(pkg):
        if f.endswith(".py") and f != "smoke.py":   # smoke() may use the oracle as the checker
            assert "oracle" not in open(os.path.join(pkg, f)).read(), f
    for f in ("models/__init__.py", "models/vit.py", "train.py"):
        assert "oracle" not in open(os.path.join(REPO, f)).read(), f


MODES = [("none", {}), ("absolute", {}), ("relative", {}), ("polynomial", {}),
         ("polynomial_perhead", {"pos_encoding": "polynomial", "poly_shared_heads": False}),
         ("rope-axial", {}), ("rope-mixed", {})]


@pytest.mark.parametrize("tag,extra", MODES)
def test_constructor_and_state_dict_surface(golden, tag, extra):
    """Same constructor, parameter count and state_dict key set (incl. the aliased
    blocks.i.attn.pos_encoding.* keys) as the reference."""
    from models.vit import VisionTransformer
    g = golden("model")
    kw = dict(pos_encoding=extra.get("pos_encoding", tag))
    kw.update({k: v for k, v in extra.items() if k != "pos_encoding"})
    m = VisionTransformer(img_size=32, patch_size=4, in_chans=3, num_classes=10, embed_dim=192, depth=6,
                          num_heads=6, mlp_ratio=4., rope_theta=100.0, poly_degree=3,
                          **{"poly_shared_heads": True, **kw})
    assert sorted(m.state_dict().keys()) == list(g[f"full/{tag}/state_keys"])
    assert sum(p.numel() for p in m.parameters()) == int(g[f"full/{tag}/n_params"])
    assert float(m.cls_token.abs().max()) == 0.0 and m.blocks[0].attn.qkv.bias is None
    assert m.num_patches == 64 and m.head_dim == 32 and m.pos_encoding_type == kw["pos_encoding"]
    if tag != "absolute":
        assert m.blocks[0].attn.pos_encoding is m.pos_embed and m.blocks[5].attn.pos_encoding is m.pos_embed
    else:
        assert m.blocks[0].attn.pos_encoding is None and m.pos_embed.pos_embed.shape == (1, 5000, 192)


def test_reference_error_behaviour(golden):
    from models.vit import VisionTransformer
    from models.rope_utils import reshape_for_broadcast
    with pytest.raises(ValueError) as e:
        VisionTransformer(pos_encoding="bogus")
    assert str(e.value) == str(golden("model")["bad_mode_message"])
    with pytest.raises(ValueError):
        reshape_for_broadcast(torch.zeros(4), torch.zeros(1, 1, 4, 8))
    assert reshape_for_broadcast(torch.zeros(64, 16), torch.zeros(2, 6, 64, 32)).shape == (1, 1, 64, 16)
    assert reshape_for_broadcast(torch.zeros(6, 64, 16), torch.zeros(2, 6, 64, 32)).shape == (1, 6, 64, 16)


def test_integer_index_buffer_bit_exact_on_host(golden):
    from models.positional_encoding import RelativePositionalEncoding
    for N in (65, 197):
        r = RelativePositionalEncoding(N - 1, num_heads=2)
        assert r.relative_position_index.dtype == torch.int64
        assert np.array_equal(r.relative_position_index.numpy(), golden("tables")[f"rel_index_{N}"])


def test_rope_mixed_init_matches_reference_rng_stream(golden):
    from models.positional_encoding import RoPEMixed
    torch.manual_seed(1234)
    m = RoPEMixed(dim=32, num_heads=6, theta=100.0)
    assert np.allclose(m.freqs.detach().numpy(), golden("tables")["mixed_init_freqs"], rtol=1e-6, atol=1e-7)


def test_flat_layout_and_shards():
    from vitpe import ddp
    offs, n = ddp.flat_layout([5, 8, 13, 1], align=8)
    assert offs == [0, 8, 16, 32] and n == 40
    assert ddp.shard_bounds(4096, 3, 8) == (1536, 2048)
    with pytest.raises(ValueError):
        ddp.shard_bounds(100, 0, 8)


def test_cpu_tensors_are_refused_not_computed():
    from models.vit import VisionTransformer
    from vitpe._lib import VitpeError
    m = VisionTransformer(embed_dim=96, depth=1, num_heads=3, pos_encoding="none")
    with pytest.raises(VitpeError, match="no CPU fallback"):
        m(torch.zeros(2, 3, 32, 32))


# ---- resident input pipeline: file readers, sharding, the oracle's transform ----------------
def _write_cifar_bin(path, n, seed):
    rng = np.random.default_rng(seed)
    rec = np.zeros((n, 3073), dtype=np.uint8)
    rec[:, 0] = rng.integers(0, 10, n)
    rec[:, 1:] = rng.integers(0, 256, (n, 3072))
    rec.tofile(path)
    return rec


def test_cifar10_binary_reader_and_mnist_idx_reader(tmp_path):
    import struct
    from vitpe import data as D
    from vitpe._lib import VitpeError
    recs = [_write_cifar_bin(tmp_path / f"data_batch_{i}.bin", 7, i) for i in range(1, 6)]
    test = _write_cifar_bin(tmp_path / "test_batch.bin", 5, 9)
    x, y = D.read_cifar10_bin(str(tmp_path), True)
    assert x.shape == (35, 3, 32, 32) and x.dtype == np.uint8 and y.dtype == np.int64
    allrec = np.concatenate(recs)
    assert np.array_equal(y, allrec[:, 0]) and np.array_equal(x.reshape(35, -1), allrec[:, 1:])   # channel-planar records
    xt, yt = D.read_cifar10_bin(str(tmp_path), False)
    assert np.array_equal(xt.reshape(5, -1), test[:, 1:]) and np.array_equal(yt, test[:, 0])
    (tmp_path / "data_batch_3.bin").write_bytes(b"\x00" * 100)
    with pytest.raises(VitpeError):
        D.read_cifar10_bin(str(tmp_path), True)
    # MNIST idx
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (4, 28, 28), dtype=np.uint8)
    lab = rng.integers(0, 10, 4).astype(np.uint8)
    (tmp_path / "t10k-images-idx3-ubyte").write_bytes(struct.pack(">IIII", 0x803, 4, 28, 28) + img.tobytes())
    (tmp_path / "t10k-labels-idx1-ubyte").write_bytes(struct.pack(">II", 0x801, 4) + lab.tobytes())
    xm, ym = D.read_mnist_idx(str(tmp_path), False, 32)
    assert xm.shape == (4, 1, 32, 32) and xm.dtype == np.uint8 and np.array_equal(ym, lab)
    x28, _ = D.read_mnist_idx(str(tmp_path), False, 28)
    assert np.array_equal(x28[:, 0], img)
    with pytest.raises(VitpeError):
        D.read_mnist_idx(str(tmp_path), True)   # train files absent / wrong magic is an error, never a download


def test_epoch_batches_shard_and_reshuffle():
    from vitpe import data as D
    n, batch, world = 103, 8, 3
    per_epoch = []
    for epoch in range(2):
        seen = []
        for rank in range(world):
            bs = list(D.epoch_batches(n, batch, epoch, seed=5, shuffle=True, rank=rank, world=world, device="cpu"))
            assert all(b.shape == (batch,) and b.dtype == torch.int64 for b in bs) and len(bs) == (n // world) // batch
            seen += [int(i) for b in bs for i in b]
        assert len(seen) == len(set(seen)) and max(seen) < n      # disjoint shards of one permutation
        per_epoch.append(seen)
    assert per_epoch[0] != per_epoch[1]                            # reshuffled every epoch
    again = [int(i) for b in D.epoch_batches(n, batch, 0, seed=5, rank=0, world=world, device="cpu") for i in b]
    assert again == per_epoch[0][:len(again)]                      # deterministic given (seed, epoch)
    order = [int(i) for b in D.epoch_batches(20, 5, 0, shuffle=False, device="cpu") for i in b]
    assert order == list(range(20))
    assert D.shard_slice(103, 2, 3) == (68, 102)


def test_oracle_input_transform_matches_its_definition():
    from oracle import vit_oracle as O
    x = torch.arange(0, 256, dtype=torch.uint8).repeat(3 * 4)[: 3 * 16 * 16].reshape(1, 3, 16, 16)
    mean, std = O.DATASET_STATS["cifar10"]
    y = O.normalize_u8(x, mean, std)
    assert y.dtype == torch.float32 and y.shape == x.shape
    for c in range(3):
        v = x[0, c].float() / 255.0
        assert torch.equal(y[0, c], (v - mean[c]) / std[c])
    from vitpe import data as D
    assert D.DATASET_STATS == O.DATASET_STATS                     # train.py:72,81 constants on both sides


def test_epoch_global_batches_keep_the_ragged_tail_on_every_rank():
    """reference DataLoader(batch_size, drop_last=False) (train.py:89-90): every sample once per epoch, last batch
    ragged (50000 % 128 = 80); all ranks make the same number of steps and the shares of a global batch are disjoint."""
    from vitpe import data as D
    n, G, world = 203, 32, 4
    steps = None
    seen, per_step_global = [], {}
    for rank in range(world):
        its = list(D.epoch_global_batches(n, G, 3, seed=7, shuffle=True, rank=rank, world=world, device="cpu"))
        steps = steps or len(its)
        assert len(its) == steps == (n + G - 1) // G
        for k, (idx, n_local, n_global) in enumerate(its):
            assert idx.dtype == torch.int64 and idx.numel() == max(n_local, 1) and 0 <= n_local <= G // world
            assert per_step_global.setdefault(k, n_global) == n_global
            seen += [int(i) for i in idx[:n_local]]
    assert sorted(seen) == list(range(n))                                  # each sample exactly once
    assert [per_step_global[k] for k in range(steps)] == [32] * 6 + [203 - 192]
    # the tail batch of 11 falls entirely into the shares of ranks 0 (8) and 1 (3); ranks 2, 3 run an empty share
    tails = [list(D.epoch_global_batches(n, G, 3, seed=7, rank=r, world=world, device="cpu"))[-1] for r in range(world)]
    assert [t[1] for t in tails] == [8, 3, 0, 0]
    order = [int(i) for idx, nl, _ in D.epoch_global_batches(10, 4, 0, shuffle=False, device="cpu") for i in idx[:nl]]
    assert order == list(range(10))
    with pytest.raises(ValueError):
        next(D.epoch_global_batches(10, 6, 0, world=4, device="cpu"))


def _run_bench(args, env_extra=None, launcher=False):
    import json
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(env_extra or {})
    bench = os.path.join(REPO, "bench.py")
    cmd = [sys.executable]
    if launcher:
        cmd += ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                "--master-port", str(29800 + os.getpid() % 150)]
    r = subprocess.run(cmd + [bench] + args, env=env, capture_output=True, text=True, timeout=300)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    return r.returncode, [json.loads(ln) for ln in lines], r.stderr


@pytest.mark.parametrize("launcher", [False, True])
def test_bench_starts_its_own_ranks_and_also_runs_under_the_launcher(launcher):
    """`python bench.py --gpus 2` (what the driver types) must start 2 ranks itself; under torch.distributed.run it is
    the rank it is told to be.  --dry-run: CPU ranks over gloo, no GPU (the JSON contract and the rendezvous only)."""
    rc, lines, err = _run_bench(["--gpus", "2", "--steps", "3", "--warmup", "1", "--dry-run"], launcher=launcher)
    assert rc == 0, err[-2000:]
    assert len(lines) == 1                                   # rank 0 prints ONE line
    ln = lines[0]
    assert ln["n_gpus"] == 2 and ln["n_ranks_seen"] == 2 and ln["steps"] == 3 and ln["warmup"] == 1
    assert ln["config"]["global_batch"] == 2 * ln["config"]["per_gpu_batch"] and ln["config"]["parallelism"] == "dp2"
    for key in ("metric", "value", "unit", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
                "comm_ms", "overlap_frac"):
        assert key in ln


def test_bench_eight_ranks_dry_run_and_rccl_channel_budget():
    """`python bench.py --gpus 8 --dry-run` (the driver's largest configuration, on CPU ranks over gloo): eight ranks
    rendezvous, the collective itself counts eight, rank 0 prints one line with the weak-scaling bookkeeping; a channel
    budget for RCCL (--rccl-channels) reaches the environment the communicator is created in and is reported."""
    rc, lines, err = _run_bench(["--gpus", "8", "--steps", "2", "--warmup", "1", "--dry-run", "--rccl-channels", "4"])
    assert rc == 0, err[-2000:]
    assert len(lines) == 1
    ln = lines[0]
    assert ln["n_gpus"] == 8 and ln["n_ranks_seen"] == 8 and ln["scaling"] == "weak"
    assert ln["config"]["parallelism"] == "dp8" and ln["config"]["global_batch"] == 8 * ln["config"]["per_gpu_batch"] == 4096
    assert ln["rccl_max_channels"] == 4 and "ddp_graph" in ln


def test_bench_refuses_a_world_size_that_contradicts_gpus():
    rc, lines, err = _run_bench(["--gpus", "2", "--dry-run"], env_extra={"WORLD_SIZE": "1", "RANK": "0"})
    assert rc != 0 and not lines


def test_bench_plain_run_is_lean_and_dumps_the_same_outputs_every_run(tmp_path):
    """A plain run prints the headline line only (no per-kernel probes, no CPU baseline: those are --full), --steps is
    the number of timed steps, and --dump-outputs writes the last step's arrays as float32 .npy, identical across runs
    with the same arguments (seeded inputs)."""
    dumps = []
    for run in ("a", "b"):
        out = tmp_path / run
        rc, lines, err = _run_bench(["--gpus", "1", "--steps", "4", "--warmup", "1", "--dry-run", "--dump-outputs", str(out)])
        assert rc == 0, err[-2000:]
        assert len(lines) == 1
        ln = lines[0]
        assert ln["steps"] == 4 and ln["warmup"] == 1 and ln["ms_per_step"] > 0
        assert not {"roofline", "other_kernels", "cpu_baseline"} & set(ln)
        files = sorted(os.listdir(out))
        assert files and all(f.endswith(".npy") for f in files)
        arrs = {f: np.load(out / f) for f in files}
        assert all(a.dtype == np.float32 for a in arrs.values()) and sum(a.nbytes for a in arrs.values()) <= 64 << 20
        dumps.append(arrs)
    assert dumps[0].keys() == dumps[1].keys()
    assert all(np.array_equal(dumps[0][k], dumps[1][k]) for k in dumps[0])
    rc, lines, err = _run_bench(["--gpus", "1", "--steps", "0", "--dry-run"])
    assert rc != 0 and not lines


def test_train_py_refuses_unsupported_geometries_up_front():
    """Every flag of the reference CLI is kept; combinations the attention kernels are not compiled for are refused by
    get_args() with the supported set, the others pass."""
    sys_path = os.path.join(REPO)
    import sys
    if sys_path not in sys.path:
        sys.path.insert(0, sys_path)
    import train as T
    for ok in ([], ["--patch_size", "8"], ["--embed_dim", "384"], ["--num_heads", "3"], ["--img_size", "64"],
               ["--img_size", "224", "--patch_size", "16", "--embed_dim", "768", "--depth", "12", "--num_heads", "12"]):
        T.get_args(ok)
    for bad in (["--num_heads", "12"], ["--img_size", "96"], ["--patch_size", "5"],
                ["--pos_encoding", "polynomial", "--poly_degree", "9"]):
        with pytest.raises(SystemExit):
            T.get_args(bad)


def test_hp_and_sched_slot_names_agree_in_header_kernels_and_python():
    """enum vitpe_hp_slot / vitpe_sched_slot of include/vitpe.h are the layout; csrc/common.h (HP_*, SCHED_*) and
    vitpe/_lib.py mirror them, and nothing else keeps the three copies equal."""
    from vitpe import _lib
    header = re.sub(r"/\*.*?\*/", " ", open(_lib.HEADER_PATH).read(), flags=re.S)
    common = open(os.path.join(_lib.PKG_ROOT, "csrc", "common.h")).read()
    for enum, prefix, count in (("vitpe_hp_slot", "HP_", 16), ("vitpe_sched_slot", "SCHED_", 8)):
        body = re.search(r"enum\s+" + enum + r"\s*\{(.*?)\}", header, flags=re.S).group(1)
        slots = {m.group(1): int(m.group(2)) for m in re.finditer(r"\bVITPE_(" + prefix + r"\w+)\s*=\s*(\d+)", body)}
        assert slots[prefix + "COUNT"] == count == len(slots) - 1
        assert sorted(v for k, v in slots.items() if k != prefix + "COUNT") == list(range(count))
        mirrored = {m.group(1): int(m.group(2)) for m in re.finditer(r"(?<![A-Z_])(" + prefix + r"\w+)\s*=\s*(\d+)", common)}
        assert mirrored == slots
        assert {k: getattr(_lib, k) for k in slots} == slots
