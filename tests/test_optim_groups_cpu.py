"""AdamW parameter groups and the per-step LR schedule -- what can be checked without a GPU: the float64 references of
tests/optim_groups_ref.py against torch.optim.AdamW with param groups and torch's SequentialLR(LinearLR,
CosineAnnealingLR), that the kernel test's inputs tell a kernel that ignores its map from one that reads it,
vit_param_groups / torch_param_groups on CPU models, the granule map, the C symbols and their host-side refusals, the
host-only argument handling of TrainEngine.set_param_groups / set_lr_schedule / set_lr, and train.py's flags."""
import ctypes
import math
import sys

import numpy as np
import pytest
import torch

import optim_groups_ref as R
from optim_host import cpu_optimizer
import train_state_ref as TS
from vitpe import _lib

PE_MODES = ["none", "absolute", "relative", "polynomial", "rope-axial", "rope-mixed"]


# ------------------------------------------------------------------------------------------ the references
def test_grouped_reference_is_torch_adamw_with_param_groups():
    n = 41 * 8 * 3 + 5
    p0, g = TS.adamw_inputs(n, seed=3)
    gid = R.span_map(n)
    eg = R.element_groups(gid, n)
    hp = TS.adamw_hp()
    w = lambda x: float(np.float32(x))   # noqa: E731  (the fp32 number, widened: what the reference reads)
    params, tgroups = [], []
    for k, (ls, ws) in enumerate(R.GROUPS4):
        idx = np.nonzero(eg == k)[0]
        prm = torch.nn.Parameter(torch.from_numpy(p0[idx].astype(np.float64)))
        prm.grad = torch.from_numpy(g[idx].astype(np.float64) * w(hp[8]))
        ghp = R.group_hp(hp, ls, ws)
        params.append((idx, prm))
        tgroups.append({"params": [prm], "lr": w(ghp[0]), "weight_decay": w(ghp[4])})
    opt = torch.optim.AdamW(tgroups, betas=(w(hp[1]), w(hp[2])), eps=w(hp[3]))
    p, m, v = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    for step in (1, 2, 3):
        bc1, bc2 = R.bias_corrections(hp, step)
        before = p
        p, m, v, delta = R.grouped_adamw_ref(p, g, m, v, hp, bc1, bc2, gid, R.GROUPS4)
        opt.step()
        for idx, prm in params:
            st = opt.state[prm]
            tp, tm, tv = prm.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()
            assert np.all(np.abs(tm - m[idx]) <= 1e-12 * np.abs(m[idx]))
            assert np.all(np.abs(tv - v[idx]) <= 1e-12 * np.abs(v[idx]))
            assert np.all(np.abs(tp - p[idx]) <= 1e-12 * (np.abs(before[idx]) + np.abs(delta[idx])))
    assert not np.array_equal(p, p0.astype(np.float64))


@pytest.mark.parametrize("case", R.SCHED_CASES)
def test_schedule_reference_is_torch_sequential_lr(case):
    base, lo, W, T, s0 = case
    prm = torch.nn.Parameter(torch.zeros(1, dtype=torch.float64))
    opt = torch.optim.SGD([prm], lr=base)
    from torch.optim.lr_scheduler import CosineAnnealingLR, LinearLR, SequentialLR
    cos = CosineAnnealingLR(opt, T_max=T - W, eta_min=lo)
    sched = SequentialLR(opt, [LinearLR(opt, start_factor=s0, total_iters=W), cos], milestones=[W]) if W > 0 else cos
    worst = 0.0
    for k in range(T + 1):
        worst = max(worst, abs(opt.param_groups[0]["lr"] - R.schedule_ref(k, base, lo, W, T, s0)))
        opt.step()
        sched.step()
    print(f"{case}: worst |closed form - torch| over k = 0..{T}: {worst:.3e} ({worst / base:.1e} of base)")
    assert worst <= 1e-12 * base
    # the ends: the start factor, the base rate at the end of the warm-up, min_lr from T on
    assert R.schedule_ref(0, base, lo, W, T, s0) == (base * s0 if W > 0 else base)
    assert R.schedule_ref(W, base, lo, W, T, s0) == base
    assert R.schedule_ref(T, base, lo, W, T, s0) == lo == R.schedule_ref(T + 5, base, lo, W, T, s0)
    assert all(k <= T + 5 for k in R.sched_ks(W, T)) and T in R.sched_ks(W, T)


@pytest.mark.parametrize("n", [n for n in R.SIZES if n >= 2048])
def test_inputs_tell_a_kernel_that_ignores_its_map(n):
    """In every group other than (1, 1) the ungrouped update misses the grouped one by more than adamw_bounds allows
    (worst element of the group: elements with p0 == 0 lose nothing to the decay and the g == 0 ones nothing to the
    step, so not every single element can differ).  m and v do not depend on lr or wd: they agree exactly."""
    p0, g = TS.adamw_inputs(n, seed=n % 1000)
    gid = R.span_map(n)
    eg = R.element_groups(gid, n)
    hp = TS.adamw_hp()
    bc1, bc2 = R.bias_corrections(hp, 1)
    z = np.zeros(n)
    grouped = R.grouped_adamw_ref(p0, g, z, z, hp, bc1, bc2, gid, R.GROUPS4)
    plain = TS.adamw_ref(p0, g, z, z, hp, bc1, bc2)
    bp, _, _ = TS.adamw_bounds(p0, *grouped)
    ratio = np.abs(plain[0] - grouped[0]) / np.where(bp > 0, bp, 1e-300)
    assert np.array_equal(plain[1], grouped[1]) and np.array_equal(plain[2], grouped[2])
    assert set(np.unique(eg)) == {0, 1, 2, 3}
    assert np.array_equal(plain[0][eg == 0], grouped[0][eg == 0])
    for k in (1, 2, 3):
        sel = ratio[eg == k]
        print(f"n {n} group {k} {R.GROUPS4[k]}: ungrouped misses by up to {sel.max():.3g} bounds, "
              f"{(sel > 1).mean():.0%} of its elements by more than one")
        assert sel.max() > 100 and (sel > 1).mean() > 0.5
    # one wavefront (64 granules) of the map holds all four groups, wherever it starts
    for start in range(0, min(gid.size - 64, 200)):
        assert set(gid[start:start + 64]) == {0, 1, 2, 3}


def test_blocks_rule_and_maps():
    assert [R.blocks(n) for n in (0, -3, 1, 8, 9, 2048, 2049, R.SWEEP, R.SWEEP - 2048, R.SWEEP + 4099)] == \
        [0, 0, 1, 1, 1, 1, 2, 2048, 2047, 2048]
    numels, group_of = [5, 16, 1, 24, 9], [3, 0, 2, 1, 2]
    offs, n_flat, gid = R.layout_map(numels, group_of)
    assert offs == [0, 8, 24, 32, 56] and n_flat == 72 and gid.dtype == np.uint8
    assert gid.tolist() == [3, 0, 0, 2, 1, 1, 1, 2, 2]
    eg = R.element_groups(gid, n_flat)
    for o, k, grp in zip(offs, numels, group_of):
        assert np.all(eg[o:o + k] == grp)
    # the engine's builder agrees, and the padding behind the last parameter keeps group 0
    from vitpe.optim import param_granule_map
    got = param_granule_map([(o, k, grp) for o, k, grp in zip(offs, numels, group_of)], n_flat + 16)
    assert got.dtype == np.uint8 and got.tolist() == gid.tolist() + [0, 0]


# ------------------------------------------------------------------------------------------ vit_param_groups
def _cpu_model(mode, qkv_bias=False, depth=3):
    from models.vit import VisionTransformer
    return VisionTransformer(img_size=16, patch_size=4, embed_dim=64, depth=depth, num_heads=2, pos_encoding=mode,
                             qkv_bias=qkv_bias)


def _expected_no_decay(model):
    names = {"cls_token", "patch_embed.bias", "norm.weight", "norm.bias", "head.bias"}
    for i in range(len(model.blocks)):
        names |= {f"blocks.{i}.{x}" for x in ("norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias", "attn.proj.bias",
                                              "mlp.fc1.bias", "mlp.fc2.bias")}
        if model.blocks[i].attn.qkv.bias is not None:
            names.add(f"blocks.{i}.attn.qkv.bias")
    names |= {n for n, _ in model.named_parameters() if n.startswith("pos_embed.")}
    return names


@pytest.mark.parametrize("qkv_bias", [False, True])
@pytest.mark.parametrize("mode", PE_MODES)
def test_vit_param_groups_follow_the_recipe(mode, qkv_bias):
    from vitpe.optim import torch_param_groups, vit_layer_id, vit_param_groups
    model = _cpu_model(mode, qkv_bias)
    named = dict(model.named_parameters())
    depth = len(model.blocks)
    pos = {"none": [], "absolute": ["pos_embed.pos_embed"], "relative": ["pos_embed.relative_position_bias_table"],
           "polynomial": ["pos_embed.coefficients"], "rope-axial": [], "rope-mixed": ["pos_embed.freqs"]}[mode]
    assert sorted(n for n in named if n.startswith("pos_embed.")) == pos
    assert ("blocks.0.attn.qkv.bias" in named) == qkv_bias
    # no_decay alone: two groups, the exact set of names
    groups = vit_param_groups(model, no_decay=True)
    assert all(g["lr_scale"] == 1.0 and g["layer_id"] is None for g in groups) and len(groups) == 2
    skipped = {n for g in groups if g["weight_decay_scale"] == 0.0 for n in g["names"]}
    assert skipped == _expected_no_decay(model)
    assert {g["weight_decay_scale"] for g in groups} == {0.0, 1.0}
    # nothing switched on: one (1, 1) group of everything
    plain = vit_param_groups(model, no_decay=False)
    assert len(plain) == 1 and plain[0]["lr_scale"] == plain[0]["weight_decay_scale"] == 1.0
    assert plain[0]["names"] == list(named)
    # layer decay: the layer ids and d ** (L + 1 - id)
    d = 0.75
    both = vit_param_groups(model, no_decay=True, layer_decay=d)
    for g in both:
        for name, prm in zip(g["names"], g["params"]):
            assert prm is named[name]
            lid = vit_layer_id(name, depth)
            want = (int(name.split(".")[1]) + 1 if name.startswith("blocks.")
                    else depth + 1 if name.split(".")[0] in ("norm", "head") else 0)
            assert lid == want == g["layer_id"], name
            assert g["lr_scale"] == d ** (depth + 1 - lid)
            assert g["weight_decay_scale"] == (0.0 if name in skipped else 1.0)
    assert {g["layer_id"] for g in both} == set(range(depth + 2))
    assert max(g["lr_scale"] for g in both) == 1.0 and min(g["lr_scale"] for g in both) == d ** (depth + 1)
    for gs in (groups, plain, both, vit_param_groups(model, no_decay=False, layer_decay=d)):
        ids = [id(p) for g in gs for p in g["params"]]
        assert len(ids) == len(set(ids)) == len(named)           # every parameter in exactly one group
        # torch_param_groups round-trips: AdamW takes it, and dividing by lr / wd gives the scales back
        tg = torch_param_groups(gs, 1e-3, 0.05)
        opt = torch.optim.AdamW(tg, lr=123.0, weight_decay=456.0)
        assert len(opt.param_groups) == len(gs)
        for og, g in zip(opt.param_groups, gs):
            assert [id(p) for p in og["params"]] == [id(p) for p in g["params"]]
            assert og["lr"] == 1e-3 * g["lr_scale"] and og["weight_decay"] == 0.05 * g["weight_decay_scale"]
            assert math.isclose(og["lr"] / 1e-3, g["lr_scale"], rel_tol=1e-15)
    with pytest.raises(_lib.VitpeError, match="layer_decay"):
        vit_param_groups(model, layer_decay=0.0)
    with pytest.raises(_lib.VitpeError, match="layer_decay"):
        vit_param_groups(model, layer_decay=float("nan"))


def test_map_of_a_model_layout_carries_every_parameters_group():
    from vitpe import ddp
    from vitpe.optim import param_granule_map, vit_param_groups
    from vitpe.route import ALIGN
    assert ALIGN == R.GRANULE
    model = _cpu_model("rope-mixed", qkv_bias=True, depth=2)
    params = list(model.parameters())
    starts, n_flat = ddp.flat_layout([p.numel() for p in params], ALIGN)
    off = {id(p): o for p, o in zip(params, starts)}
    groups = vit_param_groups(model, True, 0.75)
    spans = [(off[id(p)], p.numel(), k) for k, g in enumerate(groups, start=1) for p in g["params"]]
    gid = param_granule_map(spans, n_flat)
    assert gid.shape == (n_flat // ALIGN,)
    covered = np.zeros(gid.size, dtype=bool)
    for o, numel, k in spans:
        lo, hi = o // ALIGN, (o + numel + ALIGN - 1) // ALIGN
        assert np.all(gid[lo:hi] == k) and not covered[lo:hi].any()
        covered[lo:hi] = True
    assert covered.all()            # (every granule starts a parameter or continues one: the padding is inside them)
    assert any(p.numel() % ALIGN for p in params)


# ------------------------------------------------------------------------------------------ the C boundary
def test_new_symbols_in_header_and_library():
    protos = _lib.parse_header()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("vitpe_adamw_step_groups", 13), ("vitpe_adamw_groups_blocks", 1), ("vitpe_lr_schedule", 4)):
        assert name in protos and len(protos[name]) == nargs
        assert hasattr(handle, name)
    sig = protos["vitpe_adamw_step_groups"]
    assert sig[6] is ctypes.c_longlong and sig[7] is ctypes.c_int and sig[9] is ctypes.c_longlong and sig[11] is ctypes.c_int
    h = _lib.lib()
    for n in (0, -5, 1, 7, 8, 9, 2048, 2049, 2048 + 5, R.SWEEP, R.SWEEP - 2048, R.SWEEP - 2047, R.SWEEP + 4099, 2 ** 33):
        assert h.vitpe_adamw_groups_blocks(n) == R.blocks(n), n
    # pure host argument checks: refused before anything touches a device (the non-null values are never dereferenced)
    f = 4096
    call = h.vitpe_adamw_step_groups
    ok = dict(p=f, g=f, m=f, v=f, sh=None, hp=f, n=16, zg=1, gid=f, n_gid=2, gtab=f, ng=4)

    def refused(**over):
        a = dict(ok, **over)
        return call(a["p"], a["g"], a["m"], a["v"], a["sh"], a["hp"], a["n"], a["zg"], a["gid"], a["n_gid"], a["gtab"], a["ng"],
                    None) == 1

    for name in ("p", "g", "m", "v", "hp", "gid", "gtab"):
        assert refused(**{name: None}), name
    assert refused(n=-1) and refused(ng=0) and refused(ng=257) and refused(ng=-1)
    assert refused(n_gid=1) and refused(n=17, n_gid=2)            # ceil(17 / 8) = 3 granules
    for name in ("p", "g", "m", "v"):
        assert refused(**{name: f + 4}) and refused(**{name: f + 8}), name
    assert refused(sh=f + 4) and refused(sh=f + 2)
    assert refused(hp=None, n=0)
    assert h.vitpe_lr_schedule(None, f, 0, None) == 1 and h.vitpe_lr_schedule(f, None, 1, None) == 1


# ------------------------------------------------------------------------------------------ TrainEngine, host side
def test_set_param_groups_argument_handling_without_a_device():
    from vitpe.optim import group_scales
    w, b = torch.nn.Parameter(torch.zeros(4, 4)), torch.nn.Parameter(torch.zeros(4))
    eng, dropped = cpu_optimizer({id(w): 0})                          # the model's parameters, as _build_flat records them
    assert eng.param_groups is None and eng._gid is None and eng._gtab is None
    eng.set_param_groups(None)
    eng.set_param_groups([])
    assert eng.param_groups is None and dropped == []                  # off -> off: nothing dropped, no device needed
    for key in ("lr_scale", "weight_decay_scale"):
        for bad in (-0.1, float("nan"), float("inf"), -1e-9, "x", None):
            with pytest.raises(_lib.VitpeError, match="set_param_groups: " + key):
                eng.set_param_groups([{"params": [w], key: bad}])
    with pytest.raises(_lib.VitpeError, match="listed twice"):
        eng.set_param_groups([{"params": [w, b]}, {"params": [w], "lr_scale": 0.5}])
    with pytest.raises(_lib.VitpeError, match="listed twice"):
        eng.set_param_groups([{"params": [b, b]}])
    with pytest.raises(_lib.VitpeError, match="'params'"):
        eng.set_param_groups([{"lr_scale": 1.0}])
    with pytest.raises(_lib.VitpeError, match="'params'"):
        eng.set_param_groups([[w]])
    with pytest.raises(_lib.VitpeError, match="at most 255"):
        eng.set_param_groups([{"params": []} for _ in range(256)])
    with pytest.raises(_lib.VitpeError, match="not one of the model's"):
        eng.set_param_groups([{"params": [w]}, {"params": [b], "weight_decay_scale": 0.0}])
    assert eng.param_groups is None and dropped == []
    assert group_scales([{"params": [w], "lr_scale": np.float32(0.5)}, {"params": (b,), "weight_decay_scale": 0}]) == \
        [([w], 0.5, 1.0), ([b], 1.0, 0.0)]


def test_set_lr_schedule_argument_handling_without_a_device():
    from vitpe.optim import sched_values
    eng, dropped = cpu_optimizer()
    assert eng.lr_sched is None and eng._sched is None
    eng.set_lr_schedule(None)
    assert eng.lr_sched is None and dropped == []
    good = dict(base_lr=1e-3, total_steps=40, warmup_steps=5, min_lr=0.0, warmup_factor=0.01, done=0)
    bad = [dict(total_steps=5), dict(total_steps=4), dict(total_steps=0), dict(warmup_steps=-1), dict(warmup_factor=0.0),
           dict(warmup_factor=1.5), dict(warmup_factor=float("nan")), dict(min_lr=-1e-9), dict(min_lr=2e-3),
           dict(base_lr=float("inf")), dict(base_lr=float("nan")), dict(base_lr=-1.0), dict(done=-1), dict(total_steps=40.5),
           dict(warmup_steps=2.5), dict(total_steps=2 ** 24), dict(base_lr="x"), dict(total_steps=None)]
    for over in bad:
        with pytest.raises(_lib.VitpeError, match="set_lr_schedule"):
            eng.set_lr_schedule(**dict(good, **over))
    assert eng.lr_sched is None and eng._sched is None and dropped == []
    assert sched_values(**good) == (1e-3, 0.0, 5, 40, 0.01, 0)
    assert sched_values(3e-4, 17, 0, 1e-5, 1.0, 3) == (3e-4, 1e-5, 0, 17, 1.0, 3)
    assert sched_values(None, 0, 0, 0.0, 1e-3, 0) is None


def test_set_lr_refuses_under_a_schedule():
    eng, _ = cpu_optimizer()
    eng.lr_sched = (1e-3, 0.0, 5, 40, 0.01, 0)           # as after set_lr_schedule(1e-3, 40, 5)
    with pytest.raises(_lib.VitpeError, match="set_lr: a per-step schedule is on"):
        eng.set_lr(1e-4)


def test_train_py_optimizer_flags():
    sys.path.insert(0, _lib.REPO_ROOT)
    import train
    args = train.get_args([])
    assert args.no_decay_norm_bias is False and args.layer_decay == 0.0 and args.warmup_epochs == 0.0
    assert args.min_lr == 0.0 and args.lr_per_step is False
    args = train.get_args(["--no_decay_norm_bias", "--layer_decay", "0.75", "--warmup_epochs", "0.34", "--min_lr", "1e-5",
                           "--epochs", "1"])
    assert args.no_decay_norm_bias and args.layer_decay == 0.75 and args.warmup_epochs == 0.34 and args.min_lr == 1e-5
    assert train.get_args(["--lr_per_step", "--min_lr", "1e-4"]).lr_per_step is True
    for bad in (["--layer_decay", "-0.5"], ["--layer_decay", "1.5"], ["--layer_decay", "nan"], ["--warmup_epochs", "-1"],
                ["--warmup_epochs", "nan"], ["--warmup_epochs", "25"], ["--epochs", "2", "--warmup_epochs", "2"],
                ["--lr_per_step", "--min_lr", "-1e-5"], ["--lr_per_step", "--min_lr", "0.01"], ["--lr_per_step", "--min_lr", "nan"],
                ["--min_lr", "1e-5"]):
        with pytest.raises(SystemExit):
            train.get_args(bad)
