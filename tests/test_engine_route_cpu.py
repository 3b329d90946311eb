"""The engine's route and its shadow plan are host logic over the library's *_supported entry points: checked here without
a GPU.  The route flags of every configuration of tests/engine_trace.py must reproduce what the engine before the
reorganisation resolved (tests/golden/engine_trace.json), the implications between the flags must hold over the whole
switch space, and the shadow plan must lay out what tests/test_train_state_gpu.py finds on the device."""
import dataclasses
import itertools
import json

import numpy as np
import pytest
import torch

import engine_trace as E
import train_state_ref as R
from test_train_state_gpu import CIFAR, ENGINES, HD64
from vitpe import route as RT

VITB = dict(img_size=224, patch_size=16, embed_dim=768, num_heads=12)


def _args(geom, dtype, depth, classes=10):
    return dict(dtype=dtype, C=3, S=geom["img_size"], patch=geom["patch_size"], D=geom["embed_dim"], H=geom["num_heads"],
                hid=4 * geom["embed_dim"], depth=depth, classes=classes)


@pytest.mark.parametrize("name", list(E.CONFIGS))
def test_route_flags_are_the_ones_the_engine_resolved_before(name):
    with open(E.GOLDEN_PATH) as f:
        want = json.load(f)["configs"][name]["route"]
    cfg = E.CONFIGS[name]
    got = dataclasses.asdict(RT.resolve_route(env=cfg["env"], **E.route_args(cfg)))
    assert set(got) == set(E.ROUTE_FLAGS) and got == want


def test_resolve_route_reads_the_process_environment_by_default(monkeypatch):
    for k in E.ROUTE_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    a = _args(CIFAR, torch.bfloat16, 2)
    assert RT.resolve_route(**a).tail2
    monkeypatch.setenv("VITPE_TAIL2", "0")
    assert not RT.resolve_route(**a).tail2


def test_no_attention_kernel_is_an_error_of_the_route():
    from vitpe._lib import VitpeError
    with pytest.raises(VitpeError, match="no attention kernel for N="):
        RT.resolve_route(**_args(dict(img_size=320, patch_size=4, embed_dim=192, num_heads=6), torch.bfloat16, 2), env={})


SWITCH_VALUES = {s: (None, "1" if s == "VITPE_RECOMPUTE_LN" else "0") for s in E.ROUTE_SWITCHES}
SWITCH_VALUES["VITPE_FUSE_LN"] = (None, "fwd", "all", "off")


@pytest.mark.parametrize("geom,classes", [(CIFAR, 10), (HD64, 10), (VITB, 1000)], ids=["cifar", "hd64", "vit-b16"])
def test_implications_hold_over_the_whole_switch_space(geom, classes):
    """Every combination of the eleven switches x {bf16, fp32} x extras x fuse_ln x depth {1, 2} (VITPE_FUSE_LN stands in
    for fuse_ln=None only, so it is not varied under the other three values: the route would not see it)."""
    seen = set()
    for values in itertools.product(*SWITCH_VALUES.values()):
        env = {k: v for k, v in zip(SWITCH_VALUES, values) if v is not None}
        for dtype, extras, fuse_ln, depth in itertools.product((torch.bfloat16, torch.float32), (False, True),
                                                               (None, True, "fwd", False), (1, 2)):
            if fuse_ln is not None and "VITPE_FUSE_LN" in env:
                continue
            r = RT.resolve_route(**_args(geom, dtype, depth, classes), extras=extras, fuse_ln=fuse_ln, env=env)
            seen.add(r)
            ctx = (env, dtype, extras, fuse_ln, depth, r)
            assert r.extras == extras
            assert not r.tail2 or (r.attn_fused and r.fuse_ln and r.fuse_ln_bwd), ctx
            assert not r.lnbwd2 or r.tail2, ctx
            assert not r.fuse_lnbwd or r.lnbwd2, ctx
            assert not r.recompute_ln or (r.tail2 and r.group_wgrad), ctx
            assert not r.cls_rows or (r.tail2 and r.group_wgrad and r.fuse_head and dtype == torch.bfloat16
                                      and depth >= 2), ctx
            assert not r.attn_wide or r.attn_fused, ctx
            assert not r.attn_fused64 or not r.attn_fused, ctx
            assert not (r.fuse_ln or r.fuse_ln_bwd) or r.attn_fused, ctx
            assert not r.extras or not (r.attn_fused or r.attn_wide or r.attn_fused64 or r.fuse_ln or r.fuse_ln_bwd
                                        or r.tail2 or r.lnbwd2 or r.fuse_lnbwd or r.recompute_ln or r.cls_rows), ctx
    assert len(seen) > 1   # the switches do reach different routes at this geometry


# ------------------------------------------------------------------------------------------ the shadow plan
def _plan(name, depth=2):
    env, geom, _, dt, _, want_kinds = ENGINES[name]
    route = RT.resolve_route(**_args(geom, dt, depth), env=env)
    D = geom["embed_dim"]
    shapes = [[(3 * D, D), (D, D), (4 * D, D), (D, 4 * D)]] * depth
    offsets, off = [], 1000   # (the engine's offsets are ALIGN-aligned and increasing; what lies between does not matter)
    for blk in shapes:
        offsets.append([])
        for rows, cols in blk:
            offsets[-1].append(off)
            off += rows * cols + 2 * RT.ALIGN
    return route, shapes, offsets, RT.shadow_plan(route, shapes, offsets, D // geom["num_heads"]), want_kinds


def test_kind_constants_are_the_headers_numbers():
    assert (RT.KIND_T, RT.KIND_QKV, RT.KIND_FRAG, RT.KIND_FRAG_PHI, RT.KIND_FRAG_T, RT.KIND_FRAG_T_PHI,
            RT.KIND_QKV_WIDE) == (0, 1, 2, 3, 4, 5, 6)
    assert RT.REC_DTYPE == R.REC_DTYPE


@pytest.mark.parametrize("name", list(ENGINES))
def test_shadow_plan(name):
    route, shapes, offsets, (rec, spans, tmap, total), want_kinds = _plan(name)
    assert rec.dtype == R.REC_DTYPE
    kinds = set(rec["kind"].tolist()) | {k for k in rec["kind2"].tolist() if k >= 0}
    assert kinds == want_kinds == {k for _, k, _ in spans}
    qrec = rec[rec["src"] == offsets[0][0]]
    if name == "tail2-off":
        assert {(int(r["kind"]), int(r["kind2"])) for r in qrec} == {(1, 0), (6, -1)}
    if name == "hd64-fused64":
        assert [(int(r["kind"]), int(r["kind2"]), int(r["HD2"])) for r in qrec] == [(0, 2, 64)]
    # every span belongs to the record of its weight, is ALIGN-aligned, and no two overlap; the buffer ends with the last
    flat_shapes = [s for blk in shapes for s in blk]
    flat_offsets = [o for blk in offsets for o in blk]
    assert len(spans) == len(rec) + int((rec["kind2"] >= 0).sum())
    taken = np.zeros(total, dtype=np.int32)
    for w, kind, o in spans:
        rows, cols = flat_shapes[w]
        assert o % RT.ALIGN == 0 and o + rows * cols <= total
        taken[o:o + rows * cols] += 1
        mine = rec[rec["src"] == flat_offsets[w]]
        assert any((int(r["kind"]), int(r["dst"])) == (kind, o) or (int(r["kind2"]), int(r["dst2"])) == (kind, o) for r in mine)
        assert all((int(r["R"]), int(r["C"])) == (rows, cols) for r in mine)
    assert taken.max() == 1
    assert total % RT.ALIGN == 0 and total - max(o + flat_shapes[w][0] * flat_shapes[w][1] for w, _, o in spans) < RT.ALIGN
    # tile0 is the running sum of the records' 32x32 source tiles, and the map sends every tile to its record
    tiles = ((rec["R"] + 31) // 32) * ((rec["C"] + 31) // 32)
    assert np.array_equal(rec["tile0"], np.concatenate([[0], np.cumsum(tiles)[:-1]]))
    assert tmap.dtype == np.int16 and np.array_equal(tmap, np.repeat(np.arange(len(rec)), tiles))
    assert not rec["pad"].any()
