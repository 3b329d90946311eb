"""What a training step hands to the next one: the fp32 masters and moments (adamw_kernel), the bf16 flat copy, and every
packed / transposed weight copy (refresh_shadows_kernel), against the float64 / index-gather restatements of
tests/train_state_ref.py (checked on the CPU by tests/test_train_state_cpu.py).

Bounds (U = 2^-24, derived in train_state_ref.adamw_bounds from the roundings of adamw_kernel, not from its results):
|p - p_ref| <= 4U |p0| + 16U |delta_ref|, |m - m_ref| <= 4U |m_ref|, |v - v_ref| <= 6U |v_ref|; weight copies are bit-equal."""
import numpy as np
import pytest
import torch

import train_state_ref as R
from test_kernels_gpu import K, dev, rnd  # noqa: F401  (K: the kernels fixture)

pytestmark = pytest.mark.gpu

U = R.U


def bits(t):
    """integer view of a tensor's storage: equality of these is bit-equality (tells -0 from +0)"""
    t = t.detach().contiguous().cpu().reshape(-1)
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def worst(err, bound):
    """largest |err| / bound over the elements (0 / 0 = 0: an exact result under a zero bound passes)"""
    err, bound = np.abs(err), np.asarray(bound, dtype=np.float64)
    r = np.where(err == 0, 0.0, err / np.where(bound > 0, bound, 1e-300))
    return float(r.max())


# ------------------------------------------------------------------------------------------ 3. AdamW
def test_adamw_three_steps_at_the_precision_of_the_update(K):
    """n = 2 * 4096 * 256 + 7: every thread of the capped launch strides, with a ragged tail.  Each step is compared with
    adamw_ref started from the device's own fp32 state and its own bias corrections, so nothing accumulates; the gradient
    keeps its sign from step to step (g, 2g, 3g), so the moments do not cancel and the relative bounds on m and v hold.
    Roundings counted in train_state_ref.adamw_bounds: m 3 (bound 4U), v 5 (6U), p 3.0001 U |p0| + 14.5 U |delta|
    (4U |p0| + 16U |delta|) -- the issue's constants are the larger ones and are kept."""
    n = 2 * 4096 * 256 + 7
    p0_np, g_np = R.adamw_inputs(n)
    hp_np = R.adamw_hp()
    h = hp_np.astype(np.float64)
    p, hp = dev(torch.from_numpy(p0_np.copy())), dev(torch.from_numpy(hp_np.copy()))
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    shadow = torch.full((n,), -7.0, dtype=torch.bfloat16, device="cuda")
    zero_g = g_np == 0
    figures = []
    for step in range(1, 4):
        p_in, m_in, v_in = f64(p), f64(m), f64(v)
        g_step = (g_np * np.float32(step)).astype(np.float32)
        g = dev(torch.from_numpy(g_step.copy()))
        K.adamw_step(p, g, m, v, hp, shadow_bf16=shadow, zero_grad=True)
        torch.cuda.synchronize()
        hp_out = f64(hp)
        assert hp_out[5] == float(step)
        assert np.array_equal(hp_out[:5], h[:5]) and hp_out[8] == h[8]
        for slot, beta in ((6, h[1]), (7, h[2])):   # powf at <= 2 ulp of a value < 1, then an exact subtraction (b >= 0.5)
            assert abs(hp_out[slot] - (1.0 - beta ** step)) <= 4 * U, (step, slot)
        p_ref, m_ref, v_ref, d_ref = R.adamw_ref(p_in, g_step, m_in, v_in, hp_np, hp_out[6], hp_out[7])
        bp, bm, bv = R.adamw_bounds(p_in, p_ref, m_ref, v_ref, d_ref)
        p_out, m_out, v_out = f64(p), f64(m), f64(v)
        fig = (worst(p_out - p_ref, bp), worst(m_out - m_ref, bm), worst(v_out - v_ref, bv))
        figures.append(fig)
        print(f"adamw step {step}: worst |err| / bound  p {fig[0]:.3f}  m {fig[1]:.3f}  v {fig[2]:.3f}")
        assert fig[0] <= 1.0 and fig[1] <= 1.0 and fig[2] <= 1.0, (step, fig)
        # g == 0 on zero moments: nothing but the decay, exactly
        assert not m_out[zero_g].any() and not v_out[zero_g].any()
        decayed = (p_in[zero_g] * (1.0 - h[0] * h[4])).astype(np.float32)
        assert np.all(np.abs(p_out[zero_g] - decayed.astype(np.float64)) <= np.spacing(np.abs(decayed)).astype(np.float64))
        assert np.array_equal(p_out[zero_g & (p0_np == 0)], np.zeros(int((zero_g & (p0_np == 0)).sum())))
        assert float(g.abs().max()) == 0.0                                     # zero_grad = True
        assert torch.equal(bits(shadow), bits(p.to(torch.bfloat16)))           # the bf16 flat copy of THIS step's p
    assert np.isfinite(figures).all()


def test_adamw_flags_zero_grad_off_and_ticked(K):
    """zero_grad=False leaves g bit-unchanged; ticked=True takes hp[5..7] as given and does not advance them."""
    n = 10007
    p0_np, g_np = R.adamw_inputs(n, seed=9)
    hp_np = R.adamw_hp()
    # --- zero_grad = False
    p, g, hp = dev(torch.from_numpy(p0_np.copy())), dev(torch.from_numpy(g_np.copy())), dev(torch.from_numpy(hp_np.copy()))
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    K.adamw_step(p, g, m, v, hp, shadow_bf16=None, zero_grad=False)
    torch.cuda.synchronize()
    assert torch.equal(bits(g), bits(torch.from_numpy(g_np)))
    assert float(hp[5]) == 1.0
    p_ref, m_ref, v_ref, d_ref = R.adamw_ref(p0_np, g_np, 0 * p0_np, 0 * p0_np, hp_np, float(hp[6]), float(hp[7]))
    bp, bm, bv = R.adamw_bounds(p0_np, p_ref, m_ref, v_ref, d_ref)
    assert worst(f64(p) - p_ref, bp) <= 1 and worst(f64(m) - m_ref, bm) <= 1 and worst(f64(v) - v_ref, bv) <= 1
    # --- ticked: the caller's counter and corrections (values no tick would produce) are used and kept
    hp_t = hp_np.copy()
    hp_t[5], hp_t[6], hp_t[7] = 7.0, 0.5, 0.25
    p2, g2, hp2 = dev(torch.from_numpy(p0_np.copy())), dev(torch.from_numpy(g_np.copy())), dev(torch.from_numpy(hp_t.copy()))
    m2, v2 = torch.zeros_like(p2), torch.zeros_like(p2)
    sh2 = torch.full((n,), -7.0, dtype=torch.bfloat16, device="cuda")
    K.adamw_step(p2, g2, m2, v2, hp2, shadow_bf16=sh2, zero_grad=True, ticked=True)
    torch.cuda.synchronize()
    assert torch.equal(bits(hp2), bits(torch.from_numpy(hp_t)))
    assert float(g2.abs().max()) == 0.0
    p_ref, m_ref, v_ref, d_ref = R.adamw_ref(p0_np, g_np, 0 * p0_np, 0 * p0_np, hp_t, 0.5, 0.25)
    bp, bm, bv = R.adamw_bounds(p0_np, p_ref, m_ref, v_ref, d_ref)
    assert worst(f64(p2) - p_ref, bp) <= 1 and worst(f64(m2) - m_ref, bm) <= 1 and worst(f64(v2) - v_ref, bv) <= 1
    assert torch.equal(bits(sh2), bits(p2.to(torch.bfloat16)))
    # the corrections matter at this precision: the ticked result is far from the un-ticked one
    assert worst(f64(p2) - f64(p), bp) > 10


# ------------------------------------------------------------------------------------------ 4. refresh_shadows alone
SENTINEL = -7.0   # exact in bf16, outside the weights' range (|w| < 1, q scale 0.26)


def _standalone(K, kind, w, hd, dt):
    """the stand-alone entry point that defines shadow `kind` (None: it does not take this destination type)"""
    if kind == 0:
        return K.transpose_cast(w, dt)
    if kind == 1:
        return K.pack_qkv_weights(w, dt, w.shape[1] // hd)
    if kind == 6:
        return K.pack_qkv_weights_wide(w, dt, w.shape[1] // hd) if dt == torch.bfloat16 else None
    src = w if kind < 4 else w.t().contiguous()
    return K.pack_weight_frags(src, dt, hd, kind & 1)


@pytest.mark.parametrize("use_map", [True, False], ids=["tile_map", "scan"])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_refresh_shadows_on_a_hand_built_descriptor_list(K, dt, use_map):
    """One flat fp32 source (random everywhere, the gaps too), one sentinel-filled destination, the records of
    train_state_ref.SHADOW_CASES: every span bit-equal to shadow_ref cast with torch and to the stand-alone entry point on
    the same matrix, every element outside the spans still the sentinel.  Kind 6 is held to vitpe_pack_qkv_weights_wide
    first (bf16; the entry point has no fp32 form) and then to shadow_ref."""
    rec, tmap, n_src, n_dst, spans = R.shadow_layout()
    flat_cpu = rnd(n_src, seed=41)
    flat = dev(flat_cpu)
    dst = torch.full((n_dst,), SENTINEL, dtype=dt, device="cuda")
    desc = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
    tile_map = torch.from_numpy(tmap.copy()).cuda() if use_map else None
    K.refresh_shadows(flat, dst, desc, len(rec), int(tmap.size), tile_map)
    torch.cuda.synchronize()
    got = dst.cpu()
    expect = torch.full((n_dst,), SENTINEL, dtype=dt)
    differ = []
    for i, kind, hd, o, Rr, C in spans:
        s0 = int(rec["src"][i])
        w_cpu = flat_cpu[s0:s0 + Rr * C].view(Rr, C)
        ref = torch.from_numpy(R.shadow_ref(kind, w_cpu.numpy(), hd)).to(dt)
        expect[o:o + Rr * C] = ref
        span = got[o:o + Rr * C]
        alone = _standalone(K, kind, flat[s0:s0 + Rr * C].view(Rr, C).contiguous(), hd, dt)
        if alone is not None:   # first: the entry point that defines the layout
            n_alone = int((bits(span) != bits(alone)).sum())
            if kind == 6:
                print(f"kind 6 ({'bf16' if dt == torch.bfloat16 else 'f32'}): {n_alone} of {Rr * C} elements differ from "
                      f"vitpe_pack_qkv_weights_wide")
            if n_alone:
                differ.append((i, kind, "entry point", n_alone))
        n_ref = int((bits(span) != bits(ref)).sum())
        if kind == 6:
            print(f"kind 6 ({'bf16' if dt == torch.bfloat16 else 'f32'}): {n_ref} of {Rr * C} elements differ from shadow_ref")
        if n_ref:
            differ.append((i, kind, "shadow_ref", n_ref))
    assert not differ, differ
    assert torch.equal(bits(got), bits(expect))     # the spans again, and the sentinel everywhere else


# ------------------------------------------------------------------------------------------ 5. the engine's copies
def _records(eng):
    """the engine's own descriptor records, read back from the device"""
    return eng._desc.cpu().numpy().view(R.REC_DTYPE)


def _kind_of(eng, rec, w, view):
    """(kind, HD) of the shadow of w that `view` aliases, from the record array"""
    o = (view.data_ptr() - eng._shadow_flat.data_ptr()) // eng._shadow_flat.element_size()
    for r in rec[rec["src"] == eng._off[id(w)]]:
        if int(r["dst"]) == o:
            return int(r["kind"]), int(r["HD"])
        if int(r["kind2"]) >= 0 and int(r["dst2"]) == o:
            return int(r["kind2"]), int(r["HD2"])
    raise AssertionError("no record writes this view")


FAMILY = {"St": (0,), "Pk": (1,), "Pkw": (6,), "Fr": (2, 3), "Frt": (4, 5)}


def assert_copies_current(eng, when):
    """Every copy the engine holds of every block's qkv / proj / fc1 / fc2 weight is bit-equal to shadow_ref of the CURRENT
    fp32 master cast to the compute type; flat_s is the bf16 cast of flat_p.  Returns the set of kinds seen."""
    torch.cuda.synchronize()
    rec = _records(eng)
    n_shadows = int(len(rec) + (rec["kind2"] >= 0).sum())
    kinds, checked = set(), 0
    for bi, blk in enumerate(eng.model.blocks):
        for name, w in (("qkv", blk.attn.qkv.weight), ("proj", blk.attn.proj.weight), ("fc1", blk.mlp.fc1.weight),
                        ("fc2", blk.mlp.fc2.weight)):
            master = w.data.detach().cpu()
            assert torch.equal(bits(eng.Sh(w)), bits(master.to(eng.T))), (when, bi, name, "Sh")
            for acc, store in (("St", eng._st), ("Pk", eng._pk), ("Pkw", eng._pkw), ("Fr", eng._fr), ("Frt", eng._frt)):
                if id(w) not in store:
                    continue
                view = getattr(eng, acc)(w)
                kind, hd = _kind_of(eng, rec, w, view)
                assert kind in FAMILY[acc], (when, bi, name, acc, kind)
                ref = torch.from_numpy(R.shadow_ref(kind, master.numpy(), hd)).to(eng.T)
                n_bad = int((bits(view) != bits(ref)).sum())
                assert n_bad == 0, (when, bi, name, acc, kind, hd, n_bad)
                kinds.add(kind)
                checked += 1
    assert checked == n_shadows, (when, checked, n_shadows)    # no record's shadow was left out
    if eng.flat_s is not None:
        assert torch.equal(bits(eng.flat_s), bits(eng.flat_p.to(torch.bfloat16))), (when, "flat_s")
    else:
        assert eng.T == torch.float32
    return kinds


CIFAR = dict(img_size=32, patch_size=4, embed_dim=192, num_heads=6)
HD64 = dict(img_size=224, patch_size=16, embed_dim=128, num_heads=2)
ENGINES = {   # name: (environment, geometry, batch, compute dtype, use_graph, the record kinds it must hold)
    "default": ({}, CIFAR, 4, torch.bfloat16, True, {1, 4, 6, 2, 3, 5}),
    "default-eager": ({}, CIFAR, 4, torch.bfloat16, False, {1, 4, 6, 2, 3, 5}),
    "wide-off": ({"VITPE_ATTN_WIDE": "0"}, CIFAR, 4, torch.bfloat16, True, {1, 4, 2, 3, 5}),
    "tail2-off": ({"VITPE_TAIL2": "0"}, CIFAR, 4, torch.bfloat16, True, {1, 0, 6}),
    "fp32": ({}, CIFAR, 4, torch.float32, True, {1, 0}),
    "hd64-fused64": ({}, HD64, 2, torch.bfloat16, True, {0, 2}),
    "hd64-fused64-off": ({"VITPE_ATTN_FUSED64": "0"}, HD64, 2, torch.bfloat16, True, {0}),
}


@pytest.mark.parametrize("name", list(ENGINES))
def test_engine_copies_are_current_and_the_first_step_is_one_adamw_step(monkeypatch, name):
    """Depth 2, seeded weights (NOT rounded to bf16: the casts have something to do).  The copies are checked after
    construction, after each of two steps and after load_state_dict of perturbed weights (the post-hook, cast_flat=True).
    After the first step: flat_g is zero, the counter is 1, v = m^2 (1 - b2) / (1 - b1)^2 (the capture's warm-up steps were
    undone: three accumulated steps do not satisfy it), and flat_p is one adamw_ref step from the initial weights on the
    gradient m / (1 - b1), within the AdamW test's bound."""
    from models.vit import VisionTransformer
    from vitpe.engine import TrainEngine
    env, geom, B, dt, use_graph, want_kinds = ENGINES[name]
    for k in ("VITPE_ATTN_WIDE", "VITPE_TAIL2", "VITPE_ATTN_FUSED64", "VITPE_LNBWD2", "VITPE_FUSE_LN"):
        monkeypatch.delenv(k, raising=False)
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    torch.manual_seed(0)
    model = VisionTransformer(pos_encoding="rope-axial", depth=2, **geom).cuda()
    eng = TrainEngine(model, B, compute_dtype=dt, use_graph=use_graph)
    if "VITPE_ATTN_WIDE" not in env and dt == torch.bfloat16 and geom is CIFAR:
        assert eng.attn_wide
    if geom is HD64:
        assert eng.attn_fused64 == ("VITPE_ATTN_FUSED64" not in env) and not eng.attn_fused
    assert assert_copies_current(eng, "construction") == want_kinds
    rec = _records(eng)
    if name == "tail2-off":    # the qkv record is kind 1 with the transposed copy as its second shadow
        qrec = rec[rec["src"] == eng._off[id(model.blocks[0].attn.qkv.weight)]]
        assert {(int(r["kind"]), int(r["kind2"])) for r in qrec} == {(1, 0), (6, -1)}
    if name == "hd64-fused64":  # the ViT-B pair: transposed copy + fragment pack at chunk 64
        qrec = rec[rec["src"] == eng._off[id(model.blocks[0].attn.qkv.weight)]]
        assert [(int(r["kind"]), int(r["kind2"]), int(r["HD2"])) for r in qrec] == [(0, 2, 64)]

    gen = torch.Generator().manual_seed(11)
    S = geom["img_size"]
    images, labels = torch.randn(B, 3, S, S, generator=gen).cuda(), torch.randint(0, 10, (B,), generator=gen).cuda()
    p0 = f64(eng.flat_p)
    hp0 = eng.hp.detach().cpu().numpy().copy()
    assert hp0[5] == 0 and not eng.flat_m.any() and not eng.flat_v.any()

    eng.step(images, labels)
    assert_copies_current(eng, "step 1")
    hp1 = f64(eng.hp)
    h = hp0.astype(np.float64)
    assert hp1[5] == 1.0 and np.array_equal(hp1[:5], h[:5]) and hp1[8] == 1.0
    assert abs(hp1[6] - (1 - h[1])) <= 4 * U and abs(hp1[7] - (1 - h[2])) <= 4 * U
    assert float(eng.flat_g.abs().max()) == 0.0
    m1, v1, p1 = f64(eng.flat_m), f64(eng.flat_v), f64(eng.flat_p)
    assert np.isfinite(m1).all() and np.isfinite(v1).all() and np.isfinite(p1).all()
    # v against m: m = (1 - b1) g (1 rounding), v = (1 - b2) g g (2): 2 * 1 + 2 = 4U <= 8U, where (1 - b2) g g is a normal
    # fp32 number (below 2^-126 the result has fewer than 24 bits and no relative bound can hold)
    v_exp = m1 * m1 * (1 - h[2]) / (1 - h[1]) ** 2
    live = m1 != 0
    normal = live & (v_exp >= 2.0 ** -120)
    assert live.sum() > 0.5 * eng.n_flat and normal.sum() >= 0.99 * live.sum(), (live.sum(), normal.sum())
    fig_v = float((np.abs(v1 - v_exp)[normal] / v_exp[normal]).max() / (8 * U))
    assert not v1[~live].any()
    # p: one reference step from the initial weights on g = m / (1 - b1)
    p_ref, m_ref, v_ref, d_ref = R.adamw_ref(p0, m1 / (1 - h[1]), 0 * p0, 0 * p0, hp0, hp1[6], hp1[7])
    bp, _, _ = R.adamw_bounds(p0, p_ref, m_ref, v_ref, d_ref)
    fig_p = worst(p1 - p_ref, bp)
    print(f"{name}: after step 1  |v - v(m)| / (8U v) = {fig_v:.3f}   |p - p_ref| / bound = {fig_p:.3f}")
    assert fig_v <= 1.0 and fig_p <= 1.0, (fig_v, fig_p)
    assert np.abs(p1 - p0).max() > 0.5 * h[0]          # the weights did move by about lr

    eng.step(images, labels)
    assert_copies_current(eng, "step 2")
    assert float(eng.hp[5]) == 2.0 and float(eng.flat_g.abs().max()) == 0.0
    assert np.abs(f64(eng.flat_p) - p1).max() > 0

    gen2 = torch.Generator().manual_seed(12)
    sd = {k: (t.detach().cpu() + 0.01 * torch.randn(t.shape, generator=gen2) if t.is_floating_point() else t.detach().cpu())
          for k, t in model.state_dict().items()}
    before = eng.flat_p.clone()
    model.load_state_dict(sd)
    assert not torch.equal(before, eng.flat_p)           # the load went into the flat master
    assert_copies_current(eng, "load_state_dict")
