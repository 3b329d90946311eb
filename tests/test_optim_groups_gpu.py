"""AdamW with parameter groups and the per-step LR schedule inside the train step: vitpe_adamw_step_groups /
vitpe_lr_schedule (csrc/optim.hip) against the float64 restatements of tests/optim_groups_ref.py and, with every scale 1,
against vitpe_adamw_step bit for bit; then TrainEngine.set_param_groups / set_lr_schedule eager, in captured graphs, on the
extras route and from train.py.

Tolerances.  The grouped update is adamw_kernel's arithmetic with lr and wd replaced by fp32 products the reference forms
the same way, so train_state_ref.adamw_bounds (a count of fp32 roundings, U = 2^-24) holds unchanged, evaluated with each
group's own lr and wd.  The schedule is computed in fp64 on the device and rounded once to fp32: it can only miss the
correctly rounded float64 reference next to a rounding tie, so 1 fp32 ulp; from step T on it is min_lr itself."""
import csv
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import optim_groups_ref as R
import train_state_ref as TS
from conftest import rel_err

pytestmark = pytest.mark.gpu

GUARD = 1e3       # in front of and behind every device vector
BIG = R.SWEEP + 4099


@pytest.fixture(scope="module")
def K():
    from vitpe import kernels
    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert kernels.adamw_groups_blocks(R.SWEEP) == R.GRID_CAP == kernels.adamw_groups_blocks(BIG)   # the cap as built
    assert kernels.adamw_groups_blocks(R.SWEEP - 2048) == R.GRID_CAP - 1
    return kernels


def bits(t):
    """integer view of a tensor's storage: equality of these is bit-equality (tells -0 from +0)"""
    t = t.detach().contiguous().reshape(-1)
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(bits(a), bits(b.to(a.device))))


def f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def worst(err, bound):
    """largest |err| / bound over the elements (0 / 0 = 0: an exact result under a zero bound passes)"""
    err, bound = np.abs(err), np.asarray(bound, dtype=np.float64)
    if err.size == 0:
        return 0.0
    r = np.where(err == 0, 0.0, err / np.where(bound > 0, bound, 1e-300))
    return float(r.max())


def ulps(got, want):
    want = np.float32(want)
    return abs(float(np.float32(got)) - float(want)) / float(np.spacing(np.abs(want)))


def guarded(x, dtype=torch.float32):
    """x (numpy or tensor, 1-d) on the device 16 bytes into a buffer of guard values, 16 bytes of them behind it too
    -> (buffer, view)."""
    x = torch.from_numpy(x) if isinstance(x, np.ndarray) else x
    n, pad = x.shape[0], 16 // torch.empty(0, dtype=dtype).element_size()
    buf = torch.full((n + 2 * pad,), GUARD if dtype != torch.uint8 else 200, dtype=dtype, device="cuda")
    view = buf[pad:pad + n]
    view.copy_(x.to(dtype))
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 0
    return buf, view


def guards_intact(buf, n):
    pad = (buf.numel() - n) // 2
    fill = 200 if buf.dtype == torch.uint8 else GUARD
    return bool((buf[:pad] == fill).all()) and bool((buf[pad + n:] == fill).all())


def cast_bits(K, x):
    """bits of vitpe_cast's bf16 of x (an empty vector has nothing to cast: the call refuses a NULL source)"""
    if x.numel() == 0:
        return bits(torch.empty(0, dtype=torch.bfloat16, device="cuda"))
    return bits(K.cast(x.clone(), torch.bfloat16))


TICKED = (3.0, float(np.float32(1.0) - np.float32(0.9) ** 3), float(np.float32(1.0) - np.float32(0.999) ** 3))


def _hp(ticked, **over):
    """adamw's block with every slot the kernels do not own filled, so that a stray write shows"""
    hp = TS.adamw_hp(**over)
    hp[9:16] = [0.7, 3.0, 0.7, 2.0, 0.9, 1.0, -5.0]
    if ticked:
        hp[5:8] = TICKED
    return hp


_INPUTS = {}


def _inputs(n):
    """(p0, g, map) of size n, drawn once for every test that uses the size"""
    if n not in _INPUTS:
        # (adamw_inputs zeroes every 17th gradient from the first on and needs one that is not: the smallest sizes are
        #  cut from a draw of 64, behind its first element)
        p0, g = TS.adamw_inputs(n, seed=n % 1000) if n >= 64 else tuple(x[1:1 + n].copy() for x in TS.adamw_inputs(64, seed=n))
        _INPUTS[n] = (p0, g, R.span_map(n))
    return _INPUTS[n]


def _state(n, moments=False):
    """guarded device copies of the inputs of size n -> dict of (buffer, view); moments: m and v start non-zero with the
    gradient's sign, so that nothing cancels"""
    p0, g, gid = _inputs(n)
    m0 = (0.1 * g).astype(np.float32) if moments else np.zeros(n, np.float32)
    v0 = (0.01 * g * g).astype(np.float32) if moments else np.zeros(n, np.float32)
    st = {"p": guarded(p0), "g": guarded(g), "m": guarded(m0), "v": guarded(v0),
          "s": guarded(np.full(n, -7.0, np.float32), torch.bfloat16), "gid": guarded(gid, torch.uint8)}
    return st, (p0, g, m0, v0, gid)


# ------------------------------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("n", R.SIZES)
def test_kernel_against_the_float64_reference(K, n):
    table = np.array(R.GROUPS4, dtype=np.float32)
    gtab_buf, gtab = guarded(table.reshape(-1))
    # (zero_grad, ticked, with shadow): g cleared / kept, the tick made here / already made, shadow written / None
    for zero_grad, ticked, shadow in ((True, False, True), (False, True, False)):
        st, (p0, g0, m0, v0, gid) = _state(n)
        hp_np = _hp(ticked)
        hp = torch.from_numpy(hp_np).cuda()
        p, g, m, v, s = (st[k][1] for k in ("p", "g", "m", "v", "s"))
        K.adamw_step_groups(p, g, m, v, hp, st["gid"][1], gtab.view(-1, 2), shadow_bf16=s if shadow else None,
                            zero_grad=zero_grad, ticked=ticked)
        torch.cuda.synchronize()
        out_hp = hp.cpu().numpy()
        if ticked:
            assert out_hp.tobytes() == hp_np.tobytes()
        else:                                                                # the tick, also at n == 0
            assert out_hp[:5].tobytes() == hp_np[:5].tobytes() and out_hp[8:].tobytes() == hp_np[8:].tobytes()
            want = R.bias_corrections(hp_np, 1)
            assert out_hp[5] == 1.0 and ulps(out_hp[6], want[0]) <= 4 and ulps(out_hp[7], want[1]) <= 4
        for k in ("p", "g", "m", "v", "s", "gid"):
            assert guards_intact(st[k][0], n), k
        assert guards_intact(gtab_buf, 8) and same_bits(gtab, torch.from_numpy(table.reshape(-1)))
        assert same_bits(st["gid"][1], torch.from_numpy(gid))
        assert same_bits(g, torch.zeros(n) if zero_grad else torch.from_numpy(g0))       # cleared only with bit 0
        if shadow:
            assert torch.equal(bits(s), cast_bits(K, p))                     # vitpe_cast's rounding of the new p
        else:
            assert same_bits(s, torch.full((n,), -7.0, dtype=torch.bfloat16))
        if n == 0:
            continue
        p_ref, m_ref, v_ref, d_ref = R.grouped_adamw_ref(p0, g0, m0, v0, out_hp, float(out_hp[6]), float(out_hp[7]), gid,
                                                         R.GROUPS4)
        bp, bm, bv = TS.adamw_bounds(p0, p_ref, m_ref, v_ref, d_ref)
        fig = (worst(f64(p) - p_ref, bp), worst(f64(m) - m_ref, bm), worst(f64(v) - v_ref, bv))
        print(f"n {n} zero_grad {zero_grad} ticked {ticked}: worst |err| / bound  p {fig[0]:.3f}  m {fig[1]:.3f}  v {fig[2]:.3f}")
        assert max(fig) <= 1.0, (n, fig)
        # the (0, 0) group: its parameters keep their bits while its moments moved
        frozen = torch.from_numpy(R.element_groups(gid, n) == 3).cuda()
        if bool(frozen.any()):
            assert same_bits(p[frozen], torch.from_numpy(p0)[frozen.cpu()])
            moved = g0[frozen.cpu().numpy()] != 0
            assert bool((m[frozen].cpu().numpy()[moved] != 0).all()) and bool((v[frozen].cpu().numpy()[moved] != 0).all())
        if n >= 2048:
            assert not same_bits(p[~frozen], torch.from_numpy(p0)[~frozen.cpu()])


# ------------------------------------------------------------------------------------------ 2. bit-identity
@pytest.mark.parametrize("n", [9, 2048 + 5, BIG])
def test_unit_scales_are_adamw_step_bit_for_bit(K, n):
    gtab = torch.ones(4, 2, device="cuda")
    for zero_grad in (False, True):
        for ticked in (False, True):
            for clipped in (False, True):
                hp_np = _hp(ticked)
                hp_np[9] = np.float32(hp_np[8] * np.float32(0.37))           # hp[9] != hp[8]: bit 2 shows
                runs = []
                for grouped in (False, True):
                    st, _ = _state(n, moments=True)
                    hp = torch.from_numpy(hp_np).cuda()
                    p, g, m, v, s = (st[k][1] for k in ("p", "g", "m", "v", "s"))
                    if grouped:
                        K.adamw_step_groups(p, g, m, v, hp, st["gid"][1], gtab, shadow_bf16=s, zero_grad=zero_grad,
                                            ticked=ticked, clipped=clipped)
                    else:
                        K.adamw_step(p, g, m, v, hp, shadow_bf16=s, zero_grad=zero_grad, ticked=ticked, clipped=clipped)
                    runs.append((st, hp))
                torch.cuda.synchronize()
                (a, hp_a), (b, hp_b) = runs
                for k in ("p", "g", "m", "v", "s"):
                    assert same_bits(a[k][0], b[k][0]), (k, zero_grad, ticked, clipped)   # guards included
                assert same_bits(hp_a, hp_b)
                assert float(hp_a[5]) == (3.0 if ticked else 1.0)
                assert not same_bits(a["p"][1], torch.from_numpy(_inputs(n)[0]))
    # ... and the two gradient scales do give different updates (the comparison above is not of two no-ops)
    assert hp_np[9] != hp_np[8]


# ------------------------------------------------------------------------------------------ 3. refusals
def test_refusals_write_nothing(K):
    from vitpe import _lib as L
    n = 2048 + 5
    st, (p0, g0, m0, v0, gid) = _state(n, moments=True)
    hp_np = _hp(False)
    hp = torch.from_numpy(hp_np).cuda()
    gtab = torch.tensor(R.GROUPS4, device="cuda")
    p, g, m, v, s, gd = (st[k][1] for k in ("p", "g", "m", "v", "s", "gid"))
    stream = torch.cuda.current_stream().cuda_stream
    ok = dict(p=p.data_ptr(), g=g.data_ptr(), m=m.data_ptr(), v=v.data_ptr(), sh=s.data_ptr(), hp=hp.data_ptr(), n=n, zg=1,
              gid=gd.data_ptr(), n_gid=gd.numel(), gtab=gtab.data_ptr(), ng=4)

    def call(**over):
        a = dict(ok, **over)
        return L.lib().vitpe_adamw_step_groups(a["p"], a["g"], a["m"], a["v"], a["sh"], a["hp"], a["n"], a["zg"], a["gid"],
                                               a["n_gid"], a["gtab"], a["ng"], stream)

    for name in ("p", "g", "m", "v", "hp", "gid", "gtab"):                   # a NULL pointer with n > 0
        assert call(**{name: None}) == 1, name
    assert call(n=-1) == 1
    assert call(ng=0) == 1 and call(ng=257) == 1
    assert call(n_gid=R.n_granules(n) - 1) == 1
    for name in ("p", "g", "m", "v"):                                        # 4 and 8 bytes past a 16-byte boundary
        assert call(**{name: ok[name] + 4}) == 1 and call(**{name: ok[name] + 8}) == 1, name
    assert call(sh=ok["sh"] + 2) == 1 and call(sh=ok["sh"] + 4) == 1
    assert L.lib().vitpe_lr_schedule(None, gtab.data_ptr(), 0, stream) == 1
    assert L.lib().vitpe_lr_schedule(hp.data_ptr(), None, 0, stream) == 1
    # the binding's own checks
    for args, kw in (((p, g, m, v, hp, gd.to(torch.int32), gtab), {}), ((p, g, m, v, hp, gd[:-1], gtab), {}),
                     ((p, g, m, v, hp[:8], gd, gtab), {}), ((p, g, m, v, hp, gd, gtab.double()), {}),
                     ((p, g, m, v, hp, gd, gtab.view(-1)[:3]), {}), ((p, g[:-1], m, v, hp, gd, gtab), {}),
                     ((p, g, m, v, hp, gd, gtab), dict(shadow_bf16=s.float())), ((p.cpu(), g, m, v, hp, gd, gtab), {}),
                     ((st["p"][0][5:5 + n], g, m, v, hp, gd, gtab), {}), ((p, g, m, v, hp, None, gtab), {})):
        with pytest.raises(L.VitpeError):
            K.adamw_step_groups(*args, **kw)
    with pytest.raises(L.VitpeError):
        K.lr_schedule(hp, gtab[:3].reshape(-1))
    with pytest.raises(L.VitpeError):
        K.lr_schedule(hp[:8], gtab.reshape(-1))
    torch.cuda.synchronize()
    fresh, _ = _state(n, moments=True)
    for k in ("p", "g", "m", "v", "s", "gid"):
        assert same_bits(st[k][0], fresh[k][0]), k
    assert hp.cpu().numpy().tobytes() == hp_np.tobytes()                     # not even the tick
    assert same_bits(gtab, torch.tensor(R.GROUPS4))


# ------------------------------------------------------------------------------------------ 4. the schedule
ORIGIN = 11.0


@pytest.mark.parametrize("case", R.SCHED_CASES)
def test_lr_schedule_against_the_closed_form(K, case):
    base, lo, W, T, s0 = case
    blk0 = R.sched_block(base, lo, W, T, s0, ORIGIN)
    wide = [float(x) for x in blk0[:5]]                   # what the device reads: the fp32 numbers
    took = set()
    for k in R.sched_ks(W, T):
        for ticked in (0, 1):
            hp_np = _hp(True)
            hp_np[0] = -1.0
            hp_np[5] = ORIGIN + k + ticked
            hp, sched = torch.from_numpy(hp_np).cuda(), torch.from_numpy(blk0).cuda()
            K.lr_schedule(hp, sched, ticked=bool(ticked))
            torch.cuda.synchronize()
            out_hp, out = hp.cpu().numpy(), sched.cpu().numpy()
            ref = R.schedule_ref(k, wide[0], wide[1], int(wide[2]), int(wide[3]), wide[4])
            print(f"{case} k {k} ticked {ticked}: hp[0] {out_hp[0]!r} float64 reference {ref!r} "
                  f"difference {ulps(out_hp[0], ref) if ref else abs(float(out_hp[0])):.2f} ulp")
            if ref == 0.0:
                assert out_hp[0] == 0.0
            else:
                assert ulps(out_hp[0], ref) <= 1
            if k >= T:
                assert out_hp[0].tobytes() == blk0[1].tobytes()             # fp32(min_lr) exactly
            assert out[6].tobytes() == out_hp[0].tobytes()
            assert out_hp[1:].tobytes() == hp_np[1:].tobytes()
            assert out[:6].tobytes() == blk0[:6].tobytes() and out[7].tobytes() == blk0[7].tobytes()
            took.add("warm" if k < W else "end" if k >= T else "cos")
    assert took == ({"warm", "cos", "end"} if W > 0 else {"cos", "end"})
    # before the origin (a counter that was reset): step 0
    hp_np = _hp(True)
    hp_np[5] = ORIGIN - 4
    hp, sched = torch.from_numpy(hp_np).cuda(), torch.from_numpy(blk0).cuda()
    K.lr_schedule(hp, sched)
    assert ulps(hp[0].item(), R.schedule_ref(0, *wide[:2], int(wide[2]), int(wide[3]), wide[4])) <= 1


# ------------------------------------------------------------------------------------------ 5. - 7. TrainEngine
B = 8


def _engine(use_graph, extras=False, dt=torch.float32, B=B, **adamw):
    """The smallest geometry the engine takes: embed_dim 64, 2 heads, depth 2, 16 x 16 images in 4 x 4 patches (17
    tokens), a fixed batch of 8.  adamw: optimizer arguments of TrainEngine other than the defaults."""
    from models.vit import VisionTransformer
    from vitpe.engine import TrainEngine
    torch.manual_seed(0)
    model = VisionTransformer(img_size=16, patch_size=4, embed_dim=64, depth=2, num_heads=2, pos_encoding="absolute").cuda()
    eng = TrainEngine(model, B, compute_dtype=dt, use_graph=use_graph, extras=extras, weight_decay=0.05, **adamw)
    g = torch.Generator().manual_seed(7)
    eng.images.copy_(torch.randn(B, 3, 16, 16, generator=g))
    eng.labels.copy_(torch.randint(0, 10, (B,), generator=g))
    return eng


def _floors(bm, bv, m_ref, v_ref):
    """adamw_bounds are relative and hold for normal numbers; a real gradient also has elements whose (1 - b2) g^2 (or
    (1 - b1) g) is subnormal, where one rounding is half a subnormal spacing (2^-150) whatever the value: the same counts
    of roundings (m 4, v 6) at that absolute size there (as tests/test_grad_clip_gpu.py)."""
    tiny, sub = 2.0 ** -126, 2.0 ** -150
    return (np.where(np.abs(m_ref) < tiny, np.maximum(bm, 4 * sub), bm), np.where(np.abs(v_ref) < tiny, np.maximum(bv, 6 * sub), bv))


def _host_map(eng, groups):
    """the map and table set_param_groups must have built, restated from the engine's offsets"""
    from vitpe.optim import param_granule_map
    spans = [(eng._off[id(p)], p.numel(), k) for k, g in enumerate(groups, start=1) for p in g["params"]]
    table = [(1.0, 1.0)] + [(g["lr_scale"], g["weight_decay_scale"]) for g in groups]
    return param_granule_map(spans, eng.n_flat), table


@pytest.mark.parametrize("variant", ["plain", "clip", "extras"])
def test_engine_eager_fp32_updates_every_group_with_its_own_rates(variant):
    from vitpe.optim import vit_param_groups
    eng = _engine(False, extras=(variant == "extras"))
    groups = vit_param_groups(eng.model, True, 0.75)
    eng.set_param_groups(groups)
    gid, table = _host_map(eng, groups)
    assert np.array_equal(eng.opt._gid.cpu().numpy(), gid) and eng.opt._gid.dtype == torch.uint8
    assert np.array_equal(eng.opt._gtab.cpu().numpy(), np.array(table, dtype=np.float32))
    assert len(table) == 1 + len(groups) and len({t for t in table}) >= 7      # 4 layer ids x decay or not
    eng.forward_backward()
    if variant == "clip":
        norm = float(np.linalg.norm(f64(eng.flat_g))) * float(eng.hp[8])
        eng.set_grad_clip(0.5 * norm)
    p0, g0, m0, v0 = (f64(getattr(eng, k)) for k in ("flat_p", "flat_g", "flat_m", "flat_v"))
    eng._optimizer()
    torch.cuda.synchronize()
    hp = eng.hp.cpu().numpy()
    assert hp[5] == 1.0 and float(eng.flat_g.abs().max()) == 0.0
    hp_ref = hp.copy()
    if variant == "clip":
        assert abs(float(hp[11]) - 0.5) < 1e-3
        hp_ref[8] = hp[9]                                  # the scale the device used
    p_ref, m_ref, v_ref, d_ref = R.grouped_adamw_ref(p0, g0, m0, v0, hp_ref, float(hp[6]), float(hp[7]), gid, table)
    bp, bm, bv = TS.adamw_bounds(p0, p_ref, m_ref, v_ref, d_ref)
    bm, bv = _floors(bm, bv, m_ref, v_ref)
    figs = (worst(f64(eng.flat_p) - p_ref, bp), worst(f64(eng.flat_m) - m_ref, bm), worst(f64(eng.flat_v) - v_ref, bv))
    plain = TS.adamw_ref(p0, g0, m0, v0, hp_ref, float(hp[6]), float(hp[7]))
    miss = worst(plain[0] - p_ref, bp)
    print(f"{variant}: n_flat {eng.n_flat}, {len(groups)} groups; worst |err| / bound  p {figs[0]:.3f}  m {figs[1]:.3f}  "
          f"v {figs[2]:.3f}; the one-group update misses by {miss:.3g} bounds")
    assert max(figs) <= 1.0, figs
    assert miss > 100                                       # ... so the groups were really applied


# The replay test's rates.  Its last assertion compares two bf16 engines to 1e-5 of the largest parameter (1.0, the
# LayerNorm gains).  Their gradients differ in the last fp32 bits (the weight gradients are summed with atomics), and in
# bf16 such a difference now and then tips the rounding of one weight or activation: a relative change of up to 2^-8 in
# what it feeds, a few times that in single gradient elements, and lr times that in the step AdamW takes (its step is at
# most lr per element).  One tipped rounding at lr = 1e-3 is therefore worth about 1e-3 * 4 * 2^-8 = 1.6e-5 -- the whole
# gate (seen once this was written down: 1.08e-5 from one at lr = 8.6e-4, the same element in run after run, 7e-9
# without one) -- and at 1e-4 a tenth of it, which leaves the gate to what it is for: a launch that reads the wrong rate
# or the wrong group (the second group alone moves by 0.75 * lr per step, 1e-4 of the largest parameter).
BASE_LR, MIN_LR = 1e-4, 1e-6


def _drive(eng, groups, steps, scale_at=None):
    """`steps` steps under a W = 2, T = 6 schedule; the learning rate after every step, and flat_p after every step"""
    eng.set_param_groups(groups)
    eng.set_lr_schedule(BASE_LR, 6, warmup_steps=2, min_lr=MIN_LR, warmup_factor=0.1)
    lrs, ps = [], []
    for j in range(steps):
        if scale_at is not None and j == scale_at[0]:
            scale_at[1](eng)
        eng.step()
        lrs.append(eng.current_lr())
        ps.append(eng.flat_p.clone())
    return lrs, ps


def test_engine_captured_bf16_follows_the_schedule_and_the_groups():
    """AdamW's eps is 1e-3 in both engines, as in tests/test_ema_gpu.py's replay tests and for their reason: at 1e-8 two
    runs of ONE engine already differ by multiples of 1e-6 (the atomics' order amplified by lr / eps), which is the size
    of the 1e-5 gate."""
    from vitpe._lib import VitpeError
    eager, graph = _engine(False, dt=torch.bfloat16, eps=1e-3), _engine(True, dt=torch.bfloat16, eps=1e-3)

    def groups_of(eng, block_scale=1.0):
        head = [p for n, p in eng.model.named_parameters() if n.startswith("head.")]
        blk = [p for n, p in eng.model.named_parameters() if n.startswith("blocks.1.")]
        return [{"params": head, "lr_scale": 0.0, "weight_decay_scale": 0.0}, {"params": blk, "lr_scale": block_scale}]

    fbs = []

    def rescale(eng):                                       # the same partition, a new scale: one device write
        fbs.append(eng.graph_fb)
        eng.set_param_groups(groups_of(eng, 0.25))
        assert eng.graph_fb is fbs[-1]
        assert eng.opt._gtab.cpu().tolist() == [[1.0, 1.0], [0.0, 0.0], [0.25, 1.0]]

    p_start = graph.flat_p.clone()
    lrs_e, ps_e = _drive(eager, groups_of(eager), 8, scale_at=(4, rescale))
    assert graph.graph_fb is None
    lrs_g, ps_g = _drive(graph, groups_of(graph), 8, scale_at=(4, rescale))
    torch.cuda.synchronize()
    assert graph.graph_fb is not None and graph.graph_fb is fbs[1] and eager.graph_fb is None   # one capture for all 8
    blk = [float(x) for x in R.sched_block(BASE_LR, MIN_LR, 2, 6, 0.1, 0.0)[:5]]
    for j in range(8):
        ref = R.schedule_ref(j, blk[0], blk[1], 2, 6, blk[4])
        print(f"step {j}: lr graph {lrs_g[j]!r} eager {lrs_e[j]!r} reference {ref!r}")
        assert ulps(lrs_g[j], ref) <= 1 and ulps(lrs_e[j], ref) <= 1
    assert lrs_g[5] != lrs_g[4] and lrs_g[6] == lrs_g[7] == float(np.float32(MIN_LR))
    assert float(graph.hp[5]) == 8.0 and float(graph.opt._sched[6]) == lrs_g[7]
    # the frozen group keeps its bits over all 8 steps; the others move at every step
    head_span = [(graph._off[id(p)], p.numel()) for n, p in graph.model.named_parameters() if n.startswith("head.")]
    other = graph.model.blocks[0].mlp.fc1.weight
    o_o, o_n = graph._off[id(other)], other.numel()
    for j in range(8):
        for o, k in head_span:
            assert same_bits(ps_g[j][o:o + k], p_start[o:o + k]) and same_bits(ps_e[j][o:o + k], p_start[o:o + k])
        before = p_start if j == 0 else ps_g[j - 1]
        assert not same_bits(ps_g[j][o_o:o_o + o_n], before[o_o:o_o + o_n])
    # the new scale took effect in the replay: blocks.1 moves less from step 4 on than a constant scale would
    # (lr falls as well, so compare with blocks.0, whose scale stayed: the ratio of the two steps drops by about 4)
    b1 = graph.model.blocks[1].mlp.fc1.weight
    b_o, b_n = graph._off[id(b1)], b1.numel()

    def moved(j, o, k):
        return float((ps_g[j][o:o + k] - ps_g[j - 1][o:o + k]).abs().mean())

    ratio_before = moved(3, b_o, b_n) / moved(3, o_o, o_n)
    ratio_after = moved(4, b_o, b_n) / moved(4, o_o, o_n)
    print(f"mean |step| of blocks.1 / blocks.0: {ratio_before:.3f} before the new scale, {ratio_after:.3f} after")
    assert ratio_after < 0.5 * ratio_before
    # graph against eager, the relation of test_grad_clip_gpu.py::test_engine_graph_replay_clips_like_the_eager_engine
    err = rel_err(graph.flat_p.cpu(), eager.flat_p.cpu())
    print(f"parameters graph vs eager after 8 steps: rel err {err:.3e}")
    assert err < 1e-5
    for eng in (eager, graph):
        assert float(eng.hp[5]) == 8.0 and float(eng.flat_g.abs().max()) == 0.0
    # set_lr under the schedule refuses; a new schedule for an enabled one keeps the graph, switching off drops it
    with pytest.raises(VitpeError, match="set_lr"):
        graph.set_lr(1e-4)
    fb = graph.graph_fb
    graph.set_lr_schedule(2e-3, 10, warmup_steps=0, done=3)
    assert graph.graph_fb is fb
    graph.step()
    assert graph.graph_fb is fb and ulps(graph.current_lr(), R.schedule_ref(3, float(np.float32(2e-3)), 0.0, 0, 10, 1e-3)) <= 1
    graph.set_lr_schedule(None)
    assert graph.graph_fb is None and graph.opt.lr_sched is None
    graph.set_lr(5e-4)
    graph.step()
    assert graph.current_lr() == float(np.float32(5e-4)) and float(graph.hp[5]) == 10.0


def test_capture_leaves_the_schedule_where_it_found_it():
    eng = _engine(True, dt=torch.bfloat16)
    eng.step()                                              # a counter that is not just zero
    eng.set_lr_schedule(1e-3, 6, warmup_steps=2, warmup_factor=0.1, done=1)
    assert eng.graph_fb is None
    hp_before, sched_before = eng.hp.clone(), eng.opt._sched.clone()
    assert float(sched_before[5]) == 0.0
    eng.capture()
    torch.cuda.synchronize()
    assert same_bits(eng.hp, hp_before) and same_bits(eng.opt._sched, sched_before)
    eng.step()
    assert float(eng.hp[5]) == 2.0
    assert ulps(eng.current_lr(), R.schedule_ref(1, float(np.float32(1e-3)), 0.0, 2, 6, float(np.float32(0.1)))) <= 1


B_INERT = 4


def test_groups_and_schedule_switched_off_again_are_inert():
    """One engine never touched, one with groups and schedule set and then unset, the same seed and data, 2 captured bf16
    steps each: identical flat_p, flat_m, flat_v and hp, bit for bit.

    The batch is 4, not the 8 of the other engine tests.  At 8 this geometry's backward is not reproducible from one
    engine to the next (its weight gradients meet in fp32 atomics whose order varies): two UNTOUCHED engines differed in
    757 .. 1737 elements of flat_p after 2 steps in 9 pairs out of 9, so nothing could be told from bits there.  At 1, 2
    and 4 images they agreed in every bit in 12 pairs out of 12 (bf16, depth 1 and 2).  The test carries its own
    control: a second untouched engine must agree with the first, else the comparison says nothing and fails as such."""
    from vitpe.optim import vit_param_groups
    plain, control, toggled = (_engine(True, dt=torch.bfloat16, B=B_INERT) for _ in range(3))
    toggled.set_param_groups(vit_param_groups(toggled.model, True, 0.75))
    toggled.set_lr_schedule(1e-3, 6, warmup_steps=2)
    hp0 = toggled.hp.clone()
    toggled.set_param_groups(None)
    toggled.set_lr_schedule(None)
    assert toggled.opt.param_groups is None and toggled.opt._gid is None and toggled.opt._gtab is None
    assert toggled.opt.lr_sched is None and toggled.opt._sched is None and same_bits(toggled.hp, hp0) and same_bits(plain.hp, hp0)
    for _ in range(2):
        plain.step(); control.step(); toggled.step()
    torch.cuda.synchronize()
    for other, what in ((control, "control (untouched)"), (toggled, "toggled")):
        for name in ("flat_p", "flat_m", "flat_v", "hp"):
            a, b = getattr(other, name), getattr(plain, name)
            print(f"{what} {name}: {int((bits(a) != bits(b)).sum())} of {a.numel()} elements differ from the untouched "
                  f"engine's in their bits")
    assert float(plain.hp[5]) == 2.0 and not same_bits(plain.flat_p, _engine(False, dt=torch.bfloat16, B=B_INERT).flat_p)
    for name in ("flat_p", "flat_m", "flat_v", "hp"):
        assert same_bits(getattr(control, name), getattr(plain, name)), "the control: " + name
    for name in ("flat_p", "flat_m", "flat_v", "hp"):
        assert same_bits(getattr(toggled, name), getattr(plain, name)), name


# ------------------------------------------------------------------------------------------ 8. train.py
def test_train_py_runs_with_groups_and_schedule(tmp_path):
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(repo, "train.py"), "--synthetic", "--epochs", "1", "--steps_per_epoch", "3",
           "--no_decay_norm_bias", "--layer_decay", "0.75", "--warmup_epochs", "0.34", "--min_lr", "1e-5",
           "--batch_size", "16", "--embed_dim", "96", "--depth", "2", "--num_heads", "3",
           "--log_dir", str(tmp_path / "logs"), "--ckpt_dir", str(tmp_path / "ckpt")]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    print(res.stdout[-2000:], res.stderr[-2000:])
    assert res.returncode == 0
    logs = glob.glob(str(tmp_path / "logs" / "*.csv"))
    assert len(logs) == 1
    rows = list(csv.reader(open(logs[0]).read().splitlines()))
    assert rows[0][:6] == ["epoch", "train_loss", "train_acc", "test_loss", "test_acc", "best_acc"]
    assert len(rows) == 2 and np.isfinite(float(rows[1][1]))
