"""Weight EMA inside the train step: vitpe_ema_update / vitpe_ema_swap (csrc/optim.hip) against the float64 restatement of
tests/ema_ref.py, then TrainEngine.set_ema / ema_weights / ema_state_dict eager, in captured graphs, on the extras route
and from train.py --model_ema.

Tolerance of the update (ema_ref.ema_bound, from the kernel's arithmetic, not from its results; U = 2^-24): the device
rounds p - e once and the fma once, so |e' - ref| <= U (w |p - e| + |e'|) per element, with w = 1 - d_t formed in fp32 on
both sides from the device's own hp[15].  hp[15] itself is compared with the numpy fp32 rule to 1 ulp (a correctly rounded
division gives 0).  Over k engine steps the bounds add: each step multiplies the error it inherits by d_t < 1."""
import csv

import numpy as np
import pytest
import torch

import ema_ref as R
from conftest import rel_err

pytestmark = pytest.mark.gpu

GUARD = 1e3       # in front of and behind every device vector
SENTINEL = -5.0   # in hp[15] before a call
SIZES = R.SIZES + (R.SWEEP + 4099,)   # the last: one full sweep of the capped grid, then a second, partial one and the tail


@pytest.fixture(scope="module")
def K():
    from vitpe import kernels
    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert kernels.ema_blocks(R.SWEEP) == R.GRID_CAP == kernels.ema_blocks(R.SWEEP + 4099)   # the cap as built
    assert kernels.ema_blocks(R.SWEEP - 1024) == R.GRID_CAP - 1
    return kernels


def bits(t):
    """integer view of a tensor's storage: equality of these is bit-equality (tells -0 from +0)"""
    t = t.detach().contiguous().cpu().reshape(-1)
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


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


def guarded(x_np, dtype=torch.float32):
    """x_np on the device 16 bytes into a buffer of guard values, 16 bytes of them behind it too -> (buffer, view)."""
    n, pad = x_np.shape[0], 16 // torch.empty(0, dtype=dtype).element_size()
    buf = torch.full((n + 2 * pad,), GUARD, dtype=dtype, device="cuda")
    view = buf[pad:pad + n]
    view.copy_(torch.from_numpy(x_np).to(dtype))
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 0
    return buf, view


def cast_bits(K, x):
    """bits of vitpe_cast's bf16 of x (an empty vector has nothing to cast: the call refuses a NULL source)"""
    if x.numel() == 0:
        return bits(torch.empty(0, dtype=torch.bfloat16))
    return bits(K.cast(x.clone(), torch.bfloat16))


def guards_intact(buf, n):
    pad = (buf.numel() - n) // 2
    return bool((buf[:pad] == GUARD).all()) and bool((buf[pad + n:] == GUARD).all())


def _hp(decay, step=0.0, base=0.0):
    hp = np.zeros(16, dtype=np.float32)
    hp[:5] = [1e-3, 0.9, 0.999, 1e-8, 0.01]
    hp[5], hp[6], hp[7], hp[8] = step, 0.5, 0.25, 1.0
    hp[9:13] = [0.7, 3.0, 0.7, 2.0]
    hp[13], hp[14], hp[15] = decay, base, SENTINEL
    return hp


_INPUTS = {}


def _inputs(n):
    """(p, e, marks) of size n, drawn once for every test that uses the size."""
    if n not in _INPUTS:
        p, e = R.ema_inputs(n, seed=n % 1000)
        _INPUTS[n] = R.with_marks(p, e)
    return _INPUTS[n]


# ------------------------------------------------------------------------------------------ 1. the update kernel
DECAY, BASE = 0.9, 7.0
# (warmup, t): without warm-up; with it at t = 1 and 5 (the ramp 2/11, 6/15 is below 0.9) and t = 1000 (1001/1010 is above)
RUNS = ((0, 3), (1, 1), (1, 5), (1, 1000))


@pytest.mark.parametrize("n", SIZES)
def test_update_against_the_float64_reference(K, n):
    p_np, e_np, marks = _inputs(n)
    took = set()
    for warmup, t in RUNS:
        pbuf, p = guarded(p_np)
        ebuf, e = guarded(e_np)
        hp_np = _hp(DECAY, step=BASE + t, base=BASE)
        hp = torch.from_numpy(hp_np).cuda()
        K.ema_update(p, e, hp, warmup=bool(warmup))
        torch.cuda.synchronize()
        out_hp = hp.cpu().numpy()
        assert out_hp[:15].tobytes() == hp_np[:15].tobytes()                 # hp is only read, but for [15]
        assert guards_intact(pbuf, n) and guards_intact(ebuf, n)
        assert torch.equal(bits(p), bits(torch.from_numpy(p_np)))            # p bit for bit
        if n == 0:                                                           # nothing is launched: [15] keeps its value
            assert out_hp[15] == np.float32(SENTINEL)
            continue
        d_dev = out_hp[15]
        if not warmup:
            assert d_dev.tobytes() == hp_np[13].tobytes()
        else:
            d_ref = R.warmup_decay(hp_np[13], t)
            took.add("decay" if d_ref == hp_np[13] else "ramp")
            print(f"n {n} t {t}: hp[15] {d_dev!r} numpy fp32 {d_ref!r} difference {ulps(d_dev, d_ref):.1f} ulp")
            assert ulps(d_dev, d_ref) <= 1
        ref = R.ema_ref(p_np, e_np, d_dev)
        fig = worst(f64(e) - ref, R.ema_bound(p_np, e_np, ref, d_dev))
        print(f"n {n} warmup {warmup} t {t}: worst |err| / bound {fig:.3f}")
        assert fig <= 1.0, (n, warmup, t)
        got = bits(e)
        want_in = bits(torch.from_numpy(e_np))
        for i in marks["equal"]:                                             # the fixed point: e's bits stay
            assert got[i] == want_in[i], i
        e_out = e.cpu().numpy()
        w32 = np.float32(1.0) - np.float32(d_dev)
        for i in marks["e_zero"]:                                            # fma(w, p, 0) = fl(w p): one rounding, exact here
            assert e_out[i] == np.float32(w32 * p_np[i]), i
        for i in marks["p_zero"]:
            assert abs(float(e_out[i]) - float(ref[i])) <= R.U * (R.lerp_weight(d_dev) + 1) * abs(float(e_np[i])), i
        if n >= 4:
            assert not np.array_equal(e_out, e_np)                           # ... and the rest did move
    if n > 0:
        assert took == {"decay", "ramp"}


def test_update_refusals_write_nothing(K):
    from vitpe import _lib as L
    n = 4099
    p_np, e_np, _ = _inputs(n)
    pbuf, p = guarded(p_np)
    ebuf, e = guarded(e_np)
    hp_np = _hp(DECAY, step=3.0)
    hp = torch.from_numpy(hp_np).cuda()
    with pytest.raises(L.VitpeError):                     # a pointer 4 bytes past a 16-byte boundary
        K.ema_update(pbuf[5:5 + n], e, hp)
    with pytest.raises(L.VitpeError):
        K.ema_update(p, ebuf[3:3 + n], hp)
    with pytest.raises(L.VitpeError):
        K.ema_update(p, e, None)
    with pytest.raises(L.VitpeError):
        K.ema_update(p, e, hp[:8])
    with pytest.raises(L.VitpeError):
        K.ema_update(p.cpu(), e, hp)
    st = torch.cuda.current_stream().cuda_stream
    assert L.lib().vitpe_ema_update(p.data_ptr(), e.data_ptr(), None, n, 0, st) == 1        # NULL hp at the C boundary
    assert L.lib().vitpe_ema_update(p.data_ptr() + 4, e.data_ptr(), hp.data_ptr(), n, 0, st) == 1
    torch.cuda.synchronize()
    assert torch.equal(bits(ebuf), bits(guarded(e_np)[0])) and torch.equal(bits(pbuf), bits(guarded(p_np)[0]))
    assert hp.cpu().numpy().tobytes() == hp_np.tobytes()


# ------------------------------------------------------------------------------------------ 2. the swap kernel
@pytest.mark.parametrize("with_shadow", [True, False])
@pytest.mark.parametrize("n", SIZES)
def test_swap_exchanges_and_two_swaps_restore(K, n, with_shadow):
    p_np, e_np, _ = _inputs(n)
    pbuf, p = guarded(p_np)
    ebuf, e = guarded(e_np)
    sbuf = s = None
    if with_shadow:
        sbuf, s = guarded(np.full(n, -7.0, dtype=np.float32), torch.bfloat16)
    p_bits, e_bits = bits(torch.from_numpy(p_np)), bits(torch.from_numpy(e_np))
    K.ema_swap(p, e, shadow_bf16=s)
    torch.cuda.synchronize()
    assert torch.equal(bits(p), e_bits) and torch.equal(bits(e), p_bits)
    if with_shadow:
        assert torch.equal(bits(s), cast_bits(K, p))                                # vitpe_cast's rounding of the new p
        assert guards_intact(sbuf, n)
    K.ema_swap(p, e, shadow_bf16=s)
    torch.cuda.synchronize()
    assert torch.equal(bits(p), p_bits) and torch.equal(bits(e), e_bits)
    if with_shadow:
        assert torch.equal(bits(s), cast_bits(K, p)) and guards_intact(sbuf, n)
    assert guards_intact(pbuf, n) and guards_intact(ebuf, n)


def test_swap_refusals_write_nothing(K):
    from vitpe import _lib as L
    n = 1023
    p_np, e_np, _ = _inputs(n)
    pbuf, p = guarded(p_np)
    ebuf, e = guarded(e_np)
    sbuf, s = guarded(np.zeros(n, dtype=np.float32), torch.bfloat16)
    for args in ((pbuf[5:5 + n], e, None), (p, ebuf[6:6 + n], None), (p, e, sbuf[9:9 + n]), (p, e, s[:n - 1]),
                 (p, e, s.float())):
        with pytest.raises(L.VitpeError):
            K.ema_swap(args[0], args[1], shadow_bf16=args[2])
    torch.cuda.synchronize()
    assert torch.equal(bits(pbuf), bits(guarded(p_np)[0])) and torch.equal(bits(ebuf), bits(guarded(e_np)[0]))
    assert float(s.float().abs().max()) == 0.0


# ------------------------------------------------------------------------------------------ 3. - 6. TrainEngine
B = 8


def _engine(use_graph, extras=False, dt=torch.float32, **adamw):
    """A depth-2, 32 x 32 / patch-4 model (the geometry of the gradient-clipping engine tests) on a fixed batch of 8.
    adamw: optimizer arguments of TrainEngine other than the defaults (eps=...)."""
    from models.vit import VisionTransformer
    from vitpe.engine import TrainEngine
    torch.manual_seed(0)
    model = VisionTransformer(img_size=32, patch_size=4, embed_dim=192, depth=2, num_heads=6, pos_encoding="rope-axial").cuda()
    eng = TrainEngine(model, B, compute_dtype=dt, use_graph=use_graph, extras=extras, **adamw)
    g = torch.Generator().manual_seed(7)
    eng.images.copy_(torch.randn(B, 3, 32, 32, generator=g))
    eng.labels.copy_(torch.randint(0, 10, (B,), generator=g))
    return eng


def _recurrence(e0, snaps, d):
    """float64 average after every snapshot of flat_p, and the summed per-step bounds."""
    e, bound, out = e0, np.zeros_like(e0), []
    for p in snaps:
        nxt = R.ema_ref(p, e, d)
        bound = bound + R.ema_bound(p, e, nxt, d)
        e = nxt
        out.append((e, bound.copy()))
    return out


def test_engine_eager_fp32_follows_the_recurrence():
    eng = _engine(False)
    assert eng.opt.ema_decay is None and eng.opt.flat_e is None
    eng.step()                                            # one step before the average exists: hp[14] is not just zero
    eng.set_ema(0.9)
    assert eng.opt.ema_decay == 0.9 and eng.opt.ema_warmup is False
    assert eng.opt.flat_e.dtype == torch.float32 and eng.opt.flat_e.numel() == eng.n_flat and eng.opt.flat_e.data_ptr() % 16 == 0
    assert torch.equal(bits(eng.opt.flat_e), bits(eng.flat_p))
    e0, snaps = f64(eng.opt.flat_e), []
    for _ in range(3):
        eng.step()
        snaps.append(f64(eng.flat_p))
    torch.cuda.synchronize()
    hp = eng.hp.cpu().numpy()
    assert hp[5] == 4.0 and hp[14] == 1.0
    assert hp[13].tobytes() == np.float32(0.9).tobytes() == hp[15].tobytes()
    ref, bound = _recurrence(e0, snaps, hp[15])[-1]
    fig = worst(f64(eng.opt.flat_e) - ref, bound)
    moved = float(np.abs(ref - e0).max())
    print(f"eager fp32, 3 steps: worst |err| / summed bound {fig:.3f}; the average moved by up to {moved:.3e}")
    assert fig <= 1.0 and moved > 0
    assert not np.array_equal(f64(eng.opt.flat_e), snaps[-1])                 # the average, not a copy of the parameters
    # reset_ema: a copy of the parameters again, the warm-up's origin re-based
    eng.reset_ema()
    assert torch.equal(bits(eng.opt.flat_e), bits(eng.flat_p)) and float(eng.hp[14]) == 4.0


@pytest.mark.parametrize("extras", [False, True])
def test_engine_graph_replay_averages_like_the_eager_engine(extras):
    """(AdamW's eps is 1e-3 in both engines for the reason test_ema_switched_off_again_is_inert gives: at the default
    1e-8 the parameters of two runs of one engine already differ by up to 1e-5 of their largest, the atomics' order
    amplified by lr / eps, and the averages by a third of that.)"""
    eager, graph = _engine(False, extras, eps=1e-3), _engine(True, extras, eps=1e-3)
    for eng in (eager, graph):
        eng.set_ema(0.9)
        assert eng.graph_fb is None
    p0 = f64(graph.flat_p)
    after = []
    for step in range(3):
        eager.step(); graph.step()
        after.append(f64(graph.opt.flat_e))
        if step == 0:
            # the capture's warm-up (two real optimizer steps, then restored) leaves no trace: ONE application of the
            # recurrence leads from the initial copy to this step's parameters
            d = graph.hp[15].item()
            ref = R.ema_ref(f64(graph.flat_p), p0, d)
            fig = worst(after[0] - ref, R.ema_bound(f64(graph.flat_p), p0, ref, d))
            print(f"extras {extras}: first captured step, worst |err| / bound {fig:.3f}")
            assert fig <= 1.0
            assert float(graph.hp[5]) == 1.0 and float(graph.hp[14]) == 0.0
    assert graph.graph_fb is not None and eager.graph_fb is None
    assert not np.array_equal(after[1], after[0]) and not np.array_equal(after[2], after[1])    # it moves between replays
    err = rel_err(graph.opt.flat_e.cpu(), eager.opt.flat_e.cpu())
    err_p = rel_err(graph.flat_p.cpu(), eager.flat_p.cpu())
    print(f"extras {extras}: graph vs eager after 3 steps: rel err of the average {err:.3e}, of the parameters {err_p:.3e}")
    assert err < 1e-5
    for eng in (eager, graph):
        assert float(eng.hp[5]) == 3.0 and eng.hp[15].item() == float(np.float32(0.9))
    # a new decay for an enabled average is a device write: the captured graph stays
    fb = graph.graph_fb
    graph.set_ema(0.95)
    assert graph.graph_fb is fb and graph.hp[13].item() == float(np.float32(0.95))
    graph.step()
    assert graph.graph_fb is fb and float(graph.hp[5]) == 4.0 and graph.hp[15].item() == float(np.float32(0.95))
    # the warm-up switch is compiled into the launch: changing it drops the graph
    graph.set_ema(0.95, warmup=True)
    assert graph.graph_fb is None and graph.opt.ema_warmup is True
    graph.step()
    assert ulps(graph.hp[15].item(), R.warmup_decay(0.95, 5)) <= 1 and graph.hp[15].item() < 0.5
    # off: the graphs are dropped, the next step captures anew and nothing writes hp[13..15] or the former buffer
    fb, former = graph.graph_fb, graph.opt.flat_e
    kept, before = former.clone(), graph.hp.clone()
    graph.set_ema(None)
    assert graph.graph_fb is None and graph.opt.ema_decay is None and graph.opt.flat_e is None
    graph.step()
    torch.cuda.synchronize()
    assert graph.graph_fb is not None and graph.graph_fb is not fb and float(graph.hp[5]) == 6.0
    assert torch.equal(bits(graph.hp[13:16]), bits(before[13:16])) and torch.equal(bits(former), bits(kept))


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_ema_weights_swaps_the_average_in_and_restores_every_bit(dt):
    from vitpe._lib import VitpeError
    eng = _engine(True, dt=dt)
    with pytest.raises(VitpeError, match="EMA is off"):
        with eng.ema_weights():
            pass
    eng.set_ema(0.9)
    for _ in range(3):
        eng.step()
    fb = eng.graph_fb
    names = ["flat_p", "flat_e", "_shadow_flat"] + (["flat_s"] if dt == torch.bfloat16 else [])
    assert (eng.flat_s is not None) == (dt == torch.bfloat16)
    buf = lambda k: getattr(eng.opt if k == "flat_e" else eng, k)   # noqa: E731  (the average is the optimizer's)
    clones = {k: buf(k).clone() for k in names}
    ptrs = {k: buf(k).data_ptr() for k in names}
    images = eng.images.clone()
    sd_out = eng.ema_state_dict()
    params = dict(eng.model.named_parameters())
    assert list(sd_out) == list(eng.model.state_dict())
    assert any(not torch.equal(sd_out[k], params[k].data) for k in params)                  # the average, not the weights
    assert all(sd_out[k].data_ptr() != params[k].data_ptr() for k in params)                # clones

    def restored():
        torch.cuda.synchronize()
        return (all(torch.equal(bits(buf(k)), bits(clones[k])) for k in names)
                and all(buf(k).data_ptr() == ptrs[k] for k in names) and eng.opt.ema_swapped is False)

    with eng.ema_weights() as inside:
        assert inside is eng
        assert torch.equal(bits(eng.flat_p), bits(clones["flat_e"])) and torch.equal(bits(eng.opt.flat_e), bits(clones["flat_p"]))
        logits = eng.forward_only(images).clone()
        sd_in = eng.model.state_dict()
        assert list(sd_in) == list(sd_out) and all(torch.equal(bits(sd_in[k]), bits(sd_out[k])) for k in sd_out)
        sd_mid = eng.ema_state_dict()                                                      # the same values from inside
        assert all(torch.equal(bits(sd_mid[k]), bits(sd_out[k])) for k in sd_out)
        for call in (eng.step, eng.forward_backward, eng.capture, lambda: eng.set_ema(0.5),
                     lambda: eng.step(images, eng.labels.clone())):
            with pytest.raises(VitpeError, match="inside ema_weights"):
                call()
        with pytest.raises(VitpeError, match="inside ema_weights"):
            with eng.ema_weights():
                pass
    assert restored()
    # a second, fresh engine of the same dtype whose model loaded the average computes the same logits, bit for bit
    other = _engine(False, dt=dt)
    other.model.load_state_dict(sd_out)                   # (the engine's hook re-derives its shadows)
    want = other.forward_only(images).clone()
    torch.cuda.synchronize()
    assert torch.equal(bits(logits), bits(want))
    assert not torch.equal(bits(logits), bits(eng.forward_only(images)))                    # ... and not the weights' own
    # load_ema_state_dict is ema_state_dict's inverse
    other.set_ema(0.5)
    other.opt.flat_e.mul_(2.0)                                # (the padding between parameters stays zero, as in eng.opt.flat_e)
    p_before = other.flat_p.clone()
    other.load_ema_state_dict(sd_out)
    assert torch.equal(bits(other.opt.flat_e), bits(eng.opt.flat_e)) and torch.equal(bits(other.flat_p), bits(p_before))
    with pytest.raises(VitpeError, match="load_ema_state_dict"):
        other.load_ema_state_dict({k: v for k, v in sd_out.items() if k != "cls_token"})
    # an exception raised inside still restores
    with pytest.raises(ZeroDivisionError):
        with eng.ema_weights():
            assert eng.opt.ema_swapped is True
            1 / 0
    assert restored()
    # ... and training goes on through the same captured graph
    eng.step()
    torch.cuda.synchronize()
    assert eng.graph_fb is fb and float(eng.hp[5]) == 4.0
    assert not torch.equal(bits(eng.opt.flat_e), bits(clones["flat_e"]))


def test_ema_switched_off_again_is_inert():
    """Two engines from the same seed, one never touched, one with the average switched on and off again, three captured
    steps each.  hp[:13] (no gradient enters it) is compared bit for bit.  No geometry of this engine has a backward with a
    fixed summation order (the weight gradients, the LayerNorm and head parameter gradients are combined with fp32
    atomics), so two runs of the SAME untouched engine differ in the last bits: flat_p, flat_m, flat_v are compared with
    the tolerance the gradient-clipping replay test uses for parameters (rel_err < 1e-5).

    AdamW's eps is 1e-3 in both engines, not the default 1e-8.  The first steps move a parameter by
    lr g / (|g| + eps), whose slope in g is lr / eps where |g| << eps: 1e5 at the defaults, so an element whose gradient
    is nothing but the atomics' order (of the order of 1e-11 here, going by the size of the steps) moves by multiples
    of 1e-6 from run to run -- measured on two
    untouched engines at the defaults: flat_p rel_err 1.0e-6 .. 8.3e-6 over 12 pairs, in steps of 1.04e-6, i.e. the
    comparison would sit inside its own noise.  With eps = 1e-3 the slope is at most 1 and what is left is the relative
    noise of ordinary gradients (measured the same way: flat_p 1.1e-8 .. 1.2e-7, flat_m and flat_v up to 2.3e-7).  The
    optimizer alone has a fixed order: on identical gradients the two engines' updates
    are compared bit for bit at the end."""
    plain, toggled = _engine(True, eps=1e-3), _engine(True, eps=1e-3)
    assert float(plain.hp[3]) == float(np.float32(1e-3))
    toggled.set_ema(0.99)
    former = toggled.opt.flat_e
    toggled.set_ema(None)
    assert toggled.opt.flat_e is None and toggled.opt.ema_decay is None
    kept = former.clone()
    for _ in range(3):
        plain.step(); toggled.step()
    torch.cuda.synchronize()
    assert torch.equal(bits(plain.hp[:13]), bits(toggled.hp[:13])) and float(plain.hp[5]) == 3.0
    assert toggled.hp[13].item() == float(np.float32(0.99)) and float(toggled.hp[15]) == 0.0   # written once, by set_ema
    assert torch.equal(bits(former), bits(kept))
    for name in ("flat_p", "flat_m", "flat_v"):
        err = rel_err(getattr(toggled, name).cpu(), getattr(plain, name).cpu())
        print(f"{name}: toggled vs untouched after 3 captured steps, rel err {err:.3e}")
        assert err < 1e-5, name
    # identical gradients in, the optimizer's launches alone: bit-equal state out
    for name in ("flat_p", "flat_m", "flat_v", "hp"):
        getattr(toggled, name)[:13 if name == "hp" else None].copy_(getattr(plain, name)[:13 if name == "hp" else None])
    plain.forward_backward()
    toggled.flat_g.copy_(plain.flat_g)
    toggled.refresh_shadows()
    plain._optimizer(); toggled._optimizer()
    torch.cuda.synchronize()
    for name in ("flat_p", "flat_m", "flat_v", "flat_g", "_shadow_flat"):
        assert torch.equal(bits(getattr(plain, name)), bits(getattr(toggled, name))), name
    assert torch.equal(bits(plain.hp[:13]), bits(toggled.hp[:13])) and float(plain.hp[5]) == 4.0


# ------------------------------------------------------------------------------------------ 7. train.py
def test_train_py_model_ema_evaluates_and_checkpoints_the_average(tmp_path, monkeypatch):
    import train as T
    from models.vit import VisionTransformer
    from vitpe.engine import TrainEngine
    seen = []
    real = TrainEngine.set_ema

    def spy(self, decay, warmup=False):
        seen.append((self, decay, warmup))
        return real(self, decay, warmup=warmup)

    monkeypatch.setattr(TrainEngine, "set_ema", spy)
    common = ["--dataset", "mnist", "--pos_encoding", "rope-axial", "--batch_size", "16", "--epochs", "1", "--synthetic",
              "--steps_per_epoch", "3", "--embed_dim", "96", "--depth", "2", "--num_heads", "3", "--clip_grad", "1.0"]
    T.main(common + ["--model_ema", "0.9", "--model_ema_warmup", "--log_dir", str(tmp_path / "logs"), "--ckpt_dir",
                     str(tmp_path / "ckpt")])
    assert len(seen) == 1 and seen[0][1:] == (0.9, True)
    eng = seen[0][0]
    assert eng.opt.flat_e is not None and eng.opt.flat_e.numel() == eng.n_flat and eng.opt.ema_decay == 0.9 and eng.opt.ema_warmup
    assert eng.opt.ema_swapped is False and float(eng.hp[5]) == 3.0 and float(eng.hp[14]) == 0.0
    assert ulps(eng.hp[15].item(), R.warmup_decay(0.9, 3)) <= 1
    assert not torch.equal(bits(eng.opt.flat_e), bits(eng.flat_p))
    logs = list((tmp_path / "logs").glob("mnist_rope-axial_*.csv"))
    assert len(logs) == 1
    rows = list(csv.reader(logs[0].read_text().splitlines()))
    assert rows[0] == ["epoch", "train_loss", "train_acc", "test_loss", "test_acc", "best_acc", "ema_test_loss", "ema_test_acc"]
    assert len(rows) == 2 and len(rows[1]) == 8 and np.isfinite(float(rows[1][6])) and 0.0 <= float(rows[1][7]) <= 100.0
    ckpt = tmp_path / "ckpt" / "mnist_rope-axial_best_ema.pth"
    assert ckpt.exists()
    fresh = VisionTransformer(img_size=32, patch_size=4, in_chans=1, num_classes=10, embed_dim=96, depth=2, num_heads=3,
                              pos_encoding="rope-axial")
    sd = torch.load(ckpt, map_location="cpu")
    assert fresh.load_state_dict(sd, strict=True) is not None
    want = eng.ema_state_dict()                           # what was saved is the average, not the weights
    assert all(torch.equal(bits(sd[k]), bits(want[k])) for k in want)
    # without the flag: the reference's six columns, no EMA checkpoint, set_ema never called
    T.main(common + ["--log_dir", str(tmp_path / "logs2"), "--ckpt_dir", str(tmp_path / "ckpt2")])
    assert len(seen) == 1
    logs = list((tmp_path / "logs2").glob("mnist_rope-axial_*.csv"))
    assert len(logs) == 1
    assert logs[0].read_text().splitlines()[0] == "epoch,train_loss,train_acc,test_loss,test_acc,best_acc"
    assert not list((tmp_path / "ckpt2").glob("*ema*"))
