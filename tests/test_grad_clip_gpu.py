"""Gradient clipping by global norm inside the train step: vitpe_grad_clip (grad_sqnorm_kernel + grad_clip_finalize_kernel,
csrc/optim.hip) and the hp[9] route of adamw_kernel against the float64 restatements of tests/grad_clip_ref.py and
tests/train_state_ref.py, then TrainEngine.set_grad_clip / grad_norm eager, in captured graphs, on the extras route and
from train.py --clip_grad.

Tolerance of the norm (grad_clip_ref.norm_bound, derived from the kernel as built, not from its results; U = 2^-24): the
grid is min(1024, ceil(n / 4096)) workgroups of 256 threads, float4 i of the aligned body goes to thread i % (256 nb), so
one per-component running sum takes ceil(nvec / (256 nb)) <= 4 fma's at every n of this file (one rounding each), + 1 for
a head / tail element, + 2 (components) + 6 (wave butterfly) + 2 (four waves); the workgroups are summed in fp64.  All
summands are >= 0, so the sum of squares is within chain * U relative: chain <= 15, halved by the square root, + U for the
one rounding of gs * sqrt(.) to fp32: <= 8.5 U = 5.1e-7 relative, under the 1e-5 ceiling (a grid rule that let a thread
run hundreds of additions in a row would break it)."""
import numpy as np
import pytest
import torch

import grad_clip_ref as R
import train_state_ref as TS
from conftest import rel_err
from test_kernels_gpu import K, dev  # noqa: F401  (K: the kernels fixture)
from test_train_state_gpu import bits, f64, worst

pytestmark = pytest.mark.gpu

GUARD = 1e3   # what sits in front of and behind the vector on the device: reading it would show in every norm


def ulps(got, want):
    want = np.float32(want)
    return abs(float(np.float32(got)) - float(want)) / float(np.spacing(np.abs(want)))


def _hp(max_norm, gs=R.GS):
    hp = TS.adamw_hp(gs=gs)
    hp[9:12] = -5.0        # what the call must overwrite
    hp[12] = max_norm
    return hp


def _on_device(g_np, misaligned):
    """g_np on the device at `misaligned` floats past a 256-byte boundary, guard values around it."""
    n = g_np.shape[0]
    buf = torch.full((n + 8,), GUARD, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[misaligned:misaligned + n]
    view.copy_(torch.from_numpy(g_np))
    assert view.data_ptr() % 16 == 4 * misaligned
    return view


_REFS = {}


def _refs(n):
    """[(marks, fp32 input, float64 norm at gs = GS)] of every run at size n, computed once for both alignments."""
    if n not in _REFS:
        base = R.norm_inputs(n)
        out = []
        for marks in R.mark_groups(n):
            g = R.with_marks(base, marks)
            out.append((marks, g, R.clip_ref(g, R.GS, 1.0)[0]))
        _REFS[n] = out
    return _REFS[n]


# ------------------------------------------------------------------------------------------ 1. the norm kernel
@pytest.mark.parametrize("misaligned", [0, 1])
@pytest.mark.parametrize("n", R.SIZES)
def test_norm_and_coefficient_against_the_float64_reference(K, n, misaligned):
    """Every size at an aligned base pointer and one element past it; the bulk alone, then runs of <= 8 marked elements
    (the last index, the first indices past the head and the 4-element boundaries where the kernel changes path, the
    first index past every 4096-element boundary), each >= 10 % of the sum.  hp[10] against clip_ref within
    norm_bound(n); hp[11] and hp[9] against the formula on the device's own hp[10], 2 ulp; max_norm alternates between
    half the norm (clipping) and four times it (coef == 1 and hp[9] == hp[8] bit for bit)."""
    bound = R.norm_bound(n, misaligned)
    assert bound <= 1e-5
    nb = K.grad_clip_blocks(n)
    assert nb == min(1024, -(-n // 4096))
    worst_fig = 0.0
    for run, (marks, g_np, norm_ref) in enumerate(_refs(n)):
        factor = R.FACTORS[run % 2]
        g = _on_device(g_np, misaligned)
        hp = dev(torch.from_numpy(_hp(factor * norm_ref)))
        hp_in = hp.cpu().numpy().copy()
        partial = torch.full((nb + 2,), GUARD, dtype=torch.float32, device="cuda")
        K.grad_clip(g, hp, partial)
        out = hp.cpu().numpy()
        assert float(partial[nb]) == GUARD and float(partial[nb + 1]) == GUARD
        assert torch.equal(bits(g), bits(torch.from_numpy(g_np)))                       # the gradient itself is not scaled
        assert np.array_equal(out[:9], hp_in[:9]) and np.array_equal(out[12:], hp_in[12:])
        fig = abs(float(out[10]) - norm_ref) / norm_ref / bound
        worst_fig = max(worst_fig, fig)
        assert fig <= 1.0, (n, misaligned, run, marks, float(out[10]), norm_ref)
        coef = R.coef_from_norm(out[10], out[12])
        assert ulps(out[11], coef) <= 2, (run, out[11], coef)
        assert ulps(out[9], np.float32(out[8]) * np.float32(out[11])) <= 2
        if factor > 1:
            assert out[11] == np.float32(1.0) and out[9].tobytes() == out[8].tobytes()
        else:
            assert abs(float(out[11]) - 0.5) <= 0.5 * (bound + 1e-6 / norm_ref + 4 * R.U)
    print(f"n {n} misaligned {misaligned}: {len(_refs(n))} runs, worst |err| / bound {worst_fig:.3f} (bound {bound:.2e})")


def test_empty_gradient_and_the_refusals(K):
    from vitpe import _lib as L
    hp = dev(torch.from_numpy(_hp(1e-9)))
    K.grad_clip(torch.empty(0, dtype=torch.float32, device="cuda"), hp, torch.empty(0, dtype=torch.float32, device="cuda"))
    out = hp.cpu().numpy()
    assert out[10] == 0.0 and out[11] == 1.0 and out[9].tobytes() == out[8].tobytes()
    g = _on_device(R.norm_inputs(4099), 0)
    with pytest.raises(L.VitpeError):                     # 2 workgroups, 1 partial
        K.grad_clip(g, hp, torch.zeros(1, device="cuda"))
    with pytest.raises(L.VitpeError):
        K.grad_clip(g, hp[:8], torch.zeros(2, device="cuda"))
    with pytest.raises(L.VitpeError):
        K.grad_clip(g.cpu(), hp, torch.zeros(2, device="cuda"))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ 2. determinism
def test_two_calls_agree_bit_for_bit(K):
    n = 2 ** 20 + 3
    marks, g_np, norm_ref = _refs(n)[1]
    g = _on_device(g_np, 1)
    outs = []
    for fill in (0.0, GUARD):
        hp = dev(torch.from_numpy(_hp(0.5 * norm_ref)))
        partial = torch.full((K.grad_clip_blocks(n),), fill, dtype=torch.float32, device="cuda")
        K.grad_clip(g, hp, partial)
        outs.append((hp.cpu(), partial.cpu()))
    assert torch.equal(bits(outs[0][0][9:12]), bits(outs[1][0][9:12]))
    assert torch.equal(bits(outs[0][1]), bits(outs[1][1]))                              # every workgroup's partial as well


# ------------------------------------------------------------------------------------------ 3. AdamW bit 2
def _adamw_run(K, p0_np, g_np, hp_np, shadow=True, **flags):
    p, g, hp = dev(torch.from_numpy(p0_np.copy())), dev(torch.from_numpy(g_np.copy())), dev(torch.from_numpy(hp_np.copy()))
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    sh = torch.full((p0_np.shape[0],), -7.0, dtype=torch.bfloat16, device="cuda") if shadow else None
    K.adamw_step(p, g, m, v, hp, shadow_bf16=sh, **flags)
    torch.cuda.synchronize()
    return p, m, v, sh, g, hp


def test_adamw_takes_its_scale_from_slot_9_only_when_asked(K):
    n = 10007
    p0_np, g_np = TS.adamw_inputs(n, seed=4)
    hp_np = TS.adamw_hp()
    # hp[9] = hp[8] * 0.37: the update of a gradient scaled by THAT
    hp_c = hp_np.copy()
    hp_c[9] = np.float32(hp_c[8] * np.float32(0.37))
    p, m, v, sh, g, hp = _adamw_run(K, p0_np, g_np, hp_c, zero_grad=True, clipped=True)
    assert float(hp[5]) == 1.0 and float(g.abs().max()) == 0.0
    assert np.array_equal(hp.cpu().numpy()[8:], hp_c[8:])
    hp_ref = hp_c.copy()
    hp_ref[8] = hp_c[9]
    p_ref, m_ref, v_ref, d_ref = TS.adamw_ref(p0_np, g_np, 0 * p0_np, 0 * p0_np, hp_ref, float(hp[6]), float(hp[7]))
    bp, bm, bv = TS.adamw_bounds(p0_np, p_ref, m_ref, v_ref, d_ref)
    fig = (worst(f64(p) - p_ref, bp), worst(f64(m) - m_ref, bm), worst(f64(v) - v_ref, bv))
    print(f"adamw from hp[9]: worst |err| / bound  p {fig[0]:.3f}  m {fig[1]:.3f}  v {fig[2]:.3f}")
    assert max(fig) <= 1.0, fig
    assert torch.equal(bits(sh), bits(p.to(torch.bfloat16)))
    # ... and it is not the update of hp[8]
    p8, m8, _, _, _, _ = _adamw_run(K, p0_np, g_np, hp_c, zero_grad=True)
    assert worst(f64(m8) - m_ref, bm) > 10
    # hp[9] == hp[8]: zero_grad = 5 is zero_grad = 1 bit for bit
    hp_e = hp_np.copy()
    hp_e[9] = hp_e[8]
    a = _adamw_run(K, p0_np, g_np, hp_e, zero_grad=True, clipped=True)
    b = _adamw_run(K, p0_np, g_np, hp_e, zero_grad=True)
    for x, y in zip(a[:4], b[:4]):
        assert torch.equal(bits(x), bits(y))
    # zero_grad = 1 and 3 never read hp[9]: a sentinel there changes nothing
    hp_s = hp_np.copy()
    hp_s[9] = np.float32(-123.0)
    for ticked in (False, True):
        base_hp, sent_hp = hp_np.copy(), hp_s.copy()
        if ticked:
            for h in (base_hp, sent_hp):
                h[5], h[6], h[7] = 7.0, 0.5, 0.25
        a = _adamw_run(K, p0_np, g_np, base_hp, zero_grad=True, ticked=ticked)
        b = _adamw_run(K, p0_np, g_np, sent_hp, zero_grad=True, ticked=ticked)
        for x, y in zip(a[:4], b[:4]):
            assert torch.equal(bits(x), bits(y))
        assert float(b[5][9]) == -123.0


# ------------------------------------------------------------------------------------------ 4. / 5. TrainEngine
B = 8


def _engine(use_graph, extras=False, dt=torch.float32):
    """The depth-2, 32 x 32 / patch-4 model of tests/test_augment_gpu.py::_engine on a fixed random batch of 8."""
    from models.vit import VisionTransformer
    from vitpe.engine import TrainEngine
    torch.manual_seed(0)
    model = VisionTransformer(img_size=32, patch_size=4, embed_dim=192, depth=2, num_heads=6, pos_encoding="rope-axial").cuda()
    eng = TrainEngine(model, B, compute_dtype=dt, use_graph=use_graph, extras=extras)
    g = torch.Generator().manual_seed(7)
    eng.images.copy_(torch.randn(B, 3, 32, 32, generator=g))
    eng.labels.copy_(torch.randint(0, 10, (B,), generator=g))
    return eng


def _flat_bound(eng):
    return R.norm_bound(eng.n_flat, (eng.flat_g.data_ptr() % 16) // 4)


def _floors(bm, bv, m_ref, v_ref):
    """adamw_bounds are relative and hold for normal numbers; a real gradient also has elements whose (1 - b2) g^2 (or
    (1 - b1) g) is subnormal, where one rounding is half a subnormal spacing (2^-150) whatever the value: the same counts
    of roundings (m 4, v 6) at that absolute size there."""
    tiny, sub = 2.0 ** -126, 2.0 ** -150
    return (np.where(np.abs(m_ref) < tiny, np.maximum(bm, 4 * sub), bm), np.where(np.abs(v_ref) < tiny, np.maximum(bv, 6 * sub), bv))


def test_engine_eager_fp32_clips_to_half_the_norm():
    from vitpe._lib import VitpeError
    eng = _engine(False)
    with pytest.raises(VitpeError, match="clipping is off"):
        eng.grad_norm()
    eng.forward_backward()
    g = eng.flat_g.clone()
    gs = float(eng.hp[8])
    assert gs == 1.0
    norm_ref, _ = R.clip_ref(f64(g), gs, 1.0)
    assert norm_ref > 0
    eng.set_grad_clip(0.5 * norm_ref)
    assert eng.opt._clip_partial.numel() == K_blocks(eng.n_flat)
    p0, m0, v0 = f64(eng.flat_p), f64(eng.flat_m), f64(eng.flat_v)
    eng._optimizer()
    torch.cuda.synchronize()
    hp = eng.hp.cpu().numpy()
    bound = _flat_bound(eng)
    fig = abs(eng.grad_norm() - norm_ref) / norm_ref / bound
    print(f"engine: n_flat {eng.n_flat}, norm {norm_ref:.6g}, |err| / bound {fig:.3f} (bound {bound:.2e})")
    assert fig <= 1.0 and eng.grad_norm() == float(hp[10])
    assert ulps(hp[11], R.coef_from_norm(hp[10], hp[12])) <= 2
    assert abs(float(hp[11]) - 0.5) <= 0.5 * (bound + 1e-6 / norm_ref + 4 * R.U)
    assert ulps(hp[9], np.float32(hp[8]) * np.float32(hp[11])) <= 2
    assert hp[5] == 1.0 and float(eng.flat_g.abs().max()) == 0.0
    hp_ref = hp.copy()
    hp_ref[8] = hp[9]                                     # the scale the device used
    p_ref, m_ref, v_ref, d_ref = TS.adamw_ref(p0, f64(g), m0, v0, hp_ref, float(hp[6]), float(hp[7]))
    bp, bm, bv = TS.adamw_bounds(p0, p_ref, m_ref, v_ref, d_ref)
    bm, bv = _floors(bm, bv, m_ref, v_ref)
    figs = (worst(f64(eng.flat_p) - p_ref, bp), worst(f64(eng.flat_m) - m_ref, bm), worst(f64(eng.flat_v) - v_ref, bv))
    print(f"engine AdamW after the clip: worst |err| / bound  p {figs[0]:.3f}  m {figs[1]:.3f}  v {figs[2]:.3f}")
    assert max(figs) <= 1.0, figs
    # the same state, a max_norm nothing reaches: the unclipped scale, bit for bit
    eng2 = _engine(False)
    eng2.forward_backward()
    eng2.set_grad_clip(1e30)
    eng2._optimizer()
    hp2 = eng2.hp.cpu().numpy()
    assert hp2[11] == np.float32(1.0) and hp2[9].tobytes() == hp2[8].tobytes()
    assert abs(float(hp2[10]) - norm_ref) <= 1e-4 * norm_ref        # (its gradient is the first engine's up to the atomics' order)


def K_blocks(n):
    from vitpe import kernels
    return kernels.grad_clip_blocks(n)


@pytest.mark.parametrize("extras", [False, True])
def test_engine_graph_replay_clips_like_the_eager_engine(extras):
    from vitpe._lib import VitpeError
    eager, graph = _engine(False, extras), _engine(True, extras)
    eager.forward_backward()                              # a look at the size of the gradient, then undone
    torch.cuda.synchronize()
    norm0 = float(np.linalg.norm(f64(eager.flat_g)))
    eager.flat_g.zero_()
    max_norm = 0.5 * norm0
    norms = []
    for eng in (eager, graph):
        eng.set_grad_clip(max_norm)
        assert eng.opt.clip_max_norm == max_norm and eng.graph_fb is None
    for step in range(3):
        eager.step(); graph.step()
        norms.append((eager.grad_norm(), graph.grad_norm()))
        if step == 0:
            assert abs(norms[0][1] - norm0) <= 1e-4 * norm0 and abs(float(graph.hp[11]) - 0.5) < 1e-3
    assert graph.graph_fb is not None and eager.graph_fb is None
    assert norms[1][1] != norms[0][1] and norms[2][1] != norms[1][1]      # the replay recomputes it
    err = rel_err(graph.flat_p.cpu(), eager.flat_p.cpu())
    print(f"extras {extras}: norms (eager, graph) {norms}; parameters graph vs eager after 3 steps: rel err {err:.3e}")
    assert err < 1e-5
    for eng in (eager, graph):
        assert float(eng.hp[5]) == 3.0 and float(eng.flat_g.abs().max()) == 0.0
    # a new value for an enabled clip is a device write: the captured graph stays
    fb = graph.graph_fb
    graph.set_grad_clip(2.0 * max_norm)
    assert graph.graph_fb is fb and float(graph.hp[12]) == float(np.float32(2.0 * max_norm))
    graph.step()
    assert float(graph.hp[5]) == 4.0 and graph.graph_fb is fb
    assert ulps(float(graph.hp[11]), R.coef_from_norm(graph.hp[10].item(), graph.hp[12].item())) <= 2
    # off: the graphs are dropped, the next step captures anew and nothing writes hp[9..11] any more
    graph.set_grad_clip(None)
    assert graph.graph_fb is None and graph.opt.clip_max_norm is None
    before = graph.hp.cpu()
    graph.step()
    torch.cuda.synchronize()
    assert graph.graph_fb is not None and graph.graph_fb is not fb
    assert float(graph.hp[5]) == 5.0 and float(graph.flat_g.abs().max()) == 0.0
    assert torch.equal(bits(graph.hp[9:13]), bits(before[9:13]))
    with pytest.raises(VitpeError, match="clipping is off"):
        graph.grad_norm()


# ------------------------------------------------------------------------------------------ 6. train.py
def test_train_py_clip_grad_reaches_the_engine(tmp_path, monkeypatch):
    import train as T
    from vitpe.engine import TrainEngine
    seen = []
    real = TrainEngine.set_grad_clip

    def spy(self, max_norm):
        seen.append((self, max_norm))
        return real(self, max_norm)

    monkeypatch.setattr(TrainEngine, "set_grad_clip", spy)
    T.main(["--dataset", "mnist", "--pos_encoding", "rope-axial", "--batch_size", "16", "--epochs", "1", "--synthetic",
            "--steps_per_epoch", "3", "--embed_dim", "96", "--depth", "2", "--num_heads", "3", "--clip_grad", "1.0",
            "--log_dir", str(tmp_path / "logs"), "--ckpt_dir", str(tmp_path / "ckpt")])
    assert len(seen) == 1 and seen[0][1] == 1.0
    eng = seen[0][0]
    assert eng.opt.clip_max_norm == 1.0 and float(eng.hp[12]) == 1.0 and float(eng.hp[5]) == 3.0
    assert eng.grad_norm() > 0.0 and 0.0 < float(eng.hp[11]) <= 1.0
    logs = list((tmp_path / "logs").glob("mnist_rope-axial_*.csv"))
    assert len(logs) == 1
    assert logs[0].read_text().splitlines()[0] == "epoch,train_loss,train_acc,test_loss,test_acc,best_acc"
