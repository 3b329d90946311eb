"""The references of tests/train_state_ref.py are right and the AdamW input set has teeth -- shown without a GPU, so that
tests/test_train_state_gpu.py compares the kernels with something already checked."""
import numpy as np
import pytest
import torch

import train_state_ref as R

STEPS = 3


def _torch_adamw(p0, g, hp, steps):
    h = hp.astype(np.float64)
    p = torch.nn.Parameter(torch.from_numpy(p0.astype(np.float64)))
    opt = torch.optim.AdamW([p], lr=h[0], betas=(h[1], h[2]), eps=h[3], weight_decay=h[4])
    out = []
    for t in range(steps):
        p.grad = torch.from_numpy(g.astype(np.float64) * (t + 1) * h[8])   # torch sees the scaled gradient
        opt.step()
        st = opt.state[p]
        out.append((p.detach().numpy().copy(), st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy()))
    return out


def test_adamw_ref_matches_torch_adamw_in_float64():
    """Three steps with weight decay and a gradient scale of 0.25 on the GPU test's gradients: 1e-12 relative per element
    on p, m and v (the two differ only in float64 roundings: torch forms m by lerp).  p0 is drawn from +-[0.5, 2] here:
    with the input set's p0 = +-1e-3 the first update (+-lr) cancels p0 to 5e-8 and a per-element relative figure on p
    measures that cancellation (4e-12), not the two formulas."""
    _, g = R.adamw_inputs(4099, seed=3)
    rng = np.random.default_rng(4)
    p0 = (rng.uniform(0.5, 2.0, g.size) * rng.choice([-1.0, 1.0], size=g.size)).astype(np.float32)
    hp = R.adamw_hp()
    h = hp.astype(np.float64)
    want = _torch_adamw(p0, g, hp, STEPS)
    p, m, v = p0.astype(np.float64), np.zeros(p0.size), np.zeros(p0.size)
    for t in range(STEPS):
        p, m, v, _ = R.adamw_ref(p, g.astype(np.float64) * (t + 1), m, v, hp, 1 - h[1] ** (t + 1), 1 - h[2] ** (t + 1))
        for mine, ref in zip((p, m, v), want[t]):
            assert np.all(np.abs(mine - ref) <= 1e-12 * np.abs(ref)), t
    assert h[4] != 0 and h[8] == 0.25 and np.abs(p - p0).max() > 0


def test_adamw_input_set_is_what_the_issue_asks_for():
    p0, g = R.adamw_inputs(2 * 4096 * 256 + 7)
    a = np.abs(g[g != 0])
    assert a.min() >= 1e-15 and a.min() < 1.1e-15 and a.max() == 1.0
    assert (g == 0).sum() >= g.size // 17 and (g > 0).any() and (g < 0).any()
    assert set(np.unique(p0).tolist()) == {0.0, float(np.float32(1e-3)), -float(np.float32(1e-3)), 1.0, -1.0}
    hp = R.adamw_hp()
    gi = a.min() * hp[8]
    assert np.float32(1 - hp[2]) * gi * gi >= np.finfo(np.float32).tiny      # (1 - b2) gi^2 stays a normal number
    for val in np.unique(p0):                                                 # every p0 meets exact zeros and both signs
        sel = p0 == val
        assert (g[sel] == 0).any() and (g[sel] > 0).any() and (g[sel] < 0).any()
    # the last 7 elements (the ragged tail of the launch) are not all trivial
    assert np.count_nonzero(g[-7:]) >= 5


@pytest.mark.parametrize("variant", ["eps_in_bc", "l2_decay", "no_bc2", "scale_late"])
def test_adamw_input_set_tells_each_wrong_update_from_the_right_one(variant):
    """eps inside the bias correction, L2 decay added to the gradient, no second bias correction, the gradient scale
    applied after the moments: on the GPU test's inputs each of them leaves the bound the kernel is held to (section 3:
    4U |p0| + 16U |delta|) by at least 10x on some element of p, in every one of the three steps."""
    p0, g = R.adamw_inputs(20011, seed=5)
    hp = R.adamw_hp()
    h = hp.astype(np.float64)
    p, m, v = p0.astype(np.float64), np.zeros(p0.size), np.zeros(p0.size)
    for t in range(STEPS):
        gt = g.astype(np.float64) * (t + 1)
        bc1, bc2 = 1 - h[1] ** (t + 1), 1 - h[2] ** (t + 1)
        pr, mr, vr, dr = R.adamw_ref(p, gt, m, v, hp, bc1, bc2)
        pw, _, _, _ = R.adamw_ref(p, gt, m, v, hp, bc1, bc2, variant=variant)
        bp, _, _ = R.adamw_bounds(p, pr, mr, vr, dr)
        moved = np.abs(pw - pr) > 0
        assert moved.any() and float((np.abs(pw - pr)[moved] / bp[moved]).max()) >= 10.0, (variant, t)
        p, m, v = pr.astype(np.float32).astype(np.float64), mr.astype(np.float32).astype(np.float64), \
            vr.astype(np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------ weight copies
def _all_shadows():
    seen = []
    for (Rr, C, kind, hd, kind2, hd2) in R.SHADOW_CASES:
        seen.append((kind, Rr, C, hd))
        if kind2 >= 0:
            seen.append((kind2, Rr, C, hd2))
    # the engines' shapes (tests/test_train_state_gpu.py: D = 192 / hidden 768 at hd 32, D = 128 / hidden 512 at hd 64)
    seen += [(0, 576, 192, 0), (1, 576, 192, 32), (6, 576, 192, 32), (4, 576, 192, 64), (2, 192, 192, 192), (5, 192, 192, 192),
             (3, 768, 192, 192), (5, 768, 192, 32), (3, 192, 768, 32), (5, 192, 768, 192), (0, 768, 192, 0), (0, 192, 768, 0),
             (0, 384, 128, 0), (2, 384, 128, 64), (0, 128, 128, 0), (0, 512, 128, 0), (0, 128, 512, 0)]
    return sorted(set(seen))


def test_shadow_cases_reach_every_kind_and_every_second_kind():
    firsts = {c[2] for c in R.SHADOW_CASES}
    seconds = {c[4] for c in R.SHADOW_CASES}
    assert firsts == {0, 1, 2, 3, 6} and seconds == {-1, 0, 2, 4, 5}
    assert {k for k, *_ in _all_shadows()} == set(range(7))
    assert (192, 64, 0, 0, 2, 64) in R.SHADOW_CASES          # the ViT-B pair
    assert any(r % 32 and c % 32 for r, c, *_ in R.SHADOW_CASES)   # ragged tiles


@pytest.mark.parametrize("kind,Rr,C,hd", _all_shadows())
def test_shadow_ref_is_a_bijection(kind, Rr, C, hd):
    """arange through shadow_ref: every source element appears exactly once (kind 6 with the q scale switched off, and with
    it on exactly the q rows carry the factor)."""
    w = np.arange(Rr * C, dtype=np.float32).reshape(Rr, C)
    out = R.shadow_ref(kind, w, hd, qscale=1.0)
    assert out.dtype == np.float32 and out.shape == (Rr * C,)
    assert np.array_equal(np.sort(out), w.reshape(-1))
    assert np.array_equal(out, R.shadow_index(kind, Rr, C, hd).astype(np.float32))
    if kind == 6:
        idx = R.shadow_index(6, Rr, C, hd)
        scaled = R.shadow_ref(6, w + 1, hd)
        q = idx // C < C
        assert q.sum() == C * C
        assert np.array_equal(scaled[~q], (w + 1).reshape(-1)[idx[~q]])
        assert np.array_equal(scaled[q], (w + 1).reshape(-1)[idx[q]] * R.wide_qscale(hd))
        assert abs(float(R.wide_qscale(32)) - 1.4426950408889634 / np.sqrt(32.0)) < 2e-8


def test_shadow_ref_spot_values_from_the_header_definitions():
    """A few elements written out by hand from include/vitpe.h, so that the gathers above are not only self-consistent."""
    w = np.arange(192 * 64, dtype=np.float32).reshape(192, 64)
    W = lambda r, c: float(r * 64 + c)   # noqa: E731
    t = R.shadow_ref(0, w, 0)
    assert t[5 * 192 + 7] == W(7, 5)
    # kind 1, D = 64, hd = 32 (H = 2, NT = 2, KS = 2): block (h=1, mat=2, nt=1, ks=1), lane 16 g + cc = 16 * 3 + 5, e = 6
    blk = ((1 * 3 + 2) * 2 + 1) * 2 + 1
    pk = R.shadow_ref(1, w, 32)
    assert pk[(blk * 64 + 16 * 3 + 5) * 8 + 6] == W(2 * 64 + 1 * 32 + 16 * 1 + 5, 32 * 1 + 8 * 3 + 6)
    # kind 6, D = 64 (S = 4): block ((h=1) * 3 + mat=1) * 4 + s=3, lane r + 32 hh = 9 + 32, element j = 2 (a k row: no scale)
    blk = (1 * 3 + 1) * 4 + 3
    wide = R.shadow_ref(6, w, 32)
    assert wide[(blk * 64 + 9 + 32) * 8 + 2] == W(1 * 64 + 32 * 1 + 9, 16 * 3 + 8 * 1 + 2)
    # kind 2 (phi 0) and 3 (phi 1) at chunk 64 of [192, 64]: fragment (kc=0, nt=7, ks=1), lane 16 * 2 + 11, element 5
    frag = (0 * 12 + 7) * 2 + 1
    assert R.shadow_ref(2, w, 64)[(frag * 64 + 16 * 2 + 11) * 8 + 5] == W(16 * 7 + 11, 32 * 1 + 8 * 2 + 5)
    assert R.shadow_ref(3, w, 64)[(frag * 64 + 16 * 2 + 11) * 8 + 5] == W(16 * 7 + 11, 32 * 1 + 16 + 4 * 2 + 5 - 4)
    assert R.shadow_ref(3, w, 64)[(frag * 64 + 16 * 2 + 11) * 8 + 1] == W(16 * 7 + 11, 32 * 1 + 4 * 2 + 1)


@pytest.mark.parametrize("kind,Rr,C,hd", [s for s in _all_shadows() if s[0] in (4, 5)])
def test_transposed_frag_packs_are_the_frag_packs_of_the_transpose(kind, Rr, C, hd):
    w = np.random.default_rng(1).standard_normal((Rr, C)).astype(np.float32)
    assert np.array_equal(R.shadow_ref(kind, w, hd), R.shadow_ref(kind - 2, np.ascontiguousarray(w.T), hd))


@pytest.mark.parametrize("kind,Rr,C,hd", [s for s in _all_shadows() if s[0] in (2, 3, 4, 5)])
def test_a_wrong_k_chunk_or_a_swapped_phi_changes_the_frag_pack(kind, Rr, C, hd):
    w = np.random.default_rng(2).standard_normal((Rr, C)).astype(np.float32)
    ref = R.shadow_ref(kind, w, hd)
    assert not np.array_equal(ref, R.shadow_ref(kind ^ 1, w, hd))           # phi swapped
    K = Rr if kind >= 4 else C                                               # the packed matrix's k extent
    others = [k for k in (32, 64, 96, 128, 192, 384, 768) if k != hd and K % k == 0]
    if K // 32 > 1 and (Rr if kind < 4 else C) > 16:                         # (one k step or one row tile: the chunk is no choice)
        assert others
    for k in others:
        assert not np.array_equal(ref, R.shadow_ref(kind, w, k)), k


def test_shadow_layout_spans_are_aligned_disjoint_and_gapped():
    rec, tmap, n_src, n_dst, spans = R.shadow_layout()
    assert rec.dtype.itemsize == 56 and len(spans) == 10
    taken = np.zeros(n_dst, dtype=np.int32)
    for _, _, _, o, Rr, C in spans:
        assert o % 8 == 0 and o >= 8
        taken[o:o + Rr * C] += 1
    assert taken.max() == 1 and taken[0] == 0 and taken[-1] == 0
    edges = np.flatnonzero(np.diff(taken))                     # every span has unused elements on both sides
    assert len(edges) == 2 * len(spans)
    src_taken = np.zeros(n_src, dtype=np.int32)
    for r in rec:
        assert r["src"] % 8 == 0
        src_taken[r["src"]:r["src"] + r["R"] * r["C"]] += 1
    assert src_taken.max() == 1
    assert tmap.size == sum(((c[0] + 31) // 32) * ((c[1] + 31) // 32) for c in R.SHADOW_CASES)
    for i, r in enumerate(rec):
        n = ((r["R"] + 31) // 32) * ((r["C"] + 31) // 32)
        assert np.all(tmap[r["tile0"]:r["tile0"] + n] == i)
