"""tests/embed_ref.py checked without a GPU:

  * the case lists reach every value of every component of embed_ref.branch -- both gather branches from the three sources
    in both dtypes, both K-step counts, padded and unpadded K, every residue a square P has mod 16, one to four live
    waves, every D / 16 from 1 to 16;
  * every REFUSED entry fails exactly the one condition it names; every other case is a geometry with S % p == 0;
  * the three launches of ABOVE_CAP exceed their grid cap, no UNFOLD_CASES launch does;
  * tokens_ref equals oracle.vit_oracle.patch_embed (1e-6) and a float64 conv2d with kernel = stride = p (1e-12);
  * the integer inputs keep every partial sum an integer of magnitude <= 208 and their weights have no two equal rows
    (K = 4: no two equal (row, bias) pairs) and no two equal columns;
  * each seeded index bug -- kx and ky swapped, channel stride p instead of p^2, one patch row read from the neighbouring
    patch, the flip applied without the crop offset -- changes the patch matrix AND moves a token by more than the gate the
    GPU test applies to that case (any change at all in the integer case), so the GPU test's inputs can see it;
  * the draws of every augmented case hold a flipped and an unflipped slot and windows across each of the four borders.
"""
import pytest
import torch

import embed_ref as E
from oracle import vit_oracle as O

SOURCES = (("img", False), ("u8", False), ("u8", True))


def ids(cases):
    return ["-".join(str(v) for v in c[:-1]) for c in cases]


def _branches():
    out = set()
    for C, S, p, D, dts in E.FUSED_CASES:
        out |= {E.branch(dt, C, S, p, D, src, aug) for dt in dts for src, aug in SOURCES}
    for C, S, p, D, pad, dts in E.AUG_CASES:
        out |= {E.branch(dt, C, S, p, D, "u8", True) for dt in dts}
    return out


def test_case_lists_reach_every_branch_value():
    br = _branches()
    assert {b[0] for b in br} == {"fused"}
    want = [{"p4", "generic"}, {"img", "u8", "u8aug"}, {1, 2}, {True, False}, {0, 1, 4, 9}, {1, 2, 3, 4}, set(range(1, 17))]
    for i, w in enumerate(want, start=1):
        assert {b[i] for b in br} == w, (i, sorted({b[i] for b in br}))
    # the generic branch from each source in each dtype, and so the p == 4 branch
    for which in ("generic", "p4"):
        assert {(b[2], dt) for dt in E.BOTH for b in _branches_of(dt) if b[1] == which} == \
            {(s, dt) for s in ("img", "u8", "u8aug") for dt in E.BOTH}, which
    # the edges the issue names
    geoms = {(c[0], c[1], c[2]) for c in E.FUSED_CASES}
    Ks = {E.geometry(*g)[2] for g in geoms}
    Ps = {E.geometry(*g)[1] for g in geoms}
    assert {4, 12, 36, 64} <= Ks and {4, 16, 25, 49, 64} <= Ps
    assert {c[3] for c in E.FUSED_CASES} >= {16, 256, 48, 80, 240}
    aug_generic = [c for c in E.AUG_CASES if c[2] != 4]
    assert len(aug_generic) >= 4 and any(c[4] == c[1] for c in aug_generic)            # pad == S
    assert any(c[2] == 4 and c[3] == 256 for c in E.AUG_CASES)


def _branches_of(dt):
    out = []
    for C, S, p, D, dts in E.FUSED_CASES:
        if dt in dts:
            out += [E.branch(dt, C, S, p, D, src, aug) for src, aug in SOURCES]
    for C, S, p, D, pad, dts in E.AUG_CASES:
        if dt in dts:
            out.append(E.branch(dt, C, S, p, D, "u8", True))
    return out


def test_every_case_is_supported_and_a_whole_grid():
    for C, S, p, D, *rest in E.FUSED_CASES + E.AUG_CASES:
        assert S % p == 0
        for dt in rest[-1]:
            assert E.refusals(dt, C, S, p, D) == (), (dt, C, S, p, D)
        if rest[-1] == E.F32:                                  # fp32 only because bf16 is refused, not for convenience
            assert E.refusals("bf16", C, S, p, D) == ("K % chunk",)
    for C, S, p, D, pad, _ in E.AUG_CASES:
        assert 0 <= pad <= S
    for C, S, p in E.UNFOLD_CASES:
        assert S % p == 0


@pytest.mark.parametrize("c", E.REFUSED, ids=["-".join(str(v) for v in c[:5]) for c in E.REFUSED])
def test_refused_for_exactly_the_stated_reason(c):
    dt, C, S, p, D, why = c
    assert E.refusals(dt, C, S, p, D) == (why,)
    assert E.branch(dt, C, S, p, D, "img")[0] == why


def test_refused_covers_every_condition():
    assert {c[5] for c in E.REFUSED} == {"K > 64", "K % chunk", "P > 64", "D < 16", "D > 256", "D % 16", "S % p"}
    assert {(1, 28, 7), (3, 32, 8), (3, 36, 4)} <= {c[1:4] for c in E.REFUSED}
    assert {8, 24, 272} <= {c[4] for c in E.REFUSED}


def test_unfold_launches_and_the_caps():
    for c in E.ABOVE_CAP:
        need, cap = E.unfold_launch(*c)
        assert need > cap
    assert E.unfold_launch(*E.ABOVE_CAP[0]) == (2162688, 2097152)
    assert E.unfold_launch(*E.ABOVE_CAP[2]) == (4198400, 4194304)
    for C, S, p in E.UNFOLD_CASES:
        for dt in E.BOTH:
            kernel = "unfold8" if dt == "bf16" and p % 8 == 0 else "unfold"
            need, cap = E.unfold_launch(kernel, dt, C, S, p, E.UNFOLD_B)
            assert need <= cap
    p8 = {p // 8 for _, _, p in E.UNFOLD_CASES if p % 8 == 0}
    assert p8 == {1, 2, 3}                                      # unfold8_kernel at p = 8, 16 and 24


# ---- the reference against two independent statements ----------------------------------------------------------------------
@pytest.mark.parametrize("C,S,p,D", [(3, 32, 4, 192), (1, 32, 8, 64)])
def test_tokens_ref_equals_the_oracle(C, S, p, D):
    cfg = O.VitConfig(img_size=S, patch_size=p, in_chans=C, embed_dim=D, depth=1, num_heads=2, pos_encoding="absolute")
    params = O.closed_form_params(cfg)
    img, _ = O.closed_form_batch(cfg, 3)
    P = cfg.num_patches
    want = O.patch_embed(cfg, params, img)
    got = E.tokens_ref("f32", E.unfold_img(img, p).reshape(3, P, -1), params["patch_embed.weight"].reshape(D, -1),
                       params["patch_embed.bias"], params["cls_token"].reshape(-1), params["pos_embed.pos_embed"][0, :P])
    assert tuple(got.shape) == (3, P + 1, D) and got.dtype == torch.float64
    assert float((got - want.double()).abs().max()) < 1e-6 * float(want.abs().max())


@pytest.mark.parametrize("c", E.FUSED_CASES, ids=ids(E.FUSED_CASES))
def test_tokens_ref_equals_conv2d_in_float64(c):
    C, S, p, D, dts = c
    _, P, K = E.geometry(C, S, p)
    for dt in dts:
        img, w, bias, cls, ape = E.real_inputs(dt, C, S, p, D)
        x = E.q(img, dt)
        conv = torch.nn.functional.conv2d(x.double(), w.double().reshape(D, C, p, p), bias.double(), stride=p)
        want = conv.flatten(2).transpose(1, 2) + ape.double()
        got = E.tokens_ref(dt, E.unfold_img(img, p).reshape(-1, P, K), w, bias, cls, ape)
        assert float((got[:, 1:] - want).abs().max()) <= 1e-12 * float(want.abs().max())
        assert torch.equal(got[:, 0], cls.double().expand(img.shape[0], D))
        none = E.tokens_ref(dt, E.unfold_img(img, p).reshape(-1, P, K), w, bias, cls, None)
        assert float((none[:, 1:] + ape.double() - want).abs().max()) <= 1e-12 * float(want.abs().max())


# ---- the integer inputs ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", E.FUSED_CASES, ids=ids(E.FUSED_CASES))
def test_integer_inputs_are_exact_and_asymmetric(c):
    C, S, p, D, dts = c
    _, P, K = E.geometry(C, S, p)
    img, w, bias, cls, ape = E.int_inputs(C, S, p, D)
    for t, lim in ((img, 3), (w, 1), (bias, 8), (ape, 8), (cls, 100)):
        assert torch.equal(t, t.round()) and float(t.abs().max()) <= lim
    x = E.unfold_img(img, p).reshape(-1, P, K)
    assert float(E.abs_terms("f32", x, w, bias, ape).max()) <= 208                # bounds every partial sum in any order
    for dt in dts:                                                                   # nothing is lost in bf16
        ref = E.tokens_ref(dt, x, w, bias, cls, ape)
        assert torch.equal(ref, E.q(ref.float(), dt).double()) and torch.equal(E.q(x, dt), x)
    rows = torch.cat([w, bias[:, None]], 1) if 3 ** K < D else w
    assert len({tuple(r.tolist()) for r in rows}) == D
    assert len({tuple(col.tolist()) for col in w.t()}) == K
    assert float(w.abs().sum(1).min()) > 0 or K == 4                                 # (an all-zero row only where 81 codes repeat)


# ---- seeded index bugs -----------------------------------------------------------------------------------------------------
def _moved(dt, x, xm, w, bias, cls, ape, K):
    """(patch matrix changed, worst token change / the GPU gate of that element)"""
    ref = E.tokens_ref(dt, x, w, bias, cls, ape)
    bound = E.token_bound(dt, ref[:, 1:], E.abs_terms(dt, x, w, bias, ape), K)
    mut = E.tokens_ref(dt, xm, w, bias, cls, ape)
    return not torch.equal(E.q(x, dt), E.q(xm, dt)), E.excess(mut[:, 1:], ref[:, 1:], bound)


@pytest.mark.parametrize("bug", ["kx_ky_swapped", "channel_stride_p", "row_from_neighbour_patch"])
@pytest.mark.parametrize("c", E.FUSED_CASES, ids=ids(E.FUSED_CASES))
def test_a_wrong_gather_index_is_visible_above_the_gate(c, bug):
    C, S, p, D, dts = c
    _, P, K = E.geometry(C, S, p)
    if bug == "channel_stride_p" and C == 1:
        assert torch.equal(E.mutant_patches(E.int_inputs(C, S, p, D)[0], p, bug), E.unfold_img(E.int_inputs(C, S, p, D)[0], p))
        return                                                  # one channel: the stride is never used, the bug is none
    for dt in dts:
        for ape_on in (True, False):
            # integer case: the gate is bit equality
            img, w, bias, cls, ape = E.int_inputs(C, S, p, D)
            x, xm = E.unfold_img(img, p).reshape(-1, P, K), E.mutant_patches(img, p, bug).reshape(-1, P, K)
            ape = ape if ape_on else None
            assert not torch.equal(x, xm)
            assert not torch.equal(E.tokens_ref(dt, x, w, bias, cls, ape), E.tokens_ref(dt, xm, w, bias, cls, ape))
            # real-valued case, from fp32 images and from the uint8 dataset
            _, w, bias, cls, ape = E.real_inputs(dt, C, S, p, D)
            ape = ape if ape_on else None
            for img in (E.real_inputs(dt, C, S, p, D)[0], E.u8_images(C, S)):
                x, xm = E.unfold_img(img, p).reshape(-1, P, K), E.mutant_patches(img, p, bug).reshape(-1, P, K)
                changed, ratio = _moved(dt, x, xm, w, bias, cls, ape, K)
                assert changed and ratio > 100, (dt, ratio)


@pytest.mark.parametrize("c", E.AUG_CASES, ids=ids(E.AUG_CASES))
def test_augmented_draws_cover_flips_and_borders_and_see_a_flip_without_offset(c):
    C, S, p, D, pad, dts = c
    _, P, K = E.geometry(C, S, p)
    prm = E.draws(pad)
    assert E.draws_cover(prm, pad), prm
    assert not (prm[0] == prm[2]).all()                         # record 3 in slots 0 and 2: two independent draws
    good = E.u8_images(C, S, pad=pad)
    assert not torch.equal(good[0], good[2])
    if pad == S:                                                # a window wholly in the padding exists
        assert any(oy in (0, 2 * pad) or ox in (0, 2 * pad) for oy, ox, _ in prm)
    bad = E.flip_without_crop_offset(C, S, pad)
    for dt in dts:
        _, w, bias, cls, ape = E.real_inputs(dt, C, S, p, D)
        x, xm = E.unfold_img(good, p).reshape(-1, P, K), E.unfold_img(bad, p).reshape(-1, P, K)
        changed, ratio = _moved(dt, x, xm, w, bias, cls, ape, K)
        assert changed and ratio > 100, (dt, ratio)


def test_default_pad_draws_cover_too():
    """the u8aug source of a FUSED_CASES entry uses DEFAULT_PAD and UNFOLD_CASES use UNFOLD_PAD, with the same pair and
    slots; the above-the-cap launch draws for 352 slots"""
    assert E.draws_cover(E.draws(E.DEFAULT_PAD), E.DEFAULT_PAD)
    assert E.draws_cover(E.draws(E.UNFOLD_PAD), E.UNFOLD_PAD)
    assert E.draws_cover(E.draws(E.UNFOLD_PAD, E.ABOVE_CAP[1][5]), E.UNFOLD_PAD)


def test_a_correct_fp32_restatement_stays_inside_the_gates():
    """the bound leaves a plain fp32 (and bf16-stored) matmul inside it: the reference alone does not fail a correct kernel"""
    for C, S, p, D, dts in E.FUSED_CASES:
        _, P, K = E.geometry(C, S, p)
        for dt in dts:
            img, w, bias, cls, ape = E.real_inputs(dt, C, S, p, D)
            x = E.unfold_img(img, p).reshape(-1, P, K)
            ref = E.tokens_ref(dt, x, w, bias, cls, ape)
            got = E.q(E.q(x, dt) @ w.t() + bias + ape, dt)
            bound = E.token_bound(dt, ref[:, 1:], E.abs_terms(dt, x, w, bias, ape), K)
            assert E.excess(got, ref[:, 1:], bound) <= 1.0, (C, S, p, D, dt)
            if dt == "bf16":
                b32 = E.token_bound("f32", ref[:, 1:], E.abs_terms(dt, x, w, bias, ape), K)
                assert E.outside_rounding_interval(got, ref[:, 1:], b32) == 0
                off = got.clone()
                off[0, 0, 0] = torch.nextafter(got[0, 0, 0].bfloat16(), torch.tensor(9.0).bfloat16()).float()   # one bf16 ulp
                assert E.outside_rounding_interval(off, ref[:, 1:], b32) == 1
