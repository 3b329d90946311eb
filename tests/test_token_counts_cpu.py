"""CPU half of the token-count tests: the inputs of attn_tokens.masked_case are proved sensitive on the oracle, and the
oracle is proved well conditioned on them, so that a failure of test_token_counts_gpu.py means the kernel.

For every geometry the GPU tests run masked_case on, each simulated masking defect (attn_tokens.ref_attention) must move
the oracle's output, d qkv and d table by at least 10 x the gate the GPU test applies (10 x 3e-2 = 0.3 covers both dtypes)
under the suite's own metric rel_err.  On the suite's random inputs the same defect stays below the bf16 gate, which is
why these inputs exist (test_random_inputs_hide_an_admitted_padding_key).

The support queries are pure host functions of the built library and are checked here over whole ranges.
"""
import pytest
import torch

from attn_tokens import (DEFECTS, masked_case, masked_geoms, ref_fwd_bwd, token_case)
from conftest import rel_err
from test_kernels_gpu import ATTN_MODES, oracle_attn

SENSITIVE = 10 * 3e-2


def _defects(mode, N):
    for d in DEFECTS:
        if d.startswith("index") and mode != "relative":
            continue
        if d == "pad_key" and N % 16 == 0:      # a full last tile has no padding key
            continue
        yield d


@pytest.mark.parametrize("mode", ATTN_MODES)
def test_ref_attention_restates_the_oracle(mode):
    for N in (26, 65):
        for build in (token_case, masked_case):
            _, hd, G, xn, wqkv, dout, pe = build(mode, N, 64, 2, 2, seed=3)
            ref, dqkv_ref, g_ref = oracle_attn(mode, xn, wqkv, dout, pe, 2, "f32")
            out, dqkv, g = ref_fwd_bwd(mode, xn, wqkv, dout, pe, 2)
            assert rel_err(out, ref) < 1e-6 and rel_err(dqkv, dqkv_ref) < 1e-6
            for k in g_ref:
                assert rel_err(g[k], g_ref[k]) < 1e-5, k


@pytest.mark.parametrize("mode,N,D,H", masked_geoms())
def test_masked_inputs_expose_masking_defects(mode, N, D, H):
    _, hd, G, xn, wqkv, dout, pe = masked_case(mode, N, D, H, 2, seed=N)
    out, dqkv, g = ref_fwd_bwd(mode, xn, wqkv, dout, pe, H)
    for d in _defects(mode, N):
        o_d, dqkv_d, g_d = ref_fwd_bwd(mode, xn, wqkv, dout, pe, H, defect=d)
        assert rel_err(o_d, out) >= SENSITIVE, (d, "out", rel_err(o_d, out))
        assert rel_err(dqkv_d, dqkv) >= SENSITIVE, (d, "dqkv", rel_err(dqkv_d, dqkv))
        if mode == "relative":
            assert rel_err(g_d["table"], g["table"]) >= SENSITIVE, (d, "dtable", rel_err(g_d["table"], g["table"]))


@pytest.mark.parametrize("mode,N,D,H", masked_geoms())
def test_oracle_is_well_conditioned_on_the_masked_inputs(mode, N, D, H):
    """(a) the fp32 oracle against the same math in fp64: below 1e-5 (the fp32 gate is 1e-4);
    (b) q / k / v rounded to bf16 after the projection (what core_qkv hands the core, what the fused kernels do
        internally) against the unrounded projection: below a third of the bf16 gate."""
    _, hd, G, xn, wqkv, dout, pe = masked_case(mode, N, D, H, 2, seed=N)
    out32, _, _ = ref_fwd_bwd(mode, xn, wqkv, dout, pe, H)
    out64, _, _ = ref_fwd_bwd(mode, xn, wqkv, dout, pe, H, dtype=torch.float64)
    assert rel_err(out32, out64) < 1e-5, rel_err(out32, out64)
    o_b, _, _ = ref_fwd_bwd(mode, xn, wqkv, dout, pe, H, dt="bf16")
    o_r, _, _ = ref_fwd_bwd(mode, xn, wqkv, dout, pe, H, dt="bf16", round_qkv=True)
    assert rel_err(o_r, o_b) < 1e-2, rel_err(o_r, o_b)


@pytest.mark.parametrize("N,hd", [(72, 32), (198, 64), (207, 64)])
def test_random_inputs_hide_an_admitted_padding_key(N, hd):
    """the hole these tests close: on the suite's random inputs one admitted padding key passes the bf16 gate"""
    _, hd, G, xn, wqkv, dout, pe = token_case("relative", N, 2 * hd, 2, 2, seed=20)
    out, _, _ = ref_fwd_bwd("relative", xn, wqkv, dout, pe, 2)
    o_d, _, _ = ref_fwd_bwd("relative", xn, wqkv, dout, pe, 2, defect="pad_key")
    assert rel_err(o_d, out) < 3e-2


# ------------------------------------------------------------------------------------------ support queries
RANGES = [(17, 32), (49, 64), (65, 80), (145, 160), (193, 208), (257, 272)]
OUTSIDE = (16, 33, 48, 81, 144, 161, 192, 209, 256, 273)


def test_support_queries_over_the_whole_ranges():
    from vitpe import _lib
    h = _lib.lib()
    for hd in (32, 64):
        for lo, hi in RANGES:
            for n in range(lo, hi + 1):
                assert h.vitpe_attention_core_supported(_lib.BF16, n, hd) == 1, (n, hd)
        for n in OUTSIDE:
            assert h.vitpe_attention_core_supported(_lib.BF16, n, hd) == 0, (n, hd)
    for dt in (_lib.BF16, _lib.F32):
        for D in (192, 96):
            for n in range(65, 81):
                assert h.vitpe_fused_attention_supported(dt, n, D, 32) == 1, (dt, n, D)
            for n in (64, 81):
                assert h.vitpe_fused_attention_supported(dt, n, D, 32) == 0, (dt, n, D)
    for n in range(193, 209):
        assert h.vitpe_attention_fused64_supported(_lib.BF16, n, 2, 64) == 1, n
    for n in (192, 209):
        assert h.vitpe_attention_fused64_supported(_lib.BF16, n, 2, 64) == 0, n
    for n in range(17, 273):
        assert h.vitpe_fused_attention_wide_supported(_lib.BF16, n, 192, 32) == (n == 65), n
