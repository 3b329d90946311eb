"""Which kernels a TrainEngine step runs, decided once (Route / resolve_route), and where the weight shadows those kernels
read live (shadow_plan).  Pure host logic over the library's *_supported entry points: no device, no allocation."""
from __future__ import annotations

import dataclasses
import os

import numpy as np
import torch

from . import _lib as L
from . import kernels as K

ALIGN = 8  # elements: keeps every parameter 32-B (fp32) / 16-B (bf16 shadow) aligned


@dataclasses.dataclass(frozen=True)
class Route:
    """The flags of one engine, in dependency order (resolve_route's docstring is the table)."""
    extras: bool
    attn_fused: bool
    attn_wide: bool
    attn_fused64: bool
    fuse_ln: bool
    fuse_ln_bwd: bool
    tail2: bool
    lnbwd2: bool
    fuse_lnbwd: bool
    fuse_embed: bool
    group_wgrad: bool
    recompute_ln: bool
    fuse_head: bool
    cls_rows: bool

    def __post_init__(self):
        # a LayerNorm-operand (recompute_ln) or row-step (cls_rows) weight-gradient problem exists only in the grouped
        # launch: vitpe_gemm_tn has neither form
        assert self.group_wgrad or not (self.recompute_ln or self.cls_rows)


def resolve_route(dtype, C, S, patch, D, H, hid, depth, classes, extras=False, fuse_ln=None, env=os.environ) -> Route:
    """The route of a model of this geometry (C x S x S images in patch x patch patches, width D, H heads, MLP width hid,
    `depth` blocks, `classes` logits) in compute type `dtype`.  The only reader of the route's environment switches; each
    flag needs the ones named before it, so the lines below are the whole list of combinations that can exist.

    flag          needs                                       switch (default)        selects
    extras        the constructor's argument                  --                      per-Linear route: qkv bias, dropout, stochastic depth
    attn_fused    not extras, fused_attention_supported       --                      LN1 + qkv + PE + core in one kernel; else qkv Linear + core
    attn_wide     attn_fused, ..._wide_supported              VITPE_ATTN_WIDE (1)     32x32-tile forward (csrc/attn32.hip); 0: the 16x16-tile one
    attn_fused64  not attn_fused, not extras, ..._supported   VITPE_ATTN_FUSED64 (1)  N 197 / hd 64: projection + PE + core in one forward kernel
    fuse_ln       attn_fused, D = 192, fuse_ln is not False   VITPE_FUSE_LN (fwd |    LayerNorm inside the neighbouring kernels, forward ...
    fuse_ln_bwd   attn_fused, D = 192, fuse_ln None or True   all | off: for None)    ... and backward; 0: stand-alone LayerNorm kernels
    tail2         fuse_ln, fuse_ln_bwd, block_tail2_supported VITPE_TAIL2 (1)         proj + residual + LN2 + MLP in one kernel; 0: panel GEMMs
    lnbwd2        tail2                                       VITPE_LNBWD2 (1)        qkv data gradient + LN1 backward, wave per tile; 0: panel
    fuse_lnbwd    lnbwd2                                      VITPE_FUSE_LNBWD (1)    ... as the prologue of the tail backward below; 0: own launch
    fuse_embed    patch_embed_supported                       VITPE_FUSE_EMBED (1)    unfold + patch GEMM + bias + APE + class token + LN1 statistics
    group_wgrad   --                                          VITPE_GROUP_WGRAD (1)   a part's weight gradients in one launch; 0: a GEMM per Linear
    recompute_ln  tail2, group_wgrad                          VITPE_RECOMPUTE_LN (0)  LayerNorm outputs never stored (neutral to slower; saves memory)
    fuse_head     classes <= 64, D <= 768                     VITPE_FUSE_HEAD (1)     final LN + head + CE + head backward fused; 0: three kernels
    cls_rows      tail2, group_wgrad, fuse_head, bf16,        VITPE_CLS_ROWS (1)      top block's tail, its backward and three weight gradients on
                  depth >= 2                                                          the class rows only
    Raises VitpeError when no attention kernel takes the geometry."""
    def on(name, default="1"):
        return env.get(name, default) == "1"
    extras = bool(extras)
    N, hd = (S // patch) ** 2 + 1, D // H
    if fuse_ln is None and "VITPE_FUSE_LN" in env:
        fuse_ln = {"fwd": "fwd", "all": True, "off": False}[env["VITPE_FUSE_LN"]]
    attn_fused = not extras and K.fused_attention_supported(dtype, N, D, hd)
    if not attn_fused and not K.attention_core_supported(dtype, N, hd):
        raise L.VitpeError(f"no attention kernel for N={N}, D={D}, hd={hd}")
    attn_wide = attn_fused and K.fused_attention_wide_supported(dtype, N, D, hd) and on("VITPE_ATTN_WIDE")
    attn_fused64 = (not attn_fused and not extras and on("VITPE_ATTN_FUSED64")
                    and K.attention_fused64_supported(dtype, N, H, hd))
    ln_ok = attn_fused and D == 192   # (the 192-wide panel GEMM; the fusions hang off the fused attention's geometry)
    f_ln = ln_ok and fuse_ln is not False
    f_ln_bwd = ln_ok and (fuse_ln is True or fuse_ln is None)
    tail2 = f_ln and f_ln_bwd and on("VITPE_TAIL2") and K.block_tail2_supported(dtype, D, hid)
    lnbwd2 = tail2 and on("VITPE_LNBWD2")
    fuse_lnbwd = lnbwd2 and on("VITPE_FUSE_LNBWD")
    fuse_embed = on("VITPE_FUSE_EMBED") and K.patch_embed_supported(dtype, C, S, patch, D)
    group_wgrad = on("VITPE_GROUP_WGRAD")
    recompute_ln = tail2 and group_wgrad and on("VITPE_RECOMPUTE_LN", "0")
    fuse_head = classes <= 64 and D <= 768 and on("VITPE_FUSE_HEAD")
    cls_rows = (tail2 and group_wgrad and fuse_head and dtype == torch.bfloat16 and depth >= 2 and on("VITPE_CLS_ROWS"))
    return Route(*map(bool, (extras, attn_fused, attn_wide, attn_fused64, f_ln, f_ln_bwd, tail2, lnbwd2, fuse_lnbwd, fuse_embed,
                             group_wgrad, recompute_ln, fuse_head, cls_rows)))   # (the fields' order)


# ---- weight shadows ---------------------------------------------------------------------------
# destination layouts of vitpe_refresh_shadows (include/vitpe.h): transpose; vitpe_pack_qkv_weights; vitpe_pack_weight_frags
# of the matrix in natural / phi k order; the same two of its transpose; vitpe_pack_qkv_weights_wide
KIND_T, KIND_QKV, KIND_FRAG, KIND_FRAG_PHI, KIND_FRAG_T, KIND_FRAG_T_PHI, KIND_QKV_WIDE = range(7)

REC_DTYPE = np.dtype([("src", "<i8"), ("dst", "<i8"), ("dst2", "<i8"), ("R", "<i4"), ("C", "<i4"), ("tile0", "<i4"),
                      ("kind", "<i4"), ("HD", "<i4"), ("kind2", "<i4"), ("HD2", "<i4"), ("pad", "<i4")])


def shadow_plan(route: Route, shapes, offsets, hd):
    """The shadows the route's kernels read of every block's qkv / proj / fc1 / fc2 weight.  shapes[b] = their four
    (R, C), offsets[b] = their four element offsets in the flat parameter buffer, hd = the head dimension.
    -> (records [REC_DTYPE], one per source matrix with up to two shadows -- the source tile is loaded once for both;
        spans [(weight index 4 b + j, kind, element offset in the shadow buffer)];
        tile map int16 [tiles]: the record of every 32x32 source tile (tile0 = running sum of the records' tile counts);
        total elements of the shadow buffer)."""
    recs, spans, off, tile0 = [], [], 0, 0

    def add(w, kind, khd, kind2=-1, khd2=0):
        nonlocal off, tile0
        R, C = shapes[w // 4][w % 4]
        size = (R * C + ALIGN - 1) // ALIGN * ALIGN
        o1, o2 = off, (off + size if kind2 >= 0 else 0)
        off += size * (2 if kind2 >= 0 else 1)
        recs.append((offsets[w // 4][w % 4], o1, o2, R, C, tile0, kind, khd, kind2, khd2, 0))
        tile0 += ((R + 31) // 32) * ((C + 31) // 32)
        spans.append((w, kind, o1))
        if kind2 >= 0:
            spans.append((w, kind2, o2))

    for b in range(len(shapes)):
        qkv, proj, fc1, fc2 = range(4 * b, 4 * b + 4)
        if route.attn_fused:     # (lnbwd2: the packed transpose for the qkv data gradient; else the plain transpose)
            add(qkv, KIND_QKV, hd, *((KIND_FRAG_T, 64) if route.lnbwd2 else (KIND_T, 0)))
            if route.attn_wide:
                add(qkv, KIND_QKV_WIDE, hd)
        else:
            add(qkv, KIND_T, 0, *((KIND_FRAG, 64) if route.attn_fused64 else ()))
        if route.tail2:          # block_tail2_fwd reads the packs, block_tail2_bwd the packs of the transposes
            add(proj, KIND_FRAG, 192, KIND_FRAG_T_PHI, 192)
            add(fc1, KIND_FRAG_PHI, 192, KIND_FRAG_T_PHI, 32)
            add(fc2, KIND_FRAG_PHI, 32, KIND_FRAG_T_PHI, 192)
        else:
            for w in (proj, fc1, fc2):
                add(w, KIND_T, 0)
    rec = np.array(recs, dtype=REC_DTYPE)
    tmap = np.repeat(np.arange(len(recs), dtype=np.int16), np.diff(np.append(rec["tile0"], tile0)))
    return rec, spans, tmap, off
