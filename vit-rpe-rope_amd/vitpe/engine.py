"""Train-step engine: the MI355X replacement of the reference's step loop (train.py:108-123).

    zero_grad -> forward -> mean CE -> backward -> AdamW        (train.py:111-116,194-195)

* every parameter lives in ONE flat fp32 buffer (master), with a flat gradient buffer and flat
  AdamW moments next to it; the nn.Module's parameters are re-pointed at views of it, so
  state_dict()/checkpoints keep working and the gradient all-reduce is one contiguous bucket;
* forward and backward are explicit sequences of HIP kernels over preallocated activations
  (no autograd graph, no allocator traffic), captured once into a HIP graph and replayed;
* the loss / #correct stay on the device (no per-step host sync, cf. train.py:118,121);
* data parallel: one process per GPU, gradients summed with ONE RCCL all-reduce of the flat
  bucket per step (torch.distributed "nccl" backend == RCCL over xGMI) and averaged inside
  the fused AdamW kernel (grad_scale = 1/world).
"""
from __future__ import annotations

import contextlib
import dataclasses
import math
import os
from typing import Dict, List, Optional

import numpy as np
import torch
import torch.distributed as dist
import torch.nn as nn

from . import _lib as L
from . import ddp
from . import kernels as K
from .positional_encoding import (AbsolutePositionalEncoding, PolynomialRPE, RelativePositionalEncoding, RoPEAxial,
                                  RoPEMixed)
from .head import StepHead
from .optim import StepOptimizer
from .route import (ALIGN, KIND_FRAG, KIND_FRAG_PHI, KIND_QKV, KIND_QKV_WIDE, KIND_T, Route, resolve_route,  # noqa: F401
                    shadow_plan)
from .vit import VisionTransformer

# Dropout sites of one layer in TrainEngine.rng_table (extras=True): layer l owns rows SITES_PER_LAYER * l + SITE_*, one
# (seed, offset) pair each ("Engine route")
SITE_ATTN, SITE_PROJ, SITE_MLP1, SITE_MLP2, SITE_PATH_A, SITE_PATH_M = range(6)
SITES_PER_LAYER = 6


def site_row(layer: int, site: int) -> int:
    """Row of `site` (SITE_*) of layer `layer` in the site table."""
    return SITES_PER_LAYER * layer + site


def shift_rng_offsets(table: torch.Tensor, rank: int) -> torch.Tensor:
    """A copy of the [n, 2] int64 (seed, offset) table with rank << 48 added to every offset (mod 2^64; the seeds stay):
    data-parallel ranks that drew the same pairs (same torch seed) still never share a stream.  Pure host arithmetic on
    whatever device the table lives on."""
    inc = (int(rank) << 48) & 0xFFFFFFFFFFFFFFFF
    out = table.clone()
    out[:, 1] += inc - (1 << 64) if inc >= (1 << 63) else inc   # (two's complement: int64 addition wraps like uint64)
    return out


def new_augment_rng(device, rank: int = 0) -> torch.Tensor:
    """The (seed, offset) pair [1, 2] int64 of the augmentation stream ("Augmentation stream"): drawn from
    torch's generator of `device` (torch.manual_seed reproduces it), the offset shifted by rank << 48 like the dropout
    sites' -- data-parallel ranks never crop alike."""
    return shift_rng_offsets(K.new_rng_pairs(1, device), rank)


def engine_unsupported(model):
    """Names of the active model options TrainEngine cannot run (qkv bias, dropout, stochastic depth); [] if none."""
    active = []
    for blk in model.blocks:
        if blk.attn.qkv.bias is not None:
            active.append("qkv_bias")
        if blk.attn.attn_drop_p > 0.:
            active.append("attn_drop")
        if blk.attn.proj_drop_p > 0. or blk.mlp.drop > 0.:
            active.append("drop")
        if blk.drop_path_p > 0.:
            active.append("drop_path")
    return sorted(set(active))


class TrainEngine:
    def __init__(self, model: VisionTransformer, batch_size: int, compute_dtype=torch.bfloat16, lr=1e-3,
                 weight_decay=0.01, betas=(0.9, 0.999), eps=1e-8, process_group=None, use_graph=True, fuse_ln=None,
                 extras=False):
        """extras=True: the opt-in per-Linear route (stand-alone LayerNorm, vitpe_linear, attention core, grouped weight
        gradients) at every geometry, which runs qkv bias, dropout, attention dropout and stochastic depth; a model with
        none of them active runs the same route (a comparator for the fused default)."""
        active = engine_unsupported(model)
        if active and not extras:
            # the flat buffers and fused kernels of this engine have no bias input on the qkv projection and no dropout
            # (DESIGN.md 8): refuse instead of silently training without them
            raise NotImplementedError("TrainEngine does not support " + ", ".join(active) + " (the fused training path has "
                                      "no qkv bias and no dropout); train this model through the module path instead.  "
                                      "TrainEngine(..., extras=True) runs them on the per-Linear route")
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            raise L.VitpeError("TrainEngine needs the model on the HIP device (no CPU path)")
        self.model, self.dev, self.T, self.B = model, dev, compute_dtype, batch_size
        self.pg = process_group
        self.world = dist.get_world_size(process_group) if (dist.is_available() and dist.is_initialized()) else 1
        self.use_graph = use_graph
        m = model
        self.D, self.H, self.Lyr, self.p = m.embed_dim, m.num_heads, len(m.blocks), m.patch_size
        self.C, self.P, self.Cn = m.patch_embed.weight.shape[1], m.num_patches, m.num_classes
        self.N, self.grid = self.P + 1, int(math.sqrt(self.P))
        self.S, self.M = self.grid * self.p, self.B * self.N
        self.hid = m.blocks[0].mlp.fc1.weight.shape[0]
        # which kernels the step runs: decided here, before anything is allocated (route.resolve_route holds the table of
        # flags and switches); every flag is also an attribute of the engine (eng.tail2, eng.attn_fused, ...)
        self.route: Route = resolve_route(compute_dtype, self.C, self.S, self.p, self.D, self.H, self.hid, self.Lyr, self.Cn,
                                          extras=extras, fuse_ln=fuse_ln)
        self.__dict__.update(dataclasses.asdict(self.route))
        self._save_hidden = True
        self._build_flat(lr, weight_decay, betas, eps)
        self._build_buffers()
        self._build_rng_table()
        self.aug_rng, self.aug_pad, self.aug_hflip = None, 0, False   # set_augment()
        # gradient exchange in two buckets so the first overlaps the lower half of the backward pass:
        # flat[bucket_off:] = layers split.. + final norm + head (complete after the "upper" backward),
        # flat[:bucket_off] = class token, patch embed, PE parameters, layers 0..split-1
        self.split_layer = max(1, self.Lyr // 2)
        self.bucket_off = self._off[id(next(self.model.blocks[self.split_layer].parameters()))] \
            if self.Lyr >= 2 else 0
        self.overlap_comm = self.world > 1 and self.Lyr >= 2
        # VITPE_DDP_ALLPAIRS=1: the bucket is summed by one all-to-all + a local reduction + one all-gather (every rank
        # talks to every other rank directly: one transfer per xGMI link) instead of RCCL's all-reduce.  Opt-in until it
        # has been timed on an 8-GPU node (ddp.AllPairsSum; 2-rank gloo test on CPU)
        self.allpairs = (ddp.AllPairsSum(self.pg) if self.world > 1 and os.environ.get("VITPE_DDP_ALLPAIRS", "0") == "1"
                         else None)
        self._comm_stream = torch.cuda.Stream(device=dev) if self.allpairs is not None else None
        # VITPE_DDP_GRAPH=1: capture the two bucket all-reduces INSIDE the step's HIP graph (bucket 1 on a forked stream
        # beside the lower half of the backward): a step is then ONE replay instead of three replays stitched from the
        # host.  Off by default: RCCL capture has not run on hardware yet (no multi-GPU lease this round either) -- the
        # stitched path only uses plain torch.distributed calls.  A failed capture falls back to it.
        self.ddp_graph = self.world > 1 and os.environ.get("VITPE_DDP_GRAPH", "0") == "1"
        self._drop_graphs()
        self.steps_done = 0

    def _drop_graphs(self):
        """Forget the captured step: the next step() captures again."""
        self.graph_fb = self.graph_fb2 = self.graph_opt = None

    def _rank(self) -> int:
        return dist.get_rank(self.pg) if self.world > 1 else 0

    # ---------------------------------------------------------------- parameters / shadows
    def _build_flat(self, lr, wd, betas, eps):
        params = list(self.model.parameters())  # de-duplicated, reference named_parameters() order
        starts, n = ddp.flat_layout([prm.numel() for prm in params], ALIGN)
        offs = {id(prm): o for prm, o in zip(params, starts)}
        self.n_flat = n
        f = dict(dtype=torch.float32, device=self.dev)
        self.flat_p, self.flat_g = torch.zeros(n, **f), torch.zeros(n, **f)
        self.flat_s = torch.zeros(n, dtype=torch.bfloat16, device=self.dev) if self.T == torch.bfloat16 else None
        self._off = offs
        for prm in params:
            o = offs[id(prm)]
            view = self.flat_p[o:o + prm.numel()].view(prm.shape)
            view.copy_(prm.data)
            prm.data = view
            prm.grad = self.flat_g[o:o + prm.numel()].view(prm.shape)
        self.model.register_load_state_dict_post_hook(lambda _m, _keys: self.sync_from_model())
        # everything between the backward and the next forward: optim.StepOptimizer (the moments, the hp block, clip, EMA,
        # parameter groups, schedule); hp, flat_m and flat_v stay reachable here under their old names
        self.opt = StepOptimizer(self.flat_p, self.flat_g, self.flat_s, lr, wd, betas, eps, self.world, offs, n,
                                 self._drop_graphs)
        self.hp, self.flat_m, self.flat_v = self.opt.hp, self.opt.flat_m, self.opt.flat_v
        # transposed shadows of the GEMM weights (data-gradient GEMMs) and fragment-major packed copies (attention and
        # block-tail kernels): one flat buffer laid out by route.shadow_plan, refreshed by ONE batched kernel per step
        blocks = [(b.attn.qkv.weight, b.attn.proj.weight, b.mlp.fc1.weight, b.mlp.fc2.weight) for b in self.model.blocks]
        self._gemm_weights: List[nn.Parameter] = [w for ws in blocks for w in ws]
        rec, spans, tmap, total = shadow_plan(self.route, [[tuple(w.shape) for w in ws] for ws in blocks],
                                              [[offs[id(w)] for w in ws] for ws in blocks], self.D // self.H)
        self._shadow_flat = torch.empty(total, dtype=self.T, device=self.dev)
        # views by id(weight): KIND_T; KIND_QKV; KIND_QKV_WIDE; KIND_FRAG, KIND_FRAG_PHI; KIND_FRAG_T, KIND_FRAG_T_PHI
        self._st, self._pk, self._pkw, self._fr, self._frt = ({} for _ in range(5))   # type: Dict[int, torch.Tensor]
        for wi, kind, o in spans:
            w = self._gemm_weights[wi]
            (R, C), flat = w.shape, self._shadow_flat[o:o + w.numel()]
            if kind == KIND_T:
                self._st[id(w)] = flat.view(C, R)
            elif kind == KIND_QKV:
                self._pk[id(w)] = flat.view(R, C)
            elif kind == KIND_QKV_WIDE:
                self._pkw[id(w)] = flat
            elif kind in (KIND_FRAG, KIND_FRAG_PHI):
                self._fr[id(w)] = flat.view(R, C)
            else:
                self._frt[id(w)] = flat.view(C, R)
        self._desc = torch.from_numpy(rec.view(np.uint8).copy()).to(self.dev)
        self._ndesc, self._ntiles = len(rec), len(tmap)
        self._tile_map = torch.from_numpy(tmap).to(self.dev)
        self.refresh_shadows()

    def Pm(self, prm):  # fp32 master view
        return prm.data

    def Gr(self, prm):  # fp32 gradient view
        o = self._off[id(prm)]
        return self.flat_g[o:o + prm.numel()].view(prm.shape)

    def Sh(self, prm):  # compute-dtype shadow view (GEMM operand)
        if self.T == torch.float32:
            return prm.data
        o = self._off[id(prm)]
        return self.flat_s[o:o + prm.numel()].view(prm.shape)

    def St(self, prm):  # transposed compute-dtype shadow
        return self._st[id(prm)]

    def Pk(self, prm):  # packed qkv weights
        return self._pk[id(prm)]

    def Pkw(self, prm):  # wide pack of the qkv weights (32x32-tile attention forward)
        return self._pkw[id(prm)]

    def Fr(self, prm):  # fragment-major packed copy (block_tail2_fwd)
        return self._fr[id(prm)]

    def Frt(self, prm):  # fragment-major packed copy of the transpose (block_tail2_bwd)
        return self._frt[id(prm)]

    def _attn_fwd(self, x, blk, out, ln=None, xn_out=None):
        """The fused attention forward the step runs: the wide kernel where its geometry applies."""
        if self.attn_wide:
            return K.fused_attention_fwd_wide(x, self.Pkw(blk.attn.qkv.weight), self.H, self.pe, out=out, ln=ln, xn_out=xn_out)
        return K.fused_attention_fwd(x, self.Pk(blk.attn.qkv.weight), self.H, self.pe, out=out, ln=ln, xn_out=xn_out)

    def _attn_layer_fwd(self, l, save_qkv=True, p_drop=0.):
        """Layer l's attention forward as the step runs it, on the layer's own buffers: fused (LayerNorm staged inside when
        fuse_ln), projection + core in one kernel at hd = 64 (save_qkv: the raw projection goes to qkv_l[l] for the
        backward), or the core on qkv_l[l] -- the qkv Linear in front of that one is the caller's -- with attention
        dropout at rate p_drop inside it (extras)."""
        blk, a = self.model.blocks[l], self.act[l]
        if self.fuse_ln:   # (xn1 is None when recompute_ln)
            return self._attn_fwd(self.x[l], blk, a["a"], ln=(blk.norm1.weight.data, blk.norm1.bias.data, a["m1"], a["r1"]),
                                  xn_out=a["xn1"])
        if self.attn_fused:
            return self._attn_fwd(a["xn1"], blk, a["a"])
        if self.attn_fused64:
            return K.attention_fused64_fwd(a["xn1"], self.Fr(blk.attn.qkv.weight), self.H, self.pe,
                                           qkv_out=(self.qkv_l[l] if save_qkv else None), out=a["a"])
        if p_drop > 0.:
            return K.attention_core_fwd_drop(self.qkv_l[l], self.H, self.pe, self._site(l, SITE_ATTN, p_drop), p_drop,
                                             out=a["a"])
        return K.attention_core_fwd(self.qkv_l[l], self.H, self.pe, out=a["a"])

    def _attn_bwd(self, l, dout, p_drop=0.):
        """Layer l's attention backward as the step runs it: dout (gradient of the merged heads) -> dqkv_l[l], PE-parameter
        gradients accumulated; p_drop: the forward's attention dropout, its mask regenerated."""
        blk, a = self.model.blocks[l], self.act[l]
        if not self.attn_fused and p_drop > 0.:
            return K.attention_core_bwd_drop(self.qkv_l[l], dout, self.H, self.pe, self._site(l, SITE_ATTN, p_drop), p_drop,
                                             out=self.dqkv_l[l], **self.pe_grads)
        if not self.attn_fused:
            return K.attention_core_bwd(self.qkv_l[l], dout, self.H, self.pe, out=self.dqkv_l[l], **self.pe_grads)
        if self.recompute_ln:   # nothing normalised was stored: LayerNorm1 again while staging the raw tokens
            return K.fused_attention_bwd(self.x[l], self.Pk(blk.attn.qkv.weight), dout, self.H, self.pe, out=self.dqkv_l[l],
                                         ln=(blk.norm1.weight.data, blk.norm1.bias.data, a["m1"], a["r1"]), **self.pe_grads)
        return K.fused_attention_bwd(a["xn1"], self.Pk(blk.attn.qkv.weight), dout, self.H, self.pe, out=self.dqkv_l[l],
                                     **self.pe_grads)

    def refresh_shadows(self, cast_flat=True):
        if self.T == torch.bfloat16 and cast_flat:
            K.cast(self.flat_p, torch.bfloat16, out=self.flat_s)
        K.refresh_shadows(self.flat_p, self._shadow_flat, self._desc, self._ndesc, self._ntiles, self._tile_map)

    # ---------------------------------------------------------------- optimizer side: optim.StepOptimizer does the work
    def set_lr(self, lr: float):
        self.opt.set_lr(lr)

    def current_lr(self) -> float:
        """The learning rate of the last step; synchronises with the device."""
        return self.opt.current_lr()

    def set_param_groups(self, groups):
        """AdamW parameter groups inside the step: StepOptimizer.set_param_groups."""
        self.opt.set_param_groups(groups)

    def set_lr_schedule(self, base_lr: Optional[float], total_steps: int = 0, warmup_steps: int = 0, min_lr: float = 0.0,
                        warmup_factor: float = 1e-3, done: int = 0):
        """Linear warm-up + cosine learning rate, stepped every iteration inside the step: StepOptimizer.set_lr_schedule."""
        self.opt.set_lr_schedule(base_lr, total_steps, warmup_steps, min_lr, warmup_factor, done)

    def set_grad_clip(self, max_norm: Optional[float]):
        """clip_grad_norm_(model.parameters(), max_norm) inside the step: StepOptimizer.set_grad_clip."""
        self.opt.set_grad_clip(max_norm)

    def grad_norm(self) -> float:
        """total_norm of the last optimizer step, before clipping; synchronises with the device."""
        return self.opt.grad_norm()

    def set_ema(self, decay: Optional[float], warmup: bool = False):
        """Keep an exponential moving average of the parameters, updated inside the step: StepOptimizer.set_ema."""
        self.opt.set_ema(decay, warmup)

    def reset_ema(self):
        """Restart the average as a copy of the current parameters; captured graphs stay valid."""
        self.opt.reset_ema()

    def _ema_swap(self):
        K.ema_swap(self.flat_p, self.opt.flat_e, self.flat_s)
        self.refresh_shadows(cast_flat=False)

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the context the model IS its average: flat_p and flat_e are exchanged in place (flat_s follows under
        bf16) and the packed shadows re-derived, so forward_indexed, forward_only, eval_loss, model(images) and
        model.state_dict() all see the averaged weights -- no second set of shadows exists.  Leaving (also by an exception)
        exchanges them back: flat_p, flat_e, flat_s and the shadows return bit for bit, no pointer moves, captured graphs
        stay valid.  Training calls, capture(), set_ema() and a nested ema_weights() raise VitpeError inside."""
        self.opt.guard("ema_weights")
        self.opt.needs_ema("ema_weights")
        self._ema_swap()
        self.opt.ema_swapped = True
        try:
            yield self
        finally:
            self._ema_swap()
            self.opt.ema_swapped = False

    def _param_spans(self):
        """(state_dict key, offset into the flat buffers, parameter) of every parameter."""
        return [(name, self._off[id(prm)], prm) for name, prm in self.model.named_parameters(remove_duplicate=False)]

    def ema_state_dict(self):
        """model.state_dict() with every parameter entry replaced by a clone of its average (buffers as they are); nothing
        is swapped.  Inside ema_weights() the same values (they sit in flat_p then)."""
        self.opt.needs_ema("ema_state_dict")
        src = self.flat_p if self.opt.ema_swapped else self.opt.flat_e
        sd = self.model.state_dict()
        for name, o, prm in self._param_spans():
            sd[name] = src[o:o + prm.numel()].view(prm.shape).clone()
        return sd

    def load_ema_state_dict(self, sd):
        """The inverse of ema_state_dict(): the parameter entries of `sd` become the average (other keys are ignored; a
        missing or mis-shaped parameter raises VitpeError).  The parameters themselves are not touched."""
        self.opt.guard("load_ema_state_dict")
        self.opt.needs_ema("load_ema_state_dict")
        spans = self._param_spans()
        for name, _, prm in spans:
            if name not in sd or tuple(sd[name].shape) != tuple(prm.shape):
                raise L.VitpeError(f"load_ema_state_dict: no entry of shape {tuple(prm.shape)} for parameter {name!r}")
        for name, o, prm in spans:
            self.opt.flat_e[o:o + prm.numel()].view(prm.shape).copy_(sd[name])

    # ---------------------------------------------------------------- activations
    def _build_buffers(self):
        B, N, D, M, T, dev = self.B, self.N, self.D, self.M, self.T, self.dev
        e = lambda *s, dt=T: torch.empty(*s, dtype=dt, device=dev)  # noqa: E731
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)  # noqa: E731
        self.images = f(B, self.C, self.S, self.S)
        self.labels = torch.zeros(B, dtype=torch.int64, device=dev)
        self.patches = e(B * self.P, self.C * self.p * self.p)
        self.x = [e(B, N, D) for _ in range(self.Lyr + 1)]
        xn = (lambda: None) if self.recompute_ln else (lambda: e(B, N, D))
        self.act = []
        for blk in self.model.blocks:
            # hd (extras route, Mlp dropout): the dropped hidden activation, fc2's operand in the forward and the weight gradient
            self.act.append(dict(xn1=xn(), m1=f(M), r1=f(M), a=e(B, N, D), xmid=e(B, N, D), xn2=xn(),
                                 m2=f(M), r2=f(M), h=e(M, self.hid), u=e(M, self.hid),
                                 hd=e(M, self.hid) if self.extras and blk.mlp.drop > 0. else None))
        self._probe_scratch = None
        # Gradient tensors read by the weight-gradient GEMMs get per-layer buffers (dy = d x_out, dmid = d x_mid,
        # du, dqkv): the grouped weight-gradient launch at the end of a backward part reads all of them, so the main
        # chain must not reuse one across layers (288 GB of HBM: ~0.7 GB extra is free)
        self.dtmp = e(B, N, D)
        self.dx_out = [e(B, N, D) for _ in range(self.Lyr + 1)]   # [l] = gradient w.r.t. x[l]
        # final norm + classifier + loss + metrics: head.StepHead (it also zeroes dx_out[L], whose rows 1.. nothing writes);
        # logits, dlogits, out2 and metric_acc stay reachable here under their old names
        mdl, G = self.model, self.Gr
        self.head = StepHead(mdl.norm, mdl.head, (G(mdl.head.weight), G(mdl.head.bias), G(mdl.norm.weight), G(mdl.norm.bias)),
                             self.x[self.Lyr], self.dx_out[self.Lyr], self.labels, self.hp, T, N, self.fuse_head, self.world,
                             self.pg)
        self.logits, self.dlogits, self.out2, self.metric_acc = (self.head.logits, self.head.dlogits, self.head.out2,
                                                                 self.head.metric_acc)
        self.dx_mid = [e(B, N, D) for _ in range(self.Lyr)]
        self.du_l = [e(M, self.hid) for _ in range(self.Lyr)]
        self.dqkv_l = [e(B, N, 3 * D) for _ in range(self.Lyr)]
        self.qkv_l = [] if self.attn_fused else [e(B, N, 3 * D) for _ in range(self.Lyr)]
        # extras route: dY of fc2 / proj behind the backward of their branch's dropout + drop-path (None: the branch has neither)
        on = lambda blk, p: self.extras and (p > 0. or blk.drop_path_p > 0.)  # noqa: E731
        self.g2_l = [e(B, N, D) if on(blk, blk.mlp.drop) else None for blk in self.model.blocks]
        self.g1_l = [e(B, N, D) if on(blk, blk.attn.proj_drop_p) else None for blk in self.model.blocks]
        self.dqkv, self.du = self.dqkv_l[0], self.du_l[0]          # (bench.py times the kernels on these)
        self.da_top = None
        # Class-row mode of the TOP block (route.cls_rows; DESIGN.md 4, "Top block on the class-token rows").  The model
        # pools the class token: of x[L] only row b * N is read, of dx_out[L] only that row is non-zero, so the top block's
        # tail, its backward and its fc2 / fc1 / proj weight gradients run on the B class rows.  The invariant that replaces
        # the zeros the full-row backward used to write: the non-class rows of du_l[L-1], dx_mid[L-1] and da_top are zeroed
        # HERE and never written again (the attention backward, the block below's prologue and the qkv weight gradient sum
        # over all rows).  (Not for a one-layer model: its du_l[0] is self.du, which bench.py's probes write in full.)
        if self.cls_rows:
            # the top block's own d(attention output): dtmp is shared with the layers below, which overwrite every row
            self.da_top = torch.zeros(B, N, D, dtype=T, device=dev)
            top = self.act[self.Lyr - 1]
            for t in (self.du_l[self.Lyr - 1], self.dx_mid[self.Lyr - 1], self.x[self.Lyr], top["xmid"], top["m2"], top["r2"],
                      top["u"], top["h"], top["xn2"]):
                if t is not None:   # (forward side: no kernel reads their non-class rows; a stray read finds finite zeros)
                    t.zero_()
        self.dataset, self.batch_idx = None, None
        self._wg_groups = {}
        self.dpatch = e(B * self.P, D)
        self.ln_ws = K.layernorm_bwd_workspace(M, D, dev)
        # positional-encoding operands of the fused attention kernels
        pe = self.model.pos_embed
        mode = self.model.pos_encoding_type
        self.pe = K.PETables(mode if mode != "absolute" else "none", self.grid)
        self.pe_grads = dict(dtable=None, dcoeff=None, dfreqs=None)
        if isinstance(pe, RelativePositionalEncoding):
            self.pe.table = pe.relative_position_bias_table.data
            self.pe_grads["dtable"] = self.Gr(pe.relative_position_bias_table)
        elif isinstance(pe, PolynomialRPE):
            self.pe.coeff, self.pe.degree = pe.coefficients.data, pe.degree
            self.pe.coeff_per_head = not pe.shared_across_heads
            self.pe_grads["dcoeff"] = self.Gr(pe.coefficients)
        elif isinstance(pe, RoPEAxial):
            self.pe.cos, self.pe.sin = K.rope_axial_tables(pe.inv_freq.contiguous(), self.grid)
        elif isinstance(pe, RoPEMixed):
            self.pe.cos, self.pe.sin = K.rope_mixed_tables(pe.freqs.data, self.grid)
            self.pe_grads["dfreqs"] = self.Gr(pe.freqs)

    # ---------------------------------------------------------------- dropout sites (extras)
    def _build_rng_table(self):
        """rng_table [6 * depth, 2] int64: the (seed, offset) pair of every dropout site (SITE_* order), drawn from torch's
        device generator (torch.manual_seed reproduces a run), offsets shifted by rank << 48.  The kernels read their row
        from device memory, and the optimizer's last launch adds 1 to every offset: a replayed graph draws new masks.
        Not part of state_dict(): a resumed run restores it with set_rng_table()."""
        self.rates = [(blk.attn.attn_drop_p, blk.attn.proj_drop_p, blk.mlp.drop, blk.drop_path_p) for blk in self.model.blocks]
        self.rng_table = None
        if not self.extras:
            return
        self.rng_table = shift_rng_offsets(K.new_rng_pairs(SITES_PER_LAYER * self.Lyr, self.dev), self._rank())
        self._rng_rows = [self.rng_table[i] for i in range(self.rng_table.shape[0])]   # views: set_rng_table copies in place

    def set_rng_table(self, table: torch.Tensor):
        """Copy a [6 * depth, 2] int64 table of (seed, offset) pairs in (tests; resuming a run).  Captured graphs stay
        valid: they read the table's memory."""
        if self.rng_table is None:
            raise L.VitpeError("set_rng_table: this engine was built without extras=True")
        if table.dtype != torch.int64 or tuple(table.shape) != tuple(self.rng_table.shape):
            raise L.VitpeError(f"set_rng_table: expected an int64 tensor of shape {tuple(self.rng_table.shape)}, got "
                               f"{table.dtype} {tuple(table.shape)}")
        self.rng_table.copy_(table)

    def set_augment(self, crop_pad: int = 0, hflip: bool = False, rng: Optional[torch.Tensor] = None):
        """RandomCrop(S, padding=crop_pad) + RandomHorizontalFlip (if hflip) on the training steps' input, inside the embed
        kernel's gather from the resident dataset ("Augmentation stream"); evaluation forwards never augment.
        `engine.aug_rng` [1, 2] int64 is the stream's (seed, offset) pair: drawn from torch's device generator with the
        offset shifted by rank << 48, or a copy of `rng` (two int64 words on the device) as it is; every optimizer step
        advances the offset by 1.  Not part of state_dict() (as rng_table).  The defaults switch augmentation off.
        Captured graphs are dropped."""
        crop_pad, hflip = int(crop_pad), bool(hflip)
        if not 0 <= crop_pad <= self.S:
            raise L.VitpeError(f"set_augment: crop_pad must be in 0..{self.S} (the image size), got {crop_pad}")
        if rng is not None:
            K._check_augment(rng, crop_pad, self.S, "set_augment")
        if crop_pad == 0 and not hflip:
            self.aug_rng = None
        elif rng is not None:
            self.aug_rng = rng.to(self.dev).reshape(1, 2).clone()
        else:
            self.aug_rng = new_augment_rng(self.dev, self._rank())
        self.aug_pad, self.aug_hflip = crop_pad, hflip
        self._drop_graphs()

    def _site(self, l, site, rate):
        """The site's row of the table, or None where its rate is 0 (nothing is launched for it)."""
        return self._rng_rows[site_row(l, site)] if rate > 0. else None

    def _branch_fwd(self, l, inp, lin, resid, out, site_e, p_e, site_p, p_p):
        """out = resid + drop_path(dropout(lin(inp))): the residual GEMM epilogue when both rates are 0, else the Linear into
        a scratch (dtmp: the backward's, idle during a forward) and the fused branch kernel."""
        M, D = self.M, self.D
        if p_e == 0. and p_p == 0.:
            K.linear(inp, self.Sh(lin.weight), lin.bias.data, epi=L.EPI_BIAS_RESID, resid=resid.view(M, D), out=out.view(M, D))
            return
        K.linear(inp, self.Sh(lin.weight), lin.bias.data, out=self.dtmp.view(M, D))
        K.branch_drop_fwd(self.dtmp, self._site(l, site_e, p_e), p_e, self._site(l, site_p, p_p), p_p, resid=resid, out=out)

    # ---------------------------------------------------------------- one layer, forward
    def _layer_fwd(self, l, train):
        """Layer l in one of three shapes: LayerNorm-fused attention + the block tail (tail2); LayerNorm-fused attention +
        the panel kernels (fuse_ln); the plain per-Linear chain (extras, and every geometry without the fusions)."""
        if not self.fuse_ln:
            return self._plain_layer_fwd(l, train)
        mdl, blk, a, M, D = self.model, self.model.blocks[l], self.act[l], self.M, self.D
        # LN1 inside the attention kernel's token staging; LN2 inside fc1's operand staging; their statistics come out of
        # the producing GEMM's epilogue (proj / previous fc2)
        self._attn_layer_fwd(l)
        nxt = (self.act[l + 1]["m1"], self.act[l + 1]["r1"]) if l + 1 < self.Lyr else None
        if self.tail2:   # proj + residual + LN2 + MLP branch: one kernel per block tail
            return self._block_tail_fwd(l, blk, a, nxt)
        K.linear(a["a"].view(M, D), self.Sh(blk.attn.proj.weight), blk.attn.proj.bias.data, epi=L.EPI_BIAS_RESID,
                 resid=self.x[l].view(M, D), out=a["xmid"].view(M, D), stats=(a["m2"], a["r2"]), eps=blk.norm2.eps)
        K.linear_ln(a["xmid"].view(M, D), blk.norm2.weight.data, blk.norm2.bias.data, a["m2"], a["r2"],
                    self.Sh(blk.mlp.fc1.weight), blk.mlp.fc1.bias.data, epi=L.EPI_BIAS_GELU, u=a["u"], out=a["h"],
                    xn_out=a["xn2"].view(M, D))
        K.linear(a["h"], self.Sh(blk.mlp.fc2.weight), blk.mlp.fc2.bias.data, epi=L.EPI_BIAS_RESID,
                 resid=a["xmid"].view(M, D), out=self.x[l + 1].view(M, D), stats=nxt,
                 eps=mdl.blocks[min(l + 1, self.Lyr - 1)].norm1.eps)

    def _plain_layer_fwd(self, l, train):
        """LayerNorm, qkv Linear, attention, proj + residual, LayerNorm, fc1 + GELU, fc2 + residual, one launch each.
        train: the dropout sites run at the model's rates (evaluation: none does); a site whose rate is 0 and an absent
        qkv bias launch nothing, so a model without them runs the bare chain."""
        blk, a, xin, M, D = self.model.blocks[l], self.act[l], self.x[l], self.M, self.D
        p_attn, p_proj, p_mlp, p_path = self.rates[l] if train else (0., 0., 0., 0.)
        K.layernorm_fwd(xin, blk.norm1.weight.data, blk.norm1.bias.data, blk.norm1.eps, out=a["xn1"], mean=a["m1"], rstd=a["r1"])
        if not self.attn_fused and not self.attn_fused64:
            bq = blk.attn.qkv.bias
            K.linear(a["xn1"].view(M, D), self.Sh(blk.attn.qkv.weight), None if bq is None else bq.data,
                     out=self.qkv_l[l].view(M, 3 * D))
        self._attn_layer_fwd(l, save_qkv=self._save_hidden, p_drop=p_attn)
        self._branch_fwd(l, a["a"].view(M, D), blk.attn.proj, xin, a["xmid"], SITE_PROJ, p_proj, SITE_PATH_A, p_path)
        K.layernorm_fwd(a["xmid"], blk.norm2.weight.data, blk.norm2.bias.data, blk.norm2.eps, out=a["xn2"], mean=a["m2"],
                        rstd=a["r2"])
        K.linear(a["xn2"].view(M, D), self.Sh(blk.mlp.fc1.weight), blk.mlp.fc1.bias.data, epi=L.EPI_BIAS_GELU, u=a["u"],
                 out=a["h"])
        h = a["h"]
        if p_mlp > 0.:   # the dropped activation is what fc2 reads, forward and weight gradient
            h = K.dropout_fwd(a["h"], self._site(l, SITE_MLP1, p_mlp), p_mlp, out=a["hd"])
        self._branch_fwd(l, h, blk.mlp.fc2, a["xmid"], self.x[l + 1], SITE_MLP2, p_mlp, SITE_PATH_M, p_path)

    # ---------------------------------------------------------------- one layer, backward: four steps
    def _layer_bwd(self, l, lo, hi):
        """Backward of layer l within a part that spans layers lo..hi.  With fuse_lnbwd the last step of layer l runs as the
        prologue of layer l - 1's first (one kernel per layer boundary inside the part); per-GEMM weight gradients would
        read dx_out[l] before that kernel has written it, so the pairing needs the grouped launch."""
        paired = self.fuse_lnbwd and self.group_wgrad
        self._mlp_bwd(l, pre=paired and l < hi)
        self._proj_bwd(l)
        self._attn_bwd(l, self.da_top if self._top_cls(l) else self.dtmp, p_drop=self.rates[l][0])
        self._gemm_tn(l, "qkv")
        if not (paired and l > lo):
            self._qkv_bwd(l)

    def _mlp_bwd(self, l, pre=False):
        """x_out = xmid + drop_path(drop2(fc2(drop1(gelu(fc1(LN2(xmid))))))): dx_out[l + 1] -> du_l[l], dx_mid[l].  tail2: one
        kernel, which also leaves the projection's data gradient in dtmp (da_top in class-row mode)."""
        blk, a, M, D, G = self.model.blocks[l], self.act[l], self.M, self.D, self.Gr
        _, _, p_mlp, p_path = self.rates[l]
        dy3, dmid3, du = self.dx_out[l + 1], self.dx_mid[l], self.du_l[l]
        g2 = dy3
        if self.g2_l[l] is not None:   # fc2's dY: per layer, the grouped weight-gradient launch reads it after the chain
            g2 = K.branch_drop_bwd(dy3, self._site(l, SITE_MLP2, p_mlp), p_mlp, self._site(l, SITE_PATH_M, p_path), p_path,
                                   out=self.g2_l[l])
        self._gemm_tn(l, "fc2")
        if self.tail2:   # gelu' + both data gradients + LayerNorm2 backward + residual + the projection's data gradient
            self._block_tail_bwd(l, blk, a, pre=pre)
            self._gemm_tn(l, "fc1")
            return
        K.linear(g2.view(M, D), self.St(blk.mlp.fc2.weight), None, epi=L.EPI_GELU_BWD, u=a["u"], out=du)
        if p_mlp > 0.:   # (g2 W2) . gelu'(u) . m1 / (1 - p): the two elementwise factors commute
            K.dropout_bwd(du, self._site(l, SITE_MLP1, p_mlp), p_mlp, out=du)
        self._gemm_tn(l, "fc1")
        if self.fuse_ln_bwd:   # data gradient of fc1 + LayerNorm2 backward + residual add in one kernel
            K.linear_lnbwd(du, self.St(blk.mlp.fc1.weight), a["xmid"].view(M, D), a["m2"], a["r2"], blk.norm2.weight.data,
                           dy3.view(M, D), G(blk.norm2.weight), G(blk.norm2.bias), out=dmid3.view(M, D))
            return
        K.linear(du, self.St(blk.mlp.fc1.weight), None, out=self.dtmp.view(M, D))
        K.layernorm_bwd(self.dtmp, a["xmid"], a["m2"], a["r2"], blk.norm2.weight.data, G(blk.norm2.weight), G(blk.norm2.bias),
                        dres=dy3, out=dmid3, workspace=self.ln_ws)

    def _proj_bwd(self, l):
        """xmid = x_in + drop_path(proj_drop(proj(attn))): dx_mid[l] -> dtmp, the gradient of the merged heads (tail2: the
        tail backward has already written it)."""
        blk, M, D = self.model.blocks[l], self.M, self.D
        _, p_proj, _, p_path = self.rates[l]
        g1 = self.dx_mid[l]
        if self.g1_l[l] is not None:
            g1 = K.branch_drop_bwd(g1, self._site(l, SITE_PROJ, p_proj), p_proj, self._site(l, SITE_PATH_A, p_path), p_path,
                                   out=self.g1_l[l])
        self._gemm_tn(l, "proj")
        if not self.tail2:
            K.linear(g1.view(M, D), self.St(blk.attn.proj.weight), None, out=self.dtmp.view(M, D))

    def _qkv_bwd(self, l):
        """dqkv_l[l] -> dx_out[l]: the qkv data gradient, LayerNorm1 backward and the residual add."""
        blk, a, M, D, G = self.model.blocks[l], self.act[l], self.M, self.D, self.Gr
        dqkv, dm = self.dqkv_l[l].view(M, 3 * D), self.dx_mid[l].view(M, D)
        if self.lnbwd2:          # one kernel on the wave-per-tile mapping, packed qkv.weight^T
            K.linear_lnbwd2(dqkv, self.Frt(blk.attn.qkv.weight), self.x[l].view(M, D), a["m1"], a["r1"], blk.norm1.weight.data,
                            dm, G(blk.norm1.weight), G(blk.norm1.bias), out=self.dx_out[l].view(M, D))
        elif self.fuse_ln_bwd:   # one panel kernel on the transposed shadow
            K.linear_lnbwd(dqkv, self.St(blk.attn.qkv.weight), self.x[l].view(M, D), a["m1"], a["r1"], blk.norm1.weight.data,
                           dm, G(blk.norm1.weight), G(blk.norm1.bias), out=self.dx_out[l].view(M, D))
        else:
            K.linear(dqkv, self.St(blk.attn.qkv.weight), None, out=self.dtmp.view(M, D))
            K.layernorm_bwd(self.dtmp, self.x[l], a["m1"], a["r1"], blk.norm1.weight.data, G(blk.norm1.weight),
                            G(blk.norm1.bias), dres=self.dx_mid[l], out=self.dx_out[l], workspace=self.ln_ws)

    # ---------------------------------------------------------------- forward / backward
    def _forward(self, head=True, save=False, train=False):
        """save: keep what backward needs of the MLP hidden layer (training); evaluation writes none of it.
        train (extras route): run the dropout sites; an evaluation forward applies the qkv bias and no dropout.
        train (any route): the uint8 gather crops and flips on the augmentation stream when set_augment() switched it on."""
        self._save_hidden = save
        mdl, B, N, D, M = self.model, self.B, self.N, self.D, self.M
        ape = mdl.pos_embed.pos_embed.data[0, :self.P] if isinstance(mdl.pos_embed, AbsolutePositionalEncoding) else None
        aug = {}
        if train and self.aug_rng is not None:
            if self.dataset is None:
                raise L.VitpeError(self._AUG_NEEDS_DATASET)
            aug = dict(rng=self.aug_rng, crop_pad=self.aug_pad, hflip=self.aug_hflip)
        if self.fuse_embed:   # unfold + patch GEMM + bias + APE + class token + block 0's norm1 statistics: one kernel
            src = (dict(data=self.dataset.images, index=self.batch_idx, mean=self.dataset.mean, std=self.dataset.std, **aug)
                   if self.dataset is not None else dict(images=self.images))
            b0 = mdl.blocks[0]
            K.patch_embed(self.Sh(mdl.patch_embed.weight).view(D, -1), mdl.patch_embed.bias.data, mdl.cls_token.data.view(-1),
                          ape, self.p, self.T, out=self.x[0], patches_out=self.patches,
                          stats=(self.act[0]["m1"], self.act[0]["r1"]) if self.fuse_ln else None, eps=b0.norm1.eps, **src)
        else:
            if self.dataset is not None:   # resident uint8 dataset: gather + ToTensor + Normalize inside the unfold
                K.unfold_u8(self.dataset.images, self.batch_idx, self.dataset.mean, self.dataset.std, self.p, self.T,
                            out=self.patches, **aug)
            else:
                K.unfold(self.images, self.p, self.T, out=self.patches)
            K.patch_embed_gemm(self.patches, self.Sh(mdl.patch_embed.weight).view(D, -1), mdl.patch_embed.bias.data,
                               mdl.cls_token.data.view(-1), ape, B, self.P, out=self.x[0])
            if self.fuse_ln:
                b0 = mdl.blocks[0]
                K.layernorm_fwd(self.x[0], b0.norm1.weight.data, b0.norm1.bias.data, b0.norm1.eps, mean=self.act[0]["m1"],
                                rstd=self.act[0]["r1"], stats_only=True)
        if isinstance(mdl.pos_embed, RoPEMixed):  # learnable frequencies: tables follow the parameters
            K.rope_mixed_tables(mdl.pos_embed.freqs.data, self.grid, self.pe.cos, self.pe.sin)
        for l in range(self.Lyr):
            self._layer_fwd(l, train)
        if head:
            self.head.forward()

    def _top_cls(self, l):
        return self.cls_rows and l == self.Lyr - 1

    def _block_tail_fwd(self, l, blk, a, nxt, save=None, scratch=None):
        """save: keep gelu'(u) and gelu(u) for the backward (None: what the running _forward was asked for).
        scratch (kernel_probes, class-row mode): the FULL-row kernel of the top block, its outputs sent to these buffers."""
        M, D = self.M, self.D
        if save is None:
            save = self._save_hidden
        o = scratch if scratch is not None else dict(a, xout=self.x[l + 1])
        args = (a["a"].view(M, D), self.x[l].view(M, D), self.Fr(blk.attn.proj.weight), blk.attn.proj.bias.data,
                blk.norm2.weight.data, blk.norm2.bias.data, self.Fr(blk.mlp.fc1.weight), blk.mlp.fc1.bias.data,
                self.Fr(blk.mlp.fc2.weight), blk.mlp.fc2.bias.data)
        outs = dict(x_mid=o["xmid"].view(M, D), mean2=o["m2"], rstd2=o["r2"], out=o["xout"].view(M, D),
                    xn_out=(o["xn2"].view(M, D) if (save and not self.recompute_ln) else None),
                    gp=(o["u"].view(torch.float16) if save else None), h=(o["h"] if save else None), eps2=blk.norm2.eps)
        if self._top_cls(l) and scratch is None:   # the class rows only, in place on the full-layout buffers
            K.tail_cls_fwd(*args, self.B, self.N, **outs)
        else:
            K.block_tail2_fwd(*args, stats=nxt, eps_next=self.model.blocks[min(l + 1, self.Lyr - 1)].norm1.eps, save=save,
                              **outs)

    def _block_tail_bwd(self, l, blk, a, pre=False, scratch=None):
        """pre: the qkv data gradient + LayerNorm1 backward of block l + 1 run first in the same kernel and produce
        dx_out[l + 1] (this block's dy).  scratch: as in _block_tail_fwd."""
        M, D, G = self.M, self.D, self.Gr
        o = scratch if scratch is not None else dict(a, du=self.du_l[l], dxmid=self.dx_mid[l])
        args = (self.dx_out[l + 1].view(M, D), o["u"].view(torch.float16), self.Frt(blk.mlp.fc2.weight),
                self.Frt(blk.mlp.fc1.weight), o["xmid"].view(M, D), o["m2"], o["r2"], blk.norm2.weight.data,
                G(blk.norm2.weight), G(blk.norm2.bias), self.Frt(blk.attn.proj.weight))
        outs = dict(du=o["du"], out=o["dxmid"].view(M, D))
        if self._top_cls(l) and scratch is None:
            K.tail_cls_bwd(*args, self.B, self.N, da=self.da_top.view(M, D), **outs)
        elif pre and scratch is None:
            up, ua = self.model.blocks[l + 1], self.act[l + 1]
            K.block_tail2_bwd_pre(self.dqkv_l[l + 1].view(M, 3 * D), self.Frt(up.attn.qkv.weight), self.x[l + 1].view(M, D),
                                  ua["m1"], ua["r1"], up.norm1.weight.data, self.dx_mid[l + 1].view(M, D), G(up.norm1.weight),
                                  G(up.norm1.bias), *args, da=self.dtmp.view(M, D), **outs)
        else:
            K.block_tail2_bwd(*args, da=self.dtmp.view(M, D), **outs)

    def _tail_bytes(self, fwd: bool) -> int:
        """Algorithmic HBM bytes of one block-tail launch (what the kernel must read and write once)."""
        M, D, hid, es = self.M, self.D, self.hid, 2 if self.T == torch.bfloat16 else 4
        if fwd:   # attention output + x in; x_mid, x_out (and LN2(x_mid) unless recomputed) out; u and h out (2 x [M,hid])
            return ((4 if self.recompute_ln else 5) * M * D + 2 * M * hid) * es
        return (4 * M * D + 2 * M * hid) * es   # dy, x_mid in; d x_mid, d attn out; u in, du out

    _AUG_NEEDS_DATASET = ("augmentation is on (set_augment) but no resident dataset is attached: the crop and the flip run "
                          "inside the gather from the uint8 dataset -- attach_dataset() + step_indexed(), or augment the "
                          "images yourself with vitpe.data.augment_batch and switch it off (set_augment())")

    def _fwd_train(self):
        self._forward(head=not self.fuse_head, save=True, train=True)

    def _loss(self, tick=True):
        """tick: this loss belongs to a full step -- the fused head launch also advances the optimizer's step counter."""
        self.head.loss(tick)

    def _wgrad_problems(self, l):
        """Layer l's four nn.Linear weight gradients as (dY, X, dW, dbias[, ln[, row_step]]), in launch order: the operands
        of the grouped launch and of the per-Linear comparator alike."""
        blk, a, D, M, G = self.model.blocks[l], self.act[l], self.D, self.M, self.Gr
        # extras route: dY behind the branch's dropout / drop-path backward, X the dropped hidden activation
        g2 = self.g2_l[l] if self.g2_l[l] is not None else self.dx_out[l + 1]
        g1 = self.g1_l[l] if self.g1_l[l] is not None else self.dx_mid[l]
        fc2 = (g2.view(M, D), a["hd"] if a["hd"] is not None else a["h"], G(blk.mlp.fc2.weight), G(blk.mlp.fc2.bias))
        proj = (g1.view(M, D), a["a"].view(M, D), G(blk.attn.proj.weight), G(blk.attn.proj.bias))
        if self.recompute_ln:   # X operands LayerNorm2(x_mid) / LayerNorm1(x_in): re-normalised inside the kernel
            fc1 = (self.du_l[l], a["xmid"].view(M, D), G(blk.mlp.fc1.weight), G(blk.mlp.fc1.bias),
                   (a["m2"], a["r2"], blk.norm2.weight.data, blk.norm2.bias.data))
            qkv = (self.dqkv_l[l].view(M, 3 * D), self.x[l].view(M, D), G(blk.attn.qkv.weight), None,
                   (a["m1"], a["r1"], blk.norm1.weight.data, blk.norm1.bias.data))
        else:
            fc1 = (self.du_l[l], a["xn2"].view(M, D), G(blk.mlp.fc1.weight), G(blk.mlp.fc1.bias))
            bq = blk.attn.qkv.bias   # (extras route only)
            qkv = (self.dqkv_l[l].view(M, 3 * D), a["xn1"].view(M, D), G(blk.attn.qkv.weight), None if bq is None else G(bq))
        if self._top_cls(l):   # their dY is zero outside the class rows: contract over rows b * N only (row step N)
            fc2, fc1, proj = ((p + (None,) * (5 - len(p)) + (self.N,)) for p in (fc2, fc1, proj))
        return dict(fc2=fc2, fc1=fc1, proj=proj, qkv=qkv)

    def _embed_wgrad(self):
        mdl, G = self.model, self.Gr
        return (self.dpatch, self.patches, G(mdl.patch_embed.weight).view(self.D, -1), G(mdl.patch_embed.bias))

    def _part_layers(self, part):
        """(hi, lo) of part "all" | "upper" (head + layers L-1..split) | "lower" (layers split-1..0 + patch embed)."""
        top, split = self.Lyr - 1, self.split_layer
        return {"all": (top, 0), "upper": (top, split), "lower": (split - 1, 0)}[part]

    def _wgrad_group(self, part):
        """All weight gradients of `part` in one grouped launch (csrc/wgrad.hip) after the data-gradient chain:
        their operands sit in per-layer buffers, so nothing forces them into the chain, and one launch over
        24+ problems needs ~10x fewer atomically-combined partial blocks than 24 launches."""
        if part not in self._wg_groups:
            hi, lo = self._part_layers(part)
            probs = [p for l in range(hi, lo - 1, -1) for p in self._wgrad_problems(l).values()]
            if part != "upper":
                probs.append(self._embed_wgrad())
            # lists above the kernel-argument limit (ViT-B/16: 49 problems) go out as equal launches (25 + 24, not 28 + 21:
            # the placement of blocks over the chip works per launch)
            ng = -(-len(probs) // K.WgradGroup.MAX)
            per = -(-len(probs) // ng)
            self._wg_groups[part] = [K.WgradGroup(probs[i:i + per]) for i in range(0, len(probs), per)]
        for grp in self._wg_groups[part]:
            grp.launch()

    def _gemm_tn(self, l, name):
        """Layer l's weight gradient `name` as its own GEMM at this point of the chain (VITPE_GROUP_WGRAD=0); the default
        leaves it to _wgrad_group."""
        if not self.group_wgrad:
            K.gemm_tn(*self._wgrad_problems(l)[name])

    def _backward(self, part="all"):
        """part: "all" | "upper" (head + layers L-1..split) | "lower" (layers split-1..0 + patch embed)."""
        mdl, G = self.model, self.Gr
        hi, lo = self._part_layers(part)
        if part != "lower" and not self.fuse_head:
            self.head.backward()
        for l in range(hi, lo - 1, -1):
            self._layer_bwd(l, lo, hi)
        if part != "upper":
            dape = None
            if isinstance(mdl.pos_embed, AbsolutePositionalEncoding):
                dape = G(mdl.pos_embed.pos_embed)[0, :self.P]
            K.embed_bwd(self.dx_out[0], G(mdl.cls_token).view(-1), dape, out=self.dpatch)
            if not self.group_wgrad:
                K.gemm_tn(*self._embed_wgrad())
        if self.group_wgrad:
            self._wgrad_group(part)

    def _optimizer(self):
        self.opt.launch(self.head.ticked)
        self.head.ticked = False
        self.refresh_shadows(cast_flat=False)
        if self.extras:   # the step's last launch, after the backward has regenerated the forward's masks: the next step
            K.rng_advance(self.rng_table, 1)   # (or replay) draws new ones.  Once per step in every step shape
        if self.aug_rng is not None:   # likewise the augmentation stream: the next step crops and flips anew
            K.rng_advance(self.aug_rng, 1)

    def _allreduce(self):
        if self.allpairs is not None:
            self.allpairs(self.flat_g)
        else:
            ddp.allreduce_sum_(self.flat_g, self.pg)

    # ---------------------------------------------------------------- public API
    def set_valid(self, n_valid: int, n_valid_global: Optional[int] = None):
        """Rows [0, n_valid) of the next steps' batches are real samples, `n_valid_global` over all ranks:
        StepHead.set_valid."""
        self.head.set_valid(n_valid, n_valid_global)

    def sync_from_model(self):
        """Re-derive every weight shadow (bf16 flat copy, transposed copies, packed qkv weights) from the fp32 master
        parameters: call after editing parameters behind the engine's back (load_state_dict does it by itself)."""
        self.refresh_shadows()

    def broadcast_parameters(self, src=0):
        """Initial parameter broadcast from rank 0 so all replicas start identical."""
        if self.world > 1:
            ddp.broadcast_(self.flat_p, src, self.pg)
            self.refresh_shadows()
        if self.opt.ema_decay is not None:   # the average of parameters that have just been replaced means nothing
            self.reset_ema()

    def capture(self):
        """Warm up on a side stream, then capture forward+loss+backward (and, single-GPU, the
        optimizer) into HIP graphs.  Engine state is restored after the warm-up."""
        self.opt.guard("capture")
        # everything the two warm-up steps move: the head and the optimizer list their own (state_tensors)
        state = [self.flat_p, *self.head.state_tensors(), *self.opt.state_tensors(),
                 *(t for t in (self.rng_table, self.aug_rng) if t is not None)]
        snap = [t.clone() for t in state]
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                self._fwd_train(); self._loss(); self._backward(); self._optimizer()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        for t, c in zip(state, snap):
            t.copy_(c)
        self.flat_g.zero_()
        self.refresh_shadows()
        torch.cuda.synchronize()
        if self.ddp_graph:
            try:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    self._fwd_train(); self._loss()
                    if self.overlap_comm:
                        self._backward("upper")
                        side, main = torch.cuda.Stream(), torch.cuda.current_stream()
                        side.wait_stream(main)                        # fork: bucket 1 (head + upper layers) ...
                        with torch.cuda.stream(side):
                            dist.all_reduce(self.flat_g[self.bucket_off:], op=dist.ReduceOp.SUM, group=self.pg)
                        self._backward("lower")                       # ... beside the lower layers' backward
                        dist.all_reduce(self.flat_g[:self.bucket_off], op=dist.ReduceOp.SUM, group=self.pg)
                        main.wait_stream(side)                        # join
                    else:
                        self._backward()
                        self._allreduce()
                    self._optimizer()
                torch.cuda.synchronize()
                self.graph_fb, self.graph_fb2, self.graph_opt = g, None, None
                return
            except Exception as exc:   # noqa: BLE001  (communicator does not support capture here: the stitched path below)
                import warnings
                warnings.warn(f"VITPE_DDP_GRAPH: capturing the all-reduces failed ({exc!r}); using the host-stitched step")
                self.ddp_graph = False
                torch.cuda.synchronize()
                self.flat_g.zero_()
        # thread_local: a communicator watchdog thread touching the device must not invalidate the capture
        self.graph_fb = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph_fb, capture_error_mode="thread_local"):
            self._fwd_train(); self._loss()
            if self.world == 1:
                self._backward(); self._optimizer()
            elif self.overlap_comm:
                self._backward("upper")
            else:
                self._backward()
        if self.world > 1:
            if self.overlap_comm:
                self.graph_fb2 = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self.graph_fb2, capture_error_mode="thread_local"):
                    self._backward("lower")
            self.graph_opt = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph_opt, capture_error_mode="thread_local"):
                self._optimizer()
        torch.cuda.synchronize()

    def attach_dataset(self, dataset):
        """Feed the engine from a `vitpe.data.ResidentDataset` (uint8 images in HBM): steps then take sample
        indices (`step_indexed`) instead of image tensors.  `None` detaches.  Captured graphs are dropped."""
        if dataset is self.dataset:
            return
        if dataset is not None:
            C, S = dataset.images.shape[1], dataset.images.shape[2]
            if (C, S) != (self.C, self.S) or dataset.images.device != self.dev:
                raise L.VitpeError(f"dataset is {C}x{S}x{S} on {dataset.images.device}, engine expects "
                                   f"{self.C}x{self.S}x{self.S} on {self.dev}")
            if self.batch_idx is None:
                self.batch_idx = torch.zeros(self.B, dtype=torch.int64, device=self.dev)
        self.dataset = dataset
        self._drop_graphs()

    def _load_indices(self, idx: torch.Tensor, dataset=None):
        """Sample indices of the next batch: [n] int64 with n <= B; a short (ragged last) batch is padded by repeating
        its first index -- the padded rows are masked out of loss / accuracy / gradients by set_valid()."""
        dataset = dataset if dataset is not None else self.dataset
        if dataset is None:
            raise L.VitpeError("no dataset attached (TrainEngine.attach_dataset)")
        n = idx.shape[0] if idx.dim() == 1 else -1
        if not (1 <= n <= self.B) or idx.dtype != torch.int64:
            raise L.VitpeError(f"expected 1..{self.B} int64 sample indices, got {tuple(idx.shape)} {idx.dtype}")
        if n < self.B:
            self.batch_idx.fill_(idx[0])
            self.batch_idx[:n].copy_(idx, non_blocking=True)
        else:
            self.batch_idx.copy_(idx, non_blocking=True)
        torch.index_select(dataset.labels, 0, self.batch_idx, out=self.labels)
        return n

    def step_indexed(self, idx: torch.Tensor, n_valid_global: Optional[int] = None, n_valid: Optional[int] = None):
        """One training step on samples `idx` [n <= B] (int64, device) of the attached resident dataset.  A ragged
        batch (n < B; the reference DataLoader has no drop_last, train.py:89-90) runs through the same captured
        graph with the padding masked on the device.  `n_valid_global`: size of the global batch over all ranks
        (default n * world); `n_valid` < n marks trailing indices as padding too (a rank with an empty share)."""
        self.opt.guard("step_indexed")
        n = self._load_indices(idx)
        self.set_valid(n if n_valid is None else min(n, n_valid), n_valid_global)
        self.step()

    def forward_indexed(self, idx: torch.Tensor, dataset=None) -> torch.Tensor:
        """Logits [n, classes] for samples `idx` [n <= B] of `dataset` (default: the attached one), eager forward
        (evaluation); the labels land in `self.labels[:n]`.  Another dataset does not disturb the captured graphs."""
        keep = self.dataset
        if dataset is not None:
            if self.batch_idx is None:
                self.batch_idx = torch.zeros(self.B, dtype=torch.int64, device=self.dev)
            self.dataset = dataset
        try:
            n = self._load_indices(idx)
            self._forward()
        finally:
            self.dataset = keep
        return self.logits[:n]

    def _load_batch(self, images, labels):
        n = images.shape[0]
        if not (1 <= n <= self.B) or tuple(images.shape[1:]) != tuple(self.images.shape[1:]):
            raise L.VitpeError(f"engine was built for batches of up to {self.B} x {tuple(self.images.shape[1:])}, "
                               f"got {tuple(images.shape)}")
        if n < self.B:   # ragged batch: pad with copies of its first image (masked by set_valid)
            self.images.copy_(images[:1].expand_as(self.images))
            self.images[:n].copy_(images, non_blocking=True)
            if labels is not None:
                self.labels.fill_(0)
                self.labels[:n].copy_(labels, non_blocking=True)
        else:
            self.images.copy_(images, non_blocking=True)
            if labels is not None:
                self.labels.copy_(labels, non_blocking=True)
        return n

    def step(self, images: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None,
             n_valid_global: Optional[int] = None, exchange: bool = True):
        """One training step (train.py:109-116).  `images` [n,C,S,S] fp32 / `labels` [n] int64 on the device with
        n <= B (a ragged last batch is padded and masked, see set_valid); None re-uses the resident batch.  No host
        synchronisation.  `exchange=False` skips the gradient all-reduce (measurement of the exposed communication
        time only: the replicas diverge)."""
        self.opt.guard("step")
        if self.aug_rng is not None and self.dataset is None:   # never train silently without the crop
            raise L.VitpeError(self._AUG_NEEDS_DATASET)
        if images is not None:
            if self.dataset is not None:
                raise L.VitpeError("a resident dataset is attached: use step_indexed (or attach_dataset(None))")
            self.set_valid(self._load_batch(images, labels), n_valid_global)
        if self.use_graph:
            if self.graph_fb is None:
                self.capture()
            self.graph_fb.replay()
            if self.world > 1 and not self.ddp_graph:      # (ddp_graph: the exchange is part of the replayed graph)
                if self.overlap_comm:
                    # bucket 1 (upper layers + head) is exchanged while the lower layers' backward runs
                    w1 = w2 = None
                    if exchange and self.allpairs is not None:
                        # the all-pairs exchange is a composite (all-to-all, local sum, all-gather): bucket 1 on a side
                        # stream so that the main stream goes on with the lower layers' backward
                        main = torch.cuda.current_stream()
                        self._comm_stream.wait_stream(main)
                        with torch.cuda.stream(self._comm_stream):
                            self.allpairs(self.flat_g[self.bucket_off:])
                        self.graph_fb2.replay()
                        self.allpairs(self.flat_g[:self.bucket_off])
                        main.wait_stream(self._comm_stream)
                        self.graph_opt.replay()
                        self.steps_done += 1
                        return
                    if exchange:
                        w1 = dist.all_reduce(self.flat_g[self.bucket_off:], op=dist.ReduceOp.SUM, group=self.pg, async_op=True)
                    self.graph_fb2.replay()
                    if exchange:
                        w2 = dist.all_reduce(self.flat_g[:self.bucket_off], op=dist.ReduceOp.SUM, group=self.pg, async_op=True)
                        w1.wait(); w2.wait()
                elif exchange:
                    self._allreduce()
                self.graph_opt.replay()
        else:
            self._fwd_train(); self._loss(); self._backward()
            if exchange:
                self._allreduce()
            self._optimizer()
        self.steps_done += 1

    def forward_backward(self):
        """forward + loss + backward on the resident batch without the optimizer (tests / parity)."""
        self.opt.guard("forward_backward")
        self._fwd_train(); self._loss(tick=False); self._backward()

    def forward_only(self, images: torch.Tensor, labels: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Logits [n, classes] of `images` [n <= B, C, S, S] (eager forward on the same kernels); `labels` [n], when
        given, are loaded (and padded) with them for a following eval_loss."""
        if self.dataset is not None:
            raise L.VitpeError("a resident dataset is attached: use forward_indexed (or attach_dataset(None))")
        n = self._load_batch(images, labels)
        self._forward()
        return self.logits[:n]

    def kernel_probes(self):
        """The heavy kernels of the step as (name, [one launch closure per layer], algorithmic flop, algorithmic HBM
        bytes per launch) on the engine's OWN per-layer operands, in the variants the step runs (LayerNorm-fused
        attention with the xn side output, block tails, grouped weight gradients): bench.py rotates over the layers'
        buffers so that no launch finds its input in L2, and prices each against min(MFMA peak, HBM peak x AI).
        Gradients accumulate garbage meanwhile: callers zero flat_g afterwards."""
        if self.extras:
            raise NotImplementedError("kernel_probes: not available on an extras=True engine (the probes price the fused "
                                      "default route's kernels; build the engine without extras)")
        mdl, M, D, B, N, Hh, hid = self.model, self.M, self.D, self.B, self.N, self.H, self.hid
        G, es = self.Gr, 2 if self.T == torch.bfloat16 else 4
        hd = D // Hh
        probes = []
        attn_core_flop = 2 * 2 * N * N * hd * Hh * B
        qkv_flop = 2 * M * D * 3 * D
        # the step's own attention calls, on every layer's buffers (the backward reads dx_mid[l] where the step reads dtmp)
        attn_fwd = [(lambda l=l: self._attn_layer_fwd(l)) for l in range(self.Lyr)]
        attn_bwd = [(lambda l=l: self._attn_bwd(l, self.dx_mid[l])) for l in range(self.Lyr)]
        if self.attn_fused:
            probes.append(dict(name="attn_fwd", kernel=("attn32_fwd_kernel" if self.attn_wide else "attn_fwd_kernel") +
                               " (fused LN1+QKV-project+RoPE+QK^T+softmax+AV)",
                               fns=attn_fwd, flop=qkv_flop + attn_core_flop,
                               bytes=2 * M * D * es))           # x in, merged heads out (49 920 B / image)
            if not self.fuse_ln:
                probes[-1]["kernel"] = probes[-1]["kernel"].replace("fused LN1+", "fused ")
            probes.append(dict(name="attn_bwd", kernel="attn_bwd_kernel (recompute + dQ/dK/dV + PE gradients -> d_qkv)",
                               fns=attn_bwd, flop=2 * (qkv_flop + attn_core_flop),
                               bytes=(2 + 3) * M * D * es))     # xn, dout in; d_qkv out
        else:
            if self.attn_fused64:   # what the step runs: projection + PE + core in one kernel, raw projection written once
                probes.append(dict(name="attn_fwd", kernel="attn_fused64_fwd_kernel (QKV-project+RoPE+QK^T+softmax+AV per (image, head), + raw qkv out)",
                                   fns=attn_fwd, flop=qkv_flop + attn_core_flop, bytes=(1 + 3 + 1) * M * D * es))
            else:
                probes.append(dict(name="attn_fwd", kernel="attn_core_fwd_kernel (RoPE+QK^T+softmax+AV per (image, head))",
                                   fns=attn_fwd, flop=attn_core_flop, bytes=4 * M * D * es))
            probes.append(dict(name="attn_bwd", kernel="attn_core_bwd_kernel", fns=attn_bwd, flop=2 * attn_core_flop,
                               bytes=(3 + 1 + 3) * M * D * es))
        if self.tail2 and self.group_wgrad:
            def scr(l):
                # class-row mode: the probes time the FULL-row kernels, which write every row -- on the top block's live buffers
                # that would break the zero invariant of every later step, so its launches write to buffers of their own
                if not self._top_cls(l):
                    return None
                if self._probe_scratch is None:
                    z = lambda *s, dt=self.T: torch.zeros(*s, dtype=dt, device=self.dev)  # noqa: E731
                    zf = lambda *s: torch.zeros(*s, dtype=torch.float32, device=self.dev)  # noqa: E731
                    self._probe_scratch = dict(xmid=z(B, N, D), m2=zf(M), r2=zf(M), u=z(M, hid), h=z(M, hid),
                                               xn2=(None if self.recompute_ln else z(B, N, D)), xout=z(B, N, D),
                                               du=z(M, hid), dxmid=z(B, N, D))
                return self._probe_scratch
            def tail_f(l):
                blk, a = mdl.blocks[l], self.act[l]
                nxt = (self.act[l + 1]["m1"], self.act[l + 1]["r1"]) if l + 1 < self.Lyr else None
                sc = scr(l)
                return lambda: self._block_tail_fwd(l, blk, a, nxt, save=True, scratch=sc)   # the TRAINING instantiation, whatever ran last
            def tail_b(l):
                blk, a, sc = mdl.blocks[l], self.act[l], scr(l)
                return lambda: self._block_tail_bwd(l, blk, a, scratch=sc)
            tail_flop = 2 * M * D * D + 2 * 2 * M * D * hid
            probes.append(dict(name="block_tail_fwd",
                               kernel="block_tail2_fwd_kernel" +
                               " (proj+residual+LN2+fc1+GELU+fc2+residual+stats)",
                               fns=[tail_f(l) for l in range(self.Lyr)], flop=tail_flop,
                               bytes=self._tail_bytes(fwd=True)))
            probes.append(dict(name="block_tail_bwd",
                               kernel="block_tail2_bwd_kernel" +
                               " (gelu'+dgrad fc2/fc1+LN2 bwd+residual+dgrad proj)",
                               fns=[tail_b(l) for l in range(self.Lyr)], flop=tail_flop,
                               bytes=self._tail_bytes(fwd=False)))
            if self.fuse_lnbwd and self.Lyr > 1:
                def tail_bp(l):
                    blk, a = mdl.blocks[l], self.act[l]
                    return lambda: self._block_tail_bwd(l, blk, a, pre=True)
                # what the step runs between blocks: block l + 1's qkv data gradient + LayerNorm1 backward, then block l's
                # tail backward; dy is written once (the weight gradients read it) and not read back
                probes.append(dict(name="block_tail_bwd_pre",
                                   kernel="block_tail2_bwd_kernel<PRE> (dgrad qkv + LN1 bwd of the block above, then the tail backward)",
                                   fns=[tail_bp(l) for l in range(self.Lyr - 1)], flop=tail_flop + 2 * M * D * 3 * D,
                                   bytes=self._tail_bytes(fwd=False) + (3 * M * D + 2 * M * D) * es))
            if self.lnbwd2:
                probes.append(dict(name="dgrad_qkv_ln1_bwd", kernel="ln_bwd2_kernel (dgrad qkv + LayerNorm1 backward + residual)",
                                   fns=[(lambda l=l: self._qkv_bwd(l)) for l in range(self.Lyr)], flop=2 * M * D * 3 * D,
                                   bytes=(3 * M * D + 3 * M * D) * es))     # d_qkv, x, d x_mid in; d x out
            self._wgrad_group("all") if "all" not in self._wg_groups else None
            wg_flop = sum(2 * dy.shape[0] * dy.shape[1] * x.shape[1] for grp in self._wg_groups["all"] for dy, x, _, _ in grp.keep)
            wg_bytes = sum((dy.numel() + x.numel()) * es + dw.numel() * 4 for grp in self._wg_groups["all"] for dy, x, dw, _ in grp.keep)
            probes.append(dict(name="wgrad_group", kernel="wgrad_group_kernel (every nn.Linear weight gradient, one launch)",
                               fns=[lambda: self._wgrad_group("all")], flop=wg_flop, bytes=wg_bytes))
        return probes

    def eval_loss(self, n: int, acc: torch.Tensor, n_global: Optional[int] = None):
        """acc[0] += this rank's part of the batch-mean cross-entropy of rows [0, n) of the current logits vs self.labels,
        acc[1] += #correct, on the device: StepHead.eval_loss."""
        self.head.eval_loss(n, acc, n_global)

    def read_metrics(self, reset=True):
        """(sum since the last read of the global-batch mean loss, #correct over all ranks); the ONLY host sync:
        StepHead.read_metrics."""
        return self.head.read_metrics(reset)
