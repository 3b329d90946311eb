"""The optimizer side of the train step: everything that runs on the flat buffers between the backward and the next forward
("Optimizer side of the step").

StepOptimizer owns the state (AdamW moments, the hp block, the clip's work buffer, the weight EMA, the parameter-group map and
the schedule block), its configuration, and the order of the launches; TrainEngine forwards its public methods here.  The
argument checkers and the parameter-group builders are plain functions: host code, usable on a CPU model.  Constructing a
StepOptimizer and configuring it needs no device beyond the one its tensors live on; only launch(), current_lr() and
grad_norm() run kernels or synchronise.  One more call reaches the library: switching the clip ON asks
vitpe_grad_clip_blocks, a host-only function, for the size of the work buffer, so that needs libvitpe.so loaded (no device).
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib as L
from . import kernels as K
from ._lib import (HP_EMA_DECAY, HP_EMA_ORIGIN, HP_GRAD_SCALE, HP_LR, HP_MAX_NORM, HP_STEP, HP_TOTAL_NORM, HP_WEIGHT_DECAY,
                   SCHED_BASE_LR, SCHED_ORIGIN, SCHED_START_FACTOR)
from .route import ALIGN


# ---------------------------------------------------------------- parameter groups (host code)
def vit_layer_id(name: str, depth: int) -> int:
    """Layer index of parameter `name` for layer-wise learning-rate decay (timm's rule): 0 for the patch embedding, the
    class token and the position parameters, i + 1 for blocks.i.*, depth + 1 for the final norm and the head."""
    if name.startswith("blocks."):
        return int(name.split(".")[1]) + 1
    if name == "cls_token" or name.startswith(("patch_embed.", "pos_embed.")):
        return 0
    return depth + 1


def vit_param_groups(model, no_decay: bool = True, layer_decay: Optional[float] = None):
    """The AdamW parameter groups ViT recipes use, as set_param_groups takes them (pure host code: works on a CPU model).
    no_decay: weight_decay_scale 0 for parameters with ndim <= 1 (LayerNorm gains, biases), cls_token and everything under
    pos_embed. (the absolute table, the relative bias table, the polynomial coefficients, the rope-mixed freqs).
    layer_decay = d: lr_scale = d ** (depth + 1 - vit_layer_id(name)).  Every parameter is in exactly one group; a group
    also carries its "names" and, with layer_decay, its "layer_id" (set_param_groups ignores both)."""
    if layer_decay is not None and not (math.isfinite(float(layer_decay)) and float(layer_decay) > 0.0):
        raise L.VitpeError(f"vit_param_groups: layer_decay must be None or a finite number > 0, got {layer_decay!r}")
    depth = len(model.blocks)
    groups: Dict[tuple, dict] = {}
    for name, prm in model.named_parameters():
        skip = no_decay and (prm.ndim <= 1 or name == "cls_token" or name.startswith("pos_embed."))
        lid = vit_layer_id(name, depth) if layer_decay is not None else None
        key = (lid, skip)
        if key not in groups:
            groups[key] = {"params": [], "names": [], "layer_id": lid,
                           "lr_scale": 1.0 if lid is None else float(layer_decay) ** (depth + 1 - lid),
                           "weight_decay_scale": 0.0 if skip else 1.0}
        groups[key]["params"].append(prm)
        groups[key]["names"].append(name)
    return list(groups.values())


def torch_param_groups(groups, lr: float, weight_decay: float):
    """`groups` (vit_param_groups / set_param_groups format) as torch.optim.AdamW's param groups: the module path's
    equivalent of set_param_groups on an engine built with the same lr and weight_decay."""
    return [{"params": list(g["params"]), "lr": lr * float(g.get("lr_scale", 1.0)),
             "weight_decay": weight_decay * float(g.get("weight_decay_scale", 1.0))} for g in groups]


def param_granule_map(spans, n_flat: int):
    """uint8 [n_flat / ALIGN]: the group of every ALIGN-element granule of the flat buffers.  spans: (offset, numel, group)
    per parameter (offsets are multiples of ALIGN, so no granule spans two parameters: a parameter's last granule is its
    group's together with the zero padding in it, which every group leaves zero); a granule no parameter covers is group 0."""
    assert n_flat % ALIGN == 0
    gid = np.zeros(n_flat // ALIGN, dtype=np.uint8)
    for off, numel, k in spans:
        assert off % ALIGN == 0 and 0 <= k < 256
        gid[off // ALIGN:(off + numel + ALIGN - 1) // ALIGN] = k
    return gid


# ---------------------------------------------------------------- argument checkers (host code)
def group_scales(groups):
    """set_param_groups' argument, checked as far as host logic goes: [(params, lr_scale, weight_decay_scale)], or None
    for None / [].  VitpeError for a malformed group, a scale that is not finite and >= 0, a parameter listed twice or
    more than 255 groups (the map is one byte per granule; group 0 is the unlisted parameters')."""
    if groups is None or len(groups) == 0:
        return None
    out, seen = [], set()
    for grp in groups:
        if not isinstance(grp, dict) or "params" not in grp:
            raise L.VitpeError("set_param_groups: every group is a dict with a 'params' list")
        scales = []
        for key in ("lr_scale", "weight_decay_scale"):
            try:
                value = float(grp.get(key, 1.0))
            except (TypeError, ValueError):
                value = float("nan")
            if not math.isfinite(value) or value < 0.0:
                raise L.VitpeError(f"set_param_groups: {key} must be a finite number >= 0, got {grp.get(key)!r}")
            scales.append(value)
        params = list(grp["params"])
        for prm in params:
            if id(prm) in seen:
                raise L.VitpeError("set_param_groups: a parameter is listed twice")
            seen.add(id(prm))
        out.append((params, scales[0], scales[1]))
    if len(out) > 255:
        raise L.VitpeError(f"set_param_groups: at most 255 groups, got {len(out)}")
    return out


def sched_values(base_lr, total_steps, warmup_steps, min_lr, warmup_factor, done):
    """set_lr_schedule's arguments as (base, min, W, T, s0, done), or None for base_lr None; VitpeError unless
    T > W >= 0, 0 < s0 <= 1, 0 <= min_lr <= base_lr, done >= 0, all finite (T and done below 2^24: fp32 counters)."""
    if base_lr is None:
        return None
    try:
        base, lo, s0 = float(base_lr), float(min_lr), float(warmup_factor)
        T, W, dn = int(total_steps), int(warmup_steps), int(done)
        whole = (T == total_steps and W == warmup_steps and dn == done)
    except (TypeError, ValueError, OverflowError):
        base, whole = float("nan"), False
    if not (whole and all(math.isfinite(x) for x in (base, lo, s0)) and 0.0 <= lo <= base and 0.0 < s0 <= 1.0
            and 0 <= W < T < 2 ** 24 and 0 <= dn < 2 ** 24):
        raise L.VitpeError(f"set_lr_schedule: needs total_steps > warmup_steps >= 0, 0 < warmup_factor <= 1, "
                           f"0 <= min_lr <= base_lr and done >= 0, got base_lr={base_lr!r} total_steps={total_steps!r} "
                           f"warmup_steps={warmup_steps!r} min_lr={min_lr!r} warmup_factor={warmup_factor!r} done={done!r}")
    return base, lo, W, T, s0, dn


def ema_value(decay) -> Optional[float]:
    """set_ema's decay argument as it is kept: None for None / 0 (off), the float for 0 < decay < 1; VitpeError for
    anything else."""
    value = 0.0 if decay is None else float(decay)
    if not (math.isfinite(value) and 0.0 <= value < 1.0):
        raise L.VitpeError(f"set_ema: decay must be None, 0 or a number in (0, 1), got {decay!r}")
    return value if value > 0.0 else None


def clip_value(max_norm) -> Optional[float]:
    """set_grad_clip's argument as it is kept: None for None / 0 (off), the float for a finite max_norm > 0; VitpeError for
    anything else."""
    value = 0.0 if max_norm is None else float(max_norm)
    if not math.isfinite(value) or value < 0.0:
        raise L.VitpeError(f"set_grad_clip: max_norm must be None or a finite number >= 0, got {max_norm!r}")
    return value if value > 0.0 else None


class StepOptimizer:
    """AdamW on the flat buffers with everything the step runs around it.  flat_p / flat_g: the fp32 parameters and
    gradients; flat_s: the bf16 copy of flat_p AdamW keeps current (None under fp32); offsets: {id(parameter): offset into
    the flat buffers}; drop_graphs: called whenever a change makes the captured step stale."""

    def __init__(self, flat_p, flat_g, flat_s, lr, weight_decay, betas, eps, world, offsets, n_flat, drop_graphs):
        self.flat_p, self.flat_g, self.flat_s = flat_p, flat_g, flat_s
        self.offsets, self.n_flat, self._drop_graphs = offsets, n_flat, drop_graphs
        self.flat_m, self.flat_v = torch.zeros_like(flat_p), torch.zeros_like(flat_p)
        self.hp = torch.zeros(L.HP_COUNT, dtype=torch.float32, device=flat_p.device)   # the slots: include/vitpe.h
        self.hp[HP_LR:HP_WEIGHT_DECAY + 1] = torch.tensor([lr, betas[0], betas[1], eps, weight_decay], dtype=torch.float32)
        self.hp[HP_GRAD_SCALE] = 1.0 / world
        self.clip_max_norm = self._clip_partial = None     # set_grad_clip(): None = clipping off; the clip's work buffer
        self.ema_decay = self.flat_e = None                # set_ema(): None = no average kept
        self.ema_warmup = self.ema_swapped = False         # ema_swapped: TrainEngine.ema_weights() has flat_p and flat_e exchanged
        self.param_groups = self._gid = self._gid_host = self._gtab = None   # set_param_groups(): None = one group
        self.lr_sched = self._sched = None                 # set_lr_schedule(): None = hp[HP_LR] moves only by set_lr()

    # ---------------------------------------------------------------- the step
    def launch(self, ticked: bool):
        """The optimizer's launches of one step, in order: schedule, clip, AdamW (one group or parameter groups), EMA.
        ticked: the head's launch already advanced the step counter and bias corrections."""
        clip = self.clip_max_norm is not None
        if self.lr_sched is not None:   # hp[HP_LR] of this step, before anything reads it
            K.lr_schedule(self.hp, self._sched, ticked=ticked)
        if clip:   # after every all-reduce in every step shape: all ranks reduce the same flat_g to the same coefficient
            K.grad_clip(self.flat_g, self.hp, self._clip_partial)
        if self.param_groups is None:
            K.adamw_step(self.flat_p, self.flat_g, self.flat_m, self.flat_v, self.hp, shadow_bf16=self.flat_s,
                         ticked=ticked, zero_grad=True, clipped=clip)
        else:
            K.adamw_step_groups(self.flat_p, self.flat_g, self.flat_m, self.flat_v, self.hp, self._gid, self._gtab,
                                shadow_bf16=self.flat_s, ticked=ticked, zero_grad=True, clipped=clip)
        if self.ema_decay is not None:   # on the updated parameters; hp[HP_STEP] already counts this step
            K.ema_update(self.flat_p, self.flat_e, self.hp, self.ema_warmup)

    def state_tensors(self):
        """Every tensor a step moves here, apart from the parameters: what capture() snapshots before its warm-up steps and
        restores after them.  A new feature with state of its own registers it in this list."""
        state = [self.flat_m, self.flat_v, self.hp]
        if self.ema_decay is not None:
            state.append(self.flat_e)
        if self.lr_sched is not None:   # (sched[SCHED_LAST_LR]; hp[HP_LR] and hp[HP_STEP] return with hp)
            state.append(self._sched)
        return state

    # ---------------------------------------------------------------- learning rate
    def set_lr(self, lr: float):
        if self.lr_sched is not None:
            raise L.VitpeError("set_lr: a per-step schedule is on and writes the learning rate every step (set_lr_schedule(None) "
                               "first, or give the schedule its new base_lr)")
        self.hp[HP_LR] = lr

    def current_lr(self) -> float:
        """hp[HP_LR], the learning rate of the last step (the base rate every group scales); synchronises with the device."""
        return float(self.hp[HP_LR].item())

    def set_lr_schedule(self, base_lr: Optional[float], total_steps: int = 0, warmup_steps: int = 0, min_lr: float = 0.0,
                        warmup_factor: float = 1e-3, done: int = 0):
        """Linear warm-up + cosine learning rate, stepped every iteration inside the step ("Parameter groups and
        LR schedule"): step k = `done`, done + 1, ... of the schedule trains at
            base_lr * (warmup_factor + (1 - warmup_factor) * k / warmup_steps)                      k < warmup_steps
            min_lr + (base_lr - min_lr) * cos^2(pi / 2 * (k - warmup_steps) / (total_steps - warmup_steps))   up to total_steps
        and at min_lr from then on -- torch's SequentialLR(LinearLR, CosineAnnealingLR) stepped once per iteration.  The
        step counter is the optimizer's own, on the device, so replays of the captured step follow the schedule without a
        host write.  None as base_lr switches the schedule off (the default; hp[HP_LR] keeps its last value).  Switching on
        or off drops the captured graphs; new values for an enabled schedule (the call re-bases it: the next step is step
        `done`) are device writes and keep them.  Configuration like max_norm: not part of state_dict() -- `done=` is how a
        resumed run continues.  While it is on, set_lr() raises VitpeError."""
        new = sched_values(base_lr, total_steps, warmup_steps, min_lr, warmup_factor, done)
        if new is None:
            if self.lr_sched is not None:
                self._drop_graphs()
            self.lr_sched = self._sched = None
            return
        base, lo, W, T, s0, dn = new
        if self._sched is None:
            self._sched = torch.zeros(L.SCHED_COUNT, dtype=torch.float32, device=self.hp.device)
            self._drop_graphs()
        self._sched[SCHED_BASE_LR:SCHED_START_FACTOR + 1] = torch.tensor([base, lo, float(W), float(T), s0], dtype=torch.float32)
        # origin = step counter - done, device to device (no host read of the counter)
        self._sched[SCHED_ORIGIN:SCHED_ORIGIN + 1].copy_(self.hp[HP_STEP:HP_STEP + 1])
        if dn:
            self._sched[SCHED_ORIGIN:SCHED_ORIGIN + 1].sub_(float(dn))
        self.lr_sched = new

    # ---------------------------------------------------------------- parameter groups
    def set_param_groups(self, groups):
        """AdamW parameter groups inside the step ("Parameter groups and LR schedule"): `groups` is a list of
        {"params": [...], "lr_scale": float, "weight_decay_scale": float} (both scales default to 1, finite and >= 0); the
        parameters of a group train at lr * lr_scale with weight decay weight_decay * weight_decay_scale, parameters not
        listed at (1, 1).  vit_param_groups(model, ...) builds the usual list.  None or [] switches the groups off (the
        default: vitpe_adamw_step, one group).  Scales, not values: set_lr, set_lr_schedule and the engine's weight_decay
        keep working.  Configuration like max_norm: not part of state_dict().  Switching on or off, or another partition of
        the parameters, drops the captured graphs; the same partition with new scales is one device write and keeps them.
        A parameter listed twice or not the model's raises VitpeError.  Every rank must make the same call."""
        new = group_scales(groups)
        if new is None:
            if self.param_groups is not None:
                self._drop_graphs()
            self.param_groups = self._gid = self._gid_host = self._gtab = None
            return
        spans, table = [], [(1.0, 1.0)]
        for k, (params, lr_scale, wd_scale) in enumerate(new, start=1):
            table.append((lr_scale, wd_scale))
            for prm in params:
                if id(prm) not in self.offsets:
                    raise L.VitpeError("set_param_groups: a listed parameter is not one of the model's")
                spans.append((self.offsets[id(prm)], prm.numel(), k))
        gid = param_granule_map(spans, self.n_flat)
        gtab = torch.tensor(table, dtype=torch.float32)
        if self._gid_host is not None and self._gtab.shape == gtab.shape and np.array_equal(gid, self._gid_host):
            self._gtab.copy_(gtab)   # the captured launches read the same two buffers
        else:
            dev = self.hp.device
            self._gid_host, self._gid, self._gtab = gid, torch.from_numpy(gid).to(dev), gtab.to(dev)
            self._drop_graphs()
        self.param_groups = new

    # ---------------------------------------------------------------- gradient clipping
    def set_grad_clip(self, max_norm: Optional[float]):
        """torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm) between the backward (after every all-reduce) and
        AdamW, inside the step: the norm of the gradient AdamW uses (flat_g * grad_scale, all parameters, L2) is reduced on
        the device and the update scales the gradient by grad_scale * min(1, max_norm / (norm + 1e-6)) ("Gradient
        clipping").  None or 0 switches it off (the default).  Configuration like the learning rate: not part of
        state_dict().  Switching on or off drops the captured graphs; a new value for an enabled clip is one device
        write (hp[HP_MAX_NORM]) and keeps them.  Negative or non-finite values raise VitpeError."""
        new = clip_value(max_norm)
        if new is not None:
            if self._clip_partial is None:
                self._clip_partial = torch.zeros(K.grad_clip_blocks(self.n_flat), dtype=torch.float32, device=self.hp.device)
            self.hp[HP_MAX_NORM] = new
        if (new is None) != (self.clip_max_norm is None):
            self._drop_graphs()
        self.clip_max_norm = new

    def grad_norm(self) -> float:
        """total_norm of the last optimizer step, before clipping (what clip_grad_norm_ returns), read from
        hp[HP_TOTAL_NORM]; synchronises with the device.  Only defined while clipping is on (nothing computes the norm
        otherwise): VitpeError when it is off."""
        if self.clip_max_norm is None:
            raise L.VitpeError("grad_norm: gradient clipping is off (set_grad_clip(max_norm) first); the norm is only "
                               "computed as part of the clip")
        return float(self.hp[HP_TOTAL_NORM].item())

    # ---------------------------------------------------------------- weight EMA
    def guard(self, what):
        """VitpeError for a call that must not run while TrainEngine.ema_weights() has the average swapped in."""
        if self.ema_swapped:
            raise L.VitpeError(f"{what}: not available inside ema_weights() (the parameters are swapped with their average; "
                               f"leave the context first)")

    def needs_ema(self, what):
        if self.ema_decay is None:
            raise L.VitpeError(f"{what}: the weight EMA is off (set_ema(decay) first)")

    def set_ema(self, decay: Optional[float], warmup: bool = False):
        """Keep an exponential moving average of the parameters, updated inside the step right after AdamW (DESIGN.md,
        "Weight EMA"): flat_e += (1 - d_t) * (flat_p - flat_e), with d_t = decay, or with warmup=True
        min(decay, (1 + t) / (10 + t)) at t = optimizer steps since the average was switched on (TF's num_updates rule).
        None or 0 switches it off (the default) and frees the buffer.  Switching on allocates flat_e (4 * n_flat bytes),
        starts it as a copy of the parameters and drops the captured graphs, as do switching off and changing `warmup`; a
        new decay for an enabled average is one device write (hp[HP_EMA_DECAY]) and keeps them.  Configuration-adjacent
        state like rng_table: not part of model.state_dict() -- TrainEngine.ema_state_dict() / load_ema_state_dict() carry
        it.  Evaluate on the average inside TrainEngine.ema_weights().  Values outside [0, 1) raise VitpeError."""
        self.guard("set_ema")
        new = ema_value(decay)
        warmup = bool(warmup) and new is not None
        if new is not None:
            self.hp[HP_EMA_DECAY] = new
            if self.ema_decay is None:
                self.flat_e = torch.empty_like(self.flat_p)
                self._ema_rebase()
        else:
            self.flat_e = None
        if (new is None) != (self.ema_decay is None) or warmup != self.ema_warmup:
            self._drop_graphs()
        self.ema_decay, self.ema_warmup = new, warmup

    def _ema_rebase(self):
        """The average starts over from the parameters, its warm-up from now: the origin is the step counter, device to
        device."""
        self.flat_e.copy_(self.flat_p)
        self.hp[HP_EMA_ORIGIN:HP_EMA_ORIGIN + 1].copy_(self.hp[HP_STEP:HP_STEP + 1])

    def reset_ema(self):
        """Restart the average as a copy of the current parameters (after loading or broadcasting parameters); captured
        graphs stay valid."""
        self.guard("reset_ema")
        self.needs_ema("reset_ema")
        self._ema_rebase()
