"""The head side of the train step: the final LayerNorm of the class row, the classifier, the cross-entropy, the metrics
and their backward ("Head side of the step"; kernels: csrc/head.hip).

StepHead owns the buffers (logits, dlogits, out2, the metric accumulator, the control block, the head's work buffers), the
order of its launches and the one function that knows the control block's layout; TrainEngine forwards set_valid, eval_loss
and read_metrics here and calls forward / loss / backward where the head sits in its step.  Constructing a StepHead and
set_valid need no device beyond the one the tensors handed in live on; forward(), loss(), backward() and eval_loss() run
kernels, read_metrics() synchronises.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.distributed as dist

from . import _lib as L
from . import kernels as K


class StepHead:
    """norm / head: the model's final LayerNorm and classifier (their .data are read at every call: they are views of the
    engine's flat parameters); grads: the gradient views (d head.weight, d head.bias, d norm.weight, d norm.bias);
    x_top [B, N, D]: the last block's output; dx_top [B, N, D]: its gradient, zeroed here; labels [B] int64; hp: the
    optimizer's block (the fused launch advances its step counter); dtype: the compute dtype; n_tokens: N; fuse_head: the
    route's flag (one launch pair for the whole head) -- else head_fwd, cross_entropy_ctl and head_bwd."""

    def __init__(self, norm, head, grads, x_top, dx_top, labels, hp, dtype, n_tokens, fuse_head, world=1,
                 process_group=None):
        self.norm, self.head, self.grads = norm, head, tuple(grads)
        self.x, self.dx, self.labels, self.hp = x_top, dx_top, labels, hp
        self.T, self.N, self.fuse_head, self.world, self.pg = dtype, n_tokens, bool(fuse_head), world, process_group
        B, D, Cn, dev = x_top.shape[0], x_top.shape[2], head.weight.shape[0], x_top.device
        self.B, self.dev = B, dev
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)  # noqa: E731
        self.logits, self.dlogits = f(B, Cn), f(B, Cn)
        self.out2 = f(2)
        self.metric_acc = torch.zeros(2, dtype=torch.float32, device=dev)  # [sum of batch-mean losses, #correct]
        # the cross-entropy scalars live on the device so a captured step follows a ragged last batch (train.py:89-90)
        self.ctl = torch.zeros(4, dtype=torch.float32, device=dev)
        self.valid = None                                    # the (n_valid, n_valid_global) ctl was last written for
        self.set_valid(B)
        self._eval_ctl = self._eval_ctl_key = None           # eval_loss's block, per distinct batch shape
        self.per_image = torch.zeros(2 * B, dtype=torch.float32, device=dev)   # (loss, correct) per image
        self.ws = (f(B, D), f(B, D), f(B))                   # (xhat, yn, rstd) of the class rows, kept for the backward
        self.ws_dyn = f(B, D)
        self.ticked = False                                  # loss(tick=True) on the fused head advanced the step counter
        # Only the class rows of dx_top are ever written: head_step_kernel stores row b * N alone, and every later reader
        # (the top block's backward) takes rows 1.. as the zeros the model's class-token pooling makes them.  They are
        # zeroed HERE, once, next to the only launch that relies on it (head_bwd, the unfused route, rewrites them anyway).
        self.dx.zero_()

    def _params(self):
        return self.norm.weight.data, self.norm.bias.data, self.head.weight.data, self.head.bias.data

    # ---------------------------------------------------------------- the control block
    def _write_ctl(self, grad_scale: float, n_global: int, n: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The block ce_kernel and head_step_kernel read (csrc/head.hip): float32 {grad_scale, loss_scale = 1 / n_global,
        n_valid = n, 0}.  Written into `out` in place (captured launches read its memory), or into a new device tensor."""
        host = torch.tensor([grad_scale, 1.0 / n_global, float(n), 0.0], dtype=torch.float32)
        if out is None:
            return host.to(self.dev)
        out.copy_(host, non_blocking=False)
        return out

    def set_valid(self, n_valid: int, n_valid_global: Optional[int] = None):
        """The next steps' batches hold `n_valid` real samples in rows [0, n_valid) (the rest is padding) and the
        GLOBAL batch (all ranks) holds `n_valid_global`.  Loss = mean over the global batch (train.py:113,194),
        gradients = its gradient: dlogits are scaled by world / n_valid_global here and by 1 / world inside AdamW."""
        if n_valid_global is None:
            n_valid_global = n_valid * self.world
        if not (0 <= n_valid <= self.B and n_valid_global >= max(n_valid, 1)):
            raise L.VitpeError(f"set_valid({n_valid}, {n_valid_global}) with engine batch {self.B}")
        if self.valid != (n_valid, n_valid_global):
            self.valid = (n_valid, n_valid_global)
            self._write_ctl(self.world / n_valid_global, n_valid_global, n_valid, out=self.ctl)

    # ---------------------------------------------------------------- the step
    def forward(self):
        """Logits of x_top (evaluation, and the unfused train step, which keeps the work buffers for backward())."""
        K.head_fwd(self.x, *self._params(), self.norm.eps, save=True, logits=self.logits, ws=self.ws)

    def loss(self, tick=True):
        """tick: this loss belongs to a full step -- the fused head launch also advances the optimizer's step counter."""
        self.ticked = bool(tick and self.fuse_head)
        if self.fuse_head:   # final LayerNorm + head + CE + accuracy + dlogits + the head's backward: one launch pair
            K.head_step(self.x, *self._params(), self.labels, self.logits, self.dlogits, self.ws, self.ws_dyn, self.dx,
                        self.out2, self.metric_acc, self.per_image, self.ctl, *self.grads, eps=self.norm.eps,
                        hp_tick=(self.hp if tick else None))
            return
        K.cross_entropy_ctl(self.logits, self.labels, self.ctl, dlogits=self.dlogits, out2=self.out2,
                            metric_acc=self.metric_acc)

    def backward(self):
        """dlogits -> dx_top (every row) and the parameter gradients: the unfused route only (loss() did it when fused)."""
        K.head_bwd(self.dlogits, self.head.weight.data, self.norm.weight.data, self.ws, self.T, self.N, *self.grads,
                   dx=self.dx, ws_dyn=self.ws_dyn)

    def state_tensors(self):
        """What a step moves here and the next step reads: capture() snapshots it before its warm-up steps and restores
        it after them."""
        return [self.metric_acc]

    # ---------------------------------------------------------------- evaluation and metrics
    def eval_loss(self, n: int, acc: torch.Tensor, n_global: Optional[int] = None):
        """acc[0] += (sum of the cross-entropy of rows [0, n) of the current logits vs labels) / n_global (this rank's part
        of the batch mean, reference train.py:146-149; n_global defaults to n), acc[1] += #correct.  Device-side; leaves
        the training scalars untouched."""
        key = (n, n_global or n)
        if self._eval_ctl_key != key:   # (one host -> device copy per distinct batch shape, not per batch)
            self._eval_ctl = self._write_ctl(0.0, max(n_global or n, 1), n)
            self._eval_ctl_key = key
        K.cross_entropy_ctl(self.logits, self.labels, self._eval_ctl, dlogits=None, out2=self.out2, metric_acc=acc)

    def read_metrics(self, reset=True):
        """(sum over the steps since the last read of the global-batch mean loss, #correct over all ranks) -- the
        ONLY host sync (and, data parallel, one 2-float all-reduce per read: every rank must call it)."""
        t = self.metric_acc
        if self.world > 1:
            t = self.metric_acc.clone()
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.pg)
        v = t.tolist()
        if reset:
            self.metric_acc.zero_()
        return v[0], v[1]
