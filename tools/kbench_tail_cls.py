#!/usr/bin/env python3
"""The class-row tail kernels stand-alone: vitpe_tail_cls_fwd (training form) / vitpe_tail_cls_bwd at B = 512, N = 65,
D = 192, HID = 768, bf16, in place on full-layout [B x N, .] buffers (row step N), timed with HIP events three ways:

  hot       one operand set, launches back to back: weights and rows are served from L2 (what a probe loop sees)
  rotating  a ring of --ring operand sets (own weights, own activations), back to back: every launch finds its 0.66 MB of
            weight fragments and its rows outside the L2 (they still sit in the memory-side cache)
  flushed   one launch between two events, with a --flush_mb fill in front of it (outside the events): everything comes
            from memory, as after the rest of a training step; this is the figure to hold against the kernel trace of
            the step (profiles/*_step_kernel_stats.csv; the pair of events adds about 2 us) -- the probe-vs-trace gap is
            hot against flushed

medians of --reps repeats (min, max alongside).  --parent_lib PATH times the same entry points of ANOTHER build of
libvitpe.so (the parent commit's) in the same process on the same operands, the two builds alternating inside every repeat.
Prints one JSON line per kernel."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "vit-rpe-rope_amd"))
from vitpe import _lib as L  # noqa: E402
from vitpe import kernels as K  # noqa: E402

D = 192
bf = torch.bfloat16


def operand_set(B, N, HID, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    M = B * N

    def r(*shape, scale=1.0, dtype=bf):
        return ((torch.rand(*shape, generator=g, device="cuda") * 2 - 1) * scale).to(dtype).contiguous()

    f32 = torch.float32
    s = dict(a=r(M, D), x_in=r(M, D), bp=r(D, scale=0.1, dtype=f32), gamma=1 + r(D, scale=0.1, dtype=f32),
             beta=r(D, scale=0.1, dtype=f32), b1=r(HID, scale=0.1, dtype=f32), b2=r(D, scale=0.1, dtype=f32),
             dy=r(M, D), dgamma=torch.zeros(D, device="cuda"), dbeta=torch.zeros(D, device="cuda"))
    wp, w1, w2 = r(D, D, scale=0.07, dtype=f32), r(HID, D, scale=0.08, dtype=f32), r(D, HID, scale=0.05, dtype=f32)
    s.update(wp=K.pack_weight_frags(wp, bf, 192, 0), w1=K.pack_weight_frags(w1, bf, 192, 1), w2=K.pack_weight_frags(w2, bf, 32, 1),
             w2t=K.pack_weight_frags(w2.t().contiguous(), bf, 192, 1), w1t=K.pack_weight_frags(w1.t().contiguous(), bf, 32, 1),
             wpt=K.pack_weight_frags(wp.t().contiguous(), bf, 192, 1))
    for k, c, dt in (("x_mid", D, bf), ("xn", D, bf), ("out", D, bf), ("h", HID, bf), ("gp", HID, torch.float16),
                     ("du", HID, bf), ("dx", D, bf), ("da", D, bf)):
        s[k] = torch.zeros(M, c, dtype=dt, device="cuda")
    s["m2"], s["r2"] = torch.zeros(M, device="cuda"), torch.zeros(M, device="cuda")
    return s


def make_calls(handle, B, N, HID):
    """(fwd(s), bwd(s)) on the C ABI of one build"""
    p = L.ptr

    def fwd(s):
        L.check(handle.vitpe_tail_cls_fwd(L.BF16, p(s["a"]), p(s["x_in"]), p(s["wp"]), p(s["bp"]), p(s["gamma"]), p(s["beta"]),
                                          p(s["x_mid"]), p(s["m2"]), p(s["r2"]), p(s["xn"]), p(s["w1"]), p(s["b1"]), p(s["w2"]),
                                          p(s["b2"]), p(s["gp"]), p(s["h"]), p(s["out"]), 1e-5, B, N, D, HID, L.stream_ptr()),
                "vitpe_tail_cls_fwd")

    def bwd(s):
        L.check(handle.vitpe_tail_cls_bwd(L.BF16, p(s["dy"]), p(s["gp"]), p(s["w2t"]), p(s["w1t"]), p(s["x_mid"]), p(s["m2"]),
                                          p(s["r2"]), p(s["gamma"]), p(s["du"]), p(s["dx"]), p(s["dgamma"]), p(s["dbeta"]),
                                          p(s["wpt"]), p(s["da"]), B, N, D, HID, L.stream_ptr()), "vitpe_tail_cls_bwd")
    return fwd, bwd


def timed_loop(fn, sets, iters):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(sets[i % len(sets)])
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def timed_flushed(fn, sets, iters, flush):
    ts = []
    for i in range(iters):
        flush.add_(1)                                   # a fill of --flush_mb through the caches
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(sets[i % len(sets)])
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--tokens", type=int, default=65)
    ap.add_argument("--hidden", type=int, default=768)
    ap.add_argument("--ring", type=int, default=4)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--flush_mb", type=int, default=1024)
    ap.add_argument("--parent_lib", default=None, help="libvitpe.so of the parent commit: timed on the same operands")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    B, N, HID = a.batch, a.tokens, a.hidden
    sets = [operand_set(B, N, HID, 100 + i) for i in range(a.ring)]
    builds = {"this": make_calls(L.lib(), B, N, HID)}
    if a.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(a.parent_lib))
        for name in ("vitpe_tail_cls_fwd", "vitpe_tail_cls_bwd"):
            getattr(parent, name).argtypes = L.parse_header()[name]
            getattr(parent, name).restype = ctypes.c_int
        builds["parent"] = make_calls(parent, B, N, HID)
    flush = torch.zeros(a.flush_mb * (1 << 20) // 4, device="cuda")
    for fwd, bwd in builds.values():                    # warm-up; the forward leaves x_mid, m2, r2 and gp for the backward
        for s in sets:
            fwd(s), bwd(s)
    for ki, kernel in enumerate(("tail_cls_fwd", "tail_cls_bwd")):
        res = {(b, m): [] for b in builds for m in ("hot", "rotating", "flushed")}
        for _ in range(a.reps):
            for b, calls in builds.items():
                res[b, "hot"].append(timed_loop(calls[ki], sets[:1], a.iters))
                res[b, "rotating"].append(timed_loop(calls[ki], sets, a.iters))
                res[b, "flushed"].append(timed_flushed(calls[ki], sets, max(a.iters // 10, 5), flush))
        row = dict(kernel=kernel, B=B, N=N, HID=HID, ring=a.ring, flush_mb=a.flush_mb, workgroups=(B + 15) // 16)
        for (b, m), v in res.items():
            row[f"{b}_{m}_us"] = round(statistics.median(v), 2)
            row[f"{b}_{m}_min_max_us"] = [round(min(v), 2), round(max(v), 2)]
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
