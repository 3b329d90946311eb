"""Plain numpy / float64 restatements of AdamW with parameter groups (adamw_groups_kernel, csrc/optim.hip) and of the
per-step learning-rate schedule (lr_schedule_kernel), with the granule-map builders the tests share.  The grouped update
is train_state_ref.adamw_ref called once per group with that group's hp[0] and hp[4] scaled in fp32, as the device forms
them, so train_state_ref.adamw_bounds holds for it unchanged (the two extra fp32 products are on both sides).  Shared by
tests/test_optim_groups_cpu.py and tests/test_optim_groups_gpu.py.  No GPU and no vitpe import here."""
import math

import numpy as np

import train_state_ref as TS

U = TS.U
GRANULE = 8                              # elements per entry of the map (route.ALIGN)
THREADS, GRID_CAP = 256, 2048            # the launch of vitpe_adamw_step_groups: one lane per granule
SWEEP = GRID_CAP * THREADS * GRANULE     # elements of one full pass of the capped grid
SIZES = (0, 1, 7, 8, 9, 2048 + 5, SWEEP + 4099)

# the kernel tests' four groups (lr scale, weight-decay scale) and the lengths, in granules, of the spans that repeat over
# the buffer in that order: 41 granules a period, so every 64-lane wavefront holds all four groups
GROUPS4 = ((1.0, 1.0), (1.0, 0.0), (0.5, 1.0), (0.0, 0.0))
SPANS4 = (1, 2, 33, 5)


def blocks(n):
    """vitpe_adamw_groups_blocks: min(2048, max(1, ceil(ceil(n / 8) / 256))); 0 for n <= 0."""
    if n <= 0:
        return 0
    gran = -(-n // GRANULE)
    return min(GRID_CAP, max(1, -(-gran // THREADS)))


def n_granules(n):
    return -(-n // GRANULE)


def span_map(n, spans=SPANS4):
    """uint8 [ceil(n / 8)]: group j for spans[j] granules, in order, repeating."""
    period = np.repeat(np.arange(len(spans), dtype=np.uint8), spans)
    reps = -(-max(n_granules(n), 1) // period.size)
    return np.tile(period, reps)[:n_granules(n)].copy()


def layout_map(numels, group_of, align=GRANULE):
    """The map of a flat layout: parameter j of numels[j] elements starts at a multiple of `align` and belongs to group
    group_of[j] (the padding inside its last granule with it); a granule no parameter covers belongs to group 0.
    -> (offsets, n_flat, gid uint8 [n_flat / align])."""
    offs, n = [], 0
    for k in numels:
        offs.append(n)
        n += -(-k // align) * align
    gid = np.zeros(n // align, dtype=np.uint8)
    for o, k, grp in zip(offs, numels, group_of):
        gid[o // align:(o + k + align - 1) // align] = grp
    return offs, n, gid


def element_groups(gid, n):
    """group of every one of the n elements"""
    return np.repeat(np.asarray(gid), GRANULE)[:n]


def group_hp(hp, lr_scale, wd_scale):
    """hp with [0] and [4] multiplied by the group's scales in fp32, as the kernel does"""
    out = np.asarray(hp, dtype=np.float32).copy()
    out[0] = np.float32(out[0]) * np.float32(lr_scale)
    out[4] = np.float32(out[4]) * np.float32(wd_scale)
    return out


def grouped_adamw_ref(p, g, m, v, hp, bc1, bc2, gid, table):
    """One AdamW step in float64 with parameter groups -> (p, m, v, delta) as train_state_ref.adamw_ref returns them."""
    n = np.asarray(p).shape[0]
    eg = element_groups(gid, n)
    outs = [np.zeros(n, dtype=np.float64) for _ in range(4)]
    for k, (ls, ws) in enumerate(table):
        idx = np.nonzero(eg == k)[0]
        if idx.size == 0:
            continue
        res = TS.adamw_ref(np.asarray(p)[idx], np.asarray(g)[idx], np.asarray(m)[idx], np.asarray(v)[idx],
                           group_hp(hp, ls, ws), bc1, bc2)
        for o, r in zip(outs, res):
            o[idx] = r
    return tuple(outs)


def bias_corrections(hp, step):
    """(bc1, bc2) at step `step` in float64 from the fp32 betas (the device forms them in fp32 with powf; the tests take
    the device's own values for the reference and compare them with these to a few ulp)."""
    b1, b2 = float(np.float32(hp[1])), float(np.float32(hp[2]))
    return 1.0 - b1 ** step, 1.0 - b2 ** step


# ------------------------------------------------------------------------------------------ the schedule
# (base_lr, min_lr, warm-up steps W, total steps T, start factor s0)
SCHED_CASES = ((1e-3, 0.0, 5, 40, 0.01), (3e-4, 1e-5, 0, 17, 1.0), (1e-3, 1e-6, 3, 1000, 0.1))


def sched_ks(W, T):
    """the step indices the device test visits (negative ones dropped)"""
    ks = [0, 1, W - 1, W, W + 1, (W + T) // 2, T - 1, T, T + 5]
    return sorted({k for k in ks if k >= 0})


def schedule_ref(k, base, lo, W, T, s0):
    """Learning rate of step k in float64: linear from s0 * base to base over W steps, then
    lo + (base - lo) cos^2(pi / 2 * (k - W) / (T - W)), and lo from step T on."""
    base, lo, s0, k = float(base), float(lo), float(s0), max(float(k), 0.0)
    if k < W:
        return base * (s0 + (1.0 - s0) * k / W)
    if k >= T:
        return lo
    c = math.cos(0.5 * math.pi * ((k - W) / (T - W)))
    return lo + (base - lo) * c * c


def sched_block(base, lo, W, T, s0, origin, last=-3.0, spare=-9.0):
    """the 8-float device block of vitpe_lr_schedule"""
    return np.array([base, lo, W, T, s0, origin, last, spare], dtype=np.float32)
