"""Plain numpy / float64 restatement of the weight EMA the train step keeps (vitpe_ema_update in csrc/optim.hip,
include/vitpe.h):  e' = e + w (p - e),  w = 1 - d_t,  d_t = decay or min(decay, (1 + t) / (10 + t)).  Shared by
tests/test_ema_cpu.py (the reference is self-consistent) and tests/test_ema_gpu.py (the kernels and the engine against
it).  No GPU and no vitpe import here."""
import numpy as np

U = 2.0 ** -24   # unit roundoff of fp32

SIZES = (0, 1, 3, 4, 5, 1023, 1024, 4099)
GRID_CAP = 256 * 8                      # workgroups: 256 CUs x 8 (the kernel tests check it against the library as built)
SWEEP = GRID_CAP * 256 * 4              # elements one full sweep of the capped grid covers (256 lanes x 4 elements each)


def lerp_weight(d):
    """w = 1 - d formed in fp32, as the device forms it; returned as a Python float (exactly that fp32 value)."""
    return float(np.float32(1.0) - np.float32(d))


def ema_ref(p, e, d):
    """The float64 recurrence on the fp32 inputs: e + w (p - e) with w = float32(1) - float32(d)."""
    p, e = np.asarray(p, dtype=np.float64), np.asarray(e, dtype=np.float64)
    return e + lerp_weight(d) * (p - e)


def ema_bound(p, e, e_new, d):
    """Per-element bound of the device's e' against ema_ref: the device rounds p - e once (relative U, carried through the
    product with w) and the fma once (relative U of the result): U (w |p - e| + |e'|).  Both roundings are to nearest,
    |delta| <= U / (1 + U), so the second-order term is inside it.  Inputs of magnitude 2^-10 .. 2^4 keep every
    intermediate normal: no floor."""
    p, e = np.asarray(p, dtype=np.float64), np.asarray(e, dtype=np.float64)
    return U * (lerp_weight(d) * np.abs(p - e) + np.abs(np.asarray(e_new, dtype=np.float64)))


def warmup_decay(decay, t):
    """d_t of the warm-up rule in numpy fp32, operation by operation as the kernel: min(decay, (1 + t) / (10 + t)), t the
    number of optimizer steps since the average was switched on (TF's num_updates)."""
    t = np.float32(t)
    ramp = (np.float32(1.0) + t) / (np.float32(10.0) + t)
    return np.float32(min(np.float32(decay), np.float32(ramp)))


def ema_inputs(n, seed=0):
    """(p, e): fp32 [n] each, magnitudes log-uniform over [2^-10, 2^4], both signs, independent."""
    rng = np.random.default_rng(seed)

    def draw():
        mag = 2.0 ** rng.uniform(-10.0, 4.0, size=n)
        return (mag * rng.choice([-1.0, 1.0], size=n)).astype(np.float32)
    return draw(), draw()


def mark_indices(n):
    """Indices that get one of the three marked relations, dealt round-robin: the first and last elements, both sides of
    the boundary between the 16-byte body and the scalar tail, and the first index past a sweep of the capped grid."""
    idx = {0, 1, 2, 3, 4, 5, 4 * (n // 4) - 1, 4 * (n // 4), n - 3, n - 2, n - 1, SWEEP - 1, SWEEP, SWEEP + 1}
    return sorted(i for i in idx if 0 <= i < n)


def with_marks(p, e):
    """Copies of (p, e) with, at mark_indices in turn: p == e (the fixed point: e's bits must stay), e == 0, p == 0.
    -> (p, e, {"equal": [...], "e_zero": [...], "p_zero": [...]})"""
    p, e = np.array(p, dtype=np.float32), np.array(e, dtype=np.float32)
    kinds = {"equal": [], "e_zero": [], "p_zero": []}
    for j, i in enumerate(mark_indices(p.shape[0])):
        kind = ("equal", "e_zero", "p_zero")[j % 3]
        kinds[kind].append(i)
        if kind == "equal":
            p[i] = e[i]
        elif kind == "e_zero":
            e[i] = 0.0
        else:
            p[i] = 0.0
    return p, e, kinds
