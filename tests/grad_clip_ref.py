"""Plain numpy / float64 restatement of gradient clipping by global norm as the train step does it (vitpe_grad_clip in
csrc/optim.hip, include/vitpe.h): torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2.0) on the gradient AdamW
uses, g * gs (gs = hp[8]).  Shared by tests/test_grad_clip_cpu.py (the reference agrees with torch, the inputs
discriminate) and tests/test_grad_clip_gpu.py (the kernels against it).  No GPU and no vitpe import here."""
import numpy as np

U = 2.0 ** -24   # unit roundoff of fp32

VARIANTS = ("unscaled_norm", "no_eps", "no_clamp", "squared_norm")


def clip_ref(g, gs, max_norm, variant=None):
    """(total_norm, coef) in float64: total_norm = gs * sqrt(sum g^2), coef = min(1, max_norm / (total_norm + 1e-6)).
    g: the fp32 device values as they are (widened), gs / max_norm: widened from fp32 by the caller where they live in hp.

    variant: one of the WRONG coefficients the input set (norm_inputs / mark_groups) must tell from the right one
    ("unscaled_norm": norm of g without gs, "no_eps": no 1e-6, "no_clamp": no min(1, .), "squared_norm": clip by the
    squared norm); None = the right one.  The norm returned is the variant's own."""
    assert variant is None or variant in VARIANTS
    g = np.asarray(g, dtype=np.float64).reshape(-1)
    gs, max_norm = float(gs), float(max_norm)
    sq = float(np.sum(g * g))
    norm = np.sqrt(sq) if variant == "unscaled_norm" else gs * np.sqrt(sq)
    if variant == "squared_norm":
        norm = norm * norm
    coef = max_norm / (norm if variant == "no_eps" else norm + 1e-6)
    if variant != "no_clamp":
        coef = min(1.0, coef)
    return float(norm), float(coef)


def coef_from_norm(norm_f32, max_norm_f32):
    """The coefficient the device forms from ITS OWN fp32 norm (hp[10]) and hp[12]: float64 arithmetic on the two fp32
    values, rounded to fp32 once."""
    c = float(np.float32(max_norm_f32)) / (float(np.float32(norm_f32)) + 1e-6)
    return np.float32(min(1.0, c))


def chain_length(n, misaligned):
    """Longest chain of fp32 roundings behind one summand of grad_sqnorm_kernel's sum of squares, for n elements:
    the grid is nb = min(1024, ceil(n / 4096)) workgroups of 256 threads, the aligned body of nvec float4 is dealt out
    vector i -> thread i % (256 nb), so a thread's per-component running sum sees ceil(nvec / (256 nb)) fma's (one
    rounding each, the square included); + 1 for a head / tail element added to such a sum; + 2 for the four components,
    + 6 for the wave's butterfly, + 2 for the four waves.  The sum over workgroups is fp64 (nothing at this scale).
    misaligned: the base pointer is `misaligned` floats past a 16-byte boundary (0..3)."""
    head = min(n, (4 - misaligned) & 3)
    nvec = (n - head) // 4
    nb = min(1024, -(-n // 4096))
    per_thread = -(-nvec // (256 * nb)) if nvec else 0
    return per_thread + 1 + 2 + 6 + 2


def norm_bound(n, misaligned):
    """Relative error bound of hp[10] against clip_ref: every summand is >= 0, so the sum of squares is off by at most
    chain * U relative (first order; the (1 + U)^chain - 1 excess at chain <= 16 is below 1e-6 of it); the square root
    halves that; + U for the fp64 -> fp32 rounding of gs * sqrt(.) (its fp64 roundings are 2^-29 of that)."""
    return 0.5 * chain_length(n, misaligned) * U * (1 + 1e-6) + U * (1 + 2.0 ** -28)


def norm_inputs(n, seed=0):
    """The bulk: fp32 [n], magnitudes log-spaced over 2e-6 .. 2e-5 in a seeded random order, both signs; the sum of squares
    of 2^20 of them is 9e-5, under 3 % of eight marked elements'.  The scale is chosen for the formula, at gs = 0.25:
    every norm of the set lies between 5e-7 (one bulk element) and 1.5e-2 (eight marked ones on 2^20) -- above 3.4e-7, so
    that max_norm = 4 x norm needs the clamp at 1, and below 2e-2, so that the 1e-6 moves the coefficient by more than
    100 x the kernel test's tolerance (tests/test_grad_clip_cpu.py checks both on every input)."""
    rng = np.random.default_rng(seed)
    expo = np.linspace(np.log10(2e-6), np.log10(2e-5), n)[rng.permutation(n)]
    return ((10.0 ** expo) * rng.choice([-1.0, 1.0], size=n)).astype(np.float32)


MARK = 2e-2       # |value| of a marked element
GROUP = 8         # marked elements per run: each carries 1 / (8 + bulk / MARK^2) >= 12.1 % of the sum of squares
SIZES = (1, 3, 255, 256, 257, 4095, 4099, 2 ** 20 + 3)
GS = 0.25         # hp[8] of the kernel tests
FACTORS = (0.5, 4.0)   # max_norm / total_norm of the kernel tests: clipping to a half, and no clipping


def mark_groups(n):
    """Where a dropped head, tail, vector or slice would lose an element: the last index; the first index past a
    4-element boundary wherever the kernel's path changes there -- 4 and the last multiple of 4, and 1, 2, 3, n-2, n-3,
    n-4 (the kernel's own float4 boundaries sit 0..3 elements past the tensor's, by the alignment of the base pointer, so
    these are the first index past its head and the first of its tail at every alignment) -- and the first index past
    EVERY 4096-element boundary (4096 k; index 0 is the k = 0 one).  One vector cannot give each of hundreds of elements
    10 % of the sum, so they are dealt into runs of at most GROUP marked elements of magnitude MARK on the same bulk;
    the first run ([]) is the bulk alone."""
    marks = {0, 1, 2, 3, 4, 4 * ((n - 1) // 4), n - 1, n - 2, n - 3, n - 4} | set(range(0, n, 4096))
    marks = sorted(i for i in marks if 0 <= i < n)
    return [[]] + [marks[i:i + GROUP] for i in range(0, len(marks), GROUP)]


def with_marks(g, marks):
    """g with g[marks[j]] = +-MARK (signs alternate)."""
    out = np.array(g, dtype=np.float32)
    for j, i in enumerate(marks):
        out[i] = np.float32(MARK if j % 2 == 0 else -MARK)
    return out
