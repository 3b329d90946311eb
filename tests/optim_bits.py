"""The bits the optimizer-side kernels leave behind: what a reorganisation of csrc/optim.hip must reproduce exactly.

The kernels between the backward and the next forward (lr_schedule, grad_clip, adamw_step / adamw_step_groups, ema_update,
ema_swap) have no atomics, so on one device and one compiler their outputs are reproducible bit for bit.  run_case() drives
three consecutive optimizer steps through vitpe.kernels alone (no engine) on seeded inputs and returns the SHA-256 of every
buffer they write; the golden (tests/golden/optim_bits.json) holds one hash per case and is only ever recorded from the
commit BEFORE such a reorganisation:

    python tests/optim_bits.py --write-golden --commit HASH
"""
import hashlib
import json
import math
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "vit-rpe-rope_amd"), os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

GOLDEN_PATH = os.path.join(REPO, "tests", "golden", "optim_bits.json")
STEPS = 3
GROUP_SCALES = ((1.0, 1.0), (0.5, 0.0), (0.25, 1.0))
N_TAIL, N_BODY = 7, 2051                      # tail lanes only; vector body + the n % 8 = 3 and n % 4 = 3 tails
N_PLAIN_CAP = 4096 * 256 + 2051               # adamw_kernel's grid-stride trip past its 4096 workgroups
N_GROUPS_CAP = 2048 * 256 * 8 + 2051          # the same for adamw_groups_kernel's 2048 workgroups of 8-element lanes
HEAD_TICK_SHAPE = ("f32", 1, 1, 64, 3, 1, 1e-6)   # the smallest of head_ref.HEAD_STEP_CASES


def _case(n, groups, clipped=True, ticked=False, shadow=True, warm=True):
    return dict(n=n, groups=groups, clipped=clipped, ticked=ticked, shadow=shadow, warm=warm)


CASES = {}
for _n in (N_TAIL, N_BODY, N_PLAIN_CAP, N_GROUPS_CAP):
    for _g in (False, True):
        CASES[f"n{_n}-{'groups' if _g else 'plain'}"] = _case(_n, _g)
for _g in (False, True):
    _k = "groups" if _g else "plain"
    CASES[f"n{N_BODY}-{_k}-unclipped"] = _case(N_BODY, _g, clipped=False)
    CASES[f"n{N_BODY}-{_k}-ticked"] = _case(N_BODY, _g, ticked=True)
    CASES[f"n{N_BODY}-{_k}-noshadow"] = _case(N_BODY, _g, shadow=False)
    CASES[f"n{N_BODY}-{_k}-nowarm"] = _case(N_BODY, _g, warm=False)
CASES[f"n{N_BODY}-clip-offset1"] = dict(clip_offset=1, n=N_BODY)
CASES["head-tick"] = dict(head_tick=HEAD_TICK_SHAPE)


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        if t is not None:
            h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h


def _hp():
    hp = torch.zeros(16)
    hp[:5] = torch.tensor([1e-3, 0.9, 0.999, 1e-8, 0.05])
    hp[8] = 0.5       # grad_scale
    hp[12] = 1.0      # max_norm: far below 0.5 * sqrt(n), so the coefficient is not 1
    hp[13] = 0.99     # EMA decay
    return hp


def _run_steps(K, c):
    n = c["n"]
    gen = torch.Generator().manual_seed(1000 + n)
    dev = "cuda"
    p, m = torch.randn(n, generator=gen).to(dev), (0.1 * torch.randn(n, generator=gen)).to(dev)
    v = (0.01 * torch.rand(n, generator=gen)).to(dev)
    e = (torch.randn(n, generator=gen)).to(dev)
    grads = [torch.randn(n, generator=gen) for _ in range(STEPS)]
    gid = torch.randint(0, len(GROUP_SCALES), ((n + 7) // 8,), generator=gen, dtype=torch.uint8).to(dev)
    gtab = torch.tensor(GROUP_SCALES, dtype=torch.float32).to(dev)
    g = torch.zeros(n, device=dev)
    hp = _hp().to(dev)
    sched = torch.tensor([1e-3, 1e-5, 1.0, 40.0, 1e-3, 0.0, 0.0, 0.0]).to(dev)   # one warm-up step, then the cosine
    shadow = torch.zeros(n, dtype=torch.bfloat16, device=dev) if c["shadow"] else None
    partial = torch.zeros(K.grad_clip_blocks(n), device=dev)
    for k in range(STEPS):
        g.copy_(grads[k])
        if c["ticked"]:   # what the head's hp_tick leaves: the counter and both bias corrections of step k + 1
            hp[5:8] = torch.tensor([k + 1.0, 1.0 - math.pow(0.9, k + 1), 1.0 - math.pow(0.999, k + 1)]).to(dev)
        K.lr_schedule(hp, sched, ticked=c["ticked"])
        if c["clipped"]:
            K.grad_clip(g, hp, partial)
        kw = dict(shadow_bf16=shadow, zero_grad=k + 1 < STEPS, ticked=c["ticked"], clipped=c["clipped"])
        if c["groups"]:
            K.adamw_step_groups(p, g, m, v, hp, gid, gtab, **kw)
        else:
            K.adamw_step(p, g, m, v, hp, **kw)
        K.ema_update(p, e, hp, c["warm"])
    K.ema_swap(p, e, shadow)
    h = _sha(p, e, shadow)
    K.ema_swap(p, e, shadow)
    torch.cuda.synchronize()
    h.update(_sha(p, m, v, hp, sched, e, shadow, g).digest())
    return h.hexdigest()


def _run_clip_offset(K, c):
    """grad_clip on a view at element offset 1 of an aligned buffer: the unaligned head of grad_sqnorm_kernel."""
    n = c["n"]
    gen = torch.Generator().manual_seed(2000 + n)
    g = torch.randn(n + c["clip_offset"], generator=gen).cuda()[c["clip_offset"]:]
    assert g.data_ptr() % 16 == 4 * c["clip_offset"]
    hp = _hp().cuda()
    partial = torch.zeros(K.grad_clip_blocks(n), device="cuda")
    K.grad_clip(g, hp, partial)
    torch.cuda.synchronize()
    return _sha(hp, partial, g).hexdigest()


def _run_head_tick(K, c):
    """head_step(..., hp_tick=hp) three times: hp[5:8] after each."""
    import head_ref as H
    dt, B, N, D, Cn, nv, eps = c["head_tick"]
    x, gamma, beta, wh, bh, labels = H.head_inputs(dt, B, N, D, Cn, eps)
    gs, ls, _ = H.scales(B, nv)
    z = lambda *s: torch.zeros(*s, device="cuda")   # noqa: E731
    ctl = torch.tensor([gs, ls, float(nv), 0.0], device="cuda")
    dev = [t.cuda() for t in (gamma, beta, wh, bh, labels)]
    xd = x.cuda().to(H.DT[dt])
    hp = _hp().cuda()
    ticks = []
    for _ in range(STEPS):
        K.head_step(xd, dev[0], dev[1], dev[2], dev[3], dev[4], z(B, Cn), z(B, Cn), (z(B, D), z(B, D)), z(B, D),
                    torch.zeros(B, N, D, device="cuda", dtype=H.DT[dt]), z(2), z(2), z(2 * B), ctl, z(Cn, D), z(Cn), z(D), z(D),
                    eps=eps, hp_tick=hp)
        ticks.append(hp[5:8].clone())
    torch.cuda.synchronize()
    return _sha(*ticks).hexdigest()


def run_case(name):
    from vitpe import kernels as K
    c = CASES[name]
    if "head_tick" in c:
        return _run_head_tick(K, c)
    if "clip_offset" in c:
        return _run_clip_offset(K, c)
    return _run_steps(K, c)


def main(argv):
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--write-golden", action="store_true", help="write " + os.path.relpath(GOLDEN_PATH, REPO))
    ap.add_argument("--commit", default="", help="hash of the commit the golden is recorded from (stored in it)")
    args = ap.parse_args(argv)
    golden = {"recorded_from": args.commit, "cases": {}}
    for name in CASES:
        golden["cases"][name] = run_case(name)
        print(name, golden["cases"][name], flush=True)
    if args.write_golden:
        with open(GOLDEN_PATH, "w") as f:
            json.dump(golden, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
