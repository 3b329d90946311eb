"""The launch trace of a TrainEngine: every C-ABI call a sequence makes, in order, with its scalar arguments and its
buffer aliasing -- what a refactor of vitpe/engine.py must leave exactly as it was.

`recording()` swaps vitpe._lib._lib for a proxy over the loaded library handle.  For each vitpe_* call it notes
  * the name (without the vitpe_ prefix);
  * every non-pointer argument verbatim (floats as repr);
  * every pointer argument as None or the index of that address in order of first appearance within the recording;
  * for vitpe_wgrad_group / vitpe_wgrad_group_rows the decoded host arrays (kernels._WgradProblem records, int steps)
    in place of their host addresses.
The trailing stream argument is dropped.  Nothing in the product code knows about the recorder.

CONFIGS are the engine configurations of tests/test_engine_trace_gpu.py and tests/test_engine_route_cpu.py; the golden
(tests/golden/engine_trace.json) holds per configuration the route flags and per sequence the call names (one string,
space-separated) and the SHA-256 of the canonical full trace.  The sequences (SEQUENCES) run in order on one engine: `step`,
`eval`, `parts` always; `probes`, `ema`, `evalloss` (the head's evaluation path: eval_loss and read_metrics) and `evalother`
(an evaluation forward on a dataset that is not the attached one, then on the attached one) where the configuration asks
for them.  Run as a script on the GPU:

    python tests/engine_trace.py --dump DIR            full traces, one JSON file per configuration and sequence
    python tests/engine_trace.py --write-golden FILE   the golden (only ever from the commit BEFORE an engine refactor)
    python tests/engine_trace.py --write-golden FILE --only NAME [NAME ...] --commit HASH
                                                       record the named configurations alone and merge them into FILE: its
                                                       other entries and its "recorded_from" stay as they are, each new
                                                       entry carries its own "recorded_from"
"""
import contextlib
import ctypes
import hashlib
import json
import os
import re
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "vit-rpe-rope_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

GOLDEN_PATH = os.path.join(REPO, "tests", "golden", "engine_trace.json")

ROUTE_SWITCHES = ("VITPE_FUSE_LN", "VITPE_FUSE_EMBED", "VITPE_ATTN_WIDE", "VITPE_ATTN_FUSED64", "VITPE_TAIL2", "VITPE_LNBWD2",
                  "VITPE_FUSE_LNBWD", "VITPE_GROUP_WGRAD", "VITPE_RECOMPUTE_LN", "VITPE_FUSE_HEAD", "VITPE_CLS_ROWS")
ROUTE_FLAGS = ("attn_fused", "attn_wide", "attn_fused64", "fuse_ln", "fuse_ln_bwd", "tail2", "lnbwd2", "fuse_lnbwd",
               "fuse_embed", "fuse_head", "group_wgrad", "recompute_ln", "cls_rows", "extras")

GEOMS = {"CIFAR": dict(img_size=32, patch_size=4, embed_dim=192, num_heads=6),     # as tests/test_train_state_gpu.py
         "HD64": dict(img_size=224, patch_size=16, embed_dim=128, num_heads=2)}
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}
BATCH = 2


def _cfg(geom="CIFAR", env=None, dtype="bf16", fuse_ln=None, extras=False, model=None, pe="rope-axial", depth=3,
         dataset=False, probes=False, evalloss=False, evalother=False, optim=None):
    """dataset: True attaches a resident dataset and switches augmentation and clipping on; "plain" attaches it alone.
    evalloss: also trace the head's evaluation path (the `evalloss` sequence).
    evalother (dataset configurations): also trace forward_indexed on a second dataset (the `evalother` sequence).
    optim: the optimizer-side options, {"clip": max_norm, "ema": (decay, warmup), "groups": vit_param_groups' keywords,
    "sched": set_lr_schedule's arguments}, each applied through the engine's public method when present."""
    return dict(geom=geom, env=env or {}, dtype=dtype, fuse_ln=fuse_ln, extras=extras, model=model or {}, pe=pe, depth=depth,
                dataset=dataset, probes=probes, evalloss=evalloss, evalother=evalother, optim=optim or {})


CONFIGS = {"cifar-bf16": _cfg(probes=True, evalloss=True)}
CONFIGS["VITPE_RECOMPUTE_LN=1"] = _cfg(env={"VITPE_RECOMPUTE_LN": "1"})
for _s in ROUTE_SWITCHES:
    if _s not in ("VITPE_FUSE_LN", "VITPE_RECOMPUTE_LN"):
        CONFIGS[_s + "=0"] = _cfg(env={_s: "0"}, evalloss=(_s == "VITPE_FUSE_HEAD"))   # (the unfused head: head_bwd)
CONFIGS.update({
    "fuse_ln=fwd": _cfg(fuse_ln="fwd"),
    "fuse_ln=False": _cfg(fuse_ln=False),
    "cifar-fp32": _cfg(dtype="fp32"),
    "hd64-bf16": _cfg(geom="HD64", probes=True),
    "hd64-fused64-off": _cfg(geom="HD64", env={"VITPE_ATTN_FUSED64": "0"}),
    "extras-idle": _cfg(extras=True),
    "extras-all": _cfg(extras=True, model=dict(qkv_bias=True, drop_rate=0.1, attn_drop_rate=0.2, drop_path_rate=0.3)),
})
for _pe in ("absolute", "relative", "polynomial", "rope-axial", "rope-mixed"):
    CONFIGS["pe-" + _pe] = _cfg(pe=_pe)
CONFIGS["dataset-augment-clip"] = _cfg(dataset=True)
CONFIGS["depth-1"] = _cfg(depth=1)
# the input side on its other routes: the uint8 gather as a launch of its own (unfold_u8_aug + gemm_nt + the layernorm_fwd
# statistics), the fused embed from uint8 without augmentation (no rng_advance), the gather at p = 16 (K = 768: never fused)
CONFIGS.update({
    "dataset-unfused": _cfg(dataset=True, env={"VITPE_FUSE_EMBED": "0"}, evalother=True),
    "dataset-plain": _cfg(dataset="plain", evalother=True),
    "hd64-dataset": _cfg(geom="HD64", dataset=True, evalother=True),
})
# what runs between the backward and the next forward: schedule, clip, AdamW (plain or grouped), EMA, rng_advance
_OPTIM_ALL = dict(clip=1.0, ema=(0.99, True), groups=dict(no_decay=True, layer_decay=0.75), sched=(1e-3, 40, 5, 1e-5))
CONFIGS.update({
    "optim-all": _cfg(optim=_OPTIM_ALL),
    "optim-all-fp32": _cfg(dtype="fp32", optim=_OPTIM_ALL),      # no bf16 shadow: its pointer is null
    "optim-extras-all": _cfg(extras=True, model=CONFIGS["extras-all"]["model"], optim=_OPTIM_ALL),
    "optim-groups-only": _cfg(optim=dict(groups=_OPTIM_ALL["groups"])),
    "optim-sched-ema": _cfg(optim=dict(ema=(0.99, False), sched=_OPTIM_ALL["sched"])),   # the ticked adamw_step path
})


def route_args(cfg):
    """The host-side description of a configuration's model: what the route depends on."""
    g = GEOMS[cfg["geom"]]
    return dict(dtype=DTYPES[cfg["dtype"]], C=3, S=g["img_size"], patch=g["patch_size"], D=g["embed_dim"], H=g["num_heads"],
                hid=4 * g["embed_dim"], depth=cfg["depth"], classes=10, extras=cfg["extras"], fuse_ln=cfg["fuse_ln"])


@contextlib.contextmanager
def route_environment(env):
    """os.environ with every route switch removed and `env` set, restored afterwards."""
    saved = {k: os.environ.pop(k, None) for k in ROUTE_SWITCHES}
    os.environ.update(env)
    try:
        yield
    finally:
        for k in ROUTE_SWITCHES:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


# ------------------------------------------------------------------------------------------ the recorder
def _stream_last():
    """names of the entry points whose last parameter is the stream"""
    from vitpe import _lib as L
    src = re.sub(r"/\*.*?\*/", " ", open(L.HEADER_PATH).read(), flags=re.S)
    return {m.group(1) for m in re.finditer(r"\bint\s+(vitpe_\w+)\s*\(([^)]*)\)\s*;", src)
            if m.group(2).split(",")[-1].strip().startswith("vitpe_stream_t")}


class _Recorder:
    def __init__(self, handle):
        self._handle, self._stream_last = handle, _stream_last()
        self.calls, self._addr = [], {}

    def _ptr(self, p):
        p = getattr(p, "value", p)
        if p is None or p == 0:
            return None
        return self._addr.setdefault(int(p), len(self._addr))

    def _wgrad(self, name, args):
        from vitpe import kernels as K
        n = args[-1]
        arr = (K._WgradProblem * n).from_address(args[1])
        probs = [[self._ptr(getattr(p, f)) if t is ctypes.c_void_p else getattr(p, f) for f, t in K._WgradProblem._fields_]
                 for p in arr]
        steps = list((ctypes.c_int * n).from_address(args[2])) if name == "vitpe_wgrad_group_rows" else None
        return [args[0], probs, steps, n]

    def __getattr__(self, name):
        fn = getattr(self._handle, name)
        if not name.startswith("vitpe_"):
            return fn

        def call(*args):
            rec = args[:-1] if name in self._stream_last else args
            if name in ("vitpe_wgrad_group", "vitpe_wgrad_group_rows"):
                out = self._wgrad(name, rec)
            else:
                out = [self._ptr(a) if t is ctypes.c_void_p else (repr(float(a)) if t is ctypes.c_float else int(a))
                       for a, t in zip(rec, fn.argtypes)]
            self.calls.append([name[len("vitpe_"):]] + out)
            return fn(*args)
        return call


@contextlib.contextmanager
def recording():
    """-> the list of calls made inside the block, filled as they happen"""
    from vitpe import _lib as L
    handle = L.lib()
    rec = _Recorder(handle)
    L._lib = rec
    try:
        yield rec.calls
    finally:
        L._lib = handle


def digest(calls):
    """(names, SHA-256 of the canonical full trace)"""
    text = json.dumps(calls, separators=(",", ":"))
    return [c[0] for c in calls], hashlib.sha256(text.encode()).hexdigest()


# ------------------------------------------------------------------------------------------ engines and sequences
def build_engine(cfg):
    """(engine, images, labels, idx): depth-3 seeded model, batch 2, eager.  Call inside route_environment(cfg["env"])."""
    from vitpe.data import ResidentDataset
    from vitpe.engine import TrainEngine
    from vitpe.vit import VisionTransformer
    try:
        from vitpe.optim import vit_param_groups
    except ImportError:   # only for re-recording the optim-* goldens from 439e3f7, which keeps it in the engine's module
        from vitpe.engine import vit_param_groups
    g = GEOMS[cfg["geom"]]
    torch.manual_seed(0)
    model = VisionTransformer(pos_encoding=cfg["pe"], depth=cfg["depth"], **g, **cfg["model"]).cuda()
    eng = TrainEngine(model, BATCH, compute_dtype=DTYPES[cfg["dtype"]], use_graph=False, fuse_ln=cfg["fuse_ln"],
                      extras=cfg["extras"])
    gen = torch.Generator().manual_seed(11)
    S = g["img_size"]
    images, labels = torch.randn(BATCH, 3, S, S, generator=gen).cuda(), torch.randint(0, 10, (BATCH,), generator=gen).cuda()
    idx = None
    if cfg["dataset"]:
        ds = ResidentDataset(torch.randint(0, 256, (8, 3, S, S), generator=gen, dtype=torch.uint8),
                             torch.randint(0, 10, (8,), generator=gen), (0.5, 0.5, 0.5), (0.25, 0.25, 0.25))
        eng.attach_dataset(ds)
        if cfg["dataset"] != "plain":
            eng.set_augment(4, True)
            eng.set_grad_clip(1.0)
        idx = torch.tensor([5, 2], device="cuda")
    opt = cfg["optim"]
    if "clip" in opt:
        eng.set_grad_clip(opt["clip"])
    if "ema" in opt:
        eng.set_ema(*opt["ema"])
    if "groups" in opt:
        eng.set_param_groups(vit_param_groups(model, **opt["groups"]))
    if "sched" in opt:
        eng.set_lr_schedule(*opt["sched"])
    return eng, images, labels, idx


def _seq_step(eng, images, labels, idx):
    eng.step_indexed(idx) if idx is not None else eng.step(images, labels)


def _seq_eval(eng, images, labels, idx):
    eng.forward_indexed(idx) if idx is not None else eng.forward_only(images)


def _seq_parts(eng, images, labels, idx):
    eng._fwd_train()
    eng._loss()
    if eng.Lyr >= 2:
        eng._backward("upper")
        eng._backward("lower")
    else:   # one layer has no upper part (the engine never splits its backward): the whole backward instead
        eng._backward()


def _seq_probes(eng, images, labels, idx):
    for probe in eng.kernel_probes():
        for fn in probe["fns"]:
            fn()


def _seq_ema(eng, images, labels, idx):
    with eng.ema_weights():
        _seq_eval(eng, images, labels, idx)


def _seq_evalloss(eng, images, labels, idx):
    """The head's evaluation path: logits, then eval_loss on a full batch twice (one cached control block), on a ragged
    share of a global batch of 2 (another block), and the metrics read."""
    eng.forward_only(images, labels)
    acc = torch.zeros(2, device="cuda")
    eng.eval_loss(2, acc)
    eng.eval_loss(2, acc)
    eng.eval_loss(1, acc, 2)
    eng.read_metrics()


def _check_evalloss(calls):
    """the control block of cross_entropy_ctl (argument 6 of the call): cached for the repeated shape, new for the other"""
    ctl = [c[6] for c in calls if c[0] == "cross_entropy_ctl"]
    assert len(ctl) == 3 and ctl[0] == ctl[1] != ctl[2], ctl


def _seq_evalother(eng, images, labels, idx):
    """forward_indexed on a second 8-record dataset, then on the attached one: the gather of the first call reads the
    foreign set's images, the gather of the second the attached set's (checked against the recorder's address table)."""
    from vitpe import _lib as L
    from vitpe.data import ResidentDataset
    gen = torch.Generator().manual_seed(12)
    S = eng.S
    other = ResidentDataset(torch.randint(0, 256, (8, 3, S, S), generator=gen, dtype=torch.uint8),
                            torch.randint(0, 10, (8,), generator=gen), (0.4, 0.4, 0.4), (0.2, 0.2, 0.2))
    eng.forward_indexed(idx, dataset=other)
    eng.forward_indexed(idx)
    rec = L._lib
    data = [c[3] if c[0] == "patch_embed" else c[2] for c in rec.calls if c[0] in ("patch_embed", "unfold_u8")]
    want = [rec._addr[t.data_ptr()] for t in (other.images, eng.dataset.images)]
    assert data == want and want[0] != want[1], (data, want)


SEQUENCES = (("step", _seq_step), ("eval", _seq_eval), ("parts", _seq_parts), ("probes", _seq_probes), ("ema", _seq_ema),
             ("evalloss", _seq_evalloss), ("evalother", _seq_evalother))


def trace_config(name):
    """-> (route flags, {sequence: calls}) of CONFIGS[name], sequences in SEQUENCES order on one engine"""
    cfg = CONFIGS[name]
    with route_environment(cfg["env"]):
        eng, images, labels, idx = build_engine(cfg)
        route = {f: bool(getattr(eng, f)) for f in ROUTE_FLAGS}
        traces = {}
        for seq, run in SEQUENCES:
            if ((seq == "probes" and not cfg["probes"]) or (seq == "ema" and "ema" not in cfg["optim"])
                    or (seq == "evalloss" and not cfg["evalloss"]) or (seq == "evalother" and not cfg["evalother"])):
                continue
            with recording() as calls:
                run(eng, images, labels, idx)
            torch.cuda.synchronize()
            if seq == "evalloss":
                _check_evalloss(calls)
            traces[seq] = calls
    return route, traces


def main(argv):
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--dump", metavar="DIR", help="write every full trace to DIR/<config>.<sequence>.json")
    ap.add_argument("--write-golden", metavar="FILE", help="write the golden (names, hashes, route flags) to FILE")
    ap.add_argument("--commit", default="", help="hash of the commit the golden is recorded from (stored in it)")
    ap.add_argument("--only", nargs="+", metavar="NAME", choices=list(CONFIGS),
                    help="record these configurations alone; --write-golden then merges them into FILE")
    args = ap.parse_args(argv)
    golden = {"recorded_from": args.commit, "configs": {}}
    if args.only and args.write_golden:
        with open(args.write_golden) as f:
            golden = json.load(f)
    for name in args.only or CONFIGS:
        route, traces = trace_config(name)
        entry = {"route": route, "sequences": {}}
        if args.only:
            entry["recorded_from"] = args.commit
        for seq, calls in traces.items():
            names, sha = digest(calls)
            entry["sequences"][seq] = {"names": " ".join(names), "sha256": sha}
            if args.dump:
                os.makedirs(args.dump, exist_ok=True)
                with open(os.path.join(args.dump, f"{name}.{seq}.json"), "w") as f:
                    f.write("[\n" + ",\n".join(json.dumps(c, separators=(",", ":")) for c in calls) + "\n]\n")
        golden["configs"][name] = entry
        print(name, {s: len(c) for s, c in traces.items()}, flush=True)
    if args.write_golden:
        with open(args.write_golden, "w") as f:
            json.dump(golden, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
