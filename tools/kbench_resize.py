#!/usr/bin/env python3
"""transforms.Resize on the device (kernels.resize_u8), HIP-event timed on whole datasets: CIFAR-10 train
50 000 x 3 x 32 x 32 -> 64 and -> 224, MNIST train 60 000 x 1 x 28 x 28 -> 32, and the host path it replaces for MNIST -> 32
(torch.nn.functional.interpolate + round, wall clock).  The call runs once per dataset, so the figures are the time of
ONE call (kernel plus the upload of the coefficient tables) averaged over a few repeats into a preallocated output, and
the achieved write rate (output bytes / time) next to the MI355X HBM rates.  Prints one JSON line per measurement."""
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "vit-rpe-rope_amd"))
from vitpe import kernels as K  # noqa: E402
from kbench_heads import timeit  # noqa: E402

HBM_MEASURED_TBS = 6.29      # float4 copy on the MI355X; 8.0 TB/s is the specification


def main():
    assert torch.cuda.is_available(), "needs the MI355X"
    g = torch.Generator().manual_seed(0)
    for name, (N, C, S0), S in (("cifar10", (50000, 3, 32), 64), ("cifar10", (50000, 3, 32), 224),
                                ("mnist", (60000, 1, 28), 32)):
        host = torch.randint(0, 256, (N, C, S0, S0), generator=g, dtype=torch.uint8)
        x = host.cuda()
        out = torch.empty((N, C, S, S), dtype=torch.uint8, device="cuda")
        us = timeit(lambda: K.resize_u8(x, S, out=out), iters=10, warm=2)
        wr, rd = out.numel(), x.numel()
        rec = {"kernel": "resize_u8", "dataset": name, "N": N, "C": C, "S0": S0, "S": S, "ms": round(us / 1e3, 3),
               "write_GB": round(wr / 1e9, 3), "write_TBs": round(wr / us / 1e6, 3),
               "write_frac_of_measured_hbm": round(wr / us / 1e6 / HBM_MEASURED_TBS, 3),
               "read_plus_write_TBs": round((wr + rd) / us / 1e6, 3)}
        if name == "mnist":     # the host path that ResidentDataset.from_files used before (read_mnist_idx at img_size != 28)
            t0 = time.perf_counter()
            y = torch.nn.functional.interpolate(host.float(), size=(S, S), mode="bilinear", align_corners=False)
            y = y.round().clamp(0, 255).to(torch.uint8)
            rec["cpu_interpolate_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            rec["cpu_threads"] = torch.get_num_threads()
        del x, out
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
