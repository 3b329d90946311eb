"""A real vitpe.optim.StepOptimizer over CPU tensors, for the host-side tests of its argument handling (no device)."""
import torch


def cpu_optimizer(offsets=None, n=64):
    """(the optimizer, the list its drop-graphs callback appends to).  offsets: {id(parameter): offset}, the model's
    parameters as TrainEngine._build_flat records them."""
    from vitpe.optim import StepOptimizer
    dropped = []
    opt = StepOptimizer(torch.zeros(n), torch.zeros(n), None, 1e-3, 0.01, (0.9, 0.999), 1e-8, 1, offsets or {}, n,
                        lambda: dropped.append(1))
    return opt, dropped
