"""The reference of the weight-averaging tests: torch.optim.swa_utils.AveragedModel on CPU tensors.

`AvgRef(n, kind, decay, start)` follows a flat float32 vector of n elements the way `engine.set_averaging(kind, decay, start)`
does: `update(theta)` after every optimiser step.  Before step `start` the averaged copy is theta itself; from step `start` on
every step is an `AveragedModel.update_parameters` (the first one copies), with `get_ema_multi_avg_fn(decay)` for kind 'ema'
and `get_swa_multi_avg_fn()` for kind 'mean' — AveragedModel's own default on a device with foreach kernels: `_foreach_lerp_`
with 1 / (num_averaged + 1).  `fused_lerp` states torch.lerp's formula with its fused steps written out; the host tests guard
that this CPU's torch.lerp is that form, which the GPU tests' count of unequal bits relies on.
"""
import numpy as np
import torch
from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn, get_swa_multi_avg_fn


class _Flat(torch.nn.Module):
    def __init__(self, n):
        super().__init__()
        self.flat = torch.nn.Parameter(torch.zeros(n, dtype=torch.float32))


class AvgRef:
    def __init__(self, n, kind, decay=0.999, start=1):
        assert kind in ('ema', 'mean') and start >= 1
        self.model = _Flat(n)
        self.averaged = AveragedModel(self.model, multi_avg_fn=get_ema_multi_avg_fn(decay) if kind == 'ema' else get_swa_multi_avg_fn())
        self.start, self.steps = start, 0

    def update(self, theta):
        """theta: the weights after one more optimiser step (anything np.asarray takes); returns value()."""
        self.steps += 1
        with torch.no_grad():
            self.model.flat.copy_(torch.from_numpy(np.ascontiguousarray(np.asarray(theta, dtype=np.float32))))
        if self.steps >= self.start:
            self.averaged.update_parameters(self.model)
        return self.value()

    def value(self):
        src = self.averaged.module if self.steps >= self.start else self.model
        return src.flat.detach().numpy().copy()


def fused_lerp(a, b, w):
    """torch.lerp(a, b, w) on float32 numpy arrays with every fused multiply-add computed exactly (in float64: the product of
    two float32 is exact there, and one rounding of the exact sum to float32 is what fmaf does, up to double rounding, which
    `lerp_is_fused` below does not depend on: it compares against torch)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    w = np.float32(w)
    d = (b - a).astype(np.float32)
    if abs(w) < 0.5:
        return (np.float64(w) * d.astype(np.float64) + a.astype(np.float64)).astype(np.float32)
    return (-np.float64(np.float32(1) - w) * d.astype(np.float64) + b.astype(np.float64)).astype(np.float32)


def lerp_is_fused(n=8009, weights=(0.001, 0.1, 1.0 / 3.0, 0.5), seed=0):
    """Elements (out of n per weight) where torch.lerp on this CPU differs from the fused form."""
    rng = np.random.default_rng(seed)
    bad = 0
    for w in weights:
        a, b = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
        t = torch.lerp(torch.from_numpy(a), torch.from_numpy(b), float(w)).numpy()
        bad += int((t.view(np.int32) != fused_lerp(a, b, w).view(np.int32)).sum())
    return bad
