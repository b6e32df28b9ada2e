"""Times of the morphological profile on the device (dmf_morph_markers / _reconstruct / _stack) next to torch
composing the same definition on the device and to the numpy host route, at the sizes a user runs (profiles/band_profile.md).

    python tools/band_profile_bench.py [repeats] [rounds]

Per size (H x W, K = 8 components, P = 4 profiled at radii 2 / 4 / 6), on cuda:0:
  device       markers, the reconstruction in batches of 8 rounds with one read of the counters per batch, the stack
               (the three lib calls of dmf.engine.band_profile on scores that are on the device; no copy back)
  torch        the same planes from torch ops: the windows as max_pool2d of the negated plane padded with -inf, the
               reconstruction as `j = min(max_pool2d(j, 3, 1, 1), f)` steps on all 24 planes at once until torch.equal says stable
               (checked every 8 steps, as the device route reads its counters), the stack as cat / permute
  host         utils.morphology.profile_host, once (numpy, the CPU of the box)
The scores are smooth random fields (a sum of a few box-filtered noise planes); at 145 x 145 component 0 also carries the
serpentine of tests/morph_cases.py, so that the reconstruction has a long way to carry a value (at 512 x 512 the one-pixel-per-step
routes would need minutes for it).  Times are device events around `repeats` back-to-back calls
after a warm-up, the variants alternating inside each of `rounds` rounds; the figure is the median over the rounds.  The device
and torch results are compared bit for bit with each other and with the host route.  One JSON line per size."""
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'dual-modal-fusion_amd'), os.path.join(ROOT, 'tests'), ROOT]
from dmf import lib
from utils import morphology

SIZES = ((145, 145), (512, 512))
K, P, RADII = 8, 4, (2, 4, 6)


def timed(fn, repeats):
    """ms per call: device events around `repeats` calls."""
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(repeats):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / repeats


def scores_for(H, W):
    import morph_cases as mc
    rng = np.random.default_rng(0)
    s = np.empty((H, W, K), dtype=np.float32)
    for k in range(K):
        z = rng.standard_normal((1, 1, H, W)).astype(np.float32)
        t = torch.from_numpy(z)
        s[:, :, k] = sum(F.avg_pool2d(t, 2 * r + 1, 1, r)[0, 0].numpy() * (r + 1) for r in (1, 3, 7)) / (k + 1)
    if H * W <= 145 * 145:                                                  # (the host route needs one step per pixel of corridor)
        s[:, :, 0] += 4 * mc.serpentine(H, W)
    return s


def torch_profile(x, stats):
    """The profile [H, W, C] of the device scores x [H, W, K] from torch ops; stats['steps'] <- the elementary steps taken."""
    n = len(RADII)
    f = x[:, :, :P].permute(2, 0, 1) + 0.0
    mask = torch.cat([f, -f + 0.0])                                          # [2 P, H, W]: the closing side negated, as the kernels
    marks = torch.stack([-F.max_pool2d(F.pad(-mask[None], (r, r, r, r), value=float('-inf')), 2 * r + 1, 1)[0] + 0.0 for r in RADII], 1)
    j = marks.reshape(2 * P * n, *mask.shape[1:])
    fm = mask.repeat_interleave(n, 0)
    steps = 0
    while True:
        prev = j
        for _ in range(8):
            j = torch.minimum(F.max_pool2d(j[None], 3, 1, 1)[0], fm)
        steps += 8
        if torch.equal(j, prev):
            break
    stats['steps'] = steps
    j = j.view(2, P, n, *mask.shape[1:])
    opened, closed = j[0], -j[1] + 0.0
    bands = torch.cat([closed.flip(1), f[:, None], opened], 1).reshape(P * (2 * n + 1), *mask.shape[1:])
    return torch.cat([bands.permute(1, 2, 0), x[:, :, P:]], 2).contiguous()


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    if not torch.cuda.is_available():
        raise SystemExit('band_profile_bench needs the GPU: a CPU run gives no time')
    n = len(RADII)
    for H, W in SIZES:
        sh = scores_for(H, W)
        x = torch.from_numpy(sh).cuda()
        ws = torch.empty(lib.morph_workspace_bytes(H, W, P, n), dtype=torch.uint8, device='cuda')
        mask, X, Y, state = lib.morph_carve(ws, H, W, P, n)
        out = torch.empty(H, W, morphology.band_count(K, P, n), device='cuda')
        stats = {}

        def device_profile():
            lib.morph_markers(x, P, RADII, mask, X, Y)
            stats['rounds'] = lib.morph_reconstruct_run(mask, X, Y, n, state)
            lib.morph_stack(x, P, n, mask, X, out)

        def device_markers():
            lib.morph_markers(x, P, RADII, mask, X, Y)

        variants = (('device_ms', device_profile), ('torch_ms', lambda: torch_profile(x, stats)), ('device_markers_ms', device_markers))
        runs = {k: [] for k, _ in variants}
        for _ in range(rounds):
            for k, fn in variants:
                runs[k].append(timed(fn, repeats))
        res = {'size': [H, W], 'K': K, 'P': P, 'radii': list(RADII), 'repeats': repeats, 'rounds': rounds,
               'workspace_MB': round(ws.numel() / 1e6, 2)}
        for k, v in runs.items():
            res[k] = round(float(np.median(v)), 4)
            res[k + '_minmax'] = [round(min(v), 4), round(max(v), 4)]
        device_profile()
        got = out.cpu().numpy()
        res['device_rounds'] = stats['rounds']
        res['torch_steps'] = stats['steps']
        res['device_equals_torch'] = bool(np.array_equal(got.view(np.uint32), torch_profile(x, stats).cpu().numpy().view(np.uint32)))
        t0 = time.perf_counter()
        want, info = morphology.profile_host(sh, P, RADII)
        res['host_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
        res['host_steps_slowest_plane'] = info['rounds'][0]
        res['device_equals_host'] = bool(np.array_equal(got.view(np.uint32), want.view(np.uint32)))
        print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
