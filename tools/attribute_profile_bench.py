"""Times of the attribute profile on the device (dmf_attr_quantise / _area_levels / _stack) next to the numpy /
scipy host route, at the sizes a user runs (profiles/attribute_profile.md).

    python tools/attribute_profile_bench.py [repeats] [rounds]

Per size (H x W, K = 8 components, P = 4 profiled at the areas 25 / 100 / 400, L = 256 levels), on cuda:0:
  device_T16 / device_T8   the quantiser, every level 1 .. 255 of the 8 planes in batches of 16 (8) levels — 16 (32) calls of four
               launches, nothing read back — and the stack (the lib calls of dmf.engine.band_profile on scores that are on the
               device; no copy back)
  levels_T16   the area_levels calls alone; divided by 8 x 255 it is the time of one level of one plane inside a batch
  one_call_1   ONE dmf_attr_area_levels call of one level (128) of the two planes of one component (P = 1, T = 1): what the four
               launches of a call cost when there is next to nothing to batch
  label        one dmf_label_components call on an int32 image of the same size (the plane thresholded at level 128): three
               launches, one plane, one level — the yardstick for a level
  host         utils.attribute.profile_host, once (numpy + scipy.ndimage.label, the CPU of the box)
The scores are smooth random fields (a sum of a few box-filtered noise planes).  Times are device events around `repeats`
back-to-back calls after a warm-up, the variants alternating inside each of `rounds` rounds; the figure is the median over the
rounds, with the smallest and largest beside it.  The device result is compared bit for bit with the host route.  One JSON line
per size."""
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'dual-modal-fusion_amd'), ROOT]
from dmf import lib
from utils import attribute

SIZES = ((145, 145), (512, 512))
K, P, AREAS, L = 8, 4, (25, 100, 400), 256


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
    rng = np.random.default_rng(0)
    s = np.empty((H, W, K), dtype=np.float32)
    for k in range(K):
        t = torch.from_numpy(rng.standard_normal((1, 1, H, W)).astype(np.float32))
        s[:, :, k] = sum(F.avg_pool2d(t, 2 * r + 1, 1, r)[0, 0].numpy() * (r + 1) for r in (1, 3, 7)) / (k + 1)
    return s


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    if not torch.cuda.is_available():
        raise SystemExit('attribute_profile_bench needs the GPU: a CPU run gives no time')
    n = len(AREAS)
    for H, W in SIZES:
        sh = scores_for(H, W)
        x = torch.from_numpy(sh).cuda()
        ws = {T: torch.empty(lib.attr_workspace_bytes(H, W, P, n, T), dtype=torch.uint8, device='cuda') for T in (8, 16)}
        q = torch.empty(2 * P, H, W, dtype=torch.uint8, device='cuda')
        count = torch.empty(2 * P, n, H, W, dtype=torch.uint8, device='cuda')
        rng = torch.empty(P, 2, device='cuda')
        out = torch.empty(H, W, attribute.band_count(K, P, n), device='cuda')
        ws1 = torch.empty(lib.attr_workspace_bytes(H, W, 1, n, 1), dtype=torch.uint8, device='cuda')
        count1 = torch.empty(2, n, H, W, dtype=torch.uint8, device='cuda')

        def device_profile(T):
            lib.attr_quantise(x, P, L, q, rng, ws[T])
            lib.attr_area_run(q, AREAS, L, count, ws[T], T)
            lib.attr_stack(x, P, n, L, count, rng, out)

        device_profile(16)
        labels = (q[0] >= 128).to(torch.int32).contiguous()
        comp = torch.empty_like(labels)
        rws = torch.empty(lib.region_workspace_bytes(H, W), dtype=torch.uint8, device='cuda')
        pair = torch.stack([q[0], q[P]]).contiguous()                          # the two planes of component 0

        variants = (('device_T16_ms', lambda: device_profile(16)), ('device_T8_ms', lambda: device_profile(8)),
                    ('levels_T16_ms', lambda: lib.attr_area_run(q, AREAS, L, count, ws[16], 16)),
                    ('one_call_1_level_2_planes_ms', lambda: lib.attr_area_levels(pair, AREAS, L, 128, 1, count1, ws1, 1)),
                    ('label_components_ms', lambda: lib.label_components(labels, comp, rws)))
        runs = {k: [] for k, _ in variants}
        for _ in range(rounds):
            for k, fn in variants:
                runs[k].append(timed(fn, repeats))
        res = {'size': [H, W], 'K': K, 'P': P, 'areas': list(AREAS), 'levels': L, 'repeats': repeats, 'rounds': rounds,
               'workspace_T16_MB': round(ws[16].numel() / 1e6, 2), 'workspace_T8_MB': round(ws[8].numel() / 1e6, 2)}
        for k, v in runs.items():
            res[k] = round(float(np.median(v)), 4)
            res[k + '_minmax'] = [round(min(v), 4), round(max(v), 4)]
        res['one_level_one_plane_in_a_batch_us'] = round(res['levels_T16_ms'] * 1e3 / (2 * P * (L - 1)), 3)
        res['launches_T16'] = 3 + 4 * -(-(L - 1) // 16) + 1
        device_profile(16)
        got = out.cpu().numpy()
        t0 = time.perf_counter()
        want, _ = attribute.profile_host(sh, P, AREAS, L)
        res['host_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
        res['device_equals_host'] = bool(np.array_equal(got.view(np.uint32), want.view(np.uint32)))
        print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
