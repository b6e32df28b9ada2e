"""Times of the multi-attribute profile on the device (dmf_attr_multi_levels) next to the old entry point and the
numpy / scipy host route (profiles/attribute_multi.md).

    python tools/attribute_multi_bench.py [repeats] [rounds] [--no-host]

Per size (H x W, K = 8 components, P = 4 profiled, L = 256 levels, T = 16), on cuda:0, each variant the quantiser, every level
1 .. 255 of the 8 planes in 16 calls that read nothing back, and the stack, on scores that are on the device (no copy back):
  area_old     areas 25 / 100 / 400 through dmf_attr_area_levels (four launches a call): the parent's route
  area_new     the same areas through dmf_attr_multi_levels with no diagonal and no std (five launches a call)
  area_diag    areas 25 / 100 + diagonal 20                               (n = 3)
  all_n3       area 100 + diagonal 20 + std 20                            (n = 3, the config.yml example)
  all_n6       areas 25 / 100 + diagonals 10 / 20 + stds 10 / 20          (n = 6)
and `host`: utils.attribute.profile_host of all_n3 and all_n6, once each (numpy + scipy.ndimage, the CPU of the box).
The scores are tools/attribute_profile_bench.py's smooth random fields.  Times are device events around `repeats` back-to-back
profiles after a warm-up, the variants alternating inside each of `rounds` rounds; the figure is the median over the rounds with
the smallest and largest beside it.  The device results of area_new, all_n3 and all_n6 are compared bit for bit with the host
route.  One JSON line per size."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'dual-modal-fusion_amd'), ROOT, os.path.join(ROOT, 'tools')]
from attribute_profile_bench import K, L, P, SIZES, scores_for, timed
from dmf import lib
from utils import attribute

VARIANTS = (('area_new', (25, 100, 400), (), ()), ('area_diag', (25, 100), (20,), ()), ('all_n3', (100,), (20,), (20,)),
            ('all_n6', (25, 100), (10, 20), (10, 20)))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    repeats = int(args[0]) if len(args) > 0 else 3
    rounds = int(args[1]) if len(args) > 1 else 5
    if not torch.cuda.is_available():
        raise SystemExit('attribute_multi_bench needs the GPU: a CPU run gives no time')
    for H, W in SIZES:
        sh = scores_for(H, W)
        x = torch.from_numpy(sh).cuda()
        q = torch.empty(2 * P, H, W, dtype=torch.uint8, device='cuda')
        rng = torch.empty(P, 2, device='cuda')
        res = {'size': [H, W], 'K': K, 'P': P, 'levels': L, 'T': 16, 'repeats': repeats, 'rounds': rounds}
        runs, state = [], {}
        for name, areas, diagonals, stds in (('area_old', (25, 100, 400), (), ()),) + VARIANTS:
            n, counts = len(areas) + len(diagonals) + len(stds), (len(areas), len(diagonals), len(stds))
            nbytes = {T: lib.attr_multi_workspace_bytes(H, W, P, counts[1], counts[2], T) for T in (8, 16)}
            ws = torch.empty(nbytes[16], dtype=torch.uint8, device='cuda')
            count = torch.empty(2 * P, n, H, W, dtype=torch.uint8, device='cuda')
            out = torch.empty(H, W, attribute.band_count(K, P, n), device='cuda')

            def profile(name=name, areas=areas, diagonals=diagonals, stds=stds, n=n, counts=counts, ws=ws, count=count, out=out):
                lib.attr_quantise(x, P, L, q, rng, ws)
                if name == 'area_old':
                    lib.attr_area_run(q, areas, L, count, ws, 16)
                else:
                    lib.attr_multi_run(q, areas + diagonals + stds, counts, L, count, ws, 16)
                lib.attr_stack(x, P, n, L, count, rng, out)

            runs.append((name, profile))
            state[name] = (areas, diagonals, stds, out)
            res[name + '_workspace_T16_T8_MB'] = [round(nbytes[16] / 1e6, 2), round(nbytes[8] / 1e6, 2)]
        times = {name: [] for name, _ in runs}
        for _ in range(rounds):
            for name, fn in runs:
                times[name].append(timed(fn, repeats))
        for name, v in times.items():
            res[name + '_ms'] = round(float(np.median(v)), 4)
            res[name + '_minmax'] = [round(min(v), 4), round(max(v), 4)]
        res['area_new_over_old'] = round(res['area_new_ms'] / res['area_old_ms'], 4)
        for name, fn in runs:
            areas, diagonals, stds, out = state[name]
            if '--no-host' in sys.argv or name in ('area_old', 'area_diag'):   # (area_diag's kernels are all_n3's without the sums)
                continue
            fn()
            got = out.cpu().numpy()
            t0 = time.perf_counter()
            want, _ = attribute.profile_host(sh, P, areas, L, diagonals, stds)
            if name in ('all_n3', 'all_n6'):
                res[name + '_host_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
            res[name + '_equals_host'] = bool(np.array_equal(got.view(np.uint32), want.view(np.uint32)))
        print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
