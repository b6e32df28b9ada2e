"""Times of the noise-moments kernel (dmf_band_noise_moments) next to (a) torch composing the same on the device
and (b) dmf_band_moments at the same size, whose covariance it shares its arithmetic with (profiles/noise_adjusted.md).

    python tools/noise_moments_bench.py [repeats] [rounds]

Per size (H x W x C) and direction, on cuda:0:
  noise        dmf_band_noise_moments (two launches)
  torch        e = x[:, :-1] - x[:, 1:] (horizontal; x[:-1] - x[1:] vertical), flattened; e.T @ e / (2 M)      (fp32)
  moments      dmf_band_moments (four launches: means, covariance, finish)
Times are device events around `repeats` back-to-back calls after a warm-up, the variants alternating inside each of `rounds`
rounds; the figure is the median over the rounds.  Shares of the roofs are computed from the shapes, as
tools/band_reduce_bench.py does for the covariance: 2 N C^2 / 2 flops, the symmetric half, against the fp32 matrix peak
(157.3 Tflop/s), and ONE read of x (4 N C bytes against 8 TB/s; the neighbour's read is the same bytes again, one pixel or one row
later, and is expected to come from cache).  One JSON line per size and direction."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'dual-modal-fusion_amd'), ROOT]
from dmf import lib

SIZES = ((145, 145, 200), (512, 512, 224))
PEAK_F32_MATRIX, PEAK_HBM = 157.3e12, 8.0e12


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


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    if not torch.cuda.is_available():
        raise SystemExit('noise_moments_bench needs the GPU: a CPU run gives no time')
    for H, W, C in SIZES:
        N = H * W
        g = torch.Generator(device='cuda').manual_seed(0)
        x = torch.rand(H, W, C, device='cuda', generator=g)
        flat = x.view(N, C)
        mean = torch.empty(C, dtype=torch.float64, device='cuda')
        cov = torch.empty(C, C, dtype=torch.float64, device='cuda')
        ncov = torch.empty(C, C, dtype=torch.float64, device='cuda')
        ws = torch.empty(lib.band_moments_workspace_bytes(N, C) // 8, dtype=torch.float64, device='cuda')
        nws = torch.empty(lib.band_noise_workspace_bytes(H, W, C) // 8, dtype=torch.float64, device='cuda')
        for direction in ('horizontal', 'vertical'):
            M = H * (W - 1) if direction == 'horizontal' else (H - 1) * W

            def torch_noise():
                e = (x[:, :-1] - x[:, 1:] if direction == 'horizontal' else x[:-1] - x[1:]).reshape(-1, C)
                return e.T @ e / (2 * M)

            variants = (('noise_ms', lambda: lib.band_noise_moments(x, H, W, ncov, direction, nws)), ('torch_ms', torch_noise),
                        ('moments_ms', lambda: lib.band_moments(flat, mean, cov, ws)))
            runs = {k: [] for k, _ in variants}
            for _ in range(rounds):
                for k, fn in variants:
                    runs[k].append(timed(fn, repeats))
            res = {'size': [H, W, C], 'direction': direction, 'repeats': repeats, 'rounds': rounds,
                   'workspace_MB': round(nws.numel() * 8 / 1e6, 1)}
            for k, v in runs.items():
                res[k] = round(float(np.median(v)), 4)
                res[k + '_minmax'] = [round(min(v), 4), round(max(v), 4)]
            res['noise_over_torch'] = round(res['noise_ms'] / res['torch_ms'], 3)
            res['noise_over_moments'] = round(res['noise_ms'] / res['moments_ms'], 3)
            res['noise_share_f32_matrix'] = round(N * C * C / PEAK_F32_MATRIX / (res['noise_ms'] * 1e-3), 3)
            res['noise_share_hbm'] = round(4 * N * C / PEAK_HBM / (res['noise_ms'] * 1e-3), 3)
            # agreement of the two device routes (fp32 torch against the kernel), as a sanity figure
            lib.band_noise_moments(x, H, W, ncov, direction, nws)
            res['torch_vs_kernel_max_abs'] = float((torch_noise().double() - ncov).abs().max())
            print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
