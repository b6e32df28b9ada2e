"""Times of the two band-reduction kernels (dmf_band_moments, dmf_band_project) next to torch composing the same
on the device and to the numpy float64 host route, at the sizes a user runs (profiles/band_reduce.md).

    python tools/band_reduce_bench.py [repeats] [rounds]

Per size (H x W x C, K = 32), on cuda:0:
  moments      dmf_band_moments (four launches)          vs  torch: m = x.mean(0); d = x - m; d.T @ d / (N - 1)   (fp32)
  project      dmf_band_project                          vs  torch: (x - m) @ W                                    (fp32)
  host         utils.spectral.moments_host and the float64 projection, once (numpy, the CPU of the box)
Times are device events around `repeats` back-to-back calls after a warm-up, the variants alternating inside each of `rounds`
rounds; the figure is the median over the rounds.  Shares of the roofs are computed from the shapes: the covariance needs
N C^2 fmas on the upper triangle's tiles at least N C (C + 1) / 2 — the figure below counts 2 N C^2 / 2 flops, the symmetric
half — against the fp32 matrix peak (157.3 Tflop/s), and either kernel reads x once at least (4 N C bytes against 8 TB/s; the
moments read it twice: the means come first).  One JSON line per size."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'dual-modal-fusion_amd'), ROOT]
from dmf import lib
from utils import spectral

SIZES = ((145, 145, 200), (512, 512, 224))
K = 32
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
        raise SystemExit('band_reduce_bench needs the GPU: a CPU run gives no time')
    for H, W, C in SIZES:
        N = H * W
        g = torch.Generator(device='cuda').manual_seed(0)
        x = torch.rand(N, C, device='cuda', generator=g)
        mean = torch.empty(C, dtype=torch.float64, device='cuda')
        cov = torch.empty(C, C, dtype=torch.float64, device='cuda')
        ws = torch.empty(lib.band_moments_workspace_bytes(N, C) // 8, dtype=torch.float64, device='cuda')
        basis = torch.linalg.qr(torch.randn(C, C, device='cuda', generator=g))[0][:, :K].contiguous()
        y = torch.empty(N, K, device='cuda')

        def torch_moments():
            m = x.mean(0)
            d = x - m
            return m, d.T @ d / (N - 1)

        def torch_project():
            return (x - mean32) @ basis

        lib.band_moments(x, mean, cov, ws)
        mean32 = mean.float()
        variants = (('moments_ms', lambda: lib.band_moments(x, mean, cov, ws)), ('torch_moments_ms', torch_moments),
                    ('project_ms', lambda: lib.band_project(x, mean, basis, y)), ('torch_project_ms', torch_project))
        runs = {k: [] for k, _ in variants}
        for _ in range(rounds):
            for k, fn in variants:
                runs[k].append(timed(fn, repeats))
        res = {'size': [H, W, C], 'K': K, 'repeats': repeats, 'rounds': rounds, 'workspace_MB': round(ws.numel() * 8 / 1e6, 1)}
        for k, v in runs.items():
            res[k] = round(float(np.median(v)), 4)
            res[k + '_minmax'] = [round(min(v), 4), round(max(v), 4)]
        # agreement of the two device routes (fp32 torch against the kernels), as a sanity figure
        tm, tc = torch_moments()
        res['torch_vs_kernel_cov_max_abs'] = float((tc.double() - cov).abs().max())
        res['torch_vs_kernel_y_max_abs'] = float((torch_project() - y).abs().max())
        res['moments_share_f32_matrix'] = round(N * C * C / PEAK_F32_MATRIX / (res['moments_ms'] * 1e-3), 3)
        res['moments_share_hbm'] = round(2 * 4 * N * C / PEAK_HBM / (res['moments_ms'] * 1e-3), 3)
        res['project_share_f32_matrix'] = round(2 * N * C * K / PEAK_F32_MATRIX / (res['project_ms'] * 1e-3), 3)
        res['project_share_hbm'] = round(4 * N * (C + K) / PEAK_HBM / (res['project_ms'] * 1e-3), 3)
        # the host route, once
        xh = x.cpu().numpy()
        t0 = time.perf_counter()
        mh, ch = spectral.moments_host(xh)
        res['host_moments_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
        bh = basis.cpu().numpy()
        t0 = time.perf_counter()
        spectral.centred(xh, mh) @ bh.astype(np.float64)
        res['host_project_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
        res['host_vs_kernel_cov_max_abs'] = float(np.abs(ch - cov.cpu().numpy()).max())
        print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
