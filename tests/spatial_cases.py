"""The cases of the spatial-regularisation tests, shared by tests/test_spatial_host.py (the guards, on the float64
reference alone) and tests/test_gpu_spatial.py.  A plain module: no GPU, nothing of the HIP library.

A case is a scene of piecewise-constant regions (blocks of 5 x 4 pixels, five base spectra, 0.05 Gaussian noise, normalised to
[0, 1] as the resident scene is), logits that favour the class `region mod K` of a pixel's region (2 onehot + 1.5 N(0, 1): a
noisy per-pixel classifier whose errors the filter can repair from the pixel's own region) and a mask of about 90 % ones."""
import functools

import numpy as np

SIGMA_S, SIGMA_R = 2.0, 0.1
SIZES = ((1, 1), (2, 7), (13, 9), (33, 17), (35, 34), (64, 65))     # smaller than r + 1; one off the 16- and 32-pixel tiles
RADII = (1, 2, 3)
BANDS_F32 = (1, 3, 4, 8, 200, 224)
BANDS_F16 = (8, 200)
FILTER_K = (1, 3, 17, 64)
SCATTER_K, SCATTER_B, SCATTER_BETA = (1, 2, 3, 17, 64), (1, 63, 257), (1.0, 0.5)
BLOCK = (5, 4)
GUARD_MIN_PIXELS = 100                   # the share guards are asked of scenes of at least this many pixels


def regions(H, W):
    """[H, W] int: the region of every pixel, blocks of 5 x 4 numbered row by row."""
    i, j = np.arange(H)[:, None] // BLOCK[0], np.arange(W)[None, :] // BLOCK[1]
    return i * ((W + BLOCK[1] - 1) // BLOCK[1]) + j


@functools.lru_cache(maxsize=None)
def scene(H, W, C, half=False):
    """[H, W, C] float32 (or float16) in [0, 1]."""
    rng = np.random.default_rng(7000 + 131 * H + 17 * W + C)
    base = rng.random((5, C))
    a = base[regions(H, W) % 5] + 0.05 * rng.standard_normal((H, W, C))
    lo, hi = a.min(), a.max()
    a = ((a - lo) / (hi - lo) if hi > lo else np.zeros_like(a)).astype(np.float32)
    a = a.astype(np.float16) if half else a
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def logits(H, W, K):
    """[H W, K] float32, row i W + j for pixel (i, j)."""
    rng = np.random.default_rng(9000 + 131 * H + 17 * W + K)
    onehot = np.eye(K)[(regions(H, W) % K).reshape(-1)]
    out = (2.0 * onehot + 1.5 * rng.standard_normal((H * W, K))).astype(np.float32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def mask(H, W):
    """[H, W] uint8, about 90 % ones."""
    rng = np.random.default_rng(5000 + 131 * H + 17 * W)
    m = (rng.random((H, W)) < 0.9).astype(np.uint8)
    m.setflags(write=False)
    return m


def pixels(H, W):
    """[H W, 2] int32: every pixel, in row order."""
    return np.stack(np.meshgrid(np.arange(H), np.arange(W), indexing='ij'), 2).reshape(-1, 2).astype(np.int32)


# what every radius is run on: (H, W, K), every size with every class count; (H, W, C, half), with every band count and type
FILTER_CASES = [(H, W, K) for H, W in SIZES for K in FILTER_K]
AFFINITY_CASES = [(H, W, C, half) for H, W in SIZES for C, half in [(C, False) for C in BANDS_F32] + [(C, True) for C in BANDS_F16]]
