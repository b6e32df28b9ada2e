"""The independent reference of the morphological-profile tests: scipy.ndimage for the windows, a plain loop of
the 3 x 3 filter for the reconstruction.  It shares no code with utils/morphology.py.  float32 in gives float32 out, and all of it
is min / max: what it returns is compared bit for bit (`bits`)."""
import numpy as np
from scipy import ndimage

INF = np.float32(np.inf)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def canon(x):
    return np.asarray(x, dtype=np.float32) + np.float32(0.0)


def erode(f, r):
    return ndimage.minimum_filter(f, size=2 * r + 1, mode='constant', cval=INF)


def dilate(f, r):
    return ndimage.maximum_filter(f, size=2 * r + 1, mode='constant', cval=-INF)


def rec_dilation(marker, mask):
    """-> (R^delta(marker | mask), rounds): one pixel per round."""
    j, rounds = marker, 0
    while True:
        nxt = np.minimum(ndimage.maximum_filter(j, size=3, mode='constant', cval=-INF), mask)
        rounds += 1
        if np.array_equal(nxt, j):
            return j, rounds
        j = nxt


def rec_erosion(marker, mask):
    j, rounds = marker, 0
    while True:
        nxt = np.maximum(ndimage.minimum_filter(j, size=3, mode='constant', cval=INF), mask)
        rounds += 1
        if np.array_equal(nxt, j):
            return j, rounds
        j = nxt


def opening(f, r):
    return rec_dilation(erode(f, r), f)[0]


def closing(f, r):
    return rec_erosion(dilate(f, r), f)[0]


def profile(scores, P, radii):
    """[H, W, K + 2 n P]: per profiled component the closings from the widest radius down, the component, the openings from the
    narrowest up; then the other components as they are."""
    bands = []
    for p in range(P):
        f = canon(scores[:, :, p])
        bands += [closing(f, r) for r in reversed(radii)] + [f] + [opening(f, r) for r in radii]
    bands += [scores[:, :, k] for k in range(P, scores.shape[2])]
    return np.stack(bands, axis=-1).astype(np.float32)
