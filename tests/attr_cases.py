"""The fixtures of the attribute-profile tests.  Everything is seeded and read-only; the reference that goes with
them is tests/attr_ref.py.  The kernel's failure modes are at tile (16 x 16) and wave (64 lanes) edges, so the planes are small.

A case is (name, scores [H, W, K] float32, P, areas, L); the components P .. K - 1 are noise that has to pass through bit for bit."""
import collections
import functools

import numpy as np

import morph_cases as mc

Case = collections.namedtuple('Case', 'name scores P areas L')
BLOB_AREA = 7
# a 4-connected path through the corner where the tiles (0, 0), (0, 1), (1, 1) and (1, 0) meet (rows and columns 15 | 16): its first
# 6, 7 and 8 pixels are blobs of BLOB_AREA - 1, BLOB_AREA and BLOB_AREA + 1 pixels that lie in all four tiles
BLOB_PATH = ((15, 15), (15, 16), (16, 16), (16, 15), (17, 15), (17, 16), (17, 17), (16, 17))


def _frozen(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    a.setflags(write=False)
    return a


def areas_for(H, W):
    """[1, 7, 50, H W, H W + 1] where they fit: as a strictly increasing list."""
    return tuple(sorted({1, 7, 50, H * W, H * W + 1}))


def _with_noise(planes, seed):
    """planes [P][H, W] -> scores [H, W, P + 1]: one more component of noise (with a -0) that is not profiled."""
    H, W = planes[0].shape
    extra = np.random.default_rng(seed).standard_normal((H, W)).astype(np.float32)
    extra[0, 0] = -0.0
    return _frozen(np.stack(list(planes) + [extra], axis=2))


def smooth(H, W, seed=5):
    """A few random plane waves and a little noise: large components at every level, with ragged borders."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    f = np.zeros((H, W))
    for _ in range(5):
        ky, kx, ph = rng.uniform(-0.25, 0.25), rng.uniform(-0.25, 0.25), rng.uniform(0, 2 * np.pi)
        f += rng.uniform(0.5, 1.0) * np.sin(ky * y + kx * x + ph)
    return (f + 0.05 * rng.standard_normal((H, W))).astype(np.float32)


def checkerboard(H=33, W=34):
    y, x = np.mgrid[0:H, 0:W]
    return ((y + x) % 2).astype(np.float32)


def blobs(H=33, W=33):
    """Three planes: a blob of BLOB_AREA - 1, BLOB_AREA, BLOB_AREA + 1 pixels at 1.0 across the tile corner, on a background of 0
    with one lone bright pixel far away (so that hi = 1 whatever happens to the blob)."""
    out = []
    for extra in (-1, 0, 1):
        f = np.zeros((H, W), dtype=np.float32)
        for (i, j) in BLOB_PATH[:BLOB_AREA + extra]:
            f[i, j] = 1.0
        f[H - 1, W - 1] = 1.0
        out.append(f)
    return out


def signed_zeros(H=18, W=19, seed=6):
    return np.where(np.random.default_rng(seed).integers(0, 2, (H, W)) == 1, np.float32(-0.0), np.float32(0.0)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case, in the order of the issue's list."""
    noise = lambda H, W, seed: np.random.default_rng(seed).standard_normal((H, W)).astype(np.float32)     # noqa: E731
    made = [
        Case('row_1x40', _with_noise([noise(1, 40, 10)], 20), 1, areas_for(1, 40), 256),
        Case('column_40x1', _with_noise([noise(40, 1, 11)], 21), 1, areas_for(40, 1), 7),
        Case('small_5x4', _with_noise([noise(5, 4, 12)], 22), 1, areas_for(5, 4), 256),
        Case('past_the_tile_17x33_L2', _with_noise([noise(17, 33, 13), smooth(17, 33, 14)], 23), 2, areas_for(17, 33), 2),
        Case('past_the_tile_17x33_L7', _with_noise([noise(17, 33, 13), smooth(17, 33, 14)], 23), 2, areas_for(17, 33), 7),
        Case('past_the_tile_17x33_L256', _with_noise([noise(17, 33, 13), smooth(17, 33, 14)], 23), 2, areas_for(17, 33), 256),
        Case('smooth_64x65', _with_noise([smooth(64, 65)], 24), 1, areas_for(64, 65), 256),
        Case('serpentine_67x131', _with_noise([np.array(mc.serpentine(67, 131))], 25), 1, areas_for(67, 131), 256),
        Case('checkerboard_33x34_L2', _with_noise([checkerboard()], 26), 1, (1, 2), 2),
        Case('blobs_at_the_tile_corner', _with_noise(blobs(), 27), 3, (1, BLOB_AREA, 50), 7),
        Case('ties_67x131', _with_noise([np.array(mc.ties())], 28), 1, (1, 7, 50), 7),
        Case('constant_9x11', _with_noise([np.full((9, 11), 0.375, dtype=np.float32)], 29), 1, areas_for(9, 11), 256),
        Case('signed_zeros_18x19', _with_noise([signed_zeros(), np.array(mc.zeros(18, 19))], 30), 2, (1, 7, 50), 7),
    ]
    return {c.name: c for c in made}


NAMES = tuple(cases())
