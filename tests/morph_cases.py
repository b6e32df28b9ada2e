"""The fixtures of the morphological-profile tests.  Everything is seeded and read-only; the reference that
goes with them is tests/morph_ref.py.

The serpentine: background noise in [0, 0.25); a plateau of 1.0 that starts as a 7 x 7 room in the top left corner and leaves it
as a corridor 3 pixels wide, which runs to the right edge, turns, runs back to the left edge one wall of 2 pixels further down,
and so on to the bottom: one connected path, row by row, across the whole image.  The corridor keeps one pixel of noise between
itself and the image border, so that no clipped window fits inside it.  An erosion of radius >= 2 leaves nothing of the plateau
but the room; the reconstruction has to carry 1.0 from there down the whole corridor, across every tile border and in both
directions, where the plain opening delta_r(eps_r(f)) gives back the room alone."""
import functools

import numpy as np

SERPENTINE_SHAPES = ((33, 37), (67, 131), (130, 71))
SERPENTINE_RADII = (1, 2, 3)
ROOM, CORRIDOR, WALL = 7, 3, 2


def _frozen(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def serpentine(H, W, seed=0):
    f = np.random.default_rng(seed).random((H, W), dtype=np.float32) * np.float32(0.25)
    f[:ROOM, :ROOM] = 1.0
    f[2:2 + CORRIDOR, ROOM:W - 1] = 1.0                                   # leg 0 leaves the room to the right
    top, prev, right = ROOM + WALL, 2, True                               # the next leg's first row; the last leg's; which end turns
    while top + CORRIDOR <= H - 1:
        f[top:top + CORRIDOR, 1:W - 1] = 1.0
        cols = slice(W - 1 - CORRIDOR, W - 1) if right else slice(1, 1 + CORRIDOR)
        f[prev:top, cols] = 1.0                                           # the turn that joins the two legs at one end
        prev, top, right = top, top + CORRIDOR + WALL, not right
    return _frozen(f)


@functools.lru_cache(maxsize=None)
def ties(H=67, W=131, seed=1):
    """Many exact ties: values drawn from 7 levels."""
    levels = np.array([-1.5, -0.25, 0.0, 0.125, 0.5, 0.75, 2.0], dtype=np.float32)
    return _frozen(levels[np.random.default_rng(seed).integers(0, 7, (H, W))])


@functools.lru_cache(maxsize=None)
def zeros(H=33, W=37, seed=2):
    """-0.0 and +0.0 with a few values on either side of them."""
    levels = np.array([-0.0, 0.0, -0.0, 0.0, -1e-30, 1e-30], dtype=np.float32)
    return _frozen(levels[np.random.default_rng(seed).integers(0, 6, (H, W))])


@functools.lru_cache(maxsize=None)
def noise(H, W, seed=3):
    return _frozen(np.random.default_rng(seed).standard_normal((H, W)).astype(np.float32))


def planes():
    """name -> (plane, radii): every further plane of the issue with the radii it is profiled at."""
    return {'ties': (ties(), (1, 3)), 'zeros': (zeros(), (1, 2)), 'constant': (_frozen(np.full((9, 11), 0.375)), (1, 4)),
            'one_row': (noise(1, 70), (1, 6)), 'one_column': (noise(41, 1), (2, 5)), 'small': (noise(5, 4), (1, 6))}


@functools.lru_cache(maxsize=None)
def scores(H, W, K, seed=4):
    """Scores [H, W, K]: the serpentine, the ties plane cut to size, then noise."""
    rng = np.random.default_rng(seed)
    s = rng.standard_normal((H, W, K)).astype(np.float32)
    s[:, :, 0] = serpentine(H, W)
    if K > 1 and H <= 67 and W <= 131:
        s[:, :, 1] = ties()[:H, :W]
    return _frozen(s)
