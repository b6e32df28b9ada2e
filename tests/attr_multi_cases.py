"""The fixtures of the multi-attribute profile tests; the reference that goes with them is tests/attr_multi_ref.py.
Everything is seeded and read-only.  A case is (name, scores [H, W, K] float32, P, areas, diagonals, stds, L); the components
P .. K - 1 are noise that has to pass through bit for bit.  Each case is named for the failure it catches:

  row_1x40 / column_40x1 / small_5x4   rows shorter than a wave: a run of equal roots in a wave spans several image rows, so a box
                                       taken from "one row per run" comes out too narrow or too low
  past_the_tile_17x33_L2 / L7 / L256   components across the 16 x 16 tile border and corner; the batch sizes at L - 1 = 1, 6, 255
  ring_at_the_tile_corner_33x34        small area, large diagonal: a hollow square ring one pixel wide around the tile corner; area and
                                       diagonal disagree, and the expected levels are written out below (RING_EXPECTED)
  serpentine_67x131                    one component whose box is the whole image, met by runs from every row
  std_staircase_12x20                  the subtractive rule is not the max rule (STAIR_EXPECTED, written out by hand)
  constant_9x11                        no level at all: every std opening is level 0 and every std closing L - 1
  ties_67x131 / signed_zeros_18x19     exact ties and +-0

Thresholds come from: areas [1, 50]; diagonals [1, 6, 40, a value above the image diagonal]; stds [1, 3, L - 1]."""
import collections
import functools

import numpy as np

import attr_cases as ac
import morph_cases as mc

Case = collections.namedtuple('Case', 'name scores P areas diagonals stds L')
ABOVE = 1000                                                 # above the diagonal of every plane here

# ---- the ring: rows and columns 10 .. 21 of a 33 x 34 plane at 1.0 on 0.0, L = 4, so q = 3 on the ring and 0 elsewhere.
# The ring has 4 x 11 = 44 pixels in a 12 x 12 box (diagonal^2 = 288 = 16.97^2); it encloses 10 x 10 = 100 pixels in a 10 x 10 box
# (diagonal^2 = 200 = 14.1^2), 4-connected to nothing outside; the outside has 33 x 34 - 144 = 978 pixels in the full box.
RING_LO, RING_HI, RING_L = 10, 21, 4
RING_THRESHOLDS = dict(areas=(50,), diagonals=(16, 17), stds=(1,))
# (opened, closed) level per threshold in the regions ring / inside / outside:
#   area 50      the ring is too small at levels 1..3: opened 0.  Dual plane (ring 0, rest 3): inside and outside are large enough at
#                every level: count 3, closed 3 - 3 = 0; the ring itself has no level: closed 3 - 0 = 3.
#   diagonal 16  288 >= 256: the ring stays, opened 3.  Dual: the inside's 200 < 256 fails at every level, closed 3 - 0 = 3 — the
#                hole is filled; the outside passes: 0.
#   diagonal 17  288 < 289: the ring goes.  Dual as at 16.
#   std 1        every component of either plane is flat: nothing qualifies: opened 0, closed 3 everywhere.
RING_EXPECTED = {
    ('a', 50): dict(ring=(0, 3), inside=(0, 0), outside=(0, 0)),
    ('d', 16): dict(ring=(3, 3), inside=(0, 3), outside=(0, 0)),
    ('d', 17): dict(ring=(0, 3), inside=(0, 3), outside=(0, 0)),
    ('s', 1): dict(ring=(0, 3), inside=(0, 3), outside=(0, 3)),
}

# ---- the staircase: a 12 x 20 plane of whole numbers 0 .. 5 at L = 6 (the quantiser is then the identity): a 3 x 3 plateau at 5,
# beside it a 3 x 3 shoulder at 3, a field at 1 and one pixel at 0.  For a plateau pixel and the std threshold 1:
#   t = 5, 4   S = the plateau, 9 pixels at 5: 9 * 225 - 45^2 = 0 < 1 * 81                                      fails
#   t = 3, 2   S = plateau + shoulder, 18 pixels: 18 * 306 - 72^2 = 324 >= 1 * 324 (an exact tie)                passes
#   t = 1      S = everything but the 0: 239 pixels, sum 293, squares 527: 239 * 527 - 293^2 = 40104 < 57121    fails
# so the count is 2 where the largest qualifying level is 3; the shoulder (q = 3) also has 2, the field 0.  At the std threshold 2:
# 324 < 4 * 324, nothing qualifies.
STAIR_H, STAIR_W, STAIR_L = 12, 20, 6
STAIR_PLATEAU, STAIR_SHOULDER, STAIR_ZERO = (slice(4, 7), slice(5, 8)), (slice(4, 7), slice(8, 11)), (11, 19)
STAIR_THRESHOLDS = dict(areas=(1,), diagonals=(1,), stds=(1, 2))
STAIR_EXPECTED = {('s', 1): dict(plateau=2, shoulder=2, field=0, largest_qualifying_level=3), ('s', 2): dict(plateau=0, shoulder=0, field=0)}


def ring():
    f = np.zeros((33, 34), dtype=np.float32)
    f[RING_LO:RING_HI + 1, RING_LO:RING_HI + 1] = 1.0
    f[RING_LO + 1:RING_HI, RING_LO + 1:RING_HI] = 0.0
    return f


def ring_regions():
    """name -> boolean mask [33, 34]."""
    on = ring() > 0
    inside = np.zeros_like(on)
    inside[RING_LO + 1:RING_HI, RING_LO + 1:RING_HI] = True
    return dict(ring=on, inside=inside, outside=~on & ~inside)


def staircase():
    f = np.ones((STAIR_H, STAIR_W), dtype=np.float32)
    f[STAIR_PLATEAU] = 5.0
    f[STAIR_SHOULDER] = 3.0
    f[STAIR_ZERO] = 0.0
    return f


def stair_regions():
    f = staircase()
    return dict(plateau=f == 5, shoulder=f == 3, field=f == 1)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case."""
    noise = lambda H, W, seed: np.random.default_rng(seed).standard_normal((H, W)).astype(np.float32)     # noqa: E731
    wn = ac._with_noise
    past = lambda: wn([noise(17, 33, 13), ac.smooth(17, 33, 14)], 23)                                      # noqa: E731
    made = [
        Case('row_1x40', wn([noise(1, 40, 10)], 20), 1, (1,), (6,), (3,), 256),
        Case('column_40x1', wn([noise(40, 1, 11)], 21), 1, (1, 50), (1, 6, 40, ABOVE), (3, 6), 7),                # n = 8
        Case('small_5x4', wn([noise(5, 4, 12)], 22), 1, (1,), (1,), (1,), 256),
        Case('past_the_tile_17x33_L2', past(), 2, (1, 50), (1, 6, 40, ABOVE), (1,), 2),
        Case('past_the_tile_17x33_L7', past(), 2, (50,), (6,), (3,), 7),
        Case('past_the_tile_17x33_L256', past(), 2, (1, 50), (1, 6, 40), (1, 3, 255), 256),                        # n = 8
        Case('ring_at_the_tile_corner_33x34', wn([ring()], 31), 1, RING_THRESHOLDS['areas'], RING_THRESHOLDS['diagonals'],
             RING_THRESHOLDS['stds'], RING_L),
        Case('serpentine_67x131', wn([np.array(mc.serpentine(67, 131))], 25), 1, (50,), (40, 148), (3,), 256),
        Case('std_staircase_12x20', wn([staircase()], 32), 1, STAIR_THRESHOLDS['areas'], STAIR_THRESHOLDS['diagonals'],
             STAIR_THRESHOLDS['stds'], STAIR_L),
        Case('constant_9x11', wn([np.full((9, 11), 0.375, dtype=np.float32)], 29), 1, (1, 50), (1, 6, 40), (1, 3, 255), 256),   # n = 8
        Case('ties_67x131', wn([np.array(mc.ties())], 28), 1, (50,), (6,), (3,), 7),
        Case('signed_zeros_18x19', wn([ac.signed_zeros(), np.array(mc.zeros(18, 19))], 30), 2, (1,), (40,), (6,), 7),
    ]
    return {c.name: c for c in made}


NAMES = tuple(cases())
