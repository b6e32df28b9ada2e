"""utils.attribute — the host side of `band_profile: area`: the config keys, the band order, the definition of
the extended attribute profile (area attribute) in numpy (the drop-in route of `fast_path: 0`, and what the device route is held
to bit for bit), and `<t>_band_profile.json`.

The profile of a component f [H, W] at the areas a_1 < .. < a_n and L levels is, in this order,
    value(phi_{a_n}(q)), .., value(phi_{a_1}(q)), f, value(gamma_{a_1}(q)), .., value(gamma_{a_n}(q))
with, per component (every value read is canonicalised once as x + 0.0f, so -0 becomes +0):
    lo = min f, hi = max f                                                                                  (exact)
    q = min(L - 1, floor((((double)f - (double)lo) * (double)L) / ((double)hi - (double)lo)))               (q = 0 where hi == lo)
    gamma_a(q)(x) = the largest t in 0..q(x) such that the 4-connected component of {q >= t} that holds x has at least a pixels
                  = the number of levels t in 1..q(x) whose component qualifies (the sets are nested; level 0 always counts)
    phi_a(q)      = (L - 1) - gamma_a((L - 1) - q)
    value(c)      = (float)((double)lo + ((double)c * ((double)hi - (double)lo)) / (double)L)
A subtract, a multiply and a divide; a multiply, a divide and an add: no multiply is followed by an add, nothing can be
contracted, and from q on everything is integer."""
import json

import numpy as np

from utils.morphology import canonical, check_components, check_scores

KINDS = ('none', 'morph', 'area')
AREAS_MAX, LEVELS_MAX, AREA_LIMIT = 8, 256, 1 << 31          # DMF_ATTR_NMAX, DMF_ATTR_LEVELS_MAX (include/dmf.h); areas are int32
DEFAULT_COMPONENTS, DEFAULT_AREAS, DEFAULT_LEVELS = 4, (25, 100, 400), 256


def _whole(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def kind_of(cfg):
    """-> 'none', 'morph' or 'area' from the optional top-level key `band_profile`; anything else is refused by name."""
    kind = cfg.get('band_profile', 'none')
    kind = 'none' if kind is None or kind is False or kind == 0 else str(kind).lower()
    if kind not in KINDS:
        raise ValueError('band_profile %r is not one of %s' % (cfg.get('band_profile'), ' / '.join(KINDS)))
    return kind


def check_areas(areas):
    """-> the areas as a tuple of ints; anything but 1..8 strictly increasing whole numbers in 1..2^31 - 1 is refused by name."""
    if isinstance(areas, (str, bytes)) or not hasattr(areas, '__len__') or not 1 <= len(areas) <= AREAS_MAX:
        raise ValueError('band_profile_areas %r is not a list of 1..%d whole numbers' % (areas, AREAS_MAX))
    if not all(_whole(a) and 1 <= a < AREA_LIMIT for a in areas):
        raise ValueError('band_profile_areas %r: every area is a whole number >= 1 and < 2^31' % (list(areas),))
    if any(b <= a for a, b in zip(areas[:-1], areas[1:])):
        raise ValueError('band_profile_areas %r is not strictly increasing' % (list(areas),))
    return tuple(int(a) for a in areas)


def check_levels(L):
    if not _whole(L) or not 2 <= L <= LEVELS_MAX:
        raise ValueError('band_profile_levels %r is not a whole number in 2..%d' % (L, LEVELS_MAX))
    return int(L)


def profile_keys(cfg):
    """-> None (the kind is not area), or dict(kind='area', components, areas, levels) from the optional top-level keys
         band_profile none / morph / area (default none)     band_profile_components 1..band_reduce_bands (default 4)
         band_profile_areas 1..8 strictly increasing whole numbers >= 1 and < 2^31 (default [25, 100, 400])
         band_profile_levels 2..256 (default 256)
    which stand beside `band_reduce: pca`; with `band_reduce: none` the kind is refused by name."""
    if kind_of(cfg) != 'area':
        return None
    if cfg.get('band_reduce', 'none') in (None, False, 0, 'none'):
        raise ValueError('band_profile: area profiles the components of band_reduce: pca, and band_reduce is none')
    P = cfg.get('band_profile_components', DEFAULT_COMPONENTS)
    check_components(P, cfg.get('band_reduce_bands', 32))
    return dict(kind='area', components=int(P), areas=check_areas(cfg.get('band_profile_areas', list(DEFAULT_AREAS))),
                levels=check_levels(cfg.get('band_profile_levels', DEFAULT_LEVELS)))


def band_count(K, P, n):
    return K + 2 * n * P


def band_names(K, P, areas):
    """The band order of the profile as names: checkpoints depend on it."""
    names = []
    for p in range(P):
        names += ['pc%d_aclose_a%d' % (p + 1, a) for a in reversed(areas)] + ['pc%d' % (p + 1)]
        names += ['pc%d_aopen_a%d' % (p + 1, a) for a in areas]
    return names + ['pc%d' % (p + 1) for p in range(P, K)]


def plane_range(f):
    """(lo, hi) of the canonicalised plane, float32."""
    return np.float32(f.min()), np.float32(f.max())


def quantise(f, lo, hi, L):
    """q [H, W] int32 of the canonicalised plane f: the definition's step 2, in double, operation by operation."""
    if not hi > lo:
        return np.zeros(f.shape, dtype=np.int32)
    d = f.astype(np.float64) - np.float64(lo)
    m = d * np.float64(L)
    v = m / (np.float64(hi) - np.float64(lo))
    return np.minimum(L - 1, np.floor(v).astype(np.int64)).astype(np.int32)


def value(c, lo, hi, L):
    """Level c (an integer array) back to float32: multiply, divide, add, in double."""
    m = np.asarray(c, dtype=np.float64) * (np.float64(hi) - np.float64(lo))
    v = m / np.float64(L)
    return (np.float64(lo) + v).astype(np.float32)


_FOUR = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], dtype=bool)


def area_open_counts(q, areas, L):
    """-> count [n, H, W] int32: per area the number of levels t in 1..q(x) at which the 4-connected component of {q >= t} that
    holds x has at least that many pixels.  Threshold decomposition: one scipy.ndimage.label and one np.bincount per level."""
    from scipy import ndimage
    count = np.zeros((len(areas),) + q.shape, dtype=np.int32)
    for t in range(1, min(int(q.max()), L - 1) + 1):
        lab, _ = ndimage.label(q >= t, structure=_FOUR)
        size = np.bincount(lab.ravel())
        size[0] = 0                                                           # the background: below the level
        big = size[lab]
        for i, a in enumerate(areas):
            count[i] += big >= a
    return count


def area_open(q, area, L):
    return area_open_counts(q, (area,), L)[0]


def area_close(q, area, L):
    return (L - 1) - area_open((L - 1) - q, area, L)


def profile_host(scores, P, areas, L=DEFAULT_LEVELS):
    """`band_profile: area` on the host -> (profile [H, W, K + 2 n P] float32, info): the definition at the head of this file,
    component by component."""
    areas, L = check_areas(areas), check_levels(L)
    scores = check_scores(scores, P)
    H, W, K = scores.shape
    n = len(areas)
    out = np.empty((H, W, band_count(K, P, n)), dtype=np.float32)
    ranges = []
    for p in range(P):
        f = canonical(scores[:, :, p])
        lo, hi = plane_range(f)
        q = quantise(f, lo, hi, L)
        opened = area_open_counts(q, areas, L)
        closed = (L - 1) - area_open_counts((L - 1) - q, areas, L)
        base = p * (2 * n + 1)
        out[:, :, base + n] = f
        for i in range(n):
            out[:, :, base + n - 1 - i] = value(closed[i], lo, hi, L)
            out[:, :, base + n + 1 + i] = value(opened[i], lo, hi, L)
        ranges.append([float(lo), float(hi)])
    out[:, :, P * (2 * n + 1):] = scores[:, :, P:]
    return out, make_info(K, P, areas, L, ranges, 'host')


def make_info(K, P, areas, L, ranges, route):
    """What `<t>_band_profile.json` records for the kind area.  ranges: per profiled component [lo, hi]."""
    return dict(kind='area', components=int(P), areas=[int(a) for a in areas], levels=int(L), connectivity=4,
                range=[[float(lo), float(hi)] for lo, hi in ranges], bands=band_count(K, P, len(areas)), order=band_names(K, P, areas),
                route=route)


def save_info(path, info):
    with open(path, 'w') as f:
        json.dump(info, f, indent=1)
