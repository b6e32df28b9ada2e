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
contracted, and from q on everything is integer.

Several attributes: `band_profile_diagonals` and `band_profile_stds` beside the areas.  The threshold list is
T = areas ++ diagonals ++ stds (1 <= n <= 8) and takes the place of the areas in the order above.  For a threshold tau of
attribute A, gamma_{A,tau}(q)(x) = the number of levels t in 1..q(x) at which the 4-connected component S of {q >= t} that holds
x satisfies, in unsigned 64-bit without a division (csrc/dmf_attr_criteria.h),
    area      |S| >= tau
    diagonal  w^2 + h^2 >= tau^2          w, h: the side lengths in pixels of S's bounding box
    std       |S| sum q^2 - (sum q)^2 >= tau^2 |S|^2          the sums over the pixels of S, of the plane being opened
Area and diagonal grow with S, so the count is the largest qualifying level (the max rule); the standard deviation does not,
and the count is the subtractive rule of attribute profiles.  With both new lists empty every line runs as it did."""
import json

import numpy as np

from utils.morphology import canonical, check_components, check_scores

KINDS = ('none', 'morph', 'area')
AREAS_MAX, LEVELS_MAX, AREA_LIMIT = 8, 256, 1 << 31          # DMF_ATTR_NMAX, DMF_ATTR_LEVELS_MAX (include/dmf.h); areas are int32
DEFAULT_COMPONENTS, DEFAULT_AREAS, DEFAULT_LEVELS = 4, (25, 100, 400), 256
EXTRA_MAX, STD_PIXELS_MAX = AREAS_MAX - 1, 1 << 22          # a profile keeps an area; DMF_ATTR_STD_PIXELS_MAX (include/dmf.h)
RULE = 'qualifying levels (max rule for area and diagonal, subtractive for std)'


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


def _check_extra(key, values, limit, limit_text):
    """0..7 strictly increasing whole numbers >= 1 and < limit; None is the empty list."""
    if values is None:
        return ()
    if isinstance(values, (str, bytes)) or not hasattr(values, '__len__') or len(values) > EXTRA_MAX:
        raise ValueError('%s %r is not a list of 0..%d whole numbers' % (key, values, EXTRA_MAX))
    if not all(_whole(v) and 1 <= v < limit for v in values):
        raise ValueError('%s %r: every value is a whole number >= 1 and %s' % (key, list(values), limit_text))
    if any(b <= a for a, b in zip(values[:-1], values[1:])):
        raise ValueError('%s %r is not strictly increasing' % (key, list(values)))
    return tuple(int(v) for v in values)


def check_diagonals(diagonals):
    """-> the diagonals as a tuple of ints: 0..7 strictly increasing whole numbers in 1..2^31 - 1, in pixels."""
    return _check_extra('band_profile_diagonals', diagonals, AREA_LIMIT, '< 2^31')


def check_stds(stds, L):
    """-> the stds as a tuple of ints: 0..7 strictly increasing whole numbers in 1..L - 1, in quantisation-level units."""
    return _check_extra('band_profile_stds', stds, L, '<= band_profile_levels - 1 = %d' % (L - 1))


def check_thresholds(areas, diagonals, stds, L):
    """-> (areas, diagonals, stds) as tuples; each list by its own rule, and together at most 8 thresholds."""
    areas, L = check_areas(areas), check_levels(L)
    diagonals, stds = check_diagonals(diagonals), check_stds(stds, L)
    if len(areas) + len(diagonals) + len(stds) > AREAS_MAX:
        raise ValueError('band_profile_areas + band_profile_diagonals + band_profile_stds: %d + %d + %d thresholds are more than %d'
                         % (len(areas), len(diagonals), len(stds), AREAS_MAX))
    return areas, diagonals, stds


def check_std_extent(H, W, stds):
    if len(stds) and H * W > STD_PIXELS_MAX:
        raise ValueError('band_profile_stds: %d x %d pixels are more than 2^22 (the 64-bit products of the criterion)' % (H, W))


def check_levels(L):
    if not _whole(L) or not 2 <= L <= LEVELS_MAX:
        raise ValueError('band_profile_levels %r is not a whole number in 2..%d' % (L, LEVELS_MAX))
    return int(L)


def profile_keys(cfg):
    """-> None (the kind is not area), or dict(kind='area', components, areas, levels) from the optional top-level keys
         band_profile none / morph / area (default none)     band_profile_components 1..band_reduce_bands (default 4)
         band_profile_areas 1..8 strictly increasing whole numbers >= 1 and < 2^31 (default [25, 100, 400])
         band_profile_levels 2..256 (default 256)
    which stand beside `band_reduce: pca`; with `band_reduce: none` the kind is refused by name.
         band_profile_diagonals / band_profile_stds 0..7 strictly increasing whole numbers each (default: none);
         the dict carries `diagonals` / `stds` only where one of them is in use; with another kind they are refused by name."""
    extra = [k for k in ('band_profile_diagonals', 'band_profile_stds') if cfg.get(k) is not None and not _empty(cfg.get(k))]
    if kind_of(cfg) != 'area':
        if extra:
            raise ValueError('%s needs band_profile: area, and band_profile is %s' % (extra[0], kind_of(cfg)))
        return None
    if cfg.get('band_reduce', 'none') in (None, False, 0, 'none'):
        raise ValueError('band_profile: area profiles the components of band_reduce: pca, and band_reduce is none')
    P = cfg.get('band_profile_components', DEFAULT_COMPONENTS)
    check_components(P, cfg.get('band_reduce_bands', 32))
    keys = dict(kind='area', components=int(P), areas=check_areas(cfg.get('band_profile_areas', list(DEFAULT_AREAS))),
                levels=check_levels(cfg.get('band_profile_levels', DEFAULT_LEVELS)))
    if extra:
        _, keys['diagonals'], keys['stds'] = check_thresholds(keys['areas'], cfg.get('band_profile_diagonals'), cfg.get('band_profile_stds'),
                                                              keys['levels'])
    return keys


def _empty(v):
    return hasattr(v, '__len__') and not isinstance(v, (str, bytes)) and len(v) == 0


def band_count(K, P, n):
    return K + 2 * n * P


def band_names(K, P, areas, diagonals=(), stds=()):
    """The band order of the profile as names: checkpoints depend on it.  a / d / s: area, diagonal, std."""
    tags = ['a%d' % a for a in areas] + ['d%d' % d for d in diagonals] + ['s%d' % s for s in stds]
    names = []
    for p in range(P):
        names += ['pc%d_aclose_%s' % (p + 1, t) for t in reversed(tags)] + ['pc%d' % (p + 1)]
        names += ['pc%d_aopen_%s' % (p + 1, t) for t in tags]
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


def _crit_area(size, tau):
    return size >= np.uint64(tau)


def _crit_diagonal(w, h, tau):
    return w * w + h * h >= np.uint64(tau * tau)


def _crit_std(size, sum_q, sum_q2, tau):
    return size * sum_q2 - sum_q * sum_q >= np.uint64(tau * tau) * size * size


def open_counts(q, areas, diagonals, stds, L):
    """-> count [n, H, W] int32 for the thresholds areas ++ diagonals ++ stds: per threshold the number of levels t in 1..q(x) at
    which the component of {q >= t} that holds x meets the criterion.  Per level one scipy.ndimage.label, the sizes by np.bincount,
    the boxes by scipy.ndimage.find_objects, the sums of q and q^2 by np.bincount with float64 weights (exact: they stay below
    2^53), and the criteria in numpy's unsigned 64-bit in the form csrc/dmf_attr_criteria.h states.  With no diagonal and no std
    it is area_open_counts."""
    if not len(diagonals) and not len(stds):
        return area_open_counts(q, areas, L)
    from scipy import ndimage
    n = len(areas) + len(diagonals) + len(stds)
    count = np.zeros((n,) + q.shape, dtype=np.int32)
    flat = q.ravel().astype(np.float64)
    for t in range(1, min(int(q.max()), L - 1) + 1):
        lab, found = ndimage.label(q >= t, structure=_FOUR)
        size = np.bincount(lab.ravel(), minlength=found + 1).astype(np.uint64)
        ok = []                                                               # per threshold: does label k qualify (label 0: never)
        for a in areas:
            ok.append(_crit_area(size, a))
        if len(diagonals):
            w, h = np.zeros(found + 1, dtype=np.uint64), np.zeros(found + 1, dtype=np.uint64)
            for k, box in enumerate(ndimage.find_objects(lab), start=1):
                h[k], w[k] = box[0].stop - box[0].start, box[1].stop - box[1].start
            for d in diagonals:
                ok.append(_crit_diagonal(w, h, d))
        if len(stds):
            sum_q = np.bincount(lab.ravel(), weights=flat, minlength=found + 1).astype(np.uint64)
            sum_q2 = np.bincount(lab.ravel(), weights=flat * flat, minlength=found + 1).astype(np.uint64)
            for s in stds:
                ok.append(_crit_std(size, sum_q, sum_q2, s))
        for i, good in enumerate(ok):
            good[0] = False                                                   # the background: below the level
            count[i] += good[lab]
    return count


def profile_host(scores, P, areas, L=DEFAULT_LEVELS, diagonals=(), stds=()):
    """`band_profile: area` on the host -> (profile [H, W, K + 2 n P] float32, info): the definition at the head of this file,
    component by component.  diagonals / stds: further thresholds after the areas; with both empty every line runs
    as it did."""
    if len(diagonals) or len(stds):
        return _profile_host_multi(scores, P, areas, L, diagonals, stds)
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


def _profile_host_multi(scores, P, areas, L, diagonals, stds):
    areas, diagonals, stds = check_thresholds(areas, diagonals, stds, L)
    scores = check_scores(scores, P)
    H, W, K = scores.shape
    check_std_extent(H, W, stds)
    n = len(areas) + len(diagonals) + len(stds)
    out = np.empty((H, W, band_count(K, P, n)), dtype=np.float32)
    ranges = []
    for p in range(P):
        f = canonical(scores[:, :, p])
        lo, hi = plane_range(f)
        q = quantise(f, lo, hi, L)
        opened = open_counts(q, areas, diagonals, stds, L)
        closed = (L - 1) - open_counts((L - 1) - q, areas, diagonals, stds, L)
        base = p * (2 * n + 1)
        out[:, :, base + n] = f
        for i in range(n):
            out[:, :, base + n - 1 - i] = value(closed[i], lo, hi, L)
            out[:, :, base + n + 1 + i] = value(opened[i], lo, hi, L)
        ranges.append([float(lo), float(hi)])
    out[:, :, P * (2 * n + 1):] = scores[:, :, P:]
    return out, make_info(K, P, areas, L, ranges, 'host', diagonals, stds)


def make_info(K, P, areas, L, ranges, route, diagonals=(), stds=()):
    """What `<t>_band_profile.json` records for the kind area.  ranges: per profiled component [lo, hi].  With a diagonal or a std
    in use it gains `diagonals`, `stds` and `rule`, and `bands` / `order` count and name every threshold."""
    if not len(diagonals) and not len(stds):
        return dict(kind='area', components=int(P), areas=[int(a) for a in areas], levels=int(L), connectivity=4,
                    range=[[float(lo), float(hi)] for lo, hi in ranges], bands=band_count(K, P, len(areas)), order=band_names(K, P, areas),
                    route=route)
    n = len(areas) + len(diagonals) + len(stds)
    return dict(kind='area', components=int(P), areas=[int(a) for a in areas], diagonals=[int(d) for d in diagonals],
                stds=[int(s) for s in stds], rule=RULE, levels=int(L), connectivity=4, range=[[float(lo), float(hi)] for lo, hi in ranges],
                bands=band_count(K, P, n), order=band_names(K, P, areas, diagonals, stds), route=route)


def save_info(path, info):
    with open(path, 'w') as f:
        json.dump(info, f, indent=1)
