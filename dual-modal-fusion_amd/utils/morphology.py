"""utils.morphology — the host side of `band_profile: morph`: the config keys, the band order, the definition
of the extended morphological profile in numpy (the drop-in route of `fast_path: 0`, and what the device route is held to bit for
bit), and `<t>_band_profile.json`.

The profile of a component f [H, W] at the radii r_1 < .. < r_n is, in this order,
    phi_{r_n}(f), .., phi_{r_1}(f), f, gamma_{r_1}(f), .., gamma_{r_n}(f)
with gamma_r(f) = R^delta(eps_r(f) | f) the opening and phi_r(f) = R^eps(delta_r(f) | f) the closing by reconstruction; eps_r / delta_r
are the min / max over the (2 r + 1) x (2 r + 1) square clipped to the image, R^delta(m | f) is the limit of j <- min(delta_1(j), f) from
j = m and R^eps its dual.  Every value read is canonicalised once as x + 0.0f (-0 becomes +0), so min / max of equal values has one
answer; everything else is min / max of float32 values: no rounding, no order."""
import json

import numpy as np

KINDS = ('none', 'morph', 'area')             # area: utils/attribute.py
RADIUS_MAX, RADII_MAX = 32, 8                # DMF_MORPH_RMAX, DMF_MORPH_NMAX (include/dmf.h)
DEFAULT_COMPONENTS, DEFAULT_RADII = 4, (2, 4, 6)


def _whole(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def check_radii(radii):
    """-> the radii as a tuple of ints; anything but 1..8 strictly increasing whole numbers in 1..32 is refused by name."""
    if isinstance(radii, (str, bytes)) or not hasattr(radii, '__len__') or not 1 <= len(radii) <= RADII_MAX:
        raise ValueError('band_profile_radii %r is not a list of 1..%d whole numbers' % (radii, RADII_MAX))
    if not all(_whole(r) and 1 <= r <= RADIUS_MAX for r in radii):
        raise ValueError('band_profile_radii %r: every radius is a whole number in 1..%d' % (list(radii), RADIUS_MAX))
    if any(b <= a for a, b in zip(radii[:-1], radii[1:])):
        raise ValueError('band_profile_radii %r is not strictly increasing' % (list(radii),))
    return tuple(int(r) for r in radii)


def check_components(P, K):
    if not _whole(P) or P < 1:
        raise ValueError('band_profile_components %r is not a whole number >= 1' % (P,))
    if P > K:
        raise ValueError('band_profile_components: %d exceeds the %d components of band_reduce_bands' % (P, K))


def profile_keys(cfg):
    """-> None (the kind is none, or area: DESIGN.md §27), or dict(components, radii) from the optional top-level keys
         band_profile none / morph / area (default none)    band_profile_components 1..band_reduce_bands (default 4)
         band_profile_radii 1..8 strictly increasing whole numbers in 1..32 (default [2, 4, 6])
    which stand beside `band_reduce: pca`; with `band_reduce: none` anything but none is refused."""
    kind = cfg.get('band_profile', 'none')
    kind = 'none' if kind is None or kind is False or kind == 0 else str(kind).lower()
    if kind not in KINDS:
        raise ValueError('band_profile %r is not one of %s' % (cfg.get('band_profile'), ' / '.join(KINDS)))
    if kind != 'morph':                          # none; area: utils.attribute.profile_keys holds its keys
        return None
    if cfg.get('band_reduce', 'none') in (None, False, 0, 'none'):
        raise ValueError('band_profile: morph profiles the components of band_reduce: pca, and band_reduce is none')
    P = cfg.get('band_profile_components', DEFAULT_COMPONENTS)
    check_components(P, cfg.get('band_reduce_bands', 32))
    return dict(components=int(P), radii=check_radii(cfg.get('band_profile_radii', list(DEFAULT_RADII))))


def band_count(K, P, n):
    return K + 2 * n * P


def band_names(K, P, radii):
    """The band order of the profile as names: checkpoints depend on it."""
    names = []
    for p in range(P):
        names += ['pc%d_close_r%d' % (p + 1, r) for r in reversed(radii)] + ['pc%d' % (p + 1)]
        names += ['pc%d_open_r%d' % (p + 1, r) for r in radii]
    return names + ['pc%d' % (p + 1) for p in range(P, K)]


def canonical(x):
    """float32 with every -0 turned into +0."""
    return np.asarray(x, dtype=np.float32) + np.float32(0.0)


def _window(f, r, pick, pad):
    """min (pick = np.minimum, pad = +inf) or max over the (2 r + 1) x (2 r + 1) square clipped to the image: rows, then columns."""
    H, W = f.shape
    g = np.full((H, W + 2 * r), pad, dtype=np.float32)
    g[:, r:r + W] = f
    out = g[:, 0:W].copy()
    for d in range(1, 2 * r + 1):
        out = pick(out, g[:, d:d + W])
    g = np.full((H + 2 * r, W), pad, dtype=np.float32)
    g[r:r + H] = out
    out = g[0:H].copy()
    for d in range(1, 2 * r + 1):
        out = pick(out, g[d:d + H])
    return out


def erode(f, r):
    return _window(f, r, np.minimum, np.float32(np.inf))


def dilate(f, r):
    return _window(f, r, np.maximum, np.float32(-np.inf))


def reconstruct_by_dilation(marker, mask):
    """-> (R^delta(marker | mask), the elementary steps taken): j <- min(delta_1(j), mask) until nothing changes."""
    j, steps = marker, 0
    while True:
        nxt = np.minimum(dilate(j, 1), mask)
        steps += 1
        if np.array_equal(nxt, j):
            return j, steps
        j = nxt


def reconstruct_by_erosion(marker, mask):
    """The dual: j <- max(eps_1(j), mask) until nothing changes."""
    j, steps = marker, 0
    while True:
        nxt = np.maximum(erode(j, 1), mask)
        steps += 1
        if np.array_equal(nxt, j):
            return j, steps
        j = nxt


def opening_by_reconstruction(f, r):
    return reconstruct_by_dilation(erode(f, r), f)


def closing_by_reconstruction(f, r):
    return reconstruct_by_erosion(dilate(f, r), f)


def check_scores(scores, P):
    scores = np.asarray(scores)
    if scores.ndim != 3 or scores.dtype != np.float32:
        raise ValueError('band_profile wants the float32 scores [H, W, K] of band_reduce')
    check_components(P, scores.shape[2])
    if not np.isfinite(scores).all():
        raise ValueError('band_profile: the scores hold a value that is not finite')
    return scores


def profile_host(scores, P, radii):
    """`band_profile: morph` on the host -> (profile [H, W, K + 2 n P] float32, info): the definition at the head of this file,
    component by component, as repeated elementary steps."""
    radii = check_radii(radii)
    scores = check_scores(scores, P)
    H, W, K = scores.shape
    n = len(radii)
    out = np.empty((H, W, band_count(K, P, n)), dtype=np.float32)
    steps = []
    for p in range(P):
        f = canonical(scores[:, :, p])
        base = p * (2 * n + 1)
        out[:, :, base + n] = f
        for i, r in enumerate(radii):
            out[:, :, base + n - 1 - i], a = closing_by_reconstruction(f, r)
            out[:, :, base + n + 1 + i], b = opening_by_reconstruction(f, r)
            steps += [a, b]
    out[:, :, P * (2 * n + 1):] = scores[:, :, P:]
    return out, make_info(K, P, radii, 'host', [max(steps)])


def make_info(K, P, radii, route, rounds):
    """What `<t>_band_profile.json` records.  rounds: the reconstruction rounds of each launch batch (the device route), or the
    one count of elementary steps of the slowest plane (the host route)."""
    return dict(components=int(P), radii=[int(r) for r in radii], bands=band_count(K, P, len(radii)), order=band_names(K, P, radii),
                route=route, rounds=[int(r) for r in rounds])


def save_info(path, info):
    with open(path, 'w') as f:
        json.dump(info, f, indent=1)
