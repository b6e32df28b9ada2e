"""utils.spatial — the host side of `test.spatial` and `color.spatial`: the config keys, the report block, and
for `fast_path: 0` the arithmetic of dmf_spatial_affinity / dmf_prob_scatter / dmf_spatial_filter (include/dmf.h) in numpy
float64.  Nothing here touches the GPU library.

The filter smooths the class probabilities of a pixel over its (2r + 1)^2 window; a neighbour y of x weighs
exp(-(|x - y|^2 / (2 sigma_s^2) + mean_c (a_c(x) - a_c(y))^2 / (2 sigma_r^2))) with a the normalised primary scene, counts only
where it was classified (mask), and the sums are normalised per pixel.  Offset index k = (di + r)(2r + 1) + (dj + r)."""
import math

import numpy as np

KINDS = ('none', 'bilateral')


def spatial_keys(cfg):
    """-> dict(kind, radius, sigma_s, sigma_r, iterations, color) from the optional keys
         test.spatial none / bilateral (default none)     test.spatial_radius 1..3 (default 2)
         test.spatial_sigma_s > 0 (default 2.0)           test.spatial_sigma_r > 0 (default 0.1)
         test.spatial_iterations >= 1 (default 1)         color.spatial 0 / 1 (default 0)
    `kind` is None or 'bilateral'.  Neutral values change nothing."""
    test, color = cfg.get('test') or {}, cfg.get('color') or {}
    kind = test.get('spatial', 'none')
    kind = 'none' if kind is None or kind is False or kind == 0 else str(kind).lower()
    if kind not in KINDS:
        raise ValueError('test.spatial %r is not one of %s' % (test.get('spatial'), ' / '.join(KINDS)))
    col = color.get('spatial', 0) or 0
    if col not in (0, 1, True, False):
        raise ValueError('color.spatial is 0 or 1')
    radius, its = test.get('spatial_radius', 2), test.get('spatial_iterations', 1)
    if isinstance(radius, bool) or not isinstance(radius, int) or not 1 <= radius <= 3:
        raise ValueError('test.spatial_radius %r is not 1, 2 or 3' % (radius,))
    if isinstance(its, bool) or not isinstance(its, int) or its < 1:
        raise ValueError('test.spatial_iterations %r is not a whole number >= 1' % (its,))
    sig = []
    for name, default in (('spatial_sigma_s', 2.0), ('spatial_sigma_r', 0.1)):
        v = test.get(name, default)
        try:
            f = float(v)
        except (TypeError, ValueError):
            f = float('nan')
        if isinstance(v, bool) or not (math.isfinite(f) and f > 0):
            raise ValueError('test.%s %r is not a number > 0' % (name, v))
        sig.append(f)
    if col and kind == 'none':
        raise ValueError('color.spatial: 1 draws the map that test.spatial: bilateral regularises; test.spatial is none')
    return dict(kind=None if kind == 'none' else kind, radius=radius, sigma_s=sig[0], sigma_r=sig[1], iterations=its, color=bool(col))


def keys_in_use(keys):
    """The names of the keys that are not neutral, for a refusal."""
    return [name for name, used in (('test.spatial', keys['kind'] is not None), ('color.spatial', keys['color'])) if used]


def offsets(r):
    return [(di, dj) for di in range(-r, r + 1) for dj in range(-r, r + 1)]


def _neighbour(a, di, dj):
    """(a shifted so that cell (i, j) holds a[i + di, j + dj], zero where that is outside; [H, W] bool: inside)."""
    H, W = a.shape[:2]
    pad = max(abs(di), abs(dj))
    big = np.zeros((H + 2 * pad, W + 2 * pad) + a.shape[2:], dtype=a.dtype)
    big[pad:pad + H, pad:pad + W] = a
    ii, jj = np.arange(H)[:, None] + di, np.arange(W)[None, :] + dj
    return big[pad + di:pad + di + H, pad + dj:pad + dj + W], (ii >= 0) & (ii < H) & (jj >= 0) & (jj < W)


def affinity(scene, H, W, radius, sigma_s, sigma_r):
    """aff [H, W, n] float64 of the leading [H, W] pixels of the padded primary scene [>= H, >= W, C]; cs and cr are rounded to
    fp32 as the kernel's arguments are."""
    a = np.asarray(scene)[:H, :W].astype(np.float64)
    cs, cr = float(np.float32(1.0 / (2.0 * sigma_s ** 2))), float(np.float32(1.0 / (2.0 * sigma_r ** 2)))
    aff = np.zeros((H, W, (2 * radius + 1) ** 2))
    for k, (di, dj) in enumerate(offsets(radius)):
        b, inside = _neighbour(a, di, dj)
        d2 = np.square(a - b).sum(2) / a.shape[2]
        aff[:, :, k] = np.where(inside, np.exp(-((di * di + dj * dj) * cs + d2 * cr)), 0.0)
    return aff


def probabilities(logits, beta=1.0):
    """softmax((l - max l) beta) of logits [n, K] in float64, beta the fp32 value the kernels read."""
    l = np.asarray(logits, dtype=np.float64)
    e = np.exp((l - l.max(1, keepdims=True)) * float(np.float32(beta)))
    return e / e.sum(1, keepdims=True)


def filter_once(prob, mask, aff, radius):
    """One iteration -> (prob' [H, W, K] float64, label map [H, W] int32: the first maximal index where mask is 1, 0 elsewhere)."""
    live = np.asarray(mask) != 0
    p = np.where(live[:, :, None], np.asarray(prob, dtype=np.float64), 0.0)
    num, den = np.zeros_like(p), np.zeros(live.shape)
    for k, (di, dj) in enumerate(offsets(radius)):
        w = aff[:, :, k] * _neighbour(live.astype(np.float64), di, dj)[0]
        num += w[:, :, None] * _neighbour(p, di, dj)[0]
        den += w
    out = np.where(live[:, :, None], num / np.where(live, den, 1.0)[:, :, None], 0.0)
    return out, np.where(live, out.argmax(2), 0).astype(np.int32)


def regularise(prob, mask, aff, radius, iterations=1):
    out, labels = prob, None
    for _ in range(iterations):
        out, labels = filter_once(out, mask, aff, radius)
    return out, labels


def report(keys, matrix_before, matrix_after, changed):
    """The block of `<t>_spatial.json`: the parameters, the regularised confusion matrix (rows = prediction), OA / AA / kappa
    before and after (indicators.kappa) and the number of test pixels whose class changed."""
    from indicators.kappa import aa_oa_quiet

    def block(m):
        aa, oa, k = aa_oa_quiet(np.asarray(m, dtype=np.float64))
        return dict(OA=oa, AA=aa, kappa=k)
    return dict(kind=keys['kind'], radius=keys['radius'], sigma_s=keys['sigma_s'], sigma_r=keys['sigma_r'],
                iterations=keys['iterations'], n=int(np.asarray(matrix_after).sum()),
                matrix=np.asarray(matrix_after, dtype=np.int64).tolist(), before=block(matrix_before), after=block(matrix_after),
                changed=int(changed))
