"""Float64 numpy statement of the spatial regularisation (include/dmf.h): the bilateral affinities of a scene,
the probability scatter and one iteration of the filter.  The inputs are taken as the kernels get them (an fp32 or fp16 scene,
fp32 logits, cs / cr / beta as fp32 values); everything after that is float64.  A plain module: no GPU, nothing of the library."""
import numpy as np


def window(r):
    """[(di, dj)] in the order of the offset index k = (di + r)(2r + 1) + (dj + r)."""
    return [(di, dj) for di in range(-r, r + 1) for dj in range(-r, r + 1)]


def coefficients(sigma_s, sigma_r):
    """(cs, cr) = (1 / (2 sigma_s^2), 1 / (2 sigma_r^2)) as the fp32 values the kernel is passed."""
    return float(np.float32(1.0 / (2.0 * sigma_s ** 2))), float(np.float32(1.0 / (2.0 * sigma_r ** 2)))


def _shifted(a, di, dj, fill=0.0):
    """b[i, j] = a[i + di, j + dj] where that lies inside a, `fill` elsewhere (a [H, W, ...]); and the inside mask [H, W]."""
    H, W = a.shape[:2]
    b = np.full_like(a, fill)
    inside = np.zeros((H, W), dtype=bool)
    i0, i1, j0, j1 = max(0, -di), min(H, H - di), max(0, -dj), min(W, W - dj)
    if i0 < i1 and j0 < j1:
        b[i0:i1, j0:j1] = a[i0 + di:i1 + di, j0 + dj:j1 + dj]
        inside[i0:i1, j0:j1] = True
    return b, inside


def affinity(scene, H, W, r, sigma_s, sigma_r):
    """scene [>= H, >= W, C] (float32 or float16) -> (aff [H, W, n], E [H, W, n]) in float64: E is the exponent's argument
    (di^2 + dj^2) cs + d2 cr, aff = exp(-E) inside the scene and 0 for a neighbour outside it (E = 0 there)."""
    a = np.asarray(scene)[:H, :W].astype(np.float64)
    C = a.shape[2]
    cs, cr = coefficients(sigma_s, sigma_r)
    n = (2 * r + 1) ** 2
    aff, E = np.zeros((H, W, n)), np.zeros((H, W, n))
    for k, (di, dj) in enumerate(window(r)):
        b, inside = _shifted(a, di, dj)
        d2 = ((a - b) ** 2).sum(2) / C
        e = (di * di + dj * dj) * cs + d2 * cr
        E[:, :, k] = np.where(inside, e, 0.0)
        aff[:, :, k] = np.where(inside, np.exp(-e), 0.0)
    return aff, E


def softmax(logits, beta=1.0):
    """logits [B, K] float32, beta an fp32 value -> p [B, K] float64, with dmf_softmax_stats's t = (l - m) beta."""
    l = np.asarray(logits, dtype=np.float32).astype(np.float64)
    e = np.exp((l - l.max(1, keepdims=True)) * float(np.float32(beta)))
    return e / e.sum(1, keepdims=True)


def scatter(logits, xy, H, W, beta=1.0):
    """-> (prob [H, W, K] float64, mask [H, W] uint8): row i of softmax(logits) at pixel xy[i], zeros elsewhere."""
    xy = np.asarray(xy)
    prob = np.zeros((H, W, np.asarray(logits).shape[1]))
    mask = np.zeros((H, W), dtype=np.uint8)
    prob[xy[:, 0], xy[:, 1]] = softmax(logits, beta)
    mask[xy[:, 0], xy[:, 1]] = 1
    return prob, mask


def filter_once(prob, mask, aff, r):
    """One iteration: (out [H, W, K] float64, pred [H, W] int64 = the first maximal index of out).  A pixel with mask 0 has an
    all-zero row (and pred 0, which means nothing there)."""
    p = np.asarray(prob, dtype=np.float64)
    m = np.asarray(mask) != 0
    p = np.where(m[:, :, None], p, 0.0)                  # an unmasked neighbour counts for nothing, whatever its row holds
    num, den = np.zeros_like(p), np.zeros(m.shape)
    for k, (di, dj) in enumerate(window(r)):
        pk, _ = _shifted(p, di, dj)
        mk, _ = _shifted(m.astype(np.float64), di, dj)
        w = np.asarray(aff, dtype=np.float64)[:, :, k] * mk
        num += w[:, :, None] * pk
        den += w
    out = np.where(m[:, :, None], num / np.where(m, den, 1.0)[:, :, None], 0.0)
    return out, out.argmax(2)


def regularise(prob, mask, aff, r, iterations=1):
    out, pred = prob, None
    for _ in range(iterations):
        out, pred = filter_once(out, mask, aff, r)
    return out, pred


def top2_margin(out):
    """[H, W]: the largest minus the second largest entry of every row (K == 1: +inf)."""
    if out.shape[2] < 2:
        return np.full(out.shape[:2], np.inf)
    s = np.sort(out, axis=2)
    return s[:, :, -1] - s[:, :, -2]


def affinity_bound(aff, E, C):
    """The derived bound of the fp32 kernel against float64: |delta| <= aff (E (C + 4) + 4) 2^-24 — a C-term sum of non-negative
    fp32 terms, the divide, the two products (each relative 2^-24 on the exponent's argument E) and expf."""
    return aff * (E * (C + 4) + 4) * 2.0 ** -24


def filter_bound(out, n):
    """|delta| <= out (2 n + 4) 2^-24 where out >= 1e-30, 1e-30 below: two n-term sums of non-negative terms and the divide."""
    return np.where(out >= 1e-30, out * (2 * n + 4) * 2.0 ** -24, 1e-30)
