"""Float64 numpy statement of the superpixel voting (include/dmf.h): the SLIC grid, init, assign, update, the
iteration and the per-segment vote.  The inputs are taken as the kernels get them (an fp32 or fp16 scene, fp32 centres and
probabilities, cw as the fp32 value the kernel forms); everything after that is float64.  A plain module: no GPU, nothing of the
library, nothing of utils/segments.py."""
import numpy as np

SLOTS = [(u, v) for u in (-1, 0, 1) for v in (-1, 0, 1)]       # slot s = 3 (u + 1) + (v + 1)
U = 2.0 ** -24                                                   # the unit roundoff of fp32


def grid(H, W, S):
    """-> (gh, gw)."""
    return -(-H // S), -(-W // S)


def compact_weight(compactness, S):
    """cw = (compactness / S)^2 in double from the fp32 compactness, rounded to fp32."""
    return float(np.float32((float(np.float32(compactness)) / S) ** 2))


def candidates(H, W, S):
    """-> (cand [9, H, W] int64: the cluster of every pixel's slot, -1 where the cell lies outside the grid; valid [9, H, W])."""
    gh, gw = grid(H, W, S)
    gi, gj = np.arange(H)[:, None] // S, np.arange(W)[None, :] // S
    cand, valid = np.full((9, H, W), -1, dtype=np.int64), np.zeros((9, H, W), dtype=bool)
    for s, (u, v) in enumerate(SLOTS):
        ok = (gi + u >= 0) & (gi + u < gh) & (gj + v >= 0) & (gj + v < gw)
        valid[s] = ok
        cand[s] = np.where(ok, (gi + u) * gw + gj + v, -1)
    return cand, valid


def init(scene, H, W, S):
    """centres [Kc, C + 2] float64: cluster k at pixel (min(H - 1, gi S + S div 2), min(W - 1, gj S + S div 2))."""
    a = np.asarray(scene)[:H, :W].astype(np.float64)
    gh, gw = grid(H, W, S)
    ci = np.minimum(H - 1, np.arange(gh) * S + S // 2)
    cj = np.minimum(W - 1, np.arange(gw) * S + S // 2)
    ii, jj = np.meshgrid(ci, cj, indexing='ij')
    return np.concatenate([a[ii, jj].reshape(gh * gw, -1), ii.reshape(-1, 1).astype(np.float64), jj.reshape(-1, 1).astype(np.float64)], 1)


def distances(scene, H, W, S, compactness, centres):
    """-> (D [9, H, W] float64, +inf at a slot outside the grid; bound [9, H, W]: the derived fp32 error bound of that D).

    The bound.  d2 is a C-term fmaf chain of non-negative terms, each the square of one rounded difference (relative error of a
    term <= 3 u to first order), and one divide: |delta d2| <= d2 (C + 4) u.  The spatial part rounds di and dj (u each, so 2 u
    on a square), the two squares, their sum, the product with cw: <= 6 u relative; then one add.  Together
    |delta D| <= (d2 (C + 4) + cw sp 6 + D) u <= D (C + 8) u."""
    a = np.asarray(scene)[:H, :W].astype(np.float64)
    C = a.shape[2]
    cen = np.asarray(centres, dtype=np.float64)
    cw = compact_weight(compactness, S)
    cand, valid = candidates(H, W, S)
    ii, jj = np.arange(H)[:, None].astype(np.float64), np.arange(W)[None, :].astype(np.float64)
    D = np.full((9, H, W), np.inf)
    for s in range(9):
        k = np.where(valid[s], cand[s], 0)
        d2 = ((a - cen[k][:, :, :C]) ** 2).sum(2) / C
        sp = (ii - cen[k][:, :, C]) ** 2 + (jj - cen[k][:, :, C + 1]) ** 2
        D[s] = np.where(valid[s], d2 + cw * sp, np.inf)
    return D, np.where(np.isfinite(D), D, 0.0) * (C + 8) * U


def assign(scene, H, W, S, compactness, centres):
    """-> (seg [H, W] int64: the candidate of the smallest D, the first slot on equality; tie [H, W] bool: the float64 gap between
    the best and the second-best D is under the sum of their fp32 bounds, so an fp32 kernel may choose either)."""
    D, bound = distances(scene, H, W, S, compactness, centres)
    cand, _ = candidates(H, W, S)
    best = D.argmin(0)                                   # (numpy: the first on equality)
    seg = np.take_along_axis(cand, best[None], 0)[0]
    order = np.sort(D, axis=0)
    D2 = D.copy()
    np.put_along_axis(D2, best[None], np.inf, 0)
    second = D2.argmin(0)
    gap = order[1] - order[0]                            # (+inf with a single candidate)
    tol = np.take_along_axis(bound, best[None], 0)[0] + np.take_along_axis(bound, second[None], 0)[0]
    return seg, np.isfinite(gap) & (gap <= tol)


def members(seg, H, W, S):
    """[H, W] bool: seg is one of the pixel's candidates (anything else is a member of nothing)."""
    cand, valid = candidates(H, W, S)
    return (valid & (cand == np.asarray(seg)[None])).any(0)


def update(scene, H, W, S, seg, centres):
    """-> (centres' [Kc, C + 2] float64, counts [Kc] int64, absmean [Kc, C]: the mean of |a| over the members, for the bound).
    A cluster without a member keeps its row."""
    a = np.asarray(scene)[:H, :W].astype(np.float64)
    C = a.shape[2]
    gh, gw = grid(H, W, S)
    Kc = gh * gw
    seg = np.asarray(seg).astype(np.int64)
    m = members(seg, H, W, S)
    k = seg[m]
    counts = np.bincount(k, minlength=Kc)
    ii, jj = np.nonzero(m)
    rows = np.concatenate([a[m], ii[:, None].astype(np.float64), jj[:, None].astype(np.float64)], 1)
    sums, absum = np.zeros((Kc, C + 2)), np.zeros((Kc, C))
    np.add.at(sums, k, rows)
    np.add.at(absum, k, np.abs(a[m]))
    out = np.asarray(centres, dtype=np.float64).copy()
    live = counts > 0
    out[live] = sums[live] / counts[live][:, None]
    return out, counts, absum / np.maximum(counts, 1)[:, None]


def update_bound(absmean, centres, S):
    """|delta| of the kernel's centres against float64.  Spectrum: a cell partial is an fp32 chain over at most S^2 members
    (<= (S^2 - 1) u sum |a| to first order), the nine partials are added and divided in double, the mean is rounded once:
    <= (S^2 + 2) u mean|a| (the + 2: the last rounding, |mean| <= mean|a|, and the second-order terms, 2 / S^2 >= 1e-3 of the
    bound where they are 3e-5).  Position: exact integers, one double divide, one rounding: <= u |position| (+ 1e-30)."""
    C = absmean.shape[1]
    out = np.empty((absmean.shape[0], C + 2))
    out[:, :C] = absmean * (S * S + 2) * U + 1e-30
    out[:, C:] = np.abs(np.asarray(centres, dtype=np.float64)[:, C:]) * U + 1e-30
    return out


def slic(scene, H, W, S, compactness, iterations):
    """init, iterations x (assign, update), a last assign -> (seg, centres, counts, ties: the pixels that were a tie in ANY assign)."""
    centres = init(scene, H, W, S)
    counts = np.zeros(centres.shape[0], dtype=np.int64)
    ties = np.zeros((H, W), dtype=bool)
    for _ in range(iterations):
        seg, tie = assign(scene, H, W, S, compactness, centres)
        ties |= tie
        centres, counts, _ = update(scene, H, W, S, seg, centres)
    seg, tie = assign(scene, H, W, S, compactness, centres)
    return seg, centres, counts, ties | tie


def purity(seg, ids):
    """The share of pixels whose id (the base spectrum of their region) is their segment's most frequent one."""
    seg, ids = np.asarray(seg).reshape(-1), np.asarray(ids).reshape(-1)
    table = np.zeros((seg.max() + 1, ids.max() + 1), dtype=np.int64)
    np.add.at(table, (seg, ids), 1)
    return table.max(1).sum() / seg.size


def grid_segments(H, W, S):
    """The plain grid: every pixel in the cluster of its own cell."""
    return candidates(H, W, S)[0][4]


def softmax_rows(logits):
    """logits [n, K] float32 -> softmax [n, K] float64."""
    l = np.asarray(logits, dtype=np.float32).astype(np.float64)
    e = np.exp(l - l.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def first_max(rows):
    return np.asarray(rows).argmax(-1)                   # (numpy: the first maximal index)


def vote(prob, mask, seg, S, mode):
    """-> (segprob [Kc, K] float64, segcount [Kc] int64, labels [H, W] int64 (0 where mask is 0), rows [H, W, K]: prob_out,
    orphan [H, W] bool: masked pixels whose seg is none of their candidates and who stand for themselves)."""
    mask = np.asarray(mask) != 0
    H, W = mask.shape
    p = np.where(mask[:, :, None], np.asarray(prob, dtype=np.float64), 0.0)        # an unmasked row is never read
    K = p.shape[2]
    gh, gw = grid(H, W, S)
    seg = np.asarray(seg).astype(np.int64)
    m = members(seg, H, W, S) & mask
    k = seg[m]
    segcount = np.bincount(k, minlength=gh * gw)
    segprob = np.zeros((gh * gw, K))
    own = first_max(p)
    if mode == 'mean':
        np.add.at(segprob, k, p[m])
        segprob /= np.maximum(segcount, 1)[:, None]
    else:
        np.add.at(segprob, (k, own[m]), 1.0)
    orphan = mask & ~m
    rows = np.zeros((H, W, K))
    rows[m] = segprob[k]
    rows[orphan] = p[orphan] if mode == 'mean' else np.eye(K)[own[orphan]]
    labels = np.where(mask, first_max(rows), 0)
    return segprob, segcount, labels, rows, orphan


def vote_bound(segprob, segcount):
    """Mode mean: an fp32 chain of `count` non-negative terms and one divide: |delta| <= segprob (count + 2) u (+ 1e-30)."""
    return np.asarray(segprob) * (np.asarray(segcount)[:, None] + 2) * U + 1e-30


def vote_unclear(segprob, segcount):
    """[Kc] bool, mode mean: the float64 gap between the largest and the second largest entry of a segment's row is within the sum
    of their fp32 bounds (vote_bound), so an fp32 kernel may name either class: the label margin of the vote."""
    segprob = np.asarray(segprob)
    if segprob.shape[1] < 2:
        return np.zeros(segprob.shape[0], dtype=bool)
    s = np.sort(segprob, axis=1)
    return s[:, -1] - s[:, -2] <= (s[:, -1] + s[:, -2]) * (np.asarray(segcount) + 2) * U + 2e-30


def top2_margin(rows):
    """[...]: the largest minus the second largest entry of every row (K == 1: +inf)."""
    if rows.shape[-1] < 2:
        return np.full(rows.shape[:-1], np.inf)
    s = np.sort(rows, axis=-1)
    return s[..., -1] - s[..., -2]
