"""An independent reference for the multi-attribute profile: no code shared with utils/attribute.py or the
kernels, no threshold decomposition, Python integers throughout.  A sequential union-find takes the pixels in descending level
order; every root carries (size, box, sum q, sum q^2) of its component.  After level t is complete, every living component is
tested against every threshold, and a component that qualifies credits one level to all of its members: the credit is kept at
the root, and a root that is linked under another keeps the difference, so that a pixel's count is the sum of the credits along
its path.  Nothing assumes that a component which qualifies at one level qualifies at the next: the count is the number of
qualifying levels, whatever the attribute.  The quantiser, value() and the canonicalisation are tests/attr_ref.py's."""
import functools

import numpy as np

import attr_ref as ar


def qualifies(kind, tau, size, box, sum_q, sum_q2):
    if kind == 'a':
        return size >= tau
    if kind == 'd':
        w, h = box[1] - box[0] + 1, box[3] - box[2] + 1
        return w * w + h * h >= tau * tau
    return size * sum_q2 - sum_q * sum_q >= tau * tau * size * size


def open_counts(q, H, W, thresholds):
    """q: H W ints >= 0 in raster order; thresholds: [(kind, tau)], kind 'a' / 'd' / 's' -> per threshold the list of counts."""
    N, n = H * W, len(thresholds)
    parent = list(range(N))
    added = [False] * N
    size, box, sum_q, sum_q2 = [0] * N, [None] * N, [0] * N, [0] * N
    credit = [None] * N                    # at a root: levels credited to every member; below a root: the difference kept at the link
    alive = set()
    buckets = {}
    for x, v in enumerate(q):
        buckets.setdefault(v, []).append(x)

    def find(a):
        while parent[a] != a:
            a = parent[a]
        return a

    for t in range(max(q), 0, -1):
        for x in buckets.get(t, ()):
            i, j = divmod(x, W)
            added[x], size[x], box[x], sum_q[x], sum_q2[x], credit[x] = True, 1, [j, j, i, i], t, t * t, [0] * n
            alive.add(x)
            for ok, y in ((i > 0, x - W), (j > 0, x - 1), (j < W - 1, x + 1), (i < H - 1, x + W)):
                if ok and added[y]:
                    a, b = find(x), find(y)
                    if a == b:
                        continue
                    if size[a] < size[b]:
                        a, b = b, a
                    parent[b] = a                                             # by size: the paths stay short without compression
                    credit[b] = [cb - ca for cb, ca in zip(credit[b], credit[a])]
                    size[a] += size[b]
                    sum_q[a] += sum_q[b]
                    sum_q2[a] += sum_q2[b]
                    box[a] = [min(box[a][0], box[b][0]), max(box[a][1], box[b][1]), min(box[a][2], box[b][2]), max(box[a][3], box[b][3])]
                    alive.discard(b)
        for r in alive:
            for k, (kind, tau) in enumerate(thresholds):
                if qualifies(kind, tau, size[r], box[r], sum_q[r], sum_q2[r]):
                    credit[r][k] += 1
    out = [[0] * N for _ in range(n)]
    for x in range(N):
        if added[x]:
            a = x
            while True:
                for k in range(n):
                    out[k][x] += credit[a][k]
                if parent[a] == a:
                    break
                a = parent[a]
    return out


def profile_uncached(scores, P, areas, diagonals, stds, L):
    """-> (profile [H, W, K + 2 n P] float32, levels): levels[p] = q of component p, levels[(p, i)] = (opened, closed) levels at
    threshold i of areas ++ diagonals ++ stds."""
    scores = np.asarray(scores, dtype=np.float32)
    H, W, K = scores.shape
    thresholds = [('a', int(a)) for a in areas] + [('d', int(d)) for d in diagonals] + [('s', int(s)) for s in stds]
    n = len(thresholds)
    out = np.empty((H, W, K + 2 * n * P), dtype=np.float32)
    levels = {}
    for p in range(P):
        vals = ar.canon_list(scores[:, :, p])
        q, lo, hi = ar.quantise(vals, L)
        base = p * (2 * n + 1)
        out[:, :, base + n] = np.array(vals, dtype=np.float32).reshape(H, W)
        opened = open_counts(q, H, W, thresholds)
        dual = open_counts([L - 1 - v for v in q], H, W, thresholds)
        for i in range(n):
            closed = [L - 1 - c for c in dual[i]]
            levels[(p, i)] = (np.array(opened[i]).reshape(H, W), np.array(closed).reshape(H, W))
            out[:, :, base + n + 1 + i] = np.array([ar.value(c, lo, hi, L) for c in opened[i]], dtype=np.float32).reshape(H, W)
            out[:, :, base + n - 1 - i] = np.array([ar.value(c, lo, hi, L) for c in closed], dtype=np.float32).reshape(H, W)
        levels[p] = np.array(q).reshape(H, W)
    out[:, :, P * (2 * n + 1):] = scores[:, :, P:]
    out.setflags(write=False)
    return out, levels


@functools.lru_cache(maxsize=None)
def case_profile(name):
    """(profile, levels) of the named case of tests/attr_multi_cases.py: computed once, read-only."""
    import attr_multi_cases as amc
    c = amc.cases()[name]
    return profile_uncached(c.scores, c.P, c.areas, c.diagonals, c.stds, c.L)
