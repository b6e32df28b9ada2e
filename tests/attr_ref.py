"""An independent reference for `band_profile: area`: it shares no code with utils/attribute.py and does not
decompose into thresholds.  The quantiser and value() are written out pixel by pixel in Python floats (IEEE doubles).  The area
opening is a sequential union-find over the pixels in descending level order: a pixel joins at its own level and waits in its
component's pending list; after a level is complete, every component that was touched and has reached the area gives its pending
pixels that level — the first (highest) level at which the component that holds them is large enough.  What still waits at the
end takes level 0, which always counts."""
import functools
import math

import numpy as np


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def canon_list(plane):
    """The plane's values as Python floats, every -0 turned into +0 in float32."""
    return [float(np.float32(v) + np.float32(0.0)) for v in np.asarray(plane, dtype=np.float32).ravel()]


def quantise(vals, L):
    """-> (q as a list of ints, lo, hi)."""
    lo, hi = min(vals), max(vals)
    if hi == lo:
        return [0] * len(vals), lo, hi
    q = []
    for v in vals:
        d = v - lo
        m = d * float(L)
        q.append(min(L - 1, int(math.floor(m / (hi - lo)))))
    return q, lo, hi


def value(c, lo, hi, L):
    m = float(c) * (hi - lo)
    return np.float32(lo + m / float(L))


def area_open(q, H, W, area):
    """q: a list of H W ints >= 0 in raster order -> the opened levels as a list."""
    N = H * W
    parent = list(range(N))
    size = [0] * N
    pending = [None] * N
    added = [False] * N
    out = [0] * N
    buckets = {}
    for x, v in enumerate(q):
        buckets.setdefault(v, []).append(x)

    def find(a):
        root = a
        while parent[root] != root:
            root = parent[root]
        while parent[a] != root:
            parent[a], a = root, parent[a]
        return root

    for t in sorted(buckets, reverse=True):
        if t == 0:
            break
        for x in buckets[t]:
            added[x], size[x], pending[x] = True, 1, [x]
            i, j = divmod(x, W)
            for ok, y in ((i > 0, x - W), (j > 0, x - 1), (j < W - 1, x + 1), (i < H - 1, x + W)):
                if ok and added[y]:
                    a, b = find(x), find(y)
                    if a != b:
                        if len(pending[a]) < len(pending[b]):
                            a, b = b, a
                        parent[b] = a
                        size[a] += size[b]
                        pending[a] += pending[b]
                        pending[b] = None
        for x in buckets[t]:
            r = find(x)
            if size[r] >= area and pending[r]:
                for y in pending[r]:
                    out[y] = t
                pending[r] = []
    return out


def profile_uncached(scores, P, areas, L):
    scores = np.asarray(scores, dtype=np.float32)
    H, W, K = scores.shape
    n = len(areas)
    out = np.empty((H, W, K + 2 * n * P), dtype=np.float32)
    levels = {}
    for p in range(P):
        vals = canon_list(scores[:, :, p])
        q, lo, hi = quantise(vals, L)
        base = p * (2 * n + 1)
        out[:, :, base + n] = np.array(vals, dtype=np.float32).reshape(H, W)
        for i, a in enumerate(areas):
            opened = area_open(q, H, W, a)
            closed = [L - 1 - c for c in area_open([L - 1 - v for v in q], H, W, a)]
            levels[(p, i)] = (np.array(opened).reshape(H, W), np.array(closed).reshape(H, W))
            out[:, :, base + n + 1 + i] = np.array([value(c, lo, hi, L) for c in opened], dtype=np.float32).reshape(H, W)
            out[:, :, base + n - 1 - i] = np.array([value(c, lo, hi, L) for c in closed], dtype=np.float32).reshape(H, W)
        levels[p] = np.array(q).reshape(H, W)
    out[:, :, P * (2 * n + 1):] = scores[:, :, P:]
    out.setflags(write=False)
    return out, levels


@functools.lru_cache(maxsize=None)
def case_profile(name):
    """(profile [H, W, C] float32, levels) of the named case of tests/attr_cases.py: computed once, read-only.
    levels[p] = q of component p; levels[(p, i)] = (opened, closed) levels at area i."""
    import attr_cases as ac
    c = ac.cases()[name]
    return profile_uncached(c.scores, c.P, c.areas, c.L)
