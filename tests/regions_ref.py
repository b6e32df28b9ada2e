"""The reference of the connected-superpixel tests: the integer arithmetic that include/dmf.h states for
dmf_label_components, dmf_region_merge and dmf_region_vote, in plain Python / numpy that shares nothing with utils/.  Everything is
integers, so every comparison against it is equality."""
import numpy as np

QBITS = 36


def components(labels):
    """comp [H, W] int64: the smallest raster index of every pixel's 4-connected component of equal labels.  One flood fill per
    component, started at the pixels in raster order: the start is the component's smallest index."""
    lab = np.asarray(labels)
    H, W = lab.shape
    flat = lab.reshape(-1).tolist()
    comp = [-1] * (H * W)
    for start in range(H * W):
        if comp[start] >= 0:
            continue
        comp[start] = start
        stack, l = [start], flat[start]
        while stack:
            x = stack.pop()
            i, j = divmod(x, W)
            for ok, y in ((j > 0, x - 1), (j < W - 1, x + 1), (i > 0, x - W), (i < H - 1, x + W)):
                if ok and comp[y] < 0 and flat[y] == l:
                    comp[y] = start
                    stack.append(y)
    return np.array(comp, dtype=np.int64).reshape(H, W)


def merge(labels, comp, n_labels, min_size):
    """-> (region [H, W] int64, region_size [R], stats (R, components, absorbed), depth: the longest chain a fragment follows)."""
    lab = np.asarray(labels).reshape(-1).tolist()
    H, W = np.asarray(labels).shape
    c = np.asarray(comp).reshape(-1).tolist()
    size = {}
    for r in c:
        size[r] = size.get(r, 0) + 1
    roots = sorted(size)
    main = {}
    for r in roots:                                      # ascending roots: on equal size the earlier one stays
        k = lab[r]
        if 0 <= k < n_labels and (k not in main or size[r] > size[main[k]]):
            main[k] = r
    mains = set(main.values())
    kept = [r for r in roots if size[r] >= min_size or r in mains or r == 0]
    keep = set(kept)
    final, depth = {}, {}
    for r in roots:                                      # ascending: a target is smaller and already resolved
        if r in keep:
            final[r], depth[r] = r, 0
        else:
            t = c[r - 1] if r % W > 0 else c[r - W]
            assert t < r
            final[r], depth[r] = final[t], depth[t] + 1
    dense = {r: n for n, r in enumerate(kept)}
    region = np.array([dense[final[r]] for r in c], dtype=np.int64)
    return (region.reshape(H, W), np.bincount(region, minlength=len(kept)), (len(kept), len(roots), len(roots) - len(kept)),
            max(depth.values()))


def regions(labels, n_labels, min_size):
    comp = components(labels)
    return (comp,) + merge(labels, comp, n_labels, min_size)


def first_max(rows):
    """The smallest index at which a row is largest (no NaN in the rows given)."""
    return np.argmax(np.asarray(rows), axis=-1)


def quantise(p):
    """int64: rint(clamp(p, 0, 1) 2^36), half to even, NaN as 0 — on the fp32 value's integer mantissa M 2^(e - 24), by shifts."""
    v = np.asarray(p, dtype=np.float32)
    v = np.where(v > 0, np.minimum(v, np.float32(1)), np.float32(0)).astype(np.float64)        # (a NaN compares false)
    m, e = np.frexp(v)
    M = (m * float(1 << 24)).astype(np.int64)            # exact: an fp32 value has 24 significant bits
    assert np.array_equal(M.astype(np.float64) * np.exp2(e.astype(np.float64) - 24), v)
    s = e.astype(np.int64) - 24 + QBITS
    up = M << np.clip(s, 0, 13)                          # v <= 1: e <= 1, s <= 13
    t = np.clip(-s, 1, 30)                               # (M < 2^24: from t = 26 on everything rounds to 0)
    q, rem, half = M >> t, M & ((1 << t) - 1), 1 << (t - 1)
    down = q + ((rem > half) | ((rem == half) & (q & 1 == 1)))
    return np.where(s >= 0, up, down)


def vote(prob, mask, region, R, mode):
    """-> (regprob [R, K] float32, regcount [R], labels [H, W] (0 where mask is 0), rows [H W, K] float32: what prob_out holds,
    sums: the integer sums [R, K] int64, orphan [H, W]: masked pixels whose region is outside 0..R - 1).  The rows of prob where
    mask is 0 are never looked at."""
    H, W, K = np.asarray(prob).shape
    live = (np.asarray(mask) != 0).reshape(-1)
    reg = np.asarray(region).reshape(-1).astype(np.int64)
    flat = np.zeros((H * W, K), dtype=np.float32)
    flat[live] = np.asarray(prob, dtype=np.float32).reshape(H * W, K)[live]
    own = first_max(flat)
    member = live & (reg >= 0) & (reg < R)
    orphan = live & ~member
    count = np.bincount(reg[member], minlength=R)
    sums = np.zeros((R, K), dtype=np.int64)
    if mode == 'mean':
        np.add.at(sums, reg[member], quantise(flat[member]))
        assert sums.max(initial=0) < (1 << 62)
        # (double)sum rounds to nearest even (numpy's int64 -> float64), the divisor is exact, the quotient correctly rounded
        regprob = (sums.astype(np.float64) / (np.maximum(count, 1)[:, None] * float(1 << QBITS))).astype(np.float32)
    else:
        np.add.at(sums, (reg[member], own[member]), 1)
        regprob = sums.astype(np.float32)
    labels = np.zeros(H * W, dtype=np.int64)
    rows = np.zeros((H * W, K), dtype=np.float32)
    labels[member] = first_max(regprob)[reg[member]]
    rows[member] = regprob[reg[member]]
    labels[orphan] = own[orphan]
    rows[orphan] = flat[orphan] if mode == 'mean' else np.eye(K, dtype=np.float32)[own[orphan]]
    return regprob, count, labels.reshape(H, W), rows, sums, orphan.reshape(H, W)


MEAN_BOUND = 2.0 ** -37 + 2.0 ** -25 + 2.0 ** -50        # include/dmf.h: quantisation, one fp32 rounding, the double steps


def float64_mean(prob, mask, region, R):
    """The plain float64 mean of clamp(p, 0, 1) over every region's masked members (zeros for an empty region)."""
    p = np.clip(np.nan_to_num(np.asarray(prob, dtype=np.float64), nan=0.0), 0.0, 1.0)
    m = (np.asarray(mask) != 0) & (np.asarray(region) >= 0) & (np.asarray(region) < R)
    out = np.zeros((R, p.shape[2]))
    for r in np.unique(np.asarray(region)[m]):
        out[r] = p[m & (np.asarray(region) == r)].mean(0)
    return out


def purity(seg, ids):
    """The share of pixels whose id is their segment's most frequent one."""
    seg, ids = np.asarray(seg).reshape(-1), np.asarray(ids).reshape(-1)
    _, inv = np.unique(seg, return_inverse=True)
    table = np.zeros((inv.max() + 1, ids.max() + 1), dtype=np.int64)
    np.add.at(table, (inv, ids), 1)
    return float(table.max(1).sum()) / seg.size
