"""utils.segments — the host side of `test.segments` and `color.segments`: the config keys, the report block, and
for `fast_path: 0` the arithmetic of dmf_slic_init / dmf_slic_assign / dmf_slic_update / dmf_segment_vote (include/dmf.h) in numpy
float64.  Nothing here touches the GPU library.

The scene is over-segmented into SLIC superpixels in the pixel-centric form: cells of S x S pixels, one cluster per cell for life,
and every pixel chooses among the up to nine clusters of its own and the adjacent cells (slot s = 3 (u + 1) + (v + 1)) the one with
the smallest D = mean_c (a_c - mu_c)^2 + (compactness / S)^2 |x - centre|^2, the first slot on equality.  Every classified pixel
then takes the class of its segment: of the mean probability of the segment's classified pixels, or of their majority.
Connectivity is not enforced by SLIC itself; `test.segment_connectivity: 1` splits the segments into their
4-connected components, joins small fragments to the component before them and votes over the regions: `components`, `regions` and
`region_vote` below are that arithmetic in integers.  `test.segments: file` votes over the components of a user's label image.
`test.segment_merge: spectrum` joins a fragment to the adjacent group with the nearest mean spectrum and lets groups
of fragments grow into regions: `region_graph`, the integers and double operations of dmf_region_graph_merge."""
import math

import numpy as np

KINDS = ('none', 'slic', 'file')
VOTES = ('mean', 'majority')
MERGES = ('position', 'spectrum')
SIZE_MIN, SIZE_MAX = 4, 32


def segment_keys(cfg):
    """-> dict(kind, size, compactness, iterations, vote, color) from the optional keys
         test.segments none / slic / file (default none) test.segment_size 4..32 (default 8)
         test.segment_compactness >= 0 (default 0.1)     test.segment_iterations >= 0 (default 10)
         test.segment_vote mean / majority (default mean)  color.segments 0 / 1 (default 0)
    `kind` is None, 'slic' or 'file' (a user's label image: `region_keys` reads its path).  Neutral values change nothing."""
    test, color = cfg.get('test') or {}, cfg.get('color') or {}
    kind = test.get('segments', 'none')
    kind = 'none' if kind is None or kind is False or kind == 0 else str(kind).lower()
    if kind not in KINDS:
        raise ValueError('test.segments %r is not one of %s' % (test.get('segments'), ' / '.join(KINDS)))
    col = color.get('segments', 0) or 0
    if col not in (0, 1, True, False):
        raise ValueError('color.segments is 0 or 1')
    size, its = test.get('segment_size', 8), test.get('segment_iterations', 10)
    if isinstance(size, bool) or not isinstance(size, int) or not SIZE_MIN <= size <= SIZE_MAX:
        raise ValueError('test.segment_size %r is not a whole number in %d..%d' % (size, SIZE_MIN, SIZE_MAX))
    if isinstance(its, bool) or not isinstance(its, int) or its < 0:
        raise ValueError('test.segment_iterations %r is not a whole number >= 0' % (its,))
    comp = test.get('segment_compactness', 0.1)
    try:
        f = float(comp)
    except (TypeError, ValueError):
        f = float('nan')
    if isinstance(comp, bool) or not (math.isfinite(f) and f >= 0):
        raise ValueError('test.segment_compactness %r is not a number >= 0' % (comp,))
    vote = str(test.get('segment_vote', 'mean')).lower()
    if vote not in VOTES:
        raise ValueError('test.segment_vote %r is not one of %s' % (test.get('segment_vote'), ' / '.join(VOTES)))
    if col and kind == 'none':
        raise ValueError('color.segments: 1 draws the map that test.segments: slic votes on; test.segments is none')
    return dict(kind=None if kind == 'none' else kind, size=size, compactness=f, iterations=its, vote=vote, color=bool(col))


def region_keys(cfg, keys):
    """-> dict(connectivity, min_size, file) from the optional keys, given `segment_keys`' dict
         test.segment_connectivity 0 / 1 (default 0)     test.segment_min_size auto / n >= 1 (default auto)
         test.segment_file <path.npy>: the label image of test.segments: file, whose regions are its components
    auto is max(1, S^2 div 4) for slic (Achanta et al. 2012) and 1 for file, which implies connectivity.  Neutral values change
    nothing."""
    test = cfg.get('test') or {}
    con = test.get('segment_connectivity', 0) or 0
    if con not in (0, 1, True, False):
        raise ValueError('test.segment_connectivity is 0 or 1')
    ms = test.get('segment_min_size', 'auto')
    if ms is None or (isinstance(ms, str) and ms.lower() == 'auto'):
        ms = None
    elif isinstance(ms, bool) or not isinstance(ms, int) or not 1 <= ms < 1 << 31:
        raise ValueError('test.segment_min_size %r is not auto or a whole number >= 1' % (ms,))
    path = test.get('segment_file')
    if keys['kind'] == 'file':
        if not isinstance(path, str) or not path:
            raise ValueError('test.segments: file reads the label image test.segment_file: <path.npy>, which is not given')
        con = 1
    elif path:
        raise ValueError('test.segment_file is read by test.segments: file; test.segments is %s' % (keys['kind'] or 'none'))
    if con and keys['kind'] is None:
        raise ValueError('test.segment_connectivity: 1 connects the segments of test.segments: slic; test.segments is none')
    if ms is None:
        ms = max(1, keys['size'] ** 2 // 4) if keys['kind'] == 'slic' else 1
    return dict(connectivity=bool(con), min_size=ms, file=path if keys['kind'] == 'file' else None)


def merge_key(cfg, region):
    """-> 'position' or 'spectrum' from the optional key, given `region_keys`' dict
         test.segment_merge position / spectrum (default position): where a fragment goes
    spectrum is valid only where regions are made: test.segment_connectivity: 1 or test.segments: file."""
    given = (cfg.get('test') or {}).get('segment_merge', 'position')
    merge = 'position' if given is None else str(given).lower()
    if merge not in MERGES:
        raise ValueError('test.segment_merge %r is not one of %s' % (given, ' / '.join(MERGES)))
    if merge != 'position' and not region['connectivity']:
        raise ValueError('test.segment_merge: %s merges the fragments of test.segment_connectivity: 1 or test.segments: file; '
                         'neither is set' % merge)
    return merge


def keys_in_use(keys):
    """The names of the keys that are not neutral, for a refusal."""
    return [name for name, used in (('test.segments', keys['kind'] is not None), ('color.segments', keys['color'])) if used]


def grid(H, W, size):
    return (H + size - 1) // size, (W + size - 1) // size


def _candidates(H, W, size):
    """[(cluster index [H, W] (0 where invalid), valid [H, W])] for the nine slots in ascending order."""
    gh, gw = grid(H, W, size)
    gi, gj = np.arange(H)[:, None] // size, np.arange(W)[None, :] // size
    out = []
    for u in (-1, 0, 1):
        for v in (-1, 0, 1):
            ok = (gi + u >= 0) & (gi + u < gh) & (gj + v >= 0) & (gj + v < gw)
            out.append((np.where(ok, (gi + u) * gw + gj + v, 0), ok))
    return out


def init_centres(scene, H, W, size):
    """centres [Kc, C + 2] float64: the spectrum, row and column of the pixel in the middle of every cell."""
    a = np.asarray(scene)[:H, :W].astype(np.float64)
    gh, gw = grid(H, W, size)
    k = np.arange(gh * gw)
    i, j = np.minimum(H - 1, (k // gw) * size + size // 2), np.minimum(W - 1, (k % gw) * size + size // 2)
    return np.concatenate([a[i, j], i[:, None].astype(np.float64), j[:, None].astype(np.float64)], 1)


def assign(scene, H, W, size, compactness, centres):
    """seg [H, W] int32; cw is rounded to fp32 as the kernel's is."""
    a = np.asarray(scene)[:H, :W].astype(np.float64)
    C = a.shape[2]
    cw = float(np.float32((float(np.float32(compactness)) / size) ** 2))
    i, j = np.arange(H)[:, None].astype(np.float64), np.arange(W)[None, :].astype(np.float64)
    cands = _candidates(H, W, size)
    best, seg = np.full((H, W), np.inf), cands[4][0]     # (the pixel's own cell is the fallback)
    for k, ok in cands:
        mu = centres[k]
        D = np.square(a - mu[:, :, :C]).sum(2) / C + cw * (np.square(i - mu[:, :, C]) + np.square(j - mu[:, :, C + 1]))
        take = ok & (D < best)                           # strict: the first slot on equality
        seg = np.where(take, k, seg)
        best = np.where(take, D, best)
    return seg.astype(np.int32)


def _members(seg, H, W, size):
    m = np.zeros((H, W), dtype=bool)
    for k, ok in _candidates(H, W, size):
        m |= ok & (seg == k)
    return m


def update(scene, H, W, size, seg, centres):
    """-> (centres', counts [Kc] int32): the mean spectrum and position of every cluster's members; without one the row stays."""
    a = np.asarray(scene)[:H, :W].astype(np.float64)
    gh, gw = grid(H, W, size)
    m = _members(seg, H, W, size)
    k = np.asarray(seg)[m].astype(np.int64)
    counts = np.bincount(k, minlength=gh * gw)
    ii, jj = np.nonzero(m)
    sums = np.zeros_like(centres)
    np.add.at(sums, k, np.concatenate([a[m], ii[:, None].astype(np.float64), jj[:, None].astype(np.float64)], 1))
    out = centres.copy()
    out[counts > 0] = sums[counts > 0] / counts[counts > 0][:, None]
    return out, counts.astype(np.int32)


def slic(scene, H, W, size, compactness, iterations):
    """-> (seg [H, W] int32, centres, counts): init, `iterations` x (assign, update), a last assign."""
    centres = init_centres(scene, H, W, size)
    counts = np.zeros(centres.shape[0], dtype=np.int32)
    for _ in range(iterations):
        centres, counts = update(scene, H, W, size, assign(scene, H, W, size, compactness, centres), centres)
    return assign(scene, H, W, size, compactness, centres), centres, counts


def vote(prob, mask, seg, size, mode):
    """-> (segprob [Kc, K] float64, segcount [Kc] int32, label map [H, W] int32: 0 where mask is 0).  A masked pixel whose seg is
    none of its candidates stands for itself."""
    live = np.asarray(mask) != 0
    H, W = live.shape
    p = np.where(live[:, :, None], np.asarray(prob, dtype=np.float64), 0.0)
    gh, gw = grid(H, W, size)
    m = _members(seg, H, W, size) & live
    k = np.asarray(seg)[m].astype(np.int64)
    segcount = np.bincount(k, minlength=gh * gw)
    segprob = np.zeros((gh * gw, p.shape[2]))
    own = p.argmax(2)
    if mode == 'mean':
        np.add.at(segprob, k, p[m])
        segprob /= np.maximum(segcount, 1)[:, None]
    else:
        np.add.at(segprob, (k, own[m]), 1.0)
    labels = own.copy()
    labels[m] = segprob[k].argmax(1)
    return segprob, segcount.astype(np.int32), np.where(live, labels, 0).astype(np.int32)


# ------------------------------------------------------------------------------------------------ connected regions
# The integer arithmetic of dmf_label_components / dmf_region_merge / dmf_region_vote (include/dmf.h): equal, not close.
QBITS = 36                                   # the mean vote's fixed point: q = rint(clamp(p, 0, 1) 2^36)


def _hook(n, a, b):
    """p [n] int64: for every index the smallest index of its set, the pairs (a[i], b[i]) joined.  Hooking the larger root of every
    joined pair to the smaller one and jumping pointers, in O(log n) rounds."""
    p = np.arange(n, dtype=np.int64)
    while True:
        pa, pb = p[a], p[b]
        differ = pa != pb
        if not differ.any():
            return p
        np.minimum.at(p, np.maximum(pa, pb)[differ], np.minimum(pa, pb)[differ])
        while True:
            pp = p[p]
            if np.array_equal(pp, p):
                break
            p = pp


def _kept(flat, roots, size, n_labels, min_size):
    """DESIGN.md §24's kept rule over the ascending `roots` (their pixel counts `size`) -> bool per root: at least min_size pixels,
    or root 0, or the main component (the largest, then the smaller root) of a label in 0..n_labels - 1."""
    kept = size >= min_size
    kept[0] = True                                       # (pixel 0 is the first root)
    named = np.nonzero((flat[roots] >= 0) & (flat[roots] < n_labels))[0]
    if named.size:
        order = np.lexsort((named, -size[named], flat[roots][named]))       # by label, the largest first, then the smaller root
        first = np.concatenate([[True], np.diff(flat[roots][named][order]) != 0])
        kept[named[order][first]] = True
    return kept


def components(labels):
    """comp [H, W] int32: for every pixel the smallest raster index of its 4-connected component of equal values."""
    lab = np.asarray(labels)
    H, W = lab.shape
    idx = np.arange(H * W, dtype=np.int64).reshape(H, W)
    right, down = lab[:, 1:] == lab[:, :-1], lab[1:, :] == lab[:-1, :]
    a = np.concatenate([idx[:, 1:][right], idx[1:, :][down]])
    b = np.concatenate([idx[:, :-1][right], idx[:-1, :][down]])
    return _hook(H * W, a, b).reshape(H, W).astype(np.int32)


def regions(labels, n_labels=0, min_size=1):
    """-> (region [H, W] int32, region sizes [R] int32, dict(regions, components, absorbed)): the components of `labels`, with
    every fragment (smaller than min_size, not the main component of a label in 0..n_labels - 1, not at pixel 0) joined to the end
    of the chain of components before it: the one left of its root, above it for a root in column 0.  Regions are numbered in
    ascending order of their roots."""
    lab = np.asarray(labels)
    H, W = lab.shape
    if isinstance(min_size, bool) or int(min_size) != min_size or min_size < 1 or int(n_labels) != n_labels or n_labels < 0:
        raise ValueError('regions: min_size >= 1 and n_labels >= 0 are whole numbers')
    comp = components(lab).ravel().astype(np.int64)
    flat = lab.ravel()
    roots = np.nonzero(comp == np.arange(H * W))[0]
    size = np.bincount(comp, minlength=H * W)
    kept = np.zeros(H * W, dtype=bool)
    kept[roots] = _kept(flat, roots, size[roots], n_labels, min_size)
    target = np.arange(H * W)
    frag = roots[~kept[roots]]
    target[frag] = np.where(frag % W > 0, comp[np.maximum(frag - 1, 0)], comp[np.maximum(frag - W, 0)])
    final = target.copy()
    while True:                                          # pointer jumping: the chains end at kept roots
        nxt = final[final]
        if np.array_equal(nxt, final):
            break
        final = nxt
    dense = np.cumsum(kept) - 1
    region = dense[final[comp]]
    R = int(kept.sum())
    return (region.reshape(H, W).astype(np.int32), np.bincount(region, minlength=R).astype(np.int32),
            dict(regions=R, components=int(roots.size), absorbed=int(frag.size)))


def region_graph(labels, scene, n_labels=0, min_size=1):
    """-> (region [H, W] int32, region sizes [R] int32, dict(regions, components, absorbed, rounds)): the components of `labels`
    with the spectrum-aware merge of dmf_region_graph_merge (include/dmf.h) on the leading [H, W] pixels of `scene`
    [>= H, >= W, C] (fp32, or fp16 widened exactly).  A component's feature is the 64-bit integer sum of its pixels' quantised
    values; every component starts as a group, kept by `regions`' rule.  In a round every group that is not kept chooses, among the
    groups that share a 4-neighbour pixel pair with it, the smallest (squared distance of the mean spectra in double, id), on the
    state at the start of the round; all pairs (group, choice) are united; sums and counts add, and the new group is kept when a
    member was or its count reaches min_size.  Regions are numbered in ascending order of their smallest roots."""
    lab = np.asarray(labels)
    H, W = lab.shape
    if isinstance(min_size, bool) or int(min_size) != min_size or min_size < 1 or int(n_labels) != n_labels or n_labels < 0:
        raise ValueError('region_graph: min_size >= 1 and n_labels >= 0 are whole numbers')
    a = np.asarray(scene)[:H, :W]
    if a.ndim != 3 or a.shape[:2] != (H, W) or a.shape[2] < 1:
        raise ValueError('region_graph: the scene must hold [%d, %d] pixels of C >= 1 bands' % (H, W))
    comp = components(lab).ravel().astype(np.int64)
    flat = lab.ravel()
    is_root = comp == np.arange(H * W)
    roots = np.nonzero(is_root)[0]
    n = roots.size
    count = np.bincount(comp, minlength=H * W)[roots]
    kept = _kept(flat, roots, count, n_labels, min_size)
    index = (np.cumsum(is_root) - 1)[comp].reshape(H, W)  # the dense component index of every pixel: ascending = ascending root
    sums = np.zeros((n, a.shape[2]), dtype=np.int64)
    np.add.at(sums, index.ravel(), quantise(a.astype(np.float32).reshape(H * W, -1)))
    ea = np.concatenate([index[:, 1:].ravel(), index[1:, :].ravel()])
    eb = np.concatenate([index[:, :-1].ravel(), index[:-1, :].ravel()])
    edges = np.unique(np.stack([ea, eb], 1)[ea != eb], axis=0)
    group, rounds = np.arange(n), 0
    while not kept[np.unique(group)].all():
        rounds += 1
        f, g = group[edges[:, 0]], group[edges[:, 1]]
        pairs = np.concatenate([np.stack([f, g], 1), np.stack([g, f], 1)])
        pairs = np.unique(pairs[(pairs[:, 0] != pairs[:, 1]) & ~kept[pairs[:, 0]]], axis=0)
        mean = sums.astype(np.float64) / (count.astype(np.float64) * float(1 << QBITS))[:, None]
        d = np.zeros(len(pairs))
        for b in range(sums.shape[1]):                   # one subtraction, one product, one addition at a time: nothing contracted
            t = mean[pairs[:, 0], b] - mean[pairs[:, 1], b]
            d = d + t * t
        order = np.lexsort((pairs[:, 1], d, pairs[:, 0]))
        first = np.concatenate([[True], np.diff(pairs[order, 0]) != 0])
        cf, cg = pairs[order][first, 0], pairs[order][first, 1]
        p = _hook(n, cf, cg)
        ids = np.unique(group)
        gone = ids[p[ids] != ids]
        np.add.at(sums, p[gone], sums[gone])
        np.add.at(count, p[gone], count[gone])
        np.logical_or.at(kept, p[gone], kept[gone])
        group = p[group]
        ids = np.unique(group)
        kept[ids] |= count[ids] >= min_size
    ids = np.unique(group)
    region = np.searchsorted(ids, group)[index]
    R = int(ids.size)
    return (region.astype(np.int32), np.bincount(region.ravel(), minlength=R).astype(np.int32),
            dict(regions=R, components=int(n), absorbed=int(n) - R, rounds=rounds))


def quantise(prob):
    """int64: rint(clamp(p, 0, 1) 2^36), half to even, a NaN as 0."""
    p = np.asarray(prob, dtype=np.float32).astype(np.float64)
    return np.rint(np.where(p > 0, np.minimum(p, 1.0), 0.0) * float(1 << QBITS)).astype(np.int64)


def region_vote(prob, mask, region, R, mode):
    """-> (regprob [R, K] float32, regcount [R] int32, label map [H, W] int32: 0 where mask is 0).  mode mean: 64-bit integer sums
    of the quantised probabilities, divided once in double and rounded to fp32; majority: the counts of the first maximal classes.
    A masked pixel whose region is outside 0..R - 1 stands for itself."""
    live = np.asarray(mask) != 0
    reg = np.asarray(region)
    K = np.asarray(prob).shape[2]
    m = live & (reg >= 0) & (reg < R)
    k = reg[m].astype(np.int64)
    p = np.where(live[:, :, None], np.asarray(prob, dtype=np.float32), np.float32(0))
    own = p.argmax(2)                                    # (numpy's argmax: the first maximal index)
    regcount = np.bincount(k, minlength=R)
    acc = np.zeros((R, K), dtype=np.int64)
    if mode == 'mean':
        np.add.at(acc, k, quantise(p[m]))
        regprob = (acc.astype(np.float64) / (np.maximum(regcount, 1)[:, None].astype(np.float64) * float(1 << QBITS))).astype(np.float32)
    elif mode == 'majority':
        np.add.at(acc, (k, own[m]), 1)
        regprob = acc.astype(np.float32)
    else:
        raise ValueError('region_vote: the mode %r is not mean or majority' % (mode,))
    labels = own.copy()
    labels[m] = regprob[k].argmax(1)
    return regprob, regcount.astype(np.int32), np.where(live, labels, 0).astype(np.int32)


def load_segment_file(path, H, W):
    """The label image of `test.segment_file`: an integer [H, W] .npy array whose values fit int32 -> int32 [H, W]."""
    a = np.load(path, allow_pickle=False)
    if a.dtype.kind not in 'iu':
        raise ValueError('test.segment_file %s holds %s, not integers' % (path, a.dtype))
    if a.shape != (H, W):
        raise ValueError('test.segment_file %s has shape %s, the scene is %s' % (path, list(a.shape), [H, W]))
    if a.size and (int(a.min()) < -(1 << 31) or int(a.max()) >= 1 << 31):
        raise ValueError('test.segment_file %s holds values that do not fit int32' % path)
    return np.ascontiguousarray(a.astype(np.int32))


def region_report(block, min_size, stats, region_sizes):
    """`report`'s block with connectivity enforced: min_size, components, absorbed, regions, region_pixels."""
    sizes = np.asarray(region_sizes)
    out = dict(block)
    out.update(connectivity='enforced', min_size=int(min_size), components=int(stats['components']), absorbed=int(stats['absorbed']),
               regions=int(stats['regions']), region_pixels=dict(min=int(sizes.min()), mean=float(sizes.mean()), max=int(sizes.max())))
    if 'rounds' in stats:                                # test.segment_merge: spectrum
        out.update(merge='spectrum', rounds=int(stats['rounds']))
    return out


def report(keys, H, W, counts, matrix_before, matrix_after, changed):
    """The block of `<t>_segments.json`: the parameters, the grid, the sizes of the non-empty segments, the voted confusion matrix
    (rows = prediction), OA / AA / kappa before and after (indicators.kappa) and the number of test pixels whose class changed."""
    from indicators.kappa import aa_oa_quiet

    def block(m):
        aa, oa, k = aa_oa_quiet(np.asarray(m, dtype=np.float64))
        return dict(OA=oa, AA=aa, kappa=k)
    sizes = np.asarray(counts)[np.asarray(counts) > 0]
    if keys['kind'] == 'file':                           # no grid, no clusters: the file's values are the segments
        return dict(kind='file', vote=keys['vote'], segments=int(sizes.size),
                    segment_pixels=dict(min=int(sizes.min()), mean=float(sizes.mean()), max=int(sizes.max())) if sizes.size else None,
                    connectivity='not enforced', n=int(np.asarray(matrix_after).sum()),
                    matrix=np.asarray(matrix_after, dtype=np.int64).tolist(), before=block(matrix_before), after=block(matrix_after),
                    changed=int(changed))
    return dict(kind=keys['kind'], size=keys['size'], compactness=keys['compactness'], iterations=keys['iterations'], vote=keys['vote'],
                Kc=int(np.prod(grid(H, W, keys['size']))), segments=int(sizes.size),
                segment_pixels=dict(min=int(sizes.min()), mean=float(sizes.mean()), max=int(sizes.max())) if sizes.size else None,
                connectivity='not enforced', n=int(np.asarray(matrix_after).sum()),
                matrix=np.asarray(matrix_after, dtype=np.int64).tolist(), before=block(matrix_before), after=block(matrix_after),
                changed=int(changed))
