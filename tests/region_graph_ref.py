"""The reference of the spectrum-aware fragment merge: the arithmetic that include/dmf.h states for
dmf_region_graph_merge, in plain Python / numpy that shares nothing with utils/.  The sums are integers and every double operation
is one numpy operation of its own (numpy contracts nothing), so every comparison against it is equality.

A component's feature is the 64-bit integer sum of the quantised scene values of its pixels (regions_ref.quantise: the vote's
quantiser).  Every component starts as a group; a group is active while it is not kept.  In a round every active group chooses,
among the groups that share a 4-neighbour pixel pair with it, the one with the smallest (squared distance of the means, id); then
all pairs (group, choice) are united.  A united group is kept when a member was, or when its pixel count reaches min_size."""
import numpy as np

import regions_ref as R

SCALE = float(1 << R.QBITS)


def kept_components(labels, roots, counts, n_labels, min_size):
    """bool [n]: §24's rule for the components with the ascending `roots`: size >= min_size, main component of a label in
    0..n_labels - 1 (the largest, on equal size the smaller root), or root 0."""
    lab = np.asarray(labels).reshape(-1)
    main = {}
    for n, r in enumerate(roots.tolist()):               # ascending roots: on equal size the earlier one stays
        k = int(lab[r])
        if 0 <= k < n_labels and (k not in main or counts[n] > counts[main[k]]):
            main[k] = n
    kept = counts >= min_size
    kept[list(main.values())] = True
    kept[roots == 0] = True
    return kept


def round_bound(fragments):
    """The most rounds `fragments` initially active groups can take: 1 + floor(log2(fragments))."""
    return 0 if fragments < 1 else 1 + (int(fragments).bit_length() - 1)


def merge(labels, comp, scene, n_labels, min_size):
    """-> (region [H, W] int64, region_size [R], stats (R, components, components - R, rounds), info): `scene` [H, W, C] float32.
    info = dict(ties: how often an active group met its smallest distance at more than one neighbour, kept0: the number of
    initially kept components, fragments, per_round: the active groups at the start of every round)."""
    lab = np.asarray(labels)
    H, W = lab.shape
    a = np.asarray(scene, dtype=np.float32).reshape(H * W, -1)
    C = a.shape[1]
    roots, dense, counts = np.unique(np.asarray(comp).reshape(-1).astype(np.int64), return_inverse=True, return_counts=True)
    dense = dense.reshape(-1)
    n = roots.size
    kept0 = kept_components(lab, roots, counts, n_labels, min_size)
    order = np.argsort(dense, kind='stable')
    sums = np.add.reduceat(R.quantise(a)[order], np.searchsorted(dense[order], np.arange(n)), axis=0)     # int64 [n, C]: exact
    assert sums.shape == (n, C) and sums.max(initial=0) < 1 << 62
    img = dense.reshape(H, W)
    pairs = np.concatenate([np.stack([img[:, 1:].ravel(), img[:, :-1].ravel()], 1), np.stack([img[1:, :].ravel(), img[:-1, :].ravel()], 1)])
    pairs = np.unique(pairs[pairs[:, 0] != pairs[:, 1]], axis=0)
    # a group is named by the dense index of its smallest root: ascending dense index = ascending root
    group = np.arange(n)
    gsum, gcount, gkept = {g: sums[g].copy() for g in range(n)}, {g: int(counts[g]) for g in range(n)}, {g: bool(kept0[g]) for g in range(n)}
    held = {g: int(kept0[g]) for g in range(n)}          # the initially kept components a group holds
    rounds, ties, per_round = 0, 0, []
    fragments = int((~kept0).sum())
    while True:
        active = sorted(g for g in gkept if not gkept[g])
        if not active:
            break
        rounds += 1
        per_round.append(len(active))
        assert rounds <= round_bound(fragments), (rounds, fragments)
        ids = np.array(sorted(gkept))
        row = {g: k for k, g in enumerate(ids.tolist())}
        mean = np.stack([gsum[g].astype(np.float64) / (np.float64(gcount[g]) * SCALE) for g in ids.tolist()])
        f, g = group[pairs[:, 0]], group[pairs[:, 1]]
        both = np.concatenate([np.stack([f, g], 1), np.stack([g, f], 1)])
        both = np.unique(both[both[:, 0] != both[:, 1]], axis=0)
        is_active = np.array([not gkept[x] for x in ids.tolist()])
        both = both[is_active[[row[x] for x in both[:, 0].tolist()]]]
        mf, mg = mean[[row[x] for x in both[:, 0].tolist()]], mean[[row[x] for x in both[:, 1].tolist()]]
        d = np.zeros(len(both))
        for b in range(C):                               # ascending bands; a subtraction, a product and an addition, each rounded
            t = mf[:, b] - mg[:, b]
            d = d + t * t
        choice = {}
        for (x, y), dist in zip(both.tolist(), d.tolist()):
            if x not in choice or (dist, y) < choice[x][:2]:
                choice[x] = (dist, y, 1)
            elif dist == choice[x][0]:
                choice[x] = choice[x][:2] + (choice[x][2] + 1,)
        assert sorted(choice) == active                  # the image is connected: every active group has a neighbour
        ties += sum(1 for v in choice.values() if v[2] > 1)
        up = {g: g for g in gkept}

        def find(x):
            while up[x] != x:
                x = up[x]
            return x
        for x in active:
            p, q = find(x), find(choice[x][1])
            if p != q:
                up[max(p, q)] = min(p, q)
        nsum, ncount, nkept, nheld, had_kept = {}, {}, {}, {}, {}
        for g in sorted(gkept):
            r = find(g)
            if r not in nsum:
                nsum[r], ncount[r], nkept[r], nheld[r], had_kept[r] = np.zeros(C, dtype=np.int64), 0, False, 0, 0
            nsum[r] += gsum[g]
            ncount[r] += gcount[g]
            nkept[r] = nkept[r] or gkept[g]
            nheld[r] += held[g]
            had_kept[r] += int(gkept[g])
        assert max(had_kept.values()) <= 1 and max(nheld.values()) <= 1      # two kept regions never merge
        for r in nkept:
            nkept[r] = nkept[r] or ncount[r] >= min_size
        group = np.array([find(g) for g in group.tolist()])
        gsum, gcount, gkept, held = nsum, ncount, nkept, nheld
    ids = sorted(gkept)
    number = {g: k for k, g in enumerate(ids)}
    region = np.array([number[g] for g in group.tolist()], dtype=np.int64)[dense]
    Rn = len(ids)
    assert sum(gcount.values()) == H * W
    return (region.reshape(H, W), np.bincount(region, minlength=Rn), (Rn, int(n), int(n) - Rn, rounds),
            dict(ties=ties, kept0=int(kept0.sum()), fragments=fragments, per_round=per_round))
