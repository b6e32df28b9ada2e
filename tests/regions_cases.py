"""The cases of the connected-superpixel tests, shared by tests/test_regions_host.py (the guards, on the reference
alone) and tests/test_gpu_regions.py.  A plain module: no GPU, nothing of the HIP library.  The references are computed once per
process and handed out read-only.

Label images: every size with every pattern.  (129, 131) spans nine 16-pixel tiles on both axes; (64, 65) and (33, 17) end one
pixel past a tile.  The SLIC images are the float64 reference's (tests/segments_ref.py) of the 8-band scenes of
tests/segments_cases.py, compactness 0.05, ten iterations, with n_labels = Kc and min_size = max(1, S^2 div 4); every other pattern
runs with n_labels 0 and 2 and min_size 1, 2 and 4 (MERGES).

Recorded on the reference alone (tests/test_regions_host.py asserts them):
  * components against scipy.ndimage.label up to renaming, on every image;
  * SLIC, absorbed of components at min_size = S^2 div 4: ABSORBED below (64 x 65, S = 4: 57 of 330); the deepest chain is
    DEPTH (64 x 65, S = 16: 28);
  * with min_size 1 the regions' purity against segments_cases.ids is never below the raw segments' (a refinement):
    64 x 65 at S = 16: 0.870 -> 0.902;
  * purity after absorption is recorded, not asserted: PURITY_AFTER (64 x 65, S = 16: 0.254, where min_size 64 exceeds the true
    20-pixel regions and the left / up chains drag whole areas along)."""
import functools

import numpy as np

import segments_cases as SC
import segments_ref as SR

import regions_ref as R

SIZES = ((1, 1), (1, 70), (70, 1), (13, 9), (33, 17), (64, 65), (129, 131))
PATTERNS = ('uniform', 'checker', 'rows', 'columns', 'spiral', 'comb', 'noise', 'wide')
SLIC_S = (4, 5, 16)
MERGES = ((0, 1), (0, 2), (2, 4), (2, 1))               # (n_labels, min_size) of the synthetic patterns
VOTE_K = (1, 3, 17, 64)
VOTE_SIZES = ((1, 1), (13, 9), (33, 17), (64, 65))      # the vote is per pixel and per wave: tiles do not matter to it
CHAIN = (1, 4096)                                        # alternating labels, min_size 2, n_labels 0: a chain of 4,095

# (H, W, S) -> (absorbed, components) of the reference's SLIC image at min_size = max(1, S^2 div 4), n_labels = Kc
ABSORBED = {(1, 70, 4): (0, 18), (1, 70, 5): (0, 14), (1, 70, 16): (11, 16), (70, 1, 4): (0, 18), (70, 1, 5): (0, 14), (70, 1, 16): (6, 12),
            (13, 9, 4): (2, 14), (33, 17, 4): (6, 51), (64, 65, 4): (57, 330), (129, 131, 4): (213, 1304),
            (13, 9, 5): (1, 8), (33, 17, 5): (6, 32), (64, 65, 5): (14, 256), (129, 131, 5): (9, 1022),
            (13, 9, 16): (0, 1), (33, 17, 16): (3, 9), (64, 65, 16): (197, 217), (129, 131, 16): (906, 988)}
DEPTH = {(64, 65, 16): 28, (129, 131, 16): 56}
PURITY_RAW_TO_SPLIT = {(64, 65, 16): (0.870, 0.902)}
PURITY_AFTER = {(64, 65, 16): 0.254, (129, 131, 16): 0.243, (64, 65, 4): 0.996}


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def spiral(H, W):
    """Two labels: a one-pixel path of 1s that winds inwards from (0, 0) clockwise, one pixel of 0s between its turns."""
    a = np.zeros((H, W), dtype=np.int32)
    inside = lambda i, j: 0 <= i < H and 0 <= j < W
    i, j, di, dj = 0, 0, 0, 1
    a[0, 0] = 1
    while True:
        moved = False
        while True:                                      # on while the next cell is free and the one after it is not the path
            ni, nj = i + di, j + dj
            if not inside(ni, nj) or a[ni, nj] or (inside(ni + di, nj + dj) and a[ni + di, nj + dj]):
                break
            i, j, moved = ni, nj, True
            a[i, j] = 1
        if not moved:
            return a
        di, dj = dj, -di                                 # turn right


@functools.lru_cache(maxsize=None)
def image(H, W, pattern):
    """[H, W] int32."""
    i, j = np.arange(H)[:, None], np.arange(W)[None, :]
    rng = np.random.default_rng(2400 + 131 * H + 17 * W)
    if pattern == 'uniform':
        a = np.full((H, W), 1)
    elif pattern == 'checker':
        a = (i + j) % 2
    elif pattern == 'rows':
        a = i % 2 + 0 * j
    elif pattern == 'columns':
        a = j % 2 + 0 * i
    elif pattern == 'spiral':
        a = spiral(H, W)
    elif pattern == 'comb':                              # teeth on the even columns, joined only along the last row
        a = np.where((j % 2 == 0) | (i == H - 1), 1, 0)
    elif pattern == 'noise':                             # the site-percolation threshold of the square lattice
        a = (rng.random((H, W)) < 0.593).astype(np.int64)
    elif pattern == 'wide':
        a = np.array([-7, 0, 2 ** 31 - 1])[rng.integers(0, 3, (H, W))]
    else:
        raise KeyError(pattern)
    return _frozen(np.asarray(a).astype(np.int32))


@functools.lru_cache(maxsize=None)
def slic_image(H, W, S):
    """The float64 reference's SLIC image of the 8-band fp32 scene."""
    return _frozen(SR.slic(SC.scene(H, W, 8), H, W, S, SC.COMPACTNESS, SC.ITERATIONS)[0].astype(np.int32))


def kc(H, W, S):
    return int(np.prod(SR.grid(H, W, S)))


def auto_min_size(S):
    return max(1, S * S // 4)


# (name, H, W, n_labels, min_size): every label-image case
LABEL_CASES = [('%s' % p, H, W, n, m) for H, W in SIZES for p in PATTERNS for n, m in MERGES]
LABEL_CASES += [('slic%d' % S, H, W, kc(H, W, S), m) for H, W in SIZES for S in SLIC_S for m in (1, auto_min_size(S))]
LABEL_CASES += [('alternate', CHAIN[0], CHAIN[1], 0, 2)]

# The smallest checkerboard whose scans carry: 513 x 512 = 262,656 one-pixel components = 257 scan blocks of 1,024 cells, so the
# one-workgroup scan of the block totals goes round its 256-block loop twice.  min_size 1: R = 262,656, the dense ids cross the
# carry; min_size 2: one region, 262,655 absorbed, the deepest chain 1,023.  Not in SIZES: that would multiply every pattern.
CARRY = (513, 512)
CARRY_CASES = [('checker',) + CARRY + (0, 1), ('checker',) + CARRY + (0, 2)]
CARRY_STATS = {1: ((262656, 262656, 0), 0), 2: ((1, 262656, 262655), 1023)}       # min_size -> (stats, depth) of the reference


def labels_of(name, H, W):
    if name.startswith('slic'):
        return slic_image(H, W, int(name[4:]))
    if name == 'alternate':
        return _frozen((np.arange(W)[None, :] % 2 + np.zeros((H, 1), dtype=np.int64)).astype(np.int32))
    return image(H, W, name)


@functools.lru_cache(maxsize=None)
def components(name, H, W):
    return _frozen(R.components(labels_of(name, H, W)))


@functools.lru_cache(maxsize=None)
def reference(name, H, W, n_labels, min_size):
    """-> (comp, region, region_size, stats, depth), read-only."""
    comp = components(name, H, W)
    region, sizes, stats, depth = R.merge(labels_of(name, H, W), comp, n_labels, min_size)
    return comp, _frozen(region), _frozen(sizes), stats, depth


# the vote: the regions are the reference's of the S = 5 SLIC image at its auto min_size
def vote_inputs(H, W, K):
    """-> (prob [H, W, K] float32, mask [H, W] uint8, region [H, W] int32, R)."""
    S = 5
    region, sizes, _, _ = reference('slic%d' % S, H, W, kc(H, W, S), auto_min_size(S))[1:]
    prob = SR.softmax_rows(SC.logits(H, W, K)).reshape(H, W, K).astype(np.float32)
    return prob, SC.mask(H, W), region.astype(np.int32), len(sizes)


@functools.lru_cache(maxsize=None)
def vote_reference(H, W, K, mode):
    prob, mask, region, Rn = vote_inputs(H, W, K)
    return R.vote(prob, mask, region, Rn, mode)


VOTE_CASES = [(H, W, K) for H, W in VOTE_SIZES for K in VOTE_K]
