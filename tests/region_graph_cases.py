"""The cases of the spectrum-aware fragment merge, shared by tests/test_region_graph_host.py (the guards, on the
reference alone) and tests/test_gpu_region_graph.py.  A plain module: no GPU, nothing of the HIP library.  The references are
computed once per process and handed out read-only.

Label images: those of tests/regions_cases.py, every size with every pattern and the reference's SLIC images at S = 4, 5, 16.
(n_labels, min_size): (Kc, auto) and (Kc, 2) for SLIC; (0, 2), (2, 4) and (0, 1) for the patterns.  Scenes: the noisy fixture
scene of tests/segments_cases.py at 1, 3, 8 and 200 bands in fp32 and at 8 and 200 bands in fp16; a constant scene, where every
distance is 0 and the id alone decides; a scene with values outside [0, 1], an infinity and a NaN.  Every label case runs on every
scene.

Recorded on the reference alone (tests/test_region_graph_host.py asserts them), 8-band fp32 scene, min_size auto:
  * purity against segments_cases.ids, spectrum / position: PURITY below (64 x 65, S = 16: 0.346 / 0.254 with 43 regions in 2
    rounds against 20; 129 x 131, S = 16: 0.349 / 0.243 with 153 regions in 3 rounds against 82); over every SLIC case the
    spectrum rule is never below the positional one;
  * every size of more than one tile has a case of more than one round and a case where a group of fragments alone reaches
    min_size (R exceeds the number of initially kept components): MULTI_ROUND and GROWN name one each;
  * the SLIC cases on the noisy scenes meet no tie of distances; the constant scene's cases meet them in every case that has a
    fragment with two neighbours (the checkerboard at 129 x 131: 16,898 groups choose by id alone)."""
import functools

import numpy as np

import regions_cases as RC
import segments_cases as SC

import region_graph_ref as G

SIZES = RC.SIZES
MULTI_TILE = tuple(s for s in SIZES if max(s) > 16)
PATTERN_MERGES = ((0, 2), (2, 4), (0, 1))
SCENES = (('f32', 1), ('f32', 3), ('f32', 8), ('f32', 200), ('f16', 8), ('f16', 200), ('const', 3), ('wild', 3))
PITCH_EXTRA, ROWS_EXTRA = 3, 2                           # the device's scene is wider and taller than [H, W]
CHAIN = RC.CHAIN                                         # 1 x 4,096 alternating labels at min_size 2 on the constant scene
# The 513 x 512 checkerboard of regions_cases.CARRY on a constant one-band scene at min_size 1: no fragment, no round, and the
# second scan, over 262,656 components = 257 blocks, carries past 256 blocks.  (min_size 2 would cost the reference minutes.)
CARRY_CASE = RC.CARRY_CASES[0]
CARRY_SCENE = ('const', 1)
CARRY_STATS = (262656, 262656, 0, 0)

# (name, H, W, n_labels, min_size): every label-image case
LABEL_CASES = [(p, H, W, n, m) for H, W in SIZES for p in RC.PATTERNS for n, m in PATTERN_MERGES]
LABEL_CASES += [('slic%d' % S, H, W, RC.kc(H, W, S), m) for H, W in SIZES for S in RC.SLIC_S for m in (RC.auto_min_size(S), 2)]

# (H, W, S) -> (spectrum, position): the purity of the regions at min_size auto on the 8-band fp32 scene, to three places
PURITY = {(64, 65, 16): (0.346, 0.254), (129, 131, 16): (0.349, 0.243), (64, 65, 4): (1.000, 0.996), (13, 9, 4): (1.000, 0.974)}
STRICTLY_ABOVE = tuple(PURITY)
# (H, W) -> a case (name, n_labels, min_size) on the 8-band fp32 scene with more than one round / with R above the kept components
MULTI_ROUND = {(1, 70): ('slic16', 5, 64), (70, 1): ('slic16', 5, 64), (33, 17): ('slic5', 28, 6), (64, 65): ('slic16', 20, 64),
               (129, 131): ('slic16', 81, 64)}
GROWN = {(1, 70): ('noise', 0, 2), (70, 1): ('noise', 0, 2), (33, 17): ('noise', 0, 2), (64, 65): ('slic16', 20, 64),
         (129, 131): ('slic16', 81, 64)}


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def scene(kind, C, H, W):
    """[H, W, C] float32 or float16."""
    if kind == 'f32':
        return SC.scene(H, W, C)
    if kind == 'f16':
        return SC.scene(H, W, C, True)
    if kind == 'const':
        return _frozen(np.full((H, W, C), 0.25, dtype=np.float32))
    if kind == 'wild':                                   # values in [-1, 2]; a NaN and an infinity where the scene has room
        a = np.array(SC.scene(H, W, C)) * np.float32(3) - np.float32(1)
        a[H // 2, W // 2, 0] = np.nan
        a[H - 1, W - 1, C - 1] = np.inf
        a[0, W - 1, 0] = -np.inf
        return _frozen(a)
    raise KeyError(kind)


def padded(kind, C, H, W):
    """The scene as the device holds it: [H + ROWS_EXTRA, W + PITCH_EXTRA, C], the margin filled with a value no pixel has."""
    a = scene(kind, C, H, W)
    out = np.full((H + ROWS_EXTRA, W + PITCH_EXTRA, C), 0.75, dtype=a.dtype)
    out[:H, :W] = a
    return out


@functools.lru_cache(maxsize=None)
def reference(name, H, W, n_labels, min_size, kind, C):
    """-> (region, region_size, stats (R, components, components - R, rounds), info), read-only."""
    region, sizes, stats, info = G.merge(RC.labels_of(name, H, W), RC.components(name, H, W), np.asarray(scene(kind, C, H, W), dtype=np.float32),
                                         n_labels, min_size)
    return _frozen(region), _frozen(sizes), stats, info
