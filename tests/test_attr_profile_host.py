"""CPU: `band_profile: area` — utils.attribute.profile_host against the sequential union-find of tests/attr_ref.py
bit for bit (as uint32) on every case of tests/attr_cases.py, the consequences of the definition, the keys and their refusals, what
the C entry points decide before any launch, arch_from_cfg's band count, and the solvers on the drop-in path: `area` end to end,
and `morph` with the JSON keys and the messages it had before this kind existed."""
import copy
import ctypes as C
import json
import os
import shutil
import tempfile

import numpy as np
import pytest
import torch

import attr_cases as ac
import attr_ref as ar


def _at():
    from utils import attribute
    return attribute


# ---------------------------------------------------------------------------------------------- 1. the definition
@pytest.mark.parametrize('name', ac.NAMES)
def test_profile_host_equals_the_reference(name):
    at = _at()
    c = ac.cases()[name]
    want, _ = ar.case_profile(name)
    got, info = at.profile_host(c.scores, c.P, c.areas, c.L)
    K, n = c.scores.shape[2], len(c.areas)
    assert got.dtype == np.float32 and got.shape == c.scores.shape[:2] + (K + 2 * n * c.P,)
    assert np.array_equal(ar.bits(got), ar.bits(want))
    assert np.array_equal(ar.bits(got[:, :, c.P * (2 * n + 1):]), ar.bits(c.scores[:, :, c.P:]))      # the rest, -0 included
    assert not (ar.bits(got[:, :, :c.P * (2 * n + 1)]) == 0x80000000).any()                          # canonicalised
    assert info['route'] == 'host' and info['kind'] == 'area' and info['connectivity'] == 4 and info['levels'] == c.L
    assert info['areas'] == list(c.areas) and info['bands'] == got.shape[2] == len(info['order']) and len(info['range']) == c.P


@pytest.mark.parametrize('name', ac.NAMES)
def test_consequences_of_the_definition(name):
    """area 1 returns q itself; an area >= H W returns level 0 (opening) and L - 1 (closing) wherever the plane is not constant,
    and one > H W everywhere; gamma <= q <= phi; gamma falls and phi rises with the area."""
    at = _at()
    c = ac.cases()[name]
    H, W, _ = c.scores.shape
    for p in range(c.P):
        f = at.canonical(c.scores[:, :, p])
        lo, hi = at.plane_range(f)
        q = at.quantise(f, lo, hi, c.L)
        assert q.min() == 0 and q.max() == (c.L - 1 if hi > lo else 0)
        opened = at.area_open_counts(q, c.areas, c.L)
        closed = (c.L - 1) - at.area_open_counts((c.L - 1) - q, c.areas, c.L)
        for i, a in enumerate(c.areas):
            if a == 1:
                assert np.array_equal(opened[i], q) and np.array_equal(closed[i], q)
            if a > H * W or (a == H * W and hi > lo):
                assert not opened[i].any() and (closed[i] == c.L - 1).all()
            assert (opened[i] <= q).all() and (q <= closed[i]).all()
            if i > 0:
                assert (opened[i] <= opened[i - 1]).all() and (closed[i] >= closed[i - 1]).all()


def test_the_count_of_qualifying_levels_is_the_largest_one():
    """The sets {q >= t} are nested, so the levels that qualify at a pixel are 1 .. some t: their number is their maximum."""
    from scipy import ndimage
    at = _at()
    four = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], dtype=bool)
    for name in ('past_the_tile_17x33_L7', 'smooth_64x65', 'blobs_at_the_tile_corner', 'ties_67x131'):
        c = ac.cases()[name]
        f = at.canonical(c.scores[:, :, 0])
        q = at.quantise(f, *at.plane_range(f), c.L)
        for a in c.areas:
            largest = np.zeros(q.shape, dtype=np.int32)
            for t in range(1, c.L):
                lab, _ = ndimage.label(q >= t, structure=four)
                size = np.bincount(lab.ravel())
                size[0] = 0
                largest[size[lab] >= a] = t                                    # ascending: the last level that qualifies stays
            assert np.array_equal(largest, at.area_open(q, a, c.L)), (name, a)
            assert np.array_equal(largest, ar.case_profile(name)[1][(0, c.areas.index(a))][0]), (name, a)


def test_the_blobs_at_the_tile_corner():
    """The blob of area - 1 pixels is removed by the opening at that area, the blobs of area and area + 1 pixels stay."""
    at = _at()
    c = ac.cases()['blobs_at_the_tile_corner']
    got, _ = at.profile_host(c.scores, c.P, c.areas, c.L)
    n, i = len(c.areas), c.areas.index(ac.BLOB_AREA)
    for p, stays in enumerate((False, True, True)):
        opened = got[:, :, p * (2 * n + 1) + n + 1 + i]
        blob = [opened[y, x] for (y, x) in ac.BLOB_PATH[:ac.BLOB_AREA - 1 + p]]
        assert all(v > 0.5 for v in blob) if stays else all(v == 0 for v in blob), p
        assert opened[-1, -1] == 0                                             # the lone pixel never survives


def test_band_names_spell_the_order():
    at = _at()
    assert at.band_names(3, 1, (25, 100, 400)) == ['pc1_aclose_a400', 'pc1_aclose_a100', 'pc1_aclose_a25', 'pc1', 'pc1_aopen_a25',
                                                   'pc1_aopen_a100', 'pc1_aopen_a400', 'pc2', 'pc3']
    assert len(at.band_names(8, 4, (25, 100, 400))) == at.band_count(8, 4, 3) == 32


# ---------------------------------------------------------------------------------------------- 2. keys, arch, entry points
def _arch_cfg(**over):
    cfg = {'DATA_DICT': {'x': {'size': [40, 40, 24]}}, 'data_city': 'x', 'patch_size': 11, 'Categories_Number': 5, 'scale': 1}
    cfg.update(over)
    return cfg


def test_arch_from_cfg_counts_the_profile_bands():
    from dmf.arch import arch_from_cfg
    a = arch_from_cfg(_arch_cfg(band_reduce='pca', band_reduce_bands=8, band_profile='area'))
    assert a['C'] == 32 and a['G'] == 2                                      # the defaults: P = 4, areas [25, 100, 400]
    a = arch_from_cfg(_arch_cfg(band_reduce='pca', band_reduce_bands=6, band_profile='area', band_profile_components=2,
                                band_profile_areas=[1, 2, 3, 5, 8], band_profile_radii=[1, 2]))
    assert a['C'] == 6 + 2 * 5 * 2                                           # n from the areas, not from the radii
    a = arch_from_cfg(_arch_cfg(band_reduce='pca', band_reduce_bands=6, band_profile='morph', band_profile_components=2,
                                band_profile_areas=[1, 2, 3, 5, 8], band_profile_radii=[1, 2]))
    assert a['C'] == 6 + 2 * 2 * 2                                           # and morph as before


def test_keys_and_their_refusals():
    from utils import morphology
    at = _at()
    assert at.profile_keys({}) is None and at.profile_keys({'band_profile': 'none', 'band_profile_areas': 'junk'}) is None
    on = {'band_reduce': 'pca', 'band_reduce_bands': 8, 'band_profile': 'area'}
    assert at.profile_keys(on) == dict(kind='area', components=4, areas=(25, 100, 400), levels=256)
    assert at.profile_keys(dict(on, band_profile_components=8, band_profile_areas=[1, 2 ** 31 - 1], band_profile_levels=2)) \
        == dict(kind='area', components=8, areas=(1, 2 ** 31 - 1), levels=2)
    assert morphology.profile_keys(on) is None                                # morph's parser leaves the kind to this one
    assert at.profile_keys(dict(on, band_profile='morph')) is None           # .. and the other way round
    assert morphology.profile_keys(dict(on, band_profile='morph')) == dict(components=4, radii=(2, 4, 6))
    with pytest.raises(ValueError, match='band_profile: area profiles the components of band_reduce: pca, and band_reduce is none'):
        at.profile_keys({'band_profile': 'area'})
    for parse in (at.profile_keys, morphology.profile_keys):
        with pytest.raises(ValueError, match="band_profile 'disk' is not one of none / morph / area$"):
            parse(dict(on, band_profile='disk'))
    with pytest.raises(ValueError, match='band_profile_components: 9 exceeds the 8 components'):
        at.profile_keys(dict(on, band_profile_components=9))
    with pytest.raises(ValueError, match='band_profile_components 0 is not a whole number >= 1'):
        at.profile_keys(dict(on, band_profile_components=0))
    with pytest.raises(ValueError, match='band_profile_areas .* is not strictly increasing'):
        at.profile_keys(dict(on, band_profile_areas=[25, 25, 100]))
    for bad in ([0, 3], [25, 2 ** 31], [2.5, 3], [True, 3]):
        with pytest.raises(ValueError, match='band_profile_areas .* every area is a whole number >= 1 and < 2\\^31'):
            at.profile_keys(dict(on, band_profile_areas=bad))
    for bad in ([], list(range(1, 10)), 'abc', 25):
        with pytest.raises(ValueError, match='band_profile_areas .* is not a list of 1..8 whole numbers'):
            at.profile_keys(dict(on, band_profile_areas=bad))
    for bad in (1, 257, 16.0, True):
        with pytest.raises(ValueError, match='band_profile_levels .* is not a whole number in 2..256'):
            at.profile_keys(dict(on, band_profile_levels=bad))


def test_scores_that_are_refused():
    at = _at()
    s = ac.cases()['past_the_tile_17x33_L7'].scores.copy()
    with pytest.raises(ValueError, match='band_profile_components: 4 exceeds the 3 components'):
        at.profile_host(s, 4, (1, 2))
    with pytest.raises(ValueError, match='band_profile_levels 300 is not a whole number in 2..256'):
        at.profile_host(s, 1, (1, 2), 300)
    s[5, 6, 2] = np.nan                                                    # even in a component that is not profiled
    with pytest.raises(ValueError, match='band_profile: the scores hold a value that is not finite'):
        at.profile_host(s, 1, (1, 2))
    s[5, 6, 2] = -np.inf
    with pytest.raises(ValueError, match='not finite'):
        at.profile_host(s, 1, (1, 2))
    with pytest.raises(ValueError, match='band_profile wants the float32 scores'):
        at.profile_host(s.astype(np.float64), 1, (1, 2))


_BUF = C.create_string_buffer(4096)
PTR = C.c_void_p((C.addressof(_BUF) + 63) // 64 * 64)          # a non-null, aligned pointer that no refusal dereferences
ODD = C.c_void_p(PTR.value + 2)


def _areas(*a):
    return (C.c_int32 * len(a))(*a)


def test_the_library_declares_the_entry_points_and_sizes_the_workspace():
    from dmf import lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'dmf.h')).read()
    so = C.CDLL(lib.LIB_PATH)
    for name in ('dmf_attr_workspace_bytes', 'dmf_attr_quantise', 'dmf_attr_area_levels', 'dmf_attr_stack'):
        assert name + '(' in hdr and name in lib.EXPORTS and hasattr(so, name), name
    up16 = lambda v: (v + 15) // 16 * 16                                     # noqa: E731
    for (H, W, P, n, T) in ((67, 131, 4, 3, 16), (1, 1, 1, 1, 1), (5, 7, 3, 8, 5), (512, 512, 64, 8, 16)):
        assert lib.attr_workspace_bytes(H, W, P, n, T) == up16(8 * P) + 2 * up16(2 * P * T * H * W * 4)      # the carve include/dmf.h states
    for bad in ((0, 5, 1, 1, 1), (5, 0, 1, 1, 1), (5, 5, 0, 1, 1), (5, 5, 65, 1, 1), (5, 5, 1, 0, 1), (5, 5, 1, 9, 1), (5, 5, 1, 1, 0),
                (5, 5, 1, 1, 17), (1 << 16, 1 << 15, 1, 1, 1)):
        with pytest.raises(lib.DmfError, match='dmf_attr_workspace_bytes'):
            lib.attr_workspace_bytes(*bad)


def _levels(**kw):
    a = dict(q=PTR, H=9, W=11, P=2, areas=_areas(1, 5), n=2, L=256, first=1, levels=4, T=4, count=C.c_void_p(PTR.value + 1024),
             ws=C.c_void_p(PTR.value + 2048), ws_bytes=1 << 40)
    a.update(kw)
    from dmf import lib
    return lib._lib.dmf_attr_area_levels(a['q'], a['H'], a['W'], a['P'], a['areas'], a['n'], a['L'], a['first'], a['levels'], a['T'],
                                         a['count'], a['ws'], a['ws_bytes'], None)


def _quantise(**kw):
    a = dict(scores=PTR, H=9, W=11, K=3, pitch=3, P=2, L=256, q=C.c_void_p(PTR.value + 2048), rng=C.c_void_p(PTR.value + 3072),
             ws=C.c_void_p(PTR.value + 3584), ws_bytes=64)
    a.update(kw)
    from dmf import lib
    return lib._lib.dmf_attr_quantise(a['scores'], a['H'], a['W'], a['K'], a['pitch'], a['P'], a['L'], a['q'], a['rng'], a['ws'],
                                      a['ws_bytes'], None)


def _stack(**kw):
    a = dict(scores=PTR, H=2, W=2, K=3, pitch=3, P=2, n=2, L=256, count=C.c_void_p(PTR.value + 256), rng=C.c_void_p(PTR.value + 512),
             out=C.c_void_p(PTR.value + 1024))
    a.update(kw)
    from dmf import lib
    return lib._lib.dmf_attr_stack(a['scores'], a['H'], a['W'], a['K'], a['pitch'], a['P'], a['n'], a['L'], a['count'], a['rng'],
                                   a['out'], None)


REFUSALS = [
    ('levels: NULL q', lambda: _levels(q=None), 1), ('levels: NULL areas', lambda: _levels(areas=None), 1),
    ('levels: NULL count', lambda: _levels(count=None), 1), ('levels: NULL workspace', lambda: _levels(ws=None), 1),
    ('levels: H 0', lambda: _levels(H=0), 2), ('levels: 2^31 pixels', lambda: _levels(H=1 << 16, W=1 << 15), 2),
    ('levels: P 0', lambda: _levels(P=0), 3), ('levels: P 65', lambda: _levels(P=65), 3),
    ('levels: n 0', lambda: _levels(n=0), 4), ('levels: n 9', lambda: _levels(n=9), 4),
    ('levels: area 0', lambda: _levels(areas=_areas(0, 5)), 4), ('levels: equal areas', lambda: _levels(areas=_areas(5, 5)), 4),
    ('levels: falling areas', lambda: _levels(areas=_areas(5, 4)), 4), ('levels: a negative area', lambda: _levels(areas=_areas(-3, 4)), 4),
    ('levels: L 1', lambda: _levels(L=1), 11), ('levels: L 257', lambda: _levels(L=257), 11),
    ('levels: first 0', lambda: _levels(first=0), 10), ('levels: levels 0', lambda: _levels(levels=0), 10),
    ('levels: levels > T', lambda: _levels(levels=5), 10), ('levels: T 17', lambda: _levels(T=17, levels=17), 10),
    ('levels: past L - 1', lambda: _levels(first=253), 10), ('levels: L 2, level 2', lambda: _levels(L=2, first=2, levels=1), 10),
    ('levels: a small workspace', lambda: _levels(ws_bytes=16 + 2 * (2 * 2 * 4 * 99 * 4) - 1), 12),
    ('levels: a misaligned workspace', lambda: _levels(ws=C.c_void_p(PTR.value + 2056)), 6),
    ('levels: count inside the workspace', lambda: _levels(count=C.c_void_p(PTR.value + 2048 + 64)), 7),
    ('levels: count over q', lambda: _levels(count=C.c_void_p(PTR.value + 100)), 7),
    ('quantise: NULL scores', lambda: _quantise(scores=None), 1), ('quantise: NULL range', lambda: _quantise(rng=None), 1),
    ('quantise: W 0', lambda: _quantise(W=0), 2), ('quantise: K 65', lambda: _quantise(K=65, pitch=65), 3),
    ('quantise: P > K', lambda: _quantise(P=4), 3), ('quantise: pitch < K', lambda: _quantise(pitch=2), 5),
    ('quantise: L 1', lambda: _quantise(L=1), 11), ('quantise: L 257', lambda: _quantise(L=257), 11),
    ('quantise: a small workspace', lambda: _quantise(ws_bytes=15), 12), ('quantise: misaligned scores', lambda: _quantise(scores=ODD), 6),
    ('quantise: q over the scores', lambda: _quantise(q=C.c_void_p(PTR.value + 64)), 7),
    ('stack: NULL out', lambda: _stack(out=None), 1), ('stack: H 0', lambda: _stack(H=0), 2), ('stack: P 0', lambda: _stack(P=0), 3),
    ('stack: n 9', lambda: _stack(n=9), 4), ('stack: pitch < K', lambda: _stack(pitch=1), 5), ('stack: L 300', lambda: _stack(L=300), 11),
    ('stack: misaligned out', lambda: _stack(out=C.c_void_p(PTR.value + 1026)), 6), ('stack: out over the scores', lambda: _stack(out=PTR), 7),
    ('stack: out over count', lambda: _stack(out=C.c_void_p(PTR.value + 240)), 7),
]


@pytest.mark.parametrize('name,call,code', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_the_entry_points_refuse_before_any_launch(name, call, code):
    """Bad sizes and NULL or overlapping pointers into a host buffer: every call returns its code without touching the device."""
    from dmf import lib
    assert call() == code and code in lib._ATTR_ERRORS


# ---------------------------------------------------------------------------------------------- 3. the solvers
def _cfg(golden_dir, tmp, **over):
    import pca_cases as pca
    from test_gpu_trajectory import _setup
    _, cfg = _setup(golden_dir, tmp, device='cpu', fast_path=0, scale=1, epoch=1, **over)
    primary, aux, label = pca.solver_scene(cfg['Categories_Number'])
    d = cfg['data_address']
    np.save(d + 'ms4.tif.npy', primary); np.save(d + 'pan.tif.npy', aux); np.save(d + 'label.npy', label)
    cfg['DATA_DICT'][cfg['data_city']]['size'] = [40, 40, pca.SOLVER_BANDS]
    return cfg


def test_base_solver_with_the_kind_on_the_drop_in_path(golden_dir, capsys):
    import pca_cases as pca
    from dmf.arch import arch_from_cfg
    from solver.mainsolver import Solver
    from utils import spectral
    at = _at()
    tmp = tempfile.mkdtemp(prefix='dmf_attr_')
    try:
        cfg = _cfg(golden_dir, tmp, band_reduce='pca', band_reduce_bands=4, band_profile='area', band_profile_components=2,
                   band_profile_areas=[3, 30], band_profile_levels=64)
        torch.manual_seed(3407)
        s = Solver(cfg)
        reduced, _ = spectral.reduce_host(pca.solver_scene(cfg['Categories_Number'])[0], 4)
        want, _ = at.profile_host(reduced, 2, (3, 30), 64)
        assert s.ms.shape == (40, 40, 12) and s.ms.dtype == np.float32 and np.array_equal(ar.bits(s.ms), ar.bits(want))
        assert np.array_equal(ar.bits(want), ar.bits(ar.profile_uncached(reduced, 2, (3, 30), 64)[0]))
        assert arch_from_cfg(cfg)['C'] == 12 and s.MS.shape[2] == 12
        line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('band_profile:')]
        assert len(line) == 1 and 'area' in line[0] and '12 bands' in line[0] and line[0].endswith('host')
        info = json.load(open(cfg['RESULT_output'] + '0_band_profile.json'))
        assert set(info) == {'kind', 'components', 'areas', 'levels', 'connectivity', 'range', 'bands', 'order', 'route'}
        assert info['order'] == at.band_names(4, 2, (3, 30)) and len(info['order']) == info['bands'] == 12
        assert info['kind'] == 'area' and info['components'] == 2 and info['areas'] == [3, 30] and info['levels'] == 64
        assert info['connectivity'] == 4 and info['route'] == 'host'
        assert info['range'] == [[float(reduced[:, :, p].min()), float(reduced[:, :, p].max())] for p in range(2)]
    finally:
        shutil.rmtree(tmp)


def test_a_morph_run_keeps_its_file_and_its_messages(golden_dir, capsys):
    """With `band_profile: morph` the JSON file has the keys it had, the line printed is the one it was, and the refusals read
    as they did."""
    from solver.mainsolver import Solver
    from utils import morphology
    tmp = tempfile.mkdtemp(prefix='dmf_attr_')
    try:
        cfg = _cfg(golden_dir, os.path.join(tmp, 'a'), band_reduce='pca', band_reduce_bands=4, band_profile='morph',
                   band_profile_components=2, band_profile_radii=[1, 3], band_profile_areas=[5], band_profile_levels=9)
        torch.manual_seed(3407)
        s = Solver(cfg)
        info = json.load(open(cfg['RESULT_output'] + '0_band_profile.json'))
        assert list(info) == ['components', 'radii', 'bands', 'order', 'route', 'rounds']
        assert info == s.band_profile_info and info['order'] == morphology.band_names(4, 2, (1, 3))
        line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('band_profile:')]
        assert line == ['band_profile: 2 components at radii [1, 3], 12 bands, %d reconstruction rounds, host' % sum(info['rounds'])]
        cfg = _cfg(golden_dir, os.path.join(tmp, 'b'), band_profile='morph')
        with pytest.raises(ValueError, match='^band_profile: morph profiles the components of band_reduce: pca, and band_reduce is none$'):
            Solver(cfg)
    finally:
        shutil.rmtree(tmp)


def test_refusals_of_the_kind_in_the_solvers(golden_dir):
    from solver.mainsolver import Solver
    from solver.tostagesolver import toStageSolver
    tmp = tempfile.mkdtemp(prefix='dmf_attr_')
    try:
        cfg = _cfg(golden_dir, os.path.join(tmp, 'a'), band_profile='area')                   # band_reduce: none
        with pytest.raises(ValueError, match='band_profile: area profiles the components of band_reduce: pca'):
            Solver(cfg)
        cfg = _cfg(golden_dir, os.path.join(tmp, 'b'), band_reduce='pca', band_reduce_bands=4, band_profile='area')
        with pytest.raises(ValueError, match='band_profile is out of scope for toStageSolver'):
            toStageSolver(copy.deepcopy(cfg))
        cfg = _cfg(golden_dir, os.path.join(tmp, 'c'), band_reduce='pca', band_reduce_bands=4, band_profile='area',
                   band_profile_components=5)
        with pytest.raises(ValueError, match='band_profile_components: 5 exceeds the 4 components'):
            Solver(cfg)
        cfg = _cfg(golden_dir, os.path.join(tmp, 'd'), band_reduce='pca', band_reduce_bands=4, band_profile='area',
                   band_profile_areas=[30, 3])
        with pytest.raises(ValueError, match='not strictly increasing'):
            Solver(cfg)
        cfg = _cfg(golden_dir, os.path.join(tmp, 'e'), band_reduce='pca', band_reduce_bands=4, band_profile='area',
                   band_profile_levels=1000)
        with pytest.raises(ValueError, match='band_profile_levels 1000 is not a whole number in 2..256'):
            Solver(cfg)
        cfg = _cfg(golden_dir, os.path.join(tmp, 'f'), band_reduce='pca', band_reduce_bands=4, band_profile='disk')
        with pytest.raises(ValueError, match="band_profile 'disk' is not one of none / morph / area"):
            Solver(cfg)
        for sub in 'bcdef':                                                  # refused before any work
            assert not os.path.exists(os.path.join(tmp, sub, 'out', '0_band_reduce.npz'))
    finally:
        shutil.rmtree(tmp)
