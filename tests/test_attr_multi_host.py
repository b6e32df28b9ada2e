"""CPU: `band_profile: area` with `band_profile_diagonals` / `band_profile_stds` — the keys and their refusals,
arch_from_cfg's band count and the band names, utils.attribute.profile_host against the sequential union-find of
tests/attr_multi_ref.py bit for bit (as uint32) on every case of tests/attr_multi_cases.py, the hand-written expectations, the
consequences of the definition, today's bytes and JSON keys with both lists empty, csrc/dmf_attr_criteria.h at its extremes under
the host compiler against Python's integers, and what the new entry points decide before any launch."""
import ctypes as C
import json
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import attr_cases as ac
import attr_multi_cases as amc
import attr_multi_ref as amr
import attr_ref as ar

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ON = {'band_reduce': 'pca', 'band_reduce_bands': 8, 'band_profile': 'area'}


def _at():
    from utils import attribute
    return attribute


def _planes(c, p):
    """(q, opened [n, H, W], closed [n, H, W]) of component p of case c by the numpy route."""
    at = _at()
    f = at.canonical(c.scores[:, :, p])
    q = at.quantise(f, *at.plane_range(f), c.L)
    opened = at.open_counts(q, c.areas, c.diagonals, c.stds, c.L)
    closed = (c.L - 1) - at.open_counts((c.L - 1) - q, c.areas, c.diagonals, c.stds, c.L)
    return q, opened, closed


# ---------------------------------------------------------------------------------------------- 1. keys, arch, names
def test_keys_defaults_and_refusals():
    at = _at()
    assert at.profile_keys(ON) == dict(kind='area', components=4, areas=(25, 100, 400), levels=256)          # absent: today's dict
    assert at.profile_keys(dict(ON, band_profile_diagonals=[], band_profile_stds=None)) == at.profile_keys(ON)   # empty: as absent
    keys = at.profile_keys(dict(ON, band_profile_areas=[100], band_profile_diagonals=[20], band_profile_stds=[20]))
    assert keys == dict(kind='area', components=4, areas=(100,), levels=256, diagonals=(20,), stds=(20,))
    assert at.profile_keys(dict(ON, band_profile_diagonals=[1, 2 ** 31 - 1]))['stds'] == ()
    assert at.profile_keys(dict(ON, band_profile_levels=7, band_profile_stds=[1, 6]))['stds'] == (1, 6)
    for key in ('band_profile_diagonals', 'band_profile_stds'):
        with pytest.raises(ValueError, match='%s .* is not strictly increasing' % key):
            at.profile_keys(dict(ON, **{key: [5, 5]}))
        for bad in ('abc', 25, list(range(1, 9))):
            with pytest.raises(ValueError, match='%s .* is not a list of 0..7 whole numbers' % key):
                at.profile_keys(dict(ON, **{key: bad}))
        for kind in ('morph', 'none'):
            with pytest.raises(ValueError, match='^%s needs band_profile: area, and band_profile is %s$' % (key, kind)):
                at.profile_keys(dict(ON, band_profile=kind, **{key: [3]}))
        with pytest.raises(ValueError, match='^%s needs band_profile: area, and band_profile is none$' % key):
            at.profile_keys({key: [3]})
        assert at.profile_keys(dict(ON, band_profile='morph', **{key: []})) is None                        # empty: nothing to refuse
    for bad in ([0, 3], [3, 2 ** 31], [2.5], [True]):
        with pytest.raises(ValueError, match='band_profile_diagonals .* every value is a whole number >= 1 and < 2\\^31'):
            at.profile_keys(dict(ON, band_profile_diagonals=bad))
    for bad in ([0, 3], [3, 256], [2.5], [True]):
        with pytest.raises(ValueError, match='band_profile_stds .* every value is a whole number >= 1 and <= band_profile_levels - 1 = 255'):
            at.profile_keys(dict(ON, band_profile_stds=bad))
    with pytest.raises(ValueError, match='band_profile_stds .* <= band_profile_levels - 1 = 6'):
        at.profile_keys(dict(ON, band_profile_levels=7, band_profile_stds=[7]))
    with pytest.raises(ValueError, match='band_profile_areas \\+ band_profile_diagonals \\+ band_profile_stds: 3 \\+ 3 \\+ 3 thresholds are more than 8'):
        at.profile_keys(dict(ON, band_profile_diagonals=[1, 2, 3], band_profile_stds=[1, 2, 3]))
    assert len(at.check_thresholds((1, 2), (1, 2, 3), (1, 2, 3), 256)) == 3                                    # n = 8 is allowed


def test_stds_on_a_plane_past_2_22_pixels_are_refused_before_any_work():
    at = _at()
    with pytest.raises(ValueError, match='band_profile_stds: 2049 x 2048 pixels are more than 2\\^22'):
        at.check_std_extent(2049, 2048, (3,))
    at.check_std_extent(2048, 2048, (3,))
    at.check_std_extent(1 << 15, 1 << 15, ())                                # no std: the limit is not this one
    big = np.broadcast_to(np.zeros((1, 1, 1), dtype=np.float32), (2049, 2048, 1))
    with pytest.raises(ValueError, match='band_profile_stds: 2049 x 2048 pixels are more than 2\\^22'):
        at.profile_host(big, 1, (1,), 4, stds=(1,))


def _arch_cfg(**over):
    cfg = {'DATA_DICT': {'x': {'size': [40, 40, 24]}}, 'data_city': 'x', 'patch_size': 11, 'Categories_Number': 5, 'scale': 1}
    cfg.update(over)
    return cfg


def test_arch_from_cfg_counts_every_threshold_and_the_names_spell_the_order():
    from dmf.arch import arch_from_cfg
    at = _at()
    a = arch_from_cfg(_arch_cfg(band_reduce='pca', band_reduce_bands=8, band_profile='area', band_profile_areas=[100],
                                band_profile_diagonals=[20], band_profile_stds=[20]))
    assert a['C'] == 32 and a['G'] == 2                                      # the shipped row: 8 + 2 * 3 * 4
    a = arch_from_cfg(_arch_cfg(band_reduce='pca', band_reduce_bands=6, band_profile='area', band_profile_components=2,
                                band_profile_diagonals=[5, 9], band_profile_stds=[]))
    assert a['C'] == 6 + 2 * (3 + 2) * 2                                     # the default areas and two diagonals
    a = arch_from_cfg(_arch_cfg(band_reduce='pca', band_reduce_bands=6, band_profile='morph', band_profile_components=2,
                                band_profile_diagonals=[5, 9], band_profile_radii=[1, 2]))
    assert a['C'] == 6 + 2 * 2 * 2                                           # morph does not count them
    assert at.band_names(3, 1, (25,), (20,), (7,)) == ['pc1_aclose_s7', 'pc1_aclose_d20', 'pc1_aclose_a25', 'pc1', 'pc1_aopen_a25',
                                                       'pc1_aopen_d20', 'pc1_aopen_s7', 'pc2', 'pc3']
    assert at.band_names(3, 1, (25, 100)) == at.band_names(3, 1, (25, 100), (), ())
    assert len(at.band_names(8, 4, (100,), (20,), (20,))) == at.band_count(8, 4, 3) == 32


# ---------------------------------------------------------------------------------------------- 2. the definition
@pytest.mark.parametrize('name', amc.NAMES)
def test_profile_host_equals_the_reference(name):
    at = _at()
    c = amc.cases()[name]
    want, _ = amr.case_profile(name)
    got, info = at.profile_host(c.scores, c.P, c.areas, c.L, c.diagonals, c.stds)
    K, n = c.scores.shape[2], len(c.areas) + len(c.diagonals) + len(c.stds)
    assert got.dtype == np.float32 and got.shape == c.scores.shape[:2] + (K + 2 * n * c.P,)
    assert np.array_equal(ar.bits(got), ar.bits(want))
    assert np.array_equal(ar.bits(got[:, :, c.P * (2 * n + 1):]), ar.bits(c.scores[:, :, c.P:]))      # the rest, -0 included
    assert info['route'] == 'host' and info['areas'] == list(c.areas) and info['diagonals'] == list(c.diagonals)
    assert info['stds'] == list(c.stds) and info['rule'] == 'qualifying levels (max rule for area and diagonal, subtractive for std)'
    assert info['bands'] == got.shape[2] == len(info['order']) and info['order'] == at.band_names(K, c.P, c.areas, c.diagonals, c.stds)


def test_the_cases_hold_what_the_issue_lists():
    cs = amc.cases().values()
    assert {c.scores.shape[:2] for c in cs} >= {(1, 40), (40, 1), (5, 4), (17, 33), (33, 34), (67, 131)}
    assert {c.L for c in cs if c.scores.shape[:2] == (17, 33)} == {2, 7, 256}
    assert sum(len(c.areas) + len(c.diagonals) + len(c.stds) == 8 for c in cs) >= 1
    assert any(set(c.areas) == {1, 50} for c in cs) and any(set(c.diagonals) == {1, 6, 40, amc.ABOVE} for c in cs)
    assert any(set(c.stds) == {1, 3, c.L - 1} for c in cs)
    assert all(amc.ABOVE ** 2 > c.scores.shape[0] ** 2 + c.scores.shape[1] ** 2 for c in cs)


@pytest.mark.parametrize('name', amc.NAMES)
def test_consequences_of_the_definition(name):
    """0 <= gamma <= q <= phi <= L - 1; gamma falls and phi rises along the thresholds of one attribute; diagonal 1 and area 1
    return q; a diagonal above the image's returns level 0 / L - 1; for area and diagonal gamma is the largest qualifying level."""
    from scipy import ndimage
    c = amc.cases()[name]
    H, W, _ = c.scores.shape
    na, nd = len(c.areas), len(c.diagonals)
    kinds = [('a', a) for a in c.areas] + [('d', d) for d in c.diagonals] + [('s', s) for s in c.stds]
    four = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], dtype=bool)
    for p in range(c.P):
        q, opened, closed = _planes(c, p)
        for i, (kind, tau) in enumerate(kinds):
            assert (0 <= opened[i]).all() and (opened[i] <= q).all() and (q <= closed[i]).all() and (closed[i] <= c.L - 1).all()
            if i > 0 and kinds[i - 1][0] == kind:
                assert (opened[i] <= opened[i - 1]).all() and (closed[i] >= closed[i - 1]).all(), (kind, tau)
            if kind in 'ad' and tau == 1:
                assert np.array_equal(opened[i], q) and np.array_equal(closed[i], q)
            if kind == 'd' and tau * tau > H * H + W * W:
                assert not opened[i].any() and (closed[i] == c.L - 1).all()
            if kind in 'ad' and c.L <= 7:                                  # the max rule, level by level (small L: it is a check of a rule)
                largest = np.zeros(q.shape, dtype=np.int32)
                for t in range(1, c.L):
                    lab, found = ndimage.label(q >= t, structure=four)
                    for k, box in enumerate(ndimage.find_objects(lab), start=1):
                        h, w = box[0].stop - box[0].start, box[1].stop - box[1].start
                        size = int((lab[box] == k).sum())
                        if (size >= tau) if kind == 'a' else (w * w + h * h >= tau * tau):
                            largest[lab == k] = t
                assert np.array_equal(largest, opened[i]), (kind, tau)
        assert i + 1 == na + nd + len(c.stds)


def test_a_constant_plane_has_no_level_for_any_std():
    c = amc.cases()['constant_9x11']
    q, opened, closed = _planes(c, 0)
    assert not q.any()
    for i in range(len(c.areas) + len(c.diagonals), opened.shape[0]):
        assert not opened[i].any() and (closed[i] == c.L - 1).all()


def test_the_ring_area_and_diagonal_disagree_as_written_out():
    c = amc.cases()['ring_at_the_tile_corner_33x34']
    q, opened, closed = _planes(c, 0)
    _, levels = amr.case_profile(c.name)
    kinds = [('a', a) for a in c.areas] + [('d', d) for d in c.diagonals] + [('s', s) for s in c.stds]
    assert set(kinds) == set(amc.RING_EXPECTED)
    for i, key in enumerate(kinds):
        for region, mask in amc.ring_regions().items():
            want_open, want_close = amc.RING_EXPECTED[key][region]
            for got_open, got_close in ((opened[i], closed[i]), levels[(0, i)]):
                assert (got_open[mask] == want_open).all() and (got_close[mask] == want_close).all(), (key, region)
    ring = amc.ring_regions()['ring']
    assert (opened[0][ring] == 0).all() and (opened[1][ring] == 3).all()       # small area, large diagonal


def test_the_std_staircase_is_subtractive_and_not_the_max_rule():
    from scipy import ndimage
    c = amc.cases()['std_staircase_12x20']
    q, opened, _ = _planes(c, 0)
    _, levels = amr.case_profile(c.name)
    assert np.array_equal(q, amc.staircase().astype(np.int32))                  # the quantiser is the identity here
    first_std = len(c.areas) + len(c.diagonals)
    for i, s in enumerate(c.stds):
        for region, mask in amc.stair_regions().items():
            want = amc.STAIR_EXPECTED[('s', s)][region]
            assert (opened[first_std + i][mask] == want).all() and (levels[(0, first_std + i)][0][mask] == want).all(), (s, region)
    four = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], dtype=bool)             # the max rule for std 1 on the plateau, level by level
    plateau, largest = amc.stair_regions()['plateau'], 0
    for t in range(1, c.L):
        lab, _ = ndimage.label(q >= t, structure=four)
        k = lab[plateau][0]
        if k and all((lab[plateau] == k)):
            vals = [int(v) for v in q[lab == k]]
            if len(vals) * sum(v * v for v in vals) - sum(vals) ** 2 >= len(vals) ** 2:
                largest = t
    assert largest == amc.STAIR_EXPECTED[('s', 1)]['largest_qualifying_level'] == 3 != amc.STAIR_EXPECTED[('s', 1)]['plateau']


def test_with_both_lists_empty_profile_host_and_its_info_are_todays():
    at = _at()
    for name in ('past_the_tile_17x33_L7', 'blobs_at_the_tile_corner', 'signed_zeros_18x19'):
        c = ac.cases()[name]
        want, winfo = ar.case_profile(name)[0], at.make_info(c.scores.shape[2], c.P, c.areas, c.L, [[0, 1]] * c.P, 'host')
        for more in ({}, dict(diagonals=(), stds=()), dict(diagonals=[], stds=[])):
            got, info = at.profile_host(c.scores, c.P, c.areas, c.L, **more)
            assert got.tobytes() == np.asarray(want).tobytes()
            assert list(info) == list(winfo) == ['kind', 'components', 'areas', 'levels', 'connectivity', 'range', 'bands', 'order', 'route']
    q = np.arange(12, dtype=np.int32).reshape(3, 4) % 5
    assert np.array_equal(at.open_counts(q, (1, 3), (), (), 5), at.area_open_counts(q, (1, 3), 5))


# ---------------------------------------------------------------------------------------------- 3. the criteria header
@pytest.fixture(scope='module')
def criteria(tmp_path_factory):
    cxx = next((c for c in (shutil.which('c++'), shutil.which('g++'), shutil.which('clang++'), '/opt/rocm/llvm/bin/clang++',
                            '/opt/rocm/lib/llvm/bin/clang++') if c and os.path.exists(c)), None)
    assert cxx is not None, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('ac') / 'attr_criteria_check')
    subprocess.run([cxx, '-std=c++17', '-O1', os.path.join(REPO, 'tests', 'attr_criteria_check.cpp'), '-o', exe], check=True)

    def run(cases):
        out = subprocess.run([exe] + [' '.join(str(v) for v in c) for c in cases], check=True, capture_output=True, text=True).stdout
        got = [int(t) for t in out.split()]
        assert len(got) == len(cases)
        return got
    return run


def test_the_criteria_header_at_its_extremes_against_python_integers(criteria):
    """|S| = 2^22 with half 0 and half 255 (the largest variance and the largest products), |S| = 1, a box of 1 x (2^31 - 1), tau at
    its bounds, and the ties one either side."""
    N, top = 1 << 22, (1 << 31) - 1
    cases = []
    for size, tau in ((1, 1), (1, 2), (top, top), (top - 1, top), (top, 1), (50, 50), (49, 50)):
        cases.append(('area', size, tau))
    for box in ((0, 0, 0, top - 1), (0, top - 1, 0, 0), (5, 5, 7, 7), (0, 11, 0, 11), (10, 21, 10, 21), (0, 46340, 0, 46340)):
        for tau in (1, 2, 16, 17, 65536, top - 1, top):
            cases.append(('diag',) + box + (tau,))
    half = (N, (N // 2) * 255, (N // 2) * 255 * 255)                          # variance 127.5^2
    flat = (N, N * 255, N * 255 * 255)                                        # every pixel 255: the largest sums, variance 0
    for size, sq, sq2 in (half, flat, (1, 0, 0), (1, 255, 255 * 255), (18, 72, 306), (239, 293, 527), (2, 255, 255 * 255)):
        for tau in (1, 2, 127, 128, 255):
            cases.append(('std', size, sq, sq2, tau))
    want = []
    for c in cases:
        if c[0] == 'area':
            want.append(int(c[1] >= c[2]))
        elif c[0] == 'diag':
            w, h = c[2] - c[1] + 1, c[4] - c[3] + 1
            want.append(int(w * w + h * h >= c[5] * c[5]))
        else:
            want.append(int(c[1] * c[3] - c[2] * c[2] >= c[4] * c[4] * c[1] * c[1]))
            assert max(c[1] * c[3], c[2] * c[2], c[4] * c[4] * c[1] * c[1]) <= 1 << 60        # the header's overflow argument
    assert criteria(cases) == want
    assert 0 < sum(want) < len(want)
    assert want[cases.index(('std',) + half + (127,))] == 1 and want[cases.index(('std',) + half + (128,))] == 0
    assert want[cases.index(('std', 18, 72, 306, 1))] == 1                     # the staircase's exact tie


# ---------------------------------------------------------------------------------------------- 4. the entry points
_BUF = C.create_string_buffer(4096)
PTR = C.c_void_p((C.addressof(_BUF) + 63) // 64 * 64)          # a non-null, aligned pointer that no refusal dereferences


def _ints(*a):
    return (C.c_int32 * len(a))(*a)


def _multi(**kw):
    a = dict(q=PTR, H=5, W=7, P=2, th=_ints(1, 5, 3, 9, 2), na=2, nd=2, ns=1, L=256, first=1, levels=4, T=4,
             count=C.c_void_p(PTR.value + 1024), ws=C.c_void_p(PTR.value + 2048), ws_bytes=1 << 40)
    a.update(kw)
    from dmf import lib
    return lib._lib.dmf_attr_multi_levels(a['q'], a['H'], a['W'], a['P'], a['th'], a['na'], a['nd'], a['ns'], a['L'], a['first'], a['levels'],
                                          a['T'], a['count'], a['ws'], a['ws_bytes'], None)


REFUSALS = [
    ('NULL q', lambda: _multi(q=None), 1), ('NULL thresholds', lambda: _multi(th=None), 1), ('NULL count', lambda: _multi(count=None), 1),
    ('NULL workspace', lambda: _multi(ws=None), 1), ('H 0', lambda: _multi(H=0), 2), ('2^31 pixels', lambda: _multi(H=1 << 16, W=1 << 15), 2),
    ('P 65', lambda: _multi(P=65), 3), ('no area', lambda: _multi(na=0, nd=3), 4), ('equal areas', lambda: _multi(th=_ints(5, 5, 3, 9, 2)), 4),
    ('L 257', lambda: _multi(L=257), 11),
    ('n_diag -1', lambda: _multi(nd=-1), 14), ('n_std -1', lambda: _multi(ns=-1), 14),
    ('nine thresholds', lambda: _multi(th=_ints(1, 2, 3, 1, 2, 3, 1, 2, 3), na=3, nd=3, ns=3), 14),
    ('a diagonal of 0', lambda: _multi(th=_ints(1, 5, 0, 9, 2)), 14), ('falling diagonals', lambda: _multi(th=_ints(1, 5, 9, 3, 2)), 14),
    ('equal stds', lambda: _multi(th=_ints(1, 5, 3, 2, 2), nd=1, ns=2), 14), ('a std of 0', lambda: _multi(th=_ints(1, 5, 3, 9, 0)), 14),
    ('a std of L', lambda: _multi(th=_ints(1, 5, 3, 9, 7), L=7), 14),
    ('stds past 2^22 pixels', lambda: _multi(H=2049, W=2048), 13), ('first 0', lambda: _multi(first=0), 10),
    ('levels > T', lambda: _multi(levels=5), 10), ('past L - 1', lambda: _multi(first=253), 10),
    ('a small workspace', lambda: _multi(ws_bytes=16 + (2 + 4 + 4) * (2 * 2 * 4 * 35 * 4) - 1), 12),
    ('a misaligned workspace', lambda: _multi(ws=C.c_void_p(PTR.value + 2056)), 6),
    ('count inside the workspace', lambda: _multi(count=C.c_void_p(PTR.value + 2048 + 64)), 7),
]


@pytest.mark.parametrize('name,call,code', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_the_entry_point_refuses_before_any_launch(name, call, code):
    from dmf import lib
    assert call() == code and code in lib._ATTR_ERRORS


def test_a_diagonal_list_alone_may_start_below_the_last_area_and_2_22_pixels_pass_without_stds():
    """Each part of the list is increasing on its own; without stds the limit is H W < 2^31 (the call is refused later, by the
    workspace size, so nothing is launched)."""
    assert _multi(th=_ints(5, 9, 1, 2, 1), ws_bytes=16) == 12
    assert _multi(H=2049, W=2048, ns=0, th=_ints(1, 5, 3, 9), ws_bytes=16) == 12
    assert _multi(H=2048, W=2048, ws_bytes=16) == 12                          # exactly 2^22 pixels with a std


def test_the_library_declares_the_entry_points_and_sizes_the_workspace():
    from dmf import lib
    hdr = open(os.path.join(REPO, 'include', 'dmf.h')).read()
    so = C.CDLL(lib.LIB_PATH)
    for name in ('dmf_attr_multi_workspace_bytes', 'dmf_attr_multi_levels'):
        assert name + '(' in hdr and name in lib.EXPORTS and hasattr(so, name), name
    assert 'DMF_ATTR_STD_PIXELS_MAX 4194304LL' in hdr and lib.ATTR_STD_PIXELS_MAX == 1 << 22
    up16 = lambda v: (v + 15) // 16 * 16                                     # noqa: E731
    for (H, W, P, T) in ((67, 131, 4, 16), (1, 1, 1, 1), (5, 7, 3, 5), (512, 512, 4, 16), (145, 145, 4, 8)):
        cells = 2 * P * T * H * W
        area = lib.attr_workspace_bytes(H, W, P, 1, T)
        assert lib.attr_multi_workspace_bytes(H, W, P, 0, 0, T) == area
        assert lib.attr_multi_workspace_bytes(H, W, P, 2, 0, T) == area + 4 * up16(4 * cells)
        assert lib.attr_multi_workspace_bytes(H, W, P, 0, 7, T) == area + 2 * up16(8 * cells)
        assert lib.attr_multi_workspace_bytes(H, W, P, 3, 4, T) == area + 4 * up16(4 * cells) + 2 * up16(8 * cells)
    for bad in ((0, 5, 1, 1, 1, 1), (5, 5, 0, 1, 1, 1), (5, 5, 65, 1, 1, 1), (5, 5, 1, -1, 1, 1), (5, 5, 1, 1, -1, 1), (5, 5, 1, 8, 0, 1),
                (5, 5, 1, 4, 4, 1), (5, 5, 1, 1, 1, 0), (5, 5, 1, 1, 1, 17), (1 << 16, 1 << 15, 1, 1, 0, 1), (2049, 2048, 1, 0, 1, 1)):
        with pytest.raises(lib.DmfError, match='dmf_attr_multi_workspace_bytes'):
            lib.attr_multi_workspace_bytes(*bad)
    assert lib.attr_multi_workspace_bytes(2049, 2048, 1, 1, 0, 1) > 0            # without stds the std limit does not apply


# ---------------------------------------------------------------------------------------------- 5. the solver on the drop-in path
def _cfg(golden_dir, tmp, **over):
    import pca_cases as pca
    from test_gpu_trajectory import _setup
    _, cfg = _setup(golden_dir, tmp, device='cpu', fast_path=0, scale=1, epoch=1, **over)
    primary, aux, label = pca.solver_scene(cfg['Categories_Number'])
    d = cfg['data_address']
    np.save(d + 'ms4.tif.npy', primary); np.save(d + 'pan.tif.npy', aux); np.save(d + 'label.npy', label)
    cfg['DATA_DICT'][cfg['data_city']]['size'] = [40, 40, pca.SOLVER_BANDS]
    return cfg


def test_base_solver_with_the_three_keys_on_the_drop_in_path(golden_dir, capsys):
    import pca_cases as pca
    from dmf.arch import arch_from_cfg
    from solver.mainsolver import Solver
    from utils import spectral
    at = _at()
    tmp = tempfile.mkdtemp(prefix='dmf_attr_multi_')
    try:
        cfg = _cfg(golden_dir, os.path.join(tmp, 'a'), band_reduce='pca', band_reduce_bands=4, band_profile='area', band_profile_components=2,
                   band_profile_areas=[30], band_profile_diagonals=[9], band_profile_stds=[4], band_profile_levels=64)
        torch.manual_seed(3407)
        s = Solver(cfg)
        reduced, _ = spectral.reduce_host(pca.solver_scene(cfg['Categories_Number'])[0], 4)
        want, _ = amr.profile_uncached(reduced, 2, (30,), (9,), (4,), 64)
        assert s.ms.shape == (40, 40, 16) and s.ms.dtype == np.float32 and np.array_equal(ar.bits(s.ms), ar.bits(want))
        assert arch_from_cfg(cfg)['C'] == 16 and s.MS.shape[2] == 16
        line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('band_profile:')]
        assert len(line) == 1 and 'diagonals [9], stds [4]' in line[0] and '16 bands' in line[0] and line[0].endswith('host')
        info = json.load(open(cfg['RESULT_output'] + '0_band_profile.json'))
        assert set(info) == {'kind', 'components', 'areas', 'diagonals', 'stds', 'rule', 'levels', 'connectivity', 'range', 'bands', 'order',
                             'route'}
        assert info['order'] == at.band_names(4, 2, (30,), (9,), (4,)) and info['bands'] == 16
        assert info['areas'] == [30] and info['diagonals'] == [9] and info['stds'] == [4] and info['rule'] == at.RULE
        cfg = _cfg(golden_dir, os.path.join(tmp, 'b'), band_reduce='pca', band_reduce_bands=4, band_profile='morph',
                   band_profile_diagonals=[9])
        with pytest.raises(ValueError, match='band_profile_diagonals needs band_profile: area, and band_profile is morph'):
            Solver(cfg)
        cfg = _cfg(golden_dir, os.path.join(tmp, 'c'), band_reduce='pca', band_reduce_bands=4, band_profile='area',
                   band_profile_areas=[1, 2, 3], band_profile_diagonals=[1, 2, 3], band_profile_stds=[1, 2, 3])
        with pytest.raises(ValueError, match='thresholds are more than 8'):
            Solver(cfg)
        for sub in 'bc':                                                     # refused before any work
            assert not os.path.exists(os.path.join(tmp, sub, 'out', '0_band_reduce.npz'))
    finally:
        shutil.rmtree(tmp)
