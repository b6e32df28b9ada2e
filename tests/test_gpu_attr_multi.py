"""GPU: `band_profile: area` with diagonals and stds — dmf_attr_multi_levels through the C ABI and through
dmf.engine.band_profile against utils.attribute.profile_host and the sequential union-find of tests/attr_multi_ref.py, bit for bit
as uint32 (the definition is in integers: there is no tolerance to state); the count planes at T = 1, 8 and 16; guard words around
count, the output and the workspace; the old entry point's bytes with no diagonal and no std; the refusals; the solver."""
import json
import os
import shutil
import tempfile

import numpy as np
import pytest
import torch

import attr_cases as ac
import attr_multi_cases as amc
import attr_multi_ref as amr
import attr_ref as ar

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
GUARD = 4096


def _pitched(s, extra):
    """s [H, W, K] on the device with pixels K + extra floats apart; the gaps hold NaN."""
    H, W, K = s.shape
    buf = torch.full((H, W, K + extra), float('nan'), device=DEV)
    buf[:, :, :K] = torch.from_numpy(np.array(s)).to(DEV)
    return buf[:, :, :K]


def _guarded(shape, dtype, fill):
    """A tensor of `shape` between two guards of GUARD bytes of 0xEE -> (the view, the whole uint8 buffer, its byte count)."""
    nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    raw = torch.full((nbytes + 2 * GUARD,), 0xEE, dtype=torch.uint8, device=DEV)
    view = raw[GUARD:GUARD + nbytes].view(dtype).view(*shape)
    view.copy_(torch.full(shape, fill, dtype=dtype, device=DEV))
    return view, raw, nbytes


def _guards_intact(raw, nbytes):
    return bool((raw[:GUARD] == 0xEE).all()) and bool((raw[GUARD + nbytes:] == 0xEE).all())


def _planes(scores, P, areas, diagonals, stds, L, T, fill=0xAB, slack=256, old_entry=False):
    """The entry points on scores at a pixel pitch of K + 3 -> dict(q, count, range, out, guards, ws_tail): every output sits
    between guards and starts as `fill`; the workspace is `slack` bytes longer than the carve and sits between guards too.
    old_entry: dmf_attr_area_levels and its workspace (no diagonals, no stds)."""
    from dmf import lib
    H, W, K = scores.shape
    thresholds, counts = tuple(areas) + tuple(diagonals) + tuple(stds), (len(areas), len(diagonals), len(stds))
    n = len(thresholds)
    T = max(1, min(T, L - 1))
    sd = _pitched(scores, 3)
    need = lib.attr_workspace_bytes(H, W, P, n, T) if old_entry else lib.attr_multi_workspace_bytes(H, W, P, counts[1], counts[2], T)
    ws, ws_raw, _ = _guarded((need + slack,), torch.uint8, fill)
    q, q_raw, q_bytes = _guarded((2 * P, H, W), torch.uint8, fill)
    count, c_raw, c_bytes = _guarded((2 * P, n, H, W), torch.uint8, fill)
    rng, r_raw, r_bytes = _guarded((P, 2), torch.float32, float('nan'))
    out, o_raw, o_bytes = _guarded((H, W, K + 2 * n * P), torch.float32, float('nan'))
    lib.attr_quantise(sd, P, L, q, rng, ws)
    calls = lib.attr_area_run(q, areas, L, count, ws, T) if old_entry else lib.attr_multi_run(q, thresholds, counts, L, count, ws, T)
    lib.attr_stack(sd, P, n, L, count, rng, out)
    torch.cuda.synchronize()
    assert calls == -(-(L - 1) // T)
    guards = all(_guards_intact(r, b) for r, b in ((ws_raw, need + slack), (q_raw, q_bytes), (c_raw, c_bytes), (r_raw, r_bytes), (o_raw, o_bytes)))
    return dict(q=q.cpu().numpy(), count=count.cpu().numpy(), range=rng.cpu().numpy(), out=out.cpu().numpy(), guards=guards, need=need,
                ws_tail=ws_raw[GUARD + need:GUARD + need + slack].cpu().numpy(), fill=fill)


# ---------------------------------------------------------------------------------------------- 1. every case
@pytest.mark.parametrize('name', amc.NAMES)
def test_device_equals_profile_host_and_the_reference_at_every_batch_size(name):
    """Through the C ABI at T = 1, 8 and 16 (levels enqueued as 1 .. L - 1 in batches of T) and at a pixel pitch > K: q and count are
    the reference's integers, the stacked output is profile_host's and the reference's as uint32, every batch size gives the same
    bytes, a second run over other garbage gives the same bytes, and no guard word or workspace byte past the carve is written.
    Through the engine (T = 16, one copy back): the same profile and profile_host's info apart from the route."""
    from dmf.engine import band_profile
    from utils import attribute
    c = amc.cases()[name]
    want, levels = amr.case_profile(name)
    host, hinfo = attribute.profile_host(c.scores, c.P, c.areas, c.L, c.diagonals, c.stds)
    n = len(c.areas) + len(c.diagonals) + len(c.stds)
    runs = {T: _planes(c.scores, c.P, c.areas, c.diagonals, c.stds, c.L, T) for T in (1, 8, 16)}
    runs['again'] = _planes(c.scores, c.P, c.areas, c.diagonals, c.stds, c.L, 16, fill=0x5C)
    for T, r in runs.items():
        assert r['guards'], 'a guard word was written (T = %s)' % T
        assert (r['ws_tail'] == r['fill']).all(), 'a workspace byte past the carve was written (T = %s)' % T
        for p in range(c.P):
            assert np.array_equal(r['q'][p], levels[p]) and np.array_equal(r['q'][c.P + p], c.L - 1 - levels[p]), (T, p)
            for i in range(n):
                opened, closed = levels[(p, i)]
                assert np.array_equal(r['count'][p, i], opened), (T, p, i)
                assert np.array_equal(c.L - 1 - r['count'][c.P + p, i].astype(np.int32), closed), (T, p, i)
        assert np.array_equal(ar.bits(r['out']), ar.bits(host)), 'device and profile_host differ (T = %s)' % T
        assert np.array_equal(ar.bits(r['out']), ar.bits(want)), 'device and the reference differ (T = %s)' % T
        for k in ('q', 'count', 'range', 'out'):
            assert np.array_equal(r[k].view(np.uint8), runs[16][k].view(np.uint8)), (T, k)
    got, info = band_profile(_pitched(c.scores, 5), c.P, None, DEV, kind='area', areas=c.areas, levels=c.L, diagonals=c.diagonals, stds=c.stds)
    assert got.dtype == np.float32 and np.array_equal(ar.bits(got), ar.bits(want))
    assert info['route'] == 'device' and {k: v for k, v in info.items() if k != 'route'} == {k: v for k, v in hinfo.items() if k != 'route'}


def test_the_hand_written_levels_on_the_device():
    """The ring (area and diagonal disagree) and the staircase (subtractive, not max rule), read from the device's count planes."""
    c = amc.cases()['ring_at_the_tile_corner_33x34']
    r = _planes(c.scores, c.P, c.areas, c.diagonals, c.stds, c.L, 16)
    kinds = [('a', a) for a in c.areas] + [('d', d) for d in c.diagonals] + [('s', s) for s in c.stds]
    for i, key in enumerate(kinds):
        for region, mask in amc.ring_regions().items():
            want_open, want_close = amc.RING_EXPECTED[key][region]
            assert (r['count'][0, i][mask] == want_open).all() and (c.L - 1 - r['count'][1, i][mask].astype(int) == want_close).all(), (key, region)
    c = amc.cases()['std_staircase_12x20']
    r = _planes(c.scores, c.P, c.areas, c.diagonals, c.stds, c.L, 16)
    first_std = len(c.areas) + len(c.diagonals)
    for i, s in enumerate(c.stds):
        for region, mask in amc.stair_regions().items():
            assert (r['count'][0, first_std + i][mask] == amc.STAIR_EXPECTED[('s', s)][region]).all(), (s, region)


def test_the_accumulators_of_the_ring_as_attr_multi_carve_views_them():
    """One call of the levels 1 .. 3 of the ring (T = 4, so level plane 3 is not used): at the ring's root — its first pixel in
    raster order — every level plane holds 44 pixels, the box 10 .. 21 in both directions, sum q = 44 * 3 and sum q^2 = 44 * 9; the
    dual plane's inside holds 100 pixels in 11 .. 20.  With diagonals alone the carve has no sums, with stds alone no box."""
    from dmf import lib
    c = amc.cases()['ring_at_the_tile_corner_33x34']
    H, W, _ = c.scores.shape
    sd = torch.from_numpy(np.array(c.scores)).to(DEV)
    ws = torch.full((lib.attr_multi_workspace_bytes(H, W, 1, 2, 1, 4),), 0xAB, dtype=torch.uint8, device=DEV)
    q = torch.empty(2, H, W, dtype=torch.uint8, device=DEV)
    rng = torch.empty(1, 2, device=DEV)
    count = torch.empty(2, 4, H, W, dtype=torch.uint8, device=DEV)
    lib.attr_quantise(sd, 1, c.L, q, rng, ws)
    lib.attr_multi_levels(q, c.areas + c.diagonals + c.stds, (1, 2, 1), c.L, 1, 3, count, ws, 4)
    torch.cuda.synchronize()
    v = {k: t.cpu().numpy() for k, t in lib.attr_multi_carve(ws, H, W, 1, 2, 1, 4).items()}
    assert set(v) == {'keys', 'parent', 'size', 'xmin', 'xmax', 'ymin', 'ymax', 'sum_q', 'sum_q2'}
    ring_root, inside_root = amc.RING_LO * W + amc.RING_LO, (amc.RING_LO + 1) * W + amc.RING_LO + 1
    for l in range(3):
        at = lambda name, plane, root: int(v[name][plane, l, root])              # noqa: E731
        assert [at(k, 0, ring_root) for k in ('parent', 'size', 'xmin', 'xmax', 'ymin', 'ymax', 'sum_q', 'sum_q2')] \
            == [ring_root, 44, 10, 21, 10, 21, 44 * 3, 44 * 9], l
        assert [at(k, 1, inside_root) for k in ('parent', 'size', 'xmin', 'xmax', 'ymin', 'ymax', 'sum_q', 'sum_q2')] \
            == [inside_root, 100, 11, 20, 11, 20, 100 * 3, 100 * 9], l
    assert (v['size'][:, 3] == 0xABABABAB - (1 << 32)).all() and (v['sum_q'][:, 3] == v['sum_q'][0, 3, 0]).all()      # plane 3: as it was
    ws2 = torch.empty(lib.attr_multi_workspace_bytes(H, W, 1, 2, 0, 4), dtype=torch.uint8, device=DEV)
    assert set(lib.attr_multi_carve(ws2, H, W, 1, 2, 0, 4)) == {'keys', 'parent', 'size', 'xmin', 'xmax', 'ymin', 'ymax'}
    assert set(lib.attr_multi_carve(ws, H, W, 1, 0, 1, 4)) == {'keys', 'parent', 'size', 'sum_q', 'sum_q2'}


# ---------------------------------------------------------------------------------------------- 2. against the old entry point
@pytest.mark.parametrize('name', ['past_the_tile_17x33_L256', 'blobs_at_the_tile_corner', 'serpentine_67x131'])
def test_without_diagonals_and_stds_the_bytes_are_the_old_entry_points(name):
    from dmf import lib
    c = ac.cases()[name]
    H, W, _ = c.scores.shape
    for T in (1, 16):
        old = _planes(c.scores, c.P, c.areas, (), (), c.L, T, old_entry=True)
        new = _planes(c.scores, c.P, c.areas, (), (), c.L, T)
        assert old['need'] == new['need'] == lib.attr_workspace_bytes(H, W, c.P, len(c.areas), max(1, min(T, c.L - 1)))
        assert new['guards'] and (new['ws_tail'] == new['fill']).all()
        for k in ('q', 'count', 'range', 'out'):
            assert old[k].tobytes() == new[k].tobytes(), (T, k)


def test_the_engine_without_the_new_keys_calls_what_it_called(monkeypatch):
    from dmf import engine, lib
    c = ac.cases()['small_5x4']
    monkeypatch.setattr(lib, 'attr_multi_run', lambda *a, **k: pytest.fail('the new route ran without a diagonal or a std'))
    want, _ = ar.case_profile('small_5x4')
    for more in ({}, dict(diagonals=(), stds=()), dict(diagonals=[], stds=None)):
        got, info = engine.band_profile(np.array(c.scores), c.P, None, DEV, kind='area', areas=c.areas, levels=c.L, **more)
        assert got.tobytes() == np.asarray(want).tobytes()
        assert list(info) == ['kind', 'components', 'areas', 'levels', 'connectivity', 'range', 'bands', 'order', 'route']


# ---------------------------------------------------------------------------------------------- 3. refusals
def test_refusals_leave_the_outputs_as_they_were():
    """Bad sizes (never a bad pointer to a launch): every output keeps its fill.  Codes 13 and 14 are the new ones."""
    from dmf import lib
    from dmf.engine import band_profile
    c = amc.cases()['small_5x4']
    H, W, K = c.scores.shape
    q = torch.full((2, H, W), 7, dtype=torch.uint8, device=DEV)
    count = torch.full((2, 3, H, W), 7, dtype=torch.uint8, device=DEV)
    ws = torch.full((lib.attr_multi_workspace_bytes(H, W, 1, 1, 1, 4),), 7, dtype=torch.uint8, device=DEV)
    for th, counts, L in (((2, 5, 5), (1, 2, 0), 7), ((2, 5, 0), (1, 1, 1), 7), ((2, 5, 7), (1, 1, 1), 7), ((2, 5, 2 ** 31), (1, 1, 1), 7),
                          ((2, 3, 3), (1, 0, 2), 7)):
        with pytest.raises(lib.DmfError, match='strictly increasing diagonals >= 1 and stds in 1..L - 1'):
            lib.attr_multi_levels(q, th, counts, L, 1, 4, count, ws, 4)
    with pytest.raises(lib.DmfError, match='strictly increasing areas'):
        lib.attr_multi_levels(q, (5, 5, 3), (2, 1, 0), 7, 1, 4, count, ws, 4)
    with pytest.raises(lib.DmfError, match='do not add up'):
        lib.attr_multi_levels(q, (2, 5, 3), (1, 1, 0), 7, 1, 4, count, ws, 4)
    for first, levels, T in ((0, 4, 4), (1, 5, 4), (4, 4, 4), (1, 0, 4)):
        with pytest.raises(lib.DmfError, match='first_level, levels or T out of range'):
            lib.attr_multi_levels(q, (2, 5, 3), (1, 1, 1), 7, first, levels, count, ws, T)
    with pytest.raises(lib.DmfError, match='the workspace must be a uint8 tensor of at least'):
        lib.attr_multi_levels(q, (2, 5, 3), (1, 1, 1), 7, 1, 4, count, ws[:-16], 4)
    small = ws[:lib.attr_workspace_bytes(H, W, 1, 3, 4)]                        # enough for the areas, not for the box and the sums
    with pytest.raises(lib.DmfError, match='the workspace must be a uint8 tensor of at least'):
        lib.attr_multi_levels(q, (2, 5, 3), (1, 1, 1), 7, 1, 4, count, small, 4)
    # code 13 through the C ABI: 2^22 + 2048 pixels with a std; q and count are large enough, nothing may be written
    Hb, Wb = 2049, 2048
    qb = torch.full((2, Hb, Wb), 7, dtype=torch.uint8, device=DEV)
    cb = torch.full((2, 2, Hb, Wb), 7, dtype=torch.uint8, device=DEV)
    import ctypes as C
    rc = lib._lib.dmf_attr_multi_levels(qb.data_ptr(), Hb, Wb, 1, (C.c_int32 * 2)(5, 3), 1, 0, 1, 7, 1, 1, 1, cb.data_ptr(), ws.data_ptr(),
                                        1 << 40, None)
    assert rc == 13 and lib._ATTR_ERRORS[13] == 'stds with H W > 2^22'
    with pytest.raises(lib.DmfError, match='stds with H W > 2\\^22'):
        lib.attr_multi_levels(qb, (5, 3), (1, 0, 1), 7, 1, 1, cb, ws, 1)
    with pytest.raises(ValueError, match='band_profile_stds: 2049 x 2048 pixels are more than 2\\^22'):
        band_profile(torch.zeros(Hb, Wb, 1, device=DEV), 1, None, DEV, kind='area', areas=(5,), levels=7, stds=(3,))
    with pytest.raises(ValueError, match='thresholds are more than 8'):
        band_profile(np.array(c.scores), 1, None, DEV, kind='area', areas=(1, 2, 3), levels=7, diagonals=(1, 2, 3), stds=(1, 2, 3))
    with pytest.raises(TypeError):
        band_profile(np.array(c.scores), 1, None, DEV, kind='area', areas=(1,), levels=7, moments=(1,))
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in (q, count, ws, qb, cb))


# ---------------------------------------------------------------------------------------------- 4. the solver
def _cfg(golden_dir, tmp, **over):
    import pca_cases as pca
    from test_gpu_trajectory import _setup
    _, cfg = _setup(golden_dir, tmp, **dict(dict(epoch=1, scale=1, train_rate=0.3, verify_rate=0.1, steps_per_graph=-1, seed=123), **over))
    primary, aux, label = pca.solver_scene(cfg['Categories_Number'])
    d = cfg['data_address']
    np.save(d + 'ms4.tif.npy', primary); np.save(d + 'pan.tif.npy', aux); np.save(d + 'label.npy', label)
    cfg['DATA_DICT'][cfg['data_city']]['size'] = [40, 40, pca.SOLVER_BANDS]
    return cfg


def test_solver_with_the_three_keys_fast_path_1_and_0(golden_dir, capsys):
    """8 components, 4 of them profiled at one area, one diagonal and one std: the 32-band row, through Solver, and a few steps
    train.  Then the same
    solver's `_band_profile` with `fast` off on the scores the device route had (`band_reduce` again: it is deterministic): equal
    `self.ms` as uint32 and equal `<t>_band_profile.json` apart from the route.  The two routes are compared on the same scores
    because `band_reduce`'s own two routes agree to a tolerance, not bit for bit (tests/test_gpu_band_reduce.py), and a profile is
    compared in integers; a whole `fast_path: 0` run with the keys is tests/test_attr_multi_host.py's."""
    from dmf.engine import band_reduce
    from solver.mainsolver import Solver
    from utils import attribute
    import pca_cases as pca
    tmp = tempfile.mkdtemp(prefix='dmf_attr_multi_')
    try:
        cfg = _cfg(golden_dir, tmp, band_reduce='pca', band_reduce_bands=8, band_profile='area', band_profile_components=4,
                   band_profile_areas=[16], band_profile_diagonals=[8], band_profile_stds=[5], band_profile_levels=64, patch_size=11)
        torch.manual_seed(3407)
        s = Solver(cfg)
        assert s.ms.shape == (40, 40, 32) and s.ms.dtype == np.float32 and s.band_profile_info['route'] == 'device'
        assert s.scene.A.shape == (50, 50, 32)
        fast_ms = s.ms
        s.dataloader()
        s.train()
        assert len(s.step_losses) >= 2 and np.isfinite(s.step_losses).all() and s.cur_model.arch['C'] == 32 and s.cur_model.arch['G'] == 2
        fast = json.load(open(cfg['RESULT_output'] + '0_band_profile.json'))
        line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('band_profile:')]
        assert len(line) == 1 and 'diagonals [8], stds [5]' in line[0] and '32 bands' in line[0] and line[0].endswith('device')

        scores, _ = band_reduce(pca.solver_scene(cfg['Categories_Number'])[0].copy(), 8, False, cfg['device'])
        want, _ = attribute.profile_host(scores, 4, (16,), 64, (8,), (5,))
        assert np.array_equal(ar.bits(fast_ms), ar.bits(want)), 'self.ms is not profile_host of the same scores'
        s.fast, s.ms = False, scores                                          # fast_path: 0 from the same scores on
        slow_ms, slow_info = s._band_profile(attribute.profile_keys(cfg))
        slow = json.load(open(cfg['RESULT_output'] + '0_band_profile.json'))
        assert slow_info['route'] == slow['route'] == 'host' and fast['route'] == 'device'
        assert np.array_equal(ar.bits(slow_ms), ar.bits(fast_ms)), 'fast_path 1 and 0 give another self.ms'
        assert list(fast) == list(slow) == ['kind', 'components', 'areas', 'diagonals', 'stds', 'rule', 'levels', 'connectivity', 'range',
                                            'bands', 'order', 'route']
        assert {k: v for k, v in fast.items() if k != 'route'} == {k: v for k, v in slow.items() if k != 'route'}
        assert fast['order'] == attribute.band_names(8, 4, (16,), (8,), (5,)) and fast['bands'] == 32 and fast['rule'] == attribute.RULE
    finally:
        shutil.rmtree(tmp)
