"""GPU: `band_profile: area` — dmf_attr_quantise, dmf_attr_area_levels and dmf_attr_stack through
dmf.engine.band_profile(kind='area') against utils.attribute.profile_host and the sequential union-find of tests/attr_ref.py, bit
for bit as uint32 (the definition is in integers: there is no tolerance to state); the count planes at every batch size; the
workspace discipline; and the solver with the kind on the 32-band row."""
import json
import os
import shutil
import tempfile

import numpy as np
import pytest
import torch

import attr_cases as ac
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


def _planes(case, T, fill=0xAB, slack=0):
    """The three entry points on a case -> dict(q, count, range, out, ws_raw, need, guards): every output sits between guards and
    starts as `fill`; the workspace is `slack` bytes longer than the carve and sits between guards too."""
    from dmf import lib
    c = case
    H, W, K = c.scores.shape
    P, n, L = c.P, len(c.areas), c.L
    T = max(1, min(T, L - 1))
    sd = _pitched(c.scores, 3)
    need = lib.attr_workspace_bytes(H, W, P, n, T)
    ws, ws_raw, _ = _guarded((need + slack,), torch.uint8, fill)
    q, q_raw, q_bytes = _guarded((2 * P, H, W), torch.uint8, fill)
    count, c_raw, c_bytes = _guarded((2 * P, n, H, W), torch.uint8, fill)
    rng, r_raw, r_bytes = _guarded((P, 2), torch.float32, float('nan'))
    out, o_raw, o_bytes = _guarded((H, W, K + 2 * n * P), torch.float32, float('nan'))
    lib.attr_quantise(sd, P, L, q, rng, ws)
    calls = lib.attr_area_run(q, c.areas, L, count, ws, T)
    lib.attr_stack(sd, P, n, L, count, rng, out)
    torch.cuda.synchronize()
    assert calls == -(-(L - 1) // T)
    guards = all(_guards_intact(r, b) for r, b in ((ws_raw, need + slack), (q_raw, q_bytes), (c_raw, c_bytes), (r_raw, r_bytes), (o_raw, o_bytes)))
    return dict(q=q.cpu().numpy(), count=count.cpu().numpy(), range=rng.cpu().numpy(), out=out.cpu().numpy(), guards=guards,
                ws_tail=ws_raw[GUARD + need:GUARD + need + slack].cpu().numpy(), fill=fill)


# ---------------------------------------------------------------------------------------------- 1. every case, end to end
@pytest.mark.parametrize('name', ac.NAMES)
def test_engine_route_equals_profile_host_and_the_reference(name):
    from dmf.engine import band_profile
    from utils import attribute
    c = ac.cases()[name]
    want, levels = ar.case_profile(name)
    host, hinfo = attribute.profile_host(c.scores, c.P, c.areas, c.L)
    got, info = band_profile(_pitched(c.scores, 5), c.P, None, DEV, kind='area', areas=c.areas, levels=c.L)
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(ar.bits(got), ar.bits(host)), 'device and profile_host differ'
    assert np.array_equal(ar.bits(got), ar.bits(want)), 'device and the reference differ'
    assert info['route'] == 'device' and {k: v for k, v in info.items() if k != 'route'} == {k: v for k, v in hinfo.items() if k != 'route'}
    got2, _ = band_profile(np.array(c.scores), c.P, None, DEV, kind='area', areas=list(c.areas), levels=c.L)      # a numpy array, pitch K
    assert np.array_equal(ar.bits(got2), ar.bits(want))


def test_the_default_kind_is_morph_and_the_refusals_are_by_name():
    import morph_cases as mc
    from dmf.engine import band_profile
    from utils import morphology
    s = mc.scores(33, 37, 3)
    want, _ = morphology.profile_host(s, 2, (1, 3))
    got, info = band_profile(np.array(s), 2, (1, 3), DEV)                      # the call of before: positional, no kind
    assert np.array_equal(ar.bits(got), ar.bits(want)) and list(info) == ['components', 'radii', 'bands', 'order', 'route', 'rounds']
    bad = np.array(s)
    bad[3, 4, 2] = np.inf
    with pytest.raises(ValueError, match='band_profile: the scores hold a value that is not finite'):
        band_profile(bad, 2, None, DEV, kind='area', areas=(1, 3), levels=7)
    with pytest.raises(ValueError, match='band_profile_components: 4 exceeds the 3 components'):
        band_profile(np.array(s), 4, None, DEV, kind='area', areas=(1, 3), levels=7)
    with pytest.raises(ValueError, match='band_profile_areas .* is not strictly increasing'):
        band_profile(np.array(s), 2, None, DEV, kind='area', areas=(3, 3), levels=7)
    with pytest.raises(ValueError, match='band_profile_levels 1 is not a whole number in 2..256'):
        band_profile(np.array(s), 2, None, DEV, kind='area', areas=(1, 3), levels=1)
    with pytest.raises(ValueError, match="kind 'disk' is not one of morph / area"):
        band_profile(np.array(s), 2, (1, 3), DEV, kind='disk')


# ---------------------------------------------------------------------------------------------- 2. the planes
@pytest.mark.parametrize('name', ['past_the_tile_17x33_L256', 'serpentine_67x131', 'blobs_at_the_tile_corner'])
def test_count_planes_at_every_batch_size_and_the_workspace_discipline(name):
    """T = 1, 8 and 16 (at L = 256: last batches of 1, 7 and 15 levels) give the same q, count and range, which are the
    reference's integers; two runs in a row — the second over other garbage — are bit-identical; the guard words around q, count,
    range, out and the workspace are intact, and so is every workspace byte past the carve."""
    c = ac.cases()[name]
    _, levels = ar.case_profile(name)
    P, n, L = c.P, len(c.areas), c.L
    runs = {T: _planes(c, T, slack=256) for T in (1, 8, 16)}
    again = _planes(c, 16, fill=0x5C, slack=256)
    for T, r in list(runs.items()) + [('again', again)]:
        assert r['guards'], 'a guard word was written (T = %s)' % T
        assert (r['ws_tail'] == r['fill']).all(), 'a workspace byte past the carve was written (T = %s)' % T
        for p in range(P):
            assert np.array_equal(r['q'][p], levels[p]) and np.array_equal(r['q'][P + p], L - 1 - levels[p]), (T, p)
            for i in range(n):
                opened, closed = levels[(p, i)]
                assert np.array_equal(r['count'][p, i], opened), (T, p, i)
                assert np.array_equal(L - 1 - r['count'][P + p, i].astype(np.int32), closed), (T, p, i)
            f = ar.canon_list(c.scores[:, :, p])
            assert r['range'][p, 0] == np.float32(min(f)) and r['range'][p, 1] == np.float32(max(f))
    for T in (1, 8):
        for k in ('q', 'count', 'range', 'out'):
            assert np.array_equal(runs[T][k].view(np.uint8), runs[16][k].view(np.uint8)), (T, k)
    for k in ('q', 'count', 'range', 'out'):
        assert np.array_equal(again[k].view(np.uint8), runs[16][k].view(np.uint8)), k
    assert np.array_equal(ar.bits(runs[16]['out']), ar.bits(ar.case_profile(name)[0]))


def test_refusals_leave_the_outputs_as_they_were():
    """Bad sizes (never a bad pointer to a launch): every output keeps its fill."""
    from dmf import lib
    c = ac.cases()['small_5x4']
    H, W, K = c.scores.shape
    sd = torch.from_numpy(np.array(c.scores)).to(DEV)
    q = torch.full((2, H, W), 7, dtype=torch.uint8, device=DEV)
    count = torch.full((2, 2, H, W), 7, dtype=torch.uint8, device=DEV)
    rng = torch.full((1, 2), 7.0, device=DEV)
    out = torch.full((H, W, K + 4), 7.0, device=DEV)
    ws = torch.full((lib.attr_workspace_bytes(H, W, 1, 2, 4),), 7, dtype=torch.uint8, device=DEV)
    with pytest.raises(lib.DmfError, match='L outside 2..256'):
        lib.attr_quantise(sd, 1, 257, q, rng, ws)
    with pytest.raises(lib.DmfError, match='strictly increasing areas'):
        lib.attr_area_levels(q, (5, 5), 7, 1, 4, count, ws, 4)
    with pytest.raises(lib.DmfError, match='strictly increasing areas'):
        lib.attr_area_levels(q, (5, 2 ** 31), 7, 1, 4, count, ws, 4)
    for first, levels, T in ((0, 4, 4), (1, 5, 4), (4, 4, 4), (1, 0, 4)):
        with pytest.raises(lib.DmfError, match='first_level, levels or T out of range'):
            lib.attr_area_levels(q, (2, 5), 7, first, levels, count, ws, T)
    with pytest.raises(lib.DmfError, match='the workspace must be a uint8 tensor of at least'):
        lib.attr_area_levels(q, (2, 5), 7, 1, 4, count, ws[:-16], 4)
    with pytest.raises(lib.DmfError, match='L outside 2..256'):
        lib.attr_stack(sd, 1, 2, 1, count, rng, out)
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in (q, count, rng, out, ws))


# ---------------------------------------------------------------------------------------------- 3. the solver
def _cfg(golden_dir, tmp, **over):
    import pca_cases as pca
    from test_gpu_trajectory import _setup
    _, cfg = _setup(golden_dir, tmp, **dict(dict(epoch=1, scale=1, train_rate=0.3, verify_rate=0.1, steps_per_graph=-1, seed=123), **over))
    primary, aux, label = pca.solver_scene(cfg['Categories_Number'])
    d = cfg['data_address']
    np.save(d + 'ms4.tif.npy', primary); np.save(d + 'pan.tif.npy', aux); np.save(d + 'label.npy', label)
    cfg['DATA_DICT'][cfg['data_city']]['size'] = [40, 40, pca.SOLVER_BANDS]
    return cfg


def test_solver_with_the_kind_trains_on_the_32_band_row(golden_dir, capsys):
    """8 components, 4 of them profiled at three areas, patch 11: the row 32/1/11/1/40/2.  `self.ms` is profile_host of the scores
    the device left (the same scores: the profile is compared bit for bit), a few steps train, and the JSON file is written."""
    from dmf.engine import band_reduce
    from solver.mainsolver import Solver
    from utils import attribute
    import pca_cases as pca
    tmp = tempfile.mkdtemp(prefix='dmf_attr_')
    try:
        cfg = _cfg(golden_dir, tmp, band_reduce='pca', band_reduce_bands=8, band_profile='area', band_profile_components=4,
                   band_profile_areas=[4, 16, 64], band_profile_levels=64, patch_size=11)
        P = cfg['patch_size']
        torch.manual_seed(3407)
        s = Solver(cfg)
        assert s.ms.shape == (40, 40, 32) and s.ms.dtype == np.float32 and s.band_profile_info['route'] == 'device'
        assert s.scene.A.shape == (40 + P - 1, 40 + P - 1, 32)
        scores, _ = band_reduce(pca.solver_scene(cfg['Categories_Number'])[0].copy(), 8, False, cfg['device'])
        want, winfo = attribute.profile_host(scores, 4, (4, 16, 64), 64)
        assert np.array_equal(ar.bits(s.ms), ar.bits(want)), 'self.ms is not profile_host of the same scores'
        s.dataloader()
        s.train()
        assert len(s.step_losses) >= 2 and np.isfinite(s.step_losses).all() and s.cur_model.arch['C'] == 32 and s.cur_model.arch['G'] == 2
        info = json.load(open(cfg['RESULT_output'] + '0_band_profile.json'))
        assert set(info) == {'kind', 'components', 'areas', 'levels', 'connectivity', 'range', 'bands', 'order', 'route'}
        assert info['order'] == attribute.band_names(8, 4, (4, 16, 64)) and len(info['order']) == info['bands'] == 32
        assert info['kind'] == 'area' and info['areas'] == [4, 16, 64] and info['levels'] == 64 and info['connectivity'] == 4
        assert info['route'] == 'device' and info['range'] == winfo['range']
        assert os.path.exists(cfg['RESULT_output'] + '0_band_reduce.npz')
        line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('band_profile:')]
        assert len(line) == 1 and 'area' in line[0] and '32 bands' in line[0] and line[0].endswith('device')
    finally:
        shutil.rmtree(tmp)


def test_a_band_count_without_a_kernel_row_names_the_kind(golden_dir):
    from dmf import lib
    from solver.mainsolver import Solver
    tmp = tempfile.mkdtemp(prefix='dmf_attr_')
    try:
        cfg = _cfg(golden_dir, tmp, band_reduce='pca', band_reduce_bands=8, band_profile='area', band_profile_components=2,
                   band_profile_areas=[4, 16])
        with pytest.raises(lib.DmfError) as e:
            Solver(cfg)
        text = str(e.value)
        assert 'no compiled kernel instance for C=16' in text
        assert 'band_reduce_bands: 8 with band_profile: area needs the line "16 1 5 1 40 2"' in text
        assert not os.path.exists(cfg['RESULT_output'] + '0_band_profile.json')
    finally:
        shutil.rmtree(tmp)
