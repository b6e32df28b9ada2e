"""CPU: `band_profile: morph` — utils.morphology.profile_host against the scipy reference of tests/morph_ref.py
bit for bit on every fixture of tests/morph_cases.py, the guards that make the serpentine worth its name, the band order, the keys
and their refusals, and the key at `none`."""
import copy
import json
import os
import shutil
import tempfile

import numpy as np
import pytest
import torch

import morph_cases as mc
import morph_ref as mr


def _mo():
    from utils import morphology
    return morphology


# ---------------------------------------------------------------------------------------------- 1. the definition
@pytest.mark.parametrize('shape', mc.SERPENTINE_SHAPES)
def test_profile_host_equals_the_reference_on_the_serpentine(shape):
    mo = _mo()
    s = mc.serpentine(*shape)[:, :, None]
    got, info = mo.profile_host(s, 1, mc.SERPENTINE_RADII)
    want = mr.profile(s, 1, mc.SERPENTINE_RADII)
    assert got.dtype == np.float32 and got.shape == want.shape == shape + (7,)
    assert np.array_equal(mr.bits(got), mr.bits(want))
    assert info['route'] == 'host' and info['bands'] == 7


@pytest.mark.parametrize('name', sorted(mc.planes()))
def test_profile_host_equals_the_reference_on_the_further_planes(name):
    f, radii = mc.planes()[name]
    got, _ = _mo().profile_host(f[:, :, None], 1, radii)
    assert np.array_equal(mr.bits(got), mr.bits(mr.profile(f[:, :, None], 1, radii)))
    assert not (mr.bits(got) == 0x80000000).any()                           # no -0 leaves the profile


def test_profile_host_on_several_components():
    s = mc.scores(33, 37, 3)
    got, _ = _mo().profile_host(s, 2, (1, 3))
    assert np.array_equal(mr.bits(got), mr.bits(mr.profile(s, 2, (1, 3))))
    assert np.array_equal(mr.bits(got[:, :, 10]), mr.bits(s[:, :, 2]))     # the component that is not profiled: bit for bit


@pytest.mark.parametrize('r', mc.SERPENTINE_RADII)
@pytest.mark.parametrize('shape', mc.SERPENTINE_SHAPES)
def test_the_serpentine_guards(shape, r):
    """What makes the fixture a test of the propagation: the opening by reconstruction is not the plain opening, it restores the
    whole plateau, the one-pixel-per-round reference needs far more rounds than the image has rows or columns (r >= 2: the marker
    is the room alone), and the result has the properties of the fixed point."""
    mo = _mo()
    f = mc.serpentine(*shape)
    marker = mr.erode(f, r)
    gamma, rounds = mr.rec_dilation(marker, f)
    plain = mr.dilate(marker, r)
    differ = int((gamma != plain).sum())
    print('%d x %d, r = %d: differs from the plain opening at %d pixels, %d reference rounds' % (shape + (r, differ, rounds)))
    assert differ >= 250
    assert int((gamma == 1).sum()) == int((f == 1).sum())
    if r >= 2:
        assert not (marker[mc.ROOM:] == 1).any() and not (marker[:, mc.ROOM:] == 1).any() and rounds > 3 * max(shape)
    got, _ = mo.opening_by_reconstruction(f, r)
    assert np.array_equal(mr.bits(got), mr.bits(gamma))
    assert (marker <= got).all() and (got <= f).all()
    assert np.array_equal(got, np.minimum(mr.dilate(got, 1), f))


# ---------------------------------------------------------------------------------------------- 2. order, keys, refusals
def test_band_order_and_count():
    mo = _mo()
    assert mo.band_count(8, 4, 3) == 32
    assert mo.band_names(3, 1, (2, 4)) == ['pc1_close_r4', 'pc1_close_r2', 'pc1', 'pc1_open_r2', 'pc1_open_r4', 'pc2', 'pc3']
    s = mc.scores(33, 37, 3)
    got, info = mo.profile_host(s, 1, (2, 4))
    f = mr.canon(s[:, :, 0])
    for band, want in enumerate((mr.closing(f, 4), mr.closing(f, 2), f, mr.opening(f, 2), mr.opening(f, 4), s[:, :, 1], s[:, :, 2])):
        assert np.array_equal(mr.bits(got[:, :, band]), mr.bits(want)), info['order'][band]
    assert info['order'] == mo.band_names(3, 1, (2, 4)) and info['components'] == 1 and info['radii'] == [2, 4]
    # closings lie above the component and grow with the radius, openings below and shrink
    assert (got[:, :, 0] >= got[:, :, 1]).all() and (got[:, :, 1] >= got[:, :, 2]).all()
    assert (got[:, :, 2] >= got[:, :, 3]).all() and (got[:, :, 3] >= got[:, :, 4]).all()


def _arch_cfg(**over):
    cfg = {'DATA_DICT': {'x': {'size': [40, 40, 24]}}, 'data_city': 'x', 'patch_size': 11, 'Categories_Number': 5, 'scale': 1}
    cfg.update(over)
    return cfg


def test_arch_from_cfg_counts_the_profile_bands():
    from dmf.arch import arch_from_cfg
    assert arch_from_cfg(_arch_cfg())['C'] == 24
    assert arch_from_cfg(_arch_cfg(band_reduce='pca', band_reduce_bands=8))['C'] == 8
    assert arch_from_cfg(_arch_cfg(band_reduce='pca', band_reduce_bands=8, band_profile='none'))['C'] == 8
    a = arch_from_cfg(_arch_cfg(band_reduce='pca', band_reduce_bands=8, band_profile='morph'))
    assert a['C'] == 32 and a['G'] == 2                                      # the defaults: P = 4, radii [2, 4, 6]
    a = arch_from_cfg(_arch_cfg(band_reduce='pca', band_reduce_bands=6, band_profile='morph', band_profile_components=2,
                                band_profile_radii=[1, 2, 3, 5]))
    assert a['C'] == 6 + 2 * 4 * 2


def test_keys_and_their_refusals():
    mo = _mo()
    assert mo.profile_keys({}) is None and mo.profile_keys({'band_profile': 'none', 'band_profile_radii': 'junk'}) is None
    on = {'band_reduce': 'pca', 'band_reduce_bands': 8, 'band_profile': 'morph'}
    assert mo.profile_keys(on) == dict(components=4, radii=(2, 4, 6))
    assert mo.profile_keys(dict(on, band_profile_components=8, band_profile_radii=[1, 32])) == dict(components=8, radii=(1, 32))
    with pytest.raises(ValueError, match='band_profile: morph profiles the components of band_reduce: pca, and band_reduce is none'):
        mo.profile_keys({'band_profile': 'morph'})
    with pytest.raises(ValueError, match="band_profile 'disk' is not one of none / morph"):
        mo.profile_keys(dict(on, band_profile='disk'))
    with pytest.raises(ValueError, match='band_profile_components: 9 exceeds the 8 components'):
        mo.profile_keys(dict(on, band_profile_components=9))
    with pytest.raises(ValueError, match='band_profile_components 0 is not a whole number >= 1'):
        mo.profile_keys(dict(on, band_profile_components=0))
    with pytest.raises(ValueError, match='band_profile_radii .* is not strictly increasing'):
        mo.profile_keys(dict(on, band_profile_radii=[2, 2, 4]))
    with pytest.raises(ValueError, match='band_profile_radii .* every radius is a whole number in 1..32'):
        mo.profile_keys(dict(on, band_profile_radii=[2, 33]))
    with pytest.raises(ValueError, match='band_profile_radii .* every radius is a whole number in 1..32'):
        mo.profile_keys(dict(on, band_profile_radii=[0, 3]))
    with pytest.raises(ValueError, match='band_profile_radii .* is not a list of 1..8 whole numbers'):
        mo.profile_keys(dict(on, band_profile_radii=list(range(1, 10))))
    with pytest.raises(ValueError, match='band_profile_radii .* is not a list of 1..8 whole numbers'):
        mo.profile_keys(dict(on, band_profile_radii=[]))


def test_scores_that_are_refused():
    mo = _mo()
    s = mc.scores(33, 37, 3).copy()
    with pytest.raises(ValueError, match='band_profile_components: 4 exceeds the 3 components'):
        mo.profile_host(s, 4, (1, 2))
    s[5, 6, 2] = np.nan                                                    # even in a component that is not profiled
    with pytest.raises(ValueError, match='band_profile: the scores hold a value that is not finite'):
        mo.profile_host(s, 1, (1, 2))
    s[5, 6, 2] = np.inf
    with pytest.raises(ValueError, match='not finite'):
        mo.profile_host(s, 1, (1, 2))
    with pytest.raises(ValueError, match='band_profile wants the float32 scores'):
        mo.profile_host(s.astype(np.float64), 1, (1, 2))


def test_the_library_declares_the_entry_points():
    import ctypes
    from dmf import lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'dmf.h')).read()
    so = ctypes.CDLL(lib.LIB_PATH)
    for name in ('dmf_morph_workspace_bytes', 'dmf_morph_state_bytes', 'dmf_morph_markers', 'dmf_morph_reconstruct', 'dmf_morph_stack'):
        assert name + '(' in hdr and name in lib.EXPORTS and hasattr(so, name), name
    H, W, P, n = 67, 131, 4, 3
    tiles = -(-H // lib.MORPH_TILE) * -(-W // lib.MORPH_TILE)
    state = (4 * 2 * lib.MORPH_BATCH + 2 * (2 * n * P) * tiles + 15) // 16 * 16
    assert lib.morph_state_bytes(H, W, 2 * n * P) == state
    assert lib.morph_workspace_bytes(H, W, P, n) == (2 * P + 4 * n * P) * H * W * 4 + state      # the layout include/dmf.h states
    for bad in ((0, 5, 1, 1), (5, 5, 0, 1), (5, 5, 1, 9), (5, 5, 65, 1), (1 << 16, 1 << 15, 1, 1)):
        with pytest.raises(lib.DmfError, match='dmf_morph_workspace_bytes'):
            lib.morph_workspace_bytes(*bad)


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


def test_base_solver_with_the_key_on_the_drop_in_path(golden_dir, capsys):
    import pca_cases as pca
    from dmf.arch import arch_from_cfg
    from solver.mainsolver import Solver
    from utils import spectral
    mo = _mo()
    tmp = tempfile.mkdtemp(prefix='dmf_morph_')
    try:
        cfg = _cfg(golden_dir, tmp, band_reduce='pca', band_reduce_bands=4, band_profile='morph', band_profile_components=2,
                   band_profile_radii=[1, 3])
        torch.manual_seed(3407)
        s = Solver(cfg)
        reduced, _ = spectral.reduce_host(pca.solver_scene(cfg['Categories_Number'])[0], 4)
        want, _ = mo.profile_host(reduced, 2, (1, 3))
        assert s.ms.shape == (40, 40, 12) and s.ms.dtype == np.float32 and np.array_equal(mr.bits(s.ms), mr.bits(want))
        assert np.array_equal(mr.bits(want), mr.bits(mr.profile(reduced, 2, (1, 3))))
        assert arch_from_cfg(cfg)['C'] == 12 and s.MS.shape[2] == 12
        line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('band_profile:')]
        assert len(line) == 1 and '12 bands' in line[0] and line[0].endswith('host')
        info = json.load(open(cfg['RESULT_output'] + '0_band_profile.json'))
        assert info['order'] == mo.band_names(4, 2, (1, 3)) and len(info['order']) == info['bands'] == 12
        assert info['components'] == 2 and info['radii'] == [1, 3] and info['route'] == 'host' and len(info['rounds']) == 1
    finally:
        shutil.rmtree(tmp)


def test_the_key_at_none_leaves_the_solver_as_it_is(golden_dir):
    from dmf.arch import arch_from_cfg
    from solver.mainsolver import Solver
    tmp = tempfile.mkdtemp(prefix='dmf_morph_')
    try:
        made = []
        for sub, over in (('a', {}), ('b', {'band_profile': 'none', 'band_profile_components': 3, 'band_profile_radii': [1, 2]})):
            cfg = _cfg(golden_dir, os.path.join(tmp, sub), band_reduce='pca', band_reduce_bands=4, **over)
            torch.manual_seed(3407)
            s = Solver(cfg)
            made.append((s.ms.copy(), arch_from_cfg(cfg), s.band_profile_info))
            assert not os.path.exists(cfg['RESULT_output'] + '0_band_profile.json')
        assert made[0][0].tobytes() == made[1][0].tobytes() and made[0][0].shape == (40, 40, 4)
        assert made[0][1] == made[1][1] and made[0][2] is None and made[1][2] is None
        cfg = _cfg(golden_dir, os.path.join(tmp, 'c'))                       # and without band_reduce the scene is the raw one
        raw = np.load(cfg['data_address'] + 'ms4.tif.npy')
        assert Solver(cfg).ms.tobytes() == raw.tobytes()
    finally:
        shutil.rmtree(tmp)


def test_refusals_of_the_key_in_the_solvers(golden_dir):
    from solver.mainsolver import Solver
    from solver.tostagesolver import toStageSolver
    tmp = tempfile.mkdtemp(prefix='dmf_morph_')
    try:
        cfg = _cfg(golden_dir, os.path.join(tmp, 'a'), band_profile='morph')                  # band_reduce: none
        with pytest.raises(ValueError, match='band_profile: morph profiles the components of band_reduce: pca'):
            Solver(cfg)
        cfg = _cfg(golden_dir, os.path.join(tmp, 'b'), band_reduce='pca', band_reduce_bands=4, band_profile='morph')
        with pytest.raises(ValueError, match='band_profile is out of scope for toStageSolver'):
            toStageSolver(copy.deepcopy(cfg))
        cfg = _cfg(golden_dir, os.path.join(tmp, 'c'), band_reduce='pca', band_reduce_bands=4, band_profile='morph',
                   band_profile_components=5)
        with pytest.raises(ValueError, match='band_profile_components: 5 exceeds the 4 components'):
            Solver(cfg)
        cfg = _cfg(golden_dir, os.path.join(tmp, 'd'), band_reduce='pca', band_reduce_bands=4, band_profile='morph',
                   band_profile_radii=[3, 2])
        with pytest.raises(ValueError, match='not strictly increasing'):
            Solver(cfg)
        cfg = _cfg(golden_dir, os.path.join(tmp, 'e'), band_reduce='pca', band_reduce_bands=4, band_profile='morph',
                   band_profile_radii=[2, 40])
        with pytest.raises(ValueError, match='every radius is a whole number in 1..32'):
            Solver(cfg)
        for sub in 'bcde':                                                   # refused before any work
            assert not os.path.exists(os.path.join(tmp, sub, 'out', '0_band_reduce.npz'))
    finally:
        shutil.rmtree(tmp)
