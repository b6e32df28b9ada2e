"""CPU: the host side of `band_reduce: pca` — the fixture's guard, utils.spectral.fit_basis and reduce_host,
dmf.arch.arch_from_cfg with the key, and BaseSolver on the drop-in path.  Nothing here needs the GPU or the HIP library."""
import os
import shutil
import tempfile

import numpy as np
import pytest
import torch

import pca_cases as pca


def _spectral():
    from utils import spectral
    return spectral


# ---------------------------------------------------------------------------------------------- the fixture
@pytest.mark.parametrize('C,K', [(24, 8), (200, 32), (203, 32)])
def test_the_fixture_has_a_defined_basis(C, K):
    """A condition, not a measurement: every consecutive ratio among the first K + 1 sample eigenvalues is >= 1.5."""
    X = pca.scene(C)
    assert X.dtype == np.float32 and X.shape == (pca.H_SCENE, pca.W_SCENE, C) and X.min() == 0.0 and X.max() == 1.0
    r = pca.eigen_ratios(X, K)
    print('C = %d: eigenvalue ratios %.2f .. %.2f' % (C, r.min(), r.max()))
    assert r.min() >= pca.MIN_RATIO


def test_the_solver_scene_has_a_defined_basis():
    primary, aux, label = pca.solver_scene(5)
    assert primary.shape == (40, 40, pca.SOLVER_BANDS) and aux.shape == (40, 40) and set(np.unique(label)) == {0, 1, 2, 3, 4}
    assert pca.eigen_ratios(primary, pca.SOLVER_K).min() >= pca.MIN_RATIO


# ---------------------------------------------------------------------------------------------- fit_basis
def _moments(C=24):
    sp = _spectral()
    x = pca.scene(C).reshape(-1, C)
    return (x,) + sp.moments_host(x)


def test_fit_basis_order_sign_and_explained_variance():
    sp = _spectral()
    x, mean, cov = _moments()
    fit = sp.fit_basis(mean, cov, 8)
    lam_all = np.linalg.eigvalsh(cov)[::-1]
    assert fit['basis'].dtype == np.float32 and fit['basis'].shape == (24, 8) and fit['basis'].flags['C_CONTIGUOUS']
    assert np.all(np.diff(fit['eigenvalues']) < 0) and np.allclose(fit['eigenvalues'], lam_all[:8], rtol=1e-12, atol=0)
    assert np.allclose(fit['explained'], lam_all[:8] / lam_all.sum(), rtol=1e-12, atol=0) and fit['explained'].sum() < 1.0
    full = sp.fit_basis(mean, cov, 24)
    assert abs(full['explained'].sum() - 1.0) < 1e-12
    for k in range(8):                                   # the component of largest magnitude is positive
        v = fit['basis'][:, k]
        assert v[np.argmax(np.abs(v))] > 0
    assert np.array_equal(fit['mean'], mean)
    # eigenvectors: cov v = lambda v, in float64 before the cast
    b = fit['basis'].astype(np.float64)
    assert np.abs(cov @ b - b * fit['eigenvalues']).max() < 1e-7 * lam_all[0]


def test_the_sign_rule_takes_the_first_component_on_a_tie():
    sp = _spectral()
    v = np.array([[-0.5, 0.5, 0.1], [0.5, -0.5, -0.9], [0.5, 0.5, 0.2]])
    got = sp.sign_columns(v)
    assert np.array_equal(got, v * np.array([-1.0, 1.0, -1.0]))
    assert np.array_equal(sp.sign_columns(got), got)
    fit = sp.fit_basis(np.zeros(2), np.array([[2.0, 1.0], [1.0, 2.0]]), 2)
    assert np.allclose(fit['eigenvalues'], [3.0, 1.0]) and np.allclose(np.abs(fit['basis']), np.sqrt(0.5))
    assert fit['basis'][0, 0] * fit['basis'][1, 0] > 0 and fit['basis'][0, 1] * fit['basis'][1, 1] < 0


def test_fit_basis_columns_are_orthonormal():
    sp = _spectral()
    _, mean, cov = _moments(200)
    lam, vec = np.linalg.eigh(cov, UPLO='U')             # (fit_basis reads the upper triangle)
    fit = sp.fit_basis(mean, cov, 32)
    # to 1e-12 in float64: the columns before the cast to float32 are eigh's, re-signed
    v = vec[:, ::-1][:, :32]
    v = v * np.sign(v[np.argmax(np.abs(v), axis=0), np.arange(32)])
    assert np.abs(v.T @ v - np.eye(32)).max() < 1e-12
    assert np.array_equal(fit['basis'], v.astype(np.float32))
    # and what float32 leaves of it
    b = fit['basis'].astype(np.float64)
    assert np.abs(b.T @ b - np.eye(32)).max() < 200 * 2.0 ** -24


def test_fit_basis_whitening():
    sp = _spectral()
    x, mean, cov = _moments()
    plain, white = sp.fit_basis(mean, cov, 8), sp.fit_basis(mean, cov, 8, whiten=True)
    assert np.allclose(white['basis'], plain['basis'] / np.sqrt(plain['eigenvalues'])[None, :].astype(np.float32), rtol=1e-6)
    assert np.array_equal(white['eigenvalues'], plain['eigenvalues'])
    scores = sp.reduce_host(pca.scene(24), 8, whiten=True)[0].reshape(-1, 8).astype(np.float64)
    assert np.allclose(scores.var(axis=0, ddof=1), 1.0, atol=1e-5)
    assert np.abs(np.cov(scores, rowvar=False) - np.eye(8)).max() < 1e-5


def test_fit_basis_refusals():
    sp = _spectral()
    _, mean, cov = _moments()
    with pytest.raises(ValueError, match='band_reduce_bands'):
        sp.fit_basis(mean, cov, 25)
    with pytest.raises(ValueError, match='band_reduce_bands'):
        sp.fit_basis(mean, cov, 0)
    flat = np.diag([1.0, 0.5, 0.0])                      # a non-positive eigenvalue under whitening
    assert sp.fit_basis(np.zeros(3), flat, 3)['eigenvalues'][2] <= 1e-300
    with pytest.raises(ValueError, match='band_reduce_whiten'):
        sp.fit_basis(np.zeros(3), flat, 3, whiten=True)
    with pytest.raises(ValueError, match='band_reduce_whiten'):
        sp.fit_basis(np.zeros(3), np.diag([1.0, 0.5, -1e-9]), 3, whiten=True)
    assert sp.fit_basis(np.zeros(3), flat, 2, whiten=True)['basis'].shape == (3, 2)     # the first two are positive


def test_band_keys():
    sp = _spectral()
    assert sp.band_keys({}) == dict(kind=None, bands=32, whiten=False)
    assert sp.band_keys({'band_reduce': 'none', 'band_reduce_bands': 8})['kind'] is None
    assert sp.band_keys({'band_reduce': 'PCA', 'band_reduce_bands': 8, 'band_reduce_whiten': 1}) == dict(kind='pca', bands=8, whiten=True)
    assert sp.keys_in_use(sp.band_keys({'band_reduce': 'pca'})) == ['band_reduce'] and sp.keys_in_use(sp.band_keys({})) == []
    for bad in ({'band_reduce': 'mnf'}, {'band_reduce_bands': 0}, {'band_reduce_bands': 2.5}, {'band_reduce_bands': True},
                {'band_reduce_whiten': 2}):
        with pytest.raises(ValueError, match='band_reduce'):
            sp.band_keys(bad)


# ---------------------------------------------------------------------------------------------- reduce_host
@pytest.mark.parametrize('C,K', [(24, 8), (3, 3), (1, 1), (203, 32)])
def test_reduce_host_against_a_direct_svd(C, K):
    """The scores are the left singular vectors times the singular values of the centred scene, up to the sign rule.  The
    centred pixel is x - float32(mean) (module text of utils.spectral).  Tolerance: the basis is rounded to float32 (a relative
    2^-24 per component, C components of at most |d|_max each) and so are the scores (2^-24 |score|)."""
    sp = _spectral()
    X = pca.scene(C)
    scores, fit = sp.reduce_host(X, K)
    assert scores.dtype == np.float32 and scores.shape == (pca.H_SCENE, pca.W_SCENE, K) and fit['route'] == 'host'
    x = X.reshape(-1, C)
    d = sp.centred(x, x.astype(np.float64).mean(axis=0))
    U, S, Vt = np.linalg.svd(d, full_matrices=False)
    V = Vt[:K].T
    sign = np.sign(V[np.argmax(np.abs(V), axis=0), np.arange(K)])
    want = (U[:, :K] * S[:K]) * sign
    tol = 2.0 ** -24 * (C * np.abs(d).max() + np.abs(want).max()) + 1e-12
    err = np.abs(scores.reshape(-1, K).astype(np.float64) - want).max()
    print('C = %d, K = %d: max |scores - svd| %.2e, tolerance %.2e' % (C, K, err, tol))
    assert err <= tol
    assert np.allclose(fit['eigenvalues'], S[:K] ** 2 / (x.shape[0] - 1), rtol=1e-10, atol=1e-18)


def test_reduce_host_normalises_as_to_tensor_does_and_refuses_too_many_bands():
    sp = _spectral()
    X = pca.scene(24)
    raw = np.round(X * 1000).astype(np.uint16)           # an integer scene, as the readers deliver them
    from function.function import to_tensor
    assert np.array_equal(sp.normalise(raw), to_tensor(raw).astype(np.float32))
    a, _ = sp.reduce_host(raw, 4)
    b, _ = sp.reduce_host(to_tensor(raw), 4)              # min-max of a normalised scene is the identity
    assert np.allclose(a, b, atol=1e-6)
    with pytest.raises(ValueError, match='band_reduce_bands'):
        sp.reduce_host(X, 25)


# ---------------------------------------------------------------------------------------------- arch_from_cfg
def test_arch_from_cfg_with_the_key_on_and_off():
    from dmf.arch import arch_from_cfg, auto_groups
    cfg = {'patch_size': 11, 'Categories_Number': 17, 'data_city': 's', 'DATA_DICT': {'s': {'size': [64, 64, 103]}}, 'scale': 1,
           'aux_bands': 1, 'gmf': {'width': 40}}
    off = arch_from_cfg(cfg)
    assert off['C'] == 103 and off['G'] == 1
    assert arch_from_cfg(dict(cfg, band_reduce='none', band_reduce_bands=32)) == off
    on = arch_from_cfg(dict(cfg, band_reduce='pca'))
    assert on['C'] == 32 and on['G'] == auto_groups(32, 40) == 2
    assert arch_from_cfg(dict(cfg, band_reduce='pca', band_reduce_bands=8))['C'] == 8
    assert {k: v for k, v in on.items() if k not in ('C', 'G')} == {k: v for k, v in off.items() if k not in ('C', 'G')}


# ---------------------------------------------------------------------------------------------- BaseSolver, drop-in path
def _cfg(golden_dir, tmp, **over):
    from test_gpu_trajectory import _setup
    _, cfg = _setup(golden_dir, tmp, device='cpu', fast_path=0, scale=1, epoch=1, **over)
    primary, aux, label = pca.solver_scene(cfg['Categories_Number'])
    d = cfg['data_address']
    np.save(d + 'ms4.tif.npy', primary); np.save(d + 'pan.tif.npy', aux); np.save(d + 'label.npy', label)
    cfg['DATA_DICT'][cfg['data_city']]['size'] = [40, 40, pca.SOLVER_BANDS]
    return cfg


def test_base_solver_reduces_the_scene_on_the_drop_in_path(golden_dir, monkeypatch):
    import solver.basesolver as bs
    from solver.mainsolver import Solver
    sp = _spectral()
    tmp = tempfile.mkdtemp(prefix='dmf_pca_')
    try:
        cfg = _cfg(golden_dir, os.path.join(tmp, 'on'), band_reduce='pca', band_reduce_bands=pca.SOLVER_K)
        torch.manual_seed(3407)
        s = Solver(cfg)
        want, fit = sp.reduce_host(pca.solver_scene(cfg['Categories_Number'])[0], pca.SOLVER_K)
        assert s.ms.shape == (40, 40, pca.SOLVER_K) and s.ms.dtype == np.float32 and np.array_equal(s.ms, want)
        assert s.MS.shape == (44, 44, pca.SOLVER_K) and s.MS.min() == 0.0 and s.MS.max() == 1.0
        z = np.load(cfg['RESULT_output'] + '0_band_reduce.npz')
        assert sorted(z.files) == ['basis', 'eigenvalues', 'explained', 'mean', 'route']
        assert z['basis'].shape == (pca.SOLVER_BANDS, pca.SOLVER_K) and np.array_equal(z['basis'], fit['basis'])
        assert z['eigenvalues'].shape == (pca.SOLVER_K,) and np.all(np.diff(z['eigenvalues']) < 0) and str(z['route']) == 'host'
        assert np.array_equal(z['mean'], fit['mean']) and np.array_equal(z['explained'], fit['explained'])
        # the net is built for the components
        s.dataloader()
        s.init_model()
        assert s.model.arch['C'] == pca.SOLVER_K

        # an unchanged config: self.ms is the very array read_tif returned, and no file appears
        cfg = _cfg(golden_dir, os.path.join(tmp, 'off'))
        seen = []
        real = bs.read_tif
        monkeypatch.setattr(bs, 'read_tif', lambda c, m: seen.append(real(c, m)) or seen[-1])
        s = Solver(cfg)
        assert s.ms is seen[0] and s.band_fit is None and s.ms.shape[2] == pca.SOLVER_BANDS
        assert not os.path.exists(cfg['RESULT_output'] + '0_band_reduce.npz')
        s2 = Solver(dict(cfg, band_reduce='none', band_reduce_bands=8, band_reduce_whiten=0))
        assert s2.ms is seen[2] and s2.band_fit is None
    finally:
        shutil.rmtree(tmp)


def test_refusals_of_the_key(golden_dir):
    from solver.mainsolver import Solver
    from solver.tostagesolver import toStageSolver
    tmp = tempfile.mkdtemp(prefix='dmf_pca_')
    try:
        cfg = _cfg(golden_dir, os.path.join(tmp, 'a'), band_reduce='pca', band_reduce_bands=pca.SOLVER_BANDS + 1)
        with pytest.raises(ValueError, match='band_reduce_bands'):
            Solver(cfg)
        cfg = _cfg(golden_dir, os.path.join(tmp, 'b'), band_reduce='pca', band_reduce_bands=4)
        with pytest.raises(ValueError, match='band_reduce is out of scope for toStageSolver'):
            toStageSolver(cfg)
    finally:
        shutil.rmtree(tmp)
