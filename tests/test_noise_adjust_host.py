"""CPU: the host side of `band_reduce_noise` — the key, utils.spectral.fit_noise_adjusted and
reduce_host(noise=...), the guard that the fixture separates the noise-adjusted transform from plain PCA, and BaseSolver on the
drop-in path.  Nothing here needs the GPU or the HIP library."""
import os
import shutil
import tempfile

import numpy as np
import pytest
import torch

import noise_cases as nc
import pca_cases as pca


def _spectral():
    from utils import spectral
    return spectral


# ---------------------------------------------------------------------------------------------- the key
def test_noise_keys_defaults_spellings_and_refusals():
    sp = _spectral()
    assert sp.noise_keys({}) is None and sp.noise_keys({'band_reduce': 'pca'}) is None
    for off in ('none', 'None', None, False, 0):
        assert sp.noise_keys({'band_reduce': 'pca', 'band_reduce_noise': off}) is None
        assert sp.noise_keys({'band_reduce_noise': off}) is None               # neutral beside band_reduce: none
    for spelt, want in (('horizontal', 'horizontal'), ('Vertical', 'vertical'), ('BOTH', 'both')):
        assert sp.noise_keys({'band_reduce': 'pca', 'band_reduce_noise': spelt}) == want
    for bad in ('mnf', 'diagonal', 1, True):
        with pytest.raises(ValueError, match='band_reduce_noise'):
            sp.noise_keys({'band_reduce': 'pca', 'band_reduce_noise': bad})
    for kind in ({}, {'band_reduce': 'none'}, {'band_reduce': None}):
        with pytest.raises(ValueError, match='band_reduce_noise'):
            sp.noise_keys(dict(kind, band_reduce_noise='both'))
    # band_keys gained no entry and `band_reduce` no value
    assert sp.band_keys({}) == dict(kind=None, bands=32, whiten=False)
    assert sp.band_keys({'band_reduce': 'pca', 'band_reduce_noise': 'both'}) == dict(kind='pca', bands=32, whiten=False)
    assert sp.keys_in_use(sp.band_keys({'band_reduce_noise': 'none'})) == []
    with pytest.raises(ValueError, match='band_reduce'):
        sp.band_keys({'band_reduce': 'mnf'})


# ---------------------------------------------------------------------------------------------- fit_noise_adjusted
def _spd_pair(C=12, seed=5):
    rng = np.random.default_rng(seed)
    a, b = rng.standard_normal((3 * C, C)), rng.standard_normal((3 * C, C))
    return rng.standard_normal(C), a.T @ a / (3 * C), b.T @ b / (3 * C) + 0.1 * np.eye(C)


def _columns64(mean, cov, ncov, K, whiten=False):
    """The fit, and its float32 basis widened to float64 for the identities."""
    sp = _spectral()
    fit = sp.fit_noise_adjusted(mean, cov, ncov, K, whiten, noise='both')
    return fit, fit['basis'].astype(np.float64)


def test_fit_noise_adjusted_identities():
    """C = 12, a random SPD pair.  The float32 cast of the basis limits the identities to C 2^-23 times the sizes involved
    (every entry of B is off by 2^-24 relative at most, and a quadratic form takes two of them)."""
    sp = _spectral()
    mean, cov, ncov = _spd_pair()
    C, K = 12, 12
    fit, B = _columns64(mean, cov, ncov, K)
    nu = fit['eigenvalues']
    assert fit['basis'].dtype == np.float32 and fit['basis'].shape == (C, K) and fit['basis'].flags['C_CONTIGUOUS']
    slack = C * 2.0 ** -23 * np.abs(B).T @ np.abs(ncov) @ np.abs(B) + 1e-12
    assert (np.abs(B.T @ ncov @ B - np.eye(K)) <= slack).all()                                  # unit noise variance
    slack = C * 2.0 ** -23 * np.abs(B).T @ np.abs(cov) @ np.abs(B) + 1e-12 * nu[0]
    assert (np.abs(B.T @ cov @ B - np.diag(nu)) <= slack).all()                                 # B^T cov B = diag(nu)
    assert np.all(np.diff(nu) < 0)                                                              # descending
    # nu are the eigenvalues of ncov^-1 cov
    assert np.allclose(np.sort(np.linalg.eigvals(np.linalg.solve(ncov, cov)).real)[::-1], nu, rtol=1e-10, atol=0)
    for k in range(K):                                                                          # the sign rule
        assert B[np.argmax(np.abs(B[:, k])), k] > 0
    assert np.array_equal(fit['snr'], nu - 1.0) and fit['noise'] == 'both'
    assert np.allclose(fit['explained'], nu / nu.sum(), rtol=1e-12) and abs(fit['explained'].sum() - 1.0) < 1e-12
    assert np.allclose(fit['noise_eigenvalues'], np.linalg.eigvalsh(ncov)[::-1], rtol=1e-12) and np.array_equal(fit['mean'], mean)
    part = sp.fit_noise_adjusted(mean, cov, ncov, 5, noise='horizontal')
    assert np.array_equal(part['basis'], fit['basis'][:, :5]) and np.array_equal(part['eigenvalues'], nu[:5])
    assert part['snr'].shape == (5,) and part['explained'].sum() < 1.0 and part['noise_eigenvalues'].shape == (C,)


def test_fit_noise_adjusted_whitening_gives_unit_total_variance():
    mean, cov, ncov = _spd_pair()
    plain, _ = _columns64(mean, cov, ncov, 6)
    white, B = _columns64(mean, cov, ncov, 6, whiten=True)
    slack = 12 * 2.0 ** -23 * np.abs(B).T @ np.abs(cov) @ np.abs(B) + 1e-12
    assert (np.abs(B.T @ cov @ B - np.eye(6)) <= slack).all()
    assert np.array_equal(white['eigenvalues'], plain['eigenvalues'])
    assert np.allclose(white['basis'], plain['basis'] / np.sqrt(plain['eigenvalues'])[None, :].astype(np.float32), rtol=1e-6)


def test_white_noise_reproduces_fit_basis():
    """ncov = I: the whitening is a rotation, and the fit is plain PCA's — the same eigenvalues, the same subspaces."""
    sp = _spectral()
    mean, cov, _ = _spd_pair()
    a, b = sp.fit_noise_adjusted(mean, cov, np.eye(12), 5, noise='both'), sp.fit_basis(mean, cov, 5)
    assert np.allclose(a['eigenvalues'], b['eigenvalues'], rtol=1e-12, atol=0)
    assert np.abs(a['basis'] - b['basis']).max() < 1e-6                      # column by column: the eigenvalues are distinct
    assert nc.largest_angle(a['basis'].astype(np.float64), b['basis'].astype(np.float64)) < 1e-3
    assert np.allclose(a['explained'], b['explained'], rtol=1e-12)


def test_a_singular_noise_estimate_is_refused_by_name():
    sp = _spectral()
    mean, cov, ncov = _spd_pair()
    dup = ncov.copy()
    dup[:, 3], dup[3, :] = dup[:, 2], dup[2, :]
    dup[3, 3] = dup[2, 2]                                                    # band 3 duplicates band 2
    const = ncov.copy()
    const[:, 0] = const[0, :] = 0.0                                          # a constant band has no differences
    for bad in (dup, const, np.zeros((12, 12))):
        with pytest.raises(ValueError, match='band_reduce_noise'):
            sp.fit_noise_adjusted(mean, cov, bad, 4, noise='both')
    with pytest.raises(ValueError, match='band_reduce_bands'):
        sp.fit_noise_adjusted(mean, cov, ncov, 13, noise='both')
    X = pca.scene(6).copy()
    X[:, :, 4] = X[:, :, 1]                                                  # ... and through reduce_host
    with pytest.raises(ValueError, match='band_reduce_noise'):
        sp.reduce_host(X, 2, noise='both')
    with pytest.raises(ValueError, match='band_reduce_noise'):               # no pixel has a right neighbour
        sp.reduce_host(pca.scene(6)[:, :1], 2, noise='horizontal')
    with pytest.raises(ValueError, match='band_reduce_noise'):
        sp.reduce_host(pca.scene(6)[:1], 2, noise='both')


# ---------------------------------------------------------------------------------------------- the fixture separates the transforms
@pytest.mark.parametrize('H,W', nc.SEPARATION_SCENES)
def test_the_noise_adjusted_fit_finds_the_signal_where_pca_follows_the_loud_bands(H, W):
    """Both conditions are asserted, so a fit that silently fell back to PCA fails: plain PCA's first-4 subspace lies at a largest
    principal angle of more than 60 degrees from the signal directions, span(ncov B) of the noise-adjusted fit within 35."""
    sp = _spectral()
    X, Q = nc.smooth_scene(H, W)
    S, C = nc.SEPARATION_SIGNALS, nc.SEPARATION_BANDS
    assert X.shape == (H, W, C) and np.abs(Q.T @ Q - np.eye(S)).max() < 1e-12
    x = sp.normalise(X)
    mean, cov = sp.moments_host(x.reshape(-1, C))
    plain = sp.fit_basis(mean, cov, S)['basis'].astype(np.float64)
    ncov = sp.noise_moments_host(x, 'both')
    fit = sp.fit_noise_adjusted(mean, cov, ncov, S, noise='both')
    a_pca, a_mnf = nc.largest_angle(plain, Q), nc.largest_angle(ncov @ fit['basis'].astype(np.float64), Q)
    print('%d x %d: PCA at %.1f degrees from the signal, noise-adjusted at %.1f; SNR %s' % (H, W, a_pca, a_mnf, np.round(fit['snr'], 2)))
    assert a_pca > 60.0
    assert a_mnf < 35.0
    _, fit_r = sp.reduce_host(X, S, noise='both')                            # reduce_host takes that route
    assert np.array_equal(fit_r['basis'], fit['basis'])


def test_the_end_to_end_fixture_meets_its_guards():
    for H, W, seed in ((pca.H_SCENE, pca.W_SCENE, 0), (40, 40, 1)):
        X = nc.noisy_scene(nc.SOLVER_BANDS, H, W, seed)
        assert X.dtype == np.float32 and X.min() == 0.0 and X.max() == 1.0
        ratios, cond = nc.guards(X, 'both', nc.SOLVER_K)
        print('%d x %d: ratios %.2f .. %.2f, cond(ncov) %.2f' % (H, W, ratios.min(), ratios.max(), cond))
        assert ratios.min() >= nc.MIN_RATIO and cond <= nc.MAX_COND


# ---------------------------------------------------------------------------------------------- reduce_host
@pytest.mark.parametrize('noise', ['horizontal', 'vertical', 'both'])
def test_reduce_host_against_a_direct_restatement(noise):
    """The generalised problem solved another way: cov b = nu ncov b through the Cholesky factor of ncov, the differences by
    np.diff.  Tolerance: the two float32 bases (2^-24 relative per entry, C entries of at most |d|_max |b|_max) and the
    scores' own cast (2^-24 |score|)."""
    sp = _spectral()
    C, K = 24, 8
    X = nc.noisy_scene(C)
    H, W = X.shape[:2]
    scores, fit = sp.reduce_host(X, K, noise=noise)
    assert scores.dtype == np.float32 and scores.shape == (H, W, K) and fit['route'] == 'host' and fit['noise'] == noise
    x = X.astype(np.float64)                                                 # (already in [0, 1]: normalise is the identity)
    eh = -np.diff(x, axis=1).reshape(-1, C)
    ev = -np.diff(x, axis=0).reshape(-1, C)
    nh, nv = eh.T @ eh / (2 * H * (W - 1)), ev.T @ ev / (2 * (H - 1) * W)
    ncov = {'horizontal': nh, 'vertical': nv, 'both': (nh + nv) / 2}[noise]
    flat = x.reshape(-1, C)
    d = flat - flat.mean(axis=0).astype(np.float32).astype(np.float64)
    cov = d.T @ d / (H * W - 1)
    L = np.linalg.cholesky(ncov)
    Li = np.linalg.inv(L)
    nu, Y = np.linalg.eigh(Li @ cov @ Li.T)
    nu, B = nu[::-1][:K], (Li.T @ Y[:, ::-1])[:, :K]
    B = B * np.sign(B[np.argmax(np.abs(B), axis=0), np.arange(K)])
    want = d @ B
    assert np.allclose(fit['eigenvalues'], nu, rtol=1e-9, atol=0) and np.allclose(fit['snr'], nu - 1, rtol=1e-9, atol=1e-12)
    tol = 2.0 ** -24 * (C * np.abs(d).max() * np.abs(B).max() + np.abs(want).max()) + 1e-9 * np.abs(want).max()
    err = np.abs(scores.reshape(-1, K).astype(np.float64) - want).max()
    print('%s: max |scores - restatement| %.2e, tolerance %.2e' % (noise, err, tol))
    assert err <= tol
    # the scores have unit noise variance: their shift differences, in the direction(s) of the fit
    s = scores.astype(np.float64)
    parts = {'horizontal': [np.diff(s, axis=1)], 'vertical': [np.diff(s, axis=0)], 'both': [np.diff(s, axis=1), np.diff(s, axis=0)]}[noise]
    var = np.mean([(p.reshape(-1, K) ** 2).mean(axis=0) / 2 for p in parts], axis=0)
    assert np.allclose(var, 1.0, atol=1e-5)


def test_reduce_host_without_the_argument_is_what_it_was():
    sp = _spectral()
    X = pca.scene(24)
    a, fa = sp.reduce_host(X, 8)
    b, fb = sp.reduce_host(X, 8, False, noise=None)
    assert np.array_equal(a, b) and sorted(fa) == sorted(fb) == ['basis', 'eigenvalues', 'explained', 'mean', 'route']


# ---------------------------------------------------------------------------------------------- BaseSolver, drop-in path
def _cfg(golden_dir, tmp, **over):
    from test_gpu_trajectory import _setup
    _, cfg = _setup(golden_dir, tmp, device='cpu', fast_path=0, scale=1, epoch=1, **over)
    primary, aux, label = nc.solver_scene(cfg['Categories_Number'])
    d = cfg['data_address']
    np.save(d + 'ms4.tif.npy', primary); np.save(d + 'pan.tif.npy', aux); np.save(d + 'label.npy', label)
    cfg['DATA_DICT'][cfg['data_city']]['size'] = [40, 40, nc.SOLVER_BANDS]
    return cfg


def test_base_solver_with_the_key_on_the_drop_in_path(golden_dir, capsys):
    from solver.mainsolver import Solver
    sp = _spectral()
    K = nc.SOLVER_K
    tmp = tempfile.mkdtemp(prefix='dmf_noise_')
    try:
        cfg = _cfg(golden_dir, os.path.join(tmp, 'on'), band_reduce='pca', band_reduce_bands=K, band_reduce_noise='both')
        torch.manual_seed(3407)
        s = Solver(cfg)
        want, fit = sp.reduce_host(nc.solver_scene(cfg['Categories_Number'])[0], K, noise='both')
        assert s.ms.shape == (40, 40, K) and s.ms.dtype == np.float32 and np.array_equal(s.ms, want)
        line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('band_reduce:')]
        assert len(line) == 1 and 'noise-adjusted (both)' in line[0] and 'SNR' in line[0] and line[0].endswith('host')
        z = np.load(cfg['RESULT_output'] + '0_band_reduce.npz')
        assert sorted(z.files) == ['basis', 'eigenvalues', 'explained', 'mean', 'noise', 'noise_eigenvalues', 'route', 'snr']
        assert str(z['noise']) == 'both' and str(z['route']) == 'host' and np.array_equal(z['basis'], fit['basis'])
        assert z['snr'].shape == (K,) and np.array_equal(z['snr'], z['eigenvalues'] - 1) and np.all(np.diff(z['snr']) < 0)
        assert z['noise_eigenvalues'].shape == (nc.SOLVER_BANDS,) and np.all(z['noise_eigenvalues'] > 0)
        # the net is built for the components (it runs on the GPU only: the drop-in path trains on them in
        # tests/test_gpu_noise_adjust.py::test_solver_on_the_drop_in_path_trains_on_the_components)
        s.dataloader()
        s.init_model()
        assert s.model.arch['C'] == K

        # the key off or at none: the five arrays, and the PCA fit
        for name, over in (('off', {}), ('none', {'band_reduce_noise': 'none'})):
            cfg = _cfg(golden_dir, os.path.join(tmp, name), band_reduce='pca', band_reduce_bands=K, **over)
            s = Solver(cfg)
            z = np.load(cfg['RESULT_output'] + '0_band_reduce.npz')
            assert sorted(z.files) == ['basis', 'eigenvalues', 'explained', 'mean', 'route']
            assert np.array_equal(s.ms, sp.reduce_host(nc.solver_scene(cfg['Categories_Number'])[0], K)[0])
    finally:
        shutil.rmtree(tmp)


def test_refusals_of_the_key_in_the_solvers(golden_dir):
    from solver.mainsolver import Solver
    from solver.tostagesolver import toStageSolver
    tmp = tempfile.mkdtemp(prefix='dmf_noise_')
    try:
        cfg = _cfg(golden_dir, os.path.join(tmp, 'a'), band_reduce_noise='both')              # band_reduce: none
        with pytest.raises(ValueError, match='band_reduce_noise'):
            Solver(cfg)
        cfg = _cfg(golden_dir, os.path.join(tmp, 'b'), band_reduce='pca', band_reduce_bands=4, band_reduce_noise='vertical')
        with pytest.raises(ValueError, match='band_reduce_noise is out of scope for toStageSolver'):
            toStageSolver(cfg)
        cfg = _cfg(golden_dir, os.path.join(tmp, 'c'), band_reduce='pca', band_reduce_bands=4, band_reduce_noise='diagonal')
        with pytest.raises(ValueError, match='band_reduce_noise'):
            Solver(cfg)
        assert not os.path.exists(cfg['RESULT_output'] + '0_band_reduce.npz')
    finally:
        shutil.rmtree(tmp)
