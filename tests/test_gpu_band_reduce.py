"""GPU: `band_reduce: pca` — dmf_band_moments and dmf_band_project against float64 numpy on the same fp32
pixels, the device route against utils.spectral.reduce_host, the solver with the key against the oracle on the reduce_host
scene, and the 32-band row of the patch kernel against the oracle in the manner of tests/parity_cases.py.

Bounds (tests/pca_cases.py states them next to the references; they come from the number formats and R, never from the
kernels' output):
  mean        |mean - mean64| <= 2^-50 N max|x|
  covariance  |cov_ij - cov64_ij| <= (R + 4) 2^-24 A_ij + 2^-48 |m_i m_j|,  A_ij = sum_n |d_ni| |d_nj| / (N - 1)
  projection  |y - y64| <= (C + 3) 2^-24 sum_c |x_c - m_c| |basis_ck|
  end to end  Davis-Kahan: sin theta <= 2 |E|_F / gap with E the covariance bound and gap the smallest of the first K eigen-gaps,
              times the largest centred row norm, plus the projection bound
Every comparison prints its worst share of the bound."""
import copy
import ctypes
import os
import shutil
import tempfile

import numpy as np
import pytest
import torch

import pca_cases as pca

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def _R():
    from dmf import lib
    return lib.PCA_RUN


def _pixels(C, N):
    """The first N pixels of the fixture scene of C bands (a larger scene of the same recipe where 37 x 41 is too few)."""
    side = 37 if N <= 37 * 41 else int(np.ceil(np.sqrt(N)))
    X = pca.scene(C) if N <= 37 * 41 else pca.scene(C, side, side)
    return X.reshape(-1, C)[:N].copy()                    # (the fixture is read-only; torch wants a writable array)


def _pitched(x, extra):
    """x [N, C] on the device as rows `C + extra` floats apart; the gaps hold NaN."""
    N, C = x.shape
    buf = torch.full((N, C + extra), float('nan'), device=DEV)
    buf[:, :C] = torch.from_numpy(x).to(DEV)
    return buf[:, :C]


# ---------------------------------------------------------------------------------------------- 1. moments
def _run_moments(xd):
    from dmf import lib
    C = xd.shape[1]
    mean = torch.full((C,), float('nan'), dtype=torch.float64, device=DEV)
    cov = torch.full((C, C), float('nan'), dtype=torch.float64, device=DEV)
    lib.band_moments(xd, mean, cov)
    torch.cuda.synchronize()
    return mean.cpu().numpy(), cov.cpu().numpy()


def _check_moments(x, xd, what):
    R = _R()
    mean, cov = _run_moments(xd)
    mean64, cov64, mean_tol, cov_tol = pca.moments_ref(x, R)
    em, ec = np.abs(mean - mean64).max() / mean_tol, (np.abs(cov - cov64) / cov_tol).max()
    print('moments %s: mean at %.3f of its bound, covariance at %.3f' % (what, em, ec))
    assert np.isfinite(mean).all() and np.isfinite(cov).all()
    assert em <= 1.0 and ec <= 1.0
    assert np.array_equal(cov, cov.T), 'cov[i][j] and cov[j][i] differ ' + what
    assert (np.diagonal(cov) >= 0).all()
    mean2, cov2 = _run_moments(xd)
    assert mean.tobytes() == mean2.tobytes() and cov.tobytes() == cov2.tobytes(), 'two runs differ ' + what
    return mean, cov


def _moment_sizes():
    R = 256                                              # DMF_PCA_RUN, asserted below
    return (2, R - 1, R, R + 1, 37 * 41)


@pytest.mark.parametrize('N', _moment_sizes())
@pytest.mark.parametrize('C', pca.KERNEL_BANDS)
def test_moments_against_float64(C, N):
    assert _R() == 256
    x = _pixels(C, N)
    _check_moments(x, torch.from_numpy(x).to(DEV), '[C = %d, N = %d]' % (C, N))


def test_moments_with_a_row_pitch():
    x = _pixels(203, 37 * 41)
    xd = _pitched(x, 5)
    assert xd.stride(0) == 208 and not xd.is_contiguous()
    got = _check_moments(x, xd, '[C = 203, pitch = C + 5]')
    plain = _run_moments(torch.from_numpy(x).to(DEV))
    assert got[0].tobytes() == plain[0].tobytes() and got[1].tobytes() == plain[1].tobytes()     # the pitch changes no bit


@pytest.mark.parametrize('C,N', [(203, 103 * 256 + 7), (512, 17 * 19)])
def test_moments_where_a_slice_owns_two_runs_and_at_the_widest_scene(C, N):
    """The other paths of the plan (csrc/dmf_pca.hip, pca_plan): 10 macro-tile pairs at 203 bands leave 76 slices, so 104 runs
    put two runs into a slice; 512 bands are the 8 x 8 macro tiles, 36 pairs."""
    x = _pixels(C, N)
    _check_moments(x, torch.from_numpy(x).to(DEV), '[C = %d, N = %d]' % (C, N))


def test_moments_refusals_leave_the_outputs_as_they_were():
    from dmf import lib
    x = torch.from_numpy(_pixels(24, 300)).to(DEV)
    mean = torch.full((24,), 7.0, dtype=torch.float64, device=DEV)
    cov = torch.full((24, 24), 7.0, dtype=torch.float64, device=DEV)
    ws = torch.zeros(lib.band_moments_workspace_bytes(300, 24) // 8, dtype=torch.float64, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    f = lib._lib.dmf_band_moments
    codes = [f(None, 300, 24, 24, p(mean), p(cov), p(ws), None), f(p(x), 300, 24, 24, None, p(cov), p(ws), None),
             f(p(x), 300, 24, 24, p(mean), None, p(ws), None), f(p(x), 300, 24, 24, p(mean), p(cov), None, None),
             f(p(x), 1, 24, 24, p(mean), p(cov), p(ws), None), f(p(x), 300, 0, 24, p(mean), p(cov), p(ws), None),
             f(p(x), 300, 513, 513, p(mean), p(cov), p(ws), None), f(p(x), 300, 24, 23, p(mean), p(cov), p(ws), None),
             f(p(x), 2 ** 61, 24, 24, p(mean), p(cov), p(ws), None)]
    torch.cuda.synchronize()
    assert codes == [1, 1, 1, 1, 2, 3, 3, 5, 8]
    assert (mean == 7.0).all() and (cov == 7.0).all()
    assert lib._lib.dmf_band_moments_workspace_bytes(1, 24) == -1 and lib._lib.dmf_band_moments_workspace_bytes(300, 513) == -1
    with pytest.raises(lib.DmfError, match='N >= 2'):
        lib.band_moments(x[:1], mean, cov)
    with pytest.raises(lib.DmfError, match='workspace'):
        lib.band_moments(x, mean, cov, ws[:8])
    assert (mean == 7.0).all() and (cov == 7.0).all()


# ---------------------------------------------------------------------------------------------- 2. projection
def _basis(C, K, seed=3):
    return (np.random.default_rng(seed).standard_normal((C, K)) / np.sqrt(C)).astype(np.float32)


def _run_project(xd, mean_d, basis_d):
    from dmf import lib
    y = torch.full((xd.shape[0], basis_d.shape[1]), float('nan'), device=DEV)
    lib.band_project(xd, mean_d, basis_d, y)
    torch.cuda.synchronize()
    return y.cpu().numpy()


def _check_project(C, K, N, extra=0):
    full = _pixels(C, 37 * 41)
    mean = full.astype(np.float64).mean(axis=0)
    x, basis = full[:N], _basis(C, K)
    xd = _pitched(x, extra) if extra else torch.from_numpy(x).to(DEV)
    mean_d, basis_d = torch.from_numpy(mean).to(DEV), torch.from_numpy(basis).to(DEV)
    y = _run_project(xd, mean_d, basis_d)
    y64, tol = pca.project_ref(x, mean, basis)
    share = (np.abs(y - y64) / tol).max()
    print('project [C = %d, K = %d, N = %d%s]: at %.3f of its bound' % (C, K, N, ', pitch = C + %d' % extra if extra else '', share))
    assert np.isfinite(y).all() and share <= 1.0
    assert y.tobytes() == _run_project(xd, mean_d, basis_d).tobytes(), 'two runs differ'
    return y


PROJECT_CELLS = [(C, K) for C in pca.KERNEL_BANDS for K in (1, 8, 32) if K <= C]


@pytest.mark.parametrize('N', [1, 63, 64, 65, 37 * 41])
@pytest.mark.parametrize('C,K', PROJECT_CELLS)
def test_project_against_float64(C, K, N):
    _check_project(C, K, N)


@pytest.mark.parametrize('C,K', [(200, 17), (203, 48), (203, 64), (24, 24)])
def test_project_at_every_count_of_column_tiles(C, K):
    """K = 17, 48 and 64 are two, three and four 16-column tiles (band_project_kernel<NT>); K = C is the full rotation."""
    _check_project(C, K, 37 * 41)


def test_project_with_a_row_pitch_and_its_refusals():
    from dmf import lib
    y = _check_project(203, 32, 37 * 41, extra=5)
    assert y.tobytes() == _check_project(203, 32, 37 * 41).tobytes()                             # the pitch changes no bit
    x = torch.from_numpy(_pixels(24, 100)).to(DEV)
    mean = torch.zeros(24, dtype=torch.float64, device=DEV)
    basis = torch.from_numpy(_basis(24, 8)).to(DEV)
    out = torch.full((100, 8), 7.0, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    f = lib._lib.dmf_band_project
    codes = [f(None, 100, 24, 24, p(mean), p(basis), 8, p(out), None), f(p(x), 100, 24, 24, None, p(basis), 8, p(out), None),
             f(p(x), 100, 24, 24, p(mean), None, 8, p(out), None), f(p(x), 100, 24, 24, p(mean), p(basis), 8, None, None),
             f(p(x), -1, 24, 24, p(mean), p(basis), 8, p(out), None), f(p(x), 100, 513, 513, p(mean), p(basis), 8, p(out), None),
             f(p(x), 100, 24, 24, p(mean), p(basis), 0, p(out), None), f(p(x), 100, 24, 24, p(mean), p(basis), 25, p(out), None),
             f(p(x), 100, 200, 200, p(mean), p(basis), 65, p(out), None), f(p(x), 100, 24, 23, p(mean), p(basis), 8, p(out), None),
             f(p(x), 2 ** 61, 24, 24, p(mean), p(basis), 8, p(out), None), f(p(x), 0, 24, 24, p(mean), p(basis), 8, p(out), None)]
    torch.cuda.synchronize()
    assert codes == [1, 1, 1, 1, 2, 3, 4, 4, 4, 5, 8, 0]                                       # (N == 0: a no-op)
    assert (out == 7.0).all()
    lib.band_project(x[:0], mean, basis, out[:0])
    with pytest.raises(lib.DmfError, match='band_project wants'):
        lib.band_project(x, mean, basis, out[:50])


# ---------------------------------------------------------------------------------------------- 3. end to end on the device
def test_device_route_against_reduce_host():
    from dmf.engine import band_reduce
    from utils import spectral
    K, C = pca.SOLVER_K, 24
    raw = np.round(pca.scene(C) * 4000.0).astype(np.uint16)                  # a scene as the readers deliver it
    x = spectral.normalise(raw).reshape(-1, C)
    assert pca.eigen_ratios(x, K).min() >= pca.MIN_RATIO                     # the basis is defined (the fixture's guard)
    want, fit_h = spectral.reduce_host(raw, K)
    got, fit_d = band_reduce(raw, K, False, DEV)
    assert got.dtype == np.float32 and got.shape == want.shape and fit_d['route'] == 'device'
    # the tolerance, from the covariance bound and the fixture's smallest eigen-gap
    mean64, cov64, _, cov_tol = pca.moments_ref(x, _R())
    lam = np.linalg.eigvalsh(cov64)[::-1]
    gap = np.min(lam[:K] - lam[1:K + 1])
    d = spectral.centred(x, mean64)
    sin_theta = 2.0 * np.linalg.norm(cov_tol) / gap
    tol = sin_theta * np.linalg.norm(d, axis=1).max() + pca.project_ref(x, mean64, fit_h['basis'])[1].max()
    err = np.abs(got.astype(np.float64) - want.astype(np.float64)).max()
    print('device route vs reduce_host: max |diff| %.2e, tolerance %.2e (sin theta <= %.2e), score range %.2f'
          % (err, tol, sin_theta, float(want.max() - want.min())))
    assert tol < 1e-2 * (want.max() - want.min())                            # a tolerance below a hundredth of the scores' range
    assert err <= tol
    assert np.allclose(fit_d['eigenvalues'], fit_h['eigenvalues'], rtol=1e-5, atol=0)
    assert np.abs(fit_d['mean'] - fit_h['mean']).max() <= 2.0 ** -50 * x.shape[0]
    # whitened: unit variance of every component
    white, fit_w = band_reduce(raw, K, True, DEV)
    assert np.allclose(white.reshape(-1, K).astype(np.float64).var(axis=0, ddof=1), 1.0, atol=1e-4)
    with pytest.raises(ValueError, match='band_reduce_bands'):
        band_reduce(raw, C + 1, False, DEV)


# ---------------------------------------------------------------------------------------------- 4. the solver
def _cfg(golden_dir, tmp, **over):
    from test_gpu_trajectory import _setup
    _, cfg = _setup(golden_dir, tmp, **dict(dict(epoch=2, scale=1, train_rate=0.3, verify_rate=0.1, steps_per_graph=-1, seed=123,
                                                 band_reduce='pca', band_reduce_bands=pca.SOLVER_K), **over))
    primary, aux, label = pca.solver_scene(cfg['Categories_Number'])
    d = cfg['data_address']
    np.save(d + 'ms4.tif.npy', primary); np.save(d + 'pan.tif.npy', aux); np.save(d + 'label.npy', label)
    cfg['DATA_DICT'][cfg['data_city']]['size'] = [40, 40, pca.SOLVER_BANDS]
    cfg['test']['full'] = 1
    cfg['color']['index'] = 1
    return cfg


def test_solver_with_the_key_against_the_oracle_on_the_reduce_host_scene(golden_dir):
    """Patch 5, 8 components: the existing row 8/1/5/1/40/2.  The first step's loss and the logits of one evaluation batch agree
    with the oracle on the reduce_host scene to the tolerances tests/test_gpu_parity.py holds that row to (loss 1e-5, logits
    1e-5); test() and color() run through; the .npz holds K descending eigenvalues."""
    from dmf.engine import EvalEngine
    from function.function import data_padding, data_padding_aux
    from model.gmfnet import Net as HipNet
    from oracle import solver_ref
    from oracle.gmfnet_ref import Net as RefNet
    from solver.mainsolver import Solver
    from utils import spectral
    tmp = tempfile.mkdtemp(prefix='dmf_pca_')
    try:
        cfg = _cfg(golden_dir, tmp)
        K, P, B = pca.SOLVER_K, cfg['patch_size'], cfg['batchsize']
        torch.manual_seed(3407)
        s = Solver(cfg)
        assert s.ms.shape == (40, 40, K) and s.ms.dtype == np.float32 and s.band_fit['route'] == 'device'
        assert s.scene.A.shape == (40 + P - 1, 40 + P - 1, K)
        s.dataloader()
        rng = torch.get_rng_state()
        s.train()
        assert len(s.step_losses) == 2 * s._steps_per_epoch() and np.isfinite(s.step_losses).all()
        assert s.cur_model.arch['C'] == K and s.cur_model.arch['G'] == 2

        # the oracle on the reduce_host scene: train()'s draws again — the net's initialisation, then the first epoch's order
        primary, aux, _ = pca.solver_scene(cfg['Categories_Number'])
        reduced, _ = spectral.reduce_host(primary, K)
        MS = data_padding(reduced, cfg, 'ms').astype(np.float32)
        PAN = data_padding_aux(aux, cfg).astype(np.float32)
        ocfg = copy.deepcopy(cfg)
        ocfg['DATA_DICT'][cfg['data_city']]['size'] = [40, 40, K]            # the oracle is called with C = K
        torch.set_rng_state(rng)
        init = HipNet(cfg).state_dict()
        xy, lab = s._epoch_streams(1)
        ref = RefNet(ocfg)
        ref.load_state_dict(init)
        want, _ = solver_ref.train_steps(ref, MS, PAN, xy[0, :B].numpy(), lab[0, :B].numpy(), B, P, 1, lr=cfg['schedule']['lr'])
        print('first step: loss %.7f, oracle %.7f' % (s.step_losses[0], want[0]))
        assert abs(s.step_losses[0] - want[0]) < 1e-5

        s.test()
        s.color()
        assert s.test_matrix.sum() == len(s.test_index_loader.dataset) and len(s.label_maps) == 2
        trained = RefNet(ocfg)
        trained.load_state_dict({k: v.cpu() for k, v in s.cur_model.state_dict().items()})
        batch = xy[0, :64].numpy()
        logits, _ = EvalEngine(s.cur_model, s.scene, 64).predict(torch.from_numpy(batch).to(DEV))
        _, ref_logits = solver_ref.evaluate(trained, MS, PAN, batch, lab[0, :64].numpy(), cfg['Categories_Number'], P, 1)
        err = (logits.cpu() - ref_logits).abs().max().item()
        print('evaluation batch: logits max |diff| %.2e' % err)
        assert err < 1e-5

        z = np.load(cfg['RESULT_output'] + '0_band_reduce.npz')
        assert z['eigenvalues'].shape == (K,) and np.all(np.diff(z['eigenvalues']) < 0) and z['basis'].shape == (pca.SOLVER_BANDS, K)
        assert str(z['route']) == 'device' and np.all(z['explained'] > 0) and z['explained'].sum() < 1
        for name in ('0_weights.pth', '0_matrix.npy', '0_pic_1.png', '0_pic_2.png'):
            assert os.path.exists(cfg['RESULT_output'] + name), name
    finally:
        shutil.rmtree(tmp)


def test_solver_with_the_key_trains_in_half_precision(golden_dir):
    from solver.mainsolver import Solver
    tmp = tempfile.mkdtemp(prefix='dmf_pca_')
    try:
        cfg = _cfg(golden_dir, tmp)
        cfg['gmf'] = dict(cfg['gmf'], half=1)
        torch.manual_seed(3407)
        s = Solver(cfg)
        assert s.scene.A.dtype == torch.float16 and s.scene.A.shape[2] == pca.SOLVER_K
        s.dataloader()
        s.train()
        assert len(s.step_losses) == 2 * s._steps_per_epoch() and np.isfinite(s.step_losses).all()
    finally:
        shutil.rmtree(tmp)


def test_a_component_count_without_a_kernel_row_names_the_shapes_line(golden_dir):
    from dmf import lib
    from solver.mainsolver import Solver
    tmp = tempfile.mkdtemp(prefix='dmf_pca_')
    try:
        cfg = _cfg(golden_dir, tmp, band_reduce_bands=16)
        with pytest.raises(lib.DmfError) as e:
            Solver(cfg)
        text = str(e.value)
        assert 'no compiled kernel instance for C=16' in text and '--shapes FILE' in text      # what an unknown shape says today
        assert 'band_reduce_bands: 16 needs the line "16 1 5 1 40 2"' in text
        assert not os.path.exists(cfg['RESULT_output'] + '0_band_reduce.npz')                   # refused before any work
    finally:
        shutil.rmtree(tmp)


# ---------------------------------------------------------------------------------------------- 5. the 32-band row
@pytest.mark.parametrize('half', [False, True])
@pytest.mark.parametrize('B', pca.ROW_BATCHES)
def test_the_32_band_row_against_the_oracle(B, half):
    """Forward and train step of (32, 1, 11, 1, 40, 2, 64), gather and materialised, at the tolerances of
    tests/test_gpu_batch_walk.py: logits 1e-5, per-patch loss 2.2e-5, gradients 1e-5 + 1e-4 |ref|; half against the oracle with the
    same roundings.  The case meets the guards of tests/parity_cases.py, the open-or-shut guard of the ReLU gates included."""
    pc = pca.register_row()
    from dmf import lib
    from test_gpu_batch_walk import check_grads, check_pred, close, forward_runs, gpu_case, kind, make_input, tag
    c = gpu_case(pca.ROW, B, half)
    assert c['gate'] > pc.GATE_MARGIN and c['hip'].arch['G'] == 2
    hip, K = c['hip'], c['K']
    if half:
        lib.require_half(hip.shape)
    for mode in ('gather', 'patches'):
        what = tag(c, mode)
        r = forward_runs(c, mode)
        p = 'forward %s %s' % (kind(c), mode)
        close(p + ': logits', r['logits'], c['logits'], 1e-5, 0, 'forward logits ' + what)
        close(p + ': logits', r['logits_ce'], c['logits'], 1e-5, 0, 'forward_ce logits ' + what)
        close(p + ': loss', r['loss'], c['loss'], 2.2e-5, 0, 'forward_ce per-patch loss ' + what)
        check_pred(c, r['pred'], r['logits'], 'forward ' + what)
        inp = make_input(c, mode)
        logits = torch.full((B, K), float('nan'), device=DEV); loss = torch.full((B,), float('nan'), device=DEV)
        ws = torch.zeros(lib.workspace_bytes(hip.shape, B) // 4, device=DEV)
        lib.train_fwd_bwd(hip.shape, inp, c['theta'], hip.pool_w, c['labels_d'], 1.0 / B, logits, loss, ws)
        grad = torch.empty_like(c['theta'])
        lib.grad_reduce(hip.shape, B, ws, grad)
        torch.cuda.synchronize()
        p = 'train %s %s' % (kind(c), mode)
        close(p + ': logits', logits, c['logits'], 1e-5, 0, 'train logits ' + what)
        close(p + ': loss', loss, c['loss'], 2.2e-5, 0, 'train per-patch loss ' + what)
        check_grads(p + ': grads', c, grad, c['grads'], what)
