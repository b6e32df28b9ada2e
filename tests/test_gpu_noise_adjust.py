"""GPU: `band_reduce_noise` — dmf_band_noise_moments against float64 numpy on the same fp32 pixels, the device
route against utils.spectral.reduce_host(noise='both'), and the solver with the key against the oracle on the reduce_host scene.

Bounds (tests/noise_cases.py states and derives them next to the references; they come from the number formats and R, never from
the kernel's output):
  noise moments  |ncov_ij - ncov64_ij| <= (R + 4) 2^-24 A_ij,  A_ij = sum_p |e_pi| |e_pj| / (2 M), e the exact differences
  end to end     Davis-Kahan on the noise-whitened matrix, plus the first-order change of a column's length, times |F|_2 and the
                 largest centred row norm, plus the roundings of the bases and the projection bound
Every comparison prints its worst share of the bound."""
import copy
import ctypes
import shutil
import tempfile

import numpy as np
import pytest
import torch

import noise_cases as nc

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
CODE = {'horizontal': 0, 'vertical': 1}


def _R():
    from dmf import lib
    return lib.PCA_RUN


def _run(xd, H, W, direction):
    from dmf import lib
    C = xd.shape[-1]
    ncov = torch.full((C, C), float('nan'), dtype=torch.float64, device=DEV)
    lib.band_noise_moments(xd, H, W, ncov, direction)
    torch.cuda.synchronize()
    return ncov.cpu().numpy()


def _check(x, xd, direction, what):
    """x [H, W, C] float32 on the host, xd the same pixels on the device in whatever layout."""
    H, W, C = x.shape
    ncov = _run(xd, H, W, direction)
    ncov64, tol = nc.noise_ref(x, direction, _R())
    assert np.isfinite(ncov).all(), 'not finite ' + what
    share = (np.abs(ncov - ncov64)[tol > 0] / tol[tol > 0]).max() if (tol > 0).any() else 0.0
    print('noise moments %s %s: at %.3f of the bound' % (what, direction, share))
    assert (np.abs(ncov - ncov64) <= tol).all()
    assert np.array_equal(ncov, ncov.T), 'ncov[i][j] and ncov[j][i] differ ' + what
    assert (np.diagonal(ncov) >= 0).all()
    assert ncov.tobytes() == _run(xd, H, W, direction).tobytes(), 'two runs differ ' + what
    return ncov


def _refused(xd, H, W, C, direction):
    """The return code of a call that must not launch, with ncov checked to be as it was."""
    from dmf import lib
    ncov = torch.full((C, C), 7.0, dtype=torch.float64, device=DEV)
    ws = torch.zeros(max(lib._lib.dmf_band_noise_workspace_bytes(H, W, C), 8) // 8, dtype=torch.float64, device=DEV)
    rc = lib._lib.dmf_band_noise_moments(ctypes.c_void_p(xd.data_ptr()), H, W, C, C, CODE[direction], ctypes.c_void_p(ncov.data_ptr()),
                                         ctypes.c_void_p(ws.data_ptr()), None)
    torch.cuda.synchronize()
    assert (ncov == 7.0).all()
    return rc


# ---------------------------------------------------------------------------------------------- 1. against float64
@pytest.mark.parametrize('direction', nc.DIRECTIONS)
@pytest.mark.parametrize('H,W', nc.KERNEL_SCENES)
@pytest.mark.parametrize('C', nc.KERNEL_BANDS)
def test_noise_moments_against_float64(C, H, W, direction):
    assert _R() == 256
    x = nc.pixels(C, H, W)
    xd = torch.from_numpy(x.copy()).to(DEV)
    if nc.valid(direction, H, W):
        _check(x, xd, direction, '[%d x %d x %d]' % (H, W, C))
    else:                                                 # M < 1: code 2, nothing launched
        assert _refused(xd, H, W, C, direction) == 2


@pytest.mark.parametrize('direction', nc.DIRECTIONS)
def test_noise_moments_at_the_widest_scene(direction):
    x = nc.pixels(512, 3, 70)                             # 8 x 8 macro tiles, 36 pairs; a row end inside the second chunk
    _check(x, torch.from_numpy(x.copy()).to(DEV), direction, '[3 x 70 x 512]')


@pytest.mark.parametrize('direction', nc.DIRECTIONS)
def test_noise_moments_where_a_slice_owns_two_runs(direction):
    """As tests/test_gpu_band_reduce.py picks its N: 10 macro-tile pairs at 203 bands leave 76 slices, 103 x 257 pixels are 104
    runs of 256, so a slice owns two runs — read off the workspace, which is one 64 x 64 double tile per pair and slice."""
    from dmf import lib
    H, W, C = 103, 257, 203
    runs = -(-H * W // _R())
    slices = lib.band_noise_workspace_bytes(H, W, C) // (10 * 64 * 64 * 8)
    assert runs == 104 and slices == 52 and slices * 2 == runs
    x = nc.pixels(C, H, W)
    _check(x, torch.from_numpy(x.copy()).to(DEV), direction, '[%d x %d x %d]' % (H, W, C))


def _in_a_nan_surround(x, extra, lead):
    """x [H, W, C] on the device as pixels `C + extra` floats apart inside a NaN-filled tensor: NaN in the gaps, in `lead`
    pixels before the scene and in `lead` pixels behind it."""
    H, W, C = x.shape
    buf = torch.full((lead + H * W + lead, C + extra), float('nan'), device=DEV)
    buf[lead:lead + H * W, :C] = torch.from_numpy(x.reshape(H * W, C).copy()).to(DEV)
    return buf[lead:lead + H * W, :C]


@pytest.mark.parametrize('direction', nc.DIRECTIONS)
def test_noise_moments_with_a_row_pitch(direction):
    H, W, C = 4, 65, 203
    x = nc.pixels(C, H, W)
    buf = torch.full((H, W, C + 5), float('nan'), device=DEV)
    buf[:, :, :C] = torch.from_numpy(x.copy()).to(DEV)
    xd = buf[:, :, :C]                                    # [H, W, C], pixels C + 5 floats apart
    assert xd.stride() == (W * (C + 5), C + 5, 1) and not xd.is_contiguous()
    got = _check(x, xd, direction, '[4 x 65 x 203, pitch = C + 5]')
    assert got.tobytes() == _run(torch.from_numpy(x.copy()).to(DEV), H, W, direction).tobytes()       # the pitch changes no bit


@pytest.mark.parametrize('H,W,C', [(3, 5, 3), (4, 65, 24), (70, 9, 203)])
@pytest.mark.parametrize('direction', nc.DIRECTIONS)
def test_noise_moments_inside_a_nan_surround(direction, H, W, C):
    """Whatever lies behind the last pixel, before the first or between two pixels is never used: the pixels without the
    neighbour contribute a selected zero, not a product with zero."""
    x = nc.pixels(C, H, W)
    xd = _in_a_nan_surround(x, 5, W + 3)
    got = _check(x, xd, direction, '[%d x %d x %d in NaN]' % (H, W, C))
    assert got.tobytes() == _run(torch.from_numpy(x.copy()).to(DEV), H, W, direction).tobytes()


def test_noise_moments_refusals_leave_ncov_as_it_was():
    from dmf import lib
    H, W, C = 6, 50, 24
    x = torch.from_numpy(nc.pixels(C, H, W).copy()).to(DEV)
    ncov = torch.full((C, C), 7.0, dtype=torch.float64, device=DEV)
    ws = torch.zeros(lib.band_noise_workspace_bytes(H, W, C) // 8, dtype=torch.float64, device=DEV)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    f = lib._lib.dmf_band_noise_moments
    codes = [f(None, H, W, C, C, 0, p(ncov), p(ws), None), f(p(x), H, W, C, C, 0, None, p(ws), None),
             f(p(x), H, W, C, C, 0, p(ncov), None, None),
             f(p(x), H, W, 0, C, 0, p(ncov), p(ws), None), f(p(x), H, W, 513, 513, 0, p(ncov), p(ws), None),
             f(p(x), H, W, C, C - 1, 1, p(ncov), p(ws), None),
             f(p(x, 2), H, W, C, C, 0, p(ncov), p(ws), None), f(p(x), H, W, C, C, 1, p(ncov, 4), p(ws), None),
             f(p(x), H, W, C, C, 0, p(ncov), p(ws, 4), None),
             f(p(x), H, W, C, C, 2, p(ncov), p(ws), None), f(p(x), H, W, C, C, -1, p(ncov), p(ws), None),
             f(p(x), H, 1, C, C, 0, p(ncov), p(ws), None), f(p(x), 1, W, C, C, 1, p(ncov), p(ws), None),
             f(p(x), 0, W, C, C, 0, p(ncov), p(ws), None), f(p(x), H, 0, C, C, 1, p(ncov), p(ws), None),
             f(p(x), 2 ** 31 - 1, 2 ** 31 - 1, C, 2 ** 20, 0, p(ncov), p(ws), None)]
    torch.cuda.synchronize()
    assert codes == [1, 1, 1, 3, 3, 5, 6, 6, 6, 7, 7, 2, 2, 2, 2, 8]
    assert (ncov == 7.0).all()
    g = lib._lib.dmf_band_noise_workspace_bytes
    assert [g(0, 5, 24), g(5, 0, 24), g(1, 1, 24), g(5, 5, 0), g(5, 5, 513)] == [-1] * 5 and g(1, 2, 1) == 64 * 64 * 8
    with pytest.raises(lib.DmfError, match='no pixel has the neighbour'):
        lib.band_noise_moments(x[:, :1].contiguous(), H, 1, ncov, 'horizontal')
    with pytest.raises(lib.DmfError, match='direction'):
        lib.band_noise_moments(x, H, W, ncov, 2)
    with pytest.raises(lib.DmfError, match='workspace'):
        lib.band_noise_moments(x, H, W, ncov, 0, ws[:8])
    with pytest.raises(lib.DmfError, match='pixels'):
        lib.band_noise_moments(x.view(H * W, C), H, W + 1, ncov, 0)
    assert (ncov == 7.0).all()


# ---------------------------------------------------------------------------------------------- 2. end to end on the device
def test_device_route_against_reduce_host():
    from dmf.engine import band_reduce
    from utils import spectral
    K, C = nc.SOLVER_K, nc.SOLVER_BANDS
    raw = np.round(nc.noisy_scene(C) * 4000.0).astype(np.uint16)             # a scene as the readers deliver it
    x = spectral.normalise(raw)
    ratios, cond = nc.guards(x, 'both', K)                                   # the fixture's guards, on the float64 fit alone
    assert ratios.min() >= nc.MIN_RATIO and cond <= nc.MAX_COND
    want, fit_h = spectral.reduce_host(raw, K, noise='both')
    got, fit_d = band_reduce(raw, K, False, DEV, noise='both')
    assert got.dtype == np.float32 and got.shape == want.shape and fit_d['route'] == 'device' and fit_d['noise'] == 'both'
    assert sorted(fit_d) == sorted(fit_h)
    tol, parts = nc.route_tolerance(x, 'both', K, fit_h['basis'], _R())
    err = np.abs(got.astype(np.float64) - want.astype(np.float64)).max()
    print('device route vs reduce_host(noise=both): max |diff| %.2e, tolerance %.2e: at %.2e of the bound (sin theta <= %.2e, '
          'length %.2e, gap %.2f, cond %.2f), score range %.2f'
          % (err, tol, err / tol, parts['sin_theta'], parts['length'], parts['gap'], parts['cond'], float(want.max() - want.min())))
    assert tol < 0.1 * (want.max() - want.min())                             # a tolerance that still tells two score maps apart
    assert err <= tol
    # Weyl: an eigenvalue moves by no more than the norm of the perturbation (tests/noise_cases.py, 4: dM and |E_N|_F)
    assert np.abs(fit_d['eigenvalues'] - fit_h['eigenvalues']).max() <= parts['dM']
    assert np.abs(fit_d['noise_eigenvalues'] - fit_h['noise_eigenvalues']).max() <= parts['E_N']
    assert np.abs(fit_d['mean'] - fit_h['mean']).max() <= 2.0 ** -50 * x.shape[0] * x.shape[1]
    # one direction each, against the same reference at the same kind of tolerance
    for noise in nc.DIRECTIONS:
        w1, f1 = spectral.reduce_host(raw, K, noise=noise)
        g1, _ = band_reduce(raw, K, False, DEV, noise=noise)
        t1, _ = nc.route_tolerance(x, noise, K, f1['basis'], _R())
        e1 = np.abs(g1.astype(np.float64) - w1.astype(np.float64)).max()
        print('%s: max |diff| %.2e at %.2e of the bound' % (noise, e1, e1 / t1))
        assert e1 <= t1
    # whitened: unit total variance of every component
    white, _ = band_reduce(raw, K, True, DEV, noise='both')
    assert np.allclose(white.reshape(-1, K).astype(np.float64).var(axis=0, ddof=1), 1.0, atol=1e-4)
    # without the argument: the PCA route, bit for bit what the positional call gives
    a, fa = band_reduce(raw, K, False, DEV)
    b, fb = band_reduce(raw, K, False, DEV, noise=None)
    assert a.tobytes() == b.tobytes() and sorted(fa) == sorted(fb) == ['basis', 'eigenvalues', 'explained', 'mean', 'route']
    with pytest.raises(ValueError, match='band_reduce_noise'):
        band_reduce(raw[:, :1], 1, False, DEV, noise='horizontal')


# ---------------------------------------------------------------------------------------------- 3. the solver
def _cfg(golden_dir, tmp, **over):
    from test_gpu_trajectory import _setup
    _, cfg = _setup(golden_dir, tmp, **dict(dict(epoch=2, scale=1, train_rate=0.3, verify_rate=0.1, steps_per_graph=-1, seed=123,
                                                 band_reduce='pca', band_reduce_bands=nc.SOLVER_K, band_reduce_noise='both'), **over))
    primary, aux, label = nc.solver_scene(cfg['Categories_Number'])
    d = cfg['data_address']
    np.save(d + 'ms4.tif.npy', primary); np.save(d + 'pan.tif.npy', aux); np.save(d + 'label.npy', label)
    cfg['DATA_DICT'][cfg['data_city']]['size'] = [40, 40, nc.SOLVER_BANDS]
    cfg['test']['full'] = 1
    cfg['color']['index'] = 1
    return cfg


EXTENDED = ['basis', 'eigenvalues', 'explained', 'mean', 'noise', 'noise_eigenvalues', 'route', 'snr']


def test_solver_with_the_key_against_the_oracle_on_the_reduce_host_scene(golden_dir):
    """Patch 5, 8 noise-adjusted components of a 24-band scene: the existing row 8/1/5/1/40/2.  The first step's loss and the
    logits of one evaluation batch agree with the oracle on the reduce_host(noise='both') scene at the tolerances
    tests/test_gpu_band_reduce.py holds that row to (loss 1e-5, logits 1e-5); the .npz holds the extra arrays."""
    from dmf.engine import EvalEngine
    from function.function import data_padding, data_padding_aux
    from model.gmfnet import Net as HipNet
    from oracle import solver_ref
    from oracle.gmfnet_ref import Net as RefNet
    from solver.mainsolver import Solver
    from utils import spectral
    tmp = tempfile.mkdtemp(prefix='dmf_noise_')
    try:
        cfg = _cfg(golden_dir, tmp)
        K, P, B = nc.SOLVER_K, cfg['patch_size'], cfg['batchsize']
        torch.manual_seed(3407)
        s = Solver(cfg)
        assert s.ms.shape == (40, 40, K) and s.ms.dtype == np.float32
        assert s.band_fit['route'] == 'device' and s.band_fit['noise'] == 'both'
        s.dataloader()
        rng = torch.get_rng_state()
        s.train()
        assert len(s.step_losses) == 2 * s._steps_per_epoch() and np.isfinite(s.step_losses).all()
        assert s.cur_model.arch['C'] == K and s.cur_model.arch['G'] == 2

        primary, aux, _ = nc.solver_scene(cfg['Categories_Number'])
        reduced, _ = spectral.reduce_host(primary, K, noise='both')
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

        trained = RefNet(ocfg)
        trained.load_state_dict({k: v.cpu() for k, v in s.cur_model.state_dict().items()})
        batch = xy[0, :64].numpy()
        logits, _ = EvalEngine(s.cur_model, s.scene, 64).predict(torch.from_numpy(batch).to(DEV))
        _, ref_logits = solver_ref.evaluate(trained, MS, PAN, batch, lab[0, :64].numpy(), cfg['Categories_Number'], P, 1)
        err = (logits.cpu() - ref_logits).abs().max().item()
        print('evaluation batch: logits max |diff| %.2e' % err)
        assert err < 1e-5

        z = np.load(cfg['RESULT_output'] + '0_band_reduce.npz')
        assert sorted(z.files) == EXTENDED and str(z['route']) == 'device' and str(z['noise']) == 'both'
        assert z['basis'].shape == (nc.SOLVER_BANDS, K) and z['eigenvalues'].shape == (K,) and np.all(np.diff(z['eigenvalues']) < 0)
        assert np.array_equal(z['snr'], z['eigenvalues'] - 1) and z['noise_eigenvalues'].shape == (nc.SOLVER_BANDS,)
    finally:
        shutil.rmtree(tmp)


def test_solver_on_the_drop_in_path_trains_on_the_components(golden_dir):
    """`fast_path: 0` with the key on: reduce_host(noise=...) gives the scene, the extended .npz names the host route, and the
    drop-in path trains a few steps on the components."""
    from solver.mainsolver import Solver
    from utils import spectral
    tmp = tempfile.mkdtemp(prefix='dmf_noise_')
    try:
        cfg = _cfg(golden_dir, tmp, fast_path=0, epoch=1, band_reduce_noise='vertical')
        torch.manual_seed(3407)
        s = Solver(cfg)
        want, _ = spectral.reduce_host(nc.solver_scene(cfg['Categories_Number'])[0], nc.SOLVER_K, noise='vertical')
        assert np.array_equal(s.ms, want) and s.band_fit['route'] == 'host' and s.scene is None
        s.dataloader()
        s.train()
        assert len(s.step_losses) >= 2 and np.isfinite(s.step_losses).all()
        z = np.load(cfg['RESULT_output'] + '0_band_reduce.npz')
        assert sorted(z.files) == EXTENDED and str(z['route']) == 'host' and str(z['noise']) == 'vertical'
    finally:
        shutil.rmtree(tmp)
