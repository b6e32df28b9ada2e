"""GPU: `band_profile: morph` — dmf_morph_markers, dmf_morph_reconstruct and dmf_morph_stack against the scipy
reference of tests/morph_ref.py, bit for bit (everything is min / max of float32 values: there is no tolerance to state), the
workspace discipline, dmf.engine.band_profile against utils.morphology.profile_host, and the solver with the key against the
oracle on the profile_host scene at the tolerance tests/test_gpu_band_reduce.py holds its solver case to (first loss 1e-5)."""
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

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def _bits_equal(t, want):
    return np.array_equal(mr.bits(t.cpu().numpy()), mr.bits(want))


# ---------------------------------------------------------------------------------------------- 1. markers
def _pitched(s, extra):
    """s [H, W, K] on the device with pixels K + extra floats apart; the gaps hold NaN."""
    H, W, K = s.shape
    buf = torch.full((H, W, K + extra), float('nan'), device=DEV)
    buf[:, :, :K] = torch.from_numpy(np.array(s)).to(DEV)
    return buf[:, :, :K]


@pytest.mark.parametrize('shape', [(33, 37), (67, 131), (5, 4), (1, 70)])
def test_markers_against_the_reference(shape):
    """Smaller than one tile, one row and column past a tile multiple (64 + 3, 2 x 64 + 3; a row segment is 256), windows wider
    than the image, the widest window, and a pixel pitch of K + 5 with NaN in the gaps."""
    from dmf import lib
    H, W = shape
    K, P, radii = 3, 2, (1, 6, 32)
    n = len(radii)
    s = mc.scores(H, W, K).copy()
    s[0, 0, 0], s[H - 1, W - 1, 1] = -0.0, 0.0
    sd = _pitched(s, 5)
    mask = torch.full((2 * P, H, W), float('nan'), device=DEV)
    markers, scratch = (torch.full((2 * n * P, H, W), float('nan'), device=DEV) for _ in range(2))
    lib.morph_markers(sd, P, radii, mask, markers, scratch)
    torch.cuda.synchronize()
    for p in range(P):
        f = mr.canon(s[:, :, p])
        g = mr.canon(-f)
        assert _bits_equal(mask[p], f) and _bits_equal(mask[P + p], g), p
        for i, r in enumerate(radii):
            assert _bits_equal(markers[p * n + i], mr.erode(f, r)), (p, r)
            assert _bits_equal(markers[(P + p) * n + i], mr.erode(g, r)), (p, r)
            assert _bits_equal(markers[(P + p) * n + i], mr.canon(-mr.dilate(f, r))), (p, r)     # the closing side IS the dilation
    assert not (mr.bits(mask.cpu().numpy()) == 0x80000000).any()


def test_markers_refusals_leave_the_outputs_as_they_were():
    from dmf import lib
    H, W, K, P = 9, 11, 3, 2
    sd = torch.from_numpy(np.array(mc.scores(H, W, K))).to(DEV)
    mask = torch.full((2 * P, H, W), 7.0, device=DEV)
    markers, scratch = (torch.full((4 * P, H, W), 7.0, device=DEV) for _ in range(2))
    for radii, text in (((2, 2), 'strictly increasing'), ((1, 33), 'strictly increasing'), ((0, 1), 'strictly increasing')):
        with pytest.raises(lib.DmfError, match=text):
            lib.morph_markers(sd, P, radii, mask, markers, scratch)
    with pytest.raises(lib.DmfError, match='same memory'):
        lib.morph_markers(sd, P, (1, 2), mask, markers, markers)
    with pytest.raises(lib.DmfError, match='1 <= P <= K'):
        lib.morph_markers(sd[:, :, :1], P, (1, 2), mask, markers, scratch)
    torch.cuda.synchronize()
    assert bool((mask == 7).all()) and bool((markers == 7).all()) and bool((scratch == 7).all())


# ---------------------------------------------------------------------------------------------- 2. reconstruction
def _reconstruct(masks, markers, per_mask):
    """-> (X, Y, rounds per batch) of one whole reconstruction of the numpy planes."""
    from dmf import lib
    mask = torch.from_numpy(np.ascontiguousarray(masks)).to(DEV)
    X = torch.from_numpy(np.ascontiguousarray(markers)).to(DEV)
    Y = torch.full_like(X, float('nan'))
    L, H, W = X.shape
    state = torch.full((lib.morph_state_bytes(H, W, L),), 0xAB, dtype=torch.uint8, device=DEV)
    rounds = lib.morph_reconstruct_run(mask, X, Y, per_mask, state)
    torch.cuda.synchronize()
    return X, Y, rounds


def _reconstruction_case(name, f, radii):
    f = mr.canon(f)
    markers = np.stack([mr.erode(f, r) for r in radii])
    want = [mr.rec_dilation(m, f) for m in markers]
    X, Y, rounds = _reconstruct(f[None], markers, len(radii))
    print('%s %d x %d, radii %s: %d device rounds in batches %s; the reference needs %s'
          % (name, f.shape[0], f.shape[1], list(radii), sum(rounds), rounds, [w[1] for w in want]))
    for i in range(len(radii)):
        assert _bits_equal(X[i], want[i][0]), (name, radii[i])
    assert torch.equal(X.view(torch.int32), Y.view(torch.int32)), 'the two buffers differ at the end'
    X2, Y2, rounds2 = _reconstruct(f[None], markers, len(radii))
    assert torch.equal(X.view(torch.int32), X2.view(torch.int32)) and rounds == rounds2, 'two runs differ'
    assert all(b == 8 for b in rounds[:-1]) and 1 <= rounds[-1] <= 8
    return rounds


@pytest.mark.parametrize('shape', [(67, 131), (130, 71)])
def test_reconstruction_carries_the_plateau_down_the_serpentine(shape):
    rounds = _reconstruction_case('serpentine', mc.serpentine(*shape), (2, 3))
    assert sum(rounds) > 2                                                   # more than one tile deep: the value crossed borders


def test_reconstruction_with_ties_and_signed_zeros():
    _reconstruction_case('ties', mc.ties(), (1, 3))
    _reconstruction_case('zeros', mc.zeros(), (1, 2))
    for name in ('constant', 'one_row', 'one_column', 'small'):
        f, radii = mc.planes()[name]
        _reconstruction_case(name, f, radii)


def test_a_converged_input_stops_after_the_first_batch():
    f = mr.canon(mc.serpentine(67, 131))
    fixed = mr.rec_dilation(mr.erode(f, 2), f)[0]
    X, Y, rounds = _reconstruct(f[None], fixed[None], 1)
    assert rounds == [1]
    assert _bits_equal(X[0], fixed) and _bits_equal(Y[0], fixed)


def test_reconstruct_refusals():
    from dmf import lib
    mask, X, Y = (torch.zeros(2, 9, 11, device=DEV) for _ in range(3))
    state = torch.zeros(lib.morph_state_bytes(9, 11, 2), dtype=torch.uint8, device=DEV)
    for first, rounds in ((4, 1), (0, 9), (0, 0), (-8, 1)):
        with pytest.raises(lib.DmfError, match='first_round or rounds out of range'):
            lib.morph_reconstruct(mask, X, Y, 1, first, rounds, state)
    with pytest.raises(lib.DmfError, match='same memory'):
        lib.morph_reconstruct(mask, X, X, 1, 0, 8, state)
    with pytest.raises(lib.DmfError, match='the state needs'):
        lib.morph_reconstruct(mask, X, Y, 1, 0, 8, state[:32])


# ---------------------------------------------------------------------------------------------- 3. the workspace
def test_nothing_outside_the_workspace_is_written_and_nothing_stale_is_read():
    from dmf import lib
    H, W, K, P, radii = 67, 131, 3, 2, (1, 3)
    n, guard = len(radii), 4096
    s = mc.scores(H, W, K)
    need = lib.morph_workspace_bytes(H, W, P, n)
    raw = torch.full((need + 2 * guard,), 0xFF, dtype=torch.uint8, device=DEV)          # 0xFFFFFFFF is a NaN
    ws = raw[guard:guard + need]
    mask, X, Y, state = lib.morph_carve(ws, H, W, P, n)
    assert mask.data_ptr() == ws.data_ptr() and state.data_ptr() + state.numel() == ws.data_ptr() + need
    sd = _pitched(s, 5)
    out = torch.full((H, W, K + 2 * n * P), float('nan'), device=DEV)
    lib.morph_markers(sd, P, radii, mask, X, Y)
    rounds = lib.morph_reconstruct_run(mask, X, Y, n, state)
    lib.morph_stack(sd, P, n, mask, Y, out)                                  # either buffer holds the result
    torch.cuda.synchronize()
    assert bool((raw[:guard] == 0xFF).all()) and bool((raw[guard + need:] == 0xFF).all()), 'a guard word was written'
    got = out.cpu().numpy()
    assert np.isfinite(got).all()
    assert np.array_equal(mr.bits(got), mr.bits(mr.profile(s, P, radii)))
    print('workspace %d bytes, rounds %s' % (need, rounds))


# ---------------------------------------------------------------------------------------------- 4. the engine
def test_engine_route_equals_profile_host():
    from dmf.engine import band_profile
    from utils import morphology
    s = mc.scores(67, 131, 3)
    want, winfo = morphology.profile_host(s, 2, (1, 3))
    got, info = band_profile(np.array(s), 2, [1, 3], DEV)
    assert got.dtype == np.float32 and np.array_equal(mr.bits(got), mr.bits(want))
    assert info['route'] == 'device' and info['order'] == winfo['order'] and info['bands'] == 11 and sum(info['rounds']) >= 1
    got2, info2 = band_profile(_pitched(s, 2), 2, (1, 3), DEV)                 # a tensor on the device, with a pitch
    assert np.array_equal(mr.bits(got2), mr.bits(want)) and info2['rounds'] == info['rounds']
    bad = np.array(s)
    bad[3, 4, 2] = np.nan
    with pytest.raises(ValueError, match='band_profile: the scores hold a value that is not finite'):
        band_profile(bad, 2, (1, 3), DEV)
    with pytest.raises(ValueError, match='band_profile_components: 4 exceeds the 3 components'):
        band_profile(np.array(s), 4, (1, 3), DEV)


def test_band_reduce_leaves_the_scores_on_the_device():
    import pca_cases as pca
    from dmf.engine import band_reduce
    raw = pca.solver_scene(5)[0].copy()
    host, fit = band_reduce(raw, 8, False, DEV)
    dev, fit_d = band_reduce(raw, 8, False, DEV, on_device=True)
    assert isinstance(host, np.ndarray) and torch.is_tensor(dev) and dev.is_cuda and tuple(dev.shape) == host.shape
    assert np.array_equal(mr.bits(dev.cpu().numpy()), mr.bits(host)) and fit['route'] == fit_d['route']


# ---------------------------------------------------------------------------------------------- 5. the solver
def _cfg(golden_dir, tmp, **over):
    import pca_cases as pca
    from test_gpu_trajectory import _setup
    _, cfg = _setup(golden_dir, tmp, **dict(dict(epoch=1, scale=1, train_rate=0.3, verify_rate=0.1, steps_per_graph=-1, seed=123), **over))
    primary, aux, label = pca.solver_scene(cfg['Categories_Number'])
    d = cfg['data_address']
    np.save(d + 'ms4.tif.npy', primary); np.save(d + 'pan.tif.npy', aux); np.save(d + 'label.npy', label)
    cfg['DATA_DICT'][cfg['data_city']]['size'] = [40, 40, pca.SOLVER_BANDS]
    return cfg


def test_solver_with_the_key_against_the_oracle_on_the_profile_host_scene(golden_dir):
    """8 components, 4 of them profiled at radii 2 / 4 / 6, patch 11: the row 32/1/11/1/40/2.  The first step's loss agrees with
    the oracle on the profile_host scene to the 1e-5 of the band_reduce solver case."""
    import pca_cases as pca
    from function.function import data_padding, data_padding_aux
    from model.gmfnet import Net as HipNet
    from oracle import solver_ref
    from oracle.gmfnet_ref import Net as RefNet
    from solver.mainsolver import Solver
    from utils import morphology, spectral
    tmp = tempfile.mkdtemp(prefix='dmf_morph_')
    try:
        cfg = _cfg(golden_dir, tmp, band_reduce='pca', band_reduce_bands=8, band_profile='morph', band_profile_components=4,
                   band_profile_radii=[2, 4, 6], patch_size=11)
        P, B = cfg['patch_size'], cfg['batchsize']
        torch.manual_seed(3407)
        s = Solver(cfg)
        assert s.ms.shape == (40, 40, 32) and s.ms.dtype == np.float32 and s.band_profile_info['route'] == 'device'
        assert s.scene.A.shape == (40 + P - 1, 40 + P - 1, 32)
        s.dataloader()
        rng = torch.get_rng_state()
        s.train()
        assert np.isfinite(s.step_losses).all() and s.cur_model.arch['C'] == 32 and s.cur_model.arch['G'] == 2

        primary, aux, _ = pca.solver_scene(cfg['Categories_Number'])
        reduced, _ = spectral.reduce_host(primary, 8)
        scene, _ = morphology.profile_host(reduced, 4, (2, 4, 6))
        print('profile: device vs profile_host on the reduce_host scores, max |diff| %.2e' % np.abs(s.ms - scene).max())
        MS = data_padding(scene, cfg, 'ms').astype(np.float32)
        PAN = data_padding_aux(aux, cfg).astype(np.float32)
        ocfg = copy.deepcopy(cfg)
        ocfg['DATA_DICT'][cfg['data_city']]['size'] = [40, 40, 32]           # the oracle is called with C = 32
        torch.set_rng_state(rng)
        init = HipNet(cfg).state_dict()
        xy, lab = s._epoch_streams(1)
        ref = RefNet(ocfg)
        ref.load_state_dict(init)
        want, _ = solver_ref.train_steps(ref, MS, PAN, xy[0, :B].numpy(), lab[0, :B].numpy(), B, P, 1, lr=cfg['schedule']['lr'])
        print('first step: loss %.7f, oracle %.7f' % (s.step_losses[0], want[0]))
        assert abs(s.step_losses[0] - want[0]) < 1e-5

        info = json.load(open(cfg['RESULT_output'] + '0_band_profile.json'))
        assert info['order'] == morphology.band_names(8, 4, (2, 4, 6)) and len(info['order']) == info['bands'] == 32
        assert info['components'] == 4 and info['radii'] == [2, 4, 6] and info['route'] == 'device' and sum(info['rounds']) >= 1
        assert os.path.exists(cfg['RESULT_output'] + '0_band_reduce.npz')
    finally:
        shutil.rmtree(tmp)


def test_a_band_count_without_a_kernel_row_is_refused_before_any_work(golden_dir):
    from dmf import lib
    from solver.mainsolver import Solver
    tmp = tempfile.mkdtemp(prefix='dmf_morph_')
    try:
        cfg = _cfg(golden_dir, tmp, band_reduce='pca', band_reduce_bands=8, band_profile='morph', band_profile_components=2,
                   band_profile_radii=[1, 2])
        with pytest.raises(lib.DmfError) as e:
            Solver(cfg)
        text = str(e.value)
        assert 'no compiled kernel instance for C=16' in text and '--shapes FILE' in text
        assert 'band_reduce_bands: 8 with band_profile: morph needs the line "16 1 5 1 40 2"' in text
        assert not os.path.exists(cfg['RESULT_output'] + '0_band_reduce.npz')
        assert not os.path.exists(cfg['RESULT_output'] + '0_band_profile.json')
    finally:
        shutil.rmtree(tmp)


def test_the_key_at_none_changes_no_byte_of_a_solver_run(golden_dir):
    from solver.mainsolver import Solver
    tmp = tempfile.mkdtemp(prefix='dmf_morph_')
    try:
        runs = []
        for sub, over in (('a', {}), ('b', {'band_profile': 'none', 'band_profile_components': 3, 'band_profile_radii': [1, 2]})):
            cfg = _cfg(golden_dir, os.path.join(tmp, sub), band_reduce='pca', band_reduce_bands=8, **over)
            torch.manual_seed(3407)
            s = Solver(cfg)
            s.dataloader()
            s.train()
            weights = torch.load(cfg['RESULT_output'] + '0_weights.pth', map_location='cpu', weights_only=True)
            runs.append((s.ms.tobytes(), np.asarray(s.step_losses).tobytes(), {k: v.numpy().tobytes() for k, v in weights.items()}))
            assert not os.path.exists(cfg['RESULT_output'] + '0_band_profile.json')
        assert runs[0] == runs[1]
    finally:
        shutil.rmtree(tmp)
