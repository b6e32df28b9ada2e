"""GPU: calibrated confidence — dmf_softmax_stats against float64, dmf_calib_accum against numpy exactly,
dmf_temperature_step's fit against the same rule in float64 (tests/calib_ref.py; the guards of the cases are CPU tests in
tests/test_calibration_host.py), and the solver keys on the 40 x 40 x 8, 4-class scene of tests/test_gpu_epoch_block.py.

Observed on an MI355X (printed by the tests): statistics at most 5.0e-7 from float64 (K = 17, tol 1.5e-5; K = 64:
4.2e-7, tol 4.9e-5); the fitted beta within 2e-16 of the reference in 23 of 24 cases and 9.8e-11 in one (over, N = 255, K = 17),
where the device takes the rule's fall-back to sqrt(lo hi) at another step than numpy (asked: 1e-9); 50 sampled pixels of the
solver's maps within 2.1e-7 (tol 6.5e-6); drop-in path: the same counts in every bin, ECE within 1.4e-9."""
import functools
import json
import os
import shutil
import tempfile

import numpy as np
import pytest
import torch
from PIL import Image

import calib_ref as R

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _stats_gpu(logits, beta=None, **kw):
    """(pred, conf, margin, entropy) as numpy from one dmf_softmax_stats launch."""
    from dmf import lib
    B = logits.shape[0]
    pred = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    out = [torch.full((B,), -1.0, device=DEV) for _ in range(3)]
    inv = None if beta is None else torch.tensor([beta], dtype=torch.float32, device=DEV)
    lib.softmax_stats(_dev(logits), pred=pred, conf=out[0], margin=out[1], entropy=out[2], inv_temp=inv, **kw)
    return (pred.cpu().numpy(),) + tuple(o.cpu().numpy() for o in out)


# ------------------------------------------------------------------------------------------------ dmf_softmax_stats
@pytest.mark.parametrize('scale', R.STATS_SCALE, ids=lambda s: 'x%d' % s)
@pytest.mark.parametrize('K', R.STATS_K)
def test_softmax_stats_against_float64(K, scale):
    """Every B and beta of the case table: pred equal, conf / margin / entropy within tol(K) absolute (all three lie in
    [0, ln K] and are O(1)); the wide rows (x40) underflow e_c and still give finite values with entropy >= 0; a second run
    gives the same bits."""
    worst = 0.0
    for B in R.STATS_B:
        logits = R.stats_logits(K, B, scale)
        for beta in R.STATS_BETA:
            got = _stats_gpu(logits, None if beta == 1.0 else beta)
            want = R.stats(logits, beta)
            assert np.array_equal(got[0], want[0]), (B, beta)
            for g, w, name in zip(got[1:], want[1:], ('conf', 'margin', 'entropy')):
                assert np.isfinite(g).all() and (g >= 0).all(), (name, B, beta)
                worst = max(worst, float(np.abs(g.astype(np.float64) - w).max()))
            again = _stats_gpu(logits, None if beta == 1.0 else beta)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
    print('K = %d, logits x %d: largest absolute error %.3e, tol(K) %.3e' % (K, scale, worst, R.tol(K)))
    assert worst <= R.tol(K)


@pytest.mark.parametrize('K', R.TIE_K)
def test_ties_go_to_the_first_index_with_margin_zero(K):
    rows, first, tied = R.tie_logits(K)
    for beta in R.STATS_BETA:
        pred, conf, margin, entropy = _stats_gpu(rows, beta)
        assert np.array_equal(pred, first)
        assert np.array_equal(margin == 0.0, tied)
        want = R.stats(rows, beta)
        for g, w in zip((conf, margin, entropy), want[1:]):
            assert np.abs(g - w).max() <= R.tol(K)
    assert np.isclose(_stats_gpu(rows)[3][2], np.log(K), atol=R.tol(K))            # all equal: the entropy of the uniform law


def test_the_scatter_form_and_null_outputs():
    """23 x 37 maps, 300 distinct pixels in random order, W = 37: every cell that no row names keeps its sentinel, an output
    that is not asked for is not written, and the values are those of the row form."""
    from dmf import lib
    H, W, B, K = 23, 37, 300, 17
    rng = np.random.default_rng(5)
    cells = rng.permutation(H * W)[:B]
    xy = np.stack([cells // W, cells % W], 1).astype(np.int32)
    logits = R.stats_logits(K, 1025, 1.0)[:B]
    rows = _stats_gpu(logits, 0.5)
    label = torch.full((H, W), -7, dtype=torch.int32, device=DEV)
    planes = torch.full((3, H, W), -7.0, device=DEV)
    inv = torch.tensor([0.5], dtype=torch.float32, device=DEV)
    lib.softmax_stats(_dev(logits), pred=label, conf=planes[0], entropy=planes[2], inv_temp=inv, xy=_dev(xy), W=W)   # no margin
    label, planes = label.cpu().numpy(), planes.cpu().numpy()
    assert (planes[1] == -7.0).all()
    touched = np.zeros((H, W), dtype=bool)
    touched[xy[:, 0], xy[:, 1]] = True
    assert (label[~touched] == -7).all() and (planes[0][~touched] == -7.0).all() and (planes[2][~touched] == -7.0).all()
    assert np.array_equal(label[xy[:, 0], xy[:, 1]], rows[0])
    assert planes[0][xy[:, 0], xy[:, 1]].tobytes() == rows[1].tobytes()
    assert planes[2][xy[:, 0], xy[:, 1]].tobytes() == rows[3].tobytes()


# ------------------------------------------------------------------------------------------------ dmf_calib_accum
@pytest.mark.parametrize('nbins', [1, 10, 15])
def test_histogram_of_the_kernels_own_confidences_is_numpys(nbins):
    from dmf import lib
    K, B = 17, 1025
    logits = R.stats_logits(K, B, 1.0)
    pred, conf, _, _ = _stats_gpu(logits, 0.5)
    rng = np.random.default_rng(nbins)
    target = np.where(rng.random(B) < 0.6, pred, rng.integers(0, K, B)).astype(np.int32)
    target[::50] = -1
    target[7::50] = K                                                               # out of range on both sides: skipped
    hist = torch.zeros(nbins, 3, dtype=torch.int64, device=DEV)
    for lo, hi in ((0, 300), (300, B)):                                             # two calls add into one histogram
        lib.calib_accum(_dev(conf[lo:hi]), _dev(pred[lo:hi]), _dev(target[lo:hi]), K, hist)
    want = R.histogram(conf, pred, target, K, nbins)
    assert want[:, 0].sum() == B - 21 - 21 and np.array_equal(hist.cpu().numpy(), want)


def test_histogram_edge_rows():
    """conf == 1.0 lands in the last bin, conf == k / nbins (nbins = 8: exact) in bin k, rows with a target outside [0, K) are
    skipped; the confidence sum is exact."""
    from dmf import lib
    nbins, K = 8, 4
    conf = np.array([1.0] + [k / 8 for k in range(8)] + [0.5, 0.999], dtype=np.float32)
    pred = np.array([0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 2], dtype=np.int32)
    target = np.array([0, 1, 0, 3, 0, 0, 2, 3, 1, -1, 4], dtype=np.int32)
    hist = torch.zeros(nbins, 3, dtype=torch.int64, device=DEV)
    lib.calib_accum(_dev(conf), _dev(pred), _dev(target), K, hist)
    got = hist.cpu().numpy()
    want = np.zeros((8, 3), dtype=np.int64)
    for c, p, t in list(zip(conf, pred, target))[:9]:
        b = min(7, int(c * 8))
        want[b] += (1, int(p == t), int(c * 2 ** 32))
    assert np.array_equal(got, want) and np.array_equal(got, R.histogram(conf, pred, target, K, nbins))
    assert got[7, 0] == 2 and got[:, 0].sum() == 9


# ------------------------------------------------------------------------------------------------ the temperature fit
def _fit_gpu(logits, labels, steps=40):
    from dmf import lib
    lg, y = _dev(logits), _dev(labels)
    state = torch.empty(lib.TEMP_DOUBLES, dtype=torch.float64, device=DEV)
    ws = torch.empty(max(lib.temperature_workspace_bytes(len(labels)), 8), dtype=torch.uint8, device=DEV)
    lib.temperature_init(state)
    for _ in range(steps):
        lib.temperature_step(lg, y, state, ws, update=True)
    after = state.cpu().numpy().copy()
    lib.temperature_step(lg, y, state, ws, update=False)
    return after, state.cpu().numpy()


@pytest.mark.parametrize('K', R.FIT_K)
@pytest.mark.parametrize('N', R.FIT_N)
@pytest.mark.parametrize('kind', R.FIT_KINDS)
def test_fit_is_the_float64_rule(kind, N, K):
    logits, labels = R.fit_case(kind, N, K)
    ref = R.fit(logits, labels)
    after, evaluated = _fit_gpu(logits, labels)
    err = abs(after[0] - ref['beta']) / ref['beta']
    print('%s N=%d K=%d: beta %.15g (reference %.15g, relative difference %.2e), bracket [%.15g, %.15g], steps %d'
          % (kind, N, K, after[0], ref['beta'], err, after[4], after[5], after[6]))
    assert err <= 1e-9
    assert after[6] == 40 and after[4] <= after[0] <= after[5]
    # update = 0 only evaluates: beta, lo, hi and steps stay, nll / g / h are those at beta
    assert evaluated[[0, 4, 5, 6]].tobytes() == after[[0, 4, 5, 6]].tobytes()
    nll, g, h = R.nll_terms(logits, labels, after[0])
    # (double sums of N terms of size <= span, span^2 in two orders, exp and log within an ulp or two: 1e-10 is generous)
    span = float(logits.max() - logits.min()) + 1.0
    assert abs(evaluated[1] - nll) <= 1e-10 * N * span * max(after[0], 1.0)
    assert abs(evaluated[2] - g) <= 1e-10 * N * span and abs(evaluated[3] - h) <= 1e-10 * N * span * span


def test_fit_skips_labels_outside_the_classes_and_repeats_bit_for_bit():
    logits, labels = R.fit_case('over', 257, 17)
    more = np.concatenate([logits, logits[:40] * 3.0])
    more_labels = np.concatenate([labels, np.where(np.arange(40) % 2 == 0, -1, 17)]).astype(np.int32)
    a, b, c = _fit_gpu(logits, labels)[0], _fit_gpu(more, more_labels)[0], _fit_gpu(more, more_labels)[0]
    assert abs(a[0] - b[0]) <= 1e-9 * a[0]
    assert b.tobytes() == c.tobytes()


# ------------------------------------------------------------------------------------------------ the solver
SEED = 3407
KEYS_ON = {'test': dict(calibration=1, calibration_bins=15, temperature='fit'), 'color': dict(confidence=1)}
NETS = {'late_fusion': 'plain_native_loop', 'attention': 'attention'}


def _read(path):
    with open(path, 'rb') as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def _run(net, keys, golden_dir):
    """Two epochs of Solver.train() on the epoch-block scene, then test() and color(); with `keys` also what the calibration
    keys leave, the float64 statistics of 50 sampled pixels from `eval_engine.predict`'s logits, and the same test() / color()
    by a drop-in solver (fast_path: 0) on the weights this run saved."""
    from solver.mainsolver import Solver
    from test_gpu_epoch_block import _cfg
    tmp = tempfile.mkdtemp(prefix='dmf_calib_')
    try:
        cfg = _cfg(golden_dir, tmp, NETS[net], 1)
        cfg['epoch'] = 2
        if keys:
            for sec, val in KEYS_ON.items():
                cfg[sec] = dict(cfg[sec], **val)
        torch.manual_seed(SEED)
        s = Solver(cfg)
        s.dataloader()
        s.train()
        s.test()
        s.color()
        out = cfg['RESULT_output']
        r = dict(matrix=s.test_matrix.copy(), maps=s.label_maps, png=[_read(out + '0_pic_%d.png' % k) for k in (1, 2)],
                 files=sorted(os.listdir(out)))
        if not keys:
            return r
        r.update(calibration=s.calibration, json=json.load(open(out + '0_calibration.json')),
                 npy=[np.load(out + '0_confidence_%d.npy' % k) for k in (1, 2)],
                 conf_png=[np.asarray(Image.open(out + '0_conf_%d.png' % k)) for k in (1, 2)],
                 K=cfg['Categories_Number'])
        # 50 coloured pixels: float64 statistics of the engine's logits at the beta the solver used
        rng = np.random.default_rng(11)
        xs, ys = np.nonzero(r['npy'][0][0] > 0)
        pick = rng.permutation(len(xs))[:50]
        xy = np.stack([xs[pick], ys[pick]], 1).astype(np.int32)
        logits = s.eval_engine.predict(_dev(xy))[0].cpu().numpy()
        r.update(sample_xy=xy, sample=R.stats(logits, s._beta(s._temperature_used()[0])))
        # the engine's whole-set methods on an engine of 100-pixel chunks: the test pixels in ten chunks, the validation split
        from dmf.engine import EvalEngine
        small = EvalEngine(s.cur_model, s.scene, 100)
        beta = s._beta(s._temperature_used()[0])
        r.update(engine_hist=small.calibration(*s._test_pixels(True), 15, inv_temp=beta).cpu().numpy(),
                 engine_fit=small.fit_temperature(*s._valid_split()), engine_maps=small.confidence_maps(
                     torch.cat([s._xy_labels(b)[0] for b in s.color_index_loader1]), 40, 40, beta))
        # the drop-in path on the same weights and the same split (same seed)
        cfg0 = dict(cfg, fast_path=0, train=dict(cfg['train'], index=0))
        torch.manual_seed(SEED)
        d = Solver(cfg0)
        d.dataloader()
        d.test()
        d.color()
        r.update(dropin=d.calibration, dropin_matrix=d.test_matrix.copy(), dropin_npy=d.confidence_maps)
        return r
    finally:
        shutil.rmtree(tmp)


@pytest.mark.parametrize('net', sorted(NETS))
def test_the_keys_change_nothing_that_was_there(golden_dir, net):
    on, off = _run(net, True, golden_dir), _run(net, False, golden_dir)
    assert off['matrix'].sum() > 0 and np.array_equal(on['matrix'], off['matrix'])
    assert on['maps'][0].tobytes() == off['maps'][0].tobytes() and on['maps'][1].tobytes() == off['maps'][1].tobytes()
    assert on['png'] == off['png'] and len(on['png'][0]) > 0
    new = {'0_calibration.json', '0_confidence_1.npy', '0_confidence_2.npy', '0_conf_1.png', '0_conf_2.png'}
    assert set(on['files']) - set(off['files']) == new and set(off['files']) <= set(on['files'])


@pytest.mark.parametrize('net', sorted(NETS))
def test_the_calibration_block(golden_dir, net):
    r = _run(net, True, golden_dir)
    c = r['calibration']
    assert r['json'] == json.loads(json.dumps(c))
    hist = np.array(c['hist'], dtype=np.int64)
    assert hist.shape == (15, 3) and c['bins'] == 15
    assert hist[:, 0].sum() == r['matrix'].sum() == c['n'] and hist[:, 1].sum() == np.trace(r['matrix'])
    ece, mce = R.ece_mce(hist)
    assert abs(c['ece'] - ece) <= 1e-12 and abs(c['mce'] - mce) <= 1e-12 and 0.0 <= c['ece'] <= c['mce'] <= 1.0
    f = c['fit']
    print('%s: fit %s; ECE %.4f (before scaling %.4f), NLL %.4f (before %.4f)'
          % (net, f, c['ece'], c['before']['ece'], c['nll'], c['before']['nll']))
    assert f['steps'] == 40 and f['n'] == 56 and 2.0 ** -6 < f['beta'] < 2.0 ** 6
    assert f['nll_at_T'] <= f['nll_at_1']                   # 1 lies in the bracket and the NLL is convex in beta
    assert c['temperature'] == 1.0 / f['beta'] and c['before']['temperature'] == 1.0 and c['before']['n'] == c['n']
    assert np.array(c['before']['hist'])[:, 1].sum() == hist[:, 1].sum()            # scaling keeps every argmax


@pytest.mark.parametrize('net', sorted(NETS))
def test_the_engine_methods_in_small_chunks(golden_dir, net):
    """EvalEngine.calibration, .fit_temperature and .confidence_maps on an engine of 100-pixel chunks give what the solver got
    from its one-chunk engine: a pixel's logits do not depend on its batch, the histogram is integers, the fit is bit-reproducible."""
    r = _run(net, True, golden_dir)
    c = r['calibration']
    assert np.array_equal(r['engine_hist'], np.array(c['hist'], dtype=np.int64))
    state = r['engine_fit']
    assert state.shape == (8,) and state[0] == c['fit']['beta'] and state[6] == 40 and state[4] <= state[0] <= state[5]
    label, planes = r['engine_maps']
    assert np.array_equal(label.cpu().numpy(), r['maps'][0]) and planes.cpu().numpy().tobytes() == r['npy'][0].tobytes()


@pytest.mark.parametrize('net', sorted(NETS))
def test_the_confidence_maps(golden_dir, net):
    r = _run(net, True, golden_dir)
    K = r['K']
    m1, m2 = r['npy']
    assert m1.shape == m2.shape == (3, 40, 40) and m1.dtype == np.float32
    xy = r['sample_xy']
    assert len(xy) == 50
    worst = max(float(np.abs(m1[k][xy[:, 0], xy[:, 1]].astype(np.float64) - r['sample'][1 + k]).max()) for k in range(3))
    print('%s: 50 sampled pixels against float64, largest absolute error %.3e, tol(K) %.3e' % (net, worst, R.tol(K)))
    assert worst <= R.tol(K)
    assert np.array_equal(r['maps'][0][xy[:, 0], xy[:, 1]], r['sample'][0])
    # a pixel that is not coloured is 0 in all planes; a coloured one has a confidence of at least 1 / K
    for m, label in zip((m1, m2), r['maps']):
        assert (m[:, label == 0] == 0).all() and (m[0][label != 0] >= 1.0 / K - 1e-6).all()
    for m, png in zip((m1, m2), r['conf_png']):
        assert png.dtype == np.uint8 and np.array_equal(png, np.round(255.0 * m[0].astype(np.float64)).astype(np.uint8))


@pytest.mark.parametrize('net', sorted(NETS))
def test_the_drop_in_path_gives_the_same_block(golden_dir, net):
    r = _run(net, True, golden_dir)
    c, d = r['calibration'], r['dropin']
    print('%s: predictions that differ between the paths: %d of %d' % (net, int(np.abs(r['matrix'] - r['dropin_matrix']).sum() // 2), c['n']))
    hc, hd = np.array(c['hist'], dtype=np.int64), np.array(d['hist'], dtype=np.int64)
    print('%s: fast ECE %.12f, drop-in ECE %.12f; fitted beta %.9f / %.9f; confidence sums differ by %s (units of 2^-32)'
          % (net, c['ece'], d['ece'], c['fit']['beta'], d['fit']['beta'], (hc[:, 2] - hd[:, 2]).tolist()))
    assert (c['n'], c['bins'], c['fit']['n'], c['fit']['steps']) == (d['n'], d['bins'], d['fit']['n'], d['fit']['steps'])
    assert np.array_equal(hc[:, :2], hd[:, :2])
    if np.array_equal(hc, hd):
        assert abs(c['ece'] - d['ece']) <= 1e-12
    for block in (c, d):                                    # one function, utils/calibration.py: 1e-12 on identical histograms
        ece, mce = R.ece_mce(block['hist'])
        assert abs(block['ece'] - ece) <= 1e-12 and abs(block['mce'] - mce) <= 1e-12
    # the two paths form their logits in different fp32 orders: confidences agree to a few ulps per pixel, ECE with them
    K = r['K']
    assert np.abs(hc[:, 2] - hd[:, 2]).max() <= c['n'] * 2 ** 32 * 1e-4 and abs(c['ece'] - d['ece']) <= 1e-4
    assert abs(c['fit']['beta'] - d['fit']['beta']) <= 1e-4 * d['fit']['beta']
    assert np.abs(r['npy'][1] - r['dropin_npy'][1]).max() <= 1e-3
