"""GPU: spatial regularisation of class maps — dmf_spatial_affinity, dmf_prob_scatter and dmf_spatial_filter against
the float64 statement of tests/spatial_ref.py on the cases of tests/spatial_cases.py (whose guards are CPU tests in
tests/test_spatial_host.py), EvalEngine.probability_map / regularise end to end, and the solver keys on the 40 x 40 x 8, 4-class
scene of tests/test_gpu_calibration.py.

Bounds (derived, not fitted; each test prints its largest ratio before it asserts):
  affinity   |delta| <= aff (E (C + 4) + 4) 2^-24, E the reference's exponent argument: a C-term fp32 sum of non-negative terms,
             the divide, the two products, expf.  Out-of-scene neighbours are exactly 0, the centre exactly 1.
  scatter    calib_ref.tol(K) absolute; prob[pred] is the bits of dmf_softmax_stats's conf.
  filter     the device's own aff and fp32 prob go into the float64 reference, so only the filter's rounding is compared:
             |delta| <= out (2 n + 4) 2^-24 where out >= 1e-30, 1e-30 below.  The label map equals the reference's argmax on every
             masked pixel whose top-2 margin exceeds parity_cases.MARGIN.

Observed on an MI355X (printed by the tests): affinity at most 0.69 of its bound over 144 cases; scatter at most
5.6e-8 from float64 (tol(2) = 3.6e-6); filter at most 0.30 of its bound over 72 cases, 10 - 24 pixels per radius inside the margin;
the engine's 13 x 9 pass at 0.22 (affinity) and 0.15 (filter) of the bounds; the drop-in path's map equal to the fast path's at all
1600 pixels of the solver's scene."""
import ctypes as C
import functools
import json
import os
import shutil
import tempfile

import numpy as np
import pytest
import torch
from PIL import Image

import calib_ref
import spatial_cases as S
import spatial_ref as R
from parity_cases import MARGIN

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                 # (a copy: the cases are read-only arrays)


def _affinity_gpu(scene, H, W, r, fill=-3.0):
    from dmf import lib
    aff = torch.full((H, W, (2 * r + 1) ** 2), fill, dtype=torch.float32, device=DEV)
    lib.spatial_affinity(scene if torch.is_tensor(scene) else _dev(scene), H, W, r, S.SIGMA_S, S.SIGMA_R, aff)
    return aff


# ------------------------------------------------------------------------------------------------ dmf_spatial_affinity
@pytest.mark.parametrize('r', S.RADII)
def test_affinity_against_float64(r):
    worst, n = 0.0, (2 * r + 1) ** 2
    for H, W, Cn, half in S.AFFINITY_CASES:
        a = S.scene(H, W, Cn, half)
        got_dev = _affinity_gpu(a, H, W, r)
        got = got_dev.cpu().numpy()
        want, E = R.affinity(a, H, W, r, S.SIGMA_S, S.SIGMA_R)
        outside = want == 0.0
        assert (got[outside] == 0.0).all() and (got[:, :, (n - 1) // 2] == 1.0).all(), (H, W, Cn, half)
        assert outside.sum() == sum(1 for i in range(H) for j in range(W) for di, dj in R.window(r)
                                    if not (0 <= i + di < H and 0 <= j + dj < W))
        bound = R.affinity_bound(want, E, Cn)
        ratio = np.abs(got.astype(np.float64) - want)[~outside] / bound[~outside]
        worst = max(worst, float(ratio.max()))
        assert ratio.max() <= 1.0, (H, W, Cn, half, float(ratio.max()))
        assert torch.equal(_affinity_gpu(a, H, W, r, fill=5.0), got_dev), (H, W, Cn, half)     # two calls: the same bits
    print('r = %d: largest |delta| / bound over %d cases: %.3f' % (r, len(S.AFFINITY_CASES), worst))


@pytest.mark.parametrize('Cn,half', [(3, False), (200, False), (8, True), (1, False)])
def test_affinity_with_a_pitch_and_an_element_aligned_base(Cn, half):
    """The leading 35 x 34 pixels of a scene [37, 39, C] that starts one element into its buffer give the bits of the plain
    layout; what lies beyond column W and row H (here: huge values) is never read."""
    H, W, r = 35, 34, 2
    a = S.scene(H, W, Cn, half)
    dt = torch.float16 if half else torch.float32
    big = np.full((H + 2, W + 5, Cn), 1000.0, dtype=a.dtype)
    big[:H, :W] = a
    flat = torch.empty(big.size + 1, dtype=dt, device=DEV)
    view = flat[1:].view(big.shape)
    view.copy_(torch.from_numpy(big))
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    assert torch.equal(_affinity_gpu(view, H, W, r), _affinity_gpu(a, H, W, r))


# ------------------------------------------------------------------------------------------------ dmf_prob_scatter
@pytest.mark.parametrize('K', S.SCATTER_K)
def test_scatter_against_float64_and_softmax_stats(K):
    from dmf import lib
    H, W = 19, 23
    worst = 0.0
    for B in S.SCATTER_B:
        logits = calib_ref.stats_logits(K, B, 1.0)
        cells = np.random.default_rng(100 * K + B).permutation(H * W)[:B]
        xy = np.stack([cells // W, cells % W], 1).astype(np.int32)
        for beta in S.SCATTER_BETA:
            inv = None if beta == 1.0 else torch.tensor([beta], dtype=torch.float32, device=DEV)
            prob = torch.full((H, W, K), -7.0, device=DEV)
            mask = torch.full((H, W), 9, dtype=torch.uint8, device=DEV)
            lib.prob_scatter(_dev(logits), _dev(xy), W, prob, mask, inv_temp=inv)
            pred = torch.empty(B, dtype=torch.int32, device=DEV)
            conf = torch.empty(B, device=DEV)
            lib.softmax_stats(_dev(logits), pred=pred, conf=conf, inv_temp=inv)
            p, m = prob.cpu().numpy(), mask.cpu().numpy()
            touched = np.zeros((H, W), dtype=bool)
            touched[xy[:, 0], xy[:, 1]] = True
            assert (p[~touched] == -7.0).all() and (m[~touched] == 9).all() and (m[touched] == 1).all()
            rows = p[xy[:, 0], xy[:, 1]]
            worst = max(worst, float(np.abs(rows.astype(np.float64) - R.softmax(logits, beta)).max()))
            assert rows[np.arange(B), pred.cpu().numpy()].tobytes() == conf.cpu().numpy().tobytes(), (B, beta)
    print('K = %d: largest absolute error %.3e, tol(K) %.3e' % (K, worst, calib_ref.tol(K)))
    assert worst <= calib_ref.tol(K)


# ------------------------------------------------------------------------------------------------ dmf_spatial_filter
def _filter_inputs(H, W, K, r):
    """Device (aff, prob, mask): the kernel's own affinities of the 8-band case scene, the case's logits scattered at the masked
    pixels into a prob full of NaN (an unmasked row is never read)."""
    from dmf import lib
    aff = _affinity_gpu(S.scene(H, W, 8), H, W, r)
    mask_np = S.mask(H, W)
    keep = mask_np.reshape(-1) != 0
    prob = torch.full((H, W, K), float('nan'), device=DEV)
    mask = torch.zeros(H, W, dtype=torch.uint8, device=DEV)
    if keep.any():
        lib.prob_scatter(_dev(S.logits(H, W, K)[keep]), _dev(S.pixels(H, W)[keep]), W, prob, mask)
    assert np.array_equal(mask.cpu().numpy(), mask_np)
    return aff, prob, mask


@pytest.mark.parametrize('r', S.RADII)
def test_filter_against_float64(r):
    from dmf import lib
    worst, left_out, n = 0.0, 0, (2 * r + 1) ** 2
    for H, W, K in S.FILTER_CASES:
        aff, prob, mask = _filter_inputs(H, W, K, r)
        out = torch.full((H, W, K), -7.0, device=DEV)
        label = torch.full((H, W), -7, dtype=torch.int32, device=DEV)
        lib.spatial_filter(prob, mask, aff, out, label)
        live = mask.cpu().numpy() != 0
        want, pred = R.filter_once(np.nan_to_num(prob.cpu().numpy().astype(np.float64)), live, aff.cpu().numpy().astype(np.float64), r)
        got, lab = out.cpu().numpy(), label.cpu().numpy()
        assert (got[~live] == 0.0).all() and (lab[~live] == -7).all(), (H, W, K)
        if live.any():
            ratio = np.abs(got.astype(np.float64) - want)[live] / R.filter_bound(want, n)[live]
            worst = max(worst, float(ratio.max()))
            assert ratio.max() <= 1.0, (H, W, K, float(ratio.max()))
            clear = live & (R.top2_margin(want) > MARGIN)
            left_out += int((live & ~clear).sum())
            assert np.array_equal(lab[clear], pred[clear]), (H, W, K)
            assert (lab[live] >= 0).all() and (lab[live] < K).all()
        again, label2 = torch.empty_like(out), torch.full_like(label, -7)
        lib.spatial_filter(prob, mask, aff, again, label2)
        assert again.cpu().numpy().tobytes() == got.tobytes() and torch.equal(label2, label)
    print('r = %d: largest |delta| / bound %.3f; pixels inside the margin %d' % (r, worst, left_out))


def test_filter_refuses_an_aliased_output_and_bad_shapes():
    from dmf import lib
    H, W, K, r = 13, 9, 3, 1
    aff, prob, mask = _filter_inputs(H, W, K, r)
    label = torch.full((H, W), -7, dtype=torch.int32, device=DEV)
    before = prob.clone()
    with pytest.raises(lib.DmfError, match='overlaps'):
        lib.spatial_filter(prob, mask, aff, prob, label)
    flat = torch.zeros(2 * H * W * K, device=DEV)
    a, b = flat[:H * W * K].view(H, W, K), flat[K:K + H * W * K].view(H, W, K)        # shifted by one row of classes: they overlap
    with pytest.raises(lib.DmfError, match='overlaps'):
        lib.spatial_filter(a, mask, aff, b, label)
    assert (label == -7).all() and prob.cpu().numpy().tobytes() == before.cpu().numpy().tobytes()
    for bad in (dict(aff=aff[:, :, :8].contiguous()), dict(mask=mask[:-1].contiguous()), dict(label=label.long())):
        kw = dict(dict(aff=aff, mask=mask, label=label), **bad)
        with pytest.raises(lib.DmfError):
            lib.spatial_filter(prob, kw['mask'], kw['aff'], torch.empty_like(prob), kw['label'])
    with pytest.raises(lib.DmfError, match='radius'):
        lib.spatial_affinity(_dev(S.scene(H, W, 3)), H, W, 4, 2.0, 0.1, torch.empty(H, W, 81, device=DEV))
    with pytest.raises(lib.DmfError, match='pixels asked'):
        lib.spatial_affinity(_dev(S.scene(H, W, 3)), H + 1, W, 1, 2.0, 0.1, torch.empty(H + 1, W, 9, device=DEV))


def test_every_argument_error_returns_a_code_without_a_launch():
    """The entry points themselves (ctypes): each refusal has its code and leaves prob, mask, aff, out and label as they were."""
    from dmf import lib
    H, W, K, Cn, r, B = 7, 5, 3, 4, 1, 6
    scene = _dev(S.scene(H, W, Cn))
    logits, xy = _dev(S.logits(H, W, K)[:B]), _dev(S.pixels(H, W)[:B])
    aff, prob, out = (torch.full(s, -7.0, device=DEV) for s in ((H, W, 9), (H, W, K), (H, W, K)))
    mask = torch.full((H, W), 9, dtype=torch.uint8, device=DEV)
    label = torch.full((H, W), -7, dtype=torch.int32, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    f = lib._lib

    def scatter(logits=p(logits), B=B, K=K, xy=p(xy), W=W, prob=p(prob), mask=p(mask)):
        return f.dmf_prob_scatter(logits, B, K, None, xy, W, prob, mask, st)

    def affinity(scene=p(scene), eb=4, pitch=W, H=H, W=W, Cn=Cn, r=r, aff=p(aff)):
        return f.dmf_spatial_affinity(scene, eb, pitch, H, W, Cn, r, 0.125, 50.0, aff, st)

    def filt(pin=p(prob), mask=p(mask), aff=p(aff), H=H, W=W, K=K, r=r, pout=p(out), label=p(label)):
        return f.dmf_spatial_filter(pin, mask, aff, H, W, K, r, pout, label, st)

    want = [(scatter(logits=None), 1), (scatter(xy=None), 1), (scatter(prob=None), 1), (scatter(mask=None), 1), (scatter(B=-1), 2),
            (scatter(W=0), 2), (scatter(K=0), 3), (scatter(K=65), 3),
            (affinity(scene=None), 1), (affinity(aff=None), 1), (affinity(H=0), 2), (affinity(W=0), 2), (affinity(Cn=0), 2),
            (affinity(r=0), 4), (affinity(r=4), 4), (affinity(eb=3), 5), (affinity(eb=8), 5), (affinity(pitch=W - 1), 6),
            (affinity(scene=C.c_void_p(scene.data_ptr() + 2)), 8),
            (filt(pin=None), 1), (filt(mask=None), 1), (filt(aff=None), 1), (filt(pout=None), 1), (filt(label=None), 1),
            (filt(H=0), 2), (filt(W=-1), 2), (filt(K=0), 3), (filt(K=65), 3), (filt(r=0), 4), (filt(r=4), 4), (filt(pout=p(prob)), 7)]
    assert [rc for rc, _ in want] == [code for _, code in want]
    assert scatter(B=0) == 0                                                          # a no-op
    torch.cuda.synchronize()
    assert (aff == -7).all() and (prob == -7).all() and (out == -7).all() and (mask == 9).all() and (label == -7).all()


# ------------------------------------------------------------------------------------------------ the engine, end to end
@pytest.mark.parametrize('half,tta', [(False, None), (False, 'flips'), (True, None)], ids=['fp32', 'fp32-flips', 'fp16'])
def test_probability_map_and_regularise_through_the_engine(half, tta):
    """The 13 x 9 tiny1 scene (as a d4 atlas: slot 0 is the scene), all 117 pixels in chunks of 50."""
    from dmf import lib
    from dmf.engine import EvalEngine
    from test_gpu_augment import H, W, _case
    c = _case('tiny1', half, False)
    scene, K, r = c['scene'], c['K'], 2
    ev = EvalEngine(c['hip'], scene, 50, tta=tta)
    xy = c['xy']
    assert len(xy) == H * W == 117
    beta = 0.5
    prob, mask = ev.probability_map(xy, H, W, inv_temp=beta)
    logits = ev.collect_logits(xy).cpu().numpy()
    want_prob, want_mask = R.scatter(logits, xy, H, W, beta)
    assert np.array_equal(mask.cpu().numpy(), want_mask) and mask.dtype == torch.uint8 and want_mask.all()
    err = float(np.abs(prob.cpu().numpy().astype(np.float64) - want_prob).max())
    aff = scene.affinity(H, W, r, S.SIGMA_S, S.SIGMA_R)
    assert scene.affinity(H, W, r, S.SIGMA_S, S.SIGMA_R) is aff and scene.affinity(H, W, 1, S.SIGMA_S, S.SIGMA_R) is not aff
    aff = scene.affinity(H, W, r, S.SIGMA_S, S.SIGMA_R)
    A = c['A'].numpy()
    A = A.astype(np.float16) if half else A
    want_aff, E = R.affinity(A, H, W, r, S.SIGMA_S, S.SIGMA_R)
    inside = want_aff != 0
    ratio_a = float((np.abs(aff.cpu().numpy().astype(np.float64) - want_aff)[inside] / R.affinity_bound(want_aff, E, A.shape[2])[inside]).max())
    out, label = ev.regularise(prob, mask, aff, iterations=1)
    want, pred = R.filter_once(prob.cpu().numpy().astype(np.float64), want_mask, aff.cpu().numpy().astype(np.float64), r)
    ratio_f = float((np.abs(out.cpu().numpy().astype(np.float64) - want) / R.filter_bound(want, 25)).max())
    clear = R.top2_margin(want) > MARGIN
    print('%s, tta %s: prob error %.3e (tol %.3e); affinity %.3f and filter %.3f of their bounds; %d of 117 pixels inside the margin, '
          '%d changed class' % ('fp16' if half else 'fp32', tta, err, calib_ref.tol(K), ratio_a, ratio_f, int((~clear).sum()),
                                int((pred != want_prob.argmax(2)).sum())))
    assert err <= calib_ref.tol(K) and ratio_a <= 1.0 and ratio_f <= 1.0
    assert label.dtype == torch.int32 and np.array_equal(label.cpu().numpy()[clear], pred[clear])
    # iterations = 3 is three single calls, bit for bit; prob itself is not written
    kept = prob.clone()
    three, label3 = ev.regularise(prob, mask, aff, iterations=3)
    bufs = [torch.empty_like(prob) for _ in range(3)]
    lab = torch.zeros(H, W, dtype=torch.int32, device=DEV)
    src = prob
    for b in bufs:
        lib.spatial_filter(src, mask, aff, b, lab)
        src = b
    assert torch.equal(three, bufs[2]) and torch.equal(label3, lab) and torch.equal(prob, kept)
    with pytest.raises(lib.DmfError, match='iterations'):
        ev.regularise(prob, mask, aff, iterations=0)
    # a partial set: the cells of the other pixels are 0 in prob, mask and the label map
    some = xy[::3]
    p2, m2 = ev.probability_map(some, H, W)
    o2, l2 = ev.regularise(p2, m2, aff)
    off = m2.cpu().numpy() == 0
    assert off.sum() == 117 - len(some) and (p2.cpu().numpy()[off] == 0).all() and (o2.cpu().numpy()[off] == 0).all() \
        and (l2.cpu().numpy()[off] == 0).all()
    with pytest.raises(lib.DmfError, match='outside'):
        ev.probability_map(xy, H, W - 1)


# ------------------------------------------------------------------------------------------------ the solver
SEED = 3407
BASE = {'test': dict(calibration=1, calibration_bins=15, temperature=1.5)}        # (a fixed T: both paths read the same beta)
KEYS_ON = {'test': dict(spatial='bilateral', spatial_radius=2, spatial_sigma_s=2.0, spatial_sigma_r=0.1, spatial_iterations=1),
           'color': dict(spatial=1)}
NETS = {'late_fusion': 'plain_native_loop', 'attention': 'attention'}


def _read(path):
    with open(path, 'rb') as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def _run(net, keys, golden_dir):
    """Two epochs of Solver.train() on the epoch-block scene with the calibration on, then test() and color(); with `keys` also
    what the spatial keys leave, the engine's own regularised map with its float64 margins, and the same test() / color() by a
    drop-in solver (fast_path: 0) on the weights this run saved."""
    from solver.mainsolver import Solver
    from test_gpu_epoch_block import _cfg
    tmp = tempfile.mkdtemp(prefix='dmf_spatial_')
    try:
        cfg = _cfg(golden_dir, tmp, NETS[net], 1)
        cfg['epoch'] = 2
        for sec, val in list(BASE.items()) + (list(KEYS_ON.items()) if keys else []):
            cfg[sec] = dict(cfg[sec], **val)
        torch.manual_seed(SEED)
        s = Solver(cfg)
        s.dataloader()
        s.train()
        s.test()
        s.color()
        rng_after = torch.rand(4)
        out = cfg['RESULT_output']
        r = dict(matrix=s.test_matrix.copy(), result=list(s.result[:3]), maps=s.label_maps, rng_after=rng_after,
                 png=[_read(out + '0_pic_%d.png' % k) for k in (1, 2)], calibration=_read(out + '0_calibration.json'),
                 files=sorted(os.listdir(out)))
        if not keys:
            return r
        lut = np.asarray(cfg['DATA_DICT'][cfg['data_city']]['color'], dtype=np.uint8)
        r.update(spatial=s.spatial, json=json.load(open(out + '0_spatial.json')), spatial_maps=s.spatial_maps, lut=lut,
                 spatial_png=[np.asarray(Image.open(out + '0_pic_%d_spatial.png' % k)) for k in (1, 2)])
        # the engine's own pass over the whole scene, and the float64 margins of its result
        xy = torch.from_numpy(s._scene_pixels())
        beta = s._beta(1.5)
        prob, mask = s.eval_engine.probability_map(xy, 40, 40, beta)
        aff = s.scene.affinity(40, 40, 2, 2.0, 0.1)
        _, label = s.eval_engine.regularise(prob, mask, aff, 1)
        want, _ = R.filter_once(prob.cpu().numpy().astype(np.float64), mask.cpu().numpy(), aff.cpu().numpy().astype(np.float64), 2)
        r.update(engine_label=label.cpu().numpy(), margin=R.top2_margin(want), n_pixels=int(mask.sum().item()),
                 plain_label=s.eval_engine.label_map(xy, 40, 40).cpu().numpy())
        test_rows = np.asarray(s.test_index_loader.dataset.indices)
        r.update(test_xy=s._set_pixels(test_rows), test_lab=s.index_dataset.label[test_rows].astype(np.int64),
                 labelled_xy=s._set_pixels(s.matrix_[1]))
        cfg0 = dict(cfg, fast_path=0, train=dict(cfg['train'], index=0))
        torch.manual_seed(SEED)
        d = Solver(cfg0)
        d.dataloader()
        d.test()
        d.color()
        r.update(dropin=d.spatial, dropin_maps=d.spatial_maps)
        return r
    finally:
        shutil.rmtree(tmp)


@pytest.mark.parametrize('net', sorted(NETS))
def test_the_keys_change_nothing_that_was_there(golden_dir, net):
    on, off = _run(net, True, golden_dir), _run(net, False, golden_dir)
    assert off['matrix'].sum() > 0 and np.array_equal(on['matrix'], off['matrix']) and on['result'] == off['result']
    assert on['maps'][0].tobytes() == off['maps'][0].tobytes() and on['maps'][1].tobytes() == off['maps'][1].tobytes()
    assert on['png'] == off['png'] and len(on['png'][0]) > 0 and on['calibration'] == off['calibration'] and len(on['calibration']) > 0
    assert torch.equal(on['rng_after'], off['rng_after'])                           # torch's RNG stream is where it was
    new = {'0_spatial.json', '0_pic_1_spatial.png', '0_pic_2_spatial.png'}
    assert set(on['files']) - set(off['files']) == new and set(off['files']) <= set(on['files'])


@pytest.mark.parametrize('net', sorted(NETS))
def test_the_spatial_block(golden_dir, net):
    r = _run(net, True, golden_dir)
    b = r['spatial']
    assert r['json'] == json.loads(json.dumps(b))
    m = np.array(b['matrix'])
    assert m.shape == r['matrix'].shape and m.sum() == r['matrix'].sum() == b['n'] == len(r['test_xy'])
    assert np.array_equal(m.sum(0), r['matrix'].sum(0))                             # the same pixels: the same targets per class
    aa, oa, k = r['result']
    assert b['before'] == dict(OA=oa, AA=aa, kappa=k)
    assert (b['kind'], b['radius'], b['sigma_s'], b['sigma_r'], b['iterations']) == ('bilateral', 2, 2.0, 0.1, 1)
    x, y = r['test_xy'][:, 0], r['test_xy'][:, 1]
    want = np.zeros_like(m)
    np.add.at(want, (r['engine_label'][x, y], r['test_lab']), 1)
    assert np.array_equal(m, want)
    assert b['changed'] == int((r['engine_label'][x, y] != r['plain_label'][x, y]).sum())
    print('%s: OA %.4f -> %.4f, kappa %.4f -> %.4f, %d of %d test pixels changed class'
          % (net, b['before']['OA'], b['after']['OA'], b['before']['kappa'], b['after']['kappa'], b['changed'], b['n']))


@pytest.mark.parametrize('net', sorted(NETS))
def test_the_spatial_maps(golden_dir, net):
    r = _run(net, True, golden_dir)
    assert r['n_pixels'] == 1600                                                    # both colour sets: the whole scene
    m1, m2 = r['spatial_maps']
    assert np.array_equal(m2, r['engine_label']) and np.array_equal(r['spatial_png'][1], r['lut'][r['engine_label']])
    labelled = np.zeros((40, 40), dtype=bool)
    labelled[r['labelled_xy'][:, 0], r['labelled_xy'][:, 1]] = True
    assert 0 < labelled.sum() <= 1600 and np.array_equal(r['spatial_png'][0], r['lut'][m1])
    assert (m1[~labelled] == 0).all() and np.array_equal(m1[labelled], r['engine_label'][labelled])


@pytest.mark.parametrize('net', sorted(NETS))
def test_the_drop_in_path_gives_the_same_map_outside_the_margin(golden_dir, net):
    r = _run(net, True, golden_dir)
    clear = r['margin'] > MARGIN
    differ = r['dropin_maps'][1] != r['spatial_maps'][1]
    print('%s: %d of 1600 pixels inside the margin; the paths differ at %d pixels, %d of them outside it'
          % (net, int((~clear).sum()), int(differ.sum()), int((differ & clear).sum())))
    assert not (differ & clear).any()
    assert r['dropin']['n'] == r['spatial']['n'] and r['dropin']['radius'] == 2
