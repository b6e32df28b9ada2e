"""GPU: flip / rotate augmentation and test-time augmentation from a scene atlas.

dmf_scene_atlas against the numpy atlas of tests/aug_ref.py (bits); the untouched patch kernels reading the atlas at mapped
coordinates against the oracle fed the transformed materialised patches (forward, gradients: the tolerances of
tests/test_gpu_parity.py, unchanged) and against themselves on host-transformed scenes (bits); dmf_logits_mean against its stated
fp32 expression (bits); EvalEngine(tta=) end to end; the solver's routes with `schedule.augment` / `test.tta`.
"""
import ctypes as C
import functools
import os
import shutil
import tempfile

import numpy as np
import pytest
import torch

import aug_ref
from test_gpu_half import half_nets, scene as half_scene
from test_gpu_parity import SHAPES, _attn_nets, _scene, assert_close, nets, ref_grads

pytestmark = pytest.mark.gpu
H, W = 13, 9
SEED = 123


# ---------------------------------------------------------------------------------------------- 1. the atlas, bit for bit
def _atlas_case(rows, cols, Cn, eb, ops, src_pitch=None, slack=(0, 0), offset=0, seed=0):
    """Source of random bits (integers: no NaN compares unequal), the kernel's atlas over a poisoned dst, numpy's atlas."""
    from dmf import lib
    dt_np, dt = (np.int16, torch.int16) if eb == 2 else (np.int32, torch.int32)
    rng = np.random.default_rng(seed)
    pitch = src_pitch or cols
    info = np.iinfo(dt_np)
    X = rng.integers(info.min, info.max, size=(rows + 1, pitch, Cn), dtype=dt_np)
    flat = torch.empty(X.size + 8, dtype=dt, device='cuda')            # `offset` elements in: a base that is not 16-byte aligned
    src = flat[offset:offset + X.size].view(X.shape)
    src.copy_(torch.from_numpy(X))
    R, Wq = aug_ref.geometry(rows, cols, ops)
    R, Wq = R + slack[0], Wq + slack[1]
    dst = torch.full((len(ops) * R, Wq, Cn), -1, dtype=dt, device='cuda')
    lib.scene_atlas(src, rows, cols, ops, R, dst)
    want = aug_ref.atlas(X, rows, cols, ops, R, Wq)
    return dst, torch.from_numpy(want)


@pytest.mark.parametrize('ops', [aug_ref.FLIPS, aug_ref.D4, (0, 5)], ids=['flips', 'd4', 'op5'])
@pytest.mark.parametrize('Cn,eb', [(1, 4), (3, 4), (8, 4), (200, 4), (8, 2), (200, 2),
                                   (2, 4), (1, 2), (5, 2), (12, 4), (13, 4)])       # (the second row: units of 8 and 2 bytes, the narrow limit)
@pytest.mark.parametrize('rows,cols', [(17, 13), (41, 45), (64, 96)])
def test_scene_atlas_bits(rows, cols, Cn, eb, ops):
    got, want = _atlas_case(rows, cols, Cn, eb, ops)
    assert got.shape == want.shape and torch.equal(got.cpu(), want)


@pytest.mark.parametrize('Cn,eb', [(1, 4), (3, 4), (200, 4), (8, 2)])
def test_scene_atlas_pitch_slack_and_unaligned_base(Cn, eb):
    """src_pitch > cols; slots larger than the variants need (filler below and right of every variant); bases 4 or 2 bytes past
    a 16-byte boundary (narrower units)."""
    for kw in (dict(src_pitch=51), dict(slack=(3, 2)), dict(offset=1), dict(src_pitch=47, slack=(1, 5), offset=3)):
        for ops in (aug_ref.FLIPS, aug_ref.D4):
            got, want = _atlas_case(41, 45, Cn, eb, ops, **kw)
            assert torch.equal(got.cpu(), want), (kw, ops)


def test_scene_atlas_argument_errors_return_without_a_launch():
    from dmf import lib
    src = torch.zeros(8, 6, 3, dtype=torch.int32, device='cuda')
    dst = torch.full((2 * 8, 8, 3), 7, dtype=torch.int32, device='cuda')
    ops_t = C.c_int32 * 8

    def call(src_p=src.data_ptr(), eb=4, rows=8, cols=6, pitch=6, Cn=3, ops=(0, 5), n=2, R=8, Wq=8, dst_p=dst.data_ptr()):
        o = None if ops is None else ops_t(*(list(ops) + [0] * (8 - len(ops))))
        return lib._lib.dmf_scene_atlas(C.c_void_p(src_p), eb, rows, cols, pitch, Cn, o, n, R, Wq, C.c_void_p(dst_p), lib._stream())

    bad = [dict(src_p=None), dict(dst_p=None), dict(ops=None), dict(rows=0), dict(cols=0), dict(Cn=0), dict(pitch=5), dict(eb=1),
           dict(eb=3), dict(eb=8), dict(n=0), dict(n=9), dict(ops=(0, 8)), dict(ops=(0, -1)),
           dict(R=7, ops=(0, 1)), dict(Wq=5, ops=(0, 1)),                  # too small for a plain variant
           dict(R=8, Wq=7), dict(R=5, Wq=8),                               # transposed: slot_rows >= cols, dst_pitch >= rows
           dict(dst_p=src.data_ptr()), dict(dst_p=src.data_ptr() + 64), dict(src_p=dst.data_ptr() + 128)]
    for kw in bad:
        assert call(**kw) != 0, kw
    torch.cuda.synchronize()
    assert bool((dst == 7).all()) and bool((src == 0).all())
    assert call() == 0
    with pytest.raises(lib.DmfError, match='too small'):
        lib.scene_atlas(src, 8, 6, (0, 5), 5, torch.empty(2 * 5, 8, 3, dtype=torch.int32, device='cuda'))


# ---------------------------------------------------------------------------------------------- 2. - 4. the patch kernels on the atlas
CASES = [('tiny', False, False), ('tiny1', False, False), ('hsi', False, False), ('tiny1', True, False), ('tiny1', False, True)]


def _ids(c):
    return c[0] + ('-half' if c[1] else '') + ('-attention' if c[2] else '')


@functools.lru_cache(maxsize=None)
def _case(name, half, attention):
    """Nets, the 13 x 9 scene with its d4 atlas, every pixel in the slot the hash gives it, and the oracle's logits on the
    transformed materialised patches."""
    from dmf.engine import Scene
    C_, C2, P, S, K = SHAPES[name]
    cfg, ref, hip = _attn_nets(name) if attention else half_nets(name) if half else nets(name)
    A, Bm = (half_scene if half else _scene)(name, H, W)
    xy = aug_ref.all_pixels(H, W)
    slots = aug_ref.draw(SEED, 0, xy, 8)
    assert len(set(slots.tolist())) == 8
    a, b = aug_ref.cut(A.numpy(), Bm.numpy(), xy, P, S)
    ta, tb = torch.from_numpy(aug_ref.tf_patches(a, slots)), torch.from_numpy(aug_ref.tf_patches(b, slots))
    with torch.no_grad():
        want = ref(ta, tb)
        plain = ref(torch.from_numpy(a), torch.from_numpy(b))
    assert (want - plain).abs().max().item() > 1e-3            # the net is not symmetric: a variant is another input
    scene = Scene(A.numpy(), Bm.numpy(), 'cuda:0', half=half).atlas(P, S, 'd4')
    return dict(cfg=cfg, ref=ref, hip=hip, A=A, Bm=Bm, xy=xy, slots=slots, ta=ta, tb=tb, want=want, scene=scene, P=P, S=S, K=K)


def _forward(hip, sceneA, sceneB, xy_dev):
    from dmf import lib
    n, K = xy_dev.shape[0], hip.arch['K']
    logits = torch.empty(n, K, device='cuda')
    inp = lib.input_gather(hip.shape, sceneA, sceneB, xy_dev)
    if hip.shape.attention:
        ws = torch.empty(lib.attn_workspace_bytes(hip.shape, n), dtype=torch.uint8, device='cuda')
        lib.forward_attn(hip.shape, inp, hip.flat_parameters(), hip.pool_w, ws, logits)
    else:
        lib.forward(hip.shape, inp, hip.flat_parameters(), hip.pool_w, logits)
    return logits


@pytest.mark.parametrize('case', CASES, ids=_ids)
def test_forward_from_the_atlas_against_the_oracle_on_transformed_patches(case):
    from dmf import lib
    c = _case(*case)
    sc = c['scene']
    assert sc.ops == aug_ref.D4 and sc.extent == tuple(c['A'].shape[:2]) and sc.half == case[1]
    mapped = sc.map_xy(c['xy'], c['slots'])
    assert np.array_equal(mapped, aug_ref.map_xy(c['xy'], c['slots'], sc.ops, *sc.extent, c['P'], sc.slot_rows))
    lib.check_xy_bounds(c['hip'].shape, sc.A, sc.B, mapped)
    xyd = torch.from_numpy(mapped).cuda()
    assert torch.equal(sc.map_xy(torch.from_numpy(c['xy']).cuda(), torch.from_numpy(c['slots']).cuda()), xyd)
    for s in range(8):                                              # one slot for a device batch: the engine's short form
        one = sc.map_xy(torch.from_numpy(c['xy']).cuda(), s)
        assert one.dtype == torch.int32 and one.is_contiguous() and np.array_equal(one.cpu().numpy(), sc.map_xy(c['xy'], s))
    got = _forward(c['hip'], sc.A, sc.B, xyd)
    assert_close(got, c['want'], 2e-4 if case[2] else 1e-5, 0, 'atlas logits %s' % _ids(case))


@pytest.mark.parametrize('case', CASES, ids=_ids)
def test_atlas_logits_are_the_bits_of_a_plain_scene_of_the_transformed_scene(case):
    """Only the base address and the pitch differ between slot s of the atlas and a scene made of the variant itself."""
    from dmf.engine import Scene
    c = _case(*case)
    sc, P, S = c['scene'], c['P'], c['S']
    Hp, Wp = sc.extent
    A, Bm = c['A'].numpy(), c['Bm'].numpy()
    for s, k in enumerate(sc.ops):
        plain = Scene(np.ascontiguousarray(aug_ref.tf(A, k)), np.ascontiguousarray(aug_ref.tf(Bm[:S * Hp, :S * Wp], k)), 'cuda:0',
                      half=case[1])
        local = aug_ref.map_xy(c['xy'], 0, (k,), Hp, Wp, P, 0)                      # the map without the slot offset
        want = _forward(c['hip'], plain.A, plain.B, torch.from_numpy(local).cuda())
        got = _forward(c['hip'], sc.A, sc.B, torch.from_numpy(sc.map_xy(c['xy'], s)).cuda())
        assert torch.equal(got, want), 'variant %d' % k


@pytest.mark.parametrize('name', ['tiny', 'hsi'])
def test_train_gradients_of_a_mixed_variant_batch(name):
    from dmf import lib
    from model.gmfnet import PARAM_ORDER
    c = _case(name, False, False)
    hip, ref, K, B = c['hip'], c['ref'], c['K'], len(c['xy'])
    t = torch.randint(0, K, (B,), generator=torch.Generator().manual_seed(6))
    want_logits, want_loss, want_g = ref_grads(ref, c['ta'], c['tb'], t)
    sc = c['scene']
    xyd = torch.from_numpy(sc.map_xy(c['xy'], c['slots'])).cuda()
    inp = lib.input_gather(hip.shape, sc.A, sc.B, xyd)
    theta = hip.flat_parameters()
    logits = torch.empty(B, K, device='cuda'); loss = torch.empty(B, device='cuda')
    ws = hip.workspace(B)
    lib.train_fwd_bwd(hip.shape, inp, theta, hip.pool_w, t.int().cuda(), 1.0 / B, logits, loss, ws)
    grad = torch.empty_like(theta)
    lib.grad_reduce(hip.shape, B, ws, grad)
    assert_close(logits, want_logits, 1e-5, 0, 'train logits')
    assert abs(loss.mean().item() - want_loss) < 1e-5
    off = hip._offsets
    for i, k in enumerate(PARAM_ORDER):
        g = grad[off[i]:off[i] + want_g[k].numel()].view(want_g[k].shape)
        assert_close(g, want_g[k], 1e-5, 1e-4, 'grad %s [%s, mixed variants]' % (k, name))


def test_atlas_releases_its_source_and_serves_unmapped_coordinates():
    from dmf.engine import AtlasScene, EvalEngine, Scene
    c = _case('tiny1', False, False)
    src = Scene(c['A'].numpy(), c['Bm'].numpy(), 'cuda:0')
    keep = Scene(c['A'].numpy(), c['Bm'].numpy(), 'cuda:0')
    at = src.atlas(c['P'], c['S'], 'flips')
    assert isinstance(at, AtlasScene) and isinstance(at, Scene) and src.A is None and src.B is None
    assert at.ops == aug_ref.FLIPS and at.slot_rows == keep.A.shape[0] and tuple(at.A.shape) == (4 * keep.A.shape[0],) + tuple(keep.A.shape[1:])
    xyd = torch.from_numpy(c['xy']).cuda()
    want = EvalEngine(c['hip'], keep, 128).predict(xyd)[0].clone()
    assert torch.equal(EvalEngine(c['hip'], at, 128).predict(xyd)[0], want)          # slot 0: plain evaluation on the same object


# ---------------------------------------------------------------------------------------------- 5. dmf_logits_mean
@pytest.mark.parametrize('K', [1, 5, 17, 64])
@pytest.mark.parametrize('B', [1, 255, 257])
@pytest.mark.parametrize('V', [1, 3, 4, 8])
def test_logits_mean_is_the_stated_expression(V, B, K):
    from dmf import lib
    g = torch.Generator().manual_seed(100 * V + K)
    host = (torch.randn(V, B, K, generator=g) * 3).numpy()
    lv = torch.from_numpy(host).cuda()
    acc = host[0].copy()
    for v in range(1, V):
        acc = acc + host[v]                                          # float32 adds, in variant order
    want = torch.from_numpy(acc / np.float32(V)).cuda()              # numpy: an IEEE float32 division (torch's device kernel
    assert acc.dtype == np.float32 and want.dtype == torch.float32  # multiplies by the reciprocal of a scalar divisor)
    logits = torch.full((B, K), float('nan'), device='cuda')
    pred = torch.full((B,), -1, dtype=torch.int32, device='cuda')
    lib.logits_mean(lv, logits, pred)
    assert torch.equal(logits, want)
    assert torch.equal(pred.long(), want.argmax(1))
    if V == 1:
        assert torch.equal(logits, lv[0])
    only = torch.empty(B, K, device='cuda')
    lib.logits_mean(lv, only)                                       # pred is optional
    assert torch.equal(only, want)


def test_logits_mean_pred_is_the_first_maximum_and_errors():
    from dmf import lib
    V, B, K = 4, 130, 17
    g = torch.Generator().manual_seed(3)
    lv = torch.randint(-8, 8, (V, B, K), generator=g).float()        # small integers: sums and the division by 4 are exact
    for b in range(B):                                               # plant an exact tie of the row maximum at two or three columns
        cols = torch.randperm(K, generator=g)[:2 + b % 2]
        lv[:, b, cols] = 9.0
    mean = lv.sum(0) / V
    first = torch.tensor([int((mean[b] == mean[b].max()).nonzero()[0]) for b in range(B)])
    assert (mean.max(1).values == 9.0).all() and ((mean == 9.0).sum(1) >= 2).all()
    logits = torch.empty(B, K, device='cuda'); pred = torch.empty(B, dtype=torch.int32, device='cuda')
    lib.logits_mean(lv.cuda(), logits, pred)
    assert torch.equal(logits.cpu(), mean) and torch.equal(pred.cpu().long(), first)
    # B == 0 is a no-op; the argument errors
    lib.logits_mean(torch.empty(3, 0, K, device='cuda'), torch.empty(0, K, device='cuda'))
    p, q, st = C.c_void_p(lv.cuda().data_ptr()), C.c_void_p(logits.data_ptr()), lib._stream()
    f = lib._lib.dmf_logits_mean
    assert f(p, V, 0, K, q, None, st) == 0
    for args in ((None, V, B, K, q), (p, V, B, K, None), (p, 0, B, K, q), (p, V, -1, K, q), (p, V, B, 0, q), (p, V, B, 65, q)):
        assert f(*args, None, st) != 0, args
    with pytest.raises(lib.DmfError, match='logits_v'):
        lib.logits_mean(lv.cuda(), torch.empty(B, K + 1, device='cuda'))


# ---------------------------------------------------------------------------------------------- 6. test-time augmentation end to end
@functools.lru_cache(maxsize=None)
def _tta():
    from aug_cases import tta_case
    from dmf.engine import Scene
    from model.gmfnet import Net as HipNet
    c = tta_case()
    hip = HipNet(c['cfg'])
    hip.load_state_dict(c['state'])
    hip = hip.to('cuda:0')
    scene = Scene(c['A'].numpy(), c['Bm'].numpy(), 'cuda:0').atlas(c['P'], c['S'], 'd4')
    return c, hip, scene


def test_tta_predict_is_the_mean_of_the_single_variant_predictions():
    from dmf import lib
    from dmf.engine import EvalEngine
    c, hip, scene = _tta()
    B = 128                                                         # 437 pixels: three full chunks and one of 53
    ev, one = EvalEngine(hip, scene, B, tta='d4'), EvalEngine(hip, scene, B)
    xy = torch.from_numpy(c['xy']).cuda()
    all_logits = []
    for i in range(0, xy.shape[0], B):
        chunk = xy[i:i + B]
        per = torch.stack([one.predict(scene.map_xy(chunk, s))[0].clone() for s in range(8)])
        want, want_pred = torch.empty_like(per[0]), torch.empty(per.shape[1], dtype=torch.int32, device='cuda')
        lib.logits_mean(per.contiguous(), want, want_pred)
        logits, pred = ev.predict(chunk)
        assert torch.equal(logits, want) and torch.equal(pred, want_pred)
        all_logits.append(logits.clone())
    got = torch.cat(all_logits)
    assert_close(got, c['mean'], 1e-5, 0, 'tta mean logits')
    assert torch.equal(ev.collect_logits(c['xy']), got)
    # flips from the same atlas: the mean over its four slots
    fl = EvalEngine(hip, scene, 512, tta='flips').predict(xy)[0]
    want = c['per_variant'][0].clone()
    for l in c['per_variant'][1:4]:
        want = want + l
    assert_close(fl, want / 4.0, 1e-5, 0, 'tta flips logits')


def test_tta_confusion_and_label_map_against_the_oracle():
    from dmf.engine import EvalEngine
    c, hip, scene = _tta()
    K, safe, pred = c['K'], c['safe'].numpy(), c['pred'].numpy()
    ev = EvalEngine(hip, scene, 100, tta='d4')
    labels = np.random.default_rng(2).integers(0, K, len(pred)).astype(np.int32)
    want = np.zeros((K, K), dtype=np.int64)
    np.add.at(want, (pred[safe], labels[safe]), 1)
    assert np.array_equal(ev.confusion(c['xy'][safe], labels[safe]).cpu().numpy(), want)
    m = ev.label_map(c['xy'], c['H'], c['W']).cpu().numpy()          # written at the ORIGINAL coordinates
    assert m.shape == (c['H'], c['W'])
    assert np.array_equal(m[c['xy'][safe, 0], c['xy'][safe, 1]], pred[safe])
    lm, planes = ev.confidence_maps(c['xy'], c['H'], c['W'])
    assert np.array_equal(lm.cpu().numpy(), m) and planes.shape == (3, c['H'], c['W'])
    # the validation pass stays on the untouched scene
    xy, lab = torch.from_numpy(c['xy'][:100]).cuda(), torch.from_numpy(labels[:100]).cuda()
    plain = EvalEngine(hip, scene, 100)
    assert torch.equal(ev._predict_plain(xy)[0], plain.predict(xy)[0]) and not torch.equal(ev.predict(xy)[0], plain.predict(xy)[0])
    acc = torch.zeros(2, dtype=torch.float64, device='cuda')
    ev.valid_accum(xy, lab, acc[0:1]); plain.valid_accum(xy, lab, acc[1:2])
    assert acc[0].item() == acc[1].item() > 0


def test_tta_refusals():
    from dmf import lib
    from dmf.engine import EvalEngine, Scene
    c, hip, scene = _tta()
    plain = Scene(c['A'].numpy(), c['Bm'].numpy(), 'cuda:0')
    with pytest.raises(lib.DmfError, match='scene atlas'):
        EvalEngine(hip, plain, 64, tta='d4')
    flips = Scene(c['A'].numpy(), c['Bm'].numpy(), 'cuda:0').atlas(c['P'], c['S'], 'flips')
    with pytest.raises(lib.DmfError, match='scene atlas'):
        EvalEngine(hip, flips, 64, tta='d4')
    assert EvalEngine(hip, plain, 64, tta='none').tta_slots is None
    ev = EvalEngine(hip, scene, 64, tta='d4')
    with pytest.raises(lib.DmfError, match='outside the padded scene'):
        ev.label_map(np.array([[c['H'], 0]], dtype=np.int32), c['H'] + 1, c['W'])
    with pytest.raises(lib.DmfError, match='outside the padded scene'):
        ev.confusion(np.array([[0, -1]], dtype=np.int32), np.array([1], dtype=np.int32))


# ---------------------------------------------------------------------------------------------- 7. the solver
EPOCHS = 3


def _cfg(golden_dir, tmp, **over):
    from dmf import synth
    from test_gpu_trajectory import _setup
    keys = {k: over.pop(k) for k in ('augment', 'tta', 'epoch_block') if k in over}
    _, cfg = _setup(golden_dir, tmp, **dict(dict(epoch=EPOCHS, scale=1, batchsize=32, test_batchsize=64, color_batchsize=40,
                                                 train_rate=0.3, verify_rate=0.1, steps_per_graph=-1, seed=SEED), **over))
    primary, aux, label = synth.make_scene(24, 20, 8, 1, 1, n_classes=4, seed=3)
    d = cfg['data_address']
    np.save(d + 'ms4.tif.npy', primary); np.save(d + 'pan.tif.npy', aux); np.save(d + 'label.npy', label)
    cfg['DATA_DICT'][cfg['data_city']]['size'] = [24, 20, 8]
    cfg['train'] = dict(cfg['train'], save_every=3, epoch_block=keys.get('epoch_block', 1))
    cfg['test']['full'] = 1
    cfg['color']['index'] = 1
    if 'augment' in keys:
        cfg['schedule']['augment'] = keys['augment']
    if 'tta' in keys:
        cfg['test']['tta'] = keys['tta']
    return cfg


def _read(path):
    with open(path, 'rb') as f:
        return f.read()


def _artefacts(s, out):
    s.test()
    s.color()
    return dict(matrix=s.test_matrix.copy(), png=[_read(out + '0_pic_%d.png' % k) for k in (1, 2)])


@functools.lru_cache(maxsize=None)
def _train(golden_dir, key):
    """`Solver.train()` on the 24 x 20 synthetic scene (the net of tiny1), once per route."""
    from dmf.engine import AtlasScene
    from solver.mainsolver import Solver
    over = dict(dict(native=dict(augment='d4'), graphs=dict(augment='d4', steps_per_graph=2), block=dict(augment='d4', epoch_block=3),
                     dropin=dict(augment='d4', fast_path=0), none=dict(augment='none'), absent={})[key])
    tmp = tempfile.mkdtemp(prefix='dmf_aug_')
    try:
        cfg = _cfg(golden_dir, tmp, **over)
        torch.manual_seed(3407)
        s = Solver(cfg)
        if cfg.get('fast_path', 1):
            assert isinstance(s.scene, AtlasScene) == (key in ('native', 'graphs', 'block'))
        s.dataloader()
        s.train()
        out = cfg['RESULT_output']
        r = dict(losses=np.array(s.step_losses, dtype=np.float64), n_train=len(s.train_index_loader.dataset),
                 best=torch.load(out + '0_weights.pth', map_location='cpu', weights_only=True),
                 cur=torch.load(out + '0_curweights.pth', map_location='cpu', weights_only=True),
                 files={n: _read(out + n) for n in ('0_weights.pth', '0_curweights.pth')})
        if key == 'native':
            r.update(_artefacts(s, out))                            # tta: none, the atlas resident
        return r
    finally:
        shutil.rmtree(tmp)


def test_augmented_training_is_the_same_from_every_fast_route(golden_dir):
    from test_gpu_epoch_block import _same
    native, graphs, block = (_train(golden_dir, k) for k in ('native', 'graphs', 'block'))
    n_full, rest = divmod(native['n_train'], 32)
    assert n_full >= 2 and rest > 0                                 # full batches and a short one: both mapped
    assert len(native['losses']) == EPOCHS * (n_full + 1) and np.isfinite(native['losses']).all()
    for other in (graphs, block):
        assert native['losses'].tobytes() == other['losses'].tobytes()
        _same(native['best'], other['best'], 'weights')
        _same(native['cur'], other['cur'], 'curweights')
    # augmentation does something: the unaugmented run's losses differ from the first epoch's second step on
    plain = _train(golden_dir, 'absent')
    assert plain['losses'][0] != native['losses'][0] and len(plain['losses']) == len(native['losses'])


def test_the_drop_in_path_trains_on_the_same_patches(golden_dir):
    fast, dropin = _train(golden_dir, 'native'), _train(golden_dir, 'dropin')
    assert fast['losses'].shape == dropin['losses'].shape
    diff = np.abs(fast['losses'] - dropin['losses']).max()
    print('augment d4: fast vs drop-in step losses, max |diff| %.2e over %d steps' % (diff, len(fast['losses'])))
    assert diff < 1e-5                                              # tests/test_gpu_trajectory.py holds each path to 1e-5 of the reference


def test_augment_none_is_a_run_without_the_key(golden_dir):
    none, absent = _train(golden_dir, 'none'), _train(golden_dir, 'absent')
    assert none['losses'].tobytes() == absent['losses'].tobytes()
    from test_gpu_epoch_block import _same
    _same(none['best'], absent['best'], 'weights')


def test_test_and_color_with_and_without_tta_on_an_augmented_model(golden_dir):
    """`test.tta: flips` writes its files; with `tta: none` the confusion matrix and the PNGs of the model trained with
    augmentation are the same bytes whether the atlas is resident (the training run itself) or not (a plain scene)."""
    from dmf.engine import AtlasScene
    from solver.mainsolver import Solver
    trained = _train(golden_dir, 'native')
    for keys in (dict(), dict(tta='flips')):
        tmp = tempfile.mkdtemp(prefix='dmf_aug_')
        try:
            cfg = _cfg(golden_dir, tmp, **keys)
            out = cfg['RESULT_output']
            for n, data in trained['files'].items():
                with open(out + n, 'wb') as f:
                    f.write(data)
            torch.manual_seed(3407)
            s = Solver(cfg)
            assert isinstance(s.scene, AtlasScene) == bool(keys)
            s.dataloader()
            got = _artefacts(s, out)
            assert got['matrix'].sum() == trained['matrix'].sum() > 0 and all(len(p) > 0 for p in got['png'])
            assert os.path.exists(out + '0_matrix.npy')
            if not keys:
                assert np.array_equal(got['matrix'], trained['matrix']) and got['png'] == trained['png']
            else:
                assert s.eval_engine.tta_slots == [0, 1, 2, 3]
        finally:
            shutil.rmtree(tmp)
