"""GPU: every whole-set method of the evaluation engines over every kind of tail (`_ShardedEval._walk`, dmf/engine.py), next to
section 6 of tests/test_gpu_batch_walk.py and on its cases: the first 131 pixels of the smallest whole-set case (tiny1), through
engines of 64, 65, 131 and 200 pixels — tails of 3, 1 and none, and one partial chunk — for the plain net, `tta='flips'` on an
atlas scene, and the attention net.  Nothing here is compared with an oracle, so no pixel is left out of any assertion:
  * `collect_logits`, `confidence_maps`, `probability_map`, `calibration` (15 bins, beta 0.5), `label_map` and `confusion` give
    the same bits at the four sizes;
  * at size 64 they are what `predict` plus the one `lib.*` call per chunk give when composed by hand;
  * the empty pixel set gives zero maps, an empty [0, K] tensor and a zero histogram;
  * a pixel at x = H of the map, and one whose patch leaves the scene, are refused by every map-writing method;
  * `QuaEvalEngine.label_map` / `.confusion` agree between sizes 64 and 65 on quatiny."""
import functools

import numpy as np
import pytest
import torch

import parity_cases as pc
from test_gpu_batch_walk import gpu_case

pytestmark = pytest.mark.gpu

N, SIZES, BINS, BETA = 131, (64, 65, 131, 200), 15, 0.5
H, W = pc.H_SCENE, pc.W_SCENE
VARIANTS = ('plain', 'tta', 'attention')


@functools.lru_cache(maxsize=None)
def _setup(variant):
    """(make_engine(size), xy [N, 2] int32, labels [N] int32, K) of a variant."""
    from dmf.engine import EvalEngine, Scene
    c = gpu_case('tiny1', pc.WHOLE_SET, False, variant == 'attention')
    scene = Scene(c['A'].numpy(), c['Bm'].numpy(), 'cuda:0')
    kw = {}
    if variant == 'tta':
        scene, kw = scene.atlas(c['P'], c['S'], 'flips'), dict(tta='flips')
    return (lambda size: EvalEngine(c['hip'], scene, size, **kw)), c['xy'][:N].int(), c['labels'][:N].int(), c['K']


def _walkers(eng, xy, labels):
    """{name: numpy array} of everything the six methods give."""
    logits = eng.collect_logits(xy)
    again, lab = eng.collect_logits(xy, labels)
    assert torch.equal(logits, again) and torch.equal(lab.cpu(), torch.as_tensor(labels).int())
    lm, planes = eng.confidence_maps(xy, H, W, BETA)
    prob, mask = eng.probability_map(xy, H, W, BETA)
    out = dict(logits=logits, conf_label_map=lm, planes=planes, prob=prob, mask=mask, hist=eng.calibration(xy, labels, BINS, BETA),
               label_map=eng.label_map(xy, H, W), confusion=eng.confusion(xy, labels))
    return {k: v.cpu().numpy() for k, v in out.items()}


def _by_hand(eng, xy, labels, K):
    """The same from `predict` and one `lib.*` call per chunk of the engine's size."""
    from dmf import lib
    dev = 'cuda:0'
    xy, labels = xy.to(dev), labels.to(dev)
    n, B = xy.shape[0], eng.B
    beta = torch.tensor([BETA], dtype=torch.float32, device=dev)
    out = dict(logits=torch.empty(n, K, device=dev), conf_label_map=torch.zeros(H, W, dtype=torch.int32, device=dev),
               planes=torch.zeros(3, H, W, device=dev), prob=torch.zeros(H, W, K, device=dev),
               mask=torch.zeros(H, W, dtype=torch.uint8, device=dev), hist=torch.zeros(BINS, 3, dtype=torch.int64, device=dev),
               label_map=torch.zeros(H, W, dtype=torch.int32, device=dev), confusion=torch.zeros(K, K, dtype=torch.int64, device=dev))
    for i in range(0, n, B):
        part, lab = xy[i:i + B], labels[i:i + B]
        logits, pred = eng.predict(part)                  # (views, valid until the next call)
        out['logits'][i:i + B].copy_(logits)
        p = out['planes']
        lib.softmax_stats(logits, pred=out['conf_label_map'], conf=p[0], margin=p[1], entropy=p[2], inv_temp=beta, xy=part, W=W)
        lib.prob_scatter(logits, part, W, out['prob'], out['mask'], inv_temp=beta)
        conf, cls = torch.empty(part.shape[0], device=dev), torch.empty(part.shape[0], dtype=torch.int32, device=dev)
        lib.softmax_stats(logits, pred=cls, conf=conf, inv_temp=beta)
        lib.calib_accum(conf, cls, lab, K, out['hist'])
        lib.labelmap_write(pred, part, W, out['label_map'])
        lib.confusion_accum(pred, lab, K, out['confusion'])
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same(a, b, what):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), '%s: %s' % (what, k)


@pytest.mark.parametrize('variant', VARIANTS)
def test_every_walker_is_the_same_at_every_engine_size_and_the_hand_composition(variant):
    make, xy, labels, K = _setup(variant)
    runs = [_walkers(make(size), xy, labels) for size in SIZES]
    for size, r in zip(SIZES[1:], runs[1:]):
        _same(runs[0], r, '%s: engines of %d and %d pixels' % (variant, SIZES[0], size))
    _same(runs[0], _by_hand(make(SIZES[0]), xy, labels, K), '%s: by hand' % variant)
    # every pixel counts, once: the maps are written at the N pixels and nowhere else
    r = runs[0]
    x, y = xy[:, 0].long().numpy(), xy[:, 1].long().numpy()
    assert r['mask'].sum() == N == r['confusion'].sum() == r['hist'][:, 0].sum() and (r['mask'][x, y] == 1).all()
    assert np.array_equal(r['label_map'], r['conf_label_map']) and np.array_equal(r['label_map'][x, y], r['logits'].argmax(1))
    assert (r['planes'][0][r['mask'] == 0] == 0).all() and (r['planes'][0][x, y] > 0).all()
    assert r['prob'][x, y].argmax(1).tolist() == r['logits'].argmax(1).tolist() and len(set(r['label_map'][x, y].tolist())) >= 2


@pytest.mark.parametrize('variant', VARIANTS)
def test_the_empty_set_and_the_refusals(variant):
    from dmf import lib
    make, xy, labels, K = _setup(variant)
    eng = make(64)
    r = _walkers(eng, torch.zeros(0, 2, dtype=torch.int32), torch.zeros(0, dtype=torch.int32))
    assert r['logits'].shape == (0, K) and r['hist'].shape == (BINS, 3) and r['prob'].shape == (H, W, K)
    assert all(not v.any() for v in r.values())
    inside = xy[:3].clone()
    at_h = torch.cat([inside, torch.tensor([[20, 5]], dtype=torch.int32)])           # x = H of a 20-row map; inside the scene
    past = torch.cat([inside, torch.tensor([[H, 0]], dtype=torch.int32)])            # its patch leaves the padded scene
    for name, call in (('label map', lambda p, h: eng.label_map(p, h, W)), ('label map', lambda p, h: eng.confidence_maps(p, h, W, BETA)),
                       ('probability map', lambda p, h: eng.probability_map(p, h, W, BETA))):
        with pytest.raises(lib.DmfError, match=r'pixel outside the 20 x %d %s' % (W, name)):
            call(at_h, 20)
        with pytest.raises(lib.DmfError, match='patch window outside the padded scene'):
            call(past, H + 1)
    y_w = torch.tensor([[0, W]], dtype=torch.int32)
    with pytest.raises(lib.DmfError, match='outside the'):
        eng.label_map(y_w, H, W)


def test_stage2_label_map_and_confusion_at_a_tail_of_one_and_of_three():
    from dmf.engine import QuaEvalEngine, QuaScene
    from model.gmfnet import Net as HipNet
    q = pc.qua_eval_case()
    hip = HipNet(q['cfg'])
    hip.load_state_dict(q['state'])
    hip = hip.to('cuda:0')
    scene = QuaScene(q['scenes'], 'cuda:0')
    xy, labels = q['xy'][:N].int(), q['labels'][:N].int()
    a, b = (QuaEvalEngine(hip, scene, size) for size in (64, 65))
    maps = [e.label_map(xy, H, W).cpu() for e in (a, b)]
    mats = [e.confusion(xy, labels).cpu() for e in (a, b)]
    assert torch.equal(maps[0], maps[1]) and torch.equal(mats[0], mats[1])
    assert int(mats[0].sum()) == N and int((maps[0] != 0).sum()) <= N
    pred = a.predict(xy[:64].cuda())[1].cpu()
    assert torch.equal(maps[0][xy[:64, 0].long(), xy[:64, 1].long()], pred)
    assert not a.label_map(torch.zeros(0, 2, dtype=torch.int32), H, W).any()
