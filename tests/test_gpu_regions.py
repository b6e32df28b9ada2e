"""GPU: connected superpixels — dmf_label_components, dmf_region_merge and dmf_region_vote against the integer
reference of tests/regions_ref.py on the cases of tests/regions_cases.py (whose guards are CPU tests in
tests/test_regions_host.py), Scene.segment_regions / EvalEngine.region_vote end to end, and the solver keys on the 40 x 40 x 8,
4-class scene of tests/test_gpu_calibration.py.

Everything is integer arithmetic, so every comparison is equality: comp, region, region_size, stats, regcount, the majority counts,
the bits of the mean vote's regprob, and the labels at every pixel (no tie set).  Every output of a kernel call sits between guard
words that must stay as they were, and every call is made twice over workspaces and outputs that held different bytes.

Observed on an MI355X (printed by the tests): all 267 label images equal (148,702 components, 64,317 absorbed, the
chain of 4,095 among them); the vote bit-equal at every K in both modes; on the solver's scene 256 components, 187 absorbed, 69
regions of 3 to 62 pixels, and the drop-in path's region image and voted maps equal the fast path's at all 1,600 pixels."""
import functools
import json
import os
import shutil
import tempfile

import numpy as np
import pytest
import torch
from PIL import Image

import regions_cases as RC
import regions_ref as R

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
GUARD = 64                                               # guard elements on either side of an output


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                 # (a copy: the cases are read-only arrays)


class Guarded:
    """A contiguous device tensor of `shape` inside a larger allocation whose other elements hold a pattern."""

    def __init__(self, shape, dtype, fill):
        n = int(np.prod(shape))
        self.pattern = 85 if dtype == torch.uint8 else -12345
        self.whole = torch.full((n + 2 * GUARD,), self.pattern, dtype=dtype, device=DEV)
        self.t = self.whole[GUARD:GUARD + n].view(*shape)
        self.t.fill_(fill)
        self.n = n

    def intact(self):
        return bool((self.whole[:GUARD] == self.pattern).all() and (self.whole[GUARD + self.n:] == self.pattern).all())


def _regions_gpu(labels, n_labels, min_size, fill):
    """-> (comp, region, region_size [H W], stats [4]) as numpy; `fill` is what the outputs and the workspace held before."""
    from dmf import lib
    H, W = labels.shape
    comp, region = Guarded((H, W), torch.int32, fill), Guarded((H, W), torch.int32, fill)
    sizes, stats = Guarded((H * W,), torch.int32, fill), Guarded((4,), torch.int32, fill)
    ws = Guarded((lib.region_workspace_bytes(H, W, n_labels),), torch.uint8, fill % 251)
    lib.label_components(labels, comp.t, ws.t)
    lib.region_merge(labels, comp.t, n_labels, min_size, region.t, sizes.t, stats.t, ws.t)
    torch.cuda.synchronize()
    assert comp.intact() and region.intact() and sizes.intact() and stats.intact() and ws.intact()
    return comp.t.cpu().numpy(), region.t.cpu().numpy(), sizes.t.cpu().numpy(), stats.t.cpu().numpy()


def _check_case(case):
    name, H, W, n_labels, min_size = case
    labels = _dev(RC.labels_of(name, H, W))
    w_comp, w_region, w_sizes, w_stats, _ = RC.reference(*case)
    got = _regions_gpu(labels, n_labels, min_size, -7)
    comp, region, sizes, stats = got
    assert np.array_equal(comp, w_comp), case
    assert tuple(stats) == tuple(w_stats) + (0,), (case, stats, w_stats)
    Rn = w_stats[0]
    assert np.array_equal(region, w_region), case
    assert np.array_equal(sizes[:Rn], w_sizes) and not sizes[Rn:].any() and sizes.sum() == H * W, case
    again = _regions_gpu(labels, n_labels, min_size, 93)
    assert all(np.array_equal(a, b) for a, b in zip(got, again)), case            # two calls: the same bits
    return w_stats


# ------------------------------------------------------------------------------------------------ components, merge
@pytest.mark.parametrize('size', RC.SIZES, ids=lambda s: '%dx%d' % s)
def test_components_and_regions_equal_the_reference(size):
    cases = [c for c in RC.LABEL_CASES if (c[1], c[2]) == size]
    assert len(cases) == len(RC.PATTERNS) * len(RC.MERGES) + 2 * len(RC.SLIC_S)
    comps = absorbed = 0
    for case in cases:
        stats = _check_case(case)
        comps, absorbed = comps + stats[1], absorbed + stats[2]
    print('%d x %d: %d cases, %d components, %d absorbed, all equal' % (size + (len(cases), comps, absorbed)))


def test_a_chain_of_4095_fragments_ends_at_pixel_0():
    case = ('alternate',) + RC.CHAIN + (0, 2)
    assert case in RC.LABEL_CASES
    stats = _check_case(case)
    assert stats == (1, 4096, 4095)


def test_the_scan_of_the_block_totals_carries_past_256_blocks():
    """513 x 512 one-pixel components are 257 scan blocks: the one-workgroup scan goes round twice, and at min_size 1 the dense
    ids cross its carry; at min_size 2 all but pixel 0 are absorbed along chains of up to 1,023."""
    H, W = RC.CARRY
    assert (H * W + 1023) // 1024 == 257 and [c[3:] for c in RC.CARRY_CASES] == [(0, 1), (0, 2)]
    for case in RC.CARRY_CASES:
        want, depth = RC.CARRY_STATS[case[4]]
        assert RC.reference(*case)[3:] == (want, depth), case
        assert _check_case(case) == want


# ------------------------------------------------------------------------------------------------ vote
def _vote_gpu(prob, mask, region, Rn, mode, fill, with_out=True):
    from dmf import lib
    H, W, K = prob.shape
    regprob, regcount = Guarded((Rn, K), torch.float32, float(fill)), Guarded((Rn,), torch.int32, fill)
    label = Guarded((H, W), torch.int32, 0)
    out = Guarded((H, W, K), torch.float32, float(fill)) if with_out else None
    ws = Guarded((lib.region_vote_workspace_bytes(Rn, K),), torch.uint8, fill % 251)
    lib.region_vote(prob, mask, region, Rn, mode, regprob.t, regcount.t, label.t, ws.t, out.t if with_out else None)
    torch.cuda.synchronize()
    assert regprob.intact() and regcount.intact() and label.intact() and ws.intact() and (out is None or out.intact())
    return regprob.t.cpu().numpy(), regcount.t.cpu().numpy(), label.t.cpu().numpy(), out.t.cpu().numpy() if with_out else None


@pytest.mark.parametrize('mode', ['mean', 'majority'])
@pytest.mark.parametrize('K', RC.VOTE_K)
def test_vote_equals_the_integer_reference(K, mode):
    for H, W, k in RC.VOTE_CASES:
        if k != K:
            continue
        prob, mask, region, Rn = RC.vote_inputs(H, W, K)
        w_prob, w_count, w_label, w_rows, _, orphan = RC.vote_reference(H, W, K, mode)
        assert not orphan.any()
        dirty = np.array(prob)
        dirty[mask == 0] = np.nan                        # a NaN in every mask-0 row reaches nothing
        got = _vote_gpu(_dev(dirty), _dev(mask), _dev(region), Rn, mode, -7)
        regprob, regcount, label, out = got
        assert np.array_equal(regcount, w_count), (H, W, K, mode)
        assert regprob.tobytes() == w_prob.tobytes(), (H, W, K, mode, float(np.abs(regprob - w_prob).max()))      # bit-equal
        assert np.array_equal(label, w_label), (H, W, K, mode, int((label != w_label).sum()))      # every pixel: no tie set
        assert out.reshape(-1, K).tobytes() == w_rows.tobytes(), (H, W, K, mode)
        again = _vote_gpu(_dev(dirty), _dev(mask), _dev(region), Rn, mode, 93, with_out=False)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got[:3], again[:3]))
    print('K = %d, %s: regprob bit-equal, labels equal at every pixel' % (K, mode))


@pytest.mark.parametrize('mode', ['mean', 'majority'])
def test_one_region_that_is_the_whole_scene(mode):
    H, W, K = 64, 65, 17
    prob, mask, _, _ = RC.vote_inputs(H, W, K)
    region = np.zeros((H, W), dtype=np.int32)
    w_prob, w_count, w_label, _, _, _ = R.vote(prob, mask, region, 1, mode)
    regprob, regcount, label, _ = _vote_gpu(_dev(prob), _dev(mask), _dev(region), 1, mode, -7)
    assert regcount[0] == w_count[0] == int(mask.sum()) and regprob.tobytes() == w_prob.tobytes() and np.array_equal(label, w_label)


@pytest.mark.parametrize('mode', ['mean', 'majority'])
def test_out_of_range_region_ids_stand_for_themselves(mode):
    H, W, K = 33, 17, 3
    prob, mask, region, Rn = RC.vote_inputs(H, W, K)
    odd = np.array(region)
    odd[0, 0], odd[5, 3], odd[32, 16], odd[7, 7] = -1, Rn, 2 ** 31 - 1, -2 ** 31
    mask = np.array(mask)
    mask[0, 0] = mask[5, 3] = mask[32, 16] = 1
    w_prob, w_count, w_label, w_rows, _, orphan = R.vote(prob, mask, odd, Rn, mode)
    assert orphan.sum() == 3 + int(mask[7, 7])
    regprob, regcount, label, out = _vote_gpu(_dev(prob), _dev(mask), _dev(odd), Rn, mode, -7)
    assert np.array_equal(regcount, w_count) and regprob.tobytes() == w_prob.tobytes() and np.array_equal(label, w_label)
    assert out.reshape(-1, K).tobytes() == w_rows.tobytes()
    assert np.array_equal(label[orphan], prob[orphan].argmax(1))
    # and change nothing else: the rows of the regions that lost no pixel are those of the untouched image
    plain = R.vote(prob, mask, region, Rn, mode)[0]
    lost = np.unique(region[odd != region])
    keep = np.setdiff1d(np.arange(Rn), lost)
    assert np.array_equal(regprob[keep], plain[keep])


# ------------------------------------------------------------------------------------------------ the engine, end to end
@pytest.mark.parametrize('half', [False, True], ids=['fp32', 'fp16'])
def test_regions_and_vote_through_the_engine(half):
    """The 13 x 9 tiny1 scene (as a d4 atlas: slot 0 is the scene), all 117 pixels in chunks of 50."""
    from dmf import lib
    from dmf.engine import EvalEngine
    from test_gpu_augment import H, W, _case
    c = _case('tiny1', half, False)
    scene, S = c['scene'], 4
    ev = EvalEngine(c['hip'], scene, 50)
    prob, mask = ev.probability_map(c['xy'], H, W, inv_temp=0.5)
    seg = scene.segments(H, W, S, 0.05, 3)[0]
    gh, gw = lib.segment_grid(H, W, S)
    for min_size in (1, S * S // 4):
        region, Rn, sizes, stats = scene.segment_regions(seg, H, W, gh * gw, min_size)
        _, w_region, w_sizes, w_stats, _ = R.regions(seg.cpu().numpy(), gh * gw, min_size)
        assert (Rn, stats) == (w_stats[0], dict(regions=w_stats[0], components=w_stats[1], absorbed=w_stats[2]))
        assert region.dtype == torch.int32 and np.array_equal(region.cpu().numpy(), w_region) and np.array_equal(sizes.cpu().numpy(), w_sizes)
        for mode in ('mean', 'majority'):
            regprob, regcount, label = ev.region_vote(prob, mask, region, Rn, mode)
            w_prob, w_count, w_label, _, _, orphan = R.vote(prob.cpu().numpy(), mask.cpu().numpy(), w_region, Rn, mode)
            assert not orphan.any() and np.array_equal(regcount.cpu().numpy(), w_count) and label.dtype == torch.int32
            assert regprob.cpu().numpy().tobytes() == w_prob.tobytes() and np.array_equal(label.cpu().numpy(), w_label)
    # a partial set: label 0 where mask is 0
    some = c['xy'][::3]
    p2, m2 = ev.probability_map(some, H, W)
    l2 = ev.region_vote(p2, m2, region, Rn, 'mean')[2]
    off = m2.cpu().numpy() == 0
    assert off.sum() == 117 - len(some) and (l2.cpu().numpy()[off] == 0).all()


# ------------------------------------------------------------------------------------------------ the solver
SEED = 3407
BASE = {'test': dict(calibration=1, calibration_bins=15, temperature=1.5, spatial='bilateral', segments='slic', segment_size=5,
                     segment_compactness=0.05, segment_iterations=3, segment_vote='majority'), 'color': dict(spatial=1, segments=1)}
KEYS_ON = {'test': dict(segment_connectivity=1)}         # min_size auto: max(1, 25 div 4) = 6
NET = 'plain_native_loop'


def _read(path):
    with open(path, 'rb') as f:
        return f.read()


def _again(cfg, **test_keys):
    """test() and color() of a fresh solver on the weights the run saved, with other test keys."""
    from solver.mainsolver import Solver
    cfg = dict(cfg, test=dict(cfg['test'], **test_keys))
    torch.manual_seed(SEED)
    d = Solver(cfg)
    d.dataloader()
    d.test()
    d.color()
    return d


@functools.lru_cache(maxsize=None)
def _run(keys, golden_dir):
    """Two epochs of Solver.train() on the epoch-block scene with the calibration, the spatial filter and the SLIC vote on, then
    test() and color(); with `keys` (test.segment_connectivity: 1) also the engine's own regions and voted map, the same test() /
    color() by a drop-in solver (fast_path: 0) on the weights this run saved, and a min_size 1 run with a `file` run on its image."""
    from solver.mainsolver import Solver
    from test_gpu_epoch_block import _cfg
    tmp = tempfile.mkdtemp(prefix='dmf_regions_')
    try:
        cfg = _cfg(golden_dir, tmp, NET, 1)
        cfg['epoch'] = 2
        for sec, val in list(BASE.items()) + (list(KEYS_ON.items()) if keys else []):
            cfg[sec] = dict(cfg[sec], **val)
        torch.manual_seed(SEED)
        s = Solver(cfg)
        s.dataloader()
        s.train()
        s.test()
        s.color()
        out = cfg['RESULT_output']
        r = dict(matrix=s.test_matrix.copy(), result=list(s.result[:3]), png=[_read(out + '0_pic_%d.png' % k) for k in (1, 2)],
                 calibration=_read(out + '0_calibration.json'), spatial=_read(out + '0_spatial.json'), files=sorted(os.listdir(out)),
                 segments=s.segments, json=json.load(open(out + '0_segments.json')), npy=np.load(out + '0_segments.npy'),
                 segment_maps=s.segment_maps, segments_png=[np.asarray(Image.open(out + '0_pic_%d_segments.png' % k)) for k in (1, 2)])
        if not keys:
            return r
        r['lut'] = np.asarray(cfg['DATA_DICT'][cfg['data_city']]['color'], dtype=np.uint8)
        # the engine's own pass over the whole scene
        xy = torch.from_numpy(s._scene_pixels())
        prob, mask = s.eval_engine.probability_map(xy, 40, 40, s._beta(1.5))
        seg = s.scene.segments(40, 40, 5, 0.05, 3)[0]
        region, Rn, sizes, stats = s.scene.segment_regions(seg, 40, 40, 64, 6)
        label = s.eval_engine.region_vote(prob, mask, region, Rn, 'majority')[2]
        test_rows = np.asarray(s.test_index_loader.dataset.indices)
        r.update(engine_label=label.cpu().numpy(), engine_region=region.cpu().numpy(), engine_seg=seg.cpu().numpy(), engine_stats=stats,
                 engine_sizes=sizes.cpu().numpy(), test_xy=s._set_pixels(test_rows), test_lab=s.index_dataset.label[test_rows].astype(np.int64))
        d = _again(dict(cfg, fast_path=0, train=dict(cfg['train'], index=0)))
        r.update(dropin=d.segments, dropin_maps=d.segment_maps, dropin_region=d.segment_image)
        one = _again(cfg, segment_min_size=1)
        np.save(os.path.join(tmp, 'parcels.npy'), one.segment_image.astype(np.int64))
        f = _again(cfg, segments='file', segment_file=os.path.join(tmp, 'parcels.npy'), segment_connectivity=0, segment_min_size='auto')
        r.update(one=one.segments, one_region=one.segment_image, one_maps=one.segment_maps, file=f.segments, file_region=f.segment_image,
                 file_maps=f.segment_maps)
        with pytest.raises(ValueError, match=r'test\.segment_file .* has shape \[40, 39\], the scene is \[40, 40\]'):
            np.save(os.path.join(tmp, 'short.npy'), one.segment_image[:, :39])
            _again(cfg, segments='file', segment_file=os.path.join(tmp, 'short.npy'))
        return r
    finally:
        shutil.rmtree(tmp)


def test_the_keys_change_nothing_that_was_there(golden_dir):
    on, off = _run(True, golden_dir), _run(False, golden_dir)
    assert off['matrix'].sum() > 0 and np.array_equal(on['matrix'], off['matrix']) and on['result'] == off['result']
    assert on['png'] == off['png'] and len(on['png'][0]) > 0 and on['calibration'] == off['calibration'] and len(on['calibration']) > 0
    assert on['spatial'] == off['spatial'] and len(on['spatial']) > 0 and on['files'] == off['files']
    # with the new keys off the block is the one it was: `not enforced`, none of the new fields
    assert off['segments']['connectivity'] == 'not enforced' and not {'min_size', 'components', 'absorbed', 'regions', 'region_pixels'} & set(off['json'])
    assert np.array_equal(off['npy'], on['engine_seg'])                              # (the segment image; with the keys on: the regions)


def test_the_regions_block_and_maps(golden_dir):
    r = _run(True, golden_dir)
    b = r['segments']
    assert r['json'] == json.loads(json.dumps(b))
    st = r['engine_stats']
    assert b['connectivity'] == 'enforced' and b['min_size'] == 6
    assert (b['components'], b['absorbed'], b['regions']) == (st['components'], st['absorbed'], st['regions']) and st['regions'] == len(r['engine_sizes'])
    assert b['region_pixels'] == dict(min=int(r['engine_sizes'].min()), mean=float(r['engine_sizes'].mean()), max=int(r['engine_sizes'].max()))
    assert r['engine_sizes'].sum() == 1600 and b['Kc'] == 64 and b['vote'] == 'majority'
    w = R.regions(r['engine_seg'], 64, 6)
    assert np.array_equal(r['engine_region'], w[1]) and st['regions'] == w[3][0]
    assert r['npy'].dtype == np.int32 and np.array_equal(r['npy'], r['engine_region'])
    m = np.array(b['matrix'])
    x, y = r['test_xy'][:, 0], r['test_xy'][:, 1]
    want = np.zeros_like(m)
    np.add.at(want, (r['engine_label'][x, y], r['test_lab']), 1)
    assert np.array_equal(m, want) and m.sum() == r['matrix'].sum() == b['n']
    assert np.array_equal(r['segment_maps'][1], r['engine_label']) and np.array_equal(r['segments_png'][1], r['lut'][r['engine_label']])
    print('%d components, %d absorbed, %d regions of %d..%d pixels; OA %.4f -> %.4f'
          % (b['components'], b['absorbed'], b['regions'], b['region_pixels']['min'], b['region_pixels']['max'], b['before']['OA'], b['after']['OA']))


def test_the_drop_in_path_gives_the_same_regions_and_maps(golden_dir):
    r = _run(True, golden_dir)
    differ = int((r['dropin_region'] != r['engine_region']).sum())
    maps = [int((a != b).sum()) for a, b in zip(r['dropin_maps'], r['segment_maps'])]
    print('the drop-in path: region image differs at %d of 1600 pixels, the voted maps at %s' % (differ, maps))
    assert differ == 0 and maps == [0, 0]
    assert (r['dropin']['components'], r['dropin']['absorbed'], r['dropin']['regions']) == (r['segments']['components'], r['segments']['absorbed'], r['segments']['regions'])
    assert r['dropin']['matrix'] == r['segments']['matrix']


def test_file_mode_reproduces_the_regions_it_was_given(golden_dir):
    r = _run(True, golden_dir)
    assert r['one']['absorbed'] == 0 and r['one']['regions'] == r['one']['components'] == r['segments']['components'] and r['one']['min_size'] == 1
    assert np.array_equal(r['file_region'], r['one_region'])
    f = r['file']
    assert f['kind'] == 'file' and f['connectivity'] == 'enforced' and f['min_size'] == 1 and f['absorbed'] == 0
    assert f['regions'] == f['components'] == r['one']['regions'] and f['region_pixels'] == r['one']['region_pixels']
    assert f['matrix'] == r['one']['matrix'] and all(np.array_equal(a, b) for a, b in zip(r['file_maps'], r['one_maps']))
