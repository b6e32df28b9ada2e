"""GPU: the spectrum-aware fragment merge — dmf_region_graph_count and dmf_region_graph_merge against the reference
of tests/region_graph_ref.py on the cases of tests/region_graph_cases.py (whose guards are CPU tests in
tests/test_region_graph_host.py), Scene.segment_regions(merge='spectrum') end to end, and the key test.segment_merge on the
40 x 40 x 8, 4-class scene of tests/test_gpu_regions.py.

The sums are integers and every double operation is stated, so every comparison is equality: region, region_size and the four
statistics.  Every output and workspace sits between guard words that must stay as they were, and every call is made twice over
workspaces and outputs that held different bytes.  The device's scene is wider and taller than [H, W] (a pitch above W).

Observed on an MI355X (printed by the tests): all 1,680 cases equal (at 129 x 131 on the 8-band scene 84,292
components over the 30 label images, 38,700 absorbed, at most 3 rounds; on the constant scene 44,725 ties there); the chain of 4,095
one region in one round; on the solver's scene 256 components become 71 regions in 2 rounds (position: 69), and the drop-in path's
region image and voted maps equal the fast path's at all 1,600 pixels.  71 tests in 24 s, the slowest 3.2 s."""
import functools
import json
import os
import shutil
import tempfile

import numpy as np
import pytest
import torch
from PIL import Image

import region_graph_cases as GC
import region_graph_ref as G
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


@functools.lru_cache(maxsize=None)
def _labels_and_comp(name, H, W):
    """The label image and what dmf_label_components leaves for it, on the device (asserted against the reference once)."""
    from dmf import lib
    labels = _dev(RC.labels_of(name, H, W))
    comp = torch.empty_like(labels)
    ws = torch.empty(lib.region_workspace_bytes(H, W, 0), dtype=torch.uint8, device=DEV)
    lib.label_components(labels, comp, ws)
    assert np.array_equal(comp.cpu().numpy(), RC.components(name, H, W))
    return labels, comp


def _graph_gpu(labels, comp, scene, n_labels, min_size, fill, given=None):
    """-> (region, region_size [H W], stats [4], (components, fragments)) as numpy; `fill` is what the outputs and the workspaces
    held before.  `given`: the (components, fragments) to hand to the merge in place of the count's."""
    from dmf import lib
    H, W = labels.shape
    counts = Guarded((2,), torch.int32, fill)
    cws = Guarded((lib.region_graph_workspace_bytes(H, W, 1, n_labels, 1),), torch.uint8, fill % 251)
    lib.region_graph_count(labels, comp, n_labels, min_size, counts.t, cws.t)
    components, fragments = given or counts.t.tolist()
    region, sizes, stats = Guarded((H, W), torch.int32, fill), Guarded((H * W,), torch.int32, fill), Guarded((4,), torch.int32, fill)
    ws = Guarded((lib.region_graph_workspace_bytes(H, W, scene.shape[2], n_labels, components),), torch.uint8, fill % 251)
    lib.region_graph_merge(labels, comp, scene, n_labels, min_size, components, fragments, region.t, sizes.t, stats.t, ws.t)
    torch.cuda.synchronize()
    assert counts.intact() and cws.intact() and region.intact() and sizes.intact() and stats.intact() and ws.intact()
    return region.t.cpu().numpy(), sizes.t.cpu().numpy(), stats.t.cpu().numpy(), tuple(counts.t.tolist())


def _check_case(case, kind, C, scene):
    name, H, W, n_labels, min_size = case
    labels, comp = _labels_and_comp(name, H, W)
    w_region, w_sizes, w_stats, info = GC.reference(*case, kind, C)
    got = _graph_gpu(labels, comp, scene, n_labels, min_size, -7)
    region, sizes, stats, counts = got
    assert counts == (w_stats[1], info['fragments']), (case, kind, C, counts)
    assert tuple(stats) == tuple(w_stats), (case, kind, C, stats, w_stats)
    assert np.array_equal(region, w_region), (case, kind, C, int((region != w_region).sum()))
    Rn = w_stats[0]
    assert np.array_equal(sizes[:Rn], w_sizes) and not sizes[Rn:].any() and sizes.sum() == H * W, (case, kind, C)
    again = _graph_gpu(labels, comp, scene, n_labels, min_size, 93)
    assert all(np.array_equal(a, b) for a, b in zip(got[:3], again[:3])) and got[3] == again[3], (case, kind, C)      # two calls: the same bits
    return w_stats, info


# ------------------------------------------------------------------------------------------------ parity against the reference
@pytest.mark.parametrize('kind,C', GC.SCENES, ids=lambda v: str(v))
@pytest.mark.parametrize('size', GC.SIZES, ids=lambda s: '%dx%d' % s)
def test_regions_equal_the_reference(size, kind, C):
    cases = [c for c in GC.LABEL_CASES if (c[1], c[2]) == size]
    assert len(cases) == len(RC.PATTERNS) * len(GC.PATTERN_MERGES) + 2 * len(RC.SLIC_S)
    scene = _dev(GC.padded(kind, C, *size))
    assert scene.shape[1] > size[1] and scene.dtype == (torch.float16 if kind == 'f16' else torch.float32)
    comps = absorbed = rounds = ties = 0
    for case in cases:
        stats, info = _check_case(case, kind, C, scene)
        comps, absorbed, rounds, ties = comps + stats[1], absorbed + stats[2], max(rounds, stats[3]), ties + info['ties']
    print('%d x %d, %s %d: %d cases, %d components, %d absorbed, at most %d rounds, %d ties, all equal'
          % (size + (kind, C, len(cases), comps, absorbed, rounds, ties)))


def test_the_alternating_row_on_the_constant_scene():
    """4,095 one-pixel fragments that all choose by id alone: one round, one long union chain, one region."""
    H, W = GC.CHAIN
    labels, comp = _labels_and_comp('alternate', H, W)
    scene = _dev(GC.padded('const', 3, H, W))
    want = G.merge(RC.labels_of('alternate', H, W), RC.components('alternate', H, W), GC.scene('const', 3, H, W), 0, 2)
    assert want[2] == (1, 4096, 4095, 1) and want[3]['ties'] > 0
    for fill in (-7, 93):
        region, sizes, stats, counts = _graph_gpu(labels, comp, scene, 0, 2, fill)
        assert counts == (4096, 4095) and tuple(stats) == want[2] and not region.any() and sizes[0] == 4096 and not sizes[1:].any()


def test_the_scan_over_the_components_carries_past_256_blocks():
    """262,656 one-pixel components on a constant scene at min_size 1: no fragment and no round, but both scans (over the pixels,
    over the components) are 257 blocks, so the one-workgroup scan of the block totals goes round twice."""
    kind, C = GC.CARRY_SCENE
    name, H, W, n_labels, min_size = GC.CARRY_CASE
    assert (H * W + 1023) // 1024 == 257 and (n_labels, min_size) == (0, 1)
    stats, info = _check_case(GC.CARRY_CASE, kind, C, _dev(GC.padded(kind, C, H, W)))
    assert stats == GC.CARRY_STATS and info['fragments'] == 0


@pytest.mark.parametrize('size', GC.SIZES, ids=lambda s: '%dx%d' % s)
def test_min_size_1_equals_the_positional_merge(size):
    from dmf import lib
    H, W = size
    scene = _dev(GC.padded('f32', 3, H, W))
    for name in RC.PATTERNS + tuple('slic%d' % S for S in RC.SLIC_S):
        n_labels = RC.kc(H, W, int(name[4:])) if name.startswith('slic') else 2
        labels, comp = _labels_and_comp(name, H, W)
        region, sizes, stats, _ = _graph_gpu(labels, comp, scene, n_labels, 1, -7)
        p_region, p_sizes, p_stats = torch.empty_like(labels), torch.empty(H * W, dtype=torch.int32, device=DEV), torch.empty(4, dtype=torch.int32, device=DEV)
        ws = torch.empty(lib.region_workspace_bytes(H, W, n_labels), dtype=torch.uint8, device=DEV)
        lib.region_merge(labels, comp, n_labels, 1, p_region, p_sizes, p_stats, ws)
        assert np.array_equal(region, p_region.cpu().numpy()) and np.array_equal(sizes, p_sizes.cpu().numpy()), (size, name)
        assert stats[:3].tolist() == p_stats[:3].tolist() and stats[3] == 0 and stats[2] == 0, (size, name)


@pytest.mark.parametrize('size', [(13, 9), (64, 65)], ids=lambda s: '%dx%d' % s)
def test_foreign_contents_of_comp_end_and_stay_in_range(size):
    """comp that dmf_label_components did not write, and counts that belong to nothing: the regions are unspecified, but every
    launch ends and the guard words around the outputs and the workspaces stay as they were."""
    H, W = size
    rng = np.random.default_rng(99)
    labels = _dev(RC.image(H, W, 'noise'))
    scene = _dev(GC.padded('f32', 3, H, W))
    wild = rng.integers(-2 ** 31, 2 ** 31, (H, W)).astype(np.int32)
    near = rng.integers(-3, H * W + 3, (H, W)).astype(np.int32)
    forward = np.minimum(np.arange(H * W) + rng.integers(0, 5, H * W), H * W - 1).reshape(H, W).astype(np.int32)     # "roots" above their pixels
    for comp in (wild, near, forward, np.full((H, W), H * W - 1, dtype=np.int32)):
        for given in (None, (1, 0), (H * W, H * W - 1), (7, 6)):
            region, sizes, stats, counts = _graph_gpu(labels, _dev(comp), scene, 2, 4, -7, given)
            assert 1 <= counts[0] <= H * W and 0 <= counts[1] < counts[0]
            assert region.min() >= 0 and region.max() < H * W and 0 <= stats[3] <= 27


# ------------------------------------------------------------------------------------------------ the engine, end to end
@pytest.mark.parametrize('half', [False, True], ids=['fp32', 'fp16'])
def test_spectrum_regions_through_the_engine(half):
    """The 13 x 9 tiny1 scene (as a d4 atlas: slot 0 is the scene)."""
    from dmf import lib
    from dmf.engine import EvalEngine
    from test_gpu_augment import H, W, _case
    c = _case('tiny1', half, False)
    scene, S = c['scene'], 4
    ev = EvalEngine(c['hip'], scene, 50)
    prob, mask = ev.probability_map(c['xy'], H, W, inv_temp=0.5)
    seg = scene.segments(H, W, S, 0.05, 3)[0]
    gh, gw = lib.segment_grid(H, W, S)
    host = scene.A[:H, :W].float().cpu().numpy()
    assert scene.A.dtype == (torch.float16 if half else torch.float32) and scene.A.shape[1] > W
    labels = seg.cpu().numpy()
    for min_size in (1, S * S // 4, 9):
        region, Rn, sizes, stats = scene.segment_regions(seg, H, W, gh * gw, min_size, merge='spectrum')
        w_region, w_sizes, w_stats, _ = G.merge(labels, R.components(labels), host, gh * gw, min_size)
        assert (Rn, stats) == (w_stats[0], dict(regions=w_stats[0], components=w_stats[1], absorbed=w_stats[2], rounds=w_stats[3]))
        assert region.dtype == torch.int32 and np.array_equal(region.cpu().numpy(), w_region) and np.array_equal(sizes.cpu().numpy(), w_sizes)
        for mode in ('mean', 'majority'):
            regprob, regcount, label = ev.region_vote(prob, mask, region, Rn, mode)
            w_prob, w_count, w_label, _, _, orphan = R.vote(prob.cpu().numpy(), mask.cpu().numpy(), w_region, Rn, mode)
            assert not orphan.any() and np.array_equal(regcount.cpu().numpy(), w_count)
            assert regprob.cpu().numpy().tobytes() == w_prob.tobytes() and np.array_equal(label.cpu().numpy(), w_label)
    # the default is the positional merge, with the statistics it had
    region, Rn, sizes, stats = scene.segment_regions(seg, H, W, gh * gw, 4)
    same = scene.segment_regions(seg, H, W, gh * gw, 4, merge='position')
    assert set(stats) == {'regions', 'components', 'absorbed'} and same[3] == stats and torch.equal(same[0], region)
    with pytest.raises(lib.DmfError, match='merge'):
        scene.segment_regions(seg, H, W, gh * gw, 4, merge='nearest')


# ------------------------------------------------------------------------------------------------ the solver
SEED = 3407
NET = 'plain_native_loop'


RESULTS = ('.png', '.npy', '_segments.json', '_calibration.json', '_spatial.json')


def _files(out):
    """name -> bytes of every file of the output folder (None for the files that are no result of test() / color()).  The result
    files are removed once read, so that the next run has to write every one of them itself."""
    found = {}
    for name in sorted(os.listdir(out)):
        path = os.path.join(out, name)
        found[name] = None
        if name.endswith(RESULTS):
            with open(path, 'rb') as f:
                found[name] = f.read()
            os.remove(path)
    return found


@functools.lru_cache(maxsize=None)
def _run(golden_dir):
    """Two epochs of Solver.train() on the solver scene of tests/test_gpu_regions.py with connected regions and
    test.segment_merge: spectrum, then test() and color(); the engine's own spectrum regions and voted map; the same test() /
    color() by a drop-in solver (fast_path: 0) on the weights this run saved; and, on those weights, a run without the key and one
    with test.segment_merge: position."""
    from solver.mainsolver import Solver
    from test_gpu_epoch_block import _cfg
    from test_gpu_regions import BASE, KEYS_ON, _again
    tmp = tempfile.mkdtemp(prefix='dmf_region_graph_')
    try:
        cfg = _cfg(golden_dir, tmp, NET, 1)
        cfg['epoch'] = 2
        for sec, val in list(BASE.items()) + list(KEYS_ON.items()):
            cfg[sec] = dict(cfg[sec], **val)
        plain_cfg = dict(cfg)
        cfg = dict(cfg, test=dict(cfg['test'], segment_merge='spectrum'))
        torch.manual_seed(SEED)
        s = Solver(cfg)
        s.dataloader()
        s.train()
        s.test()
        s.color()
        out = cfg['RESULT_output']
        r = dict(matrix=s.test_matrix.copy(), segments=s.segments, json=json.load(open(out + '0_segments.json')), npy=np.load(out + '0_segments.npy'),
                 segment_maps=s.segment_maps, segments_png=[np.asarray(Image.open(out + '0_pic_%d_segments.png' % k)) for k in (1, 2)],
                 lut=np.asarray(cfg['DATA_DICT'][cfg['data_city']]['color'], dtype=np.uint8))
        xy = torch.from_numpy(s._scene_pixels())
        prob, mask = s.eval_engine.probability_map(xy, 40, 40, s._beta(1.5))
        seg = s.scene.segments(40, 40, 5, 0.05, 3)[0]
        region, Rn, sizes, stats = s.scene.segment_regions(seg, 40, 40, 64, 6, merge='spectrum')
        label = s.eval_engine.region_vote(prob, mask, region, Rn, 'majority')[2]
        test_rows = np.asarray(s.test_index_loader.dataset.indices)
        r.update(engine_label=label.cpu().numpy(), engine_region=region.cpu().numpy(), engine_seg=seg.cpu().numpy(), engine_stats=stats,
                 engine_sizes=sizes.cpu().numpy(), test_xy=s._set_pixels(test_rows), test_lab=s.index_dataset.label[test_rows].astype(np.int64),
                 host_scene=s.scene.A[:40, :40].float().cpu().numpy())
        d = _again(dict(cfg, fast_path=0, train=dict(cfg['train'], index=0)))
        r.update(dropin=d.segments, dropin_maps=d.segment_maps, dropin_region=d.segment_image)
        _files(out)                                      # (the results so far go: each of the next two runs starts without any)
        absent = _again(plain_cfg)
        r.update(absent=absent.segments, absent_files=_files(out), absent_region=absent.segment_image)
        position = _again(plain_cfg, segment_merge='position')
        r.update(position=position.segments, position_files=_files(out))
        with pytest.raises(ValueError, match=r'test\.segment_merge'):
            _again(plain_cfg, segment_connectivity=0, segment_merge='spectrum')
        return r
    finally:
        shutil.rmtree(tmp)


def test_the_key_off_changes_nothing(golden_dir):
    r = _run(golden_dir)
    assert list(r['absent_files']) == list(r['position_files']) and len(r['absent_files']) > 0
    for name, data in r['absent_files'].items():
        assert r['position_files'][name] == data and (data is None or len(data) > 0), name
    assert sum(data is not None for data in r['absent_files'].values()) >= 7          # four maps, the image, three blocks
    assert r['absent'] == r['position'] and not {'merge', 'rounds'} & set(r['absent'])
    assert not {'merge', 'rounds'} & set(json.loads(r['absent_files']['0_segments.json']))
    # and the image is the positional merge's
    w = R.regions(r['engine_seg'], 64, 6)
    assert np.array_equal(r['absent_region'], w[1]) and r['absent']['regions'] == w[3][0]


def test_the_spectrum_block_and_maps(golden_dir):
    r = _run(golden_dir)
    b = r['segments']
    assert r['json'] == json.loads(json.dumps(b))
    st = r['engine_stats']
    assert b['merge'] == 'spectrum' and b['rounds'] == st['rounds'] >= 1 and b['connectivity'] == 'enforced' and b['min_size'] == 6
    assert (b['components'], b['absorbed'], b['regions']) == (st['components'], st['absorbed'], st['regions']) and st['regions'] == len(r['engine_sizes'])
    assert b['region_pixels'] == dict(min=int(r['engine_sizes'].min()), mean=float(r['engine_sizes'].mean()), max=int(r['engine_sizes'].max()))
    w_region, w_sizes, w_stats, _ = G.merge(r['engine_seg'], R.components(r['engine_seg']), r['host_scene'], 64, 6)
    assert np.array_equal(r['engine_region'], w_region) and tuple(w_stats) == (st['regions'], st['components'], st['absorbed'], st['rounds'])
    assert r['npy'].dtype == np.int32 and np.array_equal(r['npy'], r['engine_region'])
    assert not np.array_equal(r['engine_region'], r['absent_region']) and b['components'] == r['absent']['components']
    m = np.array(b['matrix'])
    x, y = r['test_xy'][:, 0], r['test_xy'][:, 1]
    want = np.zeros_like(m)
    np.add.at(want, (r['engine_label'][x, y], r['test_lab']), 1)
    assert np.array_equal(m, want) and m.sum() == r['matrix'].sum() == b['n']
    assert np.array_equal(r['segment_maps'][1], r['engine_label']) and np.array_equal(r['segments_png'][1], r['lut'][r['engine_label']])
    print('spectrum: %d components, %d regions in %d rounds (position: %d regions); OA %.4f -> %.4f (position %.4f), single observations'
          % (b['components'], b['regions'], b['rounds'], r['absent']['regions'], b['before']['OA'], b['after']['OA'], r['absent']['after']['OA']))


def test_the_drop_in_path_gives_the_same_regions_and_maps(golden_dir):
    r = _run(golden_dir)
    differ = int((r['dropin_region'] != r['engine_region']).sum())
    maps = [int((a != b).sum()) for a, b in zip(r['dropin_maps'], r['segment_maps'])]
    print('the drop-in path: region image differs at %d of 1600 pixels, the voted maps at %s' % (differ, maps))
    assert differ == 0 and maps == [0, 0]
    assert all(r['dropin'][k] == r['segments'][k] for k in ('components', 'absorbed', 'regions', 'rounds', 'merge', 'matrix'))
