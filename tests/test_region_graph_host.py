"""CPU: the spectrum-aware fragment merge on the reference alone (tests/region_graph_ref.py), so that no test of
tests/test_gpu_region_graph.py is vacuous; the drop-in path's utils.segments.region_graph against it; the key; the agreement of
header, bindings and library; and every refusal of the entry points, which return before anything touches a device (host memory
stands in for device memory).
  (a) purity against segments_cases.ids, over every SLIC case: the spectrum rule is never below the positional one, and strictly
      above at (64, 65, 16), (129, 131, 16), (64, 65, 4) and (13, 9, 4): 0.346 / 0.254, 0.349 / 0.243, 1.000 / 0.996, 1.000 / 0.974;
  (b) every multi-tile size has a case with more than one round, and one where a group of fragments alone reaches min_size;
  (c) the constant scene's cases meet ties of distances (58,377 over 63 cases), the SLIC cases on the noisy scenes none;
  (d) rounds never exceed 1 + floor(log2(fragments)); no group ever holds two initially kept components (asserted inside the
      reference, every round of every case);
  (e) min_size 1 gives the positional reference's regions."""
import ctypes
import os

import numpy as np
import pytest

import region_graph_cases as GC
import region_graph_ref as G
import regions_cases as RC
import regions_ref as R
import segments_cases as SC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('dmf_region_graph_workspace_bytes', 'dmf_region_graph_count', 'dmf_region_graph_merge')


# ------------------------------------------------------------------------------------------------ the reference itself
def test_reference_on_a_hand_made_image():
    lab = np.array([[1, 1, 1, 1, 1],
                    [1, 7, 1, 8, 1],
                    [1, 1, 1, 9, 1],
                    [2, 2, 2, 2, 2]])
    comp = R.components(lab)
    scene = np.zeros((4, 5, 2), dtype=np.float32)
    scene[lab == 1], scene[lab == 2] = (0.25, 0.25), (0.75, 0.5)
    scene[1, 1], scene[1, 3], scene[2, 3] = (0.25, 0.5), (0.5, 0.625), (0.625, 0.5)
    # min_size 2: 7 (one pixel, enclosed by 1) joins 1; 8 and 9 are nearer to each other (d = 2 / 64) than to 1 (5 / 64 + ..) or,
    # for 9, to 2 (1 / 64 = (0.125)^2 + 0): 9 chooses 2, 8 chooses 9, and both end in 2's region
    region, sizes, stats, info = G.merge(lab, comp, scene, 0, 2)
    assert stats == (2, 5, 3, 1) and info['fragments'] == 3 and info['kept0'] == 2 and info['ties'] == 0
    assert region[1, 1] == 0 and region[1, 3] == region[2, 3] == region[3, 0] == 1 and sizes.tolist() == [13, 7]
    # with the row of 2s gone, 8 and 9 choose each other and reach min_size 2 together: a region of their own
    lab2 = np.where(lab == 2, 1, lab)
    region, sizes, stats, info = G.merge(lab2, R.components(lab2), np.where((lab == 2)[:, :, None], np.float32(0.25), scene), 0, 2)
    assert stats == (2, 4, 2, 1) and region[1, 3] == region[2, 3] == 1 and region[1, 1] == 0 and sizes.tolist() == [18, 2]
    # the positional rule sends all three to the component on their left
    assert R.merge(lab2, R.components(lab2), 0, 2)[2] == (1, 4, 3)
    assert [G.round_bound(f) for f in (0, 1, 2, 3, 4, 7, 8, 906)] == [0, 1, 2, 2, 3, 3, 4, 10]


# ------------------------------------------------------------------------------------------------ guards of the GPU cases
def test_guard_a_purity_is_never_below_the_positional_rule():
    seen = {}
    for H, W in RC.SIZES:
        ids = SC.ids(H, W)
        for S in RC.SLIC_S:
            for m in (RC.auto_min_size(S), 2):
                n = RC.kc(H, W, S)
                spectrum = R.purity(GC.reference('slic%d' % S, H, W, n, m, 'f32', 8)[0], ids)
                position = R.purity(RC.reference('slic%d' % S, H, W, n, m)[1], ids)
                assert spectrum >= position, (H, W, S, m, spectrum, position)
                if m == RC.auto_min_size(S):
                    seen[(H, W, S)] = (spectrum, position)
    for key in GC.STRICTLY_ABOVE:
        spectrum, position = seen[key]
        print('%s: purity %.3f (spectrum) against %.3f (position)' % (key, spectrum, position))
        assert spectrum > position and (round(spectrum, 3), round(position, 3)) == GC.PURITY[key], (key, spectrum, position)
    for key in ((64, 65, 16), (129, 131, 16), (64, 65, 4)):                            # the positional figures are §24's
        assert abs(seen[key][1] - RC.PURITY_AFTER[key]) < 5e-4
    st = GC.reference('slic16', 64, 65, 20, 64, 'f32', 8)
    assert st[2] == (43, 217, 174, 2) and st[3]['kept0'] == 20 == RC.reference('slic16', 64, 65, 20, 64)[3][0]
    st = GC.reference('slic16', 129, 131, 81, 64, 'f32', 8)
    assert st[2] == (153, 988, 835, 3) and st[3]['kept0'] == 82 == RC.reference('slic16', 129, 131, 81, 64)[3][0]


def test_guard_b_every_multi_tile_size_has_rounds_and_growth():
    assert set(GC.MULTI_TILE) == set(GC.MULTI_ROUND) == set(GC.GROWN) == {(1, 70), (70, 1), (33, 17), (64, 65), (129, 131)}
    for (H, W), (name, n, m) in GC.MULTI_ROUND.items():
        assert (name, H, W, n, m) in GC.LABEL_CASES
        assert GC.reference(name, H, W, n, m, 'f32', 8)[2][3] > 1, (H, W, name)
    for (H, W), (name, n, m) in GC.GROWN.items():
        assert (name, H, W, n, m) in GC.LABEL_CASES
        _, _, stats, info = GC.reference(name, H, W, n, m, 'f32', 8)
        assert stats[0] > info['kept0'], (H, W, name, stats, info['kept0'])             # a group of fragments became a region


def test_guard_c_the_constant_scene_meets_ties():
    ties = [GC.reference(*c, 'const', 3)[3]['ties'] for c in GC.LABEL_CASES]
    print('constant scene: %d ties over %d of %d cases' % (sum(ties), sum(t > 0 for t in ties), len(ties)))
    assert sum(ties) > 0
    assert GC.reference('checker', 129, 131, 0, 2, 'const', 3)[3]['ties'] > 0
    chain = G.merge(RC.labels_of('alternate', *GC.CHAIN), RC.components('alternate', *GC.CHAIN), GC.scene('const', 3, *GC.CHAIN), 0, 2)
    assert chain[2] == (1, 4096, 4095, 1) and chain[3]['ties'] == 4094               # (the last pixel has one neighbour)
    slic = sum(GC.reference(*c, kind, C)[3]['ties'] for c in GC.LABEL_CASES if c[0].startswith('slic') for kind, C in GC.SCENES if kind in ('f32', 'f16'))
    assert slic == 0                                                                   # recorded: which is why the constant scene is there


@pytest.mark.parametrize('kind,C', GC.SCENES, ids=lambda v: str(v))
def test_guard_d_rounds_stay_within_the_bound(kind, C):
    worst = 0
    for c in GC.LABEL_CASES:
        region, sizes, stats, info = GC.reference(*c, kind, C)
        assert stats[3] <= G.round_bound(info['fragments']) and len(info['per_round']) == stats[3], (c, stats, info)
        assert all(2 * b <= a for a, b in zip(info['per_round'], info['per_round'][1:])), (c, info['per_round'])      # at least halved
        assert stats[0] + stats[2] == stats[1] and sizes.sum() == c[1] * c[2] and sizes.min() >= 1 and stats[0] >= info['kept0']
        assert (stats[3] == 0) == (info['fragments'] == 0)
        worst = max(worst, stats[3])
    print('%s %d: at most %d rounds' % (kind, C, worst))


def test_guard_e_min_size_1_is_the_positional_merge():
    for c in GC.LABEL_CASES:
        if c[4] != 1:
            continue
        region, sizes, stats, _ = GC.reference(*c, 'f32', 3)
        _, w_region, w_sizes, w_stats, _ = RC.reference(*c)
        assert np.array_equal(region, w_region) and np.array_equal(sizes, w_sizes) and stats == tuple(w_stats) + (0,), c


# ------------------------------------------------------------------------------------------------ the drop-in path
@pytest.mark.parametrize('kind,C', GC.SCENES, ids=lambda v: str(v))
def test_the_drop_in_merge_equals_the_reference(kind, C):
    from utils import segments
    for c in GC.LABEL_CASES:
        name, H, W, n, m = c
        w_region, w_sizes, w_stats, _ = GC.reference(*c, kind, C)
        region, sizes, stats = segments.region_graph(RC.labels_of(name, H, W), GC.padded(kind, C, H, W), n, m)
        assert region.dtype == np.int32 and np.array_equal(region, w_region) and np.array_equal(sizes, w_sizes), (c, kind, C)
        assert stats == dict(regions=w_stats[0], components=w_stats[1], absorbed=w_stats[2], rounds=w_stats[3]), (c, kind, C)


def test_the_drop_in_merge_refuses_bad_arguments():
    from utils import segments
    lab, a = np.zeros((3, 4), dtype=np.int32), np.zeros((3, 4, 2), dtype=np.float32)
    for kw in (dict(min_size=0), dict(min_size=1.5), dict(n_labels=-1), dict(min_size=True)):
        with pytest.raises(ValueError, match='region_graph'):
            segments.region_graph(lab, a, **kw)
    with pytest.raises(ValueError, match='region_graph'):
        segments.region_graph(lab, a[:2])


# ------------------------------------------------------------------------------------------------ the key, the report
def test_the_key_parses_and_refuses():
    from utils import segments
    sk, rk = segments.segment_keys, segments.region_keys

    def merge(test):
        cfg = {'test': test}
        return segments.merge_key(cfg, rk(cfg, sk(cfg)))
    assert merge({}) == 'position' and merge({'segments': 'slic'}) == 'position' and merge({'segment_merge': 'position'}) == 'position'
    assert merge({'segments': 'slic', 'segment_connectivity': 1}) == 'position'
    assert merge({'segments': 'slic', 'segment_connectivity': 1, 'segment_merge': 'spectrum'}) == 'spectrum'
    assert merge({'segments': 'slic', 'segment_connectivity': 1, 'segment_merge': 'Spectrum'}) == 'spectrum'
    assert merge({'segments': 'file', 'segment_file': 'p.npy', 'segment_merge': 'spectrum'}) == 'spectrum'
    for test in ({'segment_merge': 'spectrum'}, {'segments': 'slic', 'segment_merge': 'spectrum'},
                 {'segments': 'slic', 'segment_connectivity': 0, 'segment_merge': 'spectrum'},
                 {'segments': 'slic', 'segment_connectivity': 1, 'segment_merge': 'nearest'}, {'segment_merge': 1}):
        with pytest.raises(ValueError, match=r'test\.segment_merge'):
            merge(test)
    # the dict of region_keys is the one it was
    cfg = {'test': {'segments': 'slic', 'segment_connectivity': 1, 'segment_merge': 'spectrum'}}
    assert rk(cfg, sk(cfg)) == dict(connectivity=True, min_size=16, file=None)


def test_the_shipped_config_documents_the_key_commented_out():
    import yaml
    text = open(os.path.join(REPO, 'dual-modal-fusion_amd', 'config.yml')).read()
    assert any(ln.strip().startswith('#') and 'segment_merge:' in ln for ln in text.splitlines())
    assert not any(k.startswith('segment') for k in yaml.safe_load(text)['test'])


def test_the_report_block_gains_merge_and_rounds_only_with_spectrum():
    from utils import segments
    keys = segments.segment_keys({'test': {'segments': 'slic', 'segment_size': 5}})
    m = np.array([[3, 1], [0, 4]], dtype=np.float64)
    plain = segments.report(keys, 13, 9, np.array([20, 30, 40, 27]), m, m, 0)
    position = segments.region_report(plain, 6, dict(regions=3, components=9, absorbed=6), np.array([50, 60, 7]))
    spectrum = segments.region_report(plain, 6, dict(regions=3, components=9, absorbed=6, rounds=2), np.array([50, 60, 7]))
    assert 'merge' not in position and 'rounds' not in position
    assert spectrum['merge'] == 'spectrum' and spectrum['rounds'] == 2 and {k: v for k, v in spectrum.items() if k not in ('merge', 'rounds')} == position


@pytest.mark.parametrize('test', [{'segments': 'file', 'segment_file': 'p.npy', 'segment_merge': 'spectrum'},
                                  {'segments': 'slic', 'segment_connectivity': 1, 'segment_merge': 'spectrum'}])
def test_tostagesolver_and_data_parallel_runs_refuse(test):
    from solver.mainsolver import Solver
    from solver.tostagesolver import toStageSolver
    from utils import calibration as cal
    from utils import segments, spatial
    cfg = {'Categories_Number': 5, 'schedule': {'loss': 'qua_loss', 'optimizer': 'ADAM', 'lr': 1e-3}, 'test': test}
    with pytest.raises(ValueError, match=r'test\.segments is out of scope for toStageSolver'):
        toStageSolver(cfg)
    s = Solver.__new__(Solver)
    s.calib, s.spat, s.world = cal.calibration_keys({}), spatial.spatial_keys({}), 2
    s.segm = segments.segment_keys({'test': test})
    for entry in ('test', 'color'):
        with pytest.raises(ValueError, match=r'test\.segments is out of scope for data-parallel runs \(2 ranks\)'):
            getattr(s, entry)()


# ------------------------------------------------------------------------------------------------ header, bindings, library
def test_the_library_declares_and_exports_the_entry_points():
    from dmf import lib
    hdr = open(os.path.join(REPO, 'include', 'dmf.h')).read()
    so = ctypes.CDLL(lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name + '(' in hdr and name in lib.EXPORTS and hasattr(so, name), name
    assert "'dmf_region_graph.hip'" in open(os.path.join(REPO, 'dual-modal-fusion_amd', 'build.py')).read()
    assert lib.version() == 307                                                        # unchanged: the symbols are found by name
    assert '#define DMF_REGION_GRAPH_ROUNDS_MAX 27' in hdr and G.round_bound(2 ** 27 - 1) == 27


def test_the_workspace_query():
    from dmf import lib
    f = lib._lib.dmf_region_graph_workspace_bytes
    up = lambda n: (n + 15) // 16 * 16
    fixed = lambda P, nl: up(nl * 8) + 2 * up(P * 4) + up((P + 1023) // 1024 * 4) + 16 + up(27 * 4) + 2 * up(P * 8)
    per = lambda n, C: 6 * up(n * 4) + up((n + 1023) // 1024 * 4) + up(n * 8) + 2 * up(n * C * 8)
    assert f(13, 9, 8, 6, 14) == fixed(117, 6) + per(14, 8)
    assert f(512, 512, 224, 4096, 30000) == fixed(512 * 512, 4096) + per(30000, 224)
    # sums and means are indexed by component: 16 C bytes each, not per pixel
    assert f(512, 512, 224, 0, 30004) - f(512, 512, 224, 0, 30000) == 4 * (16 * 224 + 6 * 4 + 8) and f(512, 512, 224, 0, 30000) < 130e6
    assert [f(0, 9, 8, 0, 1), f(13, 0, 8, 0, 1), f(13, 9, 0, 0, 1), f(13, 9, 8, -1, 1), f(13, 9, 8, 0, 0), f(13, 9, 8, 0, 118),
            f(16384, 8192, 8, 0, 1)] == [-1] * 7
    assert f(11585, 11585, 1, 0, 1) > 0                                                # just below 2^27 pixels


def test_every_argument_error_returns_a_code_without_a_launch():
    """Each refusal has its code and comes before anything is launched or dereferenced: the buffers here are host memory, filled
    with a pattern that must survive."""
    from dmf import lib
    f = lib._lib
    H, W, C, NL, NC, NF = 7, 5, 3, 6, 9, 4
    n, pitch = H * W, W + 2
    ws_bytes, cws_bytes = f.dmf_region_graph_workspace_bytes(H, W, C, NL, NC), f.dmf_region_graph_workspace_bytes(H, W, 1, NL, 1)
    bufs = dict(labels=np.full(n, 3, dtype=np.int32), comp=np.full(n, -7, dtype=np.int32), region=np.full(n, -7, dtype=np.int32),
                sizes=np.full(n, -7, dtype=np.int32), stats=np.full(4, -7, dtype=np.int32), counts=np.full(2, -7, dtype=np.int32),
                scene=np.full(H * pitch * C, 0.5, dtype=np.float32), ws=np.full(ws_bytes + 16, 9, dtype=np.uint8))
    before = {k: v.copy() for k, v in bufs.items()}
    p = {k: ctypes.c_void_p(v.ctypes.data) for k, v in bufs.items()}
    p['ws'] = ctypes.c_void_p((bufs['ws'].ctypes.data + 15) // 16 * 16)               # a 16-byte aligned start inside the allocation
    off = lambda name, nbytes: ctypes.c_void_p(p[name].value + nbytes)

    def count(labels=p['labels'], comp=p['comp'], H=H, W=W, nl=NL, ms=2, counts=p['counts'], ws=p['ws'], nbytes=cws_bytes):
        return f.dmf_region_graph_count(labels, comp, H, W, nl, ms, counts, ws, nbytes, None)

    def merge(labels=p['labels'], comp=p['comp'], scene=p['scene'], eb=4, pitch=pitch, H=H, W=W, C=C, nl=NL, ms=2, nc=NC, nf=NF,
              region=p['region'], sizes=p['sizes'], stats=p['stats'], ws=p['ws'], nbytes=ws_bytes):
        return f.dmf_region_graph_merge(labels, comp, scene, eb, pitch, H, W, C, nl, ms, nc, nf, region, sizes, stats, ws, nbytes, None)

    want = [(count(labels=None), 1), (count(comp=None), 1), (count(counts=None), 1), (count(ws=None), 1), (count(H=0), 2), (count(W=-1), 2),
            (count(ms=0), 14), (count(nl=-1), 15), (count(H=16384, W=8192), 13), (count(nbytes=cws_bytes - 1), 12), (count(nbytes=0), 12),
            (count(ws=off('ws', 8)), 8), (count(labels=off('labels', 2)), 8), (count(counts=off('counts', 1)), 8),
            (count(counts=p['labels']), 7), (count(counts=off('comp', 4 * (n - 1))), 7), (count(ws=p['comp'], nbytes=1 << 40), 7)]
    want += [(merge(labels=None), 1), (merge(comp=None), 1), (merge(scene=None), 1), (merge(region=None), 1), (merge(sizes=None), 1),
             (merge(stats=None), 1), (merge(ws=None), 1), (merge(H=0), 2), (merge(W=0), 2), (merge(C=0), 2), (merge(C=-4), 2),
             (merge(eb=1), 5), (merge(eb=8), 5), (merge(eb=0), 5), (merge(pitch=W - 1), 6), (merge(pitch=0), 6),
             (merge(ms=0), 14), (merge(ms=-3), 14), (merge(nl=-1), 15), (merge(H=16384, W=8192, pitch=8192), 13),
             (merge(nc=0), 16), (merge(nc=n + 1), 16), (merge(nf=-1), 16), (merge(nf=NC), 16),
             (merge(nbytes=ws_bytes - 1), 12), (merge(nl=NL + 2), 12), (merge(nc=NC + 1), 12), (merge(C=C + 1), 12),
             (merge(ws=off('ws', 8)), 8), (merge(region=off('region', 2)), 8), (merge(scene=off('scene', 2)), 8), (merge(scene=off('scene', 1), eb=2), 8),
             (merge(region=p['labels']), 7), (merge(region=p['comp']), 7), (merge(sizes=p['comp']), 7), (merge(stats=off('labels', 8)), 7),
             (merge(sizes=p['region']), 7), (merge(stats=off('region', 4)), 7), (merge(region=p['scene']), 7),
             (merge(stats=off('scene', 4 * (((H - 1) * pitch + W) * C - 1))), 7),
             (merge(ws=p['comp'], nbytes=1 << 40), 7), (merge(ws=p['scene'], nbytes=1 << 40), 7), (merge(ws=p['region'], nbytes=1 << 40), 7)]
    assert [rc for rc, _ in want] == [code for _, code in want]
    # the scene's margin after the last pixel is not the scene's: an output may sit there
    assert f.dmf_region_graph_workspace_bytes(H, W, C, NL, NC) == ws_bytes
    for k, v in bufs.items():
        assert np.array_equal(v, before[k]), k
