"""CPU: the float64 statement of the superpixel voting (tests/segments_ref.py) against a per-pixel loop, the drop-in
path's utils/segments.py against it, the config keys, the refusals of the out-of-scope solvers, the agreement of header, bindings
and library on the new symbols, every refusal of the entry points (which return before anything touches a device, so host memory
stands in for device memory here), and the guards of the cases that tests/test_gpu_segments.py runs (tests/segments_cases.py),
on the reference alone.

The guards.
  (a) near ties.  The kernel's labels are compared with the reference's outside the tie set: the pixels whose float64 gap
      between the best and the second-best D is under the sum of the two distances' derived fp32 bounds (segments_ref.distances).
      On scenes of at least 100 pixels that set is at most segments_cases.TIE_CAP = 0.02 of the pixels, in every assign of ten
      iterations.
  (b) purity.  On scenes with more than one cell per axis the reference's segments after ten iterations are purer than the plain
      grid: the share of pixels whose base spectrum is their segment's most frequent one.  Asserted on every such scene
      (segments_cases.check_purity).  At 33 x 17 and S = 4 the grid is already perfectly pure, which nothing exceeds: there the
      segments are asked to be perfectly pure too (seven scenes).  FINDINGS, recorded with their figures and asserted as such
      (segments_cases.PURITY_SHORTFALLS): three one-band scenes fall short of the grid — 33 x 17 x 1 at S = 4 (0.988 against
      1.000), 64 x 65 x 1 at S = 4 (0.754 against 0.812) and at S = 5 (0.694 against 0.708).
  (c) vote margin.  Mode majority is compared exactly and needs no margin.  Mode mean: a segment is inside the label margin when
      the gap of its two largest means is within the sum of their derived fp32 bounds (segments_ref.vote_unclear; hundreds of
      times tighter than the fixed 1e-4 of parity_cases.MARGIN, inside which 33 x 17, K = 64, S = 16 has one of its six segments:
      24 % of its pixels); the share of masked pixels in such segments stays under parity_cases.MARGIN_CAP (0.15) on scenes of at
      least 100 pixels.  Cases with K >= 3, at least 100 pixels and at least 3 cells per axis see at least 3 classes."""
import ctypes
import os

import numpy as np
import pytest

import segments_cases as SC
import segments_ref as R
from parity_cases import MARGIN, MARGIN_CAP

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('dmf_slic_workspace_bytes', 'dmf_slic_init', 'dmf_slic_assign', 'dmf_slic_update', 'dmf_segment_vote')


# ------------------------------------------------------------------------------------------------ the reference itself
def test_reference_against_a_per_pixel_loop():
    H, W, C, S, K = 13, 9, 3, 5, 4
    a = SC.scene(H, W, C).astype(np.float64)
    gh, gw = R.grid(H, W, S)
    assert (gh, gw) == (3, 2)
    cen = R.init(SC.scene(H, W, C), H, W, S)
    assert cen.shape == (6, C + 2) and tuple(cen[5, C:]) == (12.0, 7.0) and np.array_equal(cen[5, :C], a[12, 7])      # min(H - 1, 2 S + 2) = 12
    cw = R.compact_weight(SC.COMPACTNESS, S)
    assert cw == float(np.float32((float(np.float32(0.05)) / 5) ** 2))
    seg, _ = R.assign(SC.scene(H, W, C), H, W, S, SC.COMPACTNESS, cen)
    for i in range(H):
        for j in range(W):
            best, label = np.inf, None
            for u in (-1, 0, 1):
                for v in (-1, 0, 1):
                    ci, cj = i // S + u, j // S + v
                    if 0 <= ci < gh and 0 <= cj < gw:
                        k = ci * gw + cj
                        D = ((a[i, j] - cen[k, :C]) ** 2).sum() / C + cw * ((i - cen[k, C]) ** 2 + (j - cen[k, C + 1]) ** 2)
                        if D < best:
                            best, label = D, k
            assert seg[i, j] == label, (i, j)
    new, counts, _ = R.update(SC.scene(H, W, C), H, W, S, seg, cen)
    assert counts.sum() == H * W
    for k in range(gh * gw):
        ii, jj = np.nonzero(seg == k)
        assert counts[k] == len(ii)
        if len(ii):
            assert np.abs(new[k, :C] - a[ii, jj].mean(0)).max() <= 1e-14 and abs(new[k, C] - ii.mean()) <= 1e-12 and abs(new[k, C + 1] - jj.mean()) <= 1e-12
    # a label that is none of a pixel's candidates is a member of nothing; an emptied cluster keeps its row
    odd = seg.copy()
    odd[odd == 5] = 3                                    # (cluster 3 is a candidate of every pixel that chose 5)
    odd[0, 0], odd[1, 1] = 5, -3                         # cell (2, 1) is no candidate of pixel (0, 0)
    new2, counts2, _ = R.update(SC.scene(H, W, C), H, W, S, odd, cen)
    assert counts2[5] == 0 and np.array_equal(new2[5], cen[5]) and counts2.sum() == H * W - 2
    # the vote
    prob, mask = R.softmax_rows(SC.logits(H, W, K)).reshape(H, W, K), SC.mask(H, W)
    for mode in ('mean', 'majority'):
        segprob, segcount, labels, rows, orphan = R.vote(prob, mask, odd, S, mode)
        assert orphan.sum() == int(mask[0, 0] != 0) + int(mask[1, 1] != 0)
        for k in range(gh * gw):
            mem = (odd == k) & (mask != 0) & R.members(odd, H, W, S)
            assert segcount[k] == mem.sum()
            if mem.any():
                want = prob[mem].mean(0) if mode == 'mean' else np.bincount(prob[mem].argmax(1), minlength=K)
                assert np.abs(segprob[k] - want).max() <= 1e-14
                assert (labels[mem] == segprob[k].argmax()).all()
        assert (labels[mask == 0] == 0).all() and (rows[mask == 0] == 0).all()
        assert np.array_equal(labels[orphan], prob[orphan].argmax(1))


def test_iterations_and_untouched_rows():
    H, W, C, S = 33, 17, 8, 5
    a = SC.scene(H, W, C)
    seg, cen, counts, _ = R.slic(a, H, W, S, SC.COMPACTNESS, 3)
    c = R.init(a, H, W, S)
    for _ in range(3):
        c, n, _ = R.update(a, H, W, S, R.assign(a, H, W, S, SC.COMPACTNESS, c)[0], c)
    assert np.array_equal(cen, c) and np.array_equal(counts, n) and np.array_equal(seg, R.assign(a, H, W, S, SC.COMPACTNESS, c)[0])
    assert R.members(seg, H, W, S).all() and np.array_equal(R.slic(a, H, W, S, SC.COMPACTNESS, 0)[0], R.assign(a, H, W, S, SC.COMPACTNESS, R.init(a, H, W, S))[0])
    dirty = np.full((H, W, 3), np.nan)                   # what an unmasked row holds is never read
    mask = SC.mask(H, W)
    prob = R.softmax_rows(SC.logits(H, W, 3)).reshape(H, W, 3)
    dirty[mask != 0] = prob[mask != 0]
    for mode in ('mean', 'majority'):
        assert np.array_equal(R.vote(dirty, mask, seg, S, mode)[0], R.vote(prob, mask, seg, S, mode)[0])


# ------------------------------------------------------------------------------------------------ utils/segments.py (fast_path: 0)
@pytest.mark.parametrize('H,W,C,S,half', [(13, 9, 3, 4, False), (33, 17, 8, 5, True), (35, 34, 200, 16, False), (2, 7, 1, 4, False), (1, 1, 3, 16, False)])
def test_the_drop_in_arithmetic_is_the_reference(H, W, C, S, half):
    from utils import segments
    scene = np.pad(SC.scene(H, W, C, half), ((0, 4), (0, 6), (0, 0)), mode='edge')         # a padded scene
    assert segments.grid(H, W, S) == R.grid(H, W, S)
    cen = segments.init_centres(scene, H, W, S)
    assert np.array_equal(cen, R.init(scene, H, W, S))
    seg = segments.assign(scene, H, W, S, SC.COMPACTNESS, cen)
    want, tie = R.assign(scene, H, W, S, SC.COMPACTNESS, cen)
    assert seg.dtype == np.int32 and np.array_equal(seg[~tie], want[~tie])
    new, counts = segments.update(scene, H, W, S, want, cen)
    ref_new, ref_counts, _ = R.update(scene, H, W, S, want, cen)
    assert np.abs(new - ref_new).max() <= 1e-13 and np.array_equal(counts, ref_counts) and counts.dtype == np.int32
    got = segments.slic(scene, H, W, S, SC.COMPACTNESS, 3)
    ref = R.slic(scene, H, W, S, SC.COMPACTNESS, 3)
    if not ref[3].any():                                 # (no near tie in any of the four assigns: the same segments)
        assert np.array_equal(got[0], ref[0]) and np.abs(got[1] - ref[1]).max() <= 1e-12 and np.array_equal(got[2], ref[2])
    K = 3
    prob, mask = R.softmax_rows(SC.logits(H, W, K)).reshape(H, W, K), SC.mask(H, W)
    odd = ref[0].copy()
    odd[0, 0] = -1
    for mode in ('mean', 'majority'):
        segprob, segcount, labels = segments.vote(prob, mask, odd, S, mode)
        w_prob, w_count, w_labels, _, _ = R.vote(prob, mask, odd, S, mode)
        assert np.abs(segprob - w_prob).max() <= 1e-14 and np.array_equal(segcount, w_count)
        clear = R.top2_margin(w_prob)[np.clip(odd, 0, None)] > 1e-12
        assert labels.dtype == np.int32 and np.array_equal(labels[clear], w_labels[clear]) and (labels[mask == 0] == 0).all()


def test_the_report_block():
    from indicators.kappa import aa_oa_quiet
    from utils import segments
    keys = segments.segment_keys({'test': {'segments': 'slic', 'segment_size': 5, 'segment_vote': 'majority'}})
    before = np.array([[0, 0, 0], [0, 5, 2], [0, 1, 6]], dtype=np.float64)
    after = np.array([[0, 0, 0], [0, 6, 1], [0, 0, 7]])
    rep = segments.report(keys, 13, 9, np.array([0, 20, 30, 40, 27, 0]), before, after, 3)
    aa, oa, k = aa_oa_quiet(before)
    assert rep['before'] == dict(OA=oa, AA=aa, kappa=k) and rep['after']['OA'] == 13 / 14
    assert rep['matrix'] == after.tolist() and rep['n'] == 14 and rep['changed'] == 3
    assert (rep['kind'], rep['size'], rep['compactness'], rep['iterations'], rep['vote']) == ('slic', 5, 0.1, 10, 'majority')
    assert rep['Kc'] == 6 and rep['segments'] == 4 and rep['segment_pixels'] == dict(min=20, mean=29.25, max=40)
    assert rep['connectivity'] == 'not enforced'


# ------------------------------------------------------------------------------------------------ keys and refusals
def test_the_keys_parse_and_refuse():
    from utils import segments, spatial
    neutral = dict(kind=None, size=8, compactness=0.1, iterations=10, vote='mean', color=False)
    assert segments.segment_keys({}) == segments.segment_keys({'test': {'segments': 'none'}, 'color': {'segments': 0}}) == neutral
    assert segments.keys_in_use(neutral) == []
    on = segments.segment_keys({'test': {'segments': 'slic', 'segment_size': 16, 'segment_compactness': '0.05', 'segment_iterations': 3,
                                         'segment_vote': 'majority'}, 'color': {'segments': 1}})
    assert on == dict(kind='slic', size=16, compactness=0.05, iterations=3, vote='majority', color=True)
    assert segments.keys_in_use(on) == ['test.segments', 'color.segments']
    for bad in ({'segments': 'watershed'}, {'segment_size': 3}, {'segment_size': 33}, {'segment_size': 8.0}, {'segment_size': True},
                {'segment_compactness': -0.1}, {'segment_compactness': float('inf')}, {'segment_compactness': 'much'},
                {'segment_iterations': -1}, {'segment_iterations': 2.5}, {'segment_vote': 'median'}):
        with pytest.raises(ValueError, match=r'test\.segment'):
            segments.segment_keys({'test': bad})
    with pytest.raises(ValueError, match=r'color\.segments'):
        segments.segment_keys({'test': {'segments': 'slic'}, 'color': {'segments': 2}})
    with pytest.raises(ValueError, match=r'color\.segments'):
        segments.segment_keys({'color': {'segments': 1}})                # nothing votes on the map it would draw
    # the two features are independent: neither parser sees the other's keys
    both = {'test': {'segments': 'slic', 'spatial': 'bilateral'}}
    assert segments.segment_keys(both)['kind'] == 'slic' and spatial.spatial_keys(both)['kind'] == 'bilateral'
    assert set(spatial.spatial_keys(both)) == {'kind', 'radius', 'sigma_s', 'sigma_r', 'iterations', 'color'}


def test_the_shipped_config_documents_the_keys_commented_out():
    import yaml
    text = open(os.path.join(REPO, 'dual-modal-fusion_amd', 'config.yml')).read()
    for key in ('segments:', 'segment_size:', 'segment_compactness:', 'segment_iterations:', 'segment_vote:'):
        assert any(ln.strip().startswith('#') and key in ln for ln in text.splitlines()), key
    cfg = yaml.safe_load(text)
    assert not any(k.startswith('segment') for k in cfg['test']) and 'segments' not in cfg['color']


@pytest.mark.parametrize('section,key,val', [('test', 'segments', 'slic')])
def test_tostagesolver_refuses_the_keys_by_name(section, key, val):
    from solver.tostagesolver import toStageSolver
    cfg = {'Categories_Number': 5, 'schedule': {'loss': 'qua_loss', 'optimizer': 'ADAM', 'lr': 1e-3}, section: {key: val}}
    with pytest.raises(ValueError, match=r'%s\.%s is out of scope for toStageSolver' % (section, key)):
        toStageSolver(cfg)


@pytest.mark.parametrize('entry', ['test', 'color'])
def test_data_parallel_runs_refuse_the_keys(entry):
    from solver.mainsolver import Solver
    from utils import calibration as cal
    from utils import segments, spatial
    s = Solver.__new__(Solver)
    s.calib, s.spat, s.world = cal.calibration_keys({}), spatial.spatial_keys({}), 2
    s.segm = segments.segment_keys({'test': {'segments': 'slic'}})
    with pytest.raises(ValueError, match=r'test\.segments is out of scope for data-parallel runs \(2 ranks\)'):
        getattr(s, entry)()
    s.segm = segments.segment_keys({})
    s._single_device_scope()                                 # neutral keys: nothing to refuse


# ------------------------------------------------------------------------------------------------ header, bindings, library
def test_the_library_declares_and_exports_the_entry_points():
    from dmf import lib
    hdr = open(os.path.join(REPO, 'include', 'dmf.h')).read()
    so = ctypes.CDLL(lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name + '(' in hdr and name in lib.EXPORTS and hasattr(so, name), name
    assert "'dmf_segments.hip'" in open(os.path.join(REPO, 'dual-modal-fusion_amd', 'build.py')).read()
    assert lib.version() == 307 and '#define DMF_VERSION 307' in ' '.join(hdr.split())
    assert (lib.SEG_SMIN, lib.SEG_SMAX) == (4, 32) and '#define DMF_SEG_SMIN 4' in hdr and '#define DMF_SEG_SMAX 32' in hdr
    assert lib.VOTE_MODES == {'mean': 0, 'majority': 1} and '#define DMF_VOTE_MEAN 0' in hdr and '#define DMF_VOTE_MAJORITY 1' in hdr


def test_the_workspace_query():
    from dmf import lib
    f = lib._lib.dmf_slic_workspace_bytes
    assert f(13, 9, 3, 5) == 6 * 9 * (3 * 4 + 16) and f(512, 512, 224, 8) == 4096 * 9 * (224 * 4 + 16)
    assert [f(0, 9, 3, 5), f(13, 0, 3, 5), f(13, 9, 0, 5), f(13, 9, 3, 3), f(13, 9, 3, 33)] == [-1] * 5


def test_every_argument_error_returns_a_code_without_a_launch():
    """Each refusal has its code and comes before anything is launched or dereferenced: the buffers here are host memory, filled
    with a pattern that must survive."""
    from dmf import lib
    f = lib._lib
    H, W, Cn, S, K = 7, 5, 4, 4, 3
    Kc = 4
    ws_bytes = f.dmf_slic_workspace_bytes(H, W, Cn, S)
    bufs = dict(scene=np.full(H * W * Cn, 0.5, dtype=np.float32), centres=np.full(Kc * (Cn + 2), -7.0, dtype=np.float32),
                seg=np.full(H * W, -7, dtype=np.int32), counts=np.full(Kc, -7, dtype=np.int32), ws=np.full(ws_bytes, 9, dtype=np.uint8),
                prob=np.full(H * W * K, -7.0, dtype=np.float32), mask=np.full(H * W, 1, dtype=np.uint8),
                segprob=np.full(Kc * K, -7.0, dtype=np.float32), segcount=np.full(Kc, -7, dtype=np.int32),
                label=np.full(H * W, -7, dtype=np.int32), out=np.full(H * W * K, -7.0, dtype=np.float32))
    before = {k: v.copy() for k, v in bufs.items()}
    p = {k: ctypes.c_void_p(v.ctypes.data) for k, v in bufs.items()}
    off = lambda name, n: ctypes.c_void_p(bufs[name].ctypes.data + n)
    assert bufs['ws'].ctypes.data % 16 == 0

    def init(scene=p['scene'], eb=4, pitch=W, H=H, W=W, Cn=Cn, S=S, centres=p['centres']):
        return f.dmf_slic_init(scene, eb, pitch, H, W, Cn, S, centres, None)

    def assign(scene=p['scene'], eb=4, pitch=W, H=H, W=W, Cn=Cn, S=S, comp=0.05, centres=p['centres'], seg=p['seg']):
        return f.dmf_slic_assign(scene, eb, pitch, H, W, Cn, S, comp, centres, seg, None)

    def update(scene=p['scene'], eb=4, pitch=W, H=H, W=W, Cn=Cn, S=S, seg=p['seg'], centres=p['centres'], counts=p['counts'], ws=p['ws'],
               nbytes=ws_bytes):
        return f.dmf_slic_update(scene, eb, pitch, H, W, Cn, S, seg, centres, counts, ws, nbytes, None)

    def vote(prob=p['prob'], mask=p['mask'], seg=p['seg'], H=H, W=W, K=K, S=S, mode=0, segprob=p['segprob'], segcount=p['segcount'],
             label=p['label'], out=p['out']):
        return f.dmf_segment_vote(prob, mask, seg, H, W, K, S, mode, segprob, segcount, label, out, None)

    scene_args = lambda call: [(call(scene=None), 1), (call(H=0), 2), (call(W=0), 2), (call(Cn=0), 2), (call(S=3), 4), (call(S=33), 4),
                               (call(eb=3), 5), (call(eb=8), 5), (call(pitch=W - 1), 6), (call(scene=off('scene', 2)), 8)]
    want = scene_args(init) + [(init(centres=None), 1), (init(centres=p['scene']), 7)]
    want += scene_args(assign) + [(assign(centres=None), 1), (assign(seg=None), 1), (assign(comp=-0.1), 10), (assign(comp=float('nan')), 10),
                                  (assign(comp=float('inf')), 10), (assign(seg=p['scene']), 7), (assign(seg=p['centres']), 7)]
    want += scene_args(update) + [(update(seg=None), 1), (update(centres=None), 1), (update(counts=None), 1), (update(ws=None), 1),
                                  (update(nbytes=ws_bytes - 1), 12), (update(nbytes=0), 12), (update(ws=off('ws', 4)), 8),
                                  (update(centres=p['scene']), 7), (update(counts=p['seg']), 7), (update(ws=p['scene'], nbytes=1 << 40), 7),
                                  (update(counts=off('centres', 4)), 7)]
    want += [(vote(prob=None), 1), (vote(mask=None), 1), (vote(seg=None), 1), (vote(segprob=None), 1), (vote(segcount=None), 1),
             (vote(label=None), 1), (vote(H=0), 2), (vote(W=-1), 2), (vote(K=0), 3), (vote(K=65), 3), (vote(S=3), 4), (vote(S=33), 4),
             (vote(mode=2), 11), (vote(mode=-1), 11), (vote(out=p['prob']), 7), (vote(out=off('prob', 4 * K)), 7), (vote(label=p['seg']), 7),
             (vote(segprob=p['prob']), 7), (vote(segcount=p['mask']), 7), (vote(out=p['segprob']), 7)]
    assert [rc for rc, _ in want] == [code for _, code in want]
    for k, v in bufs.items():
        assert np.array_equal(v, before[k]), k


# ------------------------------------------------------------------------------------------------ guards of the GPU cases
@pytest.mark.parametrize('seg_size', SC.SEG_SIZES)
def test_guard_a_near_ties_and_guard_b_purity(seg_size):
    worst, gains = 0.0, []
    for H, W in SC.SIZES:
        for C, half in [(C, False) for C in SC.BANDS_F32] + [(C, True) for C in SC.BANDS_F16]:
            a = SC.scene(H, W, C, half)
            cen = R.init(a, H, W, seg_size)
            shares = []
            for _ in range(SC.ITERATIONS):
                seg, tie = R.assign(a, H, W, seg_size, SC.COMPACTNESS, cen)
                shares.append(float(tie.mean()))
                cen, _, _ = R.update(a, H, W, seg_size, seg, cen)
            seg, tie = R.assign(a, H, W, seg_size, SC.COMPACTNESS, cen)
            shares.append(float(tie.mean()))
            assert R.members(seg, H, W, seg_size).all()
            if H * W >= SC.GUARD_MIN_PIXELS:
                worst = max(worst, max(shares))
                assert max(shares) <= SC.TIE_CAP, (H, W, C, half, seg_size, max(shares))
            if SC.purity_asked(H, W, seg_size):
                got, plain = R.purity(seg, SC.ids(H, W)), R.purity(R.grid_segments(H, W, seg_size), SC.ids(H, W))
                SC.check_purity((H, W, C, half, seg_size), got, plain)
                if (H, W, C, half, seg_size) in SC.PURITY_SHORTFALLS:
                    assert not any(shares)               # no near tie in any assign: a device is asked for the same segments
                    print('  recorded shortfall: %d x %d x %d, S = %d: purity %.3f, grid %.3f' % (H, W, C, seg_size, got, plain))
                else:
                    gains.append((got, plain))
    print('S = %d: largest tie share %.4f; purity %.2f .. %.2f against the grid\'s %.2f .. %.2f'
          % (seg_size, worst, min(g for g, _ in gains), max(g for g, _ in gains), min(p for _, p in gains), max(p for _, p in gains)))


@pytest.mark.parametrize('seg_size', SC.SEG_SIZES)
def test_guard_c_vote_margin(seg_size):
    worst, loose, classes = 0.0, 0.0, []
    for H, W, K, S in SC.VOTE_CASES:
        if S != seg_size:
            continue
        seg = R.slic(SC.scene(H, W, 8), H, W, S, SC.COMPACTNESS, 3)[0]
        prob, mask = R.softmax_rows(SC.logits(H, W, K)).reshape(H, W, K), SC.mask(H, W)
        live = mask != 0
        if not live.any():
            continue
        segprob, segcount, labels, rows, orphan = R.vote(prob, mask, seg, S, 'mean')
        assert not orphan.any()
        share = float(R.vote_unclear(segprob, segcount)[seg][live].mean())
        loose = max(loose, float((R.top2_margin(rows)[live] <= MARGIN).mean()))
        if H * W >= SC.GUARD_MIN_PIXELS:
            worst = max(worst, share)
            assert share <= MARGIN_CAP, (H, W, K, S, share)
        if SC.classes_guarded(H, W, K, S):
            classes.append(len(np.unique(labels[live])))
            assert classes[-1] >= 3, (H, W, K, S, classes[-1])
    print('S = %d: largest share inside the derived margin %.4f (inside 1e-4: %.4f); classes %d .. %d'
          % (seg_size, worst, loose, min(classes), max(classes)))


def test_the_case_tables():
    assert (13, 9) in SC.SIZES and len(SC.SLIC_CASES) == 6 * 8 * 3 and len(SC.VOTE_CASES) == 6 * 4 * 3
    assert SC.SEG_SIZES == (4, 5, 16) and SC.COMPACTNESS == 0.05 and SC.VOTE_K == (1, 3, 17, 64)
    assert SC.ids(13, 9).max() <= 4 and SC.ids(64, 65).shape == (64, 65)
