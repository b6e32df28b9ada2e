"""CPU: the float64 statement of the spatial regularisation (tests/spatial_ref.py) against a brute-force loop, its
invariants, the drop-in path's utils/spatial.py against it, the config keys, the refusals of the out-of-scope solvers, and the
guards of the cases that tests/test_gpu_spatial.py runs (tests/spatial_cases.py), on the reference alone.

The guards.  The label map of the kernel is compared with the reference's argmax on every masked pixel whose top-2 margin of
`out` exceeds parity_cases.MARGIN (1e-4, hundreds of times the filter's rounding); the share that this leaves out must stay
below parity_cases.MARGIN_CAP (0.15) in EVERY case.  Two further guards make the comparison mean something and can only be
asked of a scene with room for them (at least spatial_cases.GUARD_MIN_PIXELS = 100 pixels; K >= 3): at least 3 classes are
predicted, and the filter changes the class of at least 10 % of the masked pixels against the unfiltered argmax.  (A 1 x 1 or
2 x 7 scene has 1 or 14 pixels and lies inside one or two regions; K = 1 has one class.)"""
import os

import numpy as np
import pytest

import spatial_cases as S
import spatial_ref as R
from parity_cases import MARGIN, MARGIN_CAP

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(H, W, K, r, C=8):
    """(aff, prob, mask) of a case in float64: the reference's own affinities and the softmax of the case's logits."""
    aff, _ = R.affinity(S.scene(H, W, C), H, W, r, S.SIGMA_S, S.SIGMA_R)
    mask = S.mask(H, W)
    keep = mask.reshape(-1) != 0
    prob, m = R.scatter(S.logits(H, W, K)[keep], S.pixels(H, W)[keep], H, W)
    assert np.array_equal(m, mask)
    return aff, prob, mask


# ------------------------------------------------------------------------------------------------ the reference itself
def test_reference_against_a_per_pixel_loop():
    H, W, r, C, K = 13, 9, 1, 3, 4
    a = S.scene(H, W, C).astype(np.float64)
    cs, cr = R.coefficients(S.SIGMA_S, S.SIGMA_R)
    aff, E = R.affinity(S.scene(H, W, C), H, W, r, S.SIGMA_S, S.SIGMA_R)
    _, prob, mask = _case(H, W, K, r, C)
    out, pred = R.filter_once(prob, mask, aff, r)
    for i in range(H):
        for j in range(W):
            num, den = np.zeros(K), 0.0
            for k, (di, dj) in enumerate(R.window(r)):
                y = (i + di, j + dj)
                if not (0 <= y[0] < H and 0 <= y[1] < W):
                    assert aff[i, j, k] == 0.0 and E[i, j, k] == 0.0
                    continue
                e = (di * di + dj * dj) * cs + ((a[i, j] - a[y]) ** 2).sum() / C * cr
                assert abs(E[i, j, k] - e) <= 1e-12 * max(e, 1.0) and abs(aff[i, j, k] - np.exp(-e)) <= 1e-14
                if mask[y]:
                    num += np.exp(-e) * prob[y]
                    den += np.exp(-e)
            if mask[i, j]:
                assert np.abs(out[i, j] - num / den).max() <= 1e-14 and pred[i, j] == int(np.argmax(num / den))
            else:
                assert (out[i, j] == 0).all()
    assert (aff[:, :, 4] == 1.0).all()                   # the centre
    assert R.window(2)[12] == (0, 0) and len(R.window(3)) == 49


@pytest.mark.parametrize('r', S.RADII)
def test_invariants(r):
    H, W, K = 33, 17, 17
    aff, prob, mask = _case(H, W, K, r)
    out, _ = R.filter_once(prob, mask, aff, r)
    live = mask != 0
    assert np.abs(out[live].sum(1) - 1.0).max() <= 1e-12 and (out[~live] == 0).all() and (out >= 0).all()
    n = (2 * r + 1) ** 2
    assert (aff[:, :, (n - 1) // 2] == 1.0).all() and aff.max() <= 1.0
    # a constant scene, an all-ones mask and a uniform probability map: a fixed point
    flat, _ = R.affinity(np.full((H, W, 3), 0.25, dtype=np.float32), H, W, r, S.SIGMA_S, S.SIGMA_R)
    uni = np.full((H, W, K), 1.0 / K)
    again, _ = R.regularise(uni, np.ones((H, W), dtype=np.uint8), flat, r, iterations=2)
    assert np.abs(again - uni).max() <= 1e-15
    # sigma_r -> tiny: only the centre weighs (and neighbours that equal it in every band, of which a noisy scene has none)
    sharp, _ = R.affinity(S.scene(H, W, 8), H, W, r, S.SIGMA_S, 1e-4)
    same, pred = R.filter_once(prob, mask, sharp, r)
    assert np.array_equal(pred[live], prob.argmax(2)[live]) and np.abs(same - prob)[live].max() <= 1e-12


def test_iterations_chain_and_unmasked_rows_do_not_count():
    H, W, K, r = 13, 9, 3, 2
    aff, prob, mask = _case(H, W, K, r)
    one, _ = R.filter_once(prob, mask, aff, r)
    two, _ = R.filter_once(one, mask, aff, r)
    assert np.array_equal(R.regularise(prob, mask, aff, r, iterations=2)[0], two)
    dirty = prob.copy()
    dirty[mask == 0] = np.nan                            # what an unmasked cell holds is never read
    assert np.array_equal(R.filter_once(dirty, mask, aff, r)[0], one)


# ------------------------------------------------------------------------------------------------ utils/spatial.py (fast_path: 0)
@pytest.mark.parametrize('H,W,K,r,half', [(13, 9, 3, 1, False), (33, 17, 17, 2, False), (35, 34, 64, 3, True), (2, 7, 1, 3, False), (1, 1, 3, 2, False)])
def test_the_drop_in_arithmetic_is_the_reference(H, W, K, r, half):
    from utils import spatial
    scene = np.pad(S.scene(H, W, 8, half), ((0, 4), (0, 6), (0, 0)), mode='reflect' if min(H, W) > 6 else 'edge')   # a padded scene
    aff = spatial.affinity(scene, H, W, r, S.SIGMA_S, S.SIGMA_R)
    want, _ = R.affinity(scene, H, W, r, S.SIGMA_S, S.SIGMA_R)
    assert aff.shape == (H, W, (2 * r + 1) ** 2) and np.abs(aff - want).max() <= 1e-15
    logits, mask = S.logits(H, W, K), S.mask(H, W)
    for beta in (1.0, 0.5):
        assert np.abs(spatial.probabilities(logits, beta) - R.softmax(logits, beta)).max() <= 1e-15
    keep = mask.reshape(-1) != 0
    prob, _ = R.scatter(logits[keep], S.pixels(H, W)[keep], H, W, 0.5)
    got, labels = spatial.regularise(prob, mask, aff, r, iterations=2)
    ref, pred = R.regularise(prob, mask, want, r, iterations=2)
    assert np.abs(got - ref).max() <= 1e-14
    assert labels.dtype == np.int32 and np.array_equal(labels[mask != 0], pred[mask != 0]) and (labels[mask == 0] == 0).all()


def test_the_report_block():
    from indicators.kappa import aa_oa_quiet
    from utils import spatial
    keys = spatial.spatial_keys({'test': {'spatial': 'bilateral', 'spatial_radius': 3}})
    before = np.array([[0, 0, 0], [0, 5, 2], [0, 1, 6]], dtype=np.float64)
    after = np.array([[0, 0, 0], [0, 6, 1], [0, 0, 7]])
    rep = spatial.report(keys, before, after, 3)
    aa, oa, k = aa_oa_quiet(before)
    assert rep['before'] == dict(OA=oa, AA=aa, kappa=k) and rep['after']['OA'] == 13 / 14
    assert rep['matrix'] == after.tolist() and rep['n'] == 14 and rep['changed'] == 3
    assert (rep['kind'], rep['radius'], rep['sigma_s'], rep['sigma_r'], rep['iterations']) == ('bilateral', 3, 2.0, 0.1, 1)


# ------------------------------------------------------------------------------------------------ keys and refusals
def test_the_keys_parse_and_refuse():
    from utils import spatial
    neutral = dict(kind=None, radius=2, sigma_s=2.0, sigma_r=0.1, iterations=1, color=False)
    assert spatial.spatial_keys({}) == spatial.spatial_keys({'test': {'spatial': 'none'}, 'color': {'spatial': 0}}) == neutral
    assert spatial.keys_in_use(neutral) == []
    on = spatial.spatial_keys({'test': {'spatial': 'bilateral', 'spatial_radius': 1, 'spatial_sigma_s': 3, 'spatial_sigma_r': '0.05',
                                        'spatial_iterations': 2}, 'color': {'spatial': 1}})
    assert on == dict(kind='bilateral', radius=1, sigma_s=3.0, sigma_r=0.05, iterations=2, color=True)
    assert spatial.keys_in_use(on) == ['test.spatial', 'color.spatial']
    for bad in ({'spatial': 'median'}, {'spatial_radius': 0}, {'spatial_radius': 4}, {'spatial_radius': 1.5}, {'spatial_sigma_s': 0},
                {'spatial_sigma_r': -1}, {'spatial_sigma_r': float('inf')}, {'spatial_iterations': 0}, {'spatial_iterations': True}):
        with pytest.raises(ValueError, match=r'test\.spatial'):
            spatial.spatial_keys({'test': bad})
    with pytest.raises(ValueError, match=r'color\.spatial'):
        spatial.spatial_keys({'test': {'spatial': 'bilateral'}, 'color': {'spatial': 2}})
    with pytest.raises(ValueError, match=r'color\.spatial'):
        spatial.spatial_keys({'color': {'spatial': 1}})                  # nothing regularises the map it would draw


def test_the_shipped_config_documents_the_keys_commented_out():
    import yaml
    text = open(os.path.join(REPO, 'dual-modal-fusion_amd', 'config.yml')).read()
    for key in ('spatial:', 'spatial_radius:', 'spatial_sigma_s:', 'spatial_sigma_r:', 'spatial_iterations:'):
        assert any(ln.strip().startswith('#') and key in ln for ln in text.splitlines()), key
    cfg = yaml.safe_load(text)
    assert 'spatial' not in cfg['test'] and 'spatial' not in cfg['color']


@pytest.mark.parametrize('section,key,val', [('test', 'spatial', 'bilateral')])
def test_tostagesolver_refuses_the_keys_by_name(section, key, val):
    from solver.tostagesolver import toStageSolver
    cfg = {'Categories_Number': 5, 'schedule': {'loss': 'qua_loss', 'optimizer': 'ADAM', 'lr': 1e-3}, section: {key: val}}
    with pytest.raises(ValueError, match=r'%s\.%s is out of scope for toStageSolver' % (section, key)):
        toStageSolver(cfg)


@pytest.mark.parametrize('entry', ['test', 'color'])
def test_data_parallel_runs_refuse_the_keys(entry):
    from solver.mainsolver import Solver
    from utils import calibration as cal
    from utils import spatial
    s = Solver.__new__(Solver)
    s.calib, s.world = cal.calibration_keys({}), 2
    s.spat = spatial.spatial_keys({'test': {'spatial': 'bilateral'}})
    with pytest.raises(ValueError, match=r'test\.spatial is out of scope for data-parallel runs \(2 ranks\)'):
        getattr(s, entry)()
    s.spat = spatial.spatial_keys({})
    s._spatial_scope()                                       # neutral keys: nothing to refuse


def test_the_library_declares_and_exports_the_entry_points():
    import ctypes
    from dmf import lib
    hdr = open(os.path.join(REPO, 'include', 'dmf.h')).read()
    so = ctypes.CDLL(lib.LIB_PATH)
    for name in ('dmf_prob_scatter', 'dmf_spatial_affinity', 'dmf_spatial_filter'):
        assert name + '(' in hdr and name in lib.EXPORTS and hasattr(so, name), name
    assert 'dmf_spatial.hip' in open(os.path.join(REPO, 'dual-modal-fusion_amd', 'build.py')).read()


# ------------------------------------------------------------------------------------------------ guards of the GPU cases
@pytest.mark.parametrize('r', S.RADII)
def test_guards_of_the_filter_cases(r):
    worst_margin, changed, classes = 0.0, [], []
    for H, W, K in S.FILTER_CASES:
        aff, prob, mask = _case(H, W, K, r)
        out, pred = R.filter_once(prob, mask, aff, r)
        live = mask != 0
        if not live.any():
            continue
        share = float((R.top2_margin(out)[live] <= MARGIN).mean())
        worst_margin = max(worst_margin, share)
        assert share <= MARGIN_CAP, (H, W, K, r, share)
        if H * W >= S.GUARD_MIN_PIXELS and K >= 3:
            moved = float((pred[live] != prob.argmax(2)[live]).mean())
            changed.append(moved)
            classes.append(len(np.unique(pred[live])))
            assert classes[-1] >= 3 and moved >= 0.10, (H, W, K, r, classes[-1], moved)
    print('r = %d: largest margin share %.4f; changed share %.2f .. %.2f; classes %d .. %d'
          % (r, worst_margin, min(changed), max(changed), min(classes), max(classes)))


def test_the_case_tables_and_generators():
    """13 x 9 (the end-to-end case) lies in the table above; the affinity cases cover every size, band count and type."""
    assert (13, 9) in S.SIZES and len(S.AFFINITY_CASES) == len(S.SIZES) * (len(S.BANDS_F32) + len(S.BANDS_F16))
    for H, W in S.SIZES:
        m = S.mask(H, W)
        assert m.shape == (H, W) and (H * W < 50 or 0.8 <= m.mean() <= 0.97)
    a = S.scene(35, 34, 200)
    assert a.dtype == np.float32 and a.min() == 0.0 and a.max() == 1.0 and S.scene(35, 34, 8, True).dtype == np.float16
