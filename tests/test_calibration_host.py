"""CPU: calibrated confidence as far as the host decides it — header, lib.py and the library agree on the five
new symbols; what the entry points refuse before any launch; utils/calibration.py on hand-made histograms; the config keys and
the two refusals (stage 2, data-parallel runs); and the guards of the GPU cases of tests/test_gpu_calibration.py, checked on the
float64 reference alone (tests/calib_ref.py)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import calib_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('dmf_softmax_stats', 'dmf_calib_accum', 'dmf_temperature_init', 'dmf_temperature_step', 'dmf_temperature_workspace_bytes')
_BUF = C.create_string_buffer(256)
P = C.c_void_p(C.addressof(_BUF))          # a non-null pointer that no row dereferences
NULL = None


def test_header_binding_and_library_agree_on_the_new_symbols():
    from dmf import lib
    hdr = open(os.path.join(REPO, 'include', 'dmf.h')).read()
    declared = set(re.findall(r'\b(dmf_[a-z0-9_]+)\s*\(', hdr))
    so = C.CDLL(lib.LIB_PATH)
    for name in SYMBOLS:
        assert name in declared and name in lib.EXPORTS and hasattr(so, name), name
    assert re.search(r'#define DMF_TEMP_DOUBLES 8\b', hdr) and lib.TEMP_DOUBLES == 8
    assert lib.version() == 307                              # new symbols are found by name, the version stays


# ------------------------------------------------------------------------------------------------------------- refusals
def _stats(logits=P, B=4, K=17, inv_temp=NULL, xy=NULL, W=0, pred=P, conf=NULL, margin=NULL, entropy=NULL):
    from dmf import lib
    return lib._lib.dmf_softmax_stats(logits, B, K, inv_temp, xy, W, pred, conf, margin, entropy, NULL)


def _accum(conf=P, pred=P, target=P, B=4, K=17, nbins=15, hist=P):
    from dmf import lib
    return lib._lib.dmf_calib_accum(conf, pred, target, B, K, nbins, hist, NULL)


def _step(logits=P, labels=P, N=4, K=17, state=P, ws=P):
    from dmf import lib
    return lib._lib.dmf_temperature_step(logits, labels, N, K, state, ws, 1, NULL)


def _init(state):
    from dmf import lib
    return lib._lib.dmf_temperature_init(state, NULL)


REFUSALS = [
    ('stats_null_logits', lambda: _stats(logits=NULL), 'softmax_stats: null logits'),
    ('stats_negative_B', lambda: _stats(B=-1), 'softmax_stats: negative B'),
    ('stats_K0', lambda: _stats(K=0), 'softmax_stats: 1 <= K <= DMF_KMAX'),
    ('stats_K65', lambda: _stats(K=65), 'softmax_stats: 1 <= K <= DMF_KMAX'),
    ('stats_xy_W0', lambda: _stats(xy=P, W=0), 'softmax_stats: xy needs W >= 1'),
    ('stats_no_output', lambda: _stats(pred=NULL), 'softmax_stats: every output is NULL'),
    ('accum_null', lambda: _accum(hist=NULL), 'calib_accum: null argument'),
    ('accum_nbins0', lambda: _accum(nbins=0), 'calib_accum: 1 <= nbins <= 1024'),
    ('accum_nbins1025', lambda: _accum(nbins=1025), 'calib_accum: 1 <= nbins <= 1024'),
    ('accum_negative_B', lambda: _accum(B=-1), 'calib_accum: negative B'),
    ('init_null', lambda: _init(NULL), 'temperature_init: null state'),
    ('step_null_labels', lambda: _step(labels=NULL), 'temperature_step: null logits, labels or state'),
    ('step_N0', lambda: _step(N=0), 'temperature_step: N must be positive'),
    ('step_K65', lambda: _step(K=65), 'temperature_step: 1 <= K <= DMF_KMAX'),
    ('step_null_workspace', lambda: _step(ws=NULL), 'temperature_step: null workspace'),
]


@pytest.mark.parametrize('name,call,message', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusal_before_any_launch(name, call, message):
    from dmf import lib
    assert call() == 1
    assert lib._lib.dmf_last_error().decode() == message


def test_empty_batches_and_the_workspace_size():
    from dmf import lib
    assert _stats(B=0) == 0 and _accum(B=0) == 0
    size = lib._lib.dmf_temperature_workspace_bytes
    assert [size(n) for n in (0, 1, 256, 257, 1000)] == [0, 24, 24, 48, 96] and size(-1) == -1


# ------------------------------------------------------------------------------------------- utils/calibration.py by hand
def _fixed(conf, n):
    return int(round(conf * 2 ** 32)) * n


def test_a_perfectly_calibrated_histogram_has_no_error():
    from utils import calibration as cal
    # confidences 0.25, 0.5, 0.75, 1.0 (exact in binary): 1 of 4, 2 of 4, 6 of 8 and 5 of 5 rows hit
    hist = [[4, 1, _fixed(0.25, 4)], [4, 2, _fixed(0.5, 4)], [8, 6, _fixed(0.75, 8)], [5, 5, _fixed(1.0, 5)]]
    assert cal.ece_mce(hist) == (0.0, 0.0)
    block = cal.summary(hist, nll_sum=10.5, temperature=2.0)
    assert (block['n'], block['bins'], block['ece'], block['mce'], block['nll'], block['temperature']) == (21, 4, 0.0, 0.0, 0.5, 2.0)
    assert block['hist'] == hist and R.ece_mce(hist) == (0.0, 0.0)


def test_a_single_bin_and_a_known_gap():
    from utils import calibration as cal
    one = [[10, 7, _fixed(0.875, 10)]]
    ece, mce = cal.ece_mce(one)
    assert ece == mce == abs(0.7 - 0.875)
    # two bins: gaps 0.25 (4 rows) and 0.125 (12 rows) -> ECE = (4 * 0.25 + 12 * 0.125) / 16, MCE = 0.25; an empty bin between
    two = [[4, 2, _fixed(0.25, 4)], [0, 0, 0], [12, 12, _fixed(0.875, 12)]]
    assert cal.ece_mce(two) == ((4 * 0.25 + 12 * 0.125) / 16, 0.25) == R.ece_mce(two)


def test_the_empty_histogram():
    from utils import calibration as cal
    empty = np.zeros((15, 3), dtype=np.int64)
    assert cal.ece_mce(empty) == (0.0, 0.0) == R.ece_mce(empty)
    block = cal.summary(empty, 0.0, 1.0)
    assert block['n'] == 0 and block['nll'] == 0.0 and block['bins'] == 15


def test_the_drop_in_statistics_and_fit_are_the_reference_ones():
    """utils.calibration's torch / host forms against tests/calib_ref.py: the same definitions, stated twice."""
    import torch
    from utils import calibration as cal
    logits = R.stats_logits(17, 63, 1.0)
    pred, st = cal.softmax_stats(torch.from_numpy(logits), 0.5)
    rp, rc, rm, re_ = R.stats(logits, 0.5)
    assert np.array_equal(pred.numpy(), rp)
    assert np.abs(st.numpy() - np.stack([rc, rm, re_])).max() <= 1e-14
    ties, first, tied = R.tie_logits(17)
    pred, st = cal.softmax_stats(torch.from_numpy(ties), 3.0)
    assert np.array_equal(pred.numpy(), first) and np.array_equal(st[1].numpy() == 0.0, tied)
    conf = rc.astype(np.float32)
    target = np.where(np.arange(63) % 7 == 0, 99, rp ^ (np.arange(63) % 3 == 0))
    assert np.array_equal(cal.histogram(conf, rp, target, 17, 10), R.histogram(conf, rp, target, 17, 10))
    lg, y = R.fit_case('over', 257, 17)
    f, r = cal.fit_temperature(lg, y), R.fit(lg, y)
    assert abs(f['beta'] - r['beta']) <= 1e-12 * r['beta'] and f['steps'] == r['steps'] == 40


# ------------------------------------------------------------------------------------------------------ keys and refusals
def _keys(test=None, color=None):
    from utils import calibration as cal
    return cal.calibration_keys({'test': test, 'color': color})


def test_the_keys_are_optional_and_neutral_by_default():
    neutral = dict(calibration=False, bins=15, temperature=None, confidence=False)
    assert _keys() == _keys({}, {}) == _keys({'calibration': 0, 'temperature': 'none'}, {'confidence': 0}) == neutral
    assert _keys({'calibration': 1, 'calibration_bins': 10, 'temperature': 'fit'}, {'confidence': 1}) == \
        dict(calibration=True, bins=10, temperature='fit', confidence=True)
    assert _keys({'temperature': 1.5})['temperature'] == 1.5 and _keys({'temperature': '2'})['temperature'] == 2.0
    for bad in ({'calibration': 2}, {'calibration_bins': 0}, {'calibration_bins': 1025}, {'calibration_bins': 2.5},
                {'temperature': 0}, {'temperature': -1.0}, {'temperature': 'auto'}, {'temperature': float('inf')}):
        with pytest.raises(ValueError, match=r'test\.'):
            _keys(bad)
    with pytest.raises(ValueError, match=r'color\.confidence'):
        _keys({}, {'confidence': 3})


def test_the_shipped_config_documents_the_keys_commented_out():
    import yaml
    text = open(os.path.join(REPO, 'dual-modal-fusion_amd', 'config.yml')).read()
    for key, default in (('calibration', '0'), ('calibration_bins', '15'), ('temperature', 'none'), ('confidence', '0')):
        assert '  # %s: %s' % (key, default) in text
    cfg = yaml.safe_load(text)
    assert 'calibration' not in cfg['test'] and 'confidence' not in cfg['color']


@pytest.mark.parametrize('section,key,val', [('test', 'calibration', 1), ('test', 'temperature', 'fit'), ('color', 'confidence', 1)])
def test_tostagesolver_refuses_the_keys_by_name(section, key, val):
    from solver.tostagesolver import toStageSolver
    cfg = {'Categories_Number': 5, 'schedule': {'loss': 'qua_loss', 'optimizer': 'ADAM', 'lr': 1e-3}, section: {key: val}}
    with pytest.raises(ValueError, match=r'%s\.%s is out of scope for toStageSolver' % (section, key)):
        toStageSolver(cfg)


@pytest.mark.parametrize('entry', ['test', 'color'])
def test_data_parallel_runs_refuse_the_keys(entry):
    from solver.mainsolver import Solver
    from utils import calibration as cal
    s = Solver.__new__(Solver)
    s.calib, s.world = cal.calibration_keys({'test': {'calibration': 1}}), 2
    with pytest.raises(ValueError, match=r'test\.calibration is out of scope for data-parallel runs \(2 ranks\)'):
        getattr(s, entry)()
    s.calib = cal.calibration_keys({})
    s._calibration_scope()                                   # neutral keys: nothing to refuse


# ------------------------------------------------------------------------------------ guards of the GPU cases (reference only)
@pytest.mark.parametrize('K', R.FIT_K)
@pytest.mark.parametrize('N', R.FIT_N)
@pytest.mark.parametrize('kind', R.FIT_KINDS)
def test_fit_cases_end_where_they_are_said_to(kind, N, K):
    lg, y = R.fit_case(kind, N, K)
    st = R.fit(lg, y)
    where = R.fit_expect(kind, N, K)
    _, g, h = R.nll_terms(lg, y, st['beta'])
    print('%s N=%d K=%d: beta %.15g in [%.15g, %.15g], g %.3e, h %.3e' % (kind, N, K, st['beta'], st['lo'], st['hi'], g, h))
    if where == 'interior':
        assert 2.0 ** -6 < st['beta'] < 2.0 ** 6                                   # strictly inside the bracket it started with
        assert st['lo'] <= st['beta'] <= st['hi']                                  # (a converged bracket is two neighbouring doubles)
        assert abs(g) <= 1e-9 * h * st['beta']
        if kind == 'over' and N > 1:
            assert 0.1 < st['beta'] < 0.4                                          # calibrated logits x 5
    else:
        end = 2.0 ** 6 if where == 'hi' else 2.0 ** -6
        assert abs(st['beta'] - end) <= 1e-9 * end
        assert (st['hi'] == 2.0 ** 6) if where == 'hi' else (st['lo'] == 2.0 ** -6)  # that end never moved


def test_stats_cases_have_no_near_ties_but_the_deliberate_ones():
    for K in R.STATS_K:
        for B in R.STATS_B:
            for scale in R.STATS_SCALE:
                l = np.sort(R.stats_logits(K, B, scale).astype(np.float64), 1)
                assert K == 1 or np.diff(l, axis=1).min() >= 1e-3, (K, B, scale)
    for K in R.TIE_K:
        rows, first, tied = R.tie_logits(K)
        top = np.sort(rows.astype(np.float64), 1)[:, ::-1]
        assert np.array_equal(top[:, 0] == top[:, 1], tied) and np.array_equal(rows.argmax(1), first)
        assert (rows[2] == rows[2, 0]).all() and (rows[1] == rows[1].max()).sum() == 3


# ------------------------------------------------------------------------------------ the drop-in evaluation, end to end on the CPU
def test_the_drop_in_test_and_color_leave_the_recorded_artefacts_and_rng_state(golden_dir, tmp_path):
    """`test()` + `color()` with fast_path: 0 and every evaluation key on (tests/dropin_eval_case.py) against what the commit
    named in tests/golden/g13_dropin_eval.npz left (tools/record_eval_fixtures.py dropin): the decoded artefacts, and torch's
    RNG state afterwards — exactly: it moves with every loader that is iterated, and this path has no GPU test."""
    import dropin_eval_case as D
    got = D.outputs(golden_dir, str(tmp_path))
    g = np.load(os.path.join(golden_dir, 'g13_dropin_eval.npz'), allow_pickle=False)
    assert sorted(got) == sorted(k for k in g.files if k != 'recorded_from')
    assert got['files'].tolist() == g['files'].tolist()
    assert got['rng_state'].tobytes() == g['rng_state'].tobytes()
    for name in D.TEXTS:
        assert json.loads(str(got[name])) == json.loads(str(g[name])), name
    for name in ('test_matrix',) + D.IMAGES + D.ARRAYS:
        assert got[name].dtype == g[name].dtype and got[name].shape == g[name].shape and np.array_equal(got[name], g[name]), name
