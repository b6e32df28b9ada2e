"""GPU: the recorded bits of the three row-group kernels (csrc/dmf_rows.h): dmf_softmax_stats, dmf_prob_scatter and
dmf_logits_mean on the rows of tests/row_cases.py — 300 rows at every class count that selects another group size, with exact
ties, +-80 logits and three betas — give, array by array, the bytes they gave at the commit the fixture names
(tests/golden/g12_row_kernels.npz, recorded on the MI355X by tools/record_eval_fixtures.py; it keeps the SHA-256 of every
array's `tobytes()`).  Nothing in the fixture comes from the tree under test."""
import os

import numpy as np
import pytest

import row_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def outputs():
    return C.outputs()


def test_the_fixture_covers_every_output(golden_dir, outputs):
    g = np.load(os.path.join(golden_dir, 'g12_row_kernels.npz'), allow_pickle=False)
    assert int(g['seed']) == C.SEED and g['names'].tolist() == sorted(outputs)
    per_beta = 2 * 4 + 2                                 # flat and map: pred, conf, margin, entropy; prob and mask
    assert len(outputs) == len(C.CLASSES) * (len(C.BETAS) * per_beta + 2 * 3)


def test_every_output_has_the_recorded_bytes(golden_dir, outputs):
    g = np.load(os.path.join(golden_dir, 'g12_row_kernels.npz'), allow_pickle=False)
    want = dict(zip(g['names'].tolist(), g['sha256']))
    moved = [k for k in sorted(outputs) if C.digest(outputs[k]).tobytes() != want[k].tobytes()]
    assert not moved, '%d of %d outputs differ from the bytes recorded at %s: %s' % (
        len(moved), len(outputs), g['recorded_from'], moved[:12])


def test_the_rows_are_what_they_are_said_to_be(outputs):
    """The inputs do pin the first index and do hold e == 0 terms, and what is recorded is not empty: the argmax is numpy's
    (first maximal index), a tie between all columns has margin 0, the scattered maps are the flat rows at their pixels."""
    xy = C.pixels()
    for K in C.CLASSES:
        x = C.logits(K)
        first = x.argmax(1)
        tied = (x == x.max(1, keepdims=True)).sum(1)
        assert K == 1 or ((tied[C.TIES] >= 2).all() and (tied[C.TIES] == K).any() and (tied[:C.TIES.start] == 1).all())
        assert K == 1 or (np.exp(np.float32(2.0) * (x[C.WIDE] - x[C.WIDE].max(1, keepdims=True))) == 0).any()
        for beta in C.BETAS:
            tag = 'K%d.beta%s.' % (K, beta)
            assert np.array_equal(outputs[tag + 'flat.pred'], first)
            assert K == 1 or (outputs[tag + 'flat.margin'][C.TIES] == 0).all()
            for name in ('pred', 'conf', 'margin', 'entropy'):
                m = outputs[tag + 'map.' + name].reshape(C.H, C.W)
                assert m[xy[:, 0], xy[:, 1]].tobytes() == outputs[tag + 'flat.' + name].tobytes()
            assert outputs[tag + 'mask'].sum() == C.B and outputs[tag + 'prob'][xy[:, 0], xy[:, 1], first].tobytes() == \
                outputs[tag + 'flat.conf'].tobytes()
        for V in (1, 3):
            assert np.array_equal(outputs['K%d.V%d.pred' % (K, V)], outputs['K%d.V%d.mean' % (K, V)].argmax(1))
            assert (outputs['K%d.V%d.pred' % (K, V)][C.TIES] == first[C.TIES]).all()
            assert outputs['K%d.V%d.mean' % (K, V)].tobytes() == outputs['K%d.V%d.mean_without_pred' % (K, V)].tobytes()
