"""CPU: the vacuity guards of tests/parity_cases.py for every case tests/test_gpu_batch_walk.py asks for, on the oracle alone —
class diversity, pair separation, margin cap, gradient signal (parity_cases.py states them) — and the recipe's own promises:
distinct coordinates with the scene's corners in front, labels with both ends of the class range.  No GPU, nothing of the HIP
library."""
import pytest
import torch

import parity_cases as pc


def key_id(key):
    return '-'.join(str(k) for k in key)


@pytest.mark.parametrize('key', pc.all_cases(), ids=key_id)
def test_case_guards(key):
    name, B, half, attention = key
    try:
        c = pc.case(*key)                  # asserts the four guards
        xy, t, K = c['xy'], c['labels'], c['K']
        assert xy.shape == (B, 2) and len({tuple(p) for p in xy.tolist()}) == B
        assert xy[0].tolist() == [0, 0] and xy[1].tolist() == [pc.H_SCENE - 1, pc.W_SCENE - 1]
        assert int(xy[:, 0].max()) < pc.H_SCENE and int(xy[:, 1].max()) < pc.W_SCENE and int(xy.min()) >= 0
        assert tuple(c['A'].shape[:2]) == (pc.H_SCENE + c['P'] - 1, pc.W_SCENE + c['P'] - 1)
        assert t[0] == 0 and t[1] == K - 1 and int(t.min()) >= 0 and int(t.max()) < K
        assert c['logits'].mean(0).abs().max().item() < 1e-5, 'the head is centred on the batch'
        # the centred weights are what the HIP net gets: the oracle that made the references holds them
        assert all(torch.equal(v, c['ref'].state_dict()[k]) for k, v in c['state'].items())
        if half:
            A = c['A']
            assert bool((A == 0).any()) and bool(((A != 0) & (A.abs() < 6.1e-5)).any()), 'exact zeros and fp16 subnormals'
        if (name, B, half) in pc.unit_cases() and not attention:
            dl, grads, hv = pc.unit_reference(c)      # asserts the gradient signal of the unit step's reference
            assert dl.shape == (B, K) and torch.equal(hv['dl'][:, :K], dl)
    finally:
        pc.case.cache_clear()              # (the patches of the large shapes: not kept for the rest of the run)


def test_matrix_is_what_the_gpu_tests_walk():
    walk = pc.walk_cases()
    assert {B for n, B, h in walk if n in pc.SMALL} == {255, 256, 257, 511, 512, 513, 769}
    assert {B for n, B, h in walk if n in pc.LARGE} == {257, 513}
    assert {n for n, B, h in walk} == set(pc.SMALL + pc.LARGE) and len(pc.SMALL + pc.LARGE) == 10
    assert {n for n, B, h in walk if h} == set(pc.HALF)
    unit = pc.unit_cases()
    assert {B for n, B, h in unit if n == 'qua'} >= {1023, 1024, 1025, 1281}
    assert ('hsi', 513, True) in unit and ('hsi9', 513, False) in unit and ('hsi9', 513, True) not in unit


def test_stage2_evaluation_case_guards():
    q = pc.qua_eval_case()                # asserts class diversity and the margin cap on the summed logits
    assert len({tuple(p) for p in q['xy'].tolist()}) == q['B'] == pc.WHOLE_SET
    assert q['pair_logits'].mean(0).abs().max().item() < 2e-5
