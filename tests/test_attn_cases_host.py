"""CPU: the guards of tests/attn_cases.py for every case tests/test_gpu_attn_sharp.py asks for, on the oracle alone, with the
numbers they measured printed per case (pytest -s; kept in profiles/attn_sharp.md).  This is the record that the inputs can tell
a wrong attention backward from a right one: guards 3 and 4 assert that a backward without the softmax backward, and one with
two heads exchanged, miss the gradient tolerance by more than 10 x in at least 10 elements of each tensor they name.  No GPU,
nothing of the HIP library."""
import pytest
import torch

import attn_cases as ac
import parity_cases as pc


@pytest.mark.parametrize('name,B', ac.all_cases(), ids=lambda v: str(v))
def test_case_guards(name, B):
    try:
        c = ac.case(name, B)                 # asserts the guards
        print()
        for line in ac.report(c):
            print(line)
        assert all(torch.equal(v, c['ref'].state_dict()[k]) for k, v in c['state'].items())
        assert c['logits'].shape == (B, c['K']) and c['a'].shape[0] == B
        if c['train']:
            assert set(c['grads']) == set(c['dl_grads']) == set(c['state']) - {'pool_w'}
            assert c['dl'].shape == (B, c['K']) and c['loss'].shape == (B,)
            assert all(p.grad is None or not p.grad.any() for p in c['ref'].parameters()), 'the oracle is left unchanged'
    finally:
        ac.case.cache_clear()


def test_scene_case_guards():
    c = ac.scene_case()
    assert len({tuple(p) for p in c['xy'].tolist()}) == c['B'] == 513
    print('\n%s: fp32-attention gap %.2e; %.1f %% rows within the margin' % (c['what'], c['fp32_gap'], 100 * c['close']))
    ac.scene_case.cache_clear()


@pytest.mark.parametrize('name', ['tiny1', 'hsi'])
def test_restated_attention_is_the_oracles(name):
    """attn_cases.attention, which guards 3 and 5 differentiate, is oracle.gmfnet_ref.Net.attention bit for bit in float32:
    the same logits and the same gradients."""
    cfg, ref = ac.sharp_net(name)
    a, b, t = ac.rand_batch(name, 3)
    want = pc.head_pass(ref, a, b)[3]
    want_g = ac._grads(ref, torch.nn.functional.cross_entropy(want, t))
    got = ac.restated_pass(ref, a, b)[1]
    got_g = ac._grads(ref, torch.nn.functional.cross_entropy(got, t))
    assert torch.equal(got, want)
    for k in want_g:
        assert torch.equal(got_g[k], want_g[k]), k


def test_sharp_net_is_the_usual_recipe_with_scaled_heads():
    cfg, ref = ac.sharp_net('tiny1')
    base = pc.oracle_net(pc.build_cfg('tiny1', attention=True))
    for k, v in base.state_dict().items():
        w = ref.state_dict()[k]
        if k in ('attn_wq', 'attn_wk'):
            for h, f in enumerate(ac.FACTORS_DEFAULT):
                assert torch.equal(w[32 * h:32 * h + 32], v[32 * h:32 * h + 32] * f)
        else:
            assert torch.equal(w, v)


def test_tables_are_what_the_gpu_tests_walk():
    assert {B for n, B in ac.TRAIN if n == 'tiny1'} == {2, 70, 257, 513} and {B for n, B in ac.TRAIN if n == 'hsi'} == {2, 33, 257}
    assert {B for n, B in ac.FORWARD if n == 'tiny1'} == {1, 513, 1025} and {B for n, B in ac.FORWARD if n == 'hsi'} == {1, 33}
    assert set(ac.STALE) <= set(ac.TRAIN) and ac.SCENE_FORWARD in ac.FORWARD


def test_tolerance_is_never_looser_than_the_flat_one():
    for peak in (1e-6, 2e-4, 2e-2, 1.0):
        assert ac.grad_atol(torch.tensor([peak, -peak / 3])) == min(2e-5, 1e-3 * torch.tensor(peak).item())


def test_split_attention_has_the_oracles_forward():
    cfg, ref = ac.sharp_net('tiny1')
    a, b, t = ac.rand_batch('tiny1', 3)
    with torch.no_grad():
        ya, yb = ref.branches(a, b)
        assert torch.equal(ac.attention_split(ref, ya, yb), ref.attention(ya, yb))
    g = torch.randn(1000, generator=torch.Generator().manual_seed(0)) * 1e-3
    assert ((ac.split_hi_lo(g) - g).abs() <= g.abs() * 2.0 ** -16).all()


def test_engine_steps_reference_experiment():
    """The experiment that sets tests/test_gpu_attn_sharp.py::test_sharp_engine_steps_parameters' bound, on the reference alone:
    the oracle whose q/k backward takes its gradient operands through the kernel's hi/lo bf16 split moves its parameters, after
    three Adam steps at lr 1e-2, by a 99th percentile of 4.8e-4 on the sharp net (above the 2e-4 of the flat net's engine test)
    and of 6e-5 on the usual flat one.  The GPU test's bound is 4 x attn_cases.ENGINE_SPLIT_P99; asserted here: the experiment
    gives no less than ENGINE_SPLIT_P99, so that bound is at most 4 x what the split moves the reference.
    Eight channels of the auxiliary branch are constant over a tiny1 patch (std 0 over its 25 tokens); they cancel in
    dWk = dK^T Tb, since every row of dS sums to zero, so 8 x 96 elements of attn_wk's gradient, 3.5 % of the net's parameters,
    are rounding noise of ~1e-10 around zero in the oracle as in the kernel, and Adam's g / (|g| + 1e-8) turns a difference of
    1e-9 there into a step of 0.1 lr.  The noise grows with the size of dS, hence with the sharpness."""
    for what, factors in (('flat', (1, 1, 1)), ('sharp', ac.FACTORS_DEFAULT)):
        steps, loss, tiny = ac.split_experiment(factors)
        print('\n%s net, oracle against oracle with the hi/lo split: worst loss difference %.2e; %d of 3840 attn_wk gradient '
              'elements are not zero and below 1e-8' % (what, loss, tiny))
        for i, (p99, worst, n) in enumerate(steps):
            print('  after step %d: 99th percentile %.2e, maximum %.2e, %d elements above %g' % (i + 1, p99, worst, n, ac.ENGINE_P99_FLAT))
        assert loss < ac.ENGINE_LOSS_TOL / 4
        assert tiny > 0.01 * 21949, 'more than 1 % of the parameters: a 99th percentile sees them'
        if what == 'flat':
            assert steps[-1][0] < ac.ENGINE_P99_FLAT / 2
        else:
            print('  bound of the GPU test: 4 x %.2e = %.2e' % (ac.ENGINE_SPLIT_P99, ac.ENGINE_P99))
            assert ac.ENGINE_P99 == 4 * ac.ENGINE_SPLIT_P99
            assert steps[-1][0] >= ac.ENGINE_SPLIT_P99, 'the GPU test\'s bound is wider than 4 x this experiment: lower ENGINE_SPLIT_P99'
