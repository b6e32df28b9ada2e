"""CPU: the trained-weight parity cases of tests/trained_cases.py hold their guards on the oracle alone, and the fixture they
load is the one tools/record_trained_cases.py writes.  No GPU, nothing of the HIP library.  What the guards measured is
printed per case (profiles/trained_parity.md keeps one run)."""
import numpy as np
import pytest
import torch

import parity_cases as pc
import trained_cases as tc


def test_fixture_names_shapes_and_scene_digests():
    """Exactly the names the tool writes, float32 arrays of the oracle's shapes, the recipe's scalars, and the digest of the
    scene as it is drawn HERE (trained_state asserts it: another numpy stream must not test unguarded inputs)."""
    from oracle.gmfnet_ref import Net as RefNet
    want_w, want_a = {f: set() for f in tc.WEIGHT_FILES}, set()
    assert sorted(n for names in tc.WEIGHT_FILES.values() for n in names) == sorted(tc.RECIPES)
    for name, r in tc.RECIPES.items():
        ref = RefNet(pc.build_cfg(r['row']))
        sd = ref.state_dict()
        w, a = tc.fixture_keys(name, list(sd))
        want_w[tc.weights_file(name)].update(w); want_a.update(a)
        state, adam = tc.trained_state(name)
        assert set(state) == set(sd)
        for k, v in sd.items():
            assert state[k].shape == v.shape and state[k].dtype == torch.float32, (name, k)
            assert bool(torch.isfinite(state[k]).all())
        assert torch.equal(state['pool_w'], sd['pool_w']), 'the pooling profile is the oracle\'s own'
        assert (adam is not None) == (name in tc.ADAM_CASES)
        if adam:
            assert adam['step'] == r['steps']
            for k, p in ref.named_parameters():
                for mv in ('m', 'v'):
                    assert adam[mv][k].shape == p.shape and adam[mv][k].dtype == torch.float32, (name, mv, k)
                assert bool((adam['v'][k] >= 0).all())
    for f, want in want_w.items():
        assert set(tc._npz(f)) == want
    assert set(tc._npz(tc.ADAM)) == want_a
    assert set(tc.HALF_CASES) <= set(tc.RECIPES) and all(tc.row_of(n) in pc.HALF for n in tc.HALF_CASES)


def test_a_scene_of_another_stream_is_refused(monkeypatch):
    z = dict(tc._npz(tc.weights_file('tiny-sharp')))
    z['tiny-sharp/scene_sha256'] = np.str_('0' * 64)
    monkeypatch.setattr(tc, '_npz', lambda fname: z)
    with pytest.raises(AssertionError, match='not the scene'):
        tc.trained_state('tiny-sharp')


def test_the_matrix_is_the_one_the_tests_state():
    cells = tc.cells()
    assert len(cells) == len(set(cells)) == 10
    for name, B, half in cells:
        assert B in ((257, 513) if tc.row_of(name) in ('tiny', 'tiny1') else (33,))
        assert not half or name in tc.HALF_CASES
    assert {n for n, _, h in cells if h} == set(tc.HALF_CASES)
    assert tc.ADAM_CASES == ('tiny1-sharp', 'hsi-sharp')
    for (name, B, half), seed in tc.SEEDS.items():
        assert (name, B, half) in cells and 1 <= seed <= 30


@pytest.mark.parametrize('name,B,half', tc.cells())
def test_guards(name, B, half):
    """Guards 1 .. 6 (asserted inside `case`), and that what the case hands out is what it says."""
    c = tc.case(name, B, half)
    K = c['K']
    print(tc.REPORT_HEAD)
    print(tc.report(c))
    print('  a flat softmax moves, elements beyond 10 x tolerance: ' + ', '.join('%s %d' % kv for kv in c['measured']['flat'].items()))
    assert c['logits'].dtype == torch.float64 and all(g.dtype == torch.float64 for g in c['grads'].values())
    assert c['logit_tol'] >= tc.LOGIT_TOL and c['loss_tol'] >= tc.LOSS_TOL
    # the piecewise pass is the oracle's forward, bit for bit (fp32), and the float64 net is the same net
    with torch.no_grad():
        assert torch.equal(tc.site_pass(c['ref'], c['a'], c['b'])[3], c['ref'](c['a'], c['b']))
    for k, v in c['ref'].state_dict().items():
        assert torch.equal(c['ref64'].state_dict()[k], v.double())
    # coordinates distinct and in the scene; labels in range, not all the scene's own
    assert len({tuple(p) for p in c['xy'].tolist()}) == B
    assert int(c['xy'][:, 0].max()) < pc.H_SCENE and int(c['xy'][:, 1].max()) < pc.W_SCENE and int(c['xy'].min()) >= 0
    assert 0 <= int(c['labels'].min()) and int(c['labels'].max()) < K
    # dl of the cross-entropy route is softmax - onehot over B, rows summing to zero; its padding is zero
    p = torch.softmax(c['logits'], 1)
    p[torch.arange(B), c['labels']] -= 1
    assert torch.allclose(c['dlogits'], p / B, rtol=1e-12, atol=1e-15)
    assert float(c['hv']['dl'][:, K:].abs().max()) == 0.0 and float(c['unit_hv']['dl'][:, K:].abs().max()) == 0.0
    # dh is shut exactly where h is
    assert bool(((c['hv']['h'] > 0) | (c['hv']['dh'] == 0)).all())
    if half:
        # the fp16 rounding is live: the same net without it gives other logits
        from oracle.gmfnet_ref import Net as RefNet
        r32 = RefNet(pc.build_cfg(c['row']))
        r32.load_state_dict(c['state'])
        with torch.no_grad():
            gap = (r32(c['a'], c['b']).double() - c['logits']).abs().max().item()
        print('  half: the fp16 roundings move the logits by %.2e' % gap)
        assert gap > 10 * c['logit_tol']


def test_adam_state_is_a_real_state():
    """The recorded moments are those of a trained net: a never-open unit's parameters with m = v = 0 exist (they keep theta
    bit for bit), and elsewhere v spans orders of magnitude."""
    for name in tc.ADAM_CASES:
        for B in tc.BATCHES[tc.row_of(name)]:
            c = tc.case(name, B, False)
            m, v = c['adam']['m']['fc1.weight'], c['adam']['v']['fc1.weight']
            still = (m == 0) & (v == 0) & (c['grads']['fc1.weight'] == 0)
            rows = int(still.all(1).sum())
            live = v[v > 0]
            print('%s: %d fc1 units with m = v = g = 0; v from %.1e to %.1e' % (c['what'], rows, live.min().item(), live.max().item()))
            assert rows >= 1
            assert live.max().item() / live.min().item() > 1e4
