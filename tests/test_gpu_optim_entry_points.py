"""dmf_adam_step, dmf_sgd_step, dmf_rmsprop_step and dmf_unscale_adam leave the bytes their stand-alone kernels left.

All four launch optim_step_kernel now, so comparing them with dmf_optim_step on the GPU compares a kernel with
itself.  tests/golden/g11_optim_entry_bits.json holds what the commit before the fold wrote for the cases of
tests/optim_entry_cases.py on an MI355X, as SHA-256 of the bytes of theta, m, v, grad, the scaler state, the step count and the
cursor: the GPU test asserts every one of them.  A mismatch means a product is fused or unfused differently (or a rule of the
step's end changed): write the form out with fmaf under `#pragma clang fp contract(off)`; the golden is not re-recorded.

The guards on the golden file itself need no GPU.
"""
import json
import os

import pytest

import optim_entry_cases as oc


@pytest.fixture(scope='module')
def golden(golden_dir):
    with open(os.path.join(golden_dir, 'g11_optim_entry_bits.json')) as f:
        return json.load(f)['cases']


def test_golden_holds_every_case_and_field(golden):
    assert sorted(golden) == sorted(oc.key(c) for c in oc.IDS)
    for k, h in golden.items():
        assert sorted(h) == sorted(oc.FIELDS + ('theta_in',)), k
        assert all(len(v) == 64 for v in h.values()), k


def test_golden_theta_moved_unless_the_step_was_skipped(golden):
    for name, n in oc.IDS:
        h = golden[oc.key((name, n))]
        assert (h['theta'] == h['theta_in']) == (name in oc.SKIPPED), (name, n)


def test_golden_sgd_first_and_second_step_differ(golden):
    for n in oc.SIZES:
        one, two = golden['sgd_momentum_step1-%d' % n], golden['sgd_momentum_step2-%d' % n]
        assert one['theta'] != two['theta'] and one['m'] != two['m'], n


def test_golden_inputs_are_the_modules_inputs(golden):
    """The recorded theta_in is the hash of what optim_entry_cases.inputs gives here: the cases have not drifted from the file."""
    for case in oc.IDS:
        assert oc.sha(oc.inputs(case)[0]) == golden[oc.key(case)]['theta_in'], case


@pytest.mark.gpu
@pytest.mark.parametrize('case', oc.IDS, ids=oc.key)
def test_entry_point_reproduces_the_stand_alone_kernels_bits(case, golden):
    from dmf import lib
    got, want = oc.run_case(lib, case), golden[oc.key(case)]
    bad = [f for f in want if got[f] != want[f]]
    assert not bad, '%s (%s): %s differ from the recorded bytes' % (oc.key(case), oc.CASES[case[0]][1], ', '.join(bad))
