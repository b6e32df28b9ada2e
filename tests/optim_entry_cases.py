"""Seeded cases for the flat-gradient optimiser entry points (dmf_adam_step, dmf_sgd_step, dmf_rmsprop_step, dmf_unscale_adam)
and the bytes they leave behind: shared by tests/test_gpu_optim_entry_points.py and the recorder below.  A plain module: no
fixtures, and only `lib.*` wrappers that exist on both sides of the fold of these entry points onto optim_step_kernel.

    python tests/optim_entry_cases.py record FILE

runs every case on cuda:0 and writes, per case, the SHA-256 of the bytes of theta, m, v, grad, the scaler state, the step count
and the cursor after the call, and of theta before it.  tests/golden/g11_optim_entry_bits.json is that file as the commit
BEFORE the fold wrote it on an MI355X (its own tree and library, this module copied into its tests/): the stand-alone kernels'
bits.  It is evidence about that commit and is not re-recorded.

Sizes: 255 (one partial block), 257 (two blocks, the second with one element: the ticket sees more than one block), 8,009 (the
net).  Every scale in the named cases is a power of two, so a product with it is exact; the `_third` cases repeat three of them
with grad_scale 1/3, where g = grad * grad_scale rounds and a build that fused that product into the update would show.  The
`optim_` cases are dmf_optim_step itself with its keys on: the kernel the entry points now share must not have moved either.
"""
import hashlib
import json
import os
import sys
import zlib

import torch

SIZES = (255, 257, 8009)
DEV = 'cuda:0'
ADAM = (1e-3, 0.9, 0.999, 1e-8)          # lr, beta1, beta2, eps
SCALER = (2.0, 0.5, 3)                   # growth factor, backoff factor, growth interval
STEP, CURSOR = 6, 3
FIELDS = ('theta', 'm', 'v', 'grad', 'state', 'step', 'cursor')
# name -> (entry point, what the case is about)
CASES = {
    'adam_host_step': ('adam_step', 'host step 6, grad_scale 0.5'),
    'adam_step_dev': ('adam_step', 'adam_step_dev = 6 with a cursor'),
    'sgd_plain': ('sgd_step', 'momentum 0, NULL buffer'),
    'sgd_momentum_step1': ('sgd_step', 'momentum 0.9, step 1: the buffer becomes g'),
    'sgd_momentum_step2': ('sgd_step', 'momentum 0.9, step 2'),
    'sgd_step_dev': ('sgd_step', 'momentum 0.9, step_dev = 6 with a cursor, grad_scale 0.5'),
    'rmsprop': ('rmsprop_step', 'alpha 0.9 with a cursor'),
    'unscale_finite': ('unscale_adam', 'unscaled = 0, finite gradient'),
    'unscale_grows': ('unscale_adam', 'unscaled = 0, tracker one short of the interval: the scale grows'),
    'unscale_nan': ('unscale_adam', 'unscaled = 0, one NaN element: the step is skipped'),
    'unscaled_flag0': ('unscale_adam', 'unscaled = 1, state[2] = 0'),
    'unscaled_flag1': ('unscale_adam', 'unscaled = 1, state[2] = 1 on a finite gradient: the flag alone skips the step'),
    'adam_third': ('adam_step', 'host step 6, grad_scale 1/3'),
    'sgd_third': ('sgd_step', 'momentum 0.9, step 2, grad_scale 1/3'),
    'rmsprop_third': ('rmsprop_step', 'alpha 0.9, grad_scale 1/3'),
    'optim_adamw_wd_clip': ('optim_step', 'ADAMW, weight decay 0.01, clipped to half the norm, grad_scale 0.5'),
    'optim_sgd_wd_clip': ('optim_step', 'SGD momentum 0.9, weight decay 0.01, clipped, step 2'),
    'optim_rmsprop_wd_clip': ('optim_step', 'RMSprop, weight decay 0.01, clipped'),
    'optim_adam_scaler_clip': ('optim_step', 'ADAM under the scaler (unscaled = 0), weight decay 0.01, clipped'),
}
SKIPPED = ('unscale_nan', 'unscaled_flag1')          # theta, m and v must come back untouched
IDS = [(name, n) for name in CASES for n in SIZES]


def key(case):
    return '%s-%d' % case


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def inputs(case):
    """theta, grad, m (signed: ADAM's first moment, SGD's buffer), v (positive: ADAM's second moment, RMSprop's square_avg)."""
    name, n = case
    g = torch.Generator().manual_seed(zlib.crc32(key(case).encode()))
    return (torch.randn(n, generator=g), torch.randn(n, generator=g), 0.5 * torch.randn(n, generator=g),
            torch.rand(n, generator=g) + 0.01)


def run_case(lib, case):
    """Run one case on the GPU; {field: sha256 of its bytes after the call} plus 'theta_in'."""
    name, n = case
    theta, grad, m, v = inputs(case)
    out = {'theta_in': sha(theta)}
    tracker, flag = (2.0 if name == 'unscale_grows' else 0.0), (1.0 if name == 'unscaled_flag1' else 0.0)
    if name == 'optim_adam_scaler_clip' or CASES[name][0] == 'unscale_adam':
        grad = grad * 256.0                                   # a loss-scaled gradient, scale 256
        if name == 'unscale_nan':
            grad[n // 2] = float('nan')
    th, gd, md, vd = (t.to(DEV) for t in (theta, grad, m, v))
    state = torch.tensor([256.0, tracker, flag, 1.0, 0.0, 0.0, 0.0, 0.0], device=DEV)
    step = torch.full((1,), STEP, dtype=torch.int32, device=DEV)
    cursor = torch.full((1,), CURSOR, dtype=torch.int32, device=DEV)
    if name == 'adam_host_step':
        lib.adam_step(th, gd, md, vd, *ADAM, STEP, grad_scale=0.5)
    elif name == 'adam_third':
        lib.adam_step(th, gd, md, vd, *ADAM, STEP, grad_scale=1.0 / 3.0)
    elif name == 'adam_step_dev':
        lib.adam_step(th, gd, md, vd, *ADAM, 0, adam_step_dev=step, cursor_dev=cursor)
    elif name == 'sgd_plain':
        lib.sgd_step(th, gd, None, 0.05, 0.0, 1)
    elif name == 'sgd_momentum_step1':
        lib.sgd_step(th, gd, md, 0.05, 0.9, 1)
    elif name == 'sgd_momentum_step2':
        lib.sgd_step(th, gd, md, 0.05, 0.9, 2)
    elif name == 'sgd_third':
        lib.sgd_step(th, gd, md, 0.05, 0.9, 2, grad_scale=1.0 / 3.0)
    elif name == 'sgd_step_dev':
        lib.sgd_step(th, gd, md, 0.05, 0.9, 0, grad_scale=0.5, step_dev=step, cursor_dev=cursor)
    elif name == 'rmsprop':
        lib.rmsprop_step(th, gd, vd, 2e-3, 0.9, cursor_dev=cursor)
    elif name == 'rmsprop_third':
        lib.rmsprop_step(th, gd, vd, 2e-3, 0.9, grad_scale=1.0 / 3.0)
    elif CASES[name][0] == 'optim_step':
        reg = dict(weight_decay=0.01, max_norm=0.5 * float((0.5 * inputs(case)[1]).norm()), grad_scale=0.5, cursor_dev=cursor)
        if name == 'optim_adamw_wd_clip':
            lib.optim_step('ADAMW', th, gd, md, vd, *ADAM, step=STEP, **reg)
        elif name == 'optim_sgd_wd_clip':
            lib.optim_step('SGD', th, gd, md, None, 0.05, momentum=0.9, step=2, **reg)
        elif name == 'optim_rmsprop_wd_clip':
            lib.optim_step('RMSprop', th, gd, vd, None, 2e-3, alpha=0.9, step=1, **reg)
        else:
            lib.optim_step('ADAM', th, gd, md, vd, *ADAM, step_dev=step, scaler_state=state, scaler_hparams=SCALER, **reg)
    else:                                                     # (unscaled = 1: the product with grad_scale is skipped too)
        lib.unscale_adam(th, gd, md, vd, *ADAM, state, *SCALER, step, grad_scale=0.5, cursor_dev=cursor,
                         unscaled=name.startswith('unscaled_'))
    torch.cuda.synchronize()
    out.update(zip(FIELDS, (sha(t) for t in (th, md, vd, gd, state, step, cursor))))
    return out


def record(path):
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.join(os.path.dirname(here), 'dual-modal-fusion_amd')]
    from dmf import lib
    res = {'lib_version': lib.version(), 'device': torch.cuda.get_device_name(0), 'cases': {key(c): run_case(lib, c) for c in IDS}}
    with open(path, 'w') as f:
        json.dump(res, f, indent=0, sort_keys=True)
        f.write('\n')
    print('recorded %d cases to %s' % (len(IDS), path))


if __name__ == '__main__':
    if len(sys.argv) != 3 or sys.argv[1] != 'record':
        raise SystemExit(__doc__)
    record(sys.argv[2])
