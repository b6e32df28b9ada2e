"""CPU: the criterion inside the attention network's train step as far as the host decides it — header, library
and lib.py agree on dmf_ce_denominators / dmf_train_attn_fwd_bwd_ce and the struct dmf_ce_fused; what the two entry points refuse,
with their messages (every call returns before it touches the device: the pointers are NULL or point into a host buffer that is
never read); and the CPU restatement of the denominator's summation order (tests/attn_ce_ref.py) against math.fsum."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import attn_ce_ref
from test_capi_host import ATTN, LATE, NULL, P, inp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- the C ABI
def test_header_library_and_binding_agree():
    """(Fails on a build without the feature: the symbols do not exist.)"""
    from dmf import lib
    hdr = open(os.path.join(REPO, 'include', 'dmf.h')).read()
    for name in ('dmf_ce_denominators', 'dmf_train_attn_fwd_bwd_ce'):
        assert name in lib.EXPORTS and getattr(lib._lib, name) is not None
        assert 'int32_t %s(' % name in hdr
    assert lib.version() == int(re.search(r'#define DMF_VERSION (\d+)', hdr).group(1)) >= 307
    assert ('typedef struct dmf_ce_fused {\n  const dmf_ce_params* params; const float* class_w; const int32_t* labels_global; '
            'const double* denom;\n  int32_t ranks, rank; float grad_scale; int32_t reserved;\n} dmf_ce_fused;') in hdr
    assert C.sizeof(lib.CeFused) == 48
    assert [f[0] for f in lib.CeFused._fields_] == ['params', 'class_w', 'labels_global', 'denom', 'ranks', 'rank', 'grad_scale',
                                                    'reserved']


# ---------------------------------------------------------------------------------------------- refusals
def _denoms(labels=P, N=4, rows=1, K=5, class_w=NULL, denom=P):
    from dmf import lib
    return lib._lib.dmf_ce_denominators(labels, N, rows, K, class_w, denom, NULL)


def _params(kind=0, label_smoothing=0.0, gamma=0.0):
    from dmf import lib
    return lib.CeParams(kind=kind, label_smoothing=label_smoothing, gamma=gamma)


_KEEP = []          # the CeParams a struct points to must outlive the call


def _ce(params='default', class_w=NULL, labels=P, denom=P, ranks=1, rank=0, grad_scale=1.0, reserved=0, **prm):
    from dmf import lib
    p = None
    if params == 'default':
        _KEEP.append(_params(**prm))
        p = C.pointer(_KEEP[-1])
    val = lambda x: None if x is None else x.value
    return C.byref(lib.CeFused(params=p, class_w=val(class_w), labels_global=val(labels), denom=val(denom), ranks=ranks, rank=rank,
                               grad_scale=grad_scale, reserved=reserved))


def _step(ce, s=ATTN, i=None, theta=P, pool=P, logits=P, loss=P, ws=P, aws=P):
    from dmf import lib
    i = inp() if i is None else i
    return lib._lib.dmf_train_attn_fwd_bwd_ce(C.byref(s), C.byref(i), theta, pool, ce, logits, loss, ws, aws, NULL, NULL)


INF, NAN = float('inf'), float('nan')
E = 'dmf_train_attn_fwd_bwd_ce: '
REFUSALS = [
    # dmf_ce_denominators
    ('denominators-null_labels', lambda: _denoms(labels=NULL), 'ce_denominators: null labels or denom'),
    ('denominators-null_denom', lambda: _denoms(denom=NULL), 'ce_denominators: null labels or denom'),
    ('denominators-N_0', lambda: _denoms(N=0), 'ce_denominators: N must be positive and rows >= 0'),
    ('denominators-N_negative', lambda: _denoms(N=-3), 'ce_denominators: N must be positive and rows >= 0'),
    ('denominators-rows_negative', lambda: _denoms(rows=-1), 'ce_denominators: N must be positive and rows >= 0'),
    ('denominators-K_0', lambda: _denoms(K=0), 'ce_denominators: 1 <= K <= DMF_KMAX'),
    ('denominators-K_65', lambda: _denoms(K=65), 'ce_denominators: 1 <= K <= DMF_KMAX'),
    # dmf_train_attn_fwd_bwd_ce: what dmf_train_attn_fwd_bwd refuses
    ('step-null_theta', lambda: _step(_ce(), theta=NULL), 'null argument'),
    ('step-null_pool', lambda: _step(_ce(), pool=NULL), 'null argument'),
    ('step-null_logits', lambda: _step(_ce(), logits=NULL), 'null argument'),
    ('step-null_workspace', lambda: _step(_ce(), ws=NULL), 'null argument'),
    ('step-null_attn_workspace', lambda: _step(_ce(), aws=NULL), 'null argument'),
    ('step-late_fusion', lambda: _step(_ce(), s=LATE), 'dmf_train_attn_fwd_bwd_ce needs shape->attention == 1'),
    ('step-half', lambda: _step(_ce(), i=inp(half=1)), 'fp16 scenes (dmf_input.half): late-fusion network only'),
    # ... its own struct
    ('step-null_struct', lambda: _step(NULL), E + 'null dmf_ce_fused, params, labels_global or denom'),
    ('step-null_params', lambda: _step(_ce(params=None)), E + 'null dmf_ce_fused, params, labels_global or denom'),
    ('step-null_labels', lambda: _step(_ce(labels=NULL)), E + 'null dmf_ce_fused, params, labels_global or denom'),
    ('step-null_denom', lambda: _step(_ce(denom=NULL)), E + 'null dmf_ce_fused, params, labels_global or denom'),
    ('step-reserved', lambda: _step(_ce(reserved=1)), E + 'dmf_ce_fused.reserved must be 0'),
    # ... what dmf_ce_loss refuses
    ('step-ranks_0', lambda: _step(_ce(ranks=0)), E + 'ranks must be positive and 0 <= rank < ranks'),
    ('step-rank_negative', lambda: _step(_ce(ranks=2, rank=-1)), E + 'ranks must be positive and 0 <= rank < ranks'),
    ('step-rank_is_ranks', lambda: _step(_ce(ranks=2, rank=2)), E + 'ranks must be positive and 0 <= rank < ranks'),
    ('step-negative_batch', lambda: _step(_ce(), i=inp(B=-1)), E + 'bs must be positive and 1 <= K <= DMF_KMAX'),
    ('step-batch_too_large', lambda: _step(_ce(ranks=3), i=inp(B=1 << 30)), E + 'the batch is too large'),
    ('step-kind_2', lambda: _step(_ce(kind=2)), E + 'kind must be 0 (cross-entropy) or 1 (focal)'),
    ('step-kind_negative', lambda: _step(_ce(kind=-1)), E + 'kind must be 0 (cross-entropy) or 1 (focal)'),
    ('step-eps_1', lambda: _step(_ce(label_smoothing=1.0)), E + 'label_smoothing must lie in [0, 1)'),
    ('step-eps_negative', lambda: _step(_ce(label_smoothing=-0.1)), E + 'label_smoothing must lie in [0, 1)'),
    ('step-eps_nan', lambda: _step(_ce(label_smoothing=NAN)), E + 'label_smoothing must lie in [0, 1)'),
    ('step-gamma_half', lambda: _step(_ce(kind=1, gamma=0.5)), E + 'gamma must be 0 or >= 1'),
    ('step-gamma_negative', lambda: _step(_ce(kind=1, gamma=-2.0)), E + 'gamma must be 0 or >= 1'),
    ('step-gamma_inf', lambda: _step(_ce(kind=1, gamma=INF)), E + 'gamma must be 0 or >= 1'),
    ('step-gamma_nan', lambda: _step(_ce(kind=1, gamma=NAN)), E + 'gamma must be 0 or >= 1'),
]


@pytest.mark.parametrize('name,call,message', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusal(name, call, message):
    from dmf import lib
    assert call() == 1
    assert lib._lib.dmf_last_error().decode() == message


def test_no_ops():
    """rows == 0 and an empty batch return 0 before anything is looked at."""
    assert _denoms(rows=0) == 0
    assert _step(NULL, i=inp(B=0)) == 0


def test_ce_loss_keeps_its_messages():
    """dmf_ce_loss shares its checks with the new entry point: its own prefix stays."""
    from dmf import lib
    prm = _params(kind=3)
    assert lib._lib.dmf_ce_loss(P, 1, 0, 4, 5, P, NULL, NULL, C.byref(prm), 1.0, NULL, P, P, NULL) == 1
    assert lib._lib.dmf_last_error().decode() == 'ce_loss: kind must be 0 (cross-entropy) or 1 (focal)'


def test_binding_checks_before_the_call():
    from dmf import lib
    import torch
    monkey = lib._dev
    lib._dev = lambda t, dtype, name: t
    try:
        lab, den = torch.zeros(10, dtype=torch.int32), torch.zeros(2, dtype=torch.float64)
        with pytest.raises(lib.DmfError, match='rows of 4 labels'):
            lib.ce_denominators(lab, 4, 5, den)
        with pytest.raises(lib.DmfError, match='one denominator per row'):
            lib.ce_denominators(lab, 2, 5, den)
        with pytest.raises(lib.DmfError, match='one weight per class'):
            lib.ce_denominators(lab, 5, 5, den, class_w=torch.ones(4))
        with pytest.raises(lib.DmfError, match='rank 2 of 2 ranks'):
            lib.train_attn_fwd_bwd_ce(ATTN, inp(), None, None, lab, den, lib.ce_params(), 2, 2, None, None, None, None)
        with pytest.raises(lib.DmfError, match='one label per sample of the global batch'):
            lib.train_attn_fwd_bwd_ce(ATTN, inp(B=6), None, None, lab, den, lib.ce_params(), 2, 0, None, None, None, None)
    finally:
        lib._dev = monkey


# ---------------------------------------------------------------------------------------------- the denominator's order
@pytest.mark.parametrize('weights', (False, True), ids=('ones', 'weights'))
@pytest.mark.parametrize('K', (5, 64))
@pytest.mark.parametrize('N', (1, 255, 256, 257, 1025, 40000))
def test_denominator_restatement_against_fsum(N, K, weights):
    """The strided pass and the 256-leaf tree add N positive float64 terms with at most N - 1 roundings on the way to any leaf's
    share of the result, each relative 2^-53: |D - fsum| <= N 2^-53 fsum."""
    import loss_ref
    import torch
    g = torch.Generator().manual_seed(1000 * K + N)
    y = torch.randint(0, K, (N,), generator=g).numpy()
    w = loss_ref.class_weights(K, g).numpy() if weights else None
    got = attn_ce_ref.denominator(y, K, w)
    exact = math.fsum((np.ones(K) if w is None else w.astype(np.float64))[y].tolist())
    assert abs(got - exact) <= N * 2.0 ** -53 * exact
    if not weights:
        assert got == float(N)
    # labels outside [0, K) are clamped, as the kernels clamp them
    bad = y.copy(); bad[0] = -7; bad[-1] = K + 3
    fix = y.copy(); fix[0] = 0; fix[-1] = K - 1
    assert attn_ce_ref.denominator(bad, K, w) == attn_ce_ref.denominator(fix, K, w)


def test_denominators_rows():
    y = np.arange(12) % 5
    w = np.array([0.5, 1.0, 2.0, 4.0, 8.0], dtype=np.float32)
    d = attn_ce_ref.denominators(y, 4, 5, w)
    assert d.shape == (3,) and d.tolist() == [7.5, 11.5, 13.5]
