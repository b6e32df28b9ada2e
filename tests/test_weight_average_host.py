"""CPU: weight averaging as far as the host decides it — header, library and lib.py agree on the four `_avg`
symbols and version 307; what the entry points refuse; the launch sequence of every step form of both train engines with
averaging on (recorded on CPU tensors by the recorder of tests/test_engine_update_host.py), and that nothing routes there without
it; the first averaged step from `schedule.average_start`; toStageSolver's refusal; and the guard that torch.lerp on this CPU is
the fused form the kernels state (tests/avg_ref.py), which the GPU tests' count of unequal bits relies on."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import avg_ref
from test_capi_host import ATTN, LATE, NULL, P, _BUF, inp
from test_engine_update_host import DQTL, Recorder

P2 = C.c_void_p(C.addressof(_BUF) + 128)        # a second non-null pointer: [P, P + 16) and [P2, P2 + 16) do not overlap
FAR = C.c_void_p(C.addressof(_BUF) + (1 << 26))  # ... and one that no parameter vector starting at P reaches (never dereferenced)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- the C ABI
def test_header_library_and_binding_agree():
    """(Fails on a build without the feature: the symbols do not exist.)"""
    from dmf import lib
    hdr = open(os.path.join(REPO, 'include', 'dmf.h')).read()
    for name in ('dmf_weight_average', 'dmf_optim_step_avg', 'dmf_grad_reduce_adam_avg', 'dmf_train_plan_steps_avg'):
        assert name in lib.EXPORTS and getattr(lib._lib, name) is not None
        assert 'int32_t %s(' % name in hdr
    assert '#define DMF_VERSION 307' in hdr and lib.version() == 307
    assert '#define DMF_AVG_EMA  0' in hdr and '#define DMF_AVG_MEAN 1' in hdr
    assert lib.AVG_KINDS == {'ema': 0, 'mean': 1}
    assert ('typedef struct dmf_weight_avg { float* avg; int32_t kind; float weight; int32_t start; int32_t reserved; } '
            'dmf_weight_avg;') in hdr
    assert C.sizeof(lib.WeightAvg) == 24


def test_weight_avg_forms_the_weight_in_double():
    from dmf import lib
    monkey = lib._dev
    lib._dev = lambda t, dtype, name: t
    try:
        t = torch.zeros(4)
        for decay in (0.999, 0.9, 0.5, 0.0):
            w = lib.weight_avg(t, 'ema', decay, 3)
            assert (w.kind, w.start, w.reserved) == (0, 3, 0) and w.avg == t.data_ptr()
            assert np.float32(w.weight) == np.float32(1.0 - decay)        # the float32 of the double difference
        assert lib.weight_avg(t, 'mean', start=2).kind == 1
        with pytest.raises(lib.DmfError, match='not one of'):
            lib.weight_avg(t, 'swa')
    finally:
        lib._dev = monkey


def _avg(avg=FAR, kind=0, weight=0.1, start=1, reserved=0):
    from dmf import lib
    return C.byref(lib.WeightAvg(avg=None if avg is None else avg.value, kind=kind, weight=weight, start=start, reserved=reserved))


def _sched(rows=3, table=P):
    from dmf import lib
    return C.byref(lib.HpSchedule(table=None if table is None else table.value, rows=rows, row_dev=None))


def _average(avg, theta=P, n=4, step=1, step_dev=NULL):
    from dmf import lib
    return lib._lib.dmf_weight_average(avg, theta, n, step, step_dev, NULL)


def _optim(avg, sched=NULL, theta=P, grad=P, m=P, v=P, n=4, kind=0, step=1, weight_decay=0.0):
    from dmf import lib
    return lib._lib.dmf_optim_step_avg(theta, grad, m, v, n, kind, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.99, weight_decay, 0.0, step, 1.0,
                                       NULL, NULL, NULL, 0.0, 0.0, 0, 0, NULL, sched, avg, NULL)


def _reduce(avg, sched=NULL, theta=P, m=P, B=1, step=1):
    from dmf import lib
    return lib._lib.dmf_grad_reduce_adam_avg(C.byref(LATE), B, P, theta, m, P, NULL, 1e-3, 0.9, 0.999, 1e-8, step, NULL, NULL, NULL,
                                             NULL, sched, avg, NULL)


def _plan(avg, sched=NULL, s=LATE, step_dev=P, n_steps=1):
    from dmf import lib
    i = inp()
    return lib._lib.dmf_train_plan_steps_avg(C.byref(s), C.byref(i), P, P, P, 1.0, P, P, P, P, P, 1e-3, 0.9, 0.999, 1e-8, step_dev,
                                             P, P, sched, avg, n_steps, NULL)


INF, NAN = float('inf'), float('nan')
ENTRIES = {'weight_average': _average, 'optim_step_avg': _optim, 'grad_reduce_adam_avg': _reduce, 'dmf_train_plan_steps_avg': _plan}
OWN = [   # what every entry point refuses of the averaging words: (id, keywords of _avg or None for a NULL struct, message)
    ('null_struct', None, 'null dmf_weight_avg or avg'),
    ('null_vector', dict(avg=None), 'null dmf_weight_avg or avg'),
    ('kind_2', dict(kind=2), 'unknown averaging kind (DMF_AVG_EMA, DMF_AVG_MEAN)'),
    ('kind_negative', dict(kind=-1), 'unknown averaging kind (DMF_AVG_EMA, DMF_AVG_MEAN)'),
    ('weight_0', dict(weight=0.0), 'the EMA weight (1 - decay) must lie in (0, 1]'),
    ('weight_negative', dict(weight=-0.1), 'the EMA weight (1 - decay) must lie in (0, 1]'),
    ('weight_above_1', dict(weight=1.5), 'the EMA weight (1 - decay) must lie in (0, 1]'),
    ('weight_inf', dict(weight=INF), 'the EMA weight (1 - decay) must lie in (0, 1]'),
    ('weight_nan', dict(weight=NAN), 'the EMA weight (1 - decay) must lie in (0, 1]'),
    ('start_0', dict(start=0), 'the first averaged step must be >= 1'),
    ('start_negative', dict(kind=1, start=-4), 'the first averaged step must be >= 1'),
    ('reserved', dict(reserved=1), 'dmf_weight_avg.reserved must be 0'),
]
REFUSALS = [('%s-%s' % (entry, name), (lambda call=call, kw=kw: call(NULL if kw is None else _avg(**kw))), '%s: %s' % (entry, msg))
            for entry, call in ENTRIES.items() for name, kw, msg in OWN]
REFUSALS += [
    # avg overlapping theta (the plan loop and the fused step learn n from the shape: 8,009 floats from P reach past P2)
    ('weight_average-overlap', lambda: _average(_avg(avg=P)), 'weight_average: avg overlaps theta'),
    ('weight_average-overlap_tail', lambda: _average(_avg(avg=P2), n=33), 'weight_average: avg overlaps theta'),
    ('weight_average-overlap_head', lambda: _average(_avg(avg=P), theta=P2, n=33), 'weight_average: avg overlaps theta'),
    ('optim_step_avg-overlap', lambda: _optim(_avg(avg=P)), 'optim_step_avg: avg overlaps theta'),
    ('grad_reduce_adam_avg-overlap', lambda: _reduce(_avg(avg=P2)), 'grad_reduce_adam_avg: avg overlaps theta'),
    ('dmf_train_plan_steps_avg-overlap', lambda: _plan(_avg(avg=P2)), 'dmf_train_plan_steps_avg: avg overlaps theta'),
    # the stand-alone launch's own arguments
    ('weight_average-null_theta', lambda: _average(_avg(), theta=NULL), 'weight_average: null theta'),
    ('weight_average-negative_n', lambda: _average(_avg(), n=-1), 'weight_average: negative n'),
    ('weight_average-no_step', lambda: _average(_avg(), step=0), 'weight_average: step must be positive (or step_dev given)'),
    # what the twins refuse
    ('optim_step_avg-null_grad', lambda: _optim(_avg(), grad=NULL), 'optim_step: null theta or grad'),
    ('optim_step_avg-unknown_kind', lambda: _optim(_avg(), kind=4), 'optim_step: unknown kind (DMF_OPT_ADAM, _ADAMW, _SGD, _RMSPROP)'),
    ('optim_step_avg-negative_n', lambda: _optim(_avg(), n=-1), 'optim_step: negative n'),
    ('optim_step_avg-no_step', lambda: _optim(_avg(), step=0), 'optim_step: step must be positive (or step_dev given)'),
    ('optim_step_avg-weight_decay', lambda: _optim(_avg(), weight_decay=-1.0), 'optim_step: weight_decay must be finite and >= 0'),
    ('optim_step_avg-sched_rows_0', lambda: _optim(_avg(), sched=_sched(rows=0)), 'optim_step_avg: a schedule needs rows >= 1'),
    ('optim_step_avg-sched_null_table', lambda: _optim(_avg(), sched=_sched(table=None)), 'optim_step_avg: null schedule or table'),
    ('optim_step_avg-sched_sgd_null_m', lambda: _optim(_avg(), sched=_sched(), kind=2, m=NULL),
     'optim_step: null m or v (ADAM / ADAMW need both, RMSprop m, SGD m when momentum != 0)'),
    ('grad_reduce_adam_avg-null_theta', lambda: _reduce(_avg(), theta=NULL), 'null theta'),
    ('grad_reduce_adam_avg-null_m', lambda: _reduce(_avg(), m=NULL), 'Adam needs m, v and step >= 1'),
    ('grad_reduce_adam_avg-empty_batch', lambda: _reduce(_avg(), B=0), 'batch must be positive'),
    ('grad_reduce_adam_avg-sched_rows_0', lambda: _reduce(_avg(), sched=_sched(rows=0)), 'grad_reduce_adam_sched: a schedule needs rows >= 1'),
    ('dmf_train_plan_steps_avg-null_step_dev', lambda: _plan(_avg(), step_dev=NULL),
     'null argument (dmf_train_plan_steps needs the device step count and cursor)'),
    ('dmf_train_plan_steps_avg-attention', lambda: _plan(_avg(), s=ATTN), 'dmf_train_plan_steps: late-fusion network only'),
    ('dmf_train_plan_steps_avg-negative_steps', lambda: _plan(_avg(), n_steps=-1), 'dmf_train_plan_steps: negative step count or empty batch'),
    ('dmf_train_plan_steps_avg-sched_rows_0', lambda: _plan(_avg(), sched=_sched(rows=0)), 'dmf_train_plan_steps_avg: a schedule needs rows >= 1'),
]


@pytest.mark.parametrize('name,call,message', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_avg_entry_point_refusal(name, call, message):
    from dmf import lib
    assert call() == 1
    assert lib._lib.dmf_last_error().decode() == message


def test_avg_no_ops_launch_nothing():
    assert _average(_avg(), n=0) == 0
    assert _optim(_avg(), n=0) == 0
    assert _plan(_avg(), n_steps=0) == 0                           # (no step: nothing is launched)


# ---------------------------------------------------------------------------------------------- the engines on CPU tensors
class _Rec(Recorder):
    @staticmethod
    def arg(a):
        from dmf import lib
        obj = getattr(a, '_obj', None)
        if isinstance(obj, lib.HpSchedule):
            return ('sched', obj.rows, 'row' if obj.row_dev else None)
        if isinstance(obj, lib.WeightAvg):
            return ('avg', Recorder.arg(C.c_void_p(obj.avg)), obj.kind, float(np.float32(obj.weight)), obj.start)
        return Recorder.arg(a)


@pytest.fixture
def rec(monkeypatch):
    import torch.distributed as dist
    from dmf import lib
    r = _Rec(lib._lib)
    monkeypatch.setattr(lib, '_lib', r)
    monkeypatch.setattr(lib, '_dev', lambda t, dtype, name: t)
    monkeypatch.setattr(lib, '_stream', lambda: None)
    for entry in ('all_reduce', 'all_gather', 'all_gather_into_tensor'):
        monkeypatch.setattr(dist, entry, r.collective(getattr(dist, entry), entry))
    return r


@pytest.fixture(scope='module')
def group(tmp_path_factory):
    import torch.distributed as dist
    dist.init_process_group('gloo', init_method='file://%s' % tmp_path_factory.mktemp('pg').joinpath('store'), rank=0, world_size=1)
    yield dist.group.WORLD
    dist.destroy_process_group()


def _engine(optimizer='ADAM', criterion=None, **kw):
    from dmf.engine import Scene, TrainEngine
    from model.gmfnet import Net
    cfg = {'patch_size': 11, 'Categories_Number': 17, 'data_city': 's', 'DATA_DICT': {'s': {'size': [40, 40, 200]}},
           'scale': 1, 'aux_bands': 1, 'gmf': {'width': 40, 'hidden': 64, 'pool_sigma': 2.5, 'attention': 0},
           'trans': {'embed_dim': 96, 'num_head': 3}}
    torch.manual_seed(0)
    scene = Scene(np.zeros((50, 50, 200), np.float32), np.zeros((50, 50, 1), np.float32), 'cpu')
    return TrainEngine(Net(cfg), scene, 8, lr=2e-3, optimizer=optimizer, momentum=0.5, criterion=criterion, **kw)


def _xy():
    rng = np.random.default_rng(0)
    return (torch.from_numpy(rng.integers(0, 30, (8, 2)).astype(np.int32)), torch.from_numpy(rng.integers(0, 17, 8).astype(np.int32)))


TABLE = np.array([[1e-3, 0.9, 0.999, 0.5], [5e-4, 0.85, 0.999, 0.4]], dtype=np.float32)
AVG = ('avg', 'avg', 0, float(np.float32(1.0 - 0.99)), 4)            # as the recorder shows set_averaging('ema', 0.99, 4)
F = lambda x: float(np.float32(x))


def _take(rec, eng, **extra):
    return rec.take(eng, avg=eng.avg, **extra) if eng.avg is not None else rec.take(eng, **extra)


def test_set_averaging_checks_and_state(rec):
    from dmf import lib
    eng = _engine()
    assert eng.averaged_parameters() is None and not eng._counts_on_device()
    for bad, msg in ((dict(kind='swa'), 'not one of'), (dict(kind='ema', decay=1.0), r'not in \[0, 1\)'),
                     (dict(kind='ema', decay=-0.1), r'not in \[0, 1\)'), (dict(kind='ema', decay=float('nan')), r'not in \[0, 1\)'),
                     (dict(kind='mean', start_step=0), 'at least 1')):
        with pytest.raises(lib.DmfError, match=msg):
            eng.set_averaging(**bad)
        assert eng.wavg is None
    eng.step_count, eng.graph = 5, object()
    base = eng._hparams()
    eng.set_averaging('ema', 0.99, 4)
    assert eng.graph is None                                             # a captured graph is dropped
    assert eng._counts_on_device() and int(eng.dev_step[0]) == 5          # the device counts from the host's count on
    avg = eng.averaged_parameters()
    assert avg is eng.avg and avg.data_ptr() != eng.theta.data_ptr() and torch.equal(avg, eng.theta)
    assert eng._hparams() == base + ('avg', 0, eng.wavg.weight, 4)        # kind, weight and start are launch arguments
    eng.set_averaging('mean', start_step=2)
    assert eng._hparams()[-4:] == ('avg', 1, eng.wavg.weight, 2)
    eng.theta.add_(1.0)
    with eng._state_kept():                                               # a capture's trial step must not leave a trace in avg
        eng.avg.fill_(7.0)
    assert not (eng.avg == 7.0).any()


def test_the_fused_step_routes_to_the_avg_reduce(rec):
    """Eager, from the plan, and the native loop; with and without a schedule."""
    xy, lab = _xy()
    for table in (None, TABLE):
        eng = _engine('ADAM')
        if table is not None:
            eng.set_schedule(table, 'step')
        eng.set_averaging('ema', 0.99, 4)
        sched = None if table is None else ('sched', 2, None)
        hp = (F(2e-3), F(0.9), F(0.999)) if table is None else (0.0, 0.0, 0.0)
        _take(rec, eng)
        eng.step(xy, lab)
        calls = _take(rec, eng, xy=xy, labels=lab)
        assert [c[0] for c in calls] == ['dmf_train_fwd_bwd', 'dmf_grad_reduce_adam_avg']
        assert calls[0][-2] == 'dev_step'                                 # the forward launch counts the step on the device
        assert calls[1] == ('dmf_grad_reduce_adam_avg', 'shape', 8, 'ws', 'theta', 'm', 'v', None) + hp + (
            F(1e-8), 1, 'dev_step', None, None, None, sched, AVG, None)
        eng.load_plan(torch.cat([xy, xy]), torch.cat([lab, lab]))
        _take(rec, eng)
        eng.run_plan(1, 0)
        calls = _take(rec, eng)
        assert [c[0] for c in calls] == ['dmf_train_fwd_bwd', 'dmf_grad_reduce_adam_avg']
        assert calls[1][12:] == (2, 'dev_step', 'dev_cursor', 'loss', 'loss_hist', sched, AVG, None)
        eng.run_plan(1, -1)
        calls = _take(rec, eng)
        assert [c[0] for c in calls] == ['dmf_train_plan_steps_avg']
        assert calls[0][-5:] == ('loss_hist', sched, AVG, 1, None) and calls[0][15] == F(1e-8)
        assert eng.step_count == 3


@pytest.mark.parametrize('optim,kw', [('SGD', {}), ('RMSprop', {}), ('ADAMW', dict(weight_decay=0.01)), ('ADAM', dict(clip_grad_norm=0.5)),
                                      ('ADAM', dict(weight_decay=0.1))], ids=['SGD', 'RMSprop', 'ADAMW', 'clip', 'decay'])
@pytest.mark.parametrize('scheduled', [False, True], ids=['launch-args', 'schedule'])
def test_other_optimisers_and_the_regularised_step_route_to_optim_step_avg(rec, optim, kw, scheduled):
    """The reduce launch in front is the plain dmf_grad_reduce it was: gradient and loss keep their bits."""
    xy, lab = _xy()
    eng = _engine(optim, **kw)
    if scheduled:
        eng.set_schedule(TABLE, 'epoch')
    eng.set_averaging('mean', start_step=4)
    _take(rec, eng)
    eng.step(xy, lab)
    calls = _take(rec, eng, xy=xy, labels=lab)
    assert [c[0] for c in calls] == ['dmf_train_fwd_bwd', 'dmf_grad_reduce', 'dmf_optim_step_avg']
    assert calls[1] == ('dmf_grad_reduce', 'shape', 8, 'ws', 'grad', None)
    kind = {'ADAM': 0, 'ADAMW': 1, 'SGD': 2, 'RMSprop': 3}[optim]
    c = calls[2]
    assert c[:7] == ('dmf_optim_step_avg', 'theta', 'grad', 'm', 'v', eng.theta.numel(), kind)
    assert c[7:11] == (F(2e-3), F(0.9), F(0.999), F(1e-8)) and c[11] == F(0.5)      # lr, betas, eps, momentum (unused with a schedule)
    assert c[13:15] == (F(kw.get('weight_decay', 0.0)), F(kw.get('clip_grad_norm', 0.0)))
    assert c[17] == 'dev_step'
    assert c[-3:] == (('sched', 2, 'row') if scheduled else None, ('avg', 'avg', 1, F(1.0 - 0.999), 4), None)


@pytest.mark.parametrize('scheduled', [False, True], ids=['launch-args', 'schedule'])
def test_the_scaler_step_keeps_its_reduce_and_updates_by_optim_step_avg(rec, scheduled):
    from dmf.engine import LossScaler
    xy, lab = _xy()
    eng = _engine('ADAM', scaler=LossScaler('cpu'))
    if scheduled:
        eng.set_schedule(TABLE, 'step')
    eng.set_averaging('ema', 0.99, 4)
    _take(rec, eng)
    eng.step(xy, lab)
    calls = _take(rec, eng, xy=xy, labels=lab)
    assert [c[0] for c in calls] == ['dmf_train_fwd_bwd_scaled', 'dmf_grad_reduce_scaled', 'dmf_optim_step_avg']
    assert calls[1] == ('dmf_grad_reduce_scaled', 'shape', 8, 'ws', 'grad', 'scaler', None, None, None, None)
    c = calls[2]
    assert c[17:19] == ('dev_step', None) and c[19] == 'scaler' and c[23] == 1          # the device count, the scaler, unscaled
    assert c[-2] == AVG


def test_the_criterion_step_and_the_one_rank_group(rec, group):
    xy, lab = _xy()
    eng = _engine('ADAM', criterion={'label_smoothing': 0.1})
    eng.set_averaging('ema', 0.99, 4)
    _take(rec, eng)
    eng.step(xy, lab)
    assert [c[0] for c in _take(rec, eng, xy=xy, labels=lab)] == ['dmf_forward_unit', 'dmf_ce_loss', 'dmf_backward_unit',
                                                                  'dmf_grad_reduce_adam_avg']
    eng = _engine('ADAM', process_group=group)
    eng._force_collective = True
    eng.set_averaging('ema', 0.99, 4)
    _take(rec, eng)
    eng.step(xy, lab)
    calls = _take(rec, eng, xy=xy, labels=lab)
    assert calls[1:3] == [('dmf_grad_reduce', 'shape', 8, 'ws', 'grad', None), ('all_reduce', 'grad')]
    assert [c[0] for c in calls] == ['dmf_train_fwd_bwd', 'dmf_grad_reduce', 'all_reduce', 'dmf_optim_step_avg'] and calls[3][-2] == AVG


def test_the_xgmi_route_keeps_its_launch_and_is_followed_by_the_stand_alone_one(rec, group):
    import types
    from dmf import lib
    xy, lab = _xy()
    eng = _engine('ADAM', process_group=group)
    eng._force_collective = True
    eng.comm = types.SimpleNamespace(c=lib.XgmiComm(world=1), world=1, capacity=eng.theta.numel(), rewind=lambda n: None)
    eng.set_averaging('ema', 0.99, 4)
    _take(rec, eng)
    eng.step(xy, lab)
    calls = _take(rec, eng, xy=xy, labels=lab)
    assert [c[0] for c in calls] == ['dmf_train_fwd_bwd', 'dmf_grad_reduce_xgmi_adam', 'dmf_weight_average']
    assert calls[2] == ('dmf_weight_average', AVG, 'theta', eng.theta.numel(), 1, 'dev_step', None)


@pytest.mark.parametrize('unit', [True, False], ids=['unit', 'nonunit'])
def test_stage_two_routes_too(rec, monkeypatch, unit):
    from dmf import lib
    from dmf.engine import QuaScene, QuaTrainEngine
    from model.gmfnet import Net
    if not unit:
        monkeypatch.setattr(lib, 'unit_supported', lambda shape: False)
    cfg = {'patch_size': 16, 'Categories_Number': 5, 'data_city': 's', 'DATA_DICT': {'s': {'size': [20, 20, 4]}},
           'gmf': {'width': 40, 'single_input': 1}}
    torch.manual_seed(0)
    eng = QuaTrainEngine(Net(cfg), QuaScene([np.zeros((36, 36, 4), np.float32)] * 4, 'cpu'), 8, DQTL, lr=2e-3)
    eng.set_averaging('ema', 0.99, 4)
    rng = np.random.default_rng(0)
    xy = torch.from_numpy(rng.integers(0, 20, (8, 2)).astype(np.int32))
    lab = torch.from_numpy(rng.integers(0, 5, 8).astype(np.int32))
    _take(rec, eng)
    eng.step(xy, lab)
    calls = _take(rec, eng)
    want = (['dmf_forward_unit', 'dmf_qua_loss_ranks', 'dmf_backward_unit'] if unit else
            ['dmf_forward', 'dmf_qua_loss_ranks', 'dmf_backward_dlogits']) + ['dmf_grad_reduce_adam_avg']
    assert [c[0] for c in calls] == want
    # dmf_forward counts no steps: the non-unit form hands the launch the host's count
    assert calls[-1][12:14] == (1, 'dev_step' if unit else None) and calls[-1][-2] == AVG


def test_without_averaging_nothing_routes_there(rec, group):
    """... and every launch is the one tests/test_engine_update_host.py states for the parent."""
    from dmf.engine import LossScaler
    from test_engine_update_host import _f32, expected_update
    xy, lab = _xy()
    for optim, kw in (('ADAM', {}), ('SGD', {}), ('RMSprop', {}), ('ADAM', dict(scaler=LossScaler('cpu'))), ('ADAM', dict(process_group=group))):
        eng = _engine(optim, **kw)
        collective = 'process_group' in kw
        eng._force_collective = collective
        rec.take(eng)
        eng.step(xy, lab)
        calls = rec.take(eng, xy=xy, labels=lab)
        assert not [c for c in calls if c[0].endswith('_avg') or c[0] == 'dmf_weight_average']
        dev = 'dev_step' if (optim != 'ADAM' or 'scaler' in kw) else None
        assert calls[1:] == _f32(expected_update(eng, 8, dev, None, 1.0, None, None, collective, False))


def test_eval_engine_evaluates_a_given_vector(rec):
    from dmf import lib
    from dmf.engine import EvalEngine
    eng = _engine()
    ev = EvalEngine(eng.net, eng.scene, 8)
    xy, _ = _xy()
    other = eng.theta.clone()
    ev.predict(xy)
    assert rec.take(eng, other=other)[0][3] == 'theta'
    ev.use_parameters(other)
    ev.predict(xy)
    assert rec.take(eng, other=other)[0][3] == 'other'
    ev.use_parameters(None)
    ev.predict(xy)
    assert rec.take(eng, other=other)[0][3] == 'theta'
    with pytest.raises(lib.DmfError, match='flat vector'):
        ev.use_parameters(other[:-1])


# ---------------------------------------------------------------------------------------------- the config keys
def test_averaging_keys_and_the_first_averaged_step():
    from solver.mainsolver import Solver
    from utils import utils as u
    base = {'optimizer': 'ADAM', 'lr': 1e-3}
    assert u.averaging_keys({'schedule': dict(base)}) is None                       # absent: today's path
    assert u.averaging_keys({'schedule': dict(base, weight_average='none', average_decay=0.5)}) is None
    assert u.averaging_keys({'schedule': dict(base, weight_average='ema')}) == ('ema', 0.999, 0)
    assert u.averaging_keys({'schedule': dict(base, weight_average='mean', average_start=3)}) == ('mean', 0.999, 3)
    for bad, msg in ((dict(weight_average='swa'), 'weight_average'), (dict(weight_average='ema', average_decay=1.0), 'average_decay'),
                     (dict(weight_average='ema', average_decay=-0.5), 'average_decay'),
                     (dict(weight_average='mean', average_start=-1), 'average_start'),
                     (dict(weight_average='mean', average_start=1.5), 'average_start')):
        with pytest.raises(ValueError, match=msg):
            u.averaging_keys({'schedule': dict(base, **bad)})
    s = Solver.__new__(Solver)
    for start, steps, want in ((0, 7, 1), (1, 7, 8), (3, 10, 31), (2, 1, 3)):        # average_start * steps_per_epoch + 1
        s.averaging = ('ema', 0.999, start)
        assert s._average_start_step(steps) == want


def test_config_yml_states_the_keys_commented():
    import yaml
    text = open(os.path.join(REPO, 'dual-modal-fusion_amd', 'config.yml')).read()
    for key, default in (('weight_average', 'none'), ('average_decay', '0.999'), ('average_start', '0')):
        assert '  # %s: %s' % (key, default) in text
    assert 'weight_average' not in yaml.safe_load(text)['schedule']                 # commented: absent, the neutral default


def test_tostagesolver_refuses_the_keys_by_name():
    from solver.tostagesolver import toStageSolver
    cfg = {'Categories_Number': 5, 'schedule': {'loss': 'qua_loss', 'optimizer': 'ADAM', 'lr': 1e-3, 'weight_average': 'ema'}}
    with pytest.raises(ValueError, match=r'schedule\.weight_average, schedule\.average_decay and schedule\.average_start are out of '
                                         r'scope for toStageSolver'):
        toStageSolver(cfg)


def test_the_drop_in_update_is_averaged_model():
    """utils.average_update_ (the drop-in loop's update) against AveragedModel itself, bit for bit on the CPU."""
    from utils import utils as u
    rng = np.random.default_rng(1)
    for kind in ('ema', 'mean'):
        for start in (1, 3):
            ref = avg_ref.AvgRef(257, kind, 0.9, start)
            avg = torch.zeros(257)
            for st in range(1, 7):
                theta = torch.from_numpy(rng.standard_normal(257).astype(np.float32))
                u.average_update_([avg], [theta], kind, 0.9, start, st)
                assert ref.update(theta.numpy()).tobytes() == avg.numpy().tobytes(), (kind, start, st)


# ---------------------------------------------------------------------------------------------- the guard of the GPU bit counts
def test_torch_lerp_on_this_cpu_is_the_fused_form():
    assert avg_ref.lerp_is_fused() == 0
