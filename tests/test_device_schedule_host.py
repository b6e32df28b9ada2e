"""CPU: the device-resident lr schedule as far as the host decides it — the table that `utils.schedule_table`
builds against torch's own scheduler objects, the two config keys, what `set_schedule` refuses, what a captured graph still
bakes in (`_hparams`), the three `_sched` entry points with their refusals, and the entry points an engine with a schedule
launches (recorded on CPU tensors by the recorder of tests/test_engine_update_host.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_capi_host import LATE, ATTN, NULL, P, inp
from test_engine_update_host import Recorder

SCHED = {'optimizer': 'ADAM', 'lr': 1e-3, 'base_lr': 1e-4, 'momentum': 0.9, 'alpha': 0.9, 'if_scheduler': 1}
KINDS = ('StepLR', 'LinearLR', 'CosineAnnealingLR', 'CyclicLR', 'OneCycleLR', 'ConstantLR', 'ChainedScheduler', 'ExponentialLR')
OPTIMS = ('ADAM', 'SGD', 'RMSprop')


def _f32(x):
    return np.float32(x)


def _row(group):
    """(lr, beta1, beta2, momentum) of a torch parameter group as the float32 a ctypes c_float argument becomes."""
    b1, b2 = group.get('betas', (0.9, 0.999))
    return [C.c_float(v).value for v in (group['lr'], b1, b2, group.get('momentum', 0.0) or 0.0)]


# ---------------------------------------------------------------------------------------------- utils.schedule_table
def test_the_scheduler_table_lists_every_kind():
    from utils import utils as u
    assert sorted(KINDS) == sorted(u._SCHEDULERS)


@pytest.mark.parametrize('optim', OPTIMS)
@pytest.mark.parametrize('kind', KINDS)
def test_schedule_table_is_the_sequence_of_epoch_hparams(kind, optim):
    from utils import utils as u
    rows = 60
    cfg = {'epoch': rows, 'schedule': dict(SCHED, scheduler=kind, optimizer=optim)}
    table = u.schedule_table(cfg, rows, 'epoch')
    assert table.dtype == np.float32 and table.shape == (rows, 4)
    want = np.array([_row(u.epoch_hparams(cfg, e)) for e in range(rows)], dtype=np.float32)
    assert table.tobytes() == want.tobytes()
    assert len(set(table[:, 0].tolist())) > 1                      # the lr moves: the comparison is not of constants
    if kind == 'OneCycleLR' and optim == 'ADAM':
        assert len(set(table[:, 1].tolist())) > 1                  # ... and so does beta1
    if kind == 'OneCycleLR' and optim == 'SGD':
        assert len(set(table[:, 3].tolist())) > 1                  # ... or the momentum


@pytest.mark.parametrize('kind', KINDS)
def test_schedule_table_unit_step_is_a_torch_scheduler_stepped_per_row(kind):
    """Unit step: the scheduler spans `rows` steps (OneCycleLR's total_steps) and is stepped once per row."""
    from utils import utils as u
    rows = 36                                                      # 12 epochs of 3 steps
    cfg = {'epoch': 12, 'schedule': dict(SCHED, scheduler=kind)}
    table = u.schedule_table(cfg, rows, 'step')
    p = torch.nn.Parameter(torch.zeros(1))
    opt = u.make_optimizer(cfg, [p])
    sch = u.make_scheduler(opt, cfg, total=rows)
    want = []
    for _ in range(rows):
        want.append(_row(opt.param_groups[0]))
        opt.step(); sch.step()
    assert table.tobytes() == np.array(want, dtype=np.float32).tobytes()
    if kind == 'OneCycleLR':                                       # the peak lies at half of ALL the steps, not of the epochs
        assert int(table[:, 0].argmax()) in (rows // 2 - 1, rows // 2)
        assert table[:12].tobytes() != u.schedule_table(cfg, 12, 'epoch').tobytes()


def test_schedule_table_without_a_scheduler_is_one_row():
    from utils import utils as u
    cfg = {'epoch': 9, 'schedule': dict(SCHED, if_scheduler=0, scheduler='StepLR', optimizer='SGD')}
    for unit in ('epoch', 'step'):
        t = u.schedule_table(cfg, 9, unit)
        assert t.shape == (1, 4) and t[0].tolist() == [_f32(1e-3), _f32(0.9), _f32(0.999), _f32(0.9)]
    with pytest.raises(ValueError, match='not one of'):
        u.schedule_table(cfg, 9, 'batch')
    with pytest.raises(ValueError, match='at least one row'):
        u.schedule_table(cfg, 0, 'epoch')


def test_scheduler_unit_step_needs_the_device_schedule_on_the_fast_path():
    from utils import utils as u
    cfg = {'schedule': dict(SCHED, scheduler='OneCycleLR')}
    assert u.schedule_keys(cfg, fast=True) == (False, 'epoch')                        # absent keys: today's path
    cfg['schedule'].update(device_schedule=1)
    assert u.schedule_keys(cfg, fast=True) == (True, 'epoch')
    cfg['schedule'].update(scheduler_unit='step')
    assert u.schedule_keys(cfg, fast=True) == (True, 'step')
    cfg['schedule'].update(device_schedule=0)
    assert u.schedule_keys(cfg, fast=False) == (False, 'step')                        # the drop-in path steps torch's scheduler
    with pytest.raises(ValueError, match='requires schedule.device_schedule: 1'):
        u.schedule_keys(cfg, fast=True)
    cfg['schedule'].update(scheduler_unit='batch')
    with pytest.raises(ValueError, match='scheduler_unit'):
        u.schedule_keys(cfg)


def test_config_yml_states_both_keys_with_their_neutral_defaults():
    import os
    import yaml
    from test_capi_host import lib
    cfg = yaml.safe_load(open(os.path.join(os.path.dirname(os.path.dirname(lib.__file__)), 'config.yml')))
    assert cfg['schedule']['device_schedule'] == 0 and cfg['schedule']['scheduler_unit'] == 'epoch'


# ---------------------------------------------------------------------------------------------- the engine on CPU tensors
class _Rec(Recorder):
    @staticmethod
    def arg(a):
        from dmf import lib
        obj = getattr(a, '_obj', None)
        if isinstance(obj, lib.HpSchedule):
            return ('sched', obj.rows, 'row' if obj.row_dev else None)
        return Recorder.arg(a)


@pytest.fixture
def rec(monkeypatch):
    from dmf import lib
    r = _Rec(lib._lib)
    monkeypatch.setattr(lib, '_lib', r)
    monkeypatch.setattr(lib, '_dev', lambda t, dtype, name: t)
    monkeypatch.setattr(lib, '_stream', lambda: None)
    return r


def _engine(optimizer='ADAM', criterion=None, **kw):
    from dmf.engine import Scene, TrainEngine
    from model.gmfnet import Net
    cfg = {'patch_size': 11, 'Categories_Number': 17, 'data_city': 's', 'DATA_DICT': {'s': {'size': [40, 40, 200]}},
           'scale': 1, 'aux_bands': 1, 'gmf': {'width': 40, 'hidden': 64, 'pool_sigma': 2.5, 'attention': 0},
           'trans': {'embed_dim': 96, 'num_head': 3}}
    torch.manual_seed(0)
    scene = Scene(np.zeros((50, 50, 200), np.float32), np.zeros((50, 50, 1), np.float32), 'cpu')
    return TrainEngine(Net(cfg), scene, 8, lr=2e-3, optimizer=optimizer, momentum=0.5, criterion=criterion, **kw)


TABLE = np.array([[1e-3, 0.9, 0.999, 0.5], [5e-4, 0.85, 0.999, 0.4], [0.0, 0.0, 0.0, 0.0]], dtype=np.float32)


@pytest.mark.parametrize('row,message', [
    ([np.nan, 0.9, 0.999, 0.0], 'non-finite'), ([np.inf, 0.9, 0.999, 0.0], 'non-finite'), ([1e-3, 0.9, -np.inf, 0.0], 'non-finite'),
    ([-1e-6, 0.9, 0.999, 0.0], 'negative lr'), ([1e-3, 1.0, 0.999, 0.0], r'\[0, 1\)'), ([1e-3, 0.9, 1.5, 0.0], r'\[0, 1\)'),
    ([1e-3, -0.1, 0.999, 0.0], r'\[0, 1\)'), ([1e-3, 0.9, 0.999, 1.0], r'\[0, 1\)'), ([1e-3, 0.9, 0.999, -0.5], r'\[0, 1\)')])
def test_set_schedule_refuses_rows_out_of_range(rec, row, message):
    from dmf import lib
    eng = _engine()
    bad = TABLE.copy()
    bad[1] = row
    with pytest.raises(lib.DmfError, match=message) as e:
        eng.set_schedule(bad, 'epoch')
    assert 'row 1' in str(e.value)
    assert eng.sched is None


def test_set_schedule_refuses_other_shapes_and_units(rec):
    from dmf import lib
    eng = _engine()
    for bad in (TABLE[:, :3], TABLE[0], np.zeros((0, 4), np.float32)):
        with pytest.raises(lib.DmfError, match=r'rows >= 1, 4'):
            eng.set_schedule(bad)
    with pytest.raises(lib.DmfError, match='neither epoch nor step'):
        eng.set_schedule(TABLE, 'batch')
    eng.set_schedule(TABLE, 'epoch')                               # lr 0 and betas 0 are in range
    assert eng.sched.rows == 3 and eng.hp_row is not None and eng.hp_table.dtype == torch.float32
    eng.set_epoch(2)
    assert int(eng.hp_row[0]) == 2
    eng.set_schedule(TABLE, 'step')
    assert eng.hp_row is None and not eng.sched.row_dev
    eng.set_epoch(1)                                               # unit step: nothing to do


def test_a_graph_no_longer_bakes_in_what_the_table_holds(rec):
    eng = _engine('SGD')
    base = eng._hparams()
    eng.lr *= 0.5
    assert eng._hparams() != base                                  # today's path: a new lr is a new graph
    eng.set_schedule(TABLE, 'epoch')
    base = eng._hparams()
    eng.lr, eng.b1, eng.b2, eng.momentum = 0.123, 0.5, 0.6, 0.7
    assert eng._hparams() == base
    assert not {0.123, 0.5, 0.6, 0.7} & set(base)
    eng.eps, eng.alpha = 1e-6, 0.5                                 # what stays a launch argument still invalidates a graph
    assert eng._hparams() != base


def test_set_schedule_hands_the_step_count_to_the_device(rec):
    eng = _engine('ADAM')
    assert not eng._counts_on_device()
    eng.step_count = 5
    eng.set_schedule(TABLE, 'step')
    assert eng._counts_on_device() and int(eng.dev_step[0]) == 5


def _xy():
    rng = np.random.default_rng(0)
    return (torch.from_numpy(rng.integers(0, 30, (8, 2)).astype(np.int32)), torch.from_numpy(rng.integers(0, 17, 8).astype(np.int32)))


@pytest.mark.parametrize('unit', ['epoch', 'step'])
def test_every_step_form_routes_to_the_sched_entry_points(rec, unit):
    """The fused step (eager, from the plan, the native loop), SGD, RMSprop, the scaler, the regularised step and the
    unit-gradient step: with a schedule the update is one of the three `_sched` entry points, and no lr, beta or momentum is
    among its arguments."""
    from dmf.engine import LossScaler
    xy, lab = _xy()
    sched = ('sched', 3, 'row' if unit == 'epoch' else None)
    n = None

    def names(eng):
        return [c[0] for c in rec.take(eng, xy=xy, labels=lab)]

    eng = _engine('ADAM')
    eng.set_schedule(TABLE, unit)
    rec.take(eng)
    eng.step(xy, lab)
    calls = rec.take(eng, xy=xy, labels=lab)
    assert [c[0] for c in calls] == ['dmf_train_fwd_bwd', 'dmf_grad_reduce_adam_sched']
    assert calls[0][-2] == 'dev_step'                              # the forward launch counts the step on the device
    n = eng.theta.numel()
    assert calls[1] == ('dmf_grad_reduce_adam_sched', 'shape', 8, 'ws', 'theta', 'm', 'v', None, sched, float(np.float32(1e-8)), 1,
                        'dev_step', None, None, None, None)
    eng.load_plan(torch.cat([xy, xy]), torch.cat([lab, lab]))
    rec.take(eng)
    eng.run_plan(1, 0)
    assert names(eng) == ['dmf_train_fwd_bwd', 'dmf_grad_reduce_adam_sched']
    eng.run_plan(1, -1)
    calls = rec.take(eng)
    assert [c[0] for c in calls] == ['dmf_train_plan_steps_sched'] and sched in calls[0]
    assert eng.step_count == 3

    for optim, kw in (('SGD', {}), ('RMSprop', {}), ('ADAMW', dict(weight_decay=0.01)), ('ADAM', dict(clip_grad_norm=0.5))):
        eng = _engine(optim, **kw)
        eng.set_schedule(TABLE, unit)
        rec.take(eng)
        eng.step(xy, lab)
        calls = rec.take(eng, xy=xy, labels=lab)
        assert [c[0] for c in calls] == ['dmf_train_fwd_bwd', 'dmf_grad_reduce', 'dmf_optim_step_sched'], optim
        kind = {'ADAM': 0, 'ADAMW': 1, 'SGD': 2, 'RMSprop': 3}[optim]
        assert calls[2][:8] == ('dmf_optim_step_sched', 'theta', 'grad', 'm', 'v', n, kind, sched), optim
        assert calls[2][14] == 'dev_step'

    eng = _engine('ADAM', scaler=LossScaler('cpu'))
    eng.set_schedule(TABLE, unit)
    rec.take(eng)
    eng.step(xy, lab)
    assert names(eng) == ['dmf_train_fwd_bwd_scaled', 'dmf_grad_reduce_scaled', 'dmf_optim_step_sched']

    eng = _engine('ADAM', criterion={'label_smoothing': 0.1})
    eng.set_schedule(TABLE, unit)
    rec.take(eng)
    eng.step(xy, lab)
    assert names(eng) == ['dmf_forward_unit', 'dmf_ce_loss', 'dmf_backward_unit', 'dmf_grad_reduce_adam_sched']


def test_without_a_schedule_nothing_routes_to_them(rec):
    xy, lab = _xy()
    for optim in ('ADAM', 'SGD'):
        eng = _engine(optim)
        rec.take(eng)
        eng.step(xy, lab)
        assert not [c for c in rec.take(eng, xy=xy, labels=lab) if c[0].endswith('_sched')]


# ---------------------------------------------------------------------------------------------- the C ABI
def test_the_three_entry_points_are_exported():
    """(Fails on a build without the feature: the symbols do not exist.)"""
    from dmf import lib
    hdr = open(__import__('os').path.join(__import__('os').path.dirname(__file__), '..', 'include', 'dmf.h')).read()
    for name in ('dmf_optim_step_sched', 'dmf_grad_reduce_adam_sched', 'dmf_train_plan_steps_sched'):
        assert name in lib.EXPORTS and getattr(lib._lib, name) is not None
        assert 'int32_t %s(' % name in hdr
    assert 'typedef struct dmf_hp_schedule { const float* table; int32_t rows; const int32_t* row_dev; } dmf_hp_schedule;' in hdr
    assert lib.version() >= 306
    assert C.sizeof(lib.HpSchedule) == 24


def _sched(table=P, rows=3, row_dev=NULL):
    from dmf import lib
    return C.byref(lib.HpSchedule(table=None if table is None else table.value, rows=rows,
                                  row_dev=None if row_dev is None else row_dev.value))


def _optim(sched, theta=P, grad=P, m=P, v=P, n=4, kind=0, weight_decay=0.0, max_norm=0.0, step=1, step_dev=NULL, state=NULL,
           growth=0.0, backoff=0.0, interval=0, unscaled=0):
    from dmf import lib
    return lib._lib.dmf_optim_step_sched(theta, grad, m, v, n, kind, sched, 1e-8, 0.99, weight_decay, max_norm, step, 1.0, step_dev,
                                         NULL, state, growth, backoff, interval, unscaled, NULL, NULL)


def _reduce(sched, s=LATE, B=1, ws=P, theta=P, m=P, v=P, step=1, step_dev=NULL):
    from dmf import lib
    return lib._lib.dmf_grad_reduce_adam_sched(C.byref(s), B, ws, theta, m, v, NULL, sched, 1e-8, step, step_dev, NULL, NULL, NULL, NULL)


def _plan(sched, s=LATE, i=None, theta=P, labels=P, step_dev=P, cursor=P, n_steps=1):
    from dmf import lib
    i = inp() if i is None else i
    return lib._lib.dmf_train_plan_steps_sched(C.byref(s), C.byref(i), theta, P, labels, 1.0, P, P, P, P, P, sched, 1e-8, step_dev,
                                               cursor, P, n_steps, NULL)


INF = float('inf')
SCHED_REFUSALS = [
    # the schedule itself
    ('optim_null_schedule', lambda: _optim(NULL), 'optim_step_sched: null schedule or table'),
    ('optim_null_table', lambda: _optim(_sched(table=None)), 'optim_step_sched: null schedule or table'),
    ('optim_rows_0', lambda: _optim(_sched(rows=0)), 'optim_step_sched: a schedule needs rows >= 1'),
    ('optim_rows_negative', lambda: _optim(_sched(rows=-2)), 'optim_step_sched: a schedule needs rows >= 1'),
    ('reduce_null_schedule', lambda: _reduce(NULL), 'grad_reduce_adam_sched: null schedule or table'),
    ('reduce_null_table', lambda: _reduce(_sched(table=None)), 'grad_reduce_adam_sched: null schedule or table'),
    ('reduce_rows_0', lambda: _reduce(_sched(rows=0)), 'grad_reduce_adam_sched: a schedule needs rows >= 1'),
    ('plan_null_schedule', lambda: _plan(NULL), 'dmf_train_plan_steps_sched: null schedule or table'),
    ('plan_null_table', lambda: _plan(_sched(table=None)), 'dmf_train_plan_steps_sched: null schedule or table'),
    ('plan_rows_0', lambda: _plan(_sched(rows=0)), 'dmf_train_plan_steps_sched: a schedule needs rows >= 1'),
    # what the unscheduled twins refuse
    ('optim_null_theta', lambda: _optim(_sched(), theta=NULL), 'optim_step: null theta or grad'),
    ('optim_null_grad', lambda: _optim(_sched(), grad=NULL), 'optim_step: null theta or grad'),
    ('optim_unknown_kind', lambda: _optim(_sched(), kind=4), 'optim_step: unknown kind (DMF_OPT_ADAM, _ADAMW, _SGD, _RMSPROP)'),
    ('optim_adam_null_v', lambda: _optim(_sched(), v=NULL),
     'optim_step: null m or v (ADAM / ADAMW need both, RMSprop m, SGD m when momentum != 0)'),
    ('optim_rmsprop_null_m', lambda: _optim(_sched(), kind=3, m=NULL),
     'optim_step: null m or v (ADAM / ADAMW need both, RMSprop m, SGD m when momentum != 0)'),
    # (the host cannot see the row's momentum: SGD needs its buffer whatever the row says)
    ('optim_sgd_null_m', lambda: _optim(_sched(), kind=2, m=NULL),
     'optim_step: null m or v (ADAM / ADAMW need both, RMSprop m, SGD m when momentum != 0)'),
    ('optim_negative_n', lambda: _optim(_sched(), n=-1), 'optim_step: negative n'),
    ('optim_negative_weight_decay', lambda: _optim(_sched(), weight_decay=-0.1), 'optim_step: weight_decay must be finite and >= 0'),
    ('optim_inf_max_norm', lambda: _optim(_sched(), max_norm=INF), 'optim_step: max_norm must be finite (<= 0 switches clipping off)'),
    ('optim_scaler_keys_without_state', lambda: _optim(_sched(), growth=2.0),
     'optim_step: scaler hyper-parameters (growth, backoff, interval, unscaled) without a scaler state'),
    ('optim_no_step', lambda: _optim(_sched(), step=0), 'optim_step: step must be positive (or step_dev given)'),
    ('optim_state_without_step_dev', lambda: _optim(_sched(), state=P, growth=2.0, backoff=0.5, interval=3),
     'optim_step: a scaler state needs the device step count'),
    ('optim_bad_interval', lambda: _optim(_sched(), state=P, step_dev=P, growth=2.0, backoff=0.5, interval=0),
     'optim_step: bad growth_interval / factors'),
    ('reduce_null_theta', lambda: _reduce(_sched(), theta=NULL), 'null theta'),
    ('reduce_null_workspace', lambda: _reduce(_sched(), ws=NULL), 'null argument'),
    ('reduce_empty_batch', lambda: _reduce(_sched(), B=0), 'batch must be positive'),
    ('reduce_null_m', lambda: _reduce(_sched(), m=NULL), 'Adam needs m, v and step >= 1'),
    ('reduce_no_step', lambda: _reduce(_sched(), step=0), 'Adam needs m, v and step >= 1'),
    ('plan_null_step_dev', lambda: _plan(_sched(), step_dev=NULL),
     'null argument (dmf_train_plan_steps needs the device step count and cursor)'),
    ('plan_null_cursor', lambda: _plan(_sched(), cursor=NULL),
     'null argument (dmf_train_plan_steps needs the device step count and cursor)'),
    ('plan_null_labels', lambda: _plan(_sched(), labels=NULL),
     'null argument (dmf_train_plan_steps needs the device step count and cursor)'),
    ('plan_patch_mode', lambda: _plan(_sched(), i=inp(mode=0)),
     'dmf_train_plan_steps: gather mode, no plan cursor (the batches are consecutive)'),
    ('plan_with_cursor', lambda: _plan(_sched(), i=inp(cursor=P.value)),
     'dmf_train_plan_steps: gather mode, no plan cursor (the batches are consecutive)'),
    ('plan_attention', lambda: _plan(_sched(), s=ATTN), 'dmf_train_plan_steps: late-fusion network only'),
    ('plan_negative_steps', lambda: _plan(_sched(), n_steps=-1), 'dmf_train_plan_steps: negative step count or empty batch'),
    ('plan_empty_batch', lambda: _plan(_sched(), i=inp(B=0)), 'dmf_train_plan_steps: negative step count or empty batch'),
]


@pytest.mark.parametrize('name,call,message', SCHED_REFUSALS, ids=[r[0] for r in SCHED_REFUSALS])
def test_sched_entry_point_refusal(name, call, message):
    from dmf import lib
    assert call() == 1
    assert lib._lib.dmf_last_error().decode() == message


def test_sched_no_ops_launch_nothing():
    assert _optim(_sched(), n=0) == 0                              # n == 0, as dmf_optim_step
    assert _plan(_sched(), n_steps=0) == 0                         # no steps: the loop body never runs
