"""CPU: weight decay, AdamW and gradient-norm clipping above the kernel — the factories and refusals of
utils/utils.py, the checkpoint export, the launch sequence of `_PlanEngine._update` with the keys active and neutral (under the
recording stand-in for the library of tests/test_engine_update_host.py), the exported symbol with its host-side refusals, and
the drop-in loop's `clip_grad_norm_`."""
import ctypes as C
import math
import types

import numpy as np
import pytest
import torch

from test_engine_update_host import (CRITERIA, DQTL, K17, _criterion_engine, _f32, expected_update,   # noqa: F401
                                     group, rec)


def _cfg(optimizer='ADAM', **schedule):
    s = {'optimizer': optimizer, 'lr': 2e-3, 'momentum': 0.5, 'alpha': 0.9, 'loss': 'Criterion', 'if_scheduler': 0}
    s.update(schedule)
    return {'schedule': s, 'Categories_Number': 17, 'epoch': 2}


def _params():
    return [torch.nn.Parameter(torch.randn(3, 2)), torch.nn.Parameter(torch.randn(4))]


# ------------------------------------------------------------------------------------------------ factories
@pytest.mark.parametrize('optimizer, cls', [('ADAM', torch.optim.Adam), ('SGD', torch.optim.SGD), ('RMSprop', torch.optim.RMSprop),
                                            ('ADAMW', torch.optim.AdamW)])
def test_make_optimizer_carries_weight_decay(optimizer, cls):
    from utils.utils import make_optimizer, optim_hparams
    cfg = _cfg(optimizer, weight_decay=0.01, clip_grad_norm=1.5)
    opt = make_optimizer(cfg, _params())
    assert type(opt) is cls and opt.param_groups[0]['weight_decay'] == 0.01 and opt.param_groups[0]['lr'] == 2e-3
    hp = optim_hparams(cfg)
    assert hp['optimizer'] == optimizer and hp['weight_decay'] == 0.01 and hp['clip_grad_norm'] == 1.5


def test_refusals_name_the_key():
    from utils.utils import make_optimizer, optim_hparams
    for bad in (-0.1, float('nan'), float('inf')):
        for fn in (optim_hparams, lambda c: make_optimizer(c, _params())):
            with pytest.raises(ValueError, match='weight_decay'):
                fn(_cfg('SGD', weight_decay=bad))
            with pytest.raises(ValueError, match='clip_grad_norm'):
                fn(_cfg('ADAM', clip_grad_norm=-1.0 if bad < 0 else bad))
    for fn in (optim_hparams, lambda c: make_optimizer(c, _params())):
        with pytest.raises(ValueError, match='ADAMW needs schedule.weight_decay'):
            fn(_cfg('ADAMW'))
    with pytest.raises(ValueError, match='optimizer'):
        optim_hparams(_cfg('LION', weight_decay=0.1))


@pytest.mark.parametrize('optimizer', ['ADAM', 'SGD', 'RMSprop'])
def test_neutral_values_are_todays_hparams(optimizer):
    """`weight_decay: 0`, `clip_grad_norm: null` and 0: the dict without the keys, whose old entries are what they were."""
    from utils.utils import make_optimizer, optim_hparams
    plain = optim_hparams(_cfg(optimizer))
    today = {'optimizer': optimizer, 'lr': 2e-3, 'betas': (0.9, 0.999), 'eps': 1e-8}
    if optimizer == 'SGD':
        today['momentum'] = 0.5
    if optimizer == 'RMSprop':
        today['alpha'] = 0.9
    assert plain == today                # (tests/test_host_cpu.py pins the dict of a schedule without the keys)
    for neutral in ({'weight_decay': 0}, {'weight_decay': None, 'clip_grad_norm': None}, {'weight_decay': 0.0, 'clip_grad_norm': 0}):
        want = dict(today, weight_decay=0.0)
        if 'clip_grad_norm' in neutral:
            want['clip_grad_norm'] = None
        assert optim_hparams(_cfg(optimizer, **neutral)) == want
        a, b = make_optimizer(_cfg(optimizer, **neutral), _params()), make_optimizer(_cfg(optimizer), _params())
        ga, gb = ({k: v for k, v in o.param_groups[0].items() if k != 'params'} for o in (a, b))
        assert type(a) is type(b) and ga == gb


# ------------------------------------------------------------------------------------------------ checkpoint export
@pytest.mark.parametrize('optimizer', ['ADAMW', 'ADAM', 'SGD', 'RMSprop'])
def test_export_optimizer_round_trips(optimizer):
    from utils.utils import export_optimizer, make_optimizer
    cfg = _cfg(optimizer, weight_decay=0.01, clip_grad_norm=1.0)
    params = _params()
    n = sum(p.numel() for p in params)
    m, v = torch.arange(n, dtype=torch.float32), torch.arange(n, dtype=torch.float32) + 100
    opt = export_optimizer(cfg, params, params, [0, 6], m, v, 7, group={'lr': 1e-3})      # (weight_decay: the cfg's, by make_optimizer)
    assert type(opt) is {'ADAMW': torch.optim.AdamW, 'ADAM': torch.optim.Adam, 'SGD': torch.optim.SGD,
                         'RMSprop': torch.optim.RMSprop}[optimizer]
    sd = opt.state_dict()
    assert sd['param_groups'][0]['weight_decay'] == 0.01 and sd['param_groups'][0]['lr'] == 1e-3
    fresh = make_optimizer(cfg, _params())
    assert fresh.param_groups[0]['weight_decay'] == 0.01
    fresh.load_state_dict(sd)
    assert fresh.param_groups[0]['weight_decay'] == 0.01
    key = {'ADAMW': 'exp_avg', 'ADAM': 'exp_avg', 'SGD': 'momentum_buffer', 'RMSprop': 'square_avg'}[optimizer]
    got = torch.cat([fresh.state[p][key].reshape(-1) for p in fresh.param_groups[0]['params']])
    assert torch.equal(got, m)
    if optimizer in ('ADAM', 'ADAMW'):
        assert torch.equal(torch.cat([fresh.state[p]['exp_avg_sq'].reshape(-1) for p in fresh.param_groups[0]['params']]), v)
        assert all(float(fresh.state[p]['step']) == 7 for p in fresh.param_groups[0]['params'])


# ------------------------------------------------------------------------------------------------ the launch sequence of _update
KIND = {'ADAM': 0, 'ADAMW': 1, 'SGD': 2, 'RMSprop': 3}
WD, CLIP = 0.01, 0.75


def expected_regularised(e, rows, dev_step, cursor, sum_scale, collective, norm):
    """dmf_grad_reduce -> all-reduce where the step has a collective -> dmf_optim_step."""
    sc = e.scaler
    out = [('dmf_grad_reduce', 'shape', rows, 'ws', 'grad', None)]
    if collective:
        out.append(('all_reduce', 'grad'))
    scaler = ('scaler', sc.growth_factor, sc.backoff_factor, sc.growth_interval) if sc is not None else (None, 0.0, 0.0, 0)
    out.append(('dmf_optim_step', 'theta', 'grad', 'm', 'v', e.theta.numel(), KIND[e.optim], e.lr, e.b1, e.b2, e.eps, e.momentum,
                e.alpha, e.weight_decay, e.clip_grad_norm, e.step_count, sum_scale, dev_step, cursor) + scaler + (0, norm, None))
    return _f32(out)


def _split(calls):
    """(the launches up to the backward, the update's launches)."""
    at = next(i for i, c in enumerate(calls) if c[0].startswith('dmf_grad_reduce'))
    return calls[:at], calls[at:]


def _late_engine(optim, scaler, grp, criterion=None, **reg):
    from dmf.engine import LossScaler, Scene, TrainEngine
    from model.gmfnet import Net
    cfg = {'patch_size': 11, 'Categories_Number': K17, 'data_city': 's', 'DATA_DICT': {'s': {'size': [40, 40, 200]}},
           'scale': 1, 'aux_bands': 1, 'gmf': {'width': 40, 'hidden': 64, 'pool_sigma': 2.5, 'attention': 0}}
    torch.manual_seed(0)
    scene = Scene(np.zeros((50, 50, 200), np.float32), np.zeros((50, 50, 1), np.float32), 'cpu')
    eng = TrainEngine(Net(cfg), scene, 8, lr=2e-3, process_group=grp, scaler=LossScaler('cpu') if scaler else None,
                      optimizer=optim, momentum=0.5, criterion=criterion, **reg)
    eng._force_collective = grp is not None
    return eng


def _qua_engine(optim, scaler, grp, **reg):
    from dmf.engine import LossScaler, QuaScene, QuaTrainEngine
    from model.gmfnet import Net
    cfg = {'patch_size': 16, 'Categories_Number': 5, 'data_city': 's', 'DATA_DICT': {'s': {'size': [20, 20, 4]}},
           'gmf': {'width': 40, 'single_input': 1}}
    torch.manual_seed(0)
    scene = QuaScene([np.zeros((36, 36, 4), np.float32)] * 4, 'cpu')
    eng = QuaTrainEngine(Net(cfg), scene, 8, DQTL, lr=2e-3, process_group=grp, scaler=LossScaler('cpu') if scaler else None,
                         optimizer=optim, momentum=0.5, **reg)
    eng._force_collective = grp is not None
    return eng


def _run(eng, rec, hi, K):
    """One eager step and one plan step; the recorded calls of each."""
    rng = np.random.default_rng(0)
    xy = torch.from_numpy(rng.integers(0, hi, (8, 2)).astype(np.int32))
    labels = torch.from_numpy(rng.integers(0, K, 8).astype(np.int32))
    rec.take(eng)
    eng.step(xy, labels)
    eager = rec.take(eng, xy=xy, labels=labels, norm=eng.norm)
    eng.load_plan(rng.integers(0, hi, (16, 2)).astype(np.int32), rng.integers(0, K, 16).astype(np.int32))
    rec.take(eng)
    assert eng.run_plan(1, 0) == 1
    return eager, rec.take(eng, norm_hist=eng.norm_hist, norm=eng.norm)


FORMS = [(o, s, g, net) for o in ('ADAM', 'ADAMW', 'SGD', 'RMSprop') for s in (False, True) for g in ('single', 'collective')
         for net in ('late', 'criterion', 'stage2') if not (s and o in ('SGD', 'RMSprop'))]


@pytest.mark.parametrize('optim, scaler, grp, net', FORMS, ids=['-'.join([o, 'scaler' if s else 'fp32', g, n]) for o, s, g, n in FORMS])
def test_update_with_keys_active_is_reduce_allreduce_optim_step(optim, scaler, grp, net, rec, group):
    pg = group if grp == 'collective' else None
    reg = dict(weight_decay=WD, clip_grad_norm=CLIP)

    def make(optim, **kw):
        if net == 'stage2':
            return _qua_engine(optim, scaler, pg, **kw)
        return _late_engine(optim, scaler, pg, CRITERIA['ce'] if net == 'criterion' else None, **kw)
    eng = make(optim, **reg)
    assert eng._regularised() and not getattr(eng, '_native_loop_ok', lambda: False)()
    rows, sum_scale = (32, 1.0) if net == 'stage2' else (8, 1.0)
    hi, K = (20, 5) if net == 'stage2' else (30, K17)
    eager, plan = _run(eng, rec, hi, K)
    # the launches up to the backward are those of the same engine without the keys (ADAMW: of ADAM)
    base = make('ADAM' if optim == 'ADAMW' else optim)
    assert not base._regularised()
    base_eager, base_plan = _run(base, rec, hi, K)
    dev = 'dev_step' if eng._counts_on_device() else None
    assert eng._counts_on_device() == base._counts_on_device()
    head, tail = _split(eager)
    eng.step_count = 1
    assert head == _split(base_eager)[0]
    assert tail == expected_regularised(eng, rows, dev if (net != 'stage2' or eng.unit) else None, None, sum_scale,
                                        grp == 'collective', 'norm')
    head, tail = _split(plan)
    eng.step_count = 2
    assert head == _split(base_plan)[0]
    if net == 'late':                    # the fused step records its loss in the update: the mean loss goes into loss_hist first
        assert eng.loss_hist is not None
    assert tail == expected_regularised(eng, rows, 'dev_step', 'dev_cursor', sum_scale, grp == 'collective', 'norm_hist')
    assert eng.host_cursor == 1 and eng.norm_hist.shape == eng.loss_hist.shape


@pytest.mark.parametrize('optim, scaler, grp, net', [f for f in FORMS if f[0] != 'ADAMW'],
                         ids=['-'.join([o, 'scaler' if s else 'fp32', g, n]) for o, s, g, n in FORMS if o != 'ADAMW'])
def test_update_with_neutral_keys_is_todays_sequence(optim, scaler, grp, net, rec, group):
    pg = group if grp == 'collective' else None

    def make(**kw):
        if net == 'stage2':
            return _qua_engine(optim, scaler, pg, **kw)
        return _late_engine(optim, scaler, pg, CRITERIA['ce'] if net == 'criterion' else None, **kw)
    hi, K = (20, 5) if net == 'stage2' else (30, K17)
    want = _run(make(), rec, hi, K)
    for neutral in (dict(weight_decay=0.0, clip_grad_norm=None), dict(weight_decay=0, clip_grad_norm=0)):
        eng = make(**neutral)
        assert not eng._regularised()
        assert _run(eng, rec, hi, K) == want
    assert not any(c[0] == 'dmf_optim_step' for calls in want for c in calls)
    # ... and today's update rule (tests/test_engine_update_host.py states it)
    eng = make()
    eager, plan = _run(eng, rec, hi, K)
    rows = 32 if net == 'stage2' else 8
    assert _split(plan)[1] == _f32(expected_update(eng, rows, 'dev_step', 'dev_cursor', 1.0, 'loss' if net != 'stage2' else None,
                                                   'loss_hist' if net != 'stage2' else None, grp == 'collective', False))


def test_engine_forms_follow_from_the_keys(rec, group):
    """No native launch loop, no xgmi communicator, a graph re-captured when the values change; engine-side refusals."""
    from dmf import lib
    plain = _late_engine('ADAM', False, None)
    assert plain._native_loop_ok() and not plain._regularised()
    for reg in (dict(weight_decay=WD), dict(clip_grad_norm=CLIP), dict()):
        eng = _late_engine('ADAMW' if not reg else 'ADAM', False, None, **reg)
        assert eng._regularised() and not eng._native_loop_ok()
    eng = _late_engine('ADAM', False, None, weight_decay=WD, clip_grad_norm=CLIP)
    h = eng._hparams()
    eng.clip_grad_norm = 2 * CLIP
    assert eng._hparams() != h
    eng.clip_grad_norm, eng.weight_decay = CLIP, 2 * WD
    assert eng._hparams() != h
    comm = types.SimpleNamespace(c=lib.XgmiComm(world=1), world=1, capacity=eng.theta.numel())
    from dmf.engine import TrainEngine
    with pytest.raises(lib.DmfError, match='weight_decay / clip_grad_norm'):
        TrainEngine(eng.net, eng.scene, 8, process_group=group, comm=comm, weight_decay=WD)
    for bad in (dict(weight_decay=-1.0), dict(weight_decay=float('nan')), dict(clip_grad_norm=-1.0), dict(clip_grad_norm=float('inf'))):
        with pytest.raises(lib.DmfError, match=list(bad)[0]):
            _late_engine('ADAM', False, None, **bad)
    with pytest.raises(lib.DmfError, match='loss scaler'):
        _late_engine('SGD', True, None, weight_decay=WD)
    assert _late_engine('ADAMW', True, None, weight_decay=WD).scaler is not None


def test_solver_keeps_the_xgmi_communicator_out(monkeypatch):
    """Solver._train_engine hands the one-shot exchange to the plain ADAM step only."""
    import dmf.engine
    from solver.mainsolver import Solver
    seen = []
    monkeypatch.setattr(dmf.engine, 'TrainEngine', lambda *a, **kw: seen.append(kw) or kw)
    s = object.__new__(Solver)
    s.comm, s.criterion, s.cur_model, s.scene = 'COMM', None, None, None
    kw = dict(optimizer='ADAM', scaler=None, weight_decay=0.0, clip_grad_norm=None)
    assert s._train_engine(8, kw)['comm'] == 'COMM'
    assert s._train_engine(8, dict(kw, weight_decay=WD))['comm'] is None
    assert s._train_engine(8, dict(kw, clip_grad_norm=CLIP))['comm'] is None
    assert s._train_engine(8, dict(kw, optimizer='ADAMW', weight_decay=WD))['comm'] is None


# ------------------------------------------------------------------------------------------------ the exported entry point
def test_library_exports_optim_step():
    from dmf import lib
    assert lib.version() >= 305 and 'dmf_optim_step' in lib.EXPORTS and callable(lib.optim_step)
    assert lib.OPTIM_KINDS == KIND


def test_optim_step_host_side_refusals():
    """Every refusal returns before anything touches a GPU: non-zero, and dmf_last_error() says why."""
    from dmf import lib
    L = lib._lib
    buf = (C.c_float * 8)()
    p = C.cast(buf, C.c_void_p)

    def call(theta=p, grad=p, m=p, v=p, n=8, kind=0, wd=0.0, max_norm=0.0, step=1, step_dev=None, state=None, growth=0.0,
             backoff=0.0, interval=0, unscaled=0, momentum=0.5):
        rc = L.dmf_optim_step(theta, grad, m, v, n, kind, 1e-3, 0.9, 0.999, 1e-8, momentum, 0.99, wd, max_norm, step, 1.0,
                              step_dev, None, state, growth, backoff, interval, unscaled, None, None)
        return rc, L.dmf_last_error().decode()
    for kw, text in ((dict(theta=None), 'null theta or grad'), (dict(grad=None), 'null theta or grad'),
                     (dict(m=None), 'null m or v'), (dict(v=None, kind=1), 'null m or v'),
                     (dict(m=None, kind=2), 'null m or v'), (dict(m=None, kind=3), 'null m or v'),
                     (dict(n=-1), 'negative n'), (dict(kind=4), 'unknown kind'), (dict(kind=-1), 'unknown kind'),
                     (dict(wd=-0.01), 'weight_decay'), (dict(wd=math.nan), 'weight_decay'), (dict(wd=math.inf), 'weight_decay'),
                     (dict(max_norm=math.nan), 'max_norm'), (dict(max_norm=math.inf), 'max_norm'),
                     (dict(growth=2.0, backoff=0.5, interval=2000), 'without a scaler state'),
                     (dict(unscaled=1), 'without a scaler state'),
                     (dict(state=p, growth=2.0, backoff=0.5, interval=2000), 'device step count'),
                     (dict(step=0), 'step must be positive')):
        rc, err = call(**kw)
        assert rc != 0 and text in err, (kw, rc, err)
    # what passes the checks and launches nothing: an empty vector; SGD without momentum needs no buffer
    assert call(n=0)[0] == 0
    assert call(n=0, kind=2, m=None, v=None, momentum=0.0)[0] == 0


# ------------------------------------------------------------------------------------------------ the drop-in loops
class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fc = torch.nn.Linear(4, 3)

    def forward(self, a, b=None):
        return self.fc(a)


def _dropin_solver(cls, cfg, batches):
    s = object.__new__(cls)
    s.cfg, s.DEVICE, s.epoch, s.time = cfg, 'cpu', 0, 0
    torch.manual_seed(0)
    s.cur_model = _Tiny()
    from utils.utils import make_optimizer
    s.optimizer = make_optimizer(cfg, s.cur_model.parameters())
    s.train_loader = batches
    return s


@pytest.mark.parametrize('clip', [None, 0, 0.05])
def test_dropin_loops_clip_once_per_step_when_the_key_is_set(clip, monkeypatch):
    from solver.mainsolver import Solver
    from solver.tostagesolver import toStageSolver
    calls = []
    real = torch.nn.utils.clip_grad_norm_

    def counted(params, max_norm, *a, **kw):
        calls.append(float(max_norm))
        return real(params, max_norm, *a, **kw)
    monkeypatch.setattr(torch.nn.utils, 'clip_grad_norm_', counted)
    cfg = _cfg('SGD', weight_decay=0.01)
    cfg['nohup'] = 1
    if clip is not None:
        cfg['schedule']['clip_grad_norm'] = clip
    torch.manual_seed(1)
    x, y = torch.randn(3, 5, 4), torch.randint(0, 3, (3, 5))
    s = _dropin_solver(Solver, cfg, [(x[i], x[i], y[i], 0, 0) for i in range(3)])
    s.loss = torch.nn.CrossEntropyLoss()
    assert len(s._train_epoch_dropin()) == 3
    assert calls == ([0.05] * 3 if clip else [])
    del calls[:]
    s = _dropin_solver(toStageSolver, cfg, [(x[i], x[i], x[i], x[i], y[i], 0, 0) for i in range(3)])
    s.loss = lambda output, bs, target, cfg: torch.nn.functional.cross_entropy(output[:bs], target)
    assert len(s._train_epoch_dropin()) == 3
    assert calls == ([0.05] * 3 if clip else [])
