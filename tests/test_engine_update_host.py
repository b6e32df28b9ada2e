"""CPU: the launch sequence of one train step of both train engines, for every optimiser, loss-scaler, group and net form
they accept — eager (`step`) and from the plan (`run_plan(1, 0)`), TrainEngine's criterion step included — and how the two
engines that take GLOBAL batches (TrainEngine with a criterion, QuaTrainEngine) cut this rank's shard out of them.

The library's entry points are replaced by a recorder: the host-only queries still reach the real library, every launch
returns 0 and is recorded with its scalar arguments and its pointer arguments named by the engine attribute they point
into.  The lib.py wrappers run their real argument marshalling (device checks and the stream are stubbed for CPU
tensors).  The torch.distributed collectives of the step are recorded too, on a one-rank gloo group whose collectives
are kept in the step (`_force_collective`).  `expected_update` below states the update rule after the backward."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

DQTL = {'alpha': 0.1, 'beta': 0.05, 'gamma': 1.0, 'epsilon': 1e-8, 'tao': 0.1}
HOST_QUERIES = ('dmf_version', 'dmf_last_error', 'dmf_shape_supported', 'dmf_patch_variant', 'dmf_param_layout',
                'dmf_workspace_bytes', 'dmf_attn_workspace_bytes', 'dmf_attn_train_workspace_bytes', 'dmf_half_supported',
                'dmf_unit_supported', 'dmf_xgmi_sizes')
# pointer -> name: engine attributes first (a plan may be the caller's own tensor), then the caller's eager batch
NAMED = ('theta', 'm', 'v', 'grad', 'ws', 'attn_ws', 'logits', 'dlogits', 'loss', 'gathered', 'plan_xy', 'plan_labels',
         'dev_step', 'dev_cursor', 'loss_hist')


class Ptr(int):
    """A recorded pointer argument, named when the calls are taken."""


class Recorder:
    """Stand-in for lib._lib."""

    def __init__(self, real):
        self.real, self.calls = real, []

    @staticmethod
    def arg(a):
        if isinstance(a, C.c_void_p):
            return None if a.value is None else Ptr(a.value)
        if isinstance(a, C.c_float):
            return float(np.float32(a.value))
        if isinstance(a, float):
            return float(np.float32(a))
        obj = getattr(a, '_obj', None)           # C.byref(...)
        if isinstance(obj, C.Structure):
            from dmf import lib
            if isinstance(obj, lib.Input):
                return ('input', obj.mode, obj.B) + tuple(None if p is None else Ptr(p) for p in (obj.sceneA, obj.sceneB, obj.xy)) + (
                    obj.Wp, obj.WpB, None if obj.cursor is None else Ptr(obj.cursor), obj.half)
            return {lib.Shape: 'shape', lib.QuaParams: 'params', lib.XgmiComm: 'comm', lib.CeParams: 'ce_params'}[type(obj)]
        return a

    def __getattr__(self, entry):
        if entry in HOST_QUERIES:
            return getattr(self.real, entry)

        def launch(*args):
            self.calls.append((entry,) + tuple(self.arg(a) for a in args))
            return 0
        return launch

    def collective(self, fn, entry):
        def call(*args, **kw):
            t = args[1] if entry == 'all_gather' else args[0]
            self.calls.append((entry, Ptr(t.data_ptr())))
            return fn(*args, **kw)
        return call

    def take(self, eng, **extra):
        """The calls since the last take(), pointers named by the engine's tensor (or one of `extra`) they point into."""
        tensors = {n: getattr(eng, n) for n in NAMED if getattr(eng, n, None) is not None}
        tensors.update(pool_w=eng.net.pool_w, sceneA=eng.scene.A, sceneB=eng.scene.B, **extra)
        if eng.scaler is not None:
            tensors['scaler'] = eng.scaler.state
        if getattr(getattr(eng, 'criterion', None), 'class_w', None) is not None:
            tensors['class_w'] = eng.criterion.class_w

        def name(a):
            if isinstance(a, tuple):
                return tuple(name(x) for x in a)
            if not isinstance(a, Ptr):
                return a
            for n, t in tensors.items():
                lo = t.data_ptr()
                if t.numel() and lo <= a < lo + t.numel() * t.element_size():
                    return n if a == lo else '%s+%d' % (n, a - lo)
            return '?'
        calls, self.calls = [name(c) for c in self.calls], []
        # the stage-2 loss of one rank: dmf_qua_loss_scaled(l, bs, K, ...) is dmf_qua_loss_ranks(l, 1, 0, bs, K, ...)
        return [('dmf_qua_loss_ranks', c[1], 1, 0) + c[2:] if c[0] == 'dmf_qua_loss_scaled' else c for c in calls]


@pytest.fixture(scope='module')
def group(tmp_path_factory):
    import torch.distributed as dist
    dist.init_process_group('gloo', init_method='file://%s' % tmp_path_factory.mktemp('pg').joinpath('store'),
                            rank=0, world_size=1)
    yield dist.group.WORLD
    dist.destroy_process_group()


@pytest.fixture
def rec(monkeypatch):
    import torch.distributed as dist
    from dmf import lib
    r = Recorder(lib._lib)
    monkeypatch.setattr(lib, '_lib', r)
    monkeypatch.setattr(lib, '_dev', lambda t, dtype, name: t)
    monkeypatch.setattr(lib, '_stream', lambda: None)
    for entry in ('all_reduce', 'all_gather', 'all_gather_into_tensor'):
        monkeypatch.setattr(dist, entry, r.collective(getattr(dist, entry), entry))
    return r


def expected_update(e, rows, dev_step, cursor, sum_scale, loss, loss_hist, collective, xgmi):
    """The launches (and collectives) after the backward."""
    sc, step = e.scaler, e.step_count
    hp = (e.lr, e.b1, e.b2, e.eps)
    if sc is None and e.optim == 'ADAM' and not collective:
        return [('dmf_grad_reduce_adam', 'shape', rows, 'ws', 'theta', 'm', 'v', None) + hp +
                (step, dev_step, cursor, loss, loss_hist, None)]
    if sc is None and e.optim == 'ADAM' and xgmi:
        return [('dmf_grad_reduce_xgmi_adam', 'shape', rows, 'ws', 'theta', 'm', 'v', 'comm') + hp +
                (sum_scale, dev_step, cursor, loss, loss_hist, None)]
    n = e.theta.numel()
    scaler = ('scaler', sc.growth_factor, sc.backoff_factor, sc.growth_interval) if sc is not None else ()
    if sc is not None and not collective:
        return [('dmf_grad_reduce_scaled', 'shape', rows, 'ws', 'grad', 'scaler', cursor, loss, loss_hist, None),
                ('dmf_unscale_adam', 'theta', 'grad', 'm', 'v', n) + hp + (1.0,) + scaler + (1, dev_step, None, None)]
    out = [('dmf_grad_reduce', 'shape', rows, 'ws', 'grad', None)]
    if collective:
        out.append(('all_reduce', 'grad'))
    if sc is not None:
        out.append(('dmf_unscale_adam', 'theta', 'grad', 'm', 'v', n) + hp + (sum_scale,) + scaler + (0, dev_step, cursor, None))
    elif e.optim == 'SGD':
        out.append(('dmf_sgd_step', 'theta', 'grad', 'm', n, e.lr, e.momentum, step, sum_scale, dev_step, cursor, None))
    elif e.optim == 'RMSprop':
        out.append(('dmf_rmsprop_step', 'theta', 'grad', 'm', n, e.lr, e.alpha, 1e-8, sum_scale, cursor, None))
    else:
        out.append(('dmf_adam_step', 'theta', 'grad', 'm', 'v', n) + hp + (step, sum_scale, dev_step, cursor, None))
    return out


def _f32(calls):
    """Float arguments as the float32 the C ABI takes (the recorder records them so)."""
    return [tuple(float(np.float32(a)) if isinstance(a, float) else a for a in c) for c in calls]


def _forms():
    for optim in ('ADAM', 'SGD', 'RMSprop'):
        for scaler in (False, True):
            for grp in ('single', 'collective', 'xgmi'):
                for attention in (False, True):
                    if scaler and (optim != 'ADAM' or attention or grp == 'xgmi'):
                        continue
                    if grp == 'xgmi' and optim != 'ADAM':
                        continue
                    yield '%s-%s-%s-%s' % (optim, 'scaler' if scaler else 'fp32', grp, 'attn' if attention else 'late')


def _parse(form):
    optim, scaler, grp, net = form.split('-')
    return optim, scaler == 'scaler', grp, net


# ------------------------------------------------------------------------------------------------ TrainEngine
@pytest.mark.parametrize('form', list(_forms()))
def test_train_engine_step_launches(form, rec, group):
    from dmf import lib
    from dmf.engine import LossScaler, Scene, TrainEngine
    from model.gmfnet import Net
    optim, use_scaler, grp, net_kind = _parse(form)
    cfg = {'patch_size': 11, 'Categories_Number': 17, 'data_city': 's', 'DATA_DICT': {'s': {'size': [40, 40, 200]}},
           'scale': 1, 'aux_bands': 1, 'gmf': {'width': 40, 'hidden': 64, 'pool_sigma': 2.5, 'attention': int(net_kind == 'attn')},
           'trans': {'embed_dim': 96, 'num_head': 3}}
    torch.manual_seed(0)
    net = Net(cfg)
    scene = Scene(np.zeros((50, 50, 200), np.float32), np.zeros((50, 50, 1), np.float32), 'cpu')
    B = 8
    scaler = LossScaler('cpu') if use_scaler else None
    eng = TrainEngine(net, scene, B, lr=2e-3, process_group=None if grp == 'single' else group, scaler=scaler,
                      optimizer=optim, momentum=0.5)
    if grp != 'single':
        eng._force_collective = True
    if grp == 'xgmi':         # (the constructor keeps a communicator only for world > 1)
        eng.comm = types.SimpleNamespace(c=lib.XgmiComm(world=1), world=1, capacity=eng.theta.numel(), rewind=lambda n: None)
    rng = np.random.default_rng(0)
    xy = torch.from_numpy(rng.integers(0, 30, (B, 2)).astype(np.int32))
    labels = torch.from_numpy(rng.integers(0, 17, B).astype(np.int32))
    collective, xgmi = grp != 'single', grp == 'xgmi'
    on_device = xgmi or use_scaler or optim != 'ADAM'

    def forward(dev_step, xy_name, labels_name, cursor):
        inp = ('input', 1, B, 'sceneA', 'sceneB', xy_name, 50, 50, cursor, 0)
        if net_kind == 'attn':
            return [('dmf_train_attn_fwd_bwd', 'shape', inp, 'theta', 'pool_w', labels_name, None, 1.0 / B, 'logits', 'loss',
                     'ws', 'attn_ws', dev_step, None)]
        if use_scaler:
            return [('dmf_train_fwd_bwd_scaled', 'shape', inp, 'theta', 'pool_w', labels_name, 1.0 / B, 'scaler', 'logits',
                     'loss', 'ws', dev_step, None)]
        return [('dmf_train_fwd_bwd', 'shape', inp, 'theta', 'pool_w', labels_name, 1.0 / B, 'logits', 'loss', 'ws',
                 dev_step, None)]

    rec.take(eng)
    eng.step(xy, labels)
    dev = 'dev_step' if on_device else None
    assert rec.take(eng, xy=xy, labels=labels) == _f32(forward(dev, 'xy', 'labels', None) + expected_update(
        eng, B, dev, None, 1.0, None, None, collective, xgmi))

    eng.load_plan(rng.integers(0, 30, (2 * B, 2)).astype(np.int32), rng.integers(0, 17, 2 * B).astype(np.int32))
    rec.take(eng)
    assert eng.run_plan(1, 0) == 1
    assert rec.take(eng) == _f32(forward('dev_step', 'plan_xy', 'plan_labels', 'dev_cursor') + expected_update(
        eng, B, 'dev_step', 'dev_cursor', 1.0, 'loss', 'loss_hist', collective, xgmi))
    assert eng.step_count == 2 and eng.host_cursor == 1


# ------------------------------------------------------------------------------------------------ QuaTrainEngine
def _qua_forms():
    for form in _forms():
        optim, use_scaler, grp, net_kind = _parse(form)
        if net_kind == 'late' and grp != 'xgmi':
            for unit in ('unit', 'nonunit'):
                if not (use_scaler and unit == 'nonunit'):
                    yield '%s-%s-%s-%s' % (optim, 'scaler' if use_scaler else 'fp32', grp, unit)


@pytest.mark.parametrize('form', list(_qua_forms()))
def test_stage2_engine_step_launches(form, rec, group, monkeypatch):
    from dmf import lib
    from dmf.engine import LossScaler, QuaScene, QuaTrainEngine
    from model.gmfnet import Net
    optim, use_scaler, grp, unit = _parse(form)
    unit = unit == 'unit'
    if not unit:
        monkeypatch.setattr(lib, 'unit_supported', lambda shape: False)
    cfg = {'patch_size': 16, 'Categories_Number': 5, 'data_city': 's', 'DATA_DICT': {'s': {'size': [20, 20, 4]}},
           'gmf': {'width': 40, 'single_input': 1}}
    torch.manual_seed(0)
    net = Net(cfg)
    scene = QuaScene([np.zeros((36, 36, 4), np.float32)] * 4, 'cpu')
    bs, K = 8, 5
    scaler = LossScaler('cpu') if use_scaler else None
    eng = QuaTrainEngine(net, scene, bs, DQTL, lr=2e-3, process_group=None if grp == 'single' else group, scaler=scaler,
                         optimizer=optim, momentum=0.5)
    assert eng.unit == unit
    collective = grp != 'single'
    if collective:
        eng._force_collective = True
    rng = np.random.default_rng(0)
    xy = torch.from_numpy(rng.integers(0, 20, (bs, 2)).astype(np.int32))
    labels = torch.from_numpy(rng.integers(0, K, bs).astype(np.int32))

    def launches(dev_step, xy_name, labels_name, cursor, loss_hist):
        inp = ('input', 1, 4 * bs, 'sceneA', 'sceneB', xy_name, 36, 36, cursor, 0)
        if unit:
            out = [('dmf_forward_unit', 'shape', inp, 'theta', 'pool_w', 'logits', 'ws', dev_step, None)]
        else:
            out = [('dmf_forward', 'shape', inp, 'theta', 'pool_w', 'logits', None, None)]
        if collective:
            out.append(('all_gather', 'logits'))
        out.append(('dmf_qua_loss_ranks', 'gathered' if collective else 'logits', 1, 0, bs, K, labels_name, cursor, 'params',
                    1.0, 'scaler' if use_scaler else None, 'loss', loss_hist, 'dlogits', None))
        if unit:
            out.append(('dmf_backward_unit', 'shape', 4 * bs, 'theta', 'dlogits', 'ws', None))
        else:
            out.append(('dmf_backward_dlogits', 'shape', inp, 'theta', 'pool_w', 'dlogits', 'ws', None))
        return out + expected_update(eng, 4 * bs, dev_step if unit else None, cursor, 1.0, None, None, collective, False)

    rec.take(eng)
    eng.step(xy, labels)
    dev = 'dev_step' if use_scaler else None
    assert rec.take(eng, labels=labels) == _f32(launches(dev, '?', 'labels', None, None))

    eng.load_plan(rng.integers(0, 20, (2 * bs, 2)).astype(np.int32), rng.integers(0, K, 2 * bs).astype(np.int32))
    rec.take(eng)
    assert eng.run_plan(1, 0) == 1
    assert rec.take(eng) == _f32(launches('dev_step', 'plan_xy', 'plan_labels', 'dev_cursor', 'loss_hist'))
    assert eng.step_count == 2 and eng.host_cursor == 1


# ------------------------------------------------------------------------------------------------ TrainEngine, criterion step
K17 = 17
CRITERIA = {'ce': {'kind': 'ce', 'label_smoothing': 0.1, 'class_weights': np.linspace(0.5, 2.0, K17).tolist()},
            'focal': {'kind': 'focal', 'gamma': 2.0, 'class_weights': np.linspace(2.0, 0.5, K17).tolist()}}


def _criterion_engine(spec, group=None, scaler=None, optimizer='ADAM', B=8):
    """TrainEngine with a criterion on the late-fusion shape 200/1/11/1/40/10 (the shape of the test above), K = 17."""
    from dmf.engine import Scene, TrainEngine
    from model.gmfnet import Net
    cfg = {'patch_size': 11, 'Categories_Number': K17, 'data_city': 's', 'DATA_DICT': {'s': {'size': [40, 40, 200]}},
           'scale': 1, 'aux_bands': 1, 'gmf': {'width': 40, 'hidden': 64, 'pool_sigma': 2.5, 'attention': 0},
           'trans': {'embed_dim': 96, 'num_head': 3}}
    torch.manual_seed(0)
    scene = Scene(np.zeros((50, 50, 200), np.float32), np.zeros((50, 50, 1), np.float32), 'cpu')
    return TrainEngine(Net(cfg), scene, B, lr=2e-3, process_group=group, scaler=scaler, optimizer=optimizer, momentum=0.5,
                       criterion=CRITERIA[spec])


def _criterion_forms():
    for form in _forms():
        optim, use_scaler, grp, net_kind = _parse(form)
        if net_kind == 'late' and grp != 'xgmi':
            for spec in CRITERIA:
                yield '%s-%s-%s-%s' % (optim, 'scaler' if use_scaler else 'fp32', grp, spec)


@pytest.mark.parametrize('form', list(_criterion_forms()))
def test_train_engine_criterion_step_launches(form, rec, group):
    from dmf.engine import LossScaler
    optim, use_scaler, grp, spec = _parse(form)
    B, K = 8, K17
    collective = grp != 'single'
    eng = _criterion_engine(spec, group if collective else None, LossScaler('cpu') if use_scaler else None, optim, B)
    eng._force_collective = collective
    rng = np.random.default_rng(0)
    xy = torch.from_numpy(rng.integers(0, 30, (B, 2)).astype(np.int32))
    labels = torch.from_numpy(rng.integers(0, K, B).astype(np.int32))

    def launches(dev_step, xy_name, labels_name, cursor, loss, loss_hist):
        inp = ('input', 1, B, 'sceneA', 'sceneB', xy_name, 50, 50, cursor, 0)
        return [('dmf_forward_unit', 'shape', inp, 'theta', 'pool_w', 'logits', 'ws', dev_step, None),
                ('dmf_ce_loss', 'logits', 1, 0, B, K, labels_name, cursor, 'class_w', 'ce_params', 1.0,
                 'scaler' if use_scaler else None, 'loss', 'dlogits', None),
                ('dmf_backward_unit', 'shape', B, 'theta', 'dlogits', 'ws', None)
                ] + expected_update(eng, B, dev_step, cursor, 1.0, loss, loss_hist, collective, False)

    rec.take(eng)
    eng.step(xy, labels)
    dev = 'dev_step' if eng._counts_on_device() else None
    assert (dev is not None) == (use_scaler or optim != 'ADAM')
    assert rec.take(eng, xy=xy, labels=labels) == _f32(launches(dev, 'xy', 'labels', None, None, None))

    eng.load_plan(rng.integers(0, 30, (2 * B, 2)).astype(np.int32), rng.integers(0, K, 2 * B).astype(np.int32))
    rec.take(eng)
    assert eng.run_plan(1, 0) == 1
    assert rec.take(eng) == _f32(launches('dev_step', 'plan_xy', 'plan_labels', 'dev_cursor', 'loss', 'loss_hist'))
    assert eng.step_count == 2 and eng.host_cursor == 1


# ------------------------------------------------------------------------------------------------ this rank's shard of a global batch
WORLD = 3


def _qua_engine(group, bs=8):
    from dmf.engine import QuaScene, QuaTrainEngine
    from model.gmfnet import Net
    cfg = {'patch_size': 16, 'Categories_Number': 5, 'data_city': 's', 'DATA_DICT': {'s': {'size': [20, 20, 4]}},
           'gmf': {'width': 40, 'single_input': 1}}
    torch.manual_seed(0)
    scene = QuaScene([np.zeros((36, 36, 4), np.float32)] * 4, 'cpu')
    return QuaTrainEngine(Net(cfg), scene, bs, DQTL, lr=2e-3, process_group=group)


def _as_rank(eng, rank):
    """A one-rank engine that believes it is `rank` of WORLD ranks (its collectives still run on the one-rank group)."""
    eng.world, eng.rank = WORLD, rank
    return eng


@pytest.mark.parametrize('rank', [0, WORLD - 1])
def test_criterion_load_plan_keeps_this_ranks_rows(rank, group):
    B, n = 8, 2
    eng = _as_rank(_criterion_engine('ce', group, B=B), rank)
    rng = np.random.default_rng(1)
    xy = rng.integers(0, 30, (n * B * WORLD, 2)).astype(np.int32)
    labels = rng.integers(0, K17, n * B * WORLD).astype(np.int32)
    assert eng.load_plan(xy, labels) == n
    assert np.array_equal(eng.plan_xy.numpy(), xy.reshape(n, WORLD, B, 2)[:, rank].reshape(-1, 2))
    assert eng.plan_xy.dtype == torch.int32 and eng.plan_xy.is_contiguous()
    assert np.array_equal(eng.plan_labels.numpy(), labels) and eng.plan_labels.dtype == torch.int32


@pytest.mark.parametrize('rank', [0, WORLD - 1])
def test_stage2_load_plan_keeps_this_ranks_rows(rank, rec, group):          # (rec: QuaScene launches the band mean)
    bs, n = 8, 2
    eng = _as_rank(_qua_engine(group, bs), rank)
    rng = np.random.default_rng(1)
    xy = rng.integers(0, 20, (n * bs * WORLD, 2)).astype(np.int32)
    labels = rng.integers(0, 5, n * bs * WORLD).astype(np.int32)
    assert eng.load_plan(xy, labels) == n
    mine = torch.from_numpy(xy.reshape(n, WORLD, bs, 2)[:, rank].copy())
    want = torch.cat([eng.scene.stack_xy(mine[i]) for i in range(n)])
    assert torch.equal(eng.plan_xy, want) and eng.plan_xy.dtype == torch.int32 and eng.plan_xy.is_contiguous()
    assert np.array_equal(eng.plan_labels.numpy(), labels) and eng.plan_labels.dtype == torch.int32


def _spy(monkeypatch, module, entry, seen):
    real = getattr(module, entry)

    def call(*args, **kw):
        seen.append(args)
        return real(*args, **kw)
    monkeypatch.setattr(module, entry, call)


@pytest.mark.parametrize('rank', [0, WORLD - 1])
def test_criterion_step_trains_on_this_ranks_shard(rank, rec, group, monkeypatch):
    from dmf import lib
    B = 8
    eng = _as_rank(_criterion_engine('ce', group, B=B), rank)
    rng = np.random.default_rng(2)
    xy = torch.from_numpy(rng.integers(0, 30, (WORLD * B + 1, 2)).astype(np.int32))
    labels = torch.from_numpy(rng.integers(0, K17, WORLD * B + 1).astype(np.int32))
    losses = []
    _spy(monkeypatch, lib, 'ce_loss', losses)
    rec.take(eng)
    eng.step(xy, labels)
    calls = rec.take(eng, xy=xy, labels=labels)
    at = 'xy+%d' % (rank * B * 8) if rank else 'xy'
    assert calls[0] == ('dmf_forward_unit', 'shape', ('input', 1, B, 'sceneA', 'sceneB', at, 50, 50, None, 0), 'theta',
                        'pool_w', 'logits', 'ws', 'dev_step' if eng._counts_on_device() else None, None)
    assert calls[1][:7] == ('dmf_ce_loss', 'logits', WORLD, rank, B, K17, 'labels')
    (args,) = losses
    assert args[3].numel() == WORLD * B and torch.equal(args[3], labels[:WORLD * B])
    with pytest.raises(lib.DmfError, match='no pixel each'):
        eng.step(xy[:WORLD - 1], labels[:WORLD - 1])


@pytest.mark.parametrize('rank', [0, WORLD - 1])
def test_stage2_step_trains_on_this_ranks_shard(rank, rec, group, monkeypatch):
    from dmf import lib
    bs, K = 8, 5
    eng = _as_rank(_qua_engine(group, bs), rank)
    # (the logits of the other ranks: nothing gathers them in a one-rank group)
    eng._gather = lambda n: torch.zeros(WORLD * 4 * n, K)
    rng = np.random.default_rng(2)
    xy = torch.from_numpy(rng.integers(0, 20, (WORLD * bs + 1, 2)).astype(np.int32))
    labels = torch.from_numpy(rng.integers(0, K, WORLD * bs + 1).astype(np.int32))
    gathers, losses = [], []
    _spy(monkeypatch, lib, 'input_gather', gathers)
    _spy(monkeypatch, lib, 'qua_loss_ranks', losses)
    rec.take(eng)
    eng.step(xy, labels)
    calls = rec.take(eng, labels=labels)
    (gather,), (loss,) = gathers, losses
    assert torch.equal(gather[3], eng.scene.stack_xy(xy[rank * bs:(rank + 1) * bs])) and gather[3].dtype == torch.int32
    assert calls[0][2][:3] == ('input', 1, 4 * bs)
    assert loss[1:4] == (WORLD, rank, bs)
    assert loss[4].numel() == WORLD * bs and torch.equal(loss[4], labels[:WORLD * bs])
    with pytest.raises(lib.DmfError, match='no pixel each'):
        eng.step(xy[:WORLD - 1], labels[:WORLD - 1])


# ------------------------------------------------------------------------------------------------ one plan upload
def _fused_engine(B=8, attention=0):
    """TrainEngine with the fused step on the shape of the tests above."""
    from dmf.engine import Scene, TrainEngine
    from model.gmfnet import Net
    cfg = {'patch_size': 11, 'Categories_Number': K17, 'data_city': 's', 'DATA_DICT': {'s': {'size': [40, 40, 200]}},
           'scale': 1, 'aux_bands': 1, 'gmf': {'width': 40, 'hidden': 64, 'pool_sigma': 2.5, 'attention': attention},
           'trans': {'embed_dim': 96, 'num_head': 3}}
    torch.manual_seed(0)
    scene = Scene(np.zeros((50, 50, 200), np.float32), np.zeros((50, 50, 1), np.float32), 'cpu')
    return TrainEngine(Net(cfg), scene, B, lr=2e-3)


def _stream(n, B, seed=3):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 30, (n * B, 2)).astype(np.int32), rng.integers(0, K17, n * B).astype(np.int32)


PLAN = ('plan_xy', 'plan_labels', 'plan_pack')


@pytest.mark.parametrize('make', [_fused_engine, lambda: _criterion_engine('ce')], ids=['fused', 'criterion'])
def test_load_block_loads_what_load_plan_loads(make):
    """The same stream through both loaders: the same plan tensors, step count and loss history; under a capacity the rows past
    the plan are zeros and are no steps; blocks of different lengths under one capacity stay in the same tensors."""
    B, n = 8, 3
    xy, labels = _stream(n, B)
    a, b = make(), make()
    assert a.load_plan(xy, labels) == n and b.load_block(xy, labels) == n
    names = PLAN if a.fused else PLAN[:2]
    assert (a.plan_pack is None) == (b.plan_pack is None) == (not a.fused)
    for name in names:
        ta, tb = getattr(a, name), getattr(b, name)
        assert ta.dtype == tb.dtype == torch.int32 and ta.is_contiguous() and tb.is_contiguous() and torch.equal(ta, tb), name
    assert torch.equal(a.plan_xy, torch.from_numpy(xy)) and torch.equal(a.plan_labels, torch.from_numpy(labels))
    if a.fused:
        assert torch.equal(a.plan_pack, torch.cat([a.plan_xy.view(n, 2 * B), a.plan_labels.view(n, B)], 1))
    assert a.plan_steps == b.plan_steps == n and a.loss_hist.shape == b.loss_hist.shape == (n,)
    assert a.host_cursor == b.host_cursor == 0 and not a.loss_hist.any() and not b.loss_hist.any()

    cap = 5
    assert b.load_block(xy, labels, capacity=cap) == n and b.plan_steps == n and b.loss_hist.shape == (cap,)
    for name in names:
        t = getattr(b, name)
        assert t.shape[0] == getattr(a, name).shape[0] // n * cap
        assert torch.equal(t[:getattr(a, name).shape[0]], getattr(a, name)) and not t[getattr(a, name).shape[0]:].any(), name
    where = {name: getattr(b, name).data_ptr() for name in names + ('loss_hist',)}
    xy2, labels2 = _stream(cap, B, seed=4)
    for k in (2, cap, 1):
        assert b.load_block(xy2[:k * B], labels2[:k * B], capacity=cap) == k and b.plan_steps == k
        assert {name: getattr(b, name).data_ptr() for name in where} == where, k
        assert torch.equal(b.plan_xy[:k * B], torch.from_numpy(xy2[:k * B])) and not b.plan_xy[k * B:].any()
        assert torch.equal(b.plan_labels[:k * B], torch.from_numpy(labels2[:k * B])) and not b.plan_labels[k * B:].any()
    from dmf import lib
    with pytest.raises(lib.DmfError, match='plan length must be a multiple of the batch size'):
        b.load_block(xy[:B + 1], labels[:B + 1])
    with pytest.raises(lib.DmfError, match='label outside'):
        b.load_block(xy, labels + K17)


def test_step_short_after_plan_steps_reseeds_the_device_step_counter(rec):
    """An engine that counts on the host (fused ADAM, no scaler): the eager short step takes the host count, and the plan steps
    after it read a device counter that holds it."""
    B, n, r = 8, 2, 3
    eng = _fused_engine(B)
    assert not eng._counts_on_device()
    xy, labels = _stream(2 * n, B)
    sxy, slab = _stream(2, r, seed=5)
    eng.load_block(xy, labels, sxy.reshape(2, r, 2), slab.reshape(2, r))
    assert eng.run_plan(n, 0) == n and int(eng.dev_step) == 0       # (the recorder launches nothing: the kernels count it up)
    rec.take(eng)
    eng.step_short(0)
    inp = ('input', 1, r, 'sceneA', 'sceneB', 'short_xy', 50, 50, None, 0)
    assert rec.take(eng, short_xy=eng.short_xy, short_labels=eng.short_labels) == _f32(
        [('dmf_train_fwd_bwd', 'shape', inp, 'theta', 'pool_w', 'short_labels', 1.0 / r, 'logits', 'loss', 'ws', None, None)]
        + expected_update(eng, r, None, None, 1.0, None, None, False, False))
    assert eng.step_count == n + 1 and int(eng.dev_step) == n + 1 and eng.host_cursor == n
    assert eng.run_plan(1, 0) == 1
    launch = rec.take(eng)[0]
    assert launch[0] == 'dmf_train_fwd_bwd' and launch[-2] == 'dev_step'           # adam_step_dev of the plan step


# ------------------------------------------------------------------------------------------------ one validation-loss form
def _eval_engine(form, B=8):
    from dmf.engine import EvalEngine
    train = _criterion_engine('ce', B=B) if form == 'criterion' else _fused_engine(B, attention=int(form == 'attention'))
    eng = EvalEngine(train.net, train.scene, B, criterion=CRITERIA['ce'] if form == 'criterion' else None)
    eng.logits.zero_()
    return eng


def _launches(rec, call):
    rec.calls = []
    out = call()
    calls, rec.calls = rec.calls, []
    return calls, out


HELPER = {'plain': ['dmf_forward_ce'], 'criterion': ['dmf_forward', 'dmf_ce_loss'], 'attention': []}


@pytest.mark.parametrize('form', sorted(HELPER))
def test_validation_loss_launches(form, rec):
    """`ce_sum` and `valid_accum` launch the same per-patch form; `valid_accum` then sums it by dmf_valid_accum.  The attention
    network has no per-patch form: `ce_sum` says so, `valid_accum` adds torch's cross-entropy of the logits on the device."""
    n = 5
    eng = _eval_engine(form)
    xy, labels = (torch.from_numpy(t) for t in _stream(1, n))
    acc = torch.zeros(1, dtype=torch.float64)
    summed, part = _launches(rec, lambda: eng.ce_sum(xy, labels))
    accum, _ = _launches(rec, lambda: eng.valid_accum(xy, labels, acc))
    assert [c[0] for c in summed] == HELPER[form]
    if form == 'attention':
        assert part is None and [c[0] for c in accum] == ['dmf_forward_attn']
        assert float(acc) == pytest.approx(n * np.log(K17), rel=1e-6)         # (all logits are zero)
    else:
        assert part.dtype == torch.float64 and part.dim() == 0
        assert accum == summed + [('dmf_valid_accum', eng.ce.data_ptr(), n, acc.data_ptr(), None)]
        assert float(acc) == 0.0
    assert _launches(rec, lambda: eng.valid_accum(xy[:0], labels[:0], acc))[0] == []


def test_validation_loss_falls_back_once_where_forward_ce_is_refused(rec, monkeypatch):
    """A shape without dmf_forward_ce: both take torch's cross-entropy on the logits, and the kernel is asked once."""
    from dmf import lib
    n, asked = 5, []

    def refused(*args, **kw):
        asked.append(1)
        raise lib.DmfError('forward_ce: no kernel for this shape')
    monkeypatch.setattr(lib, 'forward_ce', refused)
    xy, labels = (torch.from_numpy(t) for t in _stream(1, n))
    for first in ('ce_sum', 'valid_accum'):
        del asked[:]
        eng = _eval_engine('plain')
        acc = torch.zeros(1, dtype=torch.float64)
        for k in range(2):
            if first == 'ce_sum':
                assert _launches(rec, lambda: eng.ce_sum(xy, labels)) == ([], None)
            calls, _ = _launches(rec, lambda: eng.valid_accum(xy, labels, acc))
            assert [c[0] for c in calls] == ['dmf_forward'] and len(asked) == 1
            assert float(acc) == pytest.approx((k + 1) * n * np.log(K17), rel=1e-6)
