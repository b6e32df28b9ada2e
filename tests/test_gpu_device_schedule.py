"""GPU: the device-resident lr schedule.  The yardstick is the launch-argument path: the `_sched` entry points do
the same arithmetic on the same fp32 values (the row of the table is the float32 that ctypes makes of the launch argument), so
every comparison with it below is BIT equality, not a tolerance.

* `dmf_optim_step_sched` against `dmf_optim_step`, both units, clamped rows, step counts from the device and from the host;
  the loss scaler's skipped step under unit `step`.
* `dmf_grad_reduce_adam_sched` against `dmf_grad_reduce_adam` on the smallest late-fusion and attention nets.
* The engines: unit `step` from graphs and from the native loop against eager launch-argument steps, torch's OneCycleLR per
  batch on the CPU oracle, one stage-2 case.
* `Solver.train()`: one capture over four epochs, epoch blocks without a host synchronisation, `scheduler_unit: step` against
  the drop-in path.
"""
import functools
import shutil
import tempfile

import numpy as np
import pytest
import torch

from test_gpu_parity import SHAPES, _attn_nets, assert_close, nets, rand_batch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
KINDS = ('ADAM', 'ADAMW', 'SGD', 'RMSprop')

# five rows, every value of a column different
TABLE = np.array([[1.0e-3, 0.90, 0.999, 0.90], [2.5e-3, 0.85, 0.995, 0.80], [7.0e-4, 0.93, 0.990, 0.50], [3.0e-4, 0.80, 0.980, 0.00],
                  [1.3e-2, 0.95, 0.997, 0.65]], dtype=np.float32)
ROWS = len(TABLE)


def _bits(*tensors):
    return [t.detach().cpu().numpy().tobytes() for t in tensors]


def _i32(v):
    return torch.full((1,), int(v), dtype=torch.int32, device=DEV)


def _row_args(table, r):
    """The row as the launch arguments of the unscheduled entry point: python floats that ctypes turns back into the same fp32."""
    lr, b1, b2, mom = (float(x) for x in table[r])
    return dict(lr=lr, b1=b1, b2=b2, momentum=mom)


# ---------------------------------------------------------------------------------------------- 1. dmf_optim_step_sched
@functools.lru_cache(maxsize=None)
def _state(n):
    g = torch.Generator().manual_seed(700 + n)
    return (torch.randn(n, generator=g), torch.randn(n, generator=g), 0.5 * torch.randn(n, generator=g),
            torch.rand(n, generator=g) + 0.01)


# (name, row_dev value or None = unit step, the step count, where the count comes from, the row that must be read)
OPTIM_CASES = [('epoch_row0', 0, 6, 'host', 0), ('epoch_middle', 2, 6, 'host', 2), ('epoch_last', ROWS - 1, 6, 'dev', ROWS - 1),
               ('epoch_past_the_end', ROWS + 4, 6, 'host', ROWS - 1), ('epoch_negative', -3, 6, 'dev', 0)]
for _st, _row in ((1, 0), (ROWS, ROWS - 1), (ROWS + 3, ROWS - 1)):
    for _src in ('dev', 'host'):
        OPTIM_CASES.append(('step_st%d_%s' % (_st, _src), None, _st, _src, _row))


@pytest.mark.parametrize('reg', [False, True], ids=['plain', 'wd_clip'])
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('n', [1, 255, 256, 257, 8009])
def test_optim_step_sched_is_optim_step_on_the_rows_values(n, kind, reg):
    from dmf import lib
    theta, g, m, v = _state(n)
    table = torch.from_numpy(TABLE).to(DEV)
    keys = dict(eps=1e-8, alpha=0.9)
    if reg:
        keys.update(weight_decay=0.01, max_norm=0.5 * float(g.double().norm()))
    gd = g.to(DEV)
    for name, row_dev, st, src, row in OPTIM_CASES:
        out = []
        for sched in (False, True):
            th, md, vd = theta.to(DEV), (v if kind == 'RMSprop' else m).to(DEV), v.to(DEV)     # (RMSprop: m holds square_avg)
            hist = torch.zeros(2, device=DEV)
            count = dict(step=st) if src == 'host' else dict(step=0, step_dev=_i32(st))
            if sched:
                rd = None if row_dev is None else _i32(row_dev)
                lib.optim_step_sched(kind, th, gd, md, vd, lib.hp_schedule(table, rd), norm_hist=hist, **keys, **count)
            else:
                lib.optim_step(kind, th, gd, md, vd, norm_hist=hist, **_row_args(TABLE, row), **keys, **count)
            torch.cuda.synchronize()
            out.append(_bits(th, md, vd, hist))
        assert out[0] == out[1], (name, kind, n)
        assert out[0][0] != theta.numpy().tobytes() or float(TABLE[row, 0]) == 0.0, name          # (the step did move theta)
    # the rows differ in what the kind reads: reading the wrong row cannot go unnoticed
    th0, th1 = theta.to(DEV), theta.to(DEV)
    lib.optim_step(kind, th0, gd, v.to(DEV), v.to(DEV), step=6, **_row_args(TABLE, 0), **keys)
    lib.optim_step(kind, th1, gd, v.to(DEV), v.to(DEV), step=6, **_row_args(TABLE, 2), **keys)
    assert _bits(th0) != _bits(th1)


def test_a_skipped_scaler_step_reads_its_row_again():
    """Unit step, a three-row table, an inf in the second step's gradient: the step is skipped, the count is taken back, and the
    third launch reads row 1 (not row 2).  Everything equals the launch-argument run that is handed rows 0, 1, 1."""
    from dmf import lib
    n = 8009
    theta, g, m, v = _state(n)
    table_h = TABLE[:3].copy()
    table = torch.from_numpy(table_h).to(DEV)
    grads = [(g * s).to(DEV) for s in (64.0, 64.0, 48.0)]
    grads[1][4321] = float('inf')
    scaler = (2.0, 0.5, 2000)
    res = []
    for sched in (False, True):
        th, md, vd = theta.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        state = torch.zeros(lib.SCALER_FLOATS, device=DEV)
        lib.scaler_init(state, 64.0)
        step_dev = _i32(0)
        seen = []
        for k, row in enumerate((0, 1, 1)):
            step_dev += 1                                         # (the forward launch's part)
            before = th.clone()
            common = dict(step_dev=step_dev, scaler_state=state, scaler_hparams=scaler)
            if sched:
                lib.optim_step_sched('ADAM', th, grads[k], md, vd, lib.hp_schedule(table, None), **common)
            else:
                lib.optim_step('ADAM', th, grads[k], md, vd, **dict(_row_args(table_h, row), momentum=0.0), **common)
            torch.cuda.synchronize()
            seen.append((int(step_dev.item()), torch.equal(th, before), state.cpu().tolist()[:4]))
        assert [s[0] for s in seen] == [1, 1, 2]                  # the skipped step took its count back
        assert [s[1] for s in seen] == [False, True, False]       # ... and left theta alone
        assert seen[1][2] == [32.0, 0.0, 0.0, 1.0] and seen[2][2] == [32.0, 1.0, 0.0, 1.0]
        res.append(_bits(th, md, vd, state))
    assert res[0] == res[1]
    # reading row 2 in the third launch would have given another theta
    th, md, vd = theta.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    for k, (row, st) in enumerate(((0, 1), (2, 2))):
        lib.optim_step('ADAM', th, grads[2 * k], md, vd, step=st, grad_scale=1.0 / (64.0, 32.0)[k], **dict(_row_args(table_h, row), momentum=0.0))
    assert _bits(th)[0] != res[0][0]


# ---------------------------------------------------------------------------------------------- 2. dmf_grad_reduce_adam_sched
def _onecycle_table(rows, unit='epoch', optimizer='ADAM', lr=1e-3):
    from utils import utils as u
    cfg = {'epoch': rows, 'schedule': {'optimizer': optimizer, 'lr': lr, 'base_lr': lr / 10, 'momentum': 0.9, 'alpha': 0.9,
                                       'if_scheduler': 1, 'scheduler': 'OneCycleLR'}}
    return u.schedule_table(cfg, rows, unit), cfg


def _backward(which, B):
    """One forward + backward into a workspace that the reduce launches below only read."""
    from dmf import lib
    if which == 'attention':
        name = 'tiny1'
        cfg, ref, hip = _attn_nets(name)
    else:
        name = 'quatiny'                                          # 4 / 1 / 5 / 1 / 40 / 1: the smallest late-fusion instance
        cfg, ref, hip = nets(name)
    a, b, t = rand_batch(name, B)
    K = SHAPES[name][4]
    keep = (a.cuda(), b.cuda())
    inp = lib.input_patches(hip.shape, *keep)
    theta = hip.flat_parameters().detach().clone()
    logits, loss = torch.empty(B, K, device=DEV), torch.empty(B, device=DEV)
    ws = torch.empty(lib.workspace_bytes(hip.shape, B) // 4, device=DEV)
    if which == 'attention':
        aws = torch.empty(lib.attn_train_workspace_bytes(hip.shape, B), dtype=torch.uint8, device=DEV)
        lib.train_attn_fwd_bwd(hip.shape, inp, theta, hip.pool_w, t.int().cuda(), None, 1.0 / B, logits, loss, ws, aws)
    else:
        lib.train_fwd_bwd(hip.shape, inp, theta, hip.pool_w, t.int().cuda(), 1.0 / B, logits, loss, ws)
    torch.cuda.synchronize()
    del keep
    return hip.shape, theta, ws, loss


@pytest.mark.parametrize('which,B', [('late', 3), ('late', 257), ('attention', 2)])
def test_grad_reduce_adam_sched_is_grad_reduce_adam_on_the_rows_values(which, B):
    """The whole theta, m and v after one fused reduce + ADAM launch from a running state, an OneCycleLR table (beta1 differs
    between the rows: wave 4's bias corrections see it).  Batch 257 is a partial second round of workgroups; the attention net
    has the attention-slab blocks."""
    from dmf import lib
    rows = 6
    table_h, _ = _onecycle_table(rows)
    assert len(set(table_h[:, 0].tolist())) == rows and len(set(table_h[:, 1].tolist())) > 2
    table = torch.from_numpy(table_h).to(DEV)
    shape, theta, ws, loss = _backward(which, B)
    n = theta.numel()
    g = torch.Generator().manual_seed(B)
    m0 = (0.01 * torch.randn(n, generator=g)).to(DEV)
    v0 = (1e-4 * torch.rand(n, generator=g) + 1e-8).to(DEV)

    def run(launch):
        th, m, v, grad, hist, cur = theta.clone(), m0.clone(), v0.clone(), torch.zeros(n, device=DEV), torch.zeros(2, device=DEV), _i32(1)
        launch(th, m, v, grad, dict(cursor_dev=cur, loss=loss, loss_hist=hist))
        torch.cuda.synchronize()
        assert int(cur.item()) == 2
        return _bits(th, m, v, grad, hist)

    moved = set()
    for unit, row, st in [('epoch', 0, 7), ('epoch', 3, 7), ('epoch', rows - 1, 7), ('epoch', rows + 2, 7),
                          ('step', 0, 1), ('step', 2, 3), ('step', rows - 1, rows), ('step', rows - 1, rows + 3)]:
        read = min(row, rows - 1)
        hp = _row_args(table_h, read)
        want = run(lambda th, m, v, grad, kw: lib.grad_reduce_adam(
            shape, B, ws, th, m, v, grad, hp['lr'], hp['b1'], hp['b2'], 1e-8, 0, adam_step_dev=_i32(st), **kw))
        rd = _i32(row) if unit == 'epoch' else None
        got = run(lambda th, m, v, grad, kw: lib.grad_reduce_adam_sched(
            shape, B, ws, th, m, v, grad, lib.hp_schedule(table, rd), 1e-8, 0, adam_step_dev=_i32(st), **kw))
        assert got == want, (which, B, unit, row, st)
        assert got[0] != _bits(theta)[0]
        moved.add(got[0])
        # the step count as a host argument: the same kernel arithmetic as from the device
        host = run(lambda th, m, v, grad, kw: lib.grad_reduce_adam_sched(
            shape, B, ws, th, m, v, grad, lib.hp_schedule(table, rd), 1e-8, st, **kw))
        assert host == got, (which, B, unit, row, st, 'host step')
    assert len(moved) >= 6                                        # the rows (and step counts) gave different thetas


# ---------------------------------------------------------------------------------------------- 3. the engines
NAME = 'tiny1'
N_STEPS, BATCH, HH, WW = 12, 16, 23, 19
ENGINE_FORMS = {
    'fused_graphs': (dict(optimizer='ADAM'), 3),
    'native_loop': (dict(optimizer='ADAM'), -1),
    'sgd_graphs': (dict(optimizer='SGD'), 3),
    'adamw_clip_graphs': (dict(optimizer='ADAMW', weight_decay=0.01, clip_grad_norm=0.5), 3),
}


@functools.lru_cache(maxsize=None)
def _problem():
    from test_gpu_half import scene
    C, C2, P, S, K = SHAPES[NAME]
    A, Bm = scene(NAME, HH, WW, 61)
    g = torch.Generator().manual_seed(62)
    xy = torch.stack([torch.randint(0, HH, (N_STEPS * BATCH,), generator=g), torch.randint(0, WW, (N_STEPS * BATCH,), generator=g)], 1).int()
    t = torch.randint(0, K, (N_STEPS * BATCH,), generator=g)
    return A, Bm, xy, t


def _result(eng):
    return _bits(eng.mean_losses(), eng.theta, eng.m, eng.v) + [eng.step_count]


@pytest.mark.parametrize('form', sorted(ENGINE_FORMS))
def test_unit_step_from_graphs_equals_eager_launch_argument_steps(form):
    """OneCycleLR over 12 steps (lr and beta1, or SGD's momentum, change at every step) replayed from graphs of 3 steps, or run
    by the native loop, against eager plan steps on the launch-argument path for which Python sets lr, b1, b2 and momentum before
    every step."""
    from dmf.engine import Scene, TrainEngine
    kw, spg = ENGINE_FORMS[form]
    lr = 0.02 if kw['optimizer'] == 'SGD' else 1e-3
    table, _ = _onecycle_table(N_STEPS, 'step', 'ADAM' if kw['optimizer'] == 'ADAMW' else kw['optimizer'], lr)
    A, Bm, xy, t = _problem()
    out = []
    for sched in (False, True):
        eng = TrainEngine(nets(NAME)[2], Scene(A.numpy(), Bm.numpy(), DEV), BATCH, lr=lr, momentum=0.9, **kw)
        eng.load_plan(xy, t)
        if sched:
            eng.set_schedule(table, 'step')
            eng.run_plan(N_STEPS, spg)
            assert (eng.graph is not None) == (spg > 0)
        else:
            for k in range(N_STEPS):
                eng.lr, eng.b1, eng.b2, eng.momentum = (float(x) for x in table[k])
                eng.run_plan(1, 0)
        torch.cuda.synchronize()
        out.append(_result(eng))
    assert out[0] == out[1], form
    assert out[0][4] == N_STEPS


def test_unit_step_follows_torchs_onecycle_per_batch():
    """The same 12 batches through the CPU oracle net with torch.optim.Adam and torch's OneCycleLR stepped per batch.
    Tolerances: those of tests/test_gpu_optim_reg.py::test_engine_trajectory_with_weight_decay_and_clipping's free-running case
    (losses 2e-5 absolute; parameters 3e-5 absolute + 2e-4 relative), taken at 9 steps there and asked of 12 here."""
    from dmf.engine import Scene, TrainEngine
    from test_gpu_half import cut
    from utils import utils as u
    C, C2, P, S, K = SHAPES[NAME]
    A, Bm, xy, t = _problem()
    table, cfg = _onecycle_table(N_STEPS, 'step')
    _, ref, hip = nets(NAME)
    opt = torch.optim.Adam(ref.parameters(), lr=1e-3)
    sch = u.make_scheduler(opt, cfg, total=N_STEPS)
    want = []
    for s in range(N_STEPS):
        a, b = cut(A, Bm, xy[s * BATCH:(s + 1) * BATCH], P, S)
        opt.zero_grad()
        loss = torch.nn.functional.cross_entropy(ref(a, b), t[s * BATCH:(s + 1) * BATCH])
        loss.backward()
        opt.step()
        if s + 1 < N_STEPS:
            sch.step()
        want.append(loss.item())
    eng = TrainEngine(hip, Scene(A.numpy(), Bm.numpy(), DEV), BATCH, lr=1e-3)
    eng.set_schedule(table, 'step')
    eng.load_plan(xy, t)
    eng.run_plan(N_STEPS, 3)
    got = eng.mean_losses().numpy()
    sd = ref.state_dict()
    perr = max((v.detach().cpu().double() - sd[k].double()).abs().max().item() for k, v in hip.state_dict().items() if k in sd)
    print('OneCycleLR per batch, 12 steps: step losses max abs diff %.2e, parameters max abs diff %.2e' % (
        np.abs(got - np.array(want)).max(), perr))
    assert np.allclose(got, want, atol=2e-5), (got, want)
    for k, v in hip.state_dict().items():
        assert_close(v, sd[k], 3e-5, 2e-4, 'param %s after %d steps' % (k, N_STEPS))


def test_stage2_engine_follows_a_steplr_table_from_graphs():
    """QuaTrainEngine, unit epoch: StepLR(step_size=2, gamma=0.5) over 5 epochs of 2 steps, replayed from graphs of 2 steps,
    against the launch-argument engine whose lr Python sets per epoch (and whose graph is re-captured when it changes)."""
    from dmf.engine import QuaScene, QuaTrainEngine
    from model.gmfnet import Net as HipNet
    from test_gpu_parity import make_cfg
    C, C2, P, S, K = SHAPES['quatiny']
    cfg = make_cfg('quatiny')
    cfg['gmf']['single_input'] = 1
    dqtl = {'alpha': 1.0, 'beta': 0.5, 'gamma': 0.5, 'epsilon': 1e-8, 'tao': 2.0}
    g = torch.Generator().manual_seed(6)
    H, W, bs, per, epochs = 20, 18, 8, 2, 5
    scenes = [(torch.rand(H + P - 1, W + P - 1, C, generator=g) - 0.2).numpy() for _ in range(4)]
    xy = torch.stack([torch.randint(0, H, (epochs * per * bs,), generator=g), torch.randint(0, W, (epochs * per * bs,), generator=g)], 1).int()
    lab = torch.randint(0, K, (epochs * per * bs,), generator=g)
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.Adam([p], lr=2e-3)
    sch = torch.optim.lr_scheduler.StepLR(opt, step_size=2, gamma=0.5)
    table = []
    for _ in range(epochs):
        table.append([opt.param_groups[0]['lr'], 0.9, 0.999, 0.0])
        opt.step(); sch.step()
    table = np.array(table, dtype=np.float32)
    assert len(set(table[:, 0].tolist())) == 3
    out = []
    for sched in (False, True):
        torch.manual_seed(5)
        hip = HipNet(cfg).cuda()
        eng = QuaTrainEngine(hip, QuaScene(scenes, DEV), bs, dqtl, lr=2e-3)
        assert eng.unit
        if sched:
            eng.set_schedule(table, 'epoch')
        losses, captures = [], 0
        for e in range(epochs):
            eng.lr = float(table[e, 0])
            eng.set_epoch(e)
            eng.load_plan(xy[e * per * bs:(e + 1) * per * bs], lab[e * per * bs:(e + 1) * per * bs])
            before = eng.graph
            eng.run_plan(per, per)
            captures += eng.graph is not before
            losses.append(eng.losses())
        torch.cuda.synchronize()
        out.append(_bits(torch.cat(losses), eng.theta, eng.m, eng.v) + [captures])
    assert out[0][:4] == out[1][:4]
    assert out[0][4] == 3 and out[1][4] == 1                      # a capture per lr against one capture


# ---------------------------------------------------------------------------------------------- 4. the solver
SEED = 3407


def _solver_cfg(golden_dir, tmp, epoch_block, device_schedule, epochs=None):
    """tests/test_gpu_epoch_block.py's criterion-from-graphs variant (class weights + label smoothing: the unit-gradient step,
    steps_per_graph 2; 3 full batches and a short one per epoch) with ExponentialLR."""
    from test_gpu_epoch_block import _cfg
    cfg = _cfg(golden_dir, tmp, 'criterion_graphs', epoch_block)
    cfg['schedule'] = dict(cfg['schedule'], if_scheduler=1, scheduler='ExponentialLR', device_schedule=device_schedule)
    if epochs is not None:
        cfg['epoch'] = epochs
    return cfg


@functools.lru_cache(maxsize=None)
def _solver_run(golden_dir, epoch_block, device_schedule, epochs=None):
    """`Solver.train()` once per form: step losses, both checkpoint files, theta, the number of graph captures and, per block
    after the first, whether `_enqueue_block` ran without a host synchronisation."""
    from dmf.engine import TrainEngine
    from solver.mainsolver import Solver
    from test_gpu_epoch_block import _host_reads_raise
    from utils.utils import epoch_hparams
    mp = pytest.MonkeyPatch()
    tmp = tempfile.mkdtemp(prefix='dmf_sched_')
    try:
        cfg = _solver_cfg(golden_dir, tmp, epoch_block, device_schedule, epochs)
        torch.manual_seed(SEED)
        s = Solver(cfg)
        s.dataloader()
        captures, blocks = [], []
        real_capture = TrainEngine._capture
        mp.setattr(TrainEngine, '_capture', lambda self, n: captures.append(n) or real_capture(self, n))
        inner = s._enqueue_block

        def guarded(first, n):
            if not captures:                                      # the block with the first capture: a capture synchronises
                blocks.append((n, None))
                return inner(first, n)
            with _host_reads_raise(mp):
                inner(first, n)
            blocks.append((n, ''))
        s._enqueue_block = guarded
        s.train()
        out = cfg['RESULT_output']
        return dict(step_losses=np.array(s.step_losses, dtype=np.float64), captures=list(captures), blocks=blocks,
                    theta=s.engine.theta.detach().cpu().numpy().tobytes(), sched=s.engine.sched is not None,
                    lr0=cfg['schedule']['lr'], hp_last=dict(epoch_hparams(cfg, cfg['epoch'] - 1)),
                    best=torch.load(out + '0_weights.pth', map_location='cpu', weights_only=True),
                    cur=torch.load(out + '0_curweights.pth', map_location='cpu', weights_only=True))
    finally:
        mp.undo()
        shutil.rmtree(tmp)


def test_one_capture_serves_four_epochs_of_a_scheduler(golden_dir):
    """A criterion (unit-gradient step) from graphs of 2 steps under ExponentialLR, 4 epochs: with `device_schedule: 1` the graph
    is captured exactly once (without it, once per epoch: lr is baked in), and losses, weights and `<t>_curweights.pth` (weights,
    ADAM state, step counts, the parameter group's lr) are the same bits."""
    from test_gpu_epoch_block import _same
    dev = _solver_run(golden_dir, 1, 1, 4)
    assert dev['sched'] and dev['captures'] == [2]
    arg = _solver_run(golden_dir, 1, 0, 4)
    assert not arg['sched'] and arg['captures'] == [2] * 4
    assert len(dev['step_losses']) == 4 * 4 and np.isfinite(dev['step_losses']).all()
    assert dev['step_losses'].tobytes() == arg['step_losses'].tobytes()
    assert dev['theta'] == arg['theta']
    _same(arg['cur'], dev['cur'], 'curweights')
    _same(arg['best'], dev['best'], 'weights')
    group = dev['cur']['optimizer']['param_groups'][0]
    assert group['lr'] == dev['hp_last']['lr'] < dev['lr0']        # the group: the last epoch's lr, the scheduler's own double


def test_a_scheduler_from_graphs_does_not_synchronise_inside_a_block(golden_dir):
    """`epoch_block: 4` with `device_schedule: 1`: every `_enqueue_block` after the one with the first capture runs with every
    host read of a device tensor and every synchronize patched to raise (without the device schedule the re-capture at the next
    lr synchronises there).  Step losses and both checkpoint files equal `epoch_block: 1`, `device_schedule: 0` bit for bit."""
    from test_gpu_epoch_block import BLOCK, EPOCHS, _same
    blk = _solver_run(golden_dir, BLOCK, 1)
    assert blk['captures'] == [2]
    assert [b[0] for b in blk['blocks']] == [4, 1, 4, 1]
    assert blk['blocks'][0][1] is None and [b[1] for b in blk['blocks'][1:]] == ['', '', '']
    one = _solver_run(golden_dir, 1, 0)
    assert len(one['captures']) == EPOCHS
    assert len(one['step_losses']) == EPOCHS * 4
    assert one['step_losses'].tobytes() == blk['step_losses'].tobytes()
    _same(one['best'], blk['best'], 'weights')
    _same(one['cur'], blk['cur'], 'curweights')


def test_solver_scheduler_unit_step_follows_the_drop_in_path(golden_dir):
    """`scheduler_unit: step` with OneCycleLR through `Solver.train()`: the fast path (a table row per optimiser step, the short
    last batch counted) against the drop-in path, whose torch scheduler is stepped after every `optimizer.step()`.  Tolerance:
    tests/test_gpu_trajectory.py::test_fast_path_follows_the_other_optimizers_and_schedulers' 1e-4 on every step loss, on its
    scene and epochs."""
    from solver.mainsolver import Solver
    from test_gpu_trajectory import _setup
    runs = {}
    for fast in (1, 0):
        tmp = tempfile.mkdtemp(prefix='dmf_sched_unit_')
        try:
            g, cfg = _setup(golden_dir, tmp, fast_path=fast, epoch=5)
            cfg['schedule'] = dict(cfg['schedule'], optimizer='ADAM', scheduler='OneCycleLR', if_scheduler=1, lr=2e-3, base_lr=2e-4,
                                   momentum=0.9, alpha=0.9, scheduler_unit='step', device_schedule=fast)
            torch.manual_seed(SEED)
            s = Solver(cfg)
            s.dataloader()
            s.train()
            runs[fast] = np.array(s.step_losses)
            if fast:
                per = s._steps_per_epoch()
                assert s.engine.sched is not None and s.engine.sched.rows == 5 * per and s.engine.hp_row is None
                assert s.engine.step_count == 5 * per
                # the checkpoint's group: the row of the last step taken
                assert s.engine.lr == s._step_groups[-1]['lr'] and s.engine.b1 == s._step_groups[-1]['betas'][0]
            else:
                assert s.scheduler.total_steps == 5 * len(s.train_loader)
        finally:
            shutil.rmtree(tmp)
    lf, ld = runs[1], runs[0]
    assert lf.shape == ld.shape and len(lf) > 5
    print('scheduler_unit: step, OneCycleLR: fast vs drop-in loss diff %.2e over %d steps' % (np.abs(lf - ld).max(), len(lf)))
    assert np.abs(lf - ld).max() < 1e-4
