"""GPU: weight averaging fused into the update.

1. `dmf_weight_average` against torch's AveragedModel on the CPU (tests/avg_ref.py), within a derived bound; the number of
   elements that are not bit-equal is printed (zero where torch.lerp on the CPU is the fused form, which
   tests/test_weight_average_host.py guards).
2. `dmf_optim_step_avg`: theta, m, v and the norm history are the twin's bits, avg is `dmf_weight_average` on the twin's theta;
   a step the loss scaler skips leaves avg alone and does not count.
3. `dmf_grad_reduce_adam_avg` likewise on the smallest late-fusion and attention nets.
4. The engines: eager, graphs and the native loop agree bit for bit in theta and avg; torch's Adam + AveragedModel on the CPU
   oracle.
5. `Solver.train()`: epoch blocks against epoch by epoch, the best weights are the averaged ones, the drop-in path, and
   `weight_average: none` against a run without the key.
"""
import functools
import shutil
import tempfile

import numpy as np
import pytest
import torch

import avg_ref
from test_gpu_parity import SHAPES, _attn_nets, assert_close, nets, rand_batch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
KINDS = ('ADAM', 'ADAMW', 'SGD', 'RMSprop')
SIZES = [1, 255, 256, 257, 8009]
DECAY = 0.9                     # the horizon 1 / (1 - decay) = 10 steps is of the order of the runs below
ULP = 2.0 ** -23


def _bits(*tensors):
    return [t.detach().cpu().numpy().tobytes() for t in tensors]


def _i32(v):
    return torch.full((1,), int(v), dtype=torch.int32, device=DEV)


def _bound(kind, k, scale):
    """|avg - reference| after k averaged (lerp) steps on weights of magnitude <= scale.  One lerp differs from torch's by at
    most 1.5 ulp of a result of magnitude <= scale even where the CPU does not fuse (an fma against a multiply and an add: one
    rounding more, plus the final one), and the recursion carries the earlier error on with the factor 1 - w <= 1: the errors
    sum to at most k of them, and under a constant w to the geometric series' 1 / w.  k = 0 (copies): exactly 0."""
    steps = min(k, 1.0 / (1.0 - DECAY)) if kind == 'ema' else k
    return 1.5 * ULP * scale * steps


def _count(st, src):
    return dict(step=st) if src == 'host' else dict(step=0, step_dev=_i32(st))


# ---------------------------------------------------------------------------------------------- 1. dmf_weight_average
@pytest.mark.parametrize('start', [1, 3])
@pytest.mark.parametrize('kind', ['ema', 'mean'])
@pytest.mark.parametrize('n', SIZES)
def test_weight_average_is_torchs_averaged_model(n, kind, start):
    from dmf import lib
    rng = np.random.default_rng(1000 * n + start)
    thetas = [rng.standard_normal(n).astype(np.float32) for _ in range(6)]
    scale = max(float(np.abs(t).max()) for t in thetas)
    ref = avg_ref.AvgRef(n, kind, DECAY, start)
    want = [ref.update(t) for t in thetas]
    guard = torch.full((n + 16,), -7.0, device=DEV)                       # avg sits inside it: nothing around it may change
    got = {}
    for src in ('dev', 'host'):
        avg = guard[8:8 + n]
        avg.copy_(torch.from_numpy(rng.standard_normal(n).astype(np.float32)))      # (whatever it held: step 1 copies)
        w = lib.weight_avg(avg, kind, DECAY, start)
        unequal = 0
        for st, theta in enumerate(thetas, 1):
            lib.weight_average(w, torch.from_numpy(theta).to(DEV), **_count(st, src))
            a = avg.cpu().numpy()
            err = float(np.abs(a.astype(np.float64) - want[st - 1].astype(np.float64)).max())
            unequal += int((a.view(np.int32) != want[st - 1].view(np.int32)).sum())
            assert err <= _bound(kind, max(0, st - start), scale), (n, kind, start, src, st, err)
        print('n = %d, %s, start %d, count from the %s: %d of %d elements not bit-equal to AveragedModel over 6 steps'
              % (n, kind, start, src, unequal, 6 * n))
        got[src] = a.tobytes()
        g = guard.cpu().numpy()
        assert (g[:8] == -7.0).all() and (g[8 + n:] == -7.0).all()
    assert got['dev'] == got['host']
    assert not np.array_equal(want[-1], thetas[-1])                       # (the average is not the last theta)


# ---------------------------------------------------------------------------------------------- 2. dmf_optim_step_avg
TABLE = np.array([[1.0e-3, 0.90, 0.999, 0.90], [2.5e-3, 0.85, 0.995, 0.80], [7.0e-4, 0.93, 0.990, 0.50], [3.0e-4, 0.80, 0.980, 0.00],
                  [1.3e-2, 0.95, 0.997, 0.65]], dtype=np.float32)
START = 3
# (averaging kind, step count, where it comes from): before, at and past the first averaged step
AVG_CASES = [('ema', 2, 'dev'), ('ema', 3, 'host'), ('ema', 5, 'dev'), ('mean', 5, 'host'), ('mean', 4, 'dev')]


@functools.lru_cache(maxsize=None)
def _state(n):
    g = torch.Generator().manual_seed(900 + n)
    return (torch.randn(n, generator=g), torch.randn(n, generator=g), 0.5 * torch.randn(n, generator=g),
            torch.rand(n, generator=g) + 0.01, torch.randn(n, generator=g))


@pytest.mark.parametrize('sched', [False, True], ids=['launch-args', 'schedule'])
@pytest.mark.parametrize('reg', [False, True], ids=['plain', 'wd_clip'])
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('n', SIZES)
def test_optim_step_avg_is_its_twin_followed_by_weight_average(n, kind, reg, sched):
    from dmf import lib
    theta, g, m, v, avg0 = _state(n)
    table = torch.from_numpy(TABLE).to(DEV)
    keys = dict(eps=1e-8, alpha=0.9)
    if reg:
        keys.update(weight_decay=0.01, max_norm=0.5 * float(g.double().norm()))
    hp = dict(lr=2.5e-3, b1=0.85, b2=0.995, momentum=0.8)
    gd = g.to(DEV)
    for akind, st, src in AVG_CASES:
        out = []
        for fused in (False, True):
            th, md, vd = theta.to(DEV), (v if kind == 'RMSprop' else m).to(DEV), v.to(DEV)     # (RMSprop: m holds square_avg)
            avg, hist = avg0.to(DEV), torch.zeros(2, device=DEV)
            w = lib.weight_avg(avg, akind, DECAY, START)
            if fused:
                lib.optim_step_avg(kind, th, gd, md, vd, w, sched=lib.hp_schedule(table, None) if sched else None,
                                   norm_hist=hist, **(dict() if sched else hp), **keys, **_count(st, src))
            else:
                if sched:
                    lib.optim_step_sched(kind, th, gd, md, vd, lib.hp_schedule(table, None), norm_hist=hist, **keys, **_count(st, src))
                else:
                    lib.optim_step(kind, th, gd, md, vd, norm_hist=hist, **hp, **keys, **_count(st, src))
                lib.weight_average(w, th, **_count(st, src))
            torch.cuda.synchronize()
            out.append(_bits(th, md, vd, hist, avg))
        assert out[0] == out[1], (n, kind, akind, st, src)
        assert out[0][0] != theta.numpy().tobytes() and out[0][4] != avg0.numpy().tobytes()
        if st <= START:
            assert out[1][4] == out[1][0]                                 # copy-through: avg is the new theta


def test_a_skipped_scaler_step_leaves_the_average_alone_and_does_not_count():
    """Three steps with an inf in the second gradient, start 1, kind mean: the second launch leaves avg bit-unchanged and takes
    its count back, and the third averages with n = 1 (w = 1/2) as if the second had not happened."""
    from dmf import lib
    n = 8009
    theta, g, m, v, _ = _state(n)
    grads = [(g * s).to(DEV) for s in (64.0, 64.0, 48.0)]
    grads[1][4321] = float('inf')
    res = {}
    for fused in (False, True):
        th, md, vd = theta.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        avg = torch.zeros(n, device=DEV)
        w = lib.weight_avg(avg, 'mean', start=1)
        state = torch.zeros(lib.SCALER_FLOATS, device=DEV)
        lib.scaler_init(state, 64.0)
        step_dev, seen = _i32(0), []
        for k in range(3):
            step_dev += 1                                                 # (the forward launch's part)
            before, th_before = avg.clone(), th.clone()
            common = dict(lr=1e-3, step_dev=step_dev, scaler_state=state, scaler_hparams=(2.0, 0.5, 2000))
            if fused:
                lib.optim_step_avg('ADAM', th, grads[k], md, vd, w, **common)
            else:
                st = int(step_dev.item())                                 # (read before the launch takes it back)
                lib.optim_step('ADAM', th, grads[k], md, vd, **common)
                if not torch.equal(th, th_before):                        # the twin: average the steps that were taken
                    lib.weight_average(w, th, step=st)
            torch.cuda.synchronize()
            seen.append((int(step_dev.item()), torch.equal(avg, before), torch.equal(avg, th)))
        assert [s[0] for s in seen] == [1, 1, 2]                          # the skipped step took its count back
        assert [s[1] for s in seen] == [False, True, False]               # ... and left avg alone
        assert seen[0][2] and not seen[2][2]                              # step 1 copies, step 2 (the third launch) averages
        res[fused] = _bits(th, md, vd, state, avg)
    assert res[False] == res[True]


# ---------------------------------------------------------------------------------------------- 3. dmf_grad_reduce_adam_avg
def _backward(which, B):
    """One forward + backward into a workspace that the reduce launches below only read."""
    from dmf import lib
    name = 'tiny1'
    cfg, ref, hip = _attn_nets(name) if which == 'attention' else nets(name)
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


@pytest.mark.parametrize('sched', [False, True], ids=['launch-args', 'schedule'])
@pytest.mark.parametrize('which,B', [('late', 3), ('late', 257), ('attention', 2)])
def test_grad_reduce_adam_avg_is_its_twin_followed_by_weight_average(which, B, sched):
    """Every parameter of the net after one fused reduce + ADAM launch from a running state: fc tiles with their bias lanes, conv
    pieces, attention slabs.  Batch 257 is a partial second round of workgroups."""
    from dmf import lib
    table = torch.from_numpy(TABLE).to(DEV)
    shape, theta, ws, loss = _backward(which, B)
    n = theta.numel()
    g = torch.Generator().manual_seed(B)
    m0 = (0.01 * torch.randn(n, generator=g)).to(DEV)
    v0 = (1e-4 * torch.rand(n, generator=g) + 1e-8).to(DEV)
    avg0 = torch.randn(n, generator=g).to(DEV)
    hp = (2.5e-3, 0.85, 0.995)
    for akind, st, src in AVG_CASES:
        out = []
        for fused in (False, True):
            th, m, v, grad, hist, cur = theta.clone(), m0.clone(), v0.clone(), torch.zeros(n, device=DEV), torch.zeros(2, device=DEV), _i32(1)
            avg = avg0.clone()
            w = lib.weight_avg(avg, akind, DECAY, START)
            count = dict(adam_step_dev=_i32(st)) if src == 'dev' else {}
            host = st if src == 'host' else 0
            kw = dict(cursor_dev=cur, loss=loss, loss_hist=hist, **count)
            sc = lib.hp_schedule(table, None) if sched else None
            if fused:
                lib.grad_reduce_adam_avg(shape, B, ws, th, m, v, grad, *((0.0, 0.0, 0.0) if sched else hp), 1e-8, host, w, sched=sc, **kw)
            else:
                if sched:
                    lib.grad_reduce_adam_sched(shape, B, ws, th, m, v, grad, sc, 1e-8, host, **kw)
                else:
                    lib.grad_reduce_adam(shape, B, ws, th, m, v, grad, *hp, 1e-8, host, **kw)
                lib.weight_average(w, th, **_count(st, src))
            torch.cuda.synchronize()
            assert int(cur.item()) == 2
            out.append(_bits(th, m, v, grad, hist, avg))
        assert out[0] == out[1], (which, B, akind, st, src)
        assert out[0][0] != _bits(theta)[0] and out[0][5] != _bits(avg0)[0]
        if st <= START:
            assert out[1][5] == out[1][0]


# ---------------------------------------------------------------------------------------------- 4. the engines
NAME = 'tiny1'
N_STEPS, BATCH, HH, WW, START_STEP = 12, 16, 23, 19, 4
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


def _engine(kw, kind):
    from dmf.engine import Scene, TrainEngine
    A, Bm, xy, t = _problem()
    eng = TrainEngine(nets(NAME)[2], Scene(A.numpy(), Bm.numpy(), DEV), BATCH, lr=0.02 if kw['optimizer'] == 'SGD' else 1e-3,
                      momentum=0.9, **kw)
    eng.set_averaging(kind, DECAY, START_STEP)
    eng.load_plan(xy, t)
    return eng


@functools.lru_cache(maxsize=None)
def _eager(form, kind):
    """12 eager plan steps; after each one the bound against AveragedModel fed the engine's own thetas."""
    eng = _engine(ENGINE_FORMS[form][0], kind)
    assert torch.equal(eng.avg, eng.theta) and eng.avg.data_ptr() != eng.theta.data_ptr()
    ref = avg_ref.AvgRef(eng.theta.numel(), kind, DECAY, START_STEP)
    unequal, scale = 0, 0.0
    for k in range(1, N_STEPS + 1):
        eng.run_plan(1, 0)
        th, a = eng.theta.cpu().numpy(), eng.avg.cpu().numpy()
        want = ref.update(th)
        scale = max(scale, float(np.abs(th).max()))                       # (an average lies between the thetas it has seen)
        err = float(np.abs(a.astype(np.float64) - want.astype(np.float64)).max())
        unequal += int((a.view(np.int32) != want.view(np.int32)).sum())
        assert err <= _bound(kind, max(0, k - START_STEP), scale), (form, kind, k, err)
        assert (a.tobytes() == th.tobytes()) == (k <= START_STEP)
    print('%s, %s: %d elements not bit-equal to AveragedModel over %d eager steps' % (form, kind, unequal, N_STEPS))
    return _bits(eng.mean_losses(), eng.theta, eng.m, eng.v, eng.avg) + [eng.step_count]


@pytest.mark.parametrize('kind', ['ema', 'mean'])
@pytest.mark.parametrize('form', sorted(ENGINE_FORMS))
def test_graphs_and_the_native_loop_equal_eager_steps(form, kind):
    kw, spg = ENGINE_FORMS[form]
    want = _eager('fused_graphs' if form == 'native_loop' else form, kind)
    eng = _engine(kw, kind)
    eng.run_plan(N_STEPS, spg)
    torch.cuda.synchronize()
    assert (eng.graph is not None) == (spg > 0)
    got = _bits(eng.mean_losses(), eng.theta, eng.m, eng.v, eng.avg) + [eng.step_count]
    assert got == want, (form, kind)
    assert got[4] != got[1] and got[5] == N_STEPS


def test_averaging_leaves_the_weights_their_bits():
    """theta, m, v and the losses of the averaging engine (device step count) against the plain engine from graphs."""
    from dmf.engine import Scene, TrainEngine
    A, Bm, xy, t = _problem()
    eng = TrainEngine(nets(NAME)[2], Scene(A.numpy(), Bm.numpy(), DEV), BATCH, lr=1e-3)
    eng.load_plan(xy, t)
    eng.run_plan(N_STEPS, 3)
    torch.cuda.synchronize()
    assert _bits(eng.mean_losses(), eng.theta, eng.m, eng.v) == _eager('fused_graphs', 'ema')[:4]


def test_stage2_engine_averages_from_graphs():
    """QuaTrainEngine (the unit-gradient step around the stage-2 loss) on quatiny: graphs of 2 steps against eager steps."""
    from dmf.engine import QuaScene, QuaTrainEngine
    from model.gmfnet import Net as HipNet
    from test_gpu_parity import make_cfg
    C, C2, P, S, K = SHAPES['quatiny']
    cfg = make_cfg('quatiny')
    cfg['gmf']['single_input'] = 1
    dqtl = {'alpha': 1.0, 'beta': 0.5, 'gamma': 0.5, 'epsilon': 1e-8, 'tao': 2.0}
    g = torch.Generator().manual_seed(6)
    H, W, bs, steps = 20, 18, 8, 6
    scenes = [(torch.rand(H + P - 1, W + P - 1, C, generator=g) - 0.2).numpy() for _ in range(4)]
    xy = torch.stack([torch.randint(0, H, (steps * bs,), generator=g), torch.randint(0, W, (steps * bs,), generator=g)], 1).int()
    lab = torch.randint(0, K, (steps * bs,), generator=g)
    out = []
    for spg in (0, 2):
        torch.manual_seed(5)
        eng = QuaTrainEngine(HipNet(cfg).cuda(), QuaScene(scenes, DEV), bs, dqtl, lr=2e-3)
        assert eng.unit
        eng.set_averaging('ema', DECAY, 3)
        eng.load_plan(xy, lab)
        eng.run_plan(steps, spg)
        torch.cuda.synchronize()
        assert (eng.graph is not None) == (spg > 0)
        out.append(_bits(eng.losses(), eng.theta, eng.m, eng.v, eng.avg))
    assert out[0] == out[1]
    assert out[0][4] != out[0][1]


@pytest.mark.parametrize('kind', ['ema', 'mean'])
def test_engine_average_follows_torchs_adam_and_averaged_model(kind):
    """The same 12 batches through the CPU oracle net with torch.optim.Adam and AveragedModel (avg_ref.AvgRef on the oracle's
    flat parameters).  Tolerance: the parameter tolerance of tests/test_gpu_device_schedule.py's oracle case (3e-5 absolute +
    2e-4 relative at 12 steps) — an average of parameters that are each within a tolerance is within it."""
    from test_gpu_half import cut
    C, C2, P, S, K = SHAPES[NAME]
    A, Bm, xy, t = _problem()
    _, ref, hip = nets(NAME)
    order = hip._order()
    named = dict(ref.named_parameters())
    flat = lambda: torch.cat([named[k].detach().reshape(-1) for k in order]).numpy()
    opt = torch.optim.Adam(ref.parameters(), lr=1e-3)
    avg = avg_ref.AvgRef(sum(named[k].numel() for k in order), kind, DECAY, START_STEP)
    for s in range(N_STEPS):
        a, b = cut(A, Bm, xy[s * BATCH:(s + 1) * BATCH], P, S)
        opt.zero_grad()
        torch.nn.functional.cross_entropy(ref(a, b), t[s * BATCH:(s + 1) * BATCH]).backward()
        opt.step()
        want = avg.update(flat())
    eng = _engine(dict(optimizer='ADAM'), kind)
    assert eng.theta.numel() == want.size
    eng.run_plan(N_STEPS, 3)
    got = eng.avg.cpu()
    print('%s, 12 steps: averaged parameters max abs diff %.2e (raw parameters %.2e)' % (
        kind, float((got - torch.from_numpy(want)).abs().max()), float((eng.theta.cpu() - torch.from_numpy(flat())).abs().max())))
    assert_close(got, torch.from_numpy(want), 3e-5, 2e-4, 'averaged parameters (%s) after %d steps' % (kind, N_STEPS))
    assert not np.array_equal(want, flat())


# ---------------------------------------------------------------------------------------------- 5. the solver
SEED = 3407
EPOCHS = 6
AVERAGING = dict(weight_average='ema', average_decay=0.9, average_start=1)


def _solver_cfg(golden_dir, tmp, epoch_block, schedule, **over):
    """tests/test_gpu_epoch_block.py's scene (40 x 40; 3 full batches of 32 and a short one per epoch), the fused step from
    graphs of 2 steps, 6 epochs, `<t>_curweights.pth` every 5th."""
    from test_gpu_epoch_block import _cfg
    cfg = _cfg(golden_dir, tmp, 'fused_graphs', epoch_block)
    cfg['epoch'] = EPOCHS
    cfg['schedule'] = dict(cfg['schedule'], **schedule)
    cfg.update(over)
    return cfg


def _read(path):
    with open(path, 'rb') as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def _solver_run(golden_dir, epoch_block, averaging, key_present=True):
    """`Solver.train()` once per form: step losses, validation sums, both files (loaded, and their bytes) and per epoch of the
    epoch-by-epoch form the engine's theta and avg as they were when the epoch was recorded."""
    from solver.mainsolver import Solver
    tmp = tempfile.mkdtemp(prefix='dmf_avg_')
    try:
        schedule = dict(AVERAGING) if averaging else (dict(weight_average='none') if key_present else {})
        cfg = _solver_cfg(golden_dir, tmp, epoch_block, schedule)
        torch.manual_seed(SEED)
        s = Solver(cfg)
        s.dataloader()
        hist = []
        record = s._record_epoch

        def recording(epoch, losses, val=None):
            if epoch_block == 1 and s.engine.avg is not None:
                hist.append((s.engine.theta.detach().cpu().clone(), s.engine.avg.detach().cpu().clone()))
            return record(epoch, losses, val)
        s._record_epoch = recording
        s.train()
        out = cfg['RESULT_output']
        net = s.cur_model
        return dict(step_losses=np.array(s.step_losses, dtype=np.float64), vals=np.array(s.val_history), best_epoch=s.best_epoch,
                    hist=hist, order=net._order(), offsets=list(net._offsets), per_epoch=s._steps_per_epoch(),
                    start=s.engine.wavg.start if s.engine.wavg is not None else None,
                    best=torch.load(out + '0_weights.pth', map_location='cpu', weights_only=True),
                    cur=torch.load(out + '0_curweights.pth', map_location='cpu', weights_only=True),
                    best_bytes=_read(out + '0_weights.pth'), cur_bytes=_read(out + '0_curweights.pth'))
    finally:
        shutil.rmtree(tmp)


def _flat(sd, r):
    out = torch.zeros(sum(sd[k].numel() for k in r['order']))
    for k, o in zip(r['order'], r['offsets']):
        out[o:o + sd[k].numel()] = sd[k].reshape(-1)
    return out


def test_blocked_training_with_averaging_equals_epoch_by_epoch(golden_dir):
    from test_gpu_epoch_block import _same
    one, blk = _solver_run(golden_dir, 1, True), _solver_run(golden_dir, 3, True)
    assert one['per_epoch'] == 4 and one['start'] == 1 * 4 + 1             # average_start: 1 epoch of 3 full batches and a short one
    assert len(one['step_losses']) == EPOCHS * 4 and np.isfinite(one['step_losses']).all()
    assert one['step_losses'].tobytes() == blk['step_losses'].tobytes()
    assert one['vals'].tobytes() == blk['vals'].tobytes() and one['best_epoch'] == blk['best_epoch']
    _same(one['best'], blk['best'], 'weights')
    _same(one['cur'], blk['cur'], 'curweights')
    assert list(one['cur'].keys()) == ['state_dict', 'optimizer', 'averaged']


def test_the_best_weights_are_the_averaged_weights_of_the_best_epoch(golden_dir):
    r = _solver_run(golden_dir, 1, True)
    assert len(r['hist']) == EPOCHS
    theta0, avg0 = r['hist'][0]
    assert torch.equal(theta0, avg0)                                      # epoch 0 lies before average_start: a copy
    for theta, avg in r['hist'][1:]:
        assert not torch.equal(theta, avg)
    e = r['best_epoch']
    assert e >= 1, 'the best epoch lies before averaging started: the test would not tell avg from theta'
    theta, avg = r['hist'][e]
    best = _flat(r['best'], r)
    assert best.numpy().tobytes() == avg.numpy().tobytes() and not torch.equal(best, theta)
    # <t>_curweights.pth: the raw weights of the last epoch, and the averaged ones beside them
    theta, avg = r['hist'][-1]
    assert _flat(r['cur']['state_dict'], r).numpy().tobytes() == theta.numpy().tobytes()
    assert _flat(r['cur']['averaged'], r).numpy().tobytes() == avg.numpy().tobytes()
    assert list(r['cur']['averaged'].keys()) == list(r['cur']['state_dict'].keys())


def test_weight_average_none_is_a_run_without_the_key(golden_dir):
    a, b = _solver_run(golden_dir, 1, False, True), _solver_run(golden_dir, 1, False, False)
    assert a['best_bytes'] == b['best_bytes'] and a['cur_bytes'] == b['cur_bytes']
    assert a['step_losses'].tobytes() == b['step_losses'].tobytes() and a['vals'].tobytes() == b['vals'].tobytes()
    assert list(a['cur'].keys()) == ['state_dict', 'optimizer']


def test_solver_averaging_follows_the_drop_in_path(golden_dir):
    """20 optimiser steps (5 epochs of 4) with EMA averaging through `Solver.train()`: the fast path against the drop-in path,
    whose loop updates the average with torch's `_foreach_lerp_`.  Step losses (raw theta, which averaging does not touch): 1e-4
    on every one, the bound of tests/test_gpu_device_schedule.py::test_solver_scheduler_unit_step_follows_the_drop_in_path.  What
    depends on the average:
      * the `averaged` state dicts of the two `<t>_curweights.pth`: 3e-5 absolute + 2e-4 relative, the parameter tolerance of the
        engine's oracle case above — an average of parameters that are each within a tolerance is within it;
      * the validation sums, which both paths take of the averaged weights: n_valid x 1e-4 — the sum is n_valid times a mean
        loss, and a mean loss is held to 1e-4 above.  Compared at the epochs that set a new best: the drop-in pass leaves its
        loop as soon as its running sum passes the best one (mainsolver.py:65-75), so elsewhere its figure is a partial sum;
      * the epochs that set a new best, and with them the best epoch, are the same on both paths.
    A wrong start step, decay or kind on either path moves the second and third."""
    from solver.mainsolver import Solver
    runs = {}
    for fast in (1, 0):
        tmp = tempfile.mkdtemp(prefix='dmf_avg_dropin_')
        try:
            cfg = _solver_cfg(golden_dir, tmp, 1, dict(AVERAGING), fast_path=fast, epoch=5)
            torch.manual_seed(SEED)
            s = Solver(cfg)
            s.dataloader()
            s.train()
            assert s.averaging == ('ema', 0.9, 1)
            cur = torch.load(cfg['RESULT_output'] + '0_curweights.pth', map_location='cpu', weights_only=True)
            runs[fast] = (np.array(s.step_losses), np.array(s.val_history), cur, s.best_epoch, len(s.valid_index_loader.dataset))
            if not fast:
                assert s._avg_steps == 5 * len(s.train_loader) == 20
        finally:
            shutil.rmtree(tmp)
    lf, ld = runs[1][0], runs[0][0]
    assert lf.shape == ld.shape == (20,)
    davg = max(float((runs[1][2]['averaged'][k] - v).abs().max()) for k, v in runs[0][2]['averaged'].items() if v.is_floating_point())
    print('EMA averaging, fast vs drop-in over 20 steps: loss diff %.2e, validation sums %s vs %s, averaged weights diff %.2e' % (
        np.abs(lf - ld).max(), runs[1][1].tolist(), runs[0][1].tolist(), davg))
    assert np.abs(lf - ld).max() < 1e-4
    for k, v in runs[0][2]['averaged'].items():
        if v.is_floating_point():
            assert_close(runs[1][2]['averaged'][k], v, 3e-5, 2e-4, 'averaged %s, fast against drop-in path' % k)
    vf, vd, n_valid = runs[1][1], runs[0][1], runs[1][4]
    assert vf.shape == vd.shape == (5,) and n_valid == runs[0][4] == 56
    new_best = lambda v: [e for e in range(len(v)) if v[e] < min([np.inf] + list(v[:e]))]
    assert new_best(vf) == new_best(vd) and len(new_best(vf)) >= 3       # (several epochs past average_start among them)
    assert runs[1][3] == runs[0][3] == new_best(vf)[-1] >= 1
    for e in new_best(vf):
        assert abs(vf[e] - vd[e]) <= n_valid * 1e-4, (e, vf[e], vd[e])
    for fast in (1, 0):                                                   # both files hold an average that is not the weights
        cur = runs[fast][2]
        assert any(not torch.equal(cur['averaged'][k], v) for k, v in cur['state_dict'].items())
