"""GPU: weight decay, AdamW and gradient-norm clipping on the fast path.

* `dmf_optim_step` against torch.optim.{Adam, AdamW, SGD, RMSprop}(weight_decay=) and `clip_grad_norm_` on the CPU, one step
  from a given state, at the sizes around the 256-element block and at the net's own 8,009.
* Its composition with the loss scaler: a skipped step, the unscale, and `dmf_unscale_adam`'s bookkeeping bit for bit.
* The engines' trajectories against the oracle net driven by torch's optimiser and `clip_grad_norm_`, eager and from graphs.
* `Solver.train()` with ADAMW + clip from graphs, epoch by epoch and in blocks; one stage-2 case.
* Two data-parallel ranks over gloo: the norm is that of the all-reduced gradient.
"""
import copy
import functools
import os
import shutil
import tempfile

import numpy as np
import pytest
import torch

from test_gpu_parity import SHAPES, assert_close, make_cfg, nets

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
WD = 0.01
KINDS = ('ADAM', 'ADAMW', 'SGD', 'RMSprop')
HP = dict(ADAM=dict(lr=1e-3), ADAMW=dict(lr=1e-3), SGD=dict(lr=0.05, momentum=0.9), RMSprop=dict(lr=2e-3, alpha=0.9))


def close(got, want, what):
    """The pair tests/test_gpu_parity.py passes to assert_close for dmf_adam_step, (1e-7, 1e-6), read both ways: absolute
    1e-7 + relative 1e-6 as that call binds them, and relative 1e-7 + absolute 1e-6.  Weight decay and the clip coefficient add a
    constant number of roundings per element."""
    assert_close(got, want, 1e-7, 1e-6, what)
    assert_close(got, want, 1e-6, 1e-7, what)


# ---------------------------------------------------------------------------------------------- 1. the kernel against torch
STEP = 6


@functools.lru_cache(maxsize=None)
def _state(n, seed=0):
    g = torch.Generator().manual_seed(seed + n)
    return (torch.randn(n, generator=g), torch.randn(n, generator=g), 0.5 * torch.randn(n, generator=g),
            torch.rand(n, generator=g) + 0.01)


def _torch_step(kind, theta, g, m, v, wd, max_norm, step=STEP):
    """One step of torch's optimiser from the given state; returns (theta, m, v, the norm clip_grad_norm_ returned, coef)."""
    p = torch.nn.Parameter(theta.clone())
    p.grad = g.clone()
    hp = HP[kind]
    if kind in ('ADAM', 'ADAMW'):
        opt = (torch.optim.Adam if kind == 'ADAM' else torch.optim.AdamW)([p], weight_decay=wd, **hp)
        opt.state[p] = {'step': torch.tensor(float(step - 1)), 'exp_avg': m.clone(), 'exp_avg_sq': v.clone()}
    elif kind == 'SGD':
        opt = torch.optim.SGD([p], weight_decay=wd, **hp)
        opt.state[p] = {'momentum_buffer': m.clone()}
    else:
        opt = torch.optim.RMSprop([p], weight_decay=wd, **hp)
        opt.state[p] = {'step': torch.tensor(float(step - 1)), 'square_avg': v.clone()}
    norm = coef = None
    if max_norm:
        norm = float(torch.nn.utils.clip_grad_norm_([p], max_norm, norm_type=2))
        coef = min(1.0, max_norm / (norm + 1e-6))
    opt.step()
    st = opt.state[p]
    if kind in ('ADAM', 'ADAMW'):
        return p.detach(), st['exp_avg'], st['exp_avg_sq'], norm, coef
    return p.detach(), (st['momentum_buffer'] if kind == 'SGD' else st['square_avg']), v, norm, coef


def _dev_state(kind, theta, m, v):
    """The engine's convention: SGD and RMSprop keep their one state vector in m."""
    return theta.to(DEV), (v if kind == 'RMSprop' else m).to(DEV), v.to(DEV)


def _ulps(a, b):
    a, b = np.float32(a), np.float32(b)
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


@pytest.mark.parametrize('clip', ['off', 'half', 'double'])
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('n', [1, 255, 256, 257, 8009])
def test_optim_step_against_torch(n, kind, clip):
    from dmf import lib
    theta, g, m, v = _state(n)
    scale = 0.5
    gs = g * scale
    true_norm = float(np.sqrt((gs.double() ** 2).sum()))
    max_norm = {'off': None, 'half': 0.5 * true_norm, 'double': 2.0 * true_norm}[clip]
    want_t, want_m, want_v, ref_norm, coef = _torch_step(kind, theta, gs, m, v, WD, max_norm)
    if clip == 'half':
        assert coef < 1.0
    if clip == 'double':
        assert coef == 1.0
    th, md, vd = _dev_state(kind, theta, m, v)
    v0 = vd.clone()
    hist = torch.full((4,), -7.0, device=DEV)
    cursor = torch.zeros(1, dtype=torch.int32, device=DEV)
    lib.optim_step(kind, th, g.to(DEV), md, vd, weight_decay=WD, max_norm=max_norm, step=STEP, grad_scale=scale,
                   cursor_dev=cursor, norm_hist=hist, **HP[kind])
    torch.cuda.synchronize()
    close(th, want_t, '%s theta [n=%d, clip %s]' % (kind, n, clip))
    close(md, want_m, '%s m [n=%d, clip %s]' % (kind, n, clip))          # (SGD: the buffer, RMSprop: square_avg)
    if kind in ('ADAM', 'ADAMW'):
        close(vd, want_v, '%s v [n=%d, clip %s]' % (kind, n, clip))
    else:
        assert torch.equal(vd, v0)
    assert int(cursor.item()) == 1                                   # advanced by exactly one
    hist = hist.cpu().numpy()
    assert (hist[1:] == -7.0).all()
    if clip == 'off':
        assert hist[0] == -7.0                                       # max_norm off leaves norm_hist untouched
    else:
        # within 2 fp32 ulp of sqrt of the float64 sum of squares (the squares are exact in double; a reordered double sum
        # moves it by n 2^-52 relative); torch's own fp32 norm for comparison
        print('n=%d %s: norm_hist %.9g, float64 %.9g (%d ulp), torch %.9g' % (n, kind, hist[0], true_norm,
                                                                               _ulps(hist[0], true_norm), ref_norm))
        assert _ulps(hist[0], true_norm) <= 2


def test_optim_step_step_count_from_the_device_and_norm_at_the_cursor():
    """step_dev overrides `step`; the norm goes to norm_hist[*cursor]; SGD's first step (count 1) initialises the buffer."""
    from dmf import lib
    n = 300
    theta, g, m, v = _state(n, 1)
    max_norm = 0.5 * float(g.norm())
    want = _torch_step('ADAMW', theta, g, m, v, WD, max_norm)
    th, md, vd = _dev_state('ADAMW', theta, m, v)
    hist = torch.full((4,), -7.0, device=DEV)
    cursor = torch.full((1,), 2, dtype=torch.int32, device=DEV)
    step_dev = torch.full((1,), STEP, dtype=torch.int32, device=DEV)
    lib.optim_step('ADAMW', th, g.to(DEV), md, vd, weight_decay=WD, max_norm=max_norm, step=1, step_dev=step_dev,
                   cursor_dev=cursor, norm_hist=hist, **HP['ADAMW'])
    close(th, want[0], 'theta by the device step count')
    assert int(cursor.item()) == 3 and int(step_dev.item()) == STEP
    h = hist.cpu().numpy()
    assert (h[[0, 1, 3]] == -7.0).all() and _ulps(h[2], float(np.sqrt((g.double() ** 2).sum()))) <= 2
    # SGD, first step: buf = g + wd theta whatever the buffer held
    p = torch.nn.Parameter(theta.clone())
    p.grad = g.clone()
    opt = torch.optim.SGD([p], weight_decay=WD, **HP['SGD'])
    opt.step()
    th, md, vd = _dev_state('SGD', theta, m, v)
    lib.optim_step('SGD', th, g.to(DEV), md, None, weight_decay=WD, step=1, **HP['SGD'])
    close(th, p.detach(), 'SGD first step theta')
    close(md, opt.state[p]['momentum_buffer'], 'SGD first step buffer')


# ---------------------------------------------------------------------------------------------- 2. with the loss scaler
SCALER = (2.0, 0.5, 3)         # growth factor, backoff factor, growth interval


def _scaler_state(scale, tracker, skipped=0.0):
    return torch.tensor([scale, tracker, 0.0, skipped, 0.0, 0.0, 0.0, 0.0], device=DEV)


@pytest.mark.parametrize('n', [257, 8009])
def test_optim_step_skips_the_whole_step_on_a_non_finite_gradient(n):
    from dmf import lib
    theta, g, m, v = _state(n, 2)
    g = g.clone() * 1024.0
    g[n - 2] = float('inf')
    th, md, vd = _dev_state('ADAMW', theta, m, v)
    before = [t.clone() for t in (th, md, vd)]
    state = _scaler_state(1024.0, 2.0, 5.0)
    step_dev = torch.full((1,), STEP, dtype=torch.int32, device=DEV)
    cursor = torch.full((1,), 1, dtype=torch.int32, device=DEV)
    hist = torch.zeros(4, device=DEV)
    lib.optim_step('ADAMW', th, g.to(DEV), md, vd, weight_decay=WD, max_norm=1.0, step_dev=step_dev, cursor_dev=cursor,
                   scaler_state=state, scaler_hparams=SCALER, norm_hist=hist, **HP['ADAMW'])
    torch.cuda.synchronize()
    for got, was in zip((th, md, vd), before):
        assert torch.equal(got, was)
    s = state.cpu().tolist()
    assert s[0] == 512.0 and s[1] == 0.0 and s[2] == 0.0 and s[3] == 6.0 and s[4] == 0.0     # (s[4]: the ticket, back at 0)
    assert int(step_dev.item()) == STEP - 1 and int(cursor.item()) == 2
    assert not np.isfinite(hist.cpu().numpy()[1])


@pytest.mark.parametrize('kind', ['ADAM', 'ADAMW'])
def test_optim_step_unscales_to_the_same_theta(kind):
    """A finite gradient, scaled by 1024: the same theta, m, v as the unscaled gradient without a scaler state (the scale is a
    power of two: g * 1024 * (0.5 / 1024) is g * 0.5 exactly), and the growth tracker moves on."""
    from dmf import lib
    n = 8009
    theta, g, m, v = _state(n, 3)
    max_norm = 0.5 * float((0.5 * g).norm())
    out = []
    for scaled in (False, True):
        th, md, vd = _dev_state(kind, theta, m, v)
        step_dev = torch.full((1,), STEP, dtype=torch.int32, device=DEV)
        hist = torch.zeros(1, device=DEV)
        kw = dict(scaler_state=_scaler_state(1024.0, 0.0), scaler_hparams=SCALER) if scaled else {}
        lib.optim_step(kind, th, (g * (1024.0 if scaled else 1.0)).to(DEV), md, vd, weight_decay=WD, max_norm=max_norm,
                       grad_scale=0.5, step_dev=step_dev, norm_hist=hist, **kw, **HP[kind])
        out.append((th, md, vd, hist))
        if scaled:
            assert kw['scaler_state'].cpu().tolist()[:4] == [1024.0, 1.0, 0.0, 0.0] and int(step_dev.item()) == STEP
    for a, b in zip(*out):
        assert torch.equal(a, b)
    want = _torch_step(kind, theta, 0.5 * g, m, v, WD, max_norm)
    close(out[1][0], want[0], '%s theta under the scaler' % kind)


@pytest.mark.parametrize('case', ['finite', 'grows', 'inf'])
@pytest.mark.parametrize('n', [255, 8009])
def test_optim_step_with_neutral_keys_is_unscale_adam(n, case):
    """weight decay 0 and no clipping: theta, m, v, the scaler state, the step count and the cursor are bit for bit what
    dmf_unscale_adam(unscaled = 0) leaves on a clone."""
    from dmf import lib
    theta, g, m, v = _state(n, 4)
    g = g.clone() * 256.0
    if case == 'inf':
        g[n // 2] = float('nan')
    tracker = 2.0 if case == 'grows' else 0.0          # interval 3: the third finite step in a row grows the scale
    res = []
    for new in (False, True):
        th, md, vd = _dev_state('ADAM', theta, m, v)
        gd = g.to(DEV)
        state = _scaler_state(256.0, tracker, 1.0)
        step_dev = torch.full((1,), STEP, dtype=torch.int32, device=DEV)
        cursor = torch.full((1,), 4, dtype=torch.int32, device=DEV)
        if new:
            lib.optim_step('ADAM', th, gd, md, vd, 1e-3, 0.9, 0.999, 1e-8, grad_scale=0.5, step_dev=step_dev, cursor_dev=cursor,
                           scaler_state=state, scaler_hparams=SCALER)
            assert torch.equal(gd.cpu(), g) or case == 'inf'         # grad is only read
        else:
            lib.unscale_adam(th, gd, md, vd, 1e-3, 0.9, 0.999, 1e-8, state, *SCALER, step_dev, grad_scale=0.5, cursor_dev=cursor)
        torch.cuda.synchronize()
        res.append((th, md, vd, state, step_dev, cursor))
    for a, b, what in zip(res[0], res[1], ('theta', 'm', 'v', 'scaler state', 'step count', 'cursor')):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), (what, case, n)
    s = res[1][3].cpu().tolist()
    assert s[0] == {'finite': 256.0, 'grows': 512.0, 'inf': 128.0}[case] and int(res[1][5].item()) == 5


# ---------------------------------------------------------------------------------------------- 3. engine trajectories
CASES = {'ADAMW': dict(weight_decay=WD, clip=True), 'ADAM': dict(weight_decay=WD, clip=False),
         'SGD': dict(weight_decay=WD, clip=True), 'RMSprop': dict(weight_decay=0.0, clip=True)}
TORCH = {'ADAM': torch.optim.Adam, 'ADAMW': torch.optim.AdamW, 'SGD': torch.optim.SGD, 'RMSprop': torch.optim.RMSprop}


def _oracle_run(ref, kind, wd, max_norm, batches):
    """The oracle net under torch's optimiser (+ clip_grad_norm_ with max_norm; None: the norms are only measured)."""
    opt = TORCH[kind](ref.parameters(), weight_decay=wd, **HP[kind])
    losses, norms = [], []
    for a, b, t in batches:
        opt.zero_grad()
        loss = torch.nn.functional.cross_entropy(ref(a, b), t)
        loss.backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(ref.parameters(), max_norm if max_norm else float('inf'))))
        opt.step()
        losses.append(loss.item())
    return np.array(losses), np.array(norms)


@pytest.mark.parametrize('kind', sorted(CASES))
def test_engine_trajectory_with_weight_decay_and_clipping(kind):
    """tests/test_gpu_half.py::test_engine_with_the_references_other_optimizers with the new keys: tiny1, 9 steps of 16, its
    tolerances.  max_norm is the median of the oracle's nine norms: the reference must clip on 2 to 7 of the 9 steps."""
    from dmf.engine import Scene, TrainEngine
    from test_gpu_half import cut, scene
    name = 'tiny1'
    C, C2, P, S, K = SHAPES[name]
    n, B, H, W = 9, 16, 23, 19
    A, Bm = scene(name, H, W, 31)
    g = torch.Generator().manual_seed(32)
    xy = torch.stack([torch.randint(0, H, (n * B,), generator=g), torch.randint(0, W, (n * B,), generator=g)], 1).int()
    t = torch.randint(0, K, (n * B,), generator=g)
    batches = [cut(A, Bm, xy[s * B:(s + 1) * B], P, S) + (t[s * B:(s + 1) * B],) for s in range(n)]
    cfg, ref, hip = nets(name)
    wd, clip = CASES[kind]['weight_decay'], CASES[kind]['clip']
    max_norm = None
    if clip:
        max_norm = float(np.median(_oracle_run(copy.deepcopy(ref), kind, wd, None, batches)[1]))
    want, norms = _oracle_run(ref, kind, wd, max_norm, batches)
    if clip:
        clipped = int((norms > max_norm).sum())
        print('%s: max_norm %.6g, reference norms %s, clipped on %d of %d steps' % (kind, max_norm, norms, clipped, n))
        assert 2 <= clipped <= 7
    thetas = []
    for graph in (0, 3):
        hip_g = nets(name)[2]
        eng = TrainEngine(hip_g, Scene(A.numpy(), Bm.numpy(), DEV), B, optimizer=kind, weight_decay=wd, clip_grad_norm=max_norm,
                          **HP[kind])
        eng.load_plan(xy, t)
        eng.run_plan(n, steps_per_graph=graph)
        assert (eng.graph is not None) == bool(graph)
        got = eng.mean_losses().numpy()
        assert np.allclose(got, want, atol=2e-5), (got, want)
        sd = ref.state_dict()
        for k, v in hip_g.state_dict().items():
            assert_close(v, sd[k], 3e-5, 2e-4, '%s (graph %d): param %s after %d steps' % (kind, graph, k, n))
        gn = eng.grad_norms().numpy()
        if clip:
            assert np.allclose(gn, norms, rtol=1e-4, atol=0), (gn, norms)
        else:
            assert not gn.any()
        thetas.append((eng.theta.clone(), eng.m.clone(), eng.v.clone(), gn))
    # a step is bitwise reproducible: the graph's replay equals the eager launches
    for a, b in zip(*thetas):
        assert (a.cpu().numpy() if torch.is_tensor(a) else a).tobytes() == (b.cpu().numpy() if torch.is_tensor(b) else b).tobytes()


def test_neutral_keys_keep_the_fused_launches(monkeypatch):
    """weight_decay 0 and clip_grad_norm None / 0: the native launch loop and the fused reduce + ADAM launch, never
    dmf_optim_step; the same bits as an engine that was never given the keys."""
    from dmf import lib
    from dmf.engine import Scene, TrainEngine
    from test_gpu_half import scene
    name = 'tiny1'
    C, C2, P, S, K = SHAPES[name]
    n, B, H, W = 4, 16, 23, 19
    A, Bm = scene(name, H, W, 31)
    g = torch.Generator().manual_seed(33)
    xy = torch.stack([torch.randint(0, H, (n * B,), generator=g), torch.randint(0, W, (n * B,), generator=g)], 1).int()
    t = torch.randint(0, K, (n * B,), generator=g)
    seen = []
    for entry in ('optim_step', 'train_plan_steps', 'grad_reduce_adam'):
        real = getattr(lib, entry)
        monkeypatch.setattr(lib, entry, lambda *a, _r=real, _e=entry, **kw: seen.append(_e) or _r(*a, **kw))
    out = []
    for kw in ({}, dict(weight_decay=0.0, clip_grad_norm=None), dict(weight_decay=0, clip_grad_norm=0)):
        eng = TrainEngine(nets(name)[2], Scene(A.numpy(), Bm.numpy(), DEV), B, lr=1e-3, **kw)
        assert not eng._regularised() and eng._native_loop_ok()
        eng.load_plan(xy, t)
        eng.run_plan(2, -1)
        eng.run_plan(2, 0)
        out.append(eng.theta.cpu().numpy().tobytes())
    assert out[0] == out[1] == out[2]
    assert seen == ['train_plan_steps', 'grad_reduce_adam', 'grad_reduce_adam'] * 3


# ---------------------------------------------------------------------------------------------- 4. the solvers
SEED = 3407
EPOCHS, SAVE_EVERY, BLOCK = 8, 4, 4


def _solver_cfg(golden_dir, tmp, epoch_block):
    """The tiny synthetic scene of tests/test_gpu_epoch_block.py: 112 train pixels (3 full batches + a short one of 16)."""
    from dmf import synth
    from test_gpu_trajectory import _setup
    _, cfg = _setup(golden_dir, tmp, epoch=EPOCHS, scale=1, batchsize=32, test_batchsize=64, color_batchsize=40,
                    train_rate=0.1, verify_rate=0.05, steps_per_graph=2)
    primary, aux, label = synth.make_scene(40, 40, 8, 1, 1, n_classes=4, seed=3)
    d = cfg['data_address']
    np.save(d + 'ms4.tif.npy', primary); np.save(d + 'pan.tif.npy', aux); np.save(d + 'label.npy', label)
    cfg['DATA_DICT'][cfg['data_city']]['size'] = [40, 40, 8]
    cfg['train'] = dict(cfg['train'], save_every=SAVE_EVERY, epoch_block=epoch_block)
    cfg['schedule'] = dict(cfg['schedule'], optimizer='ADAMW', weight_decay=WD, clip_grad_norm=0.5)
    return cfg


def _solver_run(golden_dir, epoch_block):
    from solver.mainsolver import Solver
    from utils.utils import make_optimizer
    tmp = tempfile.mkdtemp(prefix='dmf_reg_')
    try:
        cfg = _solver_cfg(golden_dir, tmp, epoch_block)
        torch.manual_seed(SEED)
        s = Solver(cfg)
        s.dataloader()
        s.train()
        assert s.engine._regularised() and s.engine.graph is not None
        out = cfg['RESULT_output']
        cur = torch.load(out + '0_curweights.pth', map_location='cpu', weights_only=True)
        fresh = type(s.cur_model)(args=cfg)
        fresh.load_state_dict(cur['state_dict'])
        opt = make_optimizer(cfg, fresh.parameters())
        opt.load_state_dict(cur['optimizer'])
        assert type(opt) is torch.optim.AdamW and opt.param_groups[0]['weight_decay'] == WD
        assert cur['optimizer']['param_groups'][0]['weight_decay'] == WD
        return dict(step_losses=np.array(s.step_losses, dtype=np.float64), cur=cur,
                    best=torch.load(out + '0_weights.pth', map_location='cpu', weights_only=True))
    finally:
        shutil.rmtree(tmp)


def test_solver_adamw_clip_in_blocks_equals_epoch_by_epoch(golden_dir):
    from test_gpu_epoch_block import _same
    one, blk = _solver_run(golden_dir, 1), _solver_run(golden_dir, BLOCK)
    assert len(one['step_losses']) == EPOCHS * 4 and np.isfinite(one['step_losses']).all()
    assert one['step_losses'].tobytes() == blk['step_losses'].tobytes()
    _same(one['best'], blk['best'], 'weights')
    _same(one['cur'], blk['cur'], 'curweights')


def test_stage2_engine_sgd_with_weight_decay_and_clipping():
    """tests/test_gpu_half.py::test_stage2_engine_with_the_references_other_optimizers for SGD + weight decay + clipping: three
    steps, each from the ORACLE's state, with that test's bounds.  max_norm is half the first gradient's norm."""
    from dmf.engine import QuaScene, QuaTrainEngine
    from oracle import datapath_ref as dref
    from oracle.solver_ref import materialise4
    from oracle.gmfnet_ref import Net as RefNet
    from model.gmfnet import Net as HipNet, PARAM_ORDER
    C, C2, P, S, K = SHAPES['qua']
    cfg = make_cfg('qua')
    cfg['gmf']['single_input'] = 1
    torch.manual_seed(5)
    ref = RefNet(cfg)
    hip = HipNet(cfg); hip.load_state_dict(ref.state_dict()); hip = hip.cuda()
    dqtl = {'alpha': 1.0, 'beta': 0.5, 'gamma': 0.5, 'epsilon': 1e-8, 'tao': 2.0}
    g = torch.Generator().manual_seed(6)
    H, W, bs, n = 20, 18, 8, 3
    scenes = [(torch.rand(H + P - 1, W + P - 1, C, generator=g) - 0.2).numpy() for _ in range(4)]
    xy = torch.stack([torch.randint(0, H, (n * bs,), generator=g), torch.randint(0, W, (n * bs,), generator=g)], 1).int()
    lab = torch.randint(0, K, (n * bs,), generator=g)
    lr = 0.05

    def loss_of(net, i):
        data = materialise4(scenes, xy[i * bs:(i + 1) * bs].numpy(), P)
        return dref.qua_loss(net(data), bs, lab[i * bs:(i + 1) * bs].float(), dqtl['alpha'], dqtl['beta'], dqtl['gamma'],
                             dqtl['epsilon'], dqtl['tao'])
    probe = copy.deepcopy(ref)
    loss_of(probe, 0).backward()
    max_norm = 0.5 * float(torch.nn.utils.clip_grad_norm_(probe.parameters(), float('inf')))
    opt = torch.optim.SGD(ref.parameters(), lr=lr, momentum=0.9, weight_decay=WD)
    eng = QuaTrainEngine(hip, QuaScene(scenes, DEV), bs, dqtl, optimizer='SGD', lr=lr, momentum=0.9, weight_decay=WD,
                         clip_grad_norm=max_norm)
    off = hip._offsets
    named = dict(ref.named_parameters())
    clipped = 0
    for i in range(n):
        hip.load_state_dict(ref.state_dict())
        eng.theta = hip.flat_parameters()
        for j, k in enumerate(PARAM_ORDER):
            st = opt.state.get(named[k], {})
            eng.m[off[j]:off[j] + named[k].numel()] = (st['momentum_buffer'].reshape(-1) if 'momentum_buffer' in st
                                                       else torch.zeros(named[k].numel())).cuda()
        eng.step_count = i
        eng.dev_step.fill_(i)
        before = {k: v.detach().clone() for k, v in named.items()}
        opt.zero_grad()
        loss = loss_of(ref, i)
        loss.backward()
        raw = {k: p_.grad.detach().clone() for k, p_ in named.items()}
        norm = float(torch.nn.utils.clip_grad_norm_(ref.parameters(), max_norm))
        clipped += norm > max_norm
        opt.step()
        eng.step(xy[i * bs:(i + 1) * bs], lab[i * bs:(i + 1) * bs])
        assert abs(float(eng.loss.item()) - loss.item()) < 2e-5, (i, float(eng.loss.item()), loss.item())
        assert abs(float(eng.norm.item()) - norm) <= 1e-4 * norm, (i, float(eng.norm.item()), norm)
        got = dict(hip.named_parameters())
        for k, p_ in named.items():
            gr = raw[k].abs()
            solid = gr > 1e-3 * gr.max().clamp_min(1e-30)
            d_ref, d_got = p_.detach() - before[k], got[k].detach().cpu() - before[k]
            err = (d_got - d_ref).abs()
            assert (err[solid] <= 5e-6 + 5e-3 * d_ref.abs()[solid]).all(), (i, k, float(err[solid].max()))
            assert float(err.max()) <= 3.3 * lr, (i, k, float(err.max()))
    assert clipped >= 1


# ---------------------------------------------------------------------------------------------- 5. data parallel
DP_CLIP = 0.1


def _train_dp(rank, world, port, q):
    import torch.distributed as dist
    from test_gpu_dp import B, CFG, STEPS, _problem
    MS, PAN, xy, lab = _problem()
    from dmf.engine import Scene, TrainEngine
    from dmf.parallel import shard_batch
    from model.gmfnet import Net
    pg = None
    if world > 1:
        import datetime
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
        dist.init_process_group('gloo', rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
        pg = dist.group.WORLD
    torch.manual_seed(0)
    net = Net(CFG).to('cuda:0')
    eng = TrainEngine(net, Scene(MS, PAN, 'cuda:0'), (2 * B) // world, lr=1e-2, process_group=pg, optimizer='ADAMW',
                      weight_decay=WD, clip_grad_norm=DP_CLIP)
    gxy, glab = xy.reshape(STEPS, 2 * B, 2), lab.reshape(STEPS, 2 * B)
    lo, hi = shard_batch(2 * B, rank, world)
    eng.load_plan(gxy[:, lo:hi].reshape(-1, 2), glab[:, lo:hi].reshape(-1))
    eng.run_plan(STEPS, 0)
    torch.cuda.synchronize()
    if rank == 0:
        q.put((eng.theta.cpu().numpy(), eng.grad_norms().numpy()))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def test_two_rank_dp_clips_the_all_reduced_gradient():
    """Two ranks over gloo on one GPU against one process on the concatenated batches (tests/test_gpu_dp.py's form and bound):
    the norm and with it the clip coefficient are those of the all-reduced, 1/world-scaled gradient."""
    from test_gpu_dp import STEPS, _run_ranks
    (two, n2), (one, n1) = _run_ranks(_train_dp, 2, ()), _run_ranks(_train_dp, 1, ())
    err = np.abs(two - one).max()
    print('2-rank vs 1-rank parameters after %d clipped steps: max abs diff %.2e; norms %s vs %s' % (STEPS, err, n2, n1))
    assert len(n1) == STEPS and (n1 > DP_CLIP).all()          # every step was clipped: a per-rank norm would show
    assert np.allclose(n2, n1, rtol=1e-5, atol=0)
    assert err < 2e-5
