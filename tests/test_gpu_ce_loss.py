"""GPU: class weights, label smoothing and focal loss on the fast path.

* `dmf_ce_loss` against the torch statement of the criteria (tests/loss_ref.py) evaluated in float64 on the same logits.
  Tolerance, per evaluation: the same statement evaluated in float32 deviates from float64 by some amount (another order of
  summation, another exp / log); the kernel may deviate by at most 4x that plus 1e-7 absolute.  The gradient is held to
  exactly that.  The value, mean(loss), gets one more term, the mean over the rows of half a float32 ulp of loss[i]: the
  storage format of the per-sample terms, whose reason loss_ref.value_bound states (DESIGN.md §12 has the counts).
* Ranks: a rank's rows are bit-identical to the same rows of the one-rank call on the whole batch, also through a cursor.
* TrainEngine(criterion=...) — the unit-gradient step around the loss kernel — against the CPU oracle net trained with the torch
  criterion and torch's optimiser, at the tolerances tests/test_gpu_parity.py uses for the default criterion (step loss 1e-5,
  parameters 2e-5 absolute + 1e-4 relative): eager and from graphs, SGD, fp16 scene + loss scaler, two gloo ranks.
* Solver(cfg).run() with the new schedule keys: fast path against the drop-in path.
"""
import os
import shutil
import sys
import tempfile

import numpy as np
import pytest
import torch

import loss_ref
from loss_ref import VARIANTS, class_weights, logit_sets
from test_gpu_parity import SHAPES, assert_close, nets

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, 'dual-modal-fusion_amd')


# ---------------------------------------------------------------------------------------------- 1. the kernel


def run_kernel(z, y, spec, w, ranks=1, rank=0, cursor=None, labels=None, grad_scale=1.0, scaler_state=None):
    from dmf import lib
    zd = z.cuda().contiguous()
    loss = torch.full((z.shape[0],), float('nan'), device='cuda')
    dl = torch.full(tuple(z.shape), float('nan'), device='cuda')
    lib.ce_loss(zd, ranks, rank, (y if labels is None else labels).int().cuda(), lib.ce_params(spec['kind'], spec.get('eps', 0.0), spec.get('gamma', 0.0)),
                class_w=None if w is None else w.cuda(), loss=loss, dlogits=dl, cursor=cursor, grad_scale=grad_scale,
                scaler_state=scaler_state)
    return loss.cpu(), dl.cpu()


@pytest.mark.parametrize('bs_r', loss_ref.BS_RS)
@pytest.mark.parametrize('K', loss_ref.KS)
def test_kernel_against_torch_float64(K, bs_r):
    """K: both lane mappings (16 lanes per sample up to K = 16, a wave beyond) and their edges; bs_r: partial groups, a partial
    last workgroup, several workgroups.  Every evaluation is held to ITS OWN float32 deviation (see the module text)."""
    y, sets, w_all = loss_ref.case(K, bs_r)
    worst = [0.0, 0.0]
    plain = {}
    for name, z in sets.items():
        for vname, spec, weighted in VARIANTS:
            w = w_all if weighted else None
            ref = loss_ref.ref_spec(spec, w)
            v64, g64 = loss_ref.value_and_grad(z, y, torch.float64, **ref)
            v32, g32 = loss_ref.value_and_grad(z, y, torch.float32, **ref)
            dev_v, dev_g = (v32 - v64).abs().item(), (g32 - g64).abs().max().item()
            loss, dl = run_kernel(z, y, spec, w)
            assert torch.isfinite(loss).all() and torch.isfinite(dl).all(), (name, vname)
            err_v = (loss.double().mean() - v64).abs().item()
            err_g = (dl.double() - g64).abs().max().item()
            tol_v, tol_g = loss_ref.value_bound(dev_v, loss), 4 * dev_g + 1e-7
            print('K=%d bs_r=%d %s %-15s value %.6g: float32 %.2e kernel %.2e bound %.2e (storage term %.2e) | gradient: float32 %.2e kernel %.2e bound %.2e'
                  % (K, bs_r, name, vname, v64.item(), dev_v, err_v, tol_v, tol_v - 4 * dev_v - 1e-7, dev_g, err_g, tol_g))
            worst = [max(worst[0], err_v / tol_v), max(worst[1], err_g / tol_g)]
            assert err_v <= tol_v, (name, vname, err_v, dev_v, tol_v)
            assert err_g <= tol_g, (name, vname, err_g, dev_g)
            if vname in ('plain', 'weights'):
                plain[(name, weighted)] = (loss, dl)
            if vname.startswith('focal0'):                 # gamma = 0 reproduces kind 0 with eps = 0
                assert torch.equal(loss, plain[(name, weighted)][0]) and torch.equal(dl, plain[(name, weighted)][1]), (name, vname)
        # all-ones weights change nothing
        ones = run_kernel(z, y, dict(kind='ce'), torch.ones(K))
        assert torch.equal(ones[0], plain[(name, False)][0]) and torch.equal(ones[1], plain[(name, False)][1])
    print('K=%d bs_r=%d: worst error / bound: value %.3f gradient %.3f' % (K, bs_r, worst[0], worst[1]))


def test_value_only_and_grad_scale():
    """dlogits = NULL (the validation form) gives the same loss; grad_scale and the scaler state multiply the gradient."""
    from dmf import lib
    g = torch.Generator().manual_seed(5)
    K, n = 17, 70
    y, sets = logit_sets(K, n, g)
    w = class_weights(K, g)
    z = sets['unit']
    spec = dict(kind='ce', eps=0.1)
    loss, dl = run_kernel(z, y, spec, w)
    only = torch.zeros(n, device='cuda')
    lib.ce_loss(z.cuda(), 1, 0, y.int().cuda(), lib.ce_params('ce', 0.1), class_w=w.cuda(), loss=only)
    assert torch.equal(only.cpu(), loss)
    state = torch.zeros(lib.SCALER_FLOATS, device='cuda')
    lib.scaler_init(state, 1024.0)
    _, dl2 = run_kernel(z, y, spec, w, grad_scale=0.5, scaler_state=state)
    assert torch.equal(dl2, dl * 512.0)                    # a power of two: exact
    for bad in (dict(kind='ce', label_smoothing=1.0), dict(kind='ce', label_smoothing=-0.1), dict(kind='focal', gamma=0.5),
                dict(kind='focal', gamma=-1.0)):
        with pytest.raises(lib.DmfError):
            lib.ce_loss(z.cuda(), 1, 0, y.int().cuda(), lib.ce_params(**bad), loss=only)
    with pytest.raises(lib.DmfError):
        lib.ce_loss(z.cuda(), 1, 0, y.int().cuda(), lib.CeParams(kind=2, label_smoothing=0.0, gamma=0.0), loss=only)
    with pytest.raises(lib.DmfError):
        lib.ce_loss(torch.zeros(4, 65, device='cuda'), 1, 0, torch.zeros(4, dtype=torch.int32, device='cuda'), lib.ce_params(), loss=only)
    with pytest.raises(lib.DmfError):
        lib.ce_loss(z.cuda(), 2, 2, y.int().cuda(), lib.ce_params(), loss=only)


@pytest.mark.parametrize('bs_r,K', [(1, 5), (7, 16), (24, 17), (300, 33)])
@pytest.mark.parametrize('W', [1, 2, 3, 8])
def test_ranks_are_bit_identical(W, bs_r, K):
    """ranks = W, rank = r on rank r's rows against the one-rank call on the whole batch: the same rows bit for bit, the rank
    means of `loss` average to the one-rank mean; two plan rows through a cursor that a device kernel advances."""
    from dmf import lib
    g = torch.Generator().manual_seed(1000 * W + bs_r + K)
    N, NS = W * bs_r, 2
    z = 3.0 * torch.randn(NS, N, K, generator=g)
    lab = torch.randint(0, K, (NS * N,), generator=g)
    w = class_weights(K, g)
    cur = torch.zeros(1, dtype=torch.int32, device='cuda')
    for step in range(NS):
        assert int(cur.item()) == step
        for spec in (dict(kind='ce', eps=0.1), dict(kind='focal', gamma=2.0)):
            want_l, want_d = run_kernel(z[step], None, spec, w, labels=lab, cursor=cur)
            direct = run_kernel(z[step], lab[step * N:(step + 1) * N], spec, w)           # the cursor form reads the plan's row
            assert torch.equal(direct[0], want_l) and torch.equal(direct[1], want_d)
            means = []
            for r in range(W):
                got_l, got_d = run_kernel(z[step, r * bs_r:(r + 1) * bs_r], None, spec, w, ranks=W, rank=r, labels=lab, cursor=cur)
                assert torch.equal(got_d, want_d[r * bs_r:(r + 1) * bs_r]), (step, r, spec)
                assert torch.equal(got_l, want_l[r * bs_r:(r + 1) * bs_r]), (step, r, spec)
                means.append(got_l.mean().item())                 # (float32 means, as the loss history takes them)
            one = want_l.mean().item()
            assert abs(np.mean(means) - one) <= 4 * np.finfo(np.float32).eps * max(abs(one), 1.0), (means, one)
        # the cursor advances on the device (an optimiser launch on one dummy parameter does it, as in a train step)
        p = torch.zeros(1, device='cuda')
        lib.rmsprop_step(p, torch.zeros(1, device='cuda'), torch.zeros(1, device='cuda'), 1e-3, 0.9, cursor_dev=cur)


# ---------------------------------------------------------------------------------------------- 2. the engine
NAME = 'tiny1'                                   # 8 bands + 1, 5 x 5 patches, K = 5
N_STEPS, BATCH, HH, WW = 10, 24, 23, 19
ENGINE_W = [0.05, 1.0, 7.0, 0.4, 20.0]
CRITERIA = {'ce': dict(kind='ce', label_smoothing=0.1, gamma=0.0, class_weights=ENGINE_W),
            'focal': dict(kind='focal', label_smoothing=0.0, gamma=2.0, class_weights=ENGINE_W)}


def _ref_spec(cr):
    return dict(kind=cr['kind'], weight=None if cr['class_weights'] is None else torch.tensor(cr['class_weights'], dtype=torch.float32),
                eps=cr['label_smoothing'], gamma=cr['gamma'])


def _problem(seed=41, n=N_STEPS, B=BATCH, half=False):
    from test_gpu_half import scene
    C, C2, P, S, K = SHAPES[NAME]
    A, Bm = scene(NAME, HH, WW, seed)
    g = torch.Generator().manual_seed(seed + 1)
    xy = torch.stack([torch.randint(0, HH, (n * B,), generator=g), torch.randint(0, WW, (n * B,), generator=g)], 1).int()
    t = torch.randint(0, K, (n * B,), generator=g)
    return A, Bm, xy, t


def _oracle_run(ref, A, Bm, xy, t, cr, opt, n=N_STEPS, B=BATCH, scaler=None):
    from test_gpu_half import cut
    C, C2, P, S, K = SHAPES[NAME]
    crit = loss_ref.module(**_ref_spec(cr))
    want = []
    for s in range(n):
        a, b = cut(A, Bm, xy[s * B:(s + 1) * B], P, S)
        opt.zero_grad()
        loss = crit(ref(a, b), t[s * B:(s + 1) * B])
        if scaler is not None:
            scaler.scale(loss).backward()
            scaler.step(opt); scaler.update()
        else:
            loss.backward()
            opt.step()
        want.append(loss.item())
    return np.asarray(want)


def _check_run(tag, eng, hip, ref, want):
    got = eng.mean_losses().numpy()
    err = np.abs(got - want).max()
    sd = ref.state_dict()
    perr = max((v.detach().cpu().double() - sd[k].double()).abs().max().item() for k, v in hip.state_dict().items() if k in sd)
    print('%s: step losses max abs diff %.2e (first %.4f last %.4f), parameters max abs diff %.2e' % (tag, err, want[0], want[-1], perr))
    assert err < 1e-5, (got, want)
    for k, v in hip.state_dict().items():
        assert_close(v, sd[k], 2e-5, 1e-4, '%s: param %s after %d steps' % (tag, k, len(want)))
    return got


@pytest.mark.parametrize('which', ['ce', 'focal'])
def test_engine_adam_eager_and_graph_against_oracle(which):
    from dmf.engine import Scene, TrainEngine
    cr = CRITERIA[which]
    A, Bm, xy, t = _problem()
    runs = {}
    for graph in (0, 4):                               # 4: two replays, the remaining two steps run eagerly
        cfg, ref, hip = nets(NAME)
        want = _oracle_run(ref, A, Bm, xy, t, cr, torch.optim.Adam(ref.parameters(), lr=1e-3))
        eng = TrainEngine(hip, Scene(A.numpy(), Bm.numpy(), 'cuda:0'), BATCH, lr=1e-3, criterion=cr)
        assert not eng._native_loop_ok()
        eng.load_plan(xy, t)
        eng.run_plan(N_STEPS, steps_per_graph=graph)
        assert (eng.graph is not None) == bool(graph) and eng.step_count == N_STEPS
        runs[graph] = (_check_run('%s, ADAM, graph %d' % (which, graph), eng, hip, ref, want), eng.theta.cpu())
    assert np.array_equal(runs[0][0], runs[4][0]) and torch.equal(runs[0][1], runs[4][1])


def test_engine_short_last_batch_and_refusals(monkeypatch):
    """step() on a short batch divides by that batch's weight sum; the refusals of the criterion mode."""
    from dmf import lib
    from dmf.engine import Scene, TrainEngine
    from test_gpu_half import cut
    from test_gpu_parity import _attn_nets
    C, C2, P, S, K = SHAPES[NAME]
    cr = CRITERIA['ce']
    A, Bm, xy, t = _problem(n=1)
    cfg, ref, hip = nets(NAME)
    scene = Scene(A.numpy(), Bm.numpy(), 'cuda:0')
    eng = TrainEngine(hip, scene, BATCH, lr=1e-3, criterion=cr)
    n = 13
    a, b = cut(A, Bm, xy[:n], P, S)
    want = loss_ref.module(**_ref_spec(cr))(ref(a, b), t[:n]).item()
    eng.step(xy[:n].cuda(), t[:n].int().cuda())
    got = eng.loss[:n].mean().item()
    print('short batch of %d: loss %.6f, oracle %.6f' % (n, got, want))
    assert abs(got - want) < 1e-5
    for bad, msg in ((dict(cr, class_weights=[1.0, 0.0, 1.0, 1.0, 1.0]), '> 0'), (dict(cr, class_weights=[1.0, float('nan'), 1.0, 1.0, 1.0]), '> 0'),
                     (dict(cr, class_weights=[1.0, -2.0, 1.0, 1.0, 1.0]), '> 0'), (dict(cr, class_weights=[1.0] * 4), '5 classes'),
                     (dict(cr, label_smoothing=1.0), 'label_smoothing'), (dict(cr, kind='focal', label_smoothing=0.0, gamma=0.5), 'gamma')):
        with pytest.raises(lib.DmfError, match=msg):
            TrainEngine(hip, scene, BATCH, criterion=bad)
    monkeypatch.setattr(lib, 'unit_supported', lambda shape: False)      # (every compiled shape has the unit kernel today)
    with pytest.raises(lib.DmfError, match='dmf_unit_supported'):
        TrainEngine(hip, scene, BATCH, criterion=cr)
    monkeypatch.undo()
    acfg, aref, ahip = _attn_nets(NAME)
    with pytest.raises(lib.DmfError, match='attention'):
        TrainEngine(ahip, scene, BATCH, criterion=cr)


def test_criterion_none_is_todays_engine():
    from dmf.engine import Scene, TrainEngine
    A, Bm, xy, t = _problem(n=6)
    out = []
    for kw in ({}, {'criterion': None}):
        cfg, ref, hip = nets(NAME)
        eng = TrainEngine(hip, Scene(A.numpy(), Bm.numpy(), 'cuda:0'), BATCH, lr=1e-3, **kw)
        eng.load_plan(xy, t)
        eng.run_plan(3, steps_per_graph=3)
        eng.run_plan(3, steps_per_graph=0)
        out.append((eng.theta.cpu(), eng.mean_losses(), eng.m.cpu(), eng.v.cpu()))
    for x, y in zip(*out):
        assert torch.equal(x, y)


def test_engine_sgd_against_oracle():
    from dmf.engine import Scene, TrainEngine
    cr = CRITERIA['ce']
    A, Bm, xy, t = _problem(seed=43)
    cfg, ref, hip = nets(NAME)
    want = _oracle_run(ref, A, Bm, xy, t, cr, torch.optim.SGD(ref.parameters(), lr=0.05, momentum=0.9))
    eng = TrainEngine(hip, Scene(A.numpy(), Bm.numpy(), 'cuda:0'), BATCH, lr=0.05, optimizer='SGD', momentum=0.9, criterion=cr)
    eng.load_plan(xy, t)
    eng.run_plan(N_STEPS, steps_per_graph=4)
    _check_run('ce, SGD, graph 4', eng, hip, ref, want)


def test_engine_half_scene_and_loss_scaler_against_oracle():
    """`gmf.half: 1` + LossScaler: the oracle runs with the same roundings (fp16 primary scene and first conv weights) under
    torch.amp.GradScaler, as tests/test_gpu_half.py does for the default criterion."""
    from dmf.engine import LossScaler, Scene, TrainEngine
    from test_gpu_half import half_nets
    cr = CRITERIA['ce']
    A, Bm, xy, t = _problem(seed=45)
    cfg, ref, hip = half_nets(NAME)
    gs = torch.amp.GradScaler('cpu', init_scale=2.0 ** 12, growth_factor=2.0, backoff_factor=0.5, growth_interval=3)
    want = _oracle_run(ref, A, Bm, xy, t, cr, torch.optim.Adam(ref.parameters(), lr=1e-3), scaler=gs)
    sc = LossScaler('cuda:0', init_scale=2.0 ** 12, growth_factor=2.0, backoff_factor=0.5, growth_interval=3)
    eng = TrainEngine(hip, Scene(A.numpy(), Bm.numpy(), 'cuda:0', half=True), BATCH, lr=1e-3, scaler=sc, criterion=cr)
    eng.load_plan(xy, t)
    eng.run_plan(N_STEPS, steps_per_graph=4)
    assert sc.get_scale() == gs.get_scale() and sc.skipped_steps() == 0 and int(eng.dev_step.item()) == N_STEPS
    _check_run('ce, half scene + scaler, graph 4', eng, hip, ref, want)


# ---------------------------------------------------------------------------------------------- 3. two gloo ranks on the one GPU
DP_STEPS = 6
DP_CRITERION = dict(kind='ce', label_smoothing=0.0, gamma=0.0, class_weights=ENGINE_W)


def _dp_run(rank, world, pg):
    from dmf.engine import Scene, TrainEngine
    A, Bm, xy, t = _problem(seed=47, n=DP_STEPS)
    cfg, ref, hip = nets(NAME)
    eng = TrainEngine(hip, Scene(A.numpy(), Bm.numpy(), 'cuda:0'), BATCH // world, lr=1e-3, process_group=pg, criterion=DP_CRITERION)
    if world > 1:                                      # materialised patches are not sharded: refused with a criterion
        from dmf import lib
        C, C2, P, S, K = SHAPES[NAME]
        with pytest.raises(lib.DmfError, match='one rank only'):
            eng.step_patches(torch.zeros(2, C, P, P, device='cuda'), torch.zeros(2, C2, S * P, S * P, device='cuda'),
                             torch.zeros(2, dtype=torch.int32, device='cuda'))
    eng.load_plan(xy, t)                               # the GLOBAL batches on every rank
    eng.run_plan(DP_STEPS)
    return eng.theta.cpu().numpy(), eng.mean_losses().numpy()


def _dp_rank(rank, world, port, q):
    from test_gpu_stage2_dp import _init_group
    sys.path[:0] = [PKG, REPO]
    pg = _init_group(rank, world, port)
    q.put((rank, _dp_run(rank, world, pg)))
    import torch.distributed as dist
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_equal_one_rank_on_the_global_batches():
    from test_gpu_stage2_dp import _run_ranks
    two = _run_ranks(_dp_rank, 2, ())
    th1, l1 = _dp_run(0, 1, None)
    assert np.array_equal(two[0][0], two[1][0])
    err = np.abs(two[0][0] - th1).max()
    lerr = np.abs((two[0][1] + two[1][1]) / 2 - l1).max()      # the rank means average to the global batch loss
    print('weighted CE, 2 gloo ranks vs one rank: parameters max abs diff %.2e, mean of the rank losses vs global %.2e' % (err, lerr))
    assert err < 2e-5 and lerr < 1e-5


# ---------------------------------------------------------------------------------------------- 4. the solver
@pytest.mark.parametrize('keys', [dict(class_weights='balanced', label_smoothing=0.05), dict(class_weights='balanced', focal_gamma=2)])
def test_solver_fast_path_equals_drop_in(golden_dir, keys):
    from solver.mainsolver import Solver
    from test_gpu_trajectory import _setup
    runs = {}
    for fast in (1, 0):
        tmp = tempfile.mkdtemp(prefix='dmf_crit_solver_')
        try:
            g, cfg = _setup(golden_dir, tmp, fast_path=fast, epoch=4)
            cfg['schedule'] = dict(cfg['schedule'], **keys)
            cfg['test']['full'] = 1
            torch.manual_seed(3407)
            s = Solver(cfg)
            s.run()
            assert s.criterion is not None and s.criterion['kind'] == ('focal' if 'focal_gamma' in keys else 'ce')
            if fast:
                assert s.engine.criterion is not None and s.eval_engine.criterion is not None
            runs[fast] = (np.array(s.step_losses), s.test_matrix.copy(), list(s.criterion['class_weights']))
        finally:
            shutil.rmtree(tmp)
    lf, ld = runs[1][0], runs[0][0]
    assert lf.shape == ld.shape and len(lf) == 16 and runs[1][2] == runs[0][2]
    print('%s: fast vs drop-in step losses max abs diff %.2e over %d steps (first %.4f last %.4f)'
          % (keys, np.abs(lf - ld).max(), len(lf), lf[0], lf[-1]))
    assert np.abs(lf - ld).max() < 1e-5
    assert np.array_equal(runs[1][1], runs[0][1])
