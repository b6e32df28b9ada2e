"""GPU: data-parallel stage 2 and `gmf.half` on the solvers' fast path.

* `dmf_qua_loss_ranks` (the stage-2 loss on the logits as all_gather_into_tensor leaves them, rank-major [W][4][bs_r][K])
  against `dmf_qua_loss` on the same global batch restacked stream-major [4][W*bs_r][K]: bit-identical loss and rows, in
  all three launch forms, scaled and through a device cursor into a plan; and against the oracle's autograd.
* QuaTrainEngine with a loss scaler and a process group (2 gloo ranks on the one GPU of the box) against one rank on the
  global batches, with a pixel that only rank 1 reads poisoned so that some steps are skipped.
* The RCCL form of the stage-2 step on a ONE-rank NCCL group (`_force_collective`), eager and replayed from a hipGraph.
* Solver / toStageSolver with gmf.half: 1 against their own drop-in runs, and toStageSolver on 2 gloo ranks against 1.
Several ranks run as spawned processes that share the GPU and talk over gloo (RCCL refuses two ranks on one device).
"""
import json
import os
import shutil
import sys
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, 'dual-modal-fusion_amd')
GOLDEN = os.path.join(REPO, 'tests', 'golden')
DQTL = {'alpha': 0.1, 'beta': 0.05, 'gamma': 1.0, 'epsilon': 1e-8, 'tao': 0.1}


def _run_ranks(target, world, extra, timeout=240):
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 29100 + (os.getpid() + 11 * world) % 400
    procs = [ctx.Process(target=target, args=(r, world, port, q) + extra) for r in range(world)]
    [p.start() for p in procs]
    try:
        out = [q.get(timeout=timeout) for _ in range(world)]
    finally:
        [p.join(60) for p in procs]
        for p in procs:
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    return dict(out)                    # rank -> result


def _init_group(rank, world, port, backend='gloo'):
    import datetime
    import torch.distributed as dist
    sys.path[:0] = [PKG, REPO]
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    kw = {'device_id': torch.device('cuda', 0)} if backend == 'nccl' else {}
    torch.cuda.set_device(0)
    dist.init_process_group(backend, rank=rank, world_size=world, timeout=datetime.timedelta(seconds=90), **kw)
    return dist.group.WORLD


# ---------------------------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize('bs_r,K', [(1, 5), (24, 12), (256, 17), (600, 12)])
@pytest.mark.parametrize('W', [1, 2, 3, 8])
def test_gathered_loss_equals_the_restacked_batch(W, bs_r, K):
    """(600, 12) with 8 ranks is a global batch of 4,800 > 16 * QE_MAXG: the one-workgroup tiled form; (256, 17) the
    run-time-K tiled form; the others the element-parallel form."""
    from dmf import lib
    from oracle import datapath_ref as dref
    bs, NS = W * bs_r, 3
    g = torch.Generator().manual_seed(1000 * W + bs_r + K)
    x = 2.0 * torch.randn(NS, W, 4, bs_r, K, generator=g)          # per step: the gathered [W][4][bs_r][K]
    lab = torch.randint(0, K, (NS * bs,), generator=g)
    prm = lib.qua_params(DQTL)
    labd = lab.int().cuda()
    state = torch.zeros(lib.SCALER_FLOATS, device='cuda')
    lib.scaler_init(state, 1024.0)
    for step in range(NS):
        cur = torch.full((1,), step, dtype=torch.int32, device='cuda')
        gathered = x[step].reshape(W * 4 * bs_r, K).cuda()
        restacked = x[step].permute(1, 0, 2, 3).reshape(4 * bs, K).contiguous()
        for sc in (None, state):
            want_l, want_h = torch.zeros(1, device='cuda'), torch.zeros(NS, device='cuda')
            want_d = torch.empty(4 * bs, K, device='cuda')
            lib.qua_loss(restacked.cuda(), bs, labd, prm, loss=want_l, dlogits=want_d, cursor=cur, loss_hist=want_h,
                         scaler_state=sc)
            want_d = want_d.view(4, W, bs_r, K)
            for r in range(W):
                got_l, got_h = torch.zeros(1, device='cuda'), torch.zeros(NS, device='cuda')
                got_d = torch.full((4 * bs_r, K), float('nan'), device='cuda')
                lib.qua_loss_ranks(gathered, W, r, bs_r, labd, prm, loss=got_l, dlogits=got_d, cursor=cur, loss_hist=got_h,
                                   scaler_state=sc)
                assert torch.equal(got_l, want_l) and torch.equal(got_h, want_h), (step, r)
                assert torch.equal(got_d.view(4, bs_r, K), want_d[:, r]), (step, r, sc is not None)
            if sc is None:
                unscaled = want_d.clone()
            else:                                                  # dlogits x scale (a power of two: exact)
                assert torch.equal(want_d, unscaled * 1024.0)
        # the oracle's autograd on the global batch
        xr = restacked.clone().requires_grad_(True)
        ref = dref.qua_loss(xr, bs, lab[step * bs:(step + 1) * bs].float(), DQTL['alpha'], DQTL['beta'], DQTL['gamma'],
                            DQTL['epsilon'], DQTL['tao'])
        ref.backward()
        assert abs(want_l.item() - ref.item()) < 2e-6 * max(1.0, abs(ref.item()))
        err = (unscaled.reshape(4 * bs, K).cpu() - xr.grad).abs().max().item()
        assert err < 1e-7 + 1e-4 * xr.grad.abs().max().item(), err
    with pytest.raises(lib.DmfError):
        lib.qua_loss_ranks(gathered, W, W, bs_r, labd, prm)
    with pytest.raises(lib.DmfError):
        lib.qua_loss_ranks(gathered, W, 0, bs_r, labd, prm, dlogits=torch.empty(4 * bs, K + 1, device='cuda'))


# ---------------------------------------------------------------------------------------------- 2-3. the engine
P16 = {'patch_size': 16, 'Categories_Number': 5, 'data_city': 's', 'DATA_DICT': {'s': {'size': [20, 20, 4]}},
       'gmf': {'width': 40, 'single_input': 1, 'half': 1}}
GB, NS = 24, 6


def _stage2_problem(poison):
    """Four padded fp32 scenes and a plan of NS global batches of GB pixels.  poison: pixel (19, 19), the only patch that
    reads the bottom-right corner of stream 0, sits at global row 13 (rank 1's shard of two ranks) of steps 1 and 4, and
    that corner holds 70000 (inf in the fp16 scene)."""
    from dmf import synth
    from function.function import data_padding
    ms, _, label = synth.make_scene(20, 20, 4, 1, 1, n_classes=4, seed=5)
    g = np.random.default_rng(2)
    scenes = [data_padding(x, P16, 'ms').astype(np.float32)
              for x in (ms, ms[::-1].copy(), ms + 0.1 * g.standard_normal(ms.shape), ms * 0.5)]
    assert scenes[0].shape[0] == 20 + 16 - 1
    xy = np.stack([g.integers(0, 19, GB * NS), g.integers(0, 19, GB * NS)], 1).astype(np.int32)
    if poison:
        scenes[0][-1, -1, 0] = 70000.0
        for s in (1, 4):
            xy[s * GB + 13] = (19, 19)
    lab = np.maximum(label[xy[:, 0], xy[:, 1]], 1).astype(np.int32)
    return scenes, xy, lab


def _scaled_stage2(rank, world, port, q):
    sys.path[:0] = [PKG, REPO]
    pg = _init_group(rank, world, port) if world > 1 else None
    from dmf.engine import LossScaler, QuaScene, QuaTrainEngine
    from model.gmfnet import Net
    scenes, xy, lab = _stage2_problem(poison=True)
    torch.manual_seed(0)
    net = Net(P16).to('cuda:0')
    sc = LossScaler('cuda:0', init_scale=2.0 ** 10, growth_interval=2)
    eng = QuaTrainEngine(net, QuaScene(scenes, 'cuda:0', half=True), GB // world, DQTL, lr=1e-3, process_group=pg, scaler=sc)
    eng.load_plan(xy, lab)
    scales, skipped = [], []
    for _ in range(NS):
        eng.run_plan(1)
        scales.append(sc.get_scale())
        skipped.append(sc.skipped_steps())
    q.put((rank, (eng.theta.cpu().numpy(), eng.losses().numpy(), scales, skipped, int(eng.dev_step.item()))))
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


def test_loss_scaler_with_a_process_group_equals_one_rank():
    two = _run_ranks(_scaled_stage2, 2, ())
    one = _run_ranks(_scaled_stage2, 1, ())[0]
    th1, l1, s1, k1, d1 = one
    assert k1[-1] == 2 and k1[1] == 1 and k1[4] == 2, k1          # the two poisoned steps are skipped
    for r in (0, 1):
        th, l, s, k, d = two[r]
        assert k == k1 and s == s1 and d == d1, (r, k, k1, s, s1)
        ok = np.isfinite(l1)
        assert np.array_equal(np.isfinite(l), ok) and np.abs(l[ok] - l1[ok]).max() < 1e-5
        err = np.abs(th - th1).max()
        print('stage 2, scaler: rank %d vs one rank: parameters max abs diff %.2e' % (r, err))
        assert err < 2e-5
    assert np.array_equal(two[0][0], two[1][0]) and np.array_equal(two[0][1], two[1][1], equal_nan=True)


def _rccl_stage2(rank, world, port, q, scaled):
    sys.path[:0] = [PKG, REPO]
    pg = _init_group(0, 1, port, 'nccl')
    from dmf.engine import LossScaler, QuaScene, QuaTrainEngine
    from model.gmfnet import Net
    scenes, xy, lab = _stage2_problem(poison=False)
    out = {}
    for mode in ('single', 'eager', 'graph'):
        torch.manual_seed(0)
        net = Net(P16).to('cuda:0')
        sc = LossScaler('cuda:0', init_scale=2.0 ** 10, growth_interval=2) if scaled else None
        eng = QuaTrainEngine(net, QuaScene(scenes, 'cuda:0', half=True), GB, DQTL, lr=1e-3,
                             process_group=None if mode == 'single' else pg, scaler=sc)
        eng._force_collective = mode != 'single'   # all-gather -> qua_loss_ranks -> ... -> RCCL all-reduce, as with N ranks
        eng.load_plan(xy, lab)
        eng.run_plan(NS, 3 if mode == 'graph' else 0)
        torch.cuda.synchronize()
        out[mode] = (eng.theta.cpu().numpy(), eng.losses().numpy(), sc.get_scale() if scaled else None,
                     int(eng.dev_step.item()), eng.graph is not None, eng._graphable())
    q.put((0, out))
    import torch.distributed as dist
    dist.destroy_process_group()


@pytest.mark.parametrize('scaled', [0, 1])
def test_rccl_form_of_the_stage2_step_on_a_one_rank_group(scaled):
    """The data-parallel stage-2 step — all_gather_into_tensor, dmf_qua_loss_ranks, backward, dmf_grad_reduce, RCCL
    all-reduce, the optimiser step on the device step count — on a ONE-rank NCCL group, eagerly and replayed from a
    captured hipGraph (steps_per_graph 3), against the single-GPU unit step.  One rank is all a one-GPU box can give RCCL."""
    out = _run_ranks(_rccl_stage2, 1, (scaled,))[0]
    single, eager, graph = out['single'], out['eager'], out['graph']
    assert graph[4] and graph[5], 'the stage-2 step with its collectives was not captured in a hipGraph'
    assert np.array_equal(graph[0], eager[0]) and np.array_equal(graph[1], eager[1])
    assert graph[2] == eager[2] and graph[3] == eager[3] == NS
    print('RCCL form vs single-GPU stage-2 step: parameters %.2e, losses %.2e'
          % (np.abs(eager[0] - single[0]).max(), np.abs(eager[1] - single[1]).max()))
    assert np.abs(eager[0] - single[0]).max() < 2e-6 and np.abs(eager[1] - single[1]).max() < 1e-6
    assert eager[2] == single[2] and eager[3] == single[3]


# ---------------------------------------------------------------------------------------------- 4-5. the solvers
def _g9_cfg(tmp, **over):
    """G9's scene with its aux modality 4 x 4 mean-pooled to the primary's resolution (scale 1: the late-fusion row that
    has fp16-scene kernels)."""
    g = np.load(os.path.join(GOLDEN, 'g9_trajectory.npz'), allow_pickle=False)
    d = os.path.join(tmp, 'scene') + '/'
    os.makedirs(d, exist_ok=True)
    H, W = g['primary'].shape[:2]
    aux = g['aux'].reshape(H, 4, W, 4).mean(axis=(1, 3)).astype(g['aux'].dtype)
    np.save(d + 'ms4.tif.npy', g['primary']); np.save(d + 'pan.tif.npy', aux); np.save(d + 'label.npy', g['label'])
    cfg = json.loads(str(g['cfg']))
    cfg['scale'] = 1
    out = os.path.join(tmp, 'out_%s' % over.get('fast_path', 1)) + '/'
    os.makedirs(out, exist_ok=True)
    cfg.update(data_address=d, RESULT_output=out, RESULT_excel=os.path.join(tmp, 'r.xlsx'), nohup=1, device='cuda:0', epoch=6)
    cfg['gmf']['half'] = 1
    cfg['test']['full'] = 1
    cfg.update(over)
    return cfg


def _g10_cfg(tmp, tag, write=True, **over):
    """G10's scene at patch 16 (the stage-2 row that has fp16-scene kernels); train_rate 0.405: 110 training pixels,
    4 x 24 + an even 14.  write: put the scene and the stage-1 outputs under tmp (one writer per directory)."""
    g = np.load(os.path.join(GOLDEN, 'g10_stage2.npz'), allow_pickle=False)
    d = os.path.join(tmp, 'scene') + '/'
    w = os.path.join(tmp, 'stage1') + '/'
    out = os.path.join(tmp, 'out_%s' % tag) + '/'
    if write:
        os.makedirs(d, exist_ok=True); os.makedirs(w, exist_ok=True); os.makedirs(out, exist_ok=True)
        np.save(d + 'ms4.tif.npy', g['primary']); np.save(d + 'pan.tif.npy', g['aux']); np.save(d + 'label.npy', g['label'])
        np.save(w + 'msgan.npy', g['ms_gan']); np.save(w + 'pangan.npy', g['pan_gan'])
    cfg = json.loads(str(g['cfg']))
    cfg.update(data_address=d, expo_result=tmp + '/', RESULT_output=out, RESULT_excel=os.path.join(tmp, 'r_%s.xlsx' % tag),
               nohup=1, device='cuda:0', epoch=8, patch_size=16, train_rate=0.405)
    cfg['dqtl']['WEIGHTS'] = 'stage1/'
    cfg['gmf']['half'] = 1
    cfg['color']['index'] = 1
    cfg.update(over)
    return cfg


def _run_solver(cls, cfg):
    torch.manual_seed(3407)
    s = cls(cfg)
    s.run()
    return s


@pytest.mark.parametrize('which', ['Solver', 'toStageSolver'])
def test_solvers_honour_gmf_half_on_the_fast_path(which):
    """gmf.half: 1 — the fast path trains the fp16 scene with the device loss scaler (GradScaler's defaults), the drop-in
    path rounds its patches to fp16: the two paths of one config agree."""
    from solver.mainsolver import Solver
    from solver.tostagesolver import toStageSolver
    tmp = tempfile.mkdtemp(prefix='dmf_half_')
    try:
        if which == 'Solver':
            fast = _run_solver(Solver, _g9_cfg(tmp, fast_path=1))
            drop = _run_solver(Solver, _g9_cfg(tmp, fast_path=0))
            scene = fast.engine.scene
        else:
            fast = _run_solver(toStageSolver, _g10_cfg(tmp, 'fast', fast_path=1))
            drop = _run_solver(toStageSolver, _g10_cfg(tmp, 'drop', fast_path=0))
            scene = fast.qua_scene
            assert fast.engine.scene is scene
        assert scene.A.dtype == torch.float16 and fast.engine.scaler is not None
        assert fast.engine.scaler.skipped_steps() == 0
        a, b = np.array(fast.step_losses), np.array(drop.step_losses)
        assert a.shape == b.shape and len(a) > 0
        print('%s gmf.half: fast vs drop-in step losses max abs diff %.2e over %d steps' % (which, np.abs(a - b).max(), len(a)))
        assert np.abs(a - b).max() < 1e-5
        assert np.array_equal(fast.test_matrix, drop.test_matrix)
    finally:
        shutil.rmtree(tmp)


def _tostage_dp(rank, world, port, q, tmp):
    sys.path[:0] = [PKG, REPO]
    pg = _init_group(rank, world, port) if world > 1 else None
    from solver.tostagesolver import toStageSolver
    d = os.path.join(tmp, 'w%d' % world)                  # one run directory for all ranks (rank 0 writes the artefacts)
    cfg = _g10_cfg(d, 'dp', write=rank == 0)
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
    torch.manual_seed(3407)
    s = toStageSolver(cfg)
    if world > 1:
        s.process_group, s.rank, s.world = pg, rank, world
    s.run()
    q.put((rank, (np.array(s.step_losses), s.test_matrix, s.label_maps[1], s.cur_model.flat_parameters().cpu().numpy())))
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


def test_tostagesolver_data_parallel_equals_single_rank():
    """`toStageSolver(cfg).run()` with gmf.half: 1 on 2 data-parallel ranks (gloo): every rank trains on its shard of
    each global batch, the loss is the gathered global batch's, test and colour are sharded.  Loss trajectory, confusion
    matrix and class map equal the 1-rank run."""
    tmp = tempfile.mkdtemp(prefix='dmf_s2dp_')
    try:
        two = _run_ranks(_tostage_dp, 2, (tmp,), timeout=400)
        one = _run_ranks(_tostage_dp, 1, (tmp,), timeout=400)[0]
        for r in (0, 1):
            l, m, lm, th = two[r]
            assert l.shape == one[0].shape
            print('toStageSolver rank %d vs 1 rank: losses %.2e, parameters %.2e' % (r, np.abs(l - one[0]).max(),
                                                                                    np.abs(th - one[3]).max()))
            assert np.abs(l - one[0]).max() < 1e-5
            assert np.array_equal(m, one[1]) and np.array_equal(lm, one[2])
    finally:
        shutil.rmtree(tmp)
