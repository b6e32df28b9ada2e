"""GPU: stage 2 of the two-stage path (solver/tostagesolver.py:240-414) — the batch-level HIP kernels, the single-input
net and `toStageSolver(cfg).run()` against the fixtures the REAL reference produced (G8: qua_loss value + gradient,
train/loss_function.py; G10: toStageSolver.train/test trajectory around the CPU oracle net).

Tolerances: qua_loss value 1e-6, its gradient 1e-7 absolute (values are ~1e-2); logits 1e-5; every step loss of the
trajectory within 1e-5; best-epoch weights: 99 % within 3e-4, all within 3e-3 (see the test); identical confusion matrix; kappa within 0.001.
"""
import json
import os
import shutil
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_qua_loss_kernel_against_reference_golden(golden_dir):
    from dmf import lib
    g = np.load(os.path.join(golden_dir, 'g8_qua_loss.npz'), allow_pickle=False)
    prm = lib.qua_params(json.loads(str(g['cfg'])))
    logits = torch.from_numpy(g['logits']).cuda()
    labels = torch.from_numpy(g['target']).to(torch.int32).cuda()
    loss = torch.zeros(1, device='cuda')
    dl = torch.empty_like(logits)
    lib.qua_loss(logits, 10, labels, prm, loss=loss, dlogits=dl)
    assert abs(loss.item() - float(g['loss'])) < 1e-6
    err = (dl.cpu().numpy() - g['grad'])
    print('G8: loss diff %.2e, grad max abs diff %.2e' % (abs(loss.item() - float(g['loss'])), np.abs(err).max()))
    assert np.abs(err).max() < 1e-7
    # the module with the reference's call signature (train/loss_function.py:57) rides the same kernel
    from train.loss_function import qua_loss
    x = logits.clone().requires_grad_(True)
    v = qua_loss()(x, 10, torch.from_numpy(g['target']).cuda(), {'dqtl': json.loads(str(g['cfg']))})
    (2.0 * v).backward()
    assert abs(v.item() - float(g['loss'])) < 1e-6 and np.abs(x.grad.cpu().numpy() - 2.0 * g['grad']).max() < 2e-7


@pytest.mark.parametrize('bs,K', [(1, 5), (13, 5), (256, 17), (1100, 17)])
@pytest.mark.parametrize('coef', [(0.1, 0.05, 1.0), (0.0, 0.05, 1.0), (0.1, 0.0, 1.0), (0.3, 0.2, 0.5)])
def test_qua_loss_kernel_against_oracle(bs, K, coef):
    from dmf import lib
    from oracle import datapath_ref as dref
    alpha, beta, gamma = coef
    g = torch.Generator().manual_seed(bs * 31 + K)
    x = 2.0 * torch.randn(4 * bs, K, generator=g)
    t = torch.randint(0, K, (bs,), generator=g)
    xr = x.clone().requires_grad_(True)
    want = dref.qua_loss(xr, bs, t.float(), alpha, beta, gamma, 1e-8, 0.1)
    want.backward()
    prm = lib.QuaParams(alpha=alpha, beta=beta, gamma=gamma, epsilon=1e-8, tao=0.1)
    loss = torch.zeros(1, device='cuda')
    dl = torch.empty(4 * bs, K, device='cuda')
    lib.qua_loss(x.cuda(), bs, t.int().cuda(), prm, loss=loss, dlogits=dl, grad_scale=1.0)
    assert abs(loss.item() - want.item()) < 2e-6 * max(1.0, abs(want.item()))
    err = (dl.cpu() - xr.grad).abs().max().item()
    assert err < 1e-7 + 1e-4 * xr.grad.abs().max().item(), err
    # loss-only form (the validation loop)
    loss2 = torch.zeros(1, device='cuda')
    lib.qua_loss(x.cuda(), bs, t.int().cuda(), prm, loss=loss2)
    assert loss2.item() == loss.item()


def test_pair_argmax_and_band_mean():
    from dmf import lib
    from oracle.gmfnet_ref import band_mean
    g = torch.Generator().manual_seed(4)
    out = torch.randn(4 * 300, 17, generator=g)
    out[5] = 0.0; out[305] = 0.0                                         # an all-ties row: first index wins
    pred = torch.empty(300, dtype=torch.int32, device='cuda')
    lib.pair_argmax(out.cuda(), 300, pred)
    want = (out[:300] + out[300:600]).softmax(dim=-1).max(1)[1]
    assert torch.equal(pred.cpu().long(), want) and pred[5].item() == 0
    a = torch.rand(37, 4, 16, 16, generator=g)
    assert torch.equal(lib.band_mean_patches(a.cuda()).cpu(), band_mean(a))
    scene = torch.rand(21, 19, 4, generator=g)
    assert torch.equal(lib.band_mean_scene(scene.cuda()).cpu()[:, :, 0], band_mean(scene.permute(2, 0, 1)[None])[0, 0])


@pytest.mark.parametrize('P', [5, 16])
def test_single_input_net_forward_and_grads(P):
    """`net(data)` (tostagesolver.py:274) through the HIP path against the oracle, values and parameter gradients."""
    from oracle.gmfnet_ref import Net as RefNet
    from oracle import datapath_ref as dref
    from model.gmfnet import Net as HipNet
    from train.loss_function import qua_loss
    dq = {'alpha': 0.1, 'beta': 0.05, 'gamma': 1.0, 'epsilon': 1e-8, 'tao': 0.1}
    cfg = {'patch_size': P, 'Categories_Number': 6, 'data_city': 's', 'DATA_DICT': {'s': {'size': [32, 32, 4]}},
           'gmf': {'width': 40, 'single_input': 1}, 'dqtl': dq, 'device': 'cuda:0'}
    torch.manual_seed(0)
    ref = RefNet(cfg)
    with torch.no_grad():
        for p in ref.parameters():
            p.add_(0.05 * torch.randn_like(p))
    hip = HipNet(cfg)
    hip.load_state_dict(ref.state_dict())
    hip = hip.to('cuda:0')
    bs = 21
    g = torch.Generator().manual_seed(3)
    data = torch.rand(4 * bs, 4, P, P, generator=g)
    t = torch.randint(1, 6, (bs,), generator=g).float()
    out_r = ref(data)
    loss_r = dref.qua_loss(out_r, bs, t, dq['alpha'], dq['beta'], dq['gamma'], dq['epsilon'], dq['tao'])
    loss_r.backward()
    out_h = hip(data.cuda())
    loss_h = qua_loss()(out_h, bs, t.cuda(), cfg)
    loss_h.backward()
    assert (out_h.detach().cpu() - out_r.detach()).abs().max().item() < 1e-5
    assert abs(loss_h.item() - loss_r.item()) < 1e-6
    for (k, pr), (_, ph) in zip(ref.named_parameters(), hip.named_parameters()):
        err = (ph.grad.cpu() - pr.grad).abs().max().item()
        assert err < 1e-6 + 1e-4 * pr.grad.abs().max().item(), (k, err)
    with pytest.raises(TypeError):
        HipNet({**cfg, 'gmf': {'width': 40}}).to('cuda:0')(data.cuda())


def _setup(golden_dir, tmp, **over):
    g = np.load(os.path.join(golden_dir, 'g10_stage2.npz'), allow_pickle=False)
    d = os.path.join(tmp, 'scene') + '/'
    w = os.path.join(tmp, 'stage1') + '/'
    os.makedirs(d); os.makedirs(w)
    np.save(d + 'ms4.tif.npy', g['primary']); np.save(d + 'pan.tif.npy', g['aux']); np.save(d + 'label.npy', g['label'])
    np.save(w + 'msgan.npy', g['ms_gan']); np.save(w + 'pangan.npy', g['pan_gan'])     # stage-1 outputs (pre_trained)
    cfg = json.loads(str(g['cfg']))
    cfg.update(data_address=d, expo_result=tmp + '/', RESULT_output=os.path.join(tmp, 'out') + '/',
               RESULT_excel=os.path.join(tmp, 'r.xlsx'), nohup=1, device='cuda:0')
    cfg['dqtl']['WEIGHTS'] = 'stage1/'
    cfg.update(over)
    os.makedirs(cfg['RESULT_output'])
    return g, cfg


@pytest.mark.parametrize('fast', [1, 0])
def test_tostagesolver_reproduces_reference_trajectory(golden_dir, fast):
    from solver.tostagesolver import toStageSolver
    tmp = tempfile.mkdtemp(prefix='dmf_stage2_')
    try:
        g, cfg = _setup(golden_dir, tmp, fast_path=fast)
        torch.manual_seed(3407)
        s = toStageSolver(cfg)
        s.run()                                         # pan.npy is absent: pan2ms runs on the GPU (IHS.py:14-19)
        want = g['losses'][g['is_train_call']]
        got = np.array(s.step_losses)
        assert got.shape == want.shape, (got.shape, want.shape)
        diff = np.abs(got - want)
        print('fast=%d  stage-2 loss diff: first20 %.2e  all %.2e' % (fast, diff[:20].max(), diff.max()))
        assert diff.max() < 1e-5
        out = cfg['RESULT_output']
        best = torch.load(out + '0_weights.pth', map_location='cpu', weights_only=True)
        # ADAM divides by sqrt(v): on a channel whose ReLU is almost always off the gradient is rounding noise and the
        # update still has size ~lr, so such a channel drifts (here: channel 26 of branch A, 31 of branch B, up to
        # 1.5e-3 after 200 steps at lr 3e-3) while the loss and every prediction stay put.  Bound the bulk and the tail.
        d_all = np.concatenate([np.abs(v.numpy() - g['best.' + k]).reshape(-1) for k, v in best.items()])
        print('best-epoch weights: max abs diff %.2e, 99th percentile %.2e' % (d_all.max(), np.percentile(d_all, 99)))
        assert d_all.max() < 3e-3 and np.percentile(d_all, 99) < 3e-4
        m = np.load(out + '0_matrix.npy')
        flips = int(np.abs(m - g['test_matrix']).sum() // 2)
        print('kappa ref %.6f got %.6f  differing predictions %d / %d' % (float(g['kappa']), s.result[2], flips, int(m.sum())))
        assert m.sum() == g['test_matrix'].sum() and flips == 0 and abs(s.result[2] - float(g['kappa'])) < 1e-3
    finally:
        shutil.rmtree(tmp)


def test_tostagesolver_test_and_colour_agree_between_the_paths(golden_dir):
    """Stage 2 with `color.index: 1` on both paths: the drop-in `test()` / `color()` (`net(concat(ms, pan))` + pair_argmax over
    the materialising `test_loader` / `color_loader*`) against the fast path's (QuaEvalEngine.confusion / label_map over the
    index-only twins).  The two runs train to weights that differ by rounding only (losses within 1e-5, above); on this scene no
    prediction flips, so the test matrices and both label maps are identical: 0 differing pixels of 400 on each map."""
    from solver.tostagesolver import toStageSolver
    runs = {}
    for fast in (1, 0):
        tmp = tempfile.mkdtemp(prefix='dmf_stage2_color_')
        try:
            g, cfg = _setup(golden_dir, tmp, fast_path=fast)
            cfg['color'] = dict(cfg['color'], index=1, supervised=1, unsupervised=1)
            torch.manual_seed(3407)
            s = toStageSolver(cfg)
            s.run()
            assert os.path.exists(cfg['RESULT_output'] + '0_pic_1.png') and os.path.exists(cfg['RESULT_output'] + '0_pic_2.png')
            runs[fast] = (s.test_matrix.copy(), np.asarray(s.label_maps[0]), np.asarray(s.label_maps[1]))
        finally:
            shutil.rmtree(tmp)
    lab = g['label']
    m1, m2 = runs[1][1], runs[1][2]
    assert m1.shape == lab.shape and (m1[lab == 0] == 0).all() and (m1[lab != 0] != 0).all() and (m2[lab != 0] == m1[lab != 0]).all()
    print('stage 2 fast vs drop-in: differing pixels %d / %d (supervised map), %d / %d (both maps laid over), differing test predictions %d / %d'
          % ((runs[1][1] != runs[0][1]).sum(), m1.size, (runs[1][2] != runs[0][2]).sum(), m2.size,
             np.abs(runs[1][0] - runs[0][0]).sum() // 2, runs[1][0].sum()))
    assert runs[1][0].sum() > 0 and np.array_equal(runs[1][0], runs[0][0])
    assert np.array_equal(runs[1][1], runs[0][1]) and np.array_equal(runs[1][2], runs[0][2])


def test_stage1_is_refused_loudly(golden_dir):
    from solver.tostagesolver import toStageSolver
    tmp = tempfile.mkdtemp(prefix='dmf_stage1_')
    try:
        g, cfg = _setup(golden_dir, tmp)
        cfg['dqtl']['pre_trained'] = 0
        with pytest.raises(NotImplementedError):
            toStageSolver(cfg).run()
    finally:
        shutil.rmtree(tmp)
