"""GPU: the attention entry points where the softmax is not flat, against the CPU oracle (oracle/gmfnet_ref.py).

Inputs come from tests/attn_cases.py: the usual attention recipe with the head blocks of attn_wq / attn_wk scaled by (2, 6, 12),
so one launch holds a nearly flat head and a sharp one (mean row maximum 0.02 .. 0.06 and 0.45 .. 0.78).  Its guards run on the
CPU (tests/test_attn_cases_host.py); two of them assert that a backward without the softmax backward, and one with two heads
exchanged, miss the tolerances used here by more than 10 x in at least 10 elements of every tensor named there.

Tolerances (attn_cases states them): logits 2e-4, per-patch loss 2e-4, gradients atol_k + 2e-3 |want| per tensor k with
atol_k = min(2e-5, 1e-3 max |want_k|).

Batches: a training launch has grid min(B, 256), so 257 and 513 make a workgroup walk a second and a third patch (slab_acc's add
path, fetch_tokens' prefetch); the forward launch has grid min(B, 512), so 513 is the first batch a forward workgroup walks
twice and 1025 the first it walks three times.  tiny1 has 25 real tokens of the kernel's 128 (103 keys masked), hsi 121.

Every comparison prints its worst error relative to the tensor's maximum; one run's numbers are kept in profiles/attn_sharp.md.
"""
import functools

import numpy as np
import pytest
import torch

import attn_cases as ac
import parity_cases as pc
from test_gpu_parity import SHAPES

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def hip_net(name, factors=ac.FACTORS_DEFAULT):
    from model.gmfnet import Net as HipNet
    cfg, ref = ac.sharp_net(name, factors)
    hip = HipNet(cfg)
    hip.load_state_dict(ref.state_dict())
    return hip.to('cuda:0')


def net_of(c):
    hip = hip_net(c['name'], c.get('factors', ac.FACTORS_DEFAULT))
    assert all(torch.equal(v, hip.state_dict()[k].cpu()) for k, v in c['state'].items())
    return hip


def within(got, want, tol, what):
    """|got - want| <= tol elementwise; prints the worst error and the reference's maximum."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    err = (got - want).abs()
    peak = want.abs().max().item()
    print('%-58s max err %.2e, %.2e of max |ref| %.2e' % (what, err.max().item(), err.max().item() / (peak + 1e-300), peak))
    bad = err > tol
    assert not bad.any(), '%s: %d/%d out of tolerance, max abs err %.3e (|ref| max %.3e) at %s' % (
        what, int(bad.sum()), bad.numel(), err.max().item(), peak, np.unravel_index(int(err.argmax()), tuple(err.shape)))


def check_pred(c, pred, logits, what):
    pred = pred.cpu().long()
    assert torch.equal(pred, logits.cpu().argmax(1)), 'pred != argmax of the GPU logits ' + what
    safe = c['safe']
    assert torch.equal(pred[safe], c['pred'][safe]), 'pred != oracle class on %d safe rows %s' % (int(safe.sum()), what)


def check_grads(hip, grad, want_g, what):
    """Every parameter tensor against its tolerance; all tensors are printed before the first failure is raised."""
    grad = grad.cpu()
    off = hip._offsets
    failures = []
    for i, (k, p) in enumerate(zip(hip._order(), hip._named())):
        want = want_g[k]
        got = grad[off[i]:off[i] + p.numel()].view(p.shape)
        if k in ('attn_wq', 'attn_wk'):
            peak = want.abs().max().item()
            heads = [(got[32 * h:32 * h + 32] - want[32 * h:32 * h + 32]).abs().max().item() / peak for h in range(3)]
            print('%-58s per head, of the tensor\'s max: %s' % ('grad %s %s' % (k, what), ' '.join('%.2e' % e for e in heads)))
        try:
            within(got, want, ac.grad_tol(want).double(), 'grad %s %s' % (k, what))
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, '\n'.join(failures)


def train_step(hip, inp, B, K, labels, dlogits, loss_scale, fill=None):
    """dmf_train_attn_fwd_bwd + dmf_grad_reduce into fresh buffers -> (logits, loss, flat gradient).  fill: the byte both
    workspaces hold before the launch."""
    from dmf import lib
    logits = torch.full((B, K), float('nan'), device='cuda')
    loss = torch.full((B,), float('nan'), device='cuda') if labels is not None else None
    ws = torch.empty(lib.workspace_bytes(hip.shape, B), dtype=torch.uint8, device='cuda')
    aws = torch.empty(lib.attn_train_workspace_bytes(hip.shape, B), dtype=torch.uint8, device='cuda')
    if fill is not None:
        ws.fill_(fill); aws.fill_(fill)
    ws = ws.view(torch.float32)
    theta = hip.flat_parameters()
    lib.train_attn_fwd_bwd(hip.shape, inp, theta, hip.pool_w, labels, dlogits, loss_scale, logits, loss, ws, aws)
    grad = torch.full_like(theta, float('nan'))
    lib.grad_reduce(hip.shape, B, ws, grad)
    torch.cuda.synchronize()
    return logits, loss, grad


# ------------------------------------------------------------------------------------------------------------- 1. forward
def forward_attn(hip, inp, B, K):
    from dmf import lib
    logits = torch.full((B, K), float('nan'), device='cuda'); pred = torch.full((B,), -1, dtype=torch.int32, device='cuda')
    ws = torch.empty(lib.attn_workspace_bytes(hip.shape, B), dtype=torch.uint8, device='cuda')
    lib.forward_attn(hip.shape, inp, hip.flat_parameters(), hip.pool_w, ws, logits, pred)
    torch.cuda.synchronize()
    return logits, pred


@pytest.mark.parametrize('name,B', ac.FORWARD)
def test_sharp_forward(name, B):
    """dmf_forward_attn on materialised patches, through net(a, b) and with the class output; SCENE_FORWARD also gathered from
    a resident scene.  Logits to 2e-4 against the bf16 oracle, the class wherever the oracle's top-2 margin exceeds
    parity_cases.MARGIN, and the fp32-attention oracle more than 5e-4 away (the attention path matters)."""
    from dmf import lib
    from dmf.engine import Scene
    c = ac.case(name, B)
    hip, K = net_of(c), c['K']
    assert c['fp32_gap'] > ac.FP32_GAP and 1.0 - c['safe'].float().mean().item() <= pc.MARGIN_CAP
    ad, bd = c['a'].cuda(), c['b'].cuda()
    with torch.no_grad():
        got = hip(ad, bd)
    within(got, c['logits'], ac.LOGIT_TOL, 'forward logits %s net(a, b)' % c['what'])
    logits, pred = forward_attn(hip, lib.input_patches(hip.shape, ad, bd), B, K)
    within(logits, c['logits'], ac.LOGIT_TOL, 'forward logits %s dmf_forward_attn' % c['what'])
    check_pred(c, pred, logits, c['what'])
    if (name, B) == ac.SCENE_FORWARD:
        s = ac.scene_case()
        assert s['fp32_gap'] > ac.FP32_GAP and 1.0 - s['safe'].float().mean().item() <= pc.MARGIN_CAP
        scene = Scene(s['A'].numpy(), s['Bm'].numpy(), 'cuda:0')
        lib.check_xy_bounds(hip.shape, scene.A, scene.B, s['xy'].numpy())
        xyd = s['xy'].cuda()
        logits, pred = forward_attn(hip, lib.input_gather(hip.shape, scene.A, scene.B, xyd), B, K)
        within(logits, s['logits'], ac.LOGIT_TOL, 'forward logits %s' % s['what'])
        check_pred(s, pred, logits, s['what'])


# --------------------------------------------------------------------------------------------------------------- 2. train
@pytest.mark.parametrize('name,B', ac.TRAIN)
def test_sharp_train_cross_entropy(name, B):
    """dmf_train_attn_fwd_bwd with labels and loss_scale = 1 / B, then dmf_grad_reduce: logits, per-patch loss and every
    parameter tensor's gradient against autograd through the oracle."""
    from dmf import lib
    c = ac.case(name, B)
    hip, K = net_of(c), c['K']
    ad, bd = c['a'].cuda(), c['b'].cuda()
    logits, loss, grad = train_step(hip, lib.input_patches(hip.shape, ad, bd), B, K, c['labels'].int().cuda(), None, 1.0 / B)
    within(logits, c['logits'], ac.LOGIT_TOL, 'train logits %s' % c['what'])
    within(loss, c['loss'], ac.LOSS_TOL, 'train per-patch loss %s' % c['what'])
    check_grads(hip, grad, c['grads'], c['what'])


# ------------------------------------------------------------------------------------------------------------- 3. dlogits
@pytest.mark.parametrize('name,B', ac.TRAIN)
def test_sharp_train_from_dlogits(name, B):
    """The route net(ms, pan) + a torch loss takes: labels = None and the caller's dL/dlogits = randn(B, K) / B, against the
    oracle's logits.backward(dl)."""
    from dmf import lib
    c = ac.case(name, B)
    hip, K = net_of(c), c['K']
    ad, bd = c['a'].cuda(), c['b'].cuda()
    logits, _, grad = train_step(hip, lib.input_patches(hip.shape, ad, bd), B, K, None, c['dl'].contiguous().cuda(), 1.0)
    within(logits, c['logits'], ac.LOGIT_TOL, 'dlogits-route logits %s' % c['what'])
    check_grads(hip, grad, c['dl_grads'], c['what'] + ' from dlogits')


# --------------------------------------------------------------------------------------------------------------- 4. stale
@pytest.mark.parametrize('name,B', ac.STALE)
def test_nothing_stale_is_read(name, B):
    """The train step into fresh buffers whose workspace and attention workspace hold bytes 0x00, 0xFF (NaN patterns) and
    0x00 again: logits, loss and the reduced gradient are bit-identical in all three.  The masked keys and the pad tokens (103
    of 128 on tiny1, 7 on hsi) are never read from memory that no launch of this step wrote, and slab_acc's sum over a
    workgroup's patches has one order."""
    from dmf import lib
    c = ac.case(name, B)
    hip, K = net_of(c), c['K']
    ad, bd = c['a'].cuda(), c['b'].cuda()
    lab = c['labels'].int().cuda()
    runs = [train_step(hip, lib.input_patches(hip.shape, ad, bd), B, K, lab, None, 1.0 / B, fill) for fill in (0x00, 0xFF, 0x00)]
    for what, i in (('logits', 0), ('loss', 1), ('gradient', 2)):
        assert not torch.isnan(runs[0][i]).any(), what + ' holds a NaN'
        assert torch.equal(runs[0][i], runs[1][i]), '%s differs between the 0x00 and the 0xFF fill %s' % (what, c['what'])
        assert torch.equal(runs[0][i], runs[2][i]), '%s differs between two runs on the 0x00 fill %s' % (what, c['what'])


# -------------------------------------------------------------------------------------------------------------- 5. engine
@functools.lru_cache(maxsize=None)
def engine_run():
    """Three fused engine steps of the sharp tiny1 net (resident scene, B = 32, lr 1e-2) and torch Adam on the oracle ->
    (losses, oracle's losses, absolute parameter differences)."""
    from dmf.engine import Scene, TrainEngine
    from model.gmfnet import Net as HipNet
    from oracle import solver_ref
    e = ac.ENGINE
    C, C2, P, S, K = SHAPES[e['name']]
    cfg, ref, A, Bm, xy, lab = ac.engine_case()
    hip = HipNet(cfg)
    hip.load_state_dict(ref.state_dict())
    hip = hip.to('cuda:0')                   # a net of its own: the engine updates it
    eng = TrainEngine(hip, Scene(A.numpy(), Bm.numpy(), 'cuda:0'), e['B'], lr=e['lr'])
    eng.load_plan(xy, lab)
    eng.run_plan(e['steps'], 0)
    got_losses = eng.mean_losses().numpy()
    want_losses, _ = solver_ref.train_steps(ref, A.numpy(), Bm.numpy(), xy.numpy(), lab.numpy(), e['B'], P, S, lr=e['lr'])
    d = torch.cat([(ph.detach().cpu() - pr.detach()).abs().reshape(-1)
                   for (_, pr), (_, ph) in zip(ref.named_parameters(), hip.named_parameters())]).numpy()
    return got_losses, np.array(want_losses), d


def test_sharp_engine_steps_losses():
    """The losses of three engine steps within 5e-4 of the oracle's, and no parameter further from the oracle's than the
    2 * steps * lr Adam can move it (test_gpu_parity.test_attention_autograd_and_engine_steps)."""
    got, want, d = engine_run()
    print('sharp engine losses', got, want, 'worst difference %.2e; largest parameter difference %.2e' % (np.abs(got - want).max(), d.max()))
    assert np.abs(got - want).max() < ac.ENGINE_LOSS_TOL
    assert d.max() <= 2 * ac.ENGINE['steps'] * ac.ENGINE['lr'] + 1e-6


def test_sharp_engine_steps_parameters():
    """99th percentile of the parameter differences after the three steps < attn_cases.ENGINE_P99 = 4 x 4.5e-4 = 1.8e-3.

    test_gpu_parity.test_attention_autograd_and_engine_steps holds the flat net to 2e-4.  On the sharp net the kernel shows
    4.18e-4 on an MI355X (1.66e-4 / 3.05e-4 / 4.18e-4 after steps 1 / 2 / 3; the flat net on the same plan 1.74e-4), in attn_wk
    (318 elements above 2e-4) and attn_wq (49).  Cause and bound come from an experiment on the reference alone
    (attn_cases.split_experiment, asserted by tests/test_attn_cases_host.py::test_engine_steps_reference_experiment): eight
    channels of the auxiliary branch are constant over a tiny1 patch, and since every row of dS sums to zero their columns of
    dWk = dK^T Tb cancel: 768 gradient elements, 3.5 % of all parameters, are rounding noise of ~1e-10 around zero in the
    oracle too.  Adam's first steps, g / (|g| + 1e-8), turn a difference of 1e-9 in such an element into 0.1 lr.  The kernel
    feeds dS, dQs and dK to the matrix cores as hi + lo bf16 (relative error 2^-17, by design); the ORACLE with the same split
    on the same operands moves its own parameters by a 99th percentile of 1.97e-4 / 3.33e-4 / 4.8e-4 after steps 1 / 2 / 3
    (4.75e-4 .. 4.84e-4 with the number of CPU threads; taken as 4.5e-4).  The bound is 4 x that movement of the reference, not
    a figure of the kernel's; it stays 16 x below the 3 lr an element with a wrong gradient sign moves.  The gradients
    themselves are held to the oracle's by test_sharp_train_cross_entropy (3e-4 of each tensor's maximum at worst)."""
    got, want, d = engine_run()
    print('sharp engine parameters after 3 steps: 99th percentile diff %.2e (bound %.2e), max %.2e, %d of %d above %g' % (
        np.percentile(d, 99), ac.ENGINE_P99, d.max(), int((d > ac.ENGINE_P99_FLAT).sum()), d.size, ac.ENGINE_P99_FLAT))
    assert np.percentile(d, 99) < ac.ENGINE_P99
