"""GPU: class weights, label smoothing and the focal term inside the attention network's train step (DESIGN.md §12a:
dmf_ce_denominators, dmf_train_attn_fwd_bwd_ce, TrainEngine(attention net, criterion=..., criterion_in_kernel=True)).

The main statement is BIT-equality with the composition of the entry points that existed before (route A):
    dmf_train_attn_fwd_bwd(labels)  ->  the logits the training kernel writes
    dmf_ce_loss on them             ->  loss rows, dlogits
    dmf_train_attn_fwd_bwd(dlogits) + dmf_grad_reduce
against route B, dmf_ce_denominators + dmf_train_attn_fwd_bwd_ce + dmf_grad_reduce: `torch.equal` on logits, loss and the whole flat
gradient.  Both routes call one statement of the arithmetic (csrc/dmf_ce_math.h); the attention kernel holds class k in lane k
of a 64-lane wave for every K while dmf_ce_loss uses 16-lane groups when K <= 16 (tiny1, K = 5) and whole waves otherwise (hsi,
K = 17).  Batches: a training launch has grid min(B, 256), so 257 and 513 make a workgroup walk a second and a third patch.
Against the oracle (oracle/gmfnet_ref.py under tests/loss_ref.py's criteria, autograd, torch Adam) the tolerances are those of
tests/attn_cases.py and of test_gpu_parity.py::test_attention_autograd_and_engine_steps.
"""
import copy
import shutil
import tempfile

import numpy as np
import pytest
import torch

import attn_ce_ref
import attn_cases as ac
import loss_ref
import parity_cases as pc
from test_gpu_parity import SHAPES, _scene, rand_batch

pytestmark = pytest.mark.gpu

CRITERIA = [(n, s, w) for n, s, w in loss_ref.VARIANTS] + [('focal1.5+weights', dict(kind='focal', gamma=1.5), True)]
ORACLE_CRITERIA = {'ce': dict(kind='ce', eps=0.1), 'focal': dict(kind='focal', gamma=2.0)}     # both with class weights


def hip_of(cfg, ref):
    from model.gmfnet import Net as HipNet
    hip = HipNet(cfg)
    hip.load_state_dict(ref.state_dict())
    return hip.to('cuda:0')


_NETS = {}


def sharp(name):
    """(cfg, oracle net, HIP net) of attn_cases.sharp_net(name), built once; no test changes their weights."""
    if name not in _NETS:
        cfg, ref = ac.sharp_net(name)
        _NETS[name] = (cfg, ref, hip_of(cfg, ref))
    return _NETS[name]


def params_of(spec):
    from dmf import lib
    return lib.ce_params(spec['kind'], spec.get('eps', 0.0), spec.get('gamma', 0.0))


class Bufs:
    """Fresh outputs and workspaces of one train launch of B patches, NaN-filled where a result is expected."""

    def __init__(self, hip, B, K):
        from dmf import lib
        self.logits = torch.full((B, K), float('nan'), device='cuda')
        self.loss = torch.full((B,), float('nan'), device='cuda')
        self.ws = torch.empty(lib.workspace_bytes(hip.shape, B) // 4, device='cuda')
        self.aws = torch.empty(lib.attn_train_workspace_bytes(hip.shape, B), dtype=torch.uint8, device='cuda')


def reduce(hip, B, ws, theta):
    from dmf import lib
    grad = torch.full_like(theta, float('nan'))
    lib.grad_reduce(hip.shape, B, ws, grad)
    return grad


def kernel_logits(hip, inp, theta, B, K, own_labels):
    """Route A, first launch: the logits the training kernel writes (its fused cross-entropy is not looked at)."""
    from dmf import lib
    x = Bufs(hip, B, K)
    lib.train_attn_fwd_bwd(hip.shape, inp, theta, hip.pool_w, own_labels, None, 1.0 / B, x.logits, x.loss, x.ws, x.aws)
    return x.logits


def route_a(hip, inp, theta, B, K, logits, labels_g, spec, w, ranks=1, rank=0, cursor=None, grad_scale=1.0):
    from dmf import lib
    loss = torch.full((B,), float('nan'), device='cuda')
    dl = torch.full((B, K), float('nan'), device='cuda')
    lib.ce_loss(logits, ranks, rank, labels_g, params_of(spec), class_w=w, loss=loss, dlogits=dl, grad_scale=grad_scale, cursor=cursor)
    x = Bufs(hip, B, K)
    lib.train_attn_fwd_bwd(hip.shape, inp, theta, hip.pool_w, None, dl, 1.0, x.logits, None, x.ws, x.aws)
    return x.logits, loss, reduce(hip, B, x.ws, theta)


def route_b(hip, inp, theta, B, K, labels_g, spec, w, ranks=1, rank=0, grad_scale=1.0):
    from dmf import lib
    rows = labels_g.numel() // (ranks * B)
    denom = torch.full((rows,), float('nan'), dtype=torch.float64, device='cuda')
    lib.ce_denominators(labels_g, ranks * B, K, denom, w)
    x = Bufs(hip, B, K)
    lib.train_attn_fwd_bwd_ce(hip.shape, inp, theta, hip.pool_w, labels_g, denom, params_of(spec), ranks, rank, x.logits, x.loss, x.ws,
                              x.aws, class_w=w, grad_scale=grad_scale)
    return x.logits, x.loss, reduce(hip, B, x.ws, theta)


def same_bits(got, want, what):
    got, want = got.cpu(), want.cpu()
    assert torch.isfinite(want).all(), what + ': the composed route is not finite'
    if not torch.equal(got, want):
        bad = got != want
        d = (got.double() - want.double()).abs()
        raise AssertionError('%s: %d of %d elements differ, max |diff| %.3e (max |want| %.3e)' % (
            what, int(bad.sum()), bad.numel(), d[bad].max().item(), want.abs().max().item()))


def both_routes(hip, inp, theta, B, K, t, w, what, criteria=CRITERIA):
    """Every criterion on one batch: route A against route B, bit for bit.  The first launch of route A is shared."""
    labels = t.int().cuda()
    logits0 = kernel_logits(hip, inp, theta, B, K, labels)
    for cname, spec, weighted in criteria:
        cw = w.cuda() if weighted else None
        la, va, ga = route_a(hip, inp, theta, B, K, logits0, labels, spec, cw)
        lb, vb, gb = route_b(hip, inp, theta, B, K, labels, spec, cw)
        torch.cuda.synchronize()
        tag = '%s %s' % (what, cname)
        same_bits(la, logits0, tag + ': logits of the dlogits launch')
        same_bits(lb, logits0, tag + ': logits')
        same_bits(vb, va, tag + ': loss')
        same_bits(gb, ga, tag + ': gradient')
    return logits0


# ------------------------------------------------------------------------------ 1. bit-equality with the composed route
@pytest.mark.parametrize('name,B', [('tiny1', 1), ('tiny1', 2), ('tiny1', 257), ('tiny1', 513), ('hsi', 2), ('hsi', 33)])
def test_fused_criterion_is_the_composed_route_bit_for_bit(name, B):
    """The ten loss_ref.VARIANTS and focal with gamma 1.5 (the powf path), weights spanning 0.01 ... 50."""
    from dmf import lib
    cfg, ref, hip = sharp(name)
    K = SHAPES[name][4]
    a, b, t = rand_batch(name, B, 3)
    w = loss_ref.class_weights(K, torch.Generator().manual_seed(7))
    ad, bd = a.cuda(), b.cuda()                       # (an Input holds addresses only: the tensors must outlive it)
    inp = lib.input_patches(hip.shape, ad, bd)
    both_routes(hip, inp, hip.flat_parameters(), B, K, t, w, '[%s, B=%d]' % (name, B))


def test_wide_logits_and_an_absent_class():
    """fc2.weight x 20, and x 600: on this net (logits -0.11 .. 0.27) the first factor widens the logits to -3.5 .. 5.9, where the
    smallest p_y is 1.1e-4; only the second makes some p_y underflow in float32, which is what the case is for.  Then a batch in
    which class 0 does not occur."""
    from dmf import lib
    name, B = 'tiny1', 70
    cfg, ref, hip = sharp(name)
    K = SHAPES[name][4]
    a, b, t = rand_batch(name, B, 3)
    w = loss_ref.class_weights(K, torch.Generator().manual_seed(7))
    ad, bd = a.cuda(), b.cuda()
    inp = lib.input_patches(hip.shape, ad, bd)
    i = hip._order().index('fc2.weight')
    n = dict(zip(hip._order(), hip._named()))['fc2.weight'].numel()
    narrow = kernel_logits(hip, inp, hip.flat_parameters(), B, K, t.int().cuda()).cpu()
    zeros = {}
    for factor in (20.0, 600.0):
        theta = hip.flat_parameters().detach().clone()
        theta[hip._offsets[i]:hip._offsets[i] + n] *= factor
        logits = both_routes(hip, inp, theta, B, K, t, w, '[fc2.weight x %g]' % factor).cpu()
        py = torch.softmax(logits, 1).gather(1, t.view(-1, 1))
        zeros[factor] = int((py == 0).sum())
        print('logits x %g: range %.1f .. %.1f (the net\'s own: %.2f .. %.2f), smallest p_y %.2e, %d of %d p_y are zero in float32' % (
            factor, logits.min(), logits.max(), narrow.min(), narrow.max(), py.min(), zeros[factor], B))
        assert logits.max() - logits.min() > 0.5 * factor * (narrow.max() - narrow.min())
    assert zeros[600.0] > 0
    t2 = t.clone()
    t2[t2 == 0] = 1
    assert not (t2 == 0).any() and (t == 0).any()
    both_routes(hip, inp, hip.flat_parameters(), B, K, t2, w, '[class 0 absent]')


# ----------------------------------------------------------------------------------------------- 2. cursor and ranks
def test_cursor_and_ranks():
    """A plan of 3 rows with the cursor at row 2; then two ranks, each on its half of the global batch: loss rows bit-equal to
    the one-rank call on the whole batch, each rank's gradient bit-equal to route A with dmf_ce_loss(ranks = 2, rank = r)."""
    from dmf import lib
    name, Bh, rows = 'tiny1', 35, 3
    N = 2 * Bh
    cfg, ref, hip = sharp(name)
    K = SHAPES[name][4]
    A, Bm, xy, t, _, _ = pc.inputs(name, rows * N)
    w = loss_ref.class_weights(K, torch.Generator().manual_seed(7)).cuda()
    Ad, Bd = A.cuda(), Bm.cuda()
    lib.check_xy_bounds(hip.shape, Ad, Bd, xy.numpy())
    labels_g = t.int().cuda()                                   # [rows][N], rank-major inside a row
    cursor = torch.tensor([2], dtype=torch.int32, device='cuda')
    theta = hip.flat_parameters()
    for cname, spec in ORACLE_CRITERIA.items():
        # one rank, the whole batch
        xy_all = xy.cuda()
        inp = lib.input_gather(hip.shape, Ad, Bd, xy_all, B=N, cursor=cursor)
        logits0 = kernel_logits(hip, inp, theta, N, K, labels_g)
        la, va, ga = route_a(hip, inp, theta, N, K, logits0, labels_g, spec, w, cursor=cursor)
        lb, vb, gb = route_b(hip, inp, theta, N, K, labels_g, spec, w)
        torch.cuda.synchronize()
        same_bits(lb, logits0, cname + ' whole batch at cursor 2: logits')
        same_bits(vb, va, cname + ' whole batch at cursor 2: loss')
        same_bits(gb, ga, cname + ' whole batch at cursor 2: gradient')
        # ... and the cursor matters: row 2's samples, not row 0's
        want = logits0.cpu()
        for r in range(2):
            xy_r = xy.view(rows, 2, Bh, 2)[:, r].reshape(-1, 2).contiguous().cuda()
            own = t.view(rows, 2, Bh)[:, r].reshape(-1).int().cuda()
            inp_r = lib.input_gather(hip.shape, Ad, Bd, xy_r, B=Bh, cursor=cursor)
            lg_r = kernel_logits(hip, inp_r, theta, Bh, K, own)
            same_bits(lg_r, want[r * Bh:(r + 1) * Bh], '%s rank %d: logits against the whole batch' % (cname, r))
            _, var, gar = route_a(hip, inp_r, theta, Bh, K, lg_r, labels_g, spec, w, ranks=2, rank=r, cursor=cursor)
            lbr, vbr, gbr = route_b(hip, inp_r, theta, Bh, K, labels_g, spec, w, ranks=2, rank=r)
            torch.cuda.synchronize()
            same_bits(lbr, lg_r, '%s rank %d: logits' % (cname, r))
            same_bits(vbr, vb[r * Bh:(r + 1) * Bh], '%s rank %d: loss rows against the one-rank call' % (cname, r))
            same_bits(vbr, var, '%s rank %d: loss rows against dmf_ce_loss(ranks=2)' % (cname, r))
            same_bits(gbr, gar, '%s rank %d: gradient' % (cname, r))
    first = pc.cut(A, Bm, xy[:N], SHAPES[name][2], SHAPES[name][3])
    fa, fb = first[0].cuda(), first[1].cuda()
    lg_first = kernel_logits(hip, lib.input_patches(hip.shape, fa, fb), theta, N, K, labels_g[:N])
    assert not torch.equal(lg_first.cpu(), want), 'plan rows 0 and 2 give the same logits: the cursor is not tested'


# ----------------------------------------------------------------------------------------------------- 3. denominators
@pytest.mark.parametrize('weights', (False, True), ids=('ones', 'weights'))
@pytest.mark.parametrize('K', (5, 64))
def test_denominators_are_the_host_restatement_bit_for_bit(K, weights):
    from dmf import lib
    g = torch.Generator().manual_seed(50 + K)
    w = loss_ref.class_weights(K, g) if weights else None
    for N in (1, 255, 256, 257, 1025):
        rows = 3
        y = torch.randint(0, K, (rows * N,), generator=g).int()
        denom = torch.full((rows,), float('nan'), dtype=torch.float64, device='cuda')
        lib.ce_denominators(y.cuda(), N, K, denom, None if w is None else w.cuda())
        want = attn_ce_ref.denominators(y.numpy(), N, K, None if w is None else w.numpy())
        got = denom.cpu().numpy()
        assert got.tobytes() == want.tobytes(), 'N=%d K=%d: %s != %s' % (N, K, got.tolist(), want.tolist())


# ------------------------------------------------------------------------------------------------ 4. against the oracle
@pytest.mark.parametrize('cname', sorted(ORACLE_CRITERIA))
def test_gradient_against_autograd(cname):
    """One batch of 70 on the sharp net: logits to attn_cases.LOGIT_TOL, every gradient tensor to attn_cases.grad_tol."""
    from dmf import lib
    from test_gpu_attn_sharp import check_grads, within
    name, B = 'tiny1', 70
    cfg, ref, hip = sharp(name)
    K = SHAPES[name][4]
    a, b, t = rand_batch(name, B, 2)
    w = loss_ref.class_weights(K, torch.Generator().manual_seed(7))
    spec = ORACLE_CRITERIA[cname]
    ref.zero_grad()
    want_logits = ref(a, b)
    value = loss_ref.criterion_value(want_logits, t, **loss_ref.ref_spec(spec, w))
    value.backward()
    want_g = {k: p.grad.detach().clone() for k, p in ref.named_parameters()}
    ref.zero_grad()
    ad, bd = a.cuda(), b.cuda()
    inp = lib.input_patches(hip.shape, ad, bd)
    logits, loss, grad = route_b(hip, inp, hip.flat_parameters(), B, K, t.int().cuda(), spec, w.cuda())
    torch.cuda.synchronize()
    within(logits, want_logits, ac.LOGIT_TOL, 'logits [%s]' % cname)
    print('batch loss [%s]: got %.6f want %.6f' % (cname, loss.double().mean().item(), value.item()))
    assert abs(loss.double().mean().item() - value.item()) < ac.LOSS_TOL
    check_grads(hip, grad, want_g, '[%s, B=%d]' % (cname, B))


def _oracle_steps(ref, A, Bm, xy, lab, Bn, P, S, lr, crit):
    from oracle import solver_ref
    net = copy.deepcopy(ref)
    opt = torch.optim.Adam(net.parameters(), lr=lr)
    net.train()
    losses = []
    for i in range(0, len(xy) - Bn + 1, Bn):
        a, b = solver_ref.materialise(A.numpy(), Bm.numpy(), xy.numpy()[i:i + Bn], P, S)
        opt.zero_grad()
        loss = crit(net(a, b), lab[i:i + Bn].long())
        loss.backward()
        opt.step()
        losses.append(loss.item())
    return net, np.array(losses)


ENGINE_NETS = {
    # the net test_gpu_parity.py::test_attention_autograd_and_engine_steps steps, with that test's bounds: step losses 5e-4, 99th
    # percentile of the parameter differences 2e-4
    'flat': (None, 5e-4, 2e-4),
    # attn_cases.sharp_net: the loss bound is the same; the percentile bound is attn_cases.ENGINE_P99, four times what the
    # REFERENCE moves against itself once its q / k backward takes the kernel's hi / lo bf16 operands (attn_cases, on the CPU alone:
    # 4.75e-4).  2e-4 is not a bound for this net: measured here 6.3e-4 (ce) and 8.2e-4 (focal) on eager steps, and 4.18e-4 for the
    # plain criterion (profiles/attn_sharp.md)
    'sharp': (None, ac.ENGINE_LOSS_TOL, ac.ENGINE_P99),
}


@pytest.mark.parametrize('net', sorted(ENGINE_NETS))
@pytest.mark.parametrize('cname', sorted(ORACLE_CRITERIA))
def test_engine_steps_against_torch_adam(cname, net):
    """Three TrainEngine(criterion=..., criterion_in_kernel=True) ADAM steps of 32 patches at lr 1e-2, eager and from a captured
    graph, against torch Adam on the oracle under the same criterion (ENGINE_NETS: the nets and their bounds); the graph's weights are the eager ones, bit for
    bit.  ADAM's first steps move every element by ~lr whatever the size of its gradient, so the tail is bounded by steps * lr."""
    from dmf import lib
    from dmf.engine import Scene, TrainEngine
    e = ac.ENGINE
    C, C2, P, S, K = SHAPES[e['name']]
    cfg, ref, A, Bm, xy, lab = ac.engine_case()
    _, loss_tol, p99_tol = ENGINE_NETS[net]
    if net == 'flat':
        cfg = pc.build_cfg(e['name'], attention=True)
        ref = pc.oracle_net(cfg)
    w = loss_ref.class_weights(K, torch.Generator().manual_seed(7))
    spec = ORACLE_CRITERIA[cname]
    want_net, want_losses = _oracle_steps(ref, A, Bm, xy, lab, e['B'], P, S, e['lr'], loss_ref.module(**loss_ref.ref_spec(spec, w)))
    crit = dict(kind=spec['kind'], label_smoothing=spec.get('eps', 0.0), gamma=spec.get('gamma', 0.0), class_weights=w.tolist())
    thetas, figures = {}, {}
    for mode, per_graph in (('eager', 0), ('graph', 3)):
        hip = hip_of(cfg, ref)
        eng = TrainEngine(hip, Scene(A.numpy(), Bm.numpy(), 'cuda:0'), e['B'], lr=e['lr'], criterion=crit, criterion_in_kernel=True)
        assert not eng.fused and eng.criterion is not None
        if mode == 'eager':                           # without the keyword the constructor refuses, as it always has
            with pytest.raises(lib.DmfError, match='attention'):
                TrainEngine(hip, eng.scene, e['B'], lr=e['lr'], criterion=crit)
        eng.load_plan(xy, lab)
        eng.run_plan(e['steps'], per_graph)
        assert (eng.graph is not None) == (per_graph > 0)
        got_losses = eng.mean_losses().numpy()
        d = torch.cat([(ph.detach().cpu() - pr.detach()).abs().reshape(-1)
                       for (_, pr), (_, ph) in zip(want_net.named_parameters(), hip.named_parameters())]).numpy()
        figures[mode] = (np.abs(got_losses - want_losses).max(), np.percentile(d, 99), d.max())
        print('%s %s %s: losses %s want %s; parameters after 3 steps: 99th percentile diff %.2e, max %.2e' % (
            net, cname, mode, got_losses, want_losses, figures[mode][1], figures[mode][2]))
        thetas[mode] = eng.theta.detach().clone()
    for mode, (dl, p99, dmax) in figures.items():
        assert dl < loss_tol, (mode, dl)
        assert p99 < p99_tol and dmax <= 2 * 3 * e['lr'] + 1e-6, (mode, p99, dmax)
    assert torch.equal(thetas['eager'], thetas['graph']), 'the captured graph does not take the eager steps'


# ----------------------------------------------------------------------------- 5. criterion=None is the engine of before
def test_no_criterion_is_the_plain_engine():
    """Three eager steps of TrainEngine(attention net) against the launches that engine has always made: dmf_train_attn_fwd_bwd
    with labels and 1 / B, dmf_grad_reduce_adam."""
    from dmf import lib
    from dmf.engine import Scene, TrainEngine
    e = ac.ENGINE
    C, C2, P, S, K = SHAPES[e['name']]
    cfg, ref, A, Bm, xy, lab = ac.engine_case()
    Bn = e['B']
    scene = Scene(A.numpy(), Bm.numpy(), 'cuda:0')
    hip = hip_of(cfg, ref)
    eng = TrainEngine(hip, scene, Bn, lr=e['lr'], criterion=None)
    assert eng.fused and eng.criterion is None and eng.plan_denom is None
    hip2 = hip_of(cfg, ref)
    theta = hip2.flat_parameters()
    m, v = torch.zeros_like(theta), torch.zeros_like(theta)
    x = Bufs(hip2, Bn, K)
    for k in range(e['steps']):
        xy_k, lab_k = xy[k * Bn:(k + 1) * Bn].cuda(), lab[k * Bn:(k + 1) * Bn].cuda()
        eng.step(xy_k, lab_k)
        inp = lib.input_gather(hip2.shape, scene.A, scene.B, xy_k)
        lib.train_attn_fwd_bwd(hip2.shape, inp, theta, hip2.pool_w, lab_k, None, 1.0 / Bn, x.logits, x.loss, x.ws, x.aws)
        lib.grad_reduce_adam(hip2.shape, Bn, x.ws, theta, m, v, None, e['lr'], 0.9, 0.999, 1e-8, k + 1)
    torch.cuda.synchronize()
    assert torch.equal(eng.theta, theta) and torch.equal(eng.loss, x.loss)


# ---------------------------------------------------------------------------------------------------------- 6. the solver
def test_solver_trains_the_attention_network_with_a_criterion_on_both_paths(golden_dir):
    """`gmf.attention: 1` + `class_weights: balanced, label_smoothing: 0.05` through `Solver(cfg).run()` on the synthetic scene:
    the fast path and the drop-in path agree at the tolerances of
    test_gpu_trajectory.py::test_solver_trains_the_attention_network_on_both_paths."""
    from dmf import synth
    from solver.mainsolver import Solver
    from test_gpu_trajectory import _setup
    runs = {}
    for fast in (1, 0):
        tmp = tempfile.mkdtemp(prefix='dmf_attn_crit_solver_')
        try:
            g, cfg = _setup(golden_dir, tmp, fast_path=fast, epoch=4, scale=1)
            cfg['gmf'] = dict(cfg['gmf'], attention=1)
            cfg['trans'] = {'embed_dim': 96, 'num_head': 3}
            cfg['schedule'] = dict(cfg['schedule'], class_weights='balanced', label_smoothing=0.05)
            primary, aux, label = synth.make_scene(20, 20, 8, 1, 1, n_classes=4, seed=3)      # aux at the primary's resolution
            d = cfg['data_address']
            np.save(d + 'ms4.tif.npy', primary); np.save(d + 'pan.tif.npy', aux); np.save(d + 'label.npy', label)
            torch.manual_seed(3407)
            s = Solver(cfg)
            s.run()
            assert s.criterion is not None and s.criterion['kind'] == 'ce'
            if fast:
                assert s.engine.shape.attention and s.engine.criterion is not None and not s.engine.fused
            runs[fast] = (np.array(s.step_losses), s.test_matrix.copy(), s.result[2])
        finally:
            shutil.rmtree(tmp)
    lf, ld = runs[1][0], runs[0][0]
    assert lf.shape == ld.shape and len(lf) == 16
    print('attention solver with a criterion: fast vs drop-in loss diff %.2e, first %.4f last %.4f, kappa %.4f / %.4f'
          % (np.abs(lf - ld).max(), lf[0], lf[-1], runs[1][2], runs[0][2]))
    assert np.abs(lf - ld).max() < 2e-4 and lf[-1] < lf[0]
    assert int(np.abs(runs[1][1] - runs[0][1]).sum() // 2) <= 1
