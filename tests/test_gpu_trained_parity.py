"""GPU: the patch kernel (csrc/dmf_patch_v2.hip) and the reduce launch behind it at TRAINED weights, against the oracle in
float64 (tests/trained_cases.py; its guards run on the CPU in tests/test_trained_cases_host.py).

Every other parity module runs the seed-0 net with 0.05 noise, where the logits stay within +-0.02: the softmax of the fused
cross-entropy is flat, so dl = (1/K - onehot) / B to three digits whatever the head wave does with its maximum, its sum or its
exponential; no probability is below 1e-3; a hidden unit is open for every patch of a launch or for none; and gradients of
1e-3 are judged by the absolute term of their tolerance.  Here max |logit| reaches 8 .. 27, losses 12 .. 38, probabilities
1e-6 .. 1e-17, gradients 0.3 .. 2 (the relative term judges), and fc1 has units of all three kinds within one launch.

Everything goes through the C ABI, the way tests/test_gpu_batch_walk.py drives it.  Per case and batch:
  forward              dmf_forward and dmf_forward_ce, gather and materialised: logits, pred outside the margin cap, per-patch
                       loss; the two input modes bit-equal
  train                MODE_TRAIN + dmf_grad_reduce: logits, per-patch loss, every gradient, z / h / dh / dl of the workspace
  backward             MODE_BWD from the oracle's dL/dlogits, and the unit-gradient step (dmf_forward_unit, the caller's dl,
                       dmf_backward_unit) on the rows that have one
  half                 the same passes on the fp16 scene against the float64 oracle with the fp16 roundings
  Adam                 dmf_grad_reduce_adam from recorded moments and step count against adam_step_ref in float64 fed the
                       kernel's own gradient (the update is ill-conditioned in g where v ~ g^2 ~ 0; the gradient itself is
                       held to the oracle by the train pass)
  ten launches         bit-equal
Tolerances: trained_cases.py (logits and loss widened from the two oracles only, printed per test; gradients and head vectors
1e-5 + 1e-4 |want|).  The worst error per pass of one run is kept in profiles/trained_parity.md.
"""
import functools

import pytest
import torch

import trained_cases as tc
from test_gpu_batch_walk import make_input
from test_gpu_exit_path import split_ws
from test_gpu_seams import assert_close

pytestmark = pytest.mark.gpu

WORST = {}          # pass -> (worst abs err, max |ref|, atol, rtol)
CELLS = tc.cells()
UNIT_CELLS = [c for c in CELLS if tc.row_of(c[0]) in tc.UNIT_ROWS]
ADAM_CELLS = [c for c in CELLS if c[0] in tc.ADAM_CASES and not c[2]]


def close(pass_, got, want, atol, rtol, what):
    got, want = got.detach().cpu(), want.detach().cpu()
    err = (got.double() - want.double()).abs().max().item() if got.numel() else 0.0
    if err >= WORST.get(pass_, (-1.0,))[0]:
        WORST[pass_] = (err, want.abs().max().item(), atol, rtol)
    assert_close(got, want, atol + rtol * want.double().abs(), what)


@pytest.fixture(scope='module', autouse=True)
def worst_errors_table():
    yield
    print('\n| pass | worst abs err | max abs ref | tolerance |')
    print('|---|---|---|---|')
    for k in sorted(WORST):
        e, r, atol, rtol = WORST[k]
        print('| %s | %.2e | %.2e | %.2g%s |' % (k, e, r, atol, ' + %g ref' % rtol if rtol else ''))


@functools.lru_cache(maxsize=None)
def gpu_case(name, B, half=False):
    """The case, its HIP net and its inputs on the device (kept alive: input descriptors hold raw pointers)."""
    from model.gmfnet import PARAM_ORDER, Net as HipNet
    c = tc.case(name, B, half)
    hip = HipNet(c['cfg'])
    hip.load_state_dict(c['state'])
    hip = hip.to('cuda:0')
    A = c['A'].cuda()
    d = dict(c, hip=hip, theta=hip.flat_parameters(), Ad=A.to(torch.float16) if half else A, Bd=c['Bm'].cuda(), xyd=c['xy'].cuda(),
             ad=c['a'].cuda(), bd=c['b'].cuda(), labels_d=c['labels'].int().cuda())
    off = hip._offsets
    d['views'] = {k: (off[i], c['grads'][k].numel(), c['grads'][k].shape) for i, k in enumerate(hip._order())}
    d['slab'] = (off[8] + 31) & ~31
    d['F2'] = 2 * hip.arch['F']
    assert PARAM_ORDER == hip._order()[:12]
    print('%s: logits tolerance %.2e, loss tolerance %.2e; d_s %s' % (
        c['what'], c['logit_tol'], c['loss_tol'], ' '.join('%s %.1e' % (s, c['measured']['delta'][s]) for s in tc.SITES)))
    return d


def tag(c, *more):
    return c['what'][:-1] + ''.join(', ' + m for m in more) + ']'


def kind(c):
    return '%s %s' % (c['name'], 'half' if c['half'] else 'fp32')


def check_grads(pass_, c, grad, want_g, what):
    grad = grad.cpu()
    for k, want in want_g.items():
        o, n, shp = c['views'][k]
        close(pass_, grad[o:o + n].view(shp), want, tc.ATOL, tc.RTOL, 'grad %s %s' % (k, what))


def check_head_vectors(pass_, c, ws, want_hv, keys, what):
    got = split_ws(ws.cpu(), c['slab'], c['B'], c['F2'], 64)
    for k in keys:
        close(pass_, got[k], want_hv[k], tc.ATOL, tc.RTOL, 'workspace %s %s' % (k, what))
    return got


def check_pred(c, pred, logits, what):
    pred = pred.cpu().long()
    assert torch.equal(pred, logits.cpu().argmax(1)), 'pred != argmax of the GPU logits ' + what
    safe = c['safe']
    assert torch.equal(pred[safe], c['pred'][safe]), 'pred != oracle class on %d safe patches %s' % (int(safe.sum()), what)


def train_run(c, mode, theta=None):
    from dmf import lib
    hip, B, K = c['hip'], c['B'], c['K']
    inp = make_input(c, mode)
    logits = torch.full((B, K), float('nan'), device='cuda'); loss = torch.full((B,), float('nan'), device='cuda')
    ws = torch.zeros(lib.workspace_bytes(hip.shape, B) // 4, device='cuda')
    lib.train_fwd_bwd(hip.shape, inp, c['theta'] if theta is None else theta, hip.pool_w, c['labels_d'], 1.0 / B, logits, loss, ws)
    grad = torch.empty_like(c['theta'])
    lib.grad_reduce(hip.shape, B, ws, grad)
    torch.cuda.synchronize()
    return logits, loss, ws, grad


# ------------------------------------------------------------------------------------------------------------- 1. forward
@pytest.mark.parametrize('name,B,half', CELLS)
def test_forward(name, B, half):
    """MODE_FWD: dmf_forward with pred and dmf_forward_ce, whose loss is mx + log(se) - logit[label] at mx up to 27."""
    from dmf import lib
    c = gpu_case(name, B, half)
    hip, K = c['hip'], c['K']
    runs = {}
    for mode in ('gather', 'patches'):
        inp = make_input(c, mode)
        logits = torch.full((B, K), float('nan'), device='cuda'); pred = torch.full((B,), -1, dtype=torch.int32, device='cuda')
        lib.forward(hip.shape, inp, c['theta'], hip.pool_w, logits, pred)
        logits_ce = torch.full((B, K), float('nan'), device='cuda'); loss = torch.full((B,), float('nan'), device='cuda')
        pred_ce = torch.full((B,), -1, dtype=torch.int32, device='cuda')
        lib.forward_ce(hip.shape, inp, c['theta'], hip.pool_w, c['labels_d'], logits_ce, loss, pred_ce)
        torch.cuda.synchronize()
        r = runs[mode] = dict(logits=logits.cpu(), pred=pred.cpu(), logits_ce=logits_ce.cpu(), loss=loss.cpu(), pred_ce=pred_ce.cpu())
        what, p = tag(c, mode), 'forward %s' % kind(c)
        close(p + ': logits', r['logits'], c['logits'], c['logit_tol'], 0, 'forward logits ' + what)
        close(p + ': logits', r['logits_ce'], c['logits'], c['logit_tol'], 0, 'forward_ce logits ' + what)
        close(p + ': loss', r['loss'], c['loss'], c['loss_tol'], 0, 'forward_ce per-patch loss ' + what)
        check_pred(c, r['pred'], r['logits'], 'forward ' + what)
        check_pred(c, r['pred_ce'], r['logits_ce'], 'forward_ce ' + what)
    for k, v in runs['gather'].items():
        assert torch.equal(v, runs['patches'][k]), '%s: gather and materialised differ %s' % (k, tag(c))


# --------------------------------------------------------------------------------------------------------------- 2. train
@pytest.mark.parametrize('name,B,half', CELLS)
def test_fused_train_step(name, B, half):
    """MODE_TRAIN + the reduce, gather and materialised: the fused softmax / cross-entropy where it is not flat."""
    c = gpu_case(name, B, half)
    outs = []
    for mode in ('gather', 'patches'):
        logits, loss, ws, grad = train_run(c, mode)
        what, p = tag(c, mode), 'train %s' % kind(c)
        close(p + ': logits', logits, c['logits'], c['logit_tol'], 0, 'train logits ' + what)
        close(p + ': loss', loss, c['loss'], c['loss_tol'], 0, 'train per-patch loss ' + what)
        check_grads(p + ': grads', c, grad, c['grads'], what)
        check_head_vectors(p + ': z h dh dl', c, ws, c['hv'], ('z', 'h', 'dh', 'dl'), what)
        outs.append((logits.cpu(), loss.cpu(), grad.cpu()))
    for x, y in zip(*outs):
        assert torch.equal(x, y), 'gather and materialised differ ' + tag(c)


# ------------------------------------------------------------------------------------------- 3. the supplied-gradient routes
@pytest.mark.parametrize('name,B,half', CELLS)
def test_backward_from_dlogits(name, B, half):
    """MODE_BWD with the float64 oracle's dL/dlogits rounded to fp32."""
    from dmf import lib
    c = gpu_case(name, B, half)
    hip = c['hip']
    inp = make_input(c, 'gather')
    ws = torch.zeros(lib.workspace_bytes(hip.shape, B) // 4, device='cuda')
    dl = c['dlogits'].float().contiguous()
    lib.backward_dlogits(hip.shape, inp, c['theta'], hip.pool_w, dl.cuda(), ws)
    grad = torch.empty_like(c['theta'])
    lib.grad_reduce(hip.shape, B, ws, grad)
    torch.cuda.synchronize()
    what, p = tag(c, 'from dlogits'), 'backward %s' % kind(c)
    check_grads(p + ': grads', c, grad, c['grads'], what)
    got = check_head_vectors(p + ': z h dh dl', c, ws, c['hv'], ('z', 'h', 'dh', 'dl'), what)
    assert torch.equal(got['dl'][:, :c['K']], dl), 'dl is passed through as supplied'


def test_unit_step_rows():
    """UNIT_ROWS is what the library says: the rows of these cases with a two-launch unit-gradient step."""
    from dmf import lib
    for name, r in tc.RECIPES.items():
        c = gpu_case(name, tc.BATCHES[r['row']][0])
        assert lib.unit_supported(c['hip'].shape) == (r['row'] in tc.UNIT_ROWS), name


@pytest.mark.parametrize('name,B,half', UNIT_CELLS)
def test_unit_gradient_step(name, B, half):
    """MODE_UNIT + unit_backward_kernel + the reduce against autograd of the float64 oracle for dl = randn / B."""
    from dmf import lib
    c = gpu_case(name, B, half)
    hip, K = c['hip'], c['K']
    assert lib.unit_supported(hip.shape)
    inp = make_input(c, 'gather')
    logits = torch.full((B, K), float('nan'), device='cuda')
    ws = torch.zeros(lib.workspace_bytes(hip.shape, B) // 4, device='cuda')
    step = torch.full((1,), 7, dtype=torch.int32, device='cuda')
    lib.forward_unit(hip.shape, inp, c['theta'], hip.pool_w, logits, ws, adam_step_dev=step)
    lib.backward_unit(hip.shape, B, c['theta'], c['dl_unit'].cuda(), ws)
    grad = torch.empty_like(c['theta'])
    lib.grad_reduce(hip.shape, B, ws, grad)
    torch.cuda.synchronize()
    assert int(step.item()) == 8, 'the step count advances by exactly one'
    what, p = tag(c, 'unit step'), 'unit %s' % kind(c)
    close(p + ': logits', logits, c['logits'], c['logit_tol'], 0, 'unit-step logits ' + what)
    check_grads(p + ': grads', c, grad, c['unit_grads'], what)
    got = check_head_vectors(p + ': h dh dl', c, ws, c['unit_hv'], ('h', 'dh', 'dl'), what)
    assert torch.equal(got['dl'], c['unit_hv']['dl']), 'dl is passed through as supplied'


# ---------------------------------------------------------------------------------------------- 4. Adam at a real state
def flat_like(c, per_param):
    """Per-parameter tensors -> theta's flat layout (padding zero)."""
    flat = torch.zeros(c['theta'].numel(), dtype=torch.float32)
    for k, (o, n, shp) in c['views'].items():
        flat[o:o + n] = per_param[k].reshape(-1).float()
    return flat


@pytest.mark.parametrize('name,B,half', ADAM_CELLS)
def test_fused_adam_at_the_recorded_state(name, B, half):
    """dmf_grad_reduce_adam from the moments and the step count the oracle's Adam had when the weights were taken."""
    from dmf import lib
    from oracle.gmfnet_ref import adam_step_ref
    c = gpu_case(name, B, half)
    hip = c['hip']
    _, _, ws, grad0 = train_run(c, 'gather')
    theta = c['theta'].clone()
    m0, v0 = flat_like(c, c['adam']['m']), flat_like(c, c['adam']['v'])
    m, v = m0.cuda(), v0.cuda()
    step = c['adam']['step'] + 1
    grad = torch.empty_like(theta)
    lib.grad_reduce_adam(hip.shape, B, ws, theta, m, v, grad, c['lr'], 0.9, 0.999, 1e-8, step)
    torch.cuda.synchronize()
    assert torch.equal(grad, grad0), 'the reduce of the Adam launch gives the gradient of dmf_grad_reduce'
    g = grad0.cpu()
    th_ref, m_ref, v_ref = c['theta'].cpu().double(), m0.double(), v0.double()
    adam_step_ref(th_ref, g.double(), m_ref, v_ref, step, lr=c['lr'])
    what, p = tag(c, 'step %d' % step), 'adam %s' % kind(c)
    moved = (theta.cpu() != c['theta'].cpu()).float().mean().item()
    print('%s: %.0f %% of theta moved, largest update %.2e' % (what, 100 * moved, (th_ref - c['theta'].cpu().double()).abs().max().item()))
    close(p + ': theta', theta, th_ref, 1e-7, 1e-6, 'theta after the fused Adam ' + what)
    close(p + ': m', m, m_ref, 1e-7, 1e-6, 'exp_avg after the fused Adam ' + what)
    close(p + ': v', v, v_ref, 1e-7, 1e-6, 'exp_avg_sq after the fused Adam ' + what)
    # parameters of never-open units: m = v = g = 0, theta keeps every bit
    inside = flat_like(c, {k: torch.ones(shp) for k, (_, _, shp) in c['views'].items()}) == 1
    still = inside & (m0 == 0) & (v0 == 0) & (flat_like(c, c['grads']) == 0)
    o, n, shp = c['views']['fc1.weight']
    rows = int(still[o:o + n].view(shp).all(1).sum())
    assert rows >= 1, 'no fc1 unit with m = v = g = 0 %s' % what
    assert float(g[still].abs().max()) == 0.0, 'the kernel\'s gradient of a never-open unit is exactly zero ' + what
    assert torch.equal(theta.cpu()[still], c['theta'].cpu()[still]), 'theta of never-open units keeps every bit ' + what
    assert float(m.cpu()[still].abs().max()) == 0.0 and float(v.cpu()[still].abs().max()) == 0.0


# -------------------------------------------------------------------------------------------------------- 5. ten launches
def test_ten_launches_are_bit_equal():
    c = gpu_case('tiny1-sharp', 513)
    first = None
    for i in range(10):
        out = [t.cpu() for t in train_run(c, 'gather')]
        if first is None:
            first = out
        for x, y in zip(first, out):
            assert torch.equal(x, y), 'launch %d differs from the first' % i
    assert bool(torch.isfinite(first[3]).all())
