"""GPU: the column pipeline of the patch kernel's primary branch against the CPU oracle (oracle/gmfnet_ref.py).

Behind barrier W a conv wave runs spec_a and the depthwise rows of spat_a ONE WINDOW COLUMN AT A TIME (csrc/dmf_patch_v2.hip):
the reads of a later column are in flight while the conv step of the current one runs; behind barrier 1 the conv backward
step of a column runs between the reads of the column and the weight-gradient FMAs that consume them.  Only the order of a
lane's instructions differs from the phase-by-phase form, so every result is held to the tolerances the project already
uses for these quantities.

Shapes (23 x 19 scene, gather mode), chosen for the pipeline's edges:
  tiny1  8/1/5/1/40/2      P = 5, one 16-byte read per column: the first and last columns are most of the loop
  hsi7   200/1/7/1/40/10
  hsi    200/1/11/1/40/10  the headline shape, five reads per column
  hsi3   224/3/11/1/32/8   seven reads per column, the largest batch of reads in flight
  pan16  4/1/16/1/40/1     16-lane rows (row shifts), P = 16, one read per column
Batches 1 and 257: 257 gives one workgroup a second patch (the `it > 0` path: the slab row accumulates).

Tolerances: logits <= 1e-5, per-patch loss <= 2.2e-5, gradients <= 1e-5 + 1e-4 |ref| (tests/test_gpu_seams.py); the attention
step 2e-4 for logits and 2e-5 + 2e-3 |ref| for gradients (tests/test_gpu_parity.py); the fp16 scene as the fp32 one
(tests/test_gpu_half.py: the operands are the same fp16 values on both sides).
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = {   # name: (C, C2, P, width, K)
    'tiny1': (8, 1, 5, 40, 5),
    'hsi7': (200, 1, 7, 40, 17),
    'hsi': (200, 1, 11, 40, 17),
    'hsi3': (224, 3, 11, 32, 17),
    'pan16': (4, 1, 16, 40, 12),
}
NAMES = tuple(SHAPES)
HALF = ('tiny1', 'hsi', 'hsi3', 'pan16')   # the rows above that have an fp16-scene kernel (DMF_V2_HALF_SHAPES)
BATCHES = (1, 257)
H_SCENE, W_SCENE = 23, 19


def make_cfg(name, half=0, attention=0, sigma=2.5):
    C, C2, P, width, K = SHAPES[name]
    cfg = {'patch_size': P, 'Categories_Number': K, 'data_city': 's', 'DATA_DICT': {'s': {'size': [64, 64, C]}},
           'scale': 1, 'aux_bands': C2, 'gmf': {'width': width, 'hidden': 64, 'pool_sigma': sigma, 'attention': attention}}
    if half:
        cfg['gmf']['half'] = 1
    if attention:
        cfg['trans'] = {'embed_dim': 96, 'num_head': 3}
    return cfg


@functools.lru_cache(maxsize=None)
def nets(name, half=0, attention=0, sigma=2.5):
    from model.gmfnet import Net as HipNet
    from oracle.gmfnet_ref import Net as RefNet
    cfg = make_cfg(name, half, attention, sigma)
    torch.manual_seed(0)
    ref = RefNet(cfg)
    with torch.no_grad():
        for k, p in ref.named_parameters():
            p.add_(0.05 * torch.randn_like(p))
            if k.startswith('attn_'):
                p.mul_(3.0)
    hip = HipNet(cfg)
    hip.load_state_dict(ref.state_dict())
    return ref, hip.to('cuda:0')


def cut(A, Bm, xy, P):
    a = torch.stack([A[x:x + P, y:y + P, :].permute(2, 0, 1) for x, y in xy.tolist()]).contiguous()
    b = torch.stack([Bm[x:x + P, y:y + P, :].permute(2, 0, 1) for x, y in xy.tolist()]).contiguous()
    return a, b


def make_inputs(name, B, half=0, column=None):
    """Scene, coordinates, labels.  column: the primary scene is zero except in window column `column` of patch 0 (whose
    window then has exactly one non-zero column; the other patches see zeros or a part of that column)."""
    C, C2, P, width, K = SHAPES[name]
    g = torch.Generator().manual_seed(1000 + 7 * B + (0 if column is None else 31 * (column + 1)))
    A = torch.rand(H_SCENE + P - 1, W_SCENE + P - 1, C, generator=g)
    if half:
        A = A - 0.3
    Bm = torch.rand(H_SCENE + P - 1, W_SCENE + P - 1, C2, generator=g)
    xy = torch.stack([torch.randint(0, H_SCENE, (B,), generator=g), torch.randint(0, W_SCENE, (B,), generator=g)], 1).int()
    xy[0] = torch.tensor([H_SCENE - 1, W_SCENE - 1])
    if column is not None:
        x0, y0 = xy[0].tolist()
        keep = 4.0 * (A[x0:x0 + P, y0 + column, :].clone() + 0.5)
        A.zero_()
        A[x0:x0 + P, y0 + column, :] = keep
    t = torch.randint(0, K, (B,), generator=g)
    return A, Bm, xy, t


@functools.lru_cache(maxsize=None)
def case(name, B, half=0, column=None, sigma=2.5):
    """The oracle's results (once per case) and the device inputs."""
    from dmf import lib
    from model.gmfnet import PARAM_ORDER
    C, C2, P, width, K = SHAPES[name]
    ref, hip = nets(name, half, 0, sigma)
    A, Bm, xy, t = make_inputs(name, B, half, column)
    a, b = cut(A, Bm, xy, P)
    ref.zero_grad()
    want_logits = ref(a, b)
    want_logits.retain_grad()
    want_loss = torch.nn.functional.cross_entropy(want_logits, t, reduction='none')
    want_loss.mean().backward()
    want_g = {k: p.grad.detach().clone() for k, p in ref.named_parameters()}
    Ad = A.cuda().to(torch.float16) if half else A.cuda()
    Bd, xyd = Bm.cuda(), xy.cuda()
    inp = lib.input_gather(hip.shape, Ad, Bd, xyd)
    off = hip._offsets
    views = {k: (off[i], want_g[k].numel(), want_g[k].shape) for i, k in enumerate(PARAM_ORDER)}
    return dict(hip=hip, inp=inp, keep=(Ad, Bd, xyd), labels=t.int().cuda(), theta=hip.flat_parameters().clone(), B=B, K=K,
                views=views, want_logits=want_logits.detach(), want_loss=want_loss.detach(), want_g=want_g,
                want_dl=want_logits.grad.detach().clone())


def train_run(c):
    from dmf import lib
    hip, B, K = c['hip'], c['B'], c['K']
    logits = torch.empty(B, K, device='cuda'); loss = torch.empty(B, device='cuda')
    ws = torch.zeros(lib.workspace_bytes(hip.shape, B) // 4, device='cuda')
    lib.train_fwd_bwd(hip.shape, c['inp'], c['theta'], hip.pool_w, c['labels'], 1.0 / B, logits, loss, ws)
    grad = torch.empty_like(c['theta'])
    lib.grad_reduce(hip.shape, B, ws, grad)
    torch.cuda.synchronize()
    return dict(logits=logits.cpu(), loss=loss.cpu(), grad=grad.cpu())


def part(flat, c, k):
    o, n, shp = c['views'][k]
    return flat[o:o + n].view(shp)


def assert_close(got, want, tol, what):
    err = (got.double() - want.double()).abs()
    bad = err > tol
    print('%s: max abs err %.3e (max |ref| %.3e)' % (what, err.max().item(), want.abs().max().item()))
    assert not bad.any(), '%s: %d/%d out of tolerance, max abs err %.3e' % (what, int(bad.sum()), bad.numel(), err.max().item())


def check_grads(c, grad, tag, keys=None):
    for k, want in c['want_g'].items():
        if keys is None or k in keys:
            assert_close(part(grad, c, k), want, 1e-5 + 1e-4 * want.double().abs(), 'grad %s %s' % (k, tag))


@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('name', NAMES)
def test_train_step(name, B):
    c = case(name, B)
    r = train_run(c)
    tag = '[%s, B=%d]' % (name, B)
    assert_close(r['logits'], c['want_logits'], 1e-5, 'logits ' + tag)
    assert_close(r['loss'], c['want_loss'], 2.2e-5, 'per-patch loss ' + tag)
    check_grads(c, r['grad'], tag)


@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('name', NAMES)
def test_eval_forward(name, B):
    from dmf import lib
    c = case(name, B)
    hip = c['hip']
    logits = torch.empty(B, c['K'], device='cuda'); pred = torch.empty(B, dtype=torch.int32, device='cuda')
    lib.forward(hip.shape, c['inp'], c['theta'], hip.pool_w, logits, pred)
    torch.cuda.synchronize()
    assert_close(logits.cpu(), c['want_logits'], 1e-5, 'eval logits [%s, B=%d]' % (name, B))


@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('name', NAMES)
def test_backward_from_supplied_dlogits(name, B):
    """MODE_BWD: dL/dlogits comes from the caller (here: the oracle's, of the batch-mean loss)."""
    from dmf import lib
    c = case(name, B)
    hip = c['hip']
    ws = torch.zeros(lib.workspace_bytes(hip.shape, B) // 4, device='cuda')
    lib.backward_dlogits(hip.shape, c['inp'], c['theta'], hip.pool_w, c['want_dl'].contiguous().cuda(), ws)
    grad = torch.empty_like(c['theta'])
    lib.grad_reduce(hip.shape, B, ws, grad)
    torch.cuda.synchronize()
    check_grads(c, grad.cpu(), '[%s, B=%d, from dlogits]' % (name, B))


@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('name', ['pan16', 'hsi'])
def test_unit_gradient_step(name, B):
    """MODE_UNIT: forward + per-patch unit gradients, then the backward launch scales them by the caller's dlogits.  pan16 is
    a 16-row instance (column loop in the forward, phase-by-phase backward), hsi takes the column loop in both."""
    from dmf import lib
    c = case(name, B)
    hip = c['hip']
    logits = torch.empty(B, c['K'], device='cuda')
    ws = torch.zeros(lib.workspace_bytes(hip.shape, B) // 4, device='cuda')
    lib.forward_unit(hip.shape, c['inp'], c['theta'], hip.pool_w, logits, ws)
    lib.backward_unit(hip.shape, B, c['theta'], c['want_dl'].contiguous().cuda(), ws)
    grad = torch.empty_like(c['theta'])
    lib.grad_reduce(hip.shape, B, ws, grad)
    torch.cuda.synchronize()
    tag = '[%s, B=%d, unit]' % (name, B)
    assert_close(logits.cpu(), c['want_logits'], 1e-5, 'logits ' + tag)
    check_grads(c, grad.cpu(), tag)


@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('name', HALF)
def test_half_scene_train_step(name, B):
    """fp16 scene: v_dot2 forward, v_fma_mix weight gradient, through the same column loops."""
    c = case(name, B, 1)
    assert c['inp'].half == 1
    r = train_run(c)
    tag = '[%s, B=%d, fp16 scene]' % (name, B)
    assert_close(r['logits'], c['want_logits'], 1e-5, 'logits ' + tag)
    assert abs(r['loss'].mean().item() - c['want_loss'].mean().item()) < 1e-5
    check_grads(c, r['grad'], tag)


def test_attention_train_step():
    """MODE_TOKENS (the feature maps leave the forward column loop) + MODE_DENSE (the backward column loop from dense dL/dY2
    maps): the attention network's train step on tiny1, batch 3."""
    from dmf import lib
    name, B = 'tiny1', 3
    C, C2, P, width, K = SHAPES[name]
    ref, hip = nets(name, 0, 1)
    A, Bm, xy, t = make_inputs(name, B)
    a, b = cut(A, Bm, xy, P)
    ref.zero_grad()
    want_logits = ref(a, b)
    loss = torch.nn.functional.cross_entropy(want_logits, t)
    loss.backward()
    Ad, Bd, xyd = A.cuda(), Bm.cuda(), xy.cuda()
    inp = lib.input_gather(hip.shape, Ad, Bd, xyd)
    theta = hip.flat_parameters()
    logits = torch.empty(B, K, device='cuda'); lossv = torch.empty(B, device='cuda')
    ws = torch.zeros(lib.workspace_bytes(hip.shape, B) // 4, device='cuda')
    aws = torch.empty(lib.attn_train_workspace_bytes(hip.shape, B), dtype=torch.uint8, device='cuda')
    lib.train_attn_fwd_bwd(hip.shape, inp, theta, hip.pool_w, t.int().cuda(), None, 1.0 / B, logits, lossv, ws, aws)
    grad = torch.empty_like(theta)
    lib.grad_reduce(hip.shape, B, ws, grad)
    torch.cuda.synchronize()
    assert_close(logits.cpu(), want_logits.detach(), 2e-4, 'attention logits')
    off = hip._offsets
    wants = dict(ref.named_parameters())
    for i, (k, p) in enumerate(zip(hip._order(), hip._named())):
        want = wants[k].grad
        got = grad[off[i]:off[i] + p.numel()].view(p.shape).cpu()
        assert_close(got, want, 2e-5 + 2e-3 * want.double().abs(), 'attention grad %s' % k)


@pytest.mark.parametrize('name', NAMES)
def test_ten_launches_are_bit_equal(name):
    c = case(name, 257)
    first = train_run(c)
    assert first['grad'].abs().sum() > 0
    for i in range(9):
        r = train_run(c)
        for k in ('logits', 'loss', 'grad'):
            assert torch.equal(r[k], first[k]), '%s of launch %d' % (k, i + 2)


@pytest.mark.parametrize('sigma', [0.0, 2.5])
@pytest.mark.parametrize('name', NAMES)
def test_window_with_a_single_nonzero_column(name, sigma):
    """The window of patch 0 is zero except in ONE column; the aux branch sees a full random scene, so both branches are
    active.  A column's contribution to the gradient of spec_a.weight (and, through y1, to the logits) stands alone here: an
    off-by-one column in either loop cannot hide in a sum over columns.  (The column's values are in [2, 6): the gradient is
    linear in them, the tolerance is not.)

    sigma = 0: a FLAT pooling profile (the uniform mean of oracle.gmfnet_ref.anchor_pool_weights), columns 0, 1 and P - 1:
    every column weighs the same, so the last column — the forward's epilogue step, the last request / consume pair, the
    backward columns that hold the quad sums — carries as much gradient as the first.  sigma = 2.5: the anchor profile the
    other tests use, columns 0 and 1 only: it decays along the row (column P - 1 weighs 3e-4 of column 0 at P = 11, 1e-8 at
    P = 16), so a lost last column would pass there.  Every tested column's reference gradient must be 100 x the absolute
    tolerance or more."""
    P = SHAPES[name][2]
    for col in ((0, 1, P - 1) if sigma == 0.0 else (0, 1)):
        c = case(name, 1, 0, col, sigma)
        r = train_run(c)
        tag = '[%s, sigma %g, column %d only]' % (name, sigma, col)
        want = c['want_g']['spec_a.weight']
        print('%s: max |ref grad spec_a.weight| %.3e' % (tag, want.abs().max().item()))
        assert want.abs().max().item() >= 1e-3, 'the column carries too little gradient: the test would prove nothing'
        assert c['want_g']['spat_b.weight'].abs().max().item() > 1e-6, 'aux branch inactive'
        assert_close(r['logits'], c['want_logits'], 1e-5, 'logits ' + tag)
        check_grads(c, r['grad'], tag, keys=('spec_a.weight',))
