"""GPU: the exit of the patch kernel's train pass — from barrier 2 to the last wave's end — against the CPU oracle
(oracle/gmfnet_ref.py): the dz phase, which reads the transposed fc1.weight image in LDS with its 16-byte chunks rotated per row,
the scaled copy-out of the slab row, the head vectors z / h / dh / dl the head wave leaves in the workspace, and the head wave's
argument words (loss scale, scaler state, workspace and step-count pointers), which are in registers before the exit begins.

Shapes (23 x 19 scene, gather mode), chosen for their wave counts and for how the slab pieces fall on the threads:
  pan16  4/1/16/1/40/1    ten conv waves + head, 16-lane rows, 272 slab pieces on 704 threads
  hsi3   224/3/11/1/32/8  2F = 64 (the z vector ends with the head wave's first 64 lanes; 64 rows of the fc1 image), 424 pieces
  hsi    200/1/11/1/40/10 the headline shape, 2F = 80, 432 pieces on 576 threads
  tiny1  8/1/5/1/40/2     five conv waves, 272 pieces on 384 threads (K = 2 and 64 only)
Batches 1, 255, 257, 600: one patch per workgroup, a workgroup count below MAX_BLOCKS = 256, a tail workgroup with a second
patch, and up to three patches per workgroup (the `it > 0` path: the slab row accumulates, the head vectors of every patch go to
their own workspace rows).

Tolerances are tests/test_gpu_seams.py's: logits <= 1e-5, per-patch loss <= 2.2e-5 (two logit errors + the fast exp / log),
gradients <= 1e-5 + 1e-4 |ref|.  The workspace's head vectors are compared at the gradient tolerance: z and h are forward values
formed like the logits' inputs, dh and dl are gradients (dl = dL/dlogits, dh = dL/d(fc1 output) of the batch-mean loss).
A loss-scaler state of 2^k scales dl, and with it every gradient, exactly: compared bit for bit after dividing.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = {   # name: (C, C2, P, S, width, K)
    'pan16': (4, 1, 16, 1, 40, 12),      # 4/1/16/1/40/1
    'hsi3': (224, 3, 11, 1, 32, 17),     # 224/3/11/1/32/8
    'hsi': (200, 1, 11, 1, 40, 17),      # 200/1/11/1/40/10
    'tiny1': (8, 1, 5, 1, 40, 5),        # 8/1/5/1/40/2
}
BATCHES = (1, 255, 257, 600)
CASES = [(n, B) for n in ('pan16', 'hsi3', 'hsi') for B in BATCHES]
K_ENDS = [(n, K) for n in ('pan16', 'tiny1') for K in (2, 64)]      # KMAX = 64; batch 3
H_SCENE, W_SCENE = 23, 19
KMAX, MAX_BLOCKS = 64, 256


def make_cfg(name, K):
    C, C2, P, S, width, _ = SHAPES[name]
    return {'patch_size': P, 'Categories_Number': K, 'data_city': 's', 'DATA_DICT': {'s': {'size': [64, 64, C]}},
            'scale': S, 'aux_bands': C2, 'gmf': {'width': width, 'hidden': 64, 'pool_sigma': 2.5, 'attention': 0}}


def strip_major(flat, B, W):
    """[W/8 strips][B][8] (csrc/dmf_shapes.h: hv_index) -> [B][W]"""
    return flat.view(W // 8, B, 8).permute(1, 0, 2).reshape(B, W)


def split_ws(ws, slab, B, F2, H):
    """the regions of the workspace (csrc/dmf_shapes.h: make_ws): slab rows, then z, h, dh, dl"""
    o = MAX_BLOCKS * slab
    out = {}
    for k, W in (('z', F2), ('h', H), ('dh', H), ('dl', KMAX)):
        out[k] = strip_major(ws[o:o + B * W], B, W)
        o += B * W
    return out


def train_run(hip, inp, labels, B, K, theta, scaler=None):
    from dmf import lib
    logits = torch.empty(B, K, device='cuda'); loss = torch.empty(B, device='cuda')
    ws = torch.zeros(lib.workspace_bytes(hip.shape, B) // 4, device='cuda')
    lib.train_fwd_bwd(hip.shape, inp, theta, hip.pool_w, labels, 1.0 / B, logits, loss, ws, scaler_state=scaler)
    grad = torch.empty_like(theta)
    lib.grad_reduce(hip.shape, B, ws, grad)
    torch.cuda.synchronize()
    return dict(logits=logits.cpu(), loss=loss.cpu(), ws=ws.cpu(), grad=grad.cpu())


@functools.lru_cache(maxsize=None)
def case(name, B, K=None):
    """Oracle with its intermediates (once per case) and the inputs of the GPU runs."""
    from dmf import lib
    from model.gmfnet import PARAM_ORDER, Net as HipNet
    from oracle.gmfnet_ref import Net as RefNet
    C, C2, P, S, width, K0 = SHAPES[name]
    K = K or K0
    cfg = make_cfg(name, K)
    torch.manual_seed(0)
    ref = RefNet(cfg)
    with torch.no_grad():
        for p in ref.parameters():
            p.add_(0.05 * torch.randn_like(p))
    hip = HipNet(cfg)
    hip.load_state_dict(ref.state_dict())
    hip = hip.to('cuda:0')
    g = torch.Generator().manual_seed(1000 + 7 * B + K)
    A = torch.rand(H_SCENE + P - 1, W_SCENE + P - 1, C, generator=g)
    Bm = torch.rand(S * (H_SCENE + P - 1), S * (W_SCENE + P - 1), C2, generator=g)
    xy = torch.stack([torch.randint(0, H_SCENE, (B,), generator=g), torch.randint(0, W_SCENE, (B,), generator=g)], 1).int()
    xy[0] = torch.tensor([H_SCENE - 1, W_SCENE - 1])
    t = torch.randint(0, K, (B,), generator=g)
    a = torch.stack([A[x:x + P, y:y + P, :].permute(2, 0, 1) for x, y in xy.tolist()])
    b = torch.stack([Bm[S * x:S * x + S * P, S * y:S * y + S * P, :].permute(2, 0, 1) for x, y in xy.tolist()])
    # ---- oracle, piece by piece: the intermediates the kernel leaves in the workspace keep their gradients
    ref.zero_grad()
    z = ref.pooled(*ref.branches(a, b))
    pre = ref.fc1(z); pre.retain_grad()
    h = torch.relu(pre)
    want_logits = ref.fc2(h); want_logits.retain_grad()
    want_loss = torch.nn.functional.cross_entropy(want_logits, t, reduction='none')
    want_loss.mean().backward()
    want_g = {k: p.grad.detach().clone() for k, p in ref.named_parameters()}
    dl = torch.zeros(B, KMAX); dl[:, :K] = want_logits.grad
    want_hv = dict(z=z.detach(), h=h.detach(), dh=pre.grad.detach().clone(), dl=dl)
    Ad, Bd, xyd = A.cuda(), Bm.cuda(), xy.cuda()
    inp = lib.input_gather(hip.shape, Ad, Bd, xyd)
    off = hip._offsets
    views = {k: (off[i], want_g[k].numel(), want_g[k].shape) for i, k in enumerate(PARAM_ORDER)}
    slab = (off[8] + 31) & ~31
    return dict(hip=hip, inp=inp, keep=(Ad, Bd, xyd), labels=t.int().cuda(), theta=hip.flat_parameters().clone(), B=B, K=K,
                F2=2 * width, slab=slab, views=views, want_logits=want_logits.detach(), want_loss=want_loss.detach(),
                want_g=want_g, want_hv=want_hv)


@functools.lru_cache(maxsize=None)
def plain_run(name, B, K=None):
    c = case(name, B, K)
    return train_run(c['hip'], c['inp'], c['labels'], c['B'], c['K'], c['theta'])


def part(flat, c, k):
    o, n, shp = c['views'][k]
    return flat[o:o + n].view(shp)


def assert_close(got, want, tol, what):
    err = (got.double() - want.double()).abs()
    bad = err > tol
    print('%s: max abs err %.3e (max |ref| %.3e)' % (what, err.max().item(), want.abs().max().item()))
    assert not bad.any(), '%s: %d/%d out of tolerance, max abs err %.3e' % (what, int(bad.sum()), bad.numel(), err.max().item())


def check_against_oracle(c, r, tag):
    assert_close(r['logits'], c['want_logits'], 1e-5, 'logits ' + tag)
    assert_close(r['loss'], c['want_loss'], 2.2e-5, 'per-patch loss ' + tag)
    for k, want in c['want_g'].items():
        assert_close(part(r['grad'], c, k), want, 1e-5 + 1e-4 * want.double().abs(), 'grad %s %s' % (k, tag))


def check_head_vectors(c, ws, tag, keys=('z', 'h', 'dh', 'dl')):
    got = split_ws(ws, c['slab'], c['B'], c['F2'], 64)
    for k in keys:
        want = c['want_hv'][k]
        assert_close(got[k], want, 1e-5 + 1e-4 * want.double().abs(), 'workspace %s %s' % (k, tag))


@pytest.mark.parametrize('name,B', CASES)
def test_step_and_head_vectors_match_the_oracle(name, B):
    c = case(name, B)
    r = plain_run(name, B)
    tag = '[%s, B=%d]' % (name, B)
    check_against_oracle(c, r, tag)
    check_head_vectors(c, r['ws'], tag)


@pytest.mark.parametrize('name,K', K_ENDS)
def test_class_count_at_both_ends(name, K):
    c = case(name, 3, K)
    r = plain_run(name, 3, K)
    tag = '[%s, B=3, K=%d]' % (name, K)
    check_against_oracle(c, r, tag)
    check_head_vectors(c, r['ws'], tag)


@pytest.mark.parametrize('name,B', [(n, B) for n in ('pan16', 'hsi3', 'hsi') for B in (257, 600)])
@pytest.mark.parametrize('scale', [1.0, 1024.0])
def test_scaler_state_scales_the_gradients_exactly(name, B, scale):
    """dmf_train_fwd_bwd_scaled: dl is multiplied by loss_scale x state[0]; a power of two moves exponents only."""
    from dmf import lib
    c = case(name, B)
    r0 = plain_run(name, B)
    state = torch.zeros(lib.SCALER_FLOATS, device='cuda')
    lib.scaler_init(state, scale)
    r = train_run(c['hip'], c['inp'], c['labels'], B, c['K'], c['theta'], scaler=state)
    assert torch.equal(r['logits'], r0['logits']) and torch.equal(r['loss'], r0['loss'])
    assert torch.equal(r['grad'] / scale, r0['grad']), 'gradients of the scaled run / %g' % scale
    s0, s1 = split_ws(r0['ws'], c['slab'], B, c['F2'], 64), split_ws(r['ws'], c['slab'], B, c['F2'], 64)
    for k in ('z', 'h'):
        assert torch.equal(s1[k], s0[k]), k
    for k in ('dh', 'dl'):
        assert torch.equal(s1[k] / scale, s0[k]), k


@pytest.mark.parametrize('name,B', [(n, B) for n in ('pan16', 'hsi3', 'hsi') for B in (255, 600)])
def test_backward_from_supplied_dlogits(name, B):
    """MODE_BWD: no labels, no loss; dL/dlogits comes from the caller (here: the oracle's, of the batch-mean loss)."""
    from dmf import lib
    c = case(name, B)
    hip, K = c['hip'], c['K']
    dlogits = c['want_hv']['dl'][:, :K].contiguous().cuda()
    ws = torch.zeros(lib.workspace_bytes(hip.shape, B) // 4, device='cuda')
    lib.backward_dlogits(hip.shape, c['inp'], c['theta'], hip.pool_w, dlogits, ws)
    grad = torch.empty_like(c['theta'])
    lib.grad_reduce(hip.shape, B, ws, grad)
    torch.cuda.synchronize()
    tag = '[%s, B=%d, from dlogits]' % (name, B)
    for k, want in c['want_g'].items():
        assert_close(part(grad.cpu(), c, k), want, 1e-5 + 1e-4 * want.double().abs(), 'grad %s %s' % (k, tag))
    check_head_vectors(c, ws.cpu(), tag)
    got_dl = split_ws(ws.cpu(), c['slab'], B, c['F2'], 64)['dl']
    assert torch.equal(got_dl, c['want_hv']['dl']), 'dl is passed through as supplied'


@pytest.mark.parametrize('name,B', [(n, B) for n in ('pan16', 'hsi3', 'hsi') for B in (256, 600)])
def test_ten_launches_are_bit_equal(name, B):
    """Logits, loss and the WHOLE workspace (slab rows, head vectors; the rest stays zero) of ten launches on the same inputs."""
    c = case(name, B)
    first = train_run(c['hip'], c['inp'], c['labels'], B, c['K'], c['theta'])
    assert first['ws'][:MAX_BLOCKS * c['slab']].abs().sum() > 0
    for i in range(9):
        r = train_run(c['hip'], c['inp'], c['labels'], B, c['K'], c['theta'])
        for k in ('logits', 'loss', 'ws', 'grad'):
            assert torch.equal(r[k], first[k]), '%s of launch %d' % (k, i + 2)
