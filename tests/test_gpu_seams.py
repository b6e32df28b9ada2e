"""GPU: the seams of the two-launch train step — what the head wave stores per patch (patch kernel) and the reduce launch
whose geometry and ADAM state pointers travel in preloaded words — against the CPU oracle (oracle/gmfnet_ref.py).

Shapes: the compiled small instances 8/1/5/1/40/2 and 4/1/5/1/40/1 and the headline 200/1/11/1/40/10, all on a 23 x 19 scene in
gather mode.  Batches 1, 3, 256, 260, 600: one patch per workgroup, a tail workgroup (260 = 256 + 4), and three patches per
workgroup (the `it > 0` path past MAX_BLOCKS = 256, where a store moved in front of a value's last write would show).

Tolerances.  Logits <= 1e-5 and gradients <= 1e-5 + 1e-4 |ref| are tests/test_gpu_parity.py's.  The others follow from them:
  * per-patch loss = logsumexp(logits) - logits[label]: each term moves by at most the logit error, 2e-5 together, plus the
    fast exp / log of the kernel (absolute error ~1e-6 at these magnitudes): 2.2e-5;
  * one ADAM step from m = v = 0 with a gradient g' within t = 1e-5 + 1e-4 |g| of the oracle's g:
      m = (1 - b1) g           -> |dm| <= 0.1 t, plus 2^-20 |m| (the kernel forms 1 - b1 in fp32: 2^-22 relative, and roundings);
      v = (1 - b2) g^2         -> |dv| <= 0.001 (2 |g| t + t^2), plus 2e-5 v (0.999 as a float is 0.99900001287, so the
                                  kernel's fp32 1 - b2 is 1.3e-5 below 0.001; the bias correction carries the same factor);
      theta -= lr s(g), s(x) = x / (|x| + eps), monotone in x -> |dtheta| <= lr max(|s(g + t) - s(g)|, |s(g - t) - s(g)|)
                                  plus one ulp of theta and 16 ulp of lr for the two evaluation orders: 2^-22 (|theta| + 4 lr).
    (An element whose gradient is within t of zero may step the other way: the bound then is 2 lr, as it must be.)
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = {   # name: (C, C2, P, S, K)
    'tiny1': (8, 1, 5, 1, 5),        # 8/1/5/1/40/2
    'quatiny': (4, 1, 5, 1, 5),      # 4/1/5/1/40/1
    'hsi': (200, 1, 11, 1, 17),      # 200/1/11/1/40/10
}
BATCHES = (1, 3, 256, 260, 600)
CASES = [(n, B) for n in SHAPES for B in BATCHES]
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
H_SCENE, W_SCENE = 23, 19


def make_cfg(name):
    C, C2, P, S, K = SHAPES[name]
    return {'patch_size': P, 'Categories_Number': K, 'data_city': 's', 'DATA_DICT': {'s': {'size': [64, 64, C]}},
            'scale': S, 'aux_bands': C2, 'gmf': {'width': 40, 'hidden': 64, 'pool_sigma': 2.5, 'attention': 0}}


def gpu_step(hip, inp, labels, B, K, theta0):
    """train_fwd_bwd, then the reduce in its two modes: gradient only, and gradient + fused ADAM step 1 from m = v = 0."""
    from dmf import lib
    theta = theta0.clone()
    m, v = torch.zeros_like(theta), torch.zeros_like(theta)
    logits = torch.empty(B, K, device='cuda'); loss = torch.empty(B, device='cuda')
    ws = torch.zeros(lib.workspace_bytes(hip.shape, B) // 4, device='cuda')
    lib.train_fwd_bwd(hip.shape, inp, theta, hip.pool_w, labels, 1.0 / B, logits, loss, ws)
    grad_only = torch.empty_like(theta)
    lib.grad_reduce(hip.shape, B, ws, grad_only)
    grad = torch.empty_like(theta)
    lib.grad_reduce_adam(hip.shape, B, ws, theta, m, v, grad, LR, B1, B2, EPS, 1)
    torch.cuda.synchronize()
    return {k: t.cpu() for k, t in dict(logits=logits, loss=loss, grad_only=grad_only, grad=grad, theta=theta, m=m, v=v).items()}


@functools.lru_cache(maxsize=None)
def case(name, B):
    """Oracle (once per case) and two GPU runs on the same inputs."""
    from dmf import lib
    from model.gmfnet import PARAM_ORDER, Net as HipNet
    from oracle.gmfnet_ref import Net as RefNet
    C, C2, P, S, K = SHAPES[name]
    cfg = make_cfg(name)
    torch.manual_seed(0)
    ref = RefNet(cfg)
    with torch.no_grad():
        for p in ref.parameters():
            p.add_(0.05 * torch.randn_like(p))
    hip = HipNet(cfg)
    hip.load_state_dict(ref.state_dict())
    hip = hip.to('cuda:0')
    g = torch.Generator().manual_seed(100 + B)
    A = torch.rand(H_SCENE + P - 1, W_SCENE + P - 1, C, generator=g)
    Bm = torch.rand(S * (H_SCENE + P - 1), S * (W_SCENE + P - 1), C2, generator=g)
    xy = torch.stack([torch.randint(0, H_SCENE, (B,), generator=g), torch.randint(0, W_SCENE, (B,), generator=g)], 1).int()
    xy[0] = torch.tensor([H_SCENE - 1, W_SCENE - 1])
    t = torch.randint(0, K, (B,), generator=g)
    a = torch.stack([A[x:x + P, y:y + P, :].permute(2, 0, 1) for x, y in xy.tolist()])
    b = torch.stack([Bm[S * x:S * x + S * P, S * y:S * y + S * P, :].permute(2, 0, 1) for x, y in xy.tolist()])
    # ---- oracle: logits, per-patch loss, gradients, one torch.optim.Adam step on them
    theta_before = {k: p.detach().clone() for k, p in ref.named_parameters()}
    ref.zero_grad()
    want_logits = ref(a, b)
    want_loss = torch.nn.functional.cross_entropy(want_logits, t, reduction='none')
    want_loss.mean().backward()
    want_g = {k: p.grad.detach().clone() for k, p in ref.named_parameters()}
    torch.optim.Adam(ref.parameters(), lr=LR, betas=(B1, B2), eps=EPS).step()
    want_theta = {k: p.detach().clone() for k, p in ref.named_parameters()}
    # ---- the HIP path, twice
    Ad, Bd, xyd = A.cuda(), Bm.cuda(), xy.cuda()
    inp = lib.input_gather(hip.shape, Ad, Bd, xyd)
    theta0 = hip.flat_parameters().clone()
    labels = t.int().cuda()
    runs = [gpu_step(hip, inp, labels, B, K, theta0) for _ in range(2)]
    off = hip._offsets
    views = {k: (off[i], want_g[k].numel(), want_g[k].shape) for i, k in enumerate(PARAM_ORDER)}
    return dict(runs=runs, views=views, want_logits=want_logits.detach(), want_loss=want_loss.detach(), want_g=want_g,
                theta_before=theta_before, want_theta=want_theta, n_params=off[16])


def part(flat, c, k):
    o, n, shp = c['views'][k]
    return flat[o:o + n].view(shp)


def assert_close(got, want, tol, what):
    err = (got.double() - want.double()).abs()
    bad = err > tol
    print('%s: max abs err %.3e (max |ref| %.3e)' % (what, err.max().item(), want.abs().max().item()))
    assert not bad.any(), '%s: %d/%d out of tolerance, max abs err %.3e' % (what, int(bad.sum()), bad.numel(), err.max().item())


@pytest.mark.parametrize('name,B', CASES)
def test_step_matches_the_oracle(name, B):
    c = case(name, B)
    r = c['runs'][0]
    assert_close(r['logits'], c['want_logits'], 1e-5, 'logits [%s, B=%d]' % (name, B))
    assert abs(r['loss'].double().mean().item() - c['want_loss'].double().mean().item()) < 1e-5
    for k, want in c['want_g'].items():
        tol = 1e-5 + 1e-4 * want.double().abs()
        assert_close(part(r['grad_only'], c, k), want, tol, 'grad %s [%s, B=%d]' % (k, name, B))
    assert torch.equal(r['grad'], r['grad_only']), 'the fused-ADAM reduce and the gradient-only reduce must sum alike'


@pytest.mark.parametrize('name,B', CASES)
def test_fused_adam_step_matches_torch_adam_on_oracle_gradients(name, B):
    c = case(name, B)
    r = c['runs'][0]
    s = lambda x: x / (x.abs() + EPS)
    for k, g in c['want_g'].items():
        g = g.double()
        t = 1e-5 + 1e-4 * g.abs()
        th0, th1 = c['theta_before'][k].double(), c['want_theta'][k].double()
        tol_theta = LR * torch.maximum((s(g + t) - s(g)).abs(), (s(g - t) - s(g)).abs()) + 2.0 ** -22 * (th0.abs() + 4 * LR)
        assert_close(part(r['theta'], c, k), th1, tol_theta, 'theta %s [%s, B=%d]' % (k, name, B))
        m_want, v_want = (1 - B1) * g, (1 - B2) * g * g
        assert_close(part(r['m'], c, k), m_want, 0.1 * t + 2.0 ** -20 * m_want.abs(), 'm %s [%s, B=%d]' % (k, name, B))
        assert_close(part(r['v'], c, k), v_want, 0.001 * (2 * g.abs() * t + t * t) + 2e-5 * v_want, 'v %s [%s, B=%d]' % (k, name, B))


@pytest.mark.parametrize('name,B', CASES)
def test_two_runs_are_bit_equal(name, B):
    r0, r1 = case(name, B)['runs']
    for k in ('logits', 'loss', 'grad', 'grad_only', 'theta', 'm', 'v'):
        assert torch.equal(r0[k], r1[k]), k
    assert not torch.isnan(r0['theta']).any() and r0['theta'].numel() == case(name, B)['n_params']


@pytest.mark.parametrize('name,B', [(n, B) for n in SHAPES for B in (260, 600)])
def test_head_wave_outputs(name, B):
    """What the head wave stores per patch (logits, loss, and through the reduce the fc1 / fc2 gradients), with more than one
    patch per workgroup."""
    c = case(name, B)
    r = c['runs'][0]
    assert_close(r['logits'], c['want_logits'], 1e-5, 'logits [%s, B=%d]' % (name, B))
    assert_close(r['loss'], c['want_loss'], 2.2e-5, 'per-patch loss [%s, B=%d]' % (name, B))
    for k in ('fc1.weight', 'fc1.bias', 'fc2.weight', 'fc2.bias'):
        want = c['want_g'][k]
        assert_close(part(r['grad'], c, k), want, 1e-5 + 1e-4 * want.double().abs(), 'grad %s [%s, B=%d]' % (k, name, B))
