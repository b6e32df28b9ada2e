"""GPU: the head wave's tables in LDS, staged by LDS-DMA straight from theta (csrc/dmf_patch_v2.hip, head wavefront, first
patch of a workgroup, behind barrier W), against the CPU oracle (oracle/gmfnet_ref.py).

Two images are staged: fc2.weight as [K rounded up to 4][68] (16-byte pieces; a lane of a piece is masked where it would
fall into the 4 floats of row padding, into a row >= K or beyond the image; rows K .. K4 - 1 are zero rows written by plain
stores) and fc1.weight as the dz phase reads it, [16 row blocks][4 x 2F]: block jc holds fc1.weight[4 jc .. 4 jc + 3][i] in a
16-byte slot rotated by 4 (jc / 4) (4-byte pieces of 16 features x 4 rows; a block's first piece wraps around the row).
fc2's image feeds the logits and dh, the fc1 image feeds dz and through it EVERY conv gradient, so a misplaced element shows
in the logits or in the gradients of the conv layers.

Class counts, chosen for how the fc2 image falls on its 64-lane pieces (17 chunks per row):
   2  one piece, 34 of 64 lanes live, two zero rows
  15  255 chunks: the last lane of the last piece is beyond the image; one zero row
  17  the headline class count; 289 chunks, 33 live lanes in the fifth piece; three zero rows
  45  three zero rows behind 45 real ones (the zero rows multiply dl = 0 in the dh sums: they must BE zero)
  48  the largest class count the 200-band shape has LDS for (160 KiB): 816 chunks in 13 pieces, no zero row
  61, 64  the same two at KMAX, on the small shape: 17 full pieces at 64
Shapes: hsi 200/1/11 (2F = 80: five pieces per row block), hsi3 224/3/11 (2F = 64: four), tiny1 8/1/5 (five conv waves).
Batches 1 and 257: the second patch of a workgroup reuses the images of the first.

Tolerances are tests/test_gpu_seams.py's: logits <= 1e-5, per-patch loss <= 2.2e-5, gradients <= 1e-5 + 1e-4 |ref|.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = {   # name: (C, C2, P, width)
    'hsi': (200, 1, 11, 40),
    'hsi3': (224, 3, 11, 32),
    'tiny1': (8, 1, 5, 40),
}
CASES = [('hsi', 2, 1), ('hsi', 15, 1), ('hsi', 17, 1), ('hsi', 17, 257), ('hsi', 45, 257), ('hsi', 48, 1),
         ('hsi3', 15, 257), ('hsi3', 17, 1), ('tiny1', 2, 257), ('tiny1', 61, 1), ('tiny1', 64, 1)]
H_SCENE, W_SCENE = 23, 19


def make_cfg(name, K):
    C, C2, P, width = SHAPES[name]
    return {'patch_size': P, 'Categories_Number': K, 'data_city': 's', 'DATA_DICT': {'s': {'size': [64, 64, C]}},
            'scale': 1, 'aux_bands': C2, 'gmf': {'width': width, 'hidden': 64, 'pool_sigma': 2.5, 'attention': 0}}


@functools.lru_cache(maxsize=None)
def case(name, K, B):
    """The oracle's results (once per case) and the device inputs."""
    from dmf import lib
    from model.gmfnet import PARAM_ORDER, Net as HipNet
    from oracle.gmfnet_ref import Net as RefNet
    C, C2, P, width = SHAPES[name]
    cfg = make_cfg(name, K)
    torch.manual_seed(0)
    ref = RefNet(cfg)
    with torch.no_grad():
        for p in ref.parameters():
            p.add_(0.05 * torch.randn_like(p))
    hip = HipNet(cfg)
    hip.load_state_dict(ref.state_dict())
    hip = hip.to('cuda:0')
    g = torch.Generator().manual_seed(2000 + 7 * B + K)
    A = torch.rand(H_SCENE + P - 1, W_SCENE + P - 1, C, generator=g)
    Bm = torch.rand(H_SCENE + P - 1, W_SCENE + P - 1, C2, generator=g)
    xy = torch.stack([torch.randint(0, H_SCENE, (B,), generator=g), torch.randint(0, W_SCENE, (B,), generator=g)], 1).int()
    xy[0] = torch.tensor([H_SCENE - 1, W_SCENE - 1])
    t = torch.randint(0, K, (B,), generator=g)
    a = torch.stack([A[x:x + P, y:y + P, :].permute(2, 0, 1) for x, y in xy.tolist()]).contiguous()
    b = torch.stack([Bm[x:x + P, y:y + P, :].permute(2, 0, 1) for x, y in xy.tolist()]).contiguous()
    ref.zero_grad()
    want_logits = ref(a, b)
    want_logits.retain_grad()
    want_loss = torch.nn.functional.cross_entropy(want_logits, t, reduction='none')
    want_loss.mean().backward()
    want_g = {k: p.grad.detach().clone() for k, p in ref.named_parameters()}
    Ad, Bd, xyd = A.cuda(), Bm.cuda(), xy.cuda()
    inp = lib.input_gather(hip.shape, Ad, Bd, xyd)
    off = hip._offsets
    views = {k: (off[i], want_g[k].numel(), want_g[k].shape) for i, k in enumerate(PARAM_ORDER)}
    return dict(hip=hip, inp=inp, keep=(Ad, Bd, xyd), labels=t.int().cuda(), theta=hip.flat_parameters().clone(), B=B, K=K,
                views=views, want_logits=want_logits.detach(), want_loss=want_loss.detach(), want_g=want_g,
                want_dl=want_logits.grad.detach().clone())


def train_run(c, theta=None):
    from dmf import lib
    hip, B, K = c['hip'], c['B'], c['K']
    logits = torch.empty(B, K, device='cuda'); loss = torch.empty(B, device='cuda')
    ws = torch.zeros(lib.workspace_bytes(hip.shape, B) // 4, device='cuda')
    lib.train_fwd_bwd(hip.shape, c['inp'], c['theta'] if theta is None else theta, hip.pool_w, c['labels'], 1.0 / B, logits, loss, ws)
    grad = torch.empty_like(c['theta'])
    lib.grad_reduce(hip.shape, B, ws, grad)
    torch.cuda.synchronize()
    return dict(logits=logits.cpu(), loss=loss.cpu(), grad=grad.cpu())


def part(flat, c, k):
    o, n, shp = c['views'][k]
    return flat[o:o + n].view(shp)


def assert_close(got, want, tol, what):
    err = (got.double() - want.double()).abs()
    bad = ~(err <= tol)                      # (a NaN is out of tolerance)
    print('%s: max abs err %.3e (max |ref| %.3e)' % (what, err.max().item(), want.abs().max().item()))
    assert not bad.any(), '%s: %d/%d out of tolerance, max abs err %.3e' % (what, int(bad.sum()), bad.numel(), err.max().item())


def check_step(c, r, tag):
    assert_close(r['logits'], c['want_logits'], 1e-5, 'logits ' + tag)
    assert_close(r['loss'], c['want_loss'], 2.2e-5, 'per-patch loss ' + tag)
    for k, want in c['want_g'].items():
        assert_close(part(r['grad'], c, k), want, 1e-5 + 1e-4 * want.double().abs(), 'grad %s %s' % (k, tag))


@pytest.mark.parametrize('name,K,B', CASES)
def test_train_step(name, K, B):
    c = case(name, K, B)
    assert c['want_g']['spec_a.weight'].abs().max().item() > 1e-4, 'no gradient reaches the conv layers: dz would not be tested'
    check_step(c, train_run(c), '[%s, K=%d, B=%d]' % (name, K, B))


@pytest.mark.parametrize('name,K,B', CASES)
def test_eval_forward(name, K, B):
    """MODE_FWD stages the fc2 image only (another LDS map: no slab copies, no fc1 image)."""
    from dmf import lib
    c = case(name, K, B)
    hip = c['hip']
    logits = torch.empty(B, K, device='cuda'); pred = torch.empty(B, dtype=torch.int32, device='cuda')
    lib.forward(hip.shape, c['inp'], c['theta'], hip.pool_w, logits, pred)
    torch.cuda.synchronize()
    assert_close(logits.cpu(), c['want_logits'], 1e-5, 'eval logits [%s, K=%d, B=%d]' % (name, K, B))
    assert torch.equal(pred.cpu().long(), logits.cpu().argmax(1)), 'pred is the argmax of the returned logits'


@pytest.mark.parametrize('name,K,B', [('hsi', 15, 1), ('hsi', 45, 257), ('hsi3', 15, 257)])
def test_backward_from_supplied_dlogits(name, K, B):
    """MODE_BWD: both images, dl from the caller."""
    from dmf import lib
    c = case(name, K, B)
    hip = c['hip']
    ws = torch.zeros(lib.workspace_bytes(hip.shape, B) // 4, device='cuda')
    lib.backward_dlogits(hip.shape, c['inp'], c['theta'], hip.pool_w, c['want_dl'].contiguous().cuda(), ws)
    grad = torch.empty_like(c['theta'])
    lib.grad_reduce(hip.shape, B, ws, grad)
    torch.cuda.synchronize()
    for k, want in c['want_g'].items():
        assert_close(part(grad.cpu(), c, k), want, 1e-5 + 1e-4 * want.double().abs(), 'grad %s [%s, K=%d, B=%d, from dlogits]' % (k, name, K, B))


@pytest.mark.parametrize('name,K,B', [('hsi', 15, 1), ('hsi', 45, 257)])
def test_unit_gradient_step(name, K, B):
    """MODE_UNIT stages the fc2 image only, in the training LDS map; dz is formed by the second launch."""
    from dmf import lib
    c = case(name, K, B)
    hip = c['hip']
    logits = torch.empty(B, K, device='cuda')
    ws = torch.zeros(lib.workspace_bytes(hip.shape, B) // 4, device='cuda')
    lib.forward_unit(hip.shape, c['inp'], c['theta'], hip.pool_w, logits, ws)
    lib.backward_unit(hip.shape, B, c['theta'], c['want_dl'].contiguous().cuda(), ws)
    grad = torch.empty_like(c['theta'])
    lib.grad_reduce(hip.shape, B, ws, grad)
    torch.cuda.synchronize()
    tag = '[%s, K=%d, B=%d, unit]' % (name, K, B)
    assert_close(logits.cpu(), c['want_logits'], 1e-5, 'logits ' + tag)
    for k, want in c['want_g'].items():
        assert_close(part(grad.cpu(), c, k), want, 1e-5 + 1e-4 * want.double().abs(), 'grad %s %s' % (k, tag))


@pytest.mark.parametrize('name,K', [('hsi', 45), ('tiny1', 61)])
def test_zero_rows_after_a_launch_that_left_infinities_there(name, K):
    """The fc2 image of K = 45 (61) has three zero rows which the dh sums multiply with dl = 0.  The launch before it runs the
    same shape with K + 3 classes and fc2.weight rows K .. K + 2 = +inf, so that — where a workgroup inherits the LDS contents
    of its predecessor on the compute unit — those rows hold infinities until they are written: inf x 0 is a NaN in dh, and
    with it in every gradient."""
    dirty, c = case(name, K + 3, 257), case(name, K, 257)
    th = dirty['theta'].clone()
    o, n, shp = dirty['views']['fc2.weight']
    th[o:o + n].view(shp)[K:] = float('inf')
    train_run(dirty, th)
    r = train_run(c)
    assert torch.isfinite(r['grad']).all()
    check_step(c, r, '[%s, K=%d behind K=%d with infinite rows]' % (name, K, K + 3))


@pytest.mark.parametrize('name,K', [('hsi', 17), ('hsi3', 15)])
def test_ten_launches_are_bit_equal(name, K):
    c = case(name, K, 257)
    first = train_run(c)
    assert first['grad'].abs().sum() > 0
    for i in range(9):
        r = train_run(c)
        for k in ('logits', 'loss', 'grad'):
            assert torch.equal(r[k], first[k]), '%s of launch %d' % (k, i + 2)
