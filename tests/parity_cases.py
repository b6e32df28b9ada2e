"""Parity cases whose argmax means something: shared by tests/test_gpu_batch_walk.py (GPU) and tests/test_parity_cases_host.py
(the guards below, on the oracle alone).  A plain module: no fixtures, no GPU, nothing of the HIP library.

On the usual test inputs (seed-0 net with 0.05 noise, torch.rand scene) the oracle puts nearly every patch into ONE class: the
logits of two patches differ by ~1e-3 while the classes' biases differ by ~1e-1.  `pred == argmax` then passes for a kernel that
writes a constant.  A case here keeps that recipe and CENTRES THE HEAD: fc2.bias -= mean over the case's own batch of the
oracle's logits, on the CPU, before anything reaches the HIP net.  The logits' spread over the patches stays what it was (so the
project's absolute tolerances mean what they meant; fc2.weight is not scaled), but now it decides the class.

A case:
  nets         tests/test_gpu_parity.py::nets / test_gpu_half.py::half_nets / test_gpu_parity.py::_attn_nets (seed 0, 0.05 noise,
               attention factor 3), the oracle half of them, then the centring
  scene        37 x 41 pixels, padded to (37 + P - 1) x (41 + P - 1); torch.rand, or test_gpu_half.scene's recipe for half
  coordinates  the first B of a seeded permutation of the 1,517 pixels (no two patches alike), (0, 0) and (H-1, W-1) swapped
               into positions 0 and 1
  labels       uniform, 0 and K-1 forced into positions 0 and 1
and the oracle's logits, per-patch loss, gradients of the batch-mean loss and the head intermediates z / h / dh / dl.

Guards, asserted by `case` on the oracle alone (a case that misses one gets another seed in SEEDS; the guards stay):
  1. class diversity   at least min(K, 4) classes are each predicted for at least 2 % of the batch
  2. pair separation   patches b and b + 256 k (one workgroup's patches) differ by >= 2e-4 in some logit: 20 x the logit tolerance
  3. margin cap        at most 15 % of the patches have a top-2 margin <= 1e-4; only those are left out of class-map comparisons
  4. gradient signal   every parameter tensor has max |grad| >= 1e-4: 10 x the absolute term of the gradient tolerance.
                       Two tensors cannot: the query and key projections of the attention net reach the loss only through a
                       softmax that is nearly flat on this recipe, max |grad| 9e-6 .. 1e-4 over 22 seeds and four batches; they
                       keep the floor tests/test_gpu_parity.py::test_attention_train_grads gives them, 1e-6.  tests/attn_cases.py
                       is where those two tensors are held to more than a floor, on a recipe with sharp heads.
  5. open or shut      no fc1 pre-activation lies within 1e-5 of zero, the absolute tolerance of h: a kernel whose h is within
                       tolerance may open a ReLU gate the oracle has shut, and dh of that unit, 1 / B of a whole gradient term
                       (5e-5 at B = 513), then goes with it.  Found on the GPU: hsi7 and hsi224p9 at 513 with seed 5 hold one
                       pre-activation of 1.5e-8 and 7.5e-7, and the kernel's gate was the other one for exactly that patch.
                       About one case in three passes this by chance, hence the length of SEEDS.  Asserted where gradients
                       are compared (gradients_compared), not for the cases that only the whole-set passes classify.
"""
import functools

import torch

from test_gpu_half import scene as half_scene
from test_gpu_parity import SHAPES, _scene as rand_scene, make_cfg

H_SCENE, W_SCENE = 37, 41
KMAX, STRIDE = 64, 256                  # csrc/dmf_shapes.h: KMAX, MAX_BLOCKS
MARGIN, MARGIN_CAP = 1e-4, 0.15
PAIR_GAP, GRAD_FLOOR, CLASS_SHARE = 2e-4, 1e-4, 0.02
GRAD_FLOOR_QK = 1e-6                    # attn_wq, attn_wk: see guard 4
GATE_MARGIN = 1e-5

SMALL = ('tiny', 'tiny1', 'quatiny')
LARGE = ('hsi', 'hsi224', 'panms', 'qua', 'hsi9', 'hsi7', 'hsi224p9')
HALF = ('tiny1', 'hsi', 'hsi224', 'qua')                   # test_gpu_half.HALF: the rows with an fp16-scene kernel
SMALL_BATCHES = (255, 256, 257, 511, 512, 513, 769)
LARGE_BATCHES = (257, 513)
UNIT_SMALL = ('tiny1', 'quatiny', 'qua')
UNIT_BATCHES = SMALL_BATCHES + (1023, 1024, 1025, 1281)     # unit_backward_kernel: NPB = 4 patches per round, rounds one and two
UNIT_LARGE = (('hsi', 513), ('hsi9', 513))
ATTN_FORWARD = (('tiny1', 511), ('tiny1', 512), ('tiny1', 513), ('tiny1', 1025), ('hsi', 1025))
ATTN_TRAIN = (('tiny1', 257), ('tiny1', 513), ('hsi', 513))
WHOLE_SET = 1281
WHOLE_SET_CASES = (('tiny1', False, False), ('tiny1', True, False), ('tiny1', False, True), ('hsi', False, False))

# (name, B, half, attention) -> seed of the scene, the permutation and the labels, where the default misses a guard
SEEDS = {
    ('hsi', 257, False, False): 13, ('hsi', 513, False, True): 7, ('hsi', 513, True, False): 19, ('hsi', 1025, False, True): 7,
    ('hsi224', 257, True, False): 9, ('hsi224', 513, False, False): 8, ('hsi224', 513, True, False): 21,
    ('hsi224p9', 513, False, False): 8, ('hsi7', 257, False, False): 13, ('hsi7', 513, False, False): 50,
    ('hsi9', 257, False, False): 11, ('hsi9', 513, False, False): 144, ('panms', 257, False, False): 9,
    ('qua', 255, False, False): 7, ('qua', 256, False, False): 7, ('qua', 511, False, False): 6, ('qua', 512, False, False): 7,
    ('qua', 512, True, False): 7, ('qua', 513, False, False): 6, ('qua', 513, True, False): 7, ('qua', 769, False, False): 13,
    ('qua', 1023, False, False): 37, ('qua', 1023, True, False): 7, ('qua', 1024, False, False): 55,
    ('qua', 1024, True, False): 33, ('qua', 1025, False, False): 56, ('qua', 1025, True, False): 28,
    ('qua', 1281, False, False): 123, ('qua', 1281, True, False): 17, ('quatiny', 255, False, False): 6,
    ('quatiny', 511, False, False): 9, ('quatiny', 769, False, False): 21, ('quatiny', 1023, False, False): 6,
    ('quatiny', 1024, False, False): 11, ('quatiny', 1025, False, False): 18, ('quatiny', 1281, False, False): 36,
    ('tiny', 255, False, False): 7, ('tiny', 257, False, False): 7, ('tiny', 511, False, False): 22,
    ('tiny', 513, False, False): 15, ('tiny', 769, False, False): 12, ('tiny1', 255, True, False): 7,
    ('tiny1', 256, True, False): 7, ('tiny1', 257, True, False): 6, ('tiny1', 511, False, False): 6,
    ('tiny1', 512, False, False): 9, ('tiny1', 512, True, False): 8, ('tiny1', 513, False, False): 8,
    ('tiny1', 513, True, False): 10, ('tiny1', 769, False, False): 28, ('tiny1', 769, True, False): 36,
    ('tiny1', 1023, False, False): 56, ('tiny1', 1023, True, False): 42, ('tiny1', 1024, False, False): 28,
    ('tiny1', 1024, True, False): 10, ('tiny1', 1025, False, False): 6, ('tiny1', 1025, True, False): 135,
    ('tiny1', 1281, False, False): 57, ('tiny1', 1281, True, False): 486,
}


def walk_cases():
    """(name, B, half) of the patch-kernel matrix: forward, train and backward passes."""
    out = []
    for names, batches in ((SMALL, SMALL_BATCHES), (LARGE, LARGE_BATCHES)):
        for name in names:
            for B in batches:
                out.append((name, B, False))
                if name in HALF:
                    out.append((name, B, True))
    return out


def unit_cases():
    out = [(n, B) for n in UNIT_SMALL for B in UNIT_BATCHES] + list(UNIT_LARGE)
    return [(n, B, False) for n, B in out] + [(n, B, True) for n, B in out if n in HALF]


def all_cases():
    """Every (name, B, half, attention) some test of the matrix asks for."""
    keys = [(n, B, h, False) for n, B, h in walk_cases() + unit_cases()]
    keys += [(n, B, False, True) for n, B in ATTN_FORWARD + ATTN_TRAIN]
    keys += [(n, WHOLE_SET, h, a) for n, h, a in WHOLE_SET_CASES]
    return sorted(set(keys))


def gradients_compared(name, B, half, attention):
    """False for the cases only the whole-set passes use: forward and argmax, where guard 5 has nothing to protect."""
    if attention:
        return (name, B) in ATTN_TRAIN
    return (name, B, half) in walk_cases() + unit_cases()


def build_cfg(name, half=False, attention=False):
    cfg = make_cfg(name)
    if half:
        cfg['gmf']['half'] = 1
    if attention:
        cfg['gmf'] = dict(cfg['gmf'], attention=1)
        cfg['trans'] = {'embed_dim': 96, 'num_head': 3}
    return cfg


def oracle_net(cfg, seed=0):
    """The oracle half of nets / half_nets / _attn_nets."""
    from oracle.gmfnet_ref import Net as RefNet
    torch.manual_seed(seed)
    ref = RefNet(cfg)
    with torch.no_grad():
        for k, p in ref.named_parameters():
            p.add_(0.05 * torch.randn_like(p))
            if k.startswith('attn_'):
                p.mul_(3.0)
    return ref


def cut(A, Bm, xy, P, S):
    a = torch.stack([A[x:x + P, y:y + P, :].permute(2, 0, 1) for x, y in xy.tolist()]).contiguous()
    b = torch.stack([Bm[S * x:S * x + S * P, S * y:S * y + S * P, :].permute(2, 0, 1) for x, y in xy.tolist()]).contiguous()
    return a, b


def distinct_xy(B, g):
    """The first B pixels of a permutation of the scene, with its two corners in front."""
    n = H_SCENE * W_SCENE
    perm = torch.randperm(n, generator=g).tolist()
    for pos, pix in ((0, 0), (1, n - 1)):
        at = perm.index(pix)
        perm[pos], perm[at] = perm[at], perm[pos]
    p = torch.tensor(perm[:B])
    return torch.stack([p // W_SCENE, p % W_SCENE], 1).int()


def inputs(name, B, half=False, seed=5):
    """Scene, coordinates, labels and the materialised patches."""
    C, C2, P, S, K = SHAPES[name]
    A, Bm = (half_scene if half else rand_scene)(name, H_SCENE, W_SCENE, seed)
    g = torch.Generator().manual_seed(1000 * seed + B)
    xy = distinct_xy(B, g)
    t = torch.randint(0, K, (B,), generator=g)
    t[0], t[1] = 0, K - 1
    a, b = cut(A, Bm, xy, P, S)
    return A, Bm, xy, t, a, b


def head_pass(ref, a, b):
    """Oracle forward, piece by piece: (z, fc1 output, h, logits)."""
    ya, yb = ref.branches(a, b)
    if ref.arch['attention']:
        ya = ref.attention(ya, yb)
    z = ref.pooled(ya, yb)
    pre = ref.fc1(z)
    h = torch.relu(pre)
    return z, pre, h, ref.fc2(h)


def centre_head(ref, logits):
    with torch.no_grad():
        ref.fc2.bias -= logits.mean(0)


def class_guards(logits, what):
    """Guards 1 and 3 -> (oracle class, mask of the patches whose class stands clear of the tolerance)."""
    B, K = logits.shape
    pred = logits.argmax(1)
    counts = torch.bincount(pred, minlength=K)
    solid = int((counts >= CLASS_SHARE * B).sum())
    assert solid >= min(K, 4), '%s: the oracle predicts only %d classes for >= 2 %% of the batch each (counts %s)' % (
        what, solid, counts.tolist())
    top2 = logits.topk(2, dim=1).values
    safe = (top2[:, 0] - top2[:, 1]) > MARGIN
    close = 1.0 - safe.float().mean().item()
    assert close <= MARGIN_CAP, '%s: %.1f %% of the patches have a top-2 margin <= %g' % (what, 100 * close, MARGIN)
    return pred, safe


def pair_guard(logits, what):
    """Guard 2."""
    B = logits.shape[0]
    worst = float('inf')
    for k in range(1, (B - 1) // STRIDE + 1):
        gap = (logits[:B - STRIDE * k] - logits[STRIDE * k:]).abs().max(1).values
        worst = min(worst, gap.min().item())
    assert worst >= PAIR_GAP, '%s: two patches of one workgroup are only %.2e apart' % (what, worst)
    return worst


def gradient_guard(grads, what):
    """Guard 4."""
    for k, g in grads.items():
        floor = GRAD_FLOOR_QK if k in ('attn_wq', 'attn_wk') else GRAD_FLOOR
        assert g.abs().max().item() >= floor, '%s: max |grad %s| = %.2e' % (what, k, g.abs().max().item())


@functools.lru_cache(maxsize=None)
def case(name, B, half=False, attention=False):
    C, C2, P, S, K = SHAPES[name]
    what = '[%s, B=%d%s%s]' % (name, B, ', half' if half else '', ', attention' if attention else '')
    cfg = build_cfg(name, half, attention)
    ref = oracle_net(cfg)
    A, Bm, xy, t, a, b = inputs(name, B, half, SEEDS.get((name, B, half, attention), 5))
    with torch.no_grad():
        centre_head(ref, head_pass(ref, a, b)[3])
    state = {k: v.detach().clone() for k, v in ref.state_dict().items()}
    ref.zero_grad()
    z, pre, h, logits = head_pass(ref, a, b)
    pre.retain_grad(); logits.retain_grad()
    loss = torch.nn.functional.cross_entropy(logits, t, reduction='none')
    loss.mean().backward()
    grads = {k: p.grad.detach().clone() for k, p in ref.named_parameters()}
    dl = torch.zeros(B, KMAX)
    dlogits = logits.grad.detach().clone()
    dl[:, :K] = dlogits
    hv = dict(z=z.detach(), h=h.detach(), dh=pre.grad.detach().clone(), dl=dl)
    logits = logits.detach()
    pred, safe = class_guards(logits, what)
    pair_gap = pair_guard(logits, what)
    gradient_guard(grads, what)
    gate = pre.detach().abs().min().item()
    assert gate > GATE_MARGIN or not gradients_compared(name, B, half, attention), '%s: an fc1 pre-activation of %.2e: its ReLU gate is anybody\'s' % (what, gate)
    return dict(name=name, B=B, K=K, P=P, S=S, half=half, attention=attention, cfg=cfg, ref=ref, state=state, A=A, Bm=Bm, xy=xy,
                labels=t, a=a, b=b, logits=logits, loss=loss.detach(), grads=grads, hv=hv, dlogits=dlogits, pred=pred,
                safe=safe, pair_gap=pair_gap, gate=gate, what=what)


def unit_reference(c, seed=11):
    """The unit-gradient step's upstream gradient dl = randn / B and autograd of the oracle for it: (dl, grads, head vectors)."""
    ref, B, K = c['ref'], c['B'], c['K']
    dl = torch.randn(B, K, generator=torch.Generator().manual_seed(seed)) / B
    ref.zero_grad()
    z, pre, h, logits = head_pass(ref, c['a'], c['b'])
    pre.retain_grad()
    logits.backward(dl)
    grads = {k: p.grad.detach().clone() for k, p in ref.named_parameters()}
    gradient_guard(grads, c['what'] + ' unit step')
    full = torch.zeros(B, KMAX)
    full[:, :K] = dl
    return dl, grads, dict(z=z.detach(), h=h.detach(), dh=pre.grad.detach().clone(), dl=full)


@functools.lru_cache(maxsize=None)
def qua_eval_case(name='quatiny', B=WHOLE_SET, seed=5):
    """Stage-2 evaluation: the single-input net on four co-registered scenes; the class is the argmax of the SUM of the ms and
    pan streams' logits (tostagesolver.py:337).  The head is centred on half that sum; guards 1 and 3 hold for the sum."""
    C, C2, P, S, K = SHAPES[name]
    cfg = make_cfg(name)
    cfg['gmf']['single_input'] = 1
    ref = oracle_net(cfg)
    g = torch.Generator().manual_seed(seed)
    scenes = [torch.rand(H_SCENE + P - 1, W_SCENE + P - 1, C, generator=g) for _ in range(4)]
    xy = distinct_xy(B, g)
    t = torch.randint(0, K, (B,), generator=g)
    t[0], t[1] = 0, K - 1
    streams = [torch.stack([s[x:x + P, y:y + P, :].permute(2, 0, 1) for x, y in xy.tolist()]).contiguous() for s in scenes[:2]]
    with torch.no_grad():
        centre_head(ref, 0.5 * (ref(streams[0]) + ref(streams[1])))
        state = {k: v.detach().clone() for k, v in ref.state_dict().items()}
        pair = ref(streams[0]) + ref(streams[1])
    pred, safe = class_guards(pair, '[%s, stage-2 evaluation, %d pixels]' % (name, B))
    return dict(name=name, B=B, K=K, P=P, cfg=cfg, ref=ref, state=state, scenes=[s.numpy() for s in scenes], xy=xy, labels=t,
                pair_logits=pair, pred=pred, safe=safe)
