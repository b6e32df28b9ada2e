"""Parity cases at TRAINED weights, with a float64 reference: shared by tests/test_gpu_trained_parity.py (GPU),
tests/test_trained_cases_host.py (the guards below, on the oracle alone) and tools/record_trained_cases.py (which trains the
weights).  A plain module: no fixtures, no GPU, nothing of the HIP library.

Every other parity test of the patch kernel runs the seed-0 net with 0.05 noise: logits within +-0.02, a flat softmax,
gradients of 1e-3, hidden units open for every patch or for none (profiles/batch_walk_parity.md).  There dl is
(1/K - onehot) / B to three digits whatever the head does with its maximum, its sum or its exponential.  A case here takes
weights the CPU oracle was trained to (tests/golden/g15_trained_cases.npz, tools/record_trained_cases.py) on a synthetic scene
with class structure, so that the softmax is sharp, losses of 5 .. 38 occur, probabilities fall to 1e-17, gradients reach
1 .. 2 and the hidden units are of all three kinds.

A case:
  net          parity_cases.oracle_net(cfg) trained by torch Adam on batches of 256 random pixels (RECIPES); weights from the fixture
  scene        dmf.synth.make_scene, (37 + P - 1) x (41 + P - 1) pixels, n_classes = K, no unlabelled pixels, class blocks of
               15 or 20 pixels (larger than a patch: with the default 5 the trained units are open for all patches or for
               hardly any, and guard 3 finds no case), each modality min-max normalised; its SHA-256 is in the fixture (a numpy that draws another stream fails loudly).  Half: the
               same scene with test_gpu_half.scene's sprinkle of fp16-subnormal magnitudes and exact zeros; the device stores it
               as fp16 and the oracle (gmf.half = 1) rounds at the same places, in float64 too (_ste_f16 keeps the dtype)
  coordinates  parity_cases.distinct_xy(B)
  labels       the scene's, a quarter of them redrawn uniformly (these carry the large losses)
and, all from the FLOAT64 oracle: logits, per-patch loss, gradients of the batch-mean cross-entropy, z / h / dh / dl, and for
the supplied-gradient routes dl = randn(B, K) / B with autograd's gradients for it.

Guards, asserted by `case` on the oracle alone (a case that misses one gets another evaluation seed in SEEDS; the guards stay):
  1. the regime        -sharp: max |logit| >= 8 and mean max-prob >= 0.4; -mid: 0.3 <= mean max-prob <= 0.9; every case: at
                       least min(K, 4) classes predicted for >= 2 % of the batch, a loss >= 5, a probability <= 1e-5;
                       tiny1-sharp: a loss >= 15
  2. the softmax       the gradients dl = (1/K - onehot) / B would give (a flat softmax) miss the true ones by more than
     decides           10 x tolerance in at least 10 elements of every parameter tensor (all of them where a tensor has fewer:
                       fc2.bias of the K = 5 rows)
  3. units of all      fc1 has a unit that is never open, one that is always open and at least 8 open for 10 % .. 90 % of the
     three kinds       batch
  4. gates             with d_s = 4 x max |fp32 oracle - float64 oracle| over the ReLU inputs of site s (spec_a, spat_a, lift_b,
                       spat_b, fc1), no ReLU input of the float64 oracle lies within d_s of zero; fc1 also keeps
                       parity_cases.GATE_MARGIN.  4: a kernel that sums in another order is entitled to the oracle's own error,
                       and a few times that covers the spread between orders
  5. the reference     the fp32 oracle agrees with the float64 one within HALF of each tolerance below
     is stable
  6. margin cap        at most 15 % of the patches have a top-2 margin <= 1e-4; only those are left out of `pred` comparisons

Tolerances (tests/test_gpu_parity.py, test_gpu_seams.py, test_gpu_exit_path.py), widened only as the reference requires, from
the two oracles and never from the kernel:
  logits  max(1e-5, 4 x max |fp32 oracle - float64 oracle|)      loss  max(2.2e-5, 4 x the same over the per-patch losses)
  gradients and head vectors  1e-5 + 1e-4 |want|
"""
import copy
import functools
import hashlib
import os

import numpy as np
import torch

import parity_cases as pc
from test_gpu_parity import SHAPES

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
# weights and recipe scalars, by case, and Adam's state (two files: neither grows past the largest fixture committed before)
WEIGHT_FILES = {'g15_trained_cases.npz': ('tiny1-mid', 'tiny1-sharp', 'tiny-sharp', 'hsi-sharp')}
ADAM = 'g16_trained_adam.npz'

# case -> row, Adam steps, lr, scene seed, side of the scene's class blocks in pixels, whether Adam's state is recorded
RECIPES = {
    'tiny1-mid': dict(row='tiny1', steps=300, lr=1e-3, scene_seed=0, block=15, adam=False),
    'tiny1-sharp': dict(row='tiny1', steps=1000, lr=3e-3, scene_seed=0, block=15, adam=True),
    'tiny-sharp': dict(row='tiny', steps=400, lr=3e-3, scene_seed=0, block=15, adam=False),
    'hsi-sharp': dict(row='hsi', steps=500, lr=3e-3, scene_seed=2, block=20, adam=True),
}
# Not in the matrix, because no evaluation seed among the first 30 met the guards (numbers in profiles/trained_parity.md):
#   hsi224-mid  (hsi224)                    guard 2: a flat softmax moves 5 .. 8 of spec_a.bias's 32 elements (dead channels)
#   panms-mid   (panms)                     guard 3: 0 .. 5 units open for 10 % .. 90 % of 33 patches
TRAIN_BATCH, TRAIN_SEED = 256, 0
BATCHES = {'tiny1': (257, 513), 'tiny': (257, 513), 'hsi': (33,), 'hsi224': (33,), 'panms': (33,)}
HALF_CASES = ('tiny1-sharp', 'hsi-sharp')
ADAM_CASES = tuple(k for k, r in RECIPES.items() if r['adam'])
UNIT_ROWS = ('tiny1', 'tiny', 'hsi')            # the rows of these cases with a two-launch unit-gradient step (lib.unit_supported)
REDRAWN = 0.25
SITES = ('spec_a', 'spat_a', 'lift_b', 'spat_b', 'fc1')
LOGIT_TOL, LOSS_TOL, ATOL, RTOL = 1e-5, 2.2e-5, 1e-5, 1e-4
WIDEN = 4.0
FLAT_DECIDES, FLAT_ELEMENTS = 10.0, 10
MIXED_UNITS = 8

# (case, B, half) -> evaluation seed where the default, 1, misses a guard
SEEDS = {
    ('tiny1-sharp', 257, False): 7, ('tiny1-sharp', 257, True): 16, ('tiny1-sharp', 513, False): 4, ('tiny1-sharp', 513, True): 17,
    ('tiny-sharp', 257, False): 11, ('tiny-sharp', 513, False): 20, ('hsi-sharp', 33, False): 6, ('hsi-sharp', 33, True): 24,
}


def cells():
    """(case, B, half) of the matrix."""
    out = []
    for name, r in RECIPES.items():
        for B in BATCHES[r['row']]:
            out.append((name, B, False))
            if name in HALF_CASES:
                out.append((name, B, True))
    return out


def weights_file(name):
    return next(f for f, names in WEIGHT_FILES.items() if name in names)


def row_of(name):
    return RECIPES[name]['row']


# ---------------------------------------------------------------------------------------------------------------- the scene
def _minmax(x):
    lo, hi = float(x.min()), float(x.max())
    return ((x - lo) / (hi - lo)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def train_scene(name):
    """-> (A [H+P-1, W+P-1, C], Bm [S(H+P-1), S(W+P-1), C2], label [H+P-1, W+P-1] in 0 .. K-1, sha256 of A's and Bm's bytes)."""
    from dmf import synth                       # numpy only
    C, C2, P, S, K = SHAPES[row_of(name)]
    H, W = pc.H_SCENE + P - 1, pc.W_SCENE + P - 1
    primary, aux, label = synth.make_scene(H, W, C, C2, S, n_classes=K, seed=RECIPES[name]['scene_seed'], block=RECIPES[name]['block'],
                                             unlabelled=0)
    A = np.ascontiguousarray(_minmax(primary))
    Bm = np.ascontiguousarray(_minmax(aux).reshape(S * H, S * W, C2))
    digest = hashlib.sha256(A.tobytes() + Bm.tobytes()).hexdigest()
    return torch.from_numpy(A), torch.from_numpy(Bm), torch.from_numpy(label.astype(np.int64) - 1), digest


def half_sprinkle(A, seed):
    """test_gpu_half.scene's sprinkle: 2 % of the primary scene scaled to fp16-subnormal magnitudes, 1 % exact zeros."""
    g = torch.Generator().manual_seed(seed)
    A = A.clone()
    tiny = torch.rand(A.shape, generator=g) < 0.02
    A[tiny] *= 4e-5
    A[torch.rand(A.shape, generator=g) < 0.01] = 0.0
    return A


def inputs(name, B, half, seed):
    """Scene, coordinates, labels and the materialised patches."""
    C, C2, P, S, K = SHAPES[row_of(name)]
    A, Bm, label, _ = train_scene(name)
    if half:
        A = half_sprinkle(A, seed)
    g = torch.Generator().manual_seed(1000 * seed + B)
    xy = pc.distinct_xy(B, g)
    t = label[xy[:, 0].long(), xy[:, 1].long()].clone()
    redrawn = torch.rand(B, generator=g) < REDRAWN
    t[redrawn] = torch.randint(0, K, (int(redrawn.sum()),), generator=g)
    a, b = pc.cut(A, Bm, xy, P, S)
    return A, Bm, xy, t, a, b


# -------------------------------------------------------------------------------------------------------------- the fixture
@functools.lru_cache(maxsize=None)
def _npz(fname):
    with np.load(os.path.join(GOLDEN, fname), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def fixture_keys(name, state_keys):
    """The names tools/record_trained_cases.py writes for one case: (weights file, Adam file)."""
    w = ['%s/w/%s' % (name, k) for k in state_keys] + ['%s/%s' % (name, k) for k in ('steps', 'lr', 'scene_seed', 'block', 'scene_sha256',
                                                                                      'train_seed', 'train_batch')]
    a = []
    if RECIPES[name]['adam']:
        a = ['%s/%s/%s' % (name, mv, k) for mv in ('m', 'v') for k in state_keys if k != 'pool_w'] + ['%s/step' % name]
    return w, a


def trained_state(name):
    """-> (state_dict, dict(m=..., v=..., step=...) or None), after the recipe and the scene's digest are checked."""
    z = _npz(weights_file(name))
    r = RECIPES[name]
    assert int(z[name + '/steps']) == r['steps'] and abs(float(z[name + '/lr']) - r['lr']) < 1e-12, name
    assert int(z[name + '/scene_seed']) == r['scene_seed'] and int(z[name + '/train_seed']) == TRAIN_SEED, name
    assert int(z[name + '/train_batch']) == TRAIN_BATCH and int(z[name + '/block']) == r['block'], name
    digest = train_scene(name)[3]
    assert str(z[name + '/scene_sha256']) == digest, '%s: the scene drawn here is not the scene the weights were trained on' % name
    pre = name + '/w/'
    state = {k[len(pre):]: torch.from_numpy(v.copy()) for k, v in z.items() if k.startswith(pre)}
    adam = None
    if r['adam']:
        za = _npz(ADAM)
        adam = dict(step=int(za[name + '/step']))
        for mv in ('m', 'v'):
            p = '%s/%s/' % (name, mv)
            adam[mv] = {k[len(p):]: torch.from_numpy(v.copy()) for k, v in za.items() if k.startswith(p)}
    return state, adam


# --------------------------------------------------------------------------------------------------------------- the oracle
def site_pass(ref, a, b):
    """Oracle forward, ReLU input by ReLU input: (dict site -> ReLU input, z, h, logits).  Restates Net.branches / .forward."""
    from oracle.gmfnet_ref import _ste_f16
    F_ = torch.nn.functional
    s = {}
    if ref.arch.get('half'):
        s['spec_a'] = F_.conv2d(_ste_f16(a), _ste_f16(ref.spec_a.weight), ref.spec_a.bias, groups=ref.spec_a.groups)
    else:
        s['spec_a'] = ref.spec_a(a)
    s['spat_a'] = ref.spat_a(F_.relu(s['spec_a']))
    s['lift_b'] = ref.lift_b(b)
    s['spat_b'] = ref.spat_b(F_.relu(s['lift_b']))
    z = ref.pooled(F_.relu(s['spat_a']), F_.relu(s['spat_b']))
    s['fc1'] = ref.fc1(z)
    h = F_.relu(s['fc1'])
    return s, z, h, ref.fc2(h)


def _grads(ref, out, seed_grad=None):
    ref.zero_grad()
    out.backward(seed_grad, retain_graph=True)
    return {k: p.grad.detach().clone() for k, p in ref.named_parameters()}


def full_pass(ref, a, b, t, dl_unit):
    """Everything the tests compare, in ref's own precision."""
    s, z, h, logits = site_pass(ref, a, b)
    B, K = logits.shape
    pre = s['fc1']
    pre.retain_grad(); logits.retain_grad()
    loss = torch.nn.functional.cross_entropy(logits, t, reduction='none')
    grads = _grads(ref, loss.mean())
    dlogits, dh = logits.grad.detach().clone(), pre.grad.detach().clone()
    flat = (torch.full((B, K), 1.0 / K, dtype=logits.dtype) - torch.nn.functional.one_hot(t, K).to(logits.dtype)) / B
    flat_grads = _grads(ref, logits, flat)
    pre.grad = None
    unit_grads = _grads(ref, logits, dl_unit.to(logits.dtype))
    unit_dh = pre.grad.detach().clone()
    ref.zero_grad()
    return dict(sites={k: v.detach() for k, v in s.items()}, z=z.detach(), h=h.detach(), logits=logits.detach(), loss=loss.detach(),
                grads=grads, dlogits=dlogits, dh=dh, flat_grads=flat_grads, unit_grads=unit_grads, unit_dh=unit_dh)


def tolerance(want, atol=ATOL, rtol=RTOL):
    return atol + rtol * want.abs()


def _ratio(got, want):
    """Worst |got - want| / tolerance."""
    return ((got.double() - want.double()).abs() / tolerance(want.double())).max().item() if want.numel() else 0.0


def _pad(x, W=pc.KMAX):
    out = torch.zeros(x.shape[0], W, dtype=x.dtype)
    out[:, :x.shape[1]] = x
    return out


@functools.lru_cache(maxsize=None)
def case(name, B, half=False):
    row = row_of(name)
    C, C2, P, S, K = SHAPES[row]
    what = '[%s, B=%d%s]' % (name, B, ', half' if half else '')
    seed = SEEDS.get((name, B, half), 1)
    cfg = pc.build_cfg(row, half)
    state, adam = trained_state(name)
    from oracle.gmfnet_ref import Net as RefNet
    ref = RefNet(cfg)
    ref.load_state_dict(state)
    ref64 = copy.deepcopy(ref).double()
    A, Bm, xy, t, a, b = inputs(name, B, half, seed)
    dl_unit = torch.randn(B, K, generator=torch.Generator().manual_seed(11), dtype=torch.float64) / B
    r32 = full_pass(ref, a, b, t, dl_unit)
    r64 = full_pass(ref64, a.double(), b.double(), t, dl_unit)
    logits, loss = r64['logits'], r64['loss']
    m = {}                                                       # what the guards measured

    # 1. the regime
    prob = torch.softmax(logits, 1)
    m['max_logit'], m['max_prob'] = logits.abs().max().item(), prob.max(1).values.mean().item()
    m['max_loss'], m['min_prob'] = loss.max().item(), prob.min().item()
    if name.endswith('-sharp'):
        assert m['max_logit'] >= 8 and m['max_prob'] >= 0.4, '%s: max |logit| %.2f, mean max-prob %.3f' % (what, m['max_logit'], m['max_prob'])
    else:
        assert 0.3 <= m['max_prob'] <= 0.9, '%s: mean max-prob %.3f' % (what, m['max_prob'])
    assert m['max_loss'] >= 5, '%s: the largest loss is %.2f' % (what, m['max_loss'])
    assert m['min_prob'] <= 1e-5, '%s: the smallest probability is %.2e' % (what, m['min_prob'])
    if name == 'tiny1-sharp':
        assert m['max_loss'] >= 15, '%s: the largest loss is %.2f' % (what, m['max_loss'])
    pred, safe = pc.class_guards(logits, what)                   # and 6. margin cap
    m['close'] = 1.0 - safe.float().mean().item()

    # 2. the softmax decides
    m['flat'] = {}
    for k, g in r64['grads'].items():
        n = int(((r64['flat_grads'][k] - g).abs() > FLAT_DECIDES * tolerance(g)).sum())
        m['flat'][k] = n
        assert n >= min(FLAT_ELEMENTS, g.numel()), '%s: a flat softmax moves only %d elements of grad %s beyond 10 x tolerance' % (what, n, k)

    # 3. units of all three kinds
    share = (r64['sites']['fc1'] > 0).double().mean(0)
    m['never'], m['always'] = int((share == 0).sum()), int((share == 1).sum())
    m['mixed'] = int(((share >= 0.1) & (share <= 0.9)).sum())
    assert m['never'] >= 1 and m['always'] >= 1 and m['mixed'] >= MIXED_UNITS, '%s: fc1 units never / always / 10-90 %% open: %d / %d / %d' % (
        what, m['never'], m['always'], m['mixed'])

    # 4. gates
    m['delta'], m['gate'] = {}, {}
    for s in SITES:
        d = WIDEN * (r32['sites'][s].double() - r64['sites'][s]).abs().max().item()
        if s == 'fc1':
            d = max(d, pc.GATE_MARGIN)
        near = r64['sites'][s].abs().min().item()
        m['delta'][s], m['gate'][s] = d, near
        assert near > d, '%s: a %s ReLU input of %.2e, within %.2e of zero: its gate is anybody\'s' % (what, s, near, d)

    # tolerances, from the two oracles
    logit_gap = (r32['logits'].double() - logits).abs().max().item()
    loss_gap = (r32['loss'].double() - loss).abs().max().item()
    logit_tol, loss_tol = max(LOGIT_TOL, WIDEN * logit_gap), max(LOSS_TOL, WIDEN * loss_gap)
    m.update(logit_gap=logit_gap, loss_gap=loss_gap, logit_tol=logit_tol, loss_tol=loss_tol)

    # 5. the reference is stable
    assert logit_gap <= 0.5 * logit_tol and loss_gap <= 0.5 * loss_tol
    m['stable'] = max([_ratio(r32[k][p], r64[k][p]) for k in ('grads', 'unit_grads') for p in r64[k]]
                      + [_ratio(r32[k], r64[k]) for k in ('z', 'h', 'dh', 'dlogits', 'unit_dh')])
    assert m['stable'] <= 0.5, '%s: the fp32 oracle sits at %.3f of a tolerance from the float64 one' % (what, m['stable'])

    hv = dict(z=r64['z'], h=r64['h'], dh=r64['dh'], dl=_pad(r64['dlogits']))
    unit_hv = dict(z=r64['z'], h=r64['h'], dh=r64['unit_dh'], dl=_pad(dl_unit.float()))
    return dict(name=name, row=row, B=B, K=K, P=P, S=S, half=half, cfg=cfg, ref=ref, ref64=ref64, state=state, adam=adam,
                lr=RECIPES[name]['lr'], A=A, Bm=Bm, xy=xy, labels=t, a=a, b=b, logits=logits, loss=loss, grads=r64['grads'], hv=hv,
                dlogits=r64['dlogits'], dl_unit=dl_unit.float(), unit_grads=r64['unit_grads'], unit_hv=unit_hv, pred=pred, safe=safe,
                logit_tol=logit_tol, loss_tol=loss_tol, measured=m, what=what, seed=seed)


def report(c):
    """The guards' numbers of one case, as one table row."""
    m = c['measured']
    return '| %s | %d | %.1f | %.2f | %.1f | %.1e | %d / %d / %d | %s | %s | %.1e | %.1e | %.3f |' % (
        c['what'][1:-1], c['seed'], m['max_logit'], m['max_prob'], m['max_loss'], m['min_prob'], m['never'], m['always'], m['mixed'],
        ' '.join('%.1e' % m['delta'][s] for s in SITES), ' '.join('%.1e' % m['gate'][s] for s in SITES), m['logit_tol'], m['loss_tol'],
        m['stable'])


REPORT_HEAD = ('| case | eval seed | max abs logit | mean max-prob | max loss | min prob | fc1 units never / always / 10-90 % open | '
               'd_s: spec_a spat_a lift_b spat_b fc1 | smallest abs ReLU input, same sites | logits tol | loss tol | fp32 oracle / tolerance |\n'
               '|---|---|---|---|---|---|---|---|---|---|---|---|')
