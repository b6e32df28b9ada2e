"""The torch statement of the criteria of dmf_ce_loss, on the CPU, in the dtype asked for: what the tests of
that kernel, of the engines and of the solvers compare against.

  kind 'ce'     torch.nn.functional.cross_entropy(logits, y, weight=w, label_smoothing=eps, reduction='mean')
  kind 'focal'  sum_i w[y_i] (1 - p_i)^gamma (-log p_i) / sum_i w[y_i], p_i = softmax(logits_i)[y_i], with log(1 - p_i) formed as the
                logsumexp of the other classes' logits minus that of all (not the way utils.FocalLoss or the kernel form it)

Also the cases of the kernel test (K, bs_r, ten criteria, two sets of logits) and its bound, which a CPU test evaluates on
per-sample terms computed in float64 and rounded once to float32 (the best any float32 `loss[i]` can be).
"""
import numpy as np
import torch
import torch.nn.functional as F


def criterion_value(logits, y, kind='ce', weight=None, eps=0.0, gamma=0.0):
    """The batch loss (a 0-dim tensor of logits' dtype, differentiable)."""
    w = None if weight is None else torch.as_tensor(weight).to(logits.dtype)
    y = y.long()
    if kind == 'ce':
        return F.cross_entropy(logits, y, weight=w, label_smoothing=eps, reduction='mean')
    # written apart from utils.FocalLoss: log(1 - p_y) = logsumexp of the OTHER logits - logsumexp of all of them
    hit = torch.zeros_like(logits, dtype=torch.bool).scatter_(1, y.view(-1, 1), True)
    lse = torch.logsumexp(logits, dim=1)
    q = (torch.logsumexp(logits.masked_fill(hit, float('-inf')), dim=1) - lse).exp()
    nlp = lse - logits.gather(1, y.view(-1, 1)).squeeze(1)
    wy = w[y] if w is not None else torch.ones_like(q)
    return (wy * q.pow(gamma) * nlp).sum() / wy.sum()


def value_and_grad(logits, y, dtype, **spec):
    """(batch loss, d loss / d logits) of the criterion evaluated in `dtype` on the same logits, both as float64."""
    z = logits.detach().to(dtype).clone().requires_grad_(True)
    v = criterion_value(z, y, **spec)
    v.backward()
    return v.detach().double(), z.grad.double()


def module(kind='ce', weight=None, eps=0.0, gamma=0.0):
    """criterion_value as a callable (output, target) -> loss, for a training loop."""
    return lambda output, target: criterion_value(output, target, kind, weight, eps, gamma)


# ---------------------------------------------------------------------------------------------- the cases of the kernel test
KS, BS_RS = [2, 5, 16, 17, 33, 64], [1, 7, 16, 17, 255, 300]
VARIANTS = [('plain', dict(kind='ce'), False),
            ('weights', dict(kind='ce'), True),
            ('eps', dict(kind='ce', eps=0.1), False),
            ('eps+weights', dict(kind='ce', eps=0.1), True)] + \
           [('focal%d%s' % (gm, '+weights' if wt else ''), dict(kind='focal', gamma=float(gm)), wt)
            for gm in (0, 1, 2) for wt in (False, True)]


def class_weights(K, g):
    """K weights spanning 0.01 ... 50 (both ends present), in a shuffled order."""
    w = torch.logspace(-2, float(np.log10(50.0)), K) if K > 1 else torch.tensor([0.01])
    return w[torch.randperm(K, generator=g)].float()


def logit_sets(K, bs_r, g):
    """('unit', N(0,1)) and ('wide', scaled to +-80), each with a row whose p_y is within 1e-7 of 1 and a row with p_y < 1e-30
    (one batch row each; a one-row batch has the first kind in 'unit' and the second in 'wide')."""
    y = torch.randint(0, K, (bs_r,), generator=g)
    unit = torch.randn(bs_r, K, generator=g)
    wide = torch.randn(bs_r, K, generator=g)
    wide = wide * (80.0 / wide.abs().max())
    other = (y + 1) % K
    unit[0, y[0]] = 30.0                                   # the other logits are N(0,1): 1 - p_y ~ 1e-12
    wide[0, y[0]], wide[0, other[0]] = -80.0, 80.0         # p_y <= e^-160
    if bs_r > 1:
        unit[1, y[1]], unit[1, other[1]] = -45.0, 45.0     # p_y <= e^-90
        wide[1, y[1]] = 80.0
        wide[1, torch.arange(K) != y[1]] = wide[1, torch.arange(K) != y[1]].clamp(max=40.0)
    return y, {'unit': unit, 'wide': wide}


def case(K, bs_r):
    """(labels, {name: logits}, weights) of the kernel test's case (K, bs_r), seeded."""
    g = torch.Generator().manual_seed(100 * K + bs_r)
    y, sets = logit_sets(K, bs_r, g)
    return y, sets, class_weights(K, g)


def ref_spec(spec, w):
    return dict(kind=spec['kind'], weight=w, eps=spec.get('eps', 0.0), gamma=spec.get('gamma', 0.0))


def half_ulp32(x):
    """Half a unit in the last place of float32 at |x| (float64 tensor): the error of ONE rounding of x to float32."""
    x = x.double().abs().clamp(min=float(np.finfo(np.float32).tiny))
    return 0.5 * torch.pow(2.0, torch.floor(torch.log2(x)) - 23)


def value_bound(dev32, loss):
    """The bound on |mean(loss) - float64 value| for an output `loss` [bs_r] stored in float32:
        4 x (deviation of the same evaluation in torch float32) + 1e-7            the issue's bound
        + mean_i half_ulp32(loss[i])                                              the storage of loss[i]
    Why the second term: the value is mean(loss), and each loss[i] is a float32 — even a term computed exactly is rounded once,
    by up to half an ulp of its own size, while the float32 value of one torch evaluation is ONE rounded number that by chance
    lies anywhere between 0 and half an ulp from the float64 value.  Without the term, per-sample terms computed in float64
    and rounded once miss the bound in some evaluations (tests/test_ce_loss_host.py counts them); the term is the format's
    precision, it does not come from the kernel, and the gradient (stored per element, compared per element) needs none."""
    return 4 * dev32 + 1e-7 + half_ulp32(loss).mean().item()


def per_sample_terms(logits, y, kind='ce', weight=None, eps=0.0, gamma=0.0):
    """(t_i [bs_r], D) in float64, vectorised: batch loss = t.sum() / D."""
    z = logits.double()
    y = y.long()
    K = z.shape[1]
    w = torch.ones(K, dtype=torch.float64) if weight is None else torch.as_tensor(weight).double()
    logp = F.log_softmax(z, dim=1)
    nlp = -logp.gather(1, y.view(-1, 1)).squeeze(1)
    if kind == 'ce':
        t = (1 - eps) * w[y] * nlp + eps / K * (-(logp * w.view(1, K)).sum(1))
    else:
        hit = torch.zeros_like(z, dtype=torch.bool).scatter_(1, y.view(-1, 1), True)
        t = w[y] * logp.exp().masked_fill(hit, 0.0).sum(1).pow(gamma) * nlp
    return t, w[y].sum()
