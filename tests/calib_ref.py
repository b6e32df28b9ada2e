"""Float64 numpy statement of the calibration arithmetic and the cases the host and GPU tests share:
softmax statistics from fp32 logits and an fp32 beta, the reliability histogram, ECE / MCE, and the safeguarded Newton rule
of the temperature fit exactly as include/dmf.h states it."""
import functools
import math

import numpy as np

TWO32 = 4294967296.0


def tol(K):
    """Worst-case envelope of the fp32 kernel against float64: the rounding of the argument, expf, a K-term sum and a division."""
    return (K + 16) * (1.0 + math.log(K)) * 2.0 ** -23


def stats(logits, beta=1.0):
    """logits [B, K] float32, beta a float32 value -> pred (first maximal index), conf, margin, entropy in float64."""
    l = np.asarray(logits, dtype=np.float32).astype(np.float64)
    b = float(np.float32(beta))
    pred = l.argmax(1)                                   # numpy's argmax is the first maximal index
    t = (l - l.max(1, keepdims=True)) * b
    e = np.exp(t)
    Z = e.sum(1)
    rest = e.copy()
    rest[np.arange(len(l)), pred] = 0.0
    e2 = rest.max(1)
    s = np.where(e > 0, e * np.where(e > 0, t, 0.0), 0.0).sum(1)
    return pred.astype(np.int32), 1.0 / Z, (1.0 - e2) / Z, np.maximum(0.0, np.log(Z) - s / Z)


def histogram(conf, pred, target, K, nbins):
    """conf float32 [B] -> hist int64 [nbins, 3]: rows, hits, sum of llrint(conf * 2^32); targets outside [0, K) are skipped."""
    conf = np.asarray(conf, dtype=np.float32)
    pred, target = np.asarray(pred), np.asarray(target)
    keep = (target >= 0) & (target < K)
    b = np.minimum(nbins - 1, (conf * np.float32(nbins)).astype(np.int64))
    fixed = np.rint(conf.astype(np.float64) * TWO32).astype(np.int64)
    hist = np.zeros((nbins, 3), dtype=np.int64)
    np.add.at(hist[:, 0], b[keep], 1)
    np.add.at(hist[:, 1], b[keep], (pred[keep] == target[keep]).astype(np.int64))
    np.add.at(hist[:, 2], b[keep], fixed[keep])
    return hist


def ece_mce(hist):
    """(ECE, MCE) of hist [nbins, 3] in float64, bin by bin in index order; (0, 0) for the empty histogram."""
    hist = np.asarray(hist, dtype=np.int64)
    n = int(hist[:, 0].sum())
    ece = mce = 0.0
    for cnt, hit, fixed in hist.tolist():
        if cnt:
            gap = abs(hit / cnt - fixed / TWO32 / cnt)
            ece += cnt / n * gap
            mce = max(mce, gap)
    return ece, mce


def nll_terms(logits, labels, beta):
    """(nll, g, h): the NLL of the labelled rows at beta and its first two derivatives in beta, float64."""
    l = np.asarray(logits, dtype=np.float32).astype(np.float64)
    y = np.asarray(labels)
    keep = (y >= 0) & (y < l.shape[1])
    l, y = l[keep], y[keep]
    d = l - l.max(1, keepdims=True)
    e = np.exp(beta * d)
    Z = e.sum(1)
    mean = (e * d).sum(1) / Z
    dy = d[np.arange(len(y)), y]
    return float((np.log(Z) - beta * dy).sum()), float((mean - dy).sum()), float(((e * d * d).sum(1) / Z - mean * mean).sum())


def newton_step(state, g, h):
    """The safeguarded step on state = dict(beta, lo, hi, steps), in place."""
    beta = state['beta']
    if g > 0:
        state['hi'] = beta
    else:
        state['lo'] = beta
    lo, hi = state['lo'], state['hi']
    with np.errstate(all='ignore'):
        cand = float(np.float64(beta) - np.float64(g) / np.float64(h))
    if not (h > 0) or not math.isfinite(cand) or not (lo < cand < hi):
        cand = math.sqrt(lo * hi)
    state['beta'] = cand
    state['steps'] += 1


def fit(logits, labels, steps=40):
    """-> the state after `steps` steps, with nll, g, h of the last evaluation (at the beta that step started from)."""
    state = dict(beta=1.0, lo=2.0 ** -6, hi=2.0 ** 6, steps=0, nll=0.0, g=0.0, h=0.0)
    for _ in range(steps):
        state['nll'], state['g'], state['h'] = nll_terms(logits, labels, state['beta'])
        newton_step(state, state['g'], state['h'])
    return state


# ------------------------------------------------------------------------------------------------ cases
STATS_K = (1, 2, 3, 17, 64)
STATS_B = (1, 63, 257, 1025)
STATS_BETA = (1.0, 0.5, 3.0)
STATS_SCALE = (1.0, 40.0)


@functools.lru_cache(maxsize=None)
def stats_logits(K, B, scale):
    """Rows whose entries are at least 1e-3 apart: a random permutation of a jittered grid of spacing 0.25, times `scale`."""
    rng = np.random.default_rng(1000 * K + B + int(scale))
    base = (np.arange(K) - K / 2.0) * 0.25
    rows = np.stack([rng.permutation(base + rng.uniform(-0.1, 0.1, K)) for _ in range(B)])
    out = (rows * scale).astype(np.float32)
    out.setflags(write=False)
    return out


TIE_K = (4, 17, 64)


def tie_logits(K):
    """Five rows of K >= 4 logits: two maxima tied (first at 1), three tied (first at 0), all equal, a tie at the last two
    entries, and a tie below the maximum (no tie at the top: margin > 0)."""
    rows = np.tile((-0.5 - 0.25 * np.arange(K)).astype(np.float32), (5, 1))
    rows[0, 1] = rows[0, K - 1] = 2.0
    rows[1, 0] = rows[1, 2] = rows[1, K - 1] = 1.5
    rows[2, :] = 0.75
    rows[3, K - 2] = rows[3, K - 1] = 3.0
    rows[4, 0] = 4.0
    rows[4, 1] = rows[4, 2] = 1.0
    return rows, np.array([1, 0, 0, K - 2, 0], dtype=np.int32), np.array([True, True, True, True, False])


FIT_N = (1, 255, 257, 1000)
FIT_K = (2, 17)
FIT_KINDS = ('over', 'under', 'bound')


@functools.lru_cache(maxsize=None)
def fit_case(kind, N, K):
    """(logits [N, K] float32, labels [N] int32).  `over` / `under`: labels drawn from softmax(z), logits = z * 5 / z * 0.3
    (beta* near 0.2 / 3.3: interior).  `bound`: the label is the argmax, by a small gap: the NLL falls all the way to 2^6.
    A single row cannot be sampled into calibration: its label is the runner-up.  With K = 17 that is interior (the runner-up
    lies above the row's mean, so g < 0 at beta = 0 and g > 0 for large beta); with K = 2 the runner-up is the minimum, g > 0
    everywhere and the fit ends at 2^-6 (`fit_expect`)."""
    rng = np.random.default_rng({'over': 1, 'under': 2, 'bound': 3}[kind] * 100000 + 100 * N + K)
    if kind == 'bound':
        z = rng.standard_normal((N, K)) * 0.02
        return z.astype(np.float32), z.astype(np.float32).argmax(1).astype(np.int32)
    z = rng.standard_normal((N, K)) * 2.0
    if N == 1:
        y = np.argsort(z, 1)[:, -2]
    else:
        p = np.exp(z - z.max(1, keepdims=True))
        p /= p.sum(1, keepdims=True)
        y = np.array([rng.choice(K, p=p[i]) for i in range(N)])
    return (z * (5.0 if kind == 'over' else 0.3)).astype(np.float32), y.astype(np.int32)


def fit_expect(kind, N, K):
    """Where the fit of fit_case(kind, N, K) ends: 'interior', or at the bracket's end 'hi' (2^6) / 'lo' (2^-6)."""
    if kind == 'bound':
        return 'hi'
    return 'lo' if N == 1 and K == 2 else 'interior'
