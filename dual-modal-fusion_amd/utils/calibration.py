"""utils.calibration — the host side of `test.calibration`, `test.temperature` and `color.confidence`.

Pure functions, float64: the config keys, ECE / MCE / mean NLL from the integer reliability histogram that dmf_calib_accum
fills (or `histogram` below on the drop-in path), and for `fast_path: 0` the same statistics and the same temperature fit
from torch ops on the logits of `Net.forward`.  Nothing here touches the GPU library.

The histogram hist [nbins, 3] int64 holds per confidence bin the rows, the hits (pred == target) and the sum of the
confidences in units of 2^-32: integers, so it does not depend on the order in which the pixels were counted."""
import math

import numpy as np

TWO32 = 4294967296.0
BETA_LO, BETA_HI = 2.0 ** -6, 2.0 ** 6           # the bracket of the temperature fit (include/dmf.h: dmf_temperature_init)
FIT_STEPS = 40


def calibration_keys(cfg):
    """-> dict(calibration, bins, temperature, confidence) from the optional keys
         test.calibration 0 / 1 (default 0)      test.calibration_bins (default 15, 1..1024)
         test.temperature none / fit / a number T > 0 (default none)      color.confidence 0 / 1 (default 0)
    `temperature` is None, 'fit' or the float T.  Neutral values change nothing."""
    test, color = cfg.get('test') or {}, cfg.get('color') or {}
    on = test.get('calibration', 0) or 0
    conf = color.get('confidence', 0) or 0
    if on not in (0, 1, True, False) or conf not in (0, 1, True, False):
        raise ValueError('test.calibration and color.confidence are 0 or 1')
    bins = test.get('calibration_bins', 15)
    if isinstance(bins, bool) or not isinstance(bins, int) or not 1 <= bins <= 1024:
        raise ValueError('test.calibration_bins %r is not a whole number in 1..1024' % (bins,))
    t = test.get('temperature', 'none')
    if t is None or (isinstance(t, str) and t.lower() == 'none'):
        t = None
    elif isinstance(t, str) and t.lower() == 'fit':
        t = 'fit'
    else:
        try:
            t = float(t)
        except (TypeError, ValueError):
            t = float('nan')
        if isinstance(test.get('temperature'), bool) or not (math.isfinite(t) and t > 0):
            raise ValueError('test.temperature %r is not none, fit or a number T > 0' % (test.get('temperature'),))
    return dict(calibration=bool(on), bins=bins, temperature=t, confidence=bool(conf))


def keys_in_use(keys):
    """The names of the keys that are not neutral, for a refusal."""
    return [name for name, used in (('test.calibration', keys['calibration']), ('test.temperature', keys['temperature'] is not None),
                                    ('color.confidence', keys['confidence'])) if used]


def ece_mce(hist):
    """(ECE, MCE) of hist [nbins, 3]: ECE = sum_b n_b / N |acc_b - conf_b|, MCE the largest gap of a non-empty bin; bins in
    index order, float64; (0, 0) for the empty histogram."""
    rows = np.asarray(hist, dtype=np.int64).reshape(-1, 3).tolist()
    n = sum(r[0] for r in rows)
    ece = mce = 0.0
    for cnt, hit, fixed in rows:
        if cnt:
            gap = abs(hit / cnt - fixed / TWO32 / cnt)
            ece += cnt / n * gap
            mce = max(mce, gap)
    return ece, mce


def summary(hist, nll_sum, temperature):
    """The block that goes to `<t>_calibration.json`: temperature, bins, hist, n, ece, mce, nll (the mean over the n rows)."""
    hist = np.asarray(hist, dtype=np.int64).reshape(-1, 3)
    n = int(hist[:, 0].sum())
    ece, mce = ece_mce(hist)
    return dict(temperature=float(temperature), bins=int(hist.shape[0]), hist=hist.tolist(), n=n, ece=ece, mce=mce,
                nll=float(nll_sum) / n if n else 0.0)


# ------------------------------------------------------------------------------------------------ the drop-in path
def softmax_stats(logits, beta=1.0):
    """torch logits [B, K] -> (pred [B] int64: the first maximal index, stats [3, B] float64: conf, margin, entropy) with the
    definitions of dmf_softmax_stats, in float64."""
    import torch
    l = logits.detach().double()
    K = l.shape[1]
    m = l.max(1, keepdim=True)[0]
    idx = torch.arange(K, device=l.device).expand_as(l)
    pred = torch.where(l == m, idx, torch.full_like(idx, K)).min(1)[0]
    t = (l - m) * float(beta)
    e = torch.exp(t)
    Z = e.sum(1)
    e2 = e.masked_fill(idx == pred[:, None], 0.0).max(1)[0]
    s = torch.where(e > 0, e * t.clamp_min(-1e300), torch.zeros_like(e)).sum(1)
    return pred, torch.stack([1.0 / Z, (1.0 - e2) / Z, (torch.log(Z) - s / Z).clamp_min(0.0)])


def histogram(conf, pred, target, K, nbins):
    """numpy conf / pred / target [B] -> hist [nbins, 3] int64 by dmf_calib_accum's rule on the float32 of conf."""
    conf = np.asarray(conf).astype(np.float32)
    pred, target = np.asarray(pred), np.asarray(target)
    keep = (target >= 0) & (target < K)
    b = np.minimum(nbins - 1, (conf * np.float32(nbins)).astype(np.int64))[keep]
    hist = np.zeros((nbins, 3), dtype=np.int64)
    np.add.at(hist[:, 0], b, 1)
    np.add.at(hist[:, 1], b, (pred[keep] == target[keep]).astype(np.int64))
    np.add.at(hist[:, 2], b, np.rint(conf.astype(np.float64) * TWO32).astype(np.int64)[keep])
    return hist


def nll_terms(logits, labels, beta):
    """numpy logits [N, K], labels [N] -> (nll, g, h): the NLL summed over the rows whose label lies in [0, K), at
    beta = 1 / T, and its first two derivatives in beta (float64)."""
    l = np.asarray(logits, dtype=np.float64)
    y = np.asarray(labels).astype(np.int64)
    keep = (y >= 0) & (y < l.shape[1])
    l, y = l[keep], y[keep]
    d = l - l.max(1, keepdims=True)
    e = np.exp(beta * d)
    Z = e.sum(1)
    mean = (e * d).sum(1) / Z
    dy = d[np.arange(len(y)), y]
    return float((np.log(Z) - beta * dy).sum()), float((mean - dy).sum()), float(((e * d * d).sum(1) / Z - mean * mean).sum())


def fit_temperature(logits, labels, steps=FIT_STEPS):
    """dmf_temperature_step's safeguarded Newton iteration on the host -> dict(beta, lo, hi, steps): g > 0 moves hi to beta,
    else lo; the Newton candidate is kept if h > 0 and it is finite and strictly inside (lo, hi), else sqrt(lo hi)."""
    beta, lo, hi = 1.0, BETA_LO, BETA_HI
    for _ in range(steps):
        _, g, h = nll_terms(logits, labels, beta)
        if g > 0:
            hi = beta
        else:
            lo = beta
        cand = beta - g / h if h > 0 else float('nan')
        beta = cand if math.isfinite(cand) and lo < cand < hi else math.sqrt(lo * hi)
    return dict(beta=beta, lo=lo, hi=hi, steps=steps)
