"""The inputs of tests/test_gpu_row_kernels.py and what it runs on them: the three kernels that give a group of lanes one row of
logits (csrc/dmf_rows.h) — dmf_softmax_stats, dmf_prob_scatter, dmf_logits_mean — at every group size.  `outputs()` is run
twice: by tools/record_eval_fixtures.py on a checkout of the commit the fixture is recorded from, and by the test on the tree
under test.  The fixture keeps the SHA-256 of every output's `tobytes()`: the raw outputs (11 class counts x 3 betas, among
them probability maps of 400 x K floats) are over 1 MB."""
import hashlib

import numpy as np

SEED = 20261
B = 300                                              # two workgroups with a partial last one at L = 1, a partial one elsewhere
CLASSES = (1, 2, 3, 4, 5, 8, 9, 16, 17, 33, 64)      # every L, at a power of two and just past one
BETAS = (None, 0.5, 2.0)
H = W = 20                                           # the map the rows are scattered into
TIES, WIDE = slice(240, 270), slice(270, 300)        # rows with exact ties; rows at +-80 (e == 0 terms at beta >= 1)


def logits(K):
    """[B, K] float32: N(0, 3); a block with exact ties for the maximum, between two columns (even rows) and between all (odd
    rows); a block at +-80 with unit noise."""
    rng = np.random.default_rng(SEED + K)
    x = (3.0 * rng.standard_normal((B, K))).astype(np.float32)
    for r in range(TIES.start, TIES.stop):
        if r % 2 or K < 3:
            x[r] = x[r, 0]
        else:
            a, b = sorted(rng.choice(K, 2, replace=False))
            x[r, a] = x[r, b] = x[r].max() + 1.0
    sign = np.where(rng.random((WIDE.stop - WIDE.start, K)) < 0.5, -80.0, 80.0)
    x[WIDE] = (sign + rng.standard_normal(sign.shape)).astype(np.float32)
    return x


def pixels():
    """[B, 2] int32: B different cells of the H x W map in a permuted order."""
    cells = np.random.default_rng(SEED).permutation(H * W)[:B]
    return np.stack([cells // W, cells % W], 1).astype(np.int32)


def variants(x, V):
    """[V, B, K]: x times 1, 2, 0.5 — exact scalings, so a tie of x is a tie of every term, of the sum and of the mean."""
    return np.stack([x * s for s in (1.0, 2.0, 0.5)[:V]]).astype(np.float32)


def outputs(device='cuda:0'):
    """{name: numpy array} of everything the fixture pins, from the `dmf` that is importable."""
    import torch
    from dmf import lib

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(device)
    out = {}
    xy = dev(pixels())
    for K in CLASSES:
        x = dev(logits(K))
        for beta in BETAS:
            tag = 'K%d.beta%s.' % (K, beta)
            inv = None if beta is None else torch.tensor([beta], dtype=torch.float32, device=device)
            for where, n, kw in (('flat.', B, {}), ('map.', H * W, dict(xy=xy, W=W))):
                pred = torch.zeros(n, dtype=torch.int32, device=device)
                stats = torch.zeros(3, n, dtype=torch.float32, device=device)
                lib.softmax_stats(x, pred=pred, conf=stats[0], margin=stats[1], entropy=stats[2], inv_temp=inv, **kw)
                out[tag + where + 'pred'] = pred.cpu().numpy()
                for k, name in enumerate(('conf', 'margin', 'entropy')):
                    out[tag + where + name] = stats[k].cpu().numpy()
            prob = torch.zeros(H, W, K, dtype=torch.float32, device=device)
            mask = torch.zeros(H, W, dtype=torch.uint8, device=device)
            lib.prob_scatter(x, xy, W, prob, mask, inv_temp=inv)
            out[tag + 'prob'], out[tag + 'mask'] = prob.cpu().numpy(), mask.cpu().numpy()
        for V in (1, 3):
            lv = dev(variants(logits(K), V))
            mean, pred = torch.zeros(B, K, device=device), torch.zeros(B, dtype=torch.int32, device=device)
            lib.logits_mean(lv, mean, pred)
            out['K%d.V%d.mean' % (K, V)], out['K%d.V%d.pred' % (K, V)] = mean.cpu().numpy(), pred.cpu().numpy()
            alone = torch.zeros(B, K, device=device)
            lib.logits_mean(lv, alone, None)
            out['K%d.V%d.mean_without_pred' % (K, V)] = alone.cpu().numpy()
    return out


def digest(a):
    """SHA-256 of an array's bytes, as uint8 [32]."""
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def pack(out):
    """{name: array} -> the fixture's two arrays: the names in order and their digests [n, 32] (one zip member per output would
    cost more than the digests)."""
    names = sorted(out)
    return {'names': np.array(names), 'sha256': np.stack([digest(out[k]) for k in names])}
