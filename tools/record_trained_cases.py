#!/usr/bin/env python3
"""Record tests/golden/g15_trained_cases.npz (weights) and g16_trained_adam.npz (Adam state): the CPU oracle trained to the
weights at which tests/trained_cases.py builds its parity cases.  CPU only; nothing of the HIP side is imported.

    python tools/record_trained_cases.py --threads 8          # all cases, under a minute
    python tools/record_trained_cases.py --only tiny1-mid --steps 200 --dry        # try a recipe, print its regime, write nothing

Recorded from commit dd676bb with --threads 8.  Another torch build or thread count gives other weights in the last
digits: commit the new fixture and let tests/test_trained_cases_host.py say whether every guard still holds (a case that misses
one gets another evaluation seed in trained_cases.SEEDS).

Recipe (tests/trained_cases.py: RECIPES, train_scene): parity_cases.oracle_net(cfg) — the seed-0 net with 0.05 noise —, the
synthetic scene with class structure, min-max normalised, labels label - 1; torch.optim.Adam(lr) for `steps` steps on batches of
256 pixels drawn uniformly from the 37 x 41 anchors by a generator seeded with TRAIN_SEED; batch-mean cross-entropy.

Per case its weights file (trained_cases.WEIGHT_FILES) holds the state_dict ('<case>/w/<name>'), steps, lr, the scene seed, the SHA-256 of the normalised
scene's bytes, the batch size and the batch seed; the Adam file holds exp_avg ('<case>/m/<name>'), exp_avg_sq ('<case>/v/<name>')
and the step count of the cases RECIPES marks.  Numbers and names only.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, 'dual-modal-fusion_amd'), REPO, os.path.join(REPO, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import parity_cases as pc                       # noqa: E402
import trained_cases as tc                      # noqa: E402
from test_gpu_parity import SHAPES              # noqa: E402

MAX_BYTES = 161165                              # the largest fixture committed before these two


def train(name, steps=None, lr=None):
    r = tc.RECIPES[name]
    steps, lr = steps or r['steps'], lr or r['lr']
    row = r['row']
    C, C2, P, S, K = SHAPES[row]
    A, Bm, label, digest = tc.train_scene(name)
    ref = pc.oracle_net(pc.build_cfg(row))
    n = pc.H_SCENE * pc.W_SCENE
    every = torch.arange(n)
    xy = torch.stack([every // pc.W_SCENE, every % pc.W_SCENE], 1)
    a_all, b_all = pc.cut(A, Bm, xy, P, S)
    t_all = label[:pc.H_SCENE, :pc.W_SCENE].reshape(-1)
    opt = torch.optim.Adam(ref.parameters(), lr=lr)
    g = torch.Generator().manual_seed(tc.TRAIN_SEED)
    for step in range(steps):
        idx = torch.randint(0, n, (tc.TRAIN_BATCH,), generator=g)
        opt.zero_grad()
        loss = torch.nn.functional.cross_entropy(ref(a_all[idx], b_all[idx]), t_all[idx])
        loss.backward()
        opt.step()
    with torch.no_grad():
        logits = ref(a_all, b_all)
    prob = torch.softmax(logits, 1)
    print('%s: %d steps at lr %g, last batch loss %.3f; over the scene: max |logit| %.1f, mean max-prob %.3f, accuracy %.3f' % (
        name, steps, lr, loss.item(), logits.abs().max().item(), prob.max(1).values.mean().item(),
        (logits.argmax(1) == t_all).float().mean().item()), flush=True)
    weights = {'%s/w/%s' % (name, k): v.detach().numpy().copy() for k, v in ref.state_dict().items()}
    weights.update({name + '/steps': np.int64(steps), name + '/lr': np.float64(lr), name + '/scene_seed': np.int64(r['scene_seed']), name + '/block': np.int64(r['block']),
                    name + '/scene_sha256': np.str_(digest), name + '/train_seed': np.int64(tc.TRAIN_SEED),
                    name + '/train_batch': np.int64(tc.TRAIN_BATCH)})
    adam = {}
    if r['adam']:
        counts = set()
        for k, p in ref.named_parameters():
            st = opt.state[p]
            adam['%s/m/%s' % (name, k)] = st['exp_avg'].numpy().copy()
            adam['%s/v/%s' % (name, k)] = st['exp_avg_sq'].numpy().copy()
            counts.add(int(st['step']))
        assert counts == {steps}
        adam[name + '/step'] = np.int64(steps)
    return weights, adam


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', action='append')
    ap.add_argument('--steps', type=int)
    ap.add_argument('--lr', type=float)
    ap.add_argument('--dry', action='store_true')
    ap.add_argument('--threads', type=int, default=16)
    args = ap.parse_args()
    torch.set_num_threads(args.threads)
    weights, adam = {}, {}
    for name in args.only or tc.RECIPES:
        t0 = time.time()
        w, a = train(name, args.steps, args.lr)
        weights.update(w); adam.update(a)
        print('  %.0f s' % (time.time() - t0), flush=True)
    if args.dry or args.only:
        print('nothing written (the fixture is recorded whole)')
        return
    files = [(f, {k: v for k, v in weights.items() if k.split('/')[0] in names}) for f, names in tc.WEIGHT_FILES.items()]
    for fname, arrays in files + [(tc.ADAM, adam)]:
        path = os.path.join(tc.GOLDEN, fname)
        np.savez_compressed(path, **arrays)
        size = os.path.getsize(path)
        print('%s: %d arrays, %d bytes' % (path, len(arrays), size))
        assert size < MAX_BYTES, '%s is larger than the largest fixture before it' % fname


if __name__ == '__main__':
    main()
