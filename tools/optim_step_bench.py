"""Step time of the one-launch regularised update (dmf_optim_step: weight decay, AdamW, gradient-norm clipping) next to the
three-launch SGD step of the same process — the like-for-like baseline: the same launch count and the same dmf_grad_reduce,
with dmf_sgd_step in the place of dmf_optim_step — all replayed from captured graphs (profiles/optim_step.md).

    python tools/optim_step_bench.py [steps] [repeats] [rounds] [variants]

variants: a comma-separated subset of the variant names below (default: all).  `sgd_three_launch_baseline` alone also runs in a
checkout of the commit before dmf_optim_step (copy this file into its tools/): that is the parent-commit figure.

Shape: BASELINE configs[1] (200-band HSI + 1-band SAR, 11x11 patches, 17 logits), batch 256, graphs of 50 steps, one GPU.
The variants alternate `rounds` times (default 3) inside one process, baseline first in every round, so that clock and
thermal drift hits them alike; every figure is the median of `repeats` timed runs of `steps` steps after an untimed capture
and first replay.  One JSON line per round and a last one with the medians over the rounds and the surplus over the baseline.
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'dual-modal-fusion_amd'), ROOT]
from dmf import synth
from dmf.engine import Scene, TrainEngine
from function.function import data_padding, data_padding_aux
from model.gmfnet import Net

SHAPE = dict(size=145, bands=200, patch=11, scale=1, classes=16)
B, SPG = 256, 50
# (SGD without the new keys is the parent commit's three-launch step: dmf_train_fwd_bwd, dmf_grad_reduce, dmf_sgd_step)
VARIANTS = (('sgd_three_launch_baseline', dict(optimizer='SGD', lr=0.05, momentum=0.9)),
            ('sgd_wd_clip', dict(optimizer='SGD', lr=0.05, momentum=0.9, weight_decay=0.01, clip_grad_norm=1.0)),
            ('adamw_wd_clip', dict(optimizer='ADAMW', lr=1e-3, weight_decay=0.01, clip_grad_norm=1.0)),
            ('fused_adam_default', dict(optimizer='ADAM', lr=1e-3)))


def step_time(eng, xy, lab, steps, repeats):
    """Median over `repeats` of the time per step of `steps` steps replayed from graphs of SPG steps (us)."""
    eng.load_plan(xy, lab)
    eng.run_plan(SPG, SPG)                                  # capture + first replay: not timed
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        eng.load_plan(xy, lab)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.run_plan(steps, SPG)
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / steps * 1e6)
    return float(np.median(out)), [round(v, 2) for v in out]


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 500
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    only = sys.argv[4].split(',') if len(sys.argv) > 4 else [tag for tag, _ in VARIANTS]
    variants = [(tag, kw) for tag, kw in VARIANTS if tag in only]
    steps -= steps % SPG
    s = SHAPE
    K = s['classes'] + 1
    cfg = {'patch_size': s['patch'], 'Categories_Number': K, 'data_city': 's', 'DATA_DICT': {'s': {'size': [s['size'], s['size'], s['bands']]}},
           'scale': s['scale'], 'aux_bands': 1, 'gmf': {'width': 40, 'hidden': 64, 'pool_sigma': 2.5, 'attention': 0}}
    primary, aux, label = synth.make_scene(s['size'], s['size'], s['bands'], 1, s['scale'], n_classes=s['classes'], seed=0)
    scene = Scene(data_padding(primary, cfg, 'ms').astype(np.float32), data_padding_aux(aux, cfg).astype(np.float32), 'cuda:0')
    g = np.random.default_rng(1)
    xy = np.stack([g.integers(0, s['size'], steps * B), g.integers(0, s['size'], steps * B)], 1).astype(np.int32)
    lab = np.maximum(label[xy[:, 0], xy[:, 1]], 1).astype(np.int32)
    engines = {}
    for tag, kw in variants:
        torch.manual_seed(0)
        engines[tag] = TrainEngine(Net(cfg).cuda(), scene, B, **kw)
    n_params = engines[variants[0][0]].theta.numel()
    per_round = {tag: [] for tag, _ in variants}
    for r in range(rounds):
        res = {'round': r, 'shape': 'configs[1]', 'batch': B, 'n_params': n_params, 'steps': steps, 'steps_per_graph': SPG,
               'repeats': repeats}
        for tag, _ in variants:
            med, runs = step_time(engines[tag], xy, lab, steps, repeats)
            per_round[tag].append(med)
            res[tag + '_us_per_step'] = round(med, 2)
            res[tag + '_runs'] = runs
        print(json.dumps(res), flush=True)
    base = per_round[variants[0][0]]
    out = {'summary': 'median over %d rounds (us per step); surplus = variant - %s per round' % (rounds, variants[0][0])}
    for tag, _ in variants:
        out[tag] = round(float(np.median(per_round[tag])), 2)
        out[tag + '_spread'] = round(float(max(per_round[tag]) - min(per_round[tag])), 2)
        if tag != variants[0][0]:
            out[tag + '_surplus'] = [round(a - b, 2) for a, b in zip(per_round[tag], base)]
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
