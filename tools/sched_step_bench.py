"""Step time of the schedule instances next to the launch-argument instances of the same two kernels (DESIGN.md §15,
profiles/device_schedule.md): the fused step (dmf_train_fwd_bwd + dmf_grad_reduce_adam against dmf_grad_reduce_adam_sched) and
the dmf_optim_step route (dmf_train_fwd_bwd + dmf_grad_reduce + dmf_optim_step against dmf_optim_step_sched; ADAMW with
weight_decay 0, which is ADAM's arithmetic on that route), all replayed from captured graphs.

    python tools/sched_step_bench.py [steps] [repeats] [rounds] [variants]

Shape: BASELINE configs[1] (200-band HSI + 1-band SAR, 11x11 patches, 17 logits), batch 256, graphs of 50 steps, one GPU.
The variants alternate `rounds` times (default 5) inside one process, the launch-argument form first, so that clock and thermal
drift hits them alike; every figure is the median of `repeats` timed runs of `steps` steps after an untimed capture and first
replay.  The schedule variants read a 64-row ExponentialLR table, unit `epoch` (a device row index) and unit `step` (the row
from the step count, clamped at the table's end).  One JSON line per round and a last one with the medians over the rounds, the
spread of every variant over the rounds, and the surplus of every schedule variant over its launch-argument twin per round.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'dual-modal-fusion_amd'), ROOT, os.path.join(ROOT, 'tools')]
from dmf import synth
from dmf.engine import Scene, TrainEngine
from function.function import data_padding, data_padding_aux
from model.gmfnet import Net
from optim_step_bench import B, SHAPE, SPG, step_time

FUSED, ROUTE = dict(optimizer='ADAM', lr=1e-3), dict(optimizer='ADAMW', lr=1e-3, weight_decay=0.0)
# (tag, engine keys, schedule unit or None, the launch-argument twin)
VARIANTS = (('fused_launch_args', FUSED, None, None),
            ('fused_sched_epoch', FUSED, 'epoch', 'fused_launch_args'),
            ('fused_sched_step', FUSED, 'step', 'fused_launch_args'),
            ('optim_step_launch_args', ROUTE, None, None),
            ('optim_step_sched_epoch', ROUTE, 'epoch', 'optim_step_launch_args'),
            ('optim_step_sched_step', ROUTE, 'step', 'optim_step_launch_args'))


def table(rows=64, lr=1e-3, gamma=0.98):
    return np.array([[lr * gamma ** r, 0.9, 0.999, 0.0] for r in range(rows)], dtype=np.float32)


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 500
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    only = sys.argv[4].split(',') if len(sys.argv) > 4 else [v[0] for v in VARIANTS]
    variants = [v for v in VARIANTS if v[0] in only]
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
    for tag, kw, unit, _ in variants:
        torch.manual_seed(0)
        engines[tag] = TrainEngine(Net(cfg).cuda(), scene, B, **kw)
        if unit is not None:
            engines[tag].set_schedule(table(), unit)
            engines[tag].set_epoch(3)
    per_round = {v[0]: [] for v in variants}
    for r in range(rounds):
        res = {'round': r, 'shape': 'configs[1]', 'batch': B, 'steps': steps, 'steps_per_graph': SPG, 'repeats': repeats}
        for tag, _, _, _ in variants:
            med, runs = step_time(engines[tag], xy, lab, steps, repeats)
            per_round[tag].append(med)
            res[tag + '_us_per_step'] = round(med, 2)
            res[tag + '_runs'] = runs
        print(json.dumps(res), flush=True)
    out = {'summary': 'median over %d rounds (us per step); spread = max - min over the rounds; surplus = schedule variant - its '
                      'launch-argument twin, per round' % rounds}
    for tag, _, _, twin in variants:
        out[tag] = round(float(np.median(per_round[tag])), 2)
        out[tag + '_spread'] = round(float(max(per_round[tag]) - min(per_round[tag])), 2)
        if twin in per_round:
            out[tag + '_surplus'] = [round(a - b, 2) for a, b in zip(per_round[tag], per_round[twin])]
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
