"""Step time of weight averaging (profiles/weight_average.md): the fused step without averaging
(dmf_train_fwd_bwd + dmf_grad_reduce_adam), with the fused AVG instance (dmf_grad_reduce_adam_avg), and followed by the
stand-alone launch (dmf_grad_reduce_adam, then dmf_weight_average: what averaging costs as a kernel of its own); and the
dmf_optim_step route (dmf_train_fwd_bwd + dmf_grad_reduce + dmf_optim_step; ADAMW with weight_decay 0, which is ADAM's arithmetic
on that route) without and with averaging (dmf_optim_step_avg).  All replayed from captured graphs.

    python tools/avg_step_bench.py [steps] [repeats] [rounds] [variants]

Shape: BASELINE configs[1] (200-band HSI + 1-band SAR, 11x11 patches, 17 logits), batch 256, graphs of 50 steps, one GPU.
The variants alternate `rounds` times (default 5) inside one process, the plain form first, so that clock and thermal drift hits
them alike; every figure is the median of `repeats` timed runs of `steps` steps after an untimed capture and first replay.
Averaging is EMA with decay 0.999 from step 1.  One JSON line per round and a last one with the medians over the rounds, the
spread of every variant over the rounds, and the surplus of every averaging variant over its plain twin per round.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'dual-modal-fusion_amd'), ROOT, os.path.join(ROOT, 'tools')]
from dmf import lib, synth
from dmf.engine import Scene, TrainEngine
from function.function import data_padding, data_padding_aux
from model.gmfnet import Net
from optim_step_bench import B, SHAPE, SPG, step_time


class StandAloneAverage(TrainEngine):
    """The step as it is without averaging, followed by dmf_weight_average."""

    def _update(self, rows, dev_step, cursor, sum_scale, loss=None, loss_hist=None):
        w, self.wavg = self.wavg, None
        try:
            super()._update(rows, dev_step, cursor, sum_scale, loss, loss_hist)
        finally:
            self.wavg = w
        lib.weight_average(w, self.theta, self.step_count, step_dev=dev_step)


FUSED, ROUTE = dict(optimizer='ADAM', lr=1e-3), dict(optimizer='ADAMW', lr=1e-3, weight_decay=0.0)
# (tag, engine class, engine keys, averaging on, the plain twin)
VARIANTS = (('fused_plain', TrainEngine, FUSED, False, None),
            ('fused_avg', TrainEngine, FUSED, True, 'fused_plain'),
            ('fused_then_stand_alone', StandAloneAverage, FUSED, True, 'fused_plain'),
            ('optim_step_plain', TrainEngine, ROUTE, False, None),
            ('optim_step_avg', TrainEngine, ROUTE, True, 'optim_step_plain'))


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
    for tag, cls, kw, averaging, _ in variants:
        torch.manual_seed(0)
        engines[tag] = cls(Net(cfg).cuda(), scene, B, **kw)
        if averaging:
            engines[tag].set_averaging('ema', 0.999, 1)
    per_round = {v[0]: [] for v in variants}
    for r in range(rounds):
        res = {'round': r, 'shape': 'configs[1]', 'batch': B, 'steps': steps, 'steps_per_graph': SPG, 'repeats': repeats}
        for tag in per_round:
            med, runs = step_time(engines[tag], xy, lab, steps, repeats)
            per_round[tag].append(med)
            res[tag + '_us_per_step'] = round(med, 2)
            res[tag + '_runs'] = runs
        print(json.dumps(res), flush=True)
    out = {'summary': 'median over %d rounds (us per step); spread = max - min over the rounds; surplus = averaging variant - its '
                      'plain twin, per round' % rounds}
    for tag, _, _, _, twin in variants:
        out[tag] = round(float(np.median(per_round[tag])), 2)
        out[tag + '_spread'] = round(float(max(per_round[tag]) - min(per_round[tag])), 2)
        if twin in per_round:
            out[tag + '_surplus'] = [round(a - b, 2) for a, b in zip(per_round[tag], per_round[twin])]
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
