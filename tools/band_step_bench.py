"""Train-step time of the 32-band row (32/1/11/1/40/2: `band_reduce: pca` at its default) next to the 200-band row
(200/1/11/1/40/10) on the same box, replayed from captured graphs (profiles/band_reduce.md).

    python tools/band_step_bench.py [steps] [repeats] [rounds] [half]

Scene: the synthetic 145 x 145 x 200 scene of BASELINE configs[1]; the 32-band engine trains on its first 32 principal components
(dmf.engine.band_reduce), so both engines gather from scenes of the same extent with the same coordinates.  Batch 256, graphs
of 50 steps, ADAM, one GPU; `half` = 1 keeps both primary scenes in fp16 (gmf.half).  The two engines alternate `rounds` times
inside one process, the 200-band one first in every round; every figure is the median of `repeats` timed runs of `steps` steps
after an untimed capture and first replay.  One JSON line per round and a last one with the medians over the rounds."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'dual-modal-fusion_amd'), ROOT]
from dmf import synth
from dmf.engine import Scene, TrainEngine, band_reduce
from function.function import data_padding, data_padding_aux
from model.gmfnet import Net
from optim_step_bench import B, SHAPE, SPG, step_time


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 500
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    half = bool(int(sys.argv[4])) if len(sys.argv) > 4 else False
    steps -= steps % SPG
    s = SHAPE
    K = s['classes'] + 1
    base = {'patch_size': s['patch'], 'Categories_Number': K, 'data_city': 's', 'DATA_DICT': {'s': {'size': [s['size'], s['size'], s['bands']]}},
            'scale': s['scale'], 'aux_bands': 1, 'gmf': {'width': 40, 'hidden': 64, 'pool_sigma': 2.5, 'attention': 0, 'half': int(half)}}
    primary, aux, label = synth.make_scene(s['size'], s['size'], s['bands'], 1, s['scale'], n_classes=s['classes'], seed=0)
    reduced, fit = band_reduce(primary, 32, False, 'cuda:0')
    PAN = data_padding_aux(aux, base).astype(np.float32)
    g = np.random.default_rng(1)
    xy = np.stack([g.integers(0, s['size'], steps * B), g.integers(0, s['size'], steps * B)], 1).astype(np.int32)
    lab = np.maximum(label[xy[:, 0], xy[:, 1]], 1).astype(np.int32)
    engines = {}
    for tag, cfg, ms in (('bands200', base, primary), ('bands32', dict(base, band_reduce='pca', band_reduce_bands=32), reduced)):
        torch.manual_seed(0)
        scene = Scene(data_padding(ms, cfg, 'ms').astype(np.float32), PAN, 'cuda:0', half=half)
        engines[tag] = TrainEngine(Net(cfg).cuda(), scene, B, lr=1e-3)
    per_round = {tag: [] for tag in engines}
    for r in range(rounds):
        res = {'round': r, 'batch': B, 'steps': steps, 'steps_per_graph': SPG, 'repeats': repeats, 'half': int(half)}
        for tag, eng in engines.items():
            med, runs = step_time(eng, xy, lab, steps, repeats)
            per_round[tag].append(med)
            res[tag + '_us_per_step'] = round(med, 2)
            res[tag + '_runs'] = runs
        print(json.dumps(res), flush=True)
    out = {'summary': 'median over %d rounds (us per step)' % rounds, 'half': int(half),
           'explained_variance_32': round(float(fit['explained'].sum()), 4)}
    for tag in engines:
        out[tag] = round(float(np.median(per_round[tag])), 2)
        out[tag + '_spread'] = round(float(max(per_round[tag]) - min(per_round[tag])), 2)
    out['ratio_200_over_32'] = round(out['bands200'] / out['bands32'], 3)
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
