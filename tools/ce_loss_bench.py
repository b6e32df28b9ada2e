"""Step time of the criterion step (class weights + label smoothing, and focal: dmf_forward_unit -> dmf_ce_loss ->
dmf_backward_unit -> reduce + ADAM) next to the fused default step of the same process, both replayed from captured graphs, and
the dmf_ce_loss launch alone by HIP events around groups of replayed launches (profiles/ce_loss.md).

    python tools/ce_loss_bench.py [steps] [repeats]

Shapes: BASELINE configs[1] (200-band HSI + 1-band SAR, 11x11 patches, 17 logits) and the reference's PAN/MS shape (4-band MS +
PAN at 4x, 16x16 patches, 12 logits), batch 256.  One JSON line per shape.
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'dual-modal-fusion_amd'), ROOT]
from dmf import lib, synth
from dmf.engine import Scene, TrainEngine
from function.function import data_padding, data_padding_aux
from model.gmfnet import Net

SHAPES = {'configs[1]': dict(size=145, bands=200, patch=11, scale=1, classes=16),
          'panms': dict(size=256, bands=4, patch=16, scale=4, classes=11)}
B, SPG, GROUP = 256, 50, 50


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


def loss_launch_time(eng, lab, repeats):
    """dmf_ce_loss alone: HIP events around GROUP launches replayed from a graph, as bench.py times its kernel (us)."""
    cr = eng.criterion
    labd = torch.from_numpy(lab[:B]).to(eng.scene.device)
    logits = torch.randn(B, eng.logits.shape[1], device=eng.scene.device)

    def group():
        for _ in range(GROUP):
            lib.ce_loss(logits, 1, 0, labd, cr.params, class_w=cr.class_w, loss=eng.loss, dlogits=eng.dlogits)
    group()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        group()
    g.replay()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(max(repeats, 2))]
    torch.cuda.synchronize()
    for a, b in ev:
        a.record(); g.replay(); b.record()
    torch.cuda.synchronize()
    return float(np.mean([a.elapsed_time(b) / GROUP for a, b in ev]) * 1e3)


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 500
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    steps -= steps % SPG
    for name, s in SHAPES.items():
        K = s['classes'] + 1
        cfg = {'patch_size': s['patch'], 'Categories_Number': K, 'data_city': 's', 'DATA_DICT': {'s': {'size': [s['size'], s['size'], s['bands']]}},
               'scale': s['scale'], 'aux_bands': 1, 'gmf': {'width': 40, 'hidden': 64, 'pool_sigma': 2.5, 'attention': 0}}
        primary, aux, label = synth.make_scene(s['size'], s['size'], s['bands'], 1, s['scale'], n_classes=s['classes'], seed=0)
        scene = Scene(data_padding(primary, cfg, 'ms').astype(np.float32), data_padding_aux(aux, cfg).astype(np.float32), 'cuda:0')
        g = np.random.default_rng(1)
        xy = np.stack([g.integers(0, s['size'], steps * B), g.integers(0, s['size'], steps * B)], 1).astype(np.int32)
        lab = np.maximum(label[xy[:, 0], xy[:, 1]], 1).astype(np.int32)
        w = (1.0 / np.maximum(np.bincount(lab, minlength=K), 1)).astype(np.float64)
        w = (w / w.mean()).tolist()
        res = {'shape': name, 'batch': B, 'steps': steps, 'steps_per_graph': SPG, 'repeats': repeats}
        for tag, cr in (('fused_default', None), ('weighted_smoothed_ce', dict(kind='ce', label_smoothing=0.1, class_weights=w)),
                        ('weighted_focal_gamma2', dict(kind='focal', gamma=2.0, class_weights=w))):
            torch.manual_seed(0)
            eng = TrainEngine(Net(cfg).cuda(), scene, B, lr=1e-3, criterion=cr)
            med, runs = step_time(eng, xy, lab, steps, repeats)
            res[tag + '_us_per_step'] = round(med, 2)
            res[tag + '_runs'] = runs
            if cr is not None:
                res[tag + '_loss_launch_us'] = round(loss_launch_time(eng, lab, repeats), 2)
        print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
