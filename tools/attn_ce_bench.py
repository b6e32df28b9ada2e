"""Step time of the attention network's train step with a criterion (class weights + label smoothing, and focal) evaluated
inside the attention kernel (dmf_train_attn_fwd_bwd_ce), next to the plain attention step of the same process
and to the composition of the older entry points (route A: dmf_train_attn_fwd_bwd(labels) -> dmf_ce_loss ->
dmf_train_attn_fwd_bwd(dlogits) -> reduce + ADAM), all replayed from captured graphs (profiles/attn_criterion.md).

    python tools/attn_ce_bench.py [steps] [repeats] [batch]

Shape: BASELINE configs[2] (200-band HSI + 1-band SAR, 11x11 patches, 17 logits, cross-modal attention), batch 1024.  The variants
are timed in turn inside every repeat (alternated), so that a drift of the box moves all of them.  One JSON line.
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
from dmf.engine import Criterion, Scene, TrainEngine
from function.function import data_padding, data_padding_aux
from model.gmfnet import Net

SHAPE = dict(size=145, bands=200, patch=11, scale=1, classes=16)
SPG = 25


class Composed:
    """Route A on one fixed batch, SPG steps per captured graph: what a caller composed before the criterion was in the kernel."""

    def __init__(self, net, scene, B, xy, lab, spec, K):
        dev = scene.device
        self.net, self.shape, self.B = net, net.shape, B
        self.cr = Criterion(spec, K, dev)
        self.theta = net.flat_parameters()
        self.m, self.v = torch.zeros_like(self.theta), torch.zeros_like(self.theta)
        self.logits, self.dl = torch.empty(B, K, device=dev), torch.empty(B, K, device=dev)
        self.loss = torch.empty(B, device=dev)
        self.ws = torch.empty(lib.workspace_bytes(self.shape, B) // 4, device=dev)
        self.aws = torch.empty(lib.attn_train_workspace_bytes(self.shape, B), dtype=torch.uint8, device=dev)
        self.step_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        self.xy = torch.from_numpy(xy[:B]).to(dev)
        self.lab = torch.from_numpy(lab[:B]).to(dev)
        self.inp = lib.input_gather(self.shape, scene.A, scene.B, self.xy)
        self.graph = None

    def step(self):
        s, cr = self, self.cr
        lib.train_attn_fwd_bwd(s.shape, s.inp, s.theta, s.net.pool_w, s.lab, None, 1.0 / s.B, s.logits, None, s.ws, s.aws)
        lib.ce_loss(s.logits, 1, 0, s.lab, cr.params, class_w=cr.class_w, loss=s.loss, dlogits=s.dl)
        lib.train_attn_fwd_bwd(s.shape, s.inp, s.theta, s.net.pool_w, None, s.dl, 1.0, s.logits, None, s.ws, s.aws, adam_step_dev=s.step_dev)
        lib.grad_reduce_adam(s.shape, s.B, s.ws, s.theta, s.m, s.v, None, 1e-3, 0.9, 0.999, 1e-8, 1, adam_step_dev=s.step_dev)

    def run(self, steps):
        if self.graph is None:
            self.step()                                     # every kernel launched once before the capture
            torch.cuda.synchronize()
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                for _ in range(SPG):
                    self.step()
        for _ in range(steps // SPG):
            self.graph.replay()


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    B = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
    steps -= steps % SPG
    s = SHAPE
    K = s['classes'] + 1
    cfg = {'patch_size': s['patch'], 'Categories_Number': K, 'data_city': 's', 'DATA_DICT': {'s': {'size': [s['size'], s['size'], s['bands']]}},
           'scale': s['scale'], 'aux_bands': 1, 'gmf': {'width': 40, 'hidden': 64, 'pool_sigma': 2.5, 'attention': 1},
           'trans': {'embed_dim': 96, 'num_head': 3}}
    primary, aux, label = synth.make_scene(s['size'], s['size'], s['bands'], 1, s['scale'], n_classes=s['classes'], seed=0)
    scene = Scene(data_padding(primary, cfg, 'ms').astype(np.float32), data_padding_aux(aux, cfg).astype(np.float32), 'cuda:0')
    g = np.random.default_rng(1)
    xy = np.stack([g.integers(0, s['size'], steps * B), g.integers(0, s['size'], steps * B)], 1).astype(np.int32)
    lab = np.maximum(label[xy[:, 0], xy[:, 1]], 1).astype(np.int32)
    w = (1.0 / np.maximum(np.bincount(lab, minlength=K), 1)).astype(np.float64)
    w = (w / w.mean()).tolist()
    ce, focal = dict(kind='ce', label_smoothing=0.1, class_weights=w), dict(kind='focal', gamma=2.0, class_weights=w)
    runners = {}
    for tag, cr in (('plain', None), ('fused_weighted_smoothed_ce', ce), ('fused_weighted_focal_gamma2', focal)):
        torch.manual_seed(0)
        eng = TrainEngine(Net(cfg).cuda(), scene, B, lr=1e-3, criterion=cr, criterion_in_kernel=cr is not None)

        def run(n, eng=eng):
            eng.load_plan(xy, lab)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.run_plan(n, SPG)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / n * 1e6
        runners[tag] = run
    for tag, cr in (('composed_weighted_smoothed_ce', ce), ('composed_weighted_focal_gamma2', focal)):
        torch.manual_seed(0)
        comp = Composed(Net(cfg).cuda(), scene, B, xy, lab, cr, K)

        def run(n, comp=comp):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            comp.run(n)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / n * 1e6
        runners[tag] = run
    for run in runners.values():                            # capture + first replay: not timed
        run(SPG)
    times = {tag: [] for tag in runners}
    for _ in range(repeats):
        for tag, run in runners.items():
            times[tag].append(run(steps))
    res = {'shape': 'configs[2]', 'batch': B, 'steps': steps, 'steps_per_graph': SPG, 'repeats': repeats}
    for tag, v in times.items():
        res[tag + '_us_per_step'] = round(float(np.median(v)), 2)
        res[tag + '_runs'] = [round(x, 2) for x in v]
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
