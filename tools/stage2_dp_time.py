"""Per-step time of the data-parallel form of the stage-2 step on a ONE-rank RCCL group (`_force_collective`: all-gather,
dmf_qua_loss_ranks, backward, dmf_grad_reduce, all-reduce, ADAM), eager and replayed from hipGraphs, next to the
single-GPU unit step, at bs = 256 pixels = 1,024 stacked 16 x 16 x 4 patches.  HIP events around >= 1,000 steps after a
warm-up; one line per form.

    python tools/stage2_dp_time.py [--steps 1000] [--warmup 100] [--graph 50] [--scaler 0|1]
"""
import argparse
import datetime
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'dual-modal-fusion_amd'), ROOT]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=1000)
    ap.add_argument('--warmup', type=int, default=100)
    ap.add_argument('--graph', type=int, default=50)
    ap.add_argument('--scaler', type=int, default=0)
    args = ap.parse_args()
    import torch.distributed as dist
    from dmf import synth
    from dmf.engine import LossScaler, QuaScene, QuaTrainEngine
    from function.function import data_padding
    from model.gmfnet import Net
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29731')
    torch.cuda.set_device(0)
    dist.init_process_group('nccl', rank=0, world_size=1, timeout=datetime.timedelta(seconds=120),
                            device_id=torch.device('cuda', 0))
    H = W = 128
    bs = 256
    cfg = {'patch_size': 16, 'Categories_Number': 13, 'data_city': 's', 'DATA_DICT': {'s': {'size': [H, W, 4]}},
           'gmf': {'width': 40, 'single_input': 1, 'half': int(bool(args.scaler))}}
    dqtl = {'alpha': 0.1, 'beta': 0.05, 'gamma': 1.0, 'epsilon': 1e-8, 'tao': 0.1}
    ms, _, label = synth.make_scene(H, W, 4, 1, 1, n_classes=12, seed=0)
    g = np.random.default_rng(1)
    scenes = [data_padding(x, cfg, 'ms') for x in (ms, ms[::-1].copy(), ms + 0.1 * g.standard_normal(ms.shape), ms * 0.5)]
    n = args.warmup + args.steps
    xy = np.stack([g.integers(0, H, n * bs), g.integers(0, W, n * bs)], 1).astype(np.int32)
    lab = np.maximum(label[xy[:, 0], xy[:, 1]], 1).astype(np.int32)
    scene = QuaScene(scenes, 'cuda:0', half=bool(args.scaler))
    rows = []
    for name, forced, spg in (('single-GPU unit step, graphs of %d' % args.graph, False, args.graph),
                              ('single-GPU unit step, eager', False, 0),
                              ('one-rank RCCL form, eager', True, 0),
                              ('one-rank RCCL form, graphs of %d' % args.graph, True, args.graph)):
        torch.manual_seed(0)
        net = Net(cfg).to('cuda:0')
        sc = LossScaler('cuda:0') if args.scaler else None
        eng = QuaTrainEngine(net, scene, bs, dqtl, lr=1e-3, process_group=dist.group.WORLD if forced else None, scaler=sc)
        eng._force_collective = forced
        eng.load_plan(xy, lab)
        eng.run_plan(args.warmup, spg)
        if spg and eng.graph is None:
            raise SystemExit('%s: the step was not captured' % name)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng.run_plan(args.steps, spg)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / args.steps
        loss = float(eng.losses()[-1])
        rows.append((name, us, loss))
        print('%-42s %8.2f us per step  (%d steps, last loss %.6f)' % (name, us, args.steps, loss), flush=True)
        del eng
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
