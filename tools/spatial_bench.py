"""What the spatial regularisation costs, in one process on the GPU:

    python tools/spatial_bench.py [--reps R] [--out profiles/spatial.md]

  (a) dmf_spatial_affinity, dmf_prob_scatter and dmf_spatial_filter at the scenes of bench.py's configs[1] (145 x 145, 200 bands)
      and configs[3] (512 x 512, 224 bands), K = 17, r = 2 and 3, fp32 and (affinity) fp16 scene: time per launch by device events
      around LAUNCHES launches back to back, the bytes the kernel has to move (computed from the shapes below: `moved`) and the
      share of the HBM roof those bytes give (ROOF: the measured float4-copy rate of the part, not the datasheet's).  The
      yardstick is torch composing the same result on the same device (shifted slices; softmax + index_put), timed the same
      way, kernel and torch alternating in every round; the results are compared first.  No threshold is set: a row where the
      kernel loses says so in its `kernel_vs_torch` column (< 1 is a loss).
  (b) what `test.spatial: bilateral` adds to a whole-split test() on those two configs: the confusion pass over the test split
      (what test() does anyway) against the whole-scene probability map + affinity + filter that the keys add, wall clock around
      work that ends in a synchronise, alternating.
  (c) `Solver.test()` itself (whole split) on a solver trained for one epoch on each of the two synthetic scenes, with and without
      `test.spatial: bilateral`, alternating on the same solver: wall clock of the whole call (weights file, loaders, indicator()
      and its export included on both sides).
Needs the GPU: there is no CPU statement of a time.  Prints one JSON line; --out also writes the tables as markdown.
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, 'dual-modal-fusion_amd'), REPO]

LAUNCHES = 10
ROOF = 6.29e12           # bytes / s: the float4 copy rate measured on an MI355X (8.0e12 on the datasheet)
K = 17
SIGMA_S, SIGMA_R = 2.0, 0.1


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(LAUNCHES):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / LAUNCHES


def alternate(fns, reps):
    """{name: [ms per call, per round]}: one untimed round of every fn, then `reps` rounds in which they alternate."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            out[k].append(event_ms(fn))
    return out


def window(r):
    return [(di, dj) for di in range(-r, r + 1) for dj in range(-r, r + 1)]


def _shift(t, di, dj):
    """(slices of the destination, slices of the source) of t shifted by (di, dj) inside [H, W]."""
    H, W = t.shape[:2]
    i0, i1, j0, j1 = max(0, -di), min(H, H - di), max(0, -dj), min(W, W - dj)
    return (slice(i0, i1), slice(j0, j1)), (slice(i0 + di, i1 + di), slice(j0 + dj, j1 + dj))


def torch_affinity(scene, H, W, r, aff):
    a = scene[:H, :W].float()
    cs, cr = 1.0 / (2 * SIGMA_S ** 2), 1.0 / (2 * SIGMA_R ** 2)
    aff.zero_()
    for k, (di, dj) in enumerate(window(r)):
        d, s = _shift(a, di, dj)
        d2 = (a[d] - a[s]).square_().sum(2) / a.shape[2]
        aff[d[0], d[1], k] = torch.exp(-((di * di + dj * dj) * cs + d2 * cr))


def torch_scatter(logits, xy, prob, mask):
    prob[xy[:, 0].long(), xy[:, 1].long()] = torch.softmax(logits, 1)
    mask[xy[:, 0].long(), xy[:, 1].long()] = 1


def torch_filter(prob, mask, aff, r, out, label):
    m = mask.float()
    p = prob * m[:, :, None]
    num, den = torch.zeros_like(prob), torch.zeros_like(m)
    for k, (di, dj) in enumerate(window(r)):
        d, s = _shift(m, di, dj)
        w = aff[d[0], d[1], k] * m[s]
        num[d] += w[:, :, None] * p[s]
        den[d] += w
    out.copy_(torch.where(mask[:, :, None] != 0, num / den.clamp_min(1e-30)[:, :, None], torch.zeros_like(num)))
    label.copy_(torch.where(mask != 0, out.argmax(2).int(), label))


def bench_kernels(reps):
    import bench
    from dmf import lib
    rows = []
    for key in ('1', '3'):
        c = bench.CONFIGS[key]
        H = W = c['size']
        Cn = c['bands']
        pad = c['patch'] - 1
        g = torch.Generator(device='cuda').manual_seed(int(key))
        base = torch.rand(H + pad, W + pad, Cn, device='cuda', generator=g)
        logits = 3.0 * torch.randn(H * W, K, device='cuda', generator=g)
        xy = torch.stack(torch.meshgrid(torch.arange(H), torch.arange(W), indexing='ij'), 2).reshape(-1, 2).int().cuda()
        for r in (2, 3):
            n = (2 * r + 1) ** 2
            aff = torch.empty(H, W, n, device='cuda')
            ref = torch.empty_like(aff)
            for half in (False, True):
                scene = base.half() if half else base
                lib.spatial_affinity(scene, H, W, r, SIGMA_S, SIGMA_R, aff)
                torch_affinity(scene, H, W, r, ref)
                err = float((aff - ref).abs().max())
                t = alternate({'kernel': lambda: lib.spatial_affinity(scene, H, W, r, SIGMA_S, SIGMA_R, aff),
                               'torch': lambda: torch_affinity(scene, H, W, r, ref)}, reps)
                moved = H * W * Cn * scene.element_size() + H * W * n * 4
                rows.append(row('affinity', key, H, W, Cn, 'fp16' if half else 'fp32', r, moved, t, err))
            lib.spatial_affinity(base, H, W, r, SIGMA_S, SIGMA_R, aff)
            if r == 2:
                prob, mask = torch.zeros(H, W, K, device='cuda'), torch.zeros(H, W, dtype=torch.uint8, device='cuda')
                prob_t, mask_t = torch.zeros_like(prob), torch.zeros_like(mask)
                lib.prob_scatter(logits, xy, W, prob, mask)
                torch_scatter(logits, xy, prob_t, mask_t)
                err = float((prob - prob_t).abs().max())
                t = alternate({'kernel': lambda: lib.prob_scatter(logits, xy, W, prob, mask),
                               'torch': lambda: torch_scatter(logits, xy, prob_t, mask_t)}, reps)
                rows.append(row('scatter', key, H, W, Cn, 'fp32', '-', H * W * (2 * K * 4 + 8 + 1), t, err))
            out, out_t = torch.empty_like(prob), torch.empty_like(prob)
            label, label_t = (torch.zeros(H, W, dtype=torch.int32, device='cuda') for _ in range(2))
            lib.spatial_filter(prob, mask, aff, out, label)
            torch_filter(prob, mask, aff, r, out_t, label_t)
            err = float((out - out_t).abs().max())
            t = alternate({'kernel': lambda: lib.spatial_filter(prob, mask, aff, out, label),
                           'torch': lambda: torch_filter(prob, mask, aff, r, out_t, label_t)}, reps)
            rows.append(row('filter', key, H, W, Cn, 'fp32', r, H * W * (K * 4 + n * 4 + 1 + K * 4 + 4), t, err))
        del base, logits
    return rows


def row(kernel, key, H, W, Cn, dtype, r, moved, t, err):
    k, tt = min(t['kernel']), min(t['torch'])
    return dict(kernel=kernel, config='configs[%s]' % key, scene='%d x %d x %d' % (H, W, Cn), dtype=dtype, r=r,
                moved_mb=round(moved / 1e6, 2), kernel_ms=round(k, 4), kernel_ms_max=round(max(t['kernel']), 4),
                kernel_gb_s=round(moved / (k * 1e-3) / 1e9, 1), hbm_roof_share=round(moved / (k * 1e-3) / ROOF, 4),
                torch_ms=round(tt, 4), torch_ms_max=round(max(t['torch']), 4), kernel_vs_torch=round(tt / k, 2),
                max_abs_diff=float('%.2e' % err))


def bench_test_pass(reps):
    """The engine passes of test(): the confusion matrix over the test split, and what the keys add over the whole scene."""
    import bench
    from dmf.engine import EvalEngine, Scene
    from model.gmfnet import Net
    out = []
    for key in ('1', '3'):
        args = types.SimpleNamespace(**dict(bench.CONFIGS[key], half=0, train_rate=0.10))
        cfg = bench.make_cfg(args)
        MS, PAN, xy, lab, train, test = bench.build_problem(args, cfg)
        torch.manual_seed(0)
        net = Net(cfg).to('cuda:0')
        scene = Scene(MS, PAN, 'cuda:0')
        n = args.size
        ev = EvalEngine(net, scene, 16384)
        pixels = np.stack(np.meshgrid(np.arange(n), np.arange(n), indexing='ij'), -1).reshape(-1, 2).astype(np.int32)
        txy, tlab = xy[test], lab[test].astype(np.int32)

        def plain():
            ev.confusion(txy, tlab)

        def added():
            scene._affinity = None                       # (a first test(): the affinities are not there yet)
            prob, mask = ev.probability_map(pixels, n, n)
            ev.regularise(prob, mask, scene.affinity(n, n, 2, SIGMA_S, SIGMA_R), 1)
        times = {'test_split_confusion': [], 'spatial_keys_add': []}
        plain(); added()
        for _ in range(reps):
            for name, fn in (('test_split_confusion', plain), ('spatial_keys_add', added)):
                torch.cuda.synchronize()
                t = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t) * 1e3)
        out.append(dict(config='configs[%s]' % key, test_pixels=int(len(txy)), scene_pixels=int(len(pixels)), r=2,
                        aff_mb=round(n * n * 25 * 4 / 1e6, 1),
                        ms={k: dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))
                            for k, v in times.items()}))
        del scene, ev
    return out


def bench_solver_test(reps):
    """`Solver.test()` itself, whole split (`test.full: 1`), with and without `test.spatial: bilateral` on one trained solver, the
    two alternating; every timed call with the keys starts without the affinities and the regularised map (a first test())."""
    import contextlib
    import io
    import shutil
    import tempfile
    import bench
    from dmf import synth
    from solver.mainsolver import Solver
    from utils import spatial
    out = []
    for key in ('1', '3'):
        args = types.SimpleNamespace(**dict(bench.CONFIGS[key], half=0))
        tmp = tempfile.mkdtemp(prefix='dmf_spatial_bench_')
        try:
            d = os.path.join(tmp, 'scene') + '/'
            os.makedirs(d)
            os.makedirs(os.path.join(tmp, 'out'))
            primary, aux, label = synth.make_scene(args.size, args.size, args.bands, args.aux_bands, args.scale, n_classes=args.classes, seed=0)
            np.save(d + 'ms4.tif.npy', primary); np.save(d + 'pan.tif.npy', aux); np.save(d + 'label.npy', label)
            cfg = dict(bench.make_cfg(args), task='classification', nohup=1, model_name='gmfnet', time=1, index=0, epoch=1, device='cuda:0',
                       gpu_mode=False, batchsize=256, test_batchsize=4096, color_batchsize=4096, train_rate=0.02, verify_rate=0.01, data_new=0,
                       schedule=dict(loss='Criterion', optimizer='ADAM', if_scheduler=0, scheduler='ExponentialLR', activate='Relu', lr=1e-3,
                                     base_lr=5e-4),
                       train=dict(index=1, pretrained=0, save_best=True), test=dict(index=1, save_matrix=0, full=1),
                       color=dict(index=0, supervised=1, unsupervised=1), data_address=d, RESULT_output=os.path.join(tmp, 'out') + '/',
                       RESULT_excel=os.path.join(tmp, 'r.xlsx'))
            keys = {False: spatial.spatial_keys(cfg), True: spatial.spatial_keys(dict(cfg, test=dict(cfg['test'], spatial='bilateral')))}
            times = {False: [], True: []}
            with contextlib.redirect_stdout(io.StringIO()):
                torch.manual_seed(3407)
                s = Solver(cfg)
                s.dataloader()
                s.train()
                for on in (False, True) * (reps + 1):                     # (the first round is not kept)
                    s.spat, s._spatial_maps, s.scene._affinity = keys[on], None, None
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    s.test()
                    torch.cuda.synchronize()
                    times[on].append((time.perf_counter() - t) * 1e3)
            out.append(dict(config='configs[%s]' % key, test_pixels=int(s.test_matrix.sum()), scene_pixels=args.size ** 2, r=2,
                            changed=s.spatial['changed'],
                            test_ms={name: dict(median=round(statistics.median(v[1:]), 2), min=round(min(v[1:]), 2), max=round(max(v[1:]), 2))
                                     for name, v in (('without_keys', times[False]), ('with_keys', times[True]))}))
        finally:
            shutil.rmtree(tmp)
    return out


def table(rows):
    keys = list(rows[0])
    lines = ['| ' + ' | '.join(keys) + ' |', '|' + '---|' * len(keys)]
    return '\n'.join(lines + ['| ' + ' | '.join(str(r[k]) for k in keys) + ' |' for r in rows])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('spatial_bench.py measures on the GPU; none found')
    torch.zeros(1, device='cuda')
    res = dict(command='python tools/spatial_bench.py --reps %d' % args.reps, kernels=bench_kernels(args.reps),
               test_pass=bench_test_pass(args.reps), solver_test=bench_solver_test(args.reps))
    print(json.dumps(res))
    if args.out:
        d = os.path.dirname(args.out)
        if d:
            os.makedirs(d, exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('`%s`\n\n(a) the three kernels against torch composing the same result (ms per launch: min and max of %d alternated '
                    'rounds of %d launches; moved = the bytes the kernel must read and write, GB/s and the share of the %.2f TB/s '
                    'HBM copy roof over the min; kernel_vs_torch = torch_ms / kernel_ms)\n\n'
                    % (res['command'], args.reps, LAUNCHES, ROOF / 1e12))
            f.write(table(res['kernels']) + '\n\n(b) what the keys add to a whole-split test(), K = 17, r = 2\n\n```\n'
                    + json.dumps(res['test_pass'], indent=1) + '\n```\n\n(c) Solver.test() on the whole split, with and without the keys (ms, wall)'
                    '\n\n```\n' + json.dumps(res['solver_test'], indent=1) + '\n```\n')


if __name__ == '__main__':
    main()
