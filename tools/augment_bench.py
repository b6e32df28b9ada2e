"""What flip / rotate augmentation from a scene atlas costs, in one process on the GPU:

    python tools/augment_bench.py [--steps K] [--reps R] [--out profiles/augment.md]

  (a) dmf_scene_atlas on the padded scenes of bench.py's configs[1] (145 x 145, 200 + 1 bands, patch 11) and configs[3] (512 x 512,
      224 + 3 bands) and of a 1024 x 1024 x 4 scene with a 1-band aux scene at S = 4 (4136 x 4136: the narrow-pixel regime at a
      size that outgrows the caches), primary scene fp32 and fp16, `flips` and `d4`: time per launch by device events around LAUNCHES back to
      back, and the bytes it has to move (every variant reads its source once, every byte of the atlas is written once) per
      second.  The yardstick is the same atlas composed by torch on the device (zeros, then flip / transpose copied into the
      slots), timed the same way; the two atlases are compared bit for bit first.
  (b) the train step at configs[1], batch 256, from captured graphs, with the plan of `augment: d4` on the atlas against the
      plain plan on the plain scene: the kernels are the same instructions, so the difference is what an 8 x larger resident
      scene does to cache residency.  The two engines alternate in the same run; wall clock around replays that end in a
      synchronise.
  (c) the whole-scene label map (every pixel, chunks of 16,384) with `tta: d4` against none, alternating likewise.
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

LAUNCHES = 20


def event_ms(fn, reps):
    """Milliseconds per call of fn: LAUNCHES calls between two device events, `reps` times after one untimed round."""
    for _ in range(LAUNCHES):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(LAUNCHES):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / LAUNCHES)
    return out


def torch_atlas(src, rows, cols, ops, R, dst):
    from dmf import augment
    dst.zero_()
    for s, k in enumerate(ops):
        Y = augment.tf(src[:rows, :cols], k)
        dst[s * R:s * R + Y.shape[0], :Y.shape[1]].copy_(Y)


def bench_atlas(reps):
    import bench
    from dmf import augment, lib
    rows_out = []
    # the two scenes asked for, and a 1-band 4096 x 4096 panchromatic-sized aux scene: the aux scenes of the two configs are
    # launch-sized, and the LDS tile path of the transposed variants shows its rate only on a scene that outgrows the caches
    for key, c in (('1', bench.CONFIGS['1']), ('3', bench.CONFIGS['3']),
                   ('pan', dict(patch=11, scale=4, size=1024, bands=4, aux_bands=1))):
        P, S = c['patch'], c['scale']
        Hp = c['size'] + P - 1
        for half in (False, True):
            A = torch.rand(Hp, Hp, c['bands'], device='cuda').to(torch.float16 if half else torch.float32)
            Bm = torch.rand(S * Hp + S - 1, S * Hp + S - 1, c['aux_bands'], device='cuda')
            for name in ('flips', 'd4'):
                ops = augment.OPS[name]
                for what, src, n in (('primary', A, Hp), ('aux', Bm, S * Hp)):
                    if what == 'aux' and half:
                        continue                                     # (the aux scene is fp32 either way)
                    R, Wq = augment.atlas_geometry(n, n, ops)
                    dst = torch.empty(len(ops) * R, Wq, src.shape[2], dtype=src.dtype, device='cuda')
                    ref = torch.empty_like(dst)
                    lib.scene_atlas(src, n, n, ops, R, dst)
                    torch_atlas(src, n, n, ops, R, ref)
                    bits = torch.int16 if src.element_size() == 2 else torch.int32
                    same = torch.equal(dst.view(bits), ref.view(bits))
                    t_k = event_ms(lambda: lib.scene_atlas(src, n, n, ops, R, dst), reps)
                    t_t = event_ms(lambda: torch_atlas(src, n, n, ops, R, ref), reps)
                    moved = (len(ops) * n * n + dst.shape[0] * dst.shape[1]) * src.shape[2] * src.element_size()
                    rows_out.append(dict(config='configs[%s]' % key if key.isdigit() else '4-band MS + PAN, S = 4', scene=what, dtype=str(src.dtype).split('.')[1], ops=name,
                                         shape=list(src.shape), atlas_mb=round(dst.numel() * dst.element_size() / 2**20, 1),
                                         kernel_ms=round(min(t_k), 4), kernel_ms_max=round(max(t_k), 4),
                                         kernel_gb_s=round(moved / (min(t_k) * 1e-3) / 1e9, 1),
                                         torch_ms=round(min(t_t), 4), torch_ms_max=round(max(t_t), 4),
                                         torch_gb_s=round(moved / (min(t_t) * 1e-3) / 1e9, 1), bit_identical=bool(same)))
                    del dst, ref
    return rows_out


def problem(key):
    import bench
    from model.gmfnet import Net
    args = types.SimpleNamespace(**dict(bench.CONFIGS[key], half=0, train_rate=0.10))
    cfg = bench.make_cfg(args)
    MS, PAN, xy, lab, train, test = bench.build_problem(args, cfg)
    torch.manual_seed(0)
    net = Net(cfg).to('cuda:0')
    return args, cfg, MS, PAN, xy, lab, train, net


def bench_step(steps, reps, spg=50):
    import bench
    from dmf import augment
    from dmf.engine import Scene, TrainEngine
    args, cfg, MS, PAN, xy, lab, train, net = problem('1')
    B = args.batch
    rows = bench.make_plan(train, steps, B, seed=1)
    plain = Scene(MS, PAN, 'cuda:0')
    atlas = Scene(MS, PAN, 'cuda:0').atlas(args.patch, args.scale, 'd4')
    slots = augment.draw_slots(123, 0, xy[rows], 8)
    from model.gmfnet import Net
    engines, plans = {}, {}
    labels = torch.from_numpy(lab[rows])
    for name, scene, plan in (('none', plain, xy[rows]), ('d4', atlas, atlas.map_xy(xy[rows], slots))):
        torch.manual_seed(0)
        eng = TrainEngine(Net(cfg).to('cuda:0'), scene, B, lr=1e-3)     # (a net of its own, from the same seed)
        plans[name] = torch.from_numpy(np.ascontiguousarray(plan))
        eng.load_plan(plans[name], labels)
        eng.run_plan(steps, spg)                                  # capture + warm-up of this engine's graph
        engines[name] = eng
    torch.cuda.synchronize()
    times = {k: [] for k in engines}
    for _ in range(reps):
        for name, eng in engines.items():                           # alternating, in the same run
            eng.load_plan(plans[name], labels)                      # (a plan is consumed by its steps; the upload is not timed)
            torch.cuda.synchronize()
            t = time.perf_counter()
            eng.run_plan(steps, spg)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t) / steps * 1e6)
    return dict(batch=B, steps=steps, steps_per_graph=spg, reps=reps,
                scene_mb={'none': round((plain.A.numel() * 4 + plain.B.numel() * 4) / 2**20, 1),
                          'd4': round((atlas.A.numel() * 4 + atlas.B.numel() * 4) / 2**20, 1)},
                step_us={k: dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3)) for k, v in times.items()})


def bench_label_map(reps):
    from dmf.engine import EvalEngine, Scene
    out = []
    for key in ('1', '3'):
        args, cfg, MS, PAN, xy, lab, train, net = problem(key)
        n = args.size
        pixels = np.stack(np.meshgrid(np.arange(n), np.arange(n), indexing='ij'), -1).reshape(-1, 2).astype(np.int32)
        atlas = Scene(MS, PAN, 'cuda:0').atlas(args.patch, args.scale, 'd4')
        engines = {'none': EvalEngine(net, atlas, 16384), 'd4': EvalEngine(net, atlas, 16384, tta='d4')}
        times = {k: [] for k in engines}
        for ev in engines.values():
            ev.label_map(pixels, n, n)                              # untimed: first launches
        for _ in range(reps):
            for name, ev in engines.items():
                torch.cuda.synchronize()
                t = time.perf_counter()
                ev.label_map(pixels, n, n)
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t) * 1e3)
        out.append(dict(config='configs[%s]' % key, pixels=len(pixels), chunk=16384,
                        label_map_ms={k: dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))
                                      for k, v in times.items()}))
        del atlas, engines
    return out


def table(rows):
    keys = list(rows[0])
    lines = ['| ' + ' | '.join(keys) + ' |', '|' + '---|' * len(keys)]
    return '\n'.join(lines + ['| ' + ' | '.join(str(r[k]) for k in keys) + ' |' for r in rows])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=2000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('augment_bench.py measures on the GPU; none found')
    torch.zeros(1, device='cuda')
    res = dict(command='python tools/augment_bench.py --steps %d --reps %d' % (args.steps, args.reps),
               atlas=bench_atlas(args.reps), step=bench_step(args.steps, args.reps), label_map=bench_label_map(args.reps))
    print(json.dumps(res))
    if args.out:
        d = os.path.dirname(args.out)
        if d:
            os.makedirs(d, exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('`%s`\n\n(a) dmf_scene_atlas against torch composing the same atlas (ms per launch, min and max of %d rounds of %d '
                    'launches; GB/s = bytes read + written over the min)\n\n' % (res['command'], args.reps, LAUNCHES))
            f.write(table(res['atlas']) + '\n\n(b) train step, configs[1], from graphs\n\n```\n' + json.dumps(res['step'], indent=1))
            f.write('\n```\n\n(c) whole-scene label map\n\n```\n' + json.dumps(res['label_map'], indent=1) + '\n```\n')
    if not all(r['bit_identical'] for r in res['atlas']):
        raise SystemExit('an atlas differs from torch\'s')


if __name__ == '__main__':
    main()
