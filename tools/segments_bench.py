"""What the superpixel voting costs, in one process on the GPU:

    python tools/segments_bench.py [--reps R] [--out profiles/segments.md]

  (a) one SLIC iteration (dmf_slic_assign + dmf_slic_update) and dmf_segment_vote (mean and majority) at the scenes of bench.py's
      configs[1] (145 x 145, 200 bands) and configs[3] (512 x 512, 224 bands), S = 8, K = 17, fp32 and (the iteration) fp16 scene:
      time per call by device events around LAUNCHES calls back to back, the bytes the kernels have to move (computed from the
      shapes below: `moved`) and the share of the HBM roof those bytes give (ROOF: the measured float4-copy rate of the part, not
      the datasheet's).  The yardstick is torch composing the same arithmetic on the same device (nine masked distance maps and an
      argmin; `index_add_` sums), timed the same way, kernel and torch alternating in every round; the results are compared first.
      No threshold is set: a row where the kernel loses says so in its `kernel_vs_torch` column (< 1 is a loss).
  (b) what `test.segments: slic` adds to a whole-split test() on those two configs: the confusion pass over the test split (what
      test() does anyway) against the whole-scene probability map + ten iterations + the vote that the keys add, wall clock around
      work that ends in a synchronise, alternating.
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
K, S, COMPACTNESS = 17, 8, 0.1


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


def candidates(H, W):
    """(cand [9, H, W] int64 (0 where invalid), valid [9, H, W] bool) on the device."""
    gh, gw = (H + S - 1) // S, (W + S - 1) // S
    gi, gj = torch.arange(H, device='cuda')[:, None] // S, torch.arange(W, device='cuda')[None, :] // S
    cand, valid = [], []
    for u in (-1, 0, 1):
        for v in (-1, 0, 1):
            ok = (gi + u >= 0) & (gi + u < gh) & (gj + v >= 0) & (gj + v < gw)
            valid.append(ok)
            cand.append(torch.where(ok, (gi + u) * gw + gj + v, torch.zeros_like(gi + gj)))
    return torch.stack(cand), torch.stack(valid)


def torch_assign(a, centres, cand, valid, seg):
    H, W, Cn = a.shape
    cw = float(np.float32((COMPACTNESS / S) ** 2))
    ii, jj = torch.arange(H, device='cuda', dtype=torch.float32)[:, None], torch.arange(W, device='cuda', dtype=torch.float32)[None, :]
    D = torch.full((9, H, W), float('inf'), device='cuda')
    for s in range(9):
        mu = centres[cand[s]]
        d2 = (a - mu[:, :, :Cn]).square_().sum(2) / Cn
        sp = (ii - mu[:, :, Cn]).square() + (jj - mu[:, :, Cn + 1]).square()
        D[s] = torch.where(valid[s], d2 + cw * sp, D[s])
    seg.copy_(cand.gather(0, D.argmin(0)[None])[0])


def torch_update(a, seg, centres, counts):
    H, W, Cn = a.shape
    ii, jj = torch.meshgrid(torch.arange(H, device='cuda', dtype=torch.float32), torch.arange(W, device='cuda', dtype=torch.float32), indexing='ij')
    rows = torch.cat([a.reshape(-1, Cn), ii.reshape(-1, 1), jj.reshape(-1, 1)], 1)
    flat = seg.reshape(-1).long()
    sums = torch.zeros_like(centres).index_add_(0, flat, rows)
    n = torch.bincount(flat, minlength=centres.shape[0])
    counts.copy_(n)
    centres.copy_(torch.where(n[:, None] > 0, sums / n.clamp_min(1)[:, None], centres))


def torch_vote(prob, mask, seg, mode, segprob, segcount, label):
    m = mask != 0
    flat = seg[m].long()
    n = torch.bincount(flat, minlength=segprob.shape[0])
    segcount.copy_(n)
    segprob.zero_()
    if mode == 'mean':
        segprob.index_add_(0, flat, prob[m])
        segprob.div_(n.clamp_min(1)[:, None])
    else:
        segprob.index_put_((flat, prob[m].argmax(1)), torch.ones(flat.shape[0], device='cuda'), accumulate=True)
    label.copy_(torch.where(m, segprob.argmax(1)[seg.long()].int(), label))


def row(kernel, key, H, W, Cn, dtype, moved, t, diff):
    k, tt = min(t['kernel']), min(t['torch'])
    return dict(kernel=kernel, config='configs[%s]' % key, scene='%d x %d x %d' % (H, W, Cn), dtype=dtype,
                moved_mb=round(moved / 1e6, 2), kernel_ms=round(k, 4), kernel_ms_max=round(max(t['kernel']), 4),
                kernel_gb_s=round(moved / (k * 1e-3) / 1e9, 1), hbm_roof_share=round(moved / (k * 1e-3) / ROOF, 4),
                torch_ms=round(tt, 4), torch_ms_max=round(max(t['torch']), 4), kernel_vs_torch=round(tt / k, 2), differs=diff)


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
        # a blocky scene, so that the segments have something to follow: 11 x 13 blocks of a random spectrum, plus noise
        blocks = torch.rand((H + pad) // 11 + 1, (W + pad) // 13 + 1, Cn, device='cuda', generator=g)
        base = blocks.repeat_interleave(11, 0).repeat_interleave(13, 1)[:H + pad, :W + pad].contiguous()
        base = (base + 0.05 * torch.randn(base.shape, device='cuda', generator=g)).clamp_(0, 1)
        gh, gw = lib.segment_grid(H, W, S)
        Kc = gh * gw
        cand, valid = candidates(H, W)
        ws = torch.empty(lib.slic_workspace_bytes(H, W, Cn, S), dtype=torch.uint8, device='cuda')
        seg, seg_t = (torch.zeros(H, W, dtype=torch.int32, device='cuda') for _ in range(2))
        counts, counts_t = (torch.zeros(Kc, dtype=torch.int32, device='cuda') for _ in range(2))
        for half in (False, True):
            scene = base.half() if half else base
            a = scene[:H, :W].float().contiguous()       # (torch's side works on an fp32 copy of the scene: not timed)
            cen0 = torch.empty(Kc, Cn + 2, device='cuda')
            lib.slic_init(scene, H, W, S, cen0)
            cen, cen_t = cen0.clone(), cen0.clone()

            def kernel_iteration():
                lib.slic_assign(scene, H, W, S, COMPACTNESS, cen, seg)
                lib.slic_update(scene, H, W, S, seg, cen, counts, ws)

            def torch_iteration():
                torch_assign(a, cen_t, cand, valid, seg_t)
                torch_update(a, seg_t, cen_t, counts_t)
            kernel_iteration(); torch_iteration()
            diff = 'seg at %d of %d pixels; centres by %.2e' % (int((seg != seg_t).sum()), H * W, float((cen - cen_t).abs().max()))
            t = alternate({'kernel': kernel_iteration, 'torch': torch_iteration}, reps)
            moved = 2 * H * W * (Cn * scene.element_size() + 4) + 2 * ws.numel() + 3 * Kc * (Cn + 2) * 4
            rows.append(row('assign + update', key, H, W, Cn, 'fp16' if half else 'fp32', moved, t, diff))
        logits = 3.0 * torch.randn(H * W, K, device='cuda', generator=g)
        prob = torch.softmax(logits, 1).reshape(H, W, K).contiguous()
        mask = (torch.rand(H, W, device='cuda', generator=g) < 0.9).to(torch.uint8)
        segprob, segprob_t = (torch.zeros(Kc, K, device='cuda') for _ in range(2))
        label, label_t = (torch.zeros(H, W, dtype=torch.int32, device='cuda') for _ in range(2))
        for mode in ('mean', 'majority'):
            lib.segment_vote(prob, mask, seg, S, mode, segprob, counts, label)
            torch_vote(prob, mask, seg, mode, segprob_t, counts_t, label_t)
            diff = 'labels at %d of %d pixels; segprob by %.2e' % (int((label != label_t).sum()), H * W, float((segprob - segprob_t).abs().max()))
            t = alternate({'kernel': lambda: lib.segment_vote(prob, mask, seg, S, mode, segprob, counts, label),
                           'torch': lambda: torch_vote(prob, mask, seg, mode, segprob_t, counts_t, label_t)}, reps)
            rows.append(row('vote, ' + mode, key, H, W, Cn, 'fp32', H * W * (K * 4 + 1 + 4 + 4) + Kc * (K + 1) * 4, t, diff))
        del base, blocks, logits, prob
    return rows


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
            scene._segments = None                       # (a first test(): the segments are not there yet)
            prob, mask = ev.probability_map(pixels, n, n)
            ev.segment_vote(prob, mask, scene.segments(n, n, S, COMPACTNESS, 10)[0], S, 'mean')

        def segments_only():
            scene._segments = None
            scene.segments(n, n, S, COMPACTNESS, 10)
        fns = (('test_split_confusion', plain), ('segment_keys_add', added), ('of_which_ten_iterations', segments_only))
        times = {name: [] for name, _ in fns}
        for _, fn in fns:
            fn()
        for _ in range(reps):
            for name, fn in fns:
                torch.cuda.synchronize()
                t = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t) * 1e3)
        out.append(dict(config='configs[%s]' % key, test_pixels=int(len(txy)), scene_pixels=int(len(pixels)), S=S, iterations=10,
                        ms={k: dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))
                            for k, v in times.items()}))
        del scene, ev
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
        raise SystemExit('segments_bench.py measures on the GPU; none found')
    torch.zeros(1, device='cuda')
    res = dict(command='python tools/segments_bench.py --reps %d' % args.reps, kernels=bench_kernels(args.reps),
               test_pass=bench_test_pass(args.reps))
    print(json.dumps(res))
    if args.out:
        d = os.path.dirname(args.out)
        if d:
            os.makedirs(d, exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('`%s`\n\n(a) one SLIC iteration and the vote against torch composing the same arithmetic, S = %d, K = %d (ms per call: min '
                    'and max of %d alternated rounds of %d calls; moved = the bytes the kernels must read and write, GB/s and the share of '
                    'the %.2f TB/s HBM copy roof over the min; kernel_vs_torch = torch_ms / kernel_ms; differs = kernel against torch '
                    'after one call each)\n\n' % (res['command'], S, K, args.reps, LAUNCHES, ROOF / 1e12))
            f.write(table(res['kernels']) + '\n\n(b) what the keys add to a whole-split test(), ten iterations, vote mean (ms, wall)\n\n```\n'
                    + json.dumps(res['test_pass'], indent=1) + '\n```\n')


if __name__ == '__main__':
    main()
