"""What the connected superpixels cost, in one process on the GPU:

    python tools/regions_bench.py [--reps R] [--out profiles/regions.md]

At the scenes of bench.py's configs[1] (145 x 145, 200 bands) and configs[3] (512 x 512, 224 bands): the device's own SLIC image of
the synthetic blocky scene of tools/segments_bench.py (S = 8, compactness 0.1, ten iterations), then
  * labelling + merge (dmf_label_components + dmf_region_merge, n_labels = Kc, min_size = 16) with the one host read of the
    statistics that Scene.segment_regions ends in, wall clock around work that ends in a synchronise; and the same on a
    Bernoulli(0.593) two-label noise image of the same size (n_labels 2), which has many components and fragments where the SLIC
    image of this blocky scene has none;
  * dmf_region_vote, mean and majority, K = 17, by device events around LAUNCHES calls back to back;
against the route that the library without these entry points would force: a copy of `seg` to the host, the components there, a
copy of the region image back (wall clock, the same synchronise).  Two host routes are timed: scipy.ndimage.label once per cluster
that occurs (skipped where scipy does not import) and utils.segments.regions (numpy, the drop-in path's).  The host vote is
utils.segments.region_vote with the copies of prob / mask / region to the host and of the label map back.  The routes alternate in
every round; the results are compared first.  No threshold is set: a row where the device loses says so (`host_vs_device` < 1).
Needs the GPU: there is no CPU statement of a time.  Prints one JSON line; --out also writes the table as markdown.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, 'dual-modal-fusion_amd'), REPO]

LAUNCHES = 10
K, S, COMPACTNESS, ITERATIONS, MIN_SIZE = 17, 8, 0.1, 10, 16
SLIC_ITERATION_MS = {'1': 0.140, '3': 0.365}             # profiles/segments.md: one assign + update, fp32, for scale


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(LAUNCHES):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / LAUNCHES


def alternate(fns, reps, timer):
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            out[k].append(timer(fn))
    return out


def scipy_regions(seg):
    """The components per cluster by scipy.ndimage.label, numbered in raster order of their first pixels (min_size 1)."""
    from scipy import ndimage
    out = np.zeros(seg.shape, dtype=np.int64)
    n = 0
    for v in np.unique(seg):
        part, k = ndimage.label(seg == v)
        out[part > 0] = part[part > 0] + n
        n += k
    return out, n


def summary(v):
    return dict(min=round(min(v), 4), median=round(statistics.median(v), 4), max=round(max(v), 4))


def bench(reps):
    import bench as B
    from dmf import lib
    from utils import segments
    try:
        import scipy.ndimage  # noqa: F401
        have_scipy = True
    except ImportError:
        have_scipy = False
    rows = []
    for key in ('1', '3'):
        c = B.CONFIGS[key]
        H = W = c['size']
        Cn = c['bands']
        g = torch.Generator(device='cuda').manual_seed(int(key))
        blocks = torch.rand(H // 11 + 1, W // 13 + 1, Cn, device='cuda', generator=g)
        scene = blocks.repeat_interleave(11, 0).repeat_interleave(13, 1)[:H, :W].contiguous()
        scene = (scene + 0.05 * torch.randn(scene.shape, device='cuda', generator=g)).clamp_(0, 1)
        gh, gw = lib.segment_grid(H, W, S)
        Kc = gh * gw
        seg = torch.zeros(H, W, dtype=torch.int32, device='cuda')
        cen = torch.empty(Kc, Cn + 2, device='cuda')
        counts = torch.zeros(Kc, dtype=torch.int32, device='cuda')
        ws = torch.empty(lib.slic_workspace_bytes(H, W, Cn, S), dtype=torch.uint8, device='cuda')
        lib.slic_init(scene, H, W, S, cen)
        for _ in range(ITERATIONS):
            lib.slic_assign(scene, H, W, S, COMPACTNESS, cen, seg)
            lib.slic_update(scene, H, W, S, seg, cen, counts, ws)
        lib.slic_assign(scene, H, W, S, COMPACTNESS, cen, seg)
        del ws, scene, blocks
        comp, region = torch.empty_like(seg), torch.empty_like(seg)
        sizes, stats = torch.empty(H * W, dtype=torch.int32, device='cuda'), torch.empty(4, dtype=torch.int32, device='cuda')
        rws = torch.empty(lib.region_workspace_bytes(H, W, Kc), dtype=torch.uint8, device='cuda')
        back = torch.empty_like(seg)

        noise = (torch.rand(H, W, device='cuda', generator=g) < 0.593).to(torch.int32)       # many components, long chains
        for image, lab, n_labels in (('slic', seg, Kc), ('noise 0.593', noise, 2), ('slic', seg, Kc)):      # (the vote takes the last)
            def device_route():
                lib.label_components(lab, comp, rws)
                lib.region_merge(lab, comp, n_labels, MIN_SIZE, region, sizes, stats, rws)
                return stats.tolist()

            def numpy_route():
                r, _, st = segments.regions(lab.cpu().numpy(), n_labels, MIN_SIZE)
                back.copy_(torch.from_numpy(r))
                return st

            def scipy_route():                           # (components only: the merge would come on top)
                r, n = scipy_regions(lab.cpu().numpy())
                back.copy_(torch.from_numpy(r.astype(np.int32)))
                return n
            st_dev, st_np = device_route(), numpy_route()
            same = bool(torch.equal(back, region)) and st_dev[:3] == [st_np['regions'], st_np['components'], st_np['absorbed']]
            if len(rows) and rows[-1]['image'] == 'noise 0.593':
                continue                                 # (the second slic pass only restores `region` for the vote)
            fns = {'device': device_route, 'numpy': numpy_route}
            if have_scipy:
                assert scipy_route() == st_dev[1]
                fns['scipy'] = scipy_route
            t = alternate(fns, reps, wall_ms)
            d = min(t['device'])
            rows.append(dict(step='label + merge', image=image, config='configs[%s]' % key, scene='%d x %d' % (H, W),
                             labels=int(torch.unique(lab).numel()), components=st_dev[1], absorbed=st_dev[2], regions=st_dev[0],
                             device_ms=summary(t['device']), host_numpy_ms=summary(t['numpy']),
                             host_scipy_label_ms=summary(t['scipy']) if have_scipy else None,
                             host_vs_device=round(min(min(v) for k, v in t.items() if k != 'device') / d, 2), equal=same,
                             slic_iterations_for_scale=round(d / SLIC_ITERATION_MS[key], 2)))
        Rn = st_dev[0]
        prob = torch.softmax(3.0 * torch.randn(H * W, K, device='cuda', generator=g), 1).reshape(H, W, K).contiguous()
        mask = (torch.rand(H, W, device='cuda', generator=g) < 0.9).to(torch.uint8)
        regprob, regcount = torch.empty(Rn, K, device='cuda'), torch.empty(Rn, dtype=torch.int32, device='cuda')
        label, label_h = torch.zeros(H, W, dtype=torch.int32, device='cuda'), torch.zeros(H, W, dtype=torch.int32, device='cuda')
        vws = torch.empty(lib.region_vote_workspace_bytes(Rn, K), dtype=torch.uint8, device='cuda')
        for mode in ('mean', 'majority'):
            def device_vote():
                lib.region_vote(prob, mask, region, Rn, mode, regprob, regcount, label, vws)

            def host_vote():
                out = segments.region_vote(prob.cpu().numpy(), mask.cpu().numpy(), region.cpu().numpy(), Rn, mode)
                label_h.copy_(torch.from_numpy(out[2]))
                return out
            device_vote()
            out = host_vote()
            same = bool(torch.equal(label, label_h)) and regprob.cpu().numpy().tobytes() == out[0].tobytes()
            td = alternate({'device': device_vote}, reps, event_ms)['device']
            th = alternate({'host': host_vote}, reps, wall_ms)['host']
            rows.append(dict(step='vote, ' + mode, image='slic', config='configs[%s]' % key, scene='%d x %d' % (H, W), regions=Rn, K=K,
                             device_ms=summary(td), host_numpy_ms=summary(th), host_vs_device=round(min(th) / min(td), 2), equal=same,
                             slic_iterations_for_scale=round(min(td) / SLIC_ITERATION_MS[key], 2)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('regions_bench.py measures on the GPU; none found')
    torch.zeros(1, device='cuda')
    res = dict(command='python tools/regions_bench.py --reps %d' % args.reps, rows=bench(args.reps))
    print(json.dumps(res))
    if args.out:
        d = os.path.dirname(args.out)
        if d:
            os.makedirs(d, exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('`%s`\n\n```\n%s\n```\n' % (res['command'], json.dumps(res['rows'], indent=1)))


if __name__ == '__main__':
    main()
