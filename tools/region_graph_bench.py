"""What the spectrum-aware fragment merge costs, in one process on the GPU:

    python tools/region_graph_bench.py [--reps R] [--out FILE]

At the scenes of bench.py's configs[1] (145 x 145, 200 bands) and configs[3] (512 x 512, 224 bands), on the device's own SLIC image
of the synthetic blocky scene of tools/segments_bench.py (S = 8, compactness 0.1, ten iterations; n_labels = Kc) and on a
Bernoulli(0.593) two-label noise image of the same size (n_labels 2), the one with many fragments and many boundary pairs;
min_size 16.  Three routes from the label image to the region image, alternated in every round, wall clock around work that ends in
a synchronise:
  * spectrum, device   dmf_label_components, dmf_region_graph_count, the host read of the two counts, the workspace of that size,
                       dmf_region_graph_merge and the host read of the four statistics: what Scene.segment_regions(merge='spectrum') does;
  * spectrum, host     the route the library without these entry points would force for the same result: the label image and the
                       scene copied to the host, utils.segments.region_graph (numpy, the drop-in path's), the region image copied back;
  * position, device   dmf_label_components + dmf_region_merge with its host read: what the rule costs.
The results are compared first (`equal`: the region image and the statistics of the two spectrum routes).  No ratio is set: a row
where the device loses says so (`host_vs_device` < 1).  Needs the GPU.  Prints one JSON line; --out also writes the rows."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, 'dual-modal-fusion_amd'), REPO]

S, COMPACTNESS, ITERATIONS, MIN_SIZE = 8, 0.1, 10, 16


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def alternate(fns, reps):
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            out[k].append(wall_ms(fn))
    return out


def summary(v):
    return dict(min=round(min(v), 4), median=round(statistics.median(v), 4), max=round(max(v), 4))


def bench(reps):
    import bench as B
    from dmf import lib
    from utils import segments
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
        del ws, blocks
        comp, region, region_p, back = (torch.empty_like(seg) for _ in range(4))
        sizes, stats = torch.empty(H * W, dtype=torch.int32, device='cuda'), torch.empty(4, dtype=torch.int32, device='cuda')
        two = torch.empty(2, dtype=torch.int32, device='cuda')
        noise = (torch.rand(H, W, device='cuda', generator=g) < 0.593).to(torch.int32)
        for image, lab, n_labels in (('slic', seg, Kc), ('noise 0.593', noise, 2)):
            rws = torch.empty(max(lib.region_workspace_bytes(H, W, n_labels), lib.region_graph_workspace_bytes(H, W, 1, n_labels, 1)),
                              dtype=torch.uint8, device='cuda')
            bytes_seen = []

            def spectrum_device():
                lib.label_components(lab, comp, rws)
                lib.region_graph_count(lab, comp, n_labels, MIN_SIZE, two, rws)
                components, fragments = two.tolist()
                gws = torch.empty(lib.region_graph_workspace_bytes(H, W, Cn, n_labels, components), dtype=torch.uint8, device='cuda')
                bytes_seen.append(gws.numel())
                lib.region_graph_merge(lab, comp, scene, n_labels, MIN_SIZE, components, fragments, region, sizes, stats, gws)
                return stats.tolist(), fragments

            def spectrum_host():
                r, _, st = segments.region_graph(lab.cpu().numpy(), scene.cpu().numpy(), n_labels, MIN_SIZE)
                back.copy_(torch.from_numpy(r))
                return st

            def position_device():
                lib.label_components(lab, comp, rws)
                lib.region_merge(lab, comp, n_labels, MIN_SIZE, region_p, sizes, stats, rws)
                return stats.tolist()
            (st_dev, fragments), st_np, st_pos = spectrum_device(), spectrum_host(), position_device()
            same = bool(torch.equal(back, region)) and st_dev == [st_np['regions'], st_np['components'], st_np['absorbed'], st_np['rounds']]
            t = alternate({'device': spectrum_device, 'host': spectrum_host, 'position': position_device}, reps)
            d = min(t['device'])
            rows.append(dict(image=image, config='configs[%s]' % key, scene='%d x %d x %d' % (H, W, Cn), components=st_dev[1], fragments=fragments,
                             regions=st_dev[0], rounds=st_dev[3], rounds_enqueued=int(fragments).bit_length(), regions_position=st_pos[0],
                             workspace_mb=round(bytes_seen[0] / 1e6, 2), spectrum_device_ms=summary(t['device']),
                             spectrum_host_numpy_ms=summary(t['host']), position_device_ms=summary(t['position']),
                             host_vs_device=round(min(t['host']) / d, 2), spectrum_vs_position=round(d / min(t['position']), 2), equal=same))
            del rws
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('region_graph_bench.py measures on the GPU; none found')
    torch.zeros(1, device='cuda')
    res = dict(command='python tools/region_graph_bench.py --reps %d' % args.reps, rows=bench(args.reps))
    print(json.dumps(res))
    if args.out:
        d = os.path.dirname(args.out)
        if d:
            os.makedirs(d, exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('`%s`\n\n```\n%s\n```\n' % (res['command'], json.dumps(res['rows'], indent=1)))


if __name__ == '__main__':
    main()
