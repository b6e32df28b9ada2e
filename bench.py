#!/usr/bin/env python3
"""bench.py — training patches/s of the dual-modal fusion hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W [--config {1,2,3,4,panms}] [--dump-outputs DIR] [--full]
                                                                                  (N > 1: launched by torch.distributed.run)

Workloads (`--config`, BASELINE.json `configs` by index; default 1, the configuration the metric is quoted on):
  1      synthetic 145x145 scene, 200-band HSI + 1-band SAR, 11x11 patches, 17 logits, batch 256 per GPU, fp32   (configs[1])
  2      the same scene with the cross-modal attention block (bf16 MFMA operands), batch 1024                     (configs[2])
  3      512x512 scene, 224-band HSI + 3-band SAR, batch 256 per GPU — `--gpus 8` is configs[3] itself            (configs[3])
  4      stage 2 of the two-stage path: four 4-band 256x256 streams, 16x16 patches, qua_loss, bs 256              (configs[4])
  panms  the reference's own data shape (config.yml:27,77-110): 4-band MS + PAN at 4x, 16x16 patches
N > 1 uses the same scene with per-GPU batch B (weak scaling) and one flat fp32 gradient exchange per step.  A "step" =
forward + loss + backward + ADAM on one batch; inputs (padded scenes, the shuffled coordinate/label plan) are resident
in HBM before the timed region.

One JSON line on rank 0.  `value` = N*B*K / (max-over-ranks wall time of exactly K steps, barrier + synchronize on both
sides); `ms_per_step` = that wall time / K.  A plain run does only that: set-up, W warm-up steps, K timed steps, the line.

`--dump-outputs DIR` writes what the timed path computed in its last step, after the timed region, as float32
DIR/<name>.npy (rank 0; the inputs are seeded, so the same arguments give the same inputs in every run):
  logits       [B, K] (config 4: [4*bs, K])   logits of the last timed step's batch
  loss         [B]    (config 4: [1])         its per-patch cross-entropy (config 4: its qua_loss)
  params              the flat weights after the last step's optimiser update
  adam_m, adam_v      ADAM's moment estimates after it
  step_losses  [K]                            the mean loss of every timed step

`--full` adds what takes runs of its own.  `roofline` is for the dominant kernel: algorithmic bytes (or matrix-core flops)
per launch / its mean duration, measured here with HIP events on the launch stream in an instrumented pass of the same
steps.  `kappa` comes from training continued to `--kappa-steps` steps (independent of --steps); `cpu_baseline` = the CPU
oracle's restatement of the reference train loop (oracle/solver_ref.py) on the same batches, timed on this host (first
chunk excluded as warm-up).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(ROOT, 'dual-modal-fusion_amd'), ROOT]

HBM_PEAK = 8.0e12          # B/s, MI355X HBM3E spec (MI355X_MICROARCH.md)
MFMA_BF16_PEAK = 2.5e15    # flop/s, dense bf16 matrix-core peak (MI355X_MICROARCH.md)

CONFIGS = {
    '1': dict(size=145, bands=200, aux_bands=1, patch=11, scale=1, width=40, attention=0, batch=256, classes=16,
              name='configs[1]: synthetic 145x145 scene, 200-band HSI + 1-band SAR'),
    '2': dict(size=145, bands=200, aux_bands=1, patch=11, scale=1, width=40, attention=1, batch=1024, classes=16,
              name='configs[2]: 145x145 scene, 200-band HSI + 1-band LiDAR, cross-modal attention on (bf16 MFMA)'),
    '3': dict(size=512, bands=224, aux_bands=3, patch=11, scale=1, width=32, attention=0, batch=256, classes=16,
              name='configs[3]: 512x512 scene, 224-band HSI + 3-band SAR'),
    'panms': dict(size=256, bands=4, aux_bands=1, patch=16, scale=4, width=40, attention=0, batch=256, classes=11,
                  name='reference data shape (config.yml:27,77-110): 256x256 4-band MS + 1024x1024 PAN'),
    '4': dict(size=256, bands=4, aux_bands=1, patch=16, scale=1, width=40, attention=0, batch=256, classes=11,
              name='configs[4]: stage 2 of the two-stage path, four 4-band 256x256 streams'),
}


def make_cfg(args):
    from dmf.synth import class_colors
    K = args.classes + 1
    return {'patch_size': args.patch, 'Categories_Number': K, 'data_city': 'syn',
            'DATA_DICT': {'syn': {'size': [args.size, args.size, args.bands], 'color': class_colors(K)}},
            'scale': args.scale, 'aux_bands': args.aux_bands,
            'gmf': {'width': args.width, 'hidden': 64, 'pool_sigma': 2.5, 'attention': args.attention, 'half': args.half},
            'trans': {'embed_dim': 96, 'num_head': 3}}


def build_problem(args, cfg):
    from dmf import synth
    from function.function import data_padding, data_padding_aux, split_data_old
    primary, aux, label = synth.make_scene(args.size, args.size, args.bands, args.aux_bands, args.scale, n_classes=args.classes, seed=0)
    MS = data_padding(primary, cfg, 'ms').astype(np.float32)
    PAN = data_padding_aux(aux, cfg).astype(np.float32)
    import contextlib, io
    with contextlib.redirect_stdout(io.StringIO()):
        xyl, idx = split_data_old(label, cfg)
    labelled = np.array(idx[1])
    g = torch.Generator().manual_seed(3407)                       # test.py:8
    perm = torch.randperm(len(labelled), generator=g).numpy()
    n_train = int(args.train_rate * len(labelled))
    train, test = labelled[perm[:n_train]], labelled[perm[n_train:]]
    xy = np.concatenate([xyl[0], xyl[1]], 1).astype(np.int32)
    lab = xyl[2].reshape(-1).astype(np.int32)
    return MS, PAN, xy, lab, train, test


def make_plan(train, n_steps, B, seed):
    """Concatenated per-epoch permutations of the train pixels, cut into n_steps batches of B."""
    g = torch.Generator().manual_seed(seed)
    out = []
    need = n_steps * B
    while sum(len(o) for o in out) < need:
        out.append(train[torch.randperm(len(train), generator=g).numpy()])
    return np.concatenate(out)[:need]


def prewarm(eng, net, args, ms):
    """Device warm-up that touches NO training state: the EVAL forward launch of plan batch 0 (a different kernel symbol
    than the training step's, so rocprofv3's per-kernel averages of the step stay clean), repeated for ~`ms` milliseconds.
    A freshly started process runs its first kernels at ramping clocks; without this a short `--steps` run measures the
    ramp, not the step.  The W warm-up steps the caller asked for follow as usual."""
    from dmf import lib
    B = eng.B
    inp = lib.input_gather(eng.shape, eng.scene.A, eng.scene.B, eng.plan_xy[:B])
    logits = torch.empty_like(eng.logits)
    aws = torch.empty(lib.attn_workspace_bytes(eng.shape, B), dtype=torch.uint8, device=logits.device) if args.attention else None
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < ms:
        for _ in range(100):
            if args.attention:
                lib.forward_attn(eng.shape, inp, eng.theta, net.pool_w, aws, logits)
            else:
                lib.forward(eng.shape, inp, eng.theta, net.pool_w, logits)
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def launch_label(spg, n_steps):
    """What run_plan(n_steps, spg) actually executes: it replays the captured graph while whole graphs fit, the rest eagerly."""
    if spg < 0:
        return 'one C loop of 2 launches per step (dmf_train_plan_steps: no graph, no window copy)', 0
    if not spg:
        return 'eager', 0
    n_rep = n_steps // spg
    rest = n_steps - n_rep * spg
    if n_rep == 0:
        return 'eager', 0
    return 'hipGraph x%d steps, %d replay%s%s' % (spg, n_rep, '' if n_rep == 1 else 's', (' + %d eager steps' % rest) if rest else ''), n_rep


def exchange_matches_rccl(eng, comm, pg, step, backend):
    """Admission check of the one-shot exchange on REAL gradients (warm-up only): this rank's flat gradient of plan step
    `step`, summed over the ranks once by the exchange and once by the process group's own all_reduce."""
    import torch.distributed as dist
    from dmf import lib
    B = eng.B
    inp = lib.input_gather(eng.shape, eng.scene.A, eng.scene.B, eng.plan_xy[step * B:(step + 1) * B])
    lib.train_fwd_bwd(eng.shape, inp, eng.theta, eng.net.pool_w, eng.plan_labels[step * B:(step + 1) * B], 1.0 / B,
                      eng.logits, eng.loss, eng.ws)
    lib.grad_reduce(eng.shape, B, eng.ws, eng.grad)
    g_x = eng.grad.clone()
    comm.allreduce_(g_x)
    if backend == 'nccl':
        g_r = eng.grad.clone()
        dist.all_reduce(g_r, op=dist.ReduceOp.SUM, group=pg)
    else:
        g_r = eng.grad.cpu()
        dist.all_reduce(g_r, op=dist.ReduceOp.SUM, group=pg)
        g_r = g_r.to(g_x.device)
    torch.cuda.synchronize()
    tol = 1e-5 * float(g_r.abs().max()) + 1e-12                 # the two sums differ in order only
    err, st = float((g_x - g_r).abs().max()), comm.status()
    if st != 0 or not err <= tol:
        print('[bench] rank %d, warm-up step %d: exchange status %d, max |exchange - all_reduce| = %.3e (tolerance %.3e, max |sum| %.3e)'
              % (dist.get_rank(pg), step, st, err, tol, float(g_r.abs().max())), file=sys.stderr, flush=True)
        return False
    return True


VALU_CYCLES_PER_INSTR = 3.15     # best measured vector-issue interval of one SIMD (profiles/r2_valu_rate.txt: v_fmac_f32, 4 waves per SIMD)
SHADER_CLOCK = 2.4e9             # Hz, MI355X maximum (MI355X_MICROARCH.md)


def issue_roofline(cfgname, kernel_key, kern_ms):
    """Vector-issue roofline of the dominant kernel: the vector instructions one launch issues (SQ_INSTS_VALU, collected by
    tools/collect_r3.sh into profiles/issue_counts.json for the default shape of --config 1 / 4 / panms) / its measured duration,
    against 1024 SIMDs x clock / the best measured issue interval.  For a 4-KB patch the HBM roof says nothing (frac 0.02):
    these kernels issue ~12-17 K vector instructions per patch whatever the number of bands."""
    path = os.path.join(ROOT, 'profiles', 'issue_counts.json')
    if kern_ms is None or not os.path.exists(path):
        return None
    try:
        kern = json.load(open(path))['configs'].get(cfgname, {})
    except Exception:
        return None
    hit = [v for k, v in kern.items() if kernel_key in k and 'SQ_INSTS_VALU' in v]
    if not hit:
        return None
    n_valu, n_salu = hit[0]['SQ_INSTS_VALU'], hit[0].get('SQ_INSTS_SALU')
    peak = 1024 * SHADER_CLOCK / VALU_CYCLES_PER_INSTR
    ach = n_valu / (kern_ms * 1e-3)
    return {'bound': 'vector issue', 'achieved': ach / 1e9, 'peak': peak / 1e9, 'unit': 'G wave-instructions/s', 'frac': ach / peak,
            'valu_instructions_per_launch': n_valu, 'salu_instructions_per_launch': n_salu,
            'basis': 'SQ_INSTS_VALU per launch (profiles/issue_counts.json, default shape of this --config) / kernel_ms; peak = 1024 SIMDs x '
                     '2.4 GHz / 3.15 cycles per instruction (profiles/r2_valu_rate.txt)'}


DUMP_MAX_ELEMS = 2 << 20            # per array (8 MB of float32): six arrays stay under 64 MB


def snapshot_outputs(eng, losses, K_steps):
    """The arrays a caller of the timed path holds after its last step, copied to the host (before anything else runs)."""
    out = {'logits': eng.logits, 'loss': eng.loss, 'params': eng.theta, 'adam_m': eng.m, 'adam_v': eng.v,
           'step_losses': losses[-K_steps:]}
    return {k: v.detach().cpu().clone() for k, v in out.items()}


def dump_outputs(path, arrays):
    """--dump-outputs: one float32 DIR/<name>.npy per array; an array larger than DUMP_MAX_ELEMS is replaced by a fixed,
    seeded sample of its flattened elements (sorted indices, the same in every run)."""
    os.makedirs(path, exist_ok=True)
    for name, a in arrays.items():
        a = np.ascontiguousarray(a.numpy(), dtype=np.float32)
        if a.size > DUMP_MAX_ELEMS:
            idx = np.sort(np.random.default_rng(0).choice(a.size, DUMP_MAX_ELEMS, replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(path, name + '.npy'), a)


def spawn_ranks(n):
    """`python bench.py --gpus N` without a launcher: start N ranks of this script under torch.distributed.run as a CHILD
    process (this process has not initialised the GPU and never will), pass its output through, return its exit code."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(n), '--master-addr', '127.0.0.1',
           '--master-port', str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')           # dmabuf IPC: what RCCL and the exchange's HIP-IPC mapping need here
    rc = subprocess.call(cmd, env=env)
    if rc:
        raise SystemExit(rc)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=2000)
    ap.add_argument('--warmup', type=int, default=200)
    ap.add_argument('--config', default='1', choices=sorted(CONFIGS))
    for k, t in (('batch', int), ('size', int), ('bands', int), ('aux-bands', int), ('width', int), ('patch', int),
                 ('scale', int), ('classes', int), ('attention', int)):
        ap.add_argument('--' + k, type=t, default=None, help='overrides the --config value')
    ap.add_argument('--half', type=int, default=None, choices=[0, 1],
                    help='fp16 primary scene + fp16 spec_a operands (fp32 accumulate) + device loss scaler; default: 1 for '
                         '--config 4 (BASELINE configs[4]: "fp16 mixed precision"), else 0 (the fp32 headline)')
    ap.add_argument('--scaler', type=int, default=1, choices=[0, 1],
                    help='with --half 1: 1 = the device loss scaler with GradScaler\'s rule (the reference\'s autocast + GradScaler '
                         'semantics: a third launch per step); 0 = fp16 storage and spec_a operands only (every gradient is fp32 '
                         'in this design, the scale has no numerical job)')
    ap.add_argument('--train-rate', type=float, default=0.10)
    ap.add_argument('--steps-per-graph', type=int, default=None,
                    help='steps per captured hipGraph; 0 = eager launches from Python; -1 = one C loop of launches (dmf_train_plan_steps). '
                         'Default: -1 where that exists (one GPU, late-fusion net, no loss scaler: 15.75 against 15.97 us per step from graphs of 50), else 50')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='after the timed steps, write what the last one computed as float32 DIR/<name>.npy (rank 0)')
    ap.add_argument('--full', action='store_true',
                    help='also the figures that take runs of their own: the instrumented kernel pass (roofline), kappa after '
                         '--kappa-steps, the CPU oracle baseline')
    ap.add_argument('--kappa-steps', type=int, default=2200, help='--full: train to this many steps (from the initial weights) before kappa')
    ap.add_argument('--cpu-seconds', type=float, default=90.0, help='--full: CPU oracle budget (rank 0, N=1 only)')
    ap.add_argument('--no-cpu', action='store_true', help='--full: skip the CPU oracle')
    ap.add_argument('--no-cpu-spread', action='store_true', help='--full: skip the second CPU oracle training (kappa noise floor)')
    args = ap.parse_args()
    for k, v in CONFIGS[args.config].items():
        if k != 'name' and getattr(args, k) is None:
            setattr(args, k, v)
    if args.bands == 224 and args.width == 40:
        args.width = 32                     # the compiled 224-band instance
    if args.half is None:
        args.half = 1 if args.config == '4' else 0

    rank = int(os.environ.get('RANK', 0))
    local_rank = int(os.environ.get('LOCAL_RANK', 0))
    world = int(os.environ.get('WORLD_SIZE', 1))
    if world != args.gpus:
        if world == 1 and args.gpus > 1 and 'RANK' not in os.environ:
            return spawn_ranks(args.gpus)           # `python bench.py --gpus N` starts its own N ranks (nothing has touched the GPU yet)
        raise SystemExit('--gpus %d does not match WORLD_SIZE %d' % (args.gpus, world))
    if not torch.cuda.is_available():
        raise SystemExit('bench.py needs a GPU (the product path has no CPU fallback)')
    # rehearsal knobs for a one-GPU box (never set by the driver): all ranks on cuda:0, gloo instead of RCCL
    if os.environ.get('DMF_SINGLE_DEVICE') == '1':
        local_rank = 0
    backend = os.environ.get('DMF_DIST_BACKEND', 'nccl')
    torch.cuda.set_device(local_rank)
    dev = torch.device('cuda', local_rank)
    pg = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        if backend == 'nccl':
            dist.init_process_group('nccl', device_id=dev)
        else:
            dist.init_process_group(backend)
        pg = dist.group.WORLD
        if os.environ.get('DMF_CU_SHARE') == '1':      # rehearsal on ONE GPU: every rank on its own share of the compute units
            from dmf import xgmi as _xg                # (dmf.xgmi.cu_share_stream says why the exchange needs that there)
            torch.cuda.set_stream(_xg.cu_share_stream(rank, world, dev))
    if args.config == '4':
        return main_stage2(args, dev, pg, rank, world, backend)

    from dmf import lib
    from dmf.engine import EvalEngine, LossScaler, Scene, TrainEngine
    from model.gmfnet import Net

    cfg = make_cfg(args)
    MS, PAN, xy_tab, lab_tab, train, test = build_problem(args, cfg)
    B, K_steps, W_steps = args.batch, args.steps, args.warmup
    P, C, C2, S = args.patch, args.bands, args.aux_bands, args.scale
    torch.manual_seed(3407)
    net = Net(cfg).to(dev)
    init_state = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    scene = Scene(MS, PAN, dev, half=bool(args.half))
    scaler = lambda: LossScaler(dev) if (args.half and args.scaler) else None      # (GradScaler defaults: 65536, x2 / x0.5, every 2000)
    comm = None
    # N > 2 has only ever been exercised with all ranks on ONE GPU (tests/test_gpu_dp.py); the exchange is admitted per run
    # by the checks below and the RCCL all-reduce is the fallback
    if world > 1 and os.environ.get('DMF_ALLREDUCE', 'xgmi') == 'xgmi' and not args.half:
        from dmf import xgmi
        comm = xgmi.create(sum(p.numel() for p in net.parameters()), pg,     # None on every rank if it cannot be proven
                           timeout_ms=int(os.environ.get('DMF_XGMI_TIMEOUT_MS', 20000)))
    eng = TrainEngine(net, scene, B, lr=1e-3, process_group=pg, comm=comm, scaler=scaler())

    total = W_steps + K_steps
    plan_steps = max(total, args.kappa_steps) if args.full else total      # (the same batches either way: a prefix)
    plan_idx = make_plan(train, plan_steps, B * world, seed=1)                 # global batches of world*B
    mine = plan_idx.reshape(plan_steps, world, B)[:, rank, :].reshape(-1)      # this rank's contiguous shard per step
    eng.load_plan(xy_tab[mine], lab_tab[mine])
    prewarm_ms = prewarm(eng, net, args, 60.0)
    graphable = eng._graphable()               # one GPU, the one-shot exchange, or RCCL's all-reduce captured with the step
    want = args.steps_per_graph if args.steps_per_graph is not None else (-1 if eng._native_loop_ok() else 50)
    native = want < 0 and eng._native_loop_ok()                     # the library's own launch loop
    if want < 0 and not native:
        want = 50
    args.steps_per_graph = want
    spg = -1 if native else (min(want, K_steps) if graphable else 0)

    def sync():
        torch.cuda.synchronize()
        if world > 1:
            import torch.distributed as dist
            dist.barrier()
            torch.cuda.synchronize()

    def vote_bad(flag):
        import torch.distributed as dist
        bad = torch.tensor([1 if flag else 0], dtype=torch.int32, device=dev if backend == 'nccl' else 'cpu')
        dist.all_reduce(bad, op=dist.ReduceOp.MAX)
        return int(bad.item()) != 0

    # ---- warm-up (W steps; also builds the graph), then EXACTLY K timed steps
    exchange_note = None
    if comm is not None:
        # every warm-up step first checks the exchange against the process group's own all-reduce on that step's real
        # gradient; any mismatch or time-out on any rank sends EVERY rank to the RCCL path before anything is timed
        ok = True
        for k in range(W_steps):
            ok = exchange_matches_rccl(eng, comm, pg, k, backend) and ok
            eng.run_plan(1, 0)
        bad = vote_bad((not ok) or comm.status() != 0)
        if bad:
            exchange_note = 'one-shot exchange rejected during warm-up (mismatch against all_reduce or time-out)'
            if rank == 0:
                print('[bench] %s; falling back to the RCCL all-reduce' % exchange_note, file=sys.stderr, flush=True)
            comm = None
            net.load_state_dict(init_state)
            eng = TrainEngine(net, scene, B, lr=1e-3, process_group=pg, comm=None, scaler=scaler())
            eng.load_plan(xy_tab[mine], lab_tab[mine])
            spg = min(args.steps_per_graph, K_steps) if eng._graphable() else 0
            eng.run_plan(W_steps, spg)
    else:
        # the warm-up runs through the SAME captured graph as the timed steps (whole graphs, the rest eagerly): the first
        # replay of a graph pays its one-time upload, which belongs to the warm-up
        eng.run_plan(W_steps, spg)
    launch, n_replays = launch_label(spg, K_steps)
    if n_replays and eng.graph is None:
        try:
            eng._capture(spg)                   # capture restores state: no steps are consumed
        except RuntimeError:
            if world == 1 or comm is not None:
                raise
            eng._rccl_graph, eng.graph, spg = False, None, 0       # RCCL refused the capture: eager steps (see TrainEngine.run_plan)
            launch, n_replays = launch_label(0, K_steps)
    if n_replays and eng.graph is None:
        launch, n_replays = launch_label(0, K_steps)
    graph_warmed = False
    if n_replays and W_steps < spg:
        # the warm-up was shorter than one graph, so the graph executable has never been launched: one replay whose effects
        # are put back (still exactly W warm-up steps of training) keeps its first-launch cost out of the timed region
        graph_warmed = eng.warm_graph()
    sync()
    t0 = time.perf_counter()
    eng.run_plan(K_steps, spg if (n_replays or spg < 0) else 0)
    sync()
    dt = time.perf_counter() - t0
    if world > 1:
        import torch.distributed as dist
        t = torch.tensor([dt], device=dev if backend == 'nccl' else 'cpu', dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    if comm is not None:
        if vote_bad(comm.status() != 0):        # every rank leaves together
            raise SystemExit('rank %d: a gradient exchange timed out waiting for a peer — the timing is void' % rank)
    n_ranks_seen = 1
    if world > 1:                               # how many ranks the process group really has: a sum of ones
        import torch.distributed as dist
        one = torch.ones(1, device=dev if backend == 'nccl' else 'cpu')
        dist.all_reduce(one)
        n_ranks_seen = int(one.item())
    value = world * B * K_steps / dt
    if args.dump_outputs and rank == 0:                  # before anything below reuses the engine's buffers
        dump_outputs(args.dump_outputs, snapshot_outputs(eng, eng.mean_losses(), K_steps))

    # ---- instrumented pass (--full): mean duration of the dominant kernel, HIP events on the launch stream
    n_inst = min(max(K_steps, 100), 200)                 # (at least 100 launches, however short the timed region was: batches repeat)
    alg_patch = 2 * ((2 if args.half else 4) * P * P * C + 4 * (S * P) * (S * P) * C2)     # --half: the primary bands are 2 bytes
    kern_ms = None
    if args.full and (rank == 0 or world > 1):
        inst_idx = np.concatenate([mine[(i % plan_steps) * B:(i % plan_steps + 1) * B] for i in range(n_inst)])
        inst_plan_xy = torch.from_numpy(xy_tab[inst_idx]).to(dev)
        inst_lab = torch.from_numpy(lab_tab[inst_idx]).to(dev)
        theta2 = eng.theta.clone()
        # One event pair brackets GROUP consecutive launches of the kernel, each on its own batch of the plan, replayed from a
        # captured graph: a pair around a single 12-us launch would also time the ~2 us the command processor spends on the two
        # event packets, and launches enqueued one by one from Python (~10 us of host time each) leave the device waiting for
        # the host.  (Back-to-back launches of THIS kernel: each still pays for the write-back of its predecessor's 2 MB of
        # slab rows, which in the real step the reduce launch pays — rocprofv3's average inside the real step is ~5 % lower.)
        GROUP = 50
        n_rep = max((n_inst + GROUP - 1) // GROUP, 2)
        ws = eng.ws
        inps = [lib.input_gather(eng.shape, scene.A, scene.B, inst_plan_xy[(i % n_inst) * B:((i % n_inst) + 1) * B]) for i in range(GROUP)]

        def group():
            for i, inp in enumerate(inps):
                lb = inst_lab[(i % n_inst) * B:((i % n_inst) + 1) * B]
                if args.attention:
                    lib.train_attn_fwd_bwd(eng.shape, inp, theta2, net.pool_w, lb, None, 1.0 / B, eng.logits, eng.loss, ws, eng.attn_ws)
                else:
                    lib.train_fwd_bwd(eng.shape, inp, theta2, net.pool_w, lb, 1.0 / B, eng.logits, eng.loss, ws)
        group()                                            # (every kernel has run once before the capture)
        torch.cuda.synchronize()
        gi = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gi):
            group()
        gi.replay()                                        # first replay of a graph: not timed
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n_rep)]
        torch.cuda.synchronize()
        for a_, b_ in ev:
            a_.record()
            gi.replay()
            b_.record()
        torch.cuda.synchronize()
        kern_ms = float(np.mean([a_.elapsed_time(b_) / GROUP for a_, b_ in ev]))
    losses = eng.mean_losses().numpy() if world == 1 else np.zeros(0)

    # ---- kappa (--full): training continues to --kappa-steps (a fixed budget, not --steps), then the held-out split is
    # classified on the device; with N ranks every rank classifies its shard of the pixels and the K x K matrices are all-reduced
    done = total
    if args.full:
        if plan_steps > done:
            eng.run_plan(plan_steps - done, spg if (n_replays or spg < 0) else 0)
            done = plan_steps
        n_test = min(len(test), 8192)
        ev_eng = EvalEngine(net, scene, 2048)
        m_test = ev_eng.confusion(xy_tab[test[:n_test]], lab_tab[test[:n_test]], process_group=pg).cpu().numpy().astype(np.float64)
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        if rank != 0:
            dist.destroy_process_group()
    if rank != 0:
        return

    traffic = None
    tpath = os.path.join(ROOT, 'profiles', 'pmc_traffic.json')
    if os.path.exists(tpath) and args.config == '1':
        try:
            traffic = json.load(open(tpath)).get('patch_kernel_hbm_bytes_per_launch')
        except Exception:
            traffic = None
    v2 = bool(lib.patch_v2_used(eng.shape)) if hasattr(lib, 'patch_v2_used') else False
    roof = None
    if kern_ms is None:
        pass                                             # (a plain run: no instrumented pass)
    elif args.attention:
        # matrix-core work per patch (padded shapes, tools/attn_bench.py): forward 3 projections + QK^T + PV + out-proj, the
        # backward's recompute of it, and the backward products fed as hi/lo bf16 pairs
        fwd = 2.0 * (3 * 128 * 64 * 96 + 2 * 3 * 128 * 128 * 32 + 128 * 96 * 48)
        bwd = 2.0 * (2 * (2 * 3 * 128 * 128 * 32) + 2 * (2 * 3 * 128 * 32 * 48) + 2 * (2 * 3 * 32 * 48 * 128)) + 2.0 * 3 * 128 * 128 * 32
        flops = B * (2 * fwd + bwd)
        roof = {'bound': 'mfma', 'achieved': flops / (kern_ms * 1e-3) / 1e12, 'peak': MFMA_BF16_PEAK / 1e12, 'unit': 'TFLOP/s',
                'frac': flops / (kern_ms * 1e-3) / MFMA_BF16_PEAK, 'traffic': None,
                'kernel': 'patch_kernel<TOKENS> + attn_train_kernel + patch_kernel<DENSE> (one C call: dmf_train_attn_fwd_bwd)',
                'kernel_ms': kern_ms, 'matrix_flops_per_launch': flops}
    else:
        achieved = B * alg_patch / (kern_ms * 1e-3)
        roof = {'bound': 'hbm', 'achieved': achieved / 1e9, 'peak': HBM_PEAK / 1e9, 'unit': 'GB/s', 'frac': achieved / HBM_PEAK,
                'traffic': traffic,
                'kernel': 'dmf::%s<Shape<%d,%d,%d,%d,%d,..>, MODE_TRAIN%s>' % ('patch_v2_kernel' if v2 or args.half else 'patch_kernel', C, C2, P, S,
                                                                          net.arch['F'], ', fp16 scene' if args.half else ''),
                'kernel_ms': kern_ms, 'algorithmic_bytes_per_launch': B * alg_patch}
    out = {
        'metric': 'training patches/sec + kappa, 11x11x200 HSI + 11x11x1 SAR, 1/2/4/8 MI355X',
        'value': value, 'unit': 'patches/s', 'n_gpus': world, 'steps': K_steps, 'warmup': W_steps,
        'ms_per_step': dt / K_steps * 1e3, 'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None,
        'dtype': (('f16 scene + spec_a operands, f32 accumulate / gradients / Adam' + (', dynamic loss scale' if args.scaler else ', no loss scale')) if args.half else 'f32')
                 if not args.attention else 'f32 (attention operands bf16, f32 accumulate)', 'data': 'synthetic',
        'config': {'workload': '%s; %dx%d scene, %d + %d bands, %dx%d patches, %d logits, batch %d per GPU, fused HIP fwd+loss+bwd+Adam'
                               % (CONFIGS[args.config]['name'], args.size, args.size, C, C2, P, P, args.classes + 1, B),
                   'global_batch': B * world, 'parallelism': 'dp%d' % world, 'launch': launch,
                   'device_prewarm_ms': round(prewarm_ms, 1), 'graph_warm_replay': bool(graph_warmed),
                   'allreduce': 'none' if world == 1 else ('xgmi one-shot, fused in the reduce+Adam launch' if comm is not None
                                                           else '%s all_reduce of one flat fp32 gradient%s' % ('rccl' if backend == 'nccl' else backend,
                                                                                                                      ', captured in the step graph' if n_replays else ', host-enqueued')),
                   'n_ranks_seen': n_ranks_seen},
        'roofline': roof,
        'step_frac_of_hbm_roof': value / world * (alg_patch + 28.0 * eng.theta.numel() / B) / HBM_PEAK,
    }
    if roof is None:
        del out['roofline']
    default_shape = all(getattr(args, k) == v for k, v in CONFIGS[args.config].items() if k != 'name')
    if args.full and not args.attention and not args.half and default_shape:
        ir = issue_roofline(args.config if args.config != '3' else '', ', 1, 1, false>', kern_ms)
        if ir is not None:
            out['issue_roofline'] = ir
    if exchange_note:
        out['config']['allreduce_note'] = exchange_note
    if losses.size:
        out['loss_first_last'] = [float(losses[0]), float(losses[min(len(losses), total) - 1])]
    if not args.full:
        print(json.dumps(out), flush=True)
        if world > 1:
            import torch.distributed as dist
            dist.destroy_process_group()
        return

    from indicators.kappa import aa_oa_quiet
    aa, oa, kp = aa_oa_quiet(m_test)
    out['kappa'] = {'gpu': kp, 'oa': oa, 'aa': aa, 'test_patches': int(n_test), 'train_steps': done}

    # ---- CPU oracle on the same batches (N == 1 only): throughput baseline + kappa at equal step counts
    if world == 1 and not args.no_cpu:
        from oracle.gmfnet_ref import Net as RefNet
        from oracle import solver_ref
        n_thr = min(len(os.sched_getaffinity(0)), 16)        # the GPU box gives one GPU's job a 16-core share
        torch.set_num_threads(n_thr)
        ref = RefNet(cfg)
        ref.load_state_dict(init_state)
        opt = torch.optim.Adam(ref.parameters(), lr=1e-3)
        cpu_losses, chunk, t_chunks = [], 25, []
        t_start = time.perf_counter()
        n_goal = min(args.kappa_steps, plan_steps)
        for c0 in range(0, n_goal, chunk):
            n_c = min(chunk, n_goal - c0)
            sl = mine[c0 * B:(c0 + n_c) * B]
            t1 = time.perf_counter()
            l, opt = solver_ref.train_steps(ref, MS, PAN, xy_tab[sl], lab_tab[sl], B, P, S, optimizer=opt)
            t_chunks.append((n_c, time.perf_counter() - t1))
            cpu_losses += l
            if time.perf_counter() - t_start > args.cpu_seconds:
                break
        timed = t_chunks[1:] if len(t_chunks) > 1 else t_chunks        # first chunk = thread-pool / allocator warm-up
        n_t, t_t = sum(n for n, _ in timed), sum(t for _, t in timed)
        out['cpu_baseline'] = {'value': n_t * B / t_t, 'unit': 'patches/s', 'cores': torch.get_num_threads(), 'kind': 'port',
                               'sample': '%d of the same train steps (batch %d) after a %d-step warm-up chunk, oracle/solver_ref.py on '
                                         'torch-CPU fp32, %.1f s timed' % (n_t, B, t_chunks[0][0] if len(t_chunks) > 1 else 0, t_t)}
        n_cmp = min(len(cpu_losses), len(losses))
        if n_cmp:
            d = np.abs(np.array(cpu_losses[:n_cmp]) - losses[:n_cmp])
            out['cpu_baseline']['max_abs_loss_diff_first_20_steps'] = float(d[:20].max())
            out['cpu_baseline']['max_abs_loss_diff_first_%d_steps' % n_cmp] = float(d.max())
        # kappa of the CPU forward path on the GPU-trained weights (same weights, same patches: must be identical)
        n_kt = min(n_test, 2048)
        ref_f = RefNet(cfg)
        ref_f.load_state_dict({k: v.cpu() for k, v in net.state_dict().items()})
        m_f, _ = solver_ref.evaluate(ref_f, MS, PAN, xy_tab[test[:n_kt]], lab_tab[test[:n_kt]], args.classes + 1, P, S)
        m_g = ev_eng.confusion(xy_tab[test[:n_kt]], lab_tab[test[:n_kt]]).cpu().numpy().astype(np.float64)
        out['kappa'].update({'same_weights_test_patches': int(n_kt), 'same_weights_gpu': aa_oa_quiet(m_g)[2],
                             'same_weights_cpu_forward': aa_oa_quiet(m_f)[2],
                             'same_weights_predictions_differing': int(np.abs(m_f - m_g).sum() // 2)})
        # kappa after the SAME number of steps from the same initial weights on the same held-out patches: the CPU oracle
        # against a fresh GPU run of exactly as many steps as the CPU completed (north star: within +-0.001)
        n_k = len(cpu_losses)
        if n_k:
            m_cpu, _ = solver_ref.evaluate(ref, MS, PAN, xy_tab[test[:n_kt]], lab_tab[test[:n_kt]], args.classes + 1, P, S)
            net2 = Net(cfg).to(dev)
            net2.load_state_dict(init_state)
            eng2 = TrainEngine(net2, scene, B, lr=1e-3, scaler=scaler())
            eng2.load_plan(xy_tab[mine[:n_k * B]], lab_tab[mine[:n_k * B]])
            eng2.run_plan(n_k, 0)
            m_gpu = EvalEngine(net2, scene, 2048).confusion(xy_tab[test[:n_kt]], lab_tab[test[:n_kt]]).cpu().numpy().astype(np.float64)
            k_cpu, k_gpu = aa_oa_quiet(m_cpu)[2], aa_oa_quiet(m_gpu)[2]
            out['kappa'].update({'parity_steps': n_k, 'parity_steps_goal': n_goal, 'parity_test_patches': int(n_kt),
                                 'cpu_after_parity_steps': k_cpu, 'gpu_after_parity_steps': k_gpu,
                                 'abs_delta_kappa': abs(k_cpu - k_gpu), 'within_0.001': bool(abs(k_cpu - k_gpu) <= 1e-3),
                                 'confusion_entries_differing': int(np.abs(m_cpu - m_gpu).sum() // 2)})
            # the noise floor that delta is to be read against, measured in THIS run: the same CPU oracle, same initial weights,
            # same batches, same test patches, only the thread count (= the partition of its fp32 reductions) changed
            if not args.no_cpu_spread:
                n_thr2 = n_thr - 3 if n_thr >= 6 else n_thr + 1
                torch.set_num_threads(n_thr2)
                ref2 = RefNet(cfg)
                ref2.load_state_dict(init_state)
                opt2 = torch.optim.Adam(ref2.parameters(), lr=1e-3)
                t2 = time.perf_counter()
                for c0 in range(0, n_k, chunk):
                    n_c = min(chunk, n_k - c0)
                    sl = mine[c0 * B:(c0 + n_c) * B]
                    _, opt2 = solver_ref.train_steps(ref2, MS, PAN, xy_tab[sl], lab_tab[sl], B, P, S, optimizer=opt2)
                m_cpu2, _ = solver_ref.evaluate(ref2, MS, PAN, xy_tab[test[:n_kt]], lab_tab[test[:n_kt]], args.classes + 1, P, S)
                k_cpu2 = aa_oa_quiet(m_cpu2)[2]
                spread = abs(k_cpu - k_cpu2)
                out['kappa'].update({'cpu_second_run_threads': n_thr2, 'cpu_second_run_kappa': k_cpu2, 'cpu_kappa_spread': spread,
                                     'cpu_vs_cpu_confusion_entries_differing': int(np.abs(m_cpu - m_cpu2).sum() // 2),
                                     'abs_delta_kappa_vs_second_cpu_run': abs(k_cpu2 - k_gpu),
                                     # is the GPU run as close to a CPU run as the CPU runs are to each other?
                                     'gpu_within_cpu_run_to_run_spread': bool(min(abs(k_cpu - k_gpu), abs(k_cpu2 - k_gpu)) <= spread),
                                     'within_cpu_spread': bool(abs(k_cpu - k_gpu) <= spread),
                                     'cpu_second_run_seconds': round(time.perf_counter() - t2, 1)})
                torch.set_num_threads(n_thr)
    print(json.dumps(out), flush=True)
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()


def main_stage2(args, dev, pg=None, rank=0, world=1, backend='nccl'):
    """--config 4: the stage-2 step of the two-stage path (solver/tostagesolver.py:259-315): four stacked streams through the
    one-input net, qua_loss, backward, ADAM.  A step processes 4*bs stacked patches per GPU; `value` counts those.
    N ranks: every rank takes bs pixels of each global batch of N*bs, the logits are gathered so that the batch-coupled loss is
    the global batch's, the flat gradient is all-reduced (dmf.engine.QuaTrainEngine); eager launches, no loss scaler."""
    from dmf import lib, synth
    from dmf.engine import LossScaler, QuaScene, QuaTrainEngine
    from function.function import data_padding
    from image_convert.IHS import pan2ms_gpu
    from model.gmfnet import Net
    H = W = args.size
    bs, K_steps, W_steps = args.batch, args.steps, args.warmup
    cfg = {'patch_size': args.patch, 'Categories_Number': args.classes + 1, 'data_city': 's', 'DATA_DICT': {'s': {'size': [H, W, 4]}},
           'gmf': {'width': args.width, 'single_input': 1, 'half': args.half}, 'dqtl': {'alpha': 0.1, 'beta': 0.05, 'gamma': 1.0, 'epsilon': 1e-8, 'tao': 0.1}}
    ms, pan, label = synth.make_scene(H, W, 4, 1, 4, n_classes=args.classes, seed=0)
    pan4 = pan2ms_gpu(pan, [H, W, 4])
    g = np.random.default_rng(1)
    scenes = [data_padding(x, cfg, 'ms') for x in (ms, pan4, ms + 0.1 * g.standard_normal(ms.shape), pan4 + 0.1 * g.standard_normal(pan4.shape))]
    torch.manual_seed(0)
    net = Net(cfg).to(dev)
    init_state = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    scene = QuaScene(scenes, dev, half=bool(args.half))
    sc = LossScaler(dev) if (args.half and args.scaler and world == 1) else None        # GradScaler's defaults (tostagesolver.py:83-84)
    eng = QuaTrainEngine(net, scene, bs, cfg['dqtl'], lr=1e-3, scaler=sc, process_group=pg)
    total = W_steps + K_steps
    xy = np.stack([g.integers(0, H, total * bs * world), g.integers(0, W, total * bs * world)], 1).astype(np.int32)
    lab = np.maximum(label[xy[:, 0], xy[:, 1]], 1).astype(np.int32)
    eng.load_plan(xy, lab)                                 # global batches; the engine keeps this rank's rows
    spg = min(args.steps_per_graph if (args.steps_per_graph or 0) > 0 else (50 if args.steps_per_graph is None else 0), K_steps) if (eng.unit and world == 1) else 0
    # device warm-up that touches no training state (see prewarm()): the eval forward of the first stacked batch, ~60 ms
    inp0 = lib.input_gather(eng.shape, scene.A, scene.B, eng.plan_xy[:4 * bs])
    lg0 = torch.empty_like(eng.logits)
    t_pw = time.perf_counter()
    while (time.perf_counter() - t_pw) * 1e3 < 60.0:
        for _ in range(50):
            lib.forward(eng.shape, inp0, eng.theta, net.pool_w, lg0)
        torch.cuda.synchronize()
    eng.run_plan(W_steps, spg)                  # (the warm-up replays the same graph: see main())
    launch, n_replays = launch_label(spg, K_steps)
    if n_replays and eng.graph is None:
        eng._capture(spg)
    def sync():
        torch.cuda.synchronize()
        if world > 1:
            import torch.distributed as dist
            dist.barrier()
            torch.cuda.synchronize()
    sync()
    t0 = time.perf_counter()
    if n_replays:
        eng.run_plan(K_steps, spg)
    else:
        eng.run_plan(K_steps)
    sync()
    dt = time.perf_counter() - t0
    n_seen = 1
    if world > 1:
        import torch.distributed as dist
        t = torch.tensor([dt], device=dev if backend == 'nccl' else 'cpu', dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
        one = torch.ones(1, device=dev if backend == 'nccl' else 'cpu')
        dist.all_reduce(one)
        n_seen = int(one.item())
    losses = eng.losses().numpy()
    if args.dump_outputs and rank == 0:                  # before the instrumented pass reuses the engine's buffers
        dump_outputs(args.dump_outputs, snapshot_outputs(eng, torch.from_numpy(losses), K_steps))
    if rank != 0:
        if world > 1:
            import torch.distributed as dist
            dist.barrier()
            dist.destroy_process_group()
        return
    P = args.patch
    alg_patch = 2 * ((2 if args.half else 4) * P * P * 4 + 4 * P * P * 1)
    # dominant kernel (--full): the forward(+unit-gradient) patch kernel over the 4*bs stacked patches, HIP events on the launch stream
    kern_ms = None
    if args.full:
        n_inst = min(K_steps, 100)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n_inst)]
        inp = lib.input_gather(eng.shape, scene.A, scene.B, eng.plan_xy[:4 * bs])
        torch.cuda.synchronize()
        for i in range(n_inst):
            ev[i][0].record()
            eng.time_dominant(inp)
            ev[i][1].record()
        torch.cuda.synchronize()
        kern_ms = float(np.mean([a.elapsed_time(b) for a, b in ev[n_inst // 10:]]))
    out = {
        'metric': 'training patches/sec + kappa, 11x11x200 HSI + 11x11x1 SAR, 1/2/4/8 MI355X',
        'value': world * 4 * bs * K_steps / dt, 'unit': 'patches/s', 'n_gpus': world, 'steps': K_steps, 'warmup': W_steps,
        'ms_per_step': dt / K_steps * 1e3, 'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None,
        'dtype': ('f16 scene + spec_a operands, f32 accumulate / gradients / Adam' + (', dynamic loss scale' if args.scaler else ', no loss scale')) if args.half else 'f32',
        'data': 'synthetic',
        'config': {'workload': '%s; %dx%d patches, %d logits, bs %d (%d stacked patches per step), qua_loss, fused HIP step'
                               % (CONFIGS['4']['name'], P, P, args.classes + 1, bs, 4 * bs),
                   'global_batch': 4 * bs * world, 'parallelism': 'dp%d' % world, 'launch': launch,
                   'allreduce': 'none' if world == 1 else '%s all_gather of the logits + all_reduce of one flat fp32 gradient per step' % backend,
                   'n_ranks_seen': n_seen},
        'roofline': {'bound': 'hbm', 'achieved': 4 * bs * alg_patch / (kern_ms * 1e-3) / 1e9, 'peak': HBM_PEAK / 1e9, 'unit': 'GB/s',
                     'frac': 4 * bs * alg_patch / (kern_ms * 1e-3) / HBM_PEAK, 'traffic': None,
                     'kernel': eng.dominant_name(), 'kernel_ms': kern_ms, 'algorithmic_bytes_per_launch': 4 * bs * alg_patch}
                    if kern_ms is not None else None,
        'loss_first_last': [float(losses[0]), float(losses[-1])] if losses.size else None,
    }
    if kern_ms is None:
        del out['roofline']
    if args.full and world == 1 and all(getattr(args, k) == v for k, v in CONFIGS['4'].items() if k != 'name') and eng.unit:
        ir = issue_roofline('4', ', 5, 1, %s>' % ('true' if args.half else 'false'), kern_ms)
        if ir is not None:
            out['issue_roofline'] = ir
    if sc is not None:
        out['loss_scaler'] = {'scale': sc.get_scale(), 'skipped_steps': sc.skipped_steps()}
    if args.full and not args.no_cpu and world == 1:
        from oracle.gmfnet_ref import Net as RefNet
        from oracle import solver_ref
        torch.set_num_threads(min(len(os.sched_getaffinity(0)), 16))
        ref = RefNet(cfg)
        ref.load_state_dict(init_state)
        opt, n_done, t_chunks = None, 0, []
        t_start = time.perf_counter()
        budget = min(args.cpu_seconds, 30.0)
        while n_done < total and time.perf_counter() - t_start < budget:
            n_c = min(5, total - n_done)
            t1 = time.perf_counter()
            _, opt = solver_ref.qua_train_steps(ref, scenes, xy[n_done * bs:(n_done + n_c) * bs], lab[n_done * bs:(n_done + n_c) * bs],
                                                bs, P, cfg['dqtl'], optimizer=opt)
            t_chunks.append((n_c, time.perf_counter() - t1))
            n_done += n_c
        timed = t_chunks[1:] if len(t_chunks) > 1 else t_chunks
        n_t, t_t = sum(n for n, _ in timed), sum(t for _, t in timed)
        out['cpu_baseline'] = {'value': 4 * bs * n_t / t_t, 'unit': 'patches/s', 'cores': torch.get_num_threads(), 'kind': 'port',
                               'sample': '%d stage-2 steps (bs %d) after a warm-up chunk, oracle/solver_ref.py::qua_train_steps, %.1f s timed'
                                         % (n_t, bs, t_t)}
    print(json.dumps(out), flush=True)
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
