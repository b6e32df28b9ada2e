"""GPU: `train.epoch_block` — the two kernels behind it, and `Solver.train()` in blocks of epochs against the
same run epoch by epoch: the same kernels in the same order on bitwise reproducible steps, so step losses, best
weights and the resume checkpoint must agree bit for bit; no host synchronisation while a block is enqueued; `test()` and
`color()` go on from a blocked `train()` as from an unblocked one.
Scene: 40 x 40 pixels, 8 bands + 1 aux band at the same resolution, 5 x 5 patches, width 40, 2 groups (the smallest compiled
shape).  1,122 labelled pixels: 112 train (3 batches of 32 and a short one of 16), 56 validation (batches of 40 and 16)."""
import contextlib
import functools
import os
import shutil
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


# ---------------------------------------------------------------------------------------------- dmf_valid_accum
def _accum_case(n):
    rng = np.random.default_rng(100 + n)
    return [(rng.random(n) * s).astype(np.float32) for s in (1.0, 37.5, 1e-3)]       # non-negative, three magnitudes


@pytest.mark.parametrize('n', [1, 63, 64, 65, 300, 1025, 16384])
def test_valid_accum_is_the_double_sum_in_a_fixed_order(n):
    """Three calls into one acc against numpy's float64 sum in index order; tolerance n * 2^-52 of the sum, the bound for a
    double sum taken in another order (every term is a float32 widened exactly; the terms are non-negative).  A second run
    gives the same bits; n = 0 leaves acc as it is."""
    from dmf import lib
    parts = _accum_case(n)
    want = float(np.cumsum(np.concatenate(parts).astype(np.float64))[-1])          # (cumsum adds in index order)
    got = []
    for _ in range(2):
        acc = torch.zeros(1, dtype=torch.float64, device=DEV)
        for p in parts:
            lib.valid_accum(torch.from_numpy(p).to(DEV), n, acc)
        got.append(acc.cpu().numpy().copy())
    err = abs(float(got[0][0]) - want) / want
    print('n = %d: sum %.17g, relative error %.2e, bound %.2e' % (n, want, err, n * 2.0 ** -52))
    assert err <= n * 2.0 ** -52
    assert got[0].tobytes() == got[1].tobytes()
    acc = torch.full((1,), 2.5, dtype=torch.float64, device=DEV)
    lib.valid_accum(torch.from_numpy(parts[0]).to(DEV), 0, acc)
    assert float(acc.item()) == 2.5
    big = torch.from_numpy(parts[1]).to(DEV)                                       # only the first n terms of a longer vector count
    if n > 1:
        acc.zero_()
        lib.valid_accum(big, n - 1, acc)
        one = torch.zeros(1, dtype=torch.float64, device=DEV)
        lib.valid_accum(big[:n - 1].clone(), n - 1, one)
        assert acc.cpu().numpy().tobytes() == one.cpu().numpy().tobytes()


# ---------------------------------------------------------------------------------------------- dmf_keep_best
SUMS = [5.0, 7.0, 5.0, 3.0, float('nan'), 3.0, 2.0]
KEEPS = {0, 3, 6}                                   # strict `<`: an equal sum and a NaN are never the best


@pytest.mark.parametrize('n,shift', [(1, 0), (255, 0), (8009, 0), (4097, 0), (4097, 1)],
                         ids=['n1', 'n255', 'n8009', 'n4097', 'n4097_not_16_byte_aligned'])
def test_keep_best_keeps_the_first_strictly_smaller_sum_with_its_weights(n, shift):
    from dmf import lib
    rng = np.random.default_rng(n + shift)
    thetas = [torch.from_numpy(rng.standard_normal(n + shift).astype(np.float32)).to(DEV)[shift:] for _ in SUMS]
    acc = torch.zeros(1, dtype=torch.float64, device=DEV)
    best = torch.full((1,), float('inf'), dtype=torch.float64, device=DEV)
    best_epoch = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    guard = torch.full((n + shift + 8,), -7.0, device=DEV)                       # best_theta sits inside it: nothing around it may change
    best_theta = guard[4 + shift:4 + shift + n]
    hist = torch.full((len(SUMS) + 1,), -1.0, dtype=torch.float64, device=DEV)
    kept, kept_epoch, low = None, -1, float('inf')
    for k, v in enumerate(SUMS):
        acc.fill_(v)
        lib.keep_best(acc, best, best_epoch, k, thetas[k], best_theta, hist)
        if k in KEEPS:
            kept, kept_epoch, low = thetas[k], k, v
        assert torch.equal(best_theta, kept), k                                      # bit-equal (no NaN among the weights)
        assert int(best_epoch.item()) == kept_epoch and float(best.item()) == low, k
        assert float(acc.item()) == 0.0, k
    h = hist.cpu().numpy()
    assert np.array_equal(h[:len(SUMS)], np.array(SUMS), equal_nan=True) and h[len(SUMS)] == -1.0
    g = guard.cpu().numpy()
    assert (g[:4 + shift] == -7.0).all() and (g[4 + shift + n:] == -7.0).all()
    with pytest.raises(lib.DmfError, match='outside the validation history'):
        lib.keep_best(acc, best, best_epoch, len(SUMS) + 1, thetas[0], best_theta, hist)


# ---------------------------------------------------------------------------------------------- the solver
SEED = 3407
EPOCHS, SAVE_EVERY, BLOCK = 10, 5, 4                 # blocks of 4, 1, 4, 1 epochs

VARIANTS = {
    'plain_native_loop': {},
    'scheduler': {'schedule': dict(if_scheduler=1, scheduler='ExponentialLR')},
    'criterion_graphs': {'schedule': dict(class_weights='balanced', label_smoothing=0.05), 'steps_per_graph': 2},
    'half': {'gmf': dict(half=1)},
    # the other step forms in scope: the fused step replayed from graphs, the attention network, SGD
    'fused_graphs': {'steps_per_graph': 2},
    'attention': {'gmf': dict(attention=1), 'trans': {'embed_dim': 96, 'num_head': 3}},
    'sgd': {'schedule': dict(optimizer='SGD', lr=0.02, momentum=0.9)},
}


def _cfg(golden_dir, tmp, variant, epoch_block):
    from dmf import synth
    from test_gpu_trajectory import _setup
    _, cfg = _setup(golden_dir, tmp, epoch=EPOCHS, scale=1, batchsize=32, test_batchsize=64, color_batchsize=40,
                    train_rate=0.1, verify_rate=0.05, steps_per_graph=-1)
    primary, aux, label = synth.make_scene(40, 40, 8, 1, 1, n_classes=4, seed=3)
    d = cfg['data_address']
    np.save(d + 'ms4.tif.npy', primary); np.save(d + 'pan.tif.npy', aux); np.save(d + 'label.npy', label)
    cfg['DATA_DICT'][cfg['data_city']]['size'] = [40, 40, 8]
    cfg['train'] = dict(cfg['train'], save_every=SAVE_EVERY, epoch_block=epoch_block)
    cfg['test']['full'] = 1
    for key, val in VARIANTS[variant].items():
        cfg[key] = dict(cfg.get(key) or {}, **val) if isinstance(val, dict) else val
    return cfg


def _read(path):
    with open(path, 'rb') as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def _run(variant, epoch_block, golden_dir, after_train=False):
    """`Solver.train()` once per (variant, epoch_block), shared by the tests below.  Both forms keep the epoch ledger: the
    validation sums in `s.val_history`, the best epoch in `s.best_epoch`."""
    from solver.mainsolver import Solver
    tmp = tempfile.mkdtemp(prefix='dmf_block_')
    try:
        cfg = _cfg(golden_dir, tmp, variant, epoch_block)
        torch.manual_seed(SEED)
        s = Solver(cfg)
        s.dataloader()
        s.train()
        rng_after = torch.rand(4)
        out = cfg['RESULT_output']
        r = dict(step_losses=np.array(s.step_losses, dtype=np.float64), rng_after=rng_after, vals=np.array(s.val_history),
                 best=torch.load(out + '0_weights.pth', map_location='cpu', weights_only=True),
                 cur=torch.load(out + '0_curweights.pth', map_location='cpu', weights_only=True),
                 n_train=len(s.train_index_loader.dataset), n_valid=len(s.valid_index_loader.dataset))
        assert len(s.val_history) == EPOCHS and s.best_epoch is not None             # filled by both forms
        lows = [k for k, v in enumerate(r['vals']) if v < min([np.inf] + list(r['vals'][:k]))]
        assert s.best_epoch == lows[-1] and s.best_loss == r['vals'][lows[-1]]
        r['best_epoch'] = s.best_epoch
        if after_train:
            s.test()
            s.color()
            r.update(matrix=s.test_matrix.copy(), maps=s.label_maps, png=[_read(out + '0_pic_%d.png' % k) for k in (1, 2)])
        return r
    finally:
        shutil.rmtree(tmp)


def _same(a, b, where=''):
    """Bit-equal, through dicts and lists (a checkpoint's weights, optimiser state, step counts and parameter groups)."""
    if isinstance(a, dict):
        assert list(a.keys()) == list(b.keys()), where
        for k in a:
            _same(a[k], b[k], '%s[%r]' % (where, k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for k, (x, y) in enumerate(zip(a, b)):
            _same(x, y, '%s[%d]' % (where, k))
    elif torch.is_tensor(a):
        assert a.dtype == b.dtype and a.shape == b.shape and a.numpy().tobytes() == b.numpy().tobytes(), where
    else:
        assert a == b, where


@pytest.mark.parametrize('variant', sorted(VARIANTS))
def test_blocked_training_equals_training_epoch_by_epoch(golden_dir, variant):
    one = _run(variant, 1, golden_dir, variant == 'plain_native_loop')
    blk = _run(variant, BLOCK, golden_dir, variant == 'plain_native_loop')
    assert one['n_train'] == 112 and one['n_valid'] == 56            # 3 full batches + a short one of 16; validation 40 + 16
    # precondition, so that the best epoch cannot agree by luck: no two validation sums closer than 1e-9 relative
    v = np.sort(one['vals'])
    gap = (np.diff(v) / v[1:]).min()
    print('%s: validation sums %s, smallest relative gap %.2e, best epoch %d' % (variant, one['vals'], gap, one['best_epoch']))
    assert len(v) == EPOCHS and np.isfinite(v).all() and gap > 1e-9
    assert len(one['step_losses']) == EPOCHS * 4
    assert one['step_losses'].tobytes() == blk['step_losses'].tobytes()
    _same(one['best'], blk['best'], 'weights')
    _same(one['cur'], blk['cur'], 'curweights')
    assert one['best_epoch'] == blk['best_epoch']
    rel = np.abs(blk['vals'] - one['vals']) / one['vals']
    print('%s: validation sums, blocked vs epoch by epoch: max relative difference %.2e' % (variant, rel.max()))
    assert rel.max() <= 1e-12
    assert torch.equal(one['rng_after'], blk['rng_after'])         # the RNG stream goes on from the same state


def test_test_and_color_go_on_from_a_blocked_train(golden_dir):
    one = _run('plain_native_loop', 1, golden_dir, True)
    blk = _run('plain_native_loop', BLOCK, golden_dir, True)
    assert one['matrix'].sum() > 0 and np.array_equal(one['matrix'], blk['matrix'])
    assert np.array_equal(one['maps'][0], blk['maps'][0]) and np.array_equal(one['maps'][1], blk['maps'][1])
    assert one['png'] == blk['png'] and len(one['png'][0]) > 0


# ---------------------------------------------------------------------------------------------- no sync inside a block
@contextlib.contextmanager
def _host_reads_raise(monkeypatch):
    """Everything by which the host waits for the device or reads from it raises while this is active."""
    def refuse(name):
        def f(*a, **k):
            raise AssertionError('host synchronisation inside _enqueue_block: %s' % name)
        return f

    def on_device(name):
        inner = getattr(torch.Tensor, name)

        def f(self, *a, **k):
            if self.is_cuda:
                refuse('Tensor.%s of a device tensor' % name)()
            return inner(self, *a, **k)
        return f

    inner_to = torch.Tensor.to

    def to(self, *a, **k):
        target = [x for x in list(a) + [k.get('device')] if isinstance(x, (str, torch.device))]
        if self.is_cuda and any(torch.device(x).type == 'cpu' for x in target):
            refuse('Tensor.to(cpu) of a device tensor')()
        return inner_to(self, *a, **k)

    with monkeypatch.context() as m:
        for name in ('item', 'tolist', 'cpu', 'numpy', '__int__', '__float__', '__bool__', '__index__'):
            m.setattr(torch.Tensor, name, on_device(name))
        m.setattr(torch.Tensor, 'to', to)
        m.setattr(torch.cuda, 'synchronize', refuse('torch.cuda.synchronize'))
        m.setattr(torch.cuda.Stream, 'synchronize', refuse('Stream.synchronize'))
        m.setattr(torch.cuda.Event, 'synchronize', refuse('Event.synchronize'))
        yield


def test_no_host_sync_while_a_block_is_enqueued(golden_dir, monkeypatch):
    """The plain form (library launch loop, constant lr): `_enqueue_block` runs with every host read of a device tensor and
    every synchronize patched to raise; `_collect_block` runs unpatched."""
    from solver.mainsolver import Solver
    tmp = tempfile.mkdtemp(prefix='dmf_block_sync_')
    try:
        cfg = _cfg(golden_dir, tmp, 'plain_native_loop', BLOCK)
        torch.manual_seed(SEED)
        s = Solver(cfg)
        s.dataloader()
        inner, blocks = s._enqueue_block, []

        def guarded(first, n):
            with _host_reads_raise(monkeypatch):
                with pytest.raises(AssertionError, match='host synchronisation'):       # (the guard itself works)
                    torch.zeros(1, device=DEV).item()
                inner(first, n)
            blocks.append(n)
        s._enqueue_block = guarded
        s.train()
        assert blocks == [4, 1, 4, 1]
        want = _run('plain_native_loop', 1, golden_dir, True)
        assert np.array(s.step_losses, dtype=np.float64).tobytes() == want['step_losses'].tobytes()
    finally:
        shutil.rmtree(tmp)
