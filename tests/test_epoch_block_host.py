"""CPU: the host side of `train.epoch_block` — the batch order without the DataLoader against the real index
loader (same rows, same RNG stream afterwards), where the blocks of epochs end, the refusals of the two cases that are out of
scope, and the two new symbols of the C ABI with what they decide before any launch."""
import ctypes as C
import os
import re
import shutil
import tempfile

import numpy as np
import pytest
import torch
from torch.utils.data import Subset

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- the order helper
def _stub_solver(n_pixels=60, n_train=37, n_valid=9, batch=8):
    """A BaseSolver with only what its loaders need: a pixel table of n_pixels rows, a train split of n_train of them (batches
    of `batch`, shuffled) and a validation split (not shuffled)."""
    from solver.basesolver import BaseSolver
    from train.dataset import dataset_dual
    rng = np.random.default_rng(5)
    xyl = (rng.integers(0, 50, (n_pixels, 1)), rng.integers(0, 50, (n_pixels, 1)), rng.integers(1, 5, (n_pixels, 1)).astype(np.float64))
    s = BaseSolver.__new__(BaseSolver)
    s.num_workers = 0
    s.dataset = dataset_dual(None, None, xyl, {'patch_size': 5, 'scale': 1})
    s.index_dataset = s.dataset.index_view()
    rows = rng.permutation(n_pixels)
    s.train_loader, s.train_index_loader = s._loader(Subset(s.dataset, indices=rows[:n_train].tolist()), batch, True)
    s.valid_loader, s.valid_index_loader = s._loader(Subset(s.dataset, indices=rows[n_train:n_train + n_valid].tolist()), batch, False)
    return s


@pytest.mark.parametrize('valid_between', (False, True), ids=('train_only', 'validation_pass_between'))
def test_epoch_streams_are_the_index_loaders_batches_and_rng_stream(valid_between):
    """37 pixels in batches of 8 over three epochs: the same rows in the same order, the short batch of 5 included, and the
    global RNG in the same state afterwards — also when the (unshuffled) validation loader is iterated after every epoch, as
    `train()` does with `save_best`."""
    s = _stub_solver()
    torch.manual_seed(11)
    want = []
    for _ in range(3):
        want.append([(torch.stack([x, y], 1).to(torch.int32), lab.to(torch.int32), idx) for x, y, lab, idx in s.train_index_loader])
        if valid_between:
            for _batch in s.valid_index_loader:
                pass
    tail_want = torch.rand(3)
    assert [len(b[1]) for b in want[0]] == [8, 8, 8, 8, 5]
    assert not torch.equal(want[0][0][2], want[1][0][2])                       # (the epochs are shuffled differently)

    torch.manual_seed(11)
    xy, lab = s._epoch_streams(3, draws_after=1 if valid_between else 0)
    tail_got = torch.rand(3)
    assert xy.shape == (3, 37, 2) and lab.shape == (3, 37) and xy.dtype == lab.dtype == torch.int32
    for e in range(3):
        for k, (bxy, blab, idx) in enumerate(want[e]):
            assert torch.equal(xy[e, 8 * k:8 * k + len(blab)], bxy), (e, k)
            assert torch.equal(lab[e, 8 * k:8 * k + len(blab)], blab), (e, k)
            assert np.array_equal(s.index_dataset.label[idx.numpy()], blab.numpy())
    assert torch.equal(tail_got, tail_want)


def test_epoch_orders_without_epochs_draws_nothing():
    from solver.basesolver import epoch_orders
    torch.manual_seed(3)
    a = torch.rand(2)
    torch.manual_seed(3)
    assert epoch_orders(37, 0).shape == (0, 37)
    assert torch.equal(torch.rand(2), a)


# ---------------------------------------------------------------------------------------------- where the blocks end
def _blocks(epochs, E, every):
    from solver.mainsolver import block_length
    out, e = [], 0
    while e < epochs:
        out.append(block_length(e, E, every, epochs))
        e += out[-1]
    assert e == epochs
    return out


def test_block_boundaries():
    assert _blocks(7, 3, 2) == [2, 2, 2, 1]                 # the checkpoint every 2nd epoch cuts the blocks of 3
    assert _blocks(7, 3, 7) == [3, 3, 1]
    assert _blocks(7, 3, 100) == [3, 3, 1]
    assert _blocks(10, 4, 5) == [4, 1, 4, 1]
    assert _blocks(7, 1, 2) == [1] * 7                      # E = 1
    assert _blocks(7, 3, 1) == [1] * 7                      # save_every 1: every block is one epoch long
    assert _blocks(400, 50, 50) == [50] * 8
    assert _blocks(0, 3, 2) == []
    for epochs, E, every in ((7, 3, 2), (23, 5, 4), (10, 4, 5), (9, 9, 3)):
        ends = np.cumsum(_blocks(epochs, E, every))
        due = [e for e in range(1, epochs + 1) if e % every == 0 or e == epochs]
        assert set(due) <= set(ends.tolist()) and max(_blocks(epochs, E, every)) <= min(E, every)     # every due epoch ends a block


# ---------------------------------------------------------------------------------------------- out of scope: refused
def test_tostagesolver_refuses_epoch_blocks():
    from solver.tostagesolver import toStageSolver
    cfg = {'Categories_Number': 5, 'schedule': {'loss': 'qua_loss', 'optimizer': 'ADAM', 'lr': 1e-3}, 'train': {'epoch_block': 2}}
    with pytest.raises(ValueError, match=r'train\.epoch_block: 2 is out of scope for toStageSolver'):
        toStageSolver(cfg)


def test_data_parallel_and_nonsense_values_are_refused(golden_dir):
    from solver.mainsolver import Solver
    from test_host_cpu import _golden_scene_dir
    tmp = tempfile.mkdtemp(prefix='dmf_block_cpu_')
    try:
        g, cfg = _golden_scene_dir(golden_dir, tmp)
        cfg['device'] = 'cpu'
        cfg['train'] = dict(cfg['train'], epoch_block=2)
        torch.manual_seed(3407)
        s = Solver(cfg)
        assert s._epoch_block() == 2
        s.world = 2
        with pytest.raises(ValueError, match=r'train\.epoch_block: 2 is out of scope for data-parallel runs \(2 ranks'):
            s.train()
        assert s.model is None                                     # refused before anything was built
        s.world = 1
        cfg['train']['epoch_block'] = 0
        assert s._epoch_block() == 1                               # (0 / null: the default)
        cfg['train']['epoch_block'] = -3
        with pytest.raises(ValueError, match='not a positive number'):
            s._epoch_block()
        del cfg['train']['epoch_block']
        assert s._epoch_block() == 1
    finally:
        shutil.rmtree(tmp)


# ---------------------------------------------------------------------------------------------- the C ABI
def test_library_exports_the_two_entry_points_and_the_version_grew():
    from dmf import lib
    hdr = open(os.path.join(REPO, 'include', 'dmf.h')).read()
    assert re.search(r'\bint32_t dmf_valid_accum\s*\(const float\* loss, int32_t n, double\* acc, void\* stream\)', hdr)
    assert re.search(r'\bint32_t dmf_keep_best\s*\(double\* acc, double\* best, int32_t\* best_epoch, int32_t epoch,', hdr)
    so = C.CDLL(lib.LIB_PATH)
    for name in ('dmf_valid_accum', 'dmf_keep_best'):
        assert name in lib.EXPORTS and hasattr(so, name)
    assert lib.version() == int(re.search(r'#define DMF_VERSION (\d+)', hdr).group(1)) >= 304


_BUF = C.create_string_buffer(64)
P = C.c_void_p(C.addressof(_BUF))          # a non-null pointer that no row dereferences
Q = C.c_void_p(C.addressof(_BUF) + 32)

CALLS = [
    ('valid_accum_null_loss', lambda L: L.dmf_valid_accum(None, 4, P, None), 'null argument'),
    ('valid_accum_null_acc', lambda L: L.dmf_valid_accum(P, 4, None, None), 'null argument'),
    ('valid_accum_negative_n', lambda L: L.dmf_valid_accum(P, -1, P, None), 'valid_accum: negative n'),
    ('valid_accum_empty', lambda L: L.dmf_valid_accum(P, 0, P, None), None),
    ('keep_best_null_best', lambda L: L.dmf_keep_best(P, None, P, 0, P, Q, 4, P, None), 'null argument'),
    ('keep_best_null_theta', lambda L: L.dmf_keep_best(P, P, P, 0, None, Q, 4, P, None), 'null argument'),
    ('keep_best_null_hist', lambda L: L.dmf_keep_best(P, P, P, 0, P, Q, 4, None, None), 'null argument'),
    ('keep_best_negative_epoch', lambda L: L.dmf_keep_best(P, P, P, -1, P, Q, 4, P, None), 'keep_best: negative epoch or n'),
    ('keep_best_negative_n', lambda L: L.dmf_keep_best(P, P, P, 0, P, Q, -4, P, None), 'keep_best: negative epoch or n'),
    ('keep_best_in_place', lambda L: L.dmf_keep_best(P, P, P, 0, P, P, 4, P, None), 'keep_best: best_theta must not be theta'),
]


@pytest.mark.parametrize('name,call,message', CALLS, ids=[c[0] for c in CALLS])
def test_entry_points_decide_on_the_host_before_any_launch(name, call, message):
    from dmf import lib
    rc = call(lib._lib)
    if message is None:
        assert rc == 0                      # n == 0: a no-op, nothing is launched
    else:
        assert rc == 1 and lib._lib.dmf_last_error().decode() == message


# ---------------------------------------------------------------------------------------------- the epoch ledger
SUMS = [5.0, 7.0, 5.0, 3.0, float('nan'), 3.0, 2.0]


def test_epoch_ledger_keeps_the_strict_best_and_prints_the_two_lines(capsys):
    """`Solver._record_epoch`, which both the epoch loop and `_collect_block` call: the best epochs are 0, 3, 6 (an equal sum
    and a NaN are never the best, as dmf_keep_best decides), and the lines are the reference's."""
    from solver.mainsolver import Solver
    s = Solver.__new__(Solver)
    s.cfg, s.time, s.step_losses, s.val_history, s.best_loss, s.best_epoch = {'nohup': 1}, 2, [], [], float('inf'), 0
    moved = [s._record_epoch(e, [1.0 + e, 0.5 + e], v) for e, v in enumerate(SUMS)]
    assert moved == [True, False, False, True, False, False, True]
    assert s.best_epoch == 6 and s.best_loss == 2.0
    assert np.array_equal(np.array(s.val_history), np.array(SUMS), equal_nan=True)
    assert s.step_losses == [x + e for e in range(7) for x in (1.0, 0.5)]
    want = []
    for e in range(7):
        want += ['best epoch now is %d' % e] if e in (0, 3, 6) else []
        want += ['2 times %dth epoch is trained, loss %d.500000' % (e, e)]
    assert capsys.readouterr().out == '\n'.join(want) + '\n'
    assert want[:3] == ['best epoch now is 0', '2 times 0th epoch is trained, loss 0.500000', '2 times 1th epoch is trained, loss 1.500000']
    # no validation (no save_best), an epoch without a step, and nohup: 0
    assert s._record_epoch(7, [], None) is False and len(s.val_history) == 7 and s.best_epoch == 6
    assert capsys.readouterr().out == '2 times 7th epoch is trained, loss nan\n'
    s.cfg = {'nohup': 0}
    assert s._record_epoch(8, [0.25], 1.0) is True and s.best_epoch == 8 and s.step_losses[-1] == 0.25
    assert capsys.readouterr().out == ''


@pytest.mark.parametrize('epochs,every,due', [(7, 2, [2, 4, 6, 7]), (10, 5, [5, 10]), (7, 1, [1, 2, 3, 4, 5, 6, 7])])
def test_curweights_are_due_every_nth_epoch_and_after_the_last(epochs, every, due, monkeypatch):
    """`Solver._save_current`, which both forms call after their finished epochs, with the checkpoint writer recorded."""
    from solver import mainsolver
    written = []
    monkeypatch.setattr(mainsolver, 'save_checkpoint', lambda model, opt, path: written.append(path))
    s = mainsolver.Solver.__new__(mainsolver.Solver)
    s.cfg, s.rank, s.fast, s.EPOCH, s.time = {'train': {'save_every': every}, 'RESULT_output': 'out/'}, 0, False, epochs, 3
    s.cur_model = s.optimizer = None
    got = []
    for done in range(1, epochs + 1):
        s._save_current(done)
        got += [done] * len(written)
        del written[:]
    assert got == due
    s._save_current(due[0])
    assert written == ['out/3_curweights.pth']
    s.rank = 1
    s._save_current(due[0])
    assert len(written) == 1                                                       # rank 0 writes the artefacts
    assert set(due) <= set(np.cumsum(_blocks(epochs, 4, every)).tolist())          # a block ends wherever the file is due
