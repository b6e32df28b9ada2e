"""CPU: the host side of class weights, label smoothing and focal loss — the C ABI's new symbol, the config
keys under `schedule`, `utils.make_loss`, `balanced` weights, and every refusal that needs no GPU."""
import ctypes
import os
import re
import shutil
import tempfile

import numpy as np
import pytest
import torch

import loss_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(K=5, **keys):
    return {'Categories_Number': K, 'schedule': dict({'loss': 'Criterion', 'optimizer': 'ADAM', 'lr': 1e-3}, **keys)}


def test_library_exports_dmf_ce_loss_and_the_version_grew():
    from dmf import lib
    hdr = open(os.path.join(REPO, 'include', 'dmf.h')).read()
    assert re.search(r'\bint32_t dmf_ce_loss\s*\(', hdr) and 'typedef struct dmf_ce_params' in hdr
    assert 'dmf_ce_loss' in lib.EXPORTS and hasattr(ctypes.CDLL(lib.LIB_PATH), 'dmf_ce_loss')
    assert lib.version() == int(re.search(r'#define DMF_VERSION (\d+)', hdr).group(1)) >= 303
    assert ctypes.sizeof(lib.CeParams) == 12
    p = lib.ce_params('focal', gamma=2.0)
    assert (p.kind, p.label_smoothing, p.gamma) == (1, 0.0, 2.0) and lib.ce_params().kind == 0
    with pytest.raises(lib.DmfError, match='kind'):
        lib.ce_params('hinge')


def test_make_loss_without_the_keys_is_todays_criterion():
    from utils.utils import criterion_spec, make_loss
    cfg = _cfg()
    crit = make_loss('Criterion', cfg)
    assert type(crit) is torch.nn.CrossEntropyLoss and crit.weight is None and crit.label_smoothing == 0.0
    assert criterion_spec(cfg) is None
    assert type(make_loss('MSE', cfg)) is torch.nn.MSELoss


@pytest.mark.parametrize('keys', [dict(class_weights=[0.5, 2.0, 1.0, 7.0, 0.01]), dict(label_smoothing=0.1),
                                  dict(class_weights=[0.5, 2.0, 1.0, 7.0, 0.01], label_smoothing=0.2),
                                  dict(focal_gamma=2), dict(focal_gamma=1.5, class_weights=[0.5, 2.0, 1.0, 7.0, 0.01]),
                                  dict(focal_gamma=0, label_smoothing=0, class_weights=[1.0] * 5)])
def test_make_loss_with_keys_matches_the_float64_statement(keys):
    from utils.utils import FocalLoss, criterion_spec, make_loss
    cfg = _cfg(**keys)
    crit = make_loss('Criterion', cfg)
    spec = criterion_spec(cfg)
    focal = bool(keys.get('focal_gamma'))
    assert type(crit) is (FocalLoss if focal else torch.nn.CrossEntropyLoss) and spec['kind'] == ('focal' if focal else 'ce')
    g = torch.Generator().manual_seed(3)
    z = (2.0 * torch.randn(40, 5, generator=g)).requires_grad_(True)
    y = torch.randint(0, 5, (40,), generator=g)
    z.data[0, y[0]] = 25.0
    v = crit(z, y)
    v.backward()
    w = keys.get('class_weights')
    want_v, want_g = loss_ref.value_and_grad(z, y, torch.float64, kind=spec['kind'], weight=None if w is None else torch.tensor(w, dtype=torch.float32),
                                             eps=float(keys.get('label_smoothing') or 0), gamma=float(keys.get('focal_gamma') or 0))
    assert abs(v.item() - want_v.item()) < 1e-5 * max(1.0, abs(want_v.item()))
    assert (z.grad.double() - want_g).abs().max().item() < 1e-6


def test_neutral_keys_keep_the_plain_criterion():
    """Keys that are stated but neutral must not move a run off the fused step: no spec, today's module."""
    from utils.utils import criterion_spec, make_loss
    for keys in (dict(label_smoothing=0), dict(focal_gamma=0.0, label_smoothing=0.0, class_weights=None), dict(class_weights=None)):
        cfg = _cfg(**keys)
        assert criterion_spec(cfg) is None
        crit = make_loss('Criterion', cfg)
        assert type(crit) is torch.nn.CrossEntropyLoss and crit.weight is None and crit.label_smoothing == 0.0
    with pytest.raises(ValueError, match=r'not in \[0, 1\)'):          # (a bad value is still refused)
        criterion_spec(_cfg(label_smoothing=2, class_weights=None))


def test_value_bound_against_once_rounded_float64_terms():
    """The bound of the kernel test on the best output a float32 `loss[i]` allows — per-sample terms computed in float64 and
    rounded ONCE — over the kernel test's own 720 evaluations.  The issue's bare bound, 4 x the evaluation's float32 deviation +
    1e-7, is missed by some of them (counted and printed: DESIGN.md §12 quotes the count); with the storage term of
    loss_ref.value_bound it holds for all, with the half ulp per row that is that term's whole reason."""
    bare, total, worst = [], 0, 0.0
    for K in loss_ref.KS:
        for bs_r in loss_ref.BS_RS:
            y, sets, w_all = loss_ref.case(K, bs_r)
            for name, z in sets.items():
                for vname, spec, weighted in loss_ref.VARIANTS:
                    ref = loss_ref.ref_spec(spec, w_all if weighted else None)
                    v64, _ = loss_ref.value_and_grad(z, y, torch.float64, **ref)
                    v32, _ = loss_ref.value_and_grad(z, y, torch.float32, **ref)
                    t, D = loss_ref.per_sample_terms(z, y, **ref)
                    assert abs((t.sum() / D).item() - v64.item()) <= 1e-12 * max(1.0, abs(v64.item()))    # the two float64 statements agree
                    loss = (bs_r * t / D).float()
                    err, dev = (loss.double().mean() - v64).abs().item(), (v32 - v64).abs().item()
                    total += 1
                    if err > 4 * dev + 1e-7:
                        bare.append((K, bs_r, name, vname, err, dev))
                    tol = loss_ref.value_bound(dev, loss)
                    worst = max(worst, err / tol)
                    assert err <= tol, (K, bs_r, name, vname, err, dev, tol)
    print('once-rounded float64 terms: %d of %d evaluations miss 4 x float32 deviation + 1e-7 %s; worst error / bound with the storage term %.3f'
          % (len(bare), total, [b[:4] for b in bare], worst))
    assert total == 720 and len(bare) > 0


def test_solver_hands_global_batches_to_the_engine_under_data_parallel():
    """With a criterion the engine shards: `_rank_batches` keeps the global batches (those with a pixel for every rank), a full
    one is batchsize, and `_step_short` reads this rank's rows of the loss; without one the solver shards as before."""
    from solver.mainsolver import Solver

    class Engine:
        def __init__(self):
            self.loss = torch.arange(1.0, 9.0)
            self.seen = None

        def step(self, xy, lab):
            self.seen = (xy.clone(), lab.clone())
    s = Solver.__new__(Solver)
    s.cfg, s.world, s.rank, s.DEVICE = {'batchsize': 8}, 2, 1, 'cpu'
    s.engine = Engine()
    batches = [(torch.arange(16).view(8, 2).int(), torch.arange(8).int()), (torch.arange(10).view(5, 2).int(), torch.arange(5).int()),
               (torch.zeros(1, 2).int(), torch.zeros(1).int())]
    s.criterion = {'kind': 'ce'}
    got, full = s._rank_batches(batches)
    assert full == 8 and len(got) == 2 and all(torch.equal(g[0], b[0]) and torch.equal(g[1], b[1]) for g, b in zip(got, batches))
    val = s._step_short(*batches[1])                                    # 5 pixels, 2 ranks: 2 rows each
    assert torch.equal(s.engine.seen[0], batches[1][0]) and torch.equal(s.engine.seen[1], batches[1][1])
    assert val == pytest.approx(float(s.engine.loss[:2].mean()))
    s.criterion = None
    got, full = s._rank_batches(batches)
    assert full == 4 and len(got) == 2 and torch.equal(got[0][0], batches[0][0][4:8]) and torch.equal(got[1][1], batches[1][1][2:4])
    assert s._step_short(*got[1]) == pytest.approx(float(s.engine.loss[:2].mean()))


def test_balanced_weights_on_a_hand_made_split():
    from utils.utils import balanced_weights, criterion_spec
    labels = [1] * 6 + [2] * 3 + [4] * 1                       # 10 train pixels, classes 0 and 3 absent
    w = balanced_weights(labels, 5)
    assert np.allclose(w, [1.0, 10 / (3 * 6), 10 / (3 * 3), 1.0, 10 / (3 * 1)], rtol=1e-15)
    spec = criterion_spec(_cfg(class_weights='balanced', label_smoothing=0.05), np.array(labels, dtype=np.float64))
    assert spec == {'kind': 'ce', 'label_smoothing': 0.05, 'gamma': 0.0, 'class_weights': w}
    with pytest.raises(ValueError, match='train split'):
        criterion_spec(_cfg(class_weights='balanced'))


def test_solver_computes_balanced_weights_from_its_train_split(golden_dir):
    """`Solver.dataloader()` makes the criterion of its split; `fast_path: 0` trains with the torch module of the same numbers."""
    from solver.mainsolver import Solver
    from test_host_cpu import _golden_scene_dir
    from utils.utils import balanced_weights
    tmp = tempfile.mkdtemp(prefix='dmf_crit_cpu_')
    try:
        g, cfg = _golden_scene_dir(golden_dir, tmp)
        cfg['device'] = 'cpu'
        cfg['schedule'] = dict(cfg['schedule'], class_weights='balanced', label_smoothing=0.05)
        torch.manual_seed(3407)
        s = Solver(cfg)
        assert s.criterion is None
        s.dataloader()
        train_labels = g['label'].reshape(-1)[g['labelled'][g['split_train']]]      # (the pixel table is row-major)
        want = balanced_weights(train_labels, 5)
        assert s.criterion['class_weights'] == want and s.criterion['label_smoothing'] == 0.05 and s.criterion['kind'] == 'ce'
        assert len(set(np.round(want, 9))) > 1                    # (the split is not balanced: the weights say something)
        s.init_model()
        assert type(s.loss) is torch.nn.CrossEntropyLoss and s.loss.label_smoothing == 0.05
        assert np.allclose(s.loss.weight.numpy(), np.asarray(want, dtype=np.float32))
    finally:
        shutil.rmtree(tmp)


@pytest.mark.parametrize('keys,msg', [
    (dict(focal_gamma=2, label_smoothing=0.1), 'cannot both be non-zero'),
    (dict(class_weights=[1.0, 2.0]), 'holds 2 weights for Categories_Number 5'),
    (dict(class_weights=[1.0, 0.0, 1.0, 1.0, 1.0]), 'finite and > 0'),
    (dict(class_weights=[1.0, -1.0, 1.0, 1.0, 1.0]), 'finite and > 0'),
    (dict(class_weights=[1.0, float('inf'), 1.0, 1.0, 1.0]), 'finite and > 0'),
    (dict(class_weights=[1.0, float('nan'), 1.0, 1.0, 1.0]), 'finite and > 0'),
    (dict(class_weights='inverse'), 'balanced'),
    (dict(label_smoothing=1.0), r'not in \[0, 1\)'),
    (dict(label_smoothing=-0.5), r'not in \[0, 1\)'),
    (dict(focal_gamma=0.5), 'neither 0 nor >= 1'),
    (dict(focal_gamma=-2), 'neither 0 nor >= 1'),
])
def test_config_refusals(keys, msg):
    from utils.utils import make_loss
    with pytest.raises(ValueError, match=msg):
        make_loss('Criterion', _cfg(**keys))


def test_other_losses_and_tostagesolver_refuse_the_keys():
    from solver.tostagesolver import toStageSolver
    from utils.utils import make_loss
    with pytest.raises(ValueError, match='schedule.loss: Criterion'):
        make_loss('MSE', _cfg(label_smoothing=0.1))
    for key, val in (('class_weights', 'balanced'), ('label_smoothing', 0.1), ('focal_gamma', 2)):
        cfg = _cfg(**{key: val})
        cfg['schedule']['loss'] = 'qua_loss'
        with pytest.raises(ValueError, match='schedule.%s belongs to schedule.loss: Criterion' % key):
            toStageSolver(cfg)
        cfg['schedule']['loss'] = 'Criterion'                   # (stage 2 trains with qua_loss whatever the key says)
        with pytest.raises(ValueError, match='toStageSolver'):
            toStageSolver(cfg)


@pytest.mark.parametrize('spec,msg', [
    (dict(class_weights=[1.0, 0.0, 1.0]), 'finite and > 0'),
    (dict(class_weights=[1.0, 1e-60, 1.0]), 'finite and > 0'),          # > 0 as float64, 0 as the float32 the kernel reads
    (dict(class_weights=[1.0, float('nan'), 1.0]), 'finite and > 0'),
    (dict(class_weights=[1.0, 1.0]), '2 weights for 3 classes'),
    (dict(label_smoothing=1.0), 'label_smoothing'),
    (dict(kind='focal', gamma=0.3), 'gamma'),
    (dict(kind='focal', gamma=2.0, label_smoothing=0.1), 'label smoothing belongs to kind ce'),
    (dict(kind='hinge'), 'kind'),
])
def test_engine_criterion_refusals(spec, msg):
    """dmf.engine.Criterion, which both engines build from the spec (the engines themselves need a GPU)."""
    from dmf import lib
    from dmf.engine import Criterion
    with pytest.raises(lib.DmfError, match=msg):
        Criterion(spec, 3, 'cpu')
    ok = Criterion(dict(kind='focal', gamma=2.0, class_weights=[1.0, 2.0, 3.0]), 3, 'cpu')
    assert ok.params.kind == 1 and ok.class_w.dtype == torch.float32 and ok.class_w.tolist() == [1.0, 2.0, 3.0]
    assert Criterion({}, 3, 'cpu').class_w is None
