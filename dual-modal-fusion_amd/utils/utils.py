"""utils.utils — optimiser / loss / scheduler factories and checkpoint helpers (mirror of the reference module).

The three factories return the torch objects the reference builds from the same cfg keys (utils/utils.py:8-71):
`ADAM` is `torch.optim.Adam(params, lr)` with every other default, `Criterion` is `nn.CrossEntropyLoss()`, and the eight
scheduler kinds keep the reference's constants.  Here they are lookup tables of small constructors rather than
if-chains.  They serve the drop-in path (reference-style loop -> `model.gmfnet.Net` -> autograd); the resident-scene
fast path (dmf/engine.py) applies the same ADAM update inside `dmf_grad_reduce_adam` and takes only the hyper-parameters
from here (`adam_hparams`, `epoch_hparams`: whatever scheduler kind is configured).  This project's own optional keys on top of
the reference's: the criterion keys (`criterion_spec`), and `weight_decay`, `optimizer: ADAMW`, `clip_grad_norm` (`optim_hparams`).  Checkpoints keep the reference's layout (:82-111): `{'state_dict', 'optimizer'}`.
"""
import os
import random

import numpy as np
import torch
from torch import nn
from torch.optim import lr_scheduler as _sched

_ADAM_DEFAULTS = ((0.9, 0.999), 1e-8)          # betas, eps of torch.optim.Adam — the reference passes lr only (:12)


def weight_decay_of(s):
    """schedule.weight_decay (NEW, optional): torch's `weight_decay=` — L2 for ADAM, SGD and RMSprop, decoupled for ADAMW,
    which must state it.  Absent, null and 0 are neutral."""
    if s['optimizer'] == 'ADAMW' and s.get('weight_decay') is None:
        raise ValueError('schedule.optimizer: ADAMW needs schedule.weight_decay stated (torch.optim.AdamW(params, lr, weight_decay))')
    wd = float(s.get('weight_decay') or 0.0)
    if not (np.isfinite(wd) and wd >= 0.0):
        raise ValueError('schedule.weight_decay %r is not a finite number >= 0' % (s.get('weight_decay'),))
    return wd


def clip_grad_norm_of(s):
    """schedule.clip_grad_norm (NEW, optional): max_norm of `torch.nn.utils.clip_grad_norm_(params, max_norm)` between backward
    and step, or None: absent, null and 0 switch it off."""
    c = float(s.get('clip_grad_norm') or 0.0)
    if not (np.isfinite(c) and c >= 0.0):
        raise ValueError('schedule.clip_grad_norm %r is not a finite number > 0 (null or 0: off)' % (s.get('clip_grad_norm'),))
    return c or None


# (a neutral weight_decay is not passed on: the reference's own constructor calls stay as they are)
def _wd(s):
    wd = weight_decay_of(s)
    return {'weight_decay': wd} if wd else {}


_OPTIMIZERS = {
    'ADAM': lambda s, params: torch.optim.Adam(params, lr=s['lr'], **_wd(s)),
    'ADAMW': lambda s, params: torch.optim.AdamW(params, lr=s['lr'], weight_decay=weight_decay_of(s)),
    'SGD': lambda s, params: torch.optim.SGD(params, lr=s['lr'], momentum=s['momentum'], **_wd(s)),
    'RMSprop': lambda s, params: torch.optim.RMSprop(params, lr=s['lr'], alpha=s['alpha'], **_wd(s)),
}


def _qua():
    from train.loss_function import qua_loss      # imported late: it binds the HIP library
    return qua_loss()


_LOSSES = {
    'MSE': lambda: nn.MSELoss(reduction='mean'),
    'L1': lambda: nn.L1Loss(reduction='mean'),
    'Criterion': nn.CrossEntropyLoss,
    'KL': lambda: nn.KLDivLoss(reduction='batchmean'),
    'qua_loss': _qua,
}


def _warmup(opt):
    return _sched.LinearLR(opt, start_factor=0.1, end_factor=1, total_iters=10)


def _decay(opt):
    return _sched.ExponentialLR(optimizer=opt, gamma=0.98)


# every entry: (optimizer, cfg['schedule'], cfg) -> scheduler; `ratio` = base_lr / lr as the reference forms it
_SCHEDULERS = {
    'StepLR': lambda o, s, c: _sched.StepLR(o, step_size=50, gamma=s['base_lr'] / s['lr']),
    'LinearLR': lambda o, s, c: _warmup(o),
    'CosineAnnealingLR': lambda o, s, c: _sched.CosineAnnealingLR(o, 50, s['base_lr']),
    'CyclicLR': lambda o, s, c: _sched.CyclicLR(o, base_lr=s['base_lr'], max_lr=s['lr'], step_size_up=10,
                                                step_size_down=40, cycle_momentum=False),
    'OneCycleLR': lambda o, s, c: _sched.OneCycleLR(o, max_lr=s['lr'], pct_start=0.5, total_steps=c['epoch'],
                                                    div_factor=s['lr'] / s['base_lr'],
                                                    final_div_factor=s['lr'] / s['base_lr']),
    'ConstantLR': lambda o, s, c: _sched.ConstantLR(o, factor=s['base_lr'] / s['lr'], total_iters=10),
    'ChainedScheduler': lambda o, s, c: _sched.ChainedScheduler([_warmup(o), _decay(o)]),
    'ExponentialLR': lambda o, s, c: _decay(o),
}


def _pick(table, key, what):
    try:
        return table[key]
    except KeyError:
        raise ValueError('%s %r is not one of %s' % (what, key, sorted(table))) from None


def make_optimizer(cfg, params):
    """The torch optimiser of cfg['schedule'] (optimizer, lr, momentum / alpha, weight_decay).  schedule.clip_grad_norm is no
    part of it: the train loops call `clip_grad_norm_` (clip_grad_norm_of), the fast path clips inside dmf_optim_step."""
    clip_grad_norm_of(cfg['schedule'])
    return _pick(_OPTIMIZERS, cfg['schedule']['optimizer'], 'optimizer')(cfg['schedule'], params)


CRITERION_KEYS = ('class_weights', 'label_smoothing', 'focal_gamma')      # optional keys of cfg['schedule'] (NEW)


def criterion_keys(cfg):
    """The criterion keys that cfg['schedule'] states."""
    return [k for k in CRITERION_KEYS if k in (cfg.get('schedule') or {})]


def balanced_weights(labels, K):
    """`class_weights: balanced`: w_c = n / (n_present * n_c) for the classes present among `labels` (n of them, n_present
    distinct), 1 for the absent ones."""
    counts = np.bincount(np.asarray(labels).reshape(-1).astype(np.int64), minlength=K)[:K].astype(np.float64)
    present = counts > 0
    w = np.ones(K)
    w[present] = counts.sum() / (present.sum() * counts[present])
    return w.tolist()


def criterion_spec(cfg, train_labels=None):
    """cfg['schedule'] -> dict(kind, label_smoothing, gamma, class_weights) as dmf.engine.Criterion and `criterion_module` take
    it, or None when none of the keys is stated or every stated one has its neutral value (`class_weights: null`, 0, 0): then
    everything stays the plain cross-entropy and the fused step.  train_labels: the train
    split's labels, which `class_weights: balanced` is computed from."""
    if not criterion_keys(cfg):
        return None
    s, K = cfg['schedule'], int(cfg['Categories_Number'])
    eps, gamma = float(s.get('label_smoothing') or 0.0), float(s.get('focal_gamma') or 0.0)
    if eps != 0.0 and gamma != 0.0:
        raise ValueError('schedule.focal_gamma and schedule.label_smoothing cannot both be non-zero (got %g and %g)' % (gamma, eps))
    if not 0.0 <= eps < 1.0:
        raise ValueError('schedule.label_smoothing %g is not in [0, 1)' % eps)
    if not (gamma == 0.0 or (gamma >= 1.0 and np.isfinite(gamma))):
        raise ValueError('schedule.focal_gamma %g is neither 0 nor >= 1' % gamma)
    w = s.get('class_weights')
    if isinstance(w, str):
        if w != 'balanced':
            raise ValueError('schedule.class_weights: %r is neither a list of %d floats nor balanced' % (w, K))
        if train_labels is None:
            raise ValueError('schedule.class_weights: balanced is computed from the train split, which does not exist yet')
        w = balanced_weights(train_labels, K)
    elif w is not None:
        w = [float(x) for x in w]
        if len(w) != K:
            raise ValueError('schedule.class_weights holds %d weights for Categories_Number %d' % (len(w), K))
    if w is not None and not all(np.isfinite(x) and x > 0 for x in w):
        raise ValueError('schedule.class_weights must be finite and > 0, got %s' % w)
    if w is None and eps == 0.0 and gamma == 0.0:
        return None                # every key at its neutral value: the plain cross-entropy, which the fused step trains
    return {'kind': 'focal' if gamma != 0.0 else 'ce', 'label_smoothing': eps, 'gamma': gamma, 'class_weights': w}


class FocalLoss(nn.Module):
    """sum_i w[y_i] (1 - p_i)^gamma (-log p_i) / sum_i w[y_i], p_i = softmax(output_i)[y_i]: the focal loss with class weights,
    averaged like nn.CrossEntropyLoss(weight=w) (gamma = 0 is that loss).  1 - p_i is formed as the sum of the other classes'
    probabilities, which stays accurate when p_i -> 1."""

    def __init__(self, gamma, weight=None):
        super().__init__()
        self.gamma = float(gamma)
        self.register_buffer('weight', weight)

    def forward(self, output, target):
        logp = torch.log_softmax(output, dim=1)
        hit = torch.zeros_like(logp, dtype=torch.bool).scatter_(1, target.view(-1, 1), True)
        q = logp.exp().masked_fill(hit, 0.0).sum(1)
        w = self.weight[target] if self.weight is not None else torch.ones_like(q)
        nlp = -logp.gather(1, target.view(-1, 1)).squeeze(1)
        return (w * q.pow(self.gamma) * nlp).sum() / w.sum()


def criterion_module(spec):
    """The torch module of a criterion_spec: nn.CrossEntropyLoss(weight=, label_smoothing=) or FocalLoss."""
    w = None if spec['class_weights'] is None else torch.tensor(spec['class_weights'], dtype=torch.float32)
    if spec['kind'] == 'focal':
        return FocalLoss(spec['gamma'], w)
    return nn.CrossEntropyLoss(weight=w, label_smoothing=spec['label_smoothing'])


def make_loss(loss_type, cfg, train_labels=None):
    """schedule.loss as a torch module.  `Criterion` with criterion keys in cfg['schedule'] (class_weights, label_smoothing,
    focal_gamma): criterion_module(criterion_spec(cfg, train_labels)); no other loss takes those keys."""
    make = _pick(_LOSSES, loss_type, 'loss')
    if criterion_keys(cfg):
        if loss_type != 'Criterion':
            raise ValueError('schedule.%s belongs to schedule.loss: Criterion, not %s' % (criterion_keys(cfg)[0], loss_type))
        spec = criterion_spec(cfg, train_labels)
        if spec is not None:
            return criterion_module(spec)
    return make()


def make_scheduler(optimizer, cfg, total=None):
    """total: the number of scheduler steps of the run where that is not cfg['epoch'] (`scheduler_unit: step`: epochs x steps
    per epoch) — OneCycleLR's total_steps."""
    s = cfg['schedule']
    if not s['if_scheduler']:
        return None
    return _pick(_SCHEDULERS, s['scheduler'], 'scheduler')(optimizer, s, cfg if total is None else dict(cfg, epoch=int(total)))


SCHEDULER_UNITS = ('epoch', 'step')


def schedule_keys(cfg, fast=False):
    """(device_schedule, scheduler_unit) of cfg['schedule'] (both NEW, optional; defaults 0 and epoch).
    device_schedule: 1 — the fast path keeps lr, betas and momentum of the whole run in a table on the device
    (`schedule_table`, dmf.engine set_schedule): a captured graph and the library's launch loop follow the scheduler without a
    re-capture.  scheduler_unit: step — `scheduler.step()` after every optimiser step (torch's OneCycleLR / CyclicLR / warm-up
    usage) instead of once per epoch; on the fast path (`fast`) only the device table can change lr inside a graph or the
    launch loop, so it requires device_schedule: 1."""
    s = cfg['schedule']
    dev = bool(int(s.get('device_schedule', 0) or 0))
    unit = s.get('scheduler_unit') or 'epoch'
    if unit not in SCHEDULER_UNITS:
        raise ValueError('schedule.scheduler_unit %r is not one of %s' % (unit, ', '.join(SCHEDULER_UNITS)))
    if unit == 'step' and fast and not dev:
        raise ValueError('schedule.scheduler_unit: step on the fast path requires schedule.device_schedule: 1 (lr is a launch '
                         'argument there and cannot change inside a captured graph or the launch loop); set it, or fast_path: 0')
    return dev, unit


AVERAGE_KINDS = ('none', 'ema', 'mean')


def averaging_keys(cfg):
    """schedule.weight_average / average_decay / average_start (all NEW, optional) -> None, or (kind, decay, start_epochs):
    an averaged copy of the weights in the role of `torch.optim.swa_utils.AveragedModel`, updated after every optimiser step —
    `ema` with `get_ema_multi_avg_fn(average_decay)` (default 0.999), `mean` with its default equal average —, from the first
    step after `average_start` epochs (default 0) on, and a copy of the weights until then.  With it validation, the best
    weights and therefore test() / color() use the averaged weights."""
    s = cfg['schedule']
    kind = s.get('weight_average') or 'none'
    if kind not in AVERAGE_KINDS:
        raise ValueError('schedule.weight_average %r is not one of %s' % (kind, ', '.join(AVERAGE_KINDS)))
    if kind == 'none':
        return None
    decay = float(s.get('average_decay', 0.999))
    start = s.get('average_start', 0) or 0
    if not 0.0 <= decay < 1.0:
        raise ValueError('schedule.average_decay %r is not in [0, 1)' % (s.get('average_decay'),))
    if int(start) != start or start < 0:
        raise ValueError('schedule.average_start %r is not a whole number of epochs >= 0' % (start,))
    return kind, decay, int(start)


def average_update_(avg, params, kind, decay, start_step, step):
    """`AveragedModel.update_parameters` on lists of tensors, with torch's own ops: `step` is the 1-based count of the optimiser
    step just taken; step <= start_step copies (step == start_step is AveragedModel's first update), later steps
    `_foreach_lerp_` with 1 - decay (`get_ema_multi_avg_fn`) or 1 / (num_averaged + 1) (the default equal average)."""
    with torch.no_grad():
        if step <= start_step:
            torch._foreach_copy_(avg, params)
        else:
            torch._foreach_lerp_(avg, params, 1.0 - decay if kind == 'ema' else 1.0 / (step - start_step + 1))


def optim_hparams(cfg):
    """What the resident-scene engine needs to reproduce make_optimizer(cfg, ...): kind + the constructor arguments the
    reference passes (ADAM: lr; SGD: lr, momentum; RMSprop: lr, alpha — utils/utils.py:10-16), torch defaults otherwise; and
    this project's own keys where cfg['schedule'] states them: ADAMW, `weight_decay` (0.0 = none) and `clip_grad_norm` (None =
    off).  A schedule without the keys gives the dict it always gave; read them with .get(key)."""
    s = cfg['schedule']
    kind = s['optimizer']
    _pick(_OPTIMIZERS, kind, 'optimizer')
    out = {'optimizer': kind, 'lr': float(s['lr']), 'betas': _ADAM_DEFAULTS[0], 'eps': _ADAM_DEFAULTS[1]}
    wd, clip = weight_decay_of(s), clip_grad_norm_of(s)
    if 'weight_decay' in s:
        out['weight_decay'] = wd
    if 'clip_grad_norm' in s:
        out['clip_grad_norm'] = clip
    if kind == 'SGD':
        out['momentum'] = float(s['momentum'])
    if kind == 'RMSprop':
        out['alpha'] = float(s['alpha'])
    return out


def adam_hparams(cfg):
    """(lr, betas, eps) of the ADAM the reference constructs: lr from cfg, torch defaults otherwise."""
    if cfg['schedule']['optimizer'] != 'ADAM':
        raise ValueError('the fused HIP step implements ADAM only; got %s' % cfg['schedule']['optimizer'])
    return (float(cfg['schedule']['lr']),) + _ADAM_DEFAULTS


class _Schedule:
    """The per-epoch hyper-parameters the reference's own scheduler object would give its optimiser.

    The fused step takes lr / betas as launch arguments, so instead of re-deriving each of the eight scheduler kinds in
    closed form, the SAME torch scheduler (make_scheduler) is driven on a one-element dummy optimiser (make_optimizer: the
    same class and defaults) and its parameter group is read after every `scheduler.step()` — exactly the sequence the
    reference sees (mainsolver.py:60: one step per epoch).  OneCycleLR also cycles ADAM's beta1; that comes along."""

    def __init__(self, cfg, total=None):
        self.cfg = cfg
        self.param = torch.nn.Parameter(torch.zeros(1))
        self.opt = make_optimizer(cfg, [self.param])
        self.sched = make_scheduler(self.opt, cfg, total)
        self.seq = [self._group()]

    def _group(self):
        g = self.opt.param_groups[0]
        return {k: (tuple(v) if isinstance(v, (tuple, list)) else v) for k, v in g.items() if k != 'params'}

    def at(self, epoch):
        while len(self.seq) <= epoch:
            if self.sched is not None:
                self.opt.step()                   # (keeps torch's "scheduler before optimizer" warning quiet; the gradient is None)
                self.sched.step()
            self.seq.append(self._group())
        return self.seq[epoch]


_SCHEDULES = {}


def epoch_hparams(cfg, epoch):
    """Optimiser parameter group (lr, betas, ...) in force during epoch `epoch` (0-based), any scheduler kind."""
    key = id(cfg)
    sch = _SCHEDULES.get(key)
    if sch is None or sch.cfg is not cfg:
        sch = _SCHEDULES[key] = _Schedule(cfg)
    return sch.at(epoch)


def schedule_groups(cfg, rows, unit='epoch'):
    """The optimiser parameter groups (lr, betas, momentum ... as torch holds them) of `rows` consecutive scheduler steps:
    group i is in force after i calls of `scheduler.step()` — epoch i with unit 'epoch' (`epoch_hparams(cfg, i)`), optimiser
    step i + 1 with unit 'step', where the scheduler is built for `rows` steps in all (make_scheduler's `total`).
    schedule.if_scheduler: 0 gives one group."""
    if unit not in SCHEDULER_UNITS:
        raise ValueError('scheduler unit %r is not one of %s' % (unit, ', '.join(SCHEDULER_UNITS)))
    if rows < 1:
        raise ValueError('a schedule needs at least one row, got %d' % rows)
    sch = _Schedule(cfg, int(rows) if unit == 'step' else None)
    return [dict(sch.at(i)) for i in range(int(rows) if sch.sched is not None else 1)]


def schedule_table(cfg, rows, unit='epoch'):
    """float32 [rows, 4], row = (lr, beta1, beta2, momentum) of schedule_groups(cfg, rows, unit): the table that
    dmf.engine's set_schedule uploads.  A value the optimiser kind does not have is torch's ADAM default for the betas and 0
    for momentum; the kernels do not read it.  Every value is the float32 that the launch argument of the same step would be."""
    groups = schedule_groups(cfg, rows, unit)
    out = np.empty((len(groups), 4), dtype=np.float32)
    for i, g in enumerate(groups):
        b1, b2 = g.get('betas', _ADAM_DEFAULTS[0])
        out[i] = (g['lr'], b1, b2, g.get('momentum', 0.0) or 0.0)
    return out


def epoch_lr(cfg, epoch):
    """Learning rate after `epoch` scheduler steps, for the fused step (every scheduler kind of make_scheduler)."""
    return float(epoch_hparams(cfg, epoch)['lr'])


def export_optimizer(cfg, params, flat_params, offsets, m, v, step_count, group=None):
    """The torch optimiser `make_optimizer(cfg, params)` would be after `step_count` steps, filled from the resident-scene
    engine's flat state vectors — so that `<time>_curweights.pth` holds what the reference's `save_checkpoint(model,
    optimizer)` stores (utils/utils.py:82-88) and `load_checkpoint` (:91-102) can feed it to `make_optimizer(cfg)` again.
    Per optimiser kind (torch's own state keys):
      ADAM     m -> exp_avg, v -> exp_avg_sq, step    (ADAMW: the same keys in a torch.optim.AdamW)
      SGD      m -> momentum_buffer (only when momentum != 0 and a step has been taken, as torch creates it)
      RMSprop  m -> square_avg, step
    params: `model.parameters()` — the order the reference hands to make_optimizer, which is the order a state_dict numbers
    them in; flat_params / offsets: the same nn.Parameters in flat-vector order with their start in m / v; group:
    hyper-parameters in force (lr after the scheduler, OneCycleLR's betas / momentum) written into the parameter group."""
    opt = make_optimizer(cfg, list(params))
    kind = cfg['schedule']['optimizer']
    if group:
        for k, val in group.items():
            if k in opt.param_groups[0] and k != 'params':
                opt.param_groups[0][k] = val
    for i, p in enumerate(flat_params):
        n = p.numel()
        seg_m = m[offsets[i]:offsets[i] + n].view(p.shape).clone()
        if step_count <= 0:                       # torch creates an optimiser's state on its first step
            continue
        if kind in ('ADAM', 'ADAMW'):
            opt.state[p] = {'step': torch.tensor(float(step_count)), 'exp_avg': seg_m,
                            'exp_avg_sq': v[offsets[i]:offsets[i] + n].view(p.shape).clone()}
        elif kind == 'SGD':
            if opt.param_groups[0]['momentum'] != 0:
                opt.state[p] = {'momentum_buffer': seg_m}
        elif kind == 'RMSprop':
            opt.state[p] = {'step': torch.tensor(float(step_count)), 'square_avg': seg_m}
    return opt


# ---------------------------------------------------------------------------------------------- checkpoints
def _bundle(model, optimizer, **extra):
    d = {'state_dict': model.state_dict(), 'optimizer': optimizer.state_dict()}
    d.update(extra)
    return d


def save_checkpoint(model, optimizer, filename='my_checkpoint.pth.tar', **extra):
    torch.save(_bundle(model, optimizer, **extra), filename)


def save_point_sche(model, optimizer, schedule, filename='my_checkpoint.pth.tar'):
    torch.save(_bundle(model, optimizer, schedule=schedule.state_dict()), filename)


def load_model(checkpoint_file, model, device):
    """Weights only (a file this code or the reference wrote; loaded without unpickling arbitrary objects)."""
    state = torch.load(checkpoint_file, map_location=device, weights_only=True)
    model.load_state_dict(state['state_dict'], strict=False)
    return state


def load_checkpoint(checkpoint_file, model, optimizer, lr, device):
    state = load_model(checkpoint_file, model, device)
    optimizer.load_state_dict(state['optimizer'])
    for group in optimizer.param_groups:
        group['lr'] = lr


def seed_everything(seed=42):
    os.environ['PYTHONHASHSEED'] = str(seed)
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)
