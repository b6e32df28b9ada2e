"""solver.mainsolver — `Solver(cfg).run()`: train / test / colour (mirror of the reference Solver).

Reference behaviour kept (solver/mainsolver.py:30-209): the network is loaded by name from `model.<model_name>`;
per epoch one pass over the shuffled train loader with CE + ADAM, then the validation pass that stops as soon as
its running loss exceeds the best one (:62-76), best weights -> `<time>_weights.pth` (raw state_dict), every
epoch -> `<time>_curweights.pth` ({'state_dict','optimizer'}); `test()` fills `test_matrix[pred][target]` and calls
`indicator()`; `color()` writes `<time>_pic_1.png` / `_pic_2.png`.

Two execution paths, same arithmetic; `train()` chooses between them once, by method (`_train_epoch_fast` /
`_train_epoch_dropin`), `test()` and `color()` by the class of `self.evaluation` (solver/evaluation.py):
  * fast (default on a GPU): resident scene + epoch plan + fused HIP step (dmf/engine.py) — no patch
    materialisation, no per-step host sync, confusion matrix and label maps built on the device;
  * drop-in (`fast_path: 0`): the reference's own loop body (mainsolver.py:49-55) over materialised batches through
    `Net.forward` / autograd / torch ADAM.
`gmf.half: 1` on the fast path: fp16 resident scene and the device loss scaler (dmf.engine.LossScaler with GradScaler's
defaults) around the ADAM step — the meaning `bench.py --half 1 --scaler 1` gives the switch; SGD / RMSprop are refused
(the scaler step is ADAM), and the one-shot xgmi exchange is not used (it does not carry the scaler).
`schedule.class_weights` (a list, or `balanced`: from the train split of each `dataloader()` call), `schedule.label_smoothing`,
`schedule.focal_gamma` (all optional): the criterion becomes `nn.CrossEntropyLoss(weight=, label_smoothing=)` or the focal
loss on both paths and in the validation pass (utils.make_loss); the fast path then trains by the unit-gradient step around
`dmf_ce_loss` (TrainEngine(criterion=...), DESIGN §12: no native launch loop — set `steps_per_graph` > 0, the default -1
then steps eagerly from Python; with a scheduler add `device_schedule: 1`, or the graph is re-captured every epoch —, no xgmi
exchange, the engine shards the batches).  With `gmf.attention: 1` the same keys train on the fast path too: the attention
kernel evaluates the criterion itself (`TrainEngine(criterion_in_kernel=True)`, `dmf_train_attn_fwd_bwd_ce`), and what is said
above about `steps_per_graph`, the scheduler and the sharding holds as it stands.  Keys that are all neutral change nothing.
`schedule.weight_decay`, `schedule.optimizer: ADAMW` and `schedule.clip_grad_norm` (all optional): torch's
`weight_decay=`, `torch.optim.AdamW` and `clip_grad_norm_(params, max_norm)` between backward and step on both paths; the fast
path then updates by `dmf_optim_step` on the flat gradient (no native launch loop — set `steps_per_graph` > 0, the default -1
then steps eagerly from Python —, no xgmi exchange).  Neutral values (`weight_decay: 0`, `clip_grad_norm: null` or 0) change nothing.
`train.epoch_block: E` (default 1): `train()` chooses once between two loops that keep ONE epoch ledger (`_record_epoch`,
`_save_current`).  `_train_epochs` is the loop described above.  It is not "a block of one": toStageSolver (its validation is read
back per batch), data-parallel runs (the ranks check their exchange every epoch) and the drop-in path have no block form; the
first two refuse E > 1, the last ignores it.  `_train_blocks` (fast path, E > 1) works in blocks of up to E
epochs (`block_length`), inside which the host only enqueues (`_enqueue_block`) and then waits once (`_collect_block`): same
ledger entries, same files, same RNG stream.  One difference: `<t>_weights.pth` appears at the end of the block in which the
best epoch lies, not at that epoch (an interrupted run loses at most one block; a completed one leaves the same file).  With a
scheduler and `steps_per_graph` > 0 the engine re-captures its graph whenever lr changes, and a capture synchronises (as with
E = 1) — unless `schedule.device_schedule: 1` keeps the schedule on the device, which has no sync; nor have the library's launch
loop and a constant lr.
`schedule.device_schedule: 1` (default 0) on the fast path: lr, betas and momentum of every epoch live in a table on
the device and the optimiser kernels read their row themselves (`_set_device_schedule`), so ONE captured graph serves the whole
run, whatever the scheduler.  `schedule.scheduler_unit: step` (default epoch): `scheduler.step()` after every optimiser step
instead of once per epoch, on the drop-in path by one branch in the loop, on the fast path by a table row per step (it requires
device_schedule: 1).
`schedule.weight_average: ema | mean` (default none) with `average_decay` and `average_start` (epochs): an averaged
copy of the weights, torch's `AveragedModel`, updated after every optimiser step — on the fast path inside the update launch
(`engine.set_averaging`), on the drop-in path by `_foreach_lerp_` in the loop (`_average_dropin`).  Validation then evaluates
the averaged weights (`_on_average`), `<t>_weights.pth` holds those of the best epoch (in an epoch block dmf_keep_best is handed
them), so test() / color() classify with them; `<t>_curweights.pth` keeps the raw weights and the optimiser and gains the key
`averaged`, which test() loads with `save_best: 0`.  toStageSolver refuses the keys.
`schedule.augment: none | flips | d4` and `test.tta: none | flips | d4` (both optional): every train sample is seen as
one of the 4 flips or 8 flips and quarter turns of its patch, the variant drawn per (cfg['seed'], epoch, pixel) by a stateless
hash (`_augment_variants`: torch's RNG stream, and so batch order, splits and labels, stay those of an unaugmented run; every
rank, route and path draws the same); `test()`, `_calibrate` and `color()` classify by the mean of the logits over the variants.
Fast path: BaseSolver turns the resident scene into an atlas of the variants either key needs (`Scene.atlas`, dmf_scene_atlas), a
variant is then a mapped coordinate (`_augment_xy`, before `load_plan`, `load_block` and `step` see it, so their bounds checks see
what the kernel reads) and no train route changes; `EvalEngine(tta=)` runs one forward per variant and dmf_logits_mean.  Drop-in
path: the materialised patches are transformed (`augment.tf_batch`), the mean is torch's (`_logits_dropin`).  The validation
pass is never augmented.  With both keys `none` the scene is the plain Scene and nothing changes; toStageSolver refuses the keys.
`test.calibration`, `test.temperature`, `color.confidence`, `test.spatial`, `color.spatial` and
`test.segments`, `color.segments`: see
solver/evaluation.py, to whose class of this run's path (`self.evaluation`) `test()` and `color()` put their questions.
Data parallel (`test.py` under `torch.distributed.run`, fast path only): every rank holds the scene, iterates the SAME
shuffled index stream (same seed) and trains on its contiguous shard of each global batch (a batch that the world size
does not divide is trimmed to the largest multiple); the gradient exchange is the engine's; validation runs on every
rank (identical decisions), test / colour shard the pixels (dmf/parallel.py); rank 0 writes the artefacts.
Deliberate differences: `test()` evaluates the whole test split when `test.full: 1` (the reference always stops
after the first batch, :142 — that stays the default); the t-SNE plot inside `test()` and the visualisation
helpers (:110-136,211-441) are out of scope; `nohup: 1` does not crash (reference bug at :76).
"""
import contextlib
import importlib
import itertools
import json
import time
import types

import numpy as np
import torch
from PIL import Image
from tqdm import tqdm

from dmf import augment
from solver.basesolver import BaseSolver
from solver.evaluation import DropinEvaluation, EngineEvaluation, map2
from utils import calibration as calib
from utils import segments, spatial, spectral
from utils.utils import (average_update_, averaging_keys, clip_grad_norm_of, criterion_keys, criterion_spec, epoch_hparams, export_optimizer, make_loss, optim_hparams,
                         make_optimizer, make_scheduler, save_checkpoint, schedule_groups, schedule_keys, schedule_table)


def block_length(epoch, epoch_block, save_every, epochs):
    """Epochs in the block that starts at `epoch`: at most `epoch_block`, not past the epoch after which `<t>_curweights.pth`
    is next due (every `save_every`-th), not past the last of `epochs`.  save_every 1 makes every block one epoch long."""
    return max(1, min(epoch_block, save_every - epoch % save_every, epochs - epoch))


class Solver(BaseSolver):
    """What a stage of the two-stage path (solver.tostagesolver) states differently is gathered in the hooks below
    `train()`: `engine_loss`, `_steps_per_graph`, `_train_engine`, `_eval_engine`, `_rank_batches`, `_step_short`, and for the
    drop-in path `_train_epoch_dropin`, `_valid_pass`, `_predict_dropin`, `_test_whole_split`."""
    engine_loss = 'Criterion'                            # the schedule.loss that the fast path's train engine implements
    epoch_blocks = True                                  # `train.epoch_block` > 1 has a block form for this stage
    weight_averaging = True                              # `schedule.weight_average` is in scope for this stage
    calibrated = True                                    # `test.calibration` / `test.temperature` / `color.confidence` are in scope
    augmented = True                                     # `schedule.augment` / `test.tta` are in scope for this stage
    regularised = True                                   # `test.spatial` / `color.spatial` are in scope for this stage
    segmented = True                                     # `test.segments` / `color.segments` are in scope for this stage
    band_reduced = True                                  # `band_reduce` is in scope for this stage
    averaging = None                                     # (the constructor reads it from cfg['schedule'])
    aug_ops, tta_ops = (0,), (0,)                        # (BaseSolver reads them from schedule.augment / test.tta; (0,) = none)
    calib, spat = calib.calibration_keys({}), spatial.spatial_keys({})     # (the constructor reads them from cfg; these: neutral)
    segm = segments.segment_keys({})                     # (likewise)
    regn = segments.region_keys({}, segm)                # (likewise: test.segment_connectivity / _min_size / _file)
    merge = 'position'                                   # (likewise: test.segment_merge)
    evaluation = None                                    # solver.evaluation's class of this run's path (`_ensure_model`)
    device_schedule, scheduler_unit, _step_groups = False, 'epoch', None      # (the constructor reads them from cfg['schedule'])

    def __init__(self, cfg):
        keys = criterion_keys(cfg)
        if keys and (self.engine_loss != 'Criterion' or cfg['schedule']['loss'] != 'Criterion'):
            raise ValueError('schedule.%s belongs to schedule.loss: Criterion of Solver; %s trains with %s'
                             % (keys[0], type(self).__name__, cfg['schedule']['loss']))
        self.averaging = averaging_keys(cfg)           # None, or (kind, decay, epochs before the first averaged step)
        if self.averaging is not None and not self.weight_averaging:
            raise ValueError('schedule.weight_average, schedule.average_decay and schedule.average_start are out of scope for %s: '
                             'set weight_average to none' % type(self).__name__)
        self.calib = calib.calibration_keys(cfg)       # test.calibration / calibration_bins / temperature, color.confidence
        if calib.keys_in_use(self.calib) and not self.calibrated:
            raise ValueError('%s is out of scope for %s (its prediction is the pair argmax of two streams): leave the key out'
                             % (calib.keys_in_use(self.calib)[0], type(self).__name__))
        if augment.keys_in_use(cfg) and not self.augmented:
            raise ValueError('%s is out of scope for %s (its four streams live in one tall scene): leave the key out'
                             % (augment.keys_in_use(cfg)[0], type(self).__name__))
        self.spat = spatial.spatial_keys(cfg)          # test.spatial / spatial_radius / _sigma_s / _sigma_r / _iterations, color.spatial
        if spatial.keys_in_use(self.spat) and not self.regularised:
            raise ValueError('%s is out of scope for %s (its four streams live in one tall scene): leave the key out'
                             % (spatial.keys_in_use(self.spat)[0], type(self).__name__))
        self.segm = segments.segment_keys(cfg)         # test.segments / segment_size / _compactness / _iterations / _vote, color.segments
        if segments.keys_in_use(self.segm) and not self.segmented:
            raise ValueError('%s is out of scope for %s (its four streams live in one tall scene): leave the key out'
                             % (segments.keys_in_use(self.segm)[0], type(self).__name__))
        if spectral.noise_keys(cfg) is not None and not self.band_reduced:
            raise ValueError('band_reduce_noise is out of scope for %s (its four streams live in one tall scene): leave the key out'
                             % type(self).__name__)
        if cfg.get('band_profile', 'none') not in (None, False, 0, 'none') and not self.band_reduced:
            raise ValueError('band_profile is out of scope for %s (its four streams live in one tall scene): leave the key out'
                             % type(self).__name__)
        if spectral.keys_in_use(spectral.band_keys(cfg)) and not self.band_reduced:
            raise ValueError('band_reduce is out of scope for %s (its four streams live in one tall scene): leave the key out'
                             % type(self).__name__)
        self.regn = segments.region_keys(cfg, self.segm)   # test.segment_connectivity / segment_min_size / segment_file
        self.merge = segments.merge_key(cfg, self.regn)    # test.segment_merge
        self.spatial, self._spatial_maps = None, None  # test()'s regularisation block; the whole-scene maps of the loaded weights
        self.segments, self._segment_maps = None, None # test()'s superpixel block; the whole-scene maps of the loaded weights
        self.calibration, self._temp = None, None      # test()'s calibration block; (T, fit block or None) once it is known
        self._avg_flat, self._avg_steps = None, 0      # drop-in path: the averaged flat vector and the optimiser steps taken
        self.cfg, self.rank, self.world = cfg, 0, 1
        self._epoch_block()                            # (a stage without a block form refuses the key before anything is read)
        # schedule.device_schedule / schedule.scheduler_unit (utils.schedule_keys; `step` on the fast path needs the device table)
        self.device_schedule, self.scheduler_unit = schedule_keys(
            cfg, fast=bool(cfg.get('fast_path', 1)) and str(cfg.get('device', '')).startswith('cuda'))
        self._step_groups = None                       # unit step on the fast path: the parameter group of every step of the run
        super().__init__(cfg)
        self.criterion = None                          # criterion_spec of the cfg, made by dataloader() (None: plain cross-entropy)
        self.train_labels = None
        self.model = None
        self.cur_model = None
        self.train_time = 0
        self.test_time = 0
        self.matrix = None
        self.engine = self.eval_engine = None
        self.process_group = None                      # set by the launcher for data-parallel runs (test.py)
        self.comm = None
        self._valid_dev = None                         # the validation split on the device (epoch blocks), per dataloader() call
        self._block = None                             # the device state of a train() in blocks (_train_blocks)
        self.val_history, self.best_loss, self.best_epoch = [], float('inf'), None     # the epoch ledger (_record_epoch)
        if self.cfg['train']['pretrained']:
            self.init_model()

    def init_model(self):
        lib = importlib.import_module('model.' + self.cfg['model_name'].lower())
        self.model = lib.Net(args=self.cfg)
        self.optimizer = make_optimizer(self.cfg, self.model.parameters())
        self.loss = self._make_loss()
        self.scheduler = make_scheduler(self.optimizer, self.cfg)

    def _make_loss(self):
        """schedule.loss as a torch module; `class_weights: balanced` needs the train split, so a model that is built before
        dataloader() has run gets its criterion there."""
        if self.cfg['schedule'].get('class_weights') == 'balanced' and self.train_labels is None:
            return None
        return make_loss(self.cfg['schedule']['loss'], self.cfg, self.train_labels)

    def dataloader(self):
        """BaseSolver's splits and loaders; with criterion keys in cfg['schedule'] also the criterion of this split
        (`class_weights: balanced` is computed here, once per call, from the train split's labels: the same numbers on every
        rank of a data-parallel run, which all draw the same split)."""
        super().dataloader()
        self._valid_dev = None
        self._temp = None
        self._spatial_maps = None
        self._segment_maps = None
        if criterion_keys(self.cfg):
            self.train_labels = self.index_dataset.label[np.asarray(self.train_index_loader.dataset.indices, dtype=np.int64)]
            self.criterion = criterion_spec(self.cfg, self.train_labels)
            if self.model is not None:
                self.loss = self._make_loss()

    # ------------------------------------------------------------------ helpers of the fast path
    def _bar(self, it):
        return it if self.cfg['nohup'] else tqdm(it, leave=True)

    @staticmethod
    def _xy_labels(batch):
        x, y, label, _ = batch
        return torch.stack([x, y], 1).to(torch.int32), label.to(torch.int32)

    def _export_optimizer(self):
        """The configured optimiser (ADAM, SGD or RMSprop) with its own state keys, from the engine's flat state vectors
        (checkpoint interchange with the reference's save_checkpoint / load_checkpoint, utils/utils.py:82-102)."""
        eng = self.engine
        group = {'lr': eng.lr, 'weight_decay': eng.weight_decay}
        if eng.optim in ('ADAM', 'ADAMW'):
            group['betas'] = (eng.b1, eng.b2)
        elif eng.optim == 'SGD':
            group['momentum'] = eng.momentum
        return export_optimizer(self.cfg, self.cur_model.parameters(), self.cur_model._named(), self.cur_model._offsets, eng.m, eng.v,
                                eng.step_count, group)

    # ------------------------------------------------------------------ train
    def _epoch_block(self):
        """train.epoch_block (default 1): epochs per block of the fast path's block form."""
        E = int((self.cfg.get('train') or {}).get('epoch_block', 1) or 1)
        if E < 1:
            raise ValueError('train.epoch_block: %d is not a positive number of epochs' % E)
        if E > 1 and not self.epoch_blocks:
            raise ValueError('train.epoch_block: %d is out of scope for %s (its validation is a batch-coupled loss that is read '
                             'back per batch): set it to 1' % (E, type(self).__name__))
        if E > 1 and self.world > 1:
            raise ValueError('train.epoch_block: %d is out of scope for data-parallel runs (%d ranks: they check their gradient '
                             'exchange every epoch): set it to 1' % (E, self.world))
        return E

    def train(self):
        E = self._epoch_block()
        time1 = time.time()
        self._temp = None                              # (a fitted temperature belongs to the weights it was fitted on)
        self._spatial_maps = None                      # (and so do the regularised maps)
        self._segment_maps = None                      # (and the voted ones)
        if not self.cfg['train']['pretrained']:
            self.init_model()
        self.cur_model = self.model.to(self.DEVICE)
        if self.criterion is not None:
            self.loss = self.loss.to(self.DEVICE)             # (the class weights are a buffer of the module)
        if self.fast:
            self._make_engines()
        elif self.scheduler_unit == 'step' and self.scheduler is not None:
            # stepped after every optimiser step: the scheduler spans epochs x batches steps (OneCycleLR's total_steps)
            self.scheduler = make_scheduler(self.optimizer, self.cfg, total=self.EPOCH * len(self.train_loader))
        if self.averaging is not None and not self.fast:       # (the fast path's engine keeps its own: _make_engines)
            self._avg_flat, self._avg_steps = self.cur_model.flat_parameters().detach().clone(), 0
        self.step_losses, self.val_history, self.best_loss = [], [], float('inf')
        self.best_epoch = 0 if self.cfg['train']['save_best'] else None
        if self.fast and E > 1:
            self._train_blocks(E)
        else:
            self._train_epochs(self._train_epoch_fast if self.fast else self._train_epoch_dropin)
        self.train_time = time.time() - time1
        self.epoch = 0

    def _train_epochs(self, train_epoch):
        """Epoch by epoch: `train.epoch_block: 1`, and whatever has no block form (module text)."""
        save_best = self.cfg['train']['save_best']
        while self.epoch < self.EPOCH:
            self.cur_model.train()
            losses = train_epoch()
            val = None
            if save_best:
                self.cur_model.eval()
                with self._on_average():
                    val = self._valid_pass(self.best_loss)
            if self._record_epoch(self.epoch, losses, val) and self.rank == 0:
                best = self.cur_model.state_dict() if self.averaging is None else self._flat_state_dict(self._averaged())
                torch.save(best, self.cfg['RESULT_output'] + str(self.time) + '_weights.pth')
            self._save_current(self.epoch + 1)
            if self.world > 1:
                import torch.distributed as dist
                dist.barrier(self.process_group)               # the files exist before any rank goes on to load them
            self.epoch += 1

    # ------------------------------------------------------------------ the epoch ledger of both forms
    def _record_epoch(self, epoch, losses, val=None):
        """A finished epoch: its step losses, what `_valid_pass` or the device gave for it (None: no `save_best`; the validation
        sum, or on the drop-in path and in stage 2 the running sum at the early exit), the printed lines.  Returns whether
        the best moved — strict, the reference's `if val_loss < best_loss` and dmf_keep_best's comparison on the same double: an
        equal value and a NaN are never the best —; the caller writes `<t>_weights.pth`, at the epoch or at its block's end."""
        self.step_losses += losses
        moved = False
        if val is not None:
            self.val_history.append(val)
            moved = val < self.best_loss
            if moved:
                self.best_loss, self.best_epoch = val, epoch
                if self.cfg['nohup']:
                    print("best epoch now is {}".format(epoch))
        if self.cfg['nohup']:
            print("{} times {}th epoch is trained, loss {:.6f}".format(self.time, epoch, losses[-1] if losses else float('nan')))
        return moved

    def _save_every(self):
        return int(self.cfg['train'].get('save_every', 1) or 1)

    def _save_current(self, done):
        """`<t>_curweights.pth` (model + optimiser, mainsolver.py:83-84: what an interrupted run resumes from) after `done` finished
        epochs, where it is due: after every `train.save_every`-th (default 1 = the reference; on the fast path that is 2.8 of a
        small epoch's 5.6 ms, tools/solver_epoch_profile.sh) and after the last."""
        if self.rank == 0 and (done % self._save_every() == 0 or done == self.EPOCH):
            opt = self._export_optimizer() if self.fast else self.optimizer
            extra = {} if self.averaging is None else {'averaged': self._flat_state_dict(self._averaged())}
            save_checkpoint(self.cur_model, opt, self.cfg['RESULT_output'] + str(self.time) + '_curweights.pth', **extra)

    # ------------------------------------------------------------------ the averaged weights (schedule.weight_average)
    def _average_start_step(self, steps_per_epoch):
        """The first averaged optimiser step (1-based): the first step after `average_start` epochs."""
        return self.averaging[2] * steps_per_epoch + 1

    def _averaged(self):
        """The averaged flat vector: the engine's, or the drop-in loop's."""
        return self.engine.averaged_parameters() if self.fast else self._avg_flat

    def _average_dropin(self):
        """After `optimizer.step()` of the drop-in loop: AveragedModel.update_parameters, on the net's flat vector."""
        kind, decay, _ = self.averaging
        self._avg_steps += 1
        average_update_([self._avg_flat], [self.cur_model.flat_parameters().detach()], kind, decay,
                        self._average_start_step(len(self.train_loader)), self._avg_steps)

    @contextlib.contextmanager
    def _on_average(self):
        """The validation pass inside evaluates the averaged weights: the eval engine is pointed at them; the drop-in path's
        net holds them for the pass and gets its own back."""
        if self.averaging is None:
            yield
        elif self.fast:
            self.eval_engine.use_parameters(self._averaged())
            try:
                yield
            finally:
                self.eval_engine.use_parameters(None)
        else:
            flat = self.cur_model.flat_parameters()
            own = flat.detach().clone()
            with torch.no_grad():
                flat.copy_(self._avg_flat)
            try:
                yield
            finally:
                with torch.no_grad():
                    flat.copy_(own)

    def _loss_scaler(self, hp):
        """gmf.half: 1 on the fast path -> the device loss scaler with GradScaler's defaults; its step is ADAM (or ADAMW)."""
        if not self.half:
            return None
        if hp['optimizer'] not in ('ADAM', 'ADAMW'):
            raise ValueError('gmf.half: 1 trains with the loss scaler, whose step is ADAM or ADAMW; schedule.optimizer is %s'
                             % hp['optimizer'])
        from dmf.engine import LossScaler
        return LossScaler(self.DEVICE)

    def _make_engines(self):
        if self.cfg['schedule']['loss'] != self.engine_loss:
            raise ValueError('the fused HIP step of %s implements schedule.loss: %s' % (type(self).__name__, self.engine_loss))
        hp = optim_hparams(self.cfg)                             # ADAM (fused), SGD or RMSprop (utils/utils.py:10-16)
        if self.cfg['batchsize'] % self.world:
            raise ValueError('batchsize %d is not divisible by the %d ranks' % (self.cfg['batchsize'], self.world))
        self.engine = self._train_engine(self.cfg['batchsize'] // self.world, dict(
            lr=hp['lr'], betas=hp['betas'], eps=hp['eps'], process_group=self.process_group, scaler=self._loss_scaler(hp),
            optimizer=hp['optimizer'], momentum=hp.get('momentum', 0.0), alpha=hp.get('alpha', 0.99),
            weight_decay=hp.get('weight_decay', 0.0), clip_grad_norm=hp.get('clip_grad_norm')))
        self.eval_engine = self._eval_engine()
        self._set_device_schedule()
        if self.averaging is not None:
            self.engine.set_averaging(self.averaging[0], self.averaging[1], self._average_start_step(self._steps_per_epoch()))

    def _steps_per_epoch(self):
        """Optimiser steps of one epoch on the fast path: the full batches, and the short last one where `_rank_batches` keeps it
        (it needs a pixel for every rank)."""
        n_full, rest = divmod(len(self.train_index_loader.dataset), self.cfg['batchsize'])
        return n_full + (1 if rest >= self.world else 0)

    def _set_device_schedule(self):
        """schedule.device_schedule: 1 — the run's table of (lr, beta1, beta2, momentum) goes to the device once
        (utils.schedule_table -> engine.set_schedule); it is rebuilt from cfg by every train().  Unit epoch: one row per epoch,
        `_set_epoch_hparams` points the engine at the epoch's.  Unit step: one row per optimiser step of the run (the short
        last batch counts), found by the engine's own step count — a resumed engine indexes by the count it was given."""
        self._step_groups = None
        if not self.device_schedule:
            return
        unit = self.scheduler_unit
        rows = self.EPOCH * (self._steps_per_epoch() if unit == 'step' else 1)
        if unit == 'step':
            self._step_groups = schedule_groups(self.cfg, max(rows, 1), unit)
        self.engine.set_schedule(schedule_table(self.cfg, max(rows, 1), unit), unit)

    def _set_epoch_hparams(self, epoch):
        """The engine's host-side lr, betas and momentum of this epoch: launch arguments of its steps, or with
        device_schedule: 1 only what the checkpoint's parameter group is written from (unit step: the row of the epoch's last
        step), while the steps read the table — the row that `set_epoch` fills in, without a synchronisation."""
        eng = self.engine
        hp = epoch_hparams(self.cfg, epoch)                   # lr (and, under OneCycleLR, beta1 / momentum) of this epoch
        if self._step_groups is not None:
            hp = self._step_groups[min((epoch + 1) * self._steps_per_epoch(), len(self._step_groups)) - 1]
        if self.device_schedule:
            eng.set_epoch(epoch)
        eng.lr = float(hp['lr'])
        if 'betas' in hp:
            eng.b1, eng.b2 = float(hp['betas'][0]), float(hp['betas'][1])
        if eng.optim == 'SGD':
            eng.momentum = float(hp['momentum'])

    def _train_epoch_fast(self):
        eng = self.engine
        self._set_epoch_hparams(self.epoch)
        # the epoch's shuffled coordinates, as the batches the engine steps on and the size of a full one
        batches, B = self._rank_batches([self._xy_labels(b) for b in self.train_index_loader])
        if len(self.aug_ops) > 1:                          # schedule.augment: full batches and the short one alike, before any
            batches = [(self._augment_xy(xy, self.epoch), lab) for xy, lab in batches]      # bounds check sees them
        full = [b for b in batches if b[0].shape[0] == B]
        losses = []
        if full:
            eng.load_plan(torch.cat([b[0] for b in full]), torch.cat([b[1] for b in full]))
            eng.run_plan(len(full), self._steps_per_graph())
            losses = eng.losses().tolist()
        losses += [self._step_short(xy, lab) for xy, lab in batches if xy.shape[0] != B]    # DataLoader keeps the short last batch
        self._check_exchange()
        return losses

    # ------------------------------------------------------------------ schedule.augment / test.tta
    def _augment_variants(self, xy, epoch):
        """The variant (0..7) of every sample of epoch `epoch`, from the pixels' coordinates xy [n, 2] (numpy): the stateless
        draw of dmf.augment.draw_slots on (cfg['seed'], epoch, x, y) — the same on every rank, route and path, and after a
        resume; torch's RNG stream is not touched."""
        ops = np.asarray(self.aug_ops, dtype=np.int64)
        return ops[augment.draw_slots(int(self.cfg.get('seed') or 0), epoch, xy, len(ops))]

    def _augment_xy(self, xy, epoch):
        """Fast path: xy [n, 2] (host int32 tensor, pixel coordinates) -> the atlas coordinates of each sample's variant."""
        xy = xy.numpy()
        slot_of = np.zeros(8, dtype=np.int64)              # variant -> its slot in the atlas (every aug op is held: BaseSolver)
        slot_of[list(self.scene.ops)] = np.arange(len(self.scene.ops))
        return torch.from_numpy(self.scene.map_xy(xy, slot_of[self._augment_variants(xy, epoch)]))

    def _logits_dropin(self, data1, data2):
        """Drop-in path: the net's logits, or with `test.tta` the mean over the variants, (((l_0 + l_1) + l_2) + ...) / V."""
        if len(self.tta_ops) == 1:
            return self.cur_model(data1, data2)
        total = None
        for k in self.tta_ops:
            ks = np.full(data1.shape[0], k)
            logits = self.cur_model(augment.tf_batch(data1, ks), augment.tf_batch(data2, ks))
            total = logits if total is None else total + logits
        return total / float(len(self.tta_ops))

    # ------------------------------------------------------------------ blocks of epochs without the host (train.epoch_block)
    def _train_blocks(self, E):
        """All epochs in blocks (module text).  What dmf_valid_accum and dmf_keep_best keep across blocks lives on the device."""
        dev, f64, every = self.DEVICE, torch.float64, self._save_every()
        self._block = types.SimpleNamespace(
            acc=torch.zeros(1, dtype=f64, device=dev), best=torch.full((1,), float('inf'), dtype=f64, device=dev),
            best_epoch=torch.zeros(1, dtype=torch.int32, device=dev), best_theta=torch.zeros_like(self.engine.theta),
            val_hist=torch.zeros(max(self.EPOCH, 1), dtype=f64, device=dev),
            cap=min(E, every, self.EPOCH),               # epochs in the longest block: the plan keeps one shape
            enqueued=None)                               # (first epoch, epochs, full batches per epoch) of the block under way
        while self.epoch < self.EPOCH:
            self.cur_model.train()
            self._enqueue_block(self.epoch, block_length(self.epoch, E, every, self.EPOCH))
            self._collect_block()

    def _valid_split(self):
        """(xy [n, 2], labels [n]) int32 on the device: the validation split in loader order, checked on the host and uploaded
        once per dataloader() call."""
        if self._valid_dev is None:
            rows = np.asarray(self.valid_index_loader.dataset.indices, dtype=np.int64)
            d, K = self.index_dataset, self.cur_model.arch['K']
            xy = np.stack([d.x[rows], d.y[rows]], 1).astype(np.int32)
            lab = d.label[rows].astype(np.int32)
            self.eval_engine._check_bounds(xy)
            if len(lab) and (lab.min() < 0 or lab.max() >= K):
                raise ValueError('validation label outside [0, %d)' % K)
            self._valid_dev = (torch.from_numpy(xy).to(self.DEVICE), torch.from_numpy(lab).to(self.DEVICE))
        return self._valid_dev

    def _enqueue_block(self, first_epoch, n_epochs):
        """Enqueue epochs [first_epoch, first_epoch + n_epochs): per epoch the plan steps, the short last batch, the validation
        launches in today's batches of `color_batchsize` rows (with class weights the batching is part of the number) and
        dmf_keep_best.  NO host synchronisation: the uploads come first, on an idle device, and nothing is read back.  (With
        `steps_per_graph` > 0 and a scheduler the engine re-captures its graph when lr changes, and a capture synchronises —
        unless `schedule.device_schedule: 1` keeps lr on the device: then the graph captured in the first block is replayed to
        the end, `set_epoch` is a device fill, and a scheduler from graphs does not synchronise inside a block either.)"""
        from dmf import lib
        eng, blk, B, save_best = self.engine, self._block, self.cfg['batchsize'], self.cfg['train']['save_best']
        # the RNG draws of these epochs in today's order: the train loader's two, then the validation loader's base seed
        xy, lab = self._epoch_streams(n_epochs, draws_after=1 if save_best else 0)
        if len(self.aug_ops) > 1:                          # schedule.augment: every epoch's rows, the short batch's included
            xy = torch.stack([self._augment_xy(xy[e], first_epoch + e) for e in range(n_epochs)])
        n_full, rest = divmod(xy.shape[1], B)
        short = (xy[:, n_full * B:], lab[:, n_full * B:]) if rest else (None, None)      # DataLoader keeps the short last batch
        eng.load_block(xy[:, :n_full * B].reshape(-1, 2), lab[:, :n_full * B].reshape(-1), *short,
                       capacity=blk.cap * n_full)
        valid = self._valid_split() if save_best else None
        vb = self.cfg['color_batchsize']
        for e in range(n_epochs):
            self._set_epoch_hparams(first_epoch + e)
            if n_full:
                eng.run_plan(n_full, self._steps_per_graph())
            if rest:
                eng.step_short(e)
            if save_best:
                with torch.no_grad(), self._on_average():
                    for i in range(0, valid[0].shape[0], vb):
                        self.eval_engine.valid_accum(valid[0][i:i + vb], valid[1][i:i + vb], blk.acc)
                # (with averaging the best weights are the averaged ones, as they were validated)
                lib.keep_best(blk.acc, blk.best, blk.best_epoch, first_epoch + e, eng.theta if self.averaging is None else eng.avg,
                              blk.best_theta, blk.val_hist)
        blk.enqueued = (first_epoch, n_epochs, n_full)

    def _collect_block(self):
        """The block's one wait for the device, then what its epochs owe the host, in their order: the ledger entries (step
        losses: per epoch the full batches, then the short one), `<t>_weights.pth` from the device's copy of the best weights
        if the best moved in this block, `<t>_curweights.pth` where it is due."""
        blk = self._block
        first, n_epochs, n_full = blk.enqueued
        torch.cuda.synchronize()
        full, short = self.engine.block_losses()
        full, short = full.tolist(), None if short is None else short.tolist()
        vals = blk.val_hist[first:first + n_epochs].tolist() if self.cfg['train']['save_best'] else [None] * n_epochs
        moved = False
        for e in range(n_epochs):
            losses = full[e * n_full:(e + 1) * n_full] + ([short[e]] if short is not None else [])
            moved = self._record_epoch(first + e, losses, vals[e]) or moved
        if moved:
            if int(blk.best_epoch.item()) != self.best_epoch:
                raise RuntimeError('the device kept epoch %d as the best, the validation history says %d'
                                   % (int(blk.best_epoch.item()), self.best_epoch))
            torch.save(self._best_state_dict(), self.cfg['RESULT_output'] + str(self.time) + '_weights.pth')
        self.epoch = first + n_epochs
        self._save_current(self.epoch)
        if self.cfg['train']['save_best']:
            self.cur_model.eval()

    def _best_state_dict(self):
        """The state dict of the best epoch, from the device's copy of the best flat vector."""
        return self._flat_state_dict(self._block.best_theta)

    def _flat_state_dict(self, flat):
        """The net's state dict with a copy of the flat vector `flat` for its parameters: the net's own keys in their order,
        every parameter a piece of the copy (the net's name / offset table), the buffers as they are."""
        net, flat = self.cur_model, flat.detach().clone()
        start = dict(zip(net._order(), net._offsets))
        now = net.state_dict()
        best = type(now)((k, flat[start[k]:start[k] + v.numel()].view(v.shape) if k in start else v) for k, v in now.items())
        best._metadata = now._metadata
        return best

    def _check_exchange(self):
        """A timed-out wait of the one-shot gradient exchange leaves the ranks with different weights (the kernel sums what
        it has and goes on).  Every rank learns of it here, once per epoch and before anything is saved: all ranks stop."""
        if self.comm is None:
            return
        import torch.distributed as dist
        bad = torch.tensor([int(self.comm.status())], dtype=torch.int32,
                           device=self.DEVICE if dist.get_backend(self.process_group) == 'nccl' else 'cpu')
        dist.all_reduce(bad, op=dist.ReduceOp.MAX, group=self.process_group)
        if int(bad.item()) != 0:
            raise RuntimeError('epoch %d: a gradient exchange timed out on at least one rank; the replicas have diverged. '
                               'Restart from the last checkpoint with xgmi_exchange: 0 (RCCL all-reduce).' % self.epoch)

    # ------------------------------------------------------------------ what a stage states differently: fast path
    def _steps_per_graph(self):
        """N > 0 replays captured hipGraphs of N steps, 0 launches step by step from Python, -1 (default) hands the whole
        epoch to the library's launch loop (dmf_train_plan_steps) where that exists, else step by step."""
        return int(self.cfg.get('steps_per_graph', -1))

    def _train_engine(self, batch, kw):
        from dmf.engine import TrainEngine
        # (the one-shot exchange carries neither the scaler, nor the unit-gradient step of a criterion, nor the step with weight
        # decay or gradient-norm clipping, whose norm is taken from the all-reduced flat gradient)
        plain = kw['optimizer'] == 'ADAM' and not kw['weight_decay'] and not kw['clip_grad_norm']
        comm = self.comm if plain and kw['scaler'] is None and self.criterion is None else None
        if self.criterion is not None:
            kw = dict(kw, criterion=self.criterion)
            if self.cur_model.arch['attention']:           # ... evaluated inside the attention kernel
                kw['criterion_in_kernel'] = True
        return TrainEngine(self.cur_model, self.scene, batch, comm=comm, **kw)

    def _eval_engine(self):
        """Pixels per evaluation launch of the fast path.  `test_batchsize` / `color_batchsize` size the reference's host-fed
        loader (mainsolver.py:90-101,155-163); with the scene resident every pixel is independent of its batch, and a launch of
        256 patches is bound by the host (0.13 of the HBM roof on a 512x512x224 scene) where 16,384 reach 0.62
        (tools/eval_bench.py; identical class maps)."""
        from dmf.engine import EvalEngine
        big = 4096 if self.cur_model.arch['attention'] else 16384
        kw = {} if self.criterion is None else {'criterion': self.criterion}
        if len(self.tta_ops) > 1:                          # test.tta: test(), _calibrate and color() see the mean logits
            kw['tta'] = self.tta_ops
        return EvalEngine(self.cur_model, self.scene, max(self.cfg['test_batchsize'], self.cfg['color_batchsize'], big), **kw)

    def _rank_batches(self, batches):
        """The solver shards on the host: this rank's contiguous shard of every global batch (a remainder is dropped, see
        the module text), without the empty ones.  With a criterion the engine shards (its loss reads the global batch's
        labels): global batches, a full one is batchsize, and one with no pixel for some rank is left out."""
        if self.criterion is not None:
            return [b for b in batches if b[0].shape[0] >= self.world], self.cfg['batchsize']
        per = [b[0].shape[0] // self.world for b in batches]
        return ([(xy[self.rank * n:(self.rank + 1) * n], lab[self.rank * n:(self.rank + 1) * n])
                 for (xy, lab), n in zip(batches, per) if n], self.cfg['batchsize'] // self.world)

    def _step_short(self, xy, lab):
        self.engine.step(xy.to(self.DEVICE), lab.to(self.DEVICE))
        rows = xy.shape[0] // self.world if self.criterion is not None else xy.shape[0]      # (a criterion: xy is the global batch)
        return float(self.engine.loss[:rows].mean().item())

    # ------------------------------------------------------------------ ... and drop-in path
    def _train_epoch_dropin(self):
        loader = self._bar(self.train_loader)
        losses = []
        max_norm = clip_grad_norm_of(self.cfg['schedule'])           # schedule.clip_grad_norm (None: the reference's loop)
        per_step = self.scheduler_unit == 'step' and self.scheduler is not None
        for data1, data2, target, x, y in loader:
            if len(self.aug_ops) > 1:                                # schedule.augment: the patches the fast path reads from the atlas
                ks = self._augment_variants(np.stack([np.asarray(x), np.asarray(y)], 1), self.epoch)
                data1, data2 = augment.tf_batch(data1, ks), augment.tf_batch(data2, ks)
            data1, data2, target = data1.to(self.DEVICE), data2.to(self.DEVICE), target.to(self.DEVICE)
            self.optimizer.zero_grad()
            output = self.cur_model(data1, data2)
            loss = self.loss(output, target.long())
            loss.backward()
            if max_norm:
                torch.nn.utils.clip_grad_norm_(self.cur_model.parameters(), max_norm)
            self.optimizer.step()
            if self.averaging is not None:
                self._average_dropin()
            if per_step:
                self.scheduler.step()                                # schedule.scheduler_unit: step
            losses.append(loss.item())
            if not self.cfg['nohup']:
                loader.set_postfix(ls=losses[-1], ep=self.epoch, tm=self.time, m='train', d=self.cfg['device'])
        if self.cfg['schedule']['if_scheduler'] and not per_step:
            self.scheduler.step()
        return losses

    def _valid_pass(self, best_loss):
        ce = self.loss if self.criterion is not None else torch.nn.CrossEntropyLoss()
        with torch.no_grad():
            if self.fast:
                # The reference adds `loss.item() * n` per batch and stops once the sum passes best_loss (mainsolver.py:65-75):
                # one host sync per batch.  Here the same double-precision sum stays on the device and is read once; the terms
                # are non-negative, so "the full sum is below best_loss" decides exactly what the early exit decides.
                tot = torch.zeros((), dtype=torch.float64, device=self.DEVICE)
                for batch in self.valid_index_loader:
                    xy, lab = (t.to(self.DEVICE) for t in self._xy_labels(batch))
                    # the evaluation launch's own per-patch cross-entropy (dmf_forward_ce) where the shape has it ...
                    part = self.eval_engine.ce_sum(xy, lab)
                    if part is None:                         # ... else torch's on the logits (attention network)
                        part = ce(self._valid_logits(xy), lab.long()).double() * lab.shape[0]
                    tot += part
                return float(tot.item())
            val_loss = 0.0
            for data1, data2, target, _, _ in self.valid_loader:
                logits = self.cur_model(data1.to(self.DEVICE), data2.to(self.DEVICE))
                val_loss += ce(logits, target.to(self.DEVICE).long()).item() * target.shape[0]
                if val_loss > best_loss:
                    break
        return val_loss

    def _valid_logits(self, xy):
        """The validation pass's logits where it takes torch's loss on them: without test-time augmentation."""
        return self.eval_engine._predict_plain(xy)[0]

    def _predict_dropin(self, batch):
        """(pred [n] on the device, target [n], x, y) of a batch of the materialising loaders."""
        data1, data2, target, x, y = batch
        return self._logits_dropin(data1.to(self.DEVICE), data2.to(self.DEVICE)).data.max(1)[1], target, x, y

    def _test_whole_split(self):
        """The reference always stops after the first test batch (mainsolver.py:142); `test.full: 1` takes the whole split."""
        return bool(self.cfg['test'].get('full', 0))

    # ------------------------------------------------------------------ test
    def _load_weights(self, best):
        path = self.cfg['RESULT_output'] + str(self.time) + ('_weights.pth' if best else '_curweights.pth')
        sd = torch.load(path, map_location=self.DEVICE, weights_only=True)
        if not best:                                     # the averaged weights where they are configured and the file has them
            sd = sd['averaged'] if self.averaging is not None and 'averaged' in sd else sd['state_dict']
        self.cur_model.load_state_dict(sd)

    def _ensure_model(self):
        if self.cur_model is None:
            self.init_model()
            self.cur_model = self.model.to(self.DEVICE)
        if self.fast and self.eval_engine is None:
            self.eval_engine = self._eval_engine()
        if self.evaluation is None:                      # the evaluation path, chosen once
            self.evaluation = (EngineEvaluation if self.fast else DropinEvaluation)(self)

    def _single_device_scope(self):
        """Data-parallel runs refuse the calibration and regularisation keys (nothing of them is sharded), as `_epoch_block` does."""
        keys = calib.keys_in_use(self.calib) + spatial.keys_in_use(self.spat) + segments.keys_in_use(self.segm)
        if keys and self.world > 1:
            raise ValueError('%s is out of scope for data-parallel runs (%d ranks): leave the key out' % (keys[0], self.world))

    _calibration_scope = _spatial_scope = _single_device_scope         # the names the two refusals had while they were two

    def test(self):
        time1 = time.time()
        self._single_device_scope()
        self._ensure_model()
        self._load_weights(self.cfg['train']['save_best'])
        self.cur_model.eval()
        whole = self._test_whole_split()
        with torch.no_grad():
            matrix = self.evaluation.confusion(whole)
        self.test_time = time.time() - time1
        self.test_matrix = matrix.astype(np.float64)
        if self.calib['calibration']:
            with torch.no_grad():
                self._calibrate(whole)
        if self.spat['kind'] is not None:
            with torch.no_grad():
                self._regularise(whole)
        if self.segm['kind'] is not None:
            with torch.no_grad():
                self._segment(whole)
        if self.rank == 0:
            self.indicator()
        else:
            from indicators.kappa import aa_oa_quiet
            self.result = list(aa_oa_quiet(self.test_matrix)) + [None]

    def _test_pixels(self, whole):
        """(xy [n, 2], labels [n]) int32 on the host: the pixels test() classifies on the fast path."""
        parts = [self._xy_labels(b) for b in (self.test_index_loader if whole else itertools.islice(self.test_index_loader, 1))]
        return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])

    # ------------------------------------------------------------------ calibration (test.calibration, test.temperature)
    @staticmethod
    def _beta(T):
        """beta = 1 / T as the float32 that the kernels read, on both paths."""
        return float(np.float32(1.0 / T))

    def _temperature_used(self):
        """(T, fit block or None) of `test.temperature`, decided once per trained model: a number as it stands, none -> 1, fit ->
        temperature scaling on the VALIDATION split: 40 safeguarded Newton steps in beta = 1 / T."""
        if self._temp is None:
            t = self.calib['temperature']
            if t != 'fit':
                self._temp = (1.0 if t is None else t, None)
            else:
                with torch.no_grad():
                    n, beta, steps, nll1, nllT = self.evaluation.fit(*self.evaluation.split_logits('valid'))
                if n < 1:
                    raise ValueError('test.temperature: fit needs a validation split')
                self._temp = (1.0 / beta, dict(n=n, nll_at_1=nll1 / n, nll_at_T=nllT / n, beta=beta, steps=steps))
        return self._temp

    def _calibration_block(self, logits, labels, T):
        """The block of utils.calibration.summary at temperature T, from the logits of the test pixels."""
        return calib.summary(*self.evaluation.reliability(logits, labels, self.calib['bins'], self._beta(T)), T)

    def _calibrate(self, whole):
        """`self.calibration` and `<t>_calibration.json` over the pixels of the confusion matrix."""
        T, fit = self._temperature_used()
        logits, labels = self.evaluation.split_logits('test', whole)
        block = self._calibration_block(logits, labels, T)
        if T != 1.0:
            block['before'] = self._calibration_block(logits, labels, 1.0)
        if fit is not None:
            block['fit'] = fit
        self.calibration = block
        if self.rank == 0:
            with open(self.cfg['RESULT_output'] + str(self.time) + '_calibration.json', 'w') as f:
                json.dump(block, f, indent=1)

    # ------------------------------------------------------------------ spatial regularisation (test.spatial, color.spatial)
    def _set_pixels(self, rows):
        """xy [n, 2] int32 (numpy) of rows of the pixel table, from the index dataset's arrays: no loader, so torch's RNG stream
        stays what it is without the keys."""
        rows = np.asarray(rows, dtype=np.int64)
        d = self.index_dataset
        return np.stack([d.x[rows], d.y[rows]], 1).astype(np.int32).reshape(-1, 2)

    def _scene_pixels(self):
        """Both colour sets: every pixel of the scene (the labelled ones first)."""
        return self._set_pixels(list(self.matrix_[1]) + list(self.matrix_[0]))

    def _regularised_maps(self, best):
        """-> (plain or None, regularised) label maps [H, W] int32 (numpy) of the WHOLE scene under the loaded weights (`best`:
        which file they came from; the pair is kept per trained model and file): all pixels of both colour sets are classified at
        `test.temperature`'s beta, the probabilities go through `test.spatial_iterations` passes of the filter."""
        if self._spatial_maps is None or self._spatial_maps[0] != bool(best):
            size = self.cfg['DATA_DICT'][self.cfg['data_city']]['size']
            beta = self._beta(self._temperature_used()[0])
            self._spatial_maps = (bool(best), self.evaluation.scene_maps(self._scene_pixels(), int(size[0]), int(size[1]), beta, self.spat))
        return self._spatial_maps[1]

    def _regularise(self, whole):
        """`self.spatial` and `<t>_spatial.json`: a second confusion matrix over the pixels of the first, from the regularised
        label map at their (x, y).  `self.test_matrix` and what `indicator()` makes of it stay as they are."""
        plain, smooth = self._regularised_maps(self.cfg['train']['save_best'])
        self.spatial = spatial.report(self.spat, self.test_matrix, *self._second_matrix(whole, plain, smooth))
        self._write_block(self.spatial, '_spatial.json')

    def _second_matrix(self, whole, plain, remapped):
        """-> (confusion matrix of the whole-scene label map `remapped` over the pixels of the first matrix, how many of them
        changed class against the plain prediction)."""
        rows = np.asarray(self.test_index_loader.dataset.indices, dtype=np.int64)
        if not whole:
            rows = rows[:self.cfg['test_batchsize']]   # the first batch of the unshuffled loader
        xy, lab = self._set_pixels(rows), self.index_dataset.label[rows].astype(np.int64)
        K = self.cfg['Categories_Number']
        after = np.zeros([K, K], dtype=np.int64)
        np.add.at(after, (remapped[xy[:, 0], xy[:, 1]], lab), 1)                  # matrix[pred][target] += 1
        return after, int((remapped[xy[:, 0], xy[:, 1]] != self.evaluation.plain_at(xy, plain, *remapped.shape)).sum())

    def _write_block(self, block, suffix):
        if self.rank == 0:
            with open(self.cfg['RESULT_output'] + str(self.time) + suffix, 'w') as f:
                json.dump(block, f, indent=1)

    def _color_remapped(self, H, W, lut, remapped, name):
        """-> (map 1, map 2) of the whole-scene label map `remapped`, composed as the plain maps are — map 1 its classes on the
        labelled pixels, map 2 with the other pixels too — and written as `<t>_pic_{1,2}_<name>.png`."""
        maps = []
        for use, rows in ((self.cfg['color']['supervised'], self.matrix_[1]), (self.cfg['color']['unsupervised'], self.matrix_[0])):
            m = np.zeros([H, W], dtype=np.int32)
            if use:
                xy = self._set_pixels(rows)
                m[xy[:, 0], xy[:, 1]] = remapped[xy[:, 0], xy[:, 1]]
            maps.append(m)
        out = (maps[0], map2(maps, self.cfg['color']['unsupervised']))
        if self.cfg['color']['supervised'] and self.rank == 0:
            for n, m in enumerate(out, 1):
                Image.fromarray(lut[m]).save(self.cfg['RESULT_output'] + str(self.time) + '_pic_%d_%s.png' % (n, name))
        return out

    def _color_spatial(self, H, W, lut):
        """`<t>_pic_{1,2}_spatial.png`: the regularised classes."""
        self.spatial_maps = self._color_remapped(H, W, lut, self._regularised_maps(True)[1], 'spatial')

    # ------------------------------------------------------------------ superpixel voting (test.segments, color.segments)
    def _segmented_maps(self, best):
        """-> (plain or None, segment image [H, W] int32, voted label map [H, W] int32[, the regions' figures]) (numpy) of the WHOLE scene under the loaded
        weights (`best`: which file they came from; kept per trained model and file): all pixels of both colour sets are classified
        at `test.temperature`'s beta, the scene is segmented, and every pixel takes its segment's class.  The probability map is
        the unfiltered one, whatever `test.spatial` says."""
        if self._segment_maps is None or self._segment_maps[0] != bool(best):
            size = self.cfg['DATA_DICT'][self.cfg['data_city']]['size']
            beta = self._beta(self._temperature_used()[0])
            self._segment_maps = (bool(best), self.evaluation.scene_segments(self._scene_pixels(), int(size[0]), int(size[1]), beta, self.segm,
                                                                             dict(self.regn, merge=self.merge)))
        return self._segment_maps[1]

    def _segment(self, whole):
        """`self.segments`, `<t>_segments.json` and `<t>_segments.npy`: a second confusion matrix over the pixels of the first, from
        the voted label map at their (x, y).  `self.test_matrix` and what `indicator()` makes of it stay as they are."""
        plain, seg, voted, *extra = self._segmented_maps(self.cfg['train']['save_best'])
        H, W = seg.shape
        raw = extra[0]['raw'] if extra else seg          # (connected regions, DESIGN §24: `seg` is then the region image)
        if self.segm['kind'] == 'file':
            counts = np.unique(raw, return_counts=True)[1]
        else:
            counts = np.bincount(raw.reshape(-1), minlength=int(np.prod(segments.grid(H, W, self.segm['size']))))
        self.segments = segments.report(self.segm, H, W, counts, self.test_matrix, *self._second_matrix(whole, plain, voted))
        if extra:
            self.segments = segments.region_report(self.segments, self.regn['min_size'], extra[0], extra[0]['sizes'])
        self.segment_image = seg
        self._write_block(self.segments, '_segments.json')
        if self.rank == 0:
            np.save(self.cfg['RESULT_output'] + str(self.time) + '_segments.npy', seg)

    def _color_segments(self, H, W, lut):
        """`<t>_pic_{1,2}_segments.png`: the voted classes."""
        self.segment_maps = self._color_remapped(H, W, lut, self._segmented_maps(True)[2], 'segments')

    # ------------------------------------------------------------------ colour
    def color(self):
        self._single_device_scope()
        self._ensure_model()
        self._load_weights(True)
        self.cur_model.eval()
        size = self.cfg['DATA_DICT'][self.cfg['data_city']]['size']
        H, W = int(size[0]), int(size[1])
        lut = np.asarray(self.cfg['DATA_DICT'][self.cfg['data_city']]['color'], dtype=np.uint8)
        ev, col, out = self.evaluation, self.cfg['color'], self.cfg['RESULT_output'] + str(self.time)
        confident = self.calib['confidence']           # color.confidence: the label maps come with their confidence planes
        if confident:
            beta = self._beta(self._temperature_used()[0])
        maps, planes = [], []
        with torch.no_grad():
            for n, use in ((1, col['supervised']), (2, col['unsupervised'])):
                if use and confident:
                    m, p = ev.confidence_map(n, H, W, beta)
                    maps.append(m); planes.append(p)
                else:
                    maps.append(ev.label_map(n, H, W) if use else np.zeros([H, W], dtype=np.int32))
                    if confident:
                        planes.append(np.zeros([3, H, W], dtype=np.float32))
        self.label_maps = (maps[0], map2(maps, col['unsupervised']))
        if col['supervised'] and self.rank == 0:
            for k, m in enumerate(self.label_maps, 1):
                Image.fromarray(lut[m]).save(out + '_pic_%d.png' % k)
        if confident:
            self.confidence_maps = (planes[0], map2(maps, col['unsupervised'], planes))
            if col['supervised'] and self.rank == 0:
                for k, p in enumerate(self.confidence_maps, 1):
                    np.save(out + '_confidence_%d.npy' % k, p)
                    grey = np.round(255.0 * p[0].astype(np.float64)).clip(0, 255).astype(np.uint8)
                    Image.fromarray(grey).save(out + '_conf_%d.png' % k)
        if self.spat['color']:
            with torch.no_grad():
                self._color_spatial(H, W, lut)
        if self.segm['color']:
            with torch.no_grad():
                self._color_segments(H, W, lut)

    def run(self):
        while self.time < self.TIME:
            self.dataloader()
            if self.cfg['train']['index']:
                self.train()
            if self.cfg['test']['index']:
                self.test()
            if self.cfg['color']['index']:
                self.color()
            self.time += 1
