"""solver.tostagesolver — `toStageSolver(cfg).run()`: the reference's two-stage path (solver/tostagesolver.py:20-414).

Stage 2 is built (tostagesolver.py:240-414): the four co-registered 4-band scenes (ms, pan = `pan.npy`, ms_gan, pan_gan)
are padded, sliced by `dataset_qua_dqtl`, concatenated on the batch axis and pushed through ONE single-input network
(`model.<model_name>.Net(args=cfg)` called as `net(data)`; this build's GMFNet takes the band mean of its input as the
auxiliary modality, cfg['gmf']['single_input'] = 1), trained with `qua_loss` + ADAM, best epoch by the early-stopping
validation loop, prediction = argmax softmax(out[:bs] + out[bs:2bs]).  `train()`, the fast epoch, `test()` and `color()`
are solver.mainsolver's, with its two execution paths (evaluation: solver/evaluation.py, whose drop-in class calls `_predict_dropin`),
its epoch loop (`_train_epochs`) and its epoch ledger (`_record_epoch`, `_save_current`); what stage 2 states differently is the hooks below:

  hook                  Solver                                        toStageSolver
  engine_loss             Criterion                                     qua_loss
  _train_engine         TrainEngine on the two scenes; may carry      QuaTrainEngine on the four scenes resident as one tall scene
                        the one-shot xgmi exchange                    (forward, dmf_qua_loss, backward, reduce+ADAM)
  _eval_engine          EvalEngine                                    QuaEvalEngine (the ms and pan streams only)
  _rank_batches         the solver shards every global batch on       the engine shards (`load_plan` / `step` take global batches);
                        the host; a full one: batchsize // world      a full one: batchsize; one with no pixel for some rank is left out
  _steps_per_graph      default -1 (the library's launch loop)        default 0, and 0 unless the engine has the unit-gradient step
  _step_short           device tensors; mean per-patch loss           host tensors; the engine's batch loss
  _train_epoch_dropin   net(ms, pan), Criterion (:49-55)              net(concat of the four streams), qua_loss (:268-278; the same
  (returns the epoch's                                                HIP loss kernel behind an autograd Function)
  step losses)
  _valid_pass           cross-entropy; fast: summed on the device     qua_loss, read back per batch on both paths (early exit, :288-296)
  (the ledger's value)  (EvalEngine.ce_sum)
  _predict_dropin       argmax of net(ms, pan)                        pair_argmax of net(concat(ms, pan)) (:337)
  _test_whole_split     only with `test.full: 1` (reference: first    always (:331-341)
                        batch)
  epoch_blocks          True: `train.epoch_block` > 1 trains in       False: `train.epoch_block` > 1 is refused, the epoch loop
                        blocks of epochs (`_train_blocks`)            is the only one

Stage 1 (:86-238) trains `model.generator` / `model.discriminator`, which the reference does not ship: it
is NOT built.  Run stage 2 on stage-1 outputs that already exist (`dqtl.pre_trained: 1`: `msgan.npy`, `pangan.npy`
under cfg['expo_result'] + cfg['dqtl']['WEIGHTS'], as the reference does at :241-243).  `pan.npy` (:246) is produced
from the PAN image with `pan2ms` (image_convert/IHS.py:14-19, on the GPU) when the file does not exist.
`gmf.half: 1` on the fast path: fp16 tall scene and the device loss scaler around the ADAM step (as in solver.mainsolver).
`scene_prep: device` on the fast path: the tall scene is prepared on the GPU from the four raw scenes (QuaScene.from_raw).
Data parallel (`test.py` with `solver: toStageSolver` under `torch.distributed.run`, fast path only): every rank iterates the
same shuffled stream, the engine trains each rank on its contiguous shard of every global batch and evaluates the loss on
the gathered global batch (dmf.engine.QuaTrainEngine); the short last batch is sharded the same way (a remainder that the
world size does not divide is dropped); test / colour shard the pixels; rank 0 writes the artefacts.
Deliberate differences: label maps are written as PNG (the reference writes .jpg here and .png in Solver); `nohup: 1`
works (reference bug at :300); the t-SNE / feature visualisation helpers (:416-530) are out of scope.
"""
import os

import numpy as np
import torch

from function.function import data_padding, data_show, split_data_old
from solver.mainsolver import Solver
from train.dataset import dataset_qua_dqtl
from utils.utils import clip_grad_norm_of


class toStageSolver(Solver):
    engine_loss = 'qua_loss'
    epoch_blocks = False                                 # (its validation is a batch-coupled loss read back per batch)
    weight_averaging = False                             # (schedule.weight_average is out of scope here: refused by name)
    calibrated = False                                   # (test.calibration, test.temperature, color.confidence: refused by name)
    augmented = False                                    # (schedule.augment, test.tta: refused by name)
    regularised = False                                  # (test.spatial, color.spatial: refused by name)
    segmented = False                                    # (test.segments, color.segments: refused by name)
    band_reduced = False                                 # (band_reduce: refused by name)

    def __init__(self, cfg):
        super().__init__(cfg)
        self.qua_scene = None
        self.ms_gan = self.pan_gan = None

    # ------------------------------------------------------------------ stage 1 (not built)
    def train_stage1(self):
        raise NotImplementedError('stage 1 (GAN pre-fusion, tostagesolver.py:86-238) needs model.generator / '
                                  'model.discriminator, which the reference does not ship; provide msgan.npy / '
                                  'pangan.npy and set dqtl.pre_trained: 1')

    # ------------------------------------------------------------------ stage 2 data (tostagesolver.py:240-257)
    def train_stage2(self):
        cfg = self.cfg
        d = cfg['dqtl']
        if not d.get('pre_trained'):
            self.train_stage1()
        base = cfg.get('expo_result', '') + d.get('WEIGHTS', '')
        self.ms_gan = np.load(base + 'msgan.npy')
        self.pan_gan = np.load(base + 'pangan.npy')
        pan_path = cfg['data_address'] + '/pan.npy'
        if os.path.exists(pan_path):
            PAN = np.load(pan_path)
        else:
            from image_convert.IHS import pan2ms, pan2ms_gpu
            size = [self.ms.shape[0], self.ms.shape[1], 4]
            PAN = pan2ms_gpu(self.pan, size, self.DEVICE) if str(self.DEVICE).startswith('cuda') else pan2ms(self.pan, size)
        raw = (self.ms, PAN, self.ms_gan, self.pan_gan)
        padded = []

        def scene(k):                                   # the padded host scenes, all four on the first use of one
            def get():
                if not padded:
                    padded.extend(data_padding(x, cfg, 'ms') for x in raw)
                return padded[k]
            return get
        scenes = [scene(k) for k in range(4)]           # `scene_prep: device`: only the materialising loader calls them
        if not self.device_prep:
            scenes = [get() for get in scenes]
        label_np = np.load(cfg['data_address'] + 'label.npy')
        data_show(label_np)
        xyl_matrix, self.matrix_ = split_data_old(label_np, cfg)
        self.dataset = dataset_qua_dqtl(scenes[0], scenes[1], scenes[2], scenes[3], xyl_matrix, cfg)
        self.index_dataset = self.dataset.index_view()
        if self.fast:
            from dmf.engine import QuaScene
            if self.device_prep:
                self.qua_scene = QuaScene.from_raw(raw, cfg['patch_size'], self.DEVICE, half=self.half)
            else:
                self.qua_scene = QuaScene(scenes, self.DEVICE, half=self.half)

    # ------------------------------------------------------------------ what stage 2 states differently: fast path
    def _steps_per_graph(self):
        return int(self.cfg.get('steps_per_graph', 0)) if self.engine.unit else 0

    def _train_engine(self, batch, kw):
        from dmf.engine import QuaTrainEngine
        return QuaTrainEngine(self.cur_model, self.qua_scene, batch, self.cfg['dqtl'], **kw)

    def _eval_engine(self):
        from dmf.engine import QuaEvalEngine
        # (evaluation chunks of the engine's own size, as in Solver._eval_engine: the configured sizes belong to the host-fed loader)
        return QuaEvalEngine(self.cur_model, self.qua_scene, max(self.cfg['test_batchsize'], self.cfg['color_batchsize'], 8192),
                             self.cfg['dqtl'])

    def _rank_batches(self, batches):
        """Global batches: the engine takes this rank's shard, so a batch needs a pixel for every rank."""
        return [b for b in batches if b[0].shape[0] >= self.world], self.cfg['batchsize']

    def _step_short(self, xy, lab):
        self.engine.step(xy, lab)
        return float(self.engine.loss.item())

    # ------------------------------------------------------------------ ... and drop-in path
    def _train_epoch_dropin(self):
        loader = self._bar(self.train_loader)
        losses = []
        max_norm = clip_grad_norm_of(self.cfg['schedule'])           # schedule.clip_grad_norm (None: the reference's loop)
        per_step = self.scheduler_unit == 'step' and self.scheduler is not None
        for data1, data2, data3, data4, target, _, _ in loader:
            data = torch.concat([data1, data2, data3, data4]).to(self.DEVICE)            # tostagesolver.py:270-272
            target = target.to(self.DEVICE)
            bs = len(data1)
            self.optimizer.zero_grad()
            output = self.cur_model(data)
            loss = self.loss(output, bs, target, self.cfg)
            loss.backward()
            if max_norm:
                torch.nn.utils.clip_grad_norm_(self.cur_model.parameters(), max_norm)
            self.optimizer.step()
            if per_step:
                self.scheduler.step()                                # schedule.scheduler_unit: step
            losses.append(loss.item())
            if not self.cfg['nohup']:
                loader.set_postfix(loss=losses[-1], epoch=self.epoch, time=self.time, mode='train')
        if self.cfg['schedule']['if_scheduler'] and not per_step:
            self.scheduler.step()
        return losses

    def _valid_pass(self, best_loss):
        val_loss = 0.0
        with torch.no_grad():
            if self.fast:
                for batch in self.valid_index_loader:
                    xy, lab = self._xy_labels(batch)
                    val_loss += self.eval_engine.loss_value(xy, lab).item() * xy.shape[0]
                    if val_loss > best_loss:
                        break
            else:
                for data1, data2, data3, data4, target, _, _ in self.valid_loader:
                    data = torch.concat([data1, data2, data3, data4]).to(self.DEVICE)
                    output = self.cur_model(data)
                    val_loss += self.loss(output, len(data1), target.to(self.DEVICE), self.cfg).item() * data1.size(0)
                    if val_loss > best_loss:
                        break
        return val_loss

    def _predict_dropin(self, batch):
        from dmf import lib
        data1, data2, _, _, target, x, y = batch
        bs = len(data1)
        out = self.cur_model(torch.concat([data1, data2]).to(self.DEVICE))
        pred = torch.empty(bs, dtype=torch.int32, device=out.device)
        lib.pair_argmax(out.contiguous(), bs, pred)                                      # tostagesolver.py:337
        return pred, target, x, y

    def _test_whole_split(self):
        return True                                                                      # every batch (:331-341)

    def run(self):
        self.train_stage2()
        super().run()
