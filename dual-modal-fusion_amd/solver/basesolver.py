"""solver.basesolver — scene loading, pixel table, splits and loaders (mirror of the reference BaseSolver).

Follows solver/basesolver.py:9-126 of the reference: read `ms4.tif` / `pan.tif`, normalise + pad, load `label.npy`,
build the row-major pixel table, `dataset_dual`, `random_split` of the labelled pixels with the GLOBAL torch RNG into
train / test / valid, five DataLoaders, `indicator()`.  Additions for the GPU path: the padded scenes are also kept
resident in HBM (`self.scene`), and every loader has an index-only twin (`*_index_loader`) that yields pixel
coordinates instead of materialised patches.  Iterating either twin consumes the global RNG exactly like the
reference's loader does, so a seeded run visits the same patches in the same order.  `_epoch_streams` gives the train twin's
next passes as arrays, without the loader and with the same RNG stream (`train.epoch_block`, solver.mainsolver).
`scene_prep: device` (NEW; fast path only, the drop-in path ignores it): the resident scene is normalised, padded and converted
on the GPU from the raw scenes (dmf.engine.Scene.from_raw), and the padded host arrays `self.MS` / `self.PAN` — and with them
the arrays behind the materialising loaders — are computed only when something asks for them.
`schedule.augment` / `test.tta` (NEW): on the fast path the resident scene becomes a scene atlas of the variants
either key needs (`Scene.atlas`: V x the scene in HBM); with both `none` it stays the plain Scene.
`band_reduce: pca` (NEW): right after `read_tif`, `self.ms` is replaced by the first `band_reduce_bands` principal
components of the normalised scene, a float32 [H, W, K] array; everything after that line takes it as the raw scene.
`band_reduce_noise` (NEW) beside it: the components are the noise-adjusted ones (MNF), ordered by signal-to-noise ratio.
`band_profile: morph` (NEW) after it: `self.ms` becomes the components and the openings / closings by reconstruction of
the first `band_profile_components` of them, a float32 [H, W, K + 2 n P] array.
`band_profile: area` (NEW) in its place: the area openings / closings at `band_profile_areas`, the same band count;
`band_profile_diagonals` / `band_profile_stds` (NEW) add thresholds on the same components' box diagonal and std.
"""
import os
import time

import numpy as np
import torch
from torch.utils.data import DataLoader, Subset

from dmf import augment
from function.function import data_padding, data_padding_aux, data_show, label_mat2np, read_tif, split_data, split_data_old
from indicators.kappa import aa_oa, expo_result
from train.dataset import collate_batched, dataset_dual
from utils import attribute, morphology, spectral


def epoch_orders(n, epochs, draws_after=0):
    """The orders (int64 [epochs, n]) in which a `DataLoader(shuffle=True)` over n items visits them in its next `epochs`
    passes, consuming the GLOBAL torch RNG exactly as iterating that loader `epochs` times would.  A pass draws twice from
    it, each time as `torch.empty((), dtype=torch.int64).random_()`: the loader iterator's base seed, then the sampler's
    seed, which seeds a fresh torch.Generator for `torch.randperm(n, generator=g)`.  draws_after: that many further draws
    after every pass, the base seeds of loaders WITHOUT shuffling that are iterated once between two passes (the validation
    loader of an epoch).  tests/test_epoch_block_host.py pins this against the real loader."""
    def draw():
        return int(torch.empty((), dtype=torch.int64).random_().item())
    orders = torch.empty(epochs, n, dtype=torch.int64)
    for e in range(epochs):
        draw()
        g = torch.Generator()
        g.manual_seed(draw())
        orders[e] = torch.randperm(n, generator=g)
        for _ in range(draws_after):
            draw()
    return orders


class BaseSolver:
    def __init__(self, cfg):
        self.cfg = cfg
        self.task = cfg['task']
        self.TIME = cfg['time']
        self.time = cfg['index']
        self.EPOCH = cfg['epoch']
        self.epoch = 0
        self.DEVICE = cfg['device']
        self.timestamp = int(time.time())
        self.num_workers = cfg['threads'] if cfg.get('gpu_mode') else 0
        self.aug_ops, self.tta_ops = augment.augment_keys(cfg)      # schedule.augment, test.tta: (0,) = none

        self.ms = read_tif(cfg, 'ms')
        self.pan = read_tif(cfg, 'pan')
        self.fast = bool(cfg.get('fast_path', 1)) and str(self.DEVICE).startswith('cuda')
        self.band_fit = None                                        # band_reduce: pca — the fit (utils.spectral.fit_basis + route)
        bands = spectral.band_keys(cfg)
        spectral.noise_keys(cfg)                                    # band_reduce_noise without band_reduce: refused by name
        profile = morphology.profile_keys(cfg)                      # band_profile without band_reduce: refused by name
        area = attribute.profile_keys(cfg)                          # (always read: band_profile_diagonals / _stds without the kind
        if profile is None:                                         #  area are refused by name)
            profile = area                                          # band_profile: area, its keys carry kind='area'
        self.band_profile_info = None                               # band_profile: morph / area — the kind's make_info dict
        if bands['kind'] is not None:                              # from here on the components ARE the raw primary scene
            self.ms, self.band_fit = self._band_reduce(bands, **({} if profile is None else {'profile': profile}))
        if profile is not None:                                    # .. and here their morphological profile is
            self.ms, self.band_profile_info = self._band_profile(profile)
        prep = cfg.get('scene_prep') or 'host'
        if prep not in ('host', 'device'):
            raise ValueError('scene_prep: %s is not one of host, device' % prep)
        self.device_prep = self.fast and prep == 'device'
        self._padded = {}
        if not self.device_prep:
            self.MS, self.PAN                                   # today's order of work: both padded scenes now

        label_path = cfg['data_address'] + 'label.npy'
        if not os.path.exists(label_path):
            label_mat2np(cfg)                                   # basesolver.py:34-35
        label_np = np.load(label_path)
        data_show(label_np)
        self.label_np = label_np
        self.data_new = cfg.get('data_new') == 1
        if self.data_new:                                       # basesolver.py:28-30,38-40: fixed train / test masks
            self.train_label = np.load(cfg['data_address'] + 'train.npy')
            self.test_label = np.load(cfg['data_address'] + 'test.npy')
            xyl_matrix, self.traintest_index = split_data(self.train_label, self.test_label, label_np, cfg)
            _, self.matrix_ = split_data_old(label_np, cfg)
        else:
            xyl_matrix, self.matrix_ = split_data_old(label_np, cfg)
        self.xyl = xyl_matrix
        if cfg.get('use_h5'):
            raise AttributeError("not finished")          # as the reference (basesolver.py:45-46)
        self.dataset = dataset_dual(*((lambda: self.MS, lambda: self.PAN) if self.device_prep else (self.MS, self.PAN)),
                                    xyl_matrix, cfg)
        self.index_dataset = self.dataset.index_view()
        print('All dataset size:', len(self.dataset))
        self.records = {'Epoch': [], 'PSNR': [], 'SSIM': [], 'Loss': []}
        self.scene = None
        # gmf.half: 1 — the fast path keeps the primary scene in fp16 and trains with the device loss scaler (the drop-in
        # path rounds its patches to fp16 as they are staged, model/gmfnet.py)
        self.half = bool((cfg.get('gmf') or {}).get('half', 0))
        if self.fast:
            from dmf.engine import Scene
            if self.device_prep:
                self.scene = Scene.from_raw(self.ms, self.pan, cfg['patch_size'], int(cfg.get('scale', 4)), self.DEVICE,
                                            half=self.half)
            else:
                self.scene = Scene(self.MS, self.PAN, self.DEVICE, half=self.half)
            # schedule.augment / test.tta: the resident scene becomes an atlas of the variants either key needs;
            # with both `none` it stays the plain Scene it was
            ops = augment.union_ops(self.aug_ops, self.tta_ops)
            if len(ops) > 1:
                self.scene = self.scene.atlas(cfg['patch_size'], int(cfg.get('scale', 4)), ops)

    def _band_reduce(self, keys, profile=None):
        """`band_reduce: pca` -> (the scene's first `band_reduce_bands` principal components as a float32
        [H, W, K] array, the fit).  Fast path: dmf.engine.band_reduce (the moments and the projection on the device, the fit on the
        host); `fast_path: 0`: utils.spectral.reduce_host.  Writes `<t>_band_reduce.npz`.  `band_reduce_noise`: the
        components are the noise-adjusted ones, on either route; with the key at none no argument is added to either call.
        profile: `band_profile`'s keys when that follows — the fast path then leaves the scores on the device."""
        cfg, K = self.cfg, keys['bands']
        noise = spectral.noise_keys(cfg)
        more = {} if noise is None else {'noise': noise}
        if self.ms.ndim != 3:
            raise ValueError('band_reduce wants a primary scene [H, W, C]')
        spectral.check_bands(K, self.ms.shape[2])
        if noise is not None:
            spectral.check_noise(noise, *self.ms.shape[:2])
        if self.fast:
            from dmf import lib
            from dmf.arch import arch_from_cfg
            from dmf.engine import band_reduce
            a = arch_from_cfg(cfg)
            try:
                lib.shape_supported(lib.make_shape(a))
            except lib.DmfError as e:
                raise lib.DmfError('%s; band_reduce_bands: %d%s needs the line "%d %d %d %d %d %d" in that file'
                                   % (e, K, '' if profile is None else ' with band_profile: %s' % profile.get('kind', 'morph'), a['C'], a['C2'], a['P'], a['S'], a['F'],
                                      a['G'])) from None
            if profile is not None:
                more['on_device'] = True
            scores, fit = band_reduce(self.ms, K, keys['whiten'], self.DEVICE, **more)
        else:
            scores, fit = spectral.reduce_host(self.ms, K, keys['whiten'], **more)
        if noise is None:
            print('band_reduce: %d of %d bands, %.4f of the variance, %s' % (K, self.ms.shape[2], float(fit['explained'].sum()), fit['route']))
        else:
            print('band_reduce: %d of %d bands, noise-adjusted (%s), SNR %.4g (first) to %.4g (component %d), %s'
                  % (K, self.ms.shape[2], noise, fit['snr'][0], fit['snr'][-1], K, fit['route']))
        if cfg.get('RESULT_output'):
            os.makedirs(cfg['RESULT_output'], exist_ok=True)
            spectral.save_fit(cfg['RESULT_output'] + str(self.time) + '_band_reduce.npz', fit)
        return scores, fit

    def _band_profile(self, keys):
        """`band_profile: morph` -> (the float32 [H, W, K + 2 n P] profile of the scores in `self.ms`, its info).  Fast
        path: dmf.engine.band_profile on the scores `_band_reduce` left on the device; `fast_path: 0`:
        utils.morphology.profile_host.  Writes `<t>_band_profile.json`."""
        cfg = self.cfg
        if keys.get('kind') == 'area':
            return self._area_profile(keys)
        if self.fast:
            from dmf.engine import band_profile
            ms, info = band_profile(self.ms, keys['components'], keys['radii'], self.DEVICE)
        else:
            ms, info = morphology.profile_host(self.ms, keys['components'], keys['radii'])
        print('band_profile: %d components at radii %s, %d bands, %d reconstruction rounds, %s'
              % (info['components'], info['radii'], info['bands'], sum(info['rounds']), info['route']))
        if cfg.get('RESULT_output'):
            os.makedirs(cfg['RESULT_output'], exist_ok=True)
            morphology.save_info(cfg['RESULT_output'] + str(self.time) + '_band_profile.json', info)
        return ms, info

    def _area_profile(self, keys):
        """`band_profile: area` -> (the float32 [H, W, K + 2 n P] attribute profile of the scores in `self.ms`, its
        info).  Fast path: dmf.engine.band_profile(kind='area'); `fast_path: 0`: utils.attribute.profile_host.  Writes
        `<t>_band_profile.json`."""
        cfg = self.cfg
        more = {k: keys[k] for k in ('diagonals', 'stds') if k in keys}       # (absent: the calls of §27 as they were)
        if self.fast:
            from dmf.engine import band_profile
            ms, info = band_profile(self.ms, keys['components'], None, self.DEVICE, kind='area', areas=keys['areas'], levels=keys['levels'],
                                    **more)
        else:
            ms, info = attribute.profile_host(self.ms, keys['components'], keys['areas'], keys['levels'], **more)
        print('band_profile: area, %d components at areas %s%s, %d levels, %d bands, %s'
              % (info['components'], info['areas'], ', diagonals %s, stds %s' % (info['diagonals'], info['stds']) if more else '',
                 info['levels'], info['bands'], info['route']))
        if cfg.get('RESULT_output'):
            os.makedirs(cfg['RESULT_output'], exist_ok=True)
            attribute.save_info(cfg['RESULT_output'] + str(self.time) + '_band_profile.json', info)
        return ms, info

    @property
    def MS(self):
        """The normalised, padded primary scene on the host (computed on first use)."""
        if 'MS' not in self._padded:
            self._padded['MS'] = data_padding(self.ms, self.cfg, 'ms')
        return self._padded['MS']

    @property
    def PAN(self):
        """The normalised, padded aux scene on the host (computed on first use)."""
        if 'PAN' not in self._padded:
            self._padded['PAN'] = data_padding(self.pan, self.cfg, 'pan') if self.pan.ndim == 2 else data_padding_aux(self.pan, self.cfg)
        return self._padded['PAN']

    def _loader(self, subset, batch, shuffle):
        twin = Subset(self.index_dataset, indices=subset.indices)
        return (DataLoader(dataset=subset, batch_size=batch, shuffle=shuffle, num_workers=self.num_workers),
                DataLoader(dataset=twin, batch_size=batch, shuffle=shuffle, num_workers=0, collate_fn=collate_batched))

    def dataloader(self):
        cfg = self.cfg

        def flat(s, base):             # random_split returns Subsets of a Subset; flatten to indices into the full dataset
            return Subset(self.dataset, indices=np.asarray(base)[np.asarray(s.indices)].tolist())

        color1 = Subset(self.dataset, indices=self.matrix_[1])             # the labelled pixels
        color2 = Subset(self.dataset, indices=self.matrix_[0])
        if self.data_new:
            # basesolver.py:64-84: the whole train mask trains; the test mask is split (global RNG) into test / valid
            train = Subset(self.dataset, indices=self.traintest_index[1])
            test_data = Subset(self.dataset, indices=self.traintest_index[2])
            valid_size = int(cfg['verify_rate'] * len(test_data))
            test, valid = (flat(s, self.traintest_index[2]) for s in torch.utils.data.random_split(
                test_data, [len(test_data) - valid_size, valid_size]))
        else:                              # the labelled pixels are split (global RNG) into train / test / valid
            train_size = int(cfg['train_rate'] * len(color1))
            valid_size = int(cfg['verify_rate'] * len(color1))
            train, test, valid = (flat(s, self.matrix_[1]) for s in torch.utils.data.random_split(
                color1, [train_size, len(color1) - train_size - valid_size, valid_size]))
        self.train_loader, self.train_index_loader = self._loader(train, cfg['batchsize'], True)
        self.test_loader, self.test_index_loader = self._loader(test, cfg['test_batchsize'], False)
        self.valid_loader, self.valid_index_loader = self._loader(valid, cfg['color_batchsize'], False)
        self.color_loader1, self.color_index_loader1 = self._loader(color1, cfg['test_batchsize'], False)
        self.color_loader2, self.color_index_loader2 = self._loader(color2, cfg['test_batchsize'], False)

    def _epoch_streams(self, epochs, draws_after=0):
        """The next `epochs` passes over `train_index_loader` without the loader: (xy [epochs, n, 2], labels [epochs, n]) int32
        on the host, row for row what iterating it gives (`epoch_orders`: same order, same RNG stream), taken from the index
        dataset's arrays by fancy indexing.  Rows [k * batchsize, (k + 1) * batchsize) of a pass are its k-th batch."""
        rows = np.asarray(self.train_index_loader.dataset.indices, dtype=np.int64)
        rows = rows[epoch_orders(len(rows), epochs, draws_after).numpy()]
        d = self.index_dataset
        return (torch.from_numpy(np.stack([d.x[rows], d.y[rows]], -1).astype(np.int32)),
                torch.from_numpy(d.label[rows].astype(np.int32)))

    def indicator(self):
        if self.cfg['test']['save_matrix']:
            np.save(self.cfg['RESULT_output'] + str(self.time) + "_matrix.npy", self.test_matrix)
        result = aa_oa(self.test_matrix)
        self.result = result
        expo_result(result, self.cfg, [self.train_time, self.test_time], self.time)

    def train(self):
        raise NotImplementedError

    def eval(self):
        raise NotImplementedError

    def run(self):
        while self.time < self.TIME:
            self.train()
            self.time += 1
