"""solver.evaluation — what `Solver.test()` and `Solver.color()` ask of a trained model, answered on either execution path.

Two classes with the same methods, chosen once (`Solver._ensure_model`): `EngineEvaluation` over the fast path's eval engine
(dmf/engine.py) and `DropinEvaluation` over the materialising loaders and `Net.forward`, through the solver's hooks
`_predict_dropin` and `_logits_dropin` (with `test.tta`, DESIGN §18, both give the mean logits over the variants).  Which loader
is iterated, and how often, is part of the contract — every iteration draws from torch's global RNG: the fast path takes the
validation and scene pixels from the index dataset's arrays (no loader), the drop-in path iterates `valid_loader` for the fit.

`test.calibration: 1`, `test.calibration_bins`, `test.temperature: none | fit | T` and `color.confidence: 1` (all optional, DESIGN
§17): after the confusion matrix and over the same pixels `test()` fills the reliability histogram, ECE, MCE and the mean NLL
(`self.calibration`, `<t>_calibration.json`), at the temperature T — a number, or with `fit` the temperature-scaling fit on
the VALIDATION split (`Solver._temperature_used`, once per trained model) —, and with T != 1 the same block `before` scaling;
`color()` also writes `<t>_confidence_{1,2}.npy` (float32 [3, H, W]: confidence, margin, entropy; 0 where nothing is coloured)
and `<t>_conf_{1,2}.png` (8-bit grey, round(255 conf)), composed as the label maps are (`map2`).  Fast path: dmf_softmax_stats /
dmf_calib_accum / dmf_temperature_step on the eval engine's logits, the label maps written by dmf_softmax_stats in
dmf_labelmap_write's place; drop-in path: torch ops in float64; both through utils/calibration.py.  `indicator()` and its export
are untouched; toStageSolver and data-parallel runs refuse the keys.  Neutral values change nothing.
`test.spatial: none | bilateral` with `test.spatial_radius`, `test.spatial_sigma_s`, `test.spatial_sigma_r`, `test.spatial_iterations`,
and `color.spatial: 1` (all optional): after the confusion matrix (and the calibration) `test()` classifies the pixels
of both colour sets — the whole scene — at `test.temperature`'s beta, smooths the class probabilities over each pixel's window
with scene-guided bilateral weights and forms a second confusion matrix over the same test pixels from the regularised map
(`self.spatial`, `<t>_spatial.json`: parameters, matrix, OA / AA / kappa before and after, pixels whose class changed); `color()`
also writes `<t>_pic_{1,2}_spatial.png`, composed as the plain maps are.  Fast path: EvalEngine.probability_map, Scene.affinity and
EvalEngine.regularise (dmf_prob_scatter / dmf_spatial_affinity / dmf_spatial_filter); drop-in path: utils/spatial.py in numpy
float64.  `test_matrix`, `indicator()` and its export are untouched; toStageSolver and data-parallel runs refuse the keys.
`test.segments: none | slic` with `test.segment_size`, `test.segment_compactness`, `test.segment_iterations`, `test.segment_vote` and
`color.segments: 1` (all optional): the same flow with superpixels in the filter's place — the whole-scene probability
map (the unfiltered one, whatever `test.spatial` says), SLIC segments of the primary scene, every pixel takes its segment's class;
a second confusion matrix over the same test pixels (`self.segments`, `<t>_segments.json`, `<t>_segments.npy`: the int32 segment
image); `color()` also writes `<t>_pic_{1,2}_segments.png`.  Fast path: EvalEngine.probability_map, Scene.segments and
EvalEngine.segment_vote (dmf_slic_* / dmf_segment_vote); drop-in path: utils/segments.py in numpy float64.
`test.segment_connectivity: 1` with `test.segment_min_size`, and `test.segments: file` with `test.segment_file`: the
segment image (SLIC's, or the file's) becomes connected regions, small fragments join the component before them, and the vote runs
over the regions (Scene.segment_regions, EvalEngine.region_vote: dmf_label_components / dmf_region_merge / dmf_region_vote; drop-in
path: utils.segments.regions / region_vote, the same integers); `<t>_segments.npy` then holds the region image.
`test.segment_merge: spectrum` sends every fragment to the adjacent group with the nearest mean spectrum and lets groups
of fragments grow into regions (dmf_region_graph_count / dmf_region_graph_merge; drop-in path: utils.segments.region_graph).
"""
import itertools

import numpy as np
import torch

from utils import calibration as calib
from utils import segments, spatial


def map2(maps, unsupervised, values=None):
    """Map 2 of `values` ([..., H, W] per colour set; default: the label maps): the unsupervised set's where its LABEL is not 0."""
    values = maps if values is None else values
    return np.where(maps[1] != 0, values[1], values[0]) if unsupervised else values[0]


class _Evaluation:
    def __init__(self, solver):
        self.s = solver


class EngineEvaluation(_Evaluation):
    """The fast path: `solver.eval_engine` (read at every call: `train()` builds a new one)."""

    def _set_xy(self, n):
        return torch.cat([self.s._xy_labels(b)[0] for b in getattr(self.s, 'color_index_loader%d' % n)])

    def confusion(self, whole):
        """The whole split in evaluation chunks of the engine's own size (data parallel: every rank classifies its part of
        the pixels, the matrices are summed), or the first batch alone, which every rank classifies whole."""
        s = self.s
        return s.eval_engine.confusion(*s._test_pixels(whole), process_group=s.process_group if whole else None).cpu().numpy()

    def split_logits(self, split, whole=True):
        """(logits [n, K], labels [n]) on the device: the validation split, or the test pixels of the confusion matrix."""
        return self.s.eval_engine.collect_logits(*(self.s._valid_split() if split == 'valid' else self.s._test_pixels(whole)))

    def fit(self, logits, labels):
        """-> n, beta, steps, nll_at_1, nll_at_T (sums): 40 safeguarded Newton steps on the device, read back once."""
        at_one, state, at_fit = self.s.eval_engine.fit_temperature_of(logits, labels, steps=calib.FIT_STEPS)
        return int(labels.shape[0]), float(state[0]), int(state[6]), float(at_one[1]), float(at_fit[1])

    def reliability(self, logits, labels, bins, beta):
        eng = self.s.eval_engine
        hist = eng.calibration_of(logits, labels, bins, beta).cpu().numpy()
        return hist, float(eng.nll_of(logits, labels, beta)[1].item()) if logits.shape[0] else 0.0

    def label_map(self, n, H, W):
        return self.s.eval_engine.label_map(self._set_xy(n), H, W, process_group=self.s.process_group).cpu().numpy()

    def confidence_map(self, n, H, W, beta):
        """`label_map` with the confidence planes [3, H, W]: one dmf_softmax_stats per chunk writes all four maps."""
        m, p = self.s.eval_engine.confidence_maps(self._set_xy(n), H, W, beta)
        return m.cpu().numpy(), p.cpu().numpy()

    def scene_maps(self, xy, H, W, beta, k):
        eng = self.s.eval_engine
        prob, mask = eng.probability_map(torch.from_numpy(xy), H, W, beta)
        aff = self.s.scene.affinity(H, W, k['radius'], k['sigma_s'], k['sigma_r'])
        return None, eng.regularise(prob, mask, aff, k['iterations'])[1].cpu().numpy()

    def scene_segments(self, xy, H, W, beta, k, rk=None):
        """-> (None, segment image, voted label map): EvalEngine.probability_map, Scene.segments, EvalEngine.segment_vote.  With
        the region keys `rk` on: (None, region image, voted label map, dict(regions, components, absorbed, sizes, raw))."""
        eng = self.s.eval_engine
        prob, mask = eng.probability_map(torch.from_numpy(xy), H, W, beta)
        if rk is None or not rk['connectivity']:
            seg = self.s.scene.segments(H, W, k['size'], k['compactness'], k['iterations'])[0]
            return None, seg.cpu().numpy(), eng.segment_vote(prob, mask, seg, k['size'], k['vote'])[2].cpu().numpy()
        # connected regions: Scene.segment_regions on SLIC's image or the file's, EvalEngine.region_vote
        if k['kind'] == 'file':
            seg, n_labels = torch.from_numpy(segments.load_segment_file(rk['file'], H, W)).to(prob.device), 0
        else:
            seg, n_labels = self.s.scene.segments(H, W, k['size'], k['compactness'], k['iterations'])[0], int(np.prod(segments.grid(H, W, k['size'])))
        region, R, sizes, stats = self.s.scene.segment_regions(seg, H, W, n_labels, rk['min_size'], merge=rk.get('merge', 'position'))
        voted = eng.region_vote(prob, mask, region, R, k['vote'])[2].cpu().numpy()
        return None, region.cpu().numpy(), voted, dict(stats, sizes=sizes.cpu().numpy(), raw=seg.cpu().numpy())

    def plain_at(self, xy, plain, H, W):
        return self.s.eval_engine.label_map(torch.from_numpy(xy), H, W).cpu().numpy()[xy[:, 0], xy[:, 1]]


class DropinEvaluation(_Evaluation):
    """The drop-in path: the materialising loaders through the solver's `_predict_dropin` / `_logits_dropin`."""

    def _logits(self, loader):
        """(logits [n, K] float64, labels [n]) as numpy over the batches of a materialising loader."""
        s = self.s
        out = [(s._logits_dropin(d1.to(s.DEVICE), d2.to(s.DEVICE)).detach().double().cpu().numpy(), np.asarray(t))
               for d1, d2, t, _, _ in loader]
        return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out]).astype(np.int64)

    def _test_batches(self, whole):
        return self.s.test_loader if whole else itertools.islice(self.s.test_loader, 1)

    def confusion(self, whole):
        K = self.s.cfg['Categories_Number']
        matrix = np.zeros([K, K])
        for batch in self._test_batches(whole):
            pred, target, _, _ = self.s._predict_dropin(batch)
            np.add.at(matrix, (pred.cpu().numpy(), target.long().numpy()), 1)            # test_matrix[pred][target] += 1
        return matrix

    def split_logits(self, split, whole=True):
        return self._logits(self.s.valid_loader if split == 'valid' else self._test_batches(whole))

    def fit(self, logits, labels):
        """-> n, beta, steps, nll_at_1, nll_at_T (sums): the device's rule on the host (utils.calibration)."""
        f = calib.fit_temperature(logits, labels)
        return len(labels), f['beta'], f['steps'], calib.nll_terms(logits, labels, 1.0)[0], calib.nll_terms(logits, labels, f['beta'])[0]

    def reliability(self, logits, labels, bins, beta):
        pred, st = calib.softmax_stats(torch.from_numpy(logits), beta)
        return calib.histogram(st[0].numpy(), pred.numpy(), labels, logits.shape[1], bins), calib.nll_terms(logits, labels, beta)[0]

    def label_map(self, n, H, W):
        m = np.zeros([H, W], dtype=np.int32)
        for batch in getattr(self.s, 'color_loader%d' % n):
            pred, _, x, y = self.s._predict_dropin(batch)
            m[np.asarray(x), np.asarray(y)] = pred.cpu().numpy()
        return m

    def confidence_map(self, n, H, W, beta):
        s = self.s
        m, p = np.zeros([H, W], dtype=np.int32), np.zeros([3, H, W], dtype=np.float32)
        for data1, data2, _, x, y in getattr(s, 'color_loader%d' % n):
            logits = s._logits_dropin(data1.to(s.DEVICE), data2.to(s.DEVICE))
            x, y = np.asarray(x), np.asarray(y)
            m[x, y] = logits.data.max(1)[1].cpu().numpy()                  # (the prediction of `_predict_dropin`)
            p[:, x, y] = calib.softmax_stats(logits, beta)[1].cpu().numpy().astype(np.float32)
        return m, p

    def _scene_probabilities(self, xy, H, W, beta):
        """-> (prob [H, W, K] float64, mask, plain label map, the host's padded scene) from the logits of `Net.forward`."""
        from torch.utils.data import DataLoader, Subset
        s = self.s
        rows = list(s.matrix_[1]) + list(s.matrix_[0])
        loader = DataLoader(Subset(s.dataset, indices=rows), batch_size=s.cfg['color_batchsize'], shuffle=False,
                            num_workers=0, generator=torch.Generator())       # (a generator of its own: the global stream stays)
        logits = self._logits(loader)[0]
        prob, mask = np.zeros((H, W, logits.shape[1])), np.zeros((H, W), dtype=np.uint8)
        prob[xy[:, 0], xy[:, 1]] = spatial.probabilities(logits, beta)
        mask[xy[:, 0], xy[:, 1]] = 1
        plain = np.zeros((H, W), dtype=np.int32)
        plain[xy[:, 0], xy[:, 1]] = logits.argmax(1)
        return prob, mask, plain, s.MS.astype(np.float16) if s.half else s.MS

    def scene_maps(self, xy, H, W, beta, k):
        """-> (plain, regularised) label maps: utils.spatial in float64 on the logits of `Net.forward` and the host's padded scene."""
        prob, mask, plain, scene = self._scene_probabilities(xy, H, W, beta)
        aff = spatial.affinity(scene, H, W, k['radius'], k['sigma_s'], k['sigma_r'])
        return plain, spatial.regularise(prob, mask, aff, k['radius'], k['iterations'])[1]

    def scene_segments(self, xy, H, W, beta, k, rk=None):
        """-> (plain, segment image, voted label map): utils.segments in float64 on the same logits and scene.  With the region
        keys `rk` on: the region image in the segment image's place and dict(regions, components, absorbed, sizes, raw) after them,
        by utils.segments' integer arithmetic."""
        prob, mask, plain, scene = self._scene_probabilities(xy, H, W, beta)
        if rk is None or not rk['connectivity']:
            seg = segments.slic(scene, H, W, k['size'], k['compactness'], k['iterations'])[0]
            return plain, seg, segments.vote(prob, mask, seg, k['size'], k['vote'])[2]
        if k['kind'] == 'file':
            seg, n_labels = segments.load_segment_file(rk['file'], H, W), 0
        else:
            seg, n_labels = segments.slic(scene, H, W, k['size'], k['compactness'], k['iterations'])[0], int(np.prod(segments.grid(H, W, k['size'])))
        if rk.get('merge') == 'spectrum':                    # (the same integers and double operations as the device's)
            region, sizes, stats = segments.region_graph(seg, scene, n_labels, rk['min_size'])
        else:
            region, sizes, stats = segments.regions(seg, n_labels, rk['min_size'])
        voted = segments.region_vote(prob, mask, region, stats['regions'], k['vote'])[2]
        return plain, region, voted, dict(stats, sizes=sizes, raw=seg)

    def plain_at(self, xy, plain, H, W):
        return plain[xy[:, 0], xy[:, 1]]
