"""Resident-scene training / evaluation engine (the fast path behind the solvers).

What it removes from the reference's hot loop (solver/mainsolver.py:49-58):
  * per-item host patch slicing + 3 H2D copies per step  -> padded scenes live in HBM, patches are
    gathered on-device from pixel coordinates (`dmf_input` mode 1);
  * forward / CE / backward / Adam as separate framework ops -> two launches per step
    (`dmf_train_fwd_bwd`, `dmf_grad_reduce_adam`; with `gmf.attention` four: token kernel, attention fwd+bwd kernel,
    conv backward, reduce+Adam — `dmf_train_attn_fwd_bwd`);
  * `loss.item()` every step                               -> per-step mean loss kept on the device;
  * per-launch host work                                   -> an epoch plan (shuffled coordinates + labels) is
    uploaded once and a captured hipGraph of `steps_per_graph` steps is replayed; batch cursor and the
    Adam step count live in device memory;
  * the host between the phases of an epoch                -> `train.epoch_block`: the plan holds the full batches of several
    epochs (`TrainEngine.load_block`: host arrays, checked as they are by the ONE plan upload `_PlanEngine._upload_plan`), the
    short last batch is stepped from the device copy (`step_short`), the validation sum is formed by `EvalEngine.valid_accum`
    and judged by `dmf_keep_best`: no host sync until the block ends.
Data parallel (world_size > 1) gives identical updates on every rank, from ONE flat fp32 gradient per step: exchanged
inside the reduce + Adam launch by a `dmf.xgmi.Communicator`, or all-reduced over the process group.  What runs after the
backward, for every optimiser, loss-scaler and group form of both train engines: `_PlanEngine._update`.
"""
import contextlib
import sys

import numpy as np
import torch

from . import lib


_hip_graph_upload = None


def _upload_graph(g):
    """hipGraphUpload of a freshly captured graph: its first replay otherwise pays the upload (~20 us, measured with
    tools/graph_first.py) inside whatever the caller is timing.  Returns True when the upload happened; a missing symbol or a
    non-zero return code leaves the lazy upload in place (correct either way, only the first replay is slower)."""
    global _hip_graph_upload
    import ctypes
    if _hip_graph_upload is None:
        rt = lib.hip_runtime_of_torch()
        fn = getattr(rt, 'hipGraphUpload', None) if rt is not None else None
        if fn is None:
            _hip_graph_upload = False
        else:
            fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
            fn.restype = ctypes.c_int
            _hip_graph_upload = fn
    if not _hip_graph_upload:
        return False
    rc = _hip_graph_upload(ctypes.c_void_p(g.raw_cuda_graph_exec()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    return rc == 0


def reflect_index(i, n):
    """Source index of output index i along an axis of n samples padded at its end by reflection without the edge
    (numpy 'reflect' / cv2.BORDER_REFLECT_101, function.data_padding): the rule of dmf_scene_prepare.  Valid for i <= 2 (n - 1)."""
    return i if i < n else 2 * (n - 1) - i


def prep_route(dtype, H, W, pad, mn=None, mx=None):
    """Where a raw scene [H, W(, C)] of numpy dtype `dtype` is normalised and padded by `pad`: ('device', '') or
    ('host', why).  The host keeps what dmf_scene_prepare does not state: a dtype without a DMF_RAW_* code, a pad beyond the
    reflection's reach (numpy reflects again and again), and an integer scene whose max - min (`mn`, `mx`: its extremes, once
    they are known) is not representable in the raw type, where numpy's subtraction wraps around."""
    dtype = np.dtype(dtype)
    if lib.raw_code(dtype) is None:
        return 'host', 'dtype %s has no device code' % dtype
    if pad < 0 or pad > H - 1 or pad > W - 1:
        return 'host', 'pad %d exceeds the reflection of a %d x %d scene' % (pad, H, W)
    if mn is not None and dtype.kind in 'iu' and int(mx) - int(mn) > np.iinfo(dtype).max:
        return 'host', 'max - min = %d wraps around in %s' % (int(mx) - int(mn), dtype)
    return 'device', ''


def _prepare_on_device(raw, pad, out):
    """out [H+pad, W+pad, C] (device, fp32 / fp16) <- the normalised, padded scene of the raw numpy scene [H, W(, C)], which is
    uploaded in its own dtype and freed again.  Returns '' or, where only the extremes tell (prep_route), why the host has to
    do it.  One host sync: the two extremes are read back."""
    H, W = raw.shape[:2]
    C = raw.shape[2] if raw.ndim == 3 else 1
    name = raw.dtype.name
    raw_d = torch.from_numpy(np.ascontiguousarray(raw).reshape(-1).view(np.uint8)).to(out.device)
    minmax = torch.empty(16, dtype=torch.uint8, device=out.device)
    lib.scene_minmax(raw_d, name, minmax)
    mn, mx = minmax.cpu().numpy().view(raw.dtype)[:2]
    why = prep_route(raw.dtype, H, W, pad, mn, mx)[1]
    if not why:
        lib.scene_prepare(raw_d, name, H, W, C, minmax, pad, out)
    return why


def _host_fallback(why):
    print('dmf: scene preparation on the host (%s)' % why, flush=True)


def _noise_adjusted_fit(x, H, W, K, whiten, noise):
    """The fit of `band_reduce_noise` for the normalised scene x [H W, C] on the device -> (mean on the device,
    fit): dmf_band_moments, one dmf_band_noise_moments per direction, ONE read-back of C + C^2 (1 + directions) doubles, and
    utils.spectral.fit_noise_adjusted on the host."""
    from utils import spectral
    C = x.shape[1]
    dirs = spectral.noise_directions(noise)
    buf = torch.empty(C + C * C * (1 + len(dirs)), dtype=torch.float64, device=x.device)
    mean, mats = buf[:C], buf[C:].view(1 + len(dirs), C, C)
    lib.band_moments(x, mean, mats[0])
    ws = torch.empty(lib.band_noise_workspace_bytes(H, W, C) // 8, dtype=torch.float64, device=x.device)
    for i, d in enumerate(dirs):
        lib.band_noise_moments(x, H, W, mats[1 + i], d, ws)
    host = buf.cpu().numpy()
    hm = host[C:].reshape(1 + len(dirs), C, C)
    return mean, spectral.fit_noise_adjusted(host[:C].copy(), hm[0], spectral.combine_noise(hm[1:]), K, whiten, noise=noise)


def band_reduce(raw, K, whiten, device, noise=None, on_device=False):
    """`band_reduce: pca` on the device -> (scores [H, W, K] float32 on the host, fit).  The raw primary scene
    [H, W, C] is uploaded in its own dtype and normalised unpadded (dmf_scene_minmax / dmf_scene_prepare at pad 0, fp32) — on the
    host, saying why, where prep_route sends it there; dmf_band_moments gives mean and covariance, which are read back once
    (C + C^2 doubles) for utils.spectral.fit_basis; dmf_band_project writes the scores, which are copied back once.  `fit` is
    fit_basis's dict plus `route`.  noise: None, or a direction of `band_reduce_noise`: the noise moments join
    the read-back and the fit is fit_noise_adjusted's; everything else is as without it.  on_device: the scores are returned as
    the float32 [H, W, K] tensor on the device and not copied back (what `band_profile` takes next)."""
    from utils import spectral
    raw = np.asarray(raw)
    if raw.ndim != 3:
        raise lib.DmfError('band_reduce wants a primary scene [H, W, C]')
    H, W, C = raw.shape
    K = int(K)
    spectral.check_bands(K, C)
    if noise is not None:
        spectral.check_noise(noise, H, W)
    device = torch.device(device)
    with torch.cuda.device(device):
        x = torch.empty(H, W, C, dtype=torch.float32, device=device)
        why = prep_route(raw.dtype, H, W, 0)[1] or _prepare_on_device(raw, 0, x)
        if why:
            print('dmf: band_reduce normalises the scene on the host (%s)' % why, flush=True)
            x = torch.from_numpy(spectral.normalise(raw)).to(device)
        x = x.view(H * W, C)
        if noise is None:
            mean = torch.empty(C, dtype=torch.float64, device=device)
            cov = torch.empty(C, C, dtype=torch.float64, device=device)
            lib.band_moments(x, mean, cov)
            fit = spectral.fit_basis(mean.cpu().numpy(), cov.cpu().numpy(), K, whiten)
        else:
            mean, fit = _noise_adjusted_fit(x, H, W, K, whiten, noise)
        y = torch.empty(H * W, K, dtype=torch.float32, device=device)
        lib.band_project(x, mean, torch.from_numpy(fit['basis']).to(device), y)
        scores = y.view(H, W, K) if on_device else y.cpu().numpy().reshape(H, W, K)
    fit['route'] = 'device' if not why else 'device, normalised on the host (%s)' % why
    return scores, fit


ATTR_BATCH = 16                                  # levels per dmf_attr_area_levels call (lib.ATTR_BATCH_MAX)


def _area_profile(scores, P, areas, levels, device, batch=ATTR_BATCH):
    """`band_profile: area` on the device: dmf_attr_quantise, ceil((L - 1) / batch) dmf_attr_area_levels calls that
    read nothing back, dmf_attr_stack, and ONE copy back (the profile; the P ranges ride along for the JSON file)."""
    from utils import attribute, morphology
    areas, L = attribute.check_areas(areas), attribute.check_levels(levels)
    device = torch.device(device)
    if isinstance(scores, np.ndarray):
        scores = torch.from_numpy(np.ascontiguousarray(scores, dtype=np.float32)).to(device)
    if not (torch.is_tensor(scores) and scores.dim() == 3 and scores.dtype == torch.float32 and scores.device.type == 'cuda'):
        raise lib.DmfError('band_profile wants the float32 scores [H, W, K] of band_reduce')
    H, W, K = scores.shape
    P, n = int(P), len(areas)
    morphology.check_components(P, K)
    T = max(1, min(int(batch), L - 1))
    with torch.cuda.device(scores.device):
        if not bool(torch.isfinite(scores).all()):
            raise ValueError('band_profile: the scores hold a value that is not finite')
        ws = torch.empty(lib.attr_workspace_bytes(H, W, P, n, T), dtype=torch.uint8, device=scores.device)
        q = torch.empty(2 * P, H, W, dtype=torch.uint8, device=scores.device)
        count = torch.empty(2 * P, n, H, W, dtype=torch.uint8, device=scores.device)
        cells = H * W * attribute.band_count(K, P, n)
        both = torch.empty(cells + 2 * P, dtype=torch.float32, device=scores.device)      # the profile, then the P ranges: one copy
        out, rng = both[:cells].view(H, W, -1), both[cells:].view(P, 2)
        lib.attr_quantise(scores, P, L, q, rng, ws)
        lib.attr_area_run(q, areas, L, count, ws, T)
        lib.attr_stack(scores, P, n, L, count, rng, out)
        host = both.cpu().numpy()
        profile, ranges = host[:cells].reshape(H, W, -1), host[cells:].reshape(P, 2)
    return profile, attribute.make_info(K, P, areas, L, ranges, 'device')


def _multi_profile(scores, P, areas, diagonals, stds, levels, device, batch=ATTR_BATCH):
    """`band_profile: area` with diagonals and / or stds on the device: _area_profile with dmf_attr_multi_levels in
    the place of dmf_attr_area_levels and the threshold list areas ++ diagonals ++ stds in the place of the areas; ONE copy back."""
    from utils import attribute, morphology
    L = attribute.check_levels(levels)
    areas, diagonals, stds = attribute.check_thresholds(areas, diagonals, stds, L)
    device = torch.device(device)
    if isinstance(scores, np.ndarray):
        scores = torch.from_numpy(np.ascontiguousarray(scores, dtype=np.float32)).to(device)
    if not (torch.is_tensor(scores) and scores.dim() == 3 and scores.dtype == torch.float32 and scores.device.type == 'cuda'):
        raise lib.DmfError('band_profile wants the float32 scores [H, W, K] of band_reduce')
    H, W, K = scores.shape
    P = int(P)
    morphology.check_components(P, K)
    attribute.check_std_extent(H, W, stds)
    thresholds, counts = areas + diagonals + stds, (len(areas), len(diagonals), len(stds))
    n = len(thresholds)
    T = max(1, min(int(batch), L - 1))
    with torch.cuda.device(scores.device):
        if not bool(torch.isfinite(scores).all()):
            raise ValueError('band_profile: the scores hold a value that is not finite')
        ws = torch.empty(lib.attr_multi_workspace_bytes(H, W, P, counts[1], counts[2], T), dtype=torch.uint8, device=scores.device)
        q = torch.empty(2 * P, H, W, dtype=torch.uint8, device=scores.device)
        count = torch.empty(2 * P, n, H, W, dtype=torch.uint8, device=scores.device)
        cells = H * W * attribute.band_count(K, P, n)
        both = torch.empty(cells + 2 * P, dtype=torch.float32, device=scores.device)      # the profile, then the P ranges: one copy
        out, rng = both[:cells].view(H, W, -1), both[cells:].view(P, 2)
        lib.attr_quantise(scores, P, L, q, rng, ws)
        lib.attr_multi_run(q, thresholds, counts, L, count, ws, T)
        lib.attr_stack(scores, P, n, L, count, rng, out)
        host = both.cpu().numpy()
        profile, ranges = host[:cells].reshape(H, W, -1), host[cells:].reshape(P, 2)
    return profile, attribute.make_info(K, P, areas, L, ranges, 'device', diagonals, stds)


def band_profile(scores, P, radii, device, kind='morph', areas=None, levels=None, diagonals=(), stds=()):
    """`band_profile: morph` on the device -> (profile [H, W, K + 2 n P] float32 on the host, info).  scores: the
    float32 [H, W, K] scores of band_reduce, a numpy array or a tensor on the device (band_reduce(.., on_device=True): nothing
    travels in between).  dmf_morph_markers, the reconstruction in batches of rounds with one read of the counters per batch,
    dmf_morph_stack, and ONE copy back.  `info` is utils.morphology.make_info's dict: the band order, the route and the rounds of
    each launch batch.  A score that is not finite is refused by name.
    kind='area' (DESIGN.md §27): `areas` and `levels` in the place of `radii` (which is not read); `info` is
    utils.attribute.make_info's dict.  diagonals / stds: further thresholds over the same components; with both
    empty the calls are the ones of §27."""
    if kind == 'area':
        from utils import attribute
        if len(diagonals or ()) or len(stds or ()):
            return _multi_profile(scores, P, attribute.DEFAULT_AREAS if areas is None else areas, diagonals or (), stds or (),
                                  attribute.DEFAULT_LEVELS if levels is None else levels, device)
        return _area_profile(scores, P, attribute.DEFAULT_AREAS if areas is None else areas,
                             attribute.DEFAULT_LEVELS if levels is None else levels, device)
    if kind != 'morph':
        raise ValueError('band_profile: kind %r is not one of morph / area' % (kind,))
    from utils import morphology
    radii = morphology.check_radii(radii)
    device = torch.device(device)
    if isinstance(scores, np.ndarray):
        scores = torch.from_numpy(np.ascontiguousarray(scores, dtype=np.float32)).to(device)
    if not (torch.is_tensor(scores) and scores.dim() == 3 and scores.dtype == torch.float32 and scores.device.type == 'cuda'):
        raise lib.DmfError('band_profile wants the float32 scores [H, W, K] of band_reduce')
    H, W, K = scores.shape
    P, n = int(P), len(radii)
    morphology.check_components(P, K)
    with torch.cuda.device(scores.device):
        if not bool(torch.isfinite(scores).all()):
            raise ValueError('band_profile: the scores hold a value that is not finite')
        ws = torch.empty(lib.morph_workspace_bytes(H, W, P, n), dtype=torch.uint8, device=scores.device)
        mask, X, Y, state = lib.morph_carve(ws, H, W, P, n)
        lib.morph_markers(scores, P, radii, mask, X, Y)
        rounds = lib.morph_reconstruct_run(mask, X, Y, n, state)
        out = torch.empty(H, W, morphology.band_count(K, P, n), dtype=torch.float32, device=scores.device)
        lib.morph_stack(scores, P, n, mask, X, out)
        profile = out.cpu().numpy()
    return profile, morphology.make_info(K, P, radii, 'device', rounds)


class Scene:
    """Padded, normalised scenes resident in HBM: A [Hp, Wp, C], B [HpB, WpB, C2] (pixel-major, fp32).
    half: A is kept as IEEE fp16 (`gmf.half`; numpy's float32 -> float16 rounds to nearest even, as the oracle does)."""

    def __init__(self, primary, aux, device, half=False):
        A = np.ascontiguousarray(primary, dtype=np.float32)
        Bm = np.ascontiguousarray(aux, dtype=np.float32)
        if Bm.ndim == 2:
            Bm = Bm[:, :, None]
        self.half = bool(half)
        self.A = torch.from_numpy(A.astype(np.float16) if half else A).to(device)
        self.B = torch.from_numpy(Bm).to(device)
        self.device = torch.device(device)

    @classmethod
    def from_raw(cls, primary_raw, aux_raw, patch, scale, device, half=False):
        """The scene of `Scene(data_padding(primary_raw, ..), data_padding_aux(aux_raw, ..), device, half)`, bit for bit, with
        the normalisation, the padding (patch - 1 / scale * patch - 1) and the conversions done on the device from the raw
        scenes (`scene_prep: device`).  Falls back to exactly that host call, saying why, where prep_route sends a scene to
        the host."""
        primary_raw, aux_raw = np.asarray(primary_raw), np.asarray(aux_raw)
        if primary_raw.ndim != 3 or aux_raw.ndim not in (2, 3):
            raise lib.DmfError('from_raw wants a primary scene [H, W, C] and an aux scene [SH, SW] or [SH, SW, C2]')
        pads = (patch - 1, scale * patch - 1)
        why = ''
        for raw, pad in zip((primary_raw, aux_raw), pads):
            why = why or prep_route(raw.dtype, raw.shape[0], raw.shape[1], pad)[1]
        if not why:
            self = cls.__new__(cls)
            self.half, self.device = bool(half), torch.device(device)
            tensors = []
            for raw, pad, dt in zip((primary_raw, aux_raw), pads, (torch.float16 if half else torch.float32, torch.float32)):
                t = torch.empty(raw.shape[0] + pad, raw.shape[1] + pad, raw.shape[2] if raw.ndim == 3 else 1, dtype=dt, device=device)
                why = why or _prepare_on_device(raw, pad, t)
                tensors.append(t)
            if not why:
                self.A, self.B = tensors
                return self
        _host_fallback(why)
        from function.function import data_padding, data_padding_aux
        cfg = {'patch_size': patch, 'scale': scale}
        return cls(data_padding(primary_raw, cfg, 'ms'), data_padding_aux(aux_raw, cfg), device, half=half)

    def atlas(self, patch, scale, ops):
        """-> the `AtlasScene` of this scene for patches of `patch` pixels, aux scale `scale` and the variants `ops` (see
        dmf.augment: a name of augment.OPS or a list of 0..7 that starts with 0).  Two dmf_scene_atlas launches, fp32 or fp16
        primary scene alike.  This scene's tensors are RELEASED afterwards (A and B become None): the atlas holds the untouched
        scene in slot 0 and replaces it.  Peak memory is source plus atlas; resident afterwards is len(ops) x the scene, or more
        for a non-square scene with a transposed op, whose slots are squares of the longer side."""
        out = AtlasScene(self, patch, scale, ops)
        self.A = self.B = None
        return out

    def affinity(self, H, W, radius=2, sigma_s=2.0, sigma_r=0.1):
        """-> aff [H, W, n] float32 on the device, n = (2 radius + 1)^2: the bilateral affinities of the H x W scene that sits at
        the top-left corner of the padded primary scene (dmf_spatial_affinity; fp32 and fp16 scenes alike; of a
        scene atlas that corner is slot 0, the untouched scene).  4 n bytes per pixel; the last one is kept with its parameters
        and handed out again for the same ones."""
        key = (int(H), int(W), radius, float(sigma_s), float(sigma_r))
        kept = getattr(self, '_affinity', None)
        if kept is None or kept[0] != key:
            Hp, Wp = getattr(self, 'extent', self.A.shape[:2])
            if not (1 <= key[0] <= Hp and 1 <= key[1] <= Wp):
                raise lib.DmfError('affinity: %d x %d pixels asked of a padded scene of %d x %d' % (key[0], key[1], Hp, Wp))
            self._affinity = None                        # (the old one goes before the new one is allocated)
            aff = torch.empty(key[0], key[1], lib._window(radius), dtype=torch.float32, device=self.device)
            with torch.cuda.device(self.device):
                lib.spatial_affinity(self.A, key[0], key[1], radius, sigma_s, sigma_r, aff)
            self._affinity = kept = (key, aff)
        return kept[1]

    def segments(self, H, W, size=8, compactness=0.1, iterations=10):
        """-> (seg [H, W] int32, centres [Kc, C + 2] float32, counts [Kc] int32) on the device: the SLIC superpixels of the H x W
        scene that sits at the top-left corner of the padded primary scene (fp32 and fp16 scenes alike; of a scene
        atlas that corner is slot 0).  dmf_slic_init, `iterations` x (dmf_slic_assign, dmf_slic_update), a last dmf_slic_assign,
        all enqueued without a host synchronisation; the last result is kept with its parameters and handed out again.
        Memory: besides seg (4 bytes per pixel) and the centres, the update's workspace of 9 (4 C + 16) bytes per CELL is held
        while the iterations run and released afterwards: 33.6 MB at 512 x 512 x 224 with size 8, but 6.5 GB for a 50 M-pixel
        scene of 224 bands at size 8, and four times that at size 4 — choose the size of a large scene with that in mind."""
        if isinstance(iterations, bool) or not isinstance(iterations, int) or iterations < 0:
            raise lib.DmfError('segments: iterations = %r is not a whole number >= 0' % (iterations,))
        key = (int(H), int(W), size, float(compactness), iterations)
        kept = getattr(self, '_segments', None)
        if kept is None or kept[0] != key:
            Hp, Wp = getattr(self, 'extent', self.A.shape[:2])
            if not (1 <= key[0] <= Hp and 1 <= key[1] <= Wp):
                raise lib.DmfError('segments: %d x %d pixels asked of a padded scene of %d x %d' % (key[0], key[1], Hp, Wp))
            gh, gw = lib.segment_grid(key[0], key[1], size)
            self._segments = None                        # (the old one goes before the new one is allocated)
            dev, Cn = self.device, self.A.shape[2]
            seg = torch.empty(key[0], key[1], dtype=torch.int32, device=dev)
            centres = torch.empty(gh * gw, Cn + 2, dtype=torch.float32, device=dev)
            counts = torch.zeros(gh * gw, dtype=torch.int32, device=dev)
            with torch.cuda.device(dev):
                ws = torch.empty(lib.slic_workspace_bytes(key[0], key[1], Cn, size), dtype=torch.uint8, device=dev)
                lib.slic_init(self.A, key[0], key[1], size, centres)
                for _ in range(iterations):
                    lib.slic_assign(self.A, key[0], key[1], size, compactness, centres, seg)
                    lib.slic_update(self.A, key[0], key[1], size, seg, centres, counts, ws)
                lib.slic_assign(self.A, key[0], key[1], size, compactness, centres, seg)
            self._segments = kept = (key, (seg, centres, counts))
        return kept[1]

    def segment_regions(self, seg, H, W, n_labels=0, min_size=1, merge='position'):
        """-> (region [H, W] int32 on the device, R, region sizes [R] int32 on the device, stats): the connected regions of the
        label image seg [H, W] int32 (`segments`' image with n_labels = Kc, or any segmentation with n_labels = 0).
        dmf_label_components, then dmf_region_merge: a component smaller than `min_size` that is not the main component of a
        label in 0..n_labels - 1 joins the component before it.  stats = dict(regions, components, absorbed).  One host read (the
        four statistics) at the end; the workspace of about 16 bytes per pixel is released on return.
        merge = 'spectrum' (DESIGN.md §25): dmf_region_graph_count and dmf_region_graph_merge in dmf_region_merge's place.  A
        fragment joins the adjacent group with the nearest mean spectrum of the H x W scene at the top-left corner of the padded
        primary scene, groups of fragments grow, and one that reaches `min_size` becomes a region; stats gains `rounds`.  Two host
        reads: the two counts that size the workspace (about 24 bytes per pixel and 32 + 16 C bytes per component) and the statistics."""
        if merge not in ('position', 'spectrum'):
            raise lib.DmfError('segment_regions: merge = %r is not position or spectrum' % (merge,))
        H, W = int(H), int(W)
        if not (torch.is_tensor(seg) and seg.is_cuda and seg.dtype == torch.int32 and tuple(seg.shape) == (H, W)):
            raise lib.DmfError('segment_regions: seg must be an int32 GPU tensor [%d, %d]' % (H, W))
        seg = seg.contiguous()
        dev = seg.device
        comp, region = torch.empty_like(seg), torch.empty_like(seg)
        sizes = torch.empty(H * W, dtype=torch.int32, device=dev)
        stats = torch.empty(4, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            ws = torch.empty(lib.region_workspace_bytes(H, W, n_labels), dtype=torch.uint8, device=dev)
            lib.label_components(seg, comp, ws)
            if merge == 'spectrum':
                Hp, Wp = getattr(self, 'extent', self.A.shape[:2])
                if not (H <= Hp and W <= Wp) or self.A.device != dev:
                    raise lib.DmfError('segment_regions: %d x %d pixels asked of a padded scene of %d x %d on %s' % (H, W, Hp, Wp, self.A.device))
                counts = torch.empty(2, dtype=torch.int32, device=dev)
                ws = torch.empty(lib.region_graph_workspace_bytes(H, W, 1, n_labels, 1), dtype=torch.uint8, device=dev)
                lib.region_graph_count(seg, comp, n_labels, min_size, counts, ws)
                components, fragments = counts.tolist()
                ws = None                                # (the old one goes before the new one is allocated)
                ws = torch.empty(lib.region_graph_workspace_bytes(H, W, self.A.shape[2], n_labels, components), dtype=torch.uint8, device=dev)
                lib.region_graph_merge(seg, comp, self.A, n_labels, min_size, components, fragments, region, sizes, stats, ws)
            else:
                lib.region_merge(seg, comp, n_labels, min_size, region, sizes, stats, ws)
            R, components, absorbed, rounds = stats.tolist()
        out = dict(regions=R, components=components, absorbed=absorbed)
        if merge == 'spectrum':
            out['rounds'] = rounds
        return region, R, sizes[:R].clone(), out


class AtlasScene(Scene):
    """A `Scene` whose A and B are scene atlases: the variants `ops` of the padded scenes, stacked along the row
    axis, slot s = variant ops[s], slot 0 the untouched scene at the origin.  Every engine takes it as it takes a Scene:
    coordinates that are not mapped keep their meaning, and a patch of variant ops[s] is the ordinary patch at `map_xy(xy, s)`.
      A [V * R, Wq, C], B [V * S * R, S * Wq, C2];  ops, slot_rows = R, extent = (Hp, Wp), patch, scale."""

    def __init__(self, scene, patch, scale, ops):
        from . import augment
        self.ops = augment.ops_of(ops, 'atlas')
        self.patch, self.scale = int(patch), int(scale)
        self.half, self.device = scene.half, scene.device
        Hp, Wp = scene.A.shape[:2]
        S = self.scale
        if Hp < self.patch or Wp < self.patch or scene.B.shape[0] < S * Hp or scene.B.shape[1] < S * Wp:
            raise lib.DmfError('atlas: the aux scene %s does not hold %d x the primary scene %s, or the patch %d does not fit'
                               % (tuple(scene.B.shape), S, tuple(scene.A.shape), self.patch))
        self.extent = (Hp, Wp)
        R, Wq = augment.atlas_geometry(Hp, Wp, self.ops)
        self.slot_rows = R
        self._affine = {}                                # (slot, device) -> the constants of map_xy's one-slot form
        V = len(self.ops)
        self.A = torch.empty(V * R, Wq, scene.A.shape[2], dtype=scene.A.dtype, device=self.device)
        self.B = torch.empty(V * S * R, S * Wq, scene.B.shape[2], dtype=scene.B.dtype, device=self.device)
        with torch.cuda.device(self.device):
            lib.scene_atlas(scene.A, Hp, Wp, self.ops, R, self.A)
            lib.scene_atlas(scene.B, S * Hp, S * Wp, self.ops, S * R, self.B)       # (the last S - 1 rows / columns: read by no patch)

    def slot_of(self, op):
        """The slot that holds variant `op`."""
        if op not in self.ops:
            raise lib.DmfError('the atlas holds the variants %s, not %d' % (list(self.ops), op))
        return self.ops.index(op)

    def map_xy(self, xy, slot):
        """Atlas coordinates of the patches at xy [n, 2] (host numpy, or a device int32 tensor), each taken from `slot` (an array
        [n] or a scalar): dmf.augment.map_xy with this atlas' geometry."""
        from . import augment
        if torch.is_tensor(xy) and xy.is_cuda and isinstance(slot, int):
            # one slot for a whole device batch (test-time augmentation): the map is (x, y) or (y, x) times a sign plus an
            # offset, two small launches with the slot's constants kept on the device
            if slot == 0:
                return xy                                # the untouched scene at the origin
            key = (slot, xy.device)
            if key not in self._affine:
                k, (h, w), n = self.ops[slot], self.extent, self.patch
                if k & 4:
                    h, w = w, h
                sign = [-1 if k & 2 else 1, -1 if k & 1 else 1]
                off = [(h - n if k & 2 else 0) + slot * self.slot_rows, w - n if k & 1 else 0]
                self._affine[key] = (bool(k & 4), torch.tensor(sign, dtype=torch.int32, device=xy.device),
                                     torch.tensor(off, dtype=torch.int32, device=xy.device))
            swap, sign, off = self._affine[key]
            return (xy.flip(1) if swap else xy) * sign + off
        return augment.map_xy(xy, slot, self.ops, self.extent, self.patch, self.slot_rows)


class LossScaler:
    """Device-resident dynamic loss scale — the role of `torch.cuda.amp.GradScaler` (tostagesolver.py:83-84 builds two
    with torch's defaults; :98 / :119 scale -> step -> update).  Same defaults and update rule; the state never visits
    the host, so a captured graph carries it."""

    def __init__(self, device, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
        self.growth_factor, self.backoff_factor, self.growth_interval = float(growth_factor), float(backoff_factor), int(growth_interval)
        self.state = torch.zeros(lib.SCALER_FLOATS, device=device)
        lib.scaler_init(self.state, float(init_scale))

    def get_scale(self):
        return float(self.state[0].item())

    def skipped_steps(self):
        return int(self.state[3].item())

    def hparams(self):
        return (self.growth_factor, self.backoff_factor, self.growth_interval)


class Criterion:
    """A classification criterion beyond the plain cross-entropy fused into the patch kernel, as dmf_ce_loss takes it
    (DESIGN.md §12).  spec: dict(kind, label_smoothing, gamma, class_weights) —
      kind           'ce' (0): nn.CrossEntropyLoss(weight=class_weights, label_smoothing=label_smoothing);
                     'focal' (1): w[y] (1 - p_y)^gamma (-log p_y), mean over the batch by the same denominator sum_j w[y_j]
      class_weights  K floats, every one finite and > 0 (the denominator of every batch is then > 0), or None = all ones.
    A missing key is its neutral value."""

    def __init__(self, spec, K, device):
        kind = spec.get('kind', 'ce')
        kind = {0: 'ce', 1: 'focal'}.get(kind, kind)
        eps, gamma = float(spec.get('label_smoothing') or 0.0), float(spec.get('gamma') or 0.0)
        if kind not in lib.CE_KINDS:
            raise lib.DmfError('criterion kind %r is not one of %s' % (kind, sorted(lib.CE_KINDS)))
        if not 0.0 <= eps < 1.0:
            raise lib.DmfError('label_smoothing %r is not in [0, 1)' % eps)
        if not (gamma == 0.0 or (gamma >= 1.0 and np.isfinite(gamma))):
            raise lib.DmfError('focal gamma %r is neither 0 nor >= 1' % gamma)
        if (kind == 'ce' and gamma != 0.0) or (kind == 'focal' and eps != 0.0):
            raise lib.DmfError('label smoothing belongs to kind ce, gamma to kind focal: got kind %s, label_smoothing %g, gamma %g'
                               % (kind, eps, gamma))
        self.kind, self.label_smoothing, self.gamma = kind, eps, gamma
        self.params = lib.ce_params(kind, eps, gamma)
        self.class_w = None
        w = spec.get('class_weights')
        if w is not None:
            w = np.asarray(w, dtype=np.float32).reshape(-1)
            if w.size != K:
                raise lib.DmfError('class_weights holds %d weights for %d classes' % (w.size, K))
            if not (np.isfinite(w).all() and (w > 0).all()):
                raise lib.DmfError('class_weights must be finite and > 0 (as float32), got %s' % w.tolist())
            self.class_w = torch.from_numpy(w.copy()).to(device)


class _PlanEngine:
    """What both train engines share: parameters and optimiser state, the epoch plan on the device, and the hipGraph that
    replays steps of it.  A subclass says how one step is launched (`_plan_launch`) and what differs around a capture.
    Two kinds of step:
      * the fused step (TrainEngine without a criterion), cross-entropy inside the patch kernel: `step` / `load_plan` take
        PER-RANK batches (every rank is handed its own pixels), a captured graph reads a fixed window refilled before each
        replay, and the library's own launch loop may run the plan;
      * the unit-gradient step (TrainEngine with a criterion, QuaTrainEngine), `_unit_step` around a loss kernel that sees
        the whole batch: `step` / `load_plan` take GLOBAL batches, the same on every rank, of which rank r trains on its
        contiguous rows (`_rank_shard`, `_load_global_plan`), and a captured graph's steps read plan[cursor]."""

    def __init__(self, net, scene, lr, betas, eps, process_group, scaler, optimizer, momentum, alpha, weight_decay=0.0,
                 clip_grad_norm=None):
        if optimizer not in ('ADAM', 'ADAMW', 'SGD', 'RMSprop'):
            raise lib.DmfError('optimizer %r is not one of ADAM, ADAMW, SGD, RMSprop' % (optimizer,))
        if scaler is not None and optimizer not in ('ADAM', 'ADAMW'):
            raise lib.DmfError('%s with a loss scaler: the loss-scaler step is ADAM or ADAMW' % optimizer)
        self.optim, self.momentum, self.alpha = optimizer, float(momentum), float(alpha)
        # weight decay (L2; decoupled with ADAMW) and gradient-norm clipping: the one-launch step dmf_optim_step
        self.weight_decay, self.clip_grad_norm = float(weight_decay or 0.0), float(clip_grad_norm or 0.0)
        if not (np.isfinite(self.weight_decay) and self.weight_decay >= 0.0):
            raise lib.DmfError('weight_decay %r is not a finite number >= 0' % (weight_decay,))
        if not (np.isfinite(self.clip_grad_norm) and self.clip_grad_norm >= 0.0):
            raise lib.DmfError('clip_grad_norm %r is not a finite number >= 0 (None or 0: off)' % (clip_grad_norm,))
        self.lr, self.b1, self.b2, self.eps = float(lr), float(betas[0]), float(betas[1]), float(eps)
        self.net, self.scene, self.scaler = net, scene, scaler
        self.shape = net.shape
        lib.shape_supported(self.shape)
        if getattr(scene, 'half', False):
            lib.require_half(self.shape)
        self.pg, self.world, self.rank = process_group, 1, 0
        if process_group is not None:
            import torch.distributed as dist
            self.world, self.rank = dist.get_world_size(process_group), dist.get_rank(process_group)
        dev = scene.device
        self.theta = net.flat_parameters()
        self.m = torch.zeros_like(self.theta)
        self.v = torch.zeros_like(self.theta)
        self.grad = torch.zeros_like(self.theta)
        # device-side bookkeeping for graph replay
        self.dev_step = torch.zeros(1, dtype=torch.int32, device=dev)
        self.dev_cursor = torch.zeros(1, dtype=torch.int32, device=dev)
        self.step_count = self.host_cursor = self.plan_steps = 0
        self.plan_xy = self.plan_labels = self.loss_hist = None
        self.norm_hist = None            # pre-clip gradient norms of the plan's steps (clip_grad_norm), sized like loss_hist
        self.norm = torch.zeros(1, device=dev)       # ... and of the last eager step
        self.graph, self.graph_steps, self.graph_hparams = None, 0, None
        self.comm = None                 # the one-shot xgmi exchange (TrainEngine only)
        self._rccl_graph = True          # False once RCCL refused to be captured (run_plan), or set by a caller
        self._force_collective = False   # tests only: see _single()
        # the device-resident schedule (set_schedule): the HpSchedule the *_sched entry points take, its table and row index
        self.sched = self.hp_table = self.hp_row = self.hp_unit = None
        # the averaged copy of the weights (set_averaging): the vector, the WeightAvg the *_avg entry points take, (kind, decay, start)
        self.avg = self.wavg = self.avg_spec = None

    # ------------------------------------------------------------------ lr, betas and momentum from a table on the device
    def set_schedule(self, table, unit='epoch'):
        """Take lr, beta1, beta2 and momentum of every step from a table on the device instead of the launch arguments
        (DESIGN.md §15): every step form — the fused step, the native loop, the scaler, SGD and RMSprop forms, the regularised
        step, the unit-gradient step, `step_short` and plain eager `step` — then updates by the `_sched` entry points, and a
        captured graph or the native loop follows a scheduler without a re-capture (`_hparams`).
        table: host float32 [rows, 4], a row = (lr, beta1, beta2, momentum); checked here: finite, lr >= 0, betas and momentum
        in [0, 1).  unit 'epoch': the row is the device int that `set_epoch(e)` fills; unit 'step': the row is the 1-based count
        of optimiser steps taken - 1 (a step the loss scaler skips does not count).  Rows past the table's end read its last row.
        The step count then lives on the device for every optimiser (`_counts_on_device`).  eps, alpha, weight_decay and
        clip_grad_norm stay the engine's attributes.  `self.lr`, `self.b1`, `self.b2` and `self.momentum` are no longer read by
        a step; the solvers keep them at the current row for the checkpoint.
        Data parallel: the one-shot xGMI launch has no schedule form, so an engine that was given a communicator lets go of it
        and takes the collective route (dmf_grad_reduce -> all-reduce -> dmf_optim_step_sched), as the regularised step does."""
        if unit not in ('epoch', 'step'):
            raise lib.DmfError('schedule unit %r is neither epoch nor step' % (unit,))
        t = np.ascontiguousarray(np.asarray(table, dtype=np.float32))
        if t.ndim != 2 or t.shape[1] != 4 or t.shape[0] < 1:
            raise lib.DmfError('a schedule table is [rows >= 1, 4] (lr, beta1, beta2, momentum), got shape %s' % (t.shape,))
        if not np.isfinite(t).all():
            raise lib.DmfError('schedule table: non-finite value in row %d' % int(np.argwhere(~np.isfinite(t))[0][0]))
        if (t[:, 0] < 0).any():
            raise lib.DmfError('schedule table: negative lr in row %d' % int(np.argwhere(t[:, 0] < 0)[0][0]))
        bad = (t[:, 1:] < 0) | (t[:, 1:] >= 1)
        if bad.any():
            raise lib.DmfError('schedule table: beta1, beta2 and momentum must lie in [0, 1) (row %d)' % int(np.argwhere(bad)[0][0]))
        dev = self.scene.device
        self._device_counts_from_here()
        self.hp_table = torch.from_numpy(t.copy()).to(dev)
        self.hp_row = torch.zeros(1, dtype=torch.int32, device=dev) if unit == 'epoch' else None
        self.hp_unit = unit
        self.sched = lib.hp_schedule(self.hp_table, self.hp_row)
        self.comm = None

    # ------------------------------------------------------------------ an averaged copy of the weights, kept by the update
    def set_averaging(self, kind, decay=0.999, start_step=1):
        """Keep `self.avg`, torch's `AveragedModel` of the weights, updated by every optimiser step: kind 'ema'
        (`get_ema_multi_avg_fn(decay)`) or 'mean' (the default equal average, `decay` unused); start_step >= 1 is the first
        averaged optimiser step (AveragedModel's first `update_parameters`), until which avg is a copy of theta.  avg starts
        as a copy of theta.  Every step form then updates by the `_avg` entry points (`_update`): the fused ADAM step and the
        native loop inside the reduce + ADAM launch, every other optimiser launch inside dmf_optim_step_avg; the reduce launch in
        front of it is the one it was, so gradients and recorded losses keep their bits.  The xGMI exchange keeps its launch and
        is followed by dmf_weight_average.  The step count then lives on the device for every optimiser (`_counts_on_device`): a
        step the loss scaler skips does not count.  Averaging is local to a rank."""
        if kind not in lib.AVG_KINDS:
            raise lib.DmfError('averaging kind %r is not one of %s' % (kind, sorted(lib.AVG_KINDS)))
        decay, start_step = float(decay), int(start_step)
        if kind == 'ema' and not 0.0 <= decay < 1.0:
            raise lib.DmfError('averaging decay %r is not in [0, 1)' % (decay,))
        if start_step < 1:
            raise lib.DmfError('averaging start_step %d: the first averaged step is at least 1' % start_step)
        self._device_counts_from_here()
        self.avg = self.theta.clone()
        self.avg_spec = (kind, decay, start_step)
        self.wavg = lib.weight_avg(self.avg, kind, decay, start_step)

    def _device_counts_from_here(self):
        """set_schedule, set_averaging (their checks passed): from here on the device counts the steps, so it is handed the host's
        count where it did not count yet; and the steps take other entry points, so a captured graph is dropped."""
        self._seed_dev_step()
        self.graph = None

    def averaged_parameters(self):
        """The averaged flat vector (None without set_averaging): a live device tensor, valid weights at every moment."""
        return self.avg

    def set_epoch(self, e):
        """Unit 'epoch': the steps from here on read row e of the table (a stream-ordered device fill, no synchronisation; never
        called inside a capture).  Unit 'step', or no schedule: nothing to do."""
        if self.hp_row is not None:
            self.hp_row.fill_(int(e))

    def _hparams(self):
        """What a captured graph bakes in as launch arguments.  With a schedule lr, the betas and momentum are not among them:
        the graph survives every change of them."""
        own = ('sched', self.eps) if self.sched is not None else (self.lr, self.b1, self.b2, self.eps, self.momentum)
        # averaging: kind, the float32 weight and the first averaged step are launch arguments
        avg = ('avg', self.wavg.kind, self.wavg.weight, self.wavg.start) if self.wavg is not None else ()
        return own + (self.alpha, self.weight_decay, self.clip_grad_norm) + (
            self.scaler.hparams() if self.scaler is not None else ()) + avg

    def _regularised(self):
        """Weight decay, AdamW or gradient-norm clipping is active: every step form updates by dmf_optim_step (`_update`), so no
        fused reduce + ADAM launch, no native launch loop and no xgmi exchange.  ADAMW with weight_decay 0 is ADAM's
        arithmetic, but still this route: only dmf_optim_step knows the kind."""
        return self.weight_decay != 0.0 or self.clip_grad_norm != 0.0 or self.optim == 'ADAMW'

    def _check_labels(self, lab):                    # lab on the host, or on the device: its two extremes are then read back
        K = self.net.arch['K']
        if lab.numel() and (int(lab.min()) < 0 or int(lab.max()) >= K):
            raise lib.DmfError('label outside [0, %d)' % K)

    # ------------------------------------------------------------------ the optimiser update of one step
    def _counts_on_device(self):
        """Is the device step counter the true step count?  Then eager steps advance it too, and load_plan leaves it alone;
        otherwise eager steps use the host count `step_count` and load_plan copies it into the counter.  With a loss
        scaler it is: a skipped step takes its count back on the device.  With a schedule it is: unit 'step' finds its row
        by it.  With averaging it is: the rule reads it."""
        return self.scaler is not None or self.sched is not None or self.wavg is not None

    def _count_step(self, dev_step):
        """Count one step on the host; returns the device step counter the step's launches take (None: the host count).
        A plan step gives it; an eager step (dev_step None) takes it where `_counts_on_device()`."""
        self.step_count += 1
        return self.dev_step if dev_step is None and self._counts_on_device() else dev_step

    def _fused_adam(self):
        """ADAM, no scaler, nothing regularised: the step whose reduce launch applies ADAM itself (`_update`).  Only this step
        runs from the library's launch loop (`_native_loop_ok`) and, over RCCL, from a captured graph (`_graphable`)."""
        return self.scaler is None and self.optim == 'ADAM' and not self._regularised()

    def _in_form(self, entry, args, hp, keys):
        """THE choice between the plain, `_sched` and `_avg` form of lib's `entry` (grad_reduce_adam, optim_step,
        train_plan_steps), called with the leading `args` and the keywords `keys`: set_averaging asks for `_avg`, which takes the
        schedule too if there is one; set_schedule alone for `_sched`, which takes no `hp` (lr, b1, b2 and with optim_step momentum,
        by name: its row of the table holds them)."""
        if self.wavg is not None:
            return getattr(lib, entry + '_avg')(*args, avg=self.wavg, sched=self.sched, **hp, **keys)
        if self.sched is not None:
            return getattr(lib, entry + '_sched')(*args, sched=self.sched, **keys)
        return getattr(lib, entry)(*args, **hp, **keys)

    def _update(self, rows, dev_step, cursor, sum_scale, loss=None, loss_hist=None):
        """The launches after the backward, from the slab rows of `rows` patches in self.ws.  The reduce route, first match:
          `_fused_adam()`, one GPU        dmf_grad_reduce_adam in the engine's form (`_in_form`): reduce + ADAM in one launch;
                                          with a schedule lr and the betas go as 0.0
          `_fused_adam()`, xGMI comm      dmf_grad_reduce_xgmi_adam (the ranks' rank-ordered sum inside that launch), followed
                                          by dmf_weight_average with averaging (a schedule has let go of the communicator)
          scaler, one GPU, nothing        dmf_grad_reduce_scaled (reduce, unscale, check) -> the optimiser launch with no
          regularised                     cursor, grad_scale 1, unscaled = 1: GradScaler's unscale_, step and update
                                          (tostagesolver.py:98,119)
          everything else                 dmf_grad_reduce -> all-reduce(sum) where the step has a collective -> the mean loss
                                          into loss_hist[cursor] -> the optimiser launch with cursor and sum_scale (a scaler's
                                          check sees the SUM, so every rank takes the same skip decision); regularised, it
                                          writes the pre-clip norm into norm_hist[cursor], or into self.norm for an eager step
        The optimiser launch on self.grad (`_optimiser_launch`):
          weight decay, ADAMW, clipping,  `_optim_step`: dmf_optim_step in the engine's form — unscale and check with a scaler,
          a schedule or averaging         the norm of the whole gradient and its clipping, weight decay, the optimiser, the
                                          scaler's update, the averaged copy: one launch
          none of them                    dmf_unscale_adam (scaler) / dmf_sgd_step / dmf_rmsprop_step / dmf_adam_step
        The reduce launch does not depend on the schedule or the averaging: gradients and recorded losses keep their bits.
        sum_scale scales the all-reduced gradient: 1/world where the loss is a per-rank mean, 1 where the loss kernel
        already divided by the global batch.  dev_step: the device step counter, or None for the host count.  loss /
        loss_hist: where the step's mean loss (this rank's) is recorded; None where the loss kernel records it itself.
        SGD and RMSprop keep their one state vector in m (momentum buffer / running mean of squares)."""
        sc, fused = self.scaler, self._fused_adam()
        if fused and self._single():
            lr, b1, b2 = (0.0, 0.0, 0.0) if self.sched is not None else (self.lr, self.b1, self.b2)
            self._in_form('grad_reduce_adam', (self.shape, rows, self.ws, self.theta, self.m, self.v, None), dict(lr=lr, b1=b1, b2=b2),
                          dict(eps=self.eps, step=self.step_count, adam_step_dev=dev_step, cursor_dev=cursor, loss=loss,
                               loss_hist=loss_hist))
        elif fused and self.comm is not None:
            lib.grad_reduce_xgmi_adam(self.shape, rows, self.ws, self.theta, self.m, self.v, self.comm.c, self.lr, self.b1, self.b2,
                                      self.eps, sum_scale, dev_step, cursor_dev=cursor, loss=loss, loss_hist=loss_hist)
            if self.wavg is not None:
                lib.weight_average(self.wavg, self.theta, self.step_count, step_dev=dev_step)
        elif sc is not None and self._single() and not self._regularised():
            lib.grad_reduce_scaled(self.shape, rows, self.ws, self.grad, sc.state, cursor_dev=cursor, loss=loss,
                                   loss_hist=loss_hist)
            self._optimiser_launch(dev_step, None, 1.0, unscaled=True)
        else:
            lib.grad_reduce(self.shape, rows, self.ws, self.grad)
            if not self._single():
                self._all_reduce_grad()
            if loss_hist is not None:
                loss_hist.scatter_(0, cursor.long(), loss[:rows].mean().reshape(1))
            norm_hist = None if not self._regularised() else self.norm_hist if cursor is not None else self.norm
            self._optimiser_launch(dev_step, cursor, sum_scale, norm_hist=norm_hist)

    def _optimiser_launch(self, dev_step, cursor, sum_scale, unscaled=False, norm_hist=None):
        """The optimiser launch on self.grad (`_update`: which one)."""
        sc, hp = self.scaler, (self.lr, self.b1, self.b2, self.eps)
        if self._regularised() or self.sched is not None or self.wavg is not None:
            self._optim_step(dev_step, cursor, sum_scale, unscaled=unscaled, norm_hist=norm_hist)
        elif sc is not None:
            lib.unscale_adam(self.theta, self.grad, self.m, self.v, *hp, sc.state, *sc.hparams(), dev_step, grad_scale=sum_scale,
                             cursor_dev=cursor, unscaled=unscaled)
        elif self.optim == 'SGD':
            lib.sgd_step(self.theta, self.grad, self.m, self.lr, self.momentum, self.step_count, grad_scale=sum_scale,
                         step_dev=dev_step, cursor_dev=cursor)
        elif self.optim == 'RMSprop':
            lib.rmsprop_step(self.theta, self.grad, self.m, self.lr, self.alpha, grad_scale=sum_scale, cursor_dev=cursor)
        else:
            lib.adam_step(self.theta, self.grad, self.m, self.v, *hp, self.step_count, grad_scale=sum_scale,
                          adam_step_dev=dev_step, cursor_dev=cursor)

    def _optim_step(self, dev_step, cursor, sum_scale, unscaled=False, norm_hist=None):
        """dmf_optim_step on self.grad with the engine's optimiser, keys and scaler, in the engine's form (`_in_form`)."""
        sc = self.scaler
        keys = dict(eps=1e-8 if self.optim == 'RMSprop' else self.eps, alpha=self.alpha, weight_decay=self.weight_decay,
                    max_norm=self.clip_grad_norm, step=self.step_count, grad_scale=sum_scale, step_dev=dev_step, cursor_dev=cursor,
                    scaler_state=sc.state if sc is not None else None, scaler_hparams=sc.hparams() if sc is not None else None,
                    unscaled=unscaled, norm_hist=norm_hist)
        self._in_form('optim_step', (self.optim, self.theta, self.grad, self.m, self.v),
                      dict(lr=self.lr, b1=self.b1, b2=self.b2, momentum=self.momentum), keys)

    # ------------------------------------------------------------------ the unit-gradient step on global batches
    def _unit_step(self, inp, rows, loss_launch, dev_step, cursor, loss=None, loss_hist=None):
        """dmf_forward_unit (forward of the `rows` patches + the conv backward for a unit gradient per pooled feature) ->
        `loss_launch()` (self.logits -> value and self.dlogits) -> dmf_backward_unit (dh, dz, scaled slab rows) -> the update:
        the patches are visited ONCE.  The loss kernel has divided by the GLOBAL batch: the ranks' sum is the gradient."""
        lib.forward_unit(self.shape, inp, self.theta, self.net.pool_w, self.logits, self.ws, adam_step_dev=dev_step)
        loss_launch()
        lib.backward_unit(self.shape, rows, self.theta, self.dlogits, self.ws)
        self._update(rows, dev_step, cursor, 1.0, loss, loss_hist)

    def _rank_shard(self, xy, labels, cap):
        """Of a global eager batch (host or device): this rank's len // world rows of `xy` and, on the device, the labels of
        all ranks' rows.  The remainder that the world size does not divide is dropped."""
        xy = torch.as_tensor(xy)
        n = xy.shape[0] // self.world
        if n > cap:
            raise lib.DmfError('engine was built for batches of at most %d, got %d' % (cap, n))
        if n == 0:
            raise lib.DmfError('a batch of %d pixels gives the %d ranks no pixel each' % (xy.shape[0], self.world))
        lab = torch.as_tensor(labels)[:self.world * n].to(device=self.scene.device, dtype=torch.int32)
        return xy[self.rank * n:(self.rank + 1) * n].contiguous(), lab.contiguous()

    def _load_global_plan(self, xy_all, labels_all, per_rank, rows=None):
        """An epoch of full GLOBAL batches: xy_all [n*per_rank*world, 2], labels_all [n*per_rank*world] (host or device, any
        int type).  Rank r keeps rows [r*per_rank, (r+1)*per_rank) of every batch's pixels, as the plan coordinates
        `rows(pixels)` where the step does not gather at the pixels themselves, and the labels of the whole batches."""
        def mine(xy, n):
            if self.world > 1:
                xy = xy.view(n, self.world, per_rank, 2)[:, self.rank].reshape(-1, 2)
            return xy if rows is None else rows(xy)
        return self._upload_plan(xy_all, labels_all, per_rank * self.world, mine=mine)

    # ------------------------------------------------------------------ epoch plan + hipGraph replay
    def _upload_plan(self, xy_all, labels_all, rows, capacity=None, pack=False, mine=None):
        """THE plan upload (load_plan, _load_global_plan, load_block): xy_all [n*rows, 2], labels_all [n*rows] (host or device,
        any int type) become the loaded plan of n steps; returns n.  Bounds and labels are checked on a host copy: the caller's
        own arrays, or ONE device-to-host copy of its device tensors, which then are the plan without another upload.
        capacity (steps): the plan tensors are sized for it, padded with pixel (0, 0) and label 0, which are never stepped on.
        pack: also `plan_pack`, the stream step by step [2*rows coordinates | rows labels]: the window of a captured graph is
        refilled from it with ONE device copy per replay.  mine(xy, steps): a global plan's host pixels -> this rank's rows."""
        dev = self.scene.device
        xy, lab = torch.as_tensor(xy_all).to(torch.int32), torch.as_tensor(labels_all).to(torch.int32)
        if xy.shape[0] % rows or xy.shape[0] != lab.shape[0]:
            raise lib.DmfError('plan length must be a multiple of the %sbatch size' % ('' if mine is None else '(global) '))
        n = xy.shape[0] // rows
        cap = max(int(capacity or n), n)
        xy_h, lab_h = xy.cpu(), lab.cpu()
        if cap > n:
            xy = xy_h = torch.cat([xy_h, torch.zeros((cap - n) * rows, 2, dtype=torch.int32)])
            lab = lab_h = torch.cat([lab_h, torch.zeros((cap - n) * rows, dtype=torch.int32)])
        if mine is not None:
            xy = xy_h = mine(xy_h, cap)
        lib.check_xy_bounds(self.shape, self.scene.A, self.scene.B, xy_h.numpy())
        self._check_labels(lab_h)
        plan = dict(plan_xy=xy.to(dev).contiguous(), plan_labels=lab.to(dev).contiguous())
        if pack:
            plan['plan_pack'] = torch.cat([plan['plan_xy'].view(cap, 2 * rows), plan['plan_labels'].view(cap, rows)], 1).contiguous()
        plan.update(self._plan_extras(plan['plan_labels'], rows, cap))
        self._install_plan(n, cap, **plan)
        return n

    def _plan_extras(self, labels, rows, cap):
        """Further plan tensors (attribute name -> tensor) derived from the uploaded labels [cap * rows]; they are installed
        with the plan, so a plan of the same shape is copied into the tensors a captured graph reads."""
        return {}

    def _install_plan(self, n, capacity, **plan):
        """Make `plan` (attribute name -> device tensor, `capacity` steps long) the loaded plan of n steps and rewind to its first
        step.  A plan of the same shape is copied into the tensors already there: a captured graph keeps reading valid addresses."""
        if self.plan_xy is not None and self.plan_xy.shape == plan['plan_xy'].shape:
            for name, t in plan.items():
                getattr(self, name).copy_(t)
        else:
            for name, t in plan.items():
                setattr(self, name, t)
            self.loss_hist = torch.empty(max(capacity, 1), device=self.scene.device)
            self.norm_hist = torch.empty_like(self.loss_hist)
            self.graph = None
        self.loss_hist.zero_()
        self.norm_hist.zero_()
        self.dev_cursor.zero_()
        self.host_cursor, self.plan_steps = 0, n
        self._seed_dev_step()

    def _seed_dev_step(self):
        """Plan steps read the device step counter: where eager steps count on the host, that count goes into it."""
        if not self._counts_on_device():
            self.dev_step.fill_(self.step_count)

    def _plan_step(self):
        if self.host_cursor >= self.plan_steps:          # the kernel reads plan[cursor] unchecked: never step past the plan
            raise lib.DmfError('the loaded plan has %d steps, all of them are done' % self.plan_steps)
        self._plan_launch()
        self.host_cursor += 1

    def _steps_to_run(self, steps):
        steps = self.plan_steps - self.host_cursor if steps is None else steps
        if self.plan_xy is None or steps < 0 or self.host_cursor + steps > self.plan_steps:
            raise lib.DmfError('run_plan(%d): the loaded plan has %d steps, %d of them done' % (
                steps, self.plan_steps, self.host_cursor))
        return steps

    def run_plan(self, steps=None, steps_per_graph=0):
        """Run `steps` steps of the loaded plan (default: all).  steps_per_graph > 0 replays a captured hipGraph of that
        many steps while whole graphs fit (where `_graphable()`), the rest is launched eagerly.  No host synchronisation."""
        steps = self._steps_to_run(steps)
        done = 0
        if steps_per_graph > 0 and self._graphable():
            # lr, betas and eps are launch arguments baked into the captured graph (reference: `scheduler.step()` changes
            # the optimiser's lr every epoch, mainsolver.py:60): a change invalidates the graph — unless a schedule on the
            # device holds them (set_schedule)
            if self.graph is None or self.graph_steps != steps_per_graph or self.graph_hparams != self._hparams():
                self._capture_for_replay(steps_per_graph)
            while self.graph is not None and steps - done >= steps_per_graph:
                self._before_replay(steps_per_graph)
                self.graph.replay()
                self.step_count += steps_per_graph
                self.host_cursor += steps_per_graph
                done += steps_per_graph
        for _ in range(steps - done):
            self._plan_step()
        return steps

    @contextlib.contextmanager
    def _state_kept(self):
        """Save everything a step changes (weights, optimiser and scaler state, device step count and cursor, loss history,
        host step count and cursor) and put it back on leaving, also when the body raises.  Yields the restore function
        for a body that needs the state back early."""
        tensors = [t for t in (self.theta, self.m, self.v, self.dev_step, self.dev_cursor, self.loss_hist, self.norm_hist, self.norm,
                               self.avg) if t is not None]
        if self.scaler is not None:
            tensors.append(self.scaler.state)
        saved = [t.clone() for t in tensors]
        counts = (self.step_count, self.host_cursor)

        def restore():
            for t, s in zip(tensors, saved):
                t.copy_(s)
            self.step_count, self.host_cursor = counts
        try:
            yield restore
        finally:
            restore()

    def _capture(self, n):
        """Capture n steps of the plan in a hipGraph.  Consumes no steps: the engine ends where it began, also when the
        capture fails."""
        self.graph = None
        with self._state_kept() as restore:
            # hipFuncSetAttribute is not capturable, so every kernel must have been launched once before the capture:
            # run one step eagerly, then put back the exact pre-step state (capture itself executes nothing)
            self._plan_step()
            torch.cuda.synchronize()
            restore()
            self._prepare_capture(n)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for k in range(n):
                    self._graph_step(k)
        self.graph, self.graph_steps, self.graph_hparams = g, n, self._hparams()
        _upload_graph(g)

    def _single(self):
        """One rank and no collective in the step.  `_force_collective` (tests only) keeps the group's collectives in the step
        of a ONE-rank group, so that the RCCL form of the step — eager and captured in a hipGraph — runs on a one-GPU box."""
        return self.world == 1 and not self._force_collective

    def _rccl_capturable(self):
        """The step's collectives can be captured in a hipGraph: the group is RCCL (its collectives are capturable; gloo's run
        on the host), no capture of them has failed yet, and DMF_RCCL_GRAPH=0 does not switch it off."""
        if not self._rccl_graph:
            return False
        import os
        import torch.distributed as dist
        return dist.get_backend(self.pg) == 'nccl' and os.environ.get('DMF_RCCL_GRAPH', '1') != '0'

    def _all_reduce_grad(self):
        """self.grad <- its sum over the group: RCCL on the device, gloo through the host."""
        import torch.distributed as dist
        if dist.get_backend(self.pg) == 'nccl':
            dist.all_reduce(self.grad, op=dist.ReduceOp.SUM, group=self.pg)
        else:
            g = self.grad.cpu()
            dist.all_reduce(g, op=dist.ReduceOp.SUM, group=self.pg)
            self.grad.copy_(g)

    # hooks around the capture and replay; by default the graph's steps read plan[cursor] like eager plan steps
    def _capture_for_replay(self, n):
        try:
            self._capture(n)
        except RuntimeError as e:         # (a DmfError too: RCCL can invalidate the capture under the library's next launch)
            if self._single() or self.comm is not None:
                raise
            # RCCL's collective refused to be captured (every rank runs the same software, so every rank lands here): stay
            # on eager launches for the rest of this engine's life; the capture has put the engine's state back
            print('dmf: the step with the RCCL collectives could not be captured in a hipGraph (%s); eager launches from '
                  'here on' % e, file=sys.stderr, flush=True)
            self._rccl_graph = False
            torch.cuda.synchronize()

    def _prepare_capture(self, n):
        pass

    def _graph_step(self, k):
        self._plan_launch()

    def _before_replay(self, n):
        pass

    def losses(self):
        """Per-step mean loss of the plan steps run so far (one D2H copy)."""
        return self.loss_hist[:int(self.dev_cursor.item())].cpu()

    def grad_norms(self):
        """Per-step gradient norm BEFORE clipping — what `clip_grad_norm_` returns — of the plan steps run so far (one D2H
        copy).  Zeros without clip_grad_norm; a step the loss scaler skipped has a non-finite entry."""
        return self.norm_hist[:int(self.dev_cursor.item())].cpu()


class TrainEngine(_PlanEngine):
    """The single-stage train step on a resident scene: the fused step, or with a `criterion` the unit-gradient step around
    dmf_ce_loss (_PlanEngine: what each takes) — for the attention net the criterion inside the attention kernel, on the
    unit-gradient step's global batches.  `self.fused`, set once by the constructor, says which (True: no criterion)."""

    def __init__(self, net, scene, batch, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, process_group=None, comm=None, scaler=None,
                 optimizer='ADAM', momentum=0.0, alpha=0.99, criterion=None, weight_decay=0.0, clip_grad_norm=None,
                 criterion_in_kernel=False):
        """optimizer: 'ADAM', or the reference's other two (utils/utils.py:13-16) — 'SGD' (`momentum`) and 'RMSprop'
        (`alpha`, eps 1e-8) —, or 'ADAMW'.  weight_decay (torch's `weight_decay=`; decoupled with ADAMW) and clip_grad_norm
        (`clip_grad_norm_(params, max_norm)` between backward and step; None or 0: off) update by dmf_optim_step, without the
        xgmi exchange.  The launches after the backward: _PlanEngine._update.
        criterion: None = the plain cross-entropy fused into the patch kernel (two launches per step).  A spec of `Criterion`
        (class weights, label smoothing, focal term) trains by the unit-gradient step instead (no xgmi exchange).
        criterion_in_kernel (attention net with a criterion only): True evaluates the criterion inside the attention kernel
        (dmf_train_attn_fwd_bwd_ce) on the unit-gradient step's global batches: `step` / `load_plan` as there, the
        launches after the backward as without a criterion.  The default keeps what a caller of this constructor has always got
        for that net, the refusal (it has no unit-gradient step): whoever catches it to fall back elsewhere still does."""
        super().__init__(net, scene, lr, betas, eps, process_group, scaler, optimizer, momentum, alpha, weight_decay, clip_grad_norm)
        if scaler is not None and (comm is not None or self.shape.attention):
            raise lib.DmfError('loss scaling: late-fusion net, single GPU or RCCL data parallel (not the xgmi exchange)')
        if optimizer != 'ADAM' and comm is not None:
            raise lib.DmfError('%s: single GPU or RCCL data parallel (the fused xgmi exchange is ADAM)' % optimizer)
        if self._regularised() and comm is not None:
            raise lib.DmfError('weight_decay / clip_grad_norm: single GPU or a process group (the norm is taken after the '
                               'all-reduce; the fused xgmi exchange does not leave the flat gradient)')
        dev = scene.device
        if self.theta.device != dev:
            raise lib.DmfError('net and scene must be on the same device')
        self.B = int(batch)
        K = net.arch['K']
        self.logits = torch.empty(self.B, K, device=dev)
        self.loss = torch.zeros(self.B, device=dev)
        self.ws = torch.empty(lib.workspace_bytes(self.shape, self.B) // 4, device=dev)
        self.attn_ws = None
        if self.shape.attention:                      # token maps + dense gradient maps of the attention block
            self.attn_ws = torch.empty(lib.attn_train_workspace_bytes(self.shape, self.B), dtype=torch.uint8, device=dev)
        self.comm = comm if self.world > 1 else None
        if self.comm is not None and (self.comm.world != self.world or self.comm.capacity < self.theta.numel()):
            raise lib.DmfError('xgmi communicator does not match this engine (world / capacity)')
        self.plan_pack = self.win = None
        self.short_xy = self.short_labels = self.short_hist = None       # load_block: the epochs' short last batches
        self.short_norm = None
        self.criterion = None
        self.fused = criterion is None
        self.plan_denom = None                    # attention net with a criterion: the plan rows' denominators (float64)
        if criterion_in_kernel and (self.fused or not self.shape.attention):
            raise lib.DmfError('criterion_in_kernel belongs to the attention network with a criterion (the late-fusion net trains '
                               'a criterion by the unit-gradient step)')
        if not self.fused:
            if self.shape.attention and not criterion_in_kernel:
                raise lib.DmfError('a criterion with class weights, label smoothing or a focal term trains by the unit-gradient '
                                   'step, which the attention network does not have; criterion_in_kernel=True evaluates it '
                                   'inside the attention kernel instead')
            if not self.shape.attention and not lib.unit_supported(self.shape):
                raise lib.DmfError('a criterion with class weights, label smoothing or a focal term needs the unit-gradient '
                                   'kernel (dmf_unit_supported), which this shape does not have')
            if comm is not None:
                raise lib.DmfError('a criterion with class weights, label smoothing or a focal term: single GPU or a process '
                                   'group (not the xgmi exchange)')
            self.criterion = Criterion(criterion, K, dev)
            if self.shape.attention:              # the criterion inside the attention kernel (dmf_train_attn_fwd_bwd_ce)
                self.denom = torch.zeros(1, dtype=torch.float64, device=dev)     # ... of an eager step's batch
            else:
                self.dlogits = torch.empty(self.B, K, device=dev)

    # ------------------------------------------------------------------ eager step (host-side step count)
    def step(self, xy, labels, check=True):
        """One optimiser step on the patches at `xy` [B,2] int32 (device) with `labels` [B] int32 (device); the unit-gradient
        step: the global batch."""
        if not self.fused:
            xy, labels = self._rank_shard(xy, labels, self.B)
        if xy.shape[0] > self.B:
            raise lib.DmfError('engine was built for batches of at most %d, got %d' % (self.B, xy.shape[0]))
        if check:     # one D2H copy per call; load_plan() validates a whole epoch at once and run_plan() skips this
            lib.check_xy_bounds(self.shape, self.scene.A, self.scene.B, xy.cpu().numpy())
            self._check_labels(labels)
        inp = lib.input_gather(self.shape, self.scene.A, self.scene.B, xy)
        self._launch(inp, labels, None, None)

    def step_patches(self, a, b, labels):
        """Same step from materialised patch tensors (the reference dataloader's batch).  With a criterion: one rank only (the
        loss kernel needs the global batch's labels, and nothing shards materialised patches)."""
        if not self.fused and self.world > 1:
            raise lib.DmfError('step_patches with a criterion: one rank only (use step / load_plan, which take the global batch)')
        inp = lib.input_patches(self.shape, a, b)
        self._launch(inp, labels, None, None)

    def _counts_on_device(self):
        """As _PlanEngine's, and: the xgmi exchange numbers its rounds by the device step count, and SGD's first step is told
        by it."""
        return super()._counts_on_device() or self.comm is not None or self.optim not in ('ADAM', 'ADAMW')

    def _launch(self, inp, labels, dev_step, dev_cursor, loss_hist=None):
        dev_step = self._count_step(dev_step)
        sc, nB, cr = self.scaler, inp.B, self.criterion
        loss = self.loss if loss_hist is not None else None
        if not self.fused and self.shape.attention:
            # The criterion inside the attention kernel: the step keeps the fused step's launches.  labels: the GLOBAL batch's, and
            # its denominator — the plan's travel together (plan_denom); an eager batch's is one one-row launch ahead of the step.
            # The loss kernel's arithmetic has divided by the global batch: the ranks' sum is the gradient.
            denom = self.plan_denom if dev_cursor is not None else self.denom
            if dev_cursor is None:
                lib.ce_denominators(labels[:self.world * nB], self.world * nB, self.shape.K, denom, cr.class_w)
            lib.train_attn_fwd_bwd_ce(self.shape, inp, self.theta, self.net.pool_w, labels, denom, cr.params, self.world, self.rank,
                                      self.logits, self.loss, self.ws, self.attn_ws, class_w=cr.class_w, adam_step_dev=dev_step)
            return self._update(nB, dev_step, dev_cursor, 1.0, loss, loss_hist)
        if not self.fused:                     # labels: the GLOBAL batch's ([world * nB] at row dev_cursor)
            return self._unit_step(inp, nB, lambda: lib.ce_loss(
                self.logits[:nB], self.world, self.rank, labels, cr.params, class_w=cr.class_w, loss=self.loss,
                dlogits=self.dlogits[:nB], cursor=dev_cursor, scaler_state=sc.state if sc is not None else None),
                dev_step, dev_cursor, loss, loss_hist)
        if self.shape.attention:
            lib.train_attn_fwd_bwd(self.shape, inp, self.theta, self.net.pool_w, labels, None, 1.0 / nB, self.logits,
                                   self.loss, self.ws, self.attn_ws, adam_step_dev=dev_step)
        else:
            lib.train_fwd_bwd(self.shape, inp, self.theta, self.net.pool_w, labels, 1.0 / nB, self.logits, self.loss, self.ws,
                              adam_step_dev=dev_step, scaler_state=sc.state if sc is not None else None)
        # the loss is this rank's mean: the sum over the ranks is scaled by 1/world
        self._update(nB, dev_step, dev_cursor, 1.0 / self.world, loss, loss_hist)

    # ------------------------------------------------------------------ epoch plan + hipGraph replay
    def load_plan(self, xy_all, labels_all):
        """Upload an epoch's shuffled stream: xy_all [n*B, 2], labels_all [n*B] (host or device, any int type; _upload_plan);
        the unit-gradient step: an epoch of global batches (_load_global_plan)."""
        if not self.fused:
            return self._load_global_plan(xy_all, labels_all, self.B)
        return self._upload_plan(xy_all, labels_all, self.B, pack=True)

    def _plan_extras(self, labels, rows, cap):
        """The attention net with a criterion: the denominators travel with the labels — plan_denom [cap] float64, one
        dmf_ce_denominators launch per plan upload."""
        if self.fused or not self.shape.attention:
            return {}
        denom = torch.empty(cap, dtype=torch.float64, device=self.scene.device)
        lib.ce_denominators(labels, rows, self.shape.K, denom, self.criterion.class_w)
        return dict(plan_denom=denom)

    # ------------------------------------------------------------------ a block of epochs as one plan (train.epoch_block)
    def _host_ints(self, t, what):
        t = torch.as_tensor(t)
        if t.is_cuda:
            raise lib.DmfError('load_block takes host arrays (%s is on the device): its checks run before the upload' % what)
        return t.to(torch.int32).contiguous()

    def load_block(self, xy_all, labels_all, short_xy=None, short_labels=None, capacity=None):
        """The epoch-block form of load_plan: the full batches of SEVERAL consecutive epochs as one plan, xy_all [n*B, 2] and
        labels_all [n*B] (epoch after epoch), and the epochs' short last batches short_xy [E, r, 2], short_labels [E, r]
        (0 < r < B; None: the epochs have none).  HOST arrays only, so that loading reads nothing back from the device.
        `run_plan(steps, steps_per_graph)` then runs one epoch's steps at a time on the running cursor, with that epoch's lr /
        betas set on the engine; `step_short(e)` steps epoch e's short batch; `block_losses()` reads everything at the block's
        end.  capacity (steps, default n): blocks of different lengths keep one plan shape and with it the captured graph; the
        loss history is as long.  One GPU only."""
        if self.world != 1:
            raise lib.DmfError('load_block: one GPU only (the ranks of a data-parallel run check their exchange every epoch)')
        xy, lab = self._host_ints(xy_all, 'xy_all').reshape(-1, 2), self._host_ints(labels_all, 'labels_all').reshape(-1)
        self.short_xy = self.short_labels = self.short_hist = self.short_norm = None
        if short_xy is not None:
            sxy, slab = self._host_ints(short_xy, 'short_xy'), self._host_ints(short_labels, 'short_labels')
            if sxy.dim() != 3 or sxy.shape[2] != 2 or tuple(slab.shape) != tuple(sxy.shape[:2]) or not 0 < sxy.shape[1] <= self.B:
                raise lib.DmfError('short batches: short_xy [E, r, 2] and short_labels [E, r] with 0 < r <= %d' % self.B)
            lib.check_xy_bounds(self.shape, self.scene.A, self.scene.B, sxy.reshape(-1, 2).numpy())
            self._check_labels(slab)
        n = self._upload_plan(xy, lab, self.B, capacity=capacity or 1, pack=self.fused)      # (at least one step: tensors exist)
        if short_xy is not None:
            dev = self.scene.device
            self.short_xy, self.short_labels = sxy.to(dev), slab.to(dev)
            self.short_hist = torch.zeros(sxy.shape[0], device=dev)
            self.short_norm = torch.zeros(sxy.shape[0], device=dev)
        return n

    def step_short(self, e):
        """The short last batch of epoch e of the loaded block: one eager step on the device copy (load_block has checked it);
        its mean loss stays in short_hist[e].  No host synchronisation."""
        xy = self.short_xy[e]
        self.step(xy, self.short_labels[e], check=False)
        self.short_hist[e:e + 1].copy_(self.loss[:xy.shape[0]].mean().reshape(1))
        self.short_norm[e:e + 1].copy_(self.norm)
        self._seed_dev_step()

    def block_losses(self):
        """(per-step mean losses of the plan steps run so far, the short batches' mean losses or None), on the host: the
        block's two device-to-host copies."""
        return self.loss_hist[:self.host_cursor].cpu(), None if self.short_hist is None else self.short_hist.cpu()

    def block_grad_norms(self):
        """block_losses' counterpart for the pre-clip gradient norms (clip_grad_norm): (plan steps, short batches or None)."""
        return self.norm_hist[:self.host_cursor].cpu(), None if self.short_norm is None else self.short_norm.cpu()

    def _plan_launch(self):
        inp = lib.input_gather(self.shape, self.scene.A, self.scene.B, self.plan_xy, B=self.B, cursor=self.dev_cursor)
        self._launch(inp, self.plan_labels, self.dev_step, self.dev_cursor, self.loss_hist)

    def _fill_window(self, n):
        """Copy the next n steps of the plan into the fixed window the captured graph reads (one small async copy)."""
        self.win.copy_(self.plan_pack[self.host_cursor:self.host_cursor + n])

    def run_plan(self, steps=None, steps_per_graph=0):
        """As _PlanEngine.run_plan (graph replay on one GPU or over the xgmi communicator; RCCL: see _graphable); and
        steps_per_graph < 0 hands the steps to the library's own launch loop where `_native_loop_ok()`."""
        if steps_per_graph >= 0 or not self._native_loop_ok():
            return super().run_plan(steps, steps_per_graph)
        steps = self._steps_to_run(steps)
        # the library's own loop: 2 launches per step enqueued from C, the batches read straight from the plan (no window,
        # no graph): for a short run the fixed cost is one kernel launch instead of a window copy + a graph launch
        k0 = self.host_cursor
        inp = lib.input_gather(self.shape, self.scene.A, self.scene.B, self.plan_xy[k0 * self.B:(k0 + steps) * self.B], B=self.B)
        labels = self.plan_labels[k0 * self.B:(k0 + steps) * self.B]
        self._in_form('train_plan_steps', (self.shape, inp, self.theta, self.net.pool_w, labels, 1.0 / self.B, self.logits, self.loss,
                                           self.ws, self.m, self.v), dict(lr=self.lr, b1=self.b1, b2=self.b2),
                      dict(eps=self.eps, adam_step_dev=self.dev_step, cursor_dev=self.dev_cursor, loss_hist=self.loss_hist, n_steps=steps))
        self.step_count += steps
        self.host_cursor += steps
        return steps

    def _native_loop_ok(self):
        """run_plan(steps, steps_per_graph=-1): the C loop of dmf_train_plan_steps — late-fusion net, one GPU, the fused
        cross-entropy, the fused ADAM step."""
        return self._single() and self._fused_adam() and not self.shape.attention and self.fused

    def _graphable(self):
        """Can a step be captured in a hipGraph?  One GPU: yes.  The one-shot exchange: yes (it is part of the reduce launch).
        The RCCL all-reduce: yes when the process group is RCCL — its collectives are capturable, and a host-enqueued
        all_reduce of 32 KB per ~16-us step would otherwise bound the step by the host (DMF_RCCL_GRAPH=0 switches this off)."""
        if self._single() or self.comm is not None:
            return True
        return self._fused_adam() and self._rccl_capturable()

    def _prepare_capture(self, n):
        if not self.fused:                         # the graph's steps read plan[cursor] like eager plan steps: no window
            return
        if self.comm is not None:                  # the eager step used up an exchange sequence number; the bias is
            self.comm.rewind(1)                    # a launch argument, so it has to move BEFORE the capture
        # Inside the graph step k reads its coordinates and labels from slot k of a FIXED window (plain pointers baked
        # into the launch) instead of plan[cursor]: every kernel starts cold after the previous kernel's cache
        # write-back / invalidate, and `kernarg -> cursor -> coordinates -> gather` is one dependent miss longer than
        # `kernarg -> coordinates -> gather`.  The window is refilled from the plan before every replay.
        self.win = torch.empty(n, 3 * self.B, dtype=torch.int32, device=self.scene.device)   # per step: 2B coordinates, B labels
        if self.host_cursor + n <= self.plan_steps:
            self._fill_window(n)
        else:
            self.win.zero_()

    def _graph_step(self, k):
        if not self.fused:
            return self._plan_launch()
        inp = lib.input_gather(self.shape, self.scene.A, self.scene.B, self.win[k, :2 * self.B].view(self.B, 2))
        self._launch(inp, self.win[k, 2 * self.B:], self.dev_step, self.dev_cursor, self.loss_hist)

    def _before_replay(self, n):
        if self.fused:
            self._fill_window(n)

    def warm_graph(self):
        """One replay of the captured graph that leaves no trace (weights, optimiser state, cursors and loss history are put
        back): the first launch of a graph executable pays one-time costs of the launch machinery, which belong to a
        warm-up.  bench.py calls it when the requested warm-up is shorter than one graph.  Single GPU only: under the
        xGMI exchange a replay also advances the sequence numbers in the peers' inboxes, which cannot be put back."""
        if self.graph is None or not self._single() or self.host_cursor + self.graph_steps > self.plan_steps:
            return False
        with self._state_kept():
            if self.fused:
                self._fill_window(self.graph_steps)
            self.graph.replay()
            torch.cuda.synchronize()
        torch.cuda.synchronize()
        return True

    mean_losses = _PlanEngine.losses


class _ShardedEval:
    """The whole-set passes of both evaluation engines: confusion matrix and label map over any number of pixels, in chunks
    of the engine's size (`_walk`, the one place that shards, checks, uploads and slices).  With a process group every rank
    takes its contiguous shard of the pixels and the per-rank results are combined by an all-reduce.  An engine states two hooks:
      * `_check_bounds(xy_host)`: refuse pixels [n,2] (numpy) whose patches leave the resident scene;
      * `_chunk_forward(xy)`: pixels [n <= B, 2] on the device, already checked -> (logits or None, `pred[:n]`): one forward with
        its argmax, views valid until the next call."""

    def _check_batch(self, n):
        if n > self.B:
            raise lib.DmfError('batch larger than the engine was built for')

    def _shard(self, process_group, *tensors):
        """With a process group: this rank's contiguous shard of the rows of each tensor."""
        if process_group is None:
            return tensors
        import torch.distributed as dist
        from .parallel import shard_range
        lo, hi = shard_range(tensors[0].shape[0], dist.get_rank(process_group), dist.get_world_size(process_group))
        return tuple(t[lo:hi].contiguous() for t in tensors)

    @staticmethod
    def _all_reduce(x, process_group, allreduce_):
        """x <- allreduce_ (dmf.parallel.allreduce_sum_ / allreduce_max_) of x over the group, if one is given."""
        if process_group is None:
            return
        import torch.distributed as dist
        if dist.get_backend(process_group) == 'nccl':
            allreduce_(x, process_group)
        else:                                       # gloo (CPU tests, one-GPU rehearsal): reduce on the host
            x.copy_(allreduce_(x.cpu(), process_group))

    def _walk(self, process_group, xy_all, *more, extent=None):
        """All given pixels in chunks of `self.B` -> (rows, chunks).  At once, before anything is launched: this rank's shard of
        xy_all and of the per-pixel tensors `more` (labels) as int32; the pixels' patch bounds, checked on the host once for the
        whole set; with extent = (H, W, what) also that every pixel lies inside the [H, W] map the caller writes at (x, y); the
        upload, rows = (xy, *more) on the device.  `chunks` yields (xy, logits or None, pred, *its rows of more) per chunk."""
        rows = self._shard(process_group, *(torch.as_tensor(t).to(torch.int32) for t in (xy_all,) + more))
        host = rows[0].cpu().numpy()
        self._check_bounds(host)
        if extent is not None and len(host) and (int(host[:, 0].max()) >= extent[0] or int(host[:, 1].max()) >= extent[1]):
            raise lib.DmfError('pixel outside the %d x %d %s' % extent)                # the kernels write map[x * W + y]
        rows = tuple(t.to(self.scene.device).contiguous() for t in rows)

        def chunks(xy_all=rows[0]):
            for i in range(0, xy_all.shape[0], self.B):
                xy, *rest = (t[i:i + self.B] for t in rows)
                yield (xy, *self._chunk_forward(xy), *rest)
        return rows, chunks()

    def confusion(self, xy_all, labels_all, matrix=None, process_group=None):
        """Confusion matrix [K,K] int64 (rows = prediction) over all given pixels (mainsolver.py:137-147, tostagesolver.py:
        331-341).  With a process group the matrices of the ranks are summed (a given `matrix` is added to on every rank:
        pass zeros)."""
        from .parallel import allreduce_sum_
        K = self.net.arch['K']
        _, chunks = self._walk(process_group, xy_all, labels_all)
        if matrix is None:
            matrix = torch.zeros(K, K, dtype=torch.int64, device=self.scene.device)
        for _, _, pred, labels in chunks:
            lib.confusion_accum(pred, labels, K, matrix)
        self._all_reduce(matrix, process_group, allreduce_sum_)
        return matrix

    def label_map(self, xy_all, H, W, label_map=None, process_group=None):
        """Predicted class of every given pixel written at (x, y) of an [H, W] int32 map (mainsolver.py:171-183,
        tostagesolver.py:360-383).  With a process group the tiles are merged (every pixel is written by one rank)."""
        from .parallel import allreduce_max_
        _, chunks = self._walk(process_group, xy_all, extent=(H, W, 'label map'))
        if label_map is None:
            label_map = torch.zeros(H, W, dtype=torch.int32, device=self.scene.device)
        for xy, _, pred in chunks:
            lib.labelmap_write(pred, xy, W, label_map)
        self._all_reduce(label_map, process_group, allreduce_max_)
        return label_map


class EvalEngine(_ShardedEval):
    """Forward + argmax + on-device confusion matrix / label map (mainsolver.py:102-147,164-197)."""

    def __init__(self, net, scene, batch, criterion=None, tta=None):
        """criterion (a spec of `Criterion`, default None = plain cross-entropy): what `ce_sum` evaluates.
        tta (None, or ops as `Scene.atlas` takes them): test-time augmentation — `predict`, and with it the confusion matrix, the
        label map, the collected logits, the calibration and the confidence maps, give the mean over the variants of the logits
        (one forward per variant at the scene's mapped coordinates, then dmf_logits_mean).  The scene must be an `AtlasScene`
        that holds those variants.  The validation pass (`ce_sum`, `valid_accum`) stays on the untouched scene."""
        self.net, self.scene, self.B = net, scene, int(batch)
        self.tta_slots = None
        if tta is not None:
            from . import augment
            ops = augment.ops_of(tta, 'tta')
            if len(ops) > 1:
                if not isinstance(scene, AtlasScene) or any(k not in scene.ops for k in ops):
                    raise lib.DmfError('tta %s needs a scene atlas that holds these variants (Scene.atlas); this scene holds %s'
                                       % (list(ops), list(getattr(scene, 'ops', (0,)))))
                if (scene.patch, scene.scale) != (net.arch['P'], net.arch['S']):
                    raise lib.DmfError('tta: the atlas was built for patch %d, scale %d, the net takes %d, %d'
                                       % (scene.patch, scene.scale, net.arch['P'], net.arch['S']))
                self.tta_slots = [scene.slot_of(k) for k in ops]
                self.logits_v = torch.empty(len(ops) * self.B * net.arch['K'], device=scene.device)
        self.shape = net.shape
        lib.shape_supported(self.shape)
        dev = scene.device
        K = net.arch['K']
        self.criterion = Criterion(criterion, K, dev) if criterion is not None else None
        self.logits = torch.empty(self.B, K, device=dev)
        self.pred = torch.empty(self.B, dtype=torch.int32, device=dev)
        self.attn_ws = None
        if self.shape.attention:
            self.attn_ws = torch.empty(lib.attn_workspace_bytes(self.shape, self.B), dtype=torch.uint8, device=dev)
        self.ce = torch.zeros(self.B, device=dev)
        self._no_ce = False
        self._theta = None

    def use_parameters(self, flat=None):
        """Evaluate the flat vector `flat` (float32 on the scene's device, the net's layout — a train engine's
        `averaged_parameters()`) instead of the net's own parameters; None: the net's again.  The tensor is read at every call."""
        if flat is not None:
            lib._dev(flat, torch.float32, 'parameters')
            if flat.numel() != self.net.flat_parameters().numel() or flat.device != self.scene.device:
                raise lib.DmfError('use_parameters: a flat vector of the net\'s %d parameters on the scene\'s device'
                                   % self.net.flat_parameters().numel())
        self._theta = flat

    def _params(self):
        return self._theta if self._theta is not None else self.net.flat_parameters()

    def predict(self, xy):
        """xy [n,2] int32 device -> (logits [n,K], pred [n]) views valid until the next call."""
        if self.tta_slots is None:
            return self._predict_plain(xy)
        n, K = xy.shape[0], self.net.arch['K']
        self._check_batch(n)
        V = len(self.tta_slots)
        lv = self.logits_v[:V * n * K].view(V, n, K)
        for v, s in enumerate(self.tta_slots):
            self._forward(self.scene.map_xy(xy, s), lv[v], None)
        if n:
            lib.logits_mean(lv, self.logits[:n], self.pred)
        return self.logits[:n], self.pred[:n]

    def _forward(self, xy, logits, pred):
        inp = lib.input_gather(self.shape, self.scene.A, self.scene.B, xy)
        if self.shape.attention:
            lib.forward_attn(self.shape, inp, self._params(), self.net.pool_w, self.attn_ws, logits, pred)
        else:
            lib.forward(self.shape, inp, self._params(), self.net.pool_w, logits, pred)

    def _predict_plain(self, xy):
        """`predict` at the coordinates as they are: without test-time augmentation, and the validation pass with it."""
        n = xy.shape[0]
        self._check_batch(n)
        self._forward(xy, self.logits, self.pred)
        return self.logits[:n], self.pred[:n]

    def _patch_losses(self, xy, labels):
        """self.ce[:n] <- one validation term per patch of xy [n, 2] with labels [n] (int32 on the device); False where the
        shape has no such form, and the caller takes torch's cross-entropy on the logits of `predict`.  A property of the engine:
          a criterion            dmf_ce_loss on the logits: loss[i] = n t_i / D, in sum `criterion(output, target) * n` of the
                                 reference's validation loop (mainsolver.py:70-71);
          the attention network  none;
          otherwise              the evaluation launch's own per-patch cross-entropy (dmf_forward_ce), or none where the
                                 library refuses the shape: asked once and remembered."""
        if self.criterion is not None:
            cr = self.criterion
            lib.ce_loss(self._predict_plain(xy)[0], 1, 0, labels, cr.params, class_w=cr.class_w, loss=self.ce)
            return True
        if self.shape.attention or self._no_ce:
            return False
        inp = lib.input_gather(self.shape, self.scene.A, self.scene.B, xy)
        try:
            lib.forward_ce(self.shape, inp, self._params(), self.net.pool_w, labels, self.logits, self.ce, self.pred)
        except lib.DmfError:
            self._no_ce = True
            return False
        return True

    def ce_sum(self, xy, labels):
        """Sum of `_patch_losses` over the batch (device scalar, float64, torch's reduction); None without a per-patch form."""
        n = xy.shape[0]
        self._check_batch(n)
        if n == 0 and self.criterion is not None:
            return torch.zeros((), dtype=torch.float64, device=self.scene.device)
        return self.ce[:n].double().sum() if self._patch_losses(xy, labels) else None

    def valid_accum(self, xy, labels, acc):
        """acc [1] (device, float64) += the sum of `_patch_losses` (dmf_valid_accum), or without a per-patch form torch's
        cross-entropy on the logits, times n, added on the device.  xy is checked by the caller.  No synchronisation."""
        n = xy.shape[0]
        self._check_batch(n)
        if n == 0:
            return
        if self._patch_losses(xy, labels):
            lib.valid_accum(self.ce, n, acc)
        else:
            acc += torch.nn.functional.cross_entropy(self._predict_plain(xy)[0], labels.long()).double() * n

    def _check_bounds(self, xy_host):
        """(with test-time augmentation: the mapped coordinates of every variant used, which are what the kernel reads)"""
        if self.tta_slots is None or len(xy_host) == 0:
            lib.check_xy_bounds(self.shape, self.scene.A, self.scene.B, xy_host)
            return
        Hp, Wp = self.scene.extent
        if int(xy_host.min()) < 0 or int(xy_host[:, 0].max()) + self.shape.P > Hp or int(xy_host[:, 1].max()) + self.shape.P > Wp:
            raise lib.DmfError('patch window outside the padded scene')            # (a mapped coordinate is only then inside its slot)
        for s in self.tta_slots:
            lib.check_xy_bounds(self.shape, self.scene.A, self.scene.B, self.scene.map_xy(xy_host, s))

    def _chunk_forward(self, xy):
        return self.predict(xy)

    # ------------------------------------------------------------------ calibrated confidence
    # One device only: the solvers refuse the keys for data-parallel runs.  Everything works on `predict`'s logits, so the
    # late-fusion and the attention network share it.
    def _beta(self, inv_temp):
        """inv_temp (None, a number beta = 1 / T > 0, or a device float32 [1]) -> None or the device float32 [1]."""
        if inv_temp is None or torch.is_tensor(inv_temp):
            return inv_temp
        if not (inv_temp > 0 and np.isfinite(inv_temp)):
            raise lib.DmfError('inv_temp %r is not a finite number > 0' % (inv_temp,))
        return torch.tensor([float(inv_temp)], dtype=torch.float32, device=self.scene.device)

    def confidence_maps(self, xy_all, H, W, inv_temp=None):
        """-> (label map [H, W] int32, planes [3, H, W] float32: confidence, margin, entropy of the softmax at beta = inv_temp)
        of all given pixels, 0 elsewhere.  `label_map`'s chunks and launches, with one dmf_softmax_stats per chunk in the
        place of dmf_labelmap_write: the label map is the one `label_map` gives."""
        dev = self.scene.device
        beta = self._beta(inv_temp)
        _, chunks = self._walk(None, xy_all, extent=(H, W, 'label map'))
        label_map = torch.zeros(H, W, dtype=torch.int32, device=dev)
        planes = torch.zeros(3, H, W, dtype=torch.float32, device=dev)
        for xy, logits, _ in chunks:
            lib.softmax_stats(logits, pred=label_map, conf=planes[0], margin=planes[1], entropy=planes[2], inv_temp=beta, xy=xy, W=W)
        return label_map, planes

    # ------------------------------------------------------------------ spatial regularisation
    def probability_map(self, xy_all, H, W, inv_temp=None):
        """-> (prob [H, W, K] float32, mask [H, W] uint8): the softmax at beta = inv_temp of all given pixels and 1 where a
        pixel was given, 0 elsewhere.  `label_map`'s chunks and bounds checks, with one dmf_prob_scatter per chunk on
        `predict`'s logits: test-time augmentation and the attention net come with it."""
        dev = self.scene.device
        beta = self._beta(inv_temp)
        _, chunks = self._walk(None, xy_all, extent=(H, W, 'probability map'))
        prob = torch.zeros(H, W, self.net.arch['K'], dtype=torch.float32, device=dev)
        mask = torch.zeros(H, W, dtype=torch.uint8, device=dev)
        for xy, logits, _ in chunks:
            lib.prob_scatter(logits, xy, W, prob, mask, inv_temp=beta)
        return prob, mask

    def regularise(self, prob, mask, aff, iterations=1):
        """-> (prob' [H, W, K], label map [H, W] int32): `iterations` >= 1 passes of dmf_spatial_filter over prob / mask (as
        `probability_map` gives them) with the affinities aff [H, W, n] (`Scene.affinity`), ping-pong between two buffers; prob
        itself is not written.  The label map is the argmax of prob' where mask is 1, and 0 elsewhere."""
        if isinstance(iterations, bool) or not isinstance(iterations, int) or iterations < 1:
            raise lib.DmfError('regularise: iterations = %r is not a whole number >= 1' % (iterations,))
        label_map = torch.zeros(prob.shape[0], prob.shape[1], dtype=torch.int32, device=prob.device)
        src, bufs = prob, [torch.empty_like(prob)]
        for it in range(iterations):
            if it == 1:
                bufs.append(torch.empty_like(prob))
            dst = bufs[it % 2]
            lib.spatial_filter(src, mask, aff, dst, label_map)
            src = dst
        return src, label_map

    # ------------------------------------------------------------------ superpixel voting
    def segment_vote(self, prob, mask, seg, size, mode='mean'):
        """-> (segprob [Kc, K] float32, segcount [Kc] int32, label map [H, W] int32): one dmf_segment_vote over prob / mask (as
        `probability_map` gives them) and the segments seg [H, W] of size `size` (`Scene.segments`).  mode `mean`: a segment's row
        is the mean probability of its masked members; `majority`: their class counts.  The label map is the first maximal class
        of a masked pixel's segment, and 0 where mask is 0; prob is not written."""
        gh, gw = lib.segment_grid(prob.shape[0], prob.shape[1], size)
        segprob = torch.empty(gh * gw, prob.shape[2], dtype=torch.float32, device=prob.device)
        segcount = torch.empty(gh * gw, dtype=torch.int32, device=prob.device)
        label_map = torch.zeros(prob.shape[0], prob.shape[1], dtype=torch.int32, device=prob.device)
        with torch.cuda.device(prob.device):
            lib.segment_vote(prob, mask, seg, size, mode, segprob, segcount, label_map)
        return segprob, segcount, label_map

    # ------------------------------------------------------------------ connected superpixels
    def region_vote(self, prob, mask, region, R, mode='mean'):
        """-> (regprob [R, K] float32, regcount [R] int32, label map [H, W] int32): one dmf_region_vote over prob / mask (as
        `probability_map` gives them) and the regions 0..R - 1 of region [H, W] (`Scene.segment_regions`), which may have any shape.
        mode `mean`: a region's row is the mean probability of its masked members in exact fixed point; `majority`: their class
        counts.  The label map is the first maximal class of a masked pixel's region, and 0 where mask is 0; prob is not written."""
        regprob = torch.empty(R, prob.shape[2], dtype=torch.float32, device=prob.device)
        regcount = torch.empty(R, dtype=torch.int32, device=prob.device)
        label_map = torch.zeros(prob.shape[0], prob.shape[1], dtype=torch.int32, device=prob.device)
        with torch.cuda.device(prob.device):
            ws = torch.empty(lib.region_vote_workspace_bytes(R, prob.shape[2]), dtype=torch.uint8, device=prob.device)
            lib.region_vote(prob, mask, region, R, mode, regprob, regcount, label_map, ws)
        return regprob, regcount, label_map

    def collect_logits(self, xy_all, labels_all=None):
        """-> the logits of all given pixels in ONE device tensor [N, K] (and their labels as device int32 [N])."""
        rows, chunks = self._walk(None, xy_all, *(() if labels_all is None else (labels_all,)))
        out = torch.empty(rows[0].shape[0], self.net.arch['K'], device=self.scene.device)
        for (_, logits, *_), dst in zip(chunks, out.split(self.B)):
            dst.copy_(logits)
        return out if labels_all is None else (out, rows[1])

    def calibration_of(self, logits, labels, nbins, inv_temp=None, hist=None):
        """hist [nbins, 3] int64 (+)= the reliability histogram of device logits [n, K] / labels [n] at beta = inv_temp."""
        n, K = logits.shape
        dev = self.scene.device
        if hist is None:
            hist = torch.zeros(nbins, 3, dtype=torch.int64, device=dev)
        if n:
            conf, pred = torch.empty(n, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
            lib.softmax_stats(logits, pred=pred, conf=conf, inv_temp=self._beta(inv_temp))
            lib.calib_accum(conf, pred, labels, K, hist)
        return hist

    def calibration(self, xy_all, labels_all, nbins, inv_temp=None):
        """Reliability histogram hist [nbins, 3] int64 over all given pixels (rows, hits, confidence sum in units of 2^-32 per
        confidence bin; dmf_softmax_stats + dmf_calib_accum per chunk).  Labels outside [0, K) are skipped."""
        beta = self._beta(inv_temp)
        _, chunks = self._walk(None, xy_all, labels_all)
        hist = torch.zeros(nbins, 3, dtype=torch.int64, device=self.scene.device)
        for _, logits, _, labels in chunks:
            self.calibration_of(logits, labels, nbins, beta, hist)
        return hist

    def _temp_ws(self, n):
        """The fit's workspace, allocated on first use and grown on demand."""
        need = lib.temperature_workspace_bytes(n)
        if getattr(self, '_temp_workspace', None) is None or self._temp_workspace.numel() < need:
            self._temp_workspace = torch.empty(max(need, 24), dtype=torch.uint8, device=self.scene.device)
        return self._temp_workspace

    def nll_of(self, logits, labels, inv_temp=None):
        """-> device float64 [TEMP_DOUBLES]: dmf_temperature_step's evaluation (update = 0) of logits [n, K] / labels [n] at
        beta = inv_temp; [1] is the NLL summed over the rows."""
        state = torch.empty(lib.TEMP_DOUBLES, dtype=torch.float64, device=self.scene.device)
        lib.temperature_init(state)
        beta = self._beta(inv_temp)
        if beta is not None:
            state[0:1].copy_(beta)
        lib.temperature_step(logits, labels, state, self._temp_ws(logits.shape[0]), update=False)
        return state

    def fit_temperature_of(self, logits, labels, steps=40):
        """The temperature fit on device logits [n, K] / labels [n] -> float64 numpy [3, TEMP_DOUBLES], read once: the
        evaluation at beta = 1, the state after `steps` safeguarded Newton steps, the evaluation at the fitted beta."""
        if logits.shape[0] < 1:
            raise lib.DmfError('fit_temperature: no pixels to fit on')
        ws = self._temp_ws(logits.shape[0])
        out = torch.empty(3, lib.TEMP_DOUBLES, dtype=torch.float64, device=self.scene.device)
        at_one, state, at_fit = out[0], out[1], out[2]
        for s in (at_one, state):
            lib.temperature_init(s)
        lib.temperature_step(logits, labels, at_one, ws, update=False)
        for _ in range(steps):
            lib.temperature_step(logits, labels, state, ws, update=True)
        at_fit.copy_(state)
        lib.temperature_step(logits, labels, at_fit, ws, update=False)
        return out.cpu().numpy()

    def fit_temperature(self, xy_all, labels_all, steps=40):
        """Temperature scaling on the given split (the validation split): `steps` steps of dmf_temperature_step enqueued at
        once -> the state (float64 numpy [TEMP_DOUBLES]: beta, nll, g, h, lo, hi, steps taken, reserved), read once.
        `last_fit` keeps all three rows of `fit_temperature_of`."""
        self.last_fit = self.fit_temperature_of(*self.collect_logits(xy_all, labels_all), steps=steps)
        return self.last_fit[1]


# ====================================================================== stage 2 of the two-stage path
class QuaScene:
    """The four co-registered padded scenes of stage 2 (ms, pan, ms_gan, pan_gan; tostagesolver.py:248-257) resident
    in HBM as ONE tall pixel-major scene [4*Hp, Wp, C] plus its band mean [4*Hp, Wp, 1] (the single-input net's
    auxiliary modality).  Stream k's patch at pixel (x, y) is the tall scene's patch at (x + k*Hp, y); a window
    never crosses into the next stream because every stream carries its own bottom padding."""

    def __init__(self, scenes, device, half=False):
        if len(scenes) != 4 or any(s.shape != scenes[0].shape for s in scenes):
            raise lib.DmfError('stage 2 wants four scenes of one shape')
        self.Hp = int(scenes[0].shape[0])
        tall = np.ascontiguousarray(np.concatenate([np.asarray(s, dtype=np.float32) for s in scenes], axis=0))
        self.A = torch.from_numpy(tall).to(device)
        self.B = lib.band_mean_scene(self.A)          # (of the fp32 bands: the aux modality stays fp32)
        self.half = bool(half)
        if half:                                      # `gmf.half`: the primary scene is kept as fp16 (round to nearest even)
            self.A = self.A.to(torch.float16)
        self.device = torch.device(device)

    @classmethod
    def from_raw(cls, scenes_raw, patch, device, half=False):
        """The scene of `QuaScene([data_padding(s, ..) for s in scenes_raw], device, half)`, bit for bit, prepared on the device:
        every stream is normalised by its own extremes and written into its own quarter of the tall tensor.  Falls back to
        exactly that host call, saying why, where prep_route sends a stream to the host."""
        scenes_raw = [np.asarray(s) for s in scenes_raw]
        if len(scenes_raw) != 4 or scenes_raw[0].ndim != 3 or any(s.shape != scenes_raw[0].shape for s in scenes_raw):
            raise lib.DmfError('stage 2 wants four scenes [H, W, C] of one shape')
        H, W, C = scenes_raw[0].shape
        pad = patch - 1
        why = ''
        for s in scenes_raw:
            why = why or prep_route(s.dtype, H, W, pad)[1]
        if not why:
            Hp = H + pad
            tall = torch.empty(4 * Hp, W + pad, C, device=device)
            for k, s in enumerate(scenes_raw):
                why = why or _prepare_on_device(s, pad, tall[k * Hp:(k + 1) * Hp])
        if why:
            _host_fallback(why)
            from function.function import data_padding
            cfg = {'patch_size': patch}
            return cls([data_padding(s, cfg, 'ms') for s in scenes_raw], device, half=half)
        self = cls.__new__(cls)
        self.Hp, self.half, self.device = Hp, bool(half), torch.device(device)
        self.B = lib.band_mean_scene(tall)
        self.A = tall.to(torch.float16) if half else tall
        return self

    def stack_xy(self, xy, streams=4):
        """[n, 2] pixel coordinates -> [streams*n, 2] int32 coordinates in the tall scene, on the device `xy` lives on,
        stream-major like `torch.concat([data1, data2, data3, data4])` (tostagesolver.py:272)."""
        xy = torch.as_tensor(xy).to(torch.int32)
        out = xy.repeat(streams, 1).view(streams, xy.shape[0], 2)
        out[:, :, 0] += (torch.arange(streams, dtype=torch.int32, device=xy.device) * self.Hp)[:, None]   # stream k: k*Hp rows down
        return out.view(-1, 2)


class QuaTrainEngine(_PlanEngine):
    """Stage-2 train step (tostagesolver.py:268-278) on the resident tall scene, no host sync.  The loss couples the whole
    batch, so it cannot ride inside the per-patch kernel like cross-entropy does.  Two forms:
      * unit-gradient step (shapes with a v2 kernel): `_unit_step` on the 4*bs stacked patches around `dmf_qua_loss_ranks`;
        the step replays from a captured hipGraph (`run_plan(steps, steps_per_graph)`);
      * otherwise `dmf_forward` -> `dmf_qua_loss_ranks` -> `dmf_backward_dlogits` (recomputes the forward) -> the update.
    `step` / `load_plan` take GLOBAL batches (see _PlanEngine).  Data parallel (process_group): `all_gather_into_tensor` of the
    logits into a buffer allocated once (gloo: a host gather and one H2D copy into it) feeds the loss of the GLOBAL batch, which
    writes this rank's rows of d loss / d logits.  Over RCCL the whole step replays from a captured hipGraph like the
    single-GPU one.  The update after the backward (optimiser, loss scaler, all-reduce): _PlanEngine._update."""

    def __init__(self, net, scene, bs, dqtl, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, process_group=None, scaler=None,
                 optimizer='ADAM', momentum=0.0, alpha=0.99, weight_decay=0.0, clip_grad_norm=None):
        if not net.arch.get('single_input'):
            raise lib.DmfError('stage 2 needs the single-input net (cfg["gmf"]["single_input"] = 1)')
        super().__init__(net, scene, lr, betas, eps, process_group, scaler, optimizer, momentum, alpha, weight_decay, clip_grad_norm)
        self.bs = int(bs)
        self.unit = lib.unit_supported(self.shape)
        if scaler is not None and not self.unit:
            raise lib.DmfError('loss scaling in stage 2: unit-gradient step')
        self.params = lib.qua_params(dqtl)
        dev = scene.device
        K = net.arch['K']
        self.logits = torch.empty(4 * self.bs, K, device=dev)
        self.dlogits = torch.empty(4 * self.bs, K, device=dev)
        self.loss = torch.zeros(1, device=dev)
        self.ws = torch.empty(lib.workspace_bytes(self.shape, 4 * self.bs) // 4, device=dev)
        # data parallel: the logits of all ranks, rank-major [world][4][bs][K] as all_gather_into_tensor leaves them
        self.gathered = torch.empty(self.world * 4 * self.bs, K, device=dev) if process_group is not None else None

    def _gather(self, bs):
        """This rank's logits [4*bs, K] -> the gathered [world*4*bs, K] (rank-major)."""
        import torch.distributed as dist
        mine, out = self.logits[:4 * bs], self.gathered[:self.world * 4 * bs]
        if dist.get_backend(self.pg) == 'nccl':
            dist.all_gather_into_tensor(out, mine, group=self.pg)
        else:                                       # gloo: gather on the host, one H2D copy into the same buffer
            parts = [torch.empty(mine.shape) for _ in range(self.world)]
            dist.all_gather(parts, mine.cpu(), group=self.pg)
            out.copy_(torch.cat(parts))
        return out

    def _step(self, inp, bs, labels, cursor, loss_hist, dev_step=None):
        """One step on this rank's 4*bs stacked patches; labels: the GLOBAL batch's ([world*bs] at row cursor)."""
        dev_step = self._count_step(dev_step)

        def loss_launch():
            # the loss of the global batch from the logits of all ranks (one GPU: its own logits, world 1, rank 0)
            logits = self.logits[:4 * bs] if self._single() else self._gather(bs)
            lib.qua_loss_ranks(logits, self.world, self.rank, bs, labels, self.params, loss=self.loss,
                               dlogits=self.dlogits[:4 * bs], cursor=cursor, loss_hist=loss_hist,
                               scaler_state=self.scaler.state if self.scaler is not None else None)
        if self.unit:
            return self._unit_step(inp, 4 * bs, loss_launch, dev_step, cursor)
        lib.forward(self.shape, inp, self.theta, self.net.pool_w, self.logits)
        loss_launch()
        lib.backward_dlogits(self.shape, inp, self.theta, self.net.pool_w, self.dlogits, self.ws)
        # dmf_forward does not count steps: the non-unit form updates by the host count
        self._update(4 * bs, None, cursor, 1.0)

    def step(self, xy, labels):
        """One step on the global batch `xy` [world*bs, 2] (host or device ints) with `labels` [world*bs], e.g. the solver's
        short last batch."""
        xy, lab = self._rank_shard(xy, labels, self.bs)
        xy4 = self.scene.stack_xy(xy.cpu()).to(self.scene.device).contiguous()
        lib.check_xy_bounds(self.shape, self.scene.A, self.scene.B, xy4.cpu().numpy())
        self._check_labels(lab)
        inp = lib.input_gather(self.shape, self.scene.A, self.scene.B, xy4)
        self._step(inp, xy.shape[0], lab, None, None)

    def load_plan(self, xy_all, labels_all):
        """An epoch of full global batches (_load_global_plan); the plan holds every batch's 4*bs stacked coordinates."""
        return self._load_global_plan(xy_all, labels_all, self.bs, rows=lambda xy: torch.cat(
            [self.scene.stack_xy(batch) for batch in xy.split(self.bs)]))

    def _plan_launch(self):
        # (the captured graph runs these same launches: its steps read plan[cursor])
        inp = lib.input_gather(self.shape, self.scene.A, self.scene.B, self.plan_xy, B=4 * self.bs, cursor=self.dev_cursor)
        self._step(inp, self.bs, self.plan_labels, self.dev_cursor, self.loss_hist, self.dev_step)

    def _graphable(self):
        """The unit-gradient form on one GPU, or over an RCCL group (its all-gather and all-reduce are captured with the
        step's launches, TrainEngine's rules: _rccl_capturable); gloo steps eagerly."""
        return self.unit and (self._single() or self._rccl_capturable())

    def _capture(self, n):
        """Capture n steps (unit-gradient form, one GPU or RCCL); see _PlanEngine._capture."""
        if not self._graphable():
            raise lib.DmfError('graph replay needs the unit-gradient step on one GPU or over RCCL')
        super()._capture(n)

    # bench.py: the step's dominant launch alone (for HIP-event timing) and its name
    def time_dominant(self, inp):
        if self.unit:
            lib.forward_unit(self.shape, inp, self.theta, self.net.pool_w, self.logits, self.ws)
        else:
            lib.backward_dlogits(self.shape, inp, self.theta, self.net.pool_w, self.dlogits, self.ws)

    def dominant_name(self):
        a = self.net.arch
        if self.unit:
            return 'dmf::patch_v2_kernel<Shape<%d,%d,%d,1,%d,..>, MODE_UNIT%s> (dmf_forward_unit: forward + unit gradients of the 4*bs stacked patches)' % (
                a['C'], a['C2'], a['P'], a['F'], ', fp16 scene' if getattr(self.scene, 'half', False) else '')
        return 'dmf::patch_kernel<ShapeQua, MODE_BWD> (dmf_backward_dlogits: forward recompute + backward of the 4*bs stacked patches)'


class QuaEvalEngine(_ShardedEval):
    """Stage-2 prediction `(out[:bs] + out[bs:2*bs]).softmax(-1).argmax` (tostagesolver.py:337): only the ms and pan
    streams enter it, so only those two are computed."""

    def __init__(self, net, scene, batch, dqtl=None):
        self.net, self.scene, self.B = net, scene, int(batch)
        self.shape = net.shape
        lib.shape_supported(self.shape)
        dev = scene.device
        self.logits = torch.empty(4 * self.B, net.arch['K'], device=dev)
        self.pred = torch.empty(self.B, dtype=torch.int32, device=dev)
        self.loss = torch.zeros(1, device=dev)
        self.params = lib.qua_params(dqtl) if dqtl is not None else None

    def _forward(self, xy, streams, checked=False):
        """Logits of the first `streams` streams of the pixels xy [n,2] into self.logits[:streams*n]; returns n."""
        n = int(xy.shape[0])
        self._check_batch(n)
        xyk = self.scene.stack_xy(xy, streams)
        if not checked:
            lib.check_xy_bounds(self.shape, self.scene.A, self.scene.B, xyk.cpu().numpy())
        inp = lib.input_gather(self.shape, self.scene.A, self.scene.B, xyk.to(self.scene.device))
        lib.forward(self.shape, inp, self.net.flat_parameters(), self.net.pool_w, self.logits)
        return n

    def _check_bounds(self, xy_host):            # (only the ms and pan streams are read)
        lib.check_xy_bounds(self.shape, self.scene.A, self.scene.B, self.scene.stack_xy(xy_host, 2).numpy())

    def _chunk_forward(self, xy, checked=True):
        n = self._forward(xy, 2, checked)
        lib.pair_argmax(self.logits, n, self.pred)
        return None, self.pred[:n]

    def predict(self, xy):
        pred = self._chunk_forward(xy, checked=False)[1]
        return self.logits[:2 * pred.shape[0]], pred

    def loss_value(self, xy, labels):
        """qua_loss of a batch without gradients (the validation loop, tostagesolver.py:288-296); device scalar."""
        n = self._forward(xy, 4)
        lab = torch.as_tensor(labels).to(device=self.scene.device, dtype=torch.int32).contiguous()
        lib.qua_loss(self.logits[:4 * n], n, lab, self.params, loss=self.loss)
        return self.loss
