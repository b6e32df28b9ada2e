"""GPU: superpixel voting of class maps — dmf_slic_init, dmf_slic_assign, dmf_slic_update and dmf_segment_vote against
the float64 statement of tests/segments_ref.py on the cases of tests/segments_cases.py (whose guards are CPU tests in
tests/test_segments_host.py), Scene.segments / EvalEngine.segment_vote end to end, and the solver keys on the 40 x 40 x 8, 4-class
scene of tests/test_gpu_calibration.py.

Bounds (derived from the number formats, not fitted; each test prints its largest ratio before it asserts):
  init      bit-equal: a copy of scene values (an fp16 scene widened exactly) and of integers.
  assign    the same centres go into the float64 reference.  |delta D| <= D (C + 8) 2^-24 (segments_ref.distances: a C-term fmaf
            chain of squared rounded differences and a divide; four roundings and a product on the spatial term; one add), so the
            labels are compared outside the tie set: the pixels whose float64 gap between the best and the second-best D is within
            the sum of the two bounds.  Every label is one of its pixel's candidates, ties included.
  update    the device's own seg goes into the reference.  Counts exact.  Spectrum: |delta| <= (S^2 + 2) 2^-24 mean|a| over the
            members (a cell partial is an fp32 chain over at most S^2 members; the rest is double and one rounding).  Position:
            integers, a double divide and one rounding: <= 2^-24 |position|.
  vote      majority: integers, exactly equal.  mean: |delta| <= segprob (count + 2) 2^-24 (an fp32 chain of `count` non-negative
            terms and a divide); labels equal for the segments whose two largest means are further apart than the sum of their
            bounds (segments_ref.vote_unclear).
Every output of a kernel call sits between guard words that must stay as they were.

Observed on an MI355X (printed by the tests): init bit-equal in 144 cases; assign equal to the reference outside tie
sets of 1, 0 and 2 of 96,688 pixels (S = 4, 5, 16; two rounds per case); update at most 0.23 (spectrum) and 0.97 (position: a
correctly rounded quotient sits at up to 1.0 of its bound) of the bounds; vote mean at most 0.39 of its bound over 72 cases with no
pixel left out of the label comparison, majority exact; guard (b) on all 88 scenes with more than one cell per axis: the device's
segments purer than the grid on 78 (by at least 0.026), perfectly pure on the 7 whose grid is, the reference's figures at the 3
recorded shortfalls;
the engine's 13 x 9 pass at 0.88 (update) and 0.20 (vote) of the bounds; on the solver's scene no assign tie, the drop-in path's
segment image and majority map equal to the fast path's at all 1600 pixels."""
import ctypes as C
import functools
import json
import os
import shutil
import tempfile

import numpy as np
import pytest
import torch
from PIL import Image

import segments_cases as SC
import segments_ref as R

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
GUARD = 64                                               # guard elements on either side of an output


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                 # (a copy: the cases are read-only arrays)


class Guarded:
    """A contiguous device tensor of `shape` inside a larger allocation whose other elements hold a pattern."""

    def __init__(self, shape, dtype, fill):
        n = int(np.prod(shape))
        self.pattern = 85 if dtype == torch.uint8 else -12345
        self.whole = torch.full((n + 2 * GUARD,), self.pattern, dtype=dtype, device=DEV)
        self.t = self.whole[GUARD:GUARD + n].view(*shape)
        self.t.fill_(fill)
        self.n = n

    def intact(self):
        return bool((self.whole[:GUARD] == self.pattern).all() and (self.whole[GUARD + self.n:] == self.pattern).all())


def _cases(seg_size):
    return [c for c in SC.SLIC_CASES if c[4] == seg_size]


def _init_gpu(scene, H, W, S):
    from dmf import lib
    gh, gw = lib.segment_grid(H, W, S)
    cen = Guarded((gh * gw, scene.shape[2] + 2), torch.float32, -7.0)
    lib.slic_init(scene, H, W, S, cen.t)
    assert cen.intact()
    return cen.t


def _assign_gpu(scene, H, W, S, centres, fill=-7):
    from dmf import lib
    seg = Guarded((H, W), torch.int32, fill)
    lib.slic_assign(scene, H, W, S, SC.COMPACTNESS, centres, seg.t)
    assert seg.intact()
    return seg.t


def _update_gpu(scene, H, W, S, seg, centres, fill=9):
    """-> (centres', counts): `centres` is copied first, the call updates the copy."""
    from dmf import lib
    Cn = scene.shape[2]
    new = Guarded(tuple(centres.shape), torch.float32, 0.0)
    new.t.copy_(centres)
    counts = Guarded((centres.shape[0],), torch.int32, -7)
    ws = Guarded((lib.slic_workspace_bytes(H, W, Cn, S),), torch.uint8, fill)
    lib.slic_update(scene, H, W, S, seg, new.t, counts.t, ws.t)
    torch.cuda.synchronize()
    assert new.intact() and counts.intact() and ws.intact()
    return new.t, counts.t


# ------------------------------------------------------------------------------------------------ init, assign, update
@pytest.mark.parametrize('seg_size', SC.SEG_SIZES)
def test_init_assign_update_against_float64(seg_size):
    worst_spec, worst_pos, ties, pixels = 0.0, 0.0, 0, 0
    for H, W, Cn, half, S in _cases(seg_size):
        a = SC.scene(H, W, Cn, half)
        scene = _dev(a)
        cen = _init_gpu(scene, H, W, S)
        assert np.array_equal(cen.cpu().numpy().astype(np.float64), R.init(a, H, W, S)), (H, W, Cn, half, S)        # bit-equal
        cand, valid = R.candidates(H, W, S)
        for rnd in range(2):                             # the initial centres, then those of one update
            seg = _assign_gpu(scene, H, W, S, cen)
            got = seg.cpu().numpy()
            want, tie = R.assign(a, H, W, S, SC.COMPACTNESS, cen.cpu().numpy())
            assert np.array_equal(got[~tie], want[~tie]), (H, W, Cn, half, S, rnd, int((got != want)[~tie].sum()))
            assert (valid & (cand == got[None])).any(0).all(), (H, W, Cn, half, S, rnd)      # a candidate, ties included
            assert torch.equal(_assign_gpu(scene, H, W, S, cen, fill=5), seg)                # two calls: the same bits
            ties += int(tie.sum())
            pixels += H * W
            new, counts = _update_gpu(scene, H, W, S, seg, cen)
            ref, ref_counts, absmean = R.update(a, H, W, S, got, cen.cpu().numpy())
            assert np.array_equal(counts.cpu().numpy(), ref_counts) and ref_counts.sum() == H * W, (H, W, Cn, half, S, rnd)
            ratio = np.abs(new.cpu().numpy().astype(np.float64) - ref) / R.update_bound(absmean, ref, S)
            worst_spec, worst_pos = max(worst_spec, float(ratio[:, :Cn].max())), max(worst_pos, float(ratio[:, Cn:].max()))
            assert ratio.max() <= 1.0, (H, W, Cn, half, S, rnd, float(ratio[:, :Cn].max()), float(ratio[:, Cn:].max()))
            again, counts2 = _update_gpu(scene, H, W, S, seg, cen, fill=200)                 # another workspace content: the same bits
            assert torch.equal(again, new) and torch.equal(counts2, counts)
            cen = new
    print('S = %d: %d cases; update at most %.3f (spectrum) and %.3f (position) of the bounds; %d of %d pixels in the tie sets'
          % (seg_size, len(_cases(seg_size)), worst_spec, worst_pos, ties, pixels))


@pytest.mark.parametrize('Cn,half', [(3, False), (200, False), (8, True), (1, False)])
def test_a_pitch_and_an_element_aligned_base_give_the_bits_of_the_plain_layout(Cn, half):
    """The leading 35 x 34 pixels of a scene [37, 39, C] that starts one element into its buffer; what lies beyond column W and
    row H (here: huge values) is never read."""
    H, W, S = 35, 34, 5
    a = SC.scene(H, W, Cn, half)
    big = np.full((H + 2, W + 5, Cn), 1000.0, dtype=a.dtype)
    big[:H, :W] = a
    flat = torch.empty(big.size + 1, dtype=torch.float16 if half else torch.float32, device=DEV)
    view = flat[1:].view(big.shape)
    view.copy_(torch.from_numpy(big))
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    plain = _dev(a)
    cen, cen_v = _init_gpu(plain, H, W, S), _init_gpu(view, H, W, S)
    seg, seg_v = _assign_gpu(plain, H, W, S, cen), _assign_gpu(view, H, W, S, cen_v)
    new, counts = _update_gpu(plain, H, W, S, seg, cen)
    new_v, counts_v = _update_gpu(view, H, W, S, seg_v, cen_v)
    assert torch.equal(cen, cen_v) and torch.equal(seg, seg_v) and torch.equal(new, new_v) and torch.equal(counts, counts_v)


def test_an_emptied_cluster_keeps_its_row_and_foreign_labels_count_for_nothing():
    H, W, Cn, S = 33, 17, 8, 5
    a = SC.scene(H, W, Cn)
    scene = _dev(a)
    cen = _init_gpu(scene, H, W, S)
    seg = _assign_gpu(scene, H, W, S, cen).cpu().numpy()
    gh, gw = R.grid(H, W, S)
    k = 1 * gw + 1                                       # cell (1, 1): its members go to their own cell, its own pixels to the right
    own = R.grid_segments(H, W, S)
    odd = np.where(seg == k, np.where(own == k, k + 1, own), seg).astype(np.int32)
    odd[0, 0], odd[1, 1], odd[2, 2], odd[H - 1, W - 1] = gh * gw - 1, -1, 2 ** 31 - 1, 0       # none of these pixels' candidates
    new, counts = _update_gpu(scene, H, W, S, _dev(odd), cen)
    ref, ref_counts, absmean = R.update(a, H, W, S, odd, cen.cpu().numpy())
    assert ref_counts[k] == 0 and ref_counts.sum() == H * W - 4
    assert np.array_equal(counts.cpu().numpy(), ref_counts)
    assert torch.equal(new[k], cen[k])                   # untouched, bit for bit
    ratio = np.abs(new.cpu().numpy().astype(np.float64) - ref) / R.update_bound(absmean, ref, S)
    assert ratio.max() <= 1.0


# ------------------------------------------------------------------------------------------------ iterations
def _scene_object(a, half):
    from dmf.engine import Scene
    return Scene(np.array(a, dtype=np.float32), np.zeros(a.shape[:2], dtype=np.float32), DEV, half=half)     # (a copy: the cases are read-only)


@pytest.mark.parametrize('H,W,Cn,half,S', [(35, 34, 8, False, 5), (64, 65, 200, True, 16), (13, 9, 3, False, 4)])
def test_three_iterations_are_three_manual_rounds(H, W, Cn, half, S):
    from dmf import lib
    sc = _scene_object(SC.scene(H, W, Cn, half), half)
    seg, cen, counts = sc.segments(H, W, S, SC.COMPACTNESS, 3)
    assert sc.segments(H, W, S, SC.COMPACTNESS, 3)[0] is seg and sc.segments(H, W, S, SC.COMPACTNESS, 2)[0] is not seg
    seg, cen, counts = sc.segments(H, W, S, SC.COMPACTNESS, 3)
    c = _init_gpu(sc.A, H, W, S)
    for _ in range(3):
        c, n = _update_gpu(sc.A, H, W, S, _assign_gpu(sc.A, H, W, S, c), c)
    assert torch.equal(cen, c) and torch.equal(counts, n) and torch.equal(seg, _assign_gpu(sc.A, H, W, S, c))
    assert seg.dtype == torch.int32 and tuple(seg.shape) == (H, W) and tuple(cen.shape) == (counts.shape[0], Cn + 2)
    with pytest.raises(lib.DmfError, match='iterations'):
        sc.segments(H, W, S, SC.COMPACTNESS, -1)
    with pytest.raises(lib.DmfError, match='pixels asked'):
        sc.segments(H + 1, W, S, SC.COMPACTNESS, 1)
    with pytest.raises(lib.DmfError, match='segment size'):
        sc.segments(H, W, 3, SC.COMPACTNESS, 1)


@pytest.mark.parametrize('seg_size', SC.SEG_SIZES)
def test_the_segments_are_purer_than_the_grid(seg_size):
    """The guard's scenes (tests/test_segments_host.py, guard (b)), ten iterations on the device."""
    low, n, found = 1.0, 0, 0
    for H, W, Cn, half, S in _cases(seg_size):
        if not SC.purity_asked(H, W, S):
            continue
        plain = R.purity(R.grid_segments(H, W, S), SC.ids(H, W))
        seg = _scene_object(SC.scene(H, W, Cn, half), half).segments(H, W, S, SC.COMPACTNESS, SC.ITERATIONS)[0].cpu().numpy()
        got = R.purity(seg, SC.ids(H, W))
        SC.check_purity((H, W, Cn, half, S), got, plain)
        if (H, W, Cn, half, S) in SC.PURITY_SHORTFALLS:
            found += 1
            print('  recorded shortfall: %d x %d x %d, S = %d: purity %.3f, grid %.3f' % (H, W, Cn, S, got, plain))
        elif plain < 1.0:
            low, n = min(low, got - plain), n + 1
    print('S = %d: %d scenes purer than the grid, the smallest gain %.3f; %d recorded shortfalls' % (seg_size, n, low, found))
    assert n > 0


# ------------------------------------------------------------------------------------------------ vote
@functools.lru_cache(maxsize=None)
def _vote_segments(H, W, S):
    """The device's segments of the 8-band case scene after three iterations (numpy)."""
    return _scene_object(SC.scene(H, W, 8), False).segments(H, W, S, SC.COMPACTNESS, 3)[0].cpu().numpy()


def _vote_inputs(H, W, K):
    """Device (prob, mask): the case's logits scattered at the masked pixels into a prob full of NaN (an unmasked row is never read)."""
    from dmf import lib
    mask_np = SC.mask(H, W)
    keep = mask_np.reshape(-1) != 0
    prob = torch.full((H, W, K), float('nan'), device=DEV)
    mask = torch.zeros(H, W, dtype=torch.uint8, device=DEV)
    if keep.any():
        lib.prob_scatter(_dev(SC.logits(H, W, K)[keep]), _dev(SC.pixels(H, W)[keep]), W, prob, mask)
    return prob, mask


def _vote_gpu(prob, mask, seg, S, mode, with_out=True):
    from dmf import lib
    H, W, K = prob.shape
    gh, gw = lib.segment_grid(H, W, S)
    segprob, segcount = Guarded((gh * gw, K), torch.float32, -7.0), Guarded((gh * gw,), torch.int32, -7)
    label, out = Guarded((H, W), torch.int32, -7), Guarded((H, W, K), torch.float32, -7.0)
    lib.segment_vote(prob, mask, seg, S, mode, segprob.t, segcount.t, label.t, out.t if with_out else None)
    torch.cuda.synchronize()
    assert segprob.intact() and segcount.intact() and label.intact() and out.intact()
    assert with_out or bool((out.t == -7.0).all())
    return segprob.t, segcount.t, label.t, out.t


def _check_vote(prob, mask, seg_np, S, mode):
    """One vote against the reference -> (largest ratio to the bound, pixels left out of the label comparison)."""
    H, W, K = prob.shape
    segprob, segcount, label, out = _vote_gpu(prob, mask, _dev(seg_np.astype(np.int32)), S, mode)
    live = mask.cpu().numpy() != 0
    p64 = np.nan_to_num(prob.cpu().numpy().astype(np.float64))
    w_prob, w_count, w_label, w_rows, orphan = R.vote(p64, live, seg_np, S, mode)
    got_p, got_l, got_o = segprob.cpu().numpy(), label.cpu().numpy(), out.cpu().numpy()
    assert np.array_equal(segcount.cpu().numpy(), w_count)
    assert (got_l[~live] == -7).all() and (got_o[~live] == 0.0).all()                    # mask 0: the cell stays, the row is zeros
    assert not np.isnan(got_p).any() and not np.isnan(got_o).any()                       # no NaN of an unmasked row was read
    if mode == 'majority':
        assert np.array_equal(got_p.astype(np.float64), w_prob) and np.array_equal(got_l[live], w_label[live])
        assert np.array_equal(got_o.astype(np.float64)[live], w_rows[live])
        ratio, unclear = 0.0, np.zeros((H, W), dtype=bool)
    else:
        ratio = float((np.abs(got_p.astype(np.float64) - w_prob) / R.vote_bound(w_prob, w_count)).max())
        assert ratio <= 1.0, (H, W, K, S, ratio)
        member = live & ~orphan
        unclear = np.zeros((H, W), dtype=bool)
        unclear[member] = R.vote_unclear(w_prob, w_count)[seg_np[member]]
        clear = live & ~unclear
        assert np.array_equal(got_l[clear], w_label[clear]), (H, W, K, S)
        assert np.array_equal(got_o[member], got_p[seg_np[member]])                      # prob_out: the segment's row, bit for bit
        assert np.array_equal(got_o[orphan], prob.cpu().numpy()[orphan])                 # an orphan: its own row
    assert (got_l[live] >= 0).all() and (got_l[live] < K).all()
    again = _vote_gpu(prob, mask, _dev(seg_np.astype(np.int32)), S, mode, with_out=False)
    assert torch.equal(again[0], segprob) and torch.equal(again[1], segcount) and torch.equal(again[2], label)      # the same bits
    return ratio, int((live & unclear).sum()), orphan


@pytest.mark.parametrize('mode', ['mean', 'majority'])
@pytest.mark.parametrize('seg_size', SC.SEG_SIZES)
def test_vote_against_float64(seg_size, mode):
    worst, left_out, n = 0.0, 0, 0
    for H, W, K, S in SC.VOTE_CASES:
        if S != seg_size:
            continue
        prob, mask = _vote_inputs(H, W, K)
        ratio, unclear, orphan = _check_vote(prob, mask, _vote_segments(H, W, S), S, mode)
        assert not orphan.any()
        worst, left_out, n = max(worst, ratio), left_out + unclear, n + 1
    print('S = %d, %s: %d cases; largest |delta| / bound %.3f; pixels left out of the label comparison %d' % (seg_size, mode, n, worst, left_out))


@pytest.mark.parametrize('mode', ['mean', 'majority'])
def test_foreign_and_negative_labels_stand_for_themselves(mode):
    """A hand-made seg: labels that are none of their pixel's candidates, negative ones, huge ones.  Those pixels get their own first
    maximal class and change nothing else: every other pixel gets what it gets without them in the scene's mask."""
    H, W, K, S = 35, 34, 17, 5
    prob, mask = _vote_inputs(H, W, K)
    seg = _vote_segments(H, W, S).copy()
    gh, gw = R.grid(H, W, S)
    where = [(0, 0), (3, 7), (17, 20), (34, 33), (10, 10), (20, 5)]
    for (i, j), v in zip(where, (gh * gw - 1, -1, -2 ** 31, 0, 2 ** 31 - 1, gh * gw)):
        seg[i, j] = v
    live = mask.cpu().numpy() != 0
    _, _, orphan = _check_vote(prob, mask, seg, S, mode)
    assert orphan.sum() == sum(bool(live[i, j]) for i, j in where) > 0
    # the rest of the scene: as if those pixels were not classified at all
    mask2 = mask.clone()
    for i, j in where:
        mask2[i, j] = 0
    a = _vote_gpu(prob, mask, _dev(seg.astype(np.int32)), S, mode)
    b = _vote_gpu(prob, mask2, _dev(_vote_segments(H, W, S)), S, mode)
    rest = torch.from_numpy(live & ~orphan).to(DEV)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2][rest], b[2][rest]) and torch.equal(a[3][rest], b[3][rest])
    own = torch.from_numpy(R.first_max(np.nan_to_num(prob.cpu().numpy(), nan=-1.0))).to(DEV)
    assert torch.equal(a[2][torch.from_numpy(orphan).to(DEV)].long(), own[torch.from_numpy(orphan).to(DEV)])


def test_aliased_outputs_and_argument_errors_are_refused():
    from dmf import lib
    H, W, Cn, K, S = 13, 9, 3, 3, 4
    scene = _dev(SC.scene(H, W, Cn))
    gh, gw = lib.segment_grid(H, W, S)
    cen = _init_gpu(scene, H, W, S)
    seg = _assign_gpu(scene, H, W, S, cen)
    prob, mask = _vote_inputs(H, W, K)
    segprob, segcount = torch.full((gh * gw, K), -7.0, device=DEV), torch.full((gh * gw,), -7, dtype=torch.int32, device=DEV)
    label = torch.full((H, W), -7, dtype=torch.int32, device=DEV)
    kept = (cen.clone(), seg.clone(), prob.clone())
    with pytest.raises(lib.DmfError, match='overlaps'):
        lib.segment_vote(prob, mask, seg, S, 'mean', segprob, segcount, label, prob)
    with pytest.raises(lib.DmfError, match='overlaps'):
        lib.segment_vote(prob, mask, seg, S, 'mean', segprob, segcount, seg)
    flat = torch.zeros(2 * H * W * K, device=DEV)
    a, b = flat[:H * W * K].view(H, W, K), flat[K:K + H * W * K].view(H, W, K)            # shifted by one row of classes: they overlap
    with pytest.raises(lib.DmfError, match='overlaps'):
        lib.segment_vote(a, mask, seg, S, 'mean', segprob, segcount, label, b)
    both = torch.zeros(H * W + cen.numel(), device=DEV)                                   # centres and seg in one buffer, two words apart
    with pytest.raises(lib.DmfError, match='overlaps'):
        lib.slic_assign(scene, H, W, S, 0.05, both[:cen.numel()].view(cen.shape), both.view(torch.int32)[2:2 + H * W].view(H, W))
    with pytest.raises(lib.DmfError, match='overlaps'):
        lib.slic_update(scene, H, W, S, seg, both[:cen.numel()].view(cen.shape), both.view(torch.int32)[1:1 + gh * gw],
                        torch.zeros(lib.slic_workspace_bytes(H, W, Cn, S), dtype=torch.uint8, device=DEV))
    with pytest.raises(lib.DmfError, match='mode'):
        lib.segment_vote(prob, mask, seg, S, 'median', segprob, segcount, label)
    with pytest.raises(lib.DmfError, match='compactness'):
        lib.slic_assign(scene, H, W, S, float('nan'), cen, seg)
    with pytest.raises(lib.DmfError, match='compactness'):
        lib.slic_assign(scene, H, W, S, -1.0, cen, seg)
    with pytest.raises(lib.DmfError, match='segment size'):
        lib.slic_init(scene, H, W, 33, cen)
    with pytest.raises(lib.DmfError, match='too small'):
        lib.slic_update(scene, H, W, S, seg, cen, torch.zeros(gh * gw, dtype=torch.int32, device=DEV),
                        torch.zeros(lib.slic_workspace_bytes(H, W, Cn, S) - 1, dtype=torch.uint8, device=DEV))
    for bad in (dict(centres=cen[:-1].contiguous()), dict(seg=seg.long()), dict(seg=seg[:-1].contiguous())):
        kw = dict(dict(centres=cen, seg=seg), **bad)
        with pytest.raises(lib.DmfError):
            lib.slic_assign(scene, H, W, S, 0.05, kw['centres'], kw['seg'])
    torch.cuda.synchronize()
    assert torch.equal(cen, kept[0]) and torch.equal(seg, kept[1]) and prob.cpu().numpy().tobytes() == kept[2].cpu().numpy().tobytes()
    assert (segprob == -7).all() and (segcount == -7).all() and (label == -7).all()


# ------------------------------------------------------------------------------------------------ the engine, end to end
@pytest.mark.parametrize('half,tta', [(False, None), (False, 'flips'), (True, None)], ids=['fp32', 'fp32-flips', 'fp16'])
def test_segments_and_vote_through_the_engine(half, tta):
    """The 13 x 9 tiny1 scene (as a d4 atlas: slot 0 is the scene), all 117 pixels in chunks of 50."""
    from dmf.engine import EvalEngine
    from test_gpu_augment import H, W, _case
    c = _case('tiny1', half, False)
    scene, K, S = c['scene'], c['K'], 4
    ev = EvalEngine(c['hip'], scene, 50, tta=tta)
    xy = c['xy']
    prob, mask = ev.probability_map(xy, H, W, inv_temp=0.5)
    A = c['A'].numpy()
    A = A.astype(np.float16) if half else A
    seg, cen, counts = scene.segments(H, W, S, SC.COMPACTNESS, 3)
    assert scene.segments(H, W, S, SC.COMPACTNESS, 3)[0] is seg
    # the rounds by hand on the host's scene: every assign outside its tie set, every update inside its bounds
    cur = R.init(A, H, W, S)
    dev_c = _init_gpu(scene.A, H, W, S)
    assert np.array_equal(dev_c.cpu().numpy().astype(np.float64), cur)
    worst = 0.0
    for rnd in range(4):
        s_dev = _assign_gpu(scene.A, H, W, S, dev_c)
        want, tie = R.assign(A, H, W, S, SC.COMPACTNESS, dev_c.cpu().numpy())
        assert np.array_equal(s_dev.cpu().numpy()[~tie], want[~tie])
        if rnd == 3:
            break
        new, n = _update_gpu(scene.A, H, W, S, s_dev, dev_c)
        ref, ref_n, absmean = R.update(A, H, W, S, s_dev.cpu().numpy(), dev_c.cpu().numpy())
        ratio = float((np.abs(new.cpu().numpy().astype(np.float64) - ref) / R.update_bound(absmean, ref, S)).max())
        worst = max(worst, ratio)
        assert np.array_equal(n.cpu().numpy(), ref_n) and ratio <= 1.0
        dev_c = new
    assert torch.equal(s_dev, seg) and torch.equal(dev_c, cen) and torch.equal(n, counts)
    seg_np = seg.cpu().numpy()
    for mode in ('mean', 'majority'):
        segprob, segcount, label = ev.segment_vote(prob, mask, seg, S, mode)
        w_prob, w_count, w_label, _, orphan = R.vote(prob.cpu().numpy().astype(np.float64), mask.cpu().numpy(), seg_np, S, mode)
        assert not orphan.any() and np.array_equal(segcount.cpu().numpy(), w_count) and label.dtype == torch.int32
        if mode == 'majority':
            assert np.array_equal(segprob.cpu().numpy().astype(np.float64), w_prob) and np.array_equal(label.cpu().numpy(), w_label)
        else:
            ratio = float((np.abs(segprob.cpu().numpy().astype(np.float64) - w_prob) / R.vote_bound(w_prob, w_count)).max())
            clear = ~R.vote_unclear(w_prob, w_count)[seg_np]
            print('%s, tta %s: update %.3f and vote %.3f of their bounds; %d of 117 pixels left out'
                  % ('fp16' if half else 'fp32', tta, worst, ratio, int((~clear).sum())))
            assert ratio <= 1.0 and np.array_equal(label.cpu().numpy()[clear], w_label[clear])
    # a partial set: label 0 where mask is 0
    some = xy[::3]
    p2, m2 = ev.probability_map(some, H, W)
    l2 = ev.segment_vote(p2, m2, seg, S, 'mean')[2]
    off = m2.cpu().numpy() == 0
    assert off.sum() == 117 - len(some) and (l2.cpu().numpy()[off] == 0).all()


# ------------------------------------------------------------------------------------------------ the solver
SEED = 3407
BASE = {'test': dict(calibration=1, calibration_bins=15, temperature=1.5, spatial='bilateral'), 'color': dict(spatial=1)}
KEYS_ON = {'test': dict(segments='slic', segment_size=5, segment_compactness=0.05, segment_iterations=3, segment_vote='majority'),
           'color': dict(segments=1)}
NETS = {'late_fusion': 'plain_native_loop', 'attention': 'attention'}


def _read(path):
    with open(path, 'rb') as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def _run(net, keys, golden_dir):
    """Two epochs of Solver.train() on the epoch-block scene with the calibration and the spatial filter on, then test() and
    color(); with `keys` also what the segment keys leave, the engine's own voted map, and the same test() / color() by a drop-in
    solver (fast_path: 0) on the weights this run saved."""
    from solver.mainsolver import Solver
    from test_gpu_epoch_block import _cfg
    tmp = tempfile.mkdtemp(prefix='dmf_segments_')
    try:
        cfg = _cfg(golden_dir, tmp, NETS[net], 1)
        cfg['epoch'] = 2
        for sec, val in list(BASE.items()) + (list(KEYS_ON.items()) if keys else []):
            cfg[sec] = dict(cfg[sec], **val)
        torch.manual_seed(SEED)
        s = Solver(cfg)
        s.dataloader()
        s.train()
        s.test()
        s.color()
        rng_after = torch.rand(4)
        out = cfg['RESULT_output']
        r = dict(matrix=s.test_matrix.copy(), result=list(s.result[:3]), maps=s.label_maps, rng_after=rng_after,
                 png=[_read(out + '0_pic_%d.png' % k) for k in (1, 2)], calibration=_read(out + '0_calibration.json'),
                 spatial=_read(out + '0_spatial.json'), files=sorted(os.listdir(out)))
        if not keys:
            return r
        lut = np.asarray(cfg['DATA_DICT'][cfg['data_city']]['color'], dtype=np.uint8)
        r.update(segments=s.segments, json=json.load(open(out + '0_segments.json')), segment_maps=s.segment_maps, lut=lut,
                 npy=np.load(out + '0_segments.npy'), segments_png=[np.asarray(Image.open(out + '0_pic_%d_segments.png' % k)) for k in (1, 2)])
        # the engine's own pass over the whole scene
        xy = torch.from_numpy(s._scene_pixels())
        prob, mask = s.eval_engine.probability_map(xy, 40, 40, s._beta(1.5))
        seg = s.scene.segments(40, 40, 5, 0.05, 3)[0]
        segprob, _, label = s.eval_engine.segment_vote(prob, mask, seg, 5, 'majority')
        A = s.scene.A[:40, :40].cpu().numpy()
        r.update(engine_label=label.cpu().numpy(), engine_seg=seg.cpu().numpy(), n_pixels=int(mask.sum().item()),
                 engine_counts=segprob.cpu().numpy().astype(np.float64),
                 ties=R.slic(A, 40, 40, 5, 0.05, 3)[3], plain_label=s.eval_engine.label_map(xy, 40, 40).cpu().numpy())
        test_rows = np.asarray(s.test_index_loader.dataset.indices)
        r.update(test_xy=s._set_pixels(test_rows), test_lab=s.index_dataset.label[test_rows].astype(np.int64),
                 labelled_xy=s._set_pixels(s.matrix_[1]))
        cfg0 = dict(cfg, fast_path=0, train=dict(cfg['train'], index=0))
        torch.manual_seed(SEED)
        d = Solver(cfg0)
        d.dataloader()
        d.test()
        d.color()
        r.update(dropin=d.segments, dropin_maps=d.segment_maps, dropin_seg=d.segment_image, dropin_plain=d.label_maps[1])
        return r
    finally:
        shutil.rmtree(tmp)


@pytest.mark.parametrize('net', sorted(NETS))
def test_the_keys_change_nothing_that_was_there(golden_dir, net):
    on, off = _run(net, True, golden_dir), _run(net, False, golden_dir)
    assert off['matrix'].sum() > 0 and np.array_equal(on['matrix'], off['matrix']) and on['result'] == off['result']
    assert on['maps'][0].tobytes() == off['maps'][0].tobytes() and on['maps'][1].tobytes() == off['maps'][1].tobytes()
    assert on['png'] == off['png'] and len(on['png'][0]) > 0 and on['calibration'] == off['calibration'] and len(on['calibration']) > 0
    assert on['spatial'] == off['spatial'] and len(on['spatial']) > 0
    assert torch.equal(on['rng_after'], off['rng_after'])                           # torch's RNG stream is where it was
    new = {'0_segments.json', '0_segments.npy', '0_pic_1_segments.png', '0_pic_2_segments.png'}
    assert set(on['files']) - set(off['files']) == new and set(off['files']) <= set(on['files'])


@pytest.mark.parametrize('net', sorted(NETS))
def test_the_segments_block_and_maps(golden_dir, net):
    r = _run(net, True, golden_dir)
    b = r['segments']
    assert r['json'] == json.loads(json.dumps(b))
    m = np.array(b['matrix'])
    assert m.shape == r['matrix'].shape and m.sum() == r['matrix'].sum() == b['n'] == len(r['test_xy'])
    assert np.array_equal(m.sum(0), r['matrix'].sum(0))                             # the same pixels: the same targets per class
    aa, oa, k = r['result']
    assert b['before'] == dict(OA=oa, AA=aa, kappa=k) and b['connectivity'] == 'not enforced'
    assert (b['kind'], b['size'], b['compactness'], b['iterations'], b['vote'], b['Kc']) == ('slic', 5, 0.05, 3, 'majority', 64)
    sizes = np.bincount(r['engine_seg'].reshape(-1), minlength=64)
    assert b['segments'] == int((sizes > 0).sum()) and b['segment_pixels']['max'] == sizes.max() and sizes.sum() == 1600
    assert r['npy'].dtype == np.int32 and np.array_equal(r['npy'], r['engine_seg'])
    x, y = r['test_xy'][:, 0], r['test_xy'][:, 1]
    want = np.zeros_like(m)
    np.add.at(want, (r['engine_label'][x, y], r['test_lab']), 1)
    assert np.array_equal(m, want)
    assert b['changed'] == int((r['engine_label'][x, y] != r['plain_label'][x, y]).sum())
    assert r['n_pixels'] == 1600                                                    # both colour sets: the whole scene
    m1, m2 = r['segment_maps']
    assert np.array_equal(m2, r['engine_label']) and np.array_equal(r['segments_png'][1], r['lut'][r['engine_label']])
    labelled = np.zeros((40, 40), dtype=bool)
    labelled[r['labelled_xy'][:, 0], r['labelled_xy'][:, 1]] = True
    assert 0 < labelled.sum() <= 1600 and np.array_equal(r['segments_png'][0], r['lut'][m1])
    assert (m1[~labelled] == 0).all() and np.array_equal(m1[labelled], r['engine_label'][labelled])
    print('%s: %d segments; OA %.4f -> %.4f, kappa %.4f -> %.4f, %d of %d test pixels changed class'
          % (net, b['segments'], b['before']['OA'], b['after']['OA'], b['before']['kappa'], b['after']['kappa'], b['changed'], b['n']))


@pytest.mark.parametrize('net', sorted(NETS))
def test_the_drop_in_path_gives_the_same_majority_map_where_no_tie_was_recorded(golden_dir, net):
    """The float64 reference records the pixels that were a near tie in any of the four assigns; without one the two paths have the
    same segment image.  The majority map is then compared on every segment that has the same pixels on both paths and whose class
    the two paths' per-pixel classes cannot turn: the paths classify with different arithmetic (Net.forward against the HIP
    kernels), so a segment with d pixels whose plain class differs is compared when its two largest counts are more than 2 d apart
    (d = 0: always; equal counts then resolve to the same first class)."""
    r = _run(net, True, golden_dir)
    ties, seg_e, seg_d = r['ties'], r['engine_seg'], r['dropin_seg']
    if not ties.any():
        assert np.array_equal(seg_d, seg_e)
    same_pixels = np.ones(64, dtype=bool)
    same_pixels[np.unique(np.concatenate([seg_e[seg_e != seg_d], seg_d[seg_e != seg_d]]))] = False
    d = np.bincount(seg_e.reshape(-1), weights=(r['plain_label'] != r['dropin_plain']).reshape(-1), minlength=64)
    counts = np.sort(r['engine_counts'], axis=1)
    clear_seg = same_pixels & ((d == 0) | (counts[:, -1] - counts[:, -2] > 2 * d))
    clear = clear_seg[seg_e]
    differ = r['dropin_maps'][1] != r['segment_maps'][1]
    print('%s: %d of 1600 pixels were a tie in some assign; the segment images differ at %d pixels, the plain classes at %d; %d of 64 '
          'segments (%d pixels) are compared; the maps differ at %d pixels, %d of them compared'
          % (net, int(ties.sum()), int((seg_d != seg_e).sum()), int(d.sum()), int(clear_seg.sum()), int(clear.sum()), int(differ.sum()),
             int((differ & clear).sum())))
    assert clear.any() and not (differ & clear).any()
    # the floor of what is compared: a segment is left out only for a reason that the figures above show.  Without a tie the
    # segment images are equal, so every segment without a pixel of differing plain class is compared — all 64 where d is 0
    assert clear_seg[same_pixels & (d == 0)].all() and (ties.any() or same_pixels.all())
    if not ties.any() and not d.any():
        assert clear.all() and not differ.any()
    assert r['dropin']['n'] == r['segments']['n'] and r['dropin']['size'] == 5
