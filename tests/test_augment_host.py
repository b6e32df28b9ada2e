"""CPU: the geometry of flip / rotate augmentation — the window identity behind the scene atlas, the coordinate
map against lib.check_xy_bounds, the pinned slot draw, and what the solvers do with `schedule.augment` / `test.tta` before
anything reaches the GPU.  dmf.augment (what the product uses) is held to tests/aug_ref.py (written from the definition).
"""
import os
import shutil
import tempfile
import types

import numpy as np
import pytest
import torch

import aug_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 13, 9


def _scenes(P, S, C=3, C2=2, seed=0):
    """Padded scenes of a 13 x 9 scene as the solver holds them: A [Hp, Wp, C], Bm [S H + S P - 1, S W + S P - 1, C2]."""
    rng = np.random.default_rng(seed)
    A = rng.random((H + P - 1, W + P - 1, C)).astype(np.float32)
    Bm = rng.random((S * H + S * P - 1, S * W + S * P - 1, C2)).astype(np.float32)
    return A, Bm


@pytest.mark.parametrize('P', [5, 4])
@pytest.mark.parametrize('S', [1, 4])
@pytest.mark.parametrize('ops', [aug_ref.FLIPS, aug_ref.D4, (0, 5)])
def test_the_atlas_window_at_the_mapped_coordinate_is_the_transformed_window(P, S, ops):
    from dmf import augment
    A, Bm = _scenes(P, S)
    Hp, Wp = A.shape[:2]
    atA, atB, R = aug_ref.scene_atlases(A, Bm, P, S, ops)
    assert (R, atA.shape[1]) == augment.atlas_geometry(Hp, Wp, ops) == aug_ref.geometry(Hp, Wp, ops)
    assert atA.shape[0] == len(ops) * R and atB.shape[:2] == (len(ops) * S * R, S * atA.shape[1])
    assert np.array_equal(atA[:Hp, :Wp], A) and np.array_equal(atB[:S * Hp, :S * Wp], Bm[:S * Hp, :S * Wp])     # slot 0: the scene
    xy = aug_ref.all_pixels(H, W)
    for s, k in enumerate(ops):
        m = aug_ref.map_xy(xy, s, ops, Hp, Wp, P, R)
        assert np.array_equal(m, augment.map_xy(xy, s, ops, (Hp, Wp), P, R))
        assert np.array_equal(m, augment.map_xy(torch.from_numpy(xy), s, ops, (Hp, Wp), P, R).numpy())
        for (x, y), (mx, my) in zip(xy, m):
            assert np.array_equal(atA[mx:mx + P, my:my + P], aug_ref.tf(A[x:x + P, y:y + P], k))
            assert np.array_equal(atB[S * mx:S * mx + S * P, S * my:S * my + S * P],
                                  aug_ref.tf(Bm[S * x:S * x + S * P, S * y:S * y + S * P], k))
    # a slot per sample, as an epoch plan has it
    slots = aug_ref.draw(7, 2, xy, len(ops))
    assert np.array_equal(aug_ref.map_xy(xy, slots, ops, Hp, Wp, P, R), augment.map_xy(xy, slots, ops, (Hp, Wp), P, R))


def test_tf_of_the_product_is_the_definition():
    from dmf import augment
    X = np.arange(13 * 9 * 2).reshape(13, 9, 2)
    for k in range(8):
        assert np.array_equal(augment.tf(X, k), aug_ref.tf(X, k))
        assert np.array_equal(augment.tf(torch.from_numpy(X), k).numpy(), aug_ref.tf(X, k))
    a = np.random.default_rng(1).random((16, 3, 5, 5)).astype(np.float32)
    ks = np.arange(16) % 8
    assert np.array_equal(augment.tf_batch(torch.from_numpy(a), ks).numpy(), aug_ref.tf_patches(a, ks))


@pytest.mark.parametrize('S', [1, 4])
@pytest.mark.parametrize('ops', [aug_ref.FLIPS, aug_ref.D4])
def test_mapped_coordinates_pass_the_bounds_check_and_one_past_does_not(S, ops):
    from dmf import lib
    P = 5
    A, Bm = _scenes(P, S)
    Hp, Wp = A.shape[:2]
    atA, atB, R = aug_ref.scene_atlases(A, Bm, P, S, ops)
    shape = types.SimpleNamespace(P=P, S=S)
    xy = aug_ref.all_pixels(H, W)
    for s in range(len(ops)):
        lib.check_xy_bounds(shape, atA, atB, aug_ref.map_xy(xy, s, ops, Hp, Wp, P, R))
    # the last valid row of the last slot is the atlas' last window; one further leaves it
    last = aug_ref.map_xy(xy, len(ops) - 1, ops, Hp, Wp, P, R)
    worst = last[last[:, 0].argmax()].copy()
    assert worst[0] + P <= atA.shape[0]
    lib.check_xy_bounds(shape, atA, atB, worst[None])
    worst[0] = atA.shape[0] - P + 1
    with pytest.raises(lib.DmfError, match='outside the padded scene'):
        lib.check_xy_bounds(shape, atA, atB, worst[None])
    # without a transposed op the slots are exactly full: x + 1 past the last valid pixel of the last slot is refused
    if not any(k & 4 for k in ops):
        beyond = np.array([[(len(ops) - 1) * R + H, 0]], dtype=np.int32)
        with pytest.raises(lib.DmfError, match='outside the padded scene'):
            lib.check_xy_bounds(shape, atA, atB, beyond)


def test_the_slot_draw_is_pinned():
    from dmf import augment
    for draw in (aug_ref.draw, augment.draw_slots):
        pts = np.array([(0, 0), (0, 1), (1, 0), (144, 144), (7, 99)])
        assert draw(123, 0, pts, 8).tolist() == [6, 5, 3, 4, 3]
        assert [int(draw(123, e, pts[4:], 8)[0]) for e in range(6)] == [3, 5, 2, 2, 1, 2]
        assert [int(draw(123, e, pts[4:], 4)[0]) for e in range(6)] == [3, 1, 2, 2, 1, 2]
        assert np.bincount(draw(123, 0, aug_ref.all_pixels(37, 41), 8), minlength=8).tolist() == [184, 203, 215, 197, 171, 204, 176, 167]
        for V in (4, 8):
            assert set(draw(123, 0, aug_ref.all_pixels(H, W), V).tolist()) == set(range(V))
    xy = aug_ref.all_pixels(37, 41)
    for seed, epoch, V in ((123, 0, 8), (3407, 17, 4), (0, 0, 8), (2 ** 31, 999, 3)):
        assert np.array_equal(aug_ref.draw(seed, epoch, xy, V), augment.draw_slots(seed, epoch, xy, V))


def test_keys_and_ops():
    from dmf import augment
    assert augment.augment_keys({}) == ((0,), (0,))
    assert augment.augment_keys({'schedule': {'augment': 'none'}, 'test': {'tta': None}}) == ((0,), (0,))
    assert augment.augment_keys({'schedule': {'augment': 'flips'}, 'test': {'tta': 'd4'}}) == (aug_ref.FLIPS, aug_ref.D4)
    assert augment.union_ops(aug_ref.FLIPS, (0,)) == aug_ref.FLIPS and augment.union_ops(aug_ref.FLIPS, aug_ref.D4) == aug_ref.D4
    assert augment.keys_in_use({'test': {'tta': 'flips'}}) == ['test.tta']
    for bad in ('rot', 'D4', 'flip'):
        with pytest.raises(ValueError, match='schedule.augment'):
            augment.augment_keys({'schedule': {'augment': bad}})
    for bad in ((1, 2), (0, 0), (0, 8), ()):
        with pytest.raises(ValueError, match='start with 0'):
            augment.ops_of(bad)


def test_config_yml_states_the_keys_commented():
    import yaml
    text = open(os.path.join(REPO, 'dual-modal-fusion_amd', 'config.yml')).read()
    for key in ('augment', 'tta'):
        assert '  # %s: none' % key in text
    cfg = yaml.safe_load(text)
    assert 'augment' not in cfg['schedule'] and 'tta' not in cfg['test']                # commented: absent, the neutral default


def test_tostagesolver_refuses_both_keys_by_name():
    from solver.tostagesolver import toStageSolver
    base = {'loss': 'qua_loss', 'optimizer': 'ADAM', 'lr': 1e-3}
    with pytest.raises(ValueError, match=r'schedule\.augment is out of scope for toStageSolver'):
        toStageSolver({'Categories_Number': 5, 'schedule': dict(base, augment='d4')})
    with pytest.raises(ValueError, match=r'test\.tta is out of scope for toStageSolver'):
        toStageSolver({'Categories_Number': 5, 'schedule': dict(base), 'test': {'tta': 'flips'}})


# ---------------------------------------------------------------------------------------------- the solver, without a GPU
class FakeAtlas:
    def __init__(self, scene, patch, scale, ops):
        from dmf import augment
        self.ops, self.patch, self.scale = tuple(ops), patch, scale
        self.extent = scene.extent
        self.slot_rows = augment.atlas_geometry(*scene.extent, self.ops)[0]

    def map_xy(self, xy, slot):
        from dmf import augment
        return augment.map_xy(xy, slot, self.ops, self.extent, self.patch, self.slot_rows)


class FakeScene:
    """dmf.engine.Scene without the device: what BaseSolver does with it is on the host."""
    def __init__(self, primary, aux, device, half=False):
        self.extent = tuple(primary.shape[:2])

    def atlas(self, patch, scale, ops):
        return FakeAtlas(self, patch, scale, ops)


class FakeEngine:
    """Records what `_train_epoch_fast` hands the train engine."""
    def __init__(self):
        self.plans, self.shorts, self.lr, self.b1, self.b2, self.optim = [], [], 0.0, 0.9, 0.999, 'ADAM'
        self.loss = torch.zeros(1024)

    def load_plan(self, xy, lab):
        self.plans.append((xy.clone(), lab.clone()))

    def run_plan(self, n, spg):
        self.n = n

    def losses(self):
        return torch.zeros(self.n)

    def step(self, xy, lab):
        self.shorts.append((xy.clone(), lab.clone()))


def _solver(golden_dir, tmp, monkeypatch, **keys):
    import dmf.engine
    from solver.mainsolver import Solver
    from test_gpu_trajectory import _setup
    monkeypatch.setattr(dmf.engine, 'Scene', FakeScene)
    _, cfg = _setup(golden_dir, tmp, fast_path=1, seed=123)
    if 'augment' in keys:
        cfg['schedule']['augment'] = keys['augment']
    if 'tta' in keys:
        cfg['test']['tta'] = keys['tta']
    torch.manual_seed(3407)
    s = Solver(cfg)
    s.DEVICE = 'cpu'                                     # (only `_step_short`'s .to(device) reads it from here on)
    s.dataloader()
    return s, cfg


def _epoch(s):
    s.engine = FakeEngine()
    s.epoch = 1
    s._set_epoch_hparams = lambda e: None
    s._train_epoch_fast()
    xy = torch.cat([p[0] for p in s.engine.plans] + [p[0] for p in s.engine.shorts])
    lab = torch.cat([p[1] for p in s.engine.plans] + [p[1] for p in s.engine.shorts])
    return xy.numpy(), lab.numpy(), torch.rand(4)


def test_none_leaves_the_scene_plain_and_the_union_of_the_keys_builds_the_atlas(golden_dir, monkeypatch):
    tmp = tempfile.mkdtemp(prefix='dmf_aug_')
    try:
        for n, (keys, ops) in enumerate((({}, None), (dict(augment='none', tta='none'), None), (dict(augment='flips'), aug_ref.FLIPS),
                                         (dict(tta='d4'), aug_ref.D4), (dict(augment='flips', tta='d4'), aug_ref.D4),
                                         (dict(augment='d4', tta='flips'), aug_ref.D4))):
            s, cfg = _solver(golden_dir, os.path.join(tmp, str(n)), monkeypatch, **keys)
            if ops is None:
                assert type(s.scene) is FakeScene
            else:
                assert type(s.scene) is FakeAtlas and s.scene.ops == ops
                assert (s.scene.patch, s.scene.scale) == (cfg['patch_size'], int(cfg.get('scale', 4)))
    finally:
        shutil.rmtree(tmp)


def test_an_augmented_epoch_keeps_batch_order_labels_and_the_rng_stream(golden_dir, monkeypatch):
    tmp = tempfile.mkdtemp(prefix='dmf_aug_')
    try:
        plain, cfg = _solver(golden_dir, os.path.join(tmp, 'a'), monkeypatch)
        xy0, lab0, rng0 = _epoch(plain)
        aug, _ = _solver(golden_dir, os.path.join(tmp, 'b'), monkeypatch, augment='d4')
        xy1, lab1, rng1 = _epoch(aug)
        assert len(xy0) == len(plain.train_index_loader.dataset) > cfg['batchsize']
        assert np.array_equal(lab0, lab1) and torch.equal(rng0, rng1)
        sc = aug.scene
        slots = aug_ref.draw(cfg['seed'], 1, xy0, 8)
        assert len(set(slots.tolist())) == 8
        assert np.array_equal(xy1, aug_ref.map_xy(xy0, slots, aug_ref.D4, *sc.extent, cfg['patch_size'], sc.slot_rows))
        # the same epoch as a row of an epoch block: `_enqueue_block` maps with the same draw
        torch.manual_seed(11)
        stream = plain._epoch_streams(1)[0][0]
        assert np.array_equal(aug._augment_xy(stream, 4).numpy(),
                              aug_ref.map_xy(stream.numpy(), aug_ref.draw(cfg['seed'], 4, stream.numpy(), 8), aug_ref.D4, *sc.extent,
                                             cfg['patch_size'], sc.slot_rows))
    finally:
        shutil.rmtree(tmp)


# ---------------------------------------------------------------------------------------------- the guards of the TTA case
def test_the_tta_case_meets_its_guards_on_the_oracle_alone():
    """tests/test_gpu_augment.py compares class maps outside a top-2 margin of 1e-4 of the oracle's mean logits: the oracle
    alone leaves at most 15 % of the pixels inside it (parity_cases.MARGIN_CAP) and predicts at least four classes."""
    from aug_cases import tta_case
    from parity_cases import MARGIN_CAP
    c = tta_case()
    assert 1.0 - c['safe'].float().mean().item() <= MARGIN_CAP
    assert len(set(c['pred'].tolist())) >= 4
    # the variants differ: the test would prove nothing on a symmetric net
    assert max((c['per_variant'][0] - l).abs().max().item() for l in c['per_variant'][1:]) > 1e-3
