"""The test-time-augmentation case shared by tests/test_augment_host.py (its guards, on the oracle alone) and
tests/test_gpu_augment.py: the recipe of tests/parity_cases.py — seed-0 oracle net with 0.05 noise, torch.rand scene, every pixel
of the scene once — with the head centred on the oracle's MEAN logits over the eight dihedral variants, so that the class of
the mean is decided by the patches and not by the biases.  A plain module: no fixtures, no GPU, nothing of the HIP library.
"""
import functools

import numpy as np
import torch

import aug_ref
from parity_cases import build_cfg, centre_head, class_guards, oracle_net
from test_gpu_parity import SHAPES, _scene as rand_scene

TTA_NAME, TTA_H, TTA_W, TTA_SEED = 'tiny', 23, 19, 5      # S = 4: the aux atlas carries weight; 437 pixels


def variant_patches(A, Bm, xy, P, S, ks):
    """The materialised patches of the pixels xy, sample i transformed by variant ks[i] (torch, contiguous)."""
    a, b = aug_ref.cut(A.numpy(), Bm.numpy(), xy, P, S)
    return torch.from_numpy(aug_ref.tf_patches(a, ks)), torch.from_numpy(aug_ref.tf_patches(b, ks))


def mean_logits(per_variant):
    """(((l_0 + l_1) + l_2) + ...) / V in fp32: the expression dmf_logits_mean states."""
    total = per_variant[0].clone()
    for l in per_variant[1:]:
        total = total + l
    return total / float(len(per_variant))


def oracle_variant_logits(ref, A, Bm, xy, P, S, ops):
    with torch.no_grad():
        return [ref(*variant_patches(A, Bm, xy, P, S, np.full(len(xy), k))) for k in ops]


@functools.lru_cache(maxsize=None)
def tta_case(name=TTA_NAME, H=TTA_H, W=TTA_W, seed=TTA_SEED):
    C, C2, P, S, K = SHAPES[name]
    cfg = build_cfg(name)
    ref = oracle_net(cfg)
    A, Bm = rand_scene(name, H, W, seed)
    xy = aug_ref.all_pixels(H, W)
    centre_head(ref, mean_logits(oracle_variant_logits(ref, A, Bm, xy, P, S, aug_ref.D4)))
    per_variant = oracle_variant_logits(ref, A, Bm, xy, P, S, aug_ref.D4)
    mean = mean_logits(per_variant)
    pred, safe = class_guards(mean, '[tta %s %dx%d seed %d]' % (name, H, W, seed))     # >= 4 classes, margin cap 15 %
    return dict(name=name, cfg=cfg, ref=ref, state={k: v.detach().clone() for k, v in ref.state_dict().items()}, A=A, Bm=Bm,
                xy=xy, H=H, W=W, P=P, S=S, K=K, per_variant=per_variant, mean=mean, pred=pred, safe=safe)
