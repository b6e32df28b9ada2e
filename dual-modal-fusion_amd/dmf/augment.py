"""Flip / rotate augmentation as a re-indexing of the resident scene: the geometry, on the host.

Variant k in 0..7 of an array X [rows, cols, ...]: transpose the two leading axes if k & 4, then reverse the rows if k & 2,
then the columns if k & 1.  A scene atlas (dmf.engine.Scene.atlas, dmf_scene_atlas) stacks the variants `ops` of the padded
scene along the row axis; a patch of variant k is then an ordinary patch of the atlas at the coordinate `map_xy` gives.
Nothing here touches the GPU library: numpy, and torch only where a tensor is passed in.
"""
import numpy as np

OPS = {'none': (0,), 'flips': (0, 1, 2, 3), 'd4': (0, 1, 2, 3, 4, 5, 6, 7)}

_M64 = (1 << 64) - 1
_C0, _C1, _C2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


def ops_of(key, what='augment'):
    """The ops list of a config value: None / 'none' / 'flips' / 'd4', or an explicit sequence that starts with 0."""
    if key is None:
        return OPS['none']
    if isinstance(key, str):
        if key not in OPS:
            raise ValueError('%s: %r is not one of %s' % (what, key, sorted(OPS)))
        return OPS[key]
    ops = tuple(int(k) for k in key)
    if not ops or ops[0] != 0 or len(set(ops)) != len(ops) or len(ops) > 8 or min(ops) < 0 or max(ops) > 7:
        raise ValueError('%s: ops %r must be distinct values of 0..7 that start with 0' % (what, key))
    return ops


def union_ops(*lists):
    """One ops list (0 first, ascending) that holds every op of the given lists."""
    return tuple(sorted(set(k for ops in lists for k in ops)))


def atlas_geometry(Hp, Wp, ops):
    """(slot rows R, pitch Wq) of an atlas of a padded scene [Hp, Wp]: the scene's own without a transposed op, else square."""
    if any(k & 4 for k in ops):
        return max(Hp, Wp), max(Hp, Wp)
    return Hp, Wp


def tf(x, k):
    """Variant k of a numpy array or torch tensor whose two LEADING axes are (row, col)."""
    if k & 4:
        x = x.transpose(1, 0, *range(2, x.ndim)) if isinstance(x, np.ndarray) else x.transpose(0, 1)
    if k & 2:
        x = x[::-1] if isinstance(x, np.ndarray) else x.flip(0)
    if k & 1:
        x = x[:, ::-1] if isinstance(x, np.ndarray) else x.flip(1)
    return x


def map_xy(xy, slot, ops, extent, window, slot_rows):
    """Top-left coordinates in the atlas of the patches whose top-left in the scene is xy [n, 2] (x = row, y = col), each in
    the slot `slot` (an array [n] or a scalar).  extent = (Hp, Wp) of the padded primary scene, window = the patch size.
    numpy in, numpy int32 out; a torch int32 tensor in, a tensor on its device out."""
    Hp, Wp = extent
    if isinstance(xy, np.ndarray) or not hasattr(xy, 'device'):
        xy = np.asarray(xy)
        s = np.broadcast_to(np.asarray(slot, dtype=np.int64), (xy.shape[0],))
        k = np.asarray(ops, dtype=np.int64)[s]
        x, y = xy[:, 0].astype(np.int64), xy[:, 1].astype(np.int64)
        where, stack = np.where, lambda a, b: np.stack([a, b], 1).astype(np.int32)
    else:
        import torch
        s = torch.as_tensor(slot, device=xy.device).to(torch.int64).expand(xy.shape[0])
        k = torch.as_tensor(ops, dtype=torch.int64, device=xy.device)[s]
        x, y = xy[:, 0].to(torch.int64), xy[:, 1].to(torch.int64)
        where, stack = torch.where, lambda a, b: torch.stack([a, b], 1).to(torch.int32).contiguous()
    t = (k & 4) != 0
    x, y = where(t, y, x), where(t, x, y)
    h, w = where(t, Wp + 0 * k, Hp + 0 * k), where(t, Hp + 0 * k, Wp + 0 * k)
    x = where((k & 2) != 0, h - window - x, x)
    y = where((k & 1) != 0, w - window - y, y)
    return stack(x + s * slot_rows, y)


def draw_slots(seed, epoch, xy, V):
    """The slot in 0..V-1 of every sample of an epoch: a stateless 64-bit mix (splitmix64's finaliser) of the seed, the epoch and
    the pixel's coordinates xy [n, 2], so every rank, every route and a resumed run draw the same, and torch's RNG stream is
    not touched."""
    xy = np.asarray(xy)
    with np.errstate(over='ignore'):
        x, y = xy[:, 0].astype(np.uint64), xy[:, 1].astype(np.uint64)
        base = np.uint64(((int(seed) * _C0) + (int(epoch) * _C1)) & _M64)
        z = base + x * np.uint64(_C2) + y
        z ^= z >> np.uint64(30)
        z *= np.uint64(_C1)
        z ^= z >> np.uint64(27)
        z *= np.uint64(_C2)
        z ^= z >> np.uint64(31)
    return ((z >> np.uint64(33)) % np.uint64(V)).astype(np.int64)


def augment_keys(cfg):
    """(ops of `schedule.augment`, ops of `test.tta`) of a config; (0,) where the key is absent, null or `none`."""
    return (ops_of((cfg.get('schedule') or {}).get('augment'), 'schedule.augment'),
            ops_of((cfg.get('test') or {}).get('tta'), 'test.tta'))


def keys_in_use(cfg):
    """The names of the two keys that ask for more than the identity."""
    aug, tta = augment_keys(cfg)
    return [name for name, ops in (('schedule.augment', aug), ('test.tta', tta)) if len(ops) > 1]


def tf_batch(data, ks):
    """A batch of patches [n, C, p, p] (torch), sample i replaced by variant ks[i] of itself on its two spatial axes: what the
    drop-in path feeds the net where the fast path reads the atlas at the mapped coordinate."""
    out = data.clone()
    ks = np.asarray(ks)
    for k in np.unique(ks):
        if k:
            idx = np.nonzero(ks == k)[0]
            out[idx] = tf(data[idx].permute(2, 3, 0, 1), int(k)).permute(2, 3, 0, 1)
    return out
