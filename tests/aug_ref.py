"""numpy statement of the augmentation geometry, for the tests: variant, atlas, coordinate map, slot draw.
No GPU and nothing of the library: the functions here are written from the definition, one element or one sample at a time.
"""
import numpy as np

FLIPS = (0, 1, 2, 3)
D4 = (0, 1, 2, 3, 4, 5, 6, 7)
M64 = (1 << 64) - 1


def tf(X, k):
    """Variant k of X [rows, cols, ...]: transpose if k & 4, then reverse the rows if k & 2, then the columns if k & 1."""
    Y = np.swapaxes(X, 0, 1) if k & 4 else X
    if k & 2:
        Y = Y[::-1]
    if k & 1:
        Y = Y[:, ::-1]
    return Y


def geometry(Hp, Wp, ops):
    """(slot rows R, pitch Wq)."""
    if any(k & 4 for k in ops):
        return max(Hp, Wp), max(Hp, Wp)
    return Hp, Wp


def atlas(X, rows, cols, ops, slot_rows, pitch):
    """[len(ops) * slot_rows, pitch, C]: slot s holds tf(X[:rows, :cols], ops[s]) at its top-left corner, zero elsewhere."""
    out = np.zeros((len(ops) * slot_rows, pitch) + X.shape[2:], dtype=X.dtype)
    for s, k in enumerate(ops):
        Y = tf(X[:rows, :cols], k)
        out[s * slot_rows:s * slot_rows + Y.shape[0], :Y.shape[1]] = Y
    return out


def scene_atlases(A, Bm, P, S, ops):
    """(primary atlas, aux atlas, R) of the padded scenes A [Hp, Wp, C] and Bm [>= S Hp, >= S Wp, C2]."""
    Hp, Wp = A.shape[:2]
    R, Wq = geometry(Hp, Wp, ops)
    return atlas(A, Hp, Wp, ops, R, Wq), atlas(Bm, S * Hp, S * Wp, ops, S * R, S * Wq), R


def map_one(x, y, k, s, Hp, Wp, n, R):
    if k & 4:
        x, y, Hp, Wp = y, x, Wp, Hp
    if k & 2:
        x = Hp - n - x
    if k & 1:
        y = Wp - n - y
    return x + s * R, y


def map_xy(xy, slots, ops, Hp, Wp, n, R):
    """Atlas coordinates [n, 2] int32 of the patches at xy, sample i in slot slots[i] (variant ops[slots[i]])."""
    slots = np.broadcast_to(np.asarray(slots), (len(xy),))
    return np.array([map_one(int(x), int(y), ops[int(s)], int(s), Hp, Wp, n, R) for (x, y), s in zip(xy, slots)],
                    dtype=np.int32).reshape(-1, 2)


def draw_one(seed, epoch, x, y, V):
    z = (seed * 0x9E3779B97F4A7C15 + epoch * 0xBF58476D1CE4E5B9 + x * 0x94D049BB133111EB + y) & M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return (z >> 33) % V


def draw(seed, epoch, xy, V):
    return np.array([draw_one(int(seed), int(epoch), int(x), int(y), V) for x, y in xy], dtype=np.int64)


def all_pixels(H, W):
    return np.stack(np.meshgrid(np.arange(H), np.arange(W), indexing='ij'), -1).reshape(-1, 2).astype(np.int32)


def cut(A, Bm, xy, P, S):
    """Materialised patches a [n, C, P, P], b [n, C2, SP, SP] (numpy) of the padded scenes at top-left xy."""
    a = np.stack([A[x:x + P, y:y + P].transpose(2, 0, 1) for x, y in xy])
    b = np.stack([Bm[S * x:S * x + S * P, S * y:S * y + S * P].transpose(2, 0, 1) for x, y in xy])
    return a, b


def tf_patches(a, ks):
    """Patches [n, C, p, p], sample i transformed by variant ks[i] on its spatial axes."""
    return np.stack([np.ascontiguousarray(tf(p.transpose(1, 2, 0), int(k)).transpose(2, 0, 1)) for p, k in zip(a, ks)])
