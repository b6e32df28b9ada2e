"""The denominator of the criterion, D = sum_j w[y_j] over the N labels of one global batch, in the order the kernels take
(csrc/dmf_ce_math.h: ce_denominator), restated on the CPU in float64: thread t of 256 adds w[y_j] for j = t, t + 256, ... from 0.0
upwards, then the fixed tree `for w in 128, 64, ..., 1: red[t] += red[t + w] for t < w`.  Every addition is one IEEE float64
addition in both statements, so the result is the kernel's bits.  A plain module: no GPU, nothing of the HIP library."""
import numpy as np

THREADS = 256


def clamp_labels(labels, K):
    return np.clip(np.asarray(labels, dtype=np.int64), 0, K - 1)


def denominator(labels, K, class_w=None):
    """D of one row of labels (any int array) as a Python float; class_w: K float32 weights, None = ones."""
    y = clamp_labels(labels, K).reshape(-1)
    w = np.ones(K, dtype=np.float32) if class_w is None else np.asarray(class_w, dtype=np.float32).reshape(-1)
    assert w.size == K
    terms = w.astype(np.float64)[y]
    red = np.zeros(THREADS, dtype=np.float64)
    for j0 in range(0, terms.size, THREADS):          # pass j0 / 256 of the strided loop: thread t adds term j0 + t
        part = terms[j0:j0 + THREADS]
        red[:part.size] = red[:part.size] + part
    width = THREADS // 2
    while width > 0:
        red[:width] = red[:width] + red[width:2 * width]
        width //= 2
    return float(red[0])


def denominators(labels, N, K, class_w=None):
    """One D per row of N labels -> float64 array [rows]."""
    rows = np.asarray(labels).reshape(-1, N)
    return np.array([denominator(r, K, class_w) for r in rows], dtype=np.float64)
