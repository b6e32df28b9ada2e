"""Inputs of the band-reduction tests: shared by tests/test_band_reduce_host.py (CPU) and
tests/test_gpu_band_reduce.py (GPU).  A plain module: no fixtures, no GPU, nothing of the HIP library.

The scene is X = (Z diag(2^(-k/2))) Q^T + offsets, min-max normalised, float32: Z seeded standard normal [H W, C], Q the
orthogonal factor of a seeded normal matrix, offsets seeded per band.  Its population eigenvalues are 2^-k, a factor of 2 apart,
so the basis is well defined as far as a test asks for it (the guard: every consecutive ratio among the first K + 1 sample
eigenvalues is >= 1.5).  The project's own synth.make_scene will not do: beyond its 16 class prototypes its spectrum is
degenerate and the eigenvectors are anybody's.

Also here: the row the issue adds to the patch kernel's table, registered under the name 'pca32' with the existing parity
machinery (tests/parity_cases.py), and the float64 references of the two kernels with the bounds the tests hold them to."""
import functools

import numpy as np

H_SCENE, W_SCENE = 37, 41
KERNEL_BANDS = (1, 3, 24, 200, 203)
SOLVER_BANDS, SOLVER_K = 24, 8
MIN_RATIO = 1.5


@functools.lru_cache(maxsize=None)
def scene(C, H=H_SCENE, W=W_SCENE, seed=0):
    """The fixture scene [H, W, C] float32 in [0, 1] (read-only)."""
    rng = np.random.default_rng(1000 * seed + C)
    Z = rng.standard_normal((H * W, C)) * 2.0 ** (-0.5 * np.arange(C))
    Q = np.linalg.qr(rng.standard_normal((C, C)))[0]
    X = Z @ Q.T + rng.uniform(-1.0, 1.0, C)
    X = (X - X.min()) / (X.max() - X.min())
    X = np.ascontiguousarray(X.reshape(H, W, C), dtype=np.float32)
    X.setflags(write=False)
    return X


def eigen_ratios(X, n):
    """The n consecutive ratios of the first n + 1 sample eigenvalues of the pixels of X (float64)."""
    x = X.reshape(-1, X.shape[-1]).astype(np.float64)
    lam = np.linalg.eigvalsh(np.cov(x, rowvar=False).reshape(x.shape[1], x.shape[1]))[::-1]
    return lam[:n] / lam[1:n + 1]


# ------------------------------------------------------------------------------ float64 references and bounds
def moments_ref(x, R):
    """x [N, C] float32 -> (mean64, cov64, mean bound, cov bound [C, C]) as the issue states them:
    |mean - mean64| <= 2^-50 N max|x|;  |cov_ij - cov64_ij| <= (R + 4) 2^-24 A_ij + 2^-48 |m_i m_j|,
    A_ij = sum_n |d_ni| |d_nj| / (N - 1), d = x - float32(mean64) formed in fp32, everything else in float64."""
    N = x.shape[0]
    x64 = x.astype(np.float64)
    mean = x64.mean(axis=0)
    d = (x - mean.astype(np.float32)).astype(np.float64)          # the fp32 subtraction, widened
    cov = d.T @ d / (N - 1)
    A = np.abs(d).T @ np.abs(d) / (N - 1)
    return mean, cov, 2.0 ** -50 * N * np.abs(x64).max(), (R + 4) * 2.0 ** -24 * A + 2.0 ** -48 * np.abs(np.outer(mean, mean))


def project_ref(x, mean, basis):
    """-> (y64 [N, K], bound [N, K]): |y - y64| <= (C + 3) 2^-24 sum_c |x_c - m_c| |basis_ck|, m = float32(mean)."""
    d = (x - np.asarray(mean, dtype=np.float64).astype(np.float32)).astype(np.float64)
    b = basis.astype(np.float64)
    return d @ b, (x.shape[1] + 3) * 2.0 ** -24 * (np.abs(d) @ np.abs(b))


# ------------------------------------------------------------------------------ the solver's scene
@functools.lru_cache(maxsize=None)
def solver_scene(K_classes, H=40, W=40, seed=1):
    """(primary [H, W, 24] float32, aux [H, W] float32, label [H, W] uint8 in 1..K_classes - 1 with a tenth unlabelled):
    the fixture scene at 40 x 40, an aux scene at scale 1 and seeded labels."""
    rng = np.random.default_rng(seed)
    aux = rng.random((H, W)).astype(np.float32)
    label = rng.integers(1, K_classes, (H, W)).astype(np.uint8)
    label[rng.random((H, W)) < 0.1] = 0
    return scene(SOLVER_BANDS, H, W, seed), aux, label


# ------------------------------------------------------------------------------ the 32-band row of the patch kernel
ROW = 'pca32'
ROW_SHAPE = (32, 1, 11, 1, 17)          # (C, C2, P, S, K) as tests/test_gpu_parity.py::SHAPES lists its rows
ROW_BATCHES = (255, 257)
# (B, half) -> seed of the case where the default misses a guard of tests/parity_cases.py (the guards stay)
ROW_SEEDS = {(255, False): 6, (255, True): 7, (257, True): 7}


def register_row():
    """Makes 'pca32' a name tests/parity_cases.py::case understands (its tables are plain dicts keyed by row name)."""
    import parity_cases as pc
    from test_gpu_parity import SHAPES
    SHAPES.setdefault(ROW, ROW_SHAPE)
    for (B, half), seed in ROW_SEEDS.items():
        pc.SEEDS.setdefault((ROW, B, half, False), seed)
    return pc
