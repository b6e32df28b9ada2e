"""Inputs, float64 references and bounds of the noise-adjusted band reduction: shared by
tests/test_noise_adjust_host.py (CPU) and tests/test_gpu_noise_adjust.py (GPU).  A plain module: no fixtures, no GPU, nothing of
the HIP library.  Every bound comes from the number formats and R = DMF_PCA_RUN, never from the kernel's output.

1. The noise moments.  For a direction with pixel step s, e_p = x[p] - x[p + s] for the pixels that have the neighbour, M of
   them, and ncov64 = sum_p e_p e_p^T / (2 M) in float64 from the EXACT differences of the fp32 x.  The kernel is held to
       |ncov_ij - ncov64_ij| <= (R + 4) 2^-24 A_ij,      A_ij = sum_p |e_pi| |e_pj| / (2 M).
   Why the covariance's bound carries over, with u = 2^-24: the kernel forms fl(e) = e (1 + t), |t| <= u — ONE fp32 rounding,
   and none at all where the two values are within a factor of two of each other (Sterbenz) — so a product fl(e_i) fl(e_j)
   is e_i e_j (1 + t_i)(1 + t_j), off by at most (2 u + u^2) |e_i e_j|.  The MFMA adds the (exact) products of a run of R pixels
   as one fmaf chain: R roundings at most on any term, (1 + u)^R - 1 <= R u (1 + R u) of sum |fl(e_i) fl(e_j)|.  Together
   (R + 2) u + (R^2 + 2 R + 1) u^2 + ..., and (R + 1)^2 u = 0.004 at R = 256: below (R + 2.01) u.  The sums of runs and slices and
   the division are in double: (runs + 2) 2^-53, below 0.001 u for any scene of fewer than 2^19 runs.  (R + 4) u holds all of
   it; the covariance's bound has the same slack, of which its reference (which takes the rounded d) uses less.

2. The fixture that separates the two transforms (smooth_scene): S = 4 spatially smooth abundance maps, each the bilinear
   upsample of a 5 x 5 standard-normal field, in 4 orthonormal spectral directions with amplitudes 4 2^(-k/2), under white
   per-band noise of standard deviation f_c (1 + 0.05 c), f_c = 1.5 on every third band and 0.4 on the others.  The loud bands
   carry most of the variance, so plain PCA's first four directions follow them; the noise-adjusted fit finds the signal.

3. The fixture of the end-to-end tests (noisy_scene): like pca_cases.scene a sum of components in orthonormal spectral
   directions plus offsets, min-max normalised — but a component is a smooth map here (the 10 lowest two-dimensional cosine
   modes of the scene, unit variance, orthogonal: the shift differences hardly see them), white noise of standard deviation
   sigma_c in 1 .. 1.5 is added PER PIXEL, and component k has the direction diag(sigma) q_k and the amplitude sqrt(nu_k - 1)
   with nu_k = 2 * 1.5^(9 - k): in the noise-whitened space the covariance is I + Q diag(nu - 1) Q^T, so the population's
   generalised eigenvalues are the nu_k, a factor 1.5 apart (what the differences do see of the maps, and the sample, move them
   a little).  The guards (asserted on the CPU, on the float64 fit alone): every consecutive ratio of the first K + 1 generalised
   eigenvalues at least MIN_RATIO = 1.3, and cond(ncov) <= MAX_COND = 100 (it is below 3).

4. The end-to-end tolerance, device route against reduce_host(noise=...), by Davis-Kahan on the whitened matrix.  The host has
   (cov, ncov), the device (cov + E, ncov + E_N) with |E| and |E_N| entrywise inside the moment bounds (of `both`, E_N is the
   mean of the two directions' bounds).  With ncov = U L U^T, F = U L^(-1/2) — so |F|_2^2 = |ncov^-1|_2 = 1 / min L — and
   Mw = F^T cov F, the device's pencil in the host's whitened coordinates is (Mw + D1, I + D2), D1 = F^T E F, D2 = F^T E_N F:
   |D1|_F <= |ncov^-1|_2 |E|_F, |D2|_F <= |ncov^-1|_2 |E_N|_F.  To first order eigenvector k of the pencil moves as under the
   symmetric perturbation D1 - nu_k D2 of Mw, orthogonally to y_k:
       dM = |ncov^-1|_2 (|E|_F + nu_1 |E_N|_F),     sin theta <= 2 dM / gap,     gap = the smallest of the first K gaps of nu,
   and ALONG y_k by -(y_k^T D2 y_k) / 2 y_k, since the device's vector has unit length under I + D2, not under I.  (The sketch
   that goes by the angle alone misses this term: it is first order too.)  So
       |b_k' - b_k|_2 <= |F|_2 (2 dM / gap + |D2|_F / 2),
   and the scores of pixel n differ by at most |d_n|_2 times that.  To this come the float32 roundings of the two bases
   (2 u sum_c |d_c| |b_ck|), the device's fp32 projection (pca_cases.project_ref's bound) and the host's cast of its scores to
   float32 (u |y|)."""
import functools

import numpy as np

import pca_cases as pca

U24 = 2.0 ** -24
MIN_RATIO, MAX_COND = 1.3, 100.0
DIRECTIONS = ('horizontal', 'vertical')
SOLVER_BANDS, SOLVER_K = pca.SOLVER_BANDS, pca.SOLVER_K

# (H, W) of the kernel tests: row ends inside a 64-pixel chunk and inside a run, a last partial chunk, W = 1 past a chunk
KERNEL_SCENES = ((2, 2), (3, 5), (4, 63), (4, 65), (3, 257), (70, 9), (1, 300), (300, 1))
KERNEL_BANDS = (1, 3, 24, 203)


def valid(direction, H, W):
    """Whether any pixel of an H x W scene has the neighbour of `direction` (M >= 1)."""
    return (W if direction == 'horizontal' else H) >= 2


def pixels(C, H, W, seed=0):
    """A scene [H, W, C] float32 for the kernel tests (read-only, cached): pca_cases.scene's recipe at H x W."""
    return pca.scene(C, H, W, seed)


# ------------------------------------------------------------------------------ 1. float64 reference and bound of the moments
def differences(x, direction):
    """e [M, C] float64: the exact differences of the fp32 scene x [H, W, C] for the pixels that have the neighbour."""
    x = np.asarray(x).astype(np.float64)
    e = x[:, :-1] - x[:, 1:] if direction == 'horizontal' else x[:-1] - x[1:]
    return e.reshape(-1, x.shape[2])


def noise_ref(x, direction, R):
    """x [H, W, C] float32 -> (ncov64 [C, C], bound [C, C]): |ncov - ncov64| <= (R + 4) 2^-24 A (module text, 1)."""
    e = differences(x, direction)
    M = e.shape[0]
    return e.T @ e / (2.0 * M), (R + 4) * U24 * (np.abs(e).T @ np.abs(e)) / (2.0 * M)


def noise_ref_of(x, noise, R):
    """The same for a value of band_reduce_noise: of `both`, the mean of the two directions' references and bounds."""
    parts = [noise_ref(x, d, R) for d in (DIRECTIONS if noise == 'both' else (noise,))]
    return sum(p[0] for p in parts) / len(parts), sum(p[1] for p in parts) / len(parts)


# ------------------------------------------------------------------------------ smooth maps
def bilinear(field, H, W):
    """The bilinear upsample [H, W] of a coarse field [g, g]: its corners are the scene's corners."""
    g = field.shape[0]

    def weights(n):
        t = np.linspace(0.0, g - 1.0, n)
        return np.maximum(0.0, 1.0 - np.abs(t[:, None] - np.arange(g)[None, :]))
    return weights(H) @ field @ weights(W).T


def smooth_maps(rng, S, H, W, g):
    return np.stack([bilinear(rng.standard_normal((g, g)), H, W) for _ in range(S)], axis=-1)          # [H, W, S]


# ------------------------------------------------------------------------------ 2. the fixture that separates the transforms
SEPARATION_SEED = 0
SEPARATION_SCENES = ((24, 24), (40, 40))
SEPARATION_BANDS, SEPARATION_SIGNALS = 24, 4


@functools.lru_cache(maxsize=None)
def smooth_scene(H, W, seed=SEPARATION_SEED):
    """-> (scene [H, W, 24] float32, signal directions Q [24, 4] orthonormal), module text 2."""
    C, S = SEPARATION_BANDS, SEPARATION_SIGNALS
    rng = np.random.default_rng(seed)
    Q = np.linalg.qr(rng.standard_normal((C, S)))[0]
    amp = 4.0 * 2.0 ** (-0.5 * np.arange(S))
    signal = (smooth_maps(rng, S, H, W, 5) * amp) @ Q.T
    sigma = np.where(np.arange(C) % 3 == 0, 1.5, 0.4) * (1.0 + 0.05 * np.arange(C))
    X = np.ascontiguousarray(signal + rng.standard_normal((H, W, C)) * sigma, dtype=np.float32)
    X.setflags(write=False)
    return X, Q


def largest_angle(A, B):
    """The largest principal angle, in degrees, between the column spaces of A and B (same number of columns)."""
    qa, qb = np.linalg.qr(A)[0], np.linalg.qr(B)[0]
    s = np.linalg.svd(qa.T @ qb, compute_uv=False)
    return float(np.degrees(np.arccos(np.clip(s.min(), 0.0, 1.0))))


# ------------------------------------------------------------------------------ 3. the fixture of the end-to-end tests
NOISY_SIGNALS, NOISY_FLOOR, NOISY_STEP = 10, 2.0, 1.5


def cosine_maps(S, H, W):
    """[H, W, S]: the S lowest two-dimensional cosine modes after the constant, lowest first, each of unit variance — smooth
    (the shift differences hardly see them) and orthogonal over the scene."""
    modes = sorted(((a * a + b * b, a, b) for a in range(S + 1) for b in range(S + 1) if a + b > 0))[:S]
    i, j = (np.arange(H) + 0.5) / H, (np.arange(W) + 0.5) / W
    maps = [np.outer(np.cos(np.pi * a * i), np.cos(np.pi * b * j)) for _, a, b in modes]
    return np.stack([(m - m.mean()) / m.std() for m in maps], axis=-1)


@functools.lru_cache(maxsize=None)
def noisy_scene(C=SOLVER_BANDS, H=pca.H_SCENE, W=pca.W_SCENE, seed=0):
    """The scene [H, W, C] float32 in [0, 1] (read-only) of module text 3."""
    rng = np.random.default_rng(7000 + 1000 * seed + C)
    S = NOISY_SIGNALS
    sigma = rng.uniform(1.0, 1.5, C)
    nu = NOISY_FLOOR * NOISY_STEP ** np.arange(S - 1, -1, -1.0)
    Q = np.linalg.qr(rng.standard_normal((C, S)))[0]
    signal = (cosine_maps(S, H, W) * np.sqrt(nu - 1.0)) @ (sigma[:, None] * Q).T
    X = signal + rng.standard_normal((H, W, C)) * sigma + rng.uniform(-1.0, 1.0, C) * 10.0
    X = (X - X.min()) / (X.max() - X.min())
    X = np.ascontiguousarray(X, dtype=np.float32)
    X.setflags(write=False)
    return X


def guards(x, noise, K):
    """(the K consecutive ratios of the first K + 1 generalised eigenvalues, cond(ncov)) of the float64 fit of x [H, W, C]."""
    from utils import spectral
    H, W, C = x.shape
    _, cov = spectral.moments_host(x.reshape(-1, C))
    ncov = spectral.noise_moments_host(x, noise)
    nu = spectral.fit_noise_adjusted(np.zeros(C), cov, ncov, C, noise=noise)['eigenvalues']
    nl = np.linalg.eigvalsh(ncov)
    return nu[:K] / nu[1:K + 1], nl[-1] / nl[0]


@functools.lru_cache(maxsize=None)
def solver_scene(K_classes, H=40, W=40, seed=1):
    """(primary [H, W, 24] float32, aux [H, W] float32, label [H, W] uint8): pca_cases.solver_scene with the noisy scene."""
    _, aux, label = pca.solver_scene(K_classes, H, W, seed)
    return noisy_scene(SOLVER_BANDS, H, W, seed), aux, label


# ------------------------------------------------------------------------------ 4. the end-to-end tolerance
def route_tolerance(x, noise, K, basis, R):
    """-> (tolerance on |scores_device - scores_host|, dict of its parts) for the normalised scene x [H, W, C] float32 and the
    host's float32 basis [C, K]; module text 4.  Everything from the float64 references and the moment bounds."""
    from utils import spectral
    H, W, C = x.shape
    flat = x.reshape(-1, C)
    mean64, cov64, _, cov_tol = pca.moments_ref(flat, R)
    d = spectral.centred(flat, mean64)
    # (pca_cases.moments_ref takes the fp32-rounded d; the host's covariance takes the exact one: 2 u A apart at most)
    E = cov_tol + (2.0 * U24 + U24 ** 2) * (np.abs(d).T @ np.abs(d)) / (flat.shape[0] - 1)
    ncov64, E_N = noise_ref_of(x, noise, R)
    nl = np.linalg.eigvalsh(ncov64)
    inv = 1.0 / nl[0]                                                   # |ncov^-1|_2 = |F|_2^2
    nu = spectral.fit_noise_adjusted(mean64, spectral.moments_host(flat)[1], ncov64, C, noise=noise)['eigenvalues']
    gap = np.min(nu[:K] - nu[1:K + 1])
    dM = inv * (np.linalg.norm(E) + nu[0] * np.linalg.norm(E_N))
    sin_theta = 2.0 * dM / gap
    length = 0.5 * inv * np.linalg.norm(E_N)
    db = np.sqrt(inv) * (sin_theta + length)
    y64, proj = pca.project_ref(flat, mean64, basis)
    rounding = 2.0 * U24 * (np.abs(d) @ np.abs(basis.astype(np.float64))).max() + U24 * np.abs(y64).max()
    tol = db * np.linalg.norm(d, axis=1).max() + proj.max() + rounding
    return tol, dict(sin_theta=sin_theta, length=length, basis=db, gap=gap, nu=nu[:K + 1], cond=nl[-1] / nl[0], dM=dM,
                     E_N=np.linalg.norm(E_N))
