"""utils.spectral — the host side of `band_reduce: pca`: the config keys, the fit of the basis from the band
moments in float64, and for `fast_path: 0` (and as the tests' reference) the whole pipeline in numpy float64.  Nothing here
touches the GPU library.

The pipeline, on either route:
    x      = float32(to_tensor(scene))                        the scene's global min-max, as every scene is normalised
    mean   = the band means of x                              float64
    d      = x - float32(mean)                                the centred pixel of every later stage
    cov    = d^T d / (N - 1)                                  [C, C]
    basis  = fit_basis(mean, cov, K, whiten)                  [C, K] float32
    scores = d basis                                          [H, W, K] float32: the scene the solver goes on with
The device route (dmf.engine.band_reduce) forms d and its products in fp32 and the sums over runs of pixels in double
(include/dmf.h); this module does everything after x in float64.
`band_reduce_noise` replaces fit_basis by the noise-adjusted fit of the second half of this file."""
import numpy as np

KINDS = ('none', 'pca')


def band_keys(cfg):
    """-> dict(kind, bands, whiten) from the optional top-level keys
         band_reduce none / pca (default none)    band_reduce_bands >= 1 (default 32)    band_reduce_whiten 0 / 1 (default 0)
    `kind` is None or 'pca'.  Neutral values change nothing."""
    kind = cfg.get('band_reduce', 'none')
    kind = 'none' if kind is None or kind is False or kind == 0 else str(kind).lower()
    if kind not in KINDS:
        raise ValueError('band_reduce %r is not one of %s' % (cfg.get('band_reduce'), ' / '.join(KINDS)))
    bands = cfg.get('band_reduce_bands', 32)
    if isinstance(bands, bool) or not isinstance(bands, int) or bands < 1:
        raise ValueError('band_reduce_bands %r is not a whole number >= 1' % (bands,))
    whiten = cfg.get('band_reduce_whiten', 0) or 0
    if whiten not in (0, 1, True, False):
        raise ValueError('band_reduce_whiten is 0 or 1')
    return dict(kind=None if kind == 'none' else kind, bands=bands, whiten=bool(whiten))


def keys_in_use(keys):
    """The names of the keys that are not neutral, for a refusal."""
    return ['band_reduce'] if keys['kind'] is not None else []


def check_bands(K, C):
    if K > C:
        raise ValueError('band_reduce_bands: %d exceeds the %d bands of the scene' % (K, C))


def sign_columns(vec):
    """Every column signed so that its component of largest magnitude — the first such on a tie — is positive."""
    big = np.argmax(np.abs(vec), axis=0)                   # the first maximal index
    return vec * np.where(vec[big, np.arange(vec.shape[1])] < 0, -1.0, 1.0)[None, :]


def fit_basis(mean, cov, K, whiten=False):
    """-> dict(mean [C] float64, basis [C, K] float32, eigenvalues [K] float64, explained [K] float64) from the band means and
    the covariance [C, C] (symmetric; its upper triangle is what numpy.linalg.eigh reads after the transpose below).  The
    eigenvalues are ordered descending; every eigenvector is signed so that its component of largest magnitude (the first such
    on a tie) is positive; explained[k] = eigenvalues[k] / trace(cov).  whiten: column k is divided by sqrt(eigenvalues[k]), so
    the scores have unit variance; an eigenvalue that is not positive is refused."""
    mean = np.asarray(mean, dtype=np.float64)
    cov = np.asarray(cov, dtype=np.float64)
    C = mean.shape[0]
    if cov.shape != (C, C):
        raise ValueError('fit_basis wants mean [C] and cov [C, C]')
    K = int(K)
    if K < 1:
        raise ValueError('band_reduce_bands %r is not a whole number >= 1' % (K,))
    check_bands(K, C)
    lam, vec = np.linalg.eigh(cov, UPLO='U')               # ascending
    lam, vec = lam[::-1][:K].copy(), vec[:, ::-1][:, :K].copy()
    vec = sign_columns(vec)
    if whiten:
        if not np.all(lam > 0):
            raise ValueError('band_reduce_whiten: eigenvalue %d of the first %d is %g, not positive; lower band_reduce_bands'
                             % (int(np.argmin(lam > 0)), K, lam[np.argmin(lam > 0)]))
        vec = vec / np.sqrt(lam)[None, :]
    return dict(mean=mean, basis=np.ascontiguousarray(vec, dtype=np.float32), eigenvalues=lam,
                explained=lam / np.trace(cov))


def normalise(scene):
    """float32(to_tensor(scene)): the pixels both routes start from (dmf_scene_prepare at pad 0 gives the same bits)."""
    from function.function import to_tensor
    return np.ascontiguousarray(to_tensor(np.asarray(scene)), dtype=np.float32)


def centred(x, mean):
    """x - float32(mean) in float64: the centred pixels as every stage defines them."""
    return x.astype(np.float64) - np.asarray(mean, dtype=np.float64).astype(np.float32).astype(np.float64)


def moments_host(x):
    """(mean [C], cov [C, C]) in float64 of the pixels x [N, C]."""
    mean = x.astype(np.float64).mean(axis=0)
    d = centred(x, mean)
    return mean, d.T @ d / (x.shape[0] - 1)


def reduce_host(scene, K, whiten=False, noise=None):
    """-> (scores [H, W, K] float32, fit): the pipeline of this module's docstring in numpy float64, for a raw scene [H, W, C].
    noise: None, or a direction of `band_reduce_noise` — the basis is then fit_noise_adjusted's."""
    scene = np.asarray(scene)
    if scene.ndim != 3:
        raise ValueError('band_reduce wants a primary scene [H, W, C]')
    H, W, C = scene.shape
    check_bands(K, C)
    if H * W < 2:
        raise ValueError('band_reduce needs at least two pixels')
    x = normalise(scene).reshape(H * W, C)
    mean, cov = moments_host(x)
    if noise is None:
        fit = fit_basis(mean, cov, K, whiten)
    else:
        fit = fit_noise_adjusted(mean, cov, noise_moments_host(x.reshape(H, W, C), noise), K, whiten, noise=noise)
    scores = centred(x, mean) @ fit['basis'].astype(np.float64)
    fit['route'] = 'host'
    return scores.astype(np.float32).reshape(H, W, int(K)), fit


def save_fit(path, fit):
    """`<t>_band_reduce.npz`: mean, basis, eigenvalues, explained-variance ratios and the route taken; of a noise-adjusted fit
    also noise_eigenvalues, snr and noise (the direction)."""
    more = dict(noise_eigenvalues=fit['noise_eigenvalues'], snr=fit['snr'], noise=np.array(str(fit['noise']))) if 'noise' in fit else {}
    np.savez(path, mean=fit['mean'], basis=fit['basis'], eigenvalues=fit['eigenvalues'], explained=fit['explained'],
             route=np.array(fit['route']), **more)


# ------------------------------------------------------------------------------ band_reduce_noise
# The noise-adjusted principal component transform (Green et al. 1988; Lee et al. 1990), also maximum noise fraction, MNF: the
# noise covariance is estimated from shift differences of the scene, the noise is whitened, a PCA follows, and the components
# come ordered by signal-to-noise ratio, not by variance.  With x [H, W, C] as above and a direction with pixel step s
# (horizontal: the right neighbour in the row; vertical: the pixel below):
#     e_p      = x[p] - x[p + s]                               for every pixel that has that neighbour, 0 for the others
#     M        = the number of pixels that have it             H (W - 1) horizontal, (H - 1) W vertical
#     ncov_dir = sum_p e_p e_p^T / (2 M)                       uncentred; the 2 is the shift-difference estimator's
#     ncov     = ncov_dir, or (ncov_h + ncov_v) / 2 for `both`
#     basis    = fit_noise_adjusted(mean, cov, ncov, K, whiten)
# and the scores are (x - float32(mean)) basis as before.  The device route (dmf_band_noise_moments) forms e and its products in
# fp32 and the sums over runs of pixels in double; here e is the exact difference of the fp32 pixels, in float64.
NOISE_KINDS = ('none', 'horizontal', 'vertical', 'both')


def noise_keys(cfg):
    """-> None, or 'horizontal' / 'vertical' / 'both' from the optional top-level key
         band_reduce_noise none / horizontal / vertical / both (default none)
    which stands beside `band_reduce: pca`; with `band_reduce: none` anything but none is refused."""
    noise = cfg.get('band_reduce_noise', 'none')
    noise = 'none' if noise is None or noise is False or noise == 0 else str(noise).lower()
    if noise not in NOISE_KINDS:
        raise ValueError('band_reduce_noise %r is not one of %s' % (cfg.get('band_reduce_noise'), ' / '.join(NOISE_KINDS)))
    if noise != 'none' and band_keys(cfg)['kind'] is None:
        raise ValueError('band_reduce_noise: %s adjusts the transform of band_reduce: pca, and band_reduce is none' % noise)
    return None if noise == 'none' else noise


def noise_directions(noise):
    """The directions a value of `band_reduce_noise` asks for, in the order they are computed."""
    if noise not in NOISE_KINDS[1:]:
        raise ValueError('band_reduce_noise %r is not one of %s' % (noise, ' / '.join(NOISE_KINDS[1:])))
    return ('horizontal', 'vertical') if noise == 'both' else (noise,)


def check_noise(noise, H, W):
    """Refuses, by name, a scene in which no pixel has the neighbour a direction needs."""
    for d in noise_directions(noise):
        if (W if d == 'horizontal' else H) < 2:
            raise ValueError('band_reduce_noise: %s needs at least two %s, the scene is %d x %d'
                             % (d, 'columns' if d == 'horizontal' else 'rows', H, W))


def combine_noise(parts):
    """ncov of one direction, or the mean of the two (`both`), in float64."""
    parts = [np.asarray(p, dtype=np.float64) for p in parts]
    return parts[0] if len(parts) == 1 else (parts[0] + parts[1]) / 2.0


def noise_moments_host(x, noise):
    """ncov [C, C] in float64 of the scene x [H, W, C] (the definition above)."""
    H, W, C = x.shape
    check_noise(noise, H, W)
    x = x.astype(np.float64)
    parts = []
    for d in noise_directions(noise):
        e = (x[:, :-1] - x[:, 1:] if d == 'horizontal' else x[:-1] - x[1:]).reshape(-1, C)
        parts.append(e.T @ e / (2.0 * e.shape[0]))
    return combine_noise(parts)


def fit_noise_adjusted(mean, cov, ncov, K, whiten=False, noise=None):
    """-> fit_basis's dict with the noise-adjusted basis, plus noise_eigenvalues [C], snr [K] and noise (the direction), from the
    band means, the covariance and the noise covariance [C, C], in numpy float64:
        ncov = U L U^T (eigh);  F = U L^(-1/2);  Mw = F^T cov F, symmetrised;  eigh(Mw) descending gives nu and V;
        basis = F V[:, :K]  (unit noise variance: b^T ncov b = 1), its columns signed by sign_columns.
    eigenvalues = nu[:K] (the variance of a component in units of its noise), snr = nu[:K] - 1, explained = nu[:K] / sum(nu).
    whiten: column k is divided by sqrt(nu[k]), so the scores have unit total variance.  A noise estimate that is singular in
    float64 — its smallest eigenvalue not above C 2^-52 times its largest: the scene has a constant or duplicated band — is
    refused by name."""
    mean = np.asarray(mean, dtype=np.float64)
    cov = np.asarray(cov, dtype=np.float64)
    ncov = np.asarray(ncov, dtype=np.float64)
    C = mean.shape[0]
    if cov.shape != (C, C) or ncov.shape != (C, C):
        raise ValueError('fit_noise_adjusted wants mean [C], cov [C, C] and ncov [C, C]')
    K = int(K)
    if K < 1:
        raise ValueError('band_reduce_bands %r is not a whole number >= 1' % (K,))
    check_bands(K, C)
    nlam, U = np.linalg.eigh(ncov, UPLO='U')               # ascending
    if not nlam[0] > C * 2.0 ** -52 * nlam[-1]:
        raise ValueError('band_reduce_noise: the noise covariance is singular (eigenvalues %g .. %g): the scene has a constant or '
                         'duplicated band' % (nlam[0], nlam[-1]))
    F = U / np.sqrt(nlam)[None, :]
    Mw = F.T @ cov @ F
    nu, V = np.linalg.eigh((Mw + Mw.T) / 2.0)
    nu, V = nu[::-1].copy(), V[:, ::-1]
    vec = sign_columns(F @ V[:, :K])
    lam = nu[:K].copy()
    if whiten:
        if not np.all(lam > 0):
            raise ValueError('band_reduce_whiten: eigenvalue %d of the first %d is %g, not positive; lower band_reduce_bands'
                             % (int(np.argmin(lam > 0)), K, lam[np.argmin(lam > 0)]))
        vec = vec / np.sqrt(lam)[None, :]
    return dict(mean=mean, basis=np.ascontiguousarray(vec, dtype=np.float32), eigenvalues=lam, explained=lam / nu.sum(),
                noise_eigenvalues=nlam[::-1].copy(), snr=lam - 1.0, noise=noise)
