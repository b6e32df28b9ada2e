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
(include/dmf.h); this module does everything after x in float64."""
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


def reduce_host(scene, K, whiten=False):
    """-> (scores [H, W, K] float32, fit): the pipeline of this module's docstring in numpy float64, for a raw scene [H, W, C]."""
    scene = np.asarray(scene)
    if scene.ndim != 3:
        raise ValueError('band_reduce wants a primary scene [H, W, C]')
    H, W, C = scene.shape
    check_bands(K, C)
    if H * W < 2:
        raise ValueError('band_reduce needs at least two pixels')
    x = normalise(scene).reshape(H * W, C)
    mean, cov = moments_host(x)
    fit = fit_basis(mean, cov, K, whiten)
    scores = centred(x, mean) @ fit['basis'].astype(np.float64)
    fit['route'] = 'host'
    return scores.astype(np.float32).reshape(H, W, int(K)), fit


def save_fit(path, fit):
    """`<t>_band_reduce.npz`: mean, basis, eigenvalues, explained-variance ratios and the route taken."""
    np.savez(path, mean=fit['mean'], basis=fit['basis'], eigenvalues=fit['eigenvalues'], explained=fit['explained'],
             route=np.array(fit['route']))
