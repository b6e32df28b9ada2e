"""GPU: scene preparation on the device (dmf_scene_minmax, dmf_scene_prepare; Scene.from_raw, QuaScene.from_raw,
`scene_prep: device`) against the host path it restates.  The host function is the definition, so every comparison is bit
for bit: `Scene(data_padding(raw, ..), data_padding_aux(raw, ..), ..)` / `QuaScene([data_padding(raw, ..) ..])`, fp32 and fp16
tensors viewed as integers so that neither -0 nor a NaN can hide a difference.  While a `from_raw` constructor runs,
`function.function.to_tensor` raises: a silent fall-back to the host would fail the test instead of passing it.
"""
import shutil
import tempfile
import warnings

import numpy as np
import pytest
import torch

from test_gpu_stage2 import _setup as _setup_stage2
from test_gpu_trajectory import _setup as _setup_solver

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
DTYPES = ['uint8', 'uint16', 'int16', 'int32', 'float32', 'float64']
# (min, max) that occur once each, and the open range of every other value; integer ranges keep max - min representable
RANGES = {'uint8': (0, 255, 1, 255), 'uint16': (3, 65535, 1000, 60000), 'int16': (-10000, 20000, -9000, 9000),
          'int32': (-10**9, 10**9, -5 * 10**8, 5 * 10**8), 'float32': (-1000.5, 777.25, -500.0, 500.0),
          'float64': (-3.25e-3, 9.75e4, -1e-3, 9e4)}


def draw(dtype, shape, seed, min_first=True):
    """Seeded raw scene whose minimum and maximum occur once: at the first and the last element, or the other way round."""
    lo, hi, a, b = RANGES[dtype]
    rng = np.random.default_rng(seed)
    x = rng.integers(a, b, shape) if np.dtype(dtype).kind in 'iu' else rng.uniform(a, b, shape)
    x = x.astype(dtype)
    x.flat[0], x.flat[-1] = (lo, hi) if min_first else (hi, lo)
    return x


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def assert_same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape and got.is_contiguous(), what
    assert torch.equal(bits(got), bits(want)), what


@pytest.fixture
def no_host_prep(monkeypatch):
    """Call it once the host reference is computed: from then on the host normalisation raises."""
    def arm():
        def boom(image):
            raise AssertionError('the host to_tensor ran')
        monkeypatch.setattr('function.function.to_tensor', boom)
    return arm


def host_scene(primary, aux, patch, scale, half):
    from dmf.engine import Scene
    from function.function import data_padding, data_padding_aux
    cfg = {'patch_size': patch, 'scale': scale}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')               # (the NaN case: numpy warns about the invalid values it propagates)
        return Scene(data_padding(primary, cfg, 'ms'), data_padding_aux(aux, cfg), DEV, half=half)


def check_scene(primary, aux, patch, scale, half, arm):
    from dmf.engine import Scene
    want = host_scene(primary, aux, patch, scale, half)
    arm()
    got = Scene.from_raw(primary, aux, patch, scale, DEV, half=half)
    assert got.half == want.half and got.device == want.device
    assert_same_bits(got.A, want.A, 'A')
    assert_same_bits(got.B, want.B, 'B')
    return got


@pytest.mark.parametrize('half', [0, 1])
@pytest.mark.parametrize('dtype', DTYPES)
def test_odd_shapes_every_dtype(dtype, half, no_host_prep):
    """7 x 9 x 5 with pad 4 and a 2-D 28 x 36 with pad 19: an odd C and an odd W C make the 16-byte output pieces straddle
    pixels and rows and leave a ragged tail; the extremes sit at the first and the last element, either way round."""
    primary = draw(dtype, (7, 9, 5), 1, min_first=True)
    aux = draw(dtype, (28, 36), 2, min_first=False)
    got = check_scene(primary, aux, 5, 4, half, no_host_prep)
    assert tuple(got.A.shape) == (11, 13, 5) and tuple(got.B.shape) == (47, 55, 1)
    assert float(got.B.min()) == 0.0 and float(got.B.max()) == 1.0


@pytest.mark.parametrize('half', [0, 1])
@pytest.mark.parametrize('dtype', ['uint16', 'float32'])
@pytest.mark.parametrize('patch', [6, 1])
def test_largest_legal_reflection_and_no_padding(patch, dtype, half, no_host_prep):
    """pad = H - 1 = W - 1 on a 6 x 6 x 3 scene (every row and column but the last is reflected), and pad = 0."""
    check_scene(draw(dtype, (6, 6, 3), 3), draw(dtype, (6, 6), 4, min_first=False), patch, 1, half, no_host_prep)


def test_pad_beyond_the_reflection_goes_to_the_host(capsys):
    """pad = H: numpy reflects a second time, the kernel does not state that — the constructor says so and uses the host."""
    from dmf import lib
    primary, aux = draw('uint16', (6, 6, 3), 3), draw('uint16', (6, 6), 4)
    want = host_scene(primary, aux, 7, 1, 0)
    from dmf.engine import Scene
    got = Scene.from_raw(primary, aux, 7, 1, DEV)
    assert 'on the host' in capsys.readouterr().out
    assert_same_bits(got.A, want.A, 'A')
    assert_same_bits(got.B, want.B, 'B')
    raw = torch.from_numpy(primary.reshape(-1).view(np.uint8)).to(DEV)
    mm = torch.zeros(16, dtype=torch.uint8, device=DEV)
    with pytest.raises(lib.DmfError, match='reflection'):
        lib.scene_prepare(raw, 'uint16', 6, 6, 3, mm, 6, torch.empty(12, 12, 3, device=DEV))


def test_wrapping_integer_range_goes_to_the_host(capsys):
    """int16 scene with max - min = 60000: numpy's int16 subtraction wraps; the host path, wrap included, is the result."""
    from dmf.engine import Scene
    primary = draw('int16', (7, 9, 5), 5)
    primary.flat[0], primary.flat[-1] = -30000, 30000
    aux = draw('int16', (28, 36), 6)
    want = host_scene(primary, aux, 5, 4, 0)
    got = Scene.from_raw(primary, aux, 5, 4, DEV)
    assert 'wraps' in capsys.readouterr().out
    assert_same_bits(got.A, want.A, 'A')
    assert_same_bits(got.B, want.B, 'B')


def _minmax(x):
    from dmf import lib
    raw = torch.from_numpy(np.ascontiguousarray(x).reshape(-1).view(np.uint8)).to(DEV)
    mm = torch.zeros(16, dtype=torch.uint8, device=DEV)
    lib.scene_minmax(raw, x.dtype.name, mm)
    return mm.cpu().numpy().view(x.dtype)[:2]


def test_more_than_one_reduction_block(no_host_prep):
    """300 x 257 x 4 uint16: 151 first-stage blocks; the maximum is the very last element."""
    primary = draw('uint16', (300, 257, 4), 7)
    assert int(primary.max()) == int(primary.flat[-1]) == 65535 and int((primary == 65535).sum()) == 1
    mn, mx = _minmax(primary)
    assert (int(mn), int(mx)) == (3, 65535)
    check_scene(primary, draw('uint16', (30, 26), 8), 5, 1, 0, no_host_prep)


@pytest.mark.parametrize('dtype', DTYPES)
def test_minmax_of_an_unaligned_scene_with_ragged_ends(dtype):
    """A scene that starts one element past a 16-byte boundary and ends off one: scalar head, vector body, scalar tail; the
    extremes sit in the head and in the tail, then in the body."""
    from dmf import lib
    n = 4099
    for where in ((0, n - 1), (n // 2, n // 3)):
        x = draw(dtype, (n + 1,), 9)
        lo, hi = RANGES[dtype][:2]
        x[0] = x[-1] = x[5]
        x[1 + where[0]], x[1 + where[1]] = lo, hi
        size = x.dtype.itemsize
        raw = torch.from_numpy(x.view(np.uint8)).to(DEV)[size:]
        mm = torch.zeros(16, dtype=torch.uint8, device=DEV)
        lib.scene_minmax(raw, dtype, mm)
        got = mm.cpu().numpy().view(x.dtype)[:2]
        assert got[0] == x[1:].min() == np.dtype(dtype).type(lo) and got[1] == x[1:].max() == np.dtype(dtype).type(hi)


def test_nan_propagates_as_numpy_propagates_it(no_host_prep):
    """One NaN in an f32 scene: np.min / np.max return NaN, so the whole host scene is NaN — and so is the device's, element
    for element; a NaN-free aux scene beside it keeps its bits."""
    from dmf.engine import Scene
    primary = draw('float32', (7, 9, 5), 10)
    primary[3, 4, 2] = np.nan
    aux = draw('float32', (28, 36), 11)
    aux[20, 7] = np.nan
    clean = draw('float32', (28, 36), 12)
    mn, mx = _minmax(primary)
    assert np.isnan(mn) and np.isnan(mx)
    want = {(half, k): host_scene(primary, a, 5, 4, half) for half in (0, 1) for k, a in (('nan', aux), ('clean', clean))}
    no_host_prep()
    for (half, k), w in want.items():
        got = Scene.from_raw(primary, aux if k == 'nan' else clean, 5, 4, DEV, half=half)
        for g, t in ((got.A, w.A), (got.B, w.B)):
            assert g.dtype == t.dtype and g.shape == t.shape
            nan = torch.isnan(t)
            assert torch.equal(torch.isnan(g), nan)
            assert torch.equal(bits(g)[~nan], bits(t)[~nan])
        assert bool(torch.isnan(got.A).all()) and bool(torch.isnan(got.B).all()) == (k == 'nan')


STAGE2 = {'f64': ((12, 10, 4), ['float64'] * 4), 'mixed_odd': ((7, 9, 5), ['uint16', 'int16', 'float32', 'float64'])}


@pytest.mark.parametrize('case', list(STAGE2))
def test_stage2_tall_scene(case, no_host_prep):
    """Four scenes with patch 5, each normalised by its own range and written into its own quarter of the tall tensor; A (both
    precisions) and B equal QuaScene's.  The 7 x 9 x 5 streams of mixed dtypes end off a 16-byte boundary, so three of the
    quarters start unaligned."""
    from dmf.engine import QuaScene
    from function.function import data_padding
    shape, dtypes = STAGE2[case]
    raws = [draw(dt, shape, 20 + k, min_first=bool(k % 2)) for k, dt in enumerate(dtypes)]
    if case == 'f64':
        raws = [r * s + o for r, (s, o) in zip(raws, [(1.0, 0.0), (1e-3, 5.0), (40.0, -1e6), (7.5, 1e3)])]      # four value ranges
    padded = [data_padding(r, {'patch_size': 5}, 'ms') for r in raws]
    want = {half: QuaScene(padded, DEV, half=half) for half in (0, 1)}
    no_host_prep()
    for half in (0, 1):
        got = QuaScene.from_raw(raws, 5, DEV, half=half)
        assert got.Hp == want[half].Hp == shape[0] + 4 and got.half == bool(half) and got.device == want[half].device
        assert_same_bits(got.A, want[half].A, 'A half=%d' % half)
        assert_same_bits(got.B, want[half].B, 'B half=%d' % half)


def _one_epoch(solver_cls, cfg, stage2):
    torch.manual_seed(3407)
    s = solver_cls(cfg)
    if stage2:
        s.train_stage2()
    s.dataloader()
    s.train()
    return s


@pytest.mark.parametrize('which', ['Solver', 'toStageSolver'])
def test_solver_with_scene_prep_device(which, golden_dir, no_host_prep):
    """`scene_prep: device` trains an epoch without the host normalisation ever running; its resident scenes are bit-equal to
    the `scene_prep: host` solver's and its step losses exactly equal."""
    stage2 = which == 'toStageSolver'
    if stage2:
        from solver.tostagesolver import toStageSolver as cls
    else:
        from solver.mainsolver import Solver as cls
    setup = _setup_stage2 if stage2 else _setup_solver
    tmps = [tempfile.mkdtemp(prefix='dmf_prep_') for _ in range(2)]
    try:
        _, cfg_host = setup(golden_dir, tmps[0], fast_path=1, epoch=1, scene_prep='host')
        _, cfg_dev = setup(golden_dir, tmps[1], fast_path=1, epoch=1, scene_prep='device')
        host = _one_epoch(cls, cfg_host, stage2)
        no_host_prep()
        dev = _one_epoch(cls, cfg_dev, stage2)
        assert dev.device_prep and not host.device_prep
        assert_same_bits(dev.scene.A, host.scene.A, 'scene.A')
        assert_same_bits(dev.scene.B, host.scene.B, 'scene.B')
        if stage2:
            assert_same_bits(dev.qua_scene.A, host.qua_scene.A, 'qua_scene.A')
            assert_same_bits(dev.qua_scene.B, host.qua_scene.B, 'qua_scene.B')
        assert len(dev.step_losses) == len(host.step_losses) > 0
        assert dev.step_losses == host.step_losses
    finally:
        for t in tmps:
            shutil.rmtree(t)
