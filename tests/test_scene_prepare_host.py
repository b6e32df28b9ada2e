"""CPU-only tests of the device scene preparation's host side: where `dmf.engine.prep_route` sends a raw scene, the reflect
index rule of dmf_scene_prepare against numpy's 'reflect' padding, and the C ABI of the two entry points."""
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_prep_route_decisions():
    from dmf.engine import prep_route
    H, W = 12, 9
    # numpy's own wraparound: int16 30000 - (-30000) is not an int16
    where, why = prep_route(np.int16, H, W, 4, np.int16(-30000), np.int16(30000))
    assert where == 'host' and 'wraps' in why
    assert prep_route(np.int16, H, W, 4, np.int16(-30000), np.int16(2767)) == ('device', '')     # 32767: the largest that fits
    assert prep_route(np.int16, H, W, 4, np.int16(-30000), np.int16(2768))[0] == 'host'
    assert prep_route(np.int32, H, W, 4, np.int32(-2**31), np.int32(0))[0] == 'host'
    assert prep_route(np.uint16, H, W, 4, np.uint16(0), np.uint16(65535)) == ('device', '')
    assert prep_route(np.float32, H, W, 4, np.float32(-3e38), np.float32(3e38)) == ('device', '')   # (inf on both routes)
    # the reflection reaches H - 1 rows / W - 1 columns
    assert prep_route(np.uint16, 9, 12, 9)[0] == 'host'            # pad == H
    assert prep_route(np.uint16, 9, 12, 8) == ('device', '')       # pad == H - 1
    assert prep_route(np.uint16, 12, 9, 9)[0] == 'host'            # pad == W
    assert prep_route(np.uint16, 12, 9, 8) == ('device', '')
    assert prep_route(np.uint16, 1, 1, 0) == ('device', '')
    # dtypes without a code
    for dt in (np.bool_, np.complex64, np.complex128, np.int64, np.uint32, np.float16, np.dtype('>u2')):
        where, why = prep_route(dt, H, W, 4)
        assert where == 'host' and 'no device code' in why, dt
    for dt in (np.uint8, np.uint16, np.int16, np.int32, np.float32, np.float64):
        assert prep_route(dt, H, W, 4) == ('device', ''), dt


@pytest.mark.parametrize('H', range(2, 10))
def test_reflect_index_is_numpys_reflect(H):
    from dmf.engine import reflect_index
    for pad in range(H):
        want = np.pad(np.arange(H), (0, pad), 'reflect')
        got = np.array([reflect_index(i, H) for i in range(H + pad)])
        assert np.array_equal(got, want), (H, pad)
        assert got.min() >= 0 and got.max() < H


def test_scene_entry_points_and_dtype_codes_are_declared_and_exported():
    hdr = open(os.path.join(REPO, 'include', 'dmf.h')).read()
    for name in ('dmf_scene_minmax', 'dmf_scene_prepare'):
        assert re.search(r'\bint32_t\s+%s\s*\(' % name, hdr), name
    codes = {n: int(v) for n, v in re.findall(r'#define\s+DMF_RAW_(\w+)\s+(\d+)', hdr)}
    assert codes == {'U8': 0, 'U16': 1, 'I16': 2, 'I32': 3, 'F32': 4, 'F64': 5}
    assert int(re.search(r'#define DMF_VERSION (\d+)', hdr).group(1)) >= 302
    from dmf import lib
    assert {'dmf_scene_minmax', 'dmf_scene_prepare'} <= set(lib.EXPORTS)
    # the binding's table is the header's: same codes, and the element sizes of the numpy dtypes
    names = {'U8': 'uint8', 'U16': 'uint16', 'I16': 'int16', 'I32': 'int32', 'F32': 'float32', 'F64': 'float64'}
    assert {names[k]: v for k, v in codes.items()} == {k: v[0] for k, v in lib.RAW_DTYPES.items()}
    for name, (code, size) in lib.RAW_DTYPES.items():
        assert np.dtype(name).itemsize == size and lib.raw_code(name) == code
    assert lib.raw_code(np.bool_) is None and lib.raw_code(np.dtype('>f4')) is None


def test_to_tensor_types_are_the_ones_the_kernel_restates():
    """The arithmetic dmf_scene_prepare restates, pinned on the host: integer scenes subtract in the raw type and divide as
    float64; float32 stays float32; float64 stays float64."""
    from function.function import to_tensor
    rng = np.random.default_rng(0)
    for dt in (np.uint8, np.uint16, np.int16, np.int32):
        x = rng.integers(0, 100, (4, 5, 3)).astype(dt)
        x.flat[0], x.flat[-1] = 0, 100
        t = to_tensor(x)
        assert t.dtype == np.float64
        assert np.array_equal(t, (x - x.min()).astype(np.float64) / np.float64(dt(100)))
    assert to_tensor(rng.random((4, 5, 3)).astype(np.float32)).dtype == np.float32
    assert to_tensor(rng.random((4, 5, 3))).dtype == np.float64


def test_datasets_resolve_lazy_scenes_on_first_patch():
    from train.dataset import dataset_dual, dataset_qua_dqtl
    calls = []

    def lazy(name, arr):
        def get():
            calls.append(name)
            return arr
        return get
    cfg = {'patch_size': 3, 'scale': 2}
    ms, pan = np.arange(6 * 6 * 2, dtype=np.float64).reshape(6, 6, 2), np.arange(12 * 12, dtype=np.float64).reshape(12, 12)
    xyl = [np.array([[1.], [2.]]), np.array([[0.], [1.]]), np.array([[1.], [2.]])]
    eager, late = dataset_dual(ms, pan, xyl, cfg), dataset_dual(lazy('ms', ms), lazy('pan', pan), xyl, cfg)
    view = late.index_view()
    assert view[1] == (2, 1, 2, 1) and len(late) == 2 and calls == []          # the index view needs only the pixel table
    for a, b in zip(eager[1], late[1]):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    assert sorted(calls) == ['ms', 'pan']
    late[0]
    assert sorted(calls) == ['ms', 'pan']                                      # computed once
    four = [ms + k for k in range(4)]
    calls.clear()
    q_eager = dataset_qua_dqtl(*four, xyl, cfg)
    q_late = dataset_qua_dqtl(*[lazy(k, s) for k, s in enumerate(four)], xyl, cfg)
    assert q_late.index_view()[0] == (1, 0, 1, 0) and calls == []
    for a, b in zip(q_eager[0], q_late[0]):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    q_late[1]
    assert sorted(calls) == [0, 1, 2, 3]
