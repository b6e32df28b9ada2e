"""CPU: the helpers and case tables of tests/mem_cases.py, which tests/test_gpu_memory_discipline.py relies on — guarded buffers
(alignment, sizes, what the fills decode to), the guard check (one flipped byte at either end of either guard), and that the
tables hold every structural variant their docstring names.  No GPU, nothing of the HIP library."""
import pytest
import torch

import mem_cases as mc

FLOATS = (torch.float32, torch.float16, torch.bfloat16)
DTYPES = FLOATS + (torch.int32, torch.int64, torch.uint8, torch.float64)


def test_fills_are_as_stated():
    assert mc.FILLS == (0x00, 0xFF, 0x47, 0x00) and mc.GUARD_BYTES == 64 * 1024 and mc.CANARY == 0xA5
    # more than one slab row (the conv parameters F (C / G + 1 + 9 + 1) + F (C2 S S + 1 + 9 + 1), padded to 32 floats) of every
    # row of the table, and more than one attention token map (128 tokens x 64 channels, bf16)
    G = {'tiny1': 2, 'tiny': 2, 'quatiny': 1, 'qua': 1, 'hsi': 10, 'hsi224': 8, 'pca32': 2, 'panms': 1}
    for name, (C, C2, P, S, K, F) in mc.SHAPES.items():
        slab = (F * (C // G[name] + 11) + F * (C2 * S * S + 11) + 31) & ~31
        assert mc.GUARD_BYTES > 4 * slab
    assert mc.GUARD_BYTES > 128 * 64 * 2


@pytest.mark.parametrize('dtype', DTYPES, ids=str)
@pytest.mark.parametrize('n', [1, 3, 255, 4097])
def test_guarded_layout(dtype, n):
    for fill in mc.FILLS:
        view, whole = mc.guarded(n, dtype, 'cpu', fill)
        size = torch.empty((), dtype=dtype).element_size()
        assert view.dtype == dtype and view.shape == (n,) and view.is_contiguous()
        assert whole.dtype == torch.uint8 and whole.numel() == 2 * mc.GUARD_BYTES + n * size
        assert view.data_ptr() % 256 == 0 and view.data_ptr() == whole.data_ptr() + mc.GUARD_BYTES
        assert bool((whole[:mc.GUARD_BYTES] == mc.CANARY).all()) and bool((whole[mc.GUARD_BYTES + n * size:] == mc.CANARY).all())
        assert bool((whole[mc.GUARD_BYTES:mc.GUARD_BYTES + n * size] == fill).all())
        assert mc.intact(whole, n, dtype)
        view.zero_()                                 # writing all of the view, and nothing else, leaves the guards alone
        assert mc.intact(whole, n, dtype)


@pytest.mark.parametrize('dtype', FLOATS, ids=str)
def test_fills_decode_as_stated(dtype):
    nan, _ = mc.guarded(7, dtype, 'cpu', 0xFF)
    assert bool(torch.isnan(nan).all())
    big, _ = mc.guarded(7, dtype, 'cpu', 0x47)
    assert bool(torch.isfinite(big).all())
    want = {torch.float32: 50999.28, torch.bfloat16: 50944.0, torch.float16: 7.2773}[dtype]
    assert abs(float(big[0]) - want) <= 1e-3 * want
    zero, _ = mc.guarded(7, dtype, 'cpu', 0x00)
    assert bool((zero == 0).all())


def test_ff_is_minus_one_as_an_int():
    v, _ = mc.guarded(5, torch.int32, 'cpu', 0xFF)
    assert bool((v == -1).all())


@pytest.mark.parametrize('dtype,n', [(torch.float32, 1), (torch.float16, 255), (torch.int32, 4097)], ids=str)
def test_intact_flags_one_flipped_byte(dtype, n):
    size = torch.empty((), dtype=dtype).element_size()
    end = mc.GUARD_BYTES + n * size
    spots = {0: ('before', -mc.GUARD_BYTES), mc.GUARD_BYTES - 1: ('before', -1), end: ('behind', 0),
             end + mc.GUARD_BYTES - 1: ('behind', mc.GUARD_BYTES - 1)}
    for at, (side, offset) in spots.items():
        _, whole = mc.guarded(n, dtype, 'cpu', 0x00)
        whole[at] ^= 1
        d = mc.intact(whole, n, dtype)
        assert not d and getattr(d, side) == (offset, offset) and getattr(d, 'behind' if side == 'before' else 'before') is None
        assert str(offset) in repr(d)
    _, whole = mc.guarded(n, dtype, 'cpu', 0x00)
    whole[3] = 0; whole[mc.GUARD_BYTES - 2] = 0; whole[end + 5] = 1
    d = mc.intact(whole, n, dtype)
    assert d.before == (3 - mc.GUARD_BYTES, -2) and d.behind == (5, 5)
    # another canary: the guard contents of the scene tests
    view, whole = mc.guarded(n, dtype, 'cpu', 0x47, canary=0xFF)
    assert mc.intact(whole, n, dtype, canary=0xFF) and not mc.intact(whole, n, dtype)


def test_bits_tell_nans_apart_and_equal_nans_equal():
    a = torch.tensor([float('nan'), 1.0])
    assert not torch.equal(a, a.clone()) and torch.equal(mc.bits(a), mc.bits(a.clone()))
    assert not torch.equal(mc.bits(torch.tensor([0.0])), mc.bits(torch.tensor([-0.0])))


def test_tables_hold_every_structural_variant():
    rows = {n: mc.SHAPES[n][:4] for n in mc.ROWS}
    assert rows == {'tiny1': (8, 1, 5, 1), 'tiny': (8, 1, 5, 4), 'quatiny': (4, 1, 5, 1), 'qua': (4, 1, 16, 1),
                    'hsi': (200, 1, 11, 1), 'hsi224': (224, 3, 11, 1), 'pca32': (32, 1, 11, 1)}
    assert mc.SHAPES['panms'][:4] == (4, 1, 16, 4)
    assert mc.SHAPES['hsi224'][5] == 32 and all(s[5] == 40 for n, s in mc.SHAPES.items() if n != 'hsi224')
    assert all(1 <= s[4] <= mc.KMAX for s in mc.SHAPES.values())
    assert set(mc.LARGE) == {'hsi', 'hsi224', 'qua', 'pca32'} and set(mc.ATTN_SHAPES) == {'tiny1', 'hsi'}
    cases = mc.patch_cases()
    small = [n for n in mc.ROWS if n not in mc.LARGE]
    for n in small:
        assert {B for m, B, K in cases if m == n and K == mc.SHAPES[n][4]} == {1, 3, 255, 257, 513}
    for n in mc.LARGE:
        assert {B for m, B, K in cases if m == n} == {3, 257}
    assert {K for m, B, K in cases if m == 'tiny1'} == {2, 5, 64} and mc.KMAX == 64
    unit = mc.patch_cases(unit=True)
    assert {B for m, B, K in unit if m == 'quatiny'} == {1, 3, 255, 257, 513, 1025}
    assert all(B <= 257 for m, B, K in unit if m in mc.LARGE)
    attn = mc.attn_cases()
    assert {B for m, B, K in attn if m == 'tiny1'} == {1, 3, 257, 513} and {B for m, B, K in attn if m == 'hsi'} == {1, 3, 257, 513}
    assert mc.SHARED_WS_BATCHES == (513, 3, 257, 1)
    assert mc.TAIL_N == (1, 255, 256, 257, 4097, 8009)
    assert mc.LOSS_BS == (1, 255, 257) and mc.LOSS_K == (2, 17, 64)
    assert mc.ROW_B == (1, 255, 257) and mc.ROW_K == (1, 17, 64)
    assert mc.BAND_C == (3, 32, 200) and mc.BAND_SCENE == (13, 11) and mc.PROJECT_C == (3, 200) and mc.PROJECT_K == (1, 32)
    assert mc.TEMP_N == (1, 255, 257) and mc.TEMP_K == 17 and mc.PITCH_EXTRA == (1, 2, 3)


@pytest.mark.parametrize('name', list(mc.SHAPES))
def test_scene_batch_is_legal_and_reaches_every_edge(name):
    C, C2, P, S, K, _ = mc.SHAPES[name]
    for B, extra in ((1, 0), (3, 0), (257, 3)):
        A, Bm, xy, t, dl = mc.scene_batch(name, B, K, extra=extra)
        assert tuple(A.shape) == (mc.SCENE_H + P - 1, mc.SCENE_W + P - 1, C)
        assert tuple(Bm.shape) == (S * (mc.SCENE_H + P - 1) + extra, S * (mc.SCENE_W + P - 1) + extra, C2)
        assert xy.dtype == torch.int32 and int(xy.min()) >= 0
        assert int(xy[:, 0].max()) + P <= A.shape[0] and int(xy[:, 1].max()) + P <= A.shape[1]       # lib.check_xy_bounds' rule
        assert S * (int(xy[:, 0].max()) + P) <= Bm.shape[0] and S * (int(xy[:, 1].max()) + P) <= Bm.shape[1]
        assert int(t.min()) >= 0 and int(t.max()) < K and int(t[0]) == K - 1 and dl.shape == (B, K)
        if B >= 8:
            pts = {tuple(p) for p in xy.tolist()}
            H, W = mc.SCENE_H, mc.SCENE_W
            assert {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)} <= pts                          # the four corner windows
            assert any(x == 0 and 0 < y < W - 1 for x, y in pts) and any(x == H - 1 and 0 < y < W - 1 for x, y in pts)
            assert any(y == 0 and 0 < x < H - 1 for x, y in pts) and any(y == W - 1 and 0 < x < H - 1 for x, y in pts)
            a, b = mc.patches_of(name, A, Bm, xy[:2])
            assert tuple(a.shape) == (2, C, P, P) and tuple(b.shape) == (2, C2, S * P, S * P)
            assert torch.equal(a[0, :, P - 1, P - 1], A[-1, -1, :]) and torch.equal(b[0, :, -1, -1], Bm[S * (H + P - 1) - 1, S * (W + P - 1) - 1, :])
