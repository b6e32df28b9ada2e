"""CPU: the two geometry words of the reduce launch (csrc/dmf_shapes.h: reduce_words_pack / reduce_words_unpack).

The launch passes H, 2F, K and NCONV in two preloaded 32-bit words; the kernel derives from them the flat offsets of
fc1 / fc2 and the workspace offsets of the head vectors.  For every row of the compiled shape table, several class counts
and batch sizes, what a small host program unpacks must equal (a) the layouts of the same header, (b) the offsets the C ABI
reports (dmf_param_layout), (c) the sizes stated in include/dmf.h, written out again here, and (d) dmf_workspace_bytes.
"""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from dmf import lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, 'tests', 'reduce_words_check.cpp')
MAX_BLOCKS, KMAX = 256, 64


def table_rows():
    """The rows of DMF_V2_SHAPES as the library itself lists them when it refuses a shape."""
    s = lib.Shape(C=3, C2=1, P=3, S=1, F=4, G=1, H=64, K=5, attention=0, heads=0, E=0, reserved=0)
    assert lib._lib.dmf_shape_supported(C.byref(s)) != 0
    msg = lib._lib.dmf_last_error().decode()
    listed = msg.split('compiled (C/C2/P/S/F/G):', 1)[1].split('(K <=', 1)[0]
    rows = [tuple(int(x) for x in m) for m in re.findall(r'(\d+)/(\d+)/(\d+)/(\d+)/(\d+)/(\d+)', listed)]
    assert (200, 1, 11, 1, 40, 10) in rows and len(rows) >= 10, msg
    return sorted(set(rows))


@pytest.fixture(scope='module')
def checker(tmp_path_factory):
    cxx = next((c for c in (shutil.which('c++'), shutil.which('g++'), shutil.which('clang++'), '/opt/rocm/llvm/bin/clang++',
                            '/opt/rocm/lib/llvm/bin/clang++') if c and os.path.exists(c)), None)
    assert cxx is not None, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('rw') / 'reduce_words_check')
    subprocess.run([cxx, '-std=c++17', '-O1', SRC, '-o', exe], check=True)

    def run(cases):
        out = subprocess.run([exe] + ['%d %d %d %d %d %d %d %d %d' % c for c in cases], check=True, capture_output=True, text=True).stdout
        lines = out.strip().split('\n')
        assert len(lines) == len(cases)
        return [[int(t) for t in ln.replace('|', ' ').split()] for ln in lines]
    return run


def expected(Cc, C2, P, S, F, G, H, K, B):
    """include/dmf.h's parameter order and dmf_shapes.h's workspace order, from the sizes alone."""
    Cg, TB = Cc // G, C2 * S * S
    nconv = F * Cg + F + 9 * F + F + F * TB + F + 9 * F + F
    fc1w = nconv
    fc1b = fc1w + H * 2 * F
    fc2w = fc1b + H
    fc2b = fc2w + K * H
    slab = (nconv + 31) & ~31
    z = MAX_BLOCKS * slab
    h = z + B * 2 * F
    dh = h + B * H
    dl = dh + B * H
    return nconv, slab, [fc1w, fc1b, fc2w, fc2b], [z, h, dh, dl]


def test_unpacked_words_match_the_layouts(checker):
    cases = [r + (64, K, B) for r in table_rows() for K in (2, 17, 64) for B in (1, 3, 256, 260, 600, 1 << 20)]
    for c, got in zip(cases, checker(cases)):
        Cc, C2, P, S, F, G, H, K, B = c
        ok, w3, w4 = got[:3]
        gH, gF2, gK, gN = got[3:7]
        g_off, g_ws = got[7:11], got[11:15]
        l_off, l_ws = got[15:19], got[19:24]
        nconv, slab, e_off, e_ws = expected(*c)
        assert ok == 1, c
        assert w3 == H | (2 * F) << 8 | K << 16 and w4 == nconv, c
        assert (gH, gF2, gK, gN) == (H, 2 * F, K, nconv), c
        assert g_off == l_off == e_off, (c, g_off, l_off, e_off)
        assert l_ws[0] == 0 and g_ws == l_ws[1:] == e_ws, (c, g_ws, l_ws, e_ws)
        shape = lib.Shape(C=Cc, C2=C2, P=P, S=S, F=F, G=G, H=H, K=K, attention=0, heads=0, E=0, reserved=0)
        assert lib.param_layout(shape)[8:12] == g_off, c
        if B <= 600:
            assert lib.workspace_bytes(shape, B) == 4 * (g_ws[3] + B * KMAX + B * slab), c


def test_a_layout_the_words_cannot_hold_is_refused(checker):
    rows = checker([(200, 1, 11, 1, 40, 10, 64, 256, 256),       # K needs 9 bits
                    (200, 1, 11, 1, 128, 8, 64, 17, 256),        # 2F needs 9 bits
                    (200, 1, 11, 1, 40, 10, 256, 17, 256)])      # H needs 9 bits
    assert [r[0] for r in rows] == [0, 0, 0]
