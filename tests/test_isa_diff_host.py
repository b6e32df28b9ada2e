"""CPU: tools/isa_diff.py on two hand-written listings — what counts as identical, what is reported, when it fails.

No compiler is started: the listings are given as text, in the form `hipcc --cuda-device-only -S` writes them.
"""
import importlib.util
import io
import os

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location('isa_diff', os.path.join(REPO, 'tools', 'isa_diff.py'))
isa_diff = importlib.util.module_from_spec(spec)
spec.loader.exec_module(isa_diff)


def kernel(name, idx, body, vgpr=9, sgpr=12, scratch=0, lds=0):
    return '''\t.text
\t.protected\t{n} ; -- Begin function {n}
\t.globl\t{n}
\t.p2align\t8
\t.type\t{n},@function
{n}: ; @{n}
; %bb.0:
{b}
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.p2align\t6, 0x0
\t.amdhsa_kernel {n}
\t\t.amdhsa_group_segment_fixed_size {lds}
\t\t.amdhsa_private_segment_fixed_size {scratch}
\t\t.amdhsa_next_free_vgpr {vgpr}
\t\t.amdhsa_next_free_sgpr {sgpr}
\t.end_amdhsa_kernel
\t.text
.Lfunc_end{i}:
\t.size\t{n}, .Lfunc_end{i}-{n}
; -- End function
'''.format(n=name, i=idx, b=body, vgpr=vgpr, sgpr=sgpr, scratch=scratch, lds=lds)


LOOP = '''\tv_mov_b32_e32 v0, 0 ; comment {c}
.LBB{i}_1: ; =>This Inner Loop Header: Depth=1

\tv_add_f32_e32 v0, v0, v1
\ts_cbranch_scc1 .LBB{i}_1'''


def test_comments_blank_lines_and_label_numbers_do_not_count():
    old = isa_diff.parse_listing(kernel('_Z1av', 0, LOOP.format(c='x', i=0)) + kernel('_Z1bv', 1, LOOP.format(c='x', i=1)))
    # the same two kernels behind a new one: every local label is renumbered
    new = isa_diff.parse_listing(kernel('_Z1av', 1, LOOP.format(c='y', i=1)) + kernel('_Z1bv', 2, LOOP.format(c='z', i=2)))
    rows, gone, added = isa_diff.compare(old, new)
    assert [(r[0], r[1]) for r in rows] == [('_Z1av', False), ('_Z1bv', False)] and gone == [] and added == []
    assert rows[0][2]['insts'] == (4, 4)            # v_mov, v_add, s_cbranch, s_endpgm: no label, no directive


def test_a_changed_kernel_is_reported_with_its_figures():
    old = isa_diff.parse_listing(kernel('_Z1av', 0, LOOP.format(c='', i=0), vgpr=9, scratch=0, lds=64) + kernel('_Z1bv', 1, '\ts_nop 0'))
    new = isa_diff.parse_listing(kernel('_Z1av', 0, LOOP.format(c='', i=0) + '\n\tv_mov_b32_e32 v2, v0', vgpr=10, scratch=16, lds=64) +
                                 kernel('_Z1bv', 1, '\ts_nop 0'))
    rows, gone, added = isa_diff.compare(old, new)
    assert [(r[0], r[1]) for r in rows] == [('_Z1av', True), ('_Z1bv', False)]
    assert rows[0][2] == {'insts': (4, 5), 'vgpr': (9, 10), 'sgpr': (12, 12), 'scratch': (0, 16), 'lds': (64, 64)}
    assert isa_diff.fig(rows[0][2]['vgpr']) == '9>10' and isa_diff.fig(rows[0][2]['sgpr']) == '12'


def test_the_same_code_with_other_registers_allotted_is_a_change():
    old = isa_diff.parse_listing(kernel('_Z1av', 0, '\tv_add_f32_e32 v0, v0, v1'))
    new = isa_diff.parse_listing(kernel('_Z1av', 0, '\tv_add_f32_e32 v0, v0, v2'))
    assert isa_diff.compare(old, new)[0][0][1] is True


def test_kernels_only_one_side_has_are_named():
    old = isa_diff.parse_listing(kernel('_Z1av', 0, '\ts_nop 0') + kernel('_Z1bv', 1, '\ts_nop 0'))
    new = isa_diff.parse_listing(kernel('_Z1av', 0, '\ts_nop 0') + kernel('_Z1cv', 1, '\ts_nop 0'))
    rows, gone, added = isa_diff.compare(old, new)
    assert [r[0] for r in rows] == ['_Z1av'] and gone == ['_Z1bv'] and added == ['_Z1cv']
    text = io.StringIO()
    assert isa_diff.report('x.hip', old, new, out=text) is False          # -> exit status 1
    assert 'ONLY IN OLD' in text.getvalue() and 'ONLY IN NEW' in text.getvalue()
    assert isa_diff.report('x.hip', old, old, out=io.StringIO()) is True
