"""CPU: what tests/test_gpu_qua_parity.py rests on, checked on tests/qua_ref.py and the float64 oracle alone — every case runs in
the kernel form its row claims (against the constants of csrc/dmf_qua.hip, read as text), the reference is finite, no case
sits on a kink of the loss, both signs of both kink arguments occur in every form, the `wide` logits hold the probabilities
that make a float32 evaluation fragile, and float32 arithmetic with the kernel's limits meets a quarter of the tolerance.
No GPU, nothing of the HIP library."""
import re

import pytest
import torch

import qua_ref as qr

CELLS = [(bs, K) for _, bs, K in qr.CASES]


def test_form_restates_the_kernels_dispatch():
    src = open(qr.KERNEL_SRC).read()
    assert int(re.search(r'constexpr int QE_MAXG = (\d+);', src).group(1)) == qr.QE_MAXG
    assert int(re.search(r'constexpr int QT = (\d+);', src).group(1)) == qr.QT
    assert 'if (a.K <= 16 && a.bs <= 16 * QE_MAXG) {' in src
    assert 'const int G = (a.bs + 15) / 16;' in src
    m = re.search(r'int ts = \((\d+) \* 1024 / 4\) / \((\d+) \* a\.K\);', src)
    assert (int(m.group(1)) * 1024, int(m.group(2))) == (qr.LDS_BUDGET, qr.ROW_FLOATS)
    assert 'ts = ts > 256 ? 256 : (ts < 1 ? 1 : ts);' in src and 'if (ts > a.bs) ts = a.bs;' in src
    m = re.search(r'const size_t bytes = \(size_t\)\(QT \+ (\d+) \* ts \* a\.K\) \* sizeof\(float\);', src)
    assert int(m.group(1)) == qr.ROW_FLOATS
    assert len(re.findall(r'once(?:16|0)\.set\(reinterpret_cast<const void\*>\(&qua_loss_kernel<(?:16|0)>\), (\d+) \* 1024\)', src)) == 2
    assert all(int(v) * 1024 == qr.LDS_LIMIT for v in re.findall(r'qua_loss_kernel<\d+>\), (\d+) \* 1024\)', src))
    assert 'if (a.K <= 16) hipLaunchKernelGGL(qua_loss_kernel<16>' in src and 'else hipLaunchKernelGGL(qua_loss_kernel<0>' in src


def test_every_case_is_in_the_form_it_claims():
    for row, bs, K in qr.CASES:
        assert qr.in_row(row, bs, K), (row, bs, K, qr.form(bs, K))
        assert qr.lds_bytes(bs, K) <= qr.LDS_LIMIT
    assert {r for r, _, _ in qr.CASES} == set(qr.ROWS)
    # the edges the table is there for
    assert qr.form(3, 2) == ('element', 1) and qr.form(16, 16) == ('element', 1) and qr.form(17, 16) == ('element', 2)
    assert qr.form(4096, 16) == ('element', qr.QE_MAXG)
    assert qr.tile(4097, 16) == 240 and 4097 % 240 == 17 and qr.tile(4097, 3) == 256 and 4097 % 256 == 1
    assert qr.tile(225, 17) == qr.tile(226, 17) == 225 and qr.tile(61, 64) == 60 and qr.lds_bytes(60, 64) == 157696
    assert qr.form(130, 33) == ('tiled0', 2)
    for bs_r, K, W in qr.RANK_CASES:
        assert qr.lds_bytes(W * bs_r, K) <= qr.LDS_LIMIT
    assert [qr.form(W * bs_r, K) for bs_r, K, W in qr.RANK_CASES] == [('element', 2), ('tiled0', 1), ('tiled0', 2)]
    # test_gpu_stage2.py and test_gpu_stage2_dp.py, for the record: none of the edges above
    assert qr.form(600 * 8, 12)[0] == 'tiled16' and qr.form(256, 17) == ('tiled0', 2) and qr.form(1100, 17) == ('tiled0', 5)


@pytest.mark.parametrize('bs,K', CELLS)
def test_wide_logits_reach_zero_and_the_square_underflow(bs, K):
    t, sets = qr.case(bs, K)
    assert int(t.min()) >= 0 and int(t.max()) < K
    unit = sets['unit'].softmax(dim=-1)
    assert float(unit.min()) > 1e-12, 'the unit set stays clear of every limit'
    y = sets['wide'].softmax(dim=-1).view(4, bs, K)
    assert y.dtype == torch.float32
    for st in (0, 1):
        tiny = int(((y[st] > 0) & (y[st] < qr.TINY)).sum())
        zeros = int((y[st] == 0).sum())
        if bs >= 16:
            assert tiny >= 1 and zeros >= 1, (st, tiny, zeros)
    if bs < 16:                            # (3, 2): samples 0, 1, 2 lower p by 52, q by 60, s by 80
        assert int(((y[:2] > 0) & (y[:2] < qr.TINY)).sum()) >= 1
    # what the offsets are for, on the samples that carry them
    for i in range(min(bs, 40)):
        streams, off = qr.lowered(i)
        v = [float(y[st, i, i % K]) for st in streams]
        if off == 120.0:
            assert all(x == 0.0 for x in v)
        elif off == 80.0:
            assert all(0.0 < x < 1e-30 for x in v)
        elif off == 60.0:
            assert all(0.0 < x < qr.TINY for x in v)
    assert float(sets['wide'].double().softmax(dim=-1).min()) > 0.0, 'no float64 probability is 0: the oracle needs no limit'


def test_the_float32_oracle_is_not_a_reference_on_wide_logits():
    """Why the reference is float64: the oracle itself, in float32, has a non-finite gradient there."""
    t, sets = qr.case(33, 15)
    _, g32 = qr.value_and_grad(sets['wide'], 33, t, torch.float32, qr.COEFS[0], qr.EPS, qr.TAOS[0])
    assert not bool(torch.isfinite(g32).all())
    _, g32 = qr.value_and_grad(sets['unit'], 33, t, torch.float32, qr.COEFS[0], qr.EPS, qr.TAOS[0])
    assert bool(torch.isfinite(g32).all())


@pytest.mark.parametrize('bs,K', CELLS)
def test_no_case_sits_on_a_kink(bs, K):
    _, sets = qr.case(bs, K)
    for name in qr.SETS:
        for tao in qr.TAOS:
            d1, d2 = qr.kink_arguments(sets[name], bs, qr.EPS, tao)
            assert abs(d1) >= 1e-3 and abs(d2) >= 1e-3, (name, tao, d1, d2)


def test_both_signs_of_both_kink_arguments_in_every_form():
    seen = {row: set() for row in qr.ROWS}
    for row, bs, K in qr.CASES:
        _, sets = qr.case(bs, K)
        for name in qr.SETS:
            for tao in qr.TAOS:
                d1, d2 = qr.kink_arguments(sets[name], bs, qr.EPS, tao)
                seen[row] |= {('d1', d1 > 0), ('d2', d2 > 0)}
    for row in qr.ROWS:
        assert seen[row] == {('d1', True), ('d1', False), ('d2', True), ('d2', False)}, (row, seen[row])


@pytest.mark.parametrize('bs,K', CELLS)
def test_float64_reference_is_finite_and_float32_can_meet_a_quarter_of_the_tolerance(bs, K):
    t, sets = qr.case(bs, K)
    worst = {}
    for name in qr.SETS:
        wl = wg = 0.0
        for tao in qr.TAOS:
            for coef in qr.COEFS:
                ref_l, ref_g = qr.value_and_grad(sets[name], bs, t, torch.float64, coef, qr.EPS, tao)
                assert bool(torch.isfinite(ref_l)) and bool(torch.isfinite(ref_g).all()), (name, coef, tao)
                assert ref_g.abs().max().item() > 1e-5, 'a vanishing gradient would prove nothing'
                got_l, got_g = qr.guarded32(sets[name], bs, t, coef, qr.EPS, tao)
                tol_l, tol_g = qr.tolerances(ref_l, ref_g)
                el, eg = abs(got_l - ref_l).item(), (got_g - ref_g).abs().max().item()
                assert bool(torch.isfinite(got_g).all()) and el <= 0.25 * tol_l and eg <= 0.25 * tol_g, (name, coef, tao, el, tol_l, eg, tol_g)
                wl, wg = max(wl, el / tol_l), max(wg, eg / tol_g)
        worst[name] = (wl, wg)
    print('guarded float32 vs float64 at (%d, %d), as a share of the tolerance: ' % (bs, K)
          + ', '.join('%s loss %.3f grad %.3f' % ((n,) + worst[n]) for n in qr.SETS))


@pytest.mark.parametrize('K', qr.ARGMAX_KS)
@pytest.mark.parametrize('bs', qr.ARGMAX_BSS)
def test_pair_argmax_cases(K, bs):
    sets, first = qr.argmax_case(K, bs)
    for name in ('unit', 'gap'):
        want, safe = qr.argmax_reference(sets[name], bs)
        assert int(safe.sum()) >= 0.95 * bs, (name, int(safe.sum()), bs)
    z = sets['gap'][:bs].double() + sets['gap'][bs:].double()
    top = z.topk(2, dim=1).values
    assert float((top[:, 0] - top[:, 1]).min()) > 104.0
    a, b = sets['tie'][:bs], sets['tie'][bs:]
    z32, z64 = a + b, a.double() + b.double()
    assert torch.equal(z32.double(), z64), 'the tie rows sum exactly in float32'
    ties = (z64 == z64.max(1, keepdim=True).values)
    assert int(ties.sum(1).min()) >= 2 and torch.equal(ties.int().argmax(1), first)
    if bs >= 255 and K > 2:
        assert len(set(first.tolist())) > 2, 'the first maximal index is not always class 0'
