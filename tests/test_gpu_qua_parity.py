"""GPU: dmf_qua_loss / dmf_qua_loss_ranks in every form of the kernel, and dmf_pair_argmax, against float64.

launch_qua_loss (csrc/dmf_qua.hip) takes one of three implementations by K and bs; tests/qua_ref.py restates the dispatch and
lists the smallest batches that reach each form and each of its edges (one and 256 workgroups of the element-parallel form, the
first batch and the last-tile remainders of the tiled form, its one-tile path, K = 64 at the LDS limit).  Every case runs on two
sets of logits — `unit` (2 randn) and `wide` (one class per sample lowered by 52 .. 120, so that a probability is tiny, subnormal
or exactly 0 in float32) — with four (alpha, beta, gamma) and two tao, which between them take both signs of both absolute
values of the loss in every form.  tests/test_qua_cases_host.py checks all of that on the CPU.

The reference is the oracle (oracle/datapath_ref.py::qua_loss) evaluated in float64: in float32 it carries the kernel's own
roundings and is NaN on the `wide` set.  Tolerances are the project's (tests/test_gpu_stage2.py): loss 2e-6 max(1, |ref|),
gradient 1e-7 + 1e-4 max|ref gradient|.  Every comparison prints its worst error beside its tolerance; the worst per form and
set of one run are kept in profiles/qua_loss_parity.md.
"""
import pytest
import torch

import qua_ref as qr

pytestmark = pytest.mark.gpu

WORST = {}          # (row of the case table, set) -> [loss err, its tolerance, gradient err, its tolerance, max |ref gradient|]


def note(row, name, el, tl, eg, tg, gmax):
    w = WORST.setdefault((row, name), [0.0, 1.0, 0.0, 1.0, 0.0])
    if el / tl >= w[0] / w[1]:
        w[0], w[1] = el, tl
    if eg / tg >= w[2] / w[3]:
        w[2], w[3], w[4] = eg, tg, gmax


@pytest.fixture(scope='module', autouse=True)
def worst_errors_table():
    yield
    print('\n| form | logits | worst loss err | tolerance | worst gradient err | tolerance | max abs ref gradient |')
    print('|---|---|---|---|---|---|---|')
    for (row, name), w in sorted(WORST.items(), key=lambda kv: (qr.ROWS.index(kv[0][0]), kv[0][1])):
        print('| %s | %s | %.2e | %.2e | %.2e | %.2e | %.2e |' % ((row, name) + tuple(w)))


def run(x, bs, labels, prm, with_grad=True, **kw):
    from dmf import lib
    loss = torch.full((1,), float('nan'), device='cuda')
    dl = torch.full((4 * bs, x.shape[1]), float('nan'), device='cuda') if with_grad else None      # an unwritten element stays NaN
    lib.qua_loss(x, bs, labels, prm, loss=loss, dlogits=dl, **kw)
    torch.cuda.synchronize()
    return loss.cpu(), (dl.cpu() if with_grad else None)


@pytest.mark.parametrize('name', qr.SETS)
@pytest.mark.parametrize('row,bs,K', qr.CASES)
def test_qua_loss_against_the_float64_oracle(row, bs, K, name):
    from dmf import lib
    t, sets = qr.case(bs, K)
    x = sets[name]
    xd, td = x.cuda(), t.int().cuda()
    for tao in qr.TAOS:
        for coef in qr.COEFS:
            ref_l, ref_g = qr.value_and_grad(x, bs, t, torch.float64, coef, qr.EPS, tao)
            tol_l, tol_g = qr.tolerances(ref_l, ref_g)
            prm = lib.QuaParams(alpha=coef[0], beta=coef[1], gamma=coef[2], epsilon=qr.EPS, tao=tao)
            loss, dl = run(xd, bs, td, prm, grad_scale=1.0)
            el = abs(loss.double().item() - ref_l.item())
            eg = (dl.double() - ref_g).abs().max().item()
            n_bad = int((~torch.isfinite(dl)).sum())
            what = '[%s, bs %d, K %d, %s, coef %s, tao %g]' % (row, bs, K, name, coef, tao)
            print('%s loss err %.2e (tolerance %.2e), gradient err %.2e (tolerance %.2e), %d non-finite of %d'
                  % (what, el, tol_l, eg, tol_g, n_bad, dl.numel()))
            assert bool(torch.isfinite(loss).all()) and n_bad == 0, 'non-finite output ' + what
            note(row, name, el, tol_l, eg, tol_g, ref_g.abs().max().item())
            assert el < tol_l, 'loss ' + what
            assert eg < tol_g, 'gradient ' + what
            loss2, _ = run(xd, bs, td, prm, with_grad=False)          # the validation loop's form
            assert torch.equal(loss2, loss), 'loss-only call ' + what


@pytest.mark.parametrize('bs_r,K,W', qr.RANK_CASES)
def test_rank_rows_on_wide_logits_equal_the_restacked_batch(bs_r, K, W):
    """Every rank's rows and loss, bit for bit, and the loss scale as an exact factor — where a NaN or a limit taken in one
    form and not the other would show."""
    from dmf import lib
    bs = W * bs_r
    t, sets = qr.case(bs, K)
    restacked = sets['wide']                                                        # [4][bs][K]
    gathered = restacked.view(4, W, bs_r, K).permute(1, 0, 2, 3).reshape(W * 4 * bs_r, K).contiguous().cuda()
    td = t.int().cuda()
    state = torch.zeros(lib.SCALER_FLOATS, device='cuda')
    lib.scaler_init(state, 1024.0)
    for coef in (qr.COEFS[0], qr.COEFS[3]):
        for tao in qr.TAOS:
            prm = lib.QuaParams(alpha=coef[0], beta=coef[1], gamma=coef[2], epsilon=qr.EPS, tao=tao)
            ref_l, ref_g = qr.value_and_grad(restacked, bs, t, torch.float64, coef, qr.EPS, tao)
            tol_l, tol_g = qr.tolerances(ref_l, ref_g)
            want_l, want_d = run(restacked.cuda(), bs, td, prm)
            assert bool(torch.isfinite(want_d).all())
            el, eg = abs(want_l.double().item() - ref_l.item()), (want_d.double() - ref_g).abs().max().item()
            print('[bs_r %d, K %d, W %d, coef %s, tao %g] one rank: loss err %.2e (tolerance %.2e), gradient err %.2e (tolerance %.2e)'
                  % (bs_r, K, W, coef, tao, el, tol_l, eg, tol_g))
            assert el < tol_l and eg < tol_g
            _, scaled_d = run(restacked.cuda(), bs, td, prm, scaler_state=state)
            # a power of two: exact on every element the unscaled call could store with all its bits; below 2^-126 that call
            # rounded to a multiple of 2^-149, which the scaled one need not have done
            normal = want_d.abs() >= 2.0 ** -126
            assert torch.equal(scaled_d[normal], want_d[normal] * 1024.0), 'the scale multiplies the gradient exactly'
            assert float((scaled_d.double() - 1024.0 * want_d.double()).abs().max()) <= 1024.0 * 2.0 ** -149
            want = {None: want_d.view(4, W, bs_r, K), state: scaled_d.view(4, W, bs_r, K)}
            for r in range(W):
                for sc in (None, state):
                    got_l = torch.full((1,), float('nan'), device='cuda')
                    got_d = torch.full((4 * bs_r, K), float('nan'), device='cuda')
                    lib.qua_loss_ranks(gathered, W, r, bs_r, td, prm, loss=got_l, dlogits=got_d, scaler_state=sc)
                    torch.cuda.synchronize()
                    assert torch.equal(got_l.cpu(), want_l), (r, coef, tao)
                    assert torch.equal(got_d.cpu().view(4, bs_r, K), want[sc][:, r]), (r, coef, tao, sc is not None)


@pytest.mark.parametrize('K', qr.ARGMAX_KS)
@pytest.mark.parametrize('bs', qr.ARGMAX_BSS)
def test_pair_argmax_against_float64(K, bs):
    from dmf import lib
    sets, first = qr.argmax_case(K, bs)
    for name in ('unit', 'gap', 'tie'):
        x = sets[name]
        pred = torch.full((bs,), -1, dtype=torch.int32, device='cuda')
        lib.pair_argmax(x.cuda(), bs, pred)
        torch.cuda.synchronize()
        pred = pred.cpu().long()
        if name == 'tie':
            assert torch.equal(pred, first), 'the first maximal index wins [K %d, bs %d]' % (K, bs)
            continue
        want, safe = qr.argmax_reference(x, bs)
        print('pair_argmax [K %d, bs %d, %s]: %d of %d rows compared, %d classes' % (K, bs, name, int(safe.sum()), bs, want.unique().numel()))
        assert torch.equal(pred[safe], want[safe]), '[K %d, bs %d, %s]' % (K, bs, name)
