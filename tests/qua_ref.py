"""The stage-2 loss (`qua_loss`, train/loss_function.py:15-76) on the CPU, for the tests of dmf_qua_loss / dmf_qua_loss_ranks /
dmf_pair_argmax: the oracle (oracle/datapath_ref.py::qua_loss, unchanged) in the dtype asked for, a float32 restatement with the
kernel's limits, and the cases of tests/test_gpu_qua_parity.py — whose preconditions tests/test_qua_cases_host.py checks on the CPU.

The kernel has three forms (csrc/dmf_qua.hip::launch_qua_loss): element-parallel (K <= 16, bs <= 16 QE_MAXG), one tiled workgroup
with the class loops unrolled to 16 (K <= 16, larger batches) and one with run-time class loops (K >= 17); a tiled batch that fits
one tile of ts = min(256, 38400 / (10 K)) samples makes its softmax rows once.  `form()` restates that dispatch, CASES are the
smallest batches that reach each form and each of its edges.

Limits (include/dmf.h, beside dmf_qua_loss): y log y and its derivative are 0 at y == 0; exp(-|c / y|) and its derivative are 0
where the exponential has underflowed.  The float64 oracle needs neither on the logits used here (no float64 probability is 0);
the same oracle in float32 is NaN on the `wide` set, which is why the reference of the GPU test is float64.
"""
import functools
import os

import torch

from oracle import datapath_ref as dref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_SRC = os.path.join(REPO, 'dual-modal-fusion_amd', 'csrc', 'dmf_qua.hip')

# ------------------------------------------------------------------------------------------------------ the kernel's dispatch
QE_MAXG = 256             # workgroups of 16 samples the element-parallel form takes
QT = 1024                 # threads (and reduction floats in LDS) of the tiled form's one workgroup
LDS_BUDGET = 150 * 1024   # bytes of softmax rows and logarithms a tile may hold
ROW_FLOATS = 10           # per sample and class: 4 probabilities, 4 log(. + eps), 2 log(.)
LDS_LIMIT = 160 * 1024    # dynamic LDS the tiled kernels ask for


def tile(bs, K):
    ts = (LDS_BUDGET // 4) // (ROW_FLOATS * K)
    return min(bs, min(256, max(1, ts)))


def form(bs, K):
    """(kernel form, number of workgroups [element] or of tiles [tiled]) that launch_qua_loss takes for a batch."""
    if K <= 16 and bs <= 16 * QE_MAXG:
        return 'element', (bs + 15) // 16
    return ('tiled16' if K <= 16 else 'tiled0'), -(-bs // tile(bs, K))


def lds_bytes(bs, K):
    return (QT + ROW_FLOATS * tile(bs, K) * K) * 4


ROWS = ('element-parallel', 'tiled <16>', 'tiled <0>, one tile', 'tiled <0>, several tiles')
CASES = [(ROWS[0], 3, 2), (ROWS[0], 16, 16), (ROWS[0], 17, 16), (ROWS[0], 33, 15), (ROWS[0], 4096, 16),
         (ROWS[1], 4097, 16), (ROWS[1], 4097, 3),
         (ROWS[2], 225, 17), (ROWS[2], 60, 64),
         (ROWS[3], 226, 17), (ROWS[3], 61, 64), (ROWS[3], 130, 33)]
RANK_CASES = [(6, 16, 3), (75, 17, 3), (76, 17, 3)]           # (bs_r, K, W), on the `wide` set
COEFS = [(0.1, 0.05, 1.0), (0.0, 0.05, 1.0), (0.1, 0.0, 1.0), (0.3, 0.2, 0.5)]      # (alpha, beta, gamma) of test_gpu_stage2.py
TAOS = [0.1, -0.5]
EPS = 1e-8
SETS = ('unit', 'wide')


def in_row(row, bs, K):
    """Does (bs, K) run in the form its row of the table claims?"""
    f, n = form(bs, K)
    return {ROWS[0]: f == 'element', ROWS[1]: f == 'tiled16', ROWS[2]: f == 'tiled0' and n == 1,
            ROWS[3]: f == 'tiled0' and n > 1}[row]


# ------------------------------------------------------------------------------------------------------------- the logits
STREAMS = ((0,), (1,), (3,), (1, 2))      # p, q, s, q + r: the stream(s) whose class is lowered
OFFSETS = (52.0, 60.0, 80.0, 104.0, 120.0)
TINY = 2.6e-23                            # below it the square of a float32 probability is 0


def lowered(i):
    """(streams, offset) of sample i in the `wide` set: both cycles, all 20 pairs within any 20 consecutive samples."""
    return STREAMS[i % 4], OFFSETS[i % 5]


@functools.lru_cache(maxsize=None)
def case(bs, K):
    """(labels [bs] int64, {'unit': 2 randn, 'wide': the same with class i mod K of sample i lowered}) — logits [4 bs, K]."""
    g = torch.Generator().manual_seed(1000 * K + bs)
    unit = 2.0 * torch.randn(4 * bs, K, generator=g)
    t = torch.randint(0, K, (bs,), generator=g)
    wide = unit.clone().view(4, bs, K)
    for i in range(bs):
        streams, off = lowered(i)
        for st in streams:
            wide[st, i, i % K] -= off
    return t, {'unit': unit, 'wide': wide.view(4 * bs, K)}


# --------------------------------------------------------------------------------------------------------- the references
def value_and_grad(x, bs, t, dtype, coef, eps, tao):
    """(loss, d loss / d logits) of the oracle evaluated in `dtype` on the same logits, both as float64.  The oracle makes its
    one-hot labels in torch's default dtype, so that is `dtype` for the call: in float64 nothing of it is float32."""
    alpha, beta, gamma = coef
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        z = x.detach().to(dtype).clone().requires_grad_(True)
        v = dref.qua_loss(z, bs, t.to(dtype), alpha, beta, gamma, eps, tao)
        v.backward()
    finally:
        torch.set_default_dtype(old)
    return v.detach().double(), z.grad.double()


def kl_sums(x, bs, eps, dtype=torch.float64):
    """A1 A2 A3 B1 B2 B3 of csrc/dmf_qua.hip (D(q>p) D(r>p) D(s>p) D(p>q) D(r>q) D(s>q)) in `dtype`; d1 = A3 - A2 + tao,
    d2 = B3 - B2 + tao are the arguments of the loss's two absolute values."""
    y = x.to(dtype).softmax(dim=-1)
    p, q, r, s = y[:bs], y[bs:2 * bs], y[2 * bs:3 * bs], y[3 * bs:]

    def kl(src, tgt):
        return (torch.xlogy(tgt, tgt) - tgt * (src + eps).log()).sum() / bs
    return [kl(q, p), kl(r, p), kl(s, p), kl(p, q), kl(r, q), kl(s, q)]


def kink_arguments(x, bs, eps, tao):
    A1, A2, A3, B1, B2, B3 = kl_sums(x, bs, eps)
    return (A3 - A2 + tao).item(), (B3 - B2 + tao).item()


def guarded32(x, bs, t, coef, eps, tao):
    """The loss in float32 torch with the kernel's limits, value and gradient as float64.  Not a reference: it only shows that
    float32 arithmetic can meet the tolerance the kernel is held to against float64."""
    alpha, beta, gamma = coef
    z = x.detach().float().clone().requires_grad_(True)
    y = z.softmax(dim=-1)
    p, q, r, s = y[:bs], y[bs:2 * bs], y[2 * bs:3 * bs], y[3 * bs:]
    one, zero = torch.ones_like(p), torch.zeros_like(p)

    def xlogx(v):                                  # 0 with a zero derivative at v == 0
        on = v > 0
        return torch.where(on, v * torch.where(on, v, one).log(), zero)

    def kl(src, tgt):
        return (xlogx(tgt) - tgt * (src + eps).log()).sum() / bs

    def damp(c, v):                                # exp(-|c / v|); 0 with zero derivatives where it has underflowed
        with torch.no_grad():
            on = (v > 0) & (torch.exp(-(c / v).abs()) > 0)
        return torch.where(on, torch.exp(-(c / torch.where(on, v, one)).abs()), zero)

    A1, A2, A3, B1, B2, B3 = kl(q, p), kl(r, p), kl(s, p), kl(p, q), kl(r, q), kl(s, q)
    l12 = (A1 + A2 + (A3 - A2 + tao).abs()) + (B1 + B2 + (B3 - B2 + tao).abs())
    l3 = (damp(A3, p) + damp(B3, q)).mean()
    l = torch.zeros_like(p).scatter_(1, t.long().view(-1, 1), 1.0).softmax(dim=-1)      # softmax OF the one-hot
    l4 = (l * (l.log() - (p + q).log_softmax(dim=-1))).sum() / bs
    v = alpha * l12 + beta * l3 + gamma * l4
    v.backward()
    return v.detach().double(), z.grad.double()


def tolerances(ref_loss, ref_grad):
    """The project's own (tests/test_gpu_stage2.py::test_qua_loss_kernel_against_oracle)."""
    return 2e-6 * max(1.0, abs(float(ref_loss))), 1e-7 + 1e-4 * ref_grad.abs().max().item()


# ---------------------------------------------------------------------------------------------------- dmf_pair_argmax's cases
ARGMAX_KS, ARGMAX_BSS = (2, 17, 64), (1, 255, 256, 257)
ARGMAX_MARGIN = 1e-5


@functools.lru_cache(maxsize=None)
def argmax_case(K, bs):
    """{'unit': 2 randn, 'gap': the same with one class raised so that every other summed logit lies more than 104 below it
    (its softmax term underflows), 'tie': sums that are exactly equal at two or three classes} — logits [2 bs, K] each —
    and the first maximal index of every `tie` row."""
    g = torch.Generator().manual_seed(77 * K + bs)
    unit = 2.0 * torch.randn(2 * bs, K, generator=g)
    gap = unit.clone()
    top = torch.randint(0, K, (bs,), generator=g)
    rows = torch.arange(bs)
    gap[rows, top] += 70.0                        # 140 on the sum; the unit sums spread over about +- 12
    gap[bs + rows, top] += 70.0
    # multiples of 1/8 below 16 in magnitude: every sum is exact in float32
    a = torch.randint(-64, 0, (bs, K), generator=g).float() / 8.0
    b = torch.randint(-64, 0, (bs, K), generator=g).float() / 8.0
    first = torch.empty(bs, dtype=torch.int64)
    for i in range(bs):
        idx = torch.randperm(K, generator=g)[:min(K, 2 + i % 2)]
        a[i, idx] = torch.tensor([1.5, -0.25, 3.0])[:len(idx)]         # different addends, the same sum
        b[i, idx] = torch.tensor([0.5, 2.25, -1.0])[:len(idx)]
        first[i] = idx.min()
    return {'unit': unit, 'gap': gap, 'tie': torch.cat([a, b])}, first


def argmax_reference(x, bs):
    """(float64 argmax of the summed logits, rows whose float64 top-2 margin exceeds ARGMAX_MARGIN)."""
    z = x[:bs].double() + x[bs:2 * bs].double()
    top = z.topk(2, dim=1).values
    return z.argmax(1), (top[:, 0] - top[:, 1]) > ARGMAX_MARGIN
