"""GPU: every mode of the patch kernel past 512 patches, on class-diverse inputs, against the CPU oracle (oracle/gmfnet_ref.py).

A patch launch has grid = min(B, MAX_BLOCKS = 256); a workgroup walks patches b, b + 256, b + 512, ... with a counter `it`
(csrc/dmf_patch_v2.hip): `it == 0` stages the tables and waits at barrier X, `it > 0` accumulates the slab row in place, and in the
passes without barrier 2 (MODE_FWD, MODE_TOKENS) `(it & 1)` picks the half of the double-buffered pooled vector, so the third patch
is the first to rewrite a buffer an earlier patch used.  255 / 256 / 257 and 511 / 512 / 513 are the edges; 769 is a fourth patch.
unit_backward_kernel takes NPB = 4 patches per round, slot q <-> patch b0 + q * grid: 1,024 patches fill exactly one round, the
second starts at patch 1,024.  The attention forward has grid = min(B, 512): its third patch is patch 1,024.

Inputs come from tests/parity_cases.py: the head is centred so that the oracle's argmax takes many classes (its guards run on
the CPU in tests/test_parity_cases_host.py), no two patches of a batch are alike, and two patches of one workgroup are at least
2e-4 apart in some logit — a workgroup that mixes up its patches cannot pass.

Tolerances are the project's (tests/test_gpu_parity.py, test_gpu_seams.py, test_gpu_exit_path.py, test_gpu_half.py):
  logits <= 1e-5, per-patch loss <= 2.2e-5, gradients and workspace head vectors <= 1e-5 + 1e-4 |ref|;
  half: the same, against the oracle with the same roundings;
  attention: logits 2e-4 (batch-mean loss 2e-4), gradients 2e-5 + 2e-3 |ref|.
Every comparison prints its worst absolute error and the reference's magnitude; the worst per pass of one run are kept in
profiles/batch_walk_parity.md.
"""
import functools

import numpy as np
import pytest
import torch

import parity_cases as pc
from test_gpu_exit_path import split_ws
from test_gpu_seams import assert_close

pytestmark = pytest.mark.gpu

WORST = {}          # pass -> (worst abs err, max |ref| there, tolerance's absolute term)


def close(pass_, got, want, atol, rtol, what):
    got, want = got.detach().cpu(), want.detach().cpu()
    err = (got.double() - want.double()).abs().max().item() if got.numel() else 0.0
    if err >= WORST.get(pass_, (-1.0,))[0]:
        WORST[pass_] = (err, want.abs().max().item(), atol, rtol)
    assert_close(got, want, atol + rtol * want.double().abs(), what)


@pytest.fixture(scope='module', autouse=True)
def worst_errors_table():
    yield
    print('\n| pass | worst abs err | max abs ref | tolerance |')
    print('|---|---|---|---|')
    for k in sorted(WORST):
        e, r, atol, rtol = WORST[k]
        print('| %s | %.2e | %.2e | %g%s |' % (k, e, r, atol, ' + %g ref' % rtol if rtol else ''))


@functools.lru_cache(maxsize=None)
def gpu_case(name, B, half=False, attention=False):
    """The case, its HIP net and its inputs on the device (kept alive: input descriptors hold raw pointers)."""
    from model.gmfnet import PARAM_ORDER, Net as HipNet
    c = pc.case(name, B, half, attention)
    hip = HipNet(c['cfg'])
    hip.load_state_dict(c['state'])
    hip = hip.to('cuda:0')
    A = c['A'].cuda()
    d = dict(c, hip=hip, theta=hip.flat_parameters(), Ad=A.to(torch.float16) if half else A, Bd=c['Bm'].cuda(), xyd=c['xy'].cuda(),
             ad=c['a'].cuda(), bd=c['b'].cuda(), labels_d=c['labels'].int().cuda())
    off = hip._offsets
    d['views'] = {k: (off[i], c['grads'][k].numel(), c['grads'][k].shape) for i, k in enumerate(hip._order())}
    d['slab'] = (off[8] + 31) & ~31
    d['F2'] = 2 * hip.arch['F']
    assert PARAM_ORDER == hip._order()[:12]
    return d


def make_input(c, mode):
    from dmf import lib
    hip = c['hip']
    if mode == 'gather':
        lib.check_xy_bounds(hip.shape, c['Ad'], c['Bd'], c['xy'].numpy())
        inp = lib.input_gather(hip.shape, c['Ad'], c['Bd'], c['xyd'])
    else:
        inp = lib.input_patches(hip.shape, c['ad'], c['bd'], half=c['half'])
    assert inp.half == int(c['half'])
    return inp


def tag(c, *more):
    return c['what'][:-1] + ''.join(', ' + m for m in more) + ']'


def kind(c):
    return 'half' if c['half'] else 'fp32'


def check_grads(pass_, c, grad, want_g, what, atol=1e-5, rtol=1e-4):
    grad = grad.cpu()
    for k, want in want_g.items():
        o, n, shp = c['views'][k]
        close(pass_, grad[o:o + n].view(shp), want, atol, rtol, 'grad %s %s' % (k, what))


def check_head_vectors(pass_, c, ws, want_hv, keys, what):
    got = split_ws(ws.cpu(), c['slab'], c['B'], c['F2'], 64)
    for k in keys:
        close(pass_, got[k], want_hv[k], 1e-5, 1e-4, 'workspace %s %s' % (k, what))
    return got


def check_pred(c, pred, logits, what):
    """pred is the first maximal index of the GPU's own logits, exactly; and the oracle's class wherever the oracle's top-2
    margin stands clear of the logit tolerance."""
    pred = pred.cpu().long()
    assert torch.equal(pred, logits.cpu().argmax(1)), 'pred != argmax of the GPU logits ' + what
    safe = c['safe']
    assert torch.equal(pred[safe], c['pred'][safe]), 'pred != oracle class on %d safe patches %s' % (int(safe.sum()), what)
    print('pred %s: %d classes, %d of %d patches compared with the oracle' % (what, pred.unique().numel(), int(safe.sum()), c['B']))


# ------------------------------------------------------------------------------------------------------------- 1. forward
def forward_runs(c, mode):
    from dmf import lib
    hip, B, K = c['hip'], c['B'], c['K']
    inp = make_input(c, mode)
    logits = torch.full((B, K), float('nan'), device='cuda'); pred = torch.full((B,), -1, dtype=torch.int32, device='cuda')
    lib.forward(hip.shape, inp, c['theta'], hip.pool_w, logits, pred)
    logits_ce = torch.full((B, K), float('nan'), device='cuda'); loss = torch.full((B,), float('nan'), device='cuda')
    pred_ce = torch.full((B,), -1, dtype=torch.int32, device='cuda')
    lib.forward_ce(hip.shape, inp, c['theta'], hip.pool_w, c['labels_d'], logits_ce, loss, pred_ce)
    torch.cuda.synchronize()
    return dict(logits=logits.cpu(), pred=pred.cpu(), logits_ce=logits_ce.cpu(), loss=loss.cpu(), pred_ce=pred_ce.cpu())


@pytest.mark.parametrize('name,B,half', pc.walk_cases())
def test_forward_walk(name, B, half):
    """MODE_FWD: dmf_forward with pred and dmf_forward_ce, gather and materialised."""
    c = gpu_case(name, B, half)
    runs = {}
    for mode in ('gather', 'patches'):
        r = runs[mode] = forward_runs(c, mode)
        what = tag(c, mode)
        p = 'forward %s %s' % (kind(c), mode)
        close(p + ': logits', r['logits'], c['logits'], 1e-5, 0, 'forward logits ' + what)
        close(p + ': logits', r['logits_ce'], c['logits'], 1e-5, 0, 'forward_ce logits ' + what)
        close(p + ': loss', r['loss'], c['loss'], 2.2e-5, 0, 'forward_ce per-patch loss ' + what)
        check_pred(c, r['pred'], r['logits'], 'forward ' + what)
        check_pred(c, r['pred_ce'], r['logits_ce'], 'forward_ce ' + what)
    if B == 513:
        for k, v in runs['gather'].items():
            assert torch.equal(v, runs['patches'][k]), '%s: gather and materialised differ %s' % (k, tag(c))


# ------------------------------------------------------------------------------------- 2. train and backward outside fp32 gather
TRAIN_CELLS = [(n, B, h, m) for n, B, h in pc.walk_cases() for m in (('patches', 'gather') if h else ('patches',))]
BWD_CELLS = [(n, B, h, 'gather' if h else 'patches') for n, B, h in pc.walk_cases()]


@pytest.mark.parametrize('name,B,half,mode', TRAIN_CELLS)
def test_train_walk(name, B, half, mode):
    """MODE_TRAIN + the reduce: materialised fp32, materialised half, gather half."""
    from dmf import lib
    c = gpu_case(name, B, half)
    hip, K = c['hip'], c['K']
    inp = make_input(c, mode)
    logits = torch.full((B, K), float('nan'), device='cuda'); loss = torch.full((B,), float('nan'), device='cuda')
    ws = torch.zeros(lib.workspace_bytes(hip.shape, B) // 4, device='cuda')
    lib.train_fwd_bwd(hip.shape, inp, c['theta'], hip.pool_w, c['labels_d'], 1.0 / B, logits, loss, ws)
    grad = torch.empty_like(c['theta'])
    lib.grad_reduce(hip.shape, B, ws, grad)
    torch.cuda.synchronize()
    what, p = tag(c, mode), 'train %s %s' % (kind(c), mode)
    close(p + ': logits', logits, c['logits'], 1e-5, 0, 'train logits ' + what)
    close(p + ': loss', loss, c['loss'], 2.2e-5, 0, 'train per-patch loss ' + what)
    check_grads(p + ': grads', c, grad, c['grads'], what)
    if B == 513:
        check_head_vectors(p + ': z h dh dl', c, ws, c['hv'], ('z', 'h', 'dh', 'dl'), what)


@pytest.mark.parametrize('name,B,half,mode', BWD_CELLS)
def test_backward_dlogits_walk(name, B, half, mode):
    """MODE_BWD with the oracle's dL/dlogits: materialised fp32, gather half."""
    from dmf import lib
    c = gpu_case(name, B, half)
    hip = c['hip']
    inp = make_input(c, mode)
    ws = torch.zeros(lib.workspace_bytes(hip.shape, B) // 4, device='cuda')
    lib.backward_dlogits(hip.shape, inp, c['theta'], hip.pool_w, c['dlogits'].contiguous().cuda(), ws)
    grad = torch.empty_like(c['theta'])
    lib.grad_reduce(hip.shape, B, ws, grad)
    torch.cuda.synchronize()
    what, p = tag(c, mode, 'from dlogits'), 'backward %s %s' % (kind(c), mode)
    check_grads(p + ': grads', c, grad, c['grads'], what)
    if B == 513:
        got = check_head_vectors(p + ': z h dh dl', c, ws, c['hv'], ('z', 'h', 'dh', 'dl'), what)
        assert torch.equal(got['dl'], c['hv']['dl']), 'dl is passed through as supplied'


# ------------------------------------------------------------------------------------------------------------- 3. unit step
@pytest.mark.parametrize('name,B,half', pc.unit_cases())
def test_unit_step_walk(name, B, half):
    """MODE_UNIT + unit_backward_kernel + the reduce, gather mode, against autograd of the oracle for dl = randn / B."""
    from dmf import lib
    c = gpu_case(name, B, half)
    hip, K = c['hip'], c['K']
    assert lib.unit_supported(hip.shape)
    dl, want_g, want_hv = pc.unit_reference(c)
    inp = make_input(c, 'gather')
    logits = torch.full((B, K), float('nan'), device='cuda')
    ws = torch.zeros(lib.workspace_bytes(hip.shape, B) // 4, device='cuda')
    step = torch.full((1,), 7, dtype=torch.int32, device='cuda')
    lib.forward_unit(hip.shape, inp, c['theta'], hip.pool_w, logits, ws, adam_step_dev=step)
    lib.backward_unit(hip.shape, B, c['theta'], dl.cuda(), ws)
    grad = torch.empty_like(c['theta'])
    lib.grad_reduce(hip.shape, B, ws, grad)
    torch.cuda.synchronize()
    assert int(step.item()) == 8, 'the step count advances by exactly one'
    what, p = tag(c, 'unit step'), 'unit %s' % kind(c)
    close(p + ': logits', logits, c['logits'], 1e-5, 0, 'unit-step logits ' + what)
    check_grads(p + ': grads', c, grad, want_g, what)
    got = check_head_vectors(p + ': h dh dl', c, ws, want_hv, ('h', 'dh', 'dl'), what)
    assert torch.equal(got['dl'], want_hv['dl']), 'dl is passed through as supplied'


# ------------------------------------------------------------------------------------------------------------- 4. attention
@pytest.mark.parametrize('name,B', pc.ATTN_FORWARD)
def test_attention_forward_walk(name, B):
    """dmf_forward_attn (token pass with grid min(B, 256), attention forward with grid min(B, 512)), both input modes."""
    from dmf import lib
    c = gpu_case(name, B, False, True)
    hip, K = c['hip'], c['K']
    for mode in ('patches', 'gather'):
        inp = make_input(c, mode)
        logits = torch.full((B, K), float('nan'), device='cuda'); pred = torch.full((B,), -1, dtype=torch.int32, device='cuda')
        ws = torch.empty(lib.attn_workspace_bytes(hip.shape, B), dtype=torch.uint8, device='cuda')
        lib.forward_attn(hip.shape, inp, c['theta'], hip.pool_w, ws, logits, pred)
        torch.cuda.synchronize()
        what = tag(c, mode)
        close('attention forward %s: logits' % mode, logits, c['logits'], 2e-4, 0, 'attention logits ' + what)
        assert torch.equal(pred.cpu().long(), logits.cpu().argmax(1)), 'pred != argmax of the GPU logits ' + what
        assert pred.cpu().unique().numel() >= min(K, 4)


def attn_train(c, labels, dlogits, loss_scale):
    from dmf import lib
    hip, B, K = c['hip'], c['B'], c['K']
    inp = make_input(c, 'gather')
    logits = torch.full((B, K), float('nan'), device='cuda')
    loss = torch.full((B,), float('nan'), device='cuda') if labels is not None else None
    ws = torch.zeros(lib.workspace_bytes(hip.shape, B) // 4, device='cuda')
    aws = torch.empty(lib.attn_train_workspace_bytes(hip.shape, B), dtype=torch.uint8, device='cuda')
    lib.train_attn_fwd_bwd(hip.shape, inp, c['theta'], hip.pool_w, labels, dlogits, loss_scale, logits, loss, ws, aws)
    grad = torch.empty_like(c['theta'])
    lib.grad_reduce(hip.shape, B, ws, grad)
    torch.cuda.synchronize()
    return logits, loss, grad


def check_attention_grads(pass_, c, grad, what):
    check_grads(pass_, c, grad, c['grads'], what, 2e-5, 2e-3)
    for k, want in c['grads'].items():
        if k.startswith('attn_'):
            assert want.abs().max().item() > 1e-6, 'attention gradient vanishes: the test would prove nothing'


@pytest.mark.parametrize('name,B', pc.ATTN_TRAIN)
def test_attention_train_walk(name, B):
    """dmf_train_attn_fwd_bwd with labels, gather mode."""
    c = gpu_case(name, B, False, True)
    logits, loss, grad = attn_train(c, c['labels_d'], None, 1.0 / B)
    what = tag(c, 'gather')
    close('attention train gather: logits', logits, c['logits'], 2e-4, 0, 'attention train logits ' + what)
    mean_err = abs(loss.double().mean().item() - c['loss'].double().mean().item())
    print('attention train batch-mean loss %s: abs err %.3e' % (what, mean_err))
    assert mean_err < 2e-4
    check_attention_grads('attention train gather: grads', c, grad, what)


def test_attention_backward_from_dlogits_walk():
    """dmf_train_attn_fwd_bwd with the oracle's dL/dlogits, gather mode, tiny1 at 513."""
    c = gpu_case('tiny1', 513, False, True)
    logits, _, grad = attn_train(c, None, c['dlogits'].contiguous().cuda(), 1.0)
    what = tag(c, 'gather', 'from dlogits')
    close('attention dlogits gather: logits', logits, c['logits'], 2e-4, 0, 'attention logits ' + what)
    check_attention_grads('attention dlogits gather: grads', c, grad, what)


# ------------------------------------------------------------------------------------------------------------------ 5. ties
def tie_biases(K):
    """(bias, first maximal index): two and three equal maxima, and all entries equal; the others are distinct and lower."""
    out = []
    for idx in ((0, K - 1), (3, 4), (1, 3, K - 1), (2, 3, 4), tuple(range(K))):
        bias = -0.125 * (1 + torch.arange(K, dtype=torch.float32))
        bias[list(idx)] = 0.5
        out.append((bias, min(idx)))
    return out


@pytest.mark.parametrize('name', ['tiny1', 'hsi'])
@pytest.mark.parametrize('attention', [False, True])
def test_argmax_ties_take_the_first_maximal_index(name, attention):
    """fc2.weight = 0: every logit is exactly its bias.  The head wave's ballot / ffsll must give torch's rule."""
    from dmf import lib
    from model.gmfnet import Net as HipNet
    C, C2, P, S, K = pc.SHAPES[name]
    B = 3
    cfg = pc.build_cfg(name, False, attention)
    ref = pc.oracle_net(cfg)
    A, Bm, xy, t, a, b = pc.inputs(name, B)
    Ad, Bd, xyd, labels = A.cuda(), Bm.cuda(), xy.cuda(), t.int().cuda()
    for bias, first in tie_biases(K):
        with torch.no_grad():
            ref.fc2.weight.zero_()
            ref.fc2.bias.copy_(bias)
            want = ref(a, b)
        assert torch.equal(want, bias.expand(B, K)) and bool((want.argmax(1) == first).all())
        hip = HipNet(cfg)
        hip.load_state_dict(ref.state_dict())
        hip = hip.to('cuda:0')
        inp = lib.input_gather(hip.shape, Ad, Bd, xyd)
        theta = hip.flat_parameters()
        runs = {}
        if attention:
            logits = torch.full((B, K), float('nan'), device='cuda'); pred = torch.full((B,), -1, dtype=torch.int32, device='cuda')
            ws = torch.empty(lib.attn_workspace_bytes(hip.shape, B), dtype=torch.uint8, device='cuda')
            lib.forward_attn(hip.shape, inp, theta, hip.pool_w, ws, logits, pred)
            runs['forward_attn'] = (logits, pred)
        else:
            logits = torch.full((B, K), float('nan'), device='cuda'); pred = torch.full((B,), -1, dtype=torch.int32, device='cuda')
            lib.forward(hip.shape, inp, theta, hip.pool_w, logits, pred)
            runs['forward'] = (logits, pred)
            logits = torch.full((B, K), float('nan'), device='cuda'); pred = torch.full((B,), -1, dtype=torch.int32, device='cuda')
            loss = torch.empty(B, device='cuda')
            lib.forward_ce(hip.shape, inp, theta, hip.pool_w, labels, logits, loss, pred)
            runs['forward_ce'] = (logits, pred)
        torch.cuda.synchronize()
        for k, (logits, pred) in runs.items():
            assert torch.equal(logits.cpu(), want), '%s: the logits are the bias, bit for bit' % k
            assert pred.cpu().tolist() == [first] * B, '%s [%s]: bias %s -> pred %s, first maximal index %d' % (
                k, name, bias.tolist(), pred.cpu().tolist(), first)


# ------------------------------------------------------------------------------- 6. whole-set passes on a class-diverse net
ENGINE_SIZES = (256, 257, 600)          # 1,281 pixels: tail chunks of 1, 253 and 81


def reference_confusion(pred, labels, K):
    m = torch.zeros(K, K, dtype=torch.int64)
    m.index_put_((pred.long(), labels.long()), torch.ones(pred.numel(), dtype=torch.int64), accumulate=True)
    return m                                # rows = prediction


def whole_set_checks(make_engine, xy, labels, want_pred, safe, K, what):
    n = xy.shape[0]
    left_out = int((~safe).sum())
    assert left_out <= pc.MARGIN_CAP * n, '%d of %d pixels left out' % (left_out, n)
    x, y = xy[:, 0].long(), xy[:, 1].long()
    maps, mats = [], []
    for size in ENGINE_SIZES:
        eng = make_engine(size)
        lm = eng.label_map(xy, pc.H_SCENE, pc.W_SCENE).cpu()
        maps.append(lm)
        mats.append(eng.confusion(xy, labels.int()).cpu())
        sub = eng.confusion(xy[safe], labels[safe].int()).cpu()
        assert torch.equal(sub, reference_confusion(want_pred[safe], labels[safe], K)), 'confusion on the safe pixels, engine of %d %s' % (size, what)
        got = lm[x, y].long()
        assert torch.equal(got[safe], want_pred[safe]), 'label map on the safe pixels, engine of %d %s' % (size, what)
    for lm, m in zip(maps[1:], mats[1:]):
        assert torch.equal(lm, maps[0]) and torch.equal(m, mats[0]), 'engine sizes disagree ' + what
    assert int(mats[0].sum()) == n and torch.equal(mats[0].sum(0), torch.bincount(labels, minlength=K))
    touched = torch.zeros(pc.H_SCENE, pc.W_SCENE, dtype=torch.bool)
    touched[x, y] = True
    assert int(maps[0][~touched].abs().sum()) == 0, 'pixels outside the set stay untouched'
    print('whole set %s: %d classes on the map, %d of %d pixels left out of the oracle comparison' % (
        what, maps[0][x, y].unique().numel(), left_out, n))


@pytest.mark.parametrize('name,half,attention', pc.WHOLE_SET_CASES)
def test_label_map_and_confusion_over_the_whole_set(name, half, attention):
    """EvalEngine.label_map / .confusion over 1,281 pixels in chunks of 256, 257 and 600."""
    from dmf.engine import EvalEngine, Scene
    c = gpu_case(name, pc.WHOLE_SET, half, attention)
    scene = Scene(c['A'].numpy(), c['Bm'].numpy(), 'cuda:0', half=half)
    whole_set_checks(lambda size: EvalEngine(c['hip'], scene, size), c['xy'], c['labels'], c['pred'], c['safe'], c['K'], c['what'])


def test_stage2_label_map_and_confusion_over_the_whole_set():
    """QuaEvalEngine (argmax of the ms + pan streams' summed logits) the same way, on quatiny."""
    from dmf.engine import QuaEvalEngine, QuaScene
    from model.gmfnet import Net as HipNet
    q = pc.qua_eval_case()
    hip = HipNet(q['cfg'])
    hip.load_state_dict(q['state'])
    hip = hip.to('cuda:0')
    scene = QuaScene(q['scenes'], 'cuda:0')
    whole_set_checks(lambda size: QuaEvalEngine(hip, scene, size), q['xy'], q['labels'], q['pred'], q['safe'], q['K'],
                     '[%s, stage 2]' % q['name'])
