"""GPU: a launch reads nothing that no launch wrote, and writes nothing outside the extents its arguments state.

The engines allocate their workspaces with torch.empty and reuse them for every step, also for a smaller batch (step_short), so
"a workspace needs no initialisation" is a contract of every training run.  Every assertion here
is bit-equality of a launch with itself under other surroundings, or a check that canary bytes are intact: no oracle, no tolerance.

  a. nothing stale is read   every launch sequence once per fill of mem_cases.FILLS (0x00, 0xFF = NaN, 0x47 = a large finite value
                             that survives a ReLU, 0x00 again): workspaces and outputs come from mem_cases.guarded(.., fill), the
                             inputs and the optimiser state from pristine copies; every DEFINED output is bit-equal across the
                             runs and free of NaN, every guard intact — of the outputs and of the inputs.
  b. one workspace, several  a workspace sized for 513 patches runs 513, then 3, 257 and 1 (what step_short does): each result is
     batch sizes             bit-equal to the same launch in a fresh zero workspace.
  c. beside the scene        gather mode with the scenes, xy and labels in guarded allocations, the batch on every corner and edge
                             of the padded scene: outputs bit-equal across guard contents 0xA5, 0xFF and 0x00.
  d. tails                   optimiser, loss, row and scene-preparation launches at n = 255 / 256 / 257 ..., outputs guarded.
  e. the engines             TrainEngine, QuaTrainEngine and EvalEngine as they run, their buffers byte-filled after construction.

Defined outputs: logits [B, K], loss [B], pred [B], the reduced gradient; theta, m, v (avg) after an update; the scaler state, the
step and cursor counters, loss_hist / norm_hist at the cursor; the workspace's head vectors z, h, dh and dl[:, :K] of rows < B.
Everything else in a workspace is undefined and is not compared.  The workspaces hold float data and bf16 tokens only — no word
of them is ever an index or an address (csrc/dmf_shapes.h: make_ws; csrc/dmf_capi.hip: attn_ws) — so arbitrary bytes in them
are what torch.empty gives a training run.  Cases and helpers: tests/mem_cases.py.
"""
import functools

import numpy as np
import pytest
import torch

import mem_cases as mc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
HP = (1e-3, 0.9, 0.999, 1e-8)                     # lr, beta1, beta2, eps
SCALER_HP = (2.0, 0.5, 2000)                      # growth factor, backoff factor, growth interval


# ------------------------------------------------------------------------------------------------------------------- helpers
class Pool:
    """The guarded allocations of one run; `check` asserts that every guard is intact."""

    def __init__(self, fill=0x00, canary=mc.CANARY):
        self.fill, self.canary, self.held = fill, canary, []

    def new(self, name, shape, dtype=torch.float32, fill=None):
        n = int(np.prod(shape))
        view, whole = mc.guarded(n, dtype, DEV, self.fill if fill is None else fill, self.canary)
        self.held.append((name, whole, n, dtype))
        return view.view(*shape)

    def put(self, name, t):
        v = self.new(name, tuple(t.shape), t.dtype, 0x00)
        v.copy_(t)
        return v

    def check(self, what):
        torch.cuda.synchronize()
        for name, whole, n, dtype in self.held:
            d = mc.intact(whole, n, dtype, self.canary)
            assert d, '%s: the guards of %s are %r' % (what, name, d)


def same_bits(runs, what, labels=None):
    """Every entry of the dicts `runs` is bit-equal to the first run's, and no floating-point entry holds a NaN."""
    first = runs[0]
    for k, v in first.items():
        if v.is_floating_point():
            assert not torch.isnan(v).any(), '%s: %s holds a NaN (%d of %d)' % (what, k, int(torch.isnan(v).sum()), v.numel())
    for i, r in enumerate(runs[1:], 1):
        assert r.keys() == first.keys()
        for k, v in first.items():
            a, b = mc.bits(v), mc.bits(r[k])
            if not torch.equal(a, b):
                bad = (a != b).reshape(-1).nonzero().reshape(-1)
                raise AssertionError('%s: %s differs between %s and %s in %d of %d elements, first at %d' % (
                    what, k, labels[0] if labels else 'run 0', labels[i] if labels else 'run %d' % i, bad.numel(), a.numel(), int(bad[0])))


def fill_name(i, fill):
    return 'fill 0x%02X (run %d)' % (fill, i)


FILL_LABELS = [fill_name(i, f) for i, f in enumerate(mc.FILLS)]


class Case:
    """One shape / batch / class count: the net, and its inputs in guarded allocations (gather mode and materialised)."""

    def __init__(self, name, B, K, attention=False, half=False, extra=0, canary=mc.CANARY):
        from dmf import lib
        self.name, self.B, self.K, self.half = name, B, K, half
        self.net = mc.nets(name, K, attention)
        self.shape = self.net.shape
        A, Bm, xy, t, dl = mc.scene_batch(name, B, K, extra=extra)
        self.host = (A, Bm, xy)
        self.inputs = Pool(canary=canary)
        self.theta0 = self.net.flat_parameters().clone()
        self.theta = self.inputs.put('theta', self.theta0)
        self.pool_w = self.inputs.put('pool_w', self.net.pool_w)
        self.A = self.inputs.put('sceneA', A.to(DEV).half() if half else A.to(DEV))
        self.Bm = self.inputs.put('sceneB', Bm.to(DEV))
        self.xy = self.inputs.put('xy', xy.to(DEV))
        self.labels = self.inputs.put('labels', t.to(DEV))
        self.dl = self.inputs.put('dlogits (input)', dl.to(DEV))
        lib.check_xy_bounds(self.shape, self.A, self.Bm, xy.numpy())
        off = self.net._offsets
        self.slab = (off[8] + 31) & ~31
        self.F2 = 2 * mc.SHAPES[name][5]
        self.n = self.theta0.numel()
        self._patches = None

    def gather(self, B=None):
        from dmf import lib
        B = self.B if B is None else B
        return lib.input_gather(self.shape, self.A, self.Bm, self.xy[:B])

    def patches(self):
        from dmf import lib
        if self._patches is None:
            A, Bm, xy = self.host
            a, b = mc.patches_of(self.name, A, Bm, xy)
            self._patches = (self.inputs.put('a', a.to(DEV)), self.inputs.put('b', b.to(DEV)))
        return lib.input_patches(self.shape, *self._patches, half=self.half)

    def restore(self):
        self.theta.copy_(self.theta0)

    def heads(self, ws, B):
        """The workspace's defined head vectors of rows < B: z, h, dh and dl[:, :K]."""
        hv = mc.split_ws(ws.reshape(-1).cpu(), self.slab, B, self.F2, 64)
        hv['dl'] = hv['dl'][:, :self.K]
        return {'ws.' + k: v.contiguous() for k, v in hv.items()}


@functools.lru_cache(maxsize=2)
def case(name, B, K, attention=False, half=False):
    return Case(name, B, K, attention, half)


def ws_floats(c, B):
    from dmf import lib
    return lib.workspace_bytes(c.shape, B) // 4


def train_buffers(c, B, pool, variant, ws=None):
    """The buffers of one train sequence on B patches; `pool` makes the outputs, the optimiser state starts from zeros."""
    from dmf import lib
    rows = 4 * B if variant == 'unit_qua' else B
    b = dict(ws=pool.new('workspace', (ws_floats(c, rows),)) if ws is None else ws,
             logits=pool.new('logits', (rows, c.K)), loss=pool.new('loss', (rows,)), grad=pool.new('grad', (c.n,)))
    if variant in ('unit_ce', 'unit_qua'):
        b['dlogits'] = pool.new('dlogits', (rows, c.K))
    if variant == 'unit_qua':
        b['loss'] = pool.new('loss', (1,))
    if variant in ('adam', 'scaled', 'plan'):
        b['m'] = pool.put('m', torch.zeros(c.n, device=DEV)); b['v'] = pool.put('v', torch.zeros(c.n, device=DEV))
        b['step'] = pool.put('step', torch.zeros(1, dtype=torch.int32, device=DEV))
        b['cursor'] = pool.put('cursor', torch.zeros(1, dtype=torch.int32, device=DEV))
        b['loss_hist'] = pool.new('loss_hist', (4,))
    if variant == 'scaled':
        state = torch.zeros(lib.SCALER_FLOATS, device=DEV)
        lib.scaler_init(state, 1024.0)
        b['state'] = pool.put('scaler state', state)
    return b


def train_launch(c, B, b, variant, inp=None):
    """One train sequence on the first B patches of the case -> its defined outputs (host copies)."""
    from dmf import lib
    sh, th, pw, lab = c.shape, c.theta, c.pool_w, c.labels
    rows = B
    out = {}
    if variant in ('reduce', 'adam', 'scaled'):
        inp = c.gather(B) if inp is None else inp
        if variant == 'reduce':
            lib.train_fwd_bwd(sh, inp, th, pw, lab, 1.0 / B, b['logits'], b['loss'], b['ws'])
            lib.grad_reduce(sh, B, b['ws'], b['grad'])
        elif variant == 'adam':
            lib.train_fwd_bwd(sh, inp, th, pw, lab, 1.0 / B, b['logits'], b['loss'], b['ws'], adam_step_dev=b['step'])
            lib.grad_reduce_adam(sh, B, b['ws'], th, b['m'], b['v'], b['grad'], *HP, 0, adam_step_dev=b['step'], cursor_dev=b['cursor'],
                                 loss=b['loss'], loss_hist=b['loss_hist'])
        else:
            lib.train_fwd_bwd(sh, inp, th, pw, lab, 1.0 / B, b['logits'], b['loss'], b['ws'], adam_step_dev=b['step'],
                              scaler_state=b['state'])
            lib.grad_reduce_scaled(sh, B, b['ws'], b['grad'], b['state'], cursor_dev=b['cursor'], loss=b['loss'], loss_hist=b['loss_hist'])
            lib.unscale_adam(th, b['grad'], b['m'], b['v'], *HP, b['state'], *SCALER_HP, b['step'], unscaled=True)
        out.update(logits=b['logits'], loss=b['loss'])
    elif variant == 'dlogits':
        inp = c.gather(B) if inp is None else inp
        lib.backward_dlogits(sh, inp, th, pw, c.dl[:B], b['ws'])
        lib.grad_reduce(sh, B, b['ws'], b['grad'])
    elif variant == 'unit_ce':
        inp = c.gather(B) if inp is None else inp
        lib.forward_unit(sh, inp, th, pw, b['logits'], b['ws'])
        lib.ce_loss(b['logits'], 1, 0, lab[:B], lib.ce_params('ce', label_smoothing=0.1), loss=b['loss'], dlogits=b['dlogits'])
        lib.backward_unit(sh, B, th, b['dlogits'], b['ws'])
        lib.grad_reduce(sh, B, b['ws'], b['grad'])
        out.update(logits=b['logits'], loss=b['loss'], dlogits=b['dlogits'])
    elif variant == 'unit_qua':                   # the case holds 4 B patches: four streams of B samples
        rows = 4 * B
        inp = c.gather(rows) if inp is None else inp
        lib.forward_unit(sh, inp, th, pw, b['logits'], b['ws'])
        lib.qua_loss(b['logits'], B, lab[:B], lib.QuaParams(alpha=0.1, beta=0.05, gamma=1.0, epsilon=1e-8, tao=0.1), loss=b['loss'],
                     dlogits=b['dlogits'])
        lib.backward_unit(sh, rows, th, b['dlogits'], b['ws'])
        lib.grad_reduce(sh, rows, b['ws'], b['grad'])
        out.update(logits=b['logits'], loss=b['loss'], dlogits=b['dlogits'])
    else:
        raise ValueError(variant)
    out['grad'] = b['grad']
    if variant in ('adam', 'scaled'):
        out.update(theta=th, m=b['m'], v=b['v'], step=b['step'], cursor=b['cursor'], loss_hist=b['loss_hist'][:1])
    if variant == 'scaled':
        out['scaler state'] = b['state']
    torch.cuda.synchronize()
    out = {k: v.detach().cpu().clone() for k, v in out.items()}
    out.update(c.heads(b['ws'], rows))
    return out


def train_across_fills(c, B, variant, what, inp=None):
    runs = []
    for i, fill in enumerate(mc.FILLS):
        c.restore()
        pool = Pool(fill)
        b = train_buffers(c, B, pool, variant)
        runs.append(train_launch(c, B, b, variant, inp))
        tag = '%s, %s' % (what, fill_name(i, fill))
        pool.check(tag)
        c.inputs.check(tag)
    same_bits(runs, what, FILL_LABELS)
    return runs


def what_of(seq, name, B, K, more=''):
    return '%s [%s, B = %d, K = %d%s]' % (seq, name, B, K, more)


def cases(table):
    """parametrize('name,B,K', **cases(table))"""
    return dict(argvalues=table, ids=[mc.case_id(c) for c in table])


PATCH = mc.patch_cases()
UNIT = mc.patch_cases(unit=True)
HALF = [x for x in PATCH if x[0] in ('tiny1', 'qua', 'hsi', 'hsi224', 'pca32') and x[2] not in mc.K_ENDS]
BOTH_INPUTS = [x for x in PATCH if x[0] in ('tiny1', 'hsi') and x[2] not in mc.K_ENDS]


# =========================================================================================== a. nothing stale is read
# ----------------------------------------------------------------------------------------------- a1. the forward launches
def forward_runs(c, inp, what):
    from dmf import lib
    runs = []
    for i, fill in enumerate(mc.FILLS):
        pool = Pool(fill)
        l0, l1, l2 = (pool.new('logits', (c.B, c.K)) for _ in range(3))
        p1, p2 = pool.new('pred', (c.B,), torch.int32), pool.new('pred', (c.B,), torch.int32)
        loss = pool.new('loss', (c.B,))
        lib.forward(c.shape, inp, c.theta, c.pool_w, l0)
        lib.forward(c.shape, inp, c.theta, c.pool_w, l1, p1)
        lib.forward_ce(c.shape, inp, c.theta, c.pool_w, c.labels, l2, loss, p2)
        torch.cuda.synchronize()
        runs.append({k: v.cpu().clone() for k, v in dict(logits=l0, logits_with_pred=l1, pred=p1, ce_logits=l2, ce_loss=loss,
                                                         ce_pred=p2).items()})
        tag = '%s, %s' % (what, fill_name(i, fill))
        pool.check(tag)
        c.inputs.check(tag)
    same_bits(runs, what, FILL_LABELS)
    r = runs[0]
    assert torch.equal(r['logits'], r['logits_with_pred']) and torch.equal(r['logits'], r['ce_logits']) and torch.equal(r['pred'], r['ce_pred'])
    assert int(r['pred'].min()) >= 0 and int(r['pred'].max()) < c.K
    return r


@pytest.mark.parametrize('name,B,K', **cases(PATCH))
def test_forward_reads_nothing_stale(name, B, K):
    """dmf_forward without and with pred, dmf_forward_ce; gather and materialised input give the same bits."""
    c = case(name, B, K)
    g = forward_runs(c, c.gather(), what_of('forward, gather', name, B, K))
    p = forward_runs(c, c.patches(), what_of('forward, patches', name, B, K))
    same_bits([g, p], what_of('forward', name, B, K), ['gather', 'patches'])


@pytest.mark.parametrize('name,B,K', **cases(HALF))
def test_forward_half_reads_nothing_stale(name, B, K):
    from dmf import lib
    c = case(name, B, K, False, True)
    lib.require_half(c.shape)
    g = forward_runs(c, c.gather(), what_of('forward, fp16 scene, gather', name, B, K))
    p = forward_runs(c, c.patches(), what_of('forward, fp16 rounding, patches', name, B, K))
    same_bits([g, p], what_of('forward, fp16', name, B, K), ['gather', 'patches'])


# ------------------------------------------------------------------------------------------- a2 - a5. the train sequences
@pytest.mark.parametrize('variant', ['reduce', 'adam', 'scaled', 'dlogits'])
@pytest.mark.parametrize('name,B,K', **cases(PATCH))
def test_train_sequence_reads_nothing_stale(name, B, K, variant):
    """dmf_train_fwd_bwd -> dmf_grad_reduce | -> dmf_grad_reduce_adam | _scaled -> dmf_grad_reduce_scaled -> dmf_unscale_adam |
    dmf_backward_dlogits -> dmf_grad_reduce."""
    c = case(name, B, K)
    train_across_fills(c, B, variant, what_of(variant, name, B, K))


@pytest.mark.parametrize('name,B,K', **cases(BOTH_INPUTS))
def test_train_sequence_from_patches_and_half(name, B, K):
    """The materialised input of the fused step, and the fp16 scene: nothing stale, and patches == gather bit for bit."""
    c = case(name, B, K)
    g = train_across_fills(c, B, 'reduce', what_of('reduce, gather', name, B, K))
    p = train_across_fills(c, B, 'reduce', what_of('reduce, patches', name, B, K), inp=c.patches())
    same_bits([g[0], p[0]], what_of('reduce', name, B, K), ['gather', 'patches'])
    h = case(name, B, K, False, True)
    train_across_fills(h, B, 'reduce', what_of('reduce, fp16 scene', name, B, K))


# ------------------------------------------------------------------------------------------------- a6. the unit route
@pytest.mark.parametrize('name,B,K', **cases(UNIT))
def test_unit_route_reads_nothing_stale(name, B, K):
    """dmf_forward_unit -> dmf_ce_loss (stage 2: dmf_qua_loss on 4 x B rows) -> dmf_backward_unit -> dmf_grad_reduce."""
    from dmf import lib
    if name in mc.QUA:
        c = case(name, 4 * B, K)
        train_across_fills(c, B, 'unit_qua', what_of('unit route, qua_loss', name, 4 * B, K))
    else:
        c = case(name, B, K)
        train_across_fills(c, B, 'unit_ce', what_of('unit route, ce_loss', name, B, K))


# ------------------------------------------------------------------------------------------------ a7. the native loop
@pytest.mark.parametrize('name,B,K', **cases(PATCH))
def test_plan_steps_read_nothing_stale(name, B, K):
    """dmf_train_plan_steps: 3 steps on the consecutive batches of B patches of a plan of 3 B."""
    from dmf import lib
    steps, nb = 3, B
    c = case(name, steps * B, K)
    runs = []
    what = what_of('plan steps', name, nb, K, ', %d steps' % steps)
    for i, fill in enumerate(mc.FILLS):
        c.restore()
        pool = Pool(fill)
        b = train_buffers(c, nb, pool, 'plan')
        inp = lib.input_gather(c.shape, c.A, c.Bm, c.xy[:steps * nb], B=nb)
        lib.train_plan_steps(c.shape, inp, c.theta, c.pool_w, c.labels, 1.0 / nb, b['logits'], b['loss'], b['ws'], b['m'], b['v'], *HP,
                             b['step'], b['cursor'], b['loss_hist'], steps)
        torch.cuda.synchronize()
        out = dict(logits=b['logits'], loss=b['loss'], theta=c.theta, m=b['m'], v=b['v'], step=b['step'], cursor=b['cursor'],
                   loss_hist=b['loss_hist'][:steps])
        out = {k: v.cpu().clone() for k, v in out.items()}
        out.update(c.heads(b['ws'], nb))
        runs.append(out)
        tag = '%s, %s' % (what, fill_name(i, fill))
        pool.check(tag)
        c.inputs.check(tag)
        assert int(out['step']) == steps and int(out['cursor']) == steps
    same_bits(runs, what, FILL_LABELS)


# ---------------------------------------------------------------------------------------------------- a8. attention
def attn_buffers(c, pool, train):
    from dmf import lib
    B = c.B
    if not train:
        return dict(aws=pool.new('attention workspace', (lib.attn_workspace_bytes(c.shape, B),), torch.uint8),
                    logits=pool.new('logits', (B, c.K)), pred=pool.new('pred', (B,), torch.int32))
    return dict(aws=pool.new('attention train workspace', (lib.attn_train_workspace_bytes(c.shape, B),), torch.uint8),
                ws=pool.new('workspace', (ws_floats(c, B),)), logits=pool.new('logits', (B, c.K)), loss=pool.new('loss', (B,)),
                grad=pool.new('grad', (c.n,)))


@pytest.mark.parametrize('name,B,K', **cases(mc.attn_cases()))
@pytest.mark.parametrize('route', ['forward', 'labels', 'dlogits', 'criterion'])
def test_attention_reads_nothing_stale(name, B, K, route):
    """dmf_forward_attn; dmf_train_attn_fwd_bwd from labels and from dlogits, dmf_train_attn_fwd_bwd_ce; each -> dmf_grad_reduce."""
    from dmf import lib
    c = case(name, B, K, True)
    what = what_of('attention ' + route, name, B, K)
    inp = c.patches() if B <= 257 else c.gather()
    runs = []
    for i, fill in enumerate(mc.FILLS):
        pool = Pool(fill)
        b = attn_buffers(c, pool, route != 'forward')
        if route == 'forward':
            lib.forward_attn(c.shape, inp, c.theta, c.pool_w, b['aws'], b['logits'], b['pred'])
            out = dict(logits=b['logits'], pred=b['pred'])
        else:
            if route == 'labels':
                lib.train_attn_fwd_bwd(c.shape, inp, c.theta, c.pool_w, c.labels, None, 1.0 / B, b['logits'], b['loss'], b['ws'], b['aws'])
            elif route == 'dlogits':
                lib.train_attn_fwd_bwd(c.shape, inp, c.theta, c.pool_w, None, c.dl, 1.0, b['logits'], None, b['ws'], b['aws'])
            else:
                denom = pool.new('denom', (1,), torch.float64)
                lib.ce_denominators(c.labels, B, K, denom)
                lib.train_attn_fwd_bwd_ce(c.shape, inp, c.theta, c.pool_w, c.labels, denom, lib.ce_params('ce', label_smoothing=0.1), 1, 0,
                                          b['logits'], b['loss'], b['ws'], b['aws'])
            lib.grad_reduce(c.shape, B, b['ws'], b['grad'])
            out = dict(logits=b['logits'], grad=b['grad'])
            if route != 'dlogits':
                out['loss'] = b['loss']
        torch.cuda.synchronize()
        out = {k: v.cpu().clone() for k, v in out.items()}
        if route != 'forward':
            out.update(c.heads(b['ws'], B))
        runs.append(out)
        tag = '%s, %s' % (what, fill_name(i, fill))
        pool.check(tag)
        c.inputs.check(tag)
    same_bits(runs, what, FILL_LABELS)


# ------------------------------------------------------------------------------- a9. the other launches with a workspace
@pytest.mark.parametrize('C', mc.BAND_C)
def test_band_moments_read_nothing_stale(C):
    """dmf_band_moments and dmf_band_noise_moments (both directions) on a 13 x 11 scene."""
    from dmf import lib
    H, W = mc.BAND_SCENE
    g = torch.Generator().manual_seed(C)
    ins = Pool()
    x = ins.put('scene', torch.rand(H, W, C, generator=g).to(DEV))
    runs = []
    for i, fill in enumerate(mc.FILLS):
        pool = Pool(fill)
        mean, cov = pool.new('mean', (C,), torch.float64), pool.new('cov', (C, C), torch.float64)
        ws = pool.new('moments workspace', (lib.band_moments_workspace_bytes(H * W, C) // 8,), torch.float64)
        lib.band_moments(x.view(H * W, C), mean, cov, ws)
        out = dict(mean=mean, cov=cov)
        for d in ('horizontal', 'vertical'):
            ncov = pool.new('ncov ' + d, (C, C), torch.float64)
            nws = pool.new('noise workspace ' + d, (lib.band_noise_workspace_bytes(H, W, C) // 8,), torch.float64)
            lib.band_noise_moments(x, H, W, ncov, d, nws)
            out['ncov ' + d] = ncov
        torch.cuda.synchronize()
        runs.append({k: v.cpu().clone() for k, v in out.items()})
        tag = 'band moments [C = %d], %s' % (C, fill_name(i, fill))
        pool.check(tag)
        ins.check(tag)
    same_bits(runs, 'band moments [C = %d]' % C, FILL_LABELS)


@pytest.mark.parametrize('N', mc.TEMP_N)
def test_temperature_step_reads_nothing_stale(N):
    from dmf import lib
    K = mc.TEMP_K
    g = torch.Generator().manual_seed(N)
    ins = Pool()
    logits = ins.put('logits', (3 * torch.randn(N, K, generator=g)).to(DEV))
    labels = ins.put('labels', torch.randint(0, K, (N,), generator=g).int().to(DEV))
    runs = []
    for i, fill in enumerate(mc.FILLS):
        pool = Pool(fill)
        state = pool.new('temperature state', (lib.TEMP_DOUBLES,), torch.float64, 0x00)
        lib.temperature_init(state)
        ws = pool.new('temperature workspace', (max(lib.temperature_workspace_bytes(N), 24),), torch.uint8)
        for _ in range(2):
            lib.temperature_step(logits, labels, state, ws, update=True)
        torch.cuda.synchronize()
        runs.append(dict(state=state[:7].cpu().clone()))
        tag = 'temperature step [N = %d], %s' % (N, fill_name(i, fill))
        pool.check(tag)
        ins.check(tag)
    same_bits(runs, 'temperature step [N = %d]' % N, FILL_LABELS)


# ======================================================================================= b. one workspace, several batch sizes
@pytest.mark.parametrize('variant', ['reduce', 'dlogits', 'unit_ce'])
@pytest.mark.parametrize('name', ['tiny1', 'tiny', 'quatiny'])
def test_one_workspace_serves_smaller_batches(name, variant):
    """A guarded workspace sized for 513 patches runs 513, 3, 257 and 1 patches (rows and layout follow each batch): every
    result is bit-equal to the same launch in a fresh zero workspace — the stale content is the previous batch's data."""
    K = mc.SHAPES[name][4]
    big = mc.SHARED_WS_BATCHES[0]
    c = case(name, big, K)
    shared = Pool(0x47)
    ws = shared.new('shared workspace', (ws_floats(c, big),))
    for B in mc.SHARED_WS_BATCHES:
        what = what_of(variant + ' in the shared workspace', name, B, K)
        pool = Pool(0xFF)
        got = train_launch(c, B, train_buffers(c, B, pool, variant, ws=ws[:ws_floats(c, B)]), variant)
        fresh = Pool(0x00)
        want = train_launch(c, B, train_buffers(c, B, fresh, variant), variant)
        same_bits([want, got], what, ['a fresh zero workspace', 'the shared workspace'])
        for p in (pool, fresh, shared, c.inputs):
            p.check(what)


# ============================================================================================================ c. beside the scene
@pytest.mark.parametrize('name,extra,half', [(n, e, False) for n in ('tiny', 'panms') for e in (0,) + mc.PITCH_EXTRA] +
                         [('tiny1', 0, False), ('tiny1', 0, True), ('hsi', 0, True), ('qua', 0, False)],
                         ids=lambda x: str(x))
def test_nothing_beside_the_scene_is_read(name, extra, half):
    """Gather mode with sceneA, sceneB, xy and labels in guarded allocations whose guards hold 0xA5, 0xFF and 0x00; the batch has the
    four corner windows and one window on each edge of the padded scene (legal by lib.check_xy_bounds).  Forward and train outputs
    are bit-equal whatever the guards hold.  (tiny, panms: aux at 4x, aux pitch = 1, 2, 3 mod 4 with `extra`.)"""
    from dmf import lib
    K = mc.SHAPES[name][4]
    B = 9
    runs, labels = [], []
    for canary in (0xA5, 0xFF, 0x00):
        c = Case(name, B, K, half=half, extra=extra, canary=canary)
        if mc.SHAPES[name][3] == 4:
            assert (c.Bm.shape[1] * c.Bm.shape[2]) % 4 == extra
        pool = Pool(0x00, canary)
        logits, pred = pool.new('logits', (B, K)), pool.new('pred', (B,), torch.int32)
        lib.forward(c.shape, c.gather(), c.theta, c.pool_w, logits, pred)
        out = train_launch(c, B, train_buffers(c, B, pool, 'reduce'), 'reduce')
        torch.cuda.synchronize()
        out.update(forward_logits=logits.cpu().clone(), pred=pred.cpu().clone())
        runs.append(out)
        labels.append('guards 0x%02X' % canary)
        what = 'beside the scene [%s, extra %d, half %s], guards 0x%02X' % (name, extra, half, canary)
        pool.check(what)
        c.inputs.check(what)
    same_bits(runs, 'beside the scene [%s, extra %d, half %s]' % (name, extra, half), labels)


# ================================================================================================================ d. tails
def optim_inputs(n, nonfinite, kind='ADAM'):
    g = torch.Generator().manual_seed(n)
    theta, grad = torch.randn(n, generator=g), torch.randn(n, generator=g)
    m, v = 0.1 * torch.randn(n, generator=g), 0.01 * torch.rand(n, generator=g)
    if kind == 'RMSprop':
        m = m.abs()                                 # its one state vector is the running mean of squares
    if nonfinite:
        grad[n - 1] = float('inf')
    return theta, grad, m, v


@pytest.mark.parametrize('kind', ['ADAM', 'ADAMW', 'SGD', 'RMSprop'])
@pytest.mark.parametrize('n', mc.TAIL_N)
def test_optimiser_launches_stay_inside_n(kind, n):
    """dmf_optim_step, _sched and _avg: with and without clipping, with and without a scaler state (ADAM, ADAMW), one non-finite
    gradient element at n - 1 included; theta, m, v, avg and grad guarded, the results bit-equal across two runs."""
    from dmf import lib
    table = torch.tensor([[1e-3, 0.9, 0.999, 0.9], [5e-4, 0.8, 0.99, 0.5]], device=DEV)
    scalers = (False, True) if kind in ('ADAM', 'ADAMW') else (False,)
    for entry in ('plain', 'sched', 'avg'):
        for max_norm in (None, 0.5):
            for scaler in scalers:
                for nonfinite in ((False, True) if scaler else (False,)):
                    what = 'optim_step %s [%s, n = %d, max_norm %s, scaler %s, non-finite %s]' % (entry, kind, n, max_norm, scaler, nonfinite)
                    runs = []
                    for rep in range(2):
                        pool = Pool(0xFF)
                        th, gr, m, v = (pool.put(k, t.to(DEV)) for k, t in zip(('theta', 'grad', 'm', 'v'), optim_inputs(n, nonfinite, kind)))
                        step = pool.put('step', torch.full((1,), 2, dtype=torch.int32, device=DEV))
                        cursor = pool.put('cursor', torch.ones(1, dtype=torch.int32, device=DEV))
                        norm_hist = pool.put('norm_hist', torch.zeros(3, device=DEV))
                        keys = dict(eps=1e-8, alpha=0.99, weight_decay=0.01, max_norm=max_norm, step=3, grad_scale=0.5, step_dev=step,
                                    cursor_dev=cursor, norm_hist=norm_hist)
                        out = dict(theta=th, grad=gr, m=m, v=v, step=step, cursor=cursor, norm_hist=norm_hist)
                        if scaler:
                            st = torch.zeros(lib.SCALER_FLOATS, device=DEV)
                            lib.scaler_init(st, 8.0)
                            keys.update(scaler_state=pool.put('scaler state', st), scaler_hparams=SCALER_HP)
                            out['scaler state'] = keys['scaler_state']
                        if entry == 'plain':
                            lib.optim_step(kind, th, gr, m, v, 1e-3, 0.9, 0.999, momentum=0.9, **keys)
                        elif entry == 'sched':
                            lib.optim_step_sched(kind, th, gr, m, v, lib.hp_schedule(table), **keys)
                        else:
                            avg = pool.put('avg', th.clone())
                            lib.optim_step_avg(kind, th, gr, m, v, lib.weight_avg(avg, 'ema', 0.9, 1), lr=1e-3, momentum=0.9, **keys)
                            out['avg'] = avg
                        torch.cuda.synchronize()
                        runs.append({k: t.cpu().clone() for k, t in out.items() if k != 'grad'})
                        pool.check(what)
                        if nonfinite:
                            want = optim_inputs(n, nonfinite, kind)
                            assert torch.equal(runs[-1]['theta'], want[0]) and torch.equal(runs[-1]['m'], want[2]), what + ': a skipped step'
                        else:
                            assert not torch.equal(runs[-1]['theta'], optim_inputs(n, False)[0]), what + ': theta did not move'
                    same_bits(runs, what)


@pytest.mark.parametrize('n', mc.TAIL_N)
def test_weight_average_and_epoch_ledger_stay_inside_n(n):
    """dmf_weight_average (both kinds), dmf_valid_accum and dmf_keep_best with guarded avg, acc, best_theta and history."""
    from dmf import lib
    g = torch.Generator().manual_seed(n)
    for kind in ('ema', 'mean'):
        pool = Pool(0xFF)
        theta = pool.put('theta', torch.randn(n, generator=g).to(DEV))
        avg = pool.put('avg', torch.randn(n, generator=g).to(DEV))
        before = avg.clone()
        lib.weight_average(lib.weight_avg(avg, kind, 0.9, 1), theta, step=3)
        pool.check('weight_average %s [n = %d]' % (kind, n))
        assert not torch.equal(avg, before) and not torch.isnan(avg).any()
    pool = Pool(0xFF)
    loss = pool.put('loss', torch.rand(n, generator=g).to(DEV))
    acc = pool.put('acc', torch.zeros(1, dtype=torch.float64, device=DEV))
    lib.valid_accum(loss, n, acc)
    want = float(acc.item())
    assert abs(want - float(loss.double().sum().item())) <= n * 2.0 ** -52 * want + 1e-300
    best = pool.put('best', torch.full((1,), float('inf'), dtype=torch.float64, device=DEV))
    best_epoch = pool.put('best_epoch', torch.full((1,), -1, dtype=torch.int32, device=DEV))
    theta = pool.put('theta', torch.randn(n, generator=g).to(DEV))
    best_theta = pool.new('best_theta', (n,))
    hist = pool.put('val_hist', torch.full((3,), -1.0, dtype=torch.float64, device=DEV))
    lib.keep_best(acc, best, best_epoch, 2, theta, best_theta, hist)
    pool.check('valid_accum / keep_best [n = %d]' % n)
    assert torch.equal(best_theta, theta) and int(best_epoch.item()) == 2 and float(best.item()) == want and float(acc.item()) == 0.0
    assert hist.tolist() == [-1.0, -1.0, want]


@pytest.mark.parametrize('K', mc.LOSS_K)
@pytest.mark.parametrize('bs', mc.LOSS_BS)
def test_loss_launches_stay_inside_their_rows(bs, K):
    """dmf_ce_loss (plain, smoothed, focal) and dmf_qua_loss with guarded dlogits / loss, across the fills."""
    from dmf import lib
    g = torch.Generator().manual_seed(100 * bs + K)
    ins = Pool()
    logits = ins.put('logits', (2 * torch.randn(4 * bs, K, generator=g)).to(DEV))
    labels = ins.put('labels', torch.randint(0, K, (bs,), generator=g).int().to(DEV))
    class_w = ins.put('class_w', (0.5 + torch.rand(K, generator=g)).to(DEV))
    qp = lib.QuaParams(alpha=0.1, beta=0.05, gamma=1.0, epsilon=1e-8, tao=0.1)
    runs = []
    what = 'loss launches [bs = %d, K = %d]' % (bs, K)
    for i, fill in enumerate(mc.FILLS):
        pool = Pool(fill)
        out = {}
        for tag, params, w in (('ce', lib.ce_params('ce'), None), ('smooth', lib.ce_params('ce', label_smoothing=0.1), class_w),
                               ('focal', lib.ce_params('focal', gamma=2.0), class_w)):
            loss, dl = pool.new(tag + ' loss', (bs,)), pool.new(tag + ' dlogits', (bs, K))
            lib.ce_loss(logits[:bs], 1, 0, labels, params, class_w=w, loss=loss, dlogits=dl)
            out[tag + ' loss'], out[tag + ' dlogits'] = loss, dl
        qloss, qhist, qdl = pool.new('qua loss', (1,)), pool.new('qua loss_hist', (2,)), pool.new('qua dlogits', (4 * bs, K))
        cursor = pool.put('cursor', torch.ones(1, dtype=torch.int32, device=DEV))
        lib.qua_loss(logits, bs, torch.cat([labels, labels]), qp, loss=qloss, dlogits=qdl, cursor=cursor, loss_hist=qhist)
        out.update({'qua loss': qloss, 'qua loss_hist[cursor]': qhist[1:], 'qua dlogits': qdl})
        torch.cuda.synchronize()
        runs.append({k: v.cpu().clone() for k, v in out.items()})
        pool.check('%s, %s' % (what, fill_name(i, fill)))
        ins.check('%s, %s' % (what, fill_name(i, fill)))
    same_bits(runs, what, FILL_LABELS)


@pytest.mark.parametrize('K', mc.ROW_K)
@pytest.mark.parametrize('B', mc.ROW_B)
def test_row_launches_stay_inside_their_rows(B, K):
    """dmf_softmax_stats (row-indexed and scattered), dmf_prob_scatter, dmf_logits_mean, dmf_calib_accum, dmf_confusion_accum
    and dmf_labelmap_write with guarded outputs, across the fills (accumulated outputs start from zero: the caller's part)."""
    from dmf import lib
    g = torch.Generator().manual_seed(100 * B + K)
    H, W = 17, 16                                   # 272 pixels >= 257 rows; the last row of the batch is the last pixel
    ins = Pool()
    logits_v = ins.put('logits_v', (2 * torch.randn(3, B, K, generator=g)).to(DEV))
    logits = logits_v[0]
    target = ins.put('target', torch.randint(0, K, (B,), generator=g).int().to(DEV))
    pix = torch.randperm(H * W - 1, generator=g)[:B]          # distinct pixels
    pix[B - 1] = H * W - 1
    xy = ins.put('xy', torch.stack([pix // W, pix % W], 1).int().to(DEV))
    beta = ins.put('inv_temp', torch.tensor([0.7]).to(DEV))
    runs = []
    what = 'row launches [B = %d, K = %d]' % (B, K)
    for i, fill in enumerate(mc.FILLS):
        pool = Pool(fill)
        pred, conf, margin, ent = (pool.new(k, (B,), dt) for k, dt in (('pred', torch.int32), ('conf', torch.float32),
                                                                       ('margin', torch.float32), ('entropy', torch.float32)))
        lib.softmax_stats(logits, pred, conf, margin, ent, inv_temp=beta)
        maps = [pool.new('map ' + k, (H, W), dt, 0x00) for k, dt in (('pred', torch.int32), ('conf', torch.float32),
                                                                     ('margin', torch.float32), ('entropy', torch.float32))]
        lib.softmax_stats(logits, *maps, inv_temp=beta, xy=xy, W=W)
        prob, mask = pool.new('prob', (H, W, K), torch.float32, 0x00), pool.new('mask', (H, W), torch.uint8, 0x00)
        lib.prob_scatter(logits, xy, W, prob, mask, inv_temp=beta)
        mean, mpred = pool.new('mean logits', (B, K)), pool.new('mean pred', (B,), torch.int32)
        lib.logits_mean(logits_v, mean, mpred)
        hist = pool.new('calibration histogram', (10, 3), torch.int64, 0x00)
        lib.calib_accum(conf, pred, target, K, hist)
        matrix = pool.new('confusion matrix', (K, K), torch.int64, 0x00)
        lib.confusion_accum(pred, target, K, matrix)
        lmap = pool.new('label map', (H, W), torch.int32, 0x00)
        lib.labelmap_write(pred, xy, W, lmap)
        torch.cuda.synchronize()
        out = dict(pred=pred, conf=conf, margin=margin, entropy=ent, prob=prob, mask=mask, mean=mean, mean_pred=mpred, hist=hist,
                   matrix=matrix, label_map=lmap, **{'map %d' % j: t for j, t in enumerate(maps)})
        runs.append({k: v.cpu().clone() for k, v in out.items()})
        pool.check('%s, %s' % (what, fill_name(i, fill)))
        ins.check('%s, %s' % (what, fill_name(i, fill)))
        r = runs[-1]
        assert int(r['matrix'].sum()) == B and int(r['hist'][:, 0].sum()) == B and int(r['mask'].sum()) == B
        assert torch.equal(r['label_map'].reshape(-1)[pix], r['pred']) and torch.equal(r['map 0'].reshape(-1)[pix], r['pred'])
    same_bits(runs, what, FILL_LABELS)


@pytest.mark.parametrize('dtype', ['uint8', 'uint16', 'int16', 'int32', 'float32', 'float64'])
@pytest.mark.parametrize('half', [False, True], ids=['fp32', 'fp16'])
def test_scene_prepare_stays_inside_out(dtype, half):
    from dmf import lib
    H, W, C, pad = 13, 11, 3, 4
    rng = np.random.default_rng(7)
    raw = (rng.random((H, W, C)) * 200).astype(dtype)
    ins = Pool()
    raw_d = ins.put('raw', torch.from_numpy(raw.view(np.uint8).reshape(-1)).to(DEV))
    runs = []
    for i, fill in enumerate(mc.FILLS):
        pool = Pool(fill)
        minmax = pool.new('minmax', (16,), torch.uint8)
        out = pool.new('out', (H + pad, W + pad, C), torch.float16 if half else torch.float32)
        lib.scene_minmax(raw_d, dtype, minmax)
        lib.scene_prepare(raw_d, dtype, H, W, C, minmax, pad, out)
        torch.cuda.synchronize()
        runs.append(dict(out=out.cpu().clone(), minmax=minmax[:2 * raw.dtype.itemsize].cpu().clone()))
        pool.check('scene_prepare [%s], %s' % (dtype, fill_name(i, fill)))
        ins.check('scene_prepare [%s], %s' % (dtype, fill_name(i, fill)))
    same_bits(runs, 'scene_prepare [%s, half %s]' % (dtype, half), FILL_LABELS)


@pytest.mark.parametrize('C', mc.PROJECT_C)
@pytest.mark.parametrize('K', mc.PROJECT_K)
def test_band_project_stays_inside_out(C, K):
    from dmf import lib
    if K > C:
        K = C                                       # K <= min(C, 64): the 3-band scene projects on all 3
    N = 13 * 11
    g = torch.Generator().manual_seed(C + K)
    ins = Pool()
    x = ins.put('x', torch.rand(N, C, generator=g).to(DEV))
    mean = ins.put('mean', torch.rand(C, generator=g).double().to(DEV))
    basis = ins.put('basis', torch.randn(C, K, generator=g).to(DEV))
    runs = []
    for i, fill in enumerate(mc.FILLS):
        pool = Pool(fill)
        y = pool.new('y', (N, K))
        lib.band_project(x, mean, basis, y)
        torch.cuda.synchronize()
        runs.append(dict(y=y.cpu().clone()))
        pool.check('band_project [C = %d, K = %d], %s' % (C, K, fill_name(i, fill)))
        ins.check('band_project [C = %d, K = %d], %s' % (C, K, fill_name(i, fill)))
    same_bits(runs, 'band_project [C = %d, K = %d]' % (C, K), FILL_LABELS)


# ========================================================================================================= e. the engines
ENGINE_FORMS = {
    'fused_eager': dict(),
    'fused_graphs': dict(steps_per_graph=3),
    'native_loop': dict(steps_per_graph=-1),
    'criterion_unit': dict(engine=dict(criterion={'label_smoothing': 0.1})),
    'adamw_clip_scaler': dict(engine=dict(optimizer='ADAMW', weight_decay=0.01, clip_grad_norm=0.5), scaler=True),
    'attention': dict(attention=True),
}


def fill_bytes(t, fill):
    if t is not None:
        t.view(-1).view(torch.uint8).fill_(fill)


def engine_block(K, bs, seed):
    """2 epochs of 3 full steps of `bs` pixels plus a short batch of 5, on a 23 x 19 scene."""
    g = torch.Generator().manual_seed(seed)
    n = 2 * 3 * bs
    xy = torch.stack([torch.randint(0, mc.SCENE_H, (n,), generator=g), torch.randint(0, mc.SCENE_W, (n,), generator=g)], 1).int()
    xy[0] = torch.tensor([mc.SCENE_H - 1, mc.SCENE_W - 1])
    lab = torch.randint(0, K, (n,), generator=g).int()
    sxy = torch.stack([torch.randint(0, mc.SCENE_H, (2, 5), generator=g), torch.randint(0, mc.SCENE_W, (2, 5), generator=g)], 2).int()
    slab = torch.randint(0, K, (2, 5), generator=g).int()
    return xy, lab, sxy, slab


def run_block(eng, steps_per_graph):
    for e in range(2):
        eng.run_plan(3, steps_per_graph)
        eng.step_short(e)
    torch.cuda.synchronize()
    out = dict(theta=eng.theta, m=eng.m, v=eng.v)
    if eng.scaler is not None:
        out['scaler state'] = eng.scaler.state
    losses, short = eng.block_losses()
    norms, short_norms = eng.block_grad_norms()
    out.update(losses=losses, short_losses=short, norms=norms, short_norms=short_norms)
    return {k: v.detach().cpu().clone() for k, v in out.items()}


@pytest.mark.parametrize('form', list(ENGINE_FORMS))
def test_train_engine_does_not_depend_on_what_its_buffers_held(form):
    """TrainEngine on tiny1, batch 16: a block of 2 epochs of 3 full steps plus a short batch of 5 (load_block, run_plan,
    step_short) with eng.ws, attn_ws, logits, dlogits and grad byte-filled after construction (eng.loss stays as the engine
    made it: created zeroed on purpose)."""
    from dmf.engine import LossScaler, Scene, TrainEngine
    spec = ENGINE_FORMS[form]
    name, bs = 'tiny1', 16
    K = mc.SHAPES[name][4]
    A, Bm, _, _, _ = mc.scene_batch(name, 1, K)
    xy, lab, sxy, slab = engine_block(K, bs, 5)
    runs = []
    for fill in mc.FILLS:
        net = mc.nets(name, K, spec.get('attention', False))
        scaler = LossScaler(DEV, init_scale=1024.0) if spec.get('scaler') else None
        eng = TrainEngine(net, Scene(A.numpy(), Bm.numpy(), DEV), bs, lr=1e-3, scaler=scaler, **spec.get('engine', {}))
        for t in (eng.ws, eng.attn_ws, eng.logits, getattr(eng, 'dlogits', None), eng.grad):
            fill_bytes(t, fill)
        eng.load_block(xy.numpy(), lab.numpy(), sxy.numpy(), slab.numpy())
        runs.append(run_block(eng, spec.get('steps_per_graph', 0)))
    same_bits(runs, 'TrainEngine ' + form, FILL_LABELS)
    assert not torch.equal(runs[0]['theta'], mc.nets(name, K, spec.get('attention', False)).flat_parameters().cpu())


def test_qua_train_engine_does_not_depend_on_what_its_buffers_held():
    """QuaTrainEngine on quatiny, bs 16: 3 plan steps and an eager step of 5 samples, its buffers byte-filled."""
    from dmf.engine import QuaScene, QuaTrainEngine
    name, bs = 'quatiny', 16
    C, C2, P, S, K, _ = mc.SHAPES[name]
    g = torch.Generator().manual_seed(9)
    scenes = [torch.rand(mc.SCENE_H + P - 1, mc.SCENE_W + P - 1, C, generator=g).numpy() for _ in range(4)]
    xy, lab, sxy, slab = engine_block(K, bs, 6)
    dqtl = dict(alpha=0.1, beta=0.05, gamma=1.0, epsilon=1e-8, tao=0.1)
    runs = []
    for fill in mc.FILLS:
        cfg = mc.make_cfg(name, K)
        cfg['gmf']['single_input'] = 1
        from model.gmfnet import Net
        torch.manual_seed(0)
        net = Net(cfg)
        with torch.no_grad():
            for p in net.parameters():
                p.add_(0.05 * torch.randn_like(p))
        net = net.to(DEV)
        eng = QuaTrainEngine(net, QuaScene(scenes, DEV), bs, dqtl, lr=1e-3)
        for t in (eng.ws, eng.logits, eng.dlogits, eng.grad):
            fill_bytes(t, fill)
        eng.load_plan(xy[:3 * bs], lab[:3 * bs])
        eng.run_plan(3, 0)
        eng.step(sxy[0], slab[0])
        torch.cuda.synchronize()
        runs.append({k: v.detach().cpu().clone() for k, v in dict(theta=eng.theta, m=eng.m, v=eng.v, losses=eng.losses(),
                                                                  loss=eng.loss).items()})
    same_bits(runs, 'QuaTrainEngine', FILL_LABELS)


@pytest.mark.parametrize('attention', [False, True], ids=['late_fusion', 'attention'])
def test_eval_engine_does_not_depend_on_what_its_buffers_held(attention):
    """EvalEngine of batch 64 over 150 pixels (its last chunk is short): confusion, label_map and predict across the fills."""
    from dmf.engine import EvalEngine, Scene
    name = 'tiny1'
    K = mc.SHAPES[name][4]
    A, Bm, _, _, _ = mc.scene_batch(name, 1, K)
    g = torch.Generator().manual_seed(3)
    pix = torch.randperm(mc.SCENE_H * mc.SCENE_W, generator=g)[:150]
    xy = torch.stack([pix // mc.SCENE_W, pix % mc.SCENE_W], 1).int()
    lab = torch.randint(0, K, (150,), generator=g).int()
    net = mc.nets(name, K, attention)
    runs = []
    for fill in mc.FILLS:
        ev = EvalEngine(net, Scene(A.numpy(), Bm.numpy(), DEV), 64)
        for t in (ev.logits, ev.pred, ev.attn_ws):
            fill_bytes(t, fill)
        conf = ev.confusion(xy.numpy(), lab.numpy())
        lmap = ev.label_map(xy.numpy(), mc.SCENE_H, mc.SCENE_W)
        logits, pred = ev.predict(xy[128:].to(DEV))
        torch.cuda.synchronize()
        runs.append({k: torch.as_tensor(v).cpu().clone() for k, v in dict(confusion=conf, label_map=lmap, logits=logits, pred=pred).items()})
        assert int(runs[-1]['confusion'].sum()) == 150
    same_bits(runs, 'EvalEngine', FILL_LABELS)
