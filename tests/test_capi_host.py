"""CPU: what the C entry points decide on the host before any launch — the attention workspace sizes, the refusals with
their messages, and the empty-batch early exits.  Every call here returns before it touches the device: the pointers are
either NULL or point into a small host buffer that is never read."""
import ctypes as C

import pytest

from dmf import lib

L = lib._lib
_BUF = C.create_string_buffer(256)
P = C.c_void_p(C.addressof(_BUF))          # a non-null pointer that no row dereferences
NULL = None

ATTN_SHAPES = {'big': (200, 1, 11, 1, 40, 10), 'tiny': (8, 1, 5, 1, 40, 2)}      # C / C2 / P / S / F / G


def shape(geom=ATTN_SHAPES['big'], attention=0):
    Cc, C2, Pp, S, F, G = geom
    return lib.Shape(C=Cc, C2=C2, P=Pp, S=S, F=F, G=G, H=64, K=17, attention=attention, heads=3 if attention else 0,
                     E=96 if attention else 0, reserved=0)


def inp(B=1, mode=1, **kw):
    f = dict(mode=mode, B=B, a=P.value, b=P.value, sceneA=P.value, sceneB=P.value, xy=P.value, Wp=64, WpB=64, cursor=None,
             half=0, reserved=0)
    f.update(kw)
    return lib.Input(**f)


LATE, ATTN = shape(), shape(attention=1)

# ---------------------------------------------------------------------------------------------- attention workspace sizes
TOKENS = 2 * 128 * 64 * 2                  # two bf16 token maps of 128 tokens x 64 channels per patch
PREP_BYTES = 80640                         # bytes(0): the bf16 weight copies of every head; printed at the parent commit


def per_patch(geom, train):
    Pp, F = geom[2], geom[4]
    RS = (Pp + 3) & ~3
    return TOKENS + 2 * F * 4 + (2 * F * Pp * RS * 4 if train else 0)


def test_per_patch_bytes_are_the_documented_ones():
    assert per_patch(ATTN_SHAPES['big'], False) == per_patch(ATTN_SHAPES['tiny'], False) == 33088
    assert per_patch(ATTN_SHAPES['big'], True) == 75328
    assert per_patch(ATTN_SHAPES['tiny'], True) == 45888


@pytest.mark.parametrize('train', (False, True), ids=('forward', 'train'))
@pytest.mark.parametrize('name', sorted(ATTN_SHAPES))
def test_attention_workspace_bytes(name, train):
    s = shape(ATTN_SHAPES[name], attention=1)
    fn = L.dmf_attn_train_workspace_bytes if train else L.dmf_attn_workspace_bytes
    zero = fn(C.byref(s), 0)
    print('%s %s: bytes(0) = %d' % (name, 'train' if train else 'forward', zero))
    assert zero == PREP_BYTES
    for B in (0, 1, 3, 256, 257):
        assert fn(C.byref(s), B) - zero == B * per_patch(ATTN_SHAPES[name], train), B
    assert fn(C.byref(s), -1) == -1
    assert fn(None, 1) == -1


# ------------------------------------------------------------------------------------------------------------- refusals
def fwd(s, i, theta=P, pool=P, logits=P, pred=NULL):
    return L.dmf_forward(C.byref(s), C.byref(i), theta, pool, logits, pred, NULL)


def fwd_unit(s, i, ws=P):
    return L.dmf_forward_unit(C.byref(s), C.byref(i), P, P, P, ws, NULL, NULL)


def fwd_attn(s, i, ws=P):
    return L.dmf_forward_attn(C.byref(s), C.byref(i), P, P, ws, P, NULL, NULL)


def train_attn(s, i, labels=P, dlogits=NULL):
    return L.dmf_train_attn_fwd_bwd(C.byref(s), C.byref(i), P, P, labels, dlogits, 1.0, P, P, P, P, NULL, NULL)


BAD_INPUTS = [
    ('mode0_null_a', lambda: inp(mode=0, a=None), 'mode 0 needs a and b'),
    ('mode1_Wp0', lambda: inp(mode=1, Wp=0), 'mode 1 needs sceneA, sceneB, xy, Wp, WpB'),
    ('mode2', lambda: inp(mode=2), 'input mode must be 0 or 1'),
]

REFUSALS = [
    ('forward_null_theta', lambda: fwd(LATE, inp(), theta=NULL), 'null argument'),
    ('forward_unit_null_workspace', lambda: fwd_unit(LATE, inp(), ws=NULL), 'null argument'),
    ('forward_attn_null_workspace', lambda: fwd_attn(ATTN, inp(), ws=NULL), 'null argument'),
    ('forward_null_logits', lambda: fwd(LATE, inp(), logits=NULL), 'null logits'),
    ('forward_negative_batch', lambda: fwd(LATE, inp(B=-1)), 'negative batch'),
] + [('forward_' + n, (lambda mk=mk: fwd(LATE, mk())), msg) for n, mk, msg in BAD_INPUTS] + [
    ('forward_unit_' + n, (lambda mk=mk: fwd_unit(LATE, mk())), msg) for n, mk, msg in BAD_INPUTS] + [
    ('forward_on_attention_shape', lambda: fwd(ATTN, inp()), 'attention network: use dmf_forward_attn'),
    ('forward_attn_on_late_fusion', lambda: fwd_attn(LATE, inp()), 'dmf_forward_attn needs shape->attention == 1'),
    ('train_attn_no_labels_no_dlogits', lambda: train_attn(ATTN, inp(), labels=NULL, dlogits=NULL),
     'give exactly one of labels / dlogits'),
    ('grad_reduce_empty_batch', lambda: L.dmf_grad_reduce(C.byref(LATE), 0, P, P, NULL), 'batch must be positive'),
    ('grad_reduce_adam_null_m', lambda: L.dmf_grad_reduce_adam(C.byref(LATE), 1, P, P, NULL, P, NULL, 1e-3, 0.9, 0.999, 1e-8, 1,
                                                               NULL, NULL, NULL, NULL, NULL), 'Adam needs m, v and step >= 1'),
    # (this entry point has no host step count: the missing device one is named ahead of Adam's own refusal)
    ('grad_reduce_xgmi_adam_null_step', lambda: L.dmf_grad_reduce_xgmi_adam(
        C.byref(LATE), 1, P, P, P, P, C.byref(lib.XgmiComm(world=2, rank=0, capacity=1 << 20)), 1e-3, 0.9, 0.999, 1e-8, 1.0,
        NULL, NULL, NULL, NULL, NULL), 'the xgmi exchange needs adam_step_dev'),
]


@pytest.mark.parametrize('name,call,message', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusal(name, call, message):
    assert call() == 1
    assert L.dmf_last_error().decode() == message


# ------------------------------------------------------------------------------------------------------- empty batches
EMPTY = [
    ('forward', lambda: fwd(LATE, inp(B=0))),
    ('forward_ce', lambda: L.dmf_forward_ce(C.byref(LATE), C.byref(inp(B=0)), P, P, P, P, P, NULL, NULL)),
    ('train_fwd_bwd', lambda: L.dmf_train_fwd_bwd(C.byref(LATE), C.byref(inp(B=0)), P, P, P, 1.0, P, P, P, NULL, NULL)),
    ('train_fwd_bwd_scaled', lambda: L.dmf_train_fwd_bwd_scaled(C.byref(LATE), C.byref(inp(B=0)), P, P, P, 1.0, P, P, P, P,
                                                                 NULL, NULL)),
    ('forward_attn', lambda: fwd_attn(ATTN, inp(B=0))),
    ('train_attn_fwd_bwd', lambda: train_attn(ATTN, inp(B=0))),
    ('backward_dlogits', lambda: L.dmf_backward_dlogits(C.byref(LATE), C.byref(inp(B=0)), P, P, P, P, NULL)),
    ('forward_unit', lambda: fwd_unit(LATE, inp(B=0))),
    ('backward_unit', lambda: L.dmf_backward_unit(C.byref(LATE), 0, P, P, P, NULL)),
    ('pair_argmax', lambda: L.dmf_pair_argmax(P, 0, 17, P, NULL)),
    ('confusion_accum', lambda: L.dmf_confusion_accum(P, P, 0, 17, P, NULL)),
    ('labelmap_write', lambda: L.dmf_labelmap_write(P, P, 0, 64, P, NULL)),
]


@pytest.mark.parametrize('name,call', EMPTY, ids=[r[0] for r in EMPTY])
def test_empty_batch_is_a_no_op(name, call):
    assert call() == 0
