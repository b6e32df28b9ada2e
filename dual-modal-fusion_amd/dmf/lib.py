"""ctypes binding of libdmf_hip.so (include/dmf.h).  PyTorch is used only for device memory and streams.

The library is mandatory: importing this module without the built .so raises (there is NO CPU fallback —
the CPU statement of the arithmetic lives under oracle/ and is test infrastructure only).
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('DMF_LIB', os.path.join(_HERE, 'libdmf_hip.so'))   # DMF_LIB: diagnostic builds only
KMAX = 64


class DmfError(RuntimeError):
    pass


class Shape(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ('C', 'C2', 'P', 'S', 'F', 'G', 'H', 'K', 'attention', 'heads', 'E', 'reserved')]


class XgmiComm(C.Structure):
    _fields_ = [('world', C.c_int32), ('rank', C.c_int32), ('capacity', C.c_int64), ('timeout_ms', C.c_int32),
                ('seq_bias', C.c_int32), ('data', C.c_void_p * 16), ('flags', C.c_void_p * 16)]


class QuaParams(C.Structure):
    _fields_ = [(n, C.c_float) for n in ('alpha', 'beta', 'gamma', 'epsilon', 'tao')]


class CeParams(C.Structure):
    _fields_ = [('kind', C.c_int32), ('label_smoothing', C.c_float), ('gamma', C.c_float)]


class CeFused(C.Structure):
    """dmf_ce_fused: the criterion of dmf_train_attn_fwd_bwd_ce — labels_global / denom on the device, one row per plan step."""
    _fields_ = [('params', C.POINTER(CeParams)), ('class_w', C.c_void_p), ('labels_global', C.c_void_p), ('denom', C.c_void_p),
                ('ranks', C.c_int32), ('rank', C.c_int32), ('grad_scale', C.c_float), ('reserved', C.c_int32)]


class HpSchedule(C.Structure):
    """dmf_hp_schedule: table [rows][4] fp32 on the device, row_dev a device int32 (unit `epoch`) or NULL (unit `step`)."""
    _fields_ = [('table', C.c_void_p), ('rows', C.c_int32), ('row_dev', C.c_void_p)]


class WeightAvg(C.Structure):
    """dmf_weight_avg: avg [n] fp32 on the device, kind DMF_AVG_*, weight = float32(1 - decay) (EMA), start = first averaged step."""
    _fields_ = [('avg', C.c_void_p), ('kind', C.c_int32), ('weight', C.c_float), ('start', C.c_int32), ('reserved', C.c_int32)]


class Input(C.Structure):
    _fields_ = [('mode', C.c_int32), ('B', C.c_int32), ('a', C.c_void_p), ('b', C.c_void_p), ('sceneA', C.c_void_p),
                ('sceneB', C.c_void_p), ('xy', C.c_void_p), ('Wp', C.c_int32), ('WpB', C.c_int32), ('cursor', C.c_void_p),
                ('half', C.c_int32), ('reserved', C.c_int32)]


def _load():
    if not os.path.exists(LIB_PATH):
        raise DmfError('libdmf_hip.so is not built: run `python dual-modal-fusion_amd/build.py` '
                       '(hipcc --offload-arch=gfx950); there is no CPU fallback for the product path')
    lib = C.CDLL(LIB_PATH)
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    SP, IP, HP, AP = C.POINTER(Shape), C.POINTER(Input), C.POINTER(HpSchedule), C.POINTER(WeightAvg)
    protos = {
        'dmf_version': (i32, []),
        'dmf_last_error': (C.c_char_p, []),
        'dmf_shape_supported': (i32, [SP]),
        'dmf_patch_variant': (i32, [SP, i32]),
        'dmf_param_layout': (i32, [SP, C.POINTER(i64)]),
        'dmf_workspace_bytes': (i64, [SP, i32]),
        'dmf_forward': (i32, [SP, IP, vp, vp, vp, vp, vp]),
        'dmf_attn_workspace_bytes': (i64, [SP, i32]),
        'dmf_forward_attn': (i32, [SP, IP, vp, vp, vp, vp, vp, vp]),
        'dmf_train_fwd_bwd': (i32, [SP, IP, vp, vp, vp, f32, vp, vp, vp, vp, vp]),
        'dmf_train_fwd_bwd_scaled': (i32, [SP, IP, vp, vp, vp, f32, vp, vp, vp, vp, vp, vp]),
        'dmf_half_supported': (i32, [SP]),
        'dmf_scaler_init': (i32, [vp, f32, vp]),
        'dmf_unscale_adam': (i32, [vp, vp, vp, vp, i64, f32, f32, f32, f32, f32, vp, f32, f32, i32, i32, vp, vp, vp]),
        'dmf_grad_reduce_scaled': (i32, [SP, i32, vp, vp, vp, vp, vp, vp, vp]),
        'dmf_qua_loss_scaled': (i32, [vp, i32, i32, vp, vp, C.POINTER(QuaParams), f32, vp, vp, vp, vp, vp]),
        'dmf_qua_loss_ranks': (i32, [vp, i32, i32, i32, i32, vp, vp, C.POINTER(QuaParams), f32, vp, vp, vp, vp, vp]),
        'dmf_attn_train_workspace_bytes': (i64, [SP, i32]),
        'dmf_train_attn_fwd_bwd': (i32, [SP, IP, vp, vp, vp, vp, f32, vp, vp, vp, vp, vp, vp]),
        'dmf_backward_dlogits': (i32, [SP, IP, vp, vp, vp, vp, vp]),
        'dmf_unit_supported': (i32, [SP]),
        'dmf_forward_unit': (i32, [SP, IP, vp, vp, vp, vp, vp, vp]),
        'dmf_backward_unit': (i32, [SP, i32, vp, vp, vp, vp]),
        'dmf_grad_reduce': (i32, [SP, i32, vp, vp, vp]),
        'dmf_adam_step': (i32, [vp, vp, vp, vp, i64, f32, f32, f32, f32, i32, f32, vp, vp, vp]),
        'dmf_sgd_step': (i32, [vp, vp, vp, i64, f32, f32, i32, f32, vp, vp, vp]),
        'dmf_rmsprop_step': (i32, [vp, vp, vp, i64, f32, f32, f32, f32, vp, vp]),
        'dmf_optim_step': (i32, [vp, vp, vp, vp, i64, i32, f32, f32, f32, f32, f32, f32, f32, f32, i32, f32, vp, vp, vp, f32, f32, i32,
                                 i32, vp, vp]),
        'dmf_grad_reduce_adam': (i32, [SP, i32, vp, vp, vp, vp, vp, f32, f32, f32, f32, i32, vp, vp, vp, vp, vp]),
        'dmf_forward_ce': (i32, [SP, IP, vp, vp, vp, vp, vp, vp, vp]),
        'dmf_train_plan_steps': (i32, [SP, IP, vp, vp, vp, f32, vp, vp, vp, vp, vp, f32, f32, f32, f32, vp, vp, vp, i32, vp]),
        'dmf_optim_step_sched': (i32, [vp, vp, vp, vp, i64, i32, HP, f32, f32, f32, f32, i32, f32, vp, vp, vp, f32, f32, i32, i32, vp, vp]),
        'dmf_grad_reduce_adam_sched': (i32, [SP, i32, vp, vp, vp, vp, vp, HP, f32, i32, vp, vp, vp, vp, vp]),
        'dmf_train_plan_steps_sched': (i32, [SP, IP, vp, vp, vp, f32, vp, vp, vp, vp, vp, HP, f32, vp, vp, vp, i32, vp]),
        'dmf_weight_average': (i32, [AP, vp, i64, i32, vp, vp]),
        'dmf_optim_step_avg': (i32, [vp, vp, vp, vp, i64, i32, f32, f32, f32, f32, f32, f32, f32, f32, i32, f32, vp, vp, vp, f32, f32,
                                     i32, i32, vp, HP, AP, vp]),
        'dmf_grad_reduce_adam_avg': (i32, [SP, i32, vp, vp, vp, vp, vp, f32, f32, f32, f32, i32, vp, vp, vp, vp, HP, AP, vp]),
        'dmf_train_plan_steps_avg': (i32, [SP, IP, vp, vp, vp, f32, vp, vp, vp, vp, vp, f32, f32, f32, f32, vp, vp, vp, HP, AP, i32,
                                           vp]),
        'dmf_xgmi_sizes': (i32, [i64, i32, C.POINTER(i64), C.POINTER(i64)]),
        'dmf_xgmi_alloc': (i32, [i64, C.POINTER(vp)]),
        'dmf_xgmi_free': (i32, [vp]),
        'dmf_xgmi_export': (i32, [vp, C.c_char_p]),
        'dmf_xgmi_open': (i32, [C.c_char_p, C.POINTER(vp)]),
        'dmf_xgmi_close': (i32, [vp]),
        'dmf_xgmi_status': (i32, [C.POINTER(XgmiComm), C.POINTER(i32)]),
        'dmf_xgmi_allreduce': (i32, [C.POINTER(XgmiComm), vp, i64, i32, vp]),
        'dmf_grad_reduce_xgmi_adam': (i32, [SP, i32, vp, vp, vp, vp, C.POINTER(XgmiComm), f32, f32, f32, f32, f32, vp, vp,
                                            vp, vp, vp]),
        'dmf_qua_loss': (i32, [vp, i32, i32, vp, vp, C.POINTER(QuaParams), f32, vp, vp, vp, vp]),
        'dmf_ce_loss': (i32, [vp, i32, i32, i32, i32, vp, vp, vp, C.POINTER(CeParams), f32, vp, vp, vp, vp]),
        'dmf_ce_denominators': (i32, [vp, i32, i32, i32, vp, vp, vp]),
        'dmf_train_attn_fwd_bwd_ce': (i32, [SP, IP, vp, vp, C.POINTER(CeFused), vp, vp, vp, vp, vp, vp]),
        'dmf_pair_argmax': (i32, [vp, i32, i32, vp, vp]),
        'dmf_band_mean': (i32, [vp, i32, i64, i64, i32, vp, vp]),
        'dmf_confusion_accum': (i32, [vp, vp, i32, i32, vp, vp]),
        'dmf_labelmap_write': (i32, [vp, vp, i32, i32, vp, vp]),
        'dmf_softmax_stats': (i32, [vp, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp]),
        'dmf_calib_accum': (i32, [vp, vp, vp, i32, i32, i32, vp, vp]),
        'dmf_temperature_init': (i32, [vp, vp]),
        'dmf_temperature_workspace_bytes': (i64, [i32]),
        'dmf_temperature_step': (i32, [vp, vp, i32, i32, vp, vp, i32, vp]),
        'dmf_valid_accum': (i32, [vp, i32, vp, vp]),
        'dmf_keep_best': (i32, [vp, vp, vp, i32, vp, vp, i64, vp, vp]),
        'dmf_pan2ms': (i32, [vp, i32, i32, i32, vp, vp]),
        'dmf_scene_minmax': (i32, [vp, i32, i64, vp, vp]),
        'dmf_scene_prepare': (i32, [vp, i32, i32, i32, i32, vp, i32, i32, vp, vp]),
        'dmf_scene_atlas': (i32, [vp, i32, i32, i32, i32, i32, C.POINTER(i32), i32, i32, i32, vp, vp]),
        'dmf_logits_mean': (i32, [vp, i32, i32, i32, vp, vp, vp]),
        'dmf_prob_scatter': (i32, [vp, i32, i32, vp, vp, i32, vp, vp, vp]),
        'dmf_spatial_affinity': (i32, [vp, i32, i32, i32, i32, i32, i32, f32, f32, vp, vp]),
        'dmf_spatial_filter': (i32, [vp, vp, vp, i32, i32, i32, i32, vp, vp, vp]),
        'dmf_band_moments_workspace_bytes': (i64, [i64, i32]),
        'dmf_band_moments': (i32, [vp, i64, i32, i64, vp, vp, vp, vp]),
        'dmf_band_project': (i32, [vp, i64, i32, i64, vp, vp, i32, vp, vp]),
        'dmf_band_noise_workspace_bytes': (i64, [i32, i32, i32]),
        'dmf_band_noise_moments': (i32, [vp, i32, i32, i32, i64, i32, vp, vp, vp]),
        'dmf_slic_workspace_bytes': (i64, [i32, i32, i32, i32]),
        'dmf_slic_init': (i32, [vp, i32, i32, i32, i32, i32, i32, vp, vp]),
        'dmf_slic_assign': (i32, [vp, i32, i32, i32, i32, i32, i32, f32, vp, vp, vp]),
        'dmf_slic_update': (i32, [vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, i64, vp]),
        'dmf_segment_vote': (i32, [vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp]),
        'dmf_region_workspace_bytes': (i64, [i32, i32, i32]),
        'dmf_region_vote_workspace_bytes': (i64, [i32, i32]),
        'dmf_label_components': (i32, [vp, i32, i32, vp, vp, i64, vp]),
        'dmf_region_merge': (i32, [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, i64, vp]),
        'dmf_region_vote': (i32, [vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, i64, vp]),
        'dmf_region_graph_workspace_bytes': (i64, [i32, i32, i32, i32, i32]),
        'dmf_region_graph_count': (i32, [vp, vp, i32, i32, i32, i32, vp, vp, i64, vp]),
        'dmf_region_graph_merge': (i32, [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, i64, vp]),
        'dmf_morph_workspace_bytes': (i64, [i32, i32, i32, i32]),
        'dmf_morph_state_bytes': (i64, [i32, i32, i32]),
        'dmf_morph_markers': (i32, [vp, i32, i32, i32, i64, i32, C.POINTER(i32), i32, vp, vp, vp, vp]),
        'dmf_morph_reconstruct': (i32, [vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp]),
        'dmf_morph_stack': (i32, [vp, i32, i32, i32, i64, i32, i32, vp, vp, vp, vp]),
        'dmf_attr_workspace_bytes': (i64, [i32, i32, i32, i32, i32]),
        'dmf_attr_quantise': (i32, [vp, i32, i32, i32, i64, i32, i32, vp, vp, vp, i64, vp]),
        'dmf_attr_area_levels': (i32, [vp, i32, i32, i32, C.POINTER(i32), i32, i32, i32, i32, i32, vp, vp, i64, vp]),
        'dmf_attr_stack': (i32, [vp, i32, i32, i32, i64, i32, i32, i32, vp, vp, vp, vp]),
        'dmf_attr_multi_workspace_bytes': (i64, [i32, i32, i32, i32, i32, i32]),
        'dmf_attr_multi_levels': (i32, [vp, i32, i32, i32, C.POINTER(i32), i32, i32, i32, i32, i32, i32, i32, vp, vp, i64, vp]),
    }
    for name, (res, args) in protos.items():
        fn = getattr(lib, name)       # AttributeError here = header and library disagree
        fn.restype, fn.argtypes = res, args
    return lib, tuple(protos)


_lib, EXPORTS = _load()


def check(rc):
    if rc != 0:
        raise DmfError(_lib.dmf_last_error().decode() or 'libdmf_hip error %d' % rc)


def version():
    return _lib.dmf_version()


def make_shape(arch):
    return Shape(C=arch['C'], C2=arch['C2'], P=arch['P'], S=arch['S'], F=arch['F'], G=arch['G'], H=arch['H'],
                 K=arch['K'], attention=arch.get('attention', 0), heads=arch.get('heads', 0), E=arch.get('E', 0), reserved=0)


def shape_supported(shape):
    check(_lib.dmf_shape_supported(C.byref(shape)))


def patch_v2_used(shape, mode=1):
    """True if the train step (mode 1; 0 = forward, 2 = backward from dlogits) of this shape runs the v2 patch kernel."""
    return _lib.dmf_patch_variant(C.byref(shape), mode) == 2


def unit_supported(shape):
    """True if the two-launch unit-gradient step (forward_unit / backward_unit) exists for this shape."""
    return _lib.dmf_unit_supported(C.byref(shape)) == 0


def half_supported(shape):
    """True if the fp16-scene kernels (Input.half) exist for this shape."""
    return _lib.dmf_half_supported(C.byref(shape)) == 0


def require_half(shape):
    check(_lib.dmf_half_supported(C.byref(shape)))


SCALER_FLOATS = 8


def scaler_init(state, init_scale):
    _dev(state, torch.float32, 'scaler state')
    if state.numel() < SCALER_FLOATS:
        raise DmfError('scaler state needs %d floats' % SCALER_FLOATS)
    check(_lib.dmf_scaler_init(_ptr(state), init_scale, _stream()))


def unscale_adam(theta, grad, m, v, lr, b1, b2, eps, scaler_state, growth_factor, backoff_factor, growth_interval,
                 adam_step_dev, grad_scale=1.0, cursor_dev=None, unscaled=False):
    check(_lib.dmf_unscale_adam(_ptr(theta), _ptr(grad), _ptr(m), _ptr(v), theta.numel(), lr, b1, b2, eps, grad_scale,
                                _ptr(scaler_state), growth_factor, backoff_factor, growth_interval, int(bool(unscaled)),
                                _ptr(adam_step_dev), _ptr(cursor_dev), _stream()))


def grad_reduce_scaled(shape, B, ws, grad, scaler_state, cursor_dev=None, loss=None, loss_hist=None):
    check(_lib.dmf_grad_reduce_scaled(C.byref(shape), B, _ptr(ws), _ptr(grad), _ptr(scaler_state), _ptr(cursor_dev),
                                      _ptr(loss), _ptr(loss_hist), _stream()))


def forward_unit(shape, inp, theta, pool_w, logits, ws, adam_step_dev=None):
    check(_lib.dmf_forward_unit(C.byref(shape), C.byref(inp), _ptr(theta), _ptr(pool_w), _ptr(logits), _ptr(ws),
                                _ptr(adam_step_dev), _stream()))


def backward_unit(shape, B, theta, dlogits, ws):
    check(_lib.dmf_backward_unit(C.byref(shape), B, _ptr(theta), _ptr(dlogits), _ptr(ws), _stream()))


def param_layout(shape):
    off = (C.c_int64 * 17)()
    check(_lib.dmf_param_layout(C.byref(shape), off))
    return list(off)


def _bytes(fn, name, shape, B):
    n = fn(C.byref(shape), B)
    if n < 0:
        raise DmfError(name + ' failed')
    return n


def workspace_bytes(shape, B):
    return _bytes(_lib.dmf_workspace_bytes, 'dmf_workspace_bytes', shape, B)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(t, dtype, name):
    if not (t.is_cuda and t.dtype == dtype and t.is_contiguous()):
        raise DmfError('%s must be a contiguous %s tensor on the GPU' % (name, dtype))
    return t


def input_patches(shape, a, b, half=False):
    """mode 0: the reference dataloader's tensors, a [B,C,P,P], b [B,C2,SP,SP] (dataset.py:168-185).
    half: `a` is rounded to fp16 as the kernel stages it (the arithmetic of an fp16 scene)."""
    _dev(a, torch.float32, 'a'); _dev(b, torch.float32, 'b')
    B = a.shape[0]
    SP = shape.S * shape.P
    if tuple(a.shape) != (B, shape.C, shape.P, shape.P) or tuple(b.shape) != (B, shape.C2, SP, SP):
        raise DmfError('patch tensors %s / %s do not match shape C=%d P=%d C2=%d S=%d' %
                       (tuple(a.shape), tuple(b.shape), shape.C, shape.P, shape.C2, shape.S))
    return Input(mode=0, B=B, a=a.data_ptr(), b=b.data_ptr(), sceneA=None, sceneB=None, xy=None, Wp=0, WpB=0, cursor=None,
                 half=int(bool(half)), reserved=0)


def input_gather(shape, sceneA, sceneB, xy, B=None, cursor=None):
    """mode 1: sceneA [Hp,Wp,C], sceneB [HpB,WpB,C2] resident padded scenes, xy [B,2] int32 top-left pixels.
    With `cursor` (device int32[1]) xy is a whole epoch plan [n_steps*B, 2] and `B` the batch size.
    sceneA may be fp16 (Input.half: shapes of half_supported())."""
    half = sceneA.dtype == torch.float16
    _dev(sceneA, torch.float16 if half else torch.float32, 'sceneA'); _dev(sceneB, torch.float32, 'sceneB'); _dev(xy, torch.int32, 'xy')
    if sceneA.dim() != 3 or sceneA.shape[2] != shape.C or sceneB.dim() != 3 or sceneB.shape[2] != shape.C2:
        raise DmfError('scene tensors must be [Hp,Wp,C] and [HpB,WpB,C2]')
    if xy.dim() != 2 or xy.shape[1] != 2:
        raise DmfError('xy must be [B,2]')
    return Input(mode=1, B=xy.shape[0] if B is None else B, a=None, b=None, sceneA=sceneA.data_ptr(),
                 sceneB=sceneB.data_ptr(), xy=xy.data_ptr(), Wp=sceneA.shape[1], WpB=sceneB.shape[1],
                 cursor=None if cursor is None else cursor.data_ptr(), half=int(half), reserved=0)


def check_xy_bounds(shape, sceneA, sceneB, xy_host):
    """Host-side guard (a faulting gather can reset the GPU): every patch window must lie inside the scenes."""
    if len(xy_host) == 0:
        return
    x_max, y_max = int(xy_host[:, 0].max()), int(xy_host[:, 1].max())
    if int(xy_host.min()) < 0 or x_max + shape.P > sceneA.shape[0] or y_max + shape.P > sceneA.shape[1] or \
            shape.S * (x_max + shape.P) > sceneB.shape[0] or shape.S * (y_max + shape.P) > sceneB.shape[1]:
        raise DmfError('patch window outside the padded scene')


def forward(shape, inp, theta, pool_w, logits, pred=None):
    check(_lib.dmf_forward(C.byref(shape), C.byref(inp), _ptr(theta), _ptr(pool_w), _ptr(logits), _ptr(pred), _stream()))


def attn_workspace_bytes(shape, B):
    return _bytes(_lib.dmf_attn_workspace_bytes, 'dmf_attn_workspace_bytes', shape, B)


def forward_attn(shape, inp, theta, pool_w, ws, logits, pred=None):
    check(_lib.dmf_forward_attn(C.byref(shape), C.byref(inp), _ptr(theta), _ptr(pool_w), _ptr(ws), _ptr(logits),
                                _ptr(pred), _stream()))


def train_fwd_bwd(shape, inp, theta, pool_w, labels, loss_scale, logits, loss, ws, adam_step_dev=None, scaler_state=None):
    if scaler_state is not None:
        check(_lib.dmf_train_fwd_bwd_scaled(C.byref(shape), C.byref(inp), _ptr(theta), _ptr(pool_w), _ptr(labels),
                                            C.c_float(loss_scale), _ptr(scaler_state), _ptr(logits), _ptr(loss), _ptr(ws),
                                            _ptr(adam_step_dev), _stream()))
        return
    check(_lib.dmf_train_fwd_bwd(C.byref(shape), C.byref(inp), _ptr(theta), _ptr(pool_w), _ptr(labels),
                                 C.c_float(loss_scale), _ptr(logits), _ptr(loss), _ptr(ws), _ptr(adam_step_dev), _stream()))


def attn_train_workspace_bytes(shape, B):
    return _bytes(_lib.dmf_attn_train_workspace_bytes, 'dmf_attn_train_workspace_bytes', shape, B)


def train_attn_fwd_bwd(shape, inp, theta, pool_w, labels, dlogits, loss_scale, logits, loss, ws, attn_ws,
                       adam_step_dev=None):
    check(_lib.dmf_train_attn_fwd_bwd(C.byref(shape), C.byref(inp), _ptr(theta), _ptr(pool_w), _ptr(labels), _ptr(dlogits),
                                      loss_scale, _ptr(logits), _ptr(loss), _ptr(ws), _ptr(attn_ws), _ptr(adam_step_dev),
                                      _stream()))


def backward_dlogits(shape, inp, theta, pool_w, dlogits, ws):
    check(_lib.dmf_backward_dlogits(C.byref(shape), C.byref(inp), _ptr(theta), _ptr(pool_w), _ptr(dlogits), _ptr(ws), _stream()))


def grad_reduce(shape, B, ws, grad):
    check(_lib.dmf_grad_reduce(C.byref(shape), B, _ptr(ws), _ptr(grad), _stream()))


def adam_step(theta, grad, m, v, lr, b1, b2, eps, step, grad_scale=1.0, adam_step_dev=None, cursor_dev=None):
    check(_lib.dmf_adam_step(_ptr(theta), _ptr(grad), _ptr(m), _ptr(v), theta.numel(), lr, b1, b2, eps, step,
                             grad_scale, _ptr(adam_step_dev), _ptr(cursor_dev), _stream()))


def sgd_step(theta, grad, buf, lr, momentum, step, grad_scale=1.0, step_dev=None, cursor_dev=None):
    check(_lib.dmf_sgd_step(_ptr(theta), _ptr(grad), _ptr(buf), theta.numel(), lr, momentum, step, grad_scale, _ptr(step_dev),
                            _ptr(cursor_dev), _stream()))


def rmsprop_step(theta, grad, sq, lr, alpha, eps=1e-8, grad_scale=1.0, cursor_dev=None):
    check(_lib.dmf_rmsprop_step(_ptr(theta), _ptr(grad), _ptr(sq), theta.numel(), lr, alpha, eps, grad_scale, _ptr(cursor_dev),
                                _stream()))


OPTIM_KINDS = {'ADAM': 0, 'ADAMW': 1, 'SGD': 2, 'RMSprop': 3}          # DMF_OPT_* (include/dmf.h)


def _optim_words(kind, scaler_state, scaler_hparams):
    """What the optim_step wrappers share: -> (DMF_OPT_* of `kind`, growth_factor, backoff_factor, growth_interval), the
    scaler's three neutral without a scaler."""
    if kind not in OPTIM_KINDS:
        raise DmfError('optimizer %r is not one of %s' % (kind, sorted(OPTIM_KINDS)))
    return (OPTIM_KINDS[kind],) + (tuple(scaler_hparams) if scaler_state is not None else (0.0, 0.0, 0))


def optim_step(kind, theta, grad, m, v, lr, b1=0.9, b2=0.999, eps=1e-8, momentum=0.0, alpha=0.99, weight_decay=0.0,
               max_norm=None, step=0, grad_scale=1.0, step_dev=None, cursor_dev=None, scaler_state=None, scaler_hparams=None,
               unscaled=False, norm_hist=None):
    """One optimiser step with weight decay, AdamW and gradient-norm clipping on the flat gradient (dmf_optim_step).  kind: a
    key of OPTIM_KINDS; max_norm None or 0: no clipping; scaler_hparams (growth_factor, backoff_factor, growth_interval) go with
    scaler_state; norm_hist[cursor] gets the pre-clip norm of a clipped step."""
    kind, growth, backoff, interval = _optim_words(kind, scaler_state, scaler_hparams)
    check(_lib.dmf_optim_step(_ptr(theta), _ptr(grad), _ptr(m), _ptr(v), theta.numel(), kind, lr, b1, b2, eps,
                              momentum, alpha, weight_decay, float(max_norm or 0.0), step, grad_scale, _ptr(step_dev),
                              _ptr(cursor_dev), _ptr(scaler_state), growth, backoff, interval, int(bool(unscaled)),
                              _ptr(norm_hist), _stream()))


def hp_schedule(table, row_dev=None):
    """-> HpSchedule of a device table [rows, 4] float32 (lr, beta1, beta2, momentum per row) and the device row index
    (int32 [1]: unit `epoch`; None: unit `step`, row = step count - 1).  The caller keeps both tensors alive."""
    _dev(table, torch.float32, 'schedule table')
    if table.dim() != 2 or table.shape[1] != 4 or table.shape[0] < 1:
        raise DmfError('a schedule table is [rows >= 1, 4]: lr, beta1, beta2, momentum')
    if row_dev is not None:
        _dev(row_dev, torch.int32, 'schedule row index')
    return HpSchedule(table=table.data_ptr(), rows=table.shape[0], row_dev=None if row_dev is None else row_dev.data_ptr())


def _sched_ref(sched):
    return None if sched is None else C.byref(sched)


def optim_step_sched(kind, theta, grad, m, v, sched, eps=1e-8, alpha=0.99, weight_decay=0.0, max_norm=None, step=0,
                     grad_scale=1.0, step_dev=None, cursor_dev=None, scaler_state=None, scaler_hparams=None, unscaled=False,
                     norm_hist=None):
    """optim_step with lr, betas and momentum from the step's row of `sched` (an HpSchedule; dmf_optim_step_sched)."""
    kind, growth, backoff, interval = _optim_words(kind, scaler_state, scaler_hparams)
    check(_lib.dmf_optim_step_sched(_ptr(theta), _ptr(grad), _ptr(m), _ptr(v), theta.numel(), kind, _sched_ref(sched),
                                    eps, alpha, weight_decay, float(max_norm or 0.0), step, grad_scale, _ptr(step_dev),
                                    _ptr(cursor_dev), _ptr(scaler_state), growth, backoff, interval, int(bool(unscaled)),
                                    _ptr(norm_hist), _stream()))


def grad_reduce_adam_sched(shape, B, ws, theta, m, v, grad, sched, eps, step, adam_step_dev=None, cursor_dev=None, loss=None,
                           loss_hist=None):
    """grad_reduce_adam with lr and the betas from the step's row of `sched` (dmf_grad_reduce_adam_sched)."""
    check(_lib.dmf_grad_reduce_adam_sched(C.byref(shape), B, _ptr(ws), _ptr(theta), _ptr(m), _ptr(v), _ptr(grad), _sched_ref(sched),
                                          eps, step, _ptr(adam_step_dev), _ptr(cursor_dev), _ptr(loss), _ptr(loss_hist), _stream()))


def train_plan_steps_sched(shape, inp, theta, pool_w, labels, loss_scale, logits, loss, ws, m, v, sched, eps, adam_step_dev,
                           cursor_dev, loss_hist, n_steps):
    """train_plan_steps with lr and the betas from the steps' rows of `sched` (dmf_train_plan_steps_sched)."""
    check(_lib.dmf_train_plan_steps_sched(C.byref(shape), C.byref(inp), _ptr(theta), _ptr(pool_w), _ptr(labels), loss_scale,
                                          _ptr(logits), _ptr(loss), _ptr(ws), _ptr(m), _ptr(v), _sched_ref(sched), eps,
                                          _ptr(adam_step_dev), _ptr(cursor_dev), _ptr(loss_hist), n_steps, _stream()))


AVG_KINDS = {'ema': 0, 'mean': 1}           # DMF_AVG_* (include/dmf.h)


def weight_avg(avg, kind, decay=0.999, start=1):
    """-> WeightAvg of a device vector `avg` (float32, theta's layout): kind a key of AVG_KINDS, weight the float32 of
    1 - decay formed in double (EMA), start the first averaged optimiser step (1-based).  The caller keeps `avg` alive."""
    if kind not in AVG_KINDS:
        raise DmfError('averaging kind %r is not one of %s' % (kind, sorted(AVG_KINDS)))
    _dev(avg, torch.float32, 'avg')
    return WeightAvg(avg=avg.data_ptr(), kind=AVG_KINDS[kind], weight=1.0 - float(decay), start=int(start), reserved=0)


def _avg_ref(avg):
    return None if avg is None else C.byref(avg)


def weight_average(avg, theta, step=0, step_dev=None):
    """The averaging rule alone on theta (dmf_weight_average); avg: a WeightAvg."""
    check(_lib.dmf_weight_average(_avg_ref(avg), _ptr(theta), theta.numel(), step, _ptr(step_dev), _stream()))


def optim_step_avg(kind, theta, grad, m, v, avg, sched=None, lr=0.0, b1=0.9, b2=0.999, eps=1e-8, momentum=0.0, alpha=0.99,
                   weight_decay=0.0, max_norm=None, step=0, grad_scale=1.0, step_dev=None, cursor_dev=None, scaler_state=None,
                   scaler_hparams=None, unscaled=False, norm_hist=None):
    """optim_step (sched None) or optim_step_sched that also keeps the averaged copy `avg` (a WeightAvg; dmf_optim_step_avg)."""
    kind, growth, backoff, interval = _optim_words(kind, scaler_state, scaler_hparams)
    check(_lib.dmf_optim_step_avg(_ptr(theta), _ptr(grad), _ptr(m), _ptr(v), theta.numel(), kind, lr, b1, b2, eps,
                                  momentum, alpha, weight_decay, float(max_norm or 0.0), step, grad_scale, _ptr(step_dev),
                                  _ptr(cursor_dev), _ptr(scaler_state), growth, backoff, interval, int(bool(unscaled)),
                                  _ptr(norm_hist), _sched_ref(sched), _avg_ref(avg), _stream()))


def grad_reduce_adam_avg(shape, B, ws, theta, m, v, grad, lr, b1, b2, eps, step, avg, sched=None, adam_step_dev=None,
                         cursor_dev=None, loss=None, loss_hist=None):
    """grad_reduce_adam (sched None) or grad_reduce_adam_sched that also keeps `avg` (dmf_grad_reduce_adam_avg)."""
    check(_lib.dmf_grad_reduce_adam_avg(C.byref(shape), B, _ptr(ws), _ptr(theta), _ptr(m), _ptr(v), _ptr(grad), lr, b1, b2, eps,
                                        step, _ptr(adam_step_dev), _ptr(cursor_dev), _ptr(loss), _ptr(loss_hist),
                                        _sched_ref(sched), _avg_ref(avg), _stream()))


def train_plan_steps_avg(shape, inp, theta, pool_w, labels, loss_scale, logits, loss, ws, m, v, lr, b1, b2, eps, adam_step_dev,
                         cursor_dev, loss_hist, sched, avg, n_steps):
    """train_plan_steps / _sched whose steps also keep `avg` (dmf_train_plan_steps_avg)."""
    check(_lib.dmf_train_plan_steps_avg(C.byref(shape), C.byref(inp), _ptr(theta), _ptr(pool_w), _ptr(labels), loss_scale,
                                        _ptr(logits), _ptr(loss), _ptr(ws), _ptr(m), _ptr(v), lr, b1, b2, eps, _ptr(adam_step_dev),
                                        _ptr(cursor_dev), _ptr(loss_hist), _sched_ref(sched), _avg_ref(avg), n_steps, _stream()))


def grad_reduce_adam(shape, B, ws, theta, m, v, grad, lr, b1, b2, eps, step, adam_step_dev=None, cursor_dev=None,
                     loss=None, loss_hist=None):
    check(_lib.dmf_grad_reduce_adam(C.byref(shape), B, _ptr(ws), _ptr(theta), _ptr(m), _ptr(v), _ptr(grad),
                                    lr, b1, b2, eps, step, _ptr(adam_step_dev), _ptr(cursor_dev), _ptr(loss),
                                    _ptr(loss_hist), _stream()))


def forward_ce(shape, inp, theta, pool_w, labels, logits, loss, pred=None):
    """Evaluation forward + per-patch cross-entropy in the same launch (dmf_forward_ce); raises DmfError where the shape has no
    such kernel (the caller then uses forward() + its own loss)."""
    check(_lib.dmf_forward_ce(C.byref(shape), C.byref(inp), _ptr(theta), _ptr(pool_w), _ptr(labels), _ptr(logits), _ptr(loss),
                              _ptr(pred), _stream()))


def train_plan_steps(shape, inp, theta, pool_w, labels, loss_scale, logits, loss, ws, m, v, lr, b1, b2, eps, adam_step_dev, cursor_dev,
                     loss_hist, n_steps):
    """n_steps fused train steps on consecutive batches of a resident plan, enqueued by one C loop (dmf_train_plan_steps)."""
    check(_lib.dmf_train_plan_steps(C.byref(shape), C.byref(inp), _ptr(theta), _ptr(pool_w), _ptr(labels), loss_scale, _ptr(logits),
                                    _ptr(loss), _ptr(ws), _ptr(m), _ptr(v), lr, b1, b2, eps, _ptr(adam_step_dev), _ptr(cursor_dev),
                                    _ptr(loss_hist), n_steps, _stream()))


def grad_reduce_xgmi_adam(shape, B, ws, theta, m, v, comm, lr, b1, b2, eps, grad_scale, adam_step_dev, cursor_dev=None,
                          loss=None, loss_hist=None):
    check(_lib.dmf_grad_reduce_xgmi_adam(C.byref(shape), B, _ptr(ws), _ptr(theta), _ptr(m), _ptr(v), C.byref(comm), lr, b1,
                                         b2, eps, grad_scale, _ptr(adam_step_dev), _ptr(cursor_dev), _ptr(loss),
                                         _ptr(loss_hist), _stream()))


def hip_runtime_of_torch():
    """The libamdhip64 this process already has mapped (torch's own), found in /proc/self/maps — dlopen by bare name could
    bind a second copy of the runtime, whose stream and graph handles mean nothing to the first.  None if not found."""
    try:
        with open('/proc/self/maps') as f:
            for line in f:
                path = line.split(None, 5)[-1].strip() if line.count('/') else ''
                if 'libamdhip64.so' in path:
                    return C.CDLL(path)
    except OSError:
        pass
    return None


def xgmi_sizes(capacity, world):
    d, f = C.c_int64(), C.c_int64()
    check(_lib.dmf_xgmi_sizes(capacity, world, C.byref(d), C.byref(f)))
    return d.value, f.value


def xgmi_alloc(nbytes):
    p = C.c_void_p()
    check(_lib.dmf_xgmi_alloc(nbytes, C.byref(p)))
    return p.value


def xgmi_free(ptr):
    check(_lib.dmf_xgmi_free(C.c_void_p(ptr)))


def xgmi_export(ptr):
    h = C.create_string_buffer(64)
    check(_lib.dmf_xgmi_export(C.c_void_p(ptr), h))
    return h.raw


def xgmi_open(handle):
    p = C.c_void_p()
    check(_lib.dmf_xgmi_open(C.create_string_buffer(handle, 64), C.byref(p)))
    return p.value


def xgmi_close(ptr):
    check(_lib.dmf_xgmi_close(C.c_void_p(ptr)))


def xgmi_status(comm):
    st = C.c_int32()
    check(_lib.dmf_xgmi_status(C.byref(comm), C.byref(st)))
    return st.value


def xgmi_allreduce(comm, buf, n, seq):
    _dev(buf, torch.float32, 'buf')
    check(_lib.dmf_xgmi_allreduce(C.byref(comm), _ptr(buf), n, seq, _stream()))


def qua_params(dqtl):
    """cfg['dqtl'] -> QuaParams (train/loss_function.py:21,32,66-68)."""
    return QuaParams(alpha=dqtl['alpha'], beta=dqtl['beta'], gamma=dqtl['gamma'], epsilon=dqtl['epsilon'], tao=dqtl['tao'])


def qua_loss(logits, bs, labels, params, loss=None, dlogits=None, grad_scale=1.0, cursor=None, loss_hist=None,
             scaler_state=None):
    _dev(logits, torch.float32, 'logits'); _dev(labels, torch.int32, 'labels')
    K = logits.shape[1]
    if logits.dim() != 2 or logits.shape[0] != 4 * bs:
        raise DmfError('qua_loss wants logits [4*bs, K]')
    if cursor is None and labels.numel() < bs:
        raise DmfError('qua_loss wants one label per sample')
    if dlogits is not None:
        _dev(dlogits, torch.float32, 'dlogits')
        if dlogits.shape != logits.shape:
            raise DmfError('dlogits must have the shape of logits')
    check(_lib.dmf_qua_loss_scaled(_ptr(logits), bs, K, _ptr(labels), _ptr(cursor), C.byref(params), grad_scale,
                                   _ptr(scaler_state), _ptr(loss), _ptr(loss_hist), _ptr(dlogits), _stream()))


def qua_loss_ranks(gathered, ranks, rank, bs_r, labels_global, params, loss=None, dlogits=None, grad_scale=1.0, cursor=None,
                   loss_hist=None, scaler_state=None):
    """qua_loss of the GLOBAL batch of `ranks` data-parallel ranks from their gathered logits [ranks*4*bs_r, K] (rank-major,
    as all_gather_into_tensor leaves them); dlogits [4*bs_r, K]: rank `rank`'s rows.  ranks = 1 is qua_loss."""
    _dev(gathered, torch.float32, 'gathered'); _dev(labels_global, torch.int32, 'labels_global')
    if gathered.dim() != 2 or gathered.shape[0] != 4 * ranks * bs_r:
        raise DmfError('qua_loss_ranks wants gathered logits [ranks*4*bs_r, K]')
    if not 0 <= rank < ranks:
        raise DmfError('qua_loss_ranks: rank %d of %d ranks' % (rank, ranks))
    if cursor is None and labels_global.numel() < ranks * bs_r:
        raise DmfError('qua_loss_ranks wants one label per sample of the global batch')
    if dlogits is not None:
        _dev(dlogits, torch.float32, 'dlogits')
        if dlogits.shape != (4 * bs_r, gathered.shape[1]):
            raise DmfError('dlogits must be [4*bs_r, K]: this rank\'s rows')
    check(_lib.dmf_qua_loss_ranks(_ptr(gathered), ranks, rank, bs_r, gathered.shape[1], _ptr(labels_global), _ptr(cursor),
                                  C.byref(params), grad_scale, _ptr(scaler_state), _ptr(loss), _ptr(loss_hist), _ptr(dlogits),
                                  _stream()))


CE_KINDS = {'ce': 0, 'focal': 1}


def ce_params(kind='ce', label_smoothing=0.0, gamma=0.0):
    """-> CeParams (include/dmf.h: dmf_ce_params); kind 'ce' (class weights, label smoothing) or 'focal' (class weights, gamma)."""
    if kind not in CE_KINDS:
        raise DmfError('criterion kind %r is not one of %s' % (kind, sorted(CE_KINDS)))
    return CeParams(kind=CE_KINDS[kind], label_smoothing=float(label_smoothing), gamma=float(gamma))


def ce_loss(logits, ranks, rank, labels_global, params, class_w=None, loss=None, dlogits=None, grad_scale=1.0, cursor=None,
            scaler_state=None):
    """The weighted / smoothed cross-entropy or focal loss (dmf_ce_loss) of rank `rank`'s logits [bs_r, K] inside the GLOBAL
    batch of ranks * bs_r samples whose labels are labels_global (at row *cursor of a plan, rank-major): loss [bs_r] <-
    ranks * bs_r * t_i / D, dlogits [bs_r, K] <- d(batch loss) / d logits * grad_scale * scaler_state[0]."""
    _dev(logits, torch.float32, 'logits'); _dev(labels_global, torch.int32, 'labels_global')
    if logits.dim() != 2 or logits.shape[0] < 1:
        raise DmfError('ce_loss wants logits [bs_r, K] with at least one row')
    bs_r, K = logits.shape
    if not 0 <= rank < ranks:
        raise DmfError('ce_loss: rank %d of %d ranks' % (rank, ranks))
    if cursor is None and labels_global.numel() < ranks * bs_r:
        raise DmfError('ce_loss wants one label per sample of the global batch')
    if class_w is not None:
        _dev(class_w, torch.float32, 'class_w')
        if class_w.numel() != K:
            raise DmfError('class_w must hold one weight per class (%d), got %d' % (K, class_w.numel()))
    if loss is not None:
        _dev(loss, torch.float32, 'loss')
        if loss.numel() < bs_r:
            raise DmfError('loss must hold one term per row')
    if dlogits is not None:
        _dev(dlogits, torch.float32, 'dlogits')
        if dlogits.shape != logits.shape:
            raise DmfError('dlogits must have the shape of logits')
    check(_lib.dmf_ce_loss(_ptr(logits), ranks, rank, bs_r, K, _ptr(labels_global), _ptr(cursor), _ptr(class_w),
                           C.byref(params), grad_scale, _ptr(scaler_state), _ptr(loss), _ptr(dlogits), _stream()))


def ce_denominators(labels_global, N, K, denom, class_w=None):
    """denom[r] <- sum over the N labels of row r of labels_global [rows * N] of (double)class_w[label] (None: ones), the bits of
    the denominator dmf_ce_loss forms for that row (dmf_ce_denominators); rows = labels_global.numel() // N."""
    _dev(labels_global, torch.int32, 'labels_global'); _dev(denom, torch.float64, 'denom')
    if N < 1 or labels_global.numel() % N:
        raise DmfError('ce_denominators wants rows of %d labels, got %d labels' % (N, labels_global.numel()))
    rows = labels_global.numel() // N
    if denom.numel() < rows:
        raise DmfError('denom must hold one denominator per row (%d), got %d' % (rows, denom.numel()))
    if class_w is not None:
        _dev(class_w, torch.float32, 'class_w')
        if class_w.numel() != K:
            raise DmfError('class_w must hold one weight per class (%d), got %d' % (K, class_w.numel()))
    check(_lib.dmf_ce_denominators(_ptr(labels_global), N, rows, K, _ptr(class_w), _ptr(denom), _stream()))


def train_attn_fwd_bwd_ce(shape, inp, theta, pool_w, labels_global, denom, params, ranks, rank, logits, loss, ws, attn_ws,
                          class_w=None, grad_scale=1.0, adam_step_dev=None):
    """The attention network's train step with the criterion `params` / class_w evaluated inside the attention kernel
    (dmf_train_attn_fwd_bwd_ce): labels_global [rows, ranks * B] rank-major and denom [rows] (ce_denominators), both read at row
    *inp.cursor (row 0 without a cursor); loss [B] may be None."""
    _dev(labels_global, torch.int32, 'labels_global'); _dev(denom, torch.float64, 'denom')
    if not 0 <= rank < ranks:
        raise DmfError('train_attn_fwd_bwd_ce: rank %d of %d ranks' % (rank, ranks))
    if not inp.cursor and (labels_global.numel() < ranks * inp.B or denom.numel() < 1):
        raise DmfError('train_attn_fwd_bwd_ce wants one label per sample of the global batch and its denominator')
    if class_w is not None:
        _dev(class_w, torch.float32, 'class_w')
        if class_w.numel() != shape.K:
            raise DmfError('class_w must hold one weight per class (%d), got %d' % (shape.K, class_w.numel()))
    ce = CeFused(params=C.pointer(params), class_w=None if class_w is None else class_w.data_ptr(),
                 labels_global=labels_global.data_ptr(), denom=denom.data_ptr(), ranks=ranks, rank=rank, grad_scale=grad_scale,
                 reserved=0)
    check(_lib.dmf_train_attn_fwd_bwd_ce(C.byref(shape), C.byref(inp), _ptr(theta), _ptr(pool_w), C.byref(ce), _ptr(logits),
                                         _ptr(loss), _ptr(ws), _ptr(attn_ws), _ptr(adam_step_dev), _stream()))


def pair_argmax(logits, bs, pred):
    _dev(logits, torch.float32, 'logits'); _dev(pred, torch.int32, 'pred')
    if logits.dim() != 2 or logits.shape[0] < 2 * bs or pred.numel() < bs:
        raise DmfError('pair_argmax wants logits [>=2*bs, K] and pred [bs]')
    check(_lib.dmf_pair_argmax(_ptr(logits), bs, logits.shape[1], _ptr(pred), _stream()))


def band_mean_scene(scene):
    """[Hp, Wp, C] resident scene -> [Hp, Wp, 1] band mean."""
    _dev(scene, torch.float32, 'scene')
    out = torch.empty(scene.shape[0], scene.shape[1], 1, device=scene.device)
    check(_lib.dmf_band_mean(_ptr(scene), 0, 1, scene.shape[0] * scene.shape[1], scene.shape[2], _ptr(out), _stream()))
    return out


def band_mean_patches(a):
    """[B, C, P, P] patches -> [B, 1, P, P] band mean."""
    _dev(a, torch.float32, 'a')
    out = torch.empty(a.shape[0], 1, a.shape[2], a.shape[3], device=a.device)
    if a.shape[0]:
        check(_lib.dmf_band_mean(_ptr(a), 1, a.shape[0], a.shape[2] * a.shape[3], a.shape[1], _ptr(out), _stream()))
    return out


def confusion_accum(pred, target, K, matrix):
    check(_lib.dmf_confusion_accum(_ptr(pred), _ptr(target), pred.numel(), K, _ptr(matrix), _stream()))


def labelmap_write(pred, xy, W, label_map):
    check(_lib.dmf_labelmap_write(_ptr(pred), _ptr(xy), pred.numel(), W, _ptr(label_map), _stream()))


def softmax_stats(logits, pred=None, conf=None, margin=None, entropy=None, inv_temp=None, xy=None, W=0):
    """Argmax (first maximal index), confidence, margin and entropy of every row of logits [B, K] (dmf_softmax_stats), each
    output optional.  inv_temp: device float32 [1], beta = 1 / T (None: 1).  Without xy row i writes element i of the
    outputs; with xy [B, 2] int32 it writes element x * W + y of maps the caller has sized and whose bounds it has checked."""
    _dev(logits, torch.float32, 'logits')
    if logits.dim() != 2:
        raise DmfError('softmax_stats wants logits [B, K]')
    B, K = logits.shape
    if inv_temp is not None:
        _dev(inv_temp, torch.float32, 'inv_temp')
        if inv_temp.numel() < 1:
            raise DmfError('inv_temp holds one float')
    if xy is not None:
        _dev(xy, torch.int32, 'xy')
        if xy.dim() != 2 or tuple(xy.shape) != (B, 2):
            raise DmfError('xy must be [B, 2]')
    for t, dt, name in ((pred, torch.int32, 'pred'), (conf, torch.float32, 'conf'), (margin, torch.float32, 'margin'),
                        (entropy, torch.float32, 'entropy')):
        if t is not None:
            _dev(t, dt, name)
            if xy is None and t.numel() < B:
                raise DmfError('%s must hold one element per row' % name)
    check(_lib.dmf_softmax_stats(_ptr(logits), B, K, _ptr(inv_temp), _ptr(xy), W, _ptr(pred), _ptr(conf), _ptr(margin),
                                 _ptr(entropy), _stream()))


def calib_accum(conf, pred, target, K, hist):
    """hist [nbins, 3] int64 += the reliability histogram of conf / pred / target [B] (dmf_calib_accum): rows, hits and the
    confidence sum in units of 2^-32 per bin; rows whose target lies outside [0, K) are skipped."""
    _dev(conf, torch.float32, 'conf'); _dev(pred, torch.int32, 'pred'); _dev(target, torch.int32, 'target')
    _dev(hist, torch.int64, 'hist')
    if hist.dim() != 2 or hist.shape[1] != 3:
        raise DmfError('hist must be [nbins, 3]')
    B = conf.numel()
    if pred.numel() < B or target.numel() < B:
        raise DmfError('calib_accum: pred and target must hold one element per confidence')
    check(_lib.dmf_calib_accum(_ptr(conf), _ptr(pred), _ptr(target), B, K, hist.shape[0], _ptr(hist), _stream()))


TEMP_DOUBLES = 8                             # DMF_TEMP_DOUBLES: beta, nll, g, h, lo, hi, steps taken, reserved


def temperature_init(state):
    """state [TEMP_DOUBLES] float64 on the device <- beta = 1 in the bracket [2^-6, 2^6] (dmf_temperature_init)."""
    _dev(state, torch.float64, 'temperature state')
    if state.numel() < TEMP_DOUBLES:
        raise DmfError('temperature state needs %d doubles' % TEMP_DOUBLES)
    check(_lib.dmf_temperature_init(_ptr(state), _stream()))


def temperature_workspace_bytes(N):
    n = _lib.dmf_temperature_workspace_bytes(N)
    if n < 0:
        raise DmfError('dmf_temperature_workspace_bytes failed')
    return n


def temperature_step(logits, labels, state, ws, update=True):
    """One step of the temperature fit on logits [N, K] / labels [N] int32 (dmf_temperature_step): nll, g and h at state's beta,
    then with `update` the safeguarded Newton step.  ws: uint8, at least temperature_workspace_bytes(N)."""
    _dev(logits, torch.float32, 'logits'); _dev(labels, torch.int32, 'labels'); _dev(state, torch.float64, 'temperature state')
    if logits.dim() != 2 or labels.numel() < logits.shape[0] or state.numel() < TEMP_DOUBLES:
        raise DmfError('temperature_step wants logits [N, K], one label per row and a state of %d doubles' % TEMP_DOUBLES)
    N, K = logits.shape
    if ws is None or ws.numel() * ws.element_size() < temperature_workspace_bytes(N):
        raise DmfError('temperature_step: the workspace is smaller than temperature_workspace_bytes(%d)' % N)
    check(_lib.dmf_temperature_step(_ptr(logits), _ptr(labels), N, K, _ptr(state), _ptr(ws), int(bool(update)), _stream()))


def valid_accum(loss, n, acc):
    """acc [1] float64 += the double-precision sum of loss[:n] (float32), in a fixed order (dmf_valid_accum)."""
    _dev(loss, torch.float32, 'loss'); _dev(acc, torch.float64, 'acc')
    if n > loss.numel() or acc.numel() < 1:
        raise DmfError('valid_accum: loss holds %d terms, %d asked for' % (loss.numel(), n))
    check(_lib.dmf_valid_accum(_ptr(loss), n, _ptr(acc), _stream()))


def keep_best(acc, best, best_epoch, epoch, theta, best_theta, val_hist):
    """The end of an epoch's validation pass (dmf_keep_best): val_hist[epoch] <- acc[0]; a sum strictly below best[0] becomes
    the best, with best_epoch[0] and a copy of theta in best_theta; acc[0] <- 0.  Every tensor lives on the device."""
    for t, dt, name in ((acc, torch.float64, 'acc'), (best, torch.float64, 'best'), (best_epoch, torch.int32, 'best_epoch'),
                        (theta, torch.float32, 'theta'), (best_theta, torch.float32, 'best_theta'), (val_hist, torch.float64, 'val_hist')):
        _dev(t, dt, name)
    if not 0 <= epoch < val_hist.numel():
        raise DmfError('keep_best: epoch %d outside the validation history of %d' % (epoch, val_hist.numel()))
    if best_theta.numel() != theta.numel() or min(acc.numel(), best.numel(), best_epoch.numel()) < 1:
        raise DmfError('keep_best: best_theta must have the size of theta; acc, best and best_epoch one element')
    check(_lib.dmf_keep_best(_ptr(acc), _ptr(best), _ptr(best_epoch), epoch, _ptr(theta), _ptr(best_theta), theta.numel(),
                             _ptr(val_hist), _stream()))


def pan2ms(pan, H, W, out):
    check(_lib.dmf_pan2ms(_ptr(pan), pan.shape[1], H, W, _ptr(out), _stream()))


# DMF_RAW_* (include/dmf.h): the dtypes a raw scene may be uploaded in, by numpy name -> (code, bytes per element)
RAW_DTYPES = {'uint8': (0, 1), 'uint16': (1, 2), 'int16': (2, 2), 'int32': (3, 4), 'float32': (4, 4), 'float64': (5, 8)}


def raw_code(dtype):
    """DMF_RAW_* code of a numpy dtype, or None where it has none (bool, complex, int64, a foreign byte order ...)."""
    import numpy as np
    dtype = np.dtype(dtype)
    return RAW_DTYPES[dtype.name][0] if dtype.name in RAW_DTYPES and dtype.isnative else None


def _raw(raw, dtype_name, n):
    code, size = RAW_DTYPES[dtype_name]
    _dev(raw, torch.uint8, 'raw scene (its bytes)')
    if raw.numel() != n * size:
        raise DmfError('raw scene: %d bytes for %d %s elements' % (raw.numel(), n, dtype_name))
    return code, size


def scene_minmax(raw, dtype_name, minmax):
    """raw: the bytes of a raw scene (uint8 tensor) of numpy dtype `dtype_name`; minmax (uint8, >= 2 elements of that
    dtype) <- {min, max} in the raw dtype."""
    code, size = RAW_DTYPES[dtype_name]
    _raw(raw, dtype_name, raw.numel() // size)
    _dev(minmax, torch.uint8, 'minmax')
    if minmax.numel() < 2 * size or minmax.device != raw.device:
        raise DmfError('minmax wants two elements of the raw dtype on the scene\'s device')
    check(_lib.dmf_scene_minmax(_ptr(raw), code, raw.numel() // size, _ptr(minmax), _stream()))


def scene_prepare(raw, dtype_name, H, W, C, minmax, pad, out):
    """out [H+pad, W+pad, C] (fp32 or fp16) <- the normalised, reflect-padded scene of raw [H, W, C] (its bytes) and the
    minmax of scene_minmax."""
    code, size = _raw(raw, dtype_name, H * W * C)
    _dev(minmax, torch.uint8, 'minmax')
    if out.dtype not in (torch.float32, torch.float16):
        raise DmfError('the prepared scene is fp32 or fp16')
    _dev(out, out.dtype, 'out')
    if minmax.numel() < 2 * size or minmax.device != raw.device or out.device != raw.device:
        raise DmfError('raw scene, minmax and out must live on one device')
    if pad < 0 or out.numel() != (H + pad) * (W + pad) * C:
        raise DmfError('out must hold [%d, %d, %d] elements' % (H + pad, W + pad, C))
    check(_lib.dmf_scene_prepare(_ptr(raw), code, H, W, C, _ptr(minmax), pad, int(out.dtype == torch.float16), _ptr(out),
                                 _stream()))


# return codes of the two entry points of csrc/dmf_augment.hip, which report by code (include/dmf.h)
_ATLAS_ERRORS = {1: 'a NULL pointer', 2: 'rows, cols and C must be >= 1 and src_pitch >= cols', 3: 'elem_bytes must be 2 or 4',
                 4: 'n_ops must be 1..8 and every op 0..7', 5: 'slot_rows / dst_pitch too small for a requested variant',
                 6: 'src / dst not aligned to the element size', 7: 'dst overlaps src',
                 8: 'a row or a grid beyond 32 bits', 9: 'the launch failed'}
_MEAN_ERRORS = {1: 'a NULL pointer', 2: 'V must be >= 1 and B >= 0', 3: '1 <= K <= DMF_KMAX', 9: 'the launch failed'}


def scene_atlas(src, rows, cols, ops, slot_rows, dst):
    """dst [len(ops) * slot_rows, dst_pitch, C] <- the variants `ops` (0..7: transpose 4, reverse rows 2, reverse columns 1) of
    the leading [rows, cols] pixels of src [>= rows, src_pitch, C], one per slot, zero-filled (dmf_scene_atlas).  src and dst
    are contiguous device tensors of one 2- or 4-byte dtype; every byte of dst is written."""
    for t, name in ((src, 'src'), (dst, 'dst')):
        if not (t.is_cuda and t.is_contiguous() and t.dim() == 3 and t.element_size() in (2, 4)):
            raise DmfError('scene_atlas: %s must be a contiguous [rows, pitch, C] GPU tensor of 2- or 4-byte elements' % name)
    ops = [int(k) for k in ops]
    if src.dtype != dst.dtype or src.device != dst.device or src.shape[2] != dst.shape[2]:
        raise DmfError('scene_atlas: src and dst must share dtype, device and C')
    if rows > src.shape[0] or dst.shape[0] != len(ops) * slot_rows:
        raise DmfError('scene_atlas: src holds %d rows (%d asked for), dst %d (%d slots of %d)'
                       % (src.shape[0], rows, dst.shape[0], len(ops), slot_rows))
    rc = _lib.dmf_scene_atlas(_ptr(src), src.element_size(), rows, cols, src.shape[1], src.shape[2], (C.c_int32 * len(ops))(*ops),
                              len(ops), slot_rows, dst.shape[1], _ptr(dst), _stream())
    if rc != 0:
        raise DmfError('dmf_scene_atlas: ' + _ATLAS_ERRORS.get(rc, 'error %d' % rc))


def logits_mean(logits_v, logits, pred=None):
    """logits [B, K] <- the mean over V of logits_v [V, B, K] (fp32, summed in variant order, then / V); pred [B] int32 <- the
    first maximal index of each mean row (dmf_logits_mean)."""
    _dev(logits_v, torch.float32, 'logits_v'); _dev(logits, torch.float32, 'logits')
    if logits_v.dim() != 3 or logits_v.shape[0] < 1 or logits.dim() != 2 or tuple(logits.shape) != tuple(logits_v.shape[1:]):
        raise DmfError('logits_mean wants logits_v [V >= 1, B, K] and logits [B, K]')
    V, B, K = logits_v.shape
    if pred is not None:
        _dev(pred, torch.int32, 'pred')
        if pred.numel() < B:
            raise DmfError('pred must hold one element per row')
    if B == 0:                                  # (an empty tensor has a null data pointer)
        return
    rc = _lib.dmf_logits_mean(_ptr(logits_v), V, B, K, _ptr(logits), _ptr(pred), _stream())
    if rc != 0:
        raise DmfError('dmf_logits_mean: ' + _MEAN_ERRORS.get(rc, 'error %d' % rc))


def _code_check(errors, entry, rc):
    """An entry point that reports by return code (include/dmf.h): `errors` is its table of texts."""
    if rc != 0:
        raise DmfError('%s: %s' % (entry, errors.get(rc, 'error %d' % rc)))


def _resident_scene(entry, scene):
    if not (scene.is_cuda and scene.is_contiguous() and scene.dim() == 3 and scene.dtype in (torch.float32, torch.float16)):
        raise DmfError('%s: the scene must be a contiguous [rows, pitch, C] fp32 or fp16 GPU tensor' % entry)


# return codes of the three entry points of csrc/dmf_spatial.hip, which report by code (include/dmf.h)
_SPATIAL_ERRORS = {1: 'a NULL pointer', 2: 'H, W and C must be >= 1 (scatter: B >= 0 and W >= 1)', 3: '1 <= K <= DMF_KMAX',
                   4: 'the radius must be 1, 2 or 3', 5: 'elem_bytes must be 2 or 4', 6: 'pitch < W', 7: 'prob_out overlaps prob_in',
                   8: 'the scene is not aligned to its element size, or a grid beyond 32 bits', 9: 'the launch failed'}


def _window(radius):
    if isinstance(radius, bool) or not isinstance(radius, int) or not 1 <= radius <= 3:
        raise DmfError('the radius %r is not 1, 2 or 3' % (radius,))
    return (2 * radius + 1) ** 2


def prob_scatter(logits, xy, W, prob, mask, inv_temp=None):
    """prob [H, W, K] float32 / mask [H, W] uint8 <- the softmax at beta = inv_temp[0] (device float32 [1]; None: 1) of every row
    of logits [B, K], written at the row's pixel xy [B, 2] int32: prob[x, y, :] = e / Z as dmf_softmax_stats forms them,
    mask[x, y] = 1 (dmf_prob_scatter).  Other cells stay as they are; the caller has checked the pixels against [H, W]."""
    _dev(logits, torch.float32, 'logits'); _dev(xy, torch.int32, 'xy'); _dev(prob, torch.float32, 'prob'); _dev(mask, torch.uint8, 'mask')
    if logits.dim() != 2 or tuple(xy.shape) != (logits.shape[0], 2):
        raise DmfError('prob_scatter wants logits [B, K] and xy [B, 2]')
    B, K = logits.shape
    if inv_temp is not None:
        _dev(inv_temp, torch.float32, 'inv_temp')
        if inv_temp.numel() < 1:
            raise DmfError('inv_temp holds one float')
    if prob.dim() != 3 or prob.shape[1] != W or prob.shape[2] != K or tuple(mask.shape) != tuple(prob.shape[:2]):
        raise DmfError('prob_scatter wants prob [H, %d, %d] and mask [H, %d]' % (W, K, W))
    if B == 0:                                  # (an empty tensor has a null data pointer)
        return
    _code_check(_SPATIAL_ERRORS, 'dmf_prob_scatter',
                _lib.dmf_prob_scatter(_ptr(logits), B, K, _ptr(inv_temp), _ptr(xy), W, _ptr(prob), _ptr(mask), _stream()))


def spatial_affinity(scene, H, W, radius, sigma_s, sigma_r, aff):
    """aff [H, W, n] float32, n = (2 radius + 1)^2 <- the bilateral affinities of the leading [H, W] pixels of the resident
    scene [>= H, pitch >= W, C] (fp32 or fp16, contiguous): exp(-(|d|^2 / (2 sigma_s^2) + mean_c (a_c(x) - a_c(y))^2 /
    (2 sigma_r^2))), 0 for a neighbour outside [0, H) x [0, W), 1 at the centre (dmf_spatial_affinity)."""
    n = _window(radius)
    _resident_scene('spatial_affinity', scene)
    _dev(aff, torch.float32, 'aff')
    if H < 1 or W < 1 or H > scene.shape[0] or W > scene.shape[1]:
        raise DmfError('spatial_affinity: %d x %d pixels asked of a scene of %d x %d' % (H, W, scene.shape[0], scene.shape[1]))
    if tuple(aff.shape) != (H, W, n) or aff.device != scene.device:
        raise DmfError('spatial_affinity: aff must be [%d, %d, %d] on the scene\'s device' % (H, W, n))
    for name, s in (('sigma_s', sigma_s), ('sigma_r', sigma_r)):
        if not (s > 0 and s < float('inf')):
            raise DmfError('spatial_affinity: %s = %r is not a finite number > 0' % (name, s))
    cs, cr = 1.0 / (2.0 * float(sigma_s) ** 2), 1.0 / (2.0 * float(sigma_r) ** 2)
    _code_check(_SPATIAL_ERRORS, 'dmf_spatial_affinity', _lib.dmf_spatial_affinity(
        _ptr(scene), scene.element_size(), scene.shape[1], H, W, scene.shape[2], radius, cs, cr, _ptr(aff), _stream()))


def spatial_filter(prob_in, mask, aff, prob_out, label_map):
    """One iteration of the filter (dmf_spatial_filter): prob_out [H, W, K] <- the aff-weighted mean of prob_in over the masked
    neighbours of every masked pixel (an all-zero row elsewhere); label_map [H, W] int32 <- its first maximal index at the
    masked pixels, the other cells untouched.  aff [H, W, n]; mask [H, W] uint8; prob_out must not overlap prob_in."""
    _dev(prob_in, torch.float32, 'prob_in'); _dev(prob_out, torch.float32, 'prob_out'); _dev(mask, torch.uint8, 'mask')
    _dev(aff, torch.float32, 'aff'); _dev(label_map, torch.int32, 'label_map')
    if prob_in.dim() != 3 or aff.dim() != 3 or tuple(prob_out.shape) != tuple(prob_in.shape):
        raise DmfError('spatial_filter wants prob_in and prob_out [H, W, K] and aff [H, W, n]')
    H, W, K = prob_in.shape
    radius = {9: 1, 25: 2, 49: 3}.get(aff.shape[2])
    if radius is None or tuple(aff.shape[:2]) != (H, W) or tuple(mask.shape) != (H, W) or tuple(label_map.shape) != (H, W):
        raise DmfError('spatial_filter: aff [%d, %d, 9 | 25 | 49], mask and label_map [%d, %d] go with prob [%d, %d, %d]'
                       % (H, W, H, W, H, W, K))
    if len({t.device for t in (prob_in, prob_out, mask, aff, label_map)}) != 1:
        raise DmfError('spatial_filter: all tensors must live on one device')
    _code_check(_SPATIAL_ERRORS, 'dmf_spatial_filter', _lib.dmf_spatial_filter(
        _ptr(prob_in), _ptr(mask), _ptr(aff), H, W, K, radius, _ptr(prob_out), _ptr(label_map), _stream()))


# return codes of the entry points of csrc/dmf_segments.hip, which report by code (include/dmf.h)
SEG_SMIN, SEG_SMAX = 4, 32                      # DMF_SEG_SMIN, DMF_SEG_SMAX
VOTE_MODES = {'mean': 0, 'majority': 1}         # DMF_VOTE_MEAN, DMF_VOTE_MAJORITY
_SEGMENT_ERRORS = {1: 'a NULL pointer', 2: 'H, W and C must be >= 1', 3: '1 <= K <= DMF_KMAX', 4: 'the segment size must be 4..32',
                   5: 'elem_bytes must be 2 or 4', 6: 'pitch < W', 7: 'an output overlaps an input or another output',
                   8: 'a misaligned scene or workspace, or a grid beyond 32 bits', 9: 'a launch failed',
                   10: 'the compactness is not a finite number >= 0', 11: 'the vote mode is not mean or majority',
                   12: 'the workspace is too small'}


def segment_grid(H, W, size):
    """-> (gh, gw): the cells of an H x W scene at segment size `size` (4..32); Kc = gh gw clusters."""
    if isinstance(size, bool) or not isinstance(size, int) or not SEG_SMIN <= size <= SEG_SMAX:
        raise DmfError('the segment size %r is not a whole number in %d..%d' % (size, SEG_SMIN, SEG_SMAX))
    return (H + size - 1) // size, (W + size - 1) // size


def _segment_scene(entry, scene, H, W, size):
    """The scene arguments of the slic entry points -> (gh, gw, C, (ptr, elem_bytes, pitch, H, W, C, size))."""
    gh, gw = segment_grid(H, W, size)
    _resident_scene(entry, scene)
    if H < 1 or W < 1 or H > scene.shape[0] or W > scene.shape[1]:
        raise DmfError('%s: %d x %d pixels asked of a scene of %d x %d' % (entry, H, W, scene.shape[0], scene.shape[1]))
    Cn = scene.shape[2]
    return gh, gw, Cn, (_ptr(scene), scene.element_size(), scene.shape[1], H, W, Cn, size)


def _segment_tensor(entry, t, dtype, shape, name, device):
    _dev(t, dtype, name)
    if tuple(t.shape) != tuple(shape) or t.device != device:
        raise DmfError('%s: %s must be %s on the scene\'s device' % (entry, name, list(shape)))


def slic_workspace_bytes(H, W, Cn, size):
    n = _lib.dmf_slic_workspace_bytes(H, W, Cn, size)
    if n < 0:
        raise DmfError('dmf_slic_workspace_bytes: H, W, C >= 1 and a segment size in 4..32')
    return n


def slic_init(scene, H, W, size, centres):
    """centres [Kc, C + 2] float32 <- the spectrum and the position of the pixel in the middle of every cell of the leading
    [H, W] pixels of the resident scene [>= H, pitch >= W, C] (dmf_slic_init)."""
    gh, gw, Cn, args = _segment_scene('slic_init', scene, H, W, size)
    _segment_tensor('slic_init', centres, torch.float32, (gh * gw, Cn + 2), 'centres', scene.device)
    _code_check(_SEGMENT_ERRORS, 'dmf_slic_init', _lib.dmf_slic_init(*args, _ptr(centres), _stream()))


def slic_assign(scene, H, W, size, compactness, centres, seg):
    """seg [H, W] int32 <- for every pixel the candidate cluster with the smallest D = d2 + (compactness / size)^2 |x - centre|^2,
    the first slot on equality (dmf_slic_assign)."""
    gh, gw, Cn, args = _segment_scene('slic_assign', scene, H, W, size)
    _segment_tensor('slic_assign', centres, torch.float32, (gh * gw, Cn + 2), 'centres', scene.device)
    _segment_tensor('slic_assign', seg, torch.int32, (H, W), 'seg', scene.device)
    if not (compactness >= 0 and compactness < float('inf')):
        raise DmfError('slic_assign: compactness = %r is not a finite number >= 0' % (compactness,))
    _code_check(_SEGMENT_ERRORS, 'dmf_slic_assign', _lib.dmf_slic_assign(*args, float(compactness), _ptr(centres), _ptr(seg), _stream()))


def slic_update(scene, H, W, size, seg, centres, counts, workspace):
    """centres [Kc, C + 2], counts [Kc] int32 <- the mean spectrum and position, and the number, of every cluster's members
    (the pixels of its 3 x 3 cells with seg == k); a cluster without a member keeps its row (dmf_slic_update).  `workspace`:
    a uint8 tensor of slic_workspace_bytes(H, W, C, size) bytes."""
    gh, gw, Cn, args = _segment_scene('slic_update', scene, H, W, size)
    _segment_tensor('slic_update', centres, torch.float32, (gh * gw, Cn + 2), 'centres', scene.device)
    _segment_tensor('slic_update', seg, torch.int32, (H, W), 'seg', scene.device)
    _segment_tensor('slic_update', counts, torch.int32, (gh * gw,), 'counts', scene.device)
    _dev(workspace, torch.uint8, 'workspace')
    _code_check(_SEGMENT_ERRORS, 'dmf_slic_update',
                _lib.dmf_slic_update(*args, _ptr(seg), _ptr(centres), _ptr(counts), _ptr(workspace), workspace.numel(), _stream()))


def segment_vote(prob, mask, seg, size, mode, segprob, segcount, label_map, prob_out=None):
    """segprob [Kc, K], segcount [Kc] <- the mean probabilities (mode 'mean') or the class counts ('majority') of every segment's
    masked members; label_map [H, W] int32 <- at every masked pixel the first maximal class of its segment's row, the other cells
    untouched; prob_out (optional) [H, W, K] <- that row, zeros where mask is 0 (dmf_segment_vote)."""
    if mode not in VOTE_MODES:
        raise DmfError('segment_vote: the mode %r is not mean or majority' % (mode,))
    _dev(prob, torch.float32, 'prob'); _dev(mask, torch.uint8, 'mask'); _dev(seg, torch.int32, 'seg')
    if prob.dim() != 3 or tuple(mask.shape) != tuple(prob.shape[:2]) or tuple(seg.shape) != tuple(prob.shape[:2]):
        raise DmfError('segment_vote wants prob [H, W, K] with mask and seg [H, W]')
    H, W, K = prob.shape
    gh, gw = segment_grid(H, W, size)
    _segment_tensor('segment_vote', segprob, torch.float32, (gh * gw, K), 'segprob', prob.device)
    _segment_tensor('segment_vote', segcount, torch.int32, (gh * gw,), 'segcount', prob.device)
    _segment_tensor('segment_vote', label_map, torch.int32, (H, W), 'label_map', prob.device)
    if prob_out is not None:
        _segment_tensor('segment_vote', prob_out, torch.float32, (H, W, K), 'prob_out', prob.device)
    if mask.device != prob.device or seg.device != prob.device:
        raise DmfError('segment_vote: all tensors must live on one device')
    _code_check(_SEGMENT_ERRORS, 'dmf_segment_vote', _lib.dmf_segment_vote(
        _ptr(prob), _ptr(mask), _ptr(seg), H, W, K, size, VOTE_MODES[mode], _ptr(segprob), _ptr(segcount), _ptr(label_map), _ptr(prob_out),
        _stream()))


# return codes of the entry points of csrc/dmf_regions.hip, which report by code (include/dmf.h)
REGION_PIXELS_MAX, REGION_VOTE_PIXELS_MAX = 1 << 31, 1 << 27      # DMF_REGION_PIXELS_MAX, DMF_REGION_VOTE_PIXELS_MAX
_REGION_ERRORS = {1: 'a NULL pointer', 2: 'H, W and R must be >= 1 and R <= H W', 3: '1 <= K <= DMF_KMAX',
                  7: 'an output or the workspace overlaps an input or another output', 8: 'a misaligned pointer, or a grid beyond 32 bits',
                  9: 'a launch failed', 11: 'the vote mode is not mean or majority', 12: 'the workspace is too small',
                  13: 'too many pixels: H W < 2^31 for components and merge, < 2^27 for the vote', 14: 'min_size must be >= 1',
                  15: 'n_labels must be >= 0'}


def _whole(entry, name, v, least):
    if isinstance(v, bool) or not isinstance(v, int) or v < least or v >= 1 << 31:
        raise DmfError('%s: %s = %r is not a whole number >= %d' % (entry, name, v, least))
    return v


def _labels_preamble(entry, labels, n_labels, min_size):
    """What the merges ask of labels, n_labels and min_size -> (H, W)."""
    _dev(labels, torch.int32, 'labels')
    if labels.dim() != 2:
        raise DmfError('%s wants labels [H, W]' % entry)
    _whole(entry, 'n_labels', n_labels, 0); _whole(entry, 'min_size', min_size, 1)
    return labels.shape


def region_workspace_bytes(H, W, n_labels=0):
    n = _lib.dmf_region_workspace_bytes(H, W, n_labels)
    if n < 0:
        raise DmfError('dmf_region_workspace_bytes: H, W >= 1, n_labels >= 0 and H W < 2^31')
    return n


def region_vote_workspace_bytes(R, K):
    n = _lib.dmf_region_vote_workspace_bytes(R, K)
    if n < 0:
        raise DmfError('dmf_region_vote_workspace_bytes: R >= 1 and 1 <= K <= DMF_KMAX')
    return n


def label_components(labels, comp, workspace):
    """comp [H, W] int32 <- for every pixel the smallest raster index of its 4-connected component of equal values of
    labels [H, W] int32 (dmf_label_components).  `workspace`: a uint8 tensor of region_workspace_bytes(H, W) bytes."""
    _dev(labels, torch.int32, 'labels')
    if labels.dim() != 2:
        raise DmfError('label_components wants labels [H, W]')
    H, W = labels.shape
    _segment_tensor('label_components', comp, torch.int32, (H, W), 'comp', labels.device)
    _dev(workspace, torch.uint8, 'workspace')
    _code_check(_REGION_ERRORS, 'dmf_label_components',
                _lib.dmf_label_components(_ptr(labels), H, W, _ptr(comp), _ptr(workspace), workspace.numel(), _stream()))


def region_merge(labels, comp, n_labels, min_size, region, region_size, stats, workspace):
    """region [H, W] int32 <- the dense id of every pixel's region: its component, or for a fragment (smaller than min_size, not
    the main component of a label in 0..n_labels - 1, not at pixel 0) the end of the chain of components before it; region_size
    [H W] int32 <- the regions' pixel counts in the first R cells, 0 in the others; stats [4] int32 <- R, components, fragments
    absorbed, 0 (dmf_region_merge).  `workspace`: a uint8 tensor of region_workspace_bytes(H, W, n_labels) bytes."""
    H, W = _labels_preamble('region_merge', labels, n_labels, min_size)
    _segment_tensor('region_merge', comp, torch.int32, (H, W), 'comp', labels.device)
    _segment_tensor('region_merge', region, torch.int32, (H, W), 'region', labels.device)
    _segment_tensor('region_merge', region_size, torch.int32, (H * W,), 'region_size', labels.device)
    _segment_tensor('region_merge', stats, torch.int32, (4,), 'stats', labels.device)
    _dev(workspace, torch.uint8, 'workspace')
    _code_check(_REGION_ERRORS, 'dmf_region_merge', _lib.dmf_region_merge(
        _ptr(labels), _ptr(comp), H, W, n_labels, min_size, _ptr(region), _ptr(region_size), _ptr(stats), _ptr(workspace), workspace.numel(),
        _stream()))


def region_vote(prob, mask, region, R, mode, regprob, regcount, label_map, workspace, prob_out=None):
    """regprob [R, K], regcount [R] <- the mean probabilities in exact fixed point (mode 'mean') or the class counts ('majority') of
    the masked members of every region 0..R - 1 of region [H, W] int32; label_map [H, W] int32 <- at every masked pixel the first
    maximal class of its region's row, the other cells untouched; prob_out (optional) [H, W, K] <- that row, zeros where mask is 0
    (dmf_region_vote).  `workspace`: a uint8 tensor of region_vote_workspace_bytes(R, K) bytes."""
    if mode not in VOTE_MODES:
        raise DmfError('region_vote: the mode %r is not mean or majority' % (mode,))
    _dev(prob, torch.float32, 'prob'); _dev(mask, torch.uint8, 'mask'); _dev(region, torch.int32, 'region')
    if prob.dim() != 3 or tuple(mask.shape) != tuple(prob.shape[:2]) or tuple(region.shape) != tuple(prob.shape[:2]):
        raise DmfError('region_vote wants prob [H, W, K] with mask and region [H, W]')
    H, W, K = prob.shape
    _whole('region_vote', 'R', R, 1)
    _segment_tensor('region_vote', regprob, torch.float32, (R, K), 'regprob', prob.device)
    _segment_tensor('region_vote', regcount, torch.int32, (R,), 'regcount', prob.device)
    _segment_tensor('region_vote', label_map, torch.int32, (H, W), 'label_map', prob.device)
    if prob_out is not None:
        _segment_tensor('region_vote', prob_out, torch.float32, (H, W, K), 'prob_out', prob.device)
    _dev(workspace, torch.uint8, 'workspace')
    if mask.device != prob.device or region.device != prob.device or workspace.device != prob.device:
        raise DmfError('region_vote: all tensors must live on one device')
    _code_check(_REGION_ERRORS, 'dmf_region_vote', _lib.dmf_region_vote(
        _ptr(prob), _ptr(mask), _ptr(region), H, W, K, R, VOTE_MODES[mode], _ptr(regprob), _ptr(regcount), _ptr(label_map), _ptr(prob_out),
        _ptr(workspace), workspace.numel(), _stream()))


# the entry points of csrc/dmf_region_graph.hip, which report by code (include/dmf.h)
_REGION_GRAPH_ERRORS = dict(_REGION_ERRORS)
_REGION_GRAPH_ERRORS.update({2: 'H, W and C must be >= 1', 5: 'elem_bytes must be 2 or 4', 6: 'pitch_pixels < W', 13: 'too many pixels: H W < 2^27',
                             16: 'components outside 1..H W, or fragments outside 0..components - 1'})


def region_graph_workspace_bytes(H, W, Cn=1, n_labels=0, components=1):
    """The bytes dmf_region_graph_merge needs for `components` components of a C-band scene; with Cn = 1 and components = 1 the
    bytes of region_graph_count."""
    n = _lib.dmf_region_graph_workspace_bytes(H, W, Cn, n_labels, components)
    if n < 0:
        raise DmfError('dmf_region_graph_workspace_bytes: H, W, C >= 1, n_labels >= 0, H W < 2^27 and 1 <= components <= H W')
    return n


def region_graph_count(labels, comp, n_labels, min_size, counts, workspace):
    """counts [2] int32 <- the number of components of comp [H, W] (as label_components leaves it) and the number of fragments
    among them: smaller than min_size, not the main component of a label in 0..n_labels - 1, not at pixel 0
    (dmf_region_graph_count).  `workspace`: a uint8 tensor of region_graph_workspace_bytes(H, W, 1, n_labels, 1) bytes."""
    H, W = _labels_preamble('region_graph_count', labels, n_labels, min_size)
    _segment_tensor('region_graph_count', comp, torch.int32, (H, W), 'comp', labels.device)
    _segment_tensor('region_graph_count', counts, torch.int32, (2,), 'counts', labels.device)
    _dev(workspace, torch.uint8, 'workspace')
    _code_check(_REGION_GRAPH_ERRORS, 'dmf_region_graph_count', _lib.dmf_region_graph_count(
        _ptr(labels), _ptr(comp), H, W, n_labels, min_size, _ptr(counts), _ptr(workspace), workspace.numel(), _stream()))


def region_graph_merge(labels, comp, scene, n_labels, min_size, components, fragments, region, region_size, stats, workspace):
    """region [H, W] int32 <- the dense id of every pixel's region after the spectrum-aware merge: every fragment joins the adjacent
    group with the nearest mean spectrum of the leading [H, W] pixels of scene [>= H, pitch >= W, C] (fp32 or fp16), groups of
    fragments grow and one that reaches min_size becomes a region; region_size [H W] int32 <- the regions' pixel counts in the
    first R cells, 0 in the others; stats [4] int32 <- R, components, components - R, rounds (dmf_region_graph_merge).
    `components` and `fragments` are what region_graph_count left; `workspace`: a uint8 tensor of
    region_graph_workspace_bytes(H, W, C, n_labels, components) bytes."""
    H, W = _labels_preamble('region_graph_merge', labels, n_labels, min_size)
    _resident_scene('region_graph_merge', scene)
    if H > scene.shape[0] or W > scene.shape[1] or scene.device != labels.device:
        raise DmfError('region_graph_merge: %d x %d pixels asked of a scene of %d x %d on %s' % (H, W, scene.shape[0], scene.shape[1], scene.device))
    _whole('region_graph_merge', 'components', components, 1); _whole('region_graph_merge', 'fragments', fragments, 0)
    _segment_tensor('region_graph_merge', comp, torch.int32, (H, W), 'comp', labels.device)
    _segment_tensor('region_graph_merge', region, torch.int32, (H, W), 'region', labels.device)
    _segment_tensor('region_graph_merge', region_size, torch.int32, (H * W,), 'region_size', labels.device)
    _segment_tensor('region_graph_merge', stats, torch.int32, (4,), 'stats', labels.device)
    _dev(workspace, torch.uint8, 'workspace')
    _code_check(_REGION_GRAPH_ERRORS, 'dmf_region_graph_merge', _lib.dmf_region_graph_merge(
        _ptr(labels), _ptr(comp), _ptr(scene), scene.element_size(), scene.shape[1], H, W, scene.shape[2], n_labels, min_size, components,
        fragments, _ptr(region), _ptr(region_size), _ptr(stats), _ptr(workspace), workspace.numel(), _stream()))


# return codes of the two entry points of csrc/dmf_pca.hip, which report by code (include/dmf.h)
PCA_RUN = 256                                   # DMF_PCA_RUN: pixels one fp32 accumulator of the covariance covers
_PCA_ERRORS = {1: 'a NULL pointer', 2: 'N must be >= 2 (project: >= 0)', 3: '1 <= C <= 512', 4: '1 <= K <= min(C, 64)', 5: 'pitch < C',
               6: 'a misaligned pointer', 8: 'N * pitch beyond 64-bit byte offsets, or a grid beyond 32 bits', 9: 'a launch failed'}


def _pixels(x, name):
    """(N, C, pitch) of x: a [N, C] float32 GPU tensor whose rows are `pitch` >= C floats apart (a column slice of a
    contiguous tensor passes as it is)."""
    if not (x.is_cuda and x.dtype == torch.float32):
        raise DmfError('%s must be a %s tensor on the GPU' % (name, torch.float32))
    if x.dim() != 2 or x.shape[1] < 1 or x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        raise DmfError('%s must be [N, C] float32 with unit band stride and a row pitch >= C' % name)
    return x.shape[0], x.shape[1], x.stride(0) if x.shape[0] > 1 else x.shape[1]


def band_moments_workspace_bytes(N, C):
    n = _lib.dmf_band_moments_workspace_bytes(N, C)
    if n < 0:
        raise DmfError('dmf_band_moments: N >= 2 and 1 <= C <= 512, got N = %d, C = %d' % (N, C))
    return n


def band_moments(x, mean, cov, ws=None):
    """mean [C] / cov [C, C] float64 <- the band means and the sample covariance of the pixels x [N, C] float32 (rows `pitch`
    floats apart), the products in fp32 over runs of PCA_RUN pixels, the sums in double (dmf_band_moments).  ws: a uint8
    tensor of band_moments_workspace_bytes(N, C) bytes, allocated here when None."""
    N, C_, pitch = _pixels(x, 'x')
    _dev(mean, torch.float64, 'mean'); _dev(cov, torch.float64, 'cov')
    if tuple(mean.shape) != (C_,) or tuple(cov.shape) != (C_, C_) or mean.device != x.device or cov.device != x.device:
        raise DmfError('band_moments wants mean [%d] and cov [%d, %d] float64 on x\'s device' % (C_, C_, C_))
    need = band_moments_workspace_bytes(N, C_)
    if ws is None:
        ws = torch.empty(need // 8, dtype=torch.float64, device=x.device)
    elif not ws.is_cuda or ws.device != x.device or ws.numel() * ws.element_size() < need:
        raise DmfError('band_moments: the workspace needs %d bytes on x\'s device' % need)
    _code_check(_PCA_ERRORS, 'dmf_band_moments', _lib.dmf_band_moments(_ptr(x), N, C_, pitch, _ptr(mean), _ptr(cov), _ptr(ws), _stream()))


NOISE_DIRECTIONS = {'horizontal': 0, 'vertical': 1}
_NOISE_ERRORS = {**_PCA_ERRORS, 2: 'no pixel has the neighbour (a one-column scene horizontally, a one-row scene vertically)',
                 7: 'the direction must be 0 (horizontal) or 1 (vertical)'}


def band_noise_workspace_bytes(H, W, C):
    n = _lib.dmf_band_noise_workspace_bytes(H, W, C)
    if n < 0:
        raise DmfError('dmf_band_noise_moments: H, W >= 1, H W >= 2 and 1 <= C <= 512, got H = %d, W = %d, C = %d' % (H, W, C))
    return n


def band_noise_moments(x, H, W, ncov, direction, ws=None):
    """ncov [C, C] float64 <- sum_p e_p e_p^T / (2 M) of the scene x, [H, W, C] or flat [H W, C] float32 (pixels `pitch` floats
    apart, rows W pitch), with e_p = x[p] - x[p + s] in fp32 for the pixels that have the neighbour (direction 0 / 'horizontal':
    s = 1, 1 / 'vertical': s = W) and 0 for the others, M of them (dmf_band_noise_moments: the covariance's arithmetic).  ws: a
    tensor of band_noise_workspace_bytes(H, W, C) bytes, allocated here when None."""
    direction = NOISE_DIRECTIONS.get(direction, direction)
    if x.dim() == 3:
        if tuple(x.shape[:2]) != (H, W) or (H > 1 and W > 1 and x.stride(0) != W * x.stride(1)):
            raise DmfError('band_noise_moments wants x [H, W, C] with rows W pixels apart, or flat [H W, C]')
        x = x.as_strided((H * W, x.shape[2]), (x.stride(1) if W > 1 else x.stride(0), x.stride(2)), x.storage_offset())
    N, C_, pitch = _pixels(x, 'x')
    if N != H * W:
        raise DmfError('band_noise_moments: x has %d pixels, H W = %d' % (N, H * W))
    _dev(ncov, torch.float64, 'ncov')
    if tuple(ncov.shape) != (C_, C_) or ncov.device != x.device:
        raise DmfError('band_noise_moments wants ncov [%d, %d] float64 on x\'s device' % (C_, C_))
    need = band_noise_workspace_bytes(H, W, C_)
    if ws is None:
        ws = torch.empty(need // 8, dtype=torch.float64, device=x.device)
    elif not ws.is_cuda or ws.device != x.device or ws.numel() * ws.element_size() < need:
        raise DmfError('band_noise_moments: the workspace needs %d bytes on x\'s device' % need)
    _code_check(_NOISE_ERRORS, 'dmf_band_noise_moments',
                _lib.dmf_band_noise_moments(_ptr(x), H, W, C_, pitch, int(direction), _ptr(ncov), _ptr(ws), _stream()))


def band_project(x, mean, basis, y):
    """y [N, K] float32 <- (x - float32(mean)) basis for the pixels x [N, C] float32 (rows `pitch` floats apart), mean [C]
    float64 and basis [C, K] float32, K <= min(C, 64), accumulated in fp32 over the bands in ascending order
    (dmf_band_project)."""
    N, C_, pitch = _pixels(x, 'x')
    _dev(mean, torch.float64, 'mean'); _dev(basis, torch.float32, 'basis'); _dev(y, torch.float32, 'y')
    if tuple(mean.shape) != (C_,) or basis.dim() != 2 or basis.shape[0] != C_ or tuple(y.shape) != (N, basis.shape[1]):
        raise DmfError('band_project wants mean [C], basis [C, K] and y [N, K] for x [N, C]')
    if len({t.device for t in (x, mean, basis, y)}) != 1:
        raise DmfError('band_project: all tensors must live on one device')
    if N == 0:                                  # (an empty tensor has a null data pointer)
        return
    _code_check(_PCA_ERRORS, 'dmf_band_project',
                _lib.dmf_band_project(_ptr(x), N, C_, pitch, _ptr(mean), _ptr(basis), basis.shape[1], _ptr(y), _stream()))


# the entry points of csrc/dmf_morph.hip, which report by code (include/dmf.h)
MORPH_TILE, MORPH_BATCH = 32, 8                # DMF_MORPH_TILE, DMF_MORPH_BATCH
_MORPH_ERRORS = {1: 'a NULL pointer', 2: 'H and W must be >= 1 and H W < 2^31', 3: '1 <= K <= 64 and 1 <= P <= K (reconstruct: the plane counts)',
                 4: '1..8 strictly increasing radii in 1..32', 5: 'pitch < K', 6: 'a misaligned pointer', 7: 'two plane sets are the same memory',
                 8: 'a grid beyond 32 bits, or H W pitch beyond 64-bit byte offsets', 9: 'a launch failed', 10: 'first_round or rounds out of range'}


def morph_workspace_bytes(H, W, P, n):
    nbytes = _lib.dmf_morph_workspace_bytes(H, W, P, n)
    if nbytes < 0:
        raise DmfError('dmf_morph_workspace_bytes: H, W >= 1, H W < 2^31, 1 <= P <= 64, 1 <= n <= 8, got %r' % ((H, W, P, n),))
    return nbytes


def morph_state_bytes(H, W, planes):
    nbytes = _lib.dmf_morph_state_bytes(H, W, planes)
    if nbytes < 0:
        raise DmfError('dmf_morph_state_bytes: H, W >= 1, H W < 2^31, 1 <= planes <= 1024, got %r' % ((H, W, planes),))
    return nbytes


def morph_carve(ws, H, W, P, n):
    """(mask [2 P, H, W], X [2 n P, H, W], Y [2 n P, H, W] float32, state uint8) as views of the uint8 workspace tensor `ws` of at
    least morph_workspace_bytes(H, W, P, n) bytes, in the order include/dmf.h states."""
    need = morph_workspace_bytes(H, W, P, n)
    if not (ws.is_cuda and ws.dtype == torch.uint8 and ws.dim() == 1 and ws.is_contiguous()) or ws.numel() < need or ws.data_ptr() % 4:
        raise DmfError('morph_carve: the workspace must be a 4-byte aligned uint8 GPU tensor of at least %d bytes' % need)
    L, plane = 2 * n * P, 4 * H * W
    cuts = [0, 2 * P * plane, (2 * P + L) * plane, (2 * P + 2 * L) * plane, need]
    mask, X, Y = (ws[a:b].view(torch.float32).view(-1, H, W) for a, b in zip(cuts[:3], cuts[1:4]))
    return mask, X, Y, ws[cuts[3]:cuts[4]]


def _morph_scores(entry, scores):
    """(H, W, K, pitch) of scores: a [H, W, K] float32 GPU tensor, pixels `pitch` >= K floats apart, rows W pitch."""
    if not (scores.is_cuda and scores.dtype == torch.float32 and scores.dim() == 3 and scores.numel() > 0 and scores.stride(2) == 1):
        raise DmfError('%s: the scores must be a [H, W, K] float32 GPU tensor with unit band stride' % entry)
    H, W, K = scores.shape
    pitch = scores.stride(1) if W > 1 else (scores.stride(0) if H > 1 else K)
    if pitch < K or (H > 1 and W > 1 and scores.stride(0) != W * pitch):
        raise DmfError('%s: the pixels of the scores must be one pitch >= K apart, row after row' % entry)
    return H, W, K, pitch


def _morph_planes(entry, t, count, H, W, name, device):
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (count, H, W) and t.device == device):
        raise DmfError('%s: %s must be a contiguous [%d, %d, %d] float32 tensor on %s' % (entry, name, count, H, W, device))


def morph_markers(scores, P, radii, mask, markers, scratch):
    """mask [2 P, H, W] <- the first P components of scores [H, W, K] and their negatives, canonicalised; markers [2 n P, H, W] <-
    the erosion of its mask plane at each radius (dmf_morph_markers; `scratch`, as large as markers, holds the row pass)."""
    H, W, K, pitch = _morph_scores('morph_markers', scores)
    radii = [int(r) for r in radii]
    n = len(radii)
    _morph_planes('morph_markers', mask, 2 * P, H, W, 'mask', scores.device)
    _morph_planes('morph_markers', markers, 2 * n * P, H, W, 'markers', scores.device)
    _morph_planes('morph_markers', scratch, 2 * n * P, H, W, 'scratch', scores.device)
    _code_check(_MORPH_ERRORS, 'dmf_morph_markers', _lib.dmf_morph_markers(
        _ptr(scores), H, W, K, pitch, P, (C.c_int32 * max(n, 1))(*radii), n, _ptr(mask), _ptr(markers), _ptr(scratch), _stream()))


def morph_reconstruct(mask, X, Y, per_mask, first_round, rounds, state):
    """Enqueues the rounds first_round .. first_round + rounds - 1 of the reconstruction by dilation of the planes X [L, H, W]
    under mask [L / per_mask, H, W] (dmf_morph_reconstruct); reads nothing.  state: a uint8 tensor of morph_state_bytes(H, W, L)."""
    if not (X.is_cuda and X.dim() == 3):
        raise DmfError('morph_reconstruct: X must be a [L, H, W] float32 GPU tensor')
    L, H, W = X.shape
    _morph_planes('morph_reconstruct', X, L, H, W, 'X', X.device)
    _morph_planes('morph_reconstruct', Y, L, H, W, 'Y', X.device)
    _morph_planes('morph_reconstruct', mask, L // max(per_mask, 1), H, W, 'mask', X.device)
    if not (state.is_cuda and state.dtype == torch.uint8 and state.is_contiguous() and state.device == X.device
            and state.numel() >= morph_state_bytes(H, W, L)):
        raise DmfError('morph_reconstruct: the state needs %d bytes on X\'s device' % morph_state_bytes(H, W, L))
    _code_check(_MORPH_ERRORS, 'dmf_morph_reconstruct', _lib.dmf_morph_reconstruct(
        _ptr(mask), _ptr(X), _ptr(Y), H, W, L, per_mask, first_round, rounds, _ptr(state), _stream()))


def morph_reconstruct_run(mask, X, Y, per_mask, state):
    """The whole reconstruction: batches of MORPH_BATCH rounds, the batch's counters read once after each, until a round changed
    no tile -> the rounds that ran in each batch (the last entry ends with the round that found nothing to do).  X and Y are equal
    afterwards.  More than H W rounds is an internal error: a value moves at least one pixel per round."""
    L, H, W = X.shape
    batches, k = [], 0
    while True:
        morph_reconstruct(mask, X, Y, per_mask, k, MORPH_BATCH, state)
        counts = state[:8 * MORPH_BATCH].view(torch.int32)[(k % (2 * MORPH_BATCH)):(k % (2 * MORPH_BATCH)) + MORPH_BATCH].tolist()
        if 0 in counts:
            batches.append(counts.index(0) + 1)
            return batches
        batches.append(MORPH_BATCH)
        k += MORPH_BATCH
        if k > H * W:
            raise DmfError('morph_reconstruct_run: no fixed point after %d rounds of a %d x %d image (internal error)' % (k, H, W))


def morph_stack(scores, P, n, mask, planes, out):
    """out [H, W, K + 2 n P] float32 <- the profile in the order include/dmf.h states, from the reconstructed planes
    (dmf_morph_stack)."""
    H, W, K, pitch = _morph_scores('morph_stack', scores)
    _morph_planes('morph_stack', mask, 2 * P, H, W, 'mask', scores.device)
    _morph_planes('morph_stack', planes, 2 * n * P, H, W, 'planes', scores.device)
    if not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (H, W, K + 2 * n * P)
            and out.device == scores.device):
        raise DmfError('morph_stack: out must be a contiguous [%d, %d, %d] float32 tensor on the scores\' device' % (H, W, K + 2 * n * P))
    _code_check(_MORPH_ERRORS, 'dmf_morph_stack', _lib.dmf_morph_stack(
        _ptr(scores), H, W, K, pitch, P, n, _ptr(mask), _ptr(planes), _ptr(out), _stream()))


# the entry points of csrc/dmf_attr.hip, which report by code (include/dmf.h)
ATTR_BATCH_MAX, ATTR_LEVELS_MAX, ATTR_AREAS_MAX = 16, 256, 8     # DMF_ATTR_BATCH_MAX, DMF_ATTR_LEVELS_MAX, DMF_ATTR_NMAX
_ATTR_ERRORS = {1: 'a NULL pointer', 2: 'H and W must be >= 1 and H W < 2^31', 3: '1 <= K <= 64 and 1 <= P <= K (area_levels: 1 <= P <= 64)',
                4: '1..8 strictly increasing areas >= 1', 5: 'pitch < K', 6: 'a misaligned pointer', 7: 'an output overlaps an input or another output',
                8: 'a grid beyond 32 bits, or H W pitch beyond 64-bit byte offsets', 9: 'a launch failed',
                10: 'first_level, levels or T out of range', 11: 'L outside 2..256', 12: 'the workspace is too small',
                13: 'stds with H W > 2^22', 14: '0..7 strictly increasing diagonals >= 1 and stds in 1..L - 1, at most 8 thresholds in all'}
ATTR_STD_PIXELS_MAX = 1 << 22                                   # DMF_ATTR_STD_PIXELS_MAX


def attr_workspace_bytes(H, W, P, n, T):
    nbytes = _lib.dmf_attr_workspace_bytes(H, W, P, n, T)
    if nbytes < 0:
        raise DmfError('dmf_attr_workspace_bytes: H, W >= 1, H W < 2^31, 1 <= P <= 64, 1 <= n <= 8, 1 <= T <= 16, got %r' % ((H, W, P, n, T),))
    return nbytes


def attr_carve(ws, H, W, P, n, T):
    """(keys uint8 view of the 2 P uint32 min / max keys, parent [2 P, T, H W] int32, size [2 P, T, H W] int32) as views of the
    uint8 workspace tensor `ws` of at least attr_workspace_bytes(H, W, P, n, T) bytes, in the order include/dmf.h states."""
    need = attr_workspace_bytes(H, W, P, n, T)
    if not (ws.is_cuda and ws.dtype == torch.uint8 and ws.dim() == 1 and ws.is_contiguous()) or ws.numel() < need or ws.data_ptr() % 16:
        raise DmfError('attr_carve: the workspace must be a 16-byte aligned uint8 GPU tensor of at least %d bytes' % need)
    keys = (8 * P + 15) // 16 * 16
    planes = (2 * P * T * H * W * 4 + 15) // 16 * 16
    cells = 2 * P * T * H * W * 4
    parent, size = (ws[a:a + cells].view(torch.int32).view(2 * P, T, H * W) for a in (keys, keys + planes))
    return ws[:keys], parent, size


def _attr_workspace(entry, ws, need, device):
    if not (ws.is_cuda and ws.dtype == torch.uint8 and ws.dim() == 1 and ws.is_contiguous() and ws.device == device and ws.numel() >= need):
        raise DmfError('%s: the workspace must be a uint8 tensor of at least %d bytes on %s' % (entry, need, device))


def _attr_bytes(entry, t, shape, name, device):
    if not (t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and tuple(t.shape) == tuple(shape) and t.device == device):
        raise DmfError('%s: %s must be a contiguous %s uint8 tensor on %s' % (entry, name, list(shape), device))


def attr_quantise(scores, P, L, q, rng, ws):
    """rng [P, 2] float32 <- the exact (min, max) of the first P components of scores [H, W, K]; q [2 P, H, W] uint8 <- their
    quantised planes at L levels and the complements L - 1 - q (dmf_attr_quantise).  ws: a uint8 tensor that holds at least the
    2 P keys at the head of the workspace (16-byte aligned)."""
    H, W, K, pitch = _morph_scores('attr_quantise', scores)
    _attr_bytes('attr_quantise', q, (2 * P, H, W), 'q', scores.device)
    if not (rng.is_cuda and rng.dtype == torch.float32 and rng.is_contiguous() and tuple(rng.shape) == (P, 2) and rng.device == scores.device):
        raise DmfError('attr_quantise: range must be a contiguous [%d, 2] float32 tensor on the scores\' device' % P)
    _attr_workspace('attr_quantise', ws, (8 * max(P, 1) + 15) // 16 * 16, scores.device)
    _code_check(_ATTR_ERRORS, 'dmf_attr_quantise', _lib.dmf_attr_quantise(
        _ptr(scores), H, W, K, pitch, P, L, _ptr(q), _ptr(rng), _ptr(ws), ws.numel(), _stream()))


def attr_area_levels(q, areas, L, first_level, levels, count, ws, T):
    """Enqueues the levels first_level .. first_level + levels - 1 of every plane of q [2 P, H, W] (dmf_attr_area_levels): count
    [2 P, n, H, W] uint8 is stored by the call with first_level 1 and added to by the later ones.  Reads nothing back."""
    if not (q.is_cuda and q.dim() == 3 and q.shape[0] % 2 == 0 and q.numel() > 0):
        raise DmfError('attr_area_levels: q must be a [2 P, H, W] uint8 GPU tensor')
    P2, H, W = q.shape
    areas = [int(a) for a in areas]
    n = len(areas)
    _attr_bytes('attr_area_levels', q, (P2, H, W), 'q', q.device)
    _attr_bytes('attr_area_levels', count, (P2, n, H, W), 'count', q.device)
    if not 1 <= T <= ATTR_BATCH_MAX:
        raise DmfError('attr_area_levels: %s' % _ATTR_ERRORS[10])
    if not 1 <= n <= ATTR_AREAS_MAX or not all(1 <= a < 2 ** 31 for a in areas):          # (what an int32 cannot carry to the check)
        raise DmfError('attr_area_levels: %s' % _ATTR_ERRORS[4])
    _attr_workspace('attr_area_levels', ws, attr_workspace_bytes(H, W, P2 // 2, n, T), q.device)
    _code_check(_ATTR_ERRORS, 'dmf_attr_area_levels', _lib.dmf_attr_area_levels(
        _ptr(q), H, W, P2 // 2, (C.c_int32 * n)(*areas), n, L, first_level, levels, T, _ptr(count), _ptr(ws), ws.numel(), _stream()))


def attr_area_run(q, areas, L, count, ws, T):
    """Every level 1 .. L - 1 in ascending batches of T: ceil((L - 1) / T) calls, nothing read back -> the number of calls."""
    calls = 0
    for first in range(1, L, T):
        attr_area_levels(q, areas, L, first, min(T, L - first), count, ws, T)
        calls += 1
    return calls


def attr_stack(scores, P, n, L, count, rng, out):
    """out [H, W, K + 2 n P] float32 <- the profile in the order include/dmf.h states, from count and range (dmf_attr_stack)."""
    H, W, K, pitch = _morph_scores('attr_stack', scores)
    _attr_bytes('attr_stack', count, (2 * P, n, H, W), 'count', scores.device)
    if not (rng.is_cuda and rng.dtype == torch.float32 and rng.is_contiguous() and tuple(rng.shape) == (P, 2) and rng.device == scores.device):
        raise DmfError('attr_stack: range must be a contiguous [%d, 2] float32 tensor on the scores\' device' % P)
    if not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (H, W, K + 2 * n * P)
            and out.device == scores.device):
        raise DmfError('attr_stack: out must be a contiguous [%d, %d, %d] float32 tensor on the scores\' device' % (H, W, K + 2 * n * P))
    _code_check(_ATTR_ERRORS, 'dmf_attr_stack', _lib.dmf_attr_stack(
        _ptr(scores), H, W, K, pitch, P, n, L, _ptr(count), _ptr(rng), _ptr(out), _stream()))


# several attributes over the same components: dmf_attr_multi_workspace_bytes / dmf_attr_multi_levels
def attr_multi_workspace_bytes(H, W, P, n_diag, n_std, T):
    nbytes = _lib.dmf_attr_multi_workspace_bytes(H, W, P, n_diag, n_std, T)
    if nbytes < 0:
        raise DmfError('dmf_attr_multi_workspace_bytes: H, W >= 1, H W < 2^31 (with stds: <= 2^22), 1 <= P <= 64, 0 <= n_diag, n_std and '
                       'n_diag + n_std <= 7, 1 <= T <= 16, got %r' % ((H, W, P, n_diag, n_std, T),))
    return nbytes


def attr_multi_carve(ws, H, W, P, n_diag, n_std, T):
    """dict of views of the uint8 workspace tensor `ws` of at least attr_multi_workspace_bytes(..) bytes, in the order include/dmf.h
    states: keys, parent, size as attr_carve gives them; xmin, xmax, ymin, ymax [2 P, T, H W] int32 where n_diag > 0; sum_q, sum_q2
    [2 P, T, H W] int64 (the bits of the uint64 cells) where n_std > 0.  A plane set that was not asked for has no entry."""
    need = attr_multi_workspace_bytes(H, W, P, n_diag, n_std, T)
    if not (ws.is_cuda and ws.dtype == torch.uint8 and ws.dim() == 1 and ws.is_contiguous()) or ws.numel() < need or ws.data_ptr() % 16:
        raise DmfError('attr_multi_carve: the workspace must be a 16-byte aligned uint8 GPU tensor of at least %d bytes' % need)
    keys, parent, size = attr_carve(ws, H, W, P, 1, T)
    views = dict(keys=keys, parent=parent, size=size)
    cells = 2 * P * T * H * W
    at = attr_workspace_bytes(H, W, P, 1, T)
    for names, dtype, width in ((('xmin', 'xmax', 'ymin', 'ymax') if n_diag else (), torch.int32, 4),
                                (('sum_q', 'sum_q2') if n_std else (), torch.int64, 8)):
        for name in names:
            views[name] = ws[at:at + cells * width].view(dtype).view(2 * P, T, H * W)
            at += (cells * width + 15) // 16 * 16
    assert at == need
    return views


def attr_multi_levels(q, thresholds, counts, L, first_level, levels, count, ws, T):
    """Enqueues the levels first_level .. first_level + levels - 1 of every plane of q [2 P, H, W] (dmf_attr_multi_levels).
    thresholds: areas ++ diagonals ++ stds; counts = (n_area, n_diag, n_std).  count [2 P, n, H, W] uint8 is stored by the call with
    first_level 1 and added to by the later ones.  Reads nothing back."""
    if not (q.is_cuda and q.dim() == 3 and q.shape[0] % 2 == 0 and q.numel() > 0):
        raise DmfError('attr_multi_levels: q must be a [2 P, H, W] uint8 GPU tensor')
    P2, H, W = q.shape
    thresholds = [int(t) for t in thresholds]
    na, nd, ns = (int(c) for c in counts)
    n = len(thresholds)
    if min(na, nd, ns) < 0 or na + nd + ns != n:
        raise DmfError('attr_multi_levels: the counts %r do not add up to the %d thresholds' % ((na, nd, ns), n))
    if not 1 <= na <= ATTR_AREAS_MAX or not all(1 <= a < 2 ** 31 for a in thresholds[:na]):
        raise DmfError('attr_multi_levels: %s' % _ATTR_ERRORS[4])
    if n > ATTR_AREAS_MAX or not all(1 <= t < 2 ** 31 for t in thresholds[na:]):          # (what an int32 cannot carry to the check)
        raise DmfError('attr_multi_levels: %s' % _ATTR_ERRORS[14])
    if ns and H * W > ATTR_STD_PIXELS_MAX:
        raise DmfError('attr_multi_levels: %s' % _ATTR_ERRORS[13])
    _attr_bytes('attr_multi_levels', q, (P2, H, W), 'q', q.device)
    _attr_bytes('attr_multi_levels', count, (P2, n, H, W), 'count', q.device)
    if not 1 <= T <= ATTR_BATCH_MAX:
        raise DmfError('attr_multi_levels: %s' % _ATTR_ERRORS[10])
    _attr_workspace('attr_multi_levels', ws, attr_multi_workspace_bytes(H, W, P2 // 2, nd, ns, T), q.device)
    _code_check(_ATTR_ERRORS, 'dmf_attr_multi_levels', _lib.dmf_attr_multi_levels(
        _ptr(q), H, W, P2 // 2, (C.c_int32 * n)(*thresholds), na, nd, ns, L, first_level, levels, T, _ptr(count), _ptr(ws), ws.numel(),
        _stream()))


def attr_multi_run(q, thresholds, counts, L, count, ws, T):
    """Every level 1 .. L - 1 in ascending batches of T: ceil((L - 1) / T) calls, nothing read back -> the number of calls."""
    calls = 0
    for first in range(1, L, T):
        attr_multi_levels(q, thresholds, counts, L, first, min(T, L - first), count, ws, T)
        calls += 1
    return calls
