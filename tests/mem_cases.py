"""Cases and helpers of tests/test_gpu_memory_discipline.py (checked on the host by tests/test_mem_cases_host.py): a launch reads
nothing that no launch wrote, and writes nothing outside the extents its arguments state.  No oracle: every assertion is
bit-equality of a launch with itself under other surroundings, or a check that canary bytes are intact.

FILLS: the byte fills a buffer holds at entry.  0xFF is a NaN in fp32, fp16 and bf16 and -1 as an int32.  0x47 is a large finite
value (0x47474747 = 5.1e4 in fp32, 0x4747 = 5.1e4 in bf16 and 7.3 in fp16): the kernels' ReLU (v_med3 / fmaxf) drops a NaN, so
a stale value that passes through a max would hide behind the NaN fill.  The second 0x00 run tells "depends on the fill" from
"not deterministic".

guarded(n, dtype, device, fill) -> (view, whole): `view`, n contiguous elements whose bytes are `fill`, lies in the middle of
one allocation `whole` (uint8) between two guards of GUARD_BYTES canary bytes — more than one slab row (at most 1,728 floats)
and more than one attention token map (16 KiB).  The body starts on a 256-byte boundary and the second guard follows its last
byte directly.  intact(whole, n, dtype) is true while both guards hold the canary; otherwise it is false and carries the first
and last damaged byte before the view (offsets < 0 from the view's first byte) and behind it (offsets >= 0 from its end).

Shapes (C, C2, P, S, K, width): the smallest rows of the kernel table that differ in structure —
  tiny1    8/1/5/1    five conv waves, G = 2
  tiny     8/1/5/4    aux at 4x: the lift conv's taps, aux rows by 16-byte pieces
  quatiny  4/1/5/1    G = 1
  qua      4/1/16/1   P = 16: all 16 lanes of a row group
  hsi      200/1/11/1 G = 10, F = 40
  hsi224   224/3/11/1 C2 = 3, F = 32: another slab padding
  pca32    32/1/11/1  the 32-band row of band reduction
  panms    4/1/16/4   (beside the scene only) P = 16 with the aux at 4x
Attention: tiny1 and hsi.  Batches: 1 (a single patch), 3 (fewer patches than waves), 255 and 257 (one workgroup gets a second
patch), 513 (a third patch: the double buffer is reused), 1025 (unit route only: a second round of NPB = 4 patches).  The large
rows (LARGE) take 3 and 257 only.  K is each row's usual count; tiny1 also takes 2 and 64 = KMAX.
"""
import torch

FILLS = (0x00, 0xFF, 0x47, 0x00)
GUARD_BYTES = 64 * 1024
CANARY = 0xA5
ALIGN = 256
KMAX, MAX_BLOCKS = 64, 256

SHAPES = {   # name: (C, C2, P, S, K, width)
    'tiny1': (8, 1, 5, 1, 5, 40),
    'tiny': (8, 1, 5, 4, 5, 40),
    'quatiny': (4, 1, 5, 1, 5, 40),
    'qua': (4, 1, 16, 1, 12, 40),
    'hsi': (200, 1, 11, 1, 17, 40),
    'hsi224': (224, 3, 11, 1, 17, 32),
    'pca32': (32, 1, 11, 1, 17, 40),
    'panms': (4, 1, 16, 4, 12, 40),               # beside the scene only: the reference's own data, aux at 4x
}
ROWS = tuple(n for n in SHAPES if n != 'panms')
LARGE = ('qua', 'hsi', 'hsi224', 'pca32')
QUA = ('quatiny', 'qua')                           # stage 2: the unit route's loss is dmf_qua_loss on 4 x bs rows
ATTN_SHAPES = ('tiny1', 'hsi')
BATCHES = (1, 3, 255, 257, 513)
UNIT_BATCHES = BATCHES + (1025,)
LARGE_BATCHES = (3, 257)
K_ENDS = (2, 64)                                   # on tiny1, batch 3
ATTN_BATCHES = (1, 3, 257, 513)
SHARED_WS_BATCHES = (513, 3, 257, 1)               # one workspace sized for the first, then the others in it
TAIL_N = (1, 255, 256, 257, 4097, 8009)            # optimiser launches
LOSS_BS, LOSS_K = (1, 255, 257), (2, 17, 64)
ROW_B, ROW_K = (1, 255, 257), (1, 17, 64)          # softmax_stats, prob_scatter, logits_mean, calib, confusion, labelmap
BAND_C = (3, 32, 200)                              # band moments on a 13 x 11 scene
BAND_SCENE = (13, 11)
PROJECT_C, PROJECT_K = (3, 200), (1, 32)
TEMP_N, TEMP_K = (1, 255, 257), 17
SCENE_H, SCENE_W = 23, 19                          # pixels a patch may start at (the padded scene is P - 1 larger)
PITCH_EXTRA = (1, 2, 3)                            # aux scene pitch mod 4, S = 4


def batches_of(name, unit=False):
    if name in LARGE:
        return LARGE_BATCHES
    return UNIT_BATCHES if unit else BATCHES


def patch_cases(unit=False):
    """(name, B, K) of the late-fusion launch sequences."""
    out = [(n, B, SHAPES[n][4]) for n in ROWS for B in batches_of(n, unit)]
    return out + [('tiny1', 3, K) for K in K_ENDS]


def attn_cases():
    return [(n, B, SHAPES[n][4]) for n in ATTN_SHAPES for B in (ATTN_BATCHES if n not in LARGE else (1, 3, 257))] + \
        [('hsi', 513, SHAPES['hsi'][4])]


def case_id(c):
    return '-'.join(str(x) for x in c)


# ------------------------------------------------------------------------------------------------------------ guarded buffers
def _esize(dtype):
    return torch.empty((), dtype=dtype).element_size()


def guarded(n, dtype, device, fill, canary=CANARY):
    body = n * _esize(dtype)
    total = 2 * GUARD_BYTES + body
    raw = torch.empty(total + ALIGN, dtype=torch.uint8, device=device)
    shift = (-(raw.data_ptr() + GUARD_BYTES)) % ALIGN
    whole = raw[shift:shift + total]
    whole[:GUARD_BYTES].fill_(canary)
    whole[GUARD_BYTES + body:].fill_(canary)
    whole[GUARD_BYTES:GUARD_BYTES + body].fill_(fill)
    view = whole[GUARD_BYTES:GUARD_BYTES + body].view(dtype)
    return view, whole


class Damage:
    """The result of intact(): true when both guards hold the canary; else before / behind = (first, last) damaged byte, before
    as offsets < 0 from the view's first byte, behind as offsets >= 0 from the byte after its last, None for an untouched guard."""

    def __init__(self, before, behind):
        self.before, self.behind = before, behind

    def __bool__(self):
        return self.before is None and self.behind is None

    def __repr__(self):
        if self:
            return 'intact'
        return 'damaged: bytes %s before the view, %s behind it' % (self.before, self.behind)


def _span(g, canary, origin):
    if bool((g == canary).all()):
        return None
    bad = (g != canary).nonzero().reshape(-1)
    return int(bad[0]) + origin, int(bad[-1]) + origin


def intact(whole, n, dtype, canary=CANARY):
    body = n * _esize(dtype)
    assert whole.numel() == 2 * GUARD_BYTES + body
    return Damage(_span(whole[:GUARD_BYTES], canary, -GUARD_BYTES), _span(whole[GUARD_BYTES + body:], canary, 0))


def bits(t):
    """The tensor's bits as integers (bit-equality also where a value is a NaN)."""
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


# ------------------------------------------------------------------------------------------------------------------- networks
def make_cfg(name, K=None, attention=False):
    C, C2, P, S, K0, width = SHAPES[name]
    cfg = {'patch_size': P, 'Categories_Number': K or K0, 'data_city': 's', 'DATA_DICT': {'s': {'size': [64, 64, C]}},
           'scale': S, 'aux_bands': C2, 'gmf': {'width': width, 'hidden': 64, 'pool_sigma': 2.5, 'attention': int(attention)}}
    if attention:
        cfg['trans'] = {'embed_dim': 96, 'num_head': 3}
    return cfg


def nets(name, K=None, attention=False, device='cuda:0'):
    """model.gmfnet.Net of the row `name` with the seed-0 weights plus 0.05 noise (the attention tensors x 3, so that the path
    carries signal): tests/test_gpu_parity.py's recipe without the CPU oracle."""
    from model.gmfnet import Net
    torch.manual_seed(0)
    net = Net(make_cfg(name, K, attention))
    with torch.no_grad():
        for k, p in net.named_parameters():
            p.add_(0.05 * torch.randn_like(p))
            if k.startswith('attn_'):
                p.mul_(3.0)
    return net.to(device)


def scene_batch(name, B, K, seed=0, extra=0):
    """Host tensors of a gather-mode batch: padded scenes A [H+P-1, W+P-1, C] and Bm [S(H+P-1)+extra, S(W+P-1)+extra, C2],
    xy [B, 2] int32 whose first rows are the four corner windows and one window on each edge of the padded scene, labels [B]
    int32 with both ends of the class range, dl [B, K] = randn / B."""
    C, C2, P, S, _, _ = SHAPES[name]
    H, W = SCENE_H, SCENE_W
    g = torch.Generator().manual_seed(1000 + 7 * B + K + seed)
    A = torch.rand(H + P - 1, W + P - 1, C, generator=g)
    Bm = torch.rand(S * (H + P - 1) + extra, S * (W + P - 1) + extra, C2, generator=g)
    xy = torch.stack([torch.randint(0, H, (B,), generator=g), torch.randint(0, W, (B,), generator=g)], 1).int()
    ends = edge_windows(H, W)
    xy[:min(B, len(ends))] = ends[:min(B, len(ends))]
    t = torch.randint(0, K, (B,), generator=g).int()
    t[0] = K - 1
    if B > 1:
        t[1] = 0
    dl = torch.randn(B, K, generator=g) / B
    return A, Bm, xy, t, dl


def edge_windows(H, W):
    """The four corner windows, then one window on each edge, of a scene whose windows start in [0, H) x [0, W)."""
    return torch.tensor([[H - 1, W - 1], [0, 0], [0, W - 1], [H - 1, 0], [0, W // 2], [H - 1, W // 2], [H // 2, 0], [H // 2, W - 1]],
                        dtype=torch.int32)


def patches_of(name, A, Bm, xy):
    """The materialised input of the same batch: a [B, C, P, P], b [B, C2, SP, SP]."""
    _, _, P, S, _, _ = SHAPES[name]
    a = torch.stack([A[x:x + P, y:y + P, :].permute(2, 0, 1) for x, y in xy.tolist()]).contiguous()
    b = torch.stack([Bm[S * x:S * x + S * P, S * y:S * y + S * P, :].permute(2, 0, 1) for x, y in xy.tolist()]).contiguous()
    return a, b


def split_ws(ws, slab, B, F2, H=64):
    """tests/test_gpu_exit_path.py's split_ws: the head vectors z, h, dh, dl [B, W] of a workspace (floats)."""
    from test_gpu_exit_path import split_ws as split
    return split(ws, slab, B, F2, H)
