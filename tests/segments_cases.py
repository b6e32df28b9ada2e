"""The cases of the superpixel-voting tests, shared by tests/test_segments_host.py (the guards, on the float64
reference alone) and tests/test_gpu_segments.py.  A plain module: no GPU, nothing of the HIP library.

The scenes, logits and masks are those of tests/spatial_cases.py: piecewise-constant regions of 5 x 4 pixels drawn from five base
spectra with 0.05 Gaussian noise, logits that favour the class `region mod K`, a mask of about 90 % ones.  The base spectrum of
a pixel's region (`ids`) is what the purity guard counts."""
import spatial_cases as S

SIZES = S.SIZES                          # (1, 1), (2, 7), (13, 9), (33, 17), (35, 34), (64, 65)
SEG_SIZES = (4, 5, 16)                   # 5 divides nothing; 16 leaves one cell or one row of cells at the small sizes
BANDS_F32 = (1, 3, 4, 8, 200, 224)
BANDS_F16 = (8, 200)
COMPACTNESS = 0.05
VOTE_K = (1, 3, 17, 64)
ITERATIONS = 10
GUARD_MIN_PIXELS = S.GUARD_MIN_PIXELS    # the share guards are asked of scenes of at least this many pixels
TIE_CAP = 0.02                           # guard (a): the share of pixels left out of the label comparison

scene, logits, mask, pixels = S.scene, S.logits, S.mask, S.pixels


def ids(H, W):
    """[H, W] int: which of the five base spectra the region of every pixel was drawn from."""
    return S.regions(H, W) % 5


# (H, W, C, half, S): every size with every band count and type and every segment size
SLIC_CASES = [(H, W, C, half, seg) for H, W in SIZES for C, half in [(C, False) for C in BANDS_F32] + [(C, True) for C in BANDS_F16]
              for seg in SEG_SIZES]
# (H, W, K, S): every size with every class count and segment size; the segments are those of the 8-band fp32 scene
VOTE_CASES = [(H, W, K, seg) for H, W in SIZES for K in VOTE_K for seg in SEG_SIZES]


def cells_per_axis(H, W, seg):
    return -(-H // seg), -(-W // seg)


# Guard (b), recorded findings: the (H, W, C, half, S) at which the float64 reference's segments after ten iterations are NOT purer
# than the plain grid, with (their purity, the grid's).  All three are one-band scenes, where five scalar base values meet 0.05
# noise.  The reference records no near tie in any assign of the three, so a device is asked for the same segment image.
PURITY_SHORTFALLS = {(33, 17, 1, False, 4): (0.9875222816399287, 1.0),
                     (64, 65, 1, False, 4): (0.7540865384615385, 0.8125),
                     (64, 65, 1, False, 5): (0.6935096153846154, 0.7076923076923077)}


def purity_asked(H, W, seg):
    """Guard (b) is asked of every scene with more than one cell per axis."""
    return min(cells_per_axis(H, W, seg)) > 1


def check_purity(case, got, plain):
    """Guard (b) for one case (H, W, C, half, S): the segments' purity `got` exceeds the plain grid's `plain`.  Where the grid is
    already perfectly pure (33 x 17 at S = 4: the ids depend on the column block only there, and the 4-pixel blocks coincide
    with the cells) nothing exceeds it, and the segments are asked to be perfectly pure too.  The recorded shortfalls are asked
    for their recorded figures: a finding that moves is to be looked at, in either direction."""
    if case in PURITY_SHORTFALLS:
        assert abs(got - PURITY_SHORTFALLS[case][0]) <= 1e-12 and plain == PURITY_SHORTFALLS[case][1] and got < plain, (case, got, plain)
    elif plain == 1.0:
        assert got == 1.0, (case, got, plain)
    else:
        assert got > plain, (case, got, plain)


def classes_guarded(H, W, K, seg):
    """Where the vote is asked to show at least 3 classes: K >= 3, at least GUARD_MIN_PIXELS pixels, and at least 3 cells per axis —
    a scene of one or two cells along an axis has as few as one to six segments, and a segment has one class."""
    return K >= 3 and H * W >= GUARD_MIN_PIXELS and min(cells_per_axis(H, W, seg)) >= 3
