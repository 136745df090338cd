"""Case builders and numpy references for the per-element tests of the paste-back / alignment kernels (cf_paste.hip).

Plain helpers, no fixtures.  tests/test_paste_cases_host.py proves on the CPU, with the references alone, that these cases can see what
they claim to see (every sub-pixel fraction, every in/out state of the taps, exact rounding ties, results that a fused multiply-add would
change, geometry whose masks stay inside DeviceFaceHelper._region); tests/test_gpu_paste_kernels.py runs the kernels on them.

The references here are the ones oracle/paste_oracle.py (P below) does not already have: the blend expression, the label_lut /
clear-border / truncation definitions, the float32 linear resize, and restatements of P's uint8 warp and resize that stop at the integer
accumulator (the host test pins them to P) so that a tie can be counted.

Matrices are FORWARD matrices in cv2.warpAffine's sense (source -> destination), which is what P takes; the kernels take the
destination -> source matrix that `invert_affine` derives from it in double precision, as the host code does.
"""
import math

import numpy as np

from oracle import paste_oracle as P

F32 = np.float32


def d2s_to_fwd(d2s):
    """The forward matrix whose double-precision inverse is (up to that inversion's rounding) the given destination -> source matrix."""
    return P.invert_affine(np.asarray(d2s, dtype=np.float64))


def rot_fwd(angle, scale, tx, ty):
    c, s = math.cos(angle) * scale, math.sin(angle) * scale
    return np.array([[c, -s, tx], [s, c, ty]], dtype=np.float64)


# ---- sampling: fraction grids ---------------------------------------------------------------------------------------------------------
GRID_SRC_HW = (2, 2)
BORDERS = ((135, 133, 132), (0, 0, 0))


def grid_matrices():
    """(name, forward matrix, (dw, dh)): two magnifications of a 2 x 2 source whose 1/32-pixel steps visit every (a, b) fraction pair
    and every in/out state of the four taps: axis-aligned with a destination -> source step of exactly 1/32 px onto 104 x 104, and a
    general one rotated by 0.7 rad at scale 1/29.3 onto 144 x 144.  The rotated one's offsets put the source near the destination's
    centre: with offsets that leave it near the origin (such as (-0.3, -2.1)) no destination pixel has its taps both right of and above
    the source, whatever the destination's size, so 6 of the 25 tap states would never occur."""
    c, s = math.cos(0.7) / 29.3, math.sin(0.7) / 29.3
    return [('step_1_32', d2s_to_fwd([[1 / 32, 0, -1.2], [0, 1 / 32, -1.2]]), (104, 104)),
            ('rot_0.7_s_29.3', d2s_to_fwd([[c, -s, 0.3], [s, c, -2.9]]), (144, 144))]


def origin_grid():
    """The rotated matrix with the source left at the destination's origin (offsets (-0.3, -2.1), 104 x 104): every fraction pair and
    over 100 ties, but only 19 of the 25 tap states (see grid_matrices), so it is a further sampling case and not one of the grids."""
    c, s = math.cos(0.7) / 29.3, math.sin(0.7) / 29.3
    return ('rot_0.7_s_29.3_origin', d2s_to_fwd([[c, -s, -0.3], [s, c, -2.1]]), (104, 104))


def grid_source_u8(seed=11):
    src = np.random.default_rng(seed).integers(0, 256, GRID_SRC_HW + (3,), dtype=np.uint8)
    src[0, 0, 0], src[1, 1, 2] = 0, 255
    return src


def mixed_f32(shape, seed):
    """float32 values of mixed sign and magnitude 1e-3 .. 1e3."""
    rng = np.random.default_rng(seed)
    return (rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-3, 3, shape)).astype(F32)


def fraction_pairs(fwd, dsize):
    """Set of (a, b) 5-bit fraction pairs the destination visits."""
    _, _, a, b = P._warp_coords(fwd, *dsize)
    return set(zip(a.reshape(-1).tolist(), b.reshape(-1).tolist()))


def tap_states(fwd, dsize, sh, sw):
    """Per destination pixel the state of the tap pair on each axis: 0 both taps before the source, 1 only the second tap in,
    2 both in, 3 only the first tap in, 4 both past the source.  Returns the set of (state_x, state_y) pairs."""
    ix, iy, _, _ = P._warp_coords(fwd, *dsize)

    def state(i, n):
        return np.select([i < -1, i == -1, i < n - 1, i == n - 1], [0, 1, 2, 3], 4)

    return set(zip(state(ix, sw).reshape(-1).tolist(), state(iy, sh).reshape(-1).tolist()))


def warp_u8_acc(src, fwd, dsize, border_value=(0, 0, 0)):
    """P.warp_affine_u8 up to the 15-bit accumulator: the result is (acc + 2^14) >> 15, a tie is acc mod 2^15 == 2^14."""
    dw, dh = dsize
    h, w, c = src.shape
    ix, iy, a, b = P._warp_coords(fwd, dw, dh)
    bv = np.asarray(border_value, dtype=np.int64)[:c]
    acc = np.zeros((dh, dw, c), dtype=np.int64)
    for dy, dx, wgt in ((0, 0, (32 - a) * (32 - b)), (0, 1, a * (32 - b)), (1, 0, (32 - a) * b), (1, 1, a * b)):
        sx, sy = ix + dx, iy + dy
        ok = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
        tap = np.where(ok[..., None], src[np.clip(sy, 0, h - 1), np.clip(sx, 0, w - 1)].astype(np.int64), bv[None, None, :])
        acc += tap * (wgt * 32)[..., None]
    return acc


def warp_ties(acc):
    return int(((acc & ((1 << 15) - 1)) == (1 << 14)).sum())


# ---- sampling: further matrices -------------------------------------------------------------------------------------------------------
FURTHER_SRC_HW = (9, 13)
FURTHER_DSIZE = (27, 21)                                     # (dw, dh): 567 pixels, three blocks


def further_source_u8(seed=12, n=None):
    shape = FURTHER_SRC_HW + (3,) if n is None else (n,) + FURTHER_SRC_HW + (3,)
    src = np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)
    src.reshape(-1, 3)[0] = (0, 255, 0)
    src.reshape(-1, 3)[-1] = (255, 0, 255)
    return src


def further_matrices():
    """(name, forward matrix) against a (9, 13) source and a (21, 27) destination."""
    return [('identity', np.array([[1.0, 0, 0], [0, 1.0, 0]])),
            ('shift_+5_+3', np.array([[1.0, 0, 5], [0, 1.0, 3]])),
            ('shift_-4_-6', np.array([[1.0, 0, -4], [0, 1.0, -6]])),
            ('rot_90_exact', np.array([[0.0, -1, 12], [1.0, 0, 2]])),
            ('rot_90', rot_fwd(math.pi / 2, 1.0, 12, 2)),
            ('rot_180', rot_fwd(math.pi, 1.0, 16, 12)),
            ('mirror', np.array([[-1.0, 0, 14], [0, 1.0, 4]])),
            ('minify_8', d2s_to_fwd([[8.0, 0, -20], [0, 8.0, -30]])),
            ('magnify_37', d2s_to_fwd([[1 / 37, 0, -0.3], [0, 1 / 37, -0.2]])),
            ('magnify_37_far_edge', d2s_to_fwd([[1 / 37, 0, 11.6], [0, 1 / 37, 7.7]])),
            ('magnify_rot_inside', d2s_to_fwd([[math.cos(0.7) / 3.3, -math.sin(0.7) / 3.3, 4.1], [math.sin(0.7) / 3.3, math.cos(0.7) / 3.3, 0.2]])),
            ('shift_1e6', np.array([[1.0, 0, 1e6], [0, 1.0, -1e6]])),
            ('singular', np.array([[1.0, 2, 3], [2.0, 4, 5]]))]          # invert_affine gives all zeros: every pixel is src[0, 0]


FURTHER_DENSE = ('magnify_37', 'magnify_rot_inside')     # most pixels sum several non-zero float taps


def batch_matrices():
    """Three different matrices for the per-item-source branch."""
    return [rot_fwd(0.3, 1.7, 2.5, -1.25), np.array([[-1.2, 0.1, 20.5], [0.2, 1.9, 1.0]]), np.array([[1.0, 0, 3], [0, 1.0, 2]])]


def corner_regions(w, h, rw, rh):
    """(x, y, w, h) windows touching each corner of a w x h array."""
    return [(0, 0, rw, rh), (w - rw, 0, rw, rh), (0, h - rh, rw, rh), (w - rw, h - rh, rw, rh)]


# ---- float evaluation, separately rounded and fused -----------------------------------------------------------------------------------
def _fma(p, w, acc):
    """A fused multiply-add as this suite models it: the product held in float64, rounded once with the add."""
    return (p.astype(np.float64) * np.asarray(w, np.float64) + acc.astype(np.float64)).astype(F32)


def warp_f32_sums(src, fwd, dsize):
    """The four-tap float sum of P.warp_affine_f32, (separately rounded, fused)."""
    dw, dh = dsize
    h, w = src.shape
    ix, iy, a, b = P._warp_coords(fwd, dw, dh)
    fa, fb = a.astype(F32) / F32(32), b.astype(F32) / F32(32)
    sep, fused = np.zeros((dh, dw), F32), np.zeros((dh, dw), F32)
    for dy, dx, wgt in ((0, 0, (1 - fa) * (1 - fb)), (0, 1, fa * (1 - fb)), (1, 0, (1 - fa) * fb), (1, 1, fa * fb)):
        sx, sy = ix + dx, iy + dy
        ok = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
        tap = np.where(ok, src[np.clip(sy, 0, h - 1), np.clip(sx, 0, w - 1)], F32(0))
        sep = sep + tap * wgt.astype(F32)
        fused = _fma(tap, wgt, fused)
    return sep, fused


def gauss_row_sums(img, ksize, sigma=0.0):
    """The row pass of P.gaussian_blur, (separately rounded, fused)."""
    k = P.gaussian_kernel(ksize, sigma)
    r = ksize // 2
    h, w = img.shape
    cols = P._reflect101(np.arange(-r, w + r), w)
    sep, fused = np.zeros((h, w), F32), np.zeros((h, w), F32)
    for i in range(ksize):
        sep = sep + img[:, cols[i:i + w]] * k[i]
        fused = _fma(img[:, cols[i:i + w]], k[i], fused)
    return sep, fused


# ---- blend ----------------------------------------------------------------------------------------------------------------------------
BLEND_CANVAS_HW = (23, 29)
BLEND_FACE_HW = (16, 16)


def blend_inputs(seed=21):
    """Full-canvas inputs of paste_blend; a region's ero / soft / parse buffers are windows of these.  Masks are drawn from [0, 1] with
    exact 0 and 1 entries and entries where parse == soft; the canvas holds non-integer values in [0, 255]."""
    rng = np.random.default_rng(seed)
    ch, cw = BLEND_CANVAS_HW
    canvas = rng.uniform(0, 255, (ch, cw, 3)).astype(F32)
    masks = []
    for _ in range(3):
        m = rng.random((ch, cw)).astype(F32)
        r = rng.random((ch, cw))
        m[r < 0.03] = 0
        m[r > 0.97] = 1
        masks.append(m)
    ero, soft, parse = masks
    parse[:] = np.sqrt(parse)                                # skewed towards 1, so that min(parse, soft) is parse in a third of the pixels
    same = rng.random((ch, cw)) < 0.05
    parse[same] = soft[same]
    face = rng.integers(0, 256, BLEND_FACE_HW + (3,), dtype=np.uint8)
    face[3, 3], face[3, 4] = 0, 255
    return canvas, face, ero, soft, parse


def blend_matrices():
    """(name, forward matrix face -> canvas, dense): dense ones put the face over most of the canvas."""
    return [('magnify_rot', rot_fwd(0.7, 3.2, 22, -14), True),
            ('stretch', d2s_to_fwd([[1 / 2.3, 0, 2.1], [0, 1 / 1.9, 1.7]]), True),
            ('identity', np.array([[1.0, 0, 0], [0, 1.0, 0]]), False),
            ('shift_+5_+3', np.array([[1.0, 0, 5], [0, 1.0, 3]]), False),
            ('shift_-4_-6', np.array([[1.0, 0, -4], [0, 1.0, -6]]), False),
            ('rot_90_exact', np.array([[0.0, -1, 22], [1.0, 0, 3]]), False),
            ('mirror', np.array([[-2.1, 0, 31], [0, 1.7, -2.0]]), True),
            ('singular', np.array([[1.0, 2, 3], [2.0, 4, 5]]), False)]


def blend_regions():
    ch, cw = BLEND_CANVAS_HW
    return [(0, 0, cw, ch), (7, 5, 11, 9), (13, 11, 1, 1)] + corner_regions(cw, ch, 6, 5)


def blend_terms(canvas, face, fwd, ero, soft, parse=None):
    """m, pasted = e * restored, canvas as float32 arrays of the canvas's shape (face_restoration_helper.py:400, :432, :481-483)."""
    ch, cw = canvas.shape[:2]
    restored = P.warp_affine_u8(face, fwd, (cw, ch)).astype(F32)
    m = soft if parse is None else np.where(parse < soft, parse, soft)
    return m[:, :, None], ero[:, :, None] * restored


def blend_ref(canvas, face, fwd, ero, soft, region, parse=None):
    """m * (e * restored) + (1 - m) * canvas in numpy float32 inside region (x, y, w, h); the canvas outside it unchanged."""
    m, pasted = blend_terms(canvas, face, fwd, ero, soft, parse)
    full = m * pasted + (1 - m) * canvas
    assert full.dtype == F32
    x, y, w, h = region
    out = canvas.copy()
    out[y:y + h, x:x + w] = full[y:y + h, x:x + w]
    return out


def blend_fused(canvas, face, fwd, ero, soft, parse=None):
    """The full-canvas blend with one of the two products fused into the add: the two forms a contracting compiler can emit."""
    m, pasted = blend_terms(canvas, face, fwd, ero, soft, parse)
    return (_fma(np.broadcast_to(m, canvas.shape), pasted, (1 - m) * canvas),
            _fma(np.broadcast_to(1 - m, canvas.shape), canvas, m * pasted))


# ---- erode, gaussian ------------------------------------------------------------------------------------------------------------------
ERODE_SHAPES = ((1, 1), (1, 17), (17, 1), (5, 7), (75, 61))
ERODE_KS = (0, 1, 2, 3, 4, 5)
ERODE_K_LARGE = 40                                           # on the small shapes: a window larger than the array


def erode_inputs(shape, seed=31):
    """Random values, and 0/1 plateaus joined by ramps (what the warped square mask looks like)."""
    rng = np.random.default_rng(seed + shape[0] * 100 + shape[1])
    h, w = shape
    yy, xx = np.mgrid[0:h, 0:w]
    ramp = np.clip((np.minimum(np.minimum(xx, w - 1 - xx), np.minimum(yy, h - 1 - yy)) - 1) / 3.0, 0, 1).astype(F32)
    tilt = np.clip((xx * 0.37 + yy * 0.81) / 4.0 - 1.0, 0, 1).astype(F32)
    return [('random', rng.random(shape).astype(F32)), ('plateau', ramp), ('tilted', tilt)]


GAUSS_KSIZES = ((1, 0.0), (3, 0.0), (5, 0.0), (7, 0.0), (9, 0.0), (21, 0.0), (61, 0.0), (101, 11.0))
GAUSS_FRAMES = ((1, 64), (64, 1), (53, 57), (5, 7))
GAUSS_WINDOW_FRAME = (56, 60)


def gauss_allowed(ksize, frame_hw):
    """One reflection at the most on every axis longer than one pixel (neither side defines more); a one-pixel axis reads its only
    sample for every tap, as cv::borderInterpolate does for len == 1."""
    return all(n == 1 or ksize // 2 < n for n in frame_hw)


def gauss_windows():
    """(x, y, w, h) inside GAUSS_WINDOW_FRAME: each corner, each edge, the interior, the frame itself."""
    fh, fw = GAUSS_WINDOW_FRAME
    rw, rh = 23, 19
    mx, my = (fw - rw) // 2, (fh - rh) // 2
    return corner_regions(fw, fh, rw, rh) + [(mx, 0, rw, rh), (mx, fh - rh, rw, rh), (0, my, rw, rh), (fw - rw, my, rw, rh),
                                             (mx, my, rw, rh), (0, 0, fw, fh)]


# ---- linear resizes -------------------------------------------------------------------------------------------------------------------
RESIZE_SOURCES = ((1, 1), (1, 9), (9, 1), (2, 2), (31, 45))


def resize_targets(sh, sw):
    """(dh, dw): x2, x3, a non-integer enlargement, a reduction, 1 x 1 and identity."""
    t = [(2 * sh, 2 * sw), (3 * sh, 3 * sw), (int(sh * 1.7) + 1, int(sw * 2.3) + 1), (max(1, (sh * 2) // 3), max(1, (sw * 3) // 5)), (1, 1), (sh, sw)]
    return list(dict.fromkeys(t))


def resize_source_u8(shape, seed=41):
    src = np.random.default_rng(seed + shape[0] * 100 + shape[1]).integers(0, 256, shape + (3,), dtype=np.uint8)
    src[0, 0, 0], src[-1, -1, 2] = 0, 255
    return src


def resize_u8_acc(img, dsize):
    """P.resize_linear_u8 up to the 22-bit accumulator: the result is (acc + 2^21) >> 22, a tie is acc mod 2^22 == 2^21."""
    h, w = img.shape[:2]
    dw, dh = dsize

    def axis(n_src, n_dst):
        f = (np.arange(n_dst, dtype=np.float64) + 0.5) * (n_src / n_dst) - 0.5
        i0 = np.floor(f).astype(np.int64)
        fr = (f - i0).astype(F32)
        lo, hi = i0 < 0, i0 >= n_src - 1
        fr[lo | hi] = 0.0
        i0[lo] = 0
        i0[hi] = n_src - 1
        w1 = np.rint(fr.astype(np.float64) * 2048.0).astype(np.int64)
        return i0, np.minimum(i0 + 1, n_src - 1), 2048 - w1, w1

    x0, x1, wx0, wx1 = axis(w, dw)
    y0, y1, wy0, wy1 = axis(h, dh)
    s = img.astype(np.int64)
    r0, r1 = s[y0], s[y1]
    top = r0[:, x0] * wx0[None, :, None] + r0[:, x1] * wx1[None, :, None]
    bot = r1[:, x0] * wx0[None, :, None] + r1[:, x1] * wx1[None, :, None]
    return top * wy0[:, None, None] + bot * wy1[:, None, None]


def resize_ties(acc):
    return int(((acc & ((1 << 22) - 1)) == (1 << 21)).sum())


def resize_linear_f32(img, dsize):
    """cv2.resize(float32 plane, (dw, dh), INTER_LINEAR) (:482): f = float32((d + 0.5) * scale - 0.5), s = floor(f), f -= s, edges
    clamped to (0, 0) / (n - 1, 0); rows horizontally first (a plain copy where s + 1 is past the edge), then vertically; float32
    products and sums rounded separately."""
    h, w = img.shape
    dw, dh = dsize

    def axis(n_src, n_dst):
        f = ((np.arange(n_dst, dtype=np.float64) + 0.5) * (n_src / n_dst) - 0.5).astype(np.float32)
        s = np.floor(f).astype(np.int64)
        f = f - s.astype(np.float32)
        lo, hi = s < 0, s >= n_src - 1
        f[lo | hi] = 0
        s[lo] = 0
        s[hi] = n_src - 1
        return s, f

    sx, fx = axis(w, dw)
    sy, fy = axis(h, dh)
    one = np.float32(1)
    two = sx + 1 < w
    hr = np.where(two[None, :], img[:, sx] * (one - fx)[None, :] + img[:, np.minimum(sx + 1, w - 1)] * fx[None, :], img[:, sx])
    return hr[sy] * (one - fy)[:, None] + hr[np.minimum(sy + 1, h - 1)] * fy[:, None]


# ---- small kernels --------------------------------------------------------------------------------------------------------------------
def trunc_values():
    """Every integer 0..255, the float just below each next integer, k + 0.5, -0.0 and the smallest positive float."""
    k = np.arange(256, dtype=F32)
    return np.concatenate([k, np.nextafter(k + F32(1), F32(0)), k + F32(0.5), np.array([-0.0, np.finfo(F32).smallest_subnormal], F32)]).astype(F32)


def trunc_ref(x):
    """ndarray.astype(np.uint8) of values in (-1, 256): truncation toward zero."""
    return np.trunc(x).astype(np.int64).astype(np.uint8)


def lut_labels(nlut):
    return np.array([-1, 0, nlut - 1, nlut, 31, 32, 2 ** 31, 2 ** 40, -2 ** 40, 1, 7, nlut - 2], dtype=np.int64)


def lut_table(nlut):
    return [float(F32(3.25 * i - 17.5)) for i in range(nlut)]


def label_lut_ref(labels, lut):
    """out = lut[label] (face_restoration_helper.py:468-471); a label outside 0 .. len(lut) - 1 gives 0."""
    t = np.asarray(lut, dtype=F32)
    ok = (labels >= 0) & (labels < len(t))
    return np.where(ok, t[np.where(ok, labels, 0)], F32(0))


def scale_clear_border_ref(x, border, scale):
    """x * float32(scale) inside the border frame, exactly 0 on it whatever x holds there (:476-481)."""
    out = np.zeros_like(x)
    h, w = x.shape[1:]
    if h - 2 * border > 0 and w - 2 * border > 0:
        out[:, border:h - border, border:w - border] = x[:, border:h - border, border:w - border] * F32(scale)
    return out


SUM_LENGTHS = (1, 63, 64, 65, 64 * 256 + 1)


def sum_chunks(n):
    """(lo, hi) of the 64 fixed chunks cf_sum_f32 splits n elements into."""
    chunk = (n + 63) // 64
    return [(min(b * chunk, n), min((b + 1) * chunk, n)) for b in range(64)]


# ---- geometry product (Table 1 of the issue that introduced these tests) -----------------------------------------------------------------
FRAME_HW = (72, 96)
FACE = 64
UPSCALES = (1, 2, 3)
SIZES = (6, 19, 20, 21, 40, 90, 160, 400)
ANGLES = (0.0, 0.4, math.pi / 4, math.pi / 2, math.pi, -2.0)
CENTRES = ((48, 36), (0, 0), (95, 71), (0, 71), (95, 0), (-20, 36), (48, 100), (47.5, 35.5))


def face_affine(cx, cy, size, angle=0.0, face=FACE):
    """frame -> face similarity for a face of `size` frame pixels centred at (cx, cy), rotated by `angle`."""
    c, s = np.cos(angle), np.sin(angle)
    pts = np.array([[-0.25, -0.1], [0.25, -0.1], [0.0, 0.25]])
    src = (pts * size) @ np.array([[c, -s], [s, c]]).T + [cx, cy]
    return P.similarity_from_points(src, pts * face + face / 2)


def geometry_product():
    """(upscale, size, angle, centre) of all 3 * 8 * 6 * 8 = 1152 cases."""
    return [(u, s, a, c) for u in UPSCALES for s in SIZES for a in ANGLES for c in CENTRES]


def pipeline_cases(u):
    """64 of the 384 cases of one upscale: one angle for every (size, centre) pair, so every size and every centre occurs 8 times and
    every angle at least 8 times; the angle's offset moves with the upscale."""
    return [(u, s, a, c) for si, s in enumerate(SIZES) for ai, a in enumerate(ANGLES) for ci, c in enumerate(CENTRES)
            if (si + ci + u) % len(ANGLES) == ai]


def overlap_affines():
    """Three mutually overlapping faces (each pair shares pixels), off the product's grid."""
    return [face_affine(40, 30, 40, 0.4), face_affine(55, 38, 40, -2.0), face_affine(47.5, 35.5, 90, math.pi / 4)]


def paste_matrix(aff, u):
    """The face -> upscaled-frame matrix paste_faces_to_input_image warps with (:352-356, :393-398)."""
    inv = P.invert_affine(aff) * u
    inv[:, 2] += 0.5 * u if u > 1 else 0
    return inv


def oracle_masks(aff, u, frame_hw=FRAME_HW, face=FACE):
    """The full-frame masks of P.paste_faces for one face: (warped square mask, first erosion, second erosion, soft mask, float32 area)."""
    h_up, w_up = frame_hw[0] * u, frame_hw[1] * u
    inv_mask = P.warp_affine_f32(np.ones((face, face), F32), paste_matrix(aff, u), (w_up, h_up))
    ero = P.erode(inv_mask, int(2 * u))
    area = np.sum(ero)
    w_edge = int(area ** 0.5) // 20
    center = P.erode(ero, w_edge * 2)
    return inv_mask, ero, center, P.gaussian_blur(center, w_edge * 2 + 1), area
