"""Test helper: flow_warp from its definition (numpy), the two input families and the bound of the flow_warp tests.

The definition (include/codeformer_hip.h, cf_flow_warp) restated on its own.  For output pixel (y, x) of image b, in float32, one operation per step:
  px = float32(x) + dx,  py = float32(y) + dy                                  (flow[b, y, x] = (dx, dy))
  align_corners:      ix = px * (float32(W-1) / float32(max(W-1, 1)))
  not align_corners:  ix = px * (float32(W) / float32(max(W-1, 1))) - 0.5      (normalised by W - 1 either way: the reference's quirk)
  border:      ix < 0 -> 0, ix > W-1 -> W-1 (comparisons: a NaN stays)
  reflection:  (lo, span) = (0, W-1) | (-0.5, W);  a = |ix - lo|, r = fmod(a, 2 span), ix = (r if r <= span else 2 span - r) + lo, then the clamp
  bilinear:    sampled when ix > -1, iy > -1, ix < W, iy < H;  x0 = floor(ix), lw = ix - x0, hw = 1 - lw;  corner weights hh*hw, hh*lw, lh*hw, lh*lw for
               top-left, top-right, bottom-left, bottom-right; a corner outside the image contributes 0
  nearest:     the pixel at (rint(ix), rint(iy)), half to even; 0 outside the image
  a NaN coordinate fails every test and gives 0 in every padding mode.
Positions and weights are float32 exactly as written; the products w_i * v_i and their sum are float64.  Next to the value the helper returns
S = sum_i |w_i v_i| and the position term D (below) per output element.

The bound.  The op forms t_i = fl(w_i * v_i) and out = fl(fl(fl(t0 + t1) + t2) + t3) from the float32 weights the helper shares with it.  With
u = 2^-24, a term passes through at most one product rounding and three sum roundings, each a factor (1 + d), |d| <= u; so
  |out - sum_i w_i v_i| <= ((1 + u)^4 - 1) * S <= 4.000001 u S,   and BLEND_C = 5 covers it with the second-order terms (an fma in place of a
product and a sum only removes a rounding).  Nearest copies a pixel: S = |v| and the error is 0.
Without align_corners two more operations stand between the position and the coordinate: the product px * ratio and the subtraction of 0.5, each
rounded to within u times its result, so a coordinate computed otherwise (in wider arithmetic, say) differs by at most
  dx = u * (|px * ratio| + |ix|),   dy likewise,
and reflection and clamp do not enlarge that (slope +-1, or 0 where the clamp cuts: no term there).  The bilinear sample is continuous and piecewise linear in (ix, iy) with
|d/d ix| <= |v01 - v00| + |v11 - v10| and |d/d iy| <= |v10 - v00| + |v11 - v01| (v outside the image = 0), which gives
  D = max(dx, dy) * (|v01 - v00| + |v10 - v00| + |v11 - v10| + |v11 - v01|);   D = 0 with align_corners (ratio is 1 or 0: the product is exact) and for
nearest (whose inputs are kept 2^-10 away from a rounding tie instead: reject_ties).
  |got - ref| <= BLEND_C * 2^-24 * S + D.
Nothing here is tuned to an implementation's output.
"""
import functools

import numpy as np

f32 = np.float32
U = 2.0 ** -24
BLEND_C = 5.0
INTERPS = ('bilinear', 'nearest')
PADDINGS = ('zeros', 'border', 'reflection')
MODES = [(i, p, a) for i in INTERPS for p in PADDINGS for a in (True, False)]
FAMILIES = ('exact', 'random')
TIE_MARGIN = 2.0 ** -10


def coord(p, n, padding, align):
    """(float32 sample coordinate of the float32 positions p on an axis of n pixels, the ratio, where the border clamp cut it)."""
    assert p.dtype == f32
    ratio = f32(n - 1 if align else n) / f32(max(n - 1, 1))
    with np.errstate(invalid='ignore', over='ignore'):
        i = p * ratio
        if not align:
            i = i - f32(0.5)
        hi = f32(n - 1)
        if padding == 'reflection':
            lo, span = (f32(0), hi) if align else (f32(-0.5), f32(n))
            if span > 0:
                r = np.fmod(np.abs(i - lo), span + span)
                i = np.where(r <= span, r, (span + span) - r) + lo
        flat = np.zeros(i.shape, bool)
        if padding != 'zeros':
            flat = (i < 0) | (i > hi)
            i = np.where(i < 0, f32(0), np.where(i > hi, hi, i))
    assert i.dtype == f32
    return i, ratio, flat


def positions(flow):
    """(px, py): float32 arrays (B, H, W)."""
    flow = np.asarray(flow, f32)
    _, H, W, _ = flow.shape
    with np.errstate(invalid='ignore', over='ignore'):
        return np.arange(W, dtype=f32)[None, None, :] + flow[..., 0], np.arange(H, dtype=f32)[None, :, None] + flow[..., 1]


def warp_ref(x, flow, interp='bilinear', padding='zeros', align=True):
    """(value, S, D): float64 arrays of the shape of x."""
    x, flow = np.asarray(x, f32), np.asarray(flow, f32)
    B, C, H, W = x.shape
    assert flow.shape == (B, H, W, 2)
    px, py = positions(flow)
    (ix, rx, fx), (iy, ry, fy) = coord(px, W, padding, align), coord(py, H, padding, align)
    bi, ci = np.arange(B)[:, None, None, None], np.arange(C)[None, :, None, None]

    def take(inside, cy, cx):
        return np.where(inside[:, None], x[bi, ci, np.where(inside, cy, 0)[:, None], np.where(inside, cx, 0)[:, None]].astype(np.float64), 0.0)

    with np.errstate(invalid='ignore'):
        if interp == 'nearest':
            qx, qy = np.rint(ix), np.rint(iy)
            ok = (qx >= 0) & (qy >= 0) & (qx <= W - 1) & (qy <= H - 1)
            v = take(ok, np.where(ok, qy, 0).astype(np.int64), np.where(ok, qx, 0).astype(np.int64))
            return v + 0.0, np.abs(v), np.zeros_like(v)
        ok = (ix > f32(-1)) & (iy > f32(-1)) & (ix < f32(W)) & (iy < f32(H))
    ixs, iys = np.where(ok, ix, f32(0)), np.where(ok, iy, f32(0))
    x0f, y0f = np.floor(ixs), np.floor(iys)
    lw, lh = ixs - x0f, iys - y0f
    hw, hh = f32(1) - lw, f32(1) - lh
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    val, S, vs = np.zeros(x.shape), np.zeros(x.shape), []
    for cy, cx, cw in ((y0, x0, hh * hw), (y0, x0 + 1, hh * lw), (y0 + 1, x0, lh * hw), (y0 + 1, x0 + 1, lh * lw)):
        assert cw.dtype == f32
        inside = ok & (cy >= 0) & (cy <= H - 1) & (cx >= 0) & (cx <= W - 1)
        v = take(inside, cy, cx)
        t = np.where(inside[:, None], cw.astype(np.float64)[:, None] * v, 0.0)
        val, S = val + t, S + np.abs(t)
        vs.append(v)
    D = np.zeros(x.shape)
    if not align:
        with np.errstate(invalid='ignore', over='ignore'):
            dx = U * (np.abs(px.astype(np.float64) * float(rx)) + np.abs(px.astype(np.float64) * float(rx) - 0.5))
            dy = U * (np.abs(py.astype(np.float64) * float(ry)) + np.abs(py.astype(np.float64) * float(ry) - 0.5))
            d = np.where(ok, np.maximum(np.where(fx, 0.0, dx), np.where(fy, 0.0, dy)), 0.0)     # (a clamped coordinate does not move with the position)
        v00, v01, v10, v11 = vs
        D = d[:, None] * (np.abs(v01 - v00) + np.abs(v10 - v00) + np.abs(v11 - v10) + np.abs(v11 - v01))
    return val + 0.0, S, D


def bound(S, D):
    return BLEND_C * U * S + D


def tie_distance(flow):
    """Smallest distance, over both axes and both align_corners values, of the float64 coordinate from k + 1/2 (where rint changes)."""
    flow = np.asarray(flow, f32).astype(np.float64)
    _, H, W, _ = flow.shape
    worst = np.full(flow.shape[:3], np.inf)
    for n, p in ((W, np.arange(W)[None, None, :] + flow[..., 0]), (H, np.arange(H)[None, :, None] + flow[..., 1])):
        for i in (p * ((n - 1) / max(n - 1, 1)), p * (n / max(n - 1, 1)) - 0.5):
            worst = np.minimum(worst, np.abs(i - np.floor(i) - 0.5))
    return worst


def reject_ties(flow, rng, lim):
    """Redraw (uniform in +-lim) every flow vector whose coordinate lies within TIE_MARGIN of a rounding tie: a condition on the inputs."""
    flow = flow.copy()
    for _ in range(100):
        bad = tie_distance(flow) <= TIE_MARGIN
        if not bad.any():
            return flow
        flow[bad] = rng.uniform(-lim, lim, (int(bad.sum()), 2)).astype(f32)
    raise AssertionError('reject_ties: ties left')


def make_inputs(shape, family, seed=0):
    """(x, flow) float32.  exact: x integers in [-8, 8], flow multiples of 1/4 in [-3, 3]; with H in {5, 3} and W in {9, 17} (ratios 1.25, 1.5, 1.125,
    1.0625) every position, weight, product and partial sum is an exact float32 number.  random: normal x, flow uniform in +-1.5 max(H, W) -- zeros leaves
    the image, border clamps, reflection folds more than once -- with no coordinate near a rounding tie."""
    B, C, H, W = shape
    rng = np.random.default_rng(seed + 7919 * (B + 10 * C + 100 * H + 1000 * W) + (0 if family == 'exact' else 500))
    if family == 'exact':
        x = rng.integers(-8, 9, shape).astype(f32)
        flow = (rng.integers(-12, 13, (B, H, W, 2)) / 4.0).astype(f32)
    else:
        lim = 1.5 * max(H, W)
        x = rng.standard_normal(shape).astype(f32)
        flow = reject_ties(rng.uniform(-lim, lim, (B, H, W, 2)).astype(f32), rng, lim)
    return x, flow


def assert_exact_premise(x, flow, interp, padding, align, val):
    """The exact family's premise: the float32 coordinates are the real-number ones, and the result is a float32 number."""
    px, py = positions(flow)
    _, H, W, _ = flow.shape
    for p, n in ((px, W), (py, H)):
        i32, _, _ = coord(p, n, padding, align)
        i64 = p.astype(np.float64) * ((n - 1 if align else n) / max(n - 1, 1)) - (0.0 if align else 0.5)
        if padding == 'reflection':
            lo, span = (0.0, float(n - 1)) if align else (-0.5, float(n))
            if span > 0:
                r = np.fmod(np.abs(i64 - lo), 2 * span)
                i64 = np.where(r <= span, r, 2 * span - r) + lo
        if padding != 'zeros':
            i64 = np.clip(i64, 0.0, n - 1.0)
        assert (i32.astype(np.float64) == i64).all()
    assert (val.astype(f32).astype(np.float64) == val).all()


@functools.lru_cache(maxsize=None)
def case(shape, family, mode):
    """(x, flow, value, S, D) of a shape, family and mode (interp, padding, align), computed once per process; treat the arrays as read-only."""
    x, flow = make_inputs(shape, family)
    val, S, D = warp_ref(x, flow, *mode)
    if family == 'exact':
        assert_exact_premise(x, flow, *mode, val)
    elif mode[0] == 'nearest':
        assert (tie_distance(flow) > TIE_MARGIN).all()
    for a in (x, flow, val, S, D):
        a.setflags(write=False)
    return x, flow, val, S, D


def edge_inputs(shape, seed=3):
    """(x, flow, where): the random family with one NaN, one +inf and one 1e30 written into the flow of image 0; where = their (y, x, component)."""
    x, flow = make_inputs(shape, 'random', seed)
    _, _, H, W = shape
    where = {'nan': (1, 2, 0), 'inf': (H - 1, W - 2, 1), 'huge': (2, 0, 0)}
    flow = flow.copy()
    for k, v in (('nan', np.nan), ('inf', np.inf), ('huge', 1e30)):
        flow[(0,) + where[k]] = v
    return x, flow, where


def check(got, family, val, S, D, label=''):
    """Exact family: bitwise the helper; random family: within the per-element bound.  Prints the worst ratio."""
    got = np.asarray(got)
    assert got.shape == val.shape and got.dtype == f32
    if family == 'exact':
        ref32 = val.astype(f32)
        assert (ref32.astype(np.float64) == val).all()
        bad = int((got.view(np.uint32) != ref32.view(np.uint32)).sum())
        print(f'flow_warp {label}/exact: {bad} of {got.size} elements differ from the definition')
        assert bad == 0
    else:
        b = bound(S, D)
        err = np.abs(got.astype(np.float64) - val)
        assert np.isfinite(err).all()
        ratio = float(np.where(b > 0, err / np.maximum(b, 1e-300), np.where(err > 0, np.inf, 0.0)).max())
        print(f'flow_warp {label}/random: worst |got - ref| / bound = {ratio:.4f}')
        assert (err <= b).all(), ratio
