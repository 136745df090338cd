"""Test helper: deformable convolution from its definition (numpy), the cases and the two input families of the dcn tests.

The reference's extension is CUDA-only, so no golden of it exists; this file restates the definition on its own:
  tap k = i*kw + j; deformable group d = c // (Cin/DG);
  h = float32(y*sh - ph + i*dh) + offset[b, (d*K + k)*2, y, x],  w = float32(x*sw - pw + j*dw) + offset[b, (d*K + k)*2 + 1, y, x]   (fp32)
  val = 0 unless h > -1 and w > -1 and h < H and w < W (on the fp32 values; false for NaN); else the bilinear sample, zeros outside:
  h0 = floor(h), lh = h - h0, hh = 1 - lh (same for w), corner weights hh*hw, hh*lw, lh*hw, lh*lw -- each ONE fp32 operation;
  out[b, o, y, x] = bias[o] + sum_{c in group of o, k} weight[o, c_local, i, j] * mask[b, d*K + k, y, x] * val.
Positions and the four corner weights are float32 exactly as above; everything after them is float64.  Next to the value the helper
returns S = |bias| + sum |weight| * |mask| * sum_i |w_i * v_i| per output element, the scale of the rounding-error bound
  |got - ref| <= (n + 16) * 2^-24 * S,   n = (Cin/G) * kh * kw
(first order: n fp32 accumulations in any order with exact products, plus about six roundings in the blend, the mask multiply and the
bias, for which the 16 is slack).
"""
import functools

import numpy as np

#        name       B  Cin Cout H   W   kernel  stride  padding dilation G  DG modulated route
CASES = {
    'mod_dg4': (2, 32, 48, 19, 23, (3, 3), (1, 1), (1, 1), (1, 1), 1, 4, True, 'mfma'),
    'v1_s2d2': (1, 16, 32, 17, 21, (3, 3), (2, 2), (2, 2), (2, 2), 1, 1, False, 'mfma'),
    'groups': (1, 32, 32, 12, 12, (3, 3), (1, 1), (1, 1), (1, 1), 2, 2, True, 'mfma'),
    'k1': (1, 16, 16, 9, 9, (1, 1), (1, 1), (0, 0), (1, 1), 1, 1, True, 'mfma'),
    'tiles': (1, 16, 80, 40, 40, (3, 3), (1, 1), (1, 1), (1, 1), 1, 2, True, 'mfma'),
    'odd': (1, 6, 5, 7, 9, (3, 2), (1, 2), (1, 0), (1, 1), 1, 3, False, 'general'),
    # the paths of the MFMA kernel that the cases above do not reach (appended: a case's seed is its index in this table)
    'reuse': (1, 32, 32, 10, 18, (3, 3), (1, 1), (1, 1), (1, 1), 1, 1, True, 'mfma'),       # a sample kept for the second slab: 36 of 72 gathers
    'reuse24': (1, 48, 16, 9, 17, (3, 3), (1, 1), (1, 1), (1, 1), 1, 2, True, 'mfma'),      # Cin/DG 24: two k4 lanes of a pixel reuse, two resample
    'straddle': (2, 96, 48, 7, 18, (3, 3), (1, 1), (1, 1), (1, 1), 2, 3, True, 'mfma'),     # deformable group 1 (channels 32..63) cut by the groups at 48
    'straddle2': (1, 96, 48, 6, 17, (2, 2), (1, 1), (1, 1), (1, 1), 3, 2, False, 'mfma'),   # groups cut by the deformable groups at 48; plain op, even kernel
    'steps2': (1, 16, 8, 9, 20, (1, 2), (1, 1), (0, 1), (1, 1), 1, 1, True, 'mfma'),        # two K steps: prologue and last step, no loop, no tail
    'steps3': (1, 16, 8, 9, 20, (3, 1), (1, 1), (1, 0), (1, 1), 1, 2, False, 'mfma'),       # three: one loop iteration and the tail
    'k7': (1, 16, 16, 9, 11, (7, 7), (1, 1), (3, 3), (1, 1), 1, 1, True, 'mfma'),           # 49 taps, the route's limit
    'asym': (2, 16, 24, 11, 21, (2, 3), (1, 2), (2, 0), (2, 1), 1, 4, True, 'mfma'),        # kh != kw, sh != sw, ph != pw, dh != dw
    'gtiles': (3, 32, 160, 9, 20, (3, 3), (1, 1), (1, 1), (1, 1), 2, 2, True, 'mfma'),      # 2 groups x 2 N tiles (the second 16 of 64 wide), B 3, ragged M tiles
}
FAMILIES = ('exact', 'random')
# the MFMA cases in which a thread keeps a sample across K slabs, and those in which none does (reuse_counts below; test_dcn_host.py pins both)
REUSE_CASES = ('reuse', 'reuse24', 'straddle', 'straddle2')
NO_REUSE_CASES = ('mod_dg4', 'v1_s2d2', 'groups', 'k1', 'tiles')
# One entry (b, c, y, x) of the input per property case: in the interior, in a corner of the image, and in the last channel of a deformable
# group -- in straddle / straddle2 of the deformable group that the convolution groups cut, so its channels feed two groups' outputs.  In each reuse
# case at least one of the three lies in a slab for which the MFMA kernel keeps the previous slab's sample (reused_channels; test_dcn_host.py).
PIXELS = {
    'reuse24': ((0, 30, 4, 8), (0, 47, 8, 16), (0, 23, 3, 5)),
    'straddle': ((1, 85, 3, 9), (0, 0, 0, 17), (1, 63, 4, 2)),
    'straddle2': ((0, 70, 2, 8), (0, 95, 5, 0), (0, 47, 3, 11)),
    'asym': ((1, 9, 5, 10), (0, 15, 10, 20), (1, 3, 6, 13)),
}


def reused_channels(cin, groups, dg):
    """The input channels whose gather keeps the previous slab's sample in the MFMA kernel: thread k4 of group g walks, inside a tap, the 16-channel
    slabs of the group; its float4 (channels c .. c + 3, c = g*cin_g + 4*k4 + 16*slab) lies in deformable group d = c // (Cin/DG), and the thread
    computes a new position, corner offsets and weights only when d or the tap has moved -- so from the second slab on it reuses wherever d stays."""
    cin_g, cpdg = cin // groups, cin // dg
    kept = set()
    for g in range(groups):
        for k4 in range(4):
            cur = None
            for slab in range(cin_g // 16):
                c = g * cin_g + 4 * k4 + 16 * slab
                if c // cpdg == cur:
                    kept.update(range(c, c + 4))
                cur = c // cpdg
    return kept


def reuse_counts(cin, groups, dg, taps):
    """(reused, gathers) of one pixel's four gather threads over all groups, by the kernel's own rule: a thread walks the taps and, inside a tap,
    the slabs, and resamples when `d != cur_d || tap != cur_tap`."""
    cin_g, cpdg = cin // groups, cin // dg
    reused = gathers = 0
    for g in range(groups):
        for k4 in range(4):
            cur_d = cur_tap = -1
            for tap in range(taps):
                for slab in range(cin_g // 16):
                    d = (g * cin_g + 4 * k4 + 16 * slab) // cpdg
                    reused += not (d != cur_d or tap != cur_tap)
                    gathers += 1
                    cur_d, cur_tap = d, tap
    assert reused == taps * len(reused_channels(cin, groups, dg)) // 4     # (a tap's first slab never reuses: the tap has moved)
    return reused, gathers


def case_reuse_counts(name):
    c = CASES[name]
    return reuse_counts(c[1], c[9], c[10], c[5][0] * c[5][1])


def out_hw(H, W, kernel, stride, padding, dilation):
    return ((H + 2 * padding[0] - (dilation[0] * (kernel[0] - 1) + 1)) // stride[0] + 1,
            (W + 2 * padding[1] - (dilation[1] * (kernel[1] - 1) + 1)) // stride[1] + 1)


def make_inputs(name, family, batch=None, seed=0):
    """dict(x, offset, weight, mask, bias, stride, padding, dilation, groups, dg) of float32 numpy arrays for a case.
    exact: x integers in [-8, 8], weight integers in [-4, 4], integer bias, offsets multiples of 1/4 in [-3, 3], mask in {0, .5, 1, 2}: every
    term is a multiple of 1/32 below 64 and every partial sum, in any order, is exact in fp32.
    random: normal x, weight scaled by (cin/g * kh * kw)^-1/2, offsets uniform in [-2.5, 2.5], mask = sigmoid of normals."""
    B, cin, cout, H, W, kernel, stride, padding, dilation, G, DG, modulated, _ = CASES[name]
    B = batch or B
    rng = np.random.default_rng(seed + 1000 * list(CASES).index(name) + (0 if family == 'exact' else 500))
    K = kernel[0] * kernel[1]
    Ho, Wo = out_hw(H, W, kernel, stride, padding, dilation)
    if family == 'exact':
        x = rng.integers(-8, 9, (B, cin, H, W)).astype(np.float32)
        weight = rng.integers(-4, 5, (cout, cin // G, *kernel)).astype(np.float32)
        offset = (rng.integers(-12, 13, (B, DG * 2 * K, Ho, Wo)) / 4.0).astype(np.float32)
        mask = rng.choice(np.array([0.0, 0.5, 1.0, 2.0], np.float32), (B, DG * K, Ho, Wo))
        bias = rng.integers(-5, 6, (cout,)).astype(np.float32)
    else:
        x = rng.standard_normal((B, cin, H, W)).astype(np.float32)
        weight = (rng.standard_normal((cout, cin // G, *kernel)) * (cin // G * K) ** -0.5).astype(np.float32)
        offset = rng.uniform(-2.5, 2.5, (B, DG * 2 * K, Ho, Wo)).astype(np.float32)
        mask = (1.0 / (1.0 + np.exp(-rng.standard_normal((B, DG * K, Ho, Wo))))).astype(np.float32)
        bias = rng.standard_normal((cout,)).astype(np.float32)
    if not modulated:
        mask = bias = None
    return dict(x=x, offset=offset, weight=weight, mask=mask, bias=bias, stride=stride, padding=padding, dilation=dilation, groups=G, dg=DG)


def n_terms(weight):
    return int(weight.shape[1] * weight.shape[2] * weight.shape[3])


def bound(weight, S):
    return (n_terms(weight) + 16) * 2.0 ** -24 * S


def deform_conv_ref(x, offset, weight, mask=None, bias=None, stride=(1, 1), padding=(0, 0), dilation=(1, 1), groups=1, dg=1):
    """(value, S), float64 arrays of shape (B, Cout, Ho, Wo)."""
    f32 = np.float32
    x, offset, weight = np.asarray(x, f32), np.asarray(offset, f32), np.asarray(weight, f32)
    B, C, H, W = x.shape
    cout, cin_g, kh, kw = weight.shape
    K, cpdg = kh * kw, C // dg
    Ho, Wo = out_hw(H, W, (kh, kw), stride, padding, dilation)
    assert offset.shape == (B, dg * 2 * K, Ho, Wo)
    col = np.zeros((B, C, K, Ho, Wo))       # mask * val
    cabs = np.zeros((B, C, K, Ho, Wo))      # |mask| * sum_i |w_i v_i|
    ys, xs = np.arange(Ho, dtype=np.int64)[:, None], np.arange(Wo, dtype=np.int64)[None, :]
    bi = np.arange(B)[:, None, None, None]
    for d in range(dg):
        chans = np.arange(d * cpdg, (d + 1) * cpdg)[None, :, None, None]
        for i in range(kh):
            for j in range(kw):
                k = i * kw + j
                with np.errstate(invalid='ignore', over='ignore'):
                    h = (ys * stride[0] - padding[0] + i * dilation[0]).astype(f32) + offset[:, (d * K + k) * 2]       # (B, Ho, Wo) float32
                    w = (xs * stride[1] - padding[1] + j * dilation[1]).astype(f32) + offset[:, (d * K + k) * 2 + 1]
                    ok = (h > f32(-1)) & (w > f32(-1)) & (h < f32(H)) & (w < f32(W))
                h, w = np.where(ok, h, f32(0)), np.where(ok, w, f32(0))
                h0f, w0f = np.floor(h), np.floor(w)
                lh, lw = h - h0f, w - w0f
                hh, hw = f32(1) - lh, f32(1) - lw
                assert lh.dtype == f32 and hh.dtype == f32
                h0, w0 = h0f.astype(np.int64), w0f.astype(np.int64)
                val, vabs = np.zeros((B, cpdg, Ho, Wo)), np.zeros((B, cpdg, Ho, Wo))
                for cy, cx, cw in ((h0, w0, hh * hw), (h0, w0 + 1, hh * lw), (h0 + 1, w0, lh * hw), (h0 + 1, w0 + 1, lh * lw)):
                    assert cw.dtype == f32
                    inside = ok & (cy >= 0) & (cy <= H - 1) & (cx >= 0) & (cx <= W - 1)
                    v = x[bi, chans, np.where(inside, cy, 0)[:, None], np.where(inside, cx, 0)[:, None]].astype(np.float64)
                    t = np.where(inside[:, None], cw.astype(np.float64)[:, None] * v, 0.0)
                    val += t
                    vabs += np.abs(t)
                m = np.ones((B, Ho, Wo)) if mask is None else np.asarray(mask, f32)[:, d * K + k].astype(np.float64)
                col[:, d * cpdg:(d + 1) * cpdg, k] = m[:, None] * val
                cabs[:, d * cpdg:(d + 1) * cpdg, k] = np.abs(m)[:, None] * vabs
    w64 = weight.astype(np.float64).reshape(groups, cout // groups, cin_g * K)
    out = np.einsum('gok,bgkyx->bgoyx', w64, col.reshape(B, groups, cin_g * K, Ho, Wo)).reshape(B, cout, Ho, Wo) + 0.0   # (a sum from +0: never -0)
    S = np.einsum('gok,bgkyx->bgoyx', np.abs(w64), cabs.reshape(B, groups, cin_g * K, Ho, Wo)).reshape(B, cout, Ho, Wo)
    if bias is not None:
        b64 = np.asarray(bias, f32).astype(np.float64).reshape(1, cout, 1, 1)
        out, S = out + b64, S + np.abs(b64)
    return out, S


@functools.lru_cache(maxsize=None)
def case(name, family):
    """(inputs, value, S) of a case, computed once per process and shared by the tests; treat the arrays as read-only."""
    inp = make_inputs(name, family)
    val, S = deform_conv_ref(**inp)
    for a in (val, S, *[v for v in inp.values() if isinstance(v, np.ndarray)]):
        a.setflags(write=False)
    return inp, val, S


@functools.lru_cache(maxsize=None)
def one_pixel_case(name, which):
    """(inputs, value, S, touched): the random family of a case with x zero except entry PIXELS[name][which], which holds 1.3.  S is the sum of the
    few terms that read the entry (+ |bias|); touched marks the outputs with such a term: everywhere else the result is the bias itself
    (+0 for the plain op), whatever the kernel does with the zeros."""
    inp = dict(case(name, 'random')[0])
    x = np.zeros_like(inp['x'])
    x[PIXELS[name][which]] = np.float32(1.3)
    inp['x'] = x
    val, S = deform_conv_ref(**dict(inp, bias=None))
    touched = S > 0
    if inp['bias'] is not None:
        b64 = inp['bias'].astype(np.float64).reshape(1, -1, 1, 1)
        val, S = val + b64, S + np.abs(b64)
    for a in (x, val, S, touched):
        a.setflags(write=False)
    return inp, val, S, touched


@functools.lru_cache(maxsize=None)
def nan_pixel_case(name):
    """(inputs, value, S): the random family of a case with a NaN at entry PIXELS[name][0] of x (x alone: offsets and mask stay as they are).
    value and S are NaN exactly where a sample reads the entry with a corner inside the image, for every output channel of its group."""
    inp = dict(case(name, 'random')[0])
    x = inp['x'].copy()
    x[PIXELS[name][0]] = np.nan
    inp['x'] = x
    with np.errstate(invalid='ignore'):
        val, S = deform_conv_ref(**inp)
    assert (np.isnan(val) == np.isnan(S)).all()
    for a in (x, val, S):
        a.setflags(write=False)
    return inp, val, S


def check_one_pixel(got, name, which, label=''):
    """The bound on every element, and bitwise the bias (+0 without one) wherever no sample reads the entry."""
    inp, val, S, touched = one_pixel_case(name, which)
    got = np.asarray(got)
    assert got.shape == val.shape and got.dtype == np.float32
    assert touched.any() and not touched.all()
    b = bound(inp['weight'], S)
    err = np.abs(got.astype(np.float64) - val)
    ratio = float((err[touched] / b[touched]).max())
    want = np.zeros(got.shape, np.float32) if inp['bias'] is None else np.ascontiguousarray(np.broadcast_to(inp['bias'].reshape(1, -1, 1, 1), got.shape))
    stray = int(((got.view(np.uint32) != want.view(np.uint32)) & ~touched).sum())
    print(f'dcn {label}{name} one pixel {PIXELS[name][which]}: {int(touched.sum())} of {got.size} outputs read it, worst |got - ref| / bound = {ratio:.4f}, '
          f'{stray} others differ from the bias')
    assert stray == 0
    assert (err <= b).all(), ratio


def check_nan_pixel(got, name, label=''):
    """The NaN outputs are the reference's; every other element is within the bound of the reference computed with the NaN in place."""
    inp, val, S = nan_pixel_case(name)
    got = np.asarray(got)
    assert got.shape == val.shape and got.dtype == np.float32
    want_nan = np.isnan(val)
    assert want_nan.any() and not want_nan.all()
    wrong = int((np.isnan(got) != want_nan).sum())
    b = bound(inp['weight'], np.where(want_nan, 0.0, S))
    err = np.where(want_nan, 0.0, np.abs(np.where(np.isnan(got), np.inf, got.astype(np.float64)) - np.where(want_nan, 0.0, val)))
    ratio = float((err[~want_nan] / np.maximum(b[~want_nan], 1e-300)).max())
    print(f'dcn {label}{name} NaN at {PIXELS[name][0]}: {100.0 * want_nan.mean():.1f} % of the outputs are NaN, {wrong} elements disagree on it, '
          f'worst |got - ref| / bound elsewhere = {ratio:.4f}')
    assert wrong == 0
    assert (err <= b).all(), ratio


def check(got, name, family, inp, val, S, label=''):
    """Exact family: bitwise equal to the helper; random family: within the per-element bound.  Prints the worst ratio."""
    got = np.asarray(got)
    assert got.shape == val.shape and got.dtype == np.float32
    if family == 'exact':
        ref32 = val.astype(np.float32)
        assert (ref32.astype(np.float64) == val).all()          # the family's premise: the exact result is an fp32 number
        bad = int((got.view(np.uint32) != ref32.view(np.uint32)).sum())
        print(f'dcn {label}{name}/exact: {bad} of {got.size} elements differ from the definition')
        assert bad == 0
    else:
        b = bound(inp['weight'], S)
        err = np.abs(got.astype(np.float64) - val)
        ratio = float((err / np.maximum(b, 1e-300)).max())
        print(f'dcn {label}{name}/random: worst |got - ref| / bound = {ratio:.4f} (n = {n_terms(inp["weight"])})')
        assert (err <= b).all(), ratio
