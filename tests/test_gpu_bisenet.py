"""-m gpu: BiSeNet on the device (csrc/cf_bisenet.hip and the existing convolution / squeeze-and-excitation kernels).

The yardstick rule: with e(x) = max|x - ref64| / max|ref64|, the device must satisfy e(device) <= 8 e(float32 reference), where the float32
reference is the reference module's own CPU forward (recorded in tests/golden/bisenet_ref.npz at seeded sample positions) and ref64 the same
module in float64.  Every measured ratio is printed before it is asserted.  The kernels are checked per element: bitwise where the definition
fixes every rounding (pool, scale_add_row, bilinear, argmax), against float64 with a bound from the number of roundings where it is a sum
(stem, pooled_fc).  All weights are seeded random ones: no trained parsing_bisenet.pth was run.

Measured on an MI355X (profiles/NOTES.md, "BiSeNet"): network ratios 1.55 .. 3.18 over the 27 taps; labels equal to the float64 labels on every
pixel, 0.012 % of the pixels at most below the gap; stem |err| / bound at most 0.025; folded upsample |err| / bound at most 0.006; pooled_fc
|err| / bound at most 0.017, the sigmoid's worst |err| 3.8e-7 at c 512, B 3 (pre-activation error through the slope; at c 128, where the 2^-22
term is most of the bound: 9.7e-8 at B 1, 1.4e-7 at B 3).
"""
import numpy as np
import pytest
import torch
from torch.nn import functional as F

import bisenet_ref as R
from _tools import _bits, _np, _yardstick

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24


@pytest.fixture(scope='module')
def lib():
    from codeformer_amd import build as cf_build
    cf_build.build()
    assert torch.cuda.is_available()
    from codeformer_amd import ops
    from codeformer_amd.facelib.parsing import bisenet
    return type('Lib', (), {'ops': ops, 'A': bisenet})


@pytest.fixture(scope='module')
def nets(lib):
    return {case: R.build(lib.A.BiSeNet, case).cuda() for case in R.CASES}


@pytest.fixture(scope='module')
def taps(nets):
    """Device forward of the three cases (six outputs and the three ResNet18 features), computed once."""
    return {case: R.run_taps(nets[case], R.case_input(case).cuda()) for case in R.CASES}


@pytest.fixture(scope='module')
def labels(nets):
    return {case: nets[case].parse_labels(R.case_input(case).cuda()) for case in R.CASES}


# ---- the network ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', list(R.CASES))
def test_network_taps_against_the_reference(taps, case):
    g = R.golden()
    c = R.CASES[case]
    for k in R.TAPS:
        v = taps[case][k]
        assert v.dtype == torch.float32 and v.is_contiguous() and v.shape[0] == c['batch']
        if k in R.OUTPUTS:
            assert tuple(v.shape[2:]) == c['hw'], (k, tuple(v.shape))
        _yardstick(f'network {case} {k}', R.sample(case, k, v), g[f'{case}_{k}_f32'], g[f'{case}_{k}_f64'])


def test_forward_without_feat_is_the_first_three(nets, taps):
    out = nets['square'](R.case_input('square').cuda())
    assert len(out) == 3
    for k, v in zip(R.OUTPUTS, out):
        assert tuple(v.shape[:2]) == (2, R.NUM_CLASS)
        assert np.array_equal(_bits(v), _bits(taps['square'][k])), k


@pytest.mark.parametrize('case', list(R.CASES))
def test_labels_against_the_float64_reference(taps, labels, case):
    """parse_labels equals the float64 labels wherever the float64 top-2 gap is at least 2 * 8 * max|f32 - f64| of `out`: the gap that a
    logit error at the gate (8 e(float32 reference) on each of the two logits) cannot close.  At most 1 % of the pixels may be left out."""
    g = R.golden()
    lab = _np(labels[case])
    assert lab.dtype == np.int64 and lab.shape == g[f'{case}_labels'].shape
    safe = g[f'{case}_gap'] >= 2 * 8 * float(g[f'{case}_out_err'])
    print(f'\nlabels {case}: {1 - safe.mean():.4%} of the pixels have a float64 gap below 16 max|f32 - f64| = {16 * float(g[f"{case}_out_err"]):.3e}; '
          f'device labels differ from float64 on {(lab != g[f"{case}_labels"]).mean():.4%} of all pixels')
    assert 1 - safe.mean() <= 0.01
    assert np.array_equal(lab[safe], g[f'{case}_labels'].astype(np.int64)[safe])
    # the fused kernel against the unfused output of the same device, wherever that output's two largest values differ
    out = _np(taps[case]['out'])
    distinct = R.top2_gap(out) > 0
    assert distinct.mean() > 0.99
    assert np.array_equal(lab[distinct], out.argmax(1)[distinct])


def test_rows_and_repeats_are_bitwise(nets, taps, labels):
    for case in ('square', 'batch'):
        x = R.case_input(case).cuda()
        again, one = R.run_taps(nets[case], x), R.run_taps(nets[case], x[:1])
        for k in R.TAPS:
            assert np.array_equal(_bits(again[k]), _bits(taps[case][k])), (case, k)
            assert np.array_equal(_bits(one[k]), _bits(taps[case][k][:1])), (case, k)
        assert torch.equal(nets[case].parse_labels(x), labels[case])
        assert torch.equal(nets[case].parse_labels(x[:1]), labels[case][:1])


# ---- the stem ------------------------------------------------------------------------------------------------------------------------
def _stem(lib, x, w, b):
    return _np(lib.ops.stem7x7s2(torch.from_numpy(x).cuda(), lib.ops.pack_stem7x7(torch.from_numpy(w).cuda()), torch.from_numpy(b).cuda()))


@pytest.mark.parametrize('shape', [(2, 3, 14, 18), (1, 3, 9, 7), (1, 3, 2, 2)])
def test_stem_per_element(lib, shape):
    """Against float64 per element: (K + 1) 2^-24 sum |w x| with K = 148 products in one chain; the + 1 pays for the bias addition, and the
    bias itself is not part of the sum."""
    rng = np.random.default_rng(sum(shape))
    x = rng.uniform(-1., 1., shape).astype(np.float32)
    w = (rng.normal(0., 1., (64, 3, 7, 7)) * np.sqrt(2. / 147)).astype(np.float32)
    b = rng.normal(0., 0.5, 64).astype(np.float32)
    got = _stem(lib, x, w, b)
    pre = R.stem_ref(x, w, b, relu=False)
    mag = R.stem_ref(np.abs(x), np.abs(w), np.zeros_like(b), relu=False)
    assert got.shape == pre.shape == (shape[0], (shape[2] - 1) // 2 + 1, (shape[3] - 1) // 2 + 1, 64)
    err = np.abs(got - np.maximum(pre, 0))
    bound = (148 + 1) * EPS * mag
    print(f'\nstem {shape}: worst |err| / bound {float((err / bound).max()):.4f}')
    assert (err <= bound).all()
    assert (got >= 0).all() and (got[pre < -bound] == 0).all() and (got > 0).any() and (got == 0).any()


@pytest.mark.parametrize('hw', [(14, 18), (9, 7)])
def test_stem_impulses_return_the_weights(lib, hw):
    """One 1.0 at a corner or the centre of one channel, zeros elsewhere, bias 0, positive weights: every output is a weight, bitwise, or
    zero.  Pins the tap order, the flip, the stride phase and the padding."""
    H, W = hw
    rng = np.random.default_rng(9)
    w = rng.uniform(0.5, 1.5, (64, 3, 7, 7)).astype(np.float32)
    b = np.zeros(64, np.float32)
    pos = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2)]
    x = np.zeros((len(pos) * 3, 3, H, W), np.float32)
    for i, (y, xx) in enumerate(pos):
        for c in range(3):
            x[i * 3 + c, c, y, xx] = 1.0
    got = _stem(lib, x, w, b)
    ho, wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    want = np.zeros((len(pos) * 3, ho, wo, 64), np.float32)
    for i, (y, xx) in enumerate(pos):
        for c in range(3):
            for oy in range(ho):
                for ox in range(wo):
                    ky, kx = y - 2 * oy + 3, xx - 2 * ox + 3     # the tap of output (oy, ox) that lies on the impulse
                    if 0 <= ky < 7 and 0 <= kx < 7:
                        want[i * 3 + c, oy, ox] = w[:, c, ky, kx]
    assert (want != 0).sum() > 0
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---- the pool ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', [4, 64])
@pytest.mark.parametrize('hw', [(1, 2), (5, 4), (8, 8), (7, 9)])
def test_maxpool3s2_bitwise(lib, hw, c):
    rng = np.random.default_rng(hw[0] * 100 + hw[1] + c)
    x = torch.from_numpy(rng.normal(0., 1., (2,) + hw + (c,)).astype(np.float32))
    x[1] = -x[1].abs() - 1.0          # all negative: zero padding would win every border window
    x[0, hw[0] // 2, hw[1] // 2, 1] = float('nan')
    want = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous()
    got = lib.ops.maxpool3s2(x.cuda())
    assert tuple(got.shape) == tuple(want.shape)
    assert int(torch.isnan(got).sum()) == int(torch.isnan(want).sum()) >= 1 and bool((got[1] < 0).all())
    assert np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(_bits(got), R.maxpool3s2_ref(x.numpy()).view(np.uint32))


# ---- pooled_fc -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('act', [None, 'relu', 'sigmoid'])
@pytest.mark.parametrize('c', [128, 512])
@pytest.mark.parametrize('batch', [1, 3])
def test_pooled_fc(lib, batch, c, act):
    """Pre-activation bound (c + 2) 2^-24 (sum |w p| + |b|): c products in one chain and the bias.  The sigmoid's slope is at most 1/4, so
    its outputs get a quarter of that, plus 2^-22 for the two roundings of 1 / (1 + e) and an expf a couple of ulp off (outputs <= 1)."""
    n = 128
    rng = np.random.default_rng(batch * 1000 + c)
    p = rng.normal(0., 1., (batch, c)).astype(np.float32)
    w = (rng.normal(0., 1., (n, c)) / np.sqrt(c)).astype(np.float32)
    b = rng.normal(0., 0.5, n).astype(np.float32)
    dev = [torch.from_numpy(a).cuda() for a in (p, w, b)]
    got = _np(lib.ops.pooled_fc(*dev, act=act))
    want, mag = R.pooled_fc_ref(p, w, b, act)
    bound = (c + 2) * EPS * mag
    if act == 'sigmoid':
        bound = bound / 4 + 2.0 ** -22
    err = np.abs(got - want)
    print(f'\npooled_fc B {batch} c {c} {act}: worst |err| / bound {float((err / bound).max()):.4f}, worst |err| {float(err.max()):.3e}')
    assert got.shape == (batch, n) and (err <= bound).all()
    if act == 'relu':
        assert (got >= 0).all() and (got == 0).any()
    for r in range(batch):
        alone = lib.ops.pooled_fc(dev[0][r:r + 1].contiguous(), dev[1], dev[2], act=act)
        assert np.array_equal(_bits(alone)[0], got[r].view(np.uint32))


def test_scale_add_row_bitwise(lib):
    rng = np.random.default_rng(3)
    x = rng.normal(0., 3., (3, 5, 7, 128)).astype(np.float32)
    g, r = rng.uniform(0., 1., (3, 128)).astype(np.float32), rng.normal(0., 2., (3, 128)).astype(np.float32)
    got = lib.ops.scale_add_row(*[torch.from_numpy(a).cuda() for a in (x, g, r)])
    want = R.scale_add_row_ref(x, g, r)
    fused = (x.astype(np.float64) * g[:, None, None] + r[:, None, None]).astype(np.float32)
    assert (want != fused).any()      # (the inputs can tell a contracted multiply-add from the two roundings)
    assert np.array_equal(_bits(got), want.view(np.uint32))


# ---- bilinear ------------------------------------------------------------------------------------------------------------------------
RESIZE = [((2, 2), (16, 16)), ((4, 3), (32, 24)), ((1, 1), (8, 8)), ((8, 8), (8, 8))]


def _logits(hw, seed, batch=2, ld=20):
    return np.random.default_rng(seed).normal(0., 4., (batch,) + hw + (ld,)).astype(np.float32)


@pytest.mark.parametrize('src,dst', RESIZE)
def test_resize_bilinear_ac_bitwise(lib, src, dst):
    x = _logits(src, src[0] * 10 + dst[1])
    got = _np(lib.ops.resize_bilinear_ac(torch.from_numpy(x).cuda(), dst, c=19))
    want = R.resize_bilinear_ac_ref(x, 19, dst)
    assert got.shape == (2, 19) + dst
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    nchw = np.ascontiguousarray(x[..., :19].transpose(0, 3, 1, 2))
    if src == dst:
        assert np.array_equal(got.view(np.uint32), nchw.view(np.uint32))
    for oy, iy in ((0, 0), (dst[0] - 1, src[0] - 1)):
        for ox, ix in ((0, 0), (dst[1] - 1, src[1] - 1)):
            assert np.array_equal(got[:, :, oy, ox].view(np.uint32), nchw[:, :, iy, ix].view(np.uint32)), (oy, ox)
    t = F.interpolate(torch.from_numpy(nchw).double(), dst, mode='bilinear', align_corners=True).numpy()
    assert np.abs(got - t).max() <= 8 * EPS * np.abs(x).max()


@pytest.mark.parametrize('src,dst', RESIZE)
def test_resize_argmax_is_the_argmax_of_the_unfused_output(lib, src, dst):
    x = _logits(src, src[1] * 10 + dst[0])
    x[0, 0, 0, 5] = x[0, 0, 0, 11] = 50.0      # an exact tie at a source corner, which the corner output copies: the lower index wins
    x[1, -1, -1, 0] = x[1, -1, -1, 18] = 60.0
    xd = torch.from_numpy(x).cuda()
    full = _np(lib.ops.resize_bilinear_ac(xd, dst, c=19))
    want = full.argmax(1)                      # (numpy: the first of equal maxima)
    got = lib.ops.resize_bilinear_ac_argmax(xd, dst, c=19)
    assert got.dtype == torch.int64 and tuple(got.shape) == (2,) + dst
    assert np.array_equal(_np(got), want)
    assert _np(got)[0, 0, 0] == 5 and _np(got)[1, -1, -1] == 0
    assert (np.sort(full, 1)[:, -1] == np.sort(full, 1)[:, -2]).any()
    x[..., 19] = 1e30                          # the padding channel is never read
    assert np.array_equal(_np(lib.ops.resize_bilinear_ac_argmax(torch.from_numpy(x).cuda(), dst, c=19)), want)


# ---- what the network's parts refuse, and the dispatcher rule the network needed --------------------------------------------------------
def test_parts_have_no_device_forward_of_their_own(nets):
    net = nets['square']
    x = torch.zeros(1, 128, 8, 8, device='cuda')
    for part in (net.cp, net.cp.arm16, net.cp.conv_avg, net.ffm, net.conv_out16, net.cp.resnet.layer1[0]):
        with pytest.raises(NotImplementedError, match='no device forward of its own'):
            part(x, x) if part is net.ffm else part(x)


@pytest.mark.parametrize('hw', [(8, 8), (16, 8), (8, 24)])
def test_folded_upsample_conv_on_a_source_off_the_dense_grid(lib, hw):
    """conv2d(upsample=True) with fp32 operands and 128 output channels on a source whose width is 8 mod 16: the output lies on the 16-pixel
    grid, the source off the dense kernel's 8 x 16 tiles, and the dispatcher sends it to the general instantiation (conv_head16 on a 128x128
    face).  Per element against float64: an output is one chain of 4 * 128 products of folded taps, each the sum of up to four weights (three
    more roundings), plus the bias: (512 + 1 + 3) 2^-24 (sum |w| |x| + |b|).  Row 1 of the batch is bitwise the call on it alone."""
    rng = np.random.default_rng(hw[0] + hw[1])
    x = torch.from_numpy(rng.normal(0., 1., (2,) + hw + (128,)).astype(np.float32))
    w = torch.from_numpy((rng.normal(0., 1., (128, 128, 3, 3)) / np.sqrt(1152.)).astype(np.float32))
    b = torch.from_numpy(rng.normal(0., 0.5, 128).astype(np.float32))
    pw = lib.ops.pack_weight(w.cuda(), b.cuda(), up2x=True)
    got = lib.ops.conv2d(x.cuda(), pw, upsample=True)
    assert tuple(got.shape) == (2, 2 * hw[0], 2 * hw[1], 128)

    def ref(x_, w_, b_):
        up = F.interpolate(x_.double().permute(0, 3, 1, 2), scale_factor=2, mode='nearest')
        return F.conv2d(up, w_.double(), b_.double(), padding=1).permute(0, 2, 3, 1).numpy()
    err = np.abs(_np(got) - ref(x, w, b))
    bound = (512 + 1 + 3) * EPS * ref(x.abs(), w.abs(), b.abs())
    print(f'\nfolded upsample {hw}: worst |err| / bound {float((err / bound).max()):.4f}')
    assert (err <= bound).all()
    alone = lib.ops.conv2d(x[1:].cuda(), pw, upsample=True)
    assert np.array_equal(_bits(alone), _bits(got[1:]))
