"""-m gpu: basicsr.archs.arch_util on the device.  cf_flow_warp (both kernel forms) per element against the definition restated in tests/warp_ref.py --
exact family bitwise, random family within BLEND_C 2^-24 S + D (derived there) -- cf_pixel_shuffle_nhwc bitwise, and the blocks against float64.

The bound of the two blocks, in the style of dcn_ref.bound.  A float32 convolution of n = cin * 9 terms with exact products differs from the real
sum by at most (n + 16) u S, u = 2^-24, S = sum |w| |in| + |bias| (n accumulations in any order; the 16 is slack for the bias and the epilogue).
ResidualBlockNoBN: t = conv1(x) carries e1 = (n + 16) u S1; ReLU is 1-Lipschitz, so r = relu(t) carries e1 too; conv2 of the computed r differs from
conv2 of the real r by at most sum |w2| e1 (the first bound carried through |w2|) and adds its own (n + 16) u S2, with S2 taken on |r| + e1;
the AXPY epilogue fl(fl(c2 * res_scale) + x) adds two roundings: u |res_scale c2| + u |out| <= 2 u (|res_scale c2| + |x|) to first order.
  |got - ref| <= |res_scale| ((n + 16) u S2 + sum |w2| e1) + 2 u (|res_scale c2| + |x|)
Upsample(2, 16) is one convolution followed by a pure data movement: (n + 16) u S, pixel-shuffled like the value.

Measured on an MI355X: the whole file 5.6 s, 87 tests, the slowest 2.9 s (ResidualBlockNoBN: its last lines run F.conv2d for a width the HIP convolution
does not cover, the first such call of a process), every other below 0.2 s.  Every exact-family case is bitwise in both layouts.  Worst |got - ref| / bound:
flow_warp bilinear 0.25 - 0.49 with align_corners (the blend bound alone), 0.02 - 0.23 without (the position term is slack for an implementation that takes
the definition's steps), nearest 0; ResidualBlockNoBN(64, 0.5) 0.0020, Upsample(2, 16) 0.0170, DCNv2Pack(32, 32, 3, deformable_groups 4) 0.0087."""
import logging

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dcn_ref
import warp_ref

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
MODE_IDS = ['-'.join((i, p, 'ac' if a else 'noac')) for i, p, a in warp_ref.MODES]


@pytest.fixture(scope='module')
def ops():
    from codeformer_amd import build as cf_build
    from codeformer_amd import ops
    cf_build.build()
    assert torch.cuda.is_available()
    return ops


@pytest.fixture(scope='module')
def au(ops):
    from basicsr.archs import arch_util
    return arch_util


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _warp(au, x, flow, mode, channels_last=False):
    x = _dev(x)
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
        assert x.stride(1) == 1
    with torch.no_grad():
        out = au.flow_warp(x, _dev(flow), *mode)
    assert out.shape == x.shape and out.is_contiguous(memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    return out.cpu().contiguous().numpy()


@pytest.mark.parametrize('mode', warp_ref.MODES, ids=MODE_IDS)
@pytest.mark.parametrize('family', warp_ref.FAMILIES)
@pytest.mark.parametrize('shape', [(2, 3, 5, 9), (1, 5, 3, 17)], ids=['2x3x5x9', '1x5x3x17'])
def test_flow_warp_nchw(au, shape, family, mode):
    x, flow, val, S, D = warp_ref.case(shape, family, mode)
    warp_ref.check(_warp(au, x, flow, mode), family, val, S, D, label='nchw ' + '-'.join(map(str, shape + mode)))


@pytest.mark.parametrize('mode', warp_ref.MODES, ids=MODE_IDS)
@pytest.mark.parametrize('family', warp_ref.FAMILIES)
def test_flow_warp_channels_last(au, family, mode):
    shape = (2, 8, 5, 9)
    x, flow, val, S, D = warp_ref.case(shape, family, mode)
    warp_ref.check(_warp(au, x, flow, mode, channels_last=True), family, val, S, D, label='nhwc ' + '-'.join(map(str, shape + mode)))


@pytest.mark.parametrize('mode', [('bilinear', 'zeros', True), ('bilinear', 'reflection', False), ('nearest', 'border', False)],
                         ids=['bilinear-zeros-ac', 'bilinear-reflection-noac', 'nearest-border-noac'])
def test_flow_warp_channels_last_over_several_workgroups(au, mode):
    """(1, 20, 33, 70): 2310 pixels x 5 float4s = 46 workgroups of 256 with a ragged last one, C no multiple of 16.  The planar form on the same input (ten
    workgroups of pixels x twenty one-channel chunks) must give the same bits: both evaluate one definition with every rounding fixed."""
    shape = (1, 20, 33, 70)
    x, flow = warp_ref.make_inputs(shape, 'random')
    val, S, D = warp_ref.warp_ref(x, flow, *mode)
    if mode[0] == 'nearest':
        assert (warp_ref.tie_distance(flow) > warp_ref.TIE_MARGIN).all()
    cl, planar = _warp(au, x, flow, mode, channels_last=True), _warp(au, x, flow, mode)
    warp_ref.check(cl, 'random', val, S, D, label='nhwc ' + '-'.join(map(str, shape + mode)))
    assert (cl.view(np.uint32) == planar.view(np.uint32)).all()


def test_flow_warp_zero_flow_and_layout_fallbacks(au):
    x = torch.randn(2, 6, 5, 9, device='cuda')
    zero = torch.zeros(2, 5, 9, 2, device='cuda')
    with torch.no_grad():
        assert (_bits(au.flow_warp(x, zero)) == _bits(x)).all()
        # C % 4 != 0 in channels_last, and a strided view: the planar form after a copy
        flow = (torch.rand(2, 5, 9, 2, device='cuda') - 0.5) * 6
        want = au.flow_warp(x, flow)
        assert (_bits(au.flow_warp(x.contiguous(memory_format=torch.channels_last), flow)) == _bits(want)).all()
        wide = torch.randn(2, 6, 5, 18, device='cuda')
        assert (_bits(au.flow_warp(wide[..., ::2], flow)) == _bits(au.flow_warp(wide[..., ::2].contiguous(), flow))).all()
    with pytest.raises(RuntimeError):
        au.flow_warp(x.clone().requires_grad_(), zero)
    with pytest.raises(TypeError):
        au.flow_warp(x.half(), zero.half())
    with pytest.raises(ValueError):
        au.flow_warp(x, zero, 'bicubic')


@pytest.mark.parametrize('padding', warp_ref.PADDINGS)
@pytest.mark.parametrize('channels_last', [False, True], ids=['nchw', 'nhwc'])
def test_flow_warp_non_finite_and_huge_flow(au, padding, channels_last):
    """One NaN, one +inf and one 1e30 in the flow: each fails the in-range test on the float32 coordinate (or is clamped / folded as a float32 first), so
    nothing is read for it; the output is the definition's everywhere -- 0 at the NaN in every padding mode -- and finite."""
    shape = (2, 8, 5, 9) if channels_last else (2, 3, 5, 9)
    x, flow, where = warp_ref.edge_inputs(shape)
    for interp in warp_ref.INTERPS:
        for align in (True, False):
            mode = (interp, padding, align)
            val, S, D = warp_ref.warp_ref(x, flow, *mode)
            got = _warp(au, x, flow, mode, channels_last)
            assert np.isfinite(got).all() and np.isfinite(val).all()
            y, xx, _ = where['nan']
            assert (got[0, :, y, xx] == 0).all() and (val[0, :, y, xx] == 0).all()
            if padding != 'border':                    # zeros: outside; reflection: the remainder of inf is NaN
                y, xx, _ = where['inf']
                assert (got[0, :, y, xx] == 0).all()
            if padding == 'zeros':
                y, xx, _ = where['huge']
                assert (got[0, :, y, xx] == 0).all()
            warp_ref.check(got, 'random', val, S, D, label=f'edge {"nhwc" if channels_last else "nchw"} ' + '-'.join(map(str, mode)))


@pytest.mark.parametrize('shape,s', [((2, 5, 7, 4 * 3), 2), ((1, 3, 4, 9 * 2), 3)], ids=['s2', 's3'])
def test_pixel_shuffle_nhwc(ops, au, shape, s):
    torch.manual_seed(s)
    x = torch.randn(shape)
    want = F.pixel_shuffle(x.permute(0, 3, 1, 2), s)               # NCHW view, on the CPU
    got = ops.pixel_shuffle_nhwc(x.cuda(), s)
    assert got.shape == (shape[0], shape[1] * s, shape[2] * s, shape[3] // (s * s))
    assert (_bits(got.permute(0, 3, 1, 2)) == _bits(want)).all()
    back = au.pixel_unshuffle(got.permute(0, 3, 1, 2).contiguous(), s)
    assert (_bits(back) == _bits(x.permute(0, 3, 1, 2))).all()
    assert (_bits(back) == _bits(au.pixel_unshuffle(want, s))).all()    # device and CPU formula: the same bits
    with pytest.raises(ValueError):
        ops.pixel_shuffle_nhwc(x.cuda(), 5)


def _conv_bound(n, S):
    return (n + 16) * U * S


def test_residual_block_no_bn(au):
    torch.manual_seed(5)
    m = au.ResidualBlockNoBN(64, res_scale=0.5).eval()
    m.conv1.bias.data.normal_()
    m.conv2.bias.data.normal_()
    x = torch.randn(1, 64, 20, 36)
    d = {k: v.detach().double() for k, v in m.state_dict().items()}
    xd = x.double()
    t = F.relu(F.conv2d(xd, d['conv1.weight'], d['conv1.bias'], 1, 1))
    c2 = F.conv2d(t, d['conv2.weight'], d['conv2.bias'], 1, 1)
    ref = xd + c2 * 0.5
    n = 64 * 9
    e1 = _conv_bound(n, F.conv2d(xd.abs(), d['conv1.weight'].abs(), d['conv1.bias'].abs(), 1, 1))
    S2 = F.conv2d(t + e1, d['conv2.weight'].abs(), d['conv2.bias'].abs(), 1, 1)
    b = 0.5 * (_conv_bound(n, S2) + F.conv2d(e1, d['conv2.weight'].abs(), None, 1, 1)) + 2 * U * (0.5 * c2.abs() + xd.abs())
    m = m.cuda()
    got = m(x.cuda())
    assert got.shape == x.shape and not got.requires_grad
    err = (got.cpu().double() - ref).abs()
    print(f'ResidualBlockNoBN(64, 0.5): worst |got - ref| / bound = {float((err / b).max()):.4f}')
    assert (err <= b).all()
    assert (_bits(got) == _bits(m(x.cuda()))).all()
    # a width the HIP convolution does not cover: the documented F.conv2d route, same function
    s = au.ResidualBlockNoBN(6, res_scale=0.5).eval()
    xs = torch.randn(1, 6, 7, 9)
    with torch.no_grad():
        want = s(xs)
    assert torch.allclose(s.cuda()(xs.cuda()).cpu(), want, atol=1e-5)


def test_upsample(au):
    torch.manual_seed(6)
    m = au.Upsample(2, 16).eval()
    m[0].bias.data.normal_()
    x = torch.randn(1, 16, 12, 20)
    w, bias = m[0].weight.detach().double(), m[0].bias.detach().double()
    ref = F.pixel_shuffle(F.conv2d(x.double(), w, bias, 1, 1), 2)
    b = F.pixel_shuffle(_conv_bound(16 * 9, F.conv2d(x.double().abs(), w.abs(), bias.abs(), 1, 1)), 2)
    got = m.cuda()(x.cuda())
    assert got.shape == (1, 16, 24, 40) and not got.requires_grad
    err = (got.cpu().double() - ref).abs()
    print(f'Upsample(2, 16): worst |got - ref| / bound = {float((err / b).max()):.4f}')
    assert (err <= b).all()
    m3 = au.Upsample(3, 16).eval()
    with torch.no_grad():
        want = m3(x)
    assert torch.allclose(m3.cuda()(x.cuda()).cpu(), want, atol=1e-4) and want.shape == (1, 16, 36, 60)


def test_dcnv2pack(ops, au):
    from basicsr.ops.dcn import modulated_deform_conv
    from basicsr.utils import get_root_logger
    torch.manual_seed(7)
    m = au.DCNv2Pack(32, 32, 3, padding=1, deformable_groups=4).cuda().eval()
    m.conv_offset.weight.data.normal_(0, 0.05)
    m.bias.data.normal_()
    x, feat = torch.randn(2, 32, 19, 23, device='cuda'), torch.randn(2, 32, 19, 23, device='cuda')
    assert ops.deform_conv2d_route(x.shape, m.weight.shape, m.groups, m.deformable_groups) == 'mfma'
    records = []

    class Keep(logging.Handler):
        def emit(self, record):
            records.append(record)
    logger, h = get_root_logger(), Keep(level=logging.WARNING)
    logger.addHandler(h)
    try:
        with torch.no_grad():
            got = m(x, feat)
            offset, mask = m.offset_mask(feat)
            ref = modulated_deform_conv(x, offset, mask, m.weight, m.bias, m.stride, m.padding, m.dilation, m.groups, m.deformable_groups)
            assert (_bits(got) == _bits(ref)).all() and records == []
            val, S = dcn_ref.deform_conv_ref(x.cpu().numpy(), offset.cpu().numpy(), m.weight.cpu().numpy(), mask.cpu().numpy(), m.bias.cpu().numpy(),
                                             (1, 1), (1, 1), (1, 1), 1, 4)
            err, b = np.abs(got.cpu().numpy().astype(np.float64) - val), dcn_ref.bound(m.weight.cpu().numpy(), S)
            print(f'DCNv2Pack(32, 32, 3, dg 4): worst |got - ref| / bound = {float((err / b).max()):.4f}')
            assert (err <= b).all()
            m.conv_offset.weight.zero_()              # (on the parameters themselves: the packed conv_offset weight follows their version)
            m.conv_offset.bias.zero_()
            m.conv_offset.bias[:2 * 4 * 9] = 60
            m(x, feat)
    finally:
        logger.removeHandler(h)
    assert len(records) == 1 and records[0].getMessage().startswith('Offset abs mean is ') and records[0].getMessage().endswith(', larger than 50.')
    with pytest.raises(RuntimeError):
        m(x, feat)                                     # grad enabled, parameters require grad
