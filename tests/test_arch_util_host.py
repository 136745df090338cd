"""basicsr.archs.arch_util on the CPU: the module surface, flow_warp's float32 formula against the definition restated in tests/warp_ref.py
(exact family bitwise, random family within its bound), the shape ops, and DCNv2Pack on the CPU formula of the deformable convolution."""
import logging

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import warp_ref

NAMES = ['default_init_weights', 'make_layer', 'ResidualBlockNoBN', 'Upsample', 'flow_warp', 'resize_flow', 'pixel_unshuffle', 'DCNv2Pack',
         'trunc_normal_', 'to_1tuple', 'to_2tuple', 'to_3tuple', 'to_4tuple', 'to_ntuple']     # the public names of the reference's file
SHAPE = (2, 3, 5, 9)
MODE_IDS = ['-'.join((i, p, 'ac' if a else 'noac')) for i, p, a in warp_ref.MODES]


@pytest.fixture(scope='module')
def au():
    from basicsr.archs import arch_util
    return arch_util


def _t(a):
    return torch.from_numpy(np.array(a))


def _bits(t):
    return t.detach().contiguous().numpy().view(np.uint32)


def test_module_surface(au):
    import basicsr.archs
    import codeformer_amd.archs.arch_util as impl
    assert sorted(impl.__all__) == sorted(NAMES)
    for n in NAMES + ['_ntuple', '_no_grad_trunc_normal_']:
        assert getattr(au, n) is getattr(impl, n), n
    from basicsr.archs.arch_util import default_init_weights, make_layer, pixel_unshuffle  # noqa: F401  (rrdbnet_arch.py's first line)
    assert not any(k in NAMES for k in basicsr.archs.ARCH_REGISTRY.keys())                 # a helper module, not an arch: nothing of it is registered
    assert au.to_2tuple(3) == (3, 3) and au.to_2tuple((1, 2)) == (1, 2) and au.to_4tuple(0) == (0, 0, 0, 0) and au.to_1tuple(5) == (5,)
    assert au.to_3tuple('ab') == 'ab' and au.to_ntuple(5)(1) == (1,) * 5


def test_state_dict_keys_and_shapes(au):
    def shapes(m):
        return {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert shapes(au.ResidualBlockNoBN(16)) == {'conv1.weight': (16, 16, 3, 3), 'conv1.bias': (16,), 'conv2.weight': (16, 16, 3, 3), 'conv2.bias': (16,)}
    assert shapes(au.Upsample(4, 8)) == {'0.weight': (32, 8, 3, 3), '0.bias': (32,), '2.weight': (32, 8, 3, 3), '2.bias': (32,)}
    assert shapes(au.Upsample(3, 8)) == {'0.weight': (72, 8, 3, 3), '0.bias': (72,)}
    assert shapes(au.DCNv2Pack(16, 8, 3, padding=1, deformable_groups=2)) == {
        'weight': (8, 16, 3, 3), 'bias': (8,), 'conv_offset.weight': (54, 16, 3, 3), 'conv_offset.bias': (54,)}
    up = au.Upsample(4, 8)
    assert [type(m).__name__ for m in up] == ['Conv2d', 'PixelShuffle', 'Conv2d', 'PixelShuffle'] and isinstance(up, torch.nn.Sequential)
    with pytest.raises(ValueError, match='scale 5 is not supported. Supported scales: 2\\^n and 3.'):
        au.Upsample(5, 8)


def test_init_helpers(au):
    torch.manual_seed(0)
    conv, lin, bn = torch.nn.Conv2d(8, 8, 3), torch.nn.Linear(16, 4), torch.nn.BatchNorm2d(4)
    torch.manual_seed(1)
    au.default_init_weights([conv, torch.nn.Sequential(lin, bn)], scale=0.1, bias_fill=0.25)
    torch.manual_seed(1)
    w_conv = torch.nn.init.kaiming_normal_(torch.empty(8, 8, 3, 3)) * 0.1
    w_lin = torch.nn.init.kaiming_normal_(torch.empty(4, 16)) * 0.1
    assert torch.equal(conv.weight, w_conv) and torch.equal(lin.weight, w_lin) and (bn.weight == 1).all()
    for m in (conv, lin, bn):
        assert (m.bias == 0.25).all()
    au.default_init_weights(conv)                      # a single module, default scale 1 and bias 0
    assert (conv.bias == 0).all()
    torch.manual_seed(2)
    blk = au.ResidualBlockNoBN(8)                      # default_init_weights at 0.1: std = 0.1 * sqrt(2 / 72)
    assert (blk.conv1.bias == 0).all() and abs(float(blk.conv1.weight.detach().std()) / (0.1 * (2 / 72) ** 0.5) - 1) < 0.2
    layers = au.make_layer(au.ResidualBlockNoBN, 3, num_feat=8, res_scale=0.5)
    assert len(layers) == 3 and all(isinstance(m, au.ResidualBlockNoBN) and m.res_scale == 0.5 for m in layers)
    t = au.trunc_normal_(torch.empty(4000), mean=0.5, std=2.0, a=-1.0, b=1.5)
    assert float(t.min()) >= -1.0 and float(t.max()) <= 1.5 and t.std() > 0.3


@pytest.mark.parametrize('mode', warp_ref.MODES, ids=MODE_IDS)
@pytest.mark.parametrize('family', warp_ref.FAMILIES)
def test_flow_warp_matches_the_definition(au, family, mode):
    x, flow, val, S, D = warp_ref.case(SHAPE, family, mode)
    got = au.flow_warp(_t(x), _t(flow), *mode)
    warp_ref.check(got.numpy(), family, val, S, D, label='cpu ' + '-'.join(map(str, mode)))


@pytest.mark.parametrize('mode', warp_ref.MODES, ids=MODE_IDS)
def test_flow_warp_is_grid_sample_of_the_reference_arithmetic_where_that_is_exact(au, mode):
    """The exact family through the reference's own steps -- mesh grid + flow, 2 v / max(n-1, 1) - 1, F.grid_sample: with n - 1 a power of two and
    positions on a grid of 1/4 the normalise / un-normalise round trip is exact, so the cancelled form must give the same bits."""
    x, flow, _, _, _ = warp_ref.case(SHAPE, 'exact', mode)
    x, flow = _t(x), _t(flow)
    _, _, h, w = x.shape
    gy, gx = torch.meshgrid(torch.arange(0, h).type_as(x), torch.arange(0, w).type_as(x), indexing='ij')
    v = torch.stack((gx, gy), 2).float() + flow
    grid = torch.stack((2.0 * v[..., 0] / max(w - 1, 1) - 1.0, 2.0 * v[..., 1] / max(h - 1, 1) - 1.0), dim=3)
    ref = F.grid_sample(x, grid, mode=mode[0], padding_mode=mode[1], align_corners=mode[2])
    got = au.flow_warp(x, flow, *mode)
    assert (got == ref).all()


def test_flow_warp_zero_flow_is_the_identity(au):
    x = torch.randn(2, 3, 5, 9)
    for interp in warp_ref.INTERPS:
        for padding in warp_ref.PADDINGS:
            assert (_bits(au.flow_warp(x, torch.zeros(2, 5, 9, 2), interp, padding, True)) == _bits(x)).all()
    assert (_bits(au.flow_warp(x, torch.zeros(2, 5, 9, 2))) == _bits(x)).all()       # the defaults: bilinear, zeros, align_corners=True


@pytest.mark.parametrize('mode', warp_ref.MODES, ids=MODE_IDS)
def test_flow_warp_on_a_single_column(au, mode):
    """W = 1: max(W - 1, 1) keeps the ratio finite (0 with align_corners, 1 without)."""
    shape = (1, 2, 3, 1)
    for family in warp_ref.FAMILIES:
        x, flow = warp_ref.make_inputs(shape, family)
        val, S, D = warp_ref.warp_ref(x, flow, *mode)
        if family == 'exact':
            warp_ref.assert_exact_premise(x, flow, *mode, val)
        warp_ref.check(au.flow_warp(_t(x), _t(flow), *mode).numpy(), family, val, S, D, label='cpu column ' + '-'.join(map(str, mode)))


@pytest.mark.parametrize('mode', warp_ref.MODES, ids=MODE_IDS)
def test_flow_warp_nan_flow_gives_zero_at_that_pixel_only(au, mode):
    x, flow, _, _, _ = warp_ref.case(SHAPE, 'exact', mode)
    x = np.abs(x) + 1                                   # no zero in x: a 0 in the output can only come from the rule
    bad = flow.copy()
    bad[1, 2, 4, 0] = np.nan
    clean, got = au.flow_warp(_t(x), _t(flow), *mode), au.flow_warp(_t(x), _t(bad), *mode)
    assert (got[1, :, 2, 4] == 0).all()
    keep = torch.ones(got.shape, dtype=torch.bool)
    keep[1, :, 2, 4] = False
    assert (_bits(got)[keep.numpy()] == _bits(clean)[keep.numpy()]).all() and torch.isfinite(got).all()
    val, _, _ = warp_ref.warp_ref(x, bad, *mode)
    assert (got.numpy().astype(np.float64) == val).all()


def test_flow_warp_argument_errors(au):
    x, flow = torch.zeros(1, 2, 4, 5), torch.zeros(1, 4, 5, 2)
    with pytest.raises(ValueError):
        au.flow_warp(x, flow, 'bicubic')
    with pytest.raises(ValueError):
        au.flow_warp(x, flow, 'bilinear', 'wrap')
    with pytest.raises(ValueError):
        au.flow_warp(x, torch.zeros(2, 4, 5, 2))
    with pytest.raises(ValueError):
        au.flow_warp(x, torch.zeros(1, 4, 5, 3))
    with pytest.raises(TypeError):
        au.flow_warp(x.double(), flow.double())
    with pytest.raises(TypeError):
        au.flow_warp(x.half(), flow.half())
    with pytest.raises(AssertionError):
        au.flow_warp(x, torch.zeros(1, 5, 4, 2))       # the reference's own size assert
    from codeformer_amd import ops
    with pytest.raises(ValueError):
        ops.pixel_shuffle_nhwc(torch.zeros(1, 2, 2, 6), 2)
    with pytest.raises(TypeError):
        ops.pixel_shuffle_nhwc(torch.zeros(1, 2, 2, 8).half(), 2)


def test_pixel_unshuffle_round_trip(au):
    x = torch.randn(2, 3, 12, 18)
    for s in (2, 3):
        y = au.pixel_unshuffle(x, s)
        assert y.shape == (2, 3 * s * s, 12 // s, 18 // s)
        assert (_bits(F.pixel_shuffle(y, s)) == _bits(x)).all()
        assert y[1, (2 * s + 1) * s + 0, 3, 4] == x[1, 2, 3 * s + 1, 4 * s]
    with pytest.raises(AssertionError):
        au.pixel_unshuffle(x, 5)


def test_resize_flow(au):
    flow = torch.randn(2, 2, 6, 8)
    keep = flow.clone()
    for size_type, sizes, (oh, ow) in (('ratio', [0.5, 1.5], (3, 12)), ('shape', [9, 4], (9, 4))):
        for interp, ac in (('bilinear', False), ('bilinear', True), ('nearest', None)):
            got = au.resize_flow(flow, size_type, sizes, interp, ac)
            scaled = flow.clone()
            scaled[:, 0] *= ow / 8
            scaled[:, 1] *= oh / 6
            ref = F.interpolate(scaled, size=(oh, ow), mode=interp, align_corners=ac)
            assert got.shape == (2, 2, oh, ow) and torch.equal(got, ref)
    assert torch.equal(flow, keep)                     # the input is left alone
    with pytest.raises(ValueError, match='Size type should be ratio or shape'):
        au.resize_flow(flow, 'scale', [2, 2])


def test_residual_block_host_formula(au):
    torch.manual_seed(3)
    m = au.ResidualBlockNoBN(16, res_scale=0.5).eval()
    m.conv1.bias.data.normal_()
    m.conv2.bias.data.normal_()
    x = torch.randn(2, 16, 7, 9)
    with torch.no_grad():
        got = m(x)
        d = {k: v.double() for k, v in m.state_dict().items()}
        t = F.relu(F.conv2d(x.double(), d['conv1.weight'], d['conv1.bias'], 1, 1))
        c2 = F.conv2d(t, d['conv2.weight'], d['conv2.bias'], 1, 1)
        ref = x.double() + c2 * 0.5
        # float32 convolutions of 144 terms each: (n + 16) 2^-24 S per conv, the first carried through |w2| (derivation: test_gpu_arch_util.py)
        S1 = F.conv2d(x.double().abs(), d['conv1.weight'].abs(), d['conv1.bias'].abs(), 1, 1)
        e1 = 160 * 2.0 ** -24 * S1
        S2 = F.conv2d(t + e1, d['conv2.weight'].abs(), d['conv2.bias'].abs(), 1, 1)
        e2 = 160 * 2.0 ** -24 * S2 + F.conv2d(e1, d['conv2.weight'].abs(), None, 1, 1)
        b = 0.5 * e2 + 2 * 2.0 ** -24 * (0.5 * c2.abs() + x.double().abs())
    assert ((got.double() - ref).abs() <= b).all()
    assert m(x.requires_grad_()).requires_grad          # the CPU path is plain torch: autograd works there


def _captured(logger):
    records = []

    class H(logging.Handler):
        def emit(self, record):
            records.append(record)
    h = H(level=logging.WARNING)
    logger.addHandler(h)
    return records, h


def test_dcnv2pack_on_the_cpu(au):
    from basicsr.ops.dcn import modulated_deform_conv
    from basicsr.utils import get_root_logger
    torch.manual_seed(4)
    m = au.DCNv2Pack(16, 8, 3, padding=1, deformable_groups=2).eval()
    m.conv_offset.weight.data.normal_(0, 0.05)
    m.bias.data.normal_()
    x, feat = torch.randn(2, 16, 6, 7), torch.randn(2, 16, 6, 7)
    logger = get_root_logger()
    records, h = _captured(logger)
    try:
        with torch.no_grad():
            got = m(x, feat)
            offset, mask = m.offset_mask(feat)
            assert offset.shape == (2, 36, 6, 7) and mask.shape == (2, 18, 6, 7)
            ref = modulated_deform_conv(x, offset, mask, m.weight, m.bias, m.stride, m.padding, m.dilation, m.groups, m.deformable_groups)
            assert (_bits(got) == _bits(ref)).all()
            assert not torch.equal(got, m(x, x))                       # the offsets come from feat, not from x
            assert records == []
            m.conv_offset.weight.data.zero_()
            m.conv_offset.bias.data.zero_()
            m(x, feat)
            assert records == []                                        # zero offsets: no warning
            m.conv_offset.bias.data[:2 * 2 * 9] = 60
            m(x, feat)
    finally:
        logger.removeHandler(h)
    assert len(records) == 1 and records[0].levelno == logging.WARNING
    msg = records[0].getMessage()
    assert msg.startswith('Offset abs mean is ') and '60' in msg and msg.endswith(', larger than 50.')


def test_grad_is_refused(au):
    x, flow = torch.randn(1, 2, 4, 5), torch.zeros(1, 4, 5, 2)
    with pytest.raises(RuntimeError):
        au.flow_warp(x.clone().requires_grad_(), flow)
    with pytest.raises(RuntimeError):
        au.flow_warp(x, flow.clone().requires_grad_())
    with torch.no_grad():
        au.flow_warp(x.clone().requires_grad_(), flow)
    m = au.DCNv2Pack(16, 8, 3, padding=1)
    xx = torch.randn(1, 16, 5, 5)
    with pytest.raises(RuntimeError):
        m(xx, xx)                                      # grad enabled, parameters require grad
    with torch.no_grad():
        assert m(xx, xx).shape == (1, 8, 5, 5)
