"""-m gpu: VGGFeatureExtractor, PerceptualLoss and the perceptual metric on the device (csrc/cf_vgg.hip and the existing 3x3 convolutions).

The yardstick rule: with e(x) = max|x - ref64| / max|ref64|, the device must satisfy e(device) <= 8 e(float32 reference), where the float32
reference is the reference module's own CPU forward (recorded in tests/golden/vgg_ref.npz at seeded sample positions) or torch's CPU float32
result, and ref64 the same in float64.  The margin of 8 covers one extra rounding per folded weight and another summation order, through up
to 16 stacked convolutions.  A PerceptualLoss output is one float32 number: there e(float32 reference) counts as at least 2^-24 (see
test_vgg_host.py).  Every measured ratio is printed before it is asserted.  Everything else is bitwise or exact.

Measured on an MI355X: see profiles/NOTES.md, "VGG / perceptual".
"""
import numpy as np
import pytest
import torch
from torch.nn import functional as F

import vgg_ref as R
from _tools import _bits, _np, _yardstick

pytestmark = pytest.mark.gpu
HALF_ULP = 2.0 ** -24


@pytest.fixture(scope='module')
def lib():
    from codeformer_amd import build as cf_build
    cf_build.build()
    assert torch.cuda.is_available()
    from codeformer_amd import losses, metrics, ops
    from codeformer_amd.archs import vgg_arch
    return type('Lib', (), {'M': metrics, 'ops': ops, 'A': vgg_arch, 'LS': losses})


@pytest.fixture(scope='module')
def nets(lib):
    return {case: R.build(lib.A.VGGFeatureExtractor, case).cuda() for case in R.CASES}


@pytest.fixture(scope='module')
def taps(nets):
    """Device forward of the three cases, computed once."""
    return {case: nets[case](R.case_input(case).cuda()) for case in R.CASES}


# ---- the network ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', list(R.CASES))
def test_network_taps_against_the_reference(taps, case):
    g = R.golden()
    out = taps[case]
    assert list(out) == list(g[f'out_keys_{case}'])
    assert [','.join(str(n) for n in v.shape) for v in out.values()] == list(g[f'out_shapes_{case}'])
    for k, v in out.items():
        assert v.dtype == torch.float32 and v.is_contiguous()
        _yardstick(f'network {case} {k}', R.sample(case, k, v), g[f'{case}_{k}_f32'], g[f'{case}_{k}_f64'])


def test_network_rows_and_repeats_are_bitwise(nets, taps):
    for case in ('grid', 'odd'):
        x = R.case_input(case).cuda()
        again = nets[case](x)
        one = nets[case](x[1:2])
        for k in taps[case]:
            assert np.array_equal(_bits(again[k]), _bits(taps[case][k])), (case, k)
            assert np.array_equal(_bits(one[k]), _bits(taps[case][k][1:2])), (case, k)


def test_features_nhwc_is_forward_without_the_layout_change(nets, taps):
    f = nets['odd'].features_nhwc(R.case_input('odd').cuda())
    for k, v in f.items():
        assert np.array_equal(_bits(v.permute(0, 3, 1, 2)), _bits(taps['odd'][k])), k


def test_a_pre_bn_conv_tap_of_a_bn_type(lib):
    """convX_Y of a _bn type is the value BEFORE the BatchNorm: a launch of its own with the unfolded weight."""
    net = R.fill_state(lib.A.VGGFeatureExtractor(['conv1_1', 'bn1_1', 'pool1'], 'vgg11_bn'), 5)
    x = R.case_input('odd')
    with torch.no_grad():
        f32, f64 = net(x), net.double()(x.double())
    dev = net.float().cuda()(x.cuda())
    assert list(dev) == ['conv1_1', 'bn1_1', 'pool1']
    for k in dev:
        _yardstick(f'vgg11_bn {k}', _np(dev[k]), _np(f32[k]), _np(f64[k]))


def test_winograd_f43_switch_runs_and_stays_close(lib, nets, taps):
    """The opt-in F(4x4,3x3) route (its measured ratios stand in profiles/NOTES.md): same keys and shapes, and an error of the order of
    float32 rounding -- 1e-4 of the largest value is a hundred times what either route shows, and far below a wrong tile or tap."""
    net = R.build(lib.A.VGGFeatureExtractor, 'grid').cuda()
    net.winograd_f43 = True
    g = R.golden()
    out = net(R.case_input('grid').cuda())
    differs = False
    for k, v in out.items():
        e = R.rel_err(R.sample('grid', k, v), g[f'grid_{k}_f64'])
        e_ref = R.rel_err(g[f'grid_{k}_f32'], g[f'grid_{k}_f64'])
        print(f'\ngrid {k} with winograd_f43: e(device) {e:.3e}  ratio {e / e_ref:.3f}')
        assert e < 1e-4, (k, e)
        differs = differs or not np.array_equal(_bits(v), _bits(taps['grid'][k]))
    assert differs     # (conv1_2 at 64x64 is on the F(4,3) grid: the switch did something)


def test_winograd_f43_on_a_256x256_vgg19(lib):
    """Sixteen by sixteen F(4,3) patches per image and every 64- and 128-multiple layer on that route, where the grid case has one 64x64 image
    of them: vgg19 at 256x256, B 1, against forward_host in float64 computed here, forward_host in float32 as the float32 reference.  The
    default route is held to the factor 8 on every tap; the opt-in route is printed against it and held to the sanity bound of the test above
    (its first tap exceeds the 8: that is why it is opt-in, profiles/NOTES.md)."""
    import copy
    names = ['conv1_2', 'conv2_2', 'conv3_4', 'conv4_4', 'conv5_4', 'relu5_4']
    net = R.fill_state(lib.A.VGGFeatureExtractor(names, 'vgg19'), 44)
    x = torch.from_numpy(np.random.default_rng(45).uniform(0., 1., (1, 3, 256, 256)).astype(np.float32))
    with torch.no_grad():
        f32 = net.forward_host(x)
        f64 = copy.deepcopy(net).double().forward_host(x.double())
    dev = net.cuda()
    base = dev(x.cuda())
    dev.winograd_f43 = True
    out = dev(x.cuda())
    assert list(out) == names
    differs = 0
    for k in names:
        assert out[k].shape == f32[k].shape
        _yardstick(f'vgg19 256x256 {k}', _np(base[k]), _np(f32[k]), _np(f64[k]))
        e, e_ref = R.rel_err(_np(out[k]), _np(f64[k])), R.rel_err(_np(f32[k]), _np(f64[k]))
        print(f'vgg19 256x256 {k} with winograd_f43: e(device) {e:.3e}  ratio {e / e_ref:.3f}')
        assert e < 1e-4, (k, e)
        differs += not np.array_equal(_bits(out[k]), _bits(base[k]))
    assert differs == len(names)


@pytest.mark.parametrize('criterion', R.CRITERIA)
@pytest.mark.parametrize('case', R.LOSS_CASES)
def test_perceptual_loss_against_the_reference(lib, case, criterion):
    """The narrowest output is the style term of [odd-mse]: ratio 7.22 (e(device) 4.70e-7 against a reference value that sits at 6.5e-8 through a
    cancellation between its layer terms); with whole 9 * cin accumulation chains on the general kernel it stood at 18.6 and failed.
    profiles/NOTES.md, "VGG / perceptual"."""
    g = R.golden()
    x, gt = R.case_input(case).cuda(), R.case_input(case, 1).cuda()
    net = R.build_loss(lib.LS.PerceptualLoss, case, criterion).cuda()
    percep, style = net(x, gt)
    for t in (percep, style):
        assert t.dim() == 0 and t.dtype == torch.float32 and t.is_cuda and not t.requires_grad
    f32, f64 = g[f'loss_{case}_{criterion}_f32'], g[f'loss_{case}_{criterion}_f64']
    _yardstick(f'loss {case} {criterion} percep', float(percep), f32[0], f64[0], HALF_ULP)
    _yardstick(f'loss {case} {criterion} style', float(style), f32[1], f64[1], HALF_ULP)
    p2, s2 = net(x, gt)
    assert np.array_equal(_bits(p2), _bits(percep)) and np.array_equal(_bits(s2), _bits(style))
    net.style_weight = 0.
    assert net(x, gt)[1] is None
    with pytest.raises(RuntimeError):
        net(x.clone().requires_grad_(True), gt)
    with torch.no_grad():
        net(x.clone().requires_grad_(True), gt)


# ---- cf_vgg_input --------------------------------------------------------------------------------------------------------------------
def _input_host(view, bgr, range_norm, mean, std):
    """(B,H,W,3) CPU view -> (B,H,W,3) float32 RGB: the reference's expression, one float32 operation per step."""
    f = view.to(torch.float32) / torch.tensor(255., dtype=torch.float32) if view.dtype == torch.uint8 else view
    if bgr:
        f = f.flip(3)
    if range_norm:
        f = (f + 1) / 2
    if mean is not None:
        f = (f - torch.tensor(mean, dtype=torch.float32)) / torch.tensor(std, dtype=torch.float32)
    return f


@pytest.mark.parametrize('norm', [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize('dtype', [torch.uint8, torch.float32])
def test_vgg_input_is_bitwise_the_host_expression(lib, dtype, norm):
    range_norm, use_norm = norm
    rng = np.random.default_rng(17)
    big = rng.integers(0, 256, (3, 40, 70, 3), dtype=np.uint8) if dtype == torch.uint8 else rng.uniform(-1., 1., (3, 40, 70, 3)).astype(np.float32)
    big = torch.from_numpy(big)
    mean, std = ([0.485, 0.456, 0.406], [0.229, 0.224, 0.225]) if use_norm else (None, None)
    if use_norm:
        mean, std = (torch.tensor(v, dtype=torch.float32).tolist() for v in (mean, std))
    chw = big.permute(0, 3, 1, 2).contiguous()
    views = {'HWC': lambda t, c: t, 'CHW': lambda t, c: c.permute(0, 2, 3, 1), 'crop': lambda t, c: t[1:, 3:36, 5:67:2],
             'crop CHW': lambda t, c: c.permute(0, 2, 3, 1)[:, 1:38:3, 2:]}
    dev_big, dev_chw = big.cuda(), chw.cuda()
    for name, view in views.items():
        for bgr in (False, True):
            want = _input_host(view(big, chw), bgr, range_norm, mean, std)
            got = lib.ops.vgg_input(view(dev_big, dev_chw), bgr, range_norm, mean, std)
            assert tuple(got.shape) == tuple(want.shape[:3]) + (lib.ops.VGG_IN_CPAD,) and got.is_contiguous()
            assert np.array_equal(_bits(got[..., :3]), _bits(want)), (name, bgr)
            assert not bool(got[..., 3:].any())


def test_vgg_input_refuses_bad_arguments(lib):
    x = torch.zeros(1, 4, 4, 3, device='cuda')
    with pytest.raises(ValueError):
        lib.ops.vgg_input(x[..., :2], False)
    with pytest.raises(ValueError):
        lib.ops.vgg_input(x.double(), False)
    with pytest.raises(ValueError):
        lib.ops.vgg_input(x, False, mean=[0., 0., 0.])
    with pytest.raises(ValueError):
        lib.ops.vgg_input(x, False, c_pad=6)
    with pytest.raises(ValueError):
        lib.ops.vgg_input(x, False, out=torch.zeros(1, 4, 4, 8, device='cuda'))


# ---- ReLU / pool ---------------------------------------------------------------------------------------------------------------------
def _special(shape, seed):
    """Normal values with NaN, +inf, -inf and -0 placed so that every position of a 2x2 window holds each of them somewhere."""
    x = torch.from_numpy(np.random.default_rng(seed).normal(0., 1., shape).astype(np.float32))
    B, H, W, C = shape
    nwy, nwx = max(H // 2, 1), max(W // 2, 1)
    n = 0
    for dy in range(2):
        for dx in range(2):
            for v in (float('nan'), float('inf'), float('-inf'), -0.0):
                wy, wx = (n // nwx) % nwy, n % nwx
                x[n % B, min(2 * wy + dy, H - 1), min(2 * wx + dx, W - 1), n % C] = v
                n += 1
    return x


def _same_numbers(a, b):
    return np.array_equal(_np(a), _np(b), equal_nan=True)


@pytest.mark.parametrize('shape', [(2, 8, 6, 8), (2, 7, 5, 4), (1, 9, 8, 12), (2, 2, 3, 4), (1, 33, 47, 64)])
def test_relu_and_relu_maxpool2_against_torch(lib, shape):
    x = _special(shape, 3).cuda()
    nchw = x.permute(0, 3, 1, 2)
    want_relu = torch.relu(nchw).permute(0, 2, 3, 1)
    want_pool = F.max_pool2d(torch.relu(nchw), 2, 2).permute(0, 2, 3, 1)
    assert bool(torch.isnan(want_pool).any()) and bool(torch.isinf(want_pool).any())
    assert _same_numbers(lib.ops.relu(x), want_relu)
    assert _same_numbers(lib.ops.relu_maxpool2(x), want_pool)
    pooled, full = lib.ops.relu_maxpool2(x, full=True)
    assert _same_numbers(pooled, want_pool) and _same_numbers(full, want_relu)
    y = x.clone()
    pooled, full = lib.ops.relu_maxpool2(y, full='inplace')
    assert full is y and _same_numbers(pooled, want_pool) and _same_numbers(y, want_relu)
    y = x.clone()
    assert lib.ops.relu(y, inplace=True) is y and _same_numbers(y, want_relu)
    assert not bool(torch.signbit(lib.ops.relu(x))[~torch.isnan(x)].any())     # (+0, never -0)


def test_relu_on_a_one_pixel_wide_input_and_the_pool_refusal(lib):
    x = _special((2, 5, 1, 8), 4).cuda()
    assert _same_numbers(lib.ops.relu(x), torch.relu(x))
    for bad in (x, x.permute(0, 2, 1, 3).contiguous()):
        with pytest.raises(ValueError):      # (nn.MaxPool2d(2, 2) raises on such a map as well)
            lib.ops.relu_maxpool2(bad)
    with pytest.raises(ValueError):
        lib.ops.relu_maxpool2(torch.zeros(1, 4, 4, 6, device='cuda'))
    with pytest.raises(ValueError):
        lib.ops.relu(torch.zeros(1, 3, 3, 3, device='cuda'))


# ---- cf_gram -------------------------------------------------------------------------------------------------------------------------
def _gram64(f):
    f = f.double()
    return f.transpose(1, 2).bmm(f) / (f.shape[2] * f.shape[1])


GRAM_HW = (1, 1023, 1024, 1025, 3 * 1024 + 5)


@pytest.mark.parametrize('hw', GRAM_HW)
@pytest.mark.parametrize('c', [64, 512])
def test_gram_against_bmm(lib, c, hw):
    assert lib.ops.GRAM_CHUNK == 1024
    f = torch.from_numpy(np.random.default_rng(c + hw).normal(0., 1., (2, hw, c)).astype(np.float32))
    ft = f.transpose(1, 2).contiguous()               # the reference's (n, c, h*w) features
    f32 = ft.bmm(ft.transpose(1, 2)) / (c * hw)       # _gram_mat in float32 on the CPU
    g = lib.ops.gram(f.cuda())
    assert tuple(g.shape) == (2, c, c)
    _yardstick(f'gram c {c} hw {hw}', _np(g), _np(f32), _np(_gram64(f)))
    assert np.array_equal(_bits(g), _bits(g.transpose(1, 2))), 'not bitwise symmetric'
    assert np.array_equal(_bits(lib.ops.gram(f.cuda())), _bits(g)), 'not repeatable'
    assert np.array_equal(_bits(lib.ops.gram(f[1:].cuda())), _bits(g[1:])), 'row 1 differs from the batch of one'


@pytest.mark.parametrize('c,hw', [(64, 1025), (192, 2500)])
def test_gram_is_exact_on_small_integers(lib, c, hw):
    """Features in -3 .. 3: every product and every partial sum is an integer below 2^24, so any order of summation gives the same float."""
    f = torch.from_numpy(np.random.default_rng(c).integers(-3, 4, (2, hw, c)).astype(np.float32))
    want = (f.double().transpose(1, 2).bmm(f.double())).float() / torch.tensor(float(c * hw), dtype=torch.float32)
    assert np.array_equal(_bits(lib.ops.gram(f.cuda())), _bits(want))
    g4 = lib.ops.gram(f.view(2, hw // 5, 5, c).cuda()) if hw % 5 == 0 else None      # (B,H,W,C) is accepted as well
    assert g4 is None or np.array_equal(_bits(g4), _bits(want))


@pytest.mark.parametrize('p', [0, 1023, 1024, 2052])
def test_gram_of_a_one_hot_pixel_is_the_outer_product(lib, p):
    c, hw = 128, 2053
    v = torch.from_numpy(np.random.default_rng(p).normal(0., 1., c).astype(np.float32))
    f = torch.zeros(1, hw, c)
    f[0, p] = v
    want = (v[:, None] * v[None, :]) / torch.tensor(float(c * hw), dtype=torch.float32)
    assert np.array_equal(_bits(lib.ops.gram(f.cuda())[0]), _bits(want))


def test_gram_refuses_bad_shapes(lib):
    for shape in ((1, 16, 32), (1, 16, 576), (1, 16), (1, 0, 64)):
        with pytest.raises(ValueError):
            lib.ops.gram(torch.zeros(shape, device='cuda'))
    with pytest.raises(ValueError):
        lib.ops.gram(torch.zeros(1, 16, 128, device='cuda')[:, :, :64])
    assert lib.ops.L.load().cf_gram_workspace_elems(2, 1025, 64) == 2 * 2 * 64 * 64
    assert lib.ops.L.load().cf_gram_workspace_elems(2, 1025, 65) == -1


# ---- cf_feat_dist --------------------------------------------------------------------------------------------------------------------
def _dist64(a, b):
    """Per image (sum |d|, sum d^2) of d = one float32 subtraction, widened: every d^2 is exact in float64 (24-bit operands) and math.fsum
    rounds the exact sum once, so this side carries half an ulp and no more."""
    import math
    d = (_np(a) - _np(b)).astype(np.float64).reshape(a.shape[0], -1)
    return np.array([[math.fsum(np.abs(r)), math.fsum(r * r)] for r in d]), d


@pytest.mark.parametrize('n', [1, 5, 16383, 16384, 16385, 3 * 16384 + 8, 2 * 16384 + 3])
def test_feat_dist_against_numpy(lib, n):
    """The standard bound of a float64 sum of n terms in any order, n 2^-53 relative to the sum of |terms|, against the correctly rounded sum."""
    assert lib.ops.FEAT_CHUNK == 16384
    rng = np.random.default_rng(n)
    a, b = (torch.from_numpy(rng.normal(0., 1., (3, n)).astype(np.float32)).cuda() for _ in range(2))
    got = _np(lib.ops.feat_dist(a, b))
    want, d = _dist64(a, b)
    bound = n * 2.0 ** -53 * want
    print(f'\nfeat_dist n {n}: |device - fsum| / bound  max {float((np.abs(got - want) / bound).max()):.4f}')
    assert (np.abs(got - want) <= bound).all()
    assert np.array_equal(_bits(lib.ops.feat_dist(a, b)), got.view(np.uint64))
    assert np.array_equal(_bits(lib.ops.feat_dist(a[2:], b[2:])), got[2:].view(np.uint64))
    # the same values behind pointers that are not 16-byte aligned take the scalar loads: the same elements in the same order
    ua, ub = (torch.cat([t.new_zeros(1), t.reshape(-1)])[1:].view(3, n) for t in (a, b))
    assert ua.data_ptr() % 16 and np.array_equal(_bits(lib.ops.feat_dist(ua, ub)), got.view(np.uint64))


def test_feat_dist_is_exact_on_integers_and_sees_the_ends_of_a_chunk(lib):
    n = 2 * 16384 + 5
    rng = np.random.default_rng(1)
    a = torch.from_numpy(rng.integers(-50, 51, (2, n)).astype(np.float32))
    b = torch.from_numpy(rng.integers(-50, 51, (2, n)).astype(np.float32))
    want, _ = _dist64(a, b)
    assert np.array_equal(_np(lib.ops.feat_dist(a.cuda(), b.cuda())), want)
    for pos in (0, 16383, 16384, 2 * 16384 - 1, 2 * 16384, n - 1):
        c = a.clone()
        c[1, pos] += 3.0
        assert np.array_equal(_np(lib.ops.feat_dist(a.cuda(), c.cuda())), np.array([[0., 0.], [3., 9.]])), pos
    with pytest.raises(ValueError):
        lib.ops.feat_dist(a.cuda(), b.cuda()[:, :-1])
    with pytest.raises(TypeError):
        lib.ops.feat_dist(a.cuda().double(), b.cuda().double())


# ---- the metric ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def scorer(lib):
    torch.manual_seed(2)
    return R.fill_state(lib.M.load_vgg(vgg_type='vgg16', layer_weights={'relu1_2': 0.5, 'conv2_2': 1., 'relu3_3': 2.}), 6).cuda()


def test_perceptual_batch_rows_layouts_and_zero(lib, scorer):
    rng = np.random.default_rng(8)
    a, b = (torch.from_numpy(rng.integers(0, 256, (3, 40, 24, 3), dtype=np.uint8)).cuda() for _ in range(2))
    fa, fb = (t.cpu().flip(3).float().div(torch.tensor(255.)).permute(0, 3, 1, 2).contiguous().cuda() for t in (a, b))
    for style in (False, True):
        for crit in R.CRITERIA:
            s = lib.M.perceptual_batch(a, b, scorer, criterion=crit, style=style)
            assert s.dtype == torch.float64 and tuple(s.shape) == (3,) and s.is_cuda and bool((s > 0).all())
            for r in range(3):
                assert np.array_equal(_bits(lib.M.perceptual_batch(a[r:r + 1], b[r:r + 1], scorer, criterion=crit, style=style)), _bits(s[r:r + 1])), (crit, style, r)
            assert np.array_equal(_bits(lib.M.perceptual_batch(fa, fb, scorer, order='CHW', criterion=crit, style=style)), _bits(s)), (crit, style)
            assert np.array_equal(_np(lib.M.perceptual_batch(a, a, scorer, criterion=crit, style=style)), np.zeros(3)), (crit, style)
    assert lib.M.calculate_perceptual(a[1], b[1], scorer) == float(lib.M.perceptual_batch(a, b, scorer)[1])


def test_perceptual_batch_against_the_host_definition(lib, scorer):
    """The device score against the same definition on stock torch ops in float64 (the module in .double() on the CPU, from the bytes on),
    with the module's float32 CPU result as the float32 reference."""
    import copy
    rng = np.random.default_rng(12)
    a, b = (torch.from_numpy(rng.integers(0, 256, (2, 40, 24, 3), dtype=np.uint8)) for _ in range(2))
    host = copy.deepcopy(scorer).cpu()
    f32 = {style: lib.M.perceptual_batch(a, b, host, style=style) for style in (False, True)}
    host = host.double()
    with torch.no_grad():
        fa, fb = (host.vgg.forward_host(t.flip(3).double().div(255.).permute(0, 3, 1, 2)) for t in (a, b))
    for style in (False, True):
        f64 = 0
        for k in fa:
            ta, tb = (lib.LS.gram_host(f) if style else f for f in (fa[k], fb[k]))
            f64 = f64 + (ta - tb).abs().reshape(2, -1).mean(1) * scorer.layer_weights[k]
        dev = lib.M.perceptual_batch(a.cuda(), b.cuda(), scorer, style=style)
        _yardstick(f'perceptual_batch l1 style {style}', _np(dev), _np(f32[style]), _np(f64), HALF_ULP)


# ---- the LPIPS form ------------------------------------------------------------------------------------------------------------------
def _lpips_layer_host(fa, fb, w, dtype):
    """One layer of the published definition restated on (B,HW,C) features in `dtype`: channel-normalise, weighted squared difference, pixel mean."""
    fa, fb, w = fa.to(dtype), fb.to(dtype), w.to(dtype)
    na = fa / (fa.pow(2).sum(2, keepdim=True).sqrt() + 1e-10)
    nb = fb / (fb.pow(2).sum(2, keepdim=True).sqrt() + 1e-10)
    return (((na - nb) ** 2) * w).sum(2).mean(1).double()


@pytest.mark.parametrize('hw', [1, 255, 256, 257, 3 * 256 + 5])
@pytest.mark.parametrize('c', [64, 512])
def test_lpips_head_against_the_restatement(lib, c, hw):
    rng = np.random.default_rng(c * 7 + hw)
    fa, fb = (torch.from_numpy(rng.normal(0., 1., (3, hw, c)).astype(np.float32)) for _ in range(2))
    fa[1, hw // 2] = 0.          # an all-zero feature pixel on one side: only the 1e-10 keeps 0 / 0 away
    fa[2, 0] = 0.
    fb[2, 0] = 0.                # ... and on both
    w = torch.from_numpy(rng.uniform(0., 1., c).astype(np.float32))
    got = lib.ops.lpips_head(fa.cuda(), fb.cuda(), w.cuda())
    assert got.dtype == torch.float64 and tuple(got.shape) == (3,) and bool(torch.isfinite(got).all())
    _yardstick(f'lpips_head c {c} hw {hw}', _np(got), _np(_lpips_layer_host(fa, fb, w, torch.float32)), _np(_lpips_layer_host(fa, fb, w, torch.float64)))
    assert np.array_equal(_bits(lib.ops.lpips_head(fa.cuda(), fb.cuda(), w.cuda())), _bits(got))
    assert np.array_equal(_bits(lib.ops.lpips_head(fa[1:2].cuda(), fb[1:2].cuda(), w.cuda())), _bits(got[1:2]))
    assert np.array_equal(_np(lib.ops.lpips_head(fa.cuda(), fa.cuda(), w.cuda())), np.zeros(3))


def test_lpips_batch_against_the_restatement(lib):
    import copy
    torch.manual_seed(3)
    net = R.fill_state(lib.M.load_lpips_vgg(), 8)
    rng = np.random.default_rng(21)
    a, b = (torch.from_numpy(rng.uniform(-1., 1., (2, 40, 24, 3)).astype(np.float32)) for _ in range(2))
    lin = [torch.from_numpy(rng.uniform(0., 1., c).astype(np.float32)) for c in (64, 128, 256, 512, 512)]
    ref = {}
    for dtype in (torch.float32, torch.float64):
        host = copy.deepcopy(net).to(dtype)
        with torch.no_grad():
            fa, fb = (host.forward_host(t.permute(0, 3, 1, 2).to(dtype)) for t in (a, b))
        ref[dtype] = sum(_lpips_layer_host(fa[k].flatten(2).transpose(1, 2), fb[k].flatten(2).transpose(1, 2), w, dtype) for k, w in zip(fa, lin))
    dev = net.cuda()
    dlin = [w.cuda() for w in lin]
    got = lib.M.lpips_batch(a.cuda(), b.cuda(), dev, dlin)
    assert got.dtype == torch.float64 and tuple(got.shape) == (2,) and got.is_cuda
    _yardstick('lpips_batch', _np(got), _np(ref[torch.float32]), _np(ref[torch.float64]))
    chw = a.permute(0, 3, 1, 2).contiguous().cuda(), b.permute(0, 3, 1, 2).contiguous().cuda()
    assert np.array_equal(_bits(lib.M.lpips_batch(*chw, dev, dlin, order='CHW')), _bits(got))
    assert np.array_equal(_bits(lib.M.lpips_batch(a[1:].cuda(), b[1:].cuda(), dev, dlin)), _bits(got[1:]))
    assert np.array_equal(_np(lib.M.lpips_batch(a.cuda(), a.cuda(), dev, dlin)), np.zeros(2))
    with pytest.raises(ValueError):
        lib.M.lpips_batch(a.cuda(), b.cuda(), dev, dlin[:4])
    with pytest.raises(ValueError):
        lib.ops.lpips_head(torch.zeros(1, 4, 6, device='cuda'), torch.zeros(1, 4, 6, device='cuda'), torch.zeros(6, device='cuda'))
