"""-m gpu: ResNetArcFace and the identity metric on the device (csrc/cf_arcface.hip and the PReLU epilogues of cf_igemm.hip).

The yardstick rule: with e(x) = max|x - ref64| / max|ref64|, the device must satisfy e(device) <= 8 e(float32 reference), where the float32
reference is the reference module's own CPU forward (whole network: recorded in tests/golden/arcface_ref.npz) or the block's forward_host
(blocks and kernels alone), and ref64 the same module in float64.  The margin of 8 covers one extra rounding per folded weight and another
summation order over K up to 32768.  Every measured ratio is printed before it is asserted.  Everything else is bitwise.

Measured on an MI355X (ratio e(device) / e(float32 reference)): see profiles/NOTES.md, "ArcFace".
"""
import copy

import numpy as np
import pytest
import torch
from torch.nn import functional as F

import arcface_ref as R

pytestmark = pytest.mark.gpu
MARGIN = 8.0


@pytest.fixture(scope='module')
def lib():
    from codeformer_amd import build as cf_build
    cf_build.build()
    assert torch.cuda.is_available()
    from codeformer_amd import metrics, ops
    from codeformer_amd.archs import arcface_arch
    return type('Lib', (), {'M': metrics, 'ops': ops, 'A': arcface_arch})


@pytest.fixture(scope='module')
def nets(lib):
    return {case: R.build(lib.A.ResNetArcFace, case).cuda() for case in R.CASES}


@pytest.fixture(scope='module')
def embeddings(nets):
    """Device embeddings of both cases, computed once."""
    return {case: nets[case](R.case_input(case).cuda()) for case in R.CASES}


def _np(t):
    return t.detach().cpu().numpy()


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.numpy().view(np.uint64 if t.dtype == torch.float64 else np.uint32)


def _yardstick(what, dev, f32, f64):
    e_dev, e_ref = R.rel_err(dev, f64), R.rel_err(f32, f64)
    print(f'\n{what}: e(device) {e_dev:.3e}  e(float32 reference) {e_ref:.3e}  ratio {e_dev / e_ref if e_ref else float("inf"):.3f}')
    assert e_dev <= MARGIN * e_ref, (what, e_dev, e_ref)


# ---- the whole network ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', list(R.CASES))
def test_network_against_the_reference(embeddings, case):
    g = R.golden()
    dev = _np(embeddings[case])
    assert dev.shape == (R.CASES[case]['batch'], 512) and dev.dtype == np.float32
    _yardstick(f'network {case} embedding', dev, g[f'{case}_f32'], g[f'{case}_f64'])
    _yardstick(f'network {case} cosine', R.cosines(dev), R.cosines(g[f'{case}_f32']), R.cosines(g[f'{case}_f64']))


def test_network_rows_and_repeats_are_bitwise(nets, embeddings):
    x = R.case_input('r18').cuda()
    again = nets['r18'](x)
    assert np.array_equal(_bits(again), _bits(embeddings['r18']))
    for b in range(x.shape[0]):
        assert np.array_equal(_bits(nets['r18'](x[b:b + 1])), _bits(embeddings['r18'][b:b + 1])), b
    xs = R.case_input('se').cuda()
    assert np.array_equal(_bits(nets['se'](xs[1:2])), _bits(embeddings['se'][1:2]))


def test_a_device_call_in_training_mode_raises(nets, lib):
    net = copy.deepcopy(nets['se']).train()
    x = R.case_input('se').cuda()
    with pytest.raises(RuntimeError):
        net(x)
    with pytest.raises(RuntimeError):
        net.layer1[0](torch.zeros(1, 64, 16, 16, device='cuda'))
    with pytest.raises(ValueError):
        nets['se'](torch.zeros(1, 1, 112, 112, device='cuda'))


# ---- blocks alone --------------------------------------------------------------------------------------------------------------------
BLOCKS = {   # name: (inplanes, planes, stride, use_se, H, W)
    's1_ragged': (64, 64, 1, False, 24, 40),
    's2_shortcut': (64, 128, 2, False, 16, 32),
    's2_smallest': (256, 512, 2, False, 16, 16),
    'se_8x8': (128, 128, 1, True, 8, 8),
    'se_ragged': (128, 128, 1, True, 24, 40),
}


@pytest.mark.parametrize('slope', R.SLOPES)
@pytest.mark.parametrize('name', list(BLOCKS))
def test_block_against_its_host_forward(lib, name, slope):
    cin, cout, stride, use_se, H, W = BLOCKS[name]
    down = None
    if stride != 1 or cin != cout:
        down = torch.nn.Sequential(torch.nn.Conv2d(cin, cout, kernel_size=1, stride=stride, bias=False), torch.nn.BatchNorm2d(cout))
    seed = 300 + list(BLOCKS).index(name)
    blk = R.fill_state(lib.A.IRBlock(cin, cout, stride, down, use_se=use_se), seed, slope=slope).eval()
    x = torch.from_numpy(np.random.default_rng(seed + 50).normal(0., 1., (2, cin, H, W)).astype(np.float32))
    with torch.no_grad():
        f32 = blk(x)
        f64 = copy.deepcopy(blk).double()(x.double())
    dev = blk.cuda()(x.cuda())
    assert dev.shape == f32.shape
    _yardstick(f'block {name} slope {slope}', _np(dev), _np(f32), _np(f64))
    assert np.array_equal(_bits(blk(x[1:2].cuda())), _bits(dev[1:2]))   # row 1 alone


# ---- kernels alone -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,slope', [((2, 2, 2, 4), 0.25), ((1, 6, 10, 64), 0.25), ((1, 6, 10, 64), -0.5), ((2, 2, 2, 4), -0.5)])
def test_prelu_maxpool2_is_bitwise_torch(lib, shape, slope):
    x = torch.from_numpy(np.random.default_rng(sum(shape)).normal(0., 1., shape).astype(np.float32))   # NHWC
    nchw = x.permute(0, 3, 1, 2)
    ref = F.max_pool2d(F.prelu(nchw, torch.tensor([slope])), 2, 2).permute(0, 2, 3, 1).contiguous()
    got = lib.ops.prelu_maxpool2(x.cuda(), slope)
    assert np.array_equal(_bits(got), _bits(ref))
    if slope < 0:   # PReLU first: the other order gives another result
        assert not torch.equal(F.prelu(F.max_pool2d(nchw, 2, 2), torch.tensor([slope])).permute(0, 2, 3, 1), ref)


@pytest.mark.parametrize('shape', [(2, 8, 8, 512), (2, 24, 40, 128), (1, 17, 19, 68), (3, 1, 1, 4)])
def test_se_pool_within_hw_ulp(lib, shape):
    """Within H W ulp of the float64 mean, per channel."""
    B, H, W, C = shape
    x = torch.from_numpy(np.random.default_rng(C).normal(0.5, 1., shape).astype(np.float32))
    got = _np(lib.ops.se_pool(x.cuda()))
    x64 = x.double().view(B, H * W, C)
    mean = x64.mean(dim=1).numpy()
    bound = H * W * np.spacing(np.abs(mean).astype(np.float32)).astype(np.float64)
    err = np.abs(got - mean)
    print(f'\nse_pool {shape}: largest error / bound {float((err / bound).max()):.3e}')
    assert np.all(err <= bound)
    assert np.array_equal(_bits(lib.ops.se_pool(x[-1:].cuda())), got[-1:].view(np.uint32))   # the last image alone


@pytest.mark.parametrize('slope', R.SLOPES)
def test_se_gate_and_scale(lib, slope):
    se = R.fill_state(lib.A.SEBlock(128), 77, slope=slope).eval()
    rng = np.random.default_rng(78)
    x = torch.from_numpy(rng.normal(0., 1., (2, 128, 8, 8)).astype(np.float32))
    res = torch.from_numpy(rng.normal(0., 1., (2, 128, 8, 8)).astype(np.float32))
    pooled = x.mean(dim=(2, 3))
    se64 = copy.deepcopy(se).double()
    with torch.no_grad():
        g32, g64 = se.fc(pooled), se64.fc(pooled.double())
    sec = copy.deepcopy(se).cuda()
    gate = lib.ops.se_gate(pooled.cuda(), sec.fc[0].weight.detach(), sec.fc[0].bias.detach(), slope, sec.fc[2].weight.detach(), sec.fc[2].bias.detach())
    _yardstick(f'se_gate slope {slope}', _np(gate), _np(g32), _np(g64))
    # scale + residual + PReLU on the float32 gate: the same float32 operations as torch, so the yardstick leaves no room
    a = torch.tensor([slope])
    f32 = F.prelu(x * g32.view(2, 128, 1, 1) + res, a)
    f64 = F.prelu(x.double() * g32.double().view(2, 128, 1, 1) + res.double(), a.double())
    nhwc = [t.permute(0, 2, 3, 1).contiguous().cuda() for t in (x, res)]
    dev = lib.ops.se_scale_res_prelu(nhwc[0], g32.cuda(), nhwc[1], slope).permute(0, 3, 1, 2)
    _yardstick(f'se_scale_res_prelu slope {slope}', _np(dev), _np(f32), _np(f64))
    assert np.array_equal(_bits(dev), _bits(f32))


@pytest.mark.parametrize('N', [128, 132])
def test_fc_rows(lib, N):
    """K = 1024 (several K chunks), N = 128 (two full 64-column blocks) and 132 (a last block of four columns: the clamp and the store guard),
    1, 3 and 17 rows (two launches): fp32 against float64 under the yardstick (the float32 reference is torch's F.linear on the CPU), rows
    bitwise independent of the batch."""
    rng = np.random.default_rng(9 + N)
    x = torch.from_numpy(rng.normal(0., 1., (17, 1024)).astype(np.float32))
    w = torch.from_numpy(rng.normal(0., 1. / 32, (N, 1024)).astype(np.float32))
    b = torch.from_numpy(rng.normal(0., 1., (N,)).astype(np.float32))
    wp = lib.ops.pack_fc_rows(w.cuda())
    dev = lib.ops.fc_rows(x.cuda(), wp, b.cuda())
    _yardstick(f'fc_rows N {N}', _np(dev), _np(F.linear(x, w, b)), _np(F.linear(x.double(), w.double(), b.double())))
    for rows in ((0, 1), (2, 5), (16, 17)):
        assert np.array_equal(_bits(lib.ops.fc_rows(x[rows[0]:rows[1]].cuda(), wp, b.cuda())), _bits(dev[rows[0]:rows[1]])), rows


def test_cosine_rows(lib):
    rng = np.random.default_rng(10)
    for n in (512, 70):
        x, y = rng.normal(0., 1., (5, n)).astype(np.float32), rng.normal(0., 1., (5, n)).astype(np.float32)
        x[3] = 0
        y[4] = x[4]
        got = _np(lib.ops.cosine_rows(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()))
        x64, y64 = x.astype(np.float64), y.astype(np.float64)
        ref = (x64 * y64).sum(1) / np.maximum(np.linalg.norm(x64, axis=1) * np.linalg.norm(y64, axis=1), 1e-8)
        assert got.dtype == np.float64 and np.all(np.abs(got - ref) <= 1e-12)
        assert got[3] == 0.0 and abs(got[4] - 1) <= 1e-12


# ---- identity_input and identity_batch -----------------------------------------------------------------------------------------------
def _image(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.integers(0, 256, shape).astype(np.uint8) if dtype == 'uint8' else rng.random(shape).astype(np.float32))


@pytest.mark.parametrize('shape,dtype,order', [((2, 128, 128, 3), 'uint8', 'HWC'), ((1, 512, 512, 3), 'uint8', 'HWC'), ((2, 3, 200, 136), 'float32', 'CHW'),
                                               ((1, 64, 64, 3), 'float32', 'HWC'), ((1, 131, 77, 3), 'uint8', 'HWC')])
def test_identity_input_is_bitwise_the_host_definition(lib, shape, dtype, order):
    img = _image(shape, dtype, shape[1] + shape[2])
    host = lib.M.identity_input(img, order)
    dev = lib.M.identity_input(img.cuda(), order)
    assert dev.is_cuda and np.array_equal(_bits(dev), _bits(host))
    if shape[1:3] == (128, 128):
        assert np.array_equal(_bits(dev[:, 0]), _bits(lib.M.identity_gray_host(img)))
    if shape[1] == 512:   # exact x4: two equal taps per axis
        g = lib.M.identity_gray_host(img)[0]
        q = lambda dy, dx: g[1 + dy::4, 1 + dx::4]   # noqa: E731
        assert torch.equal(host[0, 0], 0.5 * (0.5 * q(0, 0) + 0.5 * q(0, 1)) + 0.5 * (0.5 * q(1, 0) + 0.5 * q(1, 1)))


def test_identity_input_reads_views_through_their_strides(lib):
    img = _image((3, 160, 176, 3), 'uint8', 5)
    dev = img.cuda()
    crop, crop_dev = img[:, 7:150, 11:163], dev[:, 7:150, 11:163]
    assert not crop_dev.is_contiguous()
    assert np.array_equal(_bits(lib.M.identity_input(crop_dev)), _bits(lib.M.identity_input(crop.contiguous())))
    assert np.array_equal(_bits(lib.M.identity_input(dev[1:3])), _bits(lib.M.identity_input(img)[1:3]))
    f = _image((2, 3, 90, 70), 'float32', 6)
    assert np.array_equal(_bits(lib.M.identity_input(f.cuda()[:, :, ::2, 3:], 'CHW')), _bits(lib.M.identity_input(f[:, :, ::2, 3:].contiguous(), 'CHW')))


def test_identity_batch_invariances(lib, nets):
    net = nets['r18']
    a, b = _image((3, 96, 96, 3), 'uint8', 20).cuda(), _image((3, 96, 96, 3), 'uint8', 21).cuda()
    ab = lib.M.identity_batch(a, b, net)
    assert ab.is_cuda and ab.dtype == torch.float64 and ab.shape == (3,)
    assert np.array_equal(_bits(lib.M.identity_batch(a, b, net)), _bits(ab))               # run to run
    assert np.array_equal(_bits(lib.M.identity_batch(b, a, net)), _bits(ab))               # symmetric
    for i in range(3):
        assert np.array_equal(_bits(lib.M.identity_batch(a[i:i + 1], b[i:i + 1], net)), _bits(ab[i:i + 1])), i
    assert float((lib.M.identity_batch(a, a, net) - 1).abs().max()) <= 1e-6
    one = lib.M.calculate_identity(a[0], b[0], net)
    assert isinstance(one, float) and one == float(ab[0])
    # the host path of the same definition, on the same module's forward_host
    host = lib.M.identity_batch(a.cpu(), b.cpu(), copy.deepcopy(net).cpu())
    print('identity_batch device', _np(ab), 'host', _np(host))
    # both embeddings of a pair carry a relative error of at most MARGIN * 1.3e-6 (the network gate above), and a cosine moves by at most
    # the sum of the two: 2 * 8 * 1.3e-6, doubled for the host's own float32 error
    assert float((ab.cpu() - host).abs().max()) <= 4e-5
