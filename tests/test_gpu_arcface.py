"""-m gpu: ResNetArcFace and the identity metric on the device (csrc/cf_arcface.hip and the PReLU epilogues of cf_igemm.hip).

The yardstick rule: with e(x) = max|x - ref64| / max|ref64|, the device must satisfy e(device) <= 8 e(float32 reference), where the float32
reference is the reference module's own CPU forward (whole network: recorded in tests/golden/arcface_ref.npz) or the block's forward_host
(blocks and kernels alone), and ref64 the same module in float64.  The margin of 8 covers one extra rounding per folded weight and another
summation order over K up to 32768.  Every measured ratio is printed before it is asserted.  Everything else is bitwise.

Measured on an MI355X (ratio e(device) / e(float32 reference)): see profiles/NOTES.md, "ArcFace".

Per element (the second half of this file).  The yardstick is blind to elements small next to the tensor's largest, so every kernel of
cf_arcface.hip is also held, element by element, to a bound derived from the order its comment states -- tools/arcface_check.py has the recipes,
the float64 references, the bounds and a NumPy float32 emulation of each order; tests/test_arcface_host.py shows on the CPU that the emulation
stays within 0.5 of every bound and that the exact families are exact.  Largest |error| / bound on an MI355X (every ratio is printed, `RATIO ...`):
  fc_rows  (1, 4, 256), (16, 68, 2304), (17, 128, 1024)     int_coded 0 (bitwise float64), one-hot rows bitwise fl(w[n, k] + b[n]) on both sides of every
           quarter and chunk boundary, cancel_pairs 0.0008, row_scales 0.0068, normal 0.0071
  se_gate  (2, 68, 3) 0.0258, (1, 320, 20) 0.0005, (1, 4096, 256) < 5e-5, (2, 128, 8) 0.0028, four slopes each; pre-activations of +-40 give exactly 1 and
           < 1e-14, never NaN.  Measured sigmoid figure (torch's CPU float32 sigmoid against float64 on the same pre-activations): 1.46 .. 1.90 u sigmoid(s)
  se_pool  normal 0.0519, cancel 0.0159, mixed 0.0568, int_coded 0.0039 (bitwise where H W is a power of two)
  cosine_rows  n 1, 63, 65 x rows 1, 4, 5 x norms 1, 1e-20, 1e+18: 0.0405
  prelu_maxpool2, se_scale_res_prelu, identity_input: bitwise (torch's CPU ops / the host definition)
  IRBlock without SE on the forms the network never reaches (reference: the folded dataflow in float64 on the float32-rounded folded parameters):
           128 -> 128 at 25x41 (`128`) 0.0025, 32 -> 32 at 9x5 (`32`) 0.0066, 64 -> 64 at 8x8 with batch 17 / 33 (the 32- and 64-row bn0 tables) 0.0040;
           every one of the 17 / 33 rows bitwise the row alone.  IRBlock(64, 96) has no 32-wide form: ops._cout_pad(96) is 128.
  The bounds are worst cases over every rounding and stand far above a random walk: the emulation sits at the same small ratios (the host test prints
  them), and each test asserts the kernel's ratio not below 1e-3 of the emulation's.
Whole file: 91 tests in 4.2 s (46 in 4.1 s before); the slowest new test is se_gate at (1, 4096, 256), 0.06 s.  Nothing failed on the first run.

Scratch builds with one in-range edit each (not committed; addresses, barriers and launch geometry untouched), each run once through this file and
the tests of tests/test_gpu_conv_prelu.py.  New tests of this file that fail | old ones (the yardstick tests above):
  (p1) cf_igemm.hip PReLU epilogue as max(t, a t)                 4: the reach blocks at slope 1.5 | r18, the five blocks at slope 1.5
  (p2) cf_igemm.hip RES_PRELU adds the residual after the select  8: every reach block | r18, 12 block cases
  (p3) cf_igemm.hip the padding takes the affine prologue's shift 8: every reach block | both networks, all 20 block cases
  (a4) fc_rows finish starts its chains at c = j + FC_FIN         3: fc_rows_per_element, every shape | fc_rows[128], [132] (K = 1024 is four chunks: all dropped), both networks
  (a5) se_gate layer 1 stops at c & ~63                           4: se_gate_per_element (2, 68, 3), every slope | 0 (C = 128 everywhere else)
  (a6) prelu_maxpool2 without the `t != t` clause                 1: prelu_maxpool2_non_finite_values.. | 0
Plainly: p1 - p3 and a4 are gross and the old yardstick tests catch them too, at the shapes and slopes they run; a5 and a6 are caught by the new
tests alone.  (tests/test_gpu_conv_prelu.py lists what p1 - p3 do to the per-element conv tests.)
"""
import copy

import numpy as np
import pytest
import torch
from torch.nn import functional as F

import arcface_ref as R
from _tools import _bits, _np, _yardstick

pytestmark = pytest.mark.gpu


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


# ---- the kernels of cf_arcface.hip per element (tools/arcface_check.py: recipes, float64 references, derived bounds) ---------------------
@pytest.fixture(scope='module')
def ac():
    from _tools import load_script
    return load_script('tools/arcface_check.py')


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _gate(what, got, ref, bound):
    """Print the largest |error| / bound, assert it at most 1; -> the ratio."""
    r = float((np.abs(got.astype(np.float64) - ref) / (bound + 1e-300)).max())
    print(f'\nRATIO {what}: {r:.4f} of the bound')
    assert np.all(np.isfinite(got)) and r <= 1.0, (what, r)
    return r


def _fc(lib, x, w, b):
    return _np(lib.ops.fc_rows(_t(x), lib.ops.pack_fc_rows(_t(w)), None if b is None else _t(b)))


@pytest.mark.parametrize('shape', [(1, 4, 256), (16, 68, 2304), (17, 128, 1024)])
def test_fc_rows_per_element(lib, ac, shape):
    """One chunk and a column block that is almost wholly the clamp; nine chunks (the finish's second pass), M at the launch limit, a ragged last
    block; two launches.  int_coded and the one-hot rows bitwise, every family within c u sum |w||x| + 2 u |out| per element."""
    M, N, K = shape
    for fam in ac.FC_FAMILIES:
        x, w, b = ac.fc_family(fam, shape)
        got, ref = _fc(lib, x, w, b), ac.fc_ref(x, w, b)
        r = _gate(f'fc_rows {fam} {shape}', got, ref, ac.fc_bound(x, w, b))
        e = float((np.abs(ac.fc_emulate(x, w, b).astype(np.float64) - ref) / ac.fc_bound(x, w, b)).max())
        assert r >= 1e-3 * e, (fam, shape, r, e)
        if fam == 'int_coded':
            assert np.array_equal(got.astype(np.float64), ref)
    x, w, b = ac.fc_family('normal', shape)
    ks = ac.fc_onehot_ks(K)
    wp, bd = lib.ops.pack_fc_rows(_t(w)), _t(b)
    for i in range(0, len(ks), M):      # M rows per call, as the shape says
        sel = ks[i:i + M]
        hot = np.zeros((len(sel), K), np.float32)
        hot[np.arange(len(sel)), sel] = 1.0
        got = _np(lib.ops.fc_rows(_t(hot), wp, bd))
        assert np.array_equal(_bits(torch.from_numpy(got)), _bits(torch.from_numpy((w[:, sel].T + b[None]).astype(np.float32)))), (shape, sel)
    if M > 1:   # rows bitwise independent of the batch and of M
        full = lib.ops.fc_rows(_t(x), wp, bd)
        for rows in ((0, 1), (M // 2, M // 2 + 3), (M - 1, M)):
            assert np.array_equal(_bits(lib.ops.fc_rows(_t(x[rows[0]:rows[1]]), wp, bd)), _bits(full[rows[0]:rows[1]])), rows


def test_fc_rows_workspace_query_refuses(lib):
    from codeformer_amd import lib as L
    q = L.load().cf_fc_rows_workspace_elems
    assert q(16, 68, 2304) == 9 * 16 * 68 and q(1, 4, 256) == 4
    for m, n, k in ((0, 64, 256), (17, 64, 256), (4, 64, 255), (4, 64, 128)):
        assert q(m, n, k) == -1, (m, n, k)


@pytest.mark.parametrize('slope', R.SLOPES)
@pytest.mark.parametrize('shape', [(2, 68, 3), (1, 320, 20), (1, 4096, 256), (2, 128, 8)])
def test_se_gate_per_element(lib, ac, shape, slope):
    """C off 64 and 256, r off 4, the limits 4096 / 256; pre-activations of +-40 in every seventh channel: the gate is finite, in [0, 1], within the bound."""
    p, w1, b1, w2, b2 = ac.gate_inputs(shape, slope)
    got = _np(lib.ops.se_gate(*(_t(v) for v in (p, w1, b1)), slope, _t(w2), _t(b2)))
    ref = ac.gate_ref(p, w1, b1, slope, w2, b2)
    emu, s32 = ac.gate_emulate(p, w1, b1, slope, w2, b2)
    fig = ac.sigmoid_figure(s32)
    bound = ac.gate_bound(p, w1, b1, slope, w2, b2, ref, fig)
    r = _gate(f'se_gate {shape} slope {slope} (sigmoid figure {fig:.3f} u)', got, ref['out'], bound)
    e = float((np.abs(emu.astype(np.float64) - ref['out']) / bound).max())
    assert r >= 1e-3 * e, (shape, slope, r, e)
    assert got.min() >= 0.0 and got.max() <= 1.0 and float(ref['s'].max()) > 35 and float(ref['s'].min()) < -35
    hi, lo = ref['s'] > 35, ref['s'] < -35
    assert np.all(got[hi] == 1.0) and np.all(got[lo] < 1e-14)


def test_se_gate_refuses_sizes_past_its_limits(lib):
    z = lambda *s: torch.zeros(*s, device='cuda')   # noqa: E731
    with pytest.raises(RuntimeError, match='cf_se_gate: bad dims'):
        lib.ops.se_gate(z(1, 4097), z(4, 4097), z(4), 0.25, z(4097, 4), z(4097))
    with pytest.raises(RuntimeError, match='cf_se_gate: bad dims'):
        lib.ops.se_gate(z(1, 64), z(257, 64), z(257), 0.25, z(64, 257), z(64))


@pytest.mark.parametrize('shape', [(1, 1, 1, 4), (1, 16, 16, 68), (2, 17, 19, 132)])
def test_se_pool_per_element(lib, ac, shape):
    """(31 + nrb + 2) u sum |x| / HW per channel: a bound that stands on cancelling and mixed-scale input, where H W ulp(|mean|) cannot be stated."""
    hw = shape[1] * shape[2]
    for fam in ac.SE_POOL_FAMILIES:
        x = ac.pool_family(fam, shape)
        got, ref = _np(lib.ops.se_pool(_t(x))), ac.pool_ref(x)
        r = _gate(f'se_pool {fam} {shape}', got, ref, ac.pool_bound(x))
        e = float((np.abs(ac.pool_emulate(x).astype(np.float64) - ref) / (ac.pool_bound(x) + 1e-300)).max())
        assert r >= 1e-3 * e, (fam, shape, r, e)
        if fam == 'int_coded' and hw & (hw - 1) == 0:
            assert np.array_equal(got.astype(np.float64), ref)


def test_prelu_maxpool2_non_finite_values_ties_and_signed_zeros(lib):
    """(2, 4, 6, 8): a NaN in each of the four window positions wins and stays in its window; -inf under a negative slope becomes +inf and wins; four
    equal values; -0.0 against +0.0: the bits of torch's CPU max_pool2d(prelu(x))."""
    rng = np.random.default_rng(31)
    base = torch.from_numpy(rng.normal(0., 1., (2, 4, 6, 8)).astype(np.float32))

    def both(x, slope):
        nchw = x.permute(0, 3, 1, 2)
        ref = F.max_pool2d(F.prelu(nchw, torch.tensor([slope])), 2, 2).permute(0, 2, 3, 1).contiguous()
        return lib.ops.prelu_maxpool2(x.cuda(), slope).cpu(), ref
    for slope in (0.25, -0.5):
        clean, ref = both(base, slope)
        assert np.array_equal(_bits(clean), _bits(ref))
        for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
            x = base.clone()
            x[1, 2 + dy, 2 + dx, 3] = float('nan')
            got, ref = both(x, slope)
            assert bool(torch.isnan(got[1, 1, 1, 3])) and bool(torch.isnan(ref[1, 1, 1, 3]))
            got[1, 1, 1, 3] = clean[1, 1, 1, 3]
            assert np.array_equal(_bits(got), _bits(clean)), (slope, dy, dx)
        x = base.clone()
        x[0, 0, 0, 0], x[0, 1, 3, 1], x[1, 3, 5, 7] = float('inf'), float('-inf'), float('-inf')
        x[0, 2:4, 0:2, 5] = 0.75                                     # four equal values
        x[1, 0, 0, 2], x[1, 0, 1, 2], x[1, 1, 0, 2], x[1, 1, 1, 2] = -0.0, 0.0, -0.0, -0.0      # signed zeros, either order
        x[1, 0, 2, 2], x[1, 0, 3, 2], x[1, 1, 2, 2], x[1, 1, 3, 2] = 0.0, -0.0, -0.0, -0.0
        got, ref = both(x, slope)
        assert np.array_equal(_bits(got), _bits(ref)), slope
        assert float(got[0, 0, 0, 0]) == float('inf') and float(got[0, 1, 0, 5]) == 0.75
        assert (float(got[0, 0, 1, 1]) == float('inf')) == (slope < 0) and (float(got[1, 1, 2, 7]) == float('inf')) == (slope < 0)
        assert bool(torch.isfinite(got).sum() == got.numel() - (3 if slope < 0 else 1))
    got, ref = both(x, 0.0)                                          # slope 0: 0 * (-inf) is NaN, and it wins
    assert bool(torch.isnan(got[0, 0, 1, 1])) and np.array_equal(_bits(got), _bits(ref))


def test_se_scale_res_prelu_without_residual_and_with_a_gate_per_image(lib):
    rng = np.random.default_rng(41)
    x = torch.from_numpy(rng.normal(0., 1., (3, 5, 7, 12)).astype(np.float32))      # H W C / 4 = 105 float4 per image: no multiple of the block
    res = torch.from_numpy(rng.normal(0., 1., (3, 5, 7, 12)).astype(np.float32))
    y = torch.from_numpy(rng.uniform(0., 1., (3, 12)).astype(np.float32))
    assert not torch.equal(y[0], y[1]) and not torch.equal(y[1], y[2])
    xy = x * y.view(3, 1, 1, 12)
    assert np.array_equal(_bits(lib.ops.se_scale_res_prelu(x.cuda(), y.cuda(), None, 1.0)), _bits(xy))
    for slope in R.SLOPES:
        a = torch.tensor(slope)
        for r, t in ((None, xy), (res, xy + res)):
            want = torch.where(t > 0, t, a * t)
            got = lib.ops.se_scale_res_prelu(x.cuda(), y.cuda(), None if r is None else r.cuda(), slope)
            assert np.array_equal(_bits(got), _bits(want)), (slope, r is None)
    one = lib.ops.se_scale_res_prelu(x[2:3].cuda(), y[2:3].cuda(), res[2:3].cuda(), -0.5)
    assert np.array_equal(_bits(one), _bits(lib.ops.se_scale_res_prelu(x.cuda(), y.cuda(), res.cuda(), -0.5)[2:3]))


@pytest.mark.parametrize('n', [1, 63, 65])
def test_cosine_rows_per_element(lib, ac, n):
    """rows 1, 4, 5 (four rows per block); norms 1, 1e-20 (the product falls below the 1e-8 floor: the floor decides) and 1e+18."""
    for rows in (1, 4, 5):
        for norm in (1.0, 1e-20, 1e18):
            x, y = ac.cosine_rows_family(rows, n, norm)
            got = _np(lib.ops.cosine_rows(_t(x), _t(y)))
            assert got.dtype == np.float64 and got.shape == (rows,)
            _gate(f'cosine_rows n {n} rows {rows} norm {norm:g}', got, ac.cosine_ref(x, y), ac.cosine_bound(x, y))
            if norm == 1e-20:
                assert float(np.abs(got).max()) < 1e-30 and (n > 1 or np.all(got != 0))


@pytest.mark.parametrize('dtype', ['uint8', 'float32'])
@pytest.mark.parametrize('shape', [(1, 1, 1, 3), (1, 2, 3, 3), (1, 127, 129, 3), (1, 300, 5, 3)])
def test_identity_input_small_and_odd_sizes_are_bitwise_the_host_definition(lib, shape, dtype):
    """One pixel, fewer pixels than taps, odd sizes either side of 128, a strip.  (tests/test_arcface_host.py holds the host definition against the
    float64 bilinear resize under arcface_check.identity_bound.)"""
    img = _image(shape, dtype, sum(shape))
    assert np.array_equal(_bits(lib.M.identity_input(img.cuda())), _bits(lib.M.identity_input(img)))


# ---- the block on the forms the network never reaches, per element -------------------------------------------------------------------
REACH_BLOCKS = {   # name: (planes, H, W, batch, the form conv1 and conv2 take)
    'wide_128': (128, 25, 41, 1, '128'),        # cout_pad % 128 == 0 and 1025 pixels: the first size past `narrow`
    'rung_32': (32, 9, 5, 1, '32'),
    'rows_17': (64, 8, 8, 17, '64'),            # the 32-row bn0 table
    'rows_33': (64, 8, 8, 33, '64'),            # the 64-row bn0 table
}
# (IRBlock(64, 96) does not exist on the device as a 32-wide form: ops._cout_pad(96) is 128, the packer has no cout_pad of 96)


@pytest.mark.parametrize('slope', (-0.5, 1.5))
@pytest.mark.parametrize('name', list(REACH_BLOCKS))
def test_block_on_the_forms_the_network_never_reaches(lib, ac, name, slope):
    from _tools import load_script
    c, H, W, B, form = REACH_BLOCKS[name]
    gc = load_script('tools/conv_geom_check.py')
    assert lib.ops._cout_pad(96) == 128
    for epi in gc.PRELU_EPIS:      # conv1 (AFFINE, PRELU) and conv2 (none, RES_PRELU) at the block's shape
        assert gc.route_of(0, gc.G(B, H, W, c, c, epi=epi, alpha=slope)) == ('prelu', form), (name, epi)
    blk = R.fill_state(lib.A.IRBlock(c, c, use_se=False), 500 + c + H, slope=slope).eval()
    x = torch.from_numpy(np.random.default_rng(c + B).normal(0., 1., (B, c, H, W)).astype(np.float32))
    with torch.no_grad():
        ref, bound = ac.block_ref(blk, x)
        e = float(((ac.block_emulate(blk, x).double() - ref).abs() / bound).max())
    blk = blk.cuda()
    dev = blk(x.cuda())
    r = _gate(f'IRBlock({c}, {c}) {H}x{W} batch {B} slope {slope} form {form}', _np(dev), ref.numpy(), bound.numpy())
    assert r >= 1e-3 * e, (name, r, e)
    if B > 16:
        assert blk._pre_tables(B)[0].shape[0] == B and blk._pre_tables(B)[0]._base is not None and blk._pre_tables(B)[0]._base.shape[0] == (32 if B == 17 else 64)
        for b in range(B):
            assert np.array_equal(_bits(blk(x[b:b + 1].cuda())), _bits(dev[b:b + 1])), b
