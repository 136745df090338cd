"""-m gpu: cf_deform_conv2d (the fp32-MFMA implicit GEMM with the fused bilinear gather, and the general kernel) per element against the
definition restated in tests/dcn_ref.py.  Exact family: bitwise; random family: |got - ref| <= (n + 16) 2^-24 S, worst ratio printed.
The cases, the bound and what each case is for stand in dcn_ref.py; every case is a few hundred microseconds of GPU work.  No NaN,
infinite or huge offset is sent to the GPU: their guard is the in-range test the moderate out-of-image offsets already take (checked by
reading; the CPU formula is tested on them in test_dcn_host.py).

Measured on an MI355X: the whole file 5.6 s, 77 tests, the slowest 2.8 s (the modules at their default deformable group: conv_offset has 27 and 18
channels there and goes through F.conv2d with its bias, and the first such call of a process takes 2.6 s -- timed alone; the module's own
deformable convolution is 9 ms, a second prediction below 1 ms), the next 0.19 s, every case below 0.2 s.  Every exact-family
case is bitwise on both routes.  Worst |got - ref| / bound of the random family: mod_dg4 0.0084, v1_s2d2 0.0124, groups 0.0131, k1 0.0463, tiles 0.0219,
odd (general) 0.0248; the general route forced on mod_dg4 / groups / v1_s2d2 0.0088 / 0.0131 / 0.0154; zero offsets against F.conv2d in float64
0.015 - 0.032.  The bound's 16 was not needed: no ratio comes near 1.

The second pass: the paths of the MFMA kernel that the first six cases do not reach (what each of the nine is for stands at the table of dcn_ref.py;
test_dcn_host.py pins by a model of the kernel's rule that reuse, reuse24, straddle and straddle2 keep a sample across K slabs and the five first MFMA
cases never do).  No defect was found: every new case and property passed on the kernel as it stood.  Worst |got - ref| / bound, random family,
MFMA route | general route forced (-: MFMA only):
    reuse 0.0066 | -        reuse24 0.0037 | 0.0037    straddle 0.0087 | 0.0084    straddle2 0.0222 | 0.0268    steps2 0.0366 | -
    steps3 0.0435 | -       k7 0.0024 | -              asym 0.0205 | 0.0194        gtiles 0.0266 | -
The two routes differ by at most 0.0069 of twice the bound (asym; straddle2 0.0058, the first cases 0.0044, straddle 0.0015, reuse24 0.0012) and not at
all on the exact family.  One pixel of x (twelve entries, both routes): 0.0019 - 0.0104 of the bound on the 96 - 576 outputs that read it, no other
output differs from the bias in a bit.  One NaN in x: 15.7 % (reuse24), 4.6 % (straddle), 2.1 % (straddle2), 2.3 % (asym) of the outputs are NaN, the
same set as the definition's on both routes, the rest within 0.0268.  The modules at deformable_groups = 1: 0.0044 (64 -> 64, modulated), 0.0087 (32 -> 32).

Scratch builds of cf_dcn.hip with one edit each (not committed; every address stays inside the kernel's own checks, so an edit can only give wrong
numbers), run once through this file.  old = the 32 tests of the first pass, new = the 45 of the second:
  boff[] back to CF_DCN_NO_LOAD at the top of gather   old: none.  new: 21 -- reuse, reuse24, straddle, straddle2 (both families), the route agreement, one-pixel
    (a kept sample reads nothing)                      and NaN tests of reuse24 / straddle / straddle2, the modules at their default
  prologue `nsteps > 1` -> `nsteps > 2`                old: none.  new: 2 -- steps2 (both families)
  a.sh <-> a.sw in fetch                               old: none.  new: 6 -- asym (both families), its route agreement (2), its one-pixel and NaN tests on mfma
  a.dh <-> a.dw in fetch                               old: none.  new: the same 6
  advance(nchunks, a.kh) for a.kw                      old: 1 -- test_modules_on_the_device (its (3, 5) DeformConv).  new: 10 -- steps2, steps3, asym (both
                                                       families), asym's route agreement (2), one-pixel and NaN tests
  `g = nt / a.ntn_g` -> `nt % a.groups`                old: none.  new: 3 -- gtiles (both families), its batch test on mfma
  general kernel: `c0 = c_lo`                          old: 5 -- odd (both families), zero offsets on odd, mod_dg4 forced (both): it counts channels twice
                                                       wherever DG > 1, cut or not.  new: 16 -- every forced-general case and property
  general kernel: c0 without the clamp to c_lo         old: none.  new: 6 -- straddle, straddle2 forced (both families), their NaN tests on general
  general kernel: c1 without the clamp to c_hi         old: none.  new: 8 -- those, and their one-pixel tests on general"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dcn_ref

pytestmark = pytest.mark.gpu
CASE_IDS = [(n, f) for n in dcn_ref.CASES for f in dcn_ref.FAMILIES]


@pytest.fixture(scope='module')
def ops():
    from codeformer_amd import build as cf_build
    from codeformer_amd import ops
    cf_build.build()
    assert torch.cuda.is_available()
    return ops


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


def _run(ops, inp, route=None, **over):
    a = dict(inp, **over)
    x = a['x'] if torch.is_tensor(a['x']) else _dev(a['x'])
    with torch.no_grad():
        out = ops.deform_conv2d(x, _dev(a['offset']), _dev(a['weight']), _dev(a['mask']), _dev(a['bias']), a['stride'], a['padding'],
                                a['dilation'], a['groups'], a['dg'], route=route)
    return out.cpu().numpy()


@pytest.mark.parametrize('name,family', CASE_IDS)
def test_case_matches_the_definition(ops, name, family):
    inp, val, S = dcn_ref.case(name, family)
    route = ops.deform_conv2d_route(inp['x'].shape, inp['weight'].shape, inp['groups'], inp['dg'])
    assert route == dcn_ref.CASES[name][12]
    dcn_ref.check(_run(ops, inp), name, family, inp, val, S, label=route + ' ')


@pytest.mark.parametrize('name', ['mod_dg4', 'groups', 'v1_s2d2', 'reuse24', 'straddle', 'straddle2', 'asym'])
@pytest.mark.parametrize('family', dcn_ref.FAMILIES)
def test_general_route_on_an_mfma_case(ops, name, family):
    """The general kernel forced by the `route` argument: the definition again, and the two routes within twice the bound of each other.
    straddle / straddle2 are the inputs on which its clamps of a deformable group's channel range to the group (c0, c1) cut anything."""
    inp, val, S = dcn_ref.case(name, family)
    gen, fast = _run(ops, inp, route='general'), _run(ops, inp, route='mfma')
    dcn_ref.check(gen, name, family, inp, val, S, label='general(forced) ')
    diff = np.abs(gen.astype(np.float64) - fast)
    b2 = 2 * dcn_ref.bound(inp['weight'], S)
    print(f'dcn routes {name}/{family}: worst |general - mfma| / (2 bound) = {float((diff / np.maximum(b2, 1e-300)).max()):.4f}')
    assert (diff <= b2).all()
    with pytest.raises(ValueError):
        _run(ops, dcn_ref.case('odd', family)[0], route='mfma')


@pytest.mark.parametrize('name', ['mod_dg4', 'odd'])
@pytest.mark.parametrize('sign', [1.0, -1.0])
def test_offsets_outside_the_image_leave_the_bias(ops, name, sign):
    """Every offset between the image size and image size + 5 away (moderately outside): out == bias, bitwise (zeros for the plain op)."""
    inp = dict(dcn_ref.make_inputs(name, 'random'))
    H, W = inp['x'].shape[2:]
    # a tap's base position lies within [-pad, size + pad): beyond +-(size + 2) every sample is out of range
    inp['offset'] = (sign * (max(H, W) + 2 + np.random.default_rng(5).uniform(0, 3, inp['offset'].shape))).astype(np.float32)
    assert np.abs(inp['offset']).max() <= max(H, W) + 5
    out = _run(ops, inp)
    want = np.zeros_like(out) if inp['bias'] is None else np.broadcast_to(inp['bias'].reshape(1, -1, 1, 1), out.shape)
    assert (out.view(np.uint32) == np.ascontiguousarray(want).view(np.uint32)).all()


@pytest.mark.parametrize('name', ['mod_dg4', 'v1_s2d2', 'groups', 'odd'])
def test_zero_offsets_are_the_plain_convolution(ops, name):
    inp = dict(dcn_ref.make_inputs(name, 'random'))
    inp['offset'] = np.zeros_like(inp['offset'])
    inp['mask'] = None if inp['mask'] is None else np.ones_like(inp['mask'])
    _, S = dcn_ref.deform_conv_ref(**inp)
    t = torch.from_numpy
    ref = F.conv2d(t(inp['x']).double(), t(inp['weight']).double(), None if inp['bias'] is None else t(inp['bias']).double(), inp['stride'],
                   inp['padding'], inp['dilation'], inp['groups']).numpy()
    err = np.abs(_run(ops, inp).astype(np.float64) - ref)
    b = dcn_ref.bound(inp['weight'], S)
    print(f'dcn zero offsets {name}: worst ratio {float((err / b).max()):.4f}')
    assert (err <= b).all()


@pytest.mark.parametrize('name', ['mod_dg4', 'odd'])
def test_channels_last_input_gives_the_same_bits(ops, name):
    inp, _, _ = dcn_ref.case(name, 'random')
    x = _dev(inp['x'])
    xcl = x.contiguous(memory_format=torch.channels_last)
    assert xcl.stride() != x.stride()
    a, b = _run(ops, inp, x=x), _run(ops, inp, x=xcl)
    assert (a.view(np.uint32) == b.view(np.uint32)).all()


@pytest.mark.parametrize('route', ['mfma', 'general'])
def test_batch_invariance_and_repeatability(ops, route):
    """Rows of the B = 2 call are bitwise the B = 1 calls; a second run gives the same bits."""
    inp, _, _ = dcn_ref.case('mod_dg4', 'random')
    both = _run(ops, inp, route=route)
    assert (both.view(np.uint32) == _run(ops, inp, route=route).view(np.uint32)).all()
    for b in range(2):
        one = {k: (v[b:b + 1] if k in ('x', 'offset', 'mask') else v) for k, v in inp.items()}
        assert (_run(ops, one, route=route).view(np.uint32) == both[b:b + 1].view(np.uint32)).all()


@pytest.mark.parametrize('route', ['mfma', 'general'])
def test_batch_invariance_and_repeatability_with_groups_and_n_tiles(ops, route):
    """gtiles (two groups x two N tiles, ragged M tiles): each of the three images run alone gives the bits it has inside the batch."""
    inp, _, _ = dcn_ref.case('gtiles', 'random')
    whole = _run(ops, inp, route=route)
    assert (whole.view(np.uint32) == _run(ops, inp, route=route).view(np.uint32)).all()
    for b in range(3):
        one = {k: (v[b:b + 1] if k in ('x', 'offset', 'mask') else v) for k, v in inp.items()}
        assert (_run(ops, one, route=route).view(np.uint32) == whole[b:b + 1].view(np.uint32)).all(), b


@pytest.mark.parametrize('route', ['mfma', 'general'])
@pytest.mark.parametrize('name', list(dcn_ref.PIXELS))
def test_one_pixel_of_x_reaches_the_outputs_that_sample_it(ops, name, route):
    """x zero but for one entry (interior; a corner of the image; the last channel of a deformable group, in straddle / straddle2 of the one the
    groups cut): the bound on the few terms that read it, and bitwise the bias -- +0 for the plain op -- everywhere else."""
    for which in range(3):
        dcn_ref.check_one_pixel(_run(ops, dcn_ref.one_pixel_case(name, which)[0], route=route), name, which, label=route + ' ')


@pytest.mark.parametrize('route', ['mfma', 'general'])
@pytest.mark.parametrize('name', list(dcn_ref.PIXELS))
def test_a_nan_pixel_of_x_reaches_the_outputs_that_sample_it(ops, name, route):
    """One NaN in x (offsets and mask finite and moderate, as everywhere in this file): the NaN outputs are the definition's, the rest within the
    bound."""
    dcn_ref.check_nan_pixel(_run(ops, dcn_ref.nan_pixel_case(name)[0], route=route), name, label=route + ' ')


def test_packed_weight_follows_the_weight(ops):
    """The packing kept on the weight tensor is rebuilt when the tensor is written in place."""
    inp, val, S = dcn_ref.case('groups', 'exact')
    w = _dev(inp['weight'])
    args = (_dev(inp['x']), _dev(inp['offset']), w, _dev(inp['mask']), _dev(inp['bias']), 1, 1, 1, 2, 2)
    with torch.no_grad():
        first = ops.deform_conv2d(*args).cpu().numpy()
        assert ops.deform_conv2d(*args).cpu().numpy().tobytes() == first.tobytes() and hasattr(w, '_cf_dcn')
        w.mul_(2.0)
        doubled = ops.deform_conv2d(*args).cpu().numpy()
    dcn_ref.check(first, 'groups', 'exact', inp, val, S, label='cached ')
    b = inp['bias'].reshape(1, -1, 1, 1)
    assert (doubled == 2 * (first - b) + b).all()


def _with_its_own_prediction(module, x):
    """(module(x), the offsets -- and mask -- its conv_offset predicted inside that very call)."""
    seen, predict = [], module.offset_mask
    module.offset_mask = lambda t: seen.append(predict(t)) or seen[-1]
    try:
        out = module(x)
    finally:
        del module.offset_mask
    assert len(seen) == 1
    return out, seen[0]


def test_modules_at_their_default_deformable_group(ops):
    """deformable_groups left at 1: every 16-channel slab of a tap shares one sample, so the MFMA kernel resamples on one gather of four (64
    channels) or two (32).  Against the definition, given the offsets and the mask the module predicted for itself."""
    from basicsr.ops.dcn import DeformConvPack, ModulatedDeformConvPack
    torch.manual_seed(1)
    with torch.no_grad():
        m = ModulatedDeformConvPack(64, 64, 3, padding=1).cuda().eval()
        m.conv_offset.weight.data.normal_(0, 0.05)
        m.conv_offset.bias.data.normal_(0, 0.5)
        m.bias.data.normal_()
        x = torch.randn(1, 64, 10, 18, device='cuda')
        got, (offset, mask) = _with_its_own_prediction(m, x)
        assert m.deformable_groups == 1 and offset.shape == (1, 18, 10, 18) and mask.shape == (1, 9, 10, 18)
        assert ops.deform_conv2d_route(x.shape, m.weight.shape, 1, 1) == 'mfma' and dcn_ref.reuse_counts(64, 1, 1, 9) == (108, 144)
        val, S = dcn_ref.deform_conv_ref(x.cpu().numpy(), offset.cpu().numpy(), m.weight.cpu().numpy(), mask.cpu().numpy(), m.bias.cpu().numpy(),
                                         (1, 1), (1, 1), (1, 1), 1, 1)
        err, b = np.abs(got.cpu().numpy().astype(np.float64) - val), dcn_ref.bound(m.weight.cpu().numpy(), S)
        print(f'dcn ModulatedDeformConvPack(64, 64, 3) at its default: worst |got - ref| / bound = {float((err / b).max()):.4f}')
        assert (err <= b).all()
        p = DeformConvPack(32, 32, 3, padding=1).cuda().eval()
        p.conv_offset.weight.data.normal_(0, 0.05)
        p.conv_offset.bias.data.normal_(0, 0.5)
        xs = torch.randn(1, 32, 10, 18, device='cuda')
        got, (offset,) = _with_its_own_prediction(p, xs)
        assert p.deformable_groups == 1 and offset.shape == (1, 18, 10, 18) and ops.deform_conv2d_route(xs.shape, p.weight.shape, 1, 1) == 'mfma'
        val, S = dcn_ref.deform_conv_ref(xs.cpu().numpy(), offset.cpu().numpy(), p.weight.cpu().numpy(), None, None, (1, 1), (1, 1), (1, 1), 1, 1)
        err, b = np.abs(got.cpu().numpy().astype(np.float64) - val), dcn_ref.bound(p.weight.cpu().numpy(), S)
        print(f'dcn DeformConvPack(32, 32, 3) at its default: worst |got - ref| / bound = {float((err / b).max()):.4f}')
        assert (err <= b).all()


def test_modules_on_the_device(ops):
    from basicsr.ops.dcn import DeformConv, DeformConvPack, ModulatedDeformConvPack, deform_conv, modulated_deform_conv
    torch.manual_seed(0)
    m = ModulatedDeformConvPack(32, 48, 3, stride=1, padding=1, dilation=1, deformable_groups=4).cuda().eval()
    m.conv_offset.weight.data.normal_(0, 0.05)
    m.conv_offset.bias.data.normal_(0, 0.5)
    m.bias.data.normal_()
    x = torch.randn(2, 32, 19, 23, device='cuda')
    with torch.no_grad():
        got = m(x)
        offset, mask = m.offset_mask(x)
        assert torch.equal(got, modulated_deform_conv(x, offset, mask, m.weight, m.bias, m.stride, m.padding, m.dilation, m.groups, m.deformable_groups))
        # conv_offset runs on the library's general-geometry implicit GEMM (cout 108): F.conv2d within that convolution's own bound
        raw = F.conv2d(x.double(), m.conv_offset.weight.double(), m.conv_offset.bias.double(), 1, 1)
        S = F.conv2d(x.double().abs(), m.conv_offset.weight.double().abs(), m.conv_offset.bias.double().abs(), 1, 1)
        assert offset.shape == (2, 72, 19, 23) and mask.shape == (2, 36, 19, 23)
        assert ((offset.double() - raw[:, :72]).abs() <= (288 + 16) * 2.0 ** -24 * S[:, :72]).all()
        assert ((mask.double() - torch.sigmoid(raw[:, 72:])).abs() <= (288 + 16) * 2.0 ** -24 * S[:, 72:] + 2.0 ** -23).all()   # (sigmoid: slope <= 1/4, one more rounding)
        # ... and the module against the definition, given those offsets and mask
        val, S = dcn_ref.deform_conv_ref(x.cpu().numpy(), offset.cpu().numpy(), m.weight.cpu().numpy(), mask.cpu().numpy(), m.bias.cpu().numpy(),
                                         (1, 1), (1, 1), (1, 1), 1, 4)
        assert (np.abs(got.cpu().numpy().astype(np.float64) - val) <= dcn_ref.bound(m.weight.cpu().numpy(), S)).all()
        p = DeformConvPack(16, 32, 3, padding=1, deformable_groups=2).cuda().eval()     # conv_offset: 36 channels
        p.conv_offset.weight.data.normal_(0, 0.05)
        xs = torch.randn(1, 16, 10, 11, device='cuda')
        assert torch.equal(p(xs), deform_conv(xs, *p.offset_mask(xs), p.weight, p.stride, p.padding, p.dilation, p.groups, p.deformable_groups))
        # an input smaller than the kernel: padded at the bottom / right, cropped back
        d = DeformConv(16, 8, (3, 5), padding=(1, 2)).cuda().eval()
        xs, off = torch.randn(1, 16, 2, 3, device='cuda'), torch.rand(1, 30, 2, 3, device='cuda') * 2 - 1
        small = d(xs, off)
        full = deform_conv(F.pad(xs, (0, 2, 0, 1)), F.pad(off, (0, 2, 0, 1)), d.weight, (1, 1), (1, 2))
        assert small.shape == (1, 8, 2, 3) and torch.equal(small, full[:, :, :2, :3])
        val, S = dcn_ref.deform_conv_ref(F.pad(xs, (0, 2, 0, 1)).cpu().numpy(), F.pad(off, (0, 2, 0, 1)).cpu().numpy(), d.weight.cpu().numpy(),
                                         None, None, (1, 1), (1, 2), (1, 1), 1, 1)
        assert (np.abs(small.cpu().numpy().astype(np.float64) - val[:, :, :2, :3]) <= dcn_ref.bound(d.weight.cpu().numpy(), S[:, :, :2, :3])).all()
    with pytest.raises(RuntimeError):
        m(x)                                     # grad enabled, parameters require grad
    with pytest.raises(TypeError):
        with torch.no_grad():
            modulated_deform_conv(x.half(), offset.half(), mask.half(), m.weight.half(), None, 1, 1, 1, 1, 4)
