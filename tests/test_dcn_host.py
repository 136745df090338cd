"""CPU: the basicsr.ops.dcn surface (codeformer_amd/dcn.py), the C ABI's argument checks and the float32 host formula of the deformable
convolution, against the definition restated in tests/dcn_ref.py.  No golden of the reference exists (its extension is CUDA-only): parity
is by definition."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dcn_ref
from codeformer_amd import build as cf_build
from codeformer_amd import lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('cf_deform_conv2d', 'cf_deform_conv2d_packed_elems', 'cf_pack_deform_conv_weight')
CASE_IDS = [(n, f) for n in dcn_ref.CASES for f in dcn_ref.FAMILIES]


def _t(a):
    return None if a is None else torch.from_numpy(np.array(a))   # (a copy: the shared case arrays are read-only)


def _host(inp, **over):
    from codeformer_amd.dcn import deform_conv2d_host
    a = dict(inp, **over)
    with torch.no_grad():
        return deform_conv2d_host(_t(a['x']), _t(a['offset']), _t(a['weight']), _t(a['mask']), _t(a['bias']), a['stride'], a['padding'],
                                  a['dilation'], a['groups'], a['dg'])


@pytest.fixture(scope='module')
def native():
    cf_build.build()
    return lib.load()


def test_import_surface_resolves():
    import basicsr.ops.dcn as m
    from basicsr.ops.dcn import ModulatedDeformConvPack, modulated_deform_conv  # noqa: F401
    for name in ('deform_conv', 'modulated_deform_conv', 'DeformConv', 'DeformConvPack', 'ModulatedDeformConv', 'ModulatedDeformConvPack',
                 'DeformConvFunction', 'ModulatedDeformConvFunction'):
        assert name in m.__all__ and getattr(m, name) is not None
    assert m.DeformConvFunction.apply is m.deform_conv and m.ModulatedDeformConvFunction.apply is m.modulated_deform_conv


def test_symbols_declared_and_bound(native):
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'codeformer_hip.h')).read(), flags=re.S)
    for s in NEW_SYMBOLS:
        assert re.search(r'\b%s\s*\(' % s, src), s
        assert s in lib.SIGNATURES and hasattr(native, s)
    assert lib.ABI_VERSION == 22 and native.cf_version() == 22
    assert native.cf_deform_conv2d_packed_elems(48, 32, 9, 1) == 9 * 32 * 64
    assert native.cf_deform_conv2d_packed_elems(32, 32, 9, 2) == 2 * 9 * 16 * 64
    assert native.cf_deform_conv2d_packed_elems(32, 30, 9, 4) == -1


def test_bad_arguments_are_reported_without_a_gpu(native):
    def call(x=1, off=1, w=1, out=1, B=1, cin=16, H=8, W=8, cout=16, kh=3, kw=3, s=(1, 1), p=(1, 1), d=(1, 1), G=1, DG=1, nhwc=1, route=1):
        return native.cf_deform_conv2d(x, off, None, w, None, out, B, cin, H, W, cout, kh, kw, s[0], s[1], p[0], p[1], d[0], d[1], G, DG, nhwc, route, None)
    assert call(x=None) == -1 and 'null' in lib.last_error()
    assert call(H=0) == -1 and 'bad dims' in lib.last_error()
    assert call(s=(0, 1)) == -1 and 'stride' in lib.last_error()
    assert call(G=3) == -1 and 'groups' in lib.last_error()
    assert call(DG=3) == -1 and 'deformable groups' in lib.last_error()
    assert call(route=2) == -1 and 'route' in lib.last_error()
    assert call(H=1, p=(0, 0)) == -1 and 'smaller than the dilated kernel' in lib.last_error()
    assert call(cin=24, cout=24) == -1 and 'mfma route' in lib.last_error()            # (cin/G) % 16
    assert call(cin=16, DG=8) == -1 and 'mfma route' in lib.last_error()               # (cin/DG) % 4
    assert call(kh=8, kw=8, p=(4, 4)) == -1 and 'mfma route' in lib.last_error()       # kh*kw > 49
    assert call(nhwc=0) == -1 and 'channels-last' in lib.last_error()
    assert call(x=20) == -1 and 'aligned' in lib.last_error()
    assert native.cf_pack_deform_conv_weight(None, 16, 16, 9, 1, 1, None) == -1 and 'null' in lib.last_error()
    assert native.cf_pack_deform_conv_weight(1, 16, 24, 9, 1, 1, None) == -1 and 'multiple of 16' in lib.last_error()
    assert native.cf_pack_deform_conv_weight(1, 16, 16, 50, 1, 1, None) == -1 and 'taps' in lib.last_error()
    assert native.cf_pack_deform_conv_weight(1, 16, 16, 9, 3, 1, None) == -1 and 'groups' in lib.last_error()


@pytest.mark.parametrize('name,family', CASE_IDS)
def test_host_formula_matches_the_definition(name, family):
    inp, val, S = dcn_ref.case(name, family)
    dcn_ref.check(_host(inp).numpy(), name, family, inp, val, S, label='host ')


@pytest.mark.parametrize('name', list(dcn_ref.CASES))
def test_routes(name):
    c = dcn_ref.CASES[name]
    assert ops.deform_conv2d_route((c[0], c[1], c[3], c[4]), (c[2], c[1] // c[9], *c[5]), c[9], c[10]) == c[12]


def test_which_cases_keep_a_sample_across_slabs():
    """The MFMA kernel's reuse branch by dcn_ref.reuse_counts, the model of its rule: the four reuse cases take it, the five first cases never do --
    an edit of the table cannot lose the coverage unnoticed."""
    mfma = [n for n, c in dcn_ref.CASES.items() if c[12] == 'mfma']
    assert set(dcn_ref.REUSE_CASES) | set(dcn_ref.NO_REUSE_CASES) <= set(mfma)
    counts = {n: dcn_ref.case_reuse_counts(n) for n in mfma}
    print('dcn reuse (reused, gathers):', counts)
    assert {n: counts[n] for n in dcn_ref.NO_REUSE_CASES} == {'mod_dg4': (0, 72), 'v1_s2d2': (0, 36), 'groups': (0, 72), 'k1': (0, 4), 'tiles': (0, 36)}
    for n in dcn_ref.REUSE_CASES:
        assert 0 < counts[n][0] < counts[n][1], n
    assert counts['reuse'] == (36, 72)
    # reuse24: of a pixel's four threads some reuse at a slab and some resample (channels 16..23 against 24..31)
    cin, dg = dcn_ref.CASES['reuse24'][1], dcn_ref.CASES['reuse24'][10]
    d_of = [[(4 * k4 + 16 * slab) // (cin // dg) for slab in range(cin // 16)] for k4 in range(4)]
    assert d_of == [[0, 0, 1], [0, 0, 1], [0, 1, 1], [0, 1, 1]]
    for n in set(dcn_ref.PIXELS) & set(dcn_ref.REUSE_CASES):                 # the property cases put an entry where the sample is a kept one
        c = dcn_ref.CASES[n]
        assert any(e[1] in dcn_ref.reused_channels(c[1], c[9], c[10]) for e in dcn_ref.PIXELS[n]), n
    # the modules at their default deformable_groups = 1 take it too, the benchmark's shape (64 channels, 8 deformable groups) does not
    assert dcn_ref.reuse_counts(64, 1, 1, 9) == (108, 144) and dcn_ref.reuse_counts(32, 1, 1, 9) == (36, 72) and dcn_ref.reuse_counts(64, 1, 8, 9)[0] == 0
    # the step counts of the pipeline cases: taps x slabs
    steps = {n: c[5][0] * c[5][1] * (c[1] // c[9] // 16) for n, c in dcn_ref.CASES.items()}
    assert steps['steps2'] == 2 and steps['steps3'] == 3 and steps['k1'] == 1 and steps['k7'] == 49
    # gtiles: two N tiles per group, the second 16 channels wide; straddle(2): a deformable group spans a group boundary and the reverse
    c = dcn_ref.CASES['gtiles']
    assert c[9] == 2 and c[2] // c[9] == 64 + 16 and c[0] == 3 and c[3] % 4 and c[4] % 16
    for n in ('straddle', 'straddle2'):
        c = dcn_ref.CASES[n]
        assert (c[1] // c[9]) % (c[1] // c[10]) and (c[1] // c[10]) % (c[1] // c[9])


@pytest.mark.parametrize('name', list(dcn_ref.PIXELS))
def test_one_pixel_and_nan_pixel_on_the_host_formula(name):
    """The property cases of the GPU file on the float32 host formula: one entry of x reaches only the outputs whose samples read it, and a NaN
    entry makes exactly those NaN."""
    for which in range(3):
        inp = dcn_ref.one_pixel_case(name, which)[0]
        dcn_ref.check_one_pixel(_host(inp).numpy(), name, which, label='host ')
    c = dcn_ref.CASES[name]
    cpdg, cin_g = c[1] // c[10], c[1] // c[9]
    assert (dcn_ref.PIXELS[name][2][1] + 1) % cpdg == 0                         # the last channel of a deformable group
    if c[9] > 1:                                                              # ... of one that the groups cut
        d = dcn_ref.PIXELS[name][2][1] // cpdg
        assert d * cpdg // cin_g != ((d + 1) * cpdg - 1) // cin_g
    inp, val, _ = dcn_ref.nan_pixel_case(name)
    dcn_ref.check_nan_pixel(_host(inp).numpy(), name, label='host ')
    nan = np.isnan(val)
    g = dcn_ref.PIXELS[name][0][1] // cin_g                                   # every channel of the entry's group alike, no other channel
    cout_g = c[2] // c[9]
    assert (nan[:, g * cout_g:(g + 1) * cout_g] == nan[:, g * cout_g:g * cout_g + 1]).all() and nan.sum() == cout_g * nan[:, g * cout_g].sum()
    if name == 'reuse24':
        assert abs(nan.mean() - 0.157) < 0.0005


def test_route_rule():
    r = ops.deform_conv2d_route
    assert r((1, 64, 8, 8), (64, 64, 3, 3), 1, 8) == 'mfma' and r((1, 64, 8, 8), (64, 64, 7, 7), 1, 16) == 'mfma'
    assert r((1, 64, 8, 8), (64, 64, 3, 3), 1, 32) == 'general'     # 2 channels per deformable group
    assert r((1, 24, 8, 8), (24, 24, 3, 3), 1, 1) == 'general'      # cin/G % 16
    assert r((1, 64, 8, 8), (64, 8, 3, 3), 8, 1) == 'general'
    assert r((1, 64, 8, 8), (64, 64, 8, 8), 1, 1) == 'general'      # 64 taps
    assert r((1, 32, 8, 8), (8, 32, 3, 2), 1, 2) == 'mfma'          # non-square kernels are covered


def test_zero_offsets_are_the_plain_convolution():
    """offset = 0, mask = 1: F.conv2d in float64, within the bound (S of the helper)."""
    for name in ('mod_dg4', 'v1_s2d2', 'groups', 'odd'):
        inp = dict(dcn_ref.make_inputs(name, 'random'))
        inp['offset'] = np.zeros_like(inp['offset'])
        inp['mask'] = None if inp['mask'] is None else np.ones_like(inp['mask'])
        _, S = dcn_ref.deform_conv_ref(**inp)
        ref = F.conv2d(_t(inp['x']).double(), _t(inp['weight']).double(), None if inp['bias'] is None else _t(inp['bias']).double(),
                       inp['stride'], inp['padding'], inp['dilation'], inp['groups']).numpy()
        err = np.abs(_host(inp).numpy().astype(np.float64) - ref)
        assert (err <= dcn_ref.bound(inp['weight'], S)).all(), name


@pytest.mark.parametrize('dy,dx', [(2, -1), (-3, 0), (0, 4)])
def test_integer_offsets_shift_the_input(dy, dx):
    """The same integer offset at every tap: the convolution of x shifted by it, zero-filled."""
    inp = dict(dcn_ref.make_inputs('mod_dg4', 'random'))
    off = np.zeros_like(inp['offset'])
    off[:, 0::2], off[:, 1::2] = dy, dx
    inp['offset'], inp['mask'] = off, np.ones_like(inp['mask'])
    x = inp['x']
    H, W = x.shape[2:]
    P = 1 + max(abs(dy), abs(dx))   # the padded frame (padding 1) of the image shifted by (dy, dx): a window of x zero-filled all round
    xp = np.pad(x, ((0, 0), (0, 0), (P, P), (P, P)))
    window = xp[:, :, P - 1 + dy:P - 1 + dy + H + 2, P - 1 + dx:P - 1 + dx + W + 2]
    ref = F.conv2d(_t(window).double(), _t(inp['weight']).double(), _t(inp['bias']).double(), 1, 0).numpy()
    _, S = dcn_ref.deform_conv_ref(**inp)
    assert (np.abs(_host(inp).numpy().astype(np.float64) - ref) <= dcn_ref.bound(inp['weight'], S)).all()


@pytest.mark.parametrize('sign', [1.0, -1.0])
def test_far_offsets_leave_the_bias(sign):
    inp = dict(dcn_ref.make_inputs('mod_dg4', 'random'))
    H, W = inp['x'].shape[2:]
    rng = np.random.default_rng(3)
    inp['offset'] = (sign * (max(H, W) + 5 + rng.uniform(0, 40, inp['offset'].shape))).astype(np.float32)
    out = _host(inp).numpy()
    assert (out == inp['bias'].reshape(1, -1, 1, 1)).all()
    val, _ = dcn_ref.deform_conv_ref(**inp)
    assert (val == inp['bias'].astype(np.float64).reshape(1, -1, 1, 1)).all()


@pytest.mark.parametrize('bad', [float('nan'), float('inf'), float('-inf'), 1e30, -1e30])
def test_non_finite_and_huge_offsets_sample_nothing(bad):
    """NaN / +-inf / 1e30 in either offset of a tap: that tap contributes 0, i.e. the result with the tap's mask set to 0 -- exactly."""
    inp = dict(dcn_ref.make_inputs('mod_dg4', 'exact'))
    K = 9
    for which in (0, 1):
        off, mask = inp['offset'].copy(), inp['mask'].copy()
        for d, k in ((0, 4), (3, 8), (1, 0)):
            off[:, (d * K + k) * 2 + which] = bad
            mask[:, d * K + k] = 0
        got = _host(inp, offset=off).numpy()
        want = _host(inp, mask=mask).numpy()
        assert np.isfinite(got).all() and (got == want).all()


def test_the_image_border_of_a_sample():
    """1x1 kernel on one channel, weight 1: h = -1 and h = H contribute 0, h = H - 0.5 half of the last row, h = -0.5 half of the first."""
    H, W = 5, 4
    x = torch.arange(1, H * W + 1, dtype=torch.float32).reshape(1, 1, H, W)
    w = torch.ones(1, 1, 1, 1)
    from codeformer_amd.dcn import deform_conv2d_host

    def rows_at(h):   # every output pixel (y, x) samples position (h, x): by the host formula and by the helper
        off = torch.zeros(1, 2, H, W)
        off[0, 0] = h - torch.arange(H, dtype=torch.float32)[:, None]
        got = deform_conv2d_host(x, off, w)[0, 0]
        ref, _ = dcn_ref.deform_conv_ref(x.numpy(), off.numpy(), w.numpy())
        assert (got.numpy() == ref[0, 0]).all()
        return got
    assert (rows_at(-1.0) == 0).all() and (rows_at(float(H)) == 0).all()
    assert (rows_at(H - 0.5) == 0.5 * x[0, 0, H - 1]).all()
    assert (rows_at(-0.5) == 0.5 * x[0, 0, 0]).all()
    assert (rows_at(H - 1.0) == x[0, 0, H - 1]).all()


def test_shape_errors():
    from basicsr.ops.dcn import deform_conv, modulated_deform_conv
    x, w = torch.zeros(1, 8, 6, 6), torch.zeros(4, 8, 3, 3)
    off, mask = torch.zeros(1, 18, 6, 6), torch.zeros(1, 9, 6, 6)
    assert modulated_deform_conv(x, off, mask, w, None, 1, 1, 1, 1, 1).shape == (1, 4, 6, 6)
    with pytest.raises(ValueError):
        modulated_deform_conv(x, torch.zeros(1, 16, 6, 6), mask, w, None, 1, 1, 1, 1, 1)
    with pytest.raises(ValueError):
        modulated_deform_conv(x, off, torch.zeros(1, 18, 6, 6), w, None, 1, 1, 1, 1, 1)
    with pytest.raises(ValueError):
        modulated_deform_conv(x, off, mask, w, None, 1, 1, 1, 3, 1)        # groups 3 does not divide 8
    with pytest.raises(ValueError):
        deform_conv(x, off, w, 1, 1, 1, 1, 3)                              # deformable groups 3 does not divide 8
    with pytest.raises(ValueError):
        deform_conv(x, off, torch.zeros(4, 4, 3, 3), 1, 1, 1, 1, 1)        # weight of cin/2 channels with groups 1
    with pytest.raises(ValueError):
        deform_conv(x[0], off, w)
    with pytest.raises(AssertionError):
        deform_conv(torch.zeros(3, 8, 6, 6), torch.zeros(3, 18, 6, 6), w, 1, 1, 1, 1, 1, 2)    # im2col_step 2 does not divide batch 3
    for dt in (torch.float16, torch.bfloat16):
        with pytest.raises(TypeError):
            modulated_deform_conv(x.to(dt), off.to(dt), mask.to(dt), w.to(dt), None, 1, 1, 1, 1, 1)


def test_grad_is_refused():
    from basicsr.ops.dcn import ModulatedDeformConvPack, modulated_deform_conv
    x, w = torch.zeros(1, 8, 6, 6), torch.zeros(4, 8, 3, 3, requires_grad=True)
    off, mask = torch.zeros(1, 18, 6, 6), torch.zeros(1, 9, 6, 6)
    with pytest.raises(RuntimeError):
        modulated_deform_conv(x, off, mask, w, None, 1, 1, 1, 1, 1)
    with pytest.raises(RuntimeError):
        ModulatedDeformConvPack(8, 4, 3, padding=1)(x)
    with torch.no_grad():
        assert modulated_deform_conv(x, off, mask, w, None, 1, 1, 1, 1, 1).shape == (1, 4, 6, 6)


def test_state_dict_keys_and_shapes():
    from basicsr.ops.dcn import DeformConv, DeformConvPack, ModulatedDeformConv, ModulatedDeformConvPack

    def sd(m):
        return {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert sd(DeformConv(16, 8, 3, padding=1, groups=2, deformable_groups=4)) == {'weight': (8, 8, 3, 3)}
    assert sd(DeformConvPack(16, 8, (3, 2), padding=1, deformable_groups=4)) == {
        'weight': (8, 16, 3, 2), 'conv_offset.weight': (48, 16, 3, 2), 'conv_offset.bias': (48,)}
    assert sd(ModulatedDeformConv(16, 8, 3, padding=1, groups=2)) == {'weight': (8, 8, 3, 3), 'bias': (8,)}
    assert sd(ModulatedDeformConv(16, 8, 3, bias=False)) == {'weight': (8, 16, 3, 3)}
    assert sd(ModulatedDeformConvPack(16, 8, 3, stride=1, padding=1, dilation=1, deformable_groups=2)) == {
        'weight': (8, 16, 3, 3), 'bias': (8,), 'conv_offset.weight': (54, 16, 3, 3), 'conv_offset.bias': (54,)}
    m = ModulatedDeformConvPack(16, 8, 3, padding=1, deformable_groups=2)
    assert not m.conv_offset.weight.any() and not m.conv_offset.bias.any() and not m.bias.any()
    assert 0 < float(m.weight.detach().abs().max()) <= 1.0 / (16 * 9) ** 0.5
    assert m.kernel_size == (3, 3) and m.stride == 1 and m.with_bias is True and m._version == 2
    d = DeformConvPack(16, 8, 3, padding=1)
    assert d.stride == (1, 1) and d.padding == (1, 1) and not d.conv_offset.weight.any() and d._version == 2
    with pytest.raises(AssertionError):
        DeformConv(16, 8, 3, bias=True)


def test_fresh_modulated_pack_is_half_the_convolution():
    from basicsr.ops.dcn import DeformConvPack, ModulatedDeformConvPack
    torch.manual_seed(0)
    m = ModulatedDeformConvPack(8, 6, 3, stride=1, padding=1, deformable_groups=2).eval()
    m.bias.data.normal_()
    x = torch.randn(2, 8, 7, 9)
    with torch.no_grad():
        got = m(x)
        offset, mask = m.offset_mask(x)
        want = 0.5 * F.conv2d(x.double(), m.weight.double(), None, 1, 1) + m.bias.double().reshape(1, -1, 1, 1)
        assert not offset.any() and (mask == 0.5).all() and offset.shape == (2, 36, 7, 9) and mask.shape == (2, 18, 7, 9)
        _, S = dcn_ref.deform_conv_ref(x.numpy(), offset.numpy(), m.weight.numpy(), mask.numpy(), m.bias.numpy(), (1, 1), (1, 1), (1, 1), 1, 2)
        assert (np.abs(got.double().numpy() - want.numpy()) <= dcn_ref.bound(m.weight.numpy(), S)).all()
        d = DeformConvPack(8, 6, 3, padding=1).eval()
        _, S = dcn_ref.deform_conv_ref(x.numpy(), d.offset_mask(x)[0].numpy(), d.weight.numpy(), None, None, (1, 1), (1, 1), (1, 1), 1, 1)
        assert (np.abs(d(x).double().numpy() - F.conv2d(x.double(), d.weight.double(), None, 1, 1).numpy()) <= dcn_ref.bound(d.weight.numpy(), S)).all()


def test_deform_conv_pads_an_input_smaller_than_its_kernel():
    from basicsr.ops.dcn import DeformConv, deform_conv
    torch.manual_seed(1)
    m = DeformConv(4, 3, (3, 5), padding=(1, 2)).eval()
    x, off = torch.randn(1, 4, 2, 3), torch.rand(1, 30, 2, 3)
    with torch.no_grad():
        got = m(x, off)
        full = deform_conv(F.pad(x, (0, 2, 0, 1)), F.pad(off, (0, 2, 0, 1)), m.weight, (1, 1), (1, 2))
    assert got.shape == (1, 3, 2, 3) and torch.equal(got, full[:, :, :2, :3])
