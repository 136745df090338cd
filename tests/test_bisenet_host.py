"""No GPU: BiSeNet's module tree, its host and folded dataflows against the recorded reference, the public loaders, what the device path
refuses, the numpy restatements of the kernel definitions against stock torch, and the argument checks of the cf_bisenet.hip entry points.

The gate is the yardstick of the scoring tests: e(x) = max|x - ref64| / max|ref64| at the fixture's sample positions, e(forward_host) <= 8
e(float32 reference) -- not bitwise equality, another CPU gives other float32 bits (profiles/NOTES.md).  In float64 the folded dataflow
(BatchNorm in the weights, the centre-tap shortcut, the x2 sub-pixel decomposition, the pooled single-layer gates) is the module to 1e-12.
"""
import copy

import numpy as np
import pytest
import torch
from torch.nn import functional as F

import bisenet_ref as R
from _tools import MARGIN, load_script
from codeformer_amd.facelib import parsing as P
from codeformer_amd.facelib.parsing import bisenet as A
from codeformer_amd.facelib.parsing import resnet as RN


@pytest.fixture(scope='module')
def nets():
    return {case: R.build(A.BiSeNet, case) for case in R.CASES}


def test_state_dict_is_the_reference_layout(nets):
    g = R.golden()
    net = A.BiSeNet(19)
    sd = net.state_dict()
    assert len(sd) == 191 and sorted(sd) == list(g['keys'])
    assert [','.join(str(n) for n in sd[k].shape) for k in sorted(sd)] == list(g['shapes'])
    assert sum(p.numel() for p in net.parameters()) == 13300416
    state = {k: torch.zeros([int(n) for n in s.split(',')] if s else [], dtype=sd[k].dtype) for k, s in zip(g['keys'], g['shapes'])}
    net.load_state_dict(state, strict=True)
    assert all(float(v.abs().sum()) == 0 for v in net.state_dict().values())


@pytest.mark.parametrize('case', list(R.CASES))
def test_forward_host_against_the_reference(nets, case):
    g = R.golden()
    x = R.case_input(case)
    taps = R.run_taps(nets[case], x)
    assert len(nets[case](x)) == 3 and tuple(taps['out'].shape) == (x.shape[0], 19) + tuple(x.shape[2:])
    for k in R.TAPS:
        e, e_ref = R.rel_err(R.sample(case, k, taps[k]), g[f'{case}_{k}_f64']), R.rel_err(g[f'{case}_{k}_f32'], g[f'{case}_{k}_f64'])
        print(f'\nhost {case} {k}: e {e:.3e}  e(float32 reference) {e_ref:.3e}')
        assert e <= MARGIN * e_ref, (k, e, e_ref)
    assert np.array_equal(nets[case].parse_labels(x).numpy(), taps['out'].argmax(1).numpy())


@pytest.mark.parametrize('case', list(R.CASES))
def test_forward_folded_in_float64(nets, case):
    g = R.golden()
    net = copy.deepcopy(nets[case]).double()
    x = R.case_input(case).double()
    with torch.no_grad():
        got = net.forward_folded(x, return_feat=True) + net.cp.resnet.forward_folded(x)
        assert len(net.forward_folded(x)) == 3
    for k, v in zip(R.TAPS, got):
        assert R.rel_err(R.sample(case, k, v), g[f'{case}_{k}_f64']) <= 1e-12, k


def test_up2x_decomposition_alone():
    rng = np.random.default_rng(1)
    x, w, b = (torch.from_numpy(rng.normal(0., 1., s)) for s in ((2, 4, 3, 5), (6, 4, 3, 3), (6,)))
    want = F.conv2d(F.interpolate(x, scale_factor=2, mode='nearest'), w, b, padding=1)
    assert R.rel_err(A.up2x_conv_folded(x, w, b).numpy(), want.numpy()) <= 1e-14


def test_loaders_and_shims(tmp_path, nets):
    path = str(tmp_path / 'bisenet.pth')
    torch.save(nets['square'].state_dict(), path)
    for net in (P.init_parsing_model('bisenet', model_path=path, device='cpu'), P.load_bisenet(path, device='cpu'), P.init_parsing_model(model_path=path, device='cpu')):
        assert isinstance(net, A.BiSeNet) and not net.training
        assert all(torch.equal(v, nets['square'].state_dict()[k]) for k, v in net.state_dict().items())
    for call in (lambda: P.init_parsing_model('bisenet', device='cpu'), lambda: P.init_parsing_model(device='cpu'), lambda: P.load_bisenet(None)):
        with pytest.raises(NotImplementedError, match='pass `model_path`'):
            call()
    with pytest.raises(FileNotFoundError):
        P.load_bisenet(str(tmp_path / 'absent.pth'))
    with pytest.raises(NotImplementedError):
        P.init_parsing_model('other', device='cpu')
    bad = {k: v for k, v in nets['square'].state_dict().items() if k != 'ffm.conv1.weight'}
    torch.save(bad, path)
    with pytest.raises(RuntimeError):
        P.load_bisenet(path, device='cpu')
    import facelib.parsing
    import facelib.parsing.bisenet
    import facelib.parsing.resnet
    assert facelib.parsing.BiSeNet is facelib.parsing.bisenet.BiSeNet is A.BiSeNet and facelib.parsing.load_bisenet is P.load_bisenet
    assert facelib.parsing.resnet.ResNet18 is RN.ResNet18 and facelib.parsing.resnet.BasicBlock is RN.BasicBlock
    for name in ('ConvBNReLU', 'BiSeNetOutput', 'AttentionRefinementModule', 'ContextPath', 'FeatureFusionModule'):
        assert getattr(facelib.parsing.bisenet, name) is getattr(A, name)
    for name in ('conv3x3', 'create_layer_basic'):
        assert getattr(facelib.parsing.resnet, name) is getattr(RN, name)


def test_what_the_device_path_refuses(nets):
    net = nets['square']
    net.check_device_call((2, 3, 64, 96))
    for shape in ((1, 3, 48, 64), (1, 3, 64, 72), (1, 3, 16, 32), (1, 1, 64, 64), (3, 64, 64)):
        with pytest.raises(ValueError, match='H % 32 == 0'):
            net.check_device_call(shape)
    train = copy.deepcopy(net).train()
    with pytest.raises(RuntimeError, match='eval'):
        train.check_device_call((1, 3, 64, 64))
    assert len(train(R.case_input('square'))) == 3     # (the host path follows torch in either mode)


# ---- the restatements of the kernel definitions against stock torch ------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(2, 3, 14, 18), (1, 3, 9, 7), (1, 3, 2, 2)])
def test_stem_restatement(shape):
    rng = np.random.default_rng(4)
    x, w, b = rng.normal(0., 1., shape), rng.normal(0., 1., (64, 3, 7, 7)), rng.normal(0., 1., 64)
    want = F.relu(F.conv2d(torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(b), stride=2, padding=3)).permute(0, 2, 3, 1).numpy()
    assert R.rel_err(R.stem_ref(x, w, b), want) <= 1e-12


@pytest.mark.parametrize('hw', [(1, 2), (5, 4), (8, 8), (7, 9)])
def test_pool_restatement_is_bitwise(hw):
    x = np.random.default_rng(5).normal(0., 1., (2,) + hw + (4,))
    x[1] = -np.abs(x[1]) - 1
    x[0, 0, 0, 1] = np.nan
    for a in (x, x.astype(np.float32)):
        want = F.max_pool2d(torch.from_numpy(a).permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous().numpy()
        got = R.maxpool3s2_ref(a)
        assert got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8))


@pytest.mark.parametrize('src,dst', [((2, 2), (16, 16)), ((4, 3), (32, 24)), ((1, 1), (8, 8)), ((8, 8), (8, 8)), ((3, 5), (96, 160)), ((16, 16), (128, 128))])
def test_bilinear_restatement(src, dst):
    x = np.random.default_rng(6).normal(0., 4., (2,) + src + (20,))
    nchw = torch.from_numpy(np.ascontiguousarray(x[..., :19].transpose(0, 3, 1, 2)))
    want = F.interpolate(nchw, dst, mode='bilinear', align_corners=True).numpy()
    assert R.rel_err(R.resize_bilinear_ac_ref(x, 19, dst, np.float64), want) <= 1e-12
    # in float32: the corners are copies and the identity is the input, bitwise; torch's own float32 result is a few ulp away at most
    x32 = x.astype(np.float32)
    got = R.resize_bilinear_ac_ref(x32, 19, dst)
    n32 = nchw.float().numpy()
    def lands(n_in, n_out):   # scale * (n_out - 1) rounds to n_in - 1 itself (it does for the kernel test's four shapes, not for 2/95 * 95)
        return n_out == 1 or np.float32(n_in - 1) / np.float32(n_out - 1) * np.float32(n_out - 1) == np.float32(n_in - 1)
    assert lands(src[0], dst[0]) and lands(src[1], dst[1]) or src in ((3, 5), (16, 16))
    for oy, iy in ((0, 0),) + (((dst[0] - 1, src[0] - 1),) if lands(src[0], dst[0]) else ()):
        for ox, ix in ((0, 0),) + (((dst[1] - 1, src[1] - 1),) if lands(src[1], dst[1]) else ()):
            assert np.array_equal(got[:, :, oy, ox].view(np.uint32), n32[:, :, iy, ix].view(np.uint32))
    if src == dst:
        assert np.array_equal(got.view(np.uint32), n32.view(np.uint32))
    assert np.abs(got - F.interpolate(nchw.float(), dst, mode='bilinear', align_corners=True).numpy()).max() <= 8 * 2.0 ** -24 * np.abs(x).max()


def test_fc_and_row_restatements():
    rng = np.random.default_rng(7)
    p, w, b = rng.normal(0., 1., (3, 128)), rng.normal(0., 0.1, (64, 128)), rng.normal(0., 1., 64)
    lin = F.linear(torch.from_numpy(p), torch.from_numpy(w), torch.from_numpy(b))
    for act, fn in ((None, lambda t: t), ('relu', F.relu), ('sigmoid', torch.sigmoid)):
        got, mag = R.pooled_fc_ref(p, w, b, act)
        assert R.rel_err(got, fn(lin).numpy()) <= 1e-12 and (mag >= np.abs(lin.numpy()) - 1e-12).all()
    x, g, r = rng.normal(0., 1., (3, 2, 5, 8)).astype(np.float32), rng.uniform(0., 1., (3, 8)).astype(np.float32), rng.normal(0., 1., (3, 8)).astype(np.float32)
    want = torch.from_numpy(x) * torch.from_numpy(g)[:, None, None] + torch.from_numpy(r)[:, None, None]
    assert np.array_equal(R.scale_add_row_ref(x, g, r).view(np.uint32), want.numpy().view(np.uint32))


# ---- the entry points check every argument before a launch ----------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments():
    from codeformer_amd import build as cf_build
    from codeformer_amd import lib
    cf_build.build()
    n = lib.load()
    assert n.cf_version() == 22
    P_ = 4096      # a 16-byte aligned stand-in: no call below gets as far as a launch

    def refused(status, *words):
        msg = lib.last_error()
        return status == -1 and all(w in msg for w in words)
    assert refused(n.cf_pack_stem7x7(None, P_, None), 'cf_pack_stem7x7', 'null') and refused(n.cf_pack_stem7x7(P_, None, None), 'null')
    for args in ((None, P_, P_, P_), (P_, None, P_, P_), (P_, P_, None, P_), (P_, P_, P_, None)):
        assert refused(n.cf_stem7x7s2(*args[:3], 1, 8, 8, args[3], None), 'cf_stem7x7s2', 'null'), args
    for dims in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (65536, 8, 8)):
        assert refused(n.cf_stem7x7s2(P_, P_, P_, *dims, P_, None), 'bad dims'), dims
    assert refused(n.cf_stem7x7s2(P_, P_, P_, 4096, 1 << 14, 1 << 14, P_, None), 'too large')
    assert refused(n.cf_maxpool3s2(None, 1, 4, 4, 4, P_, None), 'cf_maxpool3s2', 'null') and refused(n.cf_maxpool3s2(P_, 1, 4, 4, 4, None, None), 'null')
    assert refused(n.cf_maxpool3s2(P_, 1, 4, 4, 6, P_, None), 'c % 4') and refused(n.cf_maxpool3s2(P_, 1, 0, 4, 4, P_, None), 'bad dims')
    assert refused(n.cf_maxpool3s2(P_ + 4, 1, 4, 4, 4, P_, None), 'aligned') and refused(n.cf_maxpool3s2(P_, 1 << 20, 1 << 10, 1 << 10, 64, P_, None), 'too large')
    for args in ((None, P_, P_, P_), (P_, None, P_, P_), (P_, P_, None, P_), (P_, P_, P_, None)):
        assert refused(n.cf_pooled_fc(*args[:3], 1, 128, 128, 0, args[3], None), 'cf_pooled_fc', 'null'), args
    for c, m in ((4100, 128), (126, 128), (128, 513), (0, 128), (128, 0)):
        assert refused(n.cf_pooled_fc(P_, P_, P_, 1, c, m, 0, P_, None), 'bad dims'), (c, m)
    assert refused(n.cf_pooled_fc(P_, P_, P_, 1, 128, 128, 3, P_, None), 'act 3') and refused(n.cf_pooled_fc(P_, P_ + 8, P_, 1, 128, 128, 0, P_, None), 'aligned')
    for args in ((None, P_, P_, P_), (P_, None, P_, P_), (P_, P_, None, P_), (P_, P_, P_, None)):
        assert refused(n.cf_scale_add_row(*args[:3], 1, 4, 8, args[3], None), 'cf_scale_add_row', 'null'), args
    assert refused(n.cf_scale_add_row(P_, P_, P_, 1, 4, 6, P_, None), 'c % 4') and refused(n.cf_scale_add_row(P_, P_ + 4, P_, 1, 4, 8, P_, None), 'aligned')
    assert refused(n.cf_scale_add_row(P_, P_, P_, 1 << 20, 1 << 20, 1 << 10, P_, None), 'cf_scale_add_row', 'too large')
    for fn, who in ((n.cf_resize_bilinear_ac, 'cf_resize_bilinear_ac'), (n.cf_resize_bilinear_ac_argmax, 'cf_resize_bilinear_ac_argmax')):
        assert refused(fn(None, 1, 2, 2, 20, 19, P_, 8, 8, None), who, 'null') and refused(fn(P_, 1, 2, 2, 20, 19, None, 8, 8, None), who, 'null')
        assert refused(fn(P_, 1, 2, 2, 18, 18, P_, 8, 8, None), who, 'ld % 4') and refused(fn(P_, 1, 2, 2, 20, 21, P_, 8, 8, None), 'c <= ld')
        assert refused(fn(P_, 1, 2, 0, 20, 19, P_, 8, 8, None), 'bad dims') and refused(fn(P_, 1, 2, 2, 20, 19, P_, 0, 8, None), 'bad dims')
        assert refused(fn(P_, 1 << 10, 2, 2, 20, 19, P_, 1 << 23, 1 << 23, None), who, 'too large')
        assert refused(fn(P_ + 4, 1, 2, 2, 20, 19, P_, 8, 8, None), 'aligned') and refused(fn(P_, 1, 2, 2, 20, 19, P_, 1 << 24, 8, None), '2^24')
    # the Python wrappers refuse what they can before the library is asked
    from codeformer_amd import ops
    with pytest.raises(ValueError):
        ops.pack_stem7x7(torch.zeros(64, 3, 3, 3))
    with pytest.raises(ValueError):
        ops.pooled_fc(torch.zeros(1, 8), torch.zeros(4, 8), torch.zeros(4), act='tanh')
    with pytest.raises(ValueError):
        ops.resize_bilinear_ac(torch.zeros(1, 2, 2, 20), (8, 8), c=21)


# ---- the fixture is what the committed tool writes ------------------------------------------------------------------------------------------
@pytest.mark.skipif(not R.reference_available(), reason='the reference tree is not on this machine')
def test_fixture_is_regenerated_from_the_reference():
    g = R.golden()
    tool = load_script('tools/make_golden_bisenet.py')
    now = tool.record(R.load_reference()[1].BiSeNet)
    for case in R.CASES:
        clear = g[f'{case}_gap'] >= 1e-6      # (another CPU's float64 bits may turn an exact near-tie)
        assert clear.mean() > 0.999 and np.array_equal(now[f'{case}_labels'][clear], g[f'{case}_labels'][clear])
        for k in R.TAPS:
            assert np.array_equal(now[f'{case}_{k}_f64'].shape, g[f'{case}_{k}_f64'].shape)
            assert R.rel_err(now[f'{case}_{k}_f64'], g[f'{case}_{k}_f64']) <= 1e-12
            e_ref = R.rel_err(g[f'{case}_{k}_f32'], g[f'{case}_{k}_f64'])
            assert R.rel_err(now[f'{case}_{k}_f32'], g[f'{case}_{k}_f64']) <= MARGIN * e_ref
