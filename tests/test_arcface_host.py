"""ResNetArcFace and the identity metric on the host: registry, state_dict, initialisation, forward_host against the reference's recorded
embeddings, the folded parameters, the identity_input definition, load_arcface, and what the HIP path refuses.  No GPU."""
import numpy as np
import pytest
import torch
from torch.nn import functional as F

import arcface_ref as R
from codeformer_amd import metrics as M
from codeformer_amd.archs import arcface_arch as A
from codeformer_amd.archs.folded import need_eval


@pytest.fixture(scope='module')
def nets():
    return {case: R.build(A.ResNetArcFace, case) for case in R.CASES}


def test_registry_and_shim():
    import basicsr.archs.arcface_arch as shim
    from basicsr.utils.registry import ARCH_REGISTRY, METRIC_REGISTRY
    import basicsr.metrics as bm
    assert ARCH_REGISTRY.get('ResNetArcFace') is A.ResNetArcFace
    for name in ('ResNetArcFace', 'IRBlock', 'SEBlock', 'BasicBlock', 'Bottleneck', 'conv3x3'):
        assert getattr(shim, name) is getattr(A, name)
    assert METRIC_REGISTRY.get('calculate_identity') is M.calculate_identity
    for name in ('calculate_identity', 'identity_batch', 'identity_input', 'load_arcface', 'calculate_psnr', 'calculate_ssim'):
        assert getattr(bm, name) is getattr(M, name)


@pytest.mark.parametrize('case', list(R.CASES))
def test_state_dict_keys_and_shapes(nets, case):
    g = R.golden()
    sd = nets[case].state_dict()
    assert sorted(sd) == list(g[f'keys_{case}'])
    assert [','.join(str(n) for n in sd[k].shape) for k in sorted(sd)] == list(g[f'shapes_{case}'])


def test_default_init():
    """The reference's initialisation: BatchNorm 1 / 0, Linear bias 0, xavier-normal conv and Linear weights (std sqrt(2 / (fan_in + fan_out)));
    under torch.manual_seed(0) the same draws in the same order as the reference's class."""
    torch.manual_seed(0)
    net = A.ResNetArcFace('IRBlock', [2, 2, 2, 2], use_se=False)
    g = R.golden()
    digest = R.init_digest(net)
    if R.host_id() == str(g['torch_version']):
        assert np.array_equal(digest, g['init_r18'])
    for name, m in net.named_modules():
        if isinstance(m, (torch.nn.BatchNorm2d, torch.nn.BatchNorm1d)):
            assert torch.all(m.weight == 1) and torch.all(m.bias == 0), name
        elif isinstance(m, (torch.nn.Conv2d, torch.nn.Linear)):
            w = m.weight.detach().double()
            rf = w[0][0].numel() if w.dim() == 4 else 1
            std = (2.0 / ((w.shape[0] + w.shape[1]) * rf))**0.5
            assert abs(float(w.std()) / std - 1) <= 4.0 / (2 * w.numel())**0.5, name   # four sigma of a sample standard deviation
            assert abs(float(w.mean())) <= 4.0 * std / w.numel()**0.5, name
            if isinstance(m, torch.nn.Linear):
                assert torch.all(m.bias == 0), name
        elif isinstance(m, torch.nn.PReLU):
            assert float(m.weight.detach()) == 0.25, name


@pytest.mark.parametrize('case', list(R.CASES))
def test_forward_host_against_reference(nets, case):
    """The same ops on the same torch: bitwise under the fixture's torch version; under another one within the reference's own
    float32-against-float64 distance of its float32 embeddings.

    Known to FAIL on a CPU model other than the recording one under the same torch (AMD EPYC 9575F: |host - reference float32| 2.04e-6 /
    1.43e-6 against 1.20e-6 / 0.88e-6; torch picks its CPU kernels by CPU model): profiles/NOTES.md, "forward_host on another CPU"."""
    g = R.golden()
    with torch.no_grad():
        y = nets[case](R.case_input(case)).numpy()
    assert y.shape == (R.CASES[case]['batch'], 512) and y.dtype == np.float32
    e_host, e_ref = R.rel_err(y, g[f'{case}_f32']), R.rel_err(g[f'{case}_f32'], g[f'{case}_f64'])
    print(f'\ntorch {R.host_id()!r}, fixture {str(g["torch_version"])!r}: |host - reference float32| {e_host:.3e}, |reference float32 - float64| {e_ref:.3e}')
    if R.host_id() == str(g['torch_version']):
        assert np.array_equal(y, g[f'{case}_f32'])
    else:
        assert e_host <= e_ref


@pytest.mark.parametrize('case', list(R.CASES))
def test_folded_parameters_float64(nets, case):
    """BN into conv, bn0 as an input affine, bn4 / bn5 and the column permutation into fc5: in float64 the folded dataflow is the module."""
    import copy
    net = copy.deepcopy(nets[case]).double()
    x = R.case_input(case).double()
    with torch.no_grad():
        ref, got = net(x), net.forward_folded(x)
    assert R.rel_err(ref.numpy(), R.golden()[f'{case}_f64']) <= 1e-12
    assert R.rel_err(got.numpy(), ref.numpy()) <= 1e-12


def test_bn0_shift_is_not_folded_into_the_bias():
    """The border: folding bn0's shift into conv1's bias is exact inside and wrong by O(1) on the border, and forward_folded does not do it."""
    blk = R.fill_state(A.IRBlock(64, 64, use_se=False), 5).eval().double()
    x = torch.from_numpy(np.random.default_rng(6).normal(0., 1., (1, 64, 6, 6)))
    with torch.no_grad():
        ref, got = blk(x), blk.forward_folded(x)
        s, t = A.bn_affine(blk.bn0)
        w, b = A.fold_conv_bn(blk.conv1, blk.bn1)
        wrong = F.conv2d(x * s.view(1, -1, 1, 1), w, b + (w * t.view(1, -1, 1, 1)).sum(dim=(1, 2, 3)), padding=1)
        right = F.conv2d(x * s.view(1, -1, 1, 1) + t.view(1, -1, 1, 1), w, b, padding=1)
    assert R.rel_err(got.numpy(), ref.numpy()) <= 1e-12
    assert float((wrong - right)[:, :, 1:-1, 1:-1].abs().max()) <= 1e-9 * float(right.abs().max())
    assert float((wrong - right)[:, :, 0].abs().max()) >= 0.5   # O(1): the shifts of a bn0 have magnitude 2


def test_train_mode_on_host_follows_torch(nets):
    import copy
    net = copy.deepcopy(nets['se']).train()
    x = R.case_input('se')
    torch.manual_seed(3)
    y = net(x)
    assert y.requires_grad and y.shape == (2, 512)
    assert int(net.bn5.num_batches_tracked) == 1   # batch statistics were used and tracked


# ---- identity_input ----------------------------------------------------------------------------------------------------------------
ID_CASES = {   # name: (shape, dtype, order)
    'same': ((2, 128, 128, 3), 'uint8', 'HWC'),
    'x4': ((1, 512, 512, 3), 'uint8', 'HWC'),
    'chw': ((2, 3, 200, 136), 'float32', 'CHW'),
    'up': ((1, 64, 64, 3), 'float32', 'HWC'),
}


def id_image(name):
    shape, dtype, _ = ID_CASES[name]
    rng = np.random.default_rng(sorted(ID_CASES).index(name) + 40)
    return torch.from_numpy(rng.integers(0, 256, shape).astype(np.uint8) if dtype == 'uint8' else rng.random(shape).astype(np.float32))


@pytest.mark.parametrize('name', list(ID_CASES))
def test_identity_input_host_definition(name):
    """Against F.interpolate(bilinear, align_corners=False) of the gray image: a four-tap convex combination, so 2 ulp of the largest
    operand; bitwise the gray image at 128 x 128."""
    img, order = id_image(name), ID_CASES[name][2]
    out = M.identity_input(img, order)
    view = img.permute(0, 2, 3, 1) if order == 'CHW' else img
    gray = M.identity_gray_host(view)
    assert out.shape == (img.shape[0], 1, 128, 128) and out.dtype == torch.float32
    ref = F.interpolate(gray[:, None], size=(128, 128), mode='bilinear', align_corners=False)
    ulp = float(np.spacing(np.float32(gray.abs().max())))
    assert float((out - ref).abs().max()) <= 2 * ulp
    if name == 'same':
        assert torch.equal(out[:, 0], gray)
    # gray itself: RGB in [-1, 1], BGR order for uint8
    v = view.double() / 255. * 2 - 1 if img.dtype == torch.uint8 else view.double() * 2 - 1
    r, g_, b = (v[..., 2], v[..., 1], v[..., 0]) if img.dtype == torch.uint8 else (v[..., 0], v[..., 1], v[..., 2])
    assert float((gray.double() - (0.2989 * r + 0.5870 * g_ + 0.1140 * b)).abs().max()) <= 4 * 2.0**-24


def test_identity_input_forms():
    img = id_image('same')
    assert torch.equal(M.identity_input(img[0]), M.identity_input(img)[:1])              # one image
    assert torch.equal(M.identity_input(img.numpy()), M.identity_input(img))             # numpy
    f = img.float() / 255
    assert torch.equal(M.identity_input(f.permute(0, 3, 1, 2).contiguous(), 'CHW'), M.identity_input(f))
    with pytest.raises(TypeError):
        M.identity_input(img.double())
    with pytest.raises(ValueError):
        M.identity_input(img[..., :2])


def test_identity_host_path(nets):
    net = nets['r18']
    a, b = id_image('x4')[0], id_image('up')[0]
    v = M.calculate_identity(a, a, net)
    assert isinstance(v, float) and abs(v - 1) <= 1e-6
    f = (b * 255).round().to(torch.uint8).flip(-1)    # the float RGB image as uint8 BGR
    assert abs(M.calculate_identity(a.numpy(), f.numpy(), net) - M.calculate_identity(f, a, net)) <= 1e-12
    out = M.identity_batch(torch.stack([a, a]), torch.stack([a, a]), net)
    assert out.dtype == torch.float64 and out.shape == (2,)
    assert float(M._cosine_host(torch.zeros(1, 8), torch.ones(1, 8))) == 0.0
    with pytest.raises(ValueError):
        M.calculate_identity(torch.stack([a, a]), torch.stack([a, a]), net)


def test_load_arcface(tmp_path):
    torch.manual_seed(1)
    src = R.fill_state(A.ResNetArcFace('IRBlock', [2, 2, 2, 2], use_se=False), 9)
    path = str(tmp_path / 'arcface.pth')
    torch.save({'params_ema': {'module.' + k: v for k, v in src.state_dict().items()}}, path)
    net = M.load_arcface(path)
    assert not net.training and isinstance(net, A.ResNetArcFace)
    for k, v in src.state_dict().items():
        assert torch.equal(net.state_dict()[k], v), k
    torch.save(src.state_dict(), path)
    assert torch.equal(M.load_arcface(path).fc5.weight, src.fc5.weight)
    with pytest.raises(FileNotFoundError):
        M.load_arcface(str(tmp_path / 'missing.pth'))
    assert not M.load_arcface().training


def test_what_the_hip_path_refuses(nets):
    import copy
    net = nets['se']
    net.check_device_call((3, 1, 128, 128))
    for shape in ((3, 1, 112, 112), (3, 3, 128, 128), (1, 128, 128), (3, 1, 128, 64)):
        with pytest.raises(ValueError):
            net.check_device_call(shape)
    train = copy.deepcopy(net).train()
    with pytest.raises(RuntimeError):
        train.check_device_call((3, 1, 128, 128))
    with pytest.raises(RuntimeError):
        need_eval(train.layer1[0])
    with pytest.raises(TypeError):
        A.ResNetArcFace(A.BasicBlock, [1, 1, 1, 1])   # as in the reference: _make_layer passes use_se to every block


def test_script_identity_column(tmp_path, capsys):
    """scripts/calculate_metrics.py --identity: the column, the mean, the JSON, and the refusal without a weight source."""
    import importlib.util
    import json
    import os
    from codeformer_amd.utils.img_util import imwrite
    spec = importlib.util.spec_from_file_location('calculate_metrics_script', os.path.join(R.ROOT, 'scripts', 'calculate_metrics.py'))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    rng = np.random.default_rng(3)
    imgs = rng.integers(0, 256, (2, 2, 48, 40, 3)).astype(np.uint8)
    for i in range(2):
        imwrite(imgs[0, i], str(tmp_path / 'restored' / f'{i}.png'))
        imwrite(imgs[1, i], str(tmp_path / 'gt' / f'{i}.png'))
    dirs = ['--restored', str(tmp_path / 'restored'), '--gt', str(tmp_path / 'gt')]
    with pytest.raises(SystemExit):
        script.main(dirs + ['--identity'])
    out = tmp_path / 'out.json'
    assert script.main(dirs + ['--identity', '--random_init_seed', '4', '--json', str(out)]) == 0
    text = capsys.readouterr().out
    assert text.count('IDENTITY') == 3
    rec = json.loads(out.read_text())
    torch.manual_seed(4)
    net = M.load_arcface(device='cuda' if torch.cuda.is_available() else None)
    for i in range(2):
        a, b = (torch.from_numpy(imgs[k, i]).to(next(net.parameters()).device) for k in (0, 1))
        assert abs(rec['files'][f'{i}.png']['identity'] - M.calculate_identity(a, b, net)) <= 1e-12
    assert abs(rec['mean']['identity'] - np.mean([rec['files'][f'{i}.png']['identity'] for i in range(2)])) <= 1e-15


# ---- the per-element bounds of tools/arcface_check.py: every one a statement about the float64 reference ------------------------------------
@pytest.fixture(scope='module')
def ac():
    from _tools import load_script
    return load_script('tools/arcface_check.py')


def _ratio(got, ref, bound):
    return float((np.abs(got.astype(np.float64) - ref) / (bound + 1e-300)).max())


def test_fc_rows_emulation_within_half_of_the_bound_and_int_coded_exact(ac):
    assert ac.FC_SHAPES == ((1, 4, 256), (16, 68, 2304), (17, 128, 1024)) and ac.FC_FIN == 8 and ac.fc_coef(2304) == 64 + 3 + 2 + 7
    for shape in ac.FC_SHAPES:
        for fam in ac.FC_FAMILIES:
            x, w, b = ac.fc_family(fam, shape)
            ref, emu = ac.fc_ref(x, w, b), ac.fc_emulate(x, w, b)
            r = _ratio(emu, ref, ac.fc_bound(x, w, b))
            print(f'fc_rows {fam} {shape}: emulation {r:.4f} of the bound')
            assert r <= 0.5, (fam, shape, r)
            if fam == 'int_coded':      # whole units of 2^-5, every partial sum below 2^24 of them: float32 is exact
                S = (np.abs(x.astype(np.float64)) @ np.abs(w.astype(np.float64)).T + np.abs(b)) * 32
                assert float(S.max()) < 2 ** 24 and np.array_equal(ref * 32, np.round(ref * 32)) and np.array_equal(emu.astype(np.float64), ref)
            if fam == 'cancel_pairs':   # ill-conditioned: the sum is far below its terms
                S = np.abs(x.astype(np.float64)) @ np.abs(w.astype(np.float64)).T
                assert float(np.median(S / np.abs(ref))) >= 100
            if fam == 'row_scales' and shape[0] > 1:
                assert b is None and float(np.abs(x[-1]).max() / np.abs(x[0]).max()) > 2.0 ** 36
        ks = ac.fc_onehot_ks(shape[2])
        assert {0, 63, 64, 127, 128, 191, 192, 255, shape[2] - 1} <= set(ks) and (shape[2] == 256 or {256, shape[2] - 256, shape[2] - 257} <= set(ks))
        x, w, b = ac.fc_family('normal', shape)
        hot = np.zeros((len(ks), shape[2]), np.float32)
        hot[np.arange(len(ks)), ks] = 1.0
        assert np.array_equal(ac.fc_emulate(hot, w, b), (w[:, ks].T + b[None]).astype(np.float32))


@pytest.mark.parametrize('slope', R.SLOPES)
def test_se_gate_emulation_within_half_of_the_bound(ac, slope):
    assert ac.SE_GATE_SHAPES == ((2, 68, 3), (1, 320, 20), (1, 4096, 256), (2, 128, 8)) and ac.SLOPES == R.SLOPES
    for shape in ac.SE_GATE_SHAPES:
        args = ac.gate_inputs(shape, slope)
        p, w1, b1, w2, b2 = args
        ref = ac.gate_ref(p, w1, b1, slope, w2, b2)
        emu, s32 = ac.gate_emulate(p, w1, b1, slope, w2, b2)
        fig = ac.sigmoid_figure(s32)
        r = _ratio(emu, ref['out'], ac.gate_bound(p, w1, b1, slope, w2, b2, ref, fig))
        print(f'se_gate {shape} slope {slope}: emulation {r:.4f} of the bound; sigmoid figure {fig:.3f} u')
        assert r <= 0.5 and fig <= 4.0, (shape, slope, r, fig)
        assert float(ref['s'].max()) > 35 and float(ref['s'].min()) < -35 and np.all(np.isfinite(emu)) and emu.min() >= 0 and emu.max() <= 1


def test_se_pool_emulation_within_half_of_the_bound_and_int_coded_exact(ac):
    assert ac.SE_POOL_SHAPES == ((1, 1, 1, 4), (1, 16, 16, 68), (2, 17, 19, 132))
    for shape in ac.SE_POOL_SHAPES:
        hw = shape[1] * shape[2]
        for fam in ac.SE_POOL_FAMILIES:
            x = ac.pool_family(fam, shape)
            ref, emu = ac.pool_ref(x), ac.pool_emulate(x)
            r = _ratio(emu, ref, ac.pool_bound(x))
            print(f'se_pool {fam} {shape}: emulation {r:.4f} of the bound')
            assert r <= 0.5, (fam, shape, r)
            if fam == 'int_coded' and hw & (hw - 1) == 0:
                assert np.array_equal(emu.astype(np.float64), ref) and float(np.abs(x).max()) * hw < 2 ** 24
            if fam == 'cancel' and hw > 1:      # the mean is the ripple: far below |x|
                assert float(np.abs(ref).max()) < 1e-3 and float(np.abs(x).mean()) > 0.5
            if fam == 'mixed' and shape[3] > 4:
                assert float(np.abs(ref[:, -1]).max() / np.abs(ref[:, 0]).max()) > 2.0 ** 30


def test_cosine_rows_emulation_within_half_of_the_bound(ac):
    for n in (1, 63, 65):
        for rows in (1, 4, 5):
            for norm in (1.0, 1e-20, 1e18):
                x, y = ac.cosine_rows_family(rows, n, norm)
                ref = ac.cosine_ref(x, y)
                r = _ratio(ac.cosine_emulate(x, y), ref, ac.cosine_bound(x, y))
                assert r <= 0.5, (n, rows, norm, r)
                if norm == 1e-20:   # the floor decides
                    assert np.allclose(ref, (x.astype(np.float64) * y).sum(1) / 1e-8, rtol=1e-15) and float(np.abs(ref).max()) < 1e-30


@pytest.mark.parametrize('shape', [(1, 1, 1, 3), (1, 2, 3, 3), (1, 127, 129, 3), (1, 300, 5, 3)])
@pytest.mark.parametrize('dtype', ['uint8', 'float32'])
def test_identity_input_host_definition_per_image_bound(ac, shape, dtype):
    """The host definition against the float64 bilinear resize of the gray image under arcface_check.identity_bound."""
    rng = np.random.default_rng(sum(shape))
    img = torch.from_numpy(rng.integers(0, 256, shape).astype(np.uint8) if dtype == 'uint8' else rng.random(shape).astype(np.float32))
    out = M.identity_input(img)
    gray = M.identity_gray_host(img).double()
    ref = F.interpolate(gray[:, None], size=(128, 128), mode='bilinear', align_corners=False)
    bound = ac.identity_bound(gray.numpy())
    err = float((out.double() - ref).abs().max())
    print(f'identity_input {shape} {dtype}: |host - float64 resize| {err:.3e}, bound {float(bound[0]):.3e}')
    assert err <= float(bound[0]) and ac.identity_weights_exact(shape[1]) and ac.identity_weights_exact(shape[2]) and ac.identity_weights_exact(32767)
    if shape[1:3] == (1, 1):
        assert torch.equal(out, M.identity_gray_host(img)[:, None].expand(1, 1, 128, 128))


@pytest.mark.parametrize('cin,cout,H,W,B', [(32, 32, 9, 5, 1), (64, 64, 8, 8, 2), (128, 128, 25, 41, 1)])
@pytest.mark.parametrize('slope', (-0.5, 1.5))
def test_block_emulation_within_half_of_the_composed_bound(ac, cin, cout, H, W, B, slope):
    """arcface_check.block_ref: the float32 CPU evaluation of the folded dataflow against the float64 one on the same float32-rounded parameters;
    in float64 that dataflow is the module up to the fold's rounding."""
    blk = R.fill_state(A.IRBlock(cin, cout, use_se=False), 400 + cin + H, slope=slope).eval()
    x = torch.from_numpy(np.random.default_rng(cin + W).normal(0., 1., (B, cin, H, W)).astype(np.float32))
    with torch.no_grad():
        ref, bound = ac.block_ref(blk, x)
        r = float(((ac.block_emulate(blk, x).double() - ref).abs() / bound).max())
        mod = blk.double()(x.double())
    print(f'IRBlock({cin}, {cout}) {H}x{W} slope {slope}: emulation {r:.4f} of the bound')
    assert r <= 0.5 and bool((bound > 0).all())
    assert float((mod - ref).abs().max()) <= 1e-4 * float(ref.abs().max())      # (float32-rounded folded weights against the module in float64)
