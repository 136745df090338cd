"""ResNetArcFace and the identity metric on the host: registry, state_dict, initialisation, forward_host against the reference's recorded
embeddings, the folded parameters, the identity_input definition, load_arcface, and what the HIP path refuses.  No GPU."""
import numpy as np
import pytest
import torch
from torch.nn import functional as F

import arcface_ref as R
from codeformer_amd import metrics as M
from codeformer_amd.archs import arcface_arch as A


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
        A._need_eval(train.layer1[0])
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
