"""VGGFeatureExtractor, PerceptualLoss and the perceptual metric on the host: registry and shims, names, state_dict, initialisation, weight
loading without a download, forward_host and the host loss against the reference's recorded float64 values, and what the HIP path refuses
before it touches a device.  No GPU.

The yardstick: with e(x) = max|x - ref64| / max|ref64|, e(host) <= 8 e(float32 reference) on the recorded sample positions.  (Not bitwise:
float32 bits of the same torch differ between CPU models, profiles/NOTES.md.)  A PerceptualLoss output is ONE float32 number, and the error
of one correctly rounded float32 number is anything up to 2^-24 by luck alone: for those, e(float32 reference) counts as at least 2^-24.
"""
import os

import numpy as np
import pytest
import torch

import vgg_ref as R
from codeformer_amd import losses as LS
from codeformer_amd import metrics as M
from codeformer_amd.archs import vgg_arch as A

MARGIN = 8.0
HALF_ULP = 2.0 ** -24


def yardstick(what, got, f32, f64, floor=0.0):
    e_got, e_ref = R.rel_err(got, f64), max(R.rel_err(f32, f64), floor)
    print(f'\n{what}: e {e_got:.3e}  e(float32 reference) {e_ref:.3e}  ratio {e_got / e_ref if e_ref else float("inf"):.3f}')
    assert e_got <= MARGIN * e_ref, (what, e_got, e_ref)


@pytest.fixture(scope='module')
def nets():
    return {case: R.build(A.VGGFeatureExtractor, case) for case in R.CASES}


def test_registry_and_shims():
    import basicsr.archs.vgg_arch as shim
    import basicsr.losses as bl
    import basicsr.losses.losses as bll
    import basicsr.metrics as bm
    from basicsr.utils.registry import ARCH_REGISTRY, LOSS_REGISTRY, METRIC_REGISTRY
    assert ARCH_REGISTRY.get('VGGFeatureExtractor') is A.VGGFeatureExtractor
    assert LOSS_REGISTRY.get('PerceptualLoss') is LS.PerceptualLoss
    assert METRIC_REGISTRY.get('calculate_perceptual') is M.calculate_perceptual
    for name in ('VGG_PRETRAIN_PATH', 'NAMES', 'insert_bn', 'VGGFeatureExtractor'):
        assert getattr(shim, name) is getattr(A, name)
    assert bl.PerceptualLoss is LS.PerceptualLoss and bll.PerceptualLoss is LS.PerceptualLoss
    for name in ('calculate_perceptual', 'perceptual_batch', 'load_vgg'):
        assert getattr(bm, name) is getattr(M, name)


def test_names_agree_with_the_reference():
    g = R.golden()
    assert A.VGG_PRETRAIN_PATH == str(g['pretrain_path'])
    assert sorted(A.NAMES) == ['vgg11', 'vgg13', 'vgg16', 'vgg19']
    for t, names in A.NAMES.items():
        assert names == list(g[f'names_{t}'])
        assert A.insert_bn(names) == list(g[f'names_{t}_bn'])


@pytest.mark.parametrize('case', list(R.CASES))
def test_state_dict_and_forward_keys_and_shapes(nets, case):
    g = R.golden()
    sd = nets[case].state_dict()
    assert sorted(sd) == list(g[f'keys_{case}'])
    assert [','.join(str(n) for n in sd[k].shape) for k in sorted(sd)] == list(g[f'shapes_{case}'])
    with torch.no_grad():
        out = nets[case](R.case_input(case))
    assert list(out) == list(g[f'out_keys_{case}'])
    assert [','.join(str(n) for n in v.shape) for v in out.values()] == list(g[f'out_shapes_{case}'])
    assert all(v.dtype == torch.float32 for v in out.values())


def test_constructor_arguments_in_the_reference_order():
    import inspect
    assert list(inspect.signature(A.VGGFeatureExtractor.__init__).parameters)[1:] == [
        'layer_name_list', 'vgg_type', 'use_input_norm', 'range_norm', 'requires_grad', 'remove_pooling', 'pooling_stride']
    assert list(inspect.signature(LS.PerceptualLoss.__init__).parameters)[1:] == [
        'layer_weights', 'vgg_type', 'use_input_norm', 'range_norm', 'perceptual_weight', 'style_weight', 'criterion']
    net = A.VGGFeatureExtractor(['relu1_1'], 'vgg11', False, True, True, True, 3)
    assert not hasattr(net, 'mean') and net.range_norm and net.vgg_net.training and all(p.requires_grad for p in net.parameters())
    assert list(net.vgg_net._modules) == ['conv1_1', 'relu1_1']
    net = A.VGGFeatureExtractor(['pool1'], 'vgg11', pooling_stride=3)
    assert net.vgg_net.pool1.stride == 3 and not net.vgg_net.training and not any(p.requires_grad for p in net.parameters())


def test_default_init_draws_the_generator_as_the_full_stack_does():
    """torchvision initialises the WHOLE model before the extractor truncates it: kaiming_normal_(fan_out, relu), zero bias, BatchNorm 1 / 0,
    in module order.  The truncated extractor holds the first layers of exactly those draws."""
    torch.manual_seed(5)
    net = A.VGGFeatureExtractor(['relu2_2'], 'vgg16_bn')
    torch.manual_seed(5)
    full = A.FeaturesOnly('vgg16_bn')
    mine = [m for m in net.vgg_net if list(m.state_dict())]
    theirs = [m for m in full.features if list(m.state_dict())][:len(mine)]
    assert len(mine) == 8
    for a, b in zip(mine, theirs):
        for k, v in a.state_dict().items():
            assert torch.equal(v, b.state_dict()[k]), k
    conv = net.vgg_net.conv2_1
    assert float(conv.bias.abs().max()) == 0.0
    assert abs(float(conv.weight.std()) / np.sqrt(2.0 / (128 * 9)) - 1.0) < 0.02
    assert torch.equal(net.vgg_net.bn2_1.weight, torch.ones(128)) and torch.equal(net.vgg_net.bn2_1.bias, torch.zeros(128))


@pytest.mark.parametrize('case', list(R.CASES))
def test_forward_host_against_the_recorded_reference(nets, case):
    g = R.golden()
    with torch.no_grad():
        out = nets[case](R.case_input(case))
    for k, v in out.items():
        yardstick(f'{case} {k} forward_host', R.sample(case, k, v), g[f'{case}_{k}_f32'], g[f'{case}_{k}_f64'])


@pytest.mark.parametrize('criterion', R.CRITERIA)
@pytest.mark.parametrize('case', R.LOSS_CASES)
def test_host_loss_against_the_recorded_reference(case, criterion):
    g = R.golden()
    x, gt = R.case_input(case), R.case_input(case, 1)
    with torch.no_grad():
        percep, style = R.build_loss(LS.PerceptualLoss, case, criterion)(x, gt)
    assert percep.dim() == 0 and style.dim() == 0 and percep.dtype == torch.float32 and style.dtype == torch.float32
    f32, f64 = g[f'loss_{case}_{criterion}_f32'], g[f'loss_{case}_{criterion}_f64']
    yardstick(f'{case} {criterion} percep', float(percep), f32[0], f64[0], HALF_ULP)
    yardstick(f'{case} {criterion} style', float(style), f32[1], f64[1], HALF_ULP)


def test_loss_terms_switch_off_and_l2_is_refused():
    x, gt = R.case_input('nopool'), R.case_input('nopool', 1)
    with torch.no_grad():
        percep, style = LS.PerceptualLoss({'relu1_1': 1.}, vgg_type='vgg11')(x, gt)
        assert style is None and percep.dim() == 0
        percep, style = LS.PerceptualLoss({'relu1_1': 1.}, vgg_type='vgg11', perceptual_weight=0, style_weight=2.)(x, gt)
        assert percep is None and style.dim() == 0
    with pytest.raises(NotImplementedError):
        LS.PerceptualLoss({'relu1_1': 1.}, criterion='l2')
    with pytest.raises(NotImplementedError):
        LS.PerceptualLoss({'relu1_1': 1.}, criterion='huber')


def _torchvision_state(vgg_type, seed):
    torch.manual_seed(seed)
    full = A.FeaturesOnly(vgg_type)
    R.fill_state(full, seed)
    sd = dict(full.state_dict())
    sd['classifier.0.weight'] = torch.zeros(4, 4)
    sd['classifier.0.bias'] = torch.zeros(4)
    return full, sd


def test_a_torchvision_state_dict_loads_by_position(tmp_path, monkeypatch):
    full, sd = _torchvision_state('vgg19', 3)
    path = str(tmp_path / 'vgg19.pth')
    torch.save(sd, path)
    monkeypatch.setattr(A, 'VGG_PRETRAIN_PATH', path)
    net = A.VGGFeatureExtractor(['conv2_2', 'relu3_1'])
    assert list(net.vgg_net._modules)[-1] == 'relu3_1'
    for name, idx in (('conv1_1', 0), ('conv2_2', 7), ('conv3_1', 10)):
        assert torch.equal(net.vgg_net._modules[name].weight, sd[f'features.{idx}.weight'])
        assert torch.equal(net.vgg_net._modules[name].bias, sd[f'features.{idx}.bias'])
    monkeypatch.undo()
    loss = M.load_vgg(path, layer_weights={'conv3_4': 1.})
    assert torch.equal(loss.vgg.vgg_net.conv3_4.weight, sd['features.16.weight']) and not loss.training
    with pytest.raises(FileNotFoundError):
        M.load_vgg(str(tmp_path / 'absent.pth'))


def test_no_download_is_attempted_when_the_file_is_absent(monkeypatch):
    import codeformer_amd.utils.download_util as D

    def refuse(*a, **k):
        raise AssertionError('a download was attempted')
    monkeypatch.setattr(D, 'load_file_from_url', refuse)
    monkeypatch.setattr(torch.hub, 'load_state_dict_from_url', refuse)
    monkeypatch.setattr(torch.hub, 'download_url_to_file', refuse)
    assert not os.path.exists(A.VGG_PRETRAIN_PATH)
    import logging
    records = []
    handler = logging.Handler(level=logging.WARNING)     # (a handler of its own: get_root_logger may have switched propagation off)
    handler.emit = records.append
    logger = logging.getLogger('basicsr')
    logger.addHandler(handler)
    try:
        A.VGGFeatureExtractor(['relu1_1'], 'vgg11')
    finally:
        logger.removeHandler(handler)
    assert sum('nothing is downloaded' in r.getMessage() for r in records) == 1
    M.load_vgg(vgg_type='vgg11', layer_weights={'relu1_1': 1.})


class _FakeCuda:
    """What the entry points read of an input before their first device call: a tensor on a GPU, as far as they can tell."""
    is_cuda, requires_grad, dtype, device = True, False, torch.float32, 'cuda:0'

    def __init__(self, *shape, requires_grad=False):
        self.shape, self.requires_grad = torch.Size(shape), requires_grad

    def dim(self):
        return len(self.shape)


class _Reached(Exception):
    pass


def test_the_hip_path_refuses_before_any_device_call(nets, monkeypatch):
    """forward, features_nhwc and PerceptualLoss.forward on a CUDA tensor raise their refusals BEFORE the library is loaded, a device is
    initialised or anything is packed or launched: every such entry is replaced by one that raises _Reached, and a call that passes the checks
    is shown to get there."""
    from codeformer_amd import ops

    def reached(*a, **k):
        raise _Reached('a device call was reached')
    for name in ('vgg_input', 'conv2d', 'relu', 'relu_maxpool2', 'pack_weight', 'gram', 'feat_dist', 'to_nchw'):
        monkeypatch.setattr(ops, name, reached)
    for name in ('ensure_device', 'load'):
        monkeypatch.setattr(ops.L, name, reached)
    net = nets['grid']
    for entry in (net, net.forward, net.features_nhwc):
        with pytest.raises(_Reached):
            entry(_FakeCuda(2, 3, 64, 64))        # (passes the checks: the next thing is the device)
        for shape in ((2, 1, 64, 64), (3, 64, 64), (2, 3, 64, 8), (0, 3, 64, 64)):
            with pytest.raises(ValueError):
                entry(_FakeCuda(*shape))
    with pytest.raises(RuntimeError):
        A.VGGFeatureExtractor(['relu1_1'], 'vgg11', requires_grad=True)(_FakeCuda(1, 3, 8, 8))
    with pytest.raises(NotImplementedError):
        A.VGGFeatureExtractor(['relu2_1'], 'vgg11', pooling_stride=1)(_FakeCuda(1, 3, 8, 8))
    loss = LS.PerceptualLoss({'relu2_1': 1.}, vgg_type='vgg11', style_weight=1.)
    with pytest.raises(_Reached):
        loss(_FakeCuda(1, 3, 8, 8), _FakeCuda(1, 3, 8, 8))
    with pytest.raises(RuntimeError):
        loss(_FakeCuda(1, 3, 8, 8, requires_grad=True), _FakeCuda(1, 3, 8, 8))
    with torch.no_grad(), pytest.raises(_Reached):
        loss(_FakeCuda(1, 3, 8, 8, requires_grad=True), _FakeCuda(1, 3, 8, 8))
    for x, gt in ((_FakeCuda(1, 3, 8, 8), _FakeCuda(1, 3, 8, 6)), (_FakeCuda(1, 1, 8, 8), _FakeCuda(1, 1, 8, 8)), (_FakeCuda(1, 3, 1, 8), _FakeCuda(1, 3, 1, 8))):
        with pytest.raises(ValueError):
            loss(x, gt)
    loss.vgg.vgg_net.train()
    with pytest.raises(RuntimeError):
        loss(_FakeCuda(1, 3, 8, 8), _FakeCuda(1, 3, 8, 8))
    # check_device_call alone
    net.check_device_call((2, 3, 64, 64))
    for shape in ((2, 1, 64, 64), (3, 64, 64), (2, 3, 64, 8), (0, 3, 64, 64)):     # (64x8: pool4 would take 8x1 to zero)
        with pytest.raises(ValueError):
            net.check_device_call(shape)
    with pytest.raises(RuntimeError):
        A.VGGFeatureExtractor(['relu1_1'], 'vgg11', requires_grad=True).check_device_call((1, 3, 8, 8))
    train = A.VGGFeatureExtractor(['relu1_1'], 'vgg11_bn')
    train.vgg_net.train()
    with pytest.raises(RuntimeError):
        train.check_device_call((1, 3, 8, 8))
    with pytest.raises(NotImplementedError):
        A.VGGFeatureExtractor(['relu2_1'], 'vgg11', pooling_stride=1).check_device_call((1, 3, 8, 8))
    A.VGGFeatureExtractor(['relu2_1'], 'vgg11', remove_pooling=True, pooling_stride=1).check_device_call((1, 3, 1, 1))


def test_perceptual_batch_on_the_host():
    """uint8 BGR HWC and the equivalent float32 RGB CHW tensor give the same numbers; a == b gives exactly 0; rows are the one-image calls."""
    torch.manual_seed(1)
    net = M.load_vgg(vgg_type='vgg11', layer_weights={'relu1_1': 0.5, 'relu2_1': 1.})
    rng = np.random.default_rng(9)
    a, b = (rng.integers(0, 256, (2, 12, 10, 3), dtype=np.uint8) for _ in range(2))
    fa, fb = (torch.from_numpy(t[..., ::-1].copy()).float().div(torch.tensor(255.)).permute(0, 3, 1, 2) for t in (a, b))
    for style in (False, True):
        for crit in R.CRITERIA:
            s = M.perceptual_batch(a, b, net, criterion=crit, style=style)
            assert s.dtype == torch.float64 and tuple(s.shape) == (2,) and bool((s > 0).all())
            assert torch.equal(s, M.perceptual_batch(fa, fb, net, order='CHW', criterion=crit, style=style))
            assert torch.equal(M.perceptual_batch(a, a, net, criterion=crit, style=style), torch.zeros(2, dtype=torch.float64))
    s = M.perceptual_batch(a, b, net)
    for r in range(2):
        assert abs(M.calculate_perceptual(a[r], b[r], net) - float(s[r])) <= 1e-6 * float(s[r])
    # per image, 'l1' is the reference's loss on a batch of one
    with torch.no_grad():
        ref = net.forward_host(fa[:1], fb[:1])[0]
    assert abs(float(ref) - float(s[0])) <= 1e-5 * float(s[0])
    with pytest.raises(NotImplementedError):
        M.perceptual_batch(a, b, net, criterion='l2')
    with pytest.raises(ValueError):
        M.perceptual_batch(a, b[:, :8], net)


def test_script_perceptual_column(tmp_path, capsys):
    """scripts/calculate_metrics.py --perceptual: the column, the mean and the JSON."""
    import importlib.util
    import json
    from codeformer_amd.utils.img_util import imwrite
    spec = importlib.util.spec_from_file_location('calculate_metrics_script_vgg', os.path.join(R.ROOT, 'scripts', 'calculate_metrics.py'))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    rng = np.random.default_rng(4)
    for d in ('restored', 'gt'):
        os.makedirs(tmp_path / d)
        for n in ('a.png', 'b.png'):
            imwrite(rng.integers(0, 256, (16, 16, 3), dtype=np.uint8), str(tmp_path / d / n))
    out = str(tmp_path / 'out.json')
    assert script.main(['--restored', str(tmp_path / 'restored'), '--gt', str(tmp_path / 'gt'), '--perceptual', '--vgg_layers', 'relu1_1=1', 'relu2_1=0.5',
                        '--json', out]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 3 and all('PERCEPTUAL' in line for line in lines)
    with open(out) as fh:
        res = json.load(fh)
    assert set(res['files']['a.png']) == {'psnr', 'ssim', 'perceptual'} and res['mean']['perceptual'] > 0
    with pytest.raises(SystemExit):
        script.main(['--restored', str(tmp_path / 'restored'), '--gt', str(tmp_path / 'gt'), '--perceptual', '--vgg_layers', 'relu1_1'])


def test_the_lpips_extractor_and_its_refusals():
    """load_lpips_vgg: vgg16 on the five LPIPS taps with the scaling layer in the place of mean / std; lpips_batch is device-only."""
    torch.manual_seed(0)
    net = M.load_lpips_vgg()
    assert net.layer_name_list == ['relu1_2', 'relu2_2', 'relu3_3', 'relu4_3', 'relu5_3'] and list(net.vgg_net._modules)[-1] == 'relu5_3'
    assert torch.equal(net.mean.flatten(), torch.tensor([-.030, -.088, -.188])) and torch.equal(net.std.flatten(), torch.tensor([.458, .448, .450]))
    x = torch.zeros(1, 8, 8, 3)
    with pytest.raises(ValueError):
        M.lpips_batch(x, x, net, [torch.ones(c) for c in (64, 128, 256, 512, 512)])
    import basicsr.metrics as bm
    assert bm.lpips_batch is M.lpips_batch and bm.load_lpips_vgg is M.load_lpips_vgg
