"""Test helper of the VGG / perceptual tests: the cases, the seeded state recipe, the inputs and sample positions (regenerated from seeds,
never stored), the fixture and the loader of the reference's own vgg_arch.py and losses/losses.py.

Cases -- the smallest shapes at which each path of the device dataflow can still go wrong:
  grid    vgg19, B 2, 64x64, taps conv1_2 relu2_2 conv3_4 relu4_4 relu5_4: Winograd at 64^2 / 32^2 / 16^2, the general kernel at 8^2 / 4^2, a
          pre-ReLU tap, a ReLU tap in front of a pool
  odd     vgg16_bn, B 2, 45x37, range_norm, taps bn1_1 relu1_2 relu3_3 relu5_3: every layer off the Winograd grid, every pool floors, BatchNorm
          folded with non-trivial running statistics
  nopool  vgg11, B 1, 24x40, remove_pooling, no input norm, tap relu3_2

State recipe (fill_state; numpy.random.default_rng(seed), one draw per key in SORTED key order): conv weights normal * sqrt(2 / fan_in) (the
scale that keeps a ReLU stack O(1)), scaled per output channel by sqrt(running_var) of a BatchNorm that follows; conv biases normal * 0.1;
BatchNorm gamma uniform [0.5, 1.5] with every fifth or so negative, beta and running mean normal * 0.5, running var log-uniform [0.05, 4].
tests/golden/vgg_ref.npz (tools/make_golden_vgg.py) holds, from the REFERENCE's modules under this recipe on the CPU: the state_dict keys,
the forward keys and shapes per case, the tap values at SAMPLES seeded positions per image in float32 and (module in .double()) float64, the
PerceptualLoss outputs of the loss cases for every criterion in both precisions, and the torch version.  No weights are stored.
"""
import functools
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'vgg_ref.npz')
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle.ref_loader import REF  # noqa: E402  (where the reference tree lies when it is present)
from _tools import rel_err  # noqa: E402,F401  (beside this file; R.rel_err for the tests and tools)

SAMPLES = 1024
CASES = {
    'grid': dict(vgg_type='vgg19', batch=2, hw=(64, 64), taps=['conv1_2', 'relu2_2', 'conv3_4', 'relu4_4', 'relu5_4'], seed=11,
                 kw=dict()),
    'odd': dict(vgg_type='vgg16_bn', batch=2, hw=(45, 37), taps=['bn1_1', 'relu1_2', 'relu3_3', 'relu5_3'], seed=22,
                kw=dict(range_norm=True)),
    'nopool': dict(vgg_type='vgg11', batch=1, hw=(24, 40), taps=['relu3_2'], seed=33,
                   kw=dict(use_input_norm=False, remove_pooling=True)),
}
LOSS_CASES = ('grid', 'odd')       # (PerceptualLoss's constructor cannot ask for remove_pooling)
CRITERIA = ('l1', 'mse', 'fro')
LAYER_W = (0.1, 1.0, 0.5, 2.0, 1.0)   # layer weights of the loss cases, in tap order


def fill_state(module, seed):
    """Fill every conv / BatchNorm parameter and buffer of `module` in place from the recipe above (mean / std stay)."""
    rng = np.random.default_rng(seed)
    sd = module.state_dict()
    new = {}
    for k in sorted(sd):
        shape = tuple(sd[k].shape)
        leaf = k.rpartition('.')[2]
        if leaf == 'num_batches_tracked' or k in ('mean', 'std') or k.endswith(('vgg.mean', 'vgg.std')):
            continue
        is_bn = (k.rpartition('.')[0] + '.running_var') in sd
        if leaf == 'running_var':
            v = np.exp(rng.uniform(np.log(0.05), np.log(4.), shape))
        elif leaf == 'running_mean':
            v = rng.normal(0., 0.5, shape)
        elif is_bn and leaf == 'weight':
            v = rng.uniform(0.5, 1.5, shape) * np.where(rng.random(shape) < 0.2, -1., 1.)
        elif is_bn and leaf == 'bias':
            v = rng.normal(0., 0.5, shape)
        elif leaf == 'weight':
            v = rng.normal(0., 1., shape) * np.sqrt(2. / np.prod(shape[1:]))
        else:
            v = rng.normal(0., 0.1, shape)
        new[k] = v
    for k in sorted(new):
        if k.endswith('.weight') and new[k].ndim == 4:
            bn = k.rpartition('.')[0].replace('conv', 'bn') + '.running_var'
            if bn in new:
                new[k] = new[k] * np.sqrt(new[bn]).reshape(-1, 1, 1, 1)
    with torch.no_grad():
        for k, v in new.items():
            sd[k].copy_(torch.from_numpy(np.asarray(v)).to(sd[k].dtype))
    return module


@functools.lru_cache(maxsize=None)
def case_input(case, which=0):
    """(B,3,H,W) float32, uniform in [0, 1] (in [-1, 1] for a range_norm case); which = 1: the second image batch of the loss cases.  Read-only."""
    c = CASES[case]
    x = np.random.default_rng(c['seed'] + 7 + 100 * which).uniform(0., 1., (c['batch'], 3) + c['hw'])
    if c['kw'].get('range_norm'):
        x = 2. * x - 1.
    return torch.from_numpy(x.astype(np.float32))


def build(cls, case):
    """The case's extractor of class `cls` (this repository's or the reference's VGGFeatureExtractor) under the recipe."""
    c = CASES[case]
    return fill_state(cls(list(c['taps']), vgg_type=c['vgg_type'], **c['kw']), c['seed'])


def layer_weights(case):
    return {k: w for k, w in zip(CASES[case]['taps'], LAYER_W)}


def build_loss(cls, case, criterion, style_weight=1.0):
    """The loss case's PerceptualLoss of class `cls` under the recipe (perceptual_weight 1)."""
    c = CASES[case]
    net = cls(layer_weights(case), vgg_type=c['vgg_type'], use_input_norm=c['kw'].get('use_input_norm', True), range_norm=c['kw'].get('range_norm', False),
              perceptual_weight=1.0, style_weight=style_weight, criterion=criterion)
    fill_state(net.vgg, c['seed'])
    return net


def sample_index(case, tap, shape):
    """(B, min(SAMPLES, c*h*w)) int64: seeded positions into the flattened (c,h,w) of every image of an NCHW tap of `shape`."""
    c = CASES[case]
    n = int(np.prod(shape[1:]))
    rng = np.random.default_rng(c['seed'] * 1000 + c['taps'].index(tap))
    return np.stack([np.sort(rng.choice(n, size=min(SAMPLES, n), replace=False)) for _ in range(shape[0])])


def sample(case, tap, t):
    """The values of the NCHW tap tensor / array `t` at sample_index, (B, samples)."""
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.take_along_axis(a.reshape(a.shape[0], -1), sample_index(case, tap, a.shape), axis=1)


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def reference_available():
    return os.path.isfile(os.path.join(REF, 'basicsr/archs/vgg_arch.py'))


def torchvision_standin():
    """A stand-in for torchvision.models.vgg: this repository's own statement of the `features` stacks (vgg_arch.FeaturesOnly); the
    `pretrained` argument is ignored -- nothing is downloaded, the seeded initialisation stays."""
    from codeformer_amd.archs import vgg_arch
    mod = types.ModuleType('torchvision.models.vgg')
    for t in vgg_arch.NAMES:
        for name in (t, t + '_bn'):
            setattr(mod, name, (lambda name: lambda pretrained=False, **kw: vgg_arch.FeaturesOnly(name))(name))
    return mod


@functools.lru_cache(maxsize=None)
def load_reference():
    """(vgg_arch, losses) modules of the reference, loaded by path under stub packages, with the torchvision stand-in and an empty `lpips`
    in sys.modules while they load; this repository's own basicsr shim is put back afterwards.  Build machine only."""
    if not reference_available():
        raise RuntimeError(f'reference not found under {REF}')
    roots = ('basicsr', 'torchvision', 'lpips')
    saved = {k: v for k, v in sys.modules.items() if k.split('.')[0] in roots}
    for k in saved:
        del sys.modules[k]
    try:
        for pkg in ('basicsr', 'basicsr.utils', 'basicsr.archs', 'basicsr.losses', 'torchvision', 'torchvision.models'):
            m = types.ModuleType(pkg)
            m.__path__ = []
            sys.modules[pkg] = m
        sys.modules['lpips'] = types.ModuleType('lpips')
        sys.modules['torchvision.models.vgg'] = sys.modules['torchvision.models'].vgg = torchvision_standin()
        mods = []
        for name, path in (('basicsr.utils.registry', 'basicsr/utils/registry.py'), ('basicsr.archs.vgg_arch', 'basicsr/archs/vgg_arch.py'),
                           ('basicsr.losses.loss_util', 'basicsr/losses/loss_util.py'), ('basicsr.losses.losses', 'basicsr/losses/losses.py')):
            spec = importlib.util.spec_from_file_location(name, os.path.join(REF, path))
            mod = importlib.util.module_from_spec(spec)
            sys.modules[name] = mod
            spec.loader.exec_module(mod)
            mods.append(mod)
    finally:
        for k in [k for k in sys.modules if k.split('.')[0] in roots]:
            del sys.modules[k]
        sys.modules.update(saved)
    return mods[1], mods[3]
