"""Test helper of the ArcFace tests: the network cases, the seeded state recipe, the inputs (regenerated from seeds, never stored), the
fixture and the loader of the reference's own arcface_arch.py.

Network cases (the architecture fixes the 128 x 128 input):
  r18   layers [2,2,2,2], use_se False, B 3   the configuration identity scoring uses
  se    layers [1,1,1,1], use_se True,  B 2   every SE kernel, the smallest depth

State recipe (fill_state; numpy.random.default_rng(seed), one draw per key in SORTED key order, so it does not depend on torch's generator):
  BatchNorm   gamma uniform in [0.5, 1.5], every fifth entry or so negative; beta and running mean normal O(1), the beta of a bn0 +-[1.5, 2.5] (a
              border error of the bn0 fold then stands far above any tolerance); running var log-uniform in [1e-6, 4], so eps = 1e-5 matters
  PReLU       the slopes -0.5, 0, 0.25, 1.5 in rotation over the sorted keys (negative, zero, ordinary, above one)
  conv / fc   normal * sqrt(1 / fan_in), then scaled so that activations stay O(1) through normalisations whose running variance spans
              six decades: output channels by sqrt(var + eps) of the BatchNorm that follows (convN -> bnN, downsample.0 -> downsample.1,
              fc5 -> bn5), input channels by sqrt(var + eps) of the BatchNorm in front (bn0 -> conv1, bn4 -> fc5); fc biases normal * 0.5
tests/golden/arcface_ref.npz (tools/make_golden_arcface.py) holds, from the REFERENCE's module under this recipe: its state_dict key and
shape list, per case its CPU embeddings in float32 and, from the same module in .double(), in float64, a sha256 per key of its
torch.manual_seed(0) default initialisation, and the torch version that produced them (host_id).  No weights are stored.
"""
import functools
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'arcface_ref.npz')
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle.ref_loader import REF  # noqa: E402  (where the reference tree lies when it is present)
from _tools import rel_err  # noqa: E402,F401  (beside this file; R.rel_err for the tests and tools)

CASES = {
    'r18': dict(layers=[2, 2, 2, 2], use_se=False, batch=3, seed=101),
    'se': dict(layers=[1, 1, 1, 1], use_se=True, batch=2, seed=202),
}
SLOPES = (-0.5, 0.0, 0.25, 1.5)


def _bn_of(key):
    """Prefix of the BatchNorm that follows the conv / linear weight `key`, or None."""
    head, _, leaf = key.rpartition('.')
    mod = head.rpartition('.')[2]
    base = head[:len(head) - len(mod)]
    if mod in ('conv1', 'conv2'):
        return base + 'bn' + mod[-1]
    if mod == '0' and base.endswith('downsample.'):
        return base + '1'
    if mod == 'fc5':
        return base + 'bn5'
    return None


def fill_state(module, seed, slope=None):
    """Fill every parameter and buffer of `module` (a ResNetArcFace, or one of its blocks) in place from the recipe above.
    slope: one value for every PReLU instead of the rotation."""
    rng = np.random.default_rng(seed)
    sd = module.state_dict()
    new, n_prelu = {}, 0
    for k in sorted(sd):
        shape = tuple(sd[k].shape)
        leaf = k.rpartition('.')[2]
        parent = k.rpartition('.')[0].rpartition('.')[2]
        if leaf == 'num_batches_tracked':
            continue
        is_bn = (k.rpartition('.')[0] + '.running_var') in sd
        if leaf == 'running_var':
            v = np.exp(rng.uniform(np.log(1e-6), np.log(4.), shape))
        elif leaf == 'running_mean':
            v = rng.normal(0., 1., shape)
        elif is_bn and leaf == 'weight':
            v = rng.uniform(0.5, 1.5, shape) * np.where(rng.random(shape) < 0.2, -1., 1.)
        elif is_bn and leaf == 'bias':
            v = rng.normal(0., 1., shape)
            if parent == 'bn0':
                v = rng.uniform(1.5, 2.5, shape) * np.where(rng.random(shape) < 0.5, -1., 1.)
        elif shape == (1,) and leaf == 'weight':   # nn.PReLU()
            v = np.full(shape, SLOPES[n_prelu % len(SLOPES)] if slope is None else slope)
            n_prelu += 1
        elif leaf == 'weight':
            v = rng.normal(0., 1., shape) * np.sqrt(1. / np.prod(shape[1:]))
        else:   # Linear bias
            v = rng.normal(0., 0.5, shape)
        new[k] = v
    eps = 1e-5
    for k in sorted(new):
        if not k.endswith('.weight') or new[k].ndim < 2:
            continue
        bn = _bn_of(k)
        if bn is not None and bn + '.running_var' in new:
            new[k] = new[k] * np.sqrt(new[bn + '.running_var'] + eps).reshape((-1,) + (1,) * (new[k].ndim - 1))
        head = k.rpartition('.')[0]
        pre = head[:len(head) - len('conv1')] + 'bn0' if head.endswith('conv1') else head[:len(head) - len('fc5')] + 'bn4' if head.endswith('fc5') else None
        if pre is not None and pre + '.running_var' in new:
            s = np.sqrt(new[pre + '.running_var'] + eps)
            if new[k].ndim == 4:
                new[k] = new[k] * s.reshape(1, -1, 1, 1)
            else:   # fc5: columns in the reference's c * 64 + h * 8 + w order
                new[k] = new[k] * np.repeat(s, new[k].shape[1] // s.size)[None]
    with torch.no_grad():
        for k, v in new.items():
            sd[k].copy_(torch.from_numpy(np.asarray(v)).to(sd[k].dtype))
    return module


@functools.lru_cache(maxsize=None)
def case_input(case):
    """(B,1,128,128) float32, normal: read-only."""
    c = CASES[case]
    x = torch.from_numpy(np.random.default_rng(c['seed'] + 7).normal(0., 1., (c['batch'], 1, 128, 128)).astype(np.float32))
    return x


def build(cls, case):
    """The case's network of class `cls` (this repository's or the reference's ResNetArcFace) under the recipe, in eval mode."""
    c = CASES[case]
    return fill_state(cls('IRBlock', list(c['layers']), use_se=c['use_se']), c['seed']).eval()


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def reference_available():
    return os.path.isfile(os.path.join(REF, 'basicsr/archs/arcface_arch.py'))


@functools.lru_cache(maxsize=None)
def load_reference():
    """The reference's arcface_arch module, loaded by path under stub packages; this repository's own basicsr shim is put back afterwards."""
    if not reference_available():
        raise RuntimeError(f'reference not found under {REF}')
    saved = {k: v for k, v in sys.modules.items() if k.split('.')[0] == 'basicsr'}
    for k in saved:
        del sys.modules[k]
    try:
        for pkg in ('basicsr', 'basicsr.utils', 'basicsr.archs'):
            m = types.ModuleType(pkg)
            m.__path__ = []
            sys.modules[pkg] = m
        for name, path in (('basicsr.utils.registry', 'basicsr/utils/registry.py'), ('basicsr.archs.arcface_arch', 'basicsr/archs/arcface_arch.py')):
            spec = importlib.util.spec_from_file_location(name, os.path.join(REF, path))
            mod = importlib.util.module_from_spec(spec)
            sys.modules[name] = mod
            spec.loader.exec_module(mod)
    finally:
        for k in [k for k in sys.modules if k.split('.')[0] == 'basicsr']:
            del sys.modules[k]
        sys.modules.update(saved)
    return mod


def init_digest(net):
    """One sha256 (hex) per state_dict entry, over its bytes, in sorted key order: equal draws, equal digest, whatever sums them."""
    import hashlib
    sd = net.state_dict()
    return np.array([hashlib.sha256(sd[k].detach().contiguous().numpy().tobytes()).hexdigest() for k in sorted(sd)])


def host_id():
    """The torch version the bitwise host checks are keyed on.  (Thread count does not matter: 1, 4, 8, 16 give the same bits.  The CPU
    model does -- see test_forward_host_against_reference.)"""
    return torch.__version__


def cosines(e):
    """The cosine of every pair of rows of e, float64."""
    e = np.asarray(e, dtype=np.float64)
    n = np.linalg.norm(e, axis=1)
    return (e @ e.T) / np.maximum(np.outer(n, n), 1e-8)
