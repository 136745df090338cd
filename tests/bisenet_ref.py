"""Test helper of the BiSeNet tests: the cases, the seeded state recipe, the inputs and sample positions (regenerated from seeds, never
stored), the fixture, the loader of the reference's own facelib/parsing/{resnet,bisenet}.py, and numpy restatements of the definitions of
the five kernels of cf_bisenet.hip (include/codeformer_hip.h, "BiSeNet / face parsing").

Cases -- the smallest shapes at which each path of the device dataflow can still go wrong:
  square  B 2, 64x64     feat32 is 2x2, below every tile
  wide    B 1, 96x160    non-square, feat32 3x5 (odd), levels off the 16-pixel Winograd grid
  batch   B 3, 128x128   batch invariance; x8 / x16 bilinear upsampling over several source pixels

State recipe (fill_state; numpy.random.default_rng(seed), one draw per key in SORTED key order, the distributions of vgg_ref.fill_state): conv
weights normal * sqrt(2 / fan_in); BatchNorm gamma uniform [0.5, 1.5] with every fifth or so negative, beta and running mean normal * 0.5,
running var log-uniform [0.05, 4].  Every conv that feeds a BatchNorm is scaled per output channel by sqrt(running_var) of that BatchNorm
(conv* -> bn*, downsample.0 -> downsample.1, conv_atten -> bn_atten): without it the activations reach 1e9, with it a few hundred.  The
gate weights (conv_atten.weight, ffm.conv2.weight) are scaled by GATE_SCALE = 0.1 on top: without it nearly every sigmoid gate is saturated,
and a saturated gate hides a wrong one.  The generator asserts that at least 30 % of the gates of every case lie in [0.05, 0.95].

tests/golden/bisenet_ref.npz (tools/make_golden_bisenet.py) holds, from the REFERENCE's modules under this recipe on the CPU: the state_dict
keys and shapes; per case the six return_feat=True outputs and ResNet18's three features at SAMPLES seeded positions per image in float32
and (module in .double()) float64, the full-map scalars max|f32 - f64| and max|f64| per output, the float64 labels of `out` (uint8) and its
float64 top-2 gap (float32); the gate statistics; the torch version.  No weights are stored.
"""
import functools
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'bisenet_ref.npz')
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle.ref_loader import REF  # noqa: E402  (where the reference tree lies when it is present)
from _tools import rel_err  # noqa: E402,F401  (beside this file; R.rel_err for the tests and tools)

SAMPLES = 1024
NUM_CLASS = 19
GATE_SCALE = 0.1
GATE_BAND = (0.05, 0.95)
CASES = {
    'square': dict(batch=2, hw=(64, 64), seed=101),
    'wide': dict(batch=1, hw=(96, 160), seed=202),
    'batch': dict(batch=3, hw=(128, 128), seed=303),
}
OUTPUTS = ('out', 'out16', 'out32', 'feat', 'feat16', 'feat32')   # forward(x, return_feat=True), in its order
RES_FEATS = ('res8', 'res16', 'res32')                           # ResNet18.forward
TAPS = OUTPUTS + RES_FEATS
GATE_KEYS = ('conv_atten.weight', 'ffm.conv2.weight')


def _bn_of(key):
    """The running_var key of the BatchNorm a conv weight `key` feeds, by the naming of the two files."""
    prefix = key.rpartition('.')[0]          # the conv module
    parent, _, leaf = prefix.rpartition('.')
    if leaf == '0' and parent.endswith('downsample'):
        bn = '1'
    elif leaf == 'conv_atten':
        bn = 'bn_atten'
    elif leaf.startswith('conv'):
        bn = 'bn' + leaf[4:]
    else:
        return None
    return (parent + '.' if parent else '') + bn + '.running_var'


def fill_state(module, seed):
    """Fill every conv / BatchNorm parameter and buffer of `module` in place from the recipe above."""
    rng = np.random.default_rng(seed)
    sd = module.state_dict()
    new = {}
    for k in sorted(sd):
        shape = tuple(sd[k].shape)
        leaf = k.rpartition('.')[2]
        if leaf == 'num_batches_tracked':
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
            bn = _bn_of(k)
            if bn in new:
                new[k] = new[k] * np.sqrt(new[bn]).reshape(-1, 1, 1, 1)
            if k.endswith(GATE_KEYS):
                new[k] = new[k] * GATE_SCALE
    with torch.no_grad():
        for k, v in new.items():
            sd[k].copy_(torch.from_numpy(np.asarray(v)).to(sd[k].dtype))
    return module


@functools.lru_cache(maxsize=None)
def case_input(case):
    """(B,3,H,W) float32, uniform in [-1, 1].  Read-only."""
    c = CASES[case]
    return torch.from_numpy(np.random.default_rng(c['seed'] + 7).uniform(-1., 1., (c['batch'], 3) + c['hw']).astype(np.float32))


def build(cls, case):
    """The case's network of class `cls` (this repository's or the reference's BiSeNet) under the recipe, in eval mode."""
    return fill_state(cls(NUM_CLASS), CASES[case]['seed']).eval()


def run_taps(net, x):
    """{tap: NCHW tensor} of `net` on x: the six return_feat outputs and the three ResNet18 features, from the module's own forward."""
    with torch.no_grad():
        outs = net(x, return_feat=True)
        res = net.cp.resnet(x)
    return dict(zip(TAPS, tuple(outs) + tuple(res)))


def sample_index(case, tap, shape):
    """(B, min(SAMPLES, c*h*w)) int64: seeded positions into the flattened (c,h,w) of every image of an NCHW tap of `shape`."""
    n = int(np.prod(shape[1:]))
    rng = np.random.default_rng(CASES[case]['seed'] * 1000 + TAPS.index(tap))
    return np.stack([np.sort(rng.choice(n, size=min(SAMPLES, n), replace=False)) for _ in range(shape[0])])


def sample(case, tap, t):
    """The values of the NCHW tap tensor / array `t` at sample_index, (B, samples)."""
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.take_along_axis(a.reshape(a.shape[0], -1), sample_index(case, tap, a.shape), axis=1)


def top2_gap(logits):
    """(B,H,W): largest minus second largest over dim 1 of an NCHW array."""
    s = np.sort(np.asarray(logits), axis=1)
    return s[:, -1] - s[:, -2]


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def reference_available():
    return os.path.isfile(os.path.join(REF, 'facelib/parsing/bisenet.py'))


@functools.lru_cache(maxsize=None)
def load_reference():
    """(resnet, bisenet) modules of the reference, loaded by path under a stub package (bisenet.py imports `.resnet` relatively); this
    repository's own facelib shim is put back afterwards.  Build machine only."""
    if not reference_available():
        raise RuntimeError(f'reference not found under {REF}')
    saved = {k: v for k, v in sys.modules.items() if k.split('.')[0] == 'facelib'}
    for k in saved:
        del sys.modules[k]
    try:
        for pkg in ('facelib', 'facelib.parsing'):
            m = types.ModuleType(pkg)
            m.__path__ = []
            sys.modules[pkg] = m
        mods = []
        for name, path in (('facelib.parsing.resnet', 'facelib/parsing/resnet.py'), ('facelib.parsing.bisenet', 'facelib/parsing/bisenet.py')):
            spec = importlib.util.spec_from_file_location(name, os.path.join(REF, path))
            mod = importlib.util.module_from_spec(spec)
            sys.modules[name] = mod
            spec.loader.exec_module(mod)
            mods.append(mod)
    finally:
        for k in [k for k in sys.modules if k.split('.')[0] == 'facelib']:
            del sys.modules[k]
        sys.modules.update(saved)
    return tuple(mods)


def gate_values(net, x):
    """Every sigmoid gate `net` (a reference or repository BiSeNet on the CPU) evaluates on x, flattened: arm16, arm32 and the fusion gate."""
    got = []
    hooks = [m.register_forward_hook(lambda mod, i, o: got.append(o.detach().reshape(-1).numpy())) for m in net.modules() if isinstance(m, torch.nn.Sigmoid)]
    try:
        with torch.no_grad():
            net(x)
    finally:
        for h in hooks:
            h.remove()
    return np.concatenate(got)


# ---- numpy restatements of the kernel definitions ---------------------------------------------------------------------------------------
def stem_ref(x, w, b, dtype=np.float64, relu=True):
    """cf_stem7x7s2: x (B,3,H,W), w (64,3,7,7), b (64,) -> (B,ho,wo,64) = relu(conv 7x7 / stride 2 / zero pad 3 + b), in `dtype`."""
    x, w, b = np.asarray(x, dtype), np.asarray(w, dtype), np.asarray(b, dtype)
    B, C, H, W = x.shape
    ho, wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = np.zeros((B, C, 2 * ho + 5, 2 * wo + 5), dtype)
    xp[:, :, 3:3 + H, 3:3 + W] = x
    out = np.zeros((B, ho, wo, w.shape[0]), dtype)
    for c in range(C):        # ascending (c, ky, kx): the K order of the packed weight
        for ky in range(7):
            for kx in range(7):
                out += xp[:, c, ky:ky + 2 * ho:2, kx:kx + 2 * wo:2][..., None] * w[:, c, ky, kx]
    out = out + b
    return np.where((out > 0) | np.isnan(out), out, 0).astype(dtype) if relu else out


def maxpool3s2_ref(x):
    """cf_maxpool3s2: x (B,H,W,C) -> (B,(H-1)//2+1,(W-1)//2+1,C), the max over the taps inside the image; a NaN wins."""
    x = np.asarray(x)
    B, H, W, C = x.shape
    ho, wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out = np.full((B, ho, wo, C), -np.inf, x.dtype)
    for oy in range(ho):
        for ox in range(wo):
            win = x[:, max(2 * oy - 1, 0):min(2 * oy + 2, H), max(2 * ox - 1, 0):min(2 * ox + 2, W)].reshape(B, -1, C)
            out[:, oy, ox] = np.where(np.isnan(win).any(1), np.nan, win.max(1))
    return out


def pooled_fc_ref(p, w, b, act=None, dtype=np.float64):
    """cf_pooled_fc: (act(W p + b), sum |w p| + |b|) in `dtype`; act None | 'relu' | 'sigmoid'."""
    p, w, b = np.asarray(p, dtype), np.asarray(w, dtype), np.asarray(b, dtype)
    s = p @ w.T + b
    mag = np.abs(p) @ np.abs(w).T + np.abs(b)
    if act == 'relu':
        s = np.maximum(s, 0)
    elif act == 'sigmoid':
        s = 1 / (1 + np.exp(-s))
    return s, mag


def scale_add_row_ref(x, g, r):
    """cf_scale_add_row: x (B,H,W,C) * g (B,C) + r (B,C), the product rounded before the sum, in x's dtype."""
    x = np.asarray(x)
    t = (x * np.asarray(g, x.dtype)[:, None, None, :]).astype(x.dtype)
    return (t + np.asarray(r, x.dtype)[:, None, None, :]).astype(x.dtype)


def _ac_axis(n_in, n_out, dtype):
    scale = dtype(n_in - 1) / dtype(n_out - 1) if n_out > 1 else dtype(0)
    src = (scale * np.arange(n_out).astype(dtype)).astype(dtype)
    i0 = np.clip(src.astype(np.int64), 0, n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = (src - i0.astype(dtype)).astype(dtype)
    return i0, i1, (dtype(1) - l1).astype(dtype), l1


def resize_bilinear_ac_ref(x, c, size, dtype=np.float32):
    """cf_resize_bilinear_ac: the first c channels of x (B,h,w,ld) -> (B,c,H,W); every step one operation in `dtype`."""
    x = np.asarray(x, dtype)[..., :c]
    y0, y1, l0y, l1y = _ac_axis(x.shape[1], size[0], dtype)
    x0, x1, l0x, l1x = _ac_axis(x.shape[2], size[1], dtype)
    l0x, l1x = l0x[None, None, :, None], l1x[None, None, :, None]
    l0y, l1y = l0y[None, :, None, None], l1y[None, :, None, None]
    a, b = x[:, y0][:, :, x0], x[:, y0][:, :, x1]
    cc, d = x[:, y1][:, :, x0], x[:, y1][:, :, x1]
    top = ((l0x * a).astype(dtype) + (l1x * b).astype(dtype)).astype(dtype)
    bot = ((l0x * cc).astype(dtype) + (l1x * d).astype(dtype)).astype(dtype)
    out = ((l0y * top).astype(dtype) + (l1y * bot).astype(dtype)).astype(dtype)
    return np.ascontiguousarray(out.transpose(0, 3, 1, 2))
