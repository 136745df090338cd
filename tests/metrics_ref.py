"""Test helper of the metrics tests: the cases, the input families (regenerated from seeds, never stored), the fixture, and the loader of the
reference's own metric files.

Cases -- the smallest shapes at which a tile, a halo or a stride can go wrong, whatever the tile size:
  one    1 x 11x11   C 1  uint8    HWC  crop 0   a single SSIM output
  thin   1 x 12x43   C 3  uint8    HWC  crop 0   one ragged tile, 2x33 outputs
  crop   2 x 31x40   C 3  float32  HWC  crop 4   the crop through strides
  chw    1 x 45x76   C 3  float32  CHW  crop 0   channel stride != 1
  tiles  3 x 75x141  C 3  uint8    HWC  crop 3   59x125 outputs: several tiles in both axes, ragged last ones, B 3
Families (b against a; float32 cases add 0.25, capped at 255, so that values are not integers):
  random    b = a plus noise in +-20, clipped
  flat      200 against 201: the variance cancels exactly
  checker   a 0/255 board against its inverse: SSIM is negative and the magnitudes are the largest
  near      one LSB of one B-channel pixel differs: sse == 1, and the Y path is sensitive to one ulp
  smooth    a product of sinusoids against its shifted, offset copy
  impulses  b = a +- 9 at the corners (of the image and of the cropped region) and where rows and columns 15, 16, 31, 32, 63, 64 cross

tests/golden/metrics_ref.json holds what the reference's calculate_psnr / calculate_ssim return for every case x family x Y flag, image by image
(tools/make_golden_metrics.py).  The reference files run under a stub cv2 whose getGaussianKernel is the window's formula and whose filter2D
is a plain 121-term correlation over the valid region: the fixture pins the reference's cropping, ordering, Y conversion and channel
averaging, NOT OpenCV's filter (cv2 is not available to pin it).
"""
import functools
import importlib.util
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'metrics_ref.json')
GOLDEN_COLOR = os.path.join(ROOT, 'tests', 'golden', 'matlab_color_ref.npz')
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle.ref_loader import REF  # noqa: E402  (where the reference tree lies when it is present)

#        name     B   H    W   C  dtype      order  crop
CASES = {
    'one':   (1, 11, 11, 1, 'uint8', 'HWC', 0),
    'thin':  (1, 12, 43, 3, 'uint8', 'HWC', 0),
    'crop':  (2, 31, 40, 3, 'float32', 'HWC', 4),
    'chw':   (1, 45, 76, 3, 'float32', 'CHW', 0),
    'tiles': (3, 75, 141, 3, 'uint8', 'HWC', 3),
}
FAMILIES = ('random', 'flat', 'checker', 'near', 'smooth', 'impulses')
GRID = (15, 16, 31, 32, 63, 64)
ALL = [(c, f, y) for c in CASES for f in FAMILIES for y in (False, True)]
IDS = [f'{c}-{f}-{"y" if y else "c"}' for c, f, y in ALL]


def key(case, family, y):
    return f'{case}/{family}/{"y" if y else "c"}'


@functools.lru_cache(maxsize=None)
def inputs(case, family):
    """(a, b): two read-only arrays of the case's dtype, (B,H,W,C) for 'HWC' and (B,C,H,W) for 'CHW', integers in [0, 255] (+ 0.25 in float32)."""
    B, H, W, C, dtype, order, crop = CASES[case]
    rng = np.random.default_rng(1000 * list(CASES).index(case) + FAMILIES.index(family))
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    base = rng.integers(0, 256, (B, H, W, C))
    if family == 'random':
        a, b = base, np.clip(base + rng.integers(-20, 21, base.shape), 0, 255)
    elif family == 'flat':
        a, b = np.full(base.shape, 200), np.full(base.shape, 201)
    elif family == 'checker':
        a = np.broadcast_to((255 * ((yy + xx) % 2))[None, :, :, None], base.shape).copy()
        b = 255 - a
    elif family == 'near':
        a, b = base, base.copy()
        b[:, H // 2, W // 2, 0] ^= 1
    elif family == 'smooth':
        ph = np.arange(B)[:, None, None, None] + np.arange(C)[None, None, None, :]
        a = np.rint(127.5 + 100 * np.sin((xx[None, :, :, None] + ph) / 7.) * np.cos(yy[None, :, :, None] / 5.)).astype(np.int64)
        b = np.rint(130.5 + 100 * np.sin((xx[None, :, :, None] + ph + 1) / 7.) * np.cos(yy[None, :, :, None] / 5.)).astype(np.int64)
    else:
        a, b = base, base.copy()
        pts = {(r, c) for r in GRID for c in GRID if r < H and c < W}
        for lo in (0, crop):
            pts |= {(lo, lo), (lo, W - 1 - lo), (H - 1 - lo, lo), (H - 1 - lo, W - 1 - lo)}
        for r, c in sorted(pts):
            b[:, r, c, :] += np.where(a[:, r, c, :] < 128, 9, -9)
    out = []
    for t in (a, b):
        t = t.astype(np.uint8) if dtype == 'uint8' else np.minimum(t.astype(np.float32) + np.float32(0.25), np.float32(255))
        if order == 'CHW':
            t = t.transpose(0, 3, 1, 2)
        t = np.ascontiguousarray(t)
        t.setflags(write=False)
        out.append(t)
    return tuple(out)


def color_inputs():
    """The two images of the colour-conversion fixture: 16x16x3 uint8, and float32 in [0, 1]."""
    rng = np.random.default_rng(77)
    return rng.integers(0, 256, (16, 16, 3)).astype(np.uint8), rng.random((16, 16, 3)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def reference_available():
    return os.path.isfile(os.path.join(REF, 'basicsr/metrics/psnr_ssim.py'))


def _cv2_stub():
    cv2 = types.ModuleType('cv2')

    def getGaussianKernel(ksize, sigma):
        i = np.arange(ksize, dtype=np.float64) - (ksize - 1) / 2.
        g = np.exp(-i**2 / (2 * sigma**2))
        return (g / g.sum())[:, None]

    def filter2D(img, ddepth, window):
        kh, kw = window.shape
        h, w = img.shape
        out = np.zeros((h, w))
        acc = np.zeros((h - kh + 1, w - kw + 1))
        for i in range(kh):
            for j in range(kw):
                acc += window[i, j] * img[i:i + h - kh + 1, j:j + w - kw + 1]
        out[kh // 2:kh // 2 + acc.shape[0], kw // 2:kw // 2 + acc.shape[1]] = acc   # only the valid region is defined
        return out

    cv2.getGaussianKernel, cv2.filter2D = getGaussianKernel, filter2D
    return cv2


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


@functools.lru_cache(maxsize=None)
def load_reference():
    """(psnr_ssim, metric_util, matlab_functions) modules of the reference, loaded by path under stub packages (and the stub cv2 above);
    this repository's own basicsr shim is put back afterwards."""
    if not reference_available():
        raise RuntimeError(f'reference not found under {REF}')
    names = ('basicsr', 'cv2')
    saved = {k: v for k, v in sys.modules.items() if k.split('.')[0] in names}
    for k in saved:
        del sys.modules[k]
    try:
        for pkg in ('basicsr', 'basicsr.utils', 'basicsr.metrics'):
            m = types.ModuleType(pkg)
            m.__path__ = []
            sys.modules[pkg] = m
        sys.modules['cv2'] = _cv2_stub()
        _load('basicsr.utils.registry', f'{REF}/basicsr/utils/registry.py')
        mat = _load('basicsr.utils.matlab_functions', f'{REF}/basicsr/utils/matlab_functions.py')
        util = _load('basicsr.metrics.metric_util', f'{REF}/basicsr/metrics/metric_util.py')
        ps = _load('basicsr.metrics.psnr_ssim', f'{REF}/basicsr/metrics/psnr_ssim.py')
    finally:
        for k in [k for k in sys.modules if k.split('.')[0] in names]:
            del sys.modules[k]
        sys.modules.update(saved)
    return ps, util, mat


def per_image(fn, case, family, y):
    """[fn(a[i], b[i], crop, order, y) for every image pair of the case]."""
    a, b = inputs(case, family)
    _, _, _, _, _, order, crop = CASES[case]
    return [float(fn(a[i], b[i], crop, order, y)) for i in range(a.shape[0])]


@functools.lru_cache(maxsize=None)
def host_values(case, family, y):
    """{'psnr': [...], 'ssim': [...]} of the host definition (codeformer_amd/metrics.py), image by image; computed once."""
    from codeformer_amd import metrics
    return {'psnr': per_image(metrics.calculate_psnr, case, family, y), 'ssim': per_image(metrics.calculate_ssim, case, family, y)}


def check_against(ref, psnr, ssim, y, what):
    """The gates of the host definition (or the device) against the reference's values, image by image."""
    for r, p in zip(ref['psnr'], psnr):
        if y:   # the reference's float32 square and pairwise mean: <= 32 roundings = 4.343 * 32 * 2^-24 = 8.3e-6 dB, and one ulp of its float32 result
            assert abs(p - r) <= 1e-5 + abs(r) * 2.0**-23, (what, p, r)
        else:
            assert p == r, (what, p, r)
    for r, s in zip(ref['ssim'], ssim):
        assert abs(s - r) <= 1e-9, (what, s, r)
