"""basicsr.metrics on the host (no GPU): the float64 definition of codeformer_amd/metrics.py against the reference's recorded values
(tests/golden/metrics_ref.json, see tests/metrics_ref.py) and against the live reference where its tree is present; the registry and the
shims; the colour conversions; the error types; scripts/calculate_metrics.py; the argument checks of the C entry points.

Gates against the reference: SSIM within 1e-9 (both sides float64: a map entry's error is about 242 terms * 2^-53 * 65025 / C2 = 3e-11);
PSNR without the Y channel equal; PSNR on the Y channel within 1e-5 + |ref| 2^-23 dB (the reference's float32 square and pairwise mean take at
most about 32 roundings = 4.343 * 32 * 2^-24 = 8.3e-6 dB, and its float32 result carries one ulp)."""
import ctypes
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import metrics_ref as R

ROOT = R.ROOT
SCRIPT = os.path.join(ROOT, 'scripts', 'calculate_metrics.py')


@pytest.fixture(scope='module')
def M():
    from codeformer_amd import metrics
    return metrics


@pytest.mark.parametrize('case,family,y', R.ALL, ids=R.IDS)
def test_host_definition_matches_the_recorded_reference(M, case, family, y):
    R.check_against(R.golden()[R.key(case, family, y)], R.per_image(M.calculate_psnr, case, family, y),
                    R.per_image(M.calculate_ssim, case, family, y), y, 'host')


@pytest.mark.skipif(not R.reference_available(), reason='the reference tree is not present')
@pytest.mark.parametrize('case,family,y', R.ALL, ids=R.IDS)
def test_host_definition_matches_the_live_reference(M, case, family, y):
    ps, _, _ = R.load_reference()
    ref = {'psnr': R.per_image(ps.calculate_psnr, case, family, y), 'ssim': R.per_image(ps.calculate_ssim, case, family, y)}
    assert ref == R.golden()[R.key(case, family, y)]      # the fixture is what the reference gives today
    R.check_against(ref, R.per_image(M.calculate_psnr, case, family, y), R.per_image(M.calculate_ssim, case, family, y), y, 'host')


def test_near_family_has_a_squared_error_of_one(M):
    a, b = R.inputs('tiles', 'near')
    d = a[0].astype(np.float64) - b[0]
    assert float((d * d).sum()) == 1.0
    n = (75 - 6) * (141 - 6) * 3
    assert M.calculate_psnr(a[0], b[0], 3) == 20. * np.log10(255. / np.sqrt(1.0 / n))


def test_registry_and_shims():
    import basicsr.metrics
    import basicsr.metrics.metric_util as mu
    import basicsr.metrics.psnr_ssim as ps
    import basicsr.utils.matlab_functions as mf
    from basicsr.utils.registry import METRIC_REGISTRY
    from codeformer_amd import metrics
    assert METRIC_REGISTRY.get('calculate_psnr') is metrics.calculate_psnr is ps.calculate_psnr is basicsr.metrics.calculate_psnr
    assert METRIC_REGISTRY.get('calculate_ssim') is metrics.calculate_ssim is ps.calculate_ssim is basicsr.metrics.calculate_ssim
    assert mu.reorder_image is metrics.reorder_image and mu.to_y_channel is metrics.to_y_channel
    assert all(hasattr(mf, n) for n in ('rgb2ycbcr', 'bgr2ycbcr', 'ycbcr2rgb', 'ycbcr2bgr')) and not hasattr(mf, 'imresize')
    a, b = R.inputs('thin', 'random')
    got = basicsr.metrics.calculate_metric({'img1': a[0], 'img2': b[0]}, {'type': 'calculate_psnr', 'crop_border': 0})
    assert got == metrics.calculate_psnr(a[0], b[0], 0)


def test_colour_conversions_match_the_reference():
    from codeformer_amd.utils import matlab_functions as mf
    gold = np.load(R.GOLDEN_COLOR)
    for tag, img in zip(('u8', 'f32'), R.color_inputs()):
        for name in ('rgb2ycbcr', 'bgr2ycbcr', 'ycbcr2rgb', 'ycbcr2bgr', 'rgb2ycbcr_y', 'bgr2ycbcr_y'):
            fn = getattr(mf, name[:9])
            got = fn(img, y_only=True) if name.endswith('_y') else fn(img)
            ref = gold[f'{name}_{tag}']
            assert got.dtype == ref.dtype == img.dtype and got.shape == ref.shape, name
            if tag == 'u8':
                assert np.array_equal(got, ref), name
            else:
                assert float(np.abs(got.astype(np.float64) - ref).max()) <= 2.0**-22, name
    with pytest.raises(TypeError):
        mf.rgb2ycbcr(np.zeros((4, 4, 3), np.float64))
    with pytest.raises(TypeError):
        mf.ycbcr2bgr(np.zeros((4, 4, 3), np.int32))


def test_reorder_image_and_to_y_channel(M):
    x = np.arange(24, dtype=np.uint8).reshape(2, 3, 4)
    assert M.reorder_image(x[0]).shape == (3, 4, 1)
    assert M.reorder_image(x, 'CHW').shape == (3, 4, 2) and np.array_equal(M.reorder_image(x, 'CHW')[..., 1], x[1])
    assert M.reorder_image(x, 'HWC') is x
    with pytest.raises(ValueError):
        M.reorder_image(x, 'WHC')
    bgr = np.array([[[10, 200, 30], [255, 255, 255], [0, 0, 0]]], dtype=np.float64)
    y = M.to_y_channel(bgr)
    assert y.dtype == np.float32 and y.shape == (1, 3, 1)
    f = (bgr.astype(np.float32) / np.float32(255)).astype(np.float64)
    d = ((f[..., 0] * 24.966 + f[..., 1] * 128.553) + f[..., 2] * 65.481) + 16.0
    assert np.array_equal(y[..., 0], (d / 255.).astype(np.float32) * np.float32(255))
    assert abs(float(y[0, 1, 0]) - 235.0) < 1e-4 and abs(float(y[0, 2, 0]) - 16.0) < 1e-5     # white and black of BT.601
    g = M.to_y_channel(np.full((2, 2, 1), 77.0))
    assert g.dtype == np.float32 and g.shape == (2, 2, 1) and np.array_equal(g, np.float32(77) / np.float32(255) * np.full((2, 2, 1), np.float32(255)))


def test_error_types(M):
    a = np.zeros((16, 16, 3), np.uint8)
    for fn in (M.calculate_psnr, M.calculate_ssim):
        with pytest.raises(ValueError):
            fn(a, a, 0, input_order='WHC')
        with pytest.raises(AssertionError):
            fn(a, a[:15], 0)
    with pytest.raises(ValueError):
        M.calculate_ssim(a[:10], a[:10], 0)
    with pytest.raises(ValueError):
        M.calculate_ssim(a, a, 3)           # 10x10 after the crop
    with pytest.raises(ValueError):
        M.psnr_batch(torch.zeros(1, 16, 16, 3), torch.zeros(1, 16, 16, 3))    # device-only


@pytest.mark.parametrize('case', list(R.CASES))
def test_identical_images_give_inf_and_exactly_one(M, case):
    a, _ = R.inputs(case, 'random')
    _, _, _, _, _, order, crop = R.CASES[case]
    for y in (False, True):
        assert M.calculate_psnr(a[0], a[0].copy(), crop, order, y) == math.inf
        assert M.calculate_ssim(a[0], a[0].copy(), crop, order, y) == 1.0


def test_cpu_tensors_take_the_host_path(M):
    a, b = R.inputs('crop', 'random')
    ta, tb = torch.from_numpy(a[0].copy()), torch.from_numpy(b[0].copy())
    assert M.calculate_psnr(ta, tb, 4) == M.calculate_psnr(a[0], b[0], 4)
    assert M.calculate_ssim(ta, tb, 4, test_y_channel=True) == M.calculate_ssim(a[0], b[0], 4, test_y_channel=True)


def _run_script(*args):
    env = dict(os.environ, HIP_VISIBLE_DEVICES='', CUDA_VISIBLE_DEVICES='')
    return subprocess.run([sys.executable, SCRIPT, *args], capture_output=True, text=True, env=env, timeout=300)


def test_script_scores_a_directory(M, tmp_path):
    from codeformer_amd.utils.img_util import imwrite
    a, b = R.inputs('tiles', 'random')
    for i in range(3):
        imwrite(a[i], str(tmp_path / 'restored' / f'{i}.png'))
        imwrite(b[i], str(tmp_path / 'gt' / f'{i}.png'))
    out = tmp_path / 'out.json'
    r = _run_script('--restored', str(tmp_path / 'restored'), '--gt', str(tmp_path / 'gt'), '--crop_border', '3', '--test_y_channel', '--json', str(out))
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 4 and lines[0].startswith('0.png') and lines[-1].startswith('mean of 3')
    got = json.load(open(out))
    for i in range(3):
        assert got['files'][f'{i}.png']['psnr'] == M.calculate_psnr(a[i], b[i], 3, 'HWC', True)
        assert got['files'][f'{i}.png']['ssim'] == M.calculate_ssim(a[i], b[i], 3, 'HWC', True)
    assert got['mean']['ssim'] == float(np.mean([got['files'][f'{i}.png']['ssim'] for i in range(3)]))
    # a size mismatch and a missing partner are errors that name the file
    imwrite(b[1][:40], str(tmp_path / 'gt' / '1.png'))
    r = _run_script('--restored', str(tmp_path / 'restored'), '--gt', str(tmp_path / 'gt'))
    assert r.returncode != 0 and '1.png' in r.stderr and '141x40' in r.stderr
    os.remove(tmp_path / 'gt' / '1.png')
    r = _run_script('--restored', str(tmp_path / 'restored'), '--gt', str(tmp_path / 'gt'))
    assert r.returncode != 0 and '1.png' in r.stderr and 'no ground truth' in r.stderr


def test_c_entry_points_report_argument_errors_without_a_gpu():
    """Every call below fails a check, so nothing is launched: the pointers are placeholders, not device memory."""
    from codeformer_amd import build as cf_build
    from codeformer_amd import lib
    cf_build.build()
    n = lib.load()
    s = (ctypes.c_int64 * 4)(16 * 16 * 3, 16 * 3, 3, 1)

    def psnr(a=1, b=1, batch=1, h=16, w=16, c=3, sa=s, sb=s, dt=0, y=0, parts=1, sse=1):
        return n.cf_psnr(a, b, batch, h, w, c, sa, sb, dt, y, parts, sse, None, None)

    def ssim(a=1, b=1, batch=1, h=16, w=16, c=3, sa=s, sb=s, dt=0, y=0, parts=1, out=1):
        return n.cf_ssim(a, b, batch, h, w, c, sa, sb, dt, y, parts, out, None)

    for fn, who in ((psnr, 'cf_psnr'), (ssim, 'cf_ssim')):
        for kw in (dict(a=None), dict(b=None), dict(sa=None), dict(sb=None), dict(parts=None)):
            assert fn(**kw) == -1 and 'null' in lib.last_error() and who in lib.last_error(), kw
        assert fn(c=2) == -1 and 'channels 2' in lib.last_error()
        assert fn(c=4) == -1 and 'channels 4' in lib.last_error()
        for kw in (dict(batch=0), dict(h=0), dict(w=-1)):
            assert fn(**kw) == -1 and 'bad dims' in lib.last_error(), kw
        assert fn(dt=2) == -1 and 'dtype' in lib.last_error()
        assert fn(y=2) == -1 and 'y_channel' in lib.last_error()
        big = (ctypes.c_int64 * 4)(0, 1 << 16, 3, 1)
        assert fn(h=(1 << 15) + 1, sa=big) == -1 and '2^31' in lib.last_error()     # the last row starts at 2^15 * 2^16 elements
        assert fn(h=(1 << 15) + 1, sb=big) == -1 and '2^31' in lib.last_error()
        assert fn(sa=(ctypes.c_int64 * 4)(0, -48, 3, 1)) == -1 and 'stride' in lib.last_error()
    assert psnr(sse=None) == -1 and 'null' in lib.last_error()
    assert ssim(out=None) == -1 and 'null' in lib.last_error()
    assert ssim(h=10) == -1 and '11x11' in lib.last_error()
    assert ssim(w=10) == -1 and '11x11' in lib.last_error()
    assert n.cf_metric_parts(0, 16, 3) == -1 and n.cf_metric_parts(16, 16, 2) == -1
    assert n.cf_metric_parts(8, 8, 3) == 1 and n.cf_metric_parts(512, 512, 3) >= 64
    # tiling depends on (h, w) only: the slot count grows with the image and with the planes, never with anything else
    assert n.cf_metric_parts(512, 512, 3) == 3 * n.cf_metric_parts(512, 512, 1)
