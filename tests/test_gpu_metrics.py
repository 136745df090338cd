"""-m gpu: basicsr.metrics on the device (csrc/cf_metrics.hip) against the host definition of codeformer_amd/metrics.py and the recorded
reference (tests/metrics_ref.py holds the cases, the families and the gates).

Bounds against the host definition, both float64: SSIM within 1e-9 (a map entry's error is about 242 terms * 2^-53 * 65025 / C2 = 3e-11, whatever
the order of the taps and with or without fused multiply-adds); calculate_psnr of uint8 colour inputs EQUAL, because the squared-error sum is an
exact integer and the device path applies the host's expression to it; every other PSNR within 1e-9 dB (float64 sums of non-negative terms have
a relative error <= N 2^-53, and 20 log10 turns a relative error r of the sum into 8.7 r dB) -- on the Y path that holds only if Y has the
host's bits: one float32 ulp of one Y moves the `near` family by 1e-3 dB.  The invariances (batch row, repeat, crop, order, slice) are bitwise."""
import math

import numpy as np
import pytest
import torch

import metrics_ref as R
from _tools import _bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def M():
    from codeformer_amd import build as cf_build
    from codeformer_amd import metrics
    cf_build.build()
    assert torch.cuda.is_available()
    return metrics


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _both(M, a, b, crop, order, y):
    """(psnr_batch, ssim_batch) of two device batches."""
    return M.psnr_batch(a, b, crop, order, y), M.ssim_batch(a, b, crop, order, y)


def _same_bits(x, y):
    return all(np.array_equal(_bits(p), _bits(q)) for p, q in zip(x, y))


@pytest.mark.parametrize('case,family,y', R.ALL, ids=R.IDS)
def test_device_matches_the_host_definition(M, case, family, y):
    B, H, W, C, dtype, order, crop = R.CASES[case]
    a, b = (_dev(t) for t in R.inputs(case, family))
    host = R.host_values(case, family, y)
    pb, sb = (t.cpu().tolist() for t in _both(M, a, b, crop, order, y))
    ps = [M.calculate_psnr(a[i], b[i], crop, order, y) for i in range(B)]
    ss = [M.calculate_ssim(a[i], b[i], crop, order, y) for i in range(B)]
    print(f'{case}/{family}/{"y" if y else "c"}: max |psnr_batch - host| {max(abs(p - h) for p, h in zip(pb, host["psnr"])):.3e} dB, '
          f'|calculate_psnr - host| {max(abs(p - h) for p, h in zip(ps, host["psnr"])):.3e} dB, '
          f'|ssim - host| {max(abs(s - h) for s, h in zip(sb, host["ssim"])):.3e}')
    for i in range(B):
        assert isinstance(ps[i], float) and isinstance(ss[i], float)
        if dtype == 'uint8' and C == 3 and not y:
            assert ps[i] == host['psnr'][i]
        assert abs(ps[i] - host['psnr'][i]) <= 1e-9
        assert abs(pb[i] - host['psnr'][i]) <= 1e-9
        assert abs(ss[i] - host['ssim'][i]) <= 1e-9
        assert abs(sb[i] - host['ssim'][i]) <= 1e-9
    R.check_against(R.golden()[R.key(case, family, y)], ps, ss, y, 'device')


@pytest.mark.parametrize('y', (False, True), ids=('c', 'y'))
def test_batch_row_is_the_one_image_call_and_runs_repeat(M, y):
    B, H, W, C, dtype, order, crop = R.CASES['tiles']
    for family in ('random', 'smooth'):
        a, b = (_dev(t) for t in R.inputs('tiles', family))
        whole = _both(M, a, b, crop, order, y)
        assert _same_bits(whole, _both(M, a, b, crop, order, y))
        for i in range(B):
            one = _both(M, a[i:i + 1], b[i:i + 1], crop, order, y)
            assert _same_bits([t[i:i + 1] for t in whole], one), (family, i)
            assert math.isfinite(float(one[0])) and float(one[1]) == M.calculate_ssim(a[i], b[i], crop, order, y)


@pytest.mark.parametrize('case', ('crop', 'tiles'))
@pytest.mark.parametrize('y', (False, True), ids=('c', 'y'))
def test_crop_through_strides_is_the_contiguous_cropped_copy(M, case, y):
    B, H, W, C, dtype, order, crop = R.CASES[case]
    a, b = (_dev(t) for t in R.inputs(case, 'random'))
    ca, cb = (t[:, crop:-crop, crop:-crop].contiguous() for t in (a, b))
    assert _same_bits(_both(M, a, b, crop, order, y), _both(M, ca, cb, 0, order, y))


@pytest.mark.parametrize('y', (False, True), ids=('c', 'y'))
def test_chw_is_hwc_of_the_permuted_copy(M, y):
    a, b = (_dev(t) for t in R.inputs('chw', 'random'))
    pa, pb = (t.permute(0, 2, 3, 1).contiguous() for t in (a, b))
    assert _same_bits(_both(M, a, b, 0, 'CHW', y), _both(M, pa, pb, 0, 'HWC', y))
    assert _same_bits(_both(M, a, b, 5, 'CHW', y), _both(M, pa, pb, 5, 'HWC', y))


@pytest.mark.parametrize('case', ('crop', 'tiles'))
@pytest.mark.parametrize('y', (False, True), ids=('c', 'y'))
def test_slice_of_a_larger_tensor_is_its_contiguous_copy(M, case, y):
    B, H, W, C, dtype, order, crop = R.CASES[case]
    a, b = (_dev(t) for t in R.inputs(case, 'random'))
    big = torch.full((B + 1, H + 5, W + 7, C), 99, dtype=a.dtype, device='cuda')
    big[1:, 2:2 + H, 3:3 + W] = a
    view = big[1:, 2:2 + H, 3:3 + W]
    assert not view.is_contiguous()
    assert _same_bits(_both(M, view, b, crop, order, y), _both(M, a, b, crop, order, y))
    assert _same_bits(_both(M, b, view, 0, order, y), _both(M, b, a, 0, order, y))


def test_nan_stays_in_its_row(M):
    B, H, W, C, dtype, order, crop = R.CASES['crop']
    a, b = (_dev(t) for t in R.inputs('crop', 'random'))
    for y in (False, True):
        clean = _both(M, a, b, crop, order, y)
        bad = a.clone()
        bad[1, H // 2, W // 2, 1] = float('nan')
        got = _both(M, bad, b, crop, order, y)
        for g, c in zip(got, clean):
            assert math.isnan(float(g[1])) and np.array_equal(_bits(g[:1]), _bits(c[:1]))
        assert math.isnan(M.calculate_psnr(bad[1], b[1], crop, order, y)) and math.isnan(M.calculate_ssim(bad[1], b[1], crop, order, y))


@pytest.mark.parametrize('case', list(R.CASES))
def test_identical_images_give_inf_and_exactly_one(M, case):
    B, H, W, C, dtype, order, crop = R.CASES[case]
    a = _dev(R.inputs(case, 'random')[0])
    for y in (False, True):
        p, s = _both(M, a, a.clone(), crop, order, y)
        assert p.dtype == s.dtype == torch.float64 and p.shape == s.shape == (B,) and p.is_cuda and s.is_cuda
        assert all(v == math.inf for v in p.tolist()) and all(v == 1.0 for v in s.tolist())
        assert M.calculate_psnr(a[0], a[0].clone(), crop, order, y) == math.inf
        assert M.calculate_ssim(a[0], a[0].clone(), crop, order, y) == 1.0


def test_two_dimensional_images(M):
    a, b = R.inputs('one', 'random')
    ga, gb = _dev(a[0, :, :, 0]), _dev(b[0, :, :, 0])
    assert ga.dim() == 2
    assert M.calculate_psnr(ga, gb, 0) == M.calculate_psnr(a[0, :, :, 0], b[0, :, :, 0], 0)
    assert abs(M.calculate_ssim(ga, gb, 0) - M.calculate_ssim(a[0, :, :, 0], b[0, :, :, 0], 0)) <= 1e-9


def test_error_cases(M):
    a = torch.zeros(1, 16, 16, 3, dtype=torch.uint8, device='cuda')
    for fn in (M.psnr_batch, M.ssim_batch):
        with pytest.raises(TypeError):
            fn(a.double(), a.double())
        with pytest.raises(TypeError):
            fn(a.half(), a.half())
        with pytest.raises(TypeError):
            fn(a, a.float())
        with pytest.raises(ValueError):
            fn(a, a.cpu())
        with pytest.raises(ValueError):
            fn(a, a[:, :15])
        with pytest.raises(ValueError):
            fn(a, a, input_order='WHC')
        with pytest.raises(ValueError):
            fn(a[0], a[0])
    for fn in (M.calculate_psnr, M.calculate_ssim):
        with pytest.raises(TypeError):
            fn(a[0].to(torch.int32), a[0].to(torch.int32), 0)
        with pytest.raises(ValueError):
            fn(a[0], a[0].cpu(), 0)
        with pytest.raises(AssertionError):
            fn(a[0], a[0, :15], 0)
        with pytest.raises(ValueError):
            fn(a[0], a[0], 0, input_order='WHC')
    with pytest.raises(ValueError):
        M.ssim_batch(a[:, :10], a[:, :10])
    with pytest.raises(ValueError):
        M.calculate_ssim(a[0], a[0], 3)          # 10x10 after the crop
    with pytest.raises(ValueError):
        M.ssim_batch(a, a, crop_border=3)
    with pytest.raises(ValueError):
        M.psnr_batch(a[..., :2], a[..., :2])     # two channels


def test_restored_face_batch(M):
    """(2,512,512,3) uint8 BGR, the shape CodeFormer.restore_u8 emits, through both batched calls."""
    rng = np.random.default_rng(5)
    yy, xx = np.meshgrid(np.arange(512), np.arange(512), indexing='ij')
    a = np.rint(127.5 + 90 * np.sin(xx / 23.)[None, :, :, None] * np.cos(yy / 17.)[None, :, :, None] + rng.integers(-30, 31, (2, 512, 512, 3)))
    a = np.clip(a, 0, 255).astype(np.uint8)
    b = np.clip(a.astype(np.int64) + rng.integers(-6, 7, a.shape), 0, 255).astype(np.uint8)
    ga, gb = _dev(a), _dev(b)
    wide = torch.zeros(2, 512, 515, 3, dtype=torch.uint8, device='cuda')
    wide[:, :, 1:513] = ga      # rows that start off a 16-byte boundary take scalar loads: the same bits as the 16-byte loads of ga
    for y in (False, True):
        assert _same_bits(_both(M, wide[:, :, 1:513], gb, 0, 'HWC', y), _both(M, ga, gb, 0, 'HWC', y))
        p, s = (t.cpu().tolist() for t in _both(M, ga, gb, 0, 'HWC', y))
        for i in range(2):
            hp, hs = M.calculate_psnr(a[i], b[i], 0, 'HWC', y), M.calculate_ssim(a[i], b[i], 0, 'HWC', y)
            print(f'512x512 image {i} y={y}: |psnr - host| {abs(p[i] - hp):.3e} dB, |ssim - host| {abs(s[i] - hs):.3e}')
            assert abs(p[i] - hp) <= 1e-9 and abs(s[i] - hs) <= 1e-9
