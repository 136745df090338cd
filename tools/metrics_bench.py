#!/usr/bin/env python
"""Time metrics.psnr_batch and metrics.ssim_batch on the GPU, colour and Y channel, beside the same definition written in stock torch ops on
the same device (float64 F.conv2d with the separable window for SSIM, an elementwise float64 expression for PSNR).

Run it as its own process (`python tools/metrics_bench.py`): warm-up calls first, then `--reps` windows of `--inner` calls each, timed with
device events; the median, the quartiles (per call), the algorithmic bytes (both images read once) over the median and that rate as a share of
the measured 6.29 TB/s copy rate are printed as one JSON line per entry, with the largest difference between the two formulations."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_RATE = 6.29e12   # bytes/s: the copy rate measured on this chip (profiles/NOTES.md)


def timed(fn, warmup, reps, inner):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / inner)
    ms.sort()
    return ms[len(ms) // 2], ms[len(ms) // 4], ms[3 * len(ms) // 4]


def torch_planes(t, y):
    """(B,H,W,3) uint8 BGR -> (B,P,H,W) float64 planes of the definition, in stock torch ops."""
    if not y:
        return t.permute(0, 3, 1, 2).double()
    f = (t.float() / 255.0).double()
    d = ((f[..., 0] * 24.966 + f[..., 1] * 128.553) + f[..., 2] * 65.481) + 16.0
    return ((d / 255.0).float() * 255.0).double()[:, None]


def torch_psnr(a, b, y):
    d = torch_planes(a, y) - torch_planes(b, y)
    return 20.0 * torch.log10(255.0 / torch.sqrt((d * d).mean(dim=(1, 2, 3))))


def torch_ssim(a, b, y, g):
    x, z = torch_planes(a, y), torch_planes(b, y)
    B, P, H, W = x.shape
    planes = torch.stack((x, z, x * x, z * z, x * z), 2).reshape(B * P * 5, 1, H, W)
    f = F.conv2d(F.conv2d(planes, g.view(1, 1, 1, 11)), g.view(1, 1, 11, 1)).view(B, P, 5, H - 10, W - 10)
    mu1, mu2 = f[:, :, 0], f[:, :, 1]
    s1, s2, s12 = f[:, :, 2] - mu1 * mu1, f[:, :, 3] - mu2 * mu2, f[:, :, 4] - mu1 * mu2
    c1, c2 = (0.01 * 255)**2, (0.03 * 255)**2
    m = ((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s1 + s2 + c2))
    return m.mean(dim=(2, 3)).mean(dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--inner', type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('metrics_bench: no GPU -- nothing is measured without one')
    from codeformer_amd import metrics
    B, S = a.batch, a.size
    gen = torch.Generator(device='cuda').manual_seed(0)
    x = torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, device='cuda', generator=gen)
    noise = torch.randint(-12, 13, (B, S, S, 3), device='cuda', generator=gen)
    z = (x.long() + noise).clamp(0, 255).to(torch.uint8)
    g = torch.from_numpy(metrics.gaussian_window()).cuda()
    nbytes = 2.0 * B * S * S * 3
    with torch.no_grad():
        for y in (False, True):
            runs = (('psnr_batch', lambda: metrics.psnr_batch(x, z, test_y_channel=y), lambda: torch_psnr(x, z, y)),
                    ('ssim_batch', lambda: metrics.ssim_batch(x, z, test_y_channel=y), lambda: torch_ssim(x, z, y, g)))
            for name, hip, stock in runs:
                diff = float((hip() - stock()).abs().max())
                for impl, fn in (('hip', hip), ('stock_torch_fp64', stock)):
                    med, q1, q3 = timed(fn, a.warmup, a.reps, a.inner if impl == 'hip' else max(1, a.inner // 10))
                    print(json.dumps({'metric': name, 'impl': impl, 'y_channel': y, 'shape': [B, S, S, 3], 'dtype': 'uint8',
                                      'median_ms': round(med, 5), 'q1_ms': round(q1, 5), 'q3_ms': round(q3, 5),
                                      'algorithmic_gb_per_s': round(nbytes / med * 1e-6, 1),
                                      'share_of_copy_rate': round(nbytes / (med * 1e-3) / COPY_RATE, 4), 'max_abs_hip_minus_stock': diff,
                                      'reps': a.reps, 'device': torch.cuda.get_device_name(0)}), flush=True)


if __name__ == '__main__':
    main()
