#!/usr/bin/env python
"""Time VGGFeatureExtractor and the perceptual / style score on the GPU, and measure the opt-in F(4x4,3x3) route.

Workload: 16 pairs of 512x512x3 uint8 on vgg19, taps conv1_2 conv2_2 conv3_4 conv4_4 conv5_4 (the layers of the reference's training options).
  extractor                 the 32 images through the HIP path (features_nhwc) and through forward_host (stock torch ops) on the same device
  extractor off-grid        the same at 500x500, a size off the Winograd grid: the general fp32 kernel everywhere, wide layers in 128-channel parts
  perceptual_batch          HIP path, beside the same definition in stock torch ops (forward_host, a float64 mean of |d|)
  perceptual_batch style    the same on Gram matrices (stock: torch.bmm)
  launch table              every launch of one perceptual_batch(style=True) call, bracketed by device events (medians per launch)
  cf_gram alone             against torch.bmm at (c, hw) = (64, 512^2) and (512, 32^2), 32 images
  --f43                     extractor time with net.winograd_f43 = True, and the accuracy of both routes on the 'grid' case of tests/vgg_ref.py
                            and on a 256x256 vgg19 case: e(x) = max|x - ref64| / max|ref64| against forward_host in float64 on the CPU, over
                            e(forward_host in float32 on the CPU)

  python tools/vgg_bench.py --f43 > profiles/vgg_bench.txt

Run it as its own process; warm-up calls first, then `--reps` windows of `--inner` calls timed with device events; medians and quartiles per
call, one JSON line per entry.  Weights are a seeded random initialisation (no trained VGG checkpoint exists here): times do not depend on them."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

TAPS = ('conv1_2', 'conv2_2', 'conv3_4', 'conv4_4', 'conv5_4')


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


def launch_table(ops, fn, reps):
    """Medians (ms) per launch of `fn`: every ops.* entry point the VGG path uses is bracketed by device events for `reps` calls."""
    names = ('vgg_input', 'conv2d', 'relu', 'relu_maxpool2', 'gram', 'feat_dist')
    saved = {n: getattr(ops, n) for n in names}
    log = []

    def wrap(name, f):
        def g(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = f(*a, **k)
            e1.record()
            t = a[0]
            log.append((name, list(t.shape), e0, e1))
            return out
        return g
    runs = []
    try:
        for n in names:
            setattr(ops, n, wrap(n, saved[n]))
        for _ in range(reps):
            log.clear()
            fn()
            torch.cuda.synchronize()
            runs.append([(n, s, e0.elapsed_time(e1)) for n, s, e0, e1 in log])
    finally:
        for n in names:
            setattr(ops, n, saved[n])
    rows = []
    for i, (n, s, _) in enumerate(runs[0]):
        ts = sorted(r[i][2] for r in runs)
        rows.append({'launch': i, 'op': n, 'first_arg_shape': s, 'median_ms': round(ts[len(ts) // 2], 5)})
    return rows


def accuracy(R, what, net, x):
    """e(device) / e(float32 forward_host) per tap, for the default route and for winograd_f43, against float64 forward_host on the CPU."""
    import copy
    import numpy as np
    with torch.no_grad():
        f32 = net.forward_host(x)
        f64 = copy.deepcopy(net).double().forward_host(x.double())
    dev = net.cuda()
    for f43 in (False, True):
        dev.winograd_f43 = f43
        out = dev(x.cuda())
        for k in out:
            e_dev, e_ref = R.rel_err(out[k].cpu().numpy(), f64[k].numpy()), R.rel_err(f32[k].numpy(), f64[k].numpy())
            print(json.dumps({'entry': 'accuracy', 'case': what, 'tap': k, 'winograd_f43': f43, 'e_device': float(np.float32(e_dev)),
                              'e_float32_host': float(np.float32(e_ref)), 'ratio': round(e_dev / e_ref, 3)}), flush=True)
    dev.winograd_f43 = False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--inner', type=int, default=3)
    ap.add_argument('--f43', action='store_true', help='also measure the winograd_f43 route (time and accuracy)')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('vgg_bench: no GPU -- nothing is measured without one')
    from codeformer_amd import losses, metrics, ops
    from codeformer_amd.archs import vgg_arch as A
    B, S = a.batch, a.size
    dev = torch.cuda.get_device_name(0)

    def report(entry, fn, inner=None, **extra):
        med, q1, q3 = timed(fn, a.warmup, a.reps, inner or a.inner)
        print(json.dumps({'entry': entry, 'median_ms': round(med, 4), 'q1_ms': round(q1, 4), 'q3_ms': round(q3, 4), **extra, 'reps': a.reps, 'device': dev}), flush=True)
        return med

    torch.manual_seed(0)
    net = metrics.load_vgg(layer_weights={k: 1.0 for k in TAPS}, device='cuda')
    gen = torch.Generator(device='cuda').manual_seed(0)
    x = torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, device='cuda', generator=gen)
    z = (x.long() + torch.randint(-12, 13, x.shape, device='cuda', generator=gen)).clamp(0, 255).to(torch.uint8)

    def stock_nchw(t):
        return (t.flip(3).float() / 255.).permute(0, 3, 1, 2)

    def stock_score(style):
        fa, fb = net.vgg.forward_host(stock_nchw(x)), net.vgg.forward_host(stock_nchw(z))
        total = 0
        for k in fa:
            ta, tb = (losses.gram_host(f) if style else f for f in (fa[k], fb[k]))
            total = total + (ta - tb).double().abs().reshape(B, -1).mean(1) * net.layer_weights[k]
        return total

    with torch.no_grad():
        xf = torch.cat([stock_nchw(x), stock_nchw(z)], 0).contiguous()
        tag = dict(images=2 * B, shape=[2 * B, 3, S, S], taps=list(TAPS))
        report('extractor', lambda: net.vgg.features_nhwc(xf), impl='hip', **tag)
        report('extractor', lambda: net.vgg.forward_host(xf), impl='stock_torch', inner=1, **tag)
        if a.f43:
            net.vgg.winograd_f43 = True
            report('extractor', lambda: net.vgg.features_nhwc(xf), impl='hip, winograd_f43', **tag)
            net.vgg.winograd_f43 = False
        # a size off the Winograd grid: every layer on the general kernel, layers of more than 128 input channels in parts (_conv)
        off = a.size - 12
        xo = xf[:, :, :off, :off].contiguous()
        tag = dict(images=2 * B, shape=[2 * B, 3, off, off], taps=list(TAPS))
        report('extractor off-grid', lambda: net.vgg.features_nhwc(xo), impl='hip', **tag)
        report('extractor off-grid', lambda: net.vgg.forward_host(xo), impl='stock_torch', inner=1, **tag)
        del xo
        for style in (False, True):
            hip, stock = metrics.perceptual_batch(x, z, net, style=style), stock_score(style)
            rel = float(((hip - stock).abs() / stock.abs()).max())
            report('perceptual_batch' + (' style' if style else ''), lambda: metrics.perceptual_batch(x, z, net, style=style), impl='hip', pairs=B,
                   max_rel_hip_minus_stock=rel)
            report('perceptual_batch' + (' style' if style else ''), lambda: stock_score(style), impl='stock_torch', pairs=B, inner=1)
        for row in launch_table(ops, lambda: metrics.perceptual_batch(x, z, net, style=True), 7):
            print(json.dumps({'entry': 'launch', **row}), flush=True)
        for c, hw in ((64, 512 * 512), (512, 32 * 32)):
            f = torch.randn(2 * B, hw, c, device='cuda', generator=gen)
            ft = f.transpose(1, 2).contiguous()
            flops = 2.0 * 2 * B * c * c * hw
            for impl, fn in (('cf_gram', lambda: ops.gram(f)), ('torch.bmm', lambda: ft.bmm(ft.transpose(1, 2)) / (c * hw))):
                med = report('gram', fn, impl=impl, shape=[2 * B, hw, c])
                print(json.dumps({'entry': 'gram rate', 'impl': impl, 'c': c, 'hw': hw, 'tflops_full_matrix': round(flops / med / 1e9, 2)}), flush=True)
    if a.f43:
        import vgg_ref as R
        accuracy(R, 'grid', R.build(A.VGGFeatureExtractor, 'grid'), R.case_input('grid'))
        import numpy as np
        big = R.fill_state(A.VGGFeatureExtractor(list(TAPS) + ['relu5_4'], 'vgg19'), 44)
        accuracy(R, 'vgg19 256x256', big, torch.from_numpy(np.random.default_rng(45).uniform(0., 1., (1, 3, 256, 256)).astype(np.float32)))


if __name__ == '__main__':
    main()
