#!/usr/bin/env python
"""Time the deformable convolution on the GPU: the MFMA route, the general route, and the library's plain fp32 3x3 ops.conv2d of the same
shape as the yardstick (the same contraction without the gather).

Run it as its own process (`python tools/dcn_bench.py`): warm-up launches first, then `--reps` launches timed one by one with device
events; the median, the quartiles and the rate over the algorithmic work 2 * B * Ho * Wo * Cout * Cin/G * kh * kw are printed as one JSON
line per kernel.  The layout conversion of the NCHW input (ops.to_nhwc) is timed on its own line: the MFMA route pays it unless the caller
passes a torch.channels_last tensor, which is what the `mfma` line measures."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return ms[len(ms) // 2], ms[len(ms) // 4], ms[3 * len(ms) // 4]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--channels', type=int, default=64)
    ap.add_argument('--height', type=int, default=180)
    ap.add_argument('--width', type=int, default=320)
    ap.add_argument('--deformable-groups', type=int, default=8)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--reps', type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('dcn_bench: no GPU -- nothing is measured without one')
    from codeformer_amd import ops
    B, C, H, W, DG = a.batch, a.channels, a.height, a.width, a.deformable_groups
    torch.manual_seed(0)
    dev = 'cuda'
    x = torch.randn(B, C, H, W, device=dev)
    xcl = x.contiguous(memory_format=torch.channels_last)
    weight = torch.randn(C, C, 3, 3, device=dev) * (C * 9) ** -0.5
    bias = torch.randn(C, device=dev)
    offset = torch.empty(B, DG * 18, H, W, device=dev).uniform_(-2.5, 2.5)
    mask = torch.sigmoid(torch.randn(B, DG * 9, H, W, device=dev))
    pw = ops.pack_weight(weight, bias)
    xn = ops.to_nhwc(x)
    flops = 2.0 * B * H * W * C * C * 9
    assert ops.deform_conv2d_route(x.shape, weight.shape, 1, DG) == 'mfma'
    runs = (('mfma', lambda: ops.deform_conv2d(xcl, offset, weight, mask, bias, 1, 1, 1, 1, DG, route='mfma')),
            ('general', lambda: ops.deform_conv2d(x, offset, weight, mask, bias, 1, 1, 1, 1, DG, route='general')),
            ('conv2d_fp32_3x3', lambda: ops.conv2d(xn, pw)),
            ('to_nhwc', lambda: ops.to_nhwc(x)))
    with torch.no_grad():
        got = {k: f() for k, f in runs[:2]}
        diff = float((got['mfma'] - got['general']).abs().max())
        for name, fn in runs:
            med, q1, q3 = timed(fn, a.warmup, a.reps)
            print(json.dumps({'kernel': name, 'shape': [B, C, H, W], 'deformable_groups': DG, 'median_ms': round(med, 4), 'q1_ms': round(q1, 4),
                              'q3_ms': round(q3, 4), 'tflops': None if name == 'to_nhwc' else round(flops / med * 1e-9, 2), 'reps': a.reps,
                              'max_abs_mfma_minus_general': diff, 'device': torch.cuda.get_device_name(0)}), flush=True)


if __name__ == '__main__':
    main()
