#!/usr/bin/env python
"""Time BiSeNet on the GPU against its own forward_host (stock torch ops) on the same device.

Workload: 16 faces of 512x512, float32 in [-1, 1], BiSeNet(19) under the seeded state recipe of tests/bisenet_ref.py.
  forward          (out, out16, out32) through the HIP path and through forward_host
  parse_labels     the `out` head and the argmax inside the resize kernel, beside forward_host(x)[0].argmax(1)
  stem + pool      cf_stem7x7s2 + cf_maxpool3s2 alone, beside conv 7x7 / BatchNorm / ReLU / max_pool2d in stock torch ops
  launch table     every launch of one forward, bracketed by device events (medians per launch)
  labels           the share of pixels on which the two paths' labels differ (both are float32 evaluations of near-ties)

  python tools/bisenet_bench.py > profiles/bisenet_bench.txt

Run it as its own process; warm-up calls first, then `--reps` windows of `--inner` calls timed with device events; medians and quartiles per
call, one JSON line per entry.  Weights are seeded random ones (no trained parsing_bisenet.pth exists here): times do not depend on them."""
import argparse
import json
import os
import sys

import torch
from torch.nn import functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

OPS = ('stem7x7s2', 'maxpool3s2', 'conv2d', 'relu', 'se_pool', 'se_gate', 'pooled_fc', 'scale_add_row', 'se_scale_res_prelu', 'resize_bilinear_ac',
       'resize_bilinear_ac_argmax')


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
    """Medians (ms) per launch of `fn`: every ops.* entry point the BiSeNet path uses is bracketed by device events for `reps` calls."""
    saved = {n: getattr(ops, n) for n in OPS}
    log = []

    def wrap(name, f):
        def g(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = f(*a, **k)
            e1.record()
            log.append((name, list(a[0].shape), e0, e1))
            return out
        return g
    runs = []
    try:
        for n in OPS:
            setattr(ops, n, wrap(n, saved[n]))
        for _ in range(reps):
            log.clear()
            fn()
            torch.cuda.synchronize()
            runs.append([(n, s, e0.elapsed_time(e1)) for n, s, e0, e1 in log])
    finally:
        for n in OPS:
            setattr(ops, n, saved[n])
    rows = []
    for i, (n, s, _) in enumerate(runs[0]):
        ts = sorted(r[i][2] for r in runs)
        rows.append({'launch': i, 'op': n, 'first_arg_shape': s, 'median_ms': round(ts[len(ts) // 2], 5)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--inner', type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bisenet_bench: no GPU -- nothing is measured without one')
    import bisenet_ref as R
    from codeformer_amd import ops
    from codeformer_amd.facelib.parsing.bisenet import BiSeNet
    B, S = a.batch, a.size
    dev = torch.cuda.get_device_name(0)

    def report(entry, fn, inner=None, **extra):
        med, q1, q3 = timed(fn, a.warmup, a.reps, inner or a.inner)
        print(json.dumps({'entry': entry, 'median_ms': round(med, 4), 'q1_ms': round(q1, 4), 'q3_ms': round(q3, 4), **extra, 'reps': a.reps, 'device': dev}), flush=True)
        return med

    net = R.fill_state(BiSeNet(R.NUM_CLASS), 1).eval().cuda()
    res = net.cp.resnet
    x = torch.rand((B, 3, S, S), device='cuda', generator=torch.Generator(device='cuda').manual_seed(0)) * 2 - 1
    tag = dict(shape=[B, 3, S, S])
    with torch.no_grad():
        report('forward', lambda: net(x), impl='hip', **tag)
        report('forward', lambda: net.forward_host(x), impl='stock_torch', inner=1, **tag)
        report('parse_labels', lambda: net.parse_labels(x), impl='hip', **tag)
        report('parse_labels', lambda: net.forward_host(x)[0].argmax(1), impl='stock_torch', inner=1, **tag)
        report('stem + pool', lambda: ops.maxpool3s2(res.stem_hip(x)), impl='hip', **tag)
        report('stem + pool', lambda: res.maxpool(F.relu(res.bn1(res.conv1(x)))), impl='stock_torch', inner=1, **tag)
        for row in launch_table(ops, lambda: net(x), 7):
            print(json.dumps({'entry': 'launch', **row}), flush=True)
        differ = float((net.parse_labels(x) != net.forward_host(x)[0].argmax(1)).float().mean())
        print(json.dumps({'entry': 'labels', 'share_of_pixels_hip_differs_from_stock_torch': differ}), flush=True)


if __name__ == '__main__':
    main()
