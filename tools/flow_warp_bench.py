"""ops.flow_warp against the reference's own path on the same device, measured on an MI355X with hipEvents (warm-up 3, then --reps timed runs, each
between two events; median [min .. max]).
  workload   x (4, 64, 180, 320) float32 -- the shape of the deformable-convolution timing in the README -- flow uniform in +-4, bilinear, zeros
             padding, align_corners=True; x as NCHW planes and as torch.channels_last
  reference  what basicsr/archs/arch_util.py flow_warp does, through stock torch: mesh grid + flow, two normalisations, a stack, F.grid_sample
  bandwidth  algorithmic bytes -- x once, flow once, out once -- over the time, as a fraction of the 8.0 TB/s HBM3E peak
usage (GPU box): python tools/flow_warp_bench.py [--reps 20] [--out FILE]   prints one table, and one JSON line"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12


def reference_flow_warp(x, flow):
    _, _, h, w = x.shape
    gy, gx = torch.meshgrid(torch.arange(0, h, device=x.device, dtype=x.dtype), torch.arange(0, w, device=x.device, dtype=x.dtype), indexing='ij')
    v = torch.stack((gx, gy), 2) + flow
    grid = torch.stack((2.0 * v[..., 0] / max(w - 1, 1) - 1.0, 2.0 * v[..., 1] / max(h - 1, 1) - 1.0), dim=3)
    return F.grid_sample(x, grid, mode='bilinear', padding_mode='zeros', align_corners=True)


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available() and args.reps >= 10, 'flow_warp_bench.py needs an MI355X and at least 10 timed runs'
    from codeformer_amd import ops
    torch.manual_seed(0)
    x = torch.randn(4, 64, 180, 320, device='cuda')
    flow = (torch.rand(4, 180, 320, 2, device='cuda') * 2 - 1) * 4
    xcl = x.contiguous(memory_format=torch.channels_last)
    nbytes = 4 * (2 * x.numel() + flow.numel())
    rows = []
    with torch.no_grad():
        worst = float((ops.flow_warp(x, flow) - reference_flow_warp(x, flow)).abs().max())
        same = bool(torch.equal(ops.flow_warp(xcl, flow), ops.flow_warp(x, flow)))
        for label, fn in (('ops.flow_warp, NCHW planes', lambda: ops.flow_warp(x, flow)),
                          ('ops.flow_warp, channels_last', lambda: ops.flow_warp(xcl, flow)),
                          ('reference path (torch grid_sample), NCHW', lambda: reference_flow_warp(x, flow)),
                          ('reference path (torch grid_sample), channels_last', lambda: reference_flow_warp(xcl, flow))):
            rows.append((label,) + timed(fn, args.reps))
    lines = [f'flow_warp x (4, 64, 180, 320) fp32, flow +-4, bilinear / zeros / align_corners, {torch.cuda.get_device_name(0)}; '
             f'median [min .. max] of {args.reps} in ms; {nbytes / 1e6:.1f} MB algorithmic',
             f'  max |ops.flow_warp - reference path| = {worst:.3e}; channels_last bitwise the planar result: {same}']
    lines += [f'  {label:52s} {med:8.4f} [{lo:.4f} .. {hi:.4f}]   {nbytes / (med * 1e-3) / 1e12:5.2f} TB/s = {100 * nbytes / (med * 1e-3) / HBM_PEAK:4.1f} % of peak'
              for label, med, lo, hi in rows]
    text = '\n'.join(lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')
    print(text)
    print(json.dumps({'bytes': nbytes, 'max_abs_diff': worst, 'rows': [{'form': a, 'median_ms': round(m, 4), 'min_ms': round(lo, 4), 'max_ms': round(hi, 4),
                                                                        'tbps': round(nbytes / (m * 1e-3) / 1e12, 3)} for a, m, lo, hi in rows]}))


if __name__ == '__main__':
    main()
