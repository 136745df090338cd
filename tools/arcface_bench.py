#!/usr/bin/env python
"""Time the identity metric and ResNetArcFace ('IRBlock', [2,2,2,2], no SE: the configuration identity scoring uses) on the GPU.

  identity_batch on 16 pairs of 512x512x3 uint8, beside the same definition in stock torch ops on the same device (the host definition of
    identity_input, the module's forward_host, a float64 cosine);
  one forward at B = 1 and B = 16, HIP path and forward_host;
  fc5 (M = B, K = 32768, N = 512; a 64 MiB weight) on cf_fc_rows and on ops.linear (which takes multiples of 256 rows: the B rows are
    zero-padded to 256), against the floor 64 MiB / 6.3 TB/s;
  every new kernel against its memory floor (algorithmic bytes over 6.3 TB/s);
  every distinct convolution of the network in its ArcFace form (bn0 prologue, PReLU / residual-PReLU epilogue, centre-tap shortcut)
    beside ops.conv2d of the same shape with no prologue and no epilogue.

  python tools/arcface_bench.py > profiles/arcface_bench.txt
Kernel times (profiles/arcface_kernel_trace.txt): run the tool under a kernel trace that writes its statistics as CSV
(`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o arc -- python tools/arcface_bench.py --warmup 2 --reps 3 --inner 3`), then
  python tools/arcface_bench.py --kernel-stats DIR/.../arc_kernel_stats.csv > profiles/arcface_kernel_trace.txt
prints the rows of this library's kernels (calls, average / minimum / maximum ns, all calls of the run pooled: warm-up and timed, every
shape); no GPU is needed for that step.

Run it as its own process; warm-up calls first, then `--reps` windows of `--inner` calls timed with device events; medians and quartiles
per call, one JSON line per entry.  Event windows around eager calls include the host's launch path: an entry of 10 .. 15 us is that path,
not the kernel (a kernel trace of the same process gives the kernel times; profiles/NOTES.md holds both).  Weights are a seeded random initialisation: times do not depend on them."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_RATE = 6.3e12   # bytes/s: the achievable HBM rate VERDICT.md quotes


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


def kernel_stats(path):
    """The rows of this library's kernels in a kernel-trace statistics CSV (columns Name, Calls, AverageNs, MinNs, MaxNs), one JSON line each."""
    import csv
    import re
    with open(path, newline='') as fh:
        for r in csv.DictReader(fh):
            m = re.match(r'(?:void )?\(anonymous namespace\)::(\w+(?:<[^>]*>)?)', r['Name'])   # (torch's own kernels start with at::native)
            if m:
                print(json.dumps({'kernel': m.group(1), 'calls': int(r['Calls']), 'avg_ns': round(float(r['AverageNs'])), 'min_ns': int(r['MinNs']),
                                  'max_ns': int(r['MaxNs'])}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--kernel-stats', metavar='CSV', help='print the library kernels of a kernel-trace statistics CSV and exit')
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--inner', type=int, default=10)
    a = ap.parse_args()
    if a.kernel_stats:
        return kernel_stats(a.kernel_stats)
    if not torch.cuda.is_available():
        raise SystemExit('arcface_bench: no GPU -- nothing is measured without one')
    from codeformer_amd import metrics, ops
    B, S = a.batch, a.size
    dev = torch.cuda.get_device_name(0)

    def report(entry, fn, nbytes=None, inner=None, **extra):
        med, q1, q3 = timed(fn, a.warmup, a.reps, inner or a.inner)
        row = {'entry': entry, 'median_ms': round(med, 5), 'q1_ms': round(q1, 5), 'q3_ms': round(q3, 5), **extra}
        if nbytes is not None:
            floor = nbytes / HBM_RATE * 1e3
            row.update(algorithmic_mib=round(nbytes / 2**20, 2), floor_ms=round(floor, 5), times_floor=round(med / floor, 2))
        row.update(reps=a.reps, device=dev)
        print(json.dumps(row), flush=True)
        return med

    torch.manual_seed(0)
    net = metrics.load_arcface(device='cuda')
    gen = torch.Generator(device='cuda').manual_seed(0)
    x = torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, device='cuda', generator=gen)
    z = (x.long() + torch.randint(-12, 13, x.shape, device='cuda', generator=gen)).clamp(0, 255).to(torch.uint8)

    def stock_input(t):   # the host definition of identity_input, on the device
        gray = metrics.identity_gray_host(t)
        ax = [[v.cuda() for v in metrics._axis_host(n)] for n in t.shape[1:3]]
        (y0, y1, ly, hy), (x0, x1, lx, hx) = ax
        top, bot = gray[:, y0], gray[:, y1]
        top = hx * top[:, :, x0] + lx * top[:, :, x1]
        bot = hx * bot[:, :, x0] + lx * bot[:, :, x1]
        return (hy[:, None] * top + ly[:, None] * bot)[:, None].contiguous()

    def stock_identity():
        e = net.forward_host(torch.cat([stock_input(x), stock_input(z)], 0))
        return metrics._cosine_host(e[:B], e[B:])

    with torch.no_grad():
        diff = float((metrics.identity_batch(x, z, net) - stock_identity()).abs().max())
        report('identity_batch', lambda: metrics.identity_batch(x, z, net), impl='hip', pairs=B, shape=[B, S, S, 3], max_abs_hip_minus_stock=diff)
        report('identity_batch', stock_identity, impl='stock_torch', pairs=B, shape=[B, S, S, 3], inner=max(1, a.inner // 5))
        for b in (1, B):
            g = torch.randn(b, 1, 128, 128, device='cuda', generator=gen)
            report('forward', lambda: net(g), impl='hip', batch=b)
            report('forward', lambda: net.forward_host(g), impl='stock_torch', batch=b, inner=max(1, a.inner // 5))

        # fc5 alone
        K, N = 32768, 512
        w = torch.randn(N, K, device='cuda', generator=gen) / 181.0
        bias = torch.randn(N, device='cuda', generator=gen)
        wp, pw = ops.pack_fc_rows(w), ops.pack_weight(w, bias)
        for b in (1, B):
            rows = torch.randn(b, K, device='cuda', generator=gen)
            padded = torch.zeros(256, K, device='cuda')
            padded[:b] = rows
            err = float((ops.fc_rows(rows, wp, bias) - ops.linear(padded, pw)[:b]).abs().max())
            report('fc5', lambda: ops.fc_rows(rows, wp, bias), nbytes=4.0 * N * K, impl='cf_fc_rows', batch=b, max_abs_minus_linear=err)
            report('fc5', lambda: ops.linear(padded, pw), nbytes=4.0 * N * K, impl='ops.linear, rows zero-padded to 256', batch=b)

        # the other new kernels at the shapes the network gives them (B images)
        t = torch.randn(B, 128, 128, 64, device='cuda', generator=gen)
        report('cf_prelu_maxpool2', lambda: ops.prelu_maxpool2(t, 0.25), nbytes=4.0 * t.numel() * 1.25, shape=list(t.shape))
        report('cf_identity_input', lambda: metrics.identity_input(x), nbytes=float(x.numel()) / 4 + 4.0 * B * 128 * 128, shape=list(x.shape),
               note='x4 reduction: four of sixteen source pixels are read')
        e = torch.randn(2 * B, 512, device='cuda', generator=gen)
        report('cf_cosine_rows', lambda: ops.cosine_rows(e[:B], e[B:]), nbytes=4.0 * e.numel(), shape=[B, 512])
        for hw, c in ((64, 64), (32, 128), (16, 256), (8, 512)):
            t = torch.randn(B, hw, hw, c, device='cuda', generator=gen)
            r = torch.randn(B, hw, hw, c, device='cuda', generator=gen)
            y = torch.rand(B, c, device='cuda', generator=gen)
            w1, b1 = torch.randn(c // 16, c, device='cuda', generator=gen) / c**0.5, torch.randn(c // 16, device='cuda', generator=gen)
            w2, b2 = torch.randn(c, c // 16, device='cuda', generator=gen), torch.randn(c, device='cuda', generator=gen)
            report('cf_se_pool', lambda: ops.se_pool(t), nbytes=4.0 * t.numel(), shape=list(t.shape))
            report('cf_se_gate', lambda: ops.se_gate(y, w1, b1, 0.25, w2, b2), nbytes=4.0 * (2 * w1.numel() + 2 * y.numel()), shape=[B, c])
            report('cf_se_scale_res_prelu', lambda: ops.se_scale_res_prelu(t, y, r, 0.25), nbytes=4.0 * 3 * t.numel(), shape=list(t.shape))

        # the convolutions: ArcFace form beside the plain ops.conv2d of the same shape
        seen = set()
        h = torch.randn(B, 64, 64, 64, device='cuda', generator=gen)   # what the stem hands to layer1
        def packed(blk, which):
            w, b = blk.layer(which)[0]()
            return ops.pack_weight(w.float(), b.float())
        for blk in net._blocks():
            s, tb = blk._pre_tables(B)
            geom = dict(stride=2, pad_lo=1) if blk.stride == 2 else {}
            res = h if blk.downsample is None else ops.conv2d(h, packed(blk, 'shortcut'), **geom)
            mid = ops.conv2d(h, packed(blk, 'conv1'), prologue=ops.PRO_AFFINE, scale=s, shift=tb, epilogue=ops.EPI_PRELU, sft_w=0.25)
            layers = [('conv1: bn0 prologue, PReLU epilogue', h, packed(blk, 'conv1'), dict(prologue=ops.PRO_AFFINE, scale=s, shift=tb, epilogue=ops.EPI_PRELU, sft_w=0.25), {}),
                      ('conv2: residual + PReLU epilogue', mid, packed(blk, 'conv2'), dict(epilogue=ops.EPI_RES_PRELU, res=res, sft_w=0.25), geom)]
            if blk.downsample is not None:
                layers.append(('shortcut: 1x1 as the centre tap of a 3x3', h, packed(blk, 'shortcut'), {}, geom))
            for what, inp, pw_, fused, g2 in layers:
                key = (what, tuple(inp.shape), pw_.cout, blk.stride)
                if key not in seen:
                    seen.add(key)
                    tag = dict(shape=list(inp.shape), cout=pw_.cout, stride=blk.stride if g2 else 1)
                    report(what, lambda: ops.conv2d(inp, pw_, **fused, **g2), impl='arcface form', **tag)
                    if fused:
                        report(what, lambda: ops.conv2d(inp, pw_, **g2), impl='ops.conv2d, no prologue / epilogue', **tag)
            h = ops.conv2d(mid, packed(blk, 'conv2'), epilogue=ops.EPI_RES_PRELU, res=res, sft_w=0.25, **geom)


if __name__ == '__main__':
    main()
