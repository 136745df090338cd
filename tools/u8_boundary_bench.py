"""What the uint8 image boundary (cf_conv2d_u8, CodeFormer.restore_u8) costs and saves on an MI355X, each pair measured in the same run:

  1. cf_img_u8_to_tensor + first conv   against the first conv reading the uint8 faces          (16 faces)
  2. last conv + cf_tensor_to_img_u8    against the last conv writing the uint8 faces          (16 faces; fp32- and bf16-tensor input)
  3. the composed path (converter, forward, converter) against restore_u8, 1 and 16 faces per call, precision 'f16x2' and 'fp32'

  python tools/u8_boundary_bench.py [--repeats 30] [--warmup 5] [--items 1,2,3] [--e2e]

Every item is the median of `repeats` event-timed repetitions after `warmup` untimed ones; the two sides of a pair alternate, repetition
by repetition.  The spread given is (max - min) / median over the repetitions.  --e2e also runs tools/e2e_bench.py (256 faces, PNG -> PNG)
in a child process and prints what it reports; the same tool run in a checkout of the parent commit is the other side of that comparison.
Seed-0 random-init weights, w = 0.5, adain.  A run without a GPU fails."""
import argparse
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, 'tests', 'golden')
REAL = ('real_0143.npz', 'real_0342.npz', 'real_Solvay_conference_1927_0018.npz')


def pair(fa, fb, repeats, warmup):
    """Median ms and spread of fa and of fb, alternating."""
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    ms = ([], [])
    for _ in range(repeats):
        for k, f in enumerate((fa, fb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return [(statistics.median(m), (max(m) - min(m)) / statistics.median(m)) for m in ms]


def row(name, a, b):
    print(f'| {name} | {a[0]:.3f} | {a[1] * 100:.0f} % | {b[0]:.3f} | {b[1] * 100:.0f} % | {b[0] / a[0]:.3f} |')
    return a[0], b[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--items', default='1,2,3', help='which of the three items above to run')
    ap.add_argument('--e2e', action='store_true', help='also run tools/e2e_bench.py')
    args = ap.parse_args()
    items = {int(i) for i in args.items.split(',') if i}
    if not torch.cuda.is_available():
        raise SystemExit('u8_boundary_bench needs an MI355X')
    import codeformer_amd.archs  # noqa: F401
    from codeformer_amd import lib, ops
    from codeformer_amd.utils.registry import ARCH_REGISTRY
    print(f'build id {lib.load().cf_build_id().decode()}  {torch.cuda.get_device_name(0)}  repeats {args.repeats} warmup {args.warmup}')
    torch.manual_seed(0)
    net = ARCH_REGISTRY.get('CodeFormer')(dim_embd=512, codebook_size=1024, n_head=8, n_layers=9, connect_list=['32', '64', '128', '256']).eval().cuda()
    crops = torch.from_numpy(np.stack([np.load(os.path.join(GOLD, n))['img'] for n in REAL])).cuda()
    faces16 = crops[[i % len(REAL) for i in range(16)]].contiguous()
    print('| item | two launches / composed, ms | spread | fused / restore_u8, ms | spread | ratio |')
    print('|---|---|---|---|---|---|')

    first, last = net.encoder.blocks[0], net.generator.blocks[-1]
    pw_first, pw_last = first.pw(0), last.pw(0)
    convs = [0.0, 0.0]
    if 1 in items:
        a, b = row('first conv, 16 faces',
                   *pair(lambda: ops.conv2d(ops.img_u8_to_tensor(faces16), pw_first, in_nchw=True, emit_stats=True),
                         lambda: ops.conv2d(None, pw_first, in_nchw=True, emit_stats=True, img_in=faces16), args.repeats, args.warmup))
        convs = [a, b]
    dst = torch.empty(16, 512, 512, 3, dtype=torch.uint8, device='cuda')
    if 2 in items:
        g = torch.Generator().manual_seed(1)
        x = torch.randn(16, 512, 512, 64, generator=g).cuda()
        kw = dict(prologue=ops.PRO_AFFINE, scale=(1 + 0.1 * torch.randn(16, 64, generator=g)).cuda(), shift=(0.1 * torch.randn(16, 64, generator=g)).cuda(),
                  out_nchw=True)
        for name, xin in (('fp32 tensor', x), ('bf16 tensor', x.to(torch.bfloat16))):
            a, b = row(f'last conv, {name}, 16 faces', *pair(lambda: ops.tensor_to_img_u8(ops.conv2d(xin, pw_last, **kw)),
                                                             lambda: ops.conv2d(xin, pw_last, img_out=dst, **kw), args.repeats, args.warmup))
            if name == 'fp32 tensor':
                convs = [convs[0] + a, convs[1] + b]
        del x, xin
    if items >= {1, 2}:
        print(f'both boundary convs with their converters, fp32 tensors: {convs[0]:.3f} ms -> fused {convs[1]:.3f} ms per 16 faces')
    for precision in ('f16x2', 'fp32') if 3 in items else ():
        net.precision = precision
        for B in (1, 16):
            f = faces16[:B].contiguous()
            row(f'network, {precision}, {B} face(s) per call',
                *pair(lambda: ops.tensor_to_img_u8(net(ops.img_u8_to_tensor(f), w=0.5, adain=True)[0]),
                      lambda: net.restore_u8(f, w=0.5, adain=True, out=dst[:B]), args.repeats, args.warmup))
    if args.e2e:
        del net, dst
        torch.cuda.empty_cache()
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'e2e_bench.py'), '256'], capture_output=True, text=True, timeout=600)
        print('tools/e2e_bench.py 256:\n' + (r.stdout.strip() or r.stderr.strip()[-600:]))


if __name__ == '__main__':
    main()
