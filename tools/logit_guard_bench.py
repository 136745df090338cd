"""Price list of the logit guard (CodeFormer.logit_guard) on an MI355X: ms per forward call for the modes off / report / rerun,
16 faces and 1 face per call, precision 'f16x2' and 'fp32', on the seeded bench input and on the real-crop goldens; the flagged share
and `index_changes` (tokens of re-run faces whose code index differs between the F(4x4,3x3) and the F(2x2,3x3) encoder pass).

  python tools/logit_guard_bench.py [--steps 10] [--warmup 3]

'rerun @0' is 'rerun' with threshold 0: nothing is flagged, so it prices the read-back of the B minima alone.  Times are wall clock
around `steps` synchronised calls (median), seed-0 random-init weights, w=0.5, adain."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, 'tests', 'golden')
REAL = ('real_0143.npz', 'real_0342.npz', 'real_Solvay_conference_1927_0018.npz')


def build_net(device):
    import codeformer_amd.archs  # noqa: F401
    from codeformer_amd.utils.registry import ARCH_REGISTRY
    torch.manual_seed(0)
    return ARCH_REGISTRY.get('CodeFormer')(dim_embd=512, codebook_size=1024, n_head=8, n_layers=9,
                                           connect_list=['32', '64', '128', '256']).eval().to(device)


def inputs(device):
    """name -> (16, 3, 512, 512): the bench's seeded faces, and the three real crops of the goldens repeated to 16 faces."""
    from codeformer_amd import ops
    from oracle.synth import seeded_input
    crops = torch.from_numpy(np.stack([np.load(os.path.join(GOLD, n))['img'] for n in REAL])).to(device)
    real = ops.img_u8_to_tensor(crops)
    return {'seeded': seeded_input(16).to(device), 'real crops': real[[i % len(REAL) for i in range(16)]].contiguous()}


def timed(net, x, steps, warmup):
    for _ in range(warmup):
        net(x, w=0.5, adain=True)
    torch.cuda.synchronize()
    net.reset_guard_stats()
    ms = []
    for _ in range(steps):
        t = time.perf_counter()
        net(x, w=0.5, adain=True)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ms), net.guard_stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    net = build_net(dev)
    default_gap = net.logit_guard_gap
    data = inputs(dev)
    print('| input | faces/call | precision | mode | ms/call | vs off | flagged | re-run | index changes | smallest gap |')
    print('|---|---|---|---|---|---|---|---|---|---|')
    for name, x16 in data.items():
        for B in (16, 1):
            # one face per call: the face with the smallest gap of the set, so that 'rerun' prices a flagged call
            net.logit_guard, net.precision = 'report', 'f16x2'
            net(x16, w=0.5, adain=True, code_only=True)
            x = x16 if B == 16 else x16[int(net.last_min_gap.argmin()):][:1].contiguous()
            for precision in ('f16x2', 'fp32'):
                net.precision = precision
                base = None
                for mode, gap in (('off', default_gap), ('report', default_gap), ('rerun', 0.0), ('rerun', default_gap)):
                    net.logit_guard, net.logit_guard_gap = mode, gap
                    ms, st = timed(net, x, args.steps, args.warmup)
                    base = ms if mode == 'off' else base
                    calls = max(st['calls'], 1)
                    label = mode + (' @0' if mode == 'rerun' and gap == 0.0 else '')
                    print(f"| {name} | {B} | {precision} | {label} | {ms:.3f} | {ms - base:+.3f} | {st['flagged'] / calls:g} | "
                          f"{st['rerun_faces'] / calls:g} | {st['index_changes'] / calls:g} | {st['min_gap']:.3g} |", flush=True)
    net.logit_guard, net.logit_guard_gap = 'off', default_gap


if __name__ == '__main__':
    main()
