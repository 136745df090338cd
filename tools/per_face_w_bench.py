"""What one fidelity weight per face costs and saves, measured on an MI355X (seed-0 weights, seeded faces, adain; wall clock around work that
ends in a device synchronise, the median of --reps repetitions after a warm-up):
  (a) a 16-face step with a scalar w against the same step with a vector of 16 equal values (eager, as bench.py runs it; the forms alternate
      repetition by repetition): the price of the per-image table on the batched path, plus the host's read of the vector;
  (b) eight one-face calls at eight distinct w under graph replay: scalar (each new value warms up and captures a graph, the fifth evicts the
      first, so a second round over the same values captures again) against one-element vectors (one graph for all of them);
  (c) restore_sweep of one face at K = 8 weights against eight scalar one-face calls that each replay a warm graph.
usage (GPU box): python tools/per_face_w_bench.py [--precision f16x2] [--reps 9] [--out FILE]   prints one table, and one JSON line"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WS8 = (0.1, 0.25, 0.4, 0.5, 0.6, 0.75, 0.9, 1.0)


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--precision', default='f16x2', choices=['fp32', 'f16x2', 'bf16', 'fp16'])
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'per_face_w_bench.py needs an MI355X'
    import codeformer_amd.archs  # noqa: F401
    from codeformer_amd.utils.registry import ARCH_REGISTRY
    from oracle.synth import seeded_input
    torch.manual_seed(0)
    net = ARCH_REGISTRY.get('CodeFormer')(dim_embd=512, codebook_size=1024, n_head=8, n_layers=9, connect_list=['32', '64', '128', '256']).eval().cuda()
    net.precision = args.precision
    x16 = seeded_input(16).cuda()
    x1 = x16[:1].contiguous()
    rows = []
    with torch.no_grad():
        # (a)
        net.use_hip_graphs = False
        vec = [0.5] * 16
        vec_dev = torch.full((16,), 0.5, device='cuda')
        forms = (('scalar w = 0.5', 0.5), ('vector, 16 x 0.5 (host list)', vec), ('vector, 16 x 0.5 (device tensor: one read-back)', vec_dev))
        for _, w in forms:      # (warm-up of every form, then the three forms alternate repetition by repetition)
            net(x16, w=w, adain=True)
        torch.cuda.synchronize()
        ts = {label: [] for label, _ in forms}
        for _ in range(args.reps):
            for label, w in forms:
                t0 = time.perf_counter()
                net(x16, w=w, adain=True)
                torch.cuda.synchronize()
                ts[label].append((time.perf_counter() - t0) * 1e3)
        for label, _ in forms:
            rows.append(('a: 16-face step, eager, forms alternating', label, statistics.median(ts[label]), min(ts[label]), max(ts[label])))
        # (b)
        net.use_hip_graphs = 'auto'
        for label, form in (('scalar', lambda w: w), ('one-element vector', lambda w: [w])):
            net._graphs.clear()
            c0 = net.graph_captures

            def eight():
                for w in WS8:
                    net(x1, w=form(w), adain=True)
            first = timed(eight, 1, warm=0)
            n_first = net.graph_captures - c0
            again = timed(eight, args.reps, warm=0)
            n_later = net.graph_captures - c0 - n_first
            rows.append(('b: 8 one-face calls at 8 distinct w, graphs', f'{label}: first round ({n_first} captures)') + first)
            rows.append(('b: 8 one-face calls at 8 distinct w, graphs', f'{label}: later rounds ({n_later} captures in {args.reps} rounds)') + again)
        # (c)
        net._graphs.clear()
        rows.append(('c: one face at K = 8 weights', 'eight scalar one-face calls, one warm graph (w = 0.5 each)') +
                    timed(lambda: [net(x1, w=0.5, adain=True) for _ in WS8], args.reps))
        rows.append(('c: one face at K = 8 weights', 'restore_sweep(x, 8 weights) (eager)') + timed(lambda: net.restore_sweep(x1, WS8, adain=True), args.reps))
        net.use_hip_graphs = False
        rows.append(('c: one face at K = 8 weights', 'eight scalar one-face calls, eager') + timed(lambda: [net(x1, w=w, adain=True) for w in WS8], args.reps))
    lines = [f'precision {args.precision}, {torch.cuda.get_device_name(0)}, median [min .. max] of {args.reps} in ms']
    lines += [f'  {what:46s} {label:78s} {med:9.3f} [{lo:.3f} .. {hi:.3f}]' for what, label, med, lo, hi in rows]
    text = '\n'.join(lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')
    print(text)
    print(json.dumps({'precision': args.precision, 'rows': [{'case': a, 'form': b, 'median_ms': round(m, 3), 'min_ms': round(lo, 3), 'max_ms': round(hi, 3)}
                                                            for a, b, m, lo, hi in rows]}))


if __name__ == '__main__':
    main()
