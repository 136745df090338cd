"""RetinaFace-ResNet50 on the two backends, 'hip' (this project's kernels) and 'torch' (stock torch ops through MIOpen), on the same device in the
same run: `forward` at 640x1138 (a 1080p frame reduced to short side 640, as get_face_landmarks_5(resize=640) feeds it) with batch 1 and 4, and
`detect_faces` on a device-resident frame.  The two backends alternate round by round; each figure is the median over the rounds of a window
of `--iters` calls (100: half a second and more) closed by a device synchronise, after every shape has run once.  Outputs of the two are compared at the timed size.
Seeded weights (oracle.make_golden_retinaface): no released detector checkpoint is read.  Needs a ROCm device: without one it fails.

  python tools/detector_hip_bench.py [--rounds 5] [--iters 100] [--json out.json]
With --video N the whole-image rate of tools/video_bench.py (N frames, 3 faces each, detection stage in the loop) is taken per backend in
child processes.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from facelib.detection.retinaface.retinaface import RetinaFace  # noqa: E402
from oracle.make_golden_retinaface import CASES, build, seeded_frames  # noqa: E402

BACKENDS = ('hip', 'torch')


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--video', type=int, default=0, metavar='FRAMES')
    ap.add_argument('--json', type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('detector_hip_bench: no ROCm device (a timing taken anywhere else says nothing)')
    net = build(RetinaFace, CASES['resnet50'], device='cuda')
    frames = seeded_frames((4, 640, 1138, 3), 77)
    x = (torch.from_numpy(frames.astype(np.float32)).permute(0, 3, 1, 2) - torch.tensor([104., 117., 123.]).view(1, 3, 1, 1)).cuda()
    frame = torch.from_numpy(frames[0]).cuda()
    # a threshold that lets a few dozen rows through on these weights: the rows' way to the host, the sort and NMS are inside detect_faces
    with torch.no_grad():
        net.backend = 'torch'
        scores = net(x[:1])[1][0, :, 1]
        thr = float(torch.sort(scores, descending=True).values[40])
    work = {'forward B1': lambda: net(x[:1]), 'forward B4': lambda: net(x),
            'detect_faces': lambda: net.detect_faces(frame, conf_threshold=thr)}
    outs, times = {}, {(w, b): [] for w in work for b in BACKENDS}
    with torch.no_grad():
        for b in BACKENDS:      # warm-up of every shape, and the outputs for the comparison
            net.backend = b
            outs[b] = {w: fn() for w, fn in work.items()}
        for _ in range(args.rounds):
            for b in BACKENDS:
                net.backend = b
                for w, fn in work.items():
                    times[(w, b)].append(window(fn, args.iters))
    diff = {w: max(float((p - q).abs().max()) for p, q in zip(outs['hip'][w], outs['torch'][w])) for w in ('forward B1', 'forward B4')}
    same_rows = outs['hip']['detect_faces'].shape == outs['torch']['detect_faces'].shape
    result = {'device': torch.cuda.get_device_name(0), 'rounds': args.rounds, 'iters': args.iters, 'conf_threshold': thr, 'rows': int(outs['hip']['detect_faces'].shape[0]),
              'max_abs_diff_hip_vs_torch': diff, 'detect_faces_same_row_count': bool(same_rows), 'entries': []}
    print(f'{"entry":<14}{"hip ms":>10}{"torch ms":>10}{"hip fr/s":>10}{"torch fr/s":>11}  spread (min..max ms)')
    for w in work:
        n = 4 if w.endswith('B4') else 1
        med = {b: statistics.median(times[(w, b)]) for b in BACKENDS}
        result['entries'].append({'entry': w, **{f'{b}_ms': med[b] * 1e3 for b in BACKENDS}, **{f'{b}_frames_per_s': n / med[b] for b in BACKENDS},
                                  **{f'{b}_min_max_ms': [min(times[(w, b)]) * 1e3, max(times[(w, b)]) * 1e3] for b in BACKENDS},
                                  'hip_slower': bool(med['hip'] > med['torch'])})
        print(f'{w:<14}{med["hip"] * 1e3:>10.2f}{med["torch"] * 1e3:>10.2f}{n / med["hip"]:>10.1f}{n / med["torch"]:>11.1f}  '
              + ' / '.join(f'{b} {min(times[(w, b)]) * 1e3:.2f}..{max(times[(w, b)]) * 1e3:.2f}' for b in BACKENDS)
              + ('   <- the HIP path is slower' if med['hip'] > med['torch'] else ''), flush=True)
    print(f'max |hip - torch|: {diff}; detect_faces rows {outs["hip"]["detect_faces"].shape[0]} / {outs["torch"]["detect_faces"].shape[0]} at threshold {thr:.4f}')
    if args.video:
        result['video'] = {}
        for b in BACKENDS:      # fresh child processes: this one keeps the GPU open, so they run one after the other
            r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'video_bench.py'), str(args.video), '3', '2', 'cuda', b], capture_output=True, text=True,
                               timeout=900)
            line = (r.stdout.strip().splitlines() or [r.stderr.strip()[-400:]])[-1]
            result['video'][b] = line
            print(f'video_bench, detector backend {b}: {line}', flush=True)
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(result, f, indent=1)


if __name__ == '__main__':
    main()
