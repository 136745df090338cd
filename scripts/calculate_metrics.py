"""PSNR and SSIM (and, with --identity, identity preservation; with --perceptual, a VGG feature distance) of a directory of restored images against their ground truth.

  python scripts/calculate_metrics.py --restored DIR --gt DIR [--crop_border N] [--test_y_channel] [--batch 16] [--json OUT]
                                      [--identity (--arcface_weights PATH | --random_init_seed N)]
                                      [--perceptual [--vgg_weights PATH] [--vgg_layers NAME=W ...]]

PNGs are paired by file name and read as uint8 BGR (img_util.imread_bgr).  On a GPU, images of one size are scored in device batches
(metrics.psnr_batch / ssim_batch: the HIP kernels); without one the host definition runs image by image.  One line per file, then the
means.  A file without a partner in the other directory and a pair of different sizes are errors that name the file.
--identity adds the cosine similarity of the ArcFace embeddings of both images (metrics.identity_batch, scored in the same device batches;
whole images, crop_border does not apply).  The network's weights come from --arcface_weights (a ResNetArcFace 'IRBlock' [2,2,2,2]
checkpoint; nothing is downloaded), or, for plumbing only, from a random initialisation seeded by --random_init_seed: such a column means
nothing about identity.
--perceptual adds the L1 distance of the vgg19 features of both images (metrics.perceptual_batch; whole images), over the layers and
weights of --vgg_layers (default conv1_2=0.1 conv2_2=0.1 conv3_4=1 conv4_4=1 conv5_4=1).  The weights come from --vgg_weights (a torchvision
vgg19 state dict; nothing is downloaded); without it the network keeps a random initialisation (seeded by --random_init_seed, else 0), and the
column is plumbing only.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from basicsr.metrics import (calculate_identity, calculate_perceptual, calculate_psnr, calculate_ssim, identity_batch, load_arcface, load_vgg,  # noqa: E402
                             perceptual_batch)
from basicsr.metrics.psnr_ssim import psnr_batch, ssim_batch  # noqa: E402
from basicsr.utils.img_util import imread_bgr  # noqa: E402


def _pngs(d):
    if not os.path.isdir(d):
        raise SystemExit(f'error: {d} is not a directory')
    return sorted(f for f in os.listdir(d) if f.lower().endswith('.png'))


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--restored', required=True)
    p.add_argument('--gt', required=True)
    p.add_argument('--crop_border', type=int, default=0)
    p.add_argument('--test_y_channel', action='store_true')
    p.add_argument('--batch', type=int, default=16, help='images per device batch')
    p.add_argument('--json', default=None, help='also write the per-file values and the means here')
    p.add_argument('--identity', action='store_true', help='add the ArcFace identity column')
    p.add_argument('--arcface_weights', default=None, help='ResNetArcFace checkpoint for --identity')
    p.add_argument('--random_init_seed', type=int, default=None, help='--identity on a seeded random initialisation (plumbing only)')
    p.add_argument('--perceptual', action='store_true', help='add the VGG perceptual-distance column')
    p.add_argument('--vgg_weights', default=None, help='torchvision vgg19 state dict for --perceptual')
    p.add_argument('--vgg_layers', nargs='+', default=None, metavar='NAME=W', help='layers and weights of --perceptual')
    args = p.parse_args(argv)
    net = vgg = None
    if args.perceptual:
        try:
            layers = None if args.vgg_layers is None else {k: float(v) for k, v in (item.split('=', 1) for item in args.vgg_layers)}
        except ValueError:
            raise SystemExit('error: --vgg_layers takes NAME=WEIGHT items, e.g. conv5_4=1')
        if args.vgg_weights is None:
            torch.manual_seed(0 if args.random_init_seed is None else args.random_init_seed)
        vgg = load_vgg(args.vgg_weights, layer_weights=layers, device='cuda' if torch.cuda.is_available() else None)
    if args.identity:
        if (args.arcface_weights is None) == (args.random_init_seed is None):
            raise SystemExit('error: --identity needs exactly one of --arcface_weights PATH and --random_init_seed N')
        if args.random_init_seed is not None:
            torch.manual_seed(args.random_init_seed)
        net = load_arcface(args.arcface_weights, 'cuda' if torch.cuda.is_available() else None)
    names, gt = _pngs(args.restored), set(_pngs(args.gt))
    for n in names:
        if n not in gt:
            raise SystemExit(f'error: {n} has no ground truth in {args.gt}')
    for n in sorted(gt - set(names)):
        raise SystemExit(f'error: {n} has no restored image in {args.restored}')
    if not names:
        raise SystemExit(f'error: no PNG files in {args.restored}')
    pairs = []
    for n in names:
        a, b = imread_bgr(os.path.join(args.restored, n)), imread_bgr(os.path.join(args.gt, n))
        if a.shape != b.shape:
            raise SystemExit(f'error: {n}: restored is {a.shape[1]}x{a.shape[0]}, ground truth {b.shape[1]}x{b.shape[0]}')
        pairs.append((n, a, b))
    opt = dict(crop_border=args.crop_border, input_order='HWC', test_y_channel=args.test_y_channel)
    result = {}
    if torch.cuda.is_available():
        by_size = {}
        for item in pairs:
            by_size.setdefault(item[1].shape, []).append(item)
        for group in by_size.values():
            for i in range(0, len(group), max(1, args.batch)):
                chunk = group[i:i + max(1, args.batch)]
                a = torch.from_numpy(np.stack([c[1] for c in chunk])).cuda()
                b = torch.from_numpy(np.stack([c[2] for c in chunk])).cuda()
                ps, ss = psnr_batch(a, b, **opt).tolist(), ssim_batch(a, b, **opt).tolist()
                ids = identity_batch(a, b, net).tolist() if net is not None else [None] * len(chunk)
                pcs = perceptual_batch(a, b, vgg).tolist() if vgg is not None else [None] * len(chunk)
                for (n, _, _), pv, sv, iv, cv in zip(chunk, ps, ss, ids, pcs):
                    result[n] = {'psnr': pv, 'ssim': sv, **({} if iv is None else {'identity': iv}), **({} if cv is None else {'perceptual': cv})}
    else:
        for n, a, b in pairs:
            result[n] = {'psnr': calculate_psnr(a, b, **opt), 'ssim': calculate_ssim(a, b, **opt)}
            if net is not None:
                result[n]['identity'] = calculate_identity(a, b, net)
            if vgg is not None:
                result[n]['perceptual'] = calculate_perceptual(a, b, vgg)
    keys = ('psnr', 'ssim') + (('identity',) if net is not None else ()) + (('perceptual',) if vgg is not None else ())
    ident = lambda v: (f'\tIDENTITY {v["identity"]:.6f}' if net is not None else '') + (f'\tPERCEPTUAL {v["perceptual"]:.6f}' if vgg is not None else '')  # noqa: E731
    for n in names:
        print(f'{n}\tPSNR {result[n]["psnr"]:.6f} dB\tSSIM {result[n]["ssim"]:.6f}' + ident(result[n]))
    mean = {k: float(np.mean([result[n][k] for n in names])) for k in keys}
    print(f'mean of {len(names)}\tPSNR {mean["psnr"]:.6f} dB\tSSIM {mean["ssim"]:.6f}' + ident(mean))
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump({'files': result, 'mean': mean, 'crop_border': args.crop_border, 'test_y_channel': args.test_y_channel}, fh, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
