"""SHA-256 of what every C weight packer writes, case by case: the record that a change to the packers' code left their bits alone.

Per case the weight comes from a seeded CPU torch.Generator (randn * 0.05), the C packer is called directly with the arguments written
out in CASES into a NaN-filled buffer (a word the packer leaves unwritten shows in the digest), and the digests of the input bytes and of
the packed bytes are returned.  tests/golden/pack_digests.json holds the output of this script; tests/test_gpu_pack_digest.py
recomputes it.  The input digest tells a moved RNG stream from a packer failure.

usage: python tools/pack_digest.py > tests/golden/pack_digests.json
"""
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SCALES = (1.0, 2.0 ** 17)   # at 2^0 the lo halves of the small weights are subnormal IEEE halves


def _cases():
    """id -> (weight shape, C packer, its arguments between the weight and the buffer, 32-bit words of the buffer)"""
    c = {}

    def add(name, shape, fn, args, words):
        assert name not in c
        c[name] = (shape, fn, args, words)

    def scaled(name, shape, fn, args, words):   # args: scale -> tuple
        for s, tag in zip(SCALES, ('s0', 's17')):
            add(f'{name}_{tag}', shape, fn, args(s), words)

    # plain fp32 [taps][cin_pad/16][cout_pad][16]: 3x3, 1x1, Linear
    for co, ci, cop, cip in ((64, 32, 64, 32), (3, 32, 32, 32), (96, 24, 128, 32)):
        add(f'plain_3x3_{co}x{ci}', (co, ci, 3, 3), 'cf_pack_conv_weight', (co, ci, 9, cop, cip), 9 * cip * cop)
    add('plain_1x1_64x32', (64, 32, 1, 1), 'cf_pack_conv_weight', (64, 32, 1, 64, 32), 32 * 64)
    add('plain_linear_64x128', (64, 128), 'cf_pack_conv_weight', (64, 128, 1, 64, 128), 128 * 64)
    # bf16 / f16 direct, plain and folded (two values per word); fp32 folded
    for t, pad in (('bf16', (32, 32, 64, 32)), ('f16', (32, 32, 32, 32))):
        for co, ci, cop, cip in ((64, 32, 64, 32), (128, 64, 128, 64), pad):
            add(f'{t}_{co}x{ci}', (co, ci, 3, 3), f'cf_pack_conv_weight_{t}', (co, ci, 9, cop, cip), 9 * cip * cop // 2)
            add(f'up2x_{t}_{co}x{ci}', (co, ci, 3, 3), f'cf_pack_conv_weight_up2x_{t}', (co, ci, cop, cip), 16 * cip * cop // 2)
    for co, ci, cop, cip in ((64, 32, 64, 32), (40, 16, 64, 16)):
        add(f'up2x_fp32_{co}x{ci}', (co, ci, 3, 3), 'cf_pack_conv_weight_up2x', (co, ci, cop, cip), 16 * cip * cop)
    # split-half direct: form 0 plain 3x3, 1 folded, 2 stride 2, 3 1x1
    for form, slabs in enumerate((9, 16, 16, 1)):
        shapes = [(64, 32, 64, 32), (128, 64, 128, 64)] + ([(64, 16, 64, 16)] if form == 2 else []) + ([(40, 24, 64, 32)] if form < 2 else [])
        for co, ci, cop, cip in shapes:
            scaled(f'split_form{form}_{co}x{ci}', (co, ci) if form == 3 else (co, ci, 3, 3), 'cf_pack_conv_weight_f16x2',
                   lambda s, a=(co, ci, form, cop, cip): (*a, s), slabs * cip * cop)
    for n, k in ((64, 128), (128, 256)):
        scaled(f'linear_split_{n}x{k}', (n, k), 'cf_pack_linear_weight_f16x2', lambda s, a=(n, k): (*a, s), n * k)
    # Winograd domain: F(2,3) 16 positions, F(4,3) 36 (each slab form of the default mode), F(4,2) sub-pixel 4 x 25
    for co, ci, cop, cip in ((64, 32, 64, 32), (128, 48, 128, 48), (40, 24, 64, 32)):
        a = (co, ci, cop, cip)
        add(f'f23_fp32_{co}x{ci}', (co, ci, 3, 3), 'cf_pack_conv_weight_winograd', a, 16 * cip * cop)
        scaled(f'f23_split_{co}x{ci}', (co, ci, 3, 3), 'cf_pack_conv_weight_winograd_f16x2', lambda s, a=a: (*a, s), 16 * cip * cop)
        scaled(f'f23_bf16_{co}x{ci}', (co, ci, 3, 3), 'cf_pack_conv_weight_winograd_bf16', lambda s, a=a: (*a, s), 16 * cip * cop)
    for co, ci, cop, cip in ((64, 32, 64, 32), (128, 32, 128, 32), (128, 48, 128, 48), (40, 24, 64, 32)):
        a = (co, ci, cop, cip)
        add(f'f43_fp32_{co}x{ci}', (co, ci, 3, 3), 'cf_pack_conv_weight_winograd43', a, 36 * cip * cop)
        scaled(f'f43_split_{co}x{ci}', (co, ci, 3, 3), 'cf_pack_conv_weight_winograd43_f16x2', lambda s, a=a: (*a, s), 36 * cip * cop)
    for co, ci in ((128, 32), (128, 64)):
        add(f'f42_up_{co}x{ci}', (co, ci, 3, 3), 'cf_pack_conv_weight_winograd42_up', (co, ci, co, ci), 100 * ci * co)
    return c


CASES = _cases()


def digest(name):
    """(sha256 of the weight's bytes, sha256 of the packed bytes) of case `name`."""
    from codeformer_amd import lib as L
    shape, fn, args, words = CASES[name]
    g = torch.Generator().manual_seed(int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], 'little'))   # (a new case moves no other's)
    w = torch.randn(shape, generator=g) * 0.05
    wd = w.cuda()
    buf = torch.full((words,), float('nan'), dtype=torch.float32, device='cuda')
    L.check(getattr(L.load(), fn)(L.ptr(wd), *args, L.ptr(buf), L.stream_ptr()), fn)
    torch.cuda.synchronize()
    return hashlib.sha256(w.numpy().tobytes()).hexdigest(), hashlib.sha256(buf.cpu().numpy().tobytes()).hexdigest()


if __name__ == '__main__':
    print(json.dumps({name: dict(zip(('input', 'packed'), digest(name))) for name in sorted(CASES)}, indent=1))
