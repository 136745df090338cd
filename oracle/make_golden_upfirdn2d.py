"""Golden vectors of the REFERENCE's upfirdn2d_native (basicsr/ops/upfirdn2d/upfirdn2d.py:156-186), the only pure-torch
restatement the reference itself ships, evaluated in the build container on seeded inputs.

    python -m oracle.make_golden_upfirdn2d        # writes tests/golden/upfirdn2d_native.npz

Inputs: x = seeded_randn((2, 3, 9, 7), 6), k = seeded_randn((4, 4), 7); one output per (up, down, pad) case of CASES, stored as
`out_<i>`.  TEST INFRASTRUCTURE ONLY.
"""
import os

import numpy as np
import torch

from . import ref_loader
from .synth import seeded_randn

GOLD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden')
CASES = ((1, 1, (1, 2)), (2, 1, (2, 1)), (1, 2, (1, 1)), (2, 2, (0, 3)), (1, 1, (-1, 2)))


def main():
    if not ref_loader.available():
        raise SystemExit(f'reference not found under {ref_loader.REF}')
    src = open(os.path.join(ref_loader.REF, 'basicsr/ops/upfirdn2d/upfirdn2d.py')).read()
    ns = {'F': torch.nn.functional, 'torch': torch}
    exec(compile(src[src.index('def upfirdn2d_native'):], 'upfirdn2d_native', 'exec'), ns)
    x = seeded_randn((2, 3, 9, 7), 6)
    k = seeded_randn((4, 4), 7)
    out = {}
    for i, (up, down, pad) in enumerate(CASES):
        out[f'out_{i}'] = ns['upfirdn2d_native'](x, k, up, up, down, down, pad[0], pad[1], pad[0], pad[1]).numpy()
    path = os.path.join(GOLD, 'upfirdn2d_native.npz')
    np.savez_compressed(path, **out)
    print(path, {n: a.shape for n, a in out.items()})


if __name__ == '__main__':
    main()
