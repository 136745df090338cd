"""Record the reference's ResNetArcFace for the cases of tests/arcface_ref.py (build machine only: needs the reference tree).

Writes tests/golden/arcface_ref.npz.  The reference's basicsr/archs/arcface_arch.py is pure PyTorch; it is loaded by path under stub
packages and runs on the CPU:
  keys, shapes         its state_dict key list (sorted) and the shape of every entry, for the 'r18' and the 'se' configuration
  <case>_f32, _f64     its embeddings of the case's input under the seeded state recipe, in float32 and, from the same module in
                       .double(), in float64
  init_r18             per key a sha256 of its default initialisation under torch.manual_seed(0)
  torch_version        the torch version that produced all of it
Inputs and weights are regenerated from seeds by the helper and not stored.  Running it twice gives the same bytes.

  python tools/make_golden_arcface.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import arcface_ref as R  # noqa: E402


def main():
    ref = R.load_reference()
    arrays = {'torch_version': np.array(R.host_id())}
    for case in R.CASES:
        net = R.build(ref.ResNetArcFace, case)
        sd = net.state_dict()
        arrays[f'keys_{case}'] = np.array(sorted(sd))
        arrays[f'shapes_{case}'] = np.array([','.join(str(n) for n in sd[k].shape) for k in sorted(sd)])
        x = R.case_input(case)
        with torch.no_grad():
            arrays[f'{case}_f32'] = net(x).numpy().astype(np.float32)
            arrays[f'{case}_f64'] = net.double()(x.double()).numpy().astype(np.float64)
    torch.manual_seed(0)
    arrays['init_r18'] = R.init_digest(ref.ResNetArcFace('IRBlock', [2, 2, 2, 2], use_se=False))
    # a plain zip with fixed timestamps, so that the same arrays give the same bytes
    import io
    import zipfile
    with zipfile.ZipFile(R.GOLDEN, 'w', zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)
    print(f'{R.GOLDEN}: {os.path.getsize(R.GOLDEN)} bytes')


if __name__ == '__main__':
    main()
