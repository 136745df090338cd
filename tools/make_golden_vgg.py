"""Record the reference's VGGFeatureExtractor and PerceptualLoss for the cases of tests/vgg_ref.py (build machine only: needs the reference
tree).

Writes tests/golden/vgg_ref.npz.  The reference's basicsr/archs/vgg_arch.py and basicsr/losses/losses.py are loaded by path under stub
packages, with this repository's statement of the `features` stacks standing in for torchvision.models.vgg, and run on the CPU:
  keys_<case>, shapes_<case>     the state_dict key list (sorted) and the shape of every entry
  out_keys_<case>, out_shapes_<case>   the keys of the forward result in its order, and their shapes
  <case>_<tap>_f32, _f64         the tap's values at the helper's seeded sample positions, from the module in float32 and in .double()
  loss_<case>_<criterion>_f32, _f64   (percep, style) of PerceptualLoss with perceptual_weight = style_weight = 1
  names_<type>[_bn], pretrain_path   NAMES, insert_bn(NAMES[type]) and VGG_PRETRAIN_PATH of the reference
  torch_version                  the torch version that produced all of it
Inputs, weights and sample positions are regenerated from seeds by the helper and not stored.  Running it twice gives the same bytes.

  python tools/make_golden_vgg.py
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import vgg_ref as R  # noqa: E402


def main():
    ref_arch, ref_losses = R.load_reference()
    arrays = {'torch_version': np.array(torch.__version__)}
    for t, names in ref_arch.NAMES.items():
        arrays[f'names_{t}'] = np.array(names)
        arrays[f'names_{t}_bn'] = np.array(ref_arch.insert_bn(names))
    arrays['pretrain_path'] = np.array(ref_arch.VGG_PRETRAIN_PATH)
    for case, c in R.CASES.items():
        net = R.build(ref_arch.VGGFeatureExtractor, case)
        sd = net.state_dict()
        arrays[f'keys_{case}'] = np.array(sorted(sd))
        arrays[f'shapes_{case}'] = np.array([','.join(str(n) for n in sd[k].shape) for k in sorted(sd)])
        x = R.case_input(case)
        with torch.no_grad():
            f32 = net(x)
            f64 = net.double()(x.double())
        arrays[f'out_keys_{case}'] = np.array(list(f32))
        arrays[f'out_shapes_{case}'] = np.array([','.join(str(n) for n in f32[k].shape) for k in f32])
        for k in f32:
            arrays[f'{case}_{k}_f32'] = R.sample(case, k, f32[k]).astype(np.float32)
            arrays[f'{case}_{k}_f64'] = R.sample(case, k, f64[k]).astype(np.float64)
    for case in R.LOSS_CASES:
        x, gt = R.case_input(case), R.case_input(case, 1)
        for crit in R.CRITERIA:
            net = R.build_loss(ref_losses.PerceptualLoss, case, crit)
            with torch.no_grad():
                arrays[f'loss_{case}_{crit}_f32'] = np.array([float(v) for v in net(x, gt)], dtype=np.float32)
                arrays[f'loss_{case}_{crit}_f64'] = np.array([float(v) for v in net.double()(x.double(), gt.double())], dtype=np.float64)
    # a plain zip with fixed timestamps, so that the same arrays give the same bytes
    with zipfile.ZipFile(R.GOLDEN, 'w', zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)
    print(f'{R.GOLDEN}: {os.path.getsize(R.GOLDEN)} bytes')


if __name__ == '__main__':
    main()
