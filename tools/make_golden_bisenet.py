"""Record the reference's BiSeNet for the cases of tests/bisenet_ref.py (build machine only: needs the reference tree).

Writes tests/golden/bisenet_ref.npz.  The reference's facelib/parsing/resnet.py and bisenet.py are loaded by path under a stub package and
run on the CPU under the helper's seeded state recipe:
  keys, shapes                   the state_dict key list (sorted) and the shape of every entry
  <case>_<tap>_f32, _f64         the tap's values at the helper's seeded sample positions, from the module in float32 and in .double(); taps:
                                 the six forward(x, return_feat=True) outputs and ResNet18's three features
  <case>_<tap>_err, _max         full-map scalars max|f32 - f64| and max|f64|
  <case>_labels, <case>_gap      argmax over the classes of the float64 `out` (uint8) and its top-2 gap (float32)
  <case>_gate_band               the share of sigmoid gates inside bisenet_ref.GATE_BAND (asserted >= 30 %)
  torch_version                  the torch version that produced all of it
Inputs, weights and sample positions are regenerated from seeds by the helper and not stored.  Running it twice gives the same bytes.

  python tools/make_golden_bisenet.py
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import bisenet_ref as R  # noqa: E402


def record(cls, arrays=None):
    """The per-case arrays of BiSeNet class `cls` under the recipe (the fixture's, when cls is the reference's)."""
    arrays = {} if arrays is None else arrays
    for case in R.CASES:
        net = R.build(cls, case)
        x = R.case_input(case)
        gates = R.gate_values(net, x)
        band = float(((gates >= R.GATE_BAND[0]) & (gates <= R.GATE_BAND[1])).mean())
        assert band >= 0.30, f'{case}: only {band:.1%} of the sigmoid gates lie in {R.GATE_BAND}: adjust bisenet_ref.GATE_SCALE'
        arrays[f'{case}_gate_band'] = np.array(band)
        f32 = R.run_taps(net, x)
        f64 = R.run_taps(net.double(), x.double())
        for k in R.TAPS:
            a32, a64 = f32[k].numpy(), f64[k].numpy()
            arrays[f'{case}_{k}_f32'] = R.sample(case, k, a32).astype(np.float32)
            arrays[f'{case}_{k}_f64'] = R.sample(case, k, a64).astype(np.float64)
            arrays[f'{case}_{k}_err'] = np.array(np.abs(a32.astype(np.float64) - a64).max())
            arrays[f'{case}_{k}_max'] = np.array(np.abs(a64).max())
        out64 = f64['out'].numpy()
        arrays[f'{case}_labels'] = out64.argmax(1).astype(np.uint8)
        arrays[f'{case}_gap'] = R.top2_gap(out64).astype(np.float32)
        small = float((arrays[f'{case}_gap'] < 16 * arrays[f'{case}_out_err']).mean())
        differ = float((f32['out'].numpy().argmax(1) != out64.argmax(1)).mean())
        print(f'{case}: gates in band {band:.1%}; max|out| {float(arrays[f"{case}_out_max"]):.1f}; pixels with a gap below 16 max|f32 - f64| '
              f'{small:.3%}; float32 and float64 labels differ on {differ:.3%}')
    return arrays


def main():
    _, ref_bisenet = R.load_reference()
    sd = ref_bisenet.BiSeNet(R.NUM_CLASS).state_dict()
    arrays = {'torch_version': np.array(torch.__version__), 'keys': np.array(sorted(sd)),
              'shapes': np.array([','.join(str(n) for n in sd[k].shape) for k in sorted(sd)])}
    record(ref_bisenet.BiSeNet, arrays)
    # a plain zip with fixed timestamps, so that the same arrays give the same bytes
    with zipfile.ZipFile(R.GOLDEN, 'w', zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)
    print(f'{R.GOLDEN}: {os.path.getsize(R.GOLDEN)} bytes')


if __name__ == '__main__':
    main()
