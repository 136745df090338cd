"""Record the reference's RetinaFace-ResNet50 forward for the cases of tests/retinaface_hip_ref.py (build machine only: needs the reference tree).

Writes tests/golden/retinaface_hip_ref.npz.  The reference's facelib/detection/retinaface classes are loaded by oracle.ref_loader and run on
the CPU under oracle.ref_loader.torchvision_stub with the seeded weights of oracle.make_golden_retinaface.build:
  <case>_loc32, _conf32, _ldm32   the module's own float32 forward (bbox regressions, softmax, landmark regressions)
  <case>_loc64, _conf64, _ldm64   the same module in .double() on the same input
  <case>_priors                   PriorBox of the case's image size (float32)
  flow_thr, flow_gap              for the case retinaface_hip_ref.FLOW_CASE: the middle and the width of the widest gap between neighbouring float64
                                  scores in retinaface_hip_ref.SCORE_BAND
  flow_rows<i>, flow_margin       image i's float64 detection rows at that threshold (retinaface_hip_ref.flow64 on the float64 forward, decode of
                                  the reference's retinaface_utils checked against it here) and the smallest |IoU - nms| over all candidate pairs
  torch_version                   the torch version that produced all of it
Only arrays go into the file; inputs and weights are regenerated from seeds.  Running it twice gives the same bytes.

  python tools/make_golden_retinaface_hip.py
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import retinaface_hip_ref as R  # noqa: E402
from oracle import ref_loader  # noqa: E402


def main():
    torch.set_num_threads(os.cpu_count())
    rf, _, utils = ref_loader.load_reference_retinaface()
    arrays = {'torch_version': np.array(torch.__version__)}
    with ref_loader.torchvision_stub():
        net = R.build(rf.RetinaFace)
    for case, c in R.CASES.items():
        x = R.case_input(case)
        with torch.no_grad():
            o32 = [t.numpy().copy() for t in net.float()(x)]
            o64 = [t.numpy().copy() for t in net.double()(x.double())]
        net.float()
        for name, a, b in zip(R.OUTS, o32, o64):
            arrays[f'{case}_{name}32'], arrays[f'{case}_{name}64'] = a.astype(np.float32), b.astype(np.float64)
            print(f'{case} {name}: max|f32 - f64| {np.abs(a.astype(np.float64) - b).max():.3e}, max|f64| {np.abs(b).max():.3f}')
        h, w = c['shape'][1:3]
        pri = utils.PriorBox(net.cfg, image_size=(h, w)).forward()
        arrays[f'{case}_priors'] = pri.numpy().astype(np.float32)
        if case == R.FLOW_CASE:
            loc, conf, ldm = o64
            thr, gap = R.pick_threshold(conf[:, :, 1])
            margins = []
            for i in range(loc.shape[0]):
                rows, m = R.flow64(loc[i], conf[i], ldm[i], pri.numpy(), w, h, thr)
                # the helper's decode against the reference's own, both in float64
                ref_boxes = utils.decode(torch.from_numpy(loc[i]), pri.double(), net.cfg['variance']) * torch.tensor([w, h, w, h], dtype=torch.float64)
                mine = R.decode64(loc[i], ldm[i], pri.numpy(), w, h)[0]
                assert np.abs(ref_boxes.numpy() - mine).max() < 1e-9
                arrays[f'flow_rows{i}'] = rows
                margins.append(m)
                print(f'{case} image {i}: {int((conf[i, :, 1] > thr).sum())} candidates, {rows.shape[0]} rows after NMS, IoU margin {m:.3e}')
            arrays['flow_thr'], arrays['flow_gap'], arrays['flow_margin'] = np.array(thr), np.array(gap), np.array(min(margins))
            print(f'{case}: threshold {thr:.6f}, gap {gap:.3e}')
    # a plain zip with fixed timestamps, so that the same arrays give the same bytes
    with zipfile.ZipFile(R.GOLDEN, 'w', zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)
    print(f'{R.GOLDEN}: {os.path.getsize(R.GOLDEN)} bytes')


if __name__ == '__main__':
    main()
