"""Record the reference's metric values for the cases of tests/metrics_ref.py (build machine only: needs the reference tree).

Writes tests/golden/metrics_ref.json -- calculate_psnr / calculate_ssim of the reference's basicsr/metrics/psnr_ssim.py for every case x
family x Y flag, image by image -- and tests/golden/matlab_color_ref.npz -- rgb2ycbcr, bgr2ycbcr (also y_only), ycbcr2rgb, ycbcr2bgr of
the reference's pure-numpy basicsr/utils/matlab_functions.py on a 16x16x3 uint8 and a float32 image.  Inputs are regenerated from seeds by
the helper and not stored.

The reference's files are loaded by path under stub packages, with a stub cv2: getGaussianKernel is the window's formula and filter2D a
plain correlation over the valid region.  The fixture therefore pins the reference's cropping, ordering, Y conversion and channel averaging,
NOT OpenCV's filter: cv2 is not available to pin it.

  python tools/make_golden_metrics.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import metrics_ref as R  # noqa: E402


def main():
    ps, _, mat = R.load_reference()
    out = {'_note': 'the reference under a stub cv2 (numpy window and valid-region correlation): pins cropping, ordering, Y conversion and '
                    'channel averaging, not the filter of OpenCV'}
    for case, family, y in R.ALL:
        out[R.key(case, family, y)] = {'psnr': R.per_image(ps.calculate_psnr, case, family, y),
                                       'ssim': R.per_image(ps.calculate_ssim, case, family, y)}
    with open(R.GOLDEN, 'w') as fh:
        json.dump(out, fh, indent=0, sort_keys=True)
        fh.write('\n')
    u8, f32 = R.color_inputs()
    arrays = {}
    for tag, img in (('u8', u8), ('f32', f32)):
        for name in ('rgb2ycbcr', 'bgr2ycbcr', 'ycbcr2rgb', 'ycbcr2bgr'):
            arrays[f'{name}_{tag}'] = getattr(mat, name)(img)
        for name in ('rgb2ycbcr', 'bgr2ycbcr'):
            arrays[f'{name}_y_{tag}'] = getattr(mat, name)(img, y_only=True)
    np.savez_compressed(R.GOLDEN_COLOR, **arrays)
    print(f'{R.GOLDEN}: {os.path.getsize(R.GOLDEN)} bytes; {R.GOLDEN_COLOR}: {os.path.getsize(R.GOLDEN_COLOR)} bytes')


if __name__ == '__main__':
    main()
