"""BT.601 colour conversions in Matlab's convention (the reference's basicsr/utils/matlab_functions.py:169-347), host numpy.

rgb2ycbcr / bgr2ycbcr / ycbcr2rgb / ycbcr2bgr follow the reference's dtype rules: a uint8 image in [0, 255] gives a rounded uint8 image, a
float32 image in [0, 1] gives a float32 image in [0, 1], anything else is a TypeError.  The arithmetic: the image as float32 in [0, 1], one
float64 product with the 3x3 matrix, the offset, back to the input's range.  codeformer_amd.metrics scores the Y channel with the same numbers.

`imresize` (Matlab's antialiased bicubic resize, the other function of the reference's module) is not provided.
"""
import numpy as np

__all__ = ['rgb2ycbcr', 'bgr2ycbcr', 'ycbcr2rgb', 'ycbcr2bgr']

# rows: the R, G, B weights of Y, Cb, Cr for an image in [0, 1] and a result in [0, 255]
_TO_YCBCR = np.array([[65.481, 128.553, 24.966], [-37.797, -74.203, 112.0], [112.0, -93.786, -18.214]])
_YCBCR_OFFSET = np.array([16., 128., 128.])
# rows: the Y, Cb, Cr weights of R, G, B
_TO_RGB = np.array([[0.00456621, 0., 0.00625893], [0.00456621, -0.00153632, -0.00318811], [0.00456621, 0.00791071, 0.]])
_RGB_OFFSET = np.array([-222.921, 135.576, -276.836])


def _unit_float32(img):
    """The image as float32 in [0, 1]."""
    if img.dtype == np.float32:
        return img.astype(np.float32)
    if img.dtype == np.uint8:
        return img.astype(np.float32) / np.float32(255.)
    raise TypeError(f'The img type should be np.float32 or np.uint8, but got {img.dtype}')


def _as_input_type(img, dtype):
    """A float image in [0, 255] in the type and range of the input: uint8 rounded, float32 in [0, 1]."""
    if dtype == np.uint8:
        return img.round().astype(np.uint8)
    return (img / 255.).astype(np.float32)


def _to_ycbcr(img, order, y_only):
    f = _unit_float32(img)
    m = _TO_YCBCR[:, order]   # columns in the channel order of the image
    if y_only:
        out = np.dot(f, m[0]) + 16.0
    else:
        out = np.matmul(f, m.T) + _YCBCR_OFFSET
    return _as_input_type(out, img.dtype)


def _from_ycbcr(img, order):
    f = _unit_float32(img) * np.float32(255.)
    out = np.matmul(f, _TO_RGB[order].T) * 255.0 + _RGB_OFFSET[order]
    return _as_input_type(out, img.dtype)


def rgb2ycbcr(img, y_only=False):
    """RGB (h,w,3) -> YCbCr, or the Y plane (h,w) with y_only."""
    return _to_ycbcr(img, [0, 1, 2], y_only)


def bgr2ycbcr(img, y_only=False):
    """BGR (h,w,3) -> YCbCr, or the Y plane (h,w) with y_only."""
    return _to_ycbcr(img, [2, 1, 0], y_only)


def ycbcr2rgb(img):
    """YCbCr (h,w,3) -> RGB."""
    return _from_ycbcr(img, [0, 1, 2])


def ycbcr2bgr(img):
    """YCbCr (h,w,3) -> BGR."""
    return _from_ycbcr(img, [2, 1, 0])
