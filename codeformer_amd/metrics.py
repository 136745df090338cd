"""PSNR and SSIM of images and image batches (the reference's basicsr/metrics/psnr_ssim.py:9-128 and metric_util.py:6-45).

Two paths, one definition (it also stands at "quality metrics" in include/codeformer_hip.h):
  host    numpy arrays and CPU tensors: the reference's arithmetic in float64, written out without cv2.
  device  CUDA (ROCm) tensors, uint8 or float32: the HIP kernels of csrc/cf_metrics.hip through ops.psnr / ops.ssim.  Crop and order are
          expressed through strides, nothing is copied, and there is no other path for a GPU tensor.

Preparation of both images: reorder_image ((h,w) -> (h,w,1); 'CHW' -> HWC), crop_border pixels off every side, and with test_y_channel a
3-channel image is BGR and becomes one channel in the reference's float32 rounding (to_y_channel below); everything after that is float64.
PSNR: sse = sum (a-b)^2 over pixels and channels, mse = sse / N, inf when mse == 0, else 20 log10(255 / sqrt(mse)).  (The reference's Y path
falls into float32 because its to_y_channel returns float32; here it stays in float64, which moves the result by less than 1e-5 dB.)
SSIM: the window g[i] = exp(-(i-5)^2 / (2 1.5^2)) / sum = cv2.getGaussianKernel(11, 1.5), applied along the rows and then the columns, valid
region only (the reference's [5:-5, 5:-5]); C1 = (0.01 255)^2, C2 = (0.03 255)^2; the mean of
((2 mu1 mu2 + C1)(2 s12 + C2)) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2)) per channel, then the mean over channels.
Deviation: an image smaller than 11x11 after the crop raises ValueError (the reference returns the NaN of an empty mean).

calculate_psnr / calculate_ssim keep the reference's positional signature and return a Python float; psnr_batch / ssim_batch are new,
device-only, and return a (B,) float64 tensor on the device without a synchronisation.

Identity preservation, the third full-reference score of face restoration: the cosine similarity of the ArcFace embeddings
(archs/arcface_arch.py ResNetArcFace) of the restored face and the ground truth.  identity_input is the image front end, stated as a
definition ("ArcFace / identity metric" in include/codeformer_hip.h): RGB in [-1, 1], gray = 0.2989 R + 0.5870 G + 0.1140 B, then a bilinear
resize to 128 x 128 with half-pixel centres, edge clamp and no antialiasing -- gray first, resize second, every step one float32 operation,
so the host definition (torch ops on the CPU) and the kernel give the same bits.  identity_batch / calculate_identity / load_arcface
follow; no trained ArcFace checkpoint ships with or was run through this code.

A perceptual score: perceptual_batch / calculate_perceptual give, per image pair, sum_k w_k criterion(f_k(a), f_k(b)) over the VGG layers of a
losses.PerceptualLoss (load_vgg builds one), or the same on the Gram matrices (style).  No trained VGG checkpoint ships with or was run
through this code either.
"""
import numpy as np
import torch

from .utils.registry import METRIC_REGISTRY

__all__ = ['calculate_psnr', 'calculate_ssim', 'psnr_batch', 'ssim_batch', 'reorder_image', 'to_y_channel', 'identity_input', 'identity_batch',
           'calculate_identity', 'load_arcface', 'perceptual_batch', 'calculate_perceptual', 'load_vgg', 'lpips_batch', 'load_lpips_vgg']

ORDERS = ('HWC', 'CHW')
C1 = (0.01 * 255)**2
C2 = (0.03 * 255)**2


def _check_order(input_order):
    if input_order not in ORDERS:
        raise ValueError(f'Wrong input_order {input_order}. Supported input_orders are "HWC" and "CHW"')


def reorder_image(img, input_order='HWC'):
    """(h,w) -> (h,w,1); (c,h,w) with 'CHW' -> (h,w,c); (h,w,c) as it is."""
    _check_order(input_order)
    if len(img.shape) == 2:
        img = img[..., None]
    if input_order == 'CHW':
        img = img.transpose(1, 2, 0)
    return img


def to_y_channel(img):
    """The Y of YCbCr (BT.601) of a BGR image with values in [0, 255], float32 and not rounded to integers; a 1-channel image only takes
    the float32 round trip.  Every step is one operation: f = float32(v) / float32(255); d = ((f_b 24.966 + f_g 128.553) + f_r 65.481) + 16
    in float64; Y = float32(float32(d / 255) * float32(255))."""
    f = img.astype(np.float32) / np.float32(255.)
    if f.ndim == 3 and f.shape[2] == 3:
        d = f.astype(np.float64)
        d = ((d[..., 0] * 24.966 + d[..., 1] * 128.553) + d[..., 2] * 65.481) + 16.0
        f = (d / 255.).astype(np.float32)[..., None]
    return f * np.float32(255.)


def _prepare(img, crop_border, input_order, test_y_channel):
    img = reorder_image(img, input_order=input_order).astype(np.float64)
    if crop_border != 0:
        img = img[crop_border:-crop_border, crop_border:-crop_border, ...]
    if test_y_channel:
        img = to_y_channel(img).astype(np.float64)
    return img


def _psnr_of_sse(sse, count):
    mse = sse / count
    if mse == 0:
        return float('inf')
    return float(20. * np.log10(255. / np.sqrt(mse)))


def gaussian_window():
    g = np.exp(-(np.arange(11, dtype=np.float64) - 5.)**2 / (2 * 1.5**2))
    return g / g.sum()


def _filter_valid(img, g):
    """The separable window over the valid region of a (h,w) float64 plane: along the rows, then along the columns, taps in ascending order."""
    h, w = img.shape
    rows = np.zeros((h, w - 10))
    for k in range(11):
        rows += g[k] * img[:, k:k + w - 10]
    out = np.zeros((h - 10, w - 10))
    for k in range(11):
        out += g[k] * rows[k:k + h - 10]
    return out


def _ssim_plane(img1, img2):
    g = gaussian_window()
    mu1, mu2 = _filter_valid(img1, g), _filter_valid(img2, g)
    mu1_sq, mu2_sq, mu1_mu2 = mu1**2, mu2**2, mu1 * mu2
    sigma1_sq = _filter_valid(img1**2, g) - mu1_sq
    sigma2_sq = _filter_valid(img2**2, g) - mu2_sq
    sigma12 = _filter_valid(img1 * img2, g) - mu1_mu2
    ssim_map = ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))
    return ssim_map.mean()


def _host_pair(img1, img2):
    """numpy arrays of both images when the host path applies (arrays, CPU tensors); None for two device tensors."""
    t1, t2 = torch.is_tensor(img1), torch.is_tensor(img2)
    if t1 and t2 and (img1.is_cuda or img2.is_cuda):
        if img1.device != img2.device:
            raise ValueError(f'the images lie on different devices ({img1.device}, {img2.device})')
        return None
    if (t1 and img1.is_cuda) or (t2 and img2.is_cuda):
        raise ValueError('one image is a device tensor and the other is not')
    return tuple(t.detach().numpy() if torch.is_tensor(t) else np.asarray(t) for t in (img1, img2))


def _device_view(t, crop_border, input_order):
    """(1,H,W,C) or (B,H,W,C) view of a device tensor: the order through a permutation, the crop through a slice -- strides only."""
    if t.dtype not in (torch.uint8, torch.float32):
        raise TypeError(f'device metrics take uint8 or float32 tensors, got {t.dtype}')
    t = t.detach()
    if t.dim() == 2:
        t = t[None, :, :, None]
    elif t.dim() == 3:
        t = (t.permute(1, 2, 0) if input_order == 'CHW' else t)[None]
    elif t.dim() == 4:
        t = t.permute(0, 2, 3, 1) if input_order == 'CHW' else t
    else:
        raise ValueError(f'an image is (h,w), (h,w,c) or (c,h,w) and a batch 4-D, got {tuple(t.shape)}')
    c = int(crop_border)
    if c != 0:
        t = t[:, c:-c, c:-c]
    if min(t.shape) < 1:
        raise ValueError(f'nothing is left of the image after crop_border {crop_border}')
    return t


@METRIC_REGISTRY.register()
def calculate_psnr(img1, img2, crop_border, input_order='HWC', test_y_channel=False):
    """PSNR of two images with values in [0, 255]: numpy arrays / CPU tensors on the host, uint8 or float32 CUDA tensors ((h,w), (h,w,c) or
    (c,h,w)) through the HIP kernel.  crop_border pixels on every side take no part; test_y_channel scores the Y channel of a BGR image.
    A Python float.  The device path reads back the squared-error sum and applies the host path's expression: for uint8 colour inputs the
    sum is exact and the result has the host path's bits."""
    assert img1.shape == img2.shape, (f'Image shapes are differnet: {img1.shape}, {img2.shape}.')
    _check_order(input_order)
    pair = _host_pair(img1, img2)
    if pair is None:
        from . import ops
        a, b = (_device_view(t, crop_border, input_order) for t in (img1, img2))
        if img1.dim() == 4:
            raise ValueError('calculate_psnr takes one image pair (psnr_batch takes batches)')
        sse, _ = ops.psnr(a, b, test_y_channel)
        _, H, W, C = a.shape
        return _psnr_of_sse(float(sse.item()), H * W * (1 if test_y_channel else C))
    img1, img2 = (_prepare(i, crop_border, input_order, test_y_channel) for i in pair)
    d = img1 - img2
    return _psnr_of_sse(float(np.sum(d * d)), d.size)


@METRIC_REGISTRY.register()
def calculate_ssim(img1, img2, crop_border, input_order='HWC', test_y_channel=False):
    """SSIM of two images with values in [0, 255] (per channel, then averaged); the arguments of calculate_psnr.  A Python float."""
    assert img1.shape == img2.shape, (f'Image shapes are differnet: {img1.shape}, {img2.shape}.')
    _check_order(input_order)
    pair = _host_pair(img1, img2)
    if pair is None:
        from . import ops
        a, b = (_device_view(t, crop_border, input_order) for t in (img1, img2))
        if img1.dim() == 4:
            raise ValueError('calculate_ssim takes one image pair (ssim_batch takes batches)')
        return float(ops.ssim(a, b, test_y_channel).item())
    img1, img2 = (_prepare(i, crop_border, input_order, test_y_channel) for i in pair)
    if img1.shape[0] < 11 or img1.shape[1] < 11:
        raise ValueError(f'the image ({img1.shape[0]}x{img1.shape[1]} after the crop) is smaller than the 11x11 window')
    return float(np.array([_ssim_plane(img1[..., i], img2[..., i]) for i in range(img1.shape[2])]).mean())


def _batch_views(a, b, crop_border, input_order):
    _check_order(input_order)
    if not (torch.is_tensor(a) and torch.is_tensor(b) and a.is_cuda and b.is_cuda):
        raise ValueError('psnr_batch / ssim_batch take CUDA (ROCm) tensors; calculate_psnr / calculate_ssim score host images')
    if a.device != b.device:
        raise ValueError(f'the batches lie on different devices ({a.device}, {b.device})')
    if a.dim() != 4 or tuple(a.shape) != tuple(b.shape):
        raise ValueError(f'two 4-D batches of one shape are needed, got {tuple(a.shape)} and {tuple(b.shape)}')
    return _device_view(a, crop_border, input_order), _device_view(b, crop_border, input_order)


def psnr_batch(a, b, crop_border=0, input_order='HWC', test_y_channel=False):
    """PSNR of every image pair of two device batches -- (B,H,W,C) for 'HWC', (B,C,H,W) for 'CHW', uint8 or float32 with values in
    [0, 255], any strides -- as a (B,) float64 tensor on the device, without a synchronisation.  (B,512,512,3) uint8 BGR is what
    CodeFormer.restore_u8 returns."""
    from . import ops
    return ops.psnr(*_batch_views(a, b, crop_border, input_order), test_y_channel)[1]


def ssim_batch(a, b, crop_border=0, input_order='HWC', test_y_channel=False):
    """SSIM of every image pair of two device batches; the arguments and the result of psnr_batch."""
    from . import ops
    return ops.ssim(*_batch_views(a, b, crop_border, input_order), test_y_channel)


# ---- identity preservation ----------------------------------------------------------------------------------------------------------------
ID_SIZE = 128
GRAY = (0.2989, 0.5870, 0.1140)


def _identity_view(img, order, what='identity_input'):
    """(B,H,W,3) view of a tensor: uint8 BGR or float32 RGB in [0, 1], one image or a batch, 'HWC' or 'CHW' -- strides only."""
    _check_order(order)
    if img.dtype not in (torch.uint8, torch.float32):
        raise TypeError(f'{what} takes uint8 (BGR) or float32 (RGB in [0, 1]) images, got {img.dtype}')
    t = img.detach()
    if t.dim() == 3:
        t = t[None]
    if t.dim() != 4:
        raise ValueError(f'an image is (h,w,3) or (3,h,w) and a batch 4-D, got {tuple(img.shape)}')
    if order == 'CHW':
        t = t.permute(0, 2, 3, 1)
    if t.shape[3] != 3 or min(t.shape) < 1:
        raise ValueError(f'{what} needs 3-channel images, got {tuple(img.shape)} with order {order}')
    return t


def _axis_host(n):
    """Source indices and weights of the 128 output positions along an axis of n pixels: src = (o + 0.5) * (n / 128) - 0.5, clamped at 0."""
    o = torch.arange(ID_SIZE, dtype=torch.float32)
    scale = torch.tensor(float(n), dtype=torch.float32) / torch.tensor(float(ID_SIZE), dtype=torch.float32)
    src = (o + 0.5) * scale
    src = (src - 0.5).clamp_min(0.)
    f = torch.floor(src)
    lo = src - f
    i0 = f.long().clamp(0, n - 1)
    return i0, (i0 + 1).clamp_max(n - 1), lo, 1.0 - lo


def identity_gray_host(t):
    """(B,H,W,3) CPU view -> (B,H,W) float32 gray of the RGB image in [-1, 1]."""
    f = t.to(torch.float32) / torch.tensor(255., dtype=torch.float32) if t.dtype == torch.uint8 else t
    v = f * 2.0
    v = v - 1.0
    r, g, b = (v[..., 2], v[..., 1], v[..., 0]) if t.dtype == torch.uint8 else (v[..., 0], v[..., 1], v[..., 2])
    return (GRAY[0] * r + GRAY[1] * g) + GRAY[2] * b


def _identity_input_host(t):
    gray = identity_gray_host(t)
    y0, y1, ly, hy = _axis_host(t.shape[1])
    x0, x1, lx, hx = _axis_host(t.shape[2])
    top, bot = gray[:, y0], gray[:, y1]
    top = hx * top[:, :, x0] + lx * top[:, :, x1]
    bot = hx * bot[:, :, x0] + lx * bot[:, :, x1]
    return (hy[:, None] * top + ly[:, None] * bot)[:, None].contiguous()


def identity_input(img, order='HWC'):
    """The input of the identity network, (B,1,128,128) float32, from uint8 BGR images ((B,H,W,3): what CodeFormer.restore_u8 returns) or
    float32 RGB images in [0, 1] ((B,H,W,3), or (B,3,H,W) with order 'CHW'); one image gives B = 1.  CUDA tensors go through one HIP launch
    that reads the image through its strides (a crop or a slice needs no copy); numpy arrays and CPU tensors take the host definition, whose
    bits the kernel reproduces."""
    if not torch.is_tensor(img):
        img = torch.from_numpy(np.ascontiguousarray(img))
    t = _identity_view(img, order)
    if t.is_cuda:
        from . import ops
        return ops.identity_input(t, bgr=t.dtype == torch.uint8)
    return _identity_input_host(t)


def _cosine_host(x, y):
    x, y = x.double(), y.double()
    den = (x.norm(dim=1) * y.norm(dim=1)).clamp_min(1e-8)
    return (x * y).sum(dim=1) / den


def identity_batch(a, b, net, order='HWC'):
    """Identity preservation of every image pair of two batches: cosine(net(identity_input(a)), net(identity_input(b))) as a (B,) float64
    tensor on the inputs' device, the cosine x.y / max(|x| |y|, 1e-8) taken in float64 from the float32 embeddings.  On the device nothing
    is copied to the host and nothing synchronises; both batches pass the network in one call (row r of a batch is bitwise the call on r alone)."""
    xa, xb = identity_input(a, order), identity_input(b, order)
    if xa.shape != xb.shape or xa.device != xb.device:
        raise ValueError(f'two batches of one size on one device are needed, got {tuple(xa.shape)} on {xa.device} and {tuple(xb.shape)} on {xb.device}')
    n = xa.shape[0]
    with torch.no_grad():
        e = net(torch.cat([xa, xb], 0))
    if e.is_cuda:
        from . import ops
        return ops.cosine_rows(e[:n], e[n:])
    return _cosine_host(e[:n], e[n:])


@METRIC_REGISTRY.register()
def calculate_identity(img1, img2, net, input_order='HWC'):
    """Identity preservation of one image pair ((h,w,3) or (3,h,w); uint8 BGR or float32 RGB in [0, 1]) under the embedding network `net`
    (load_arcface).  numpy arrays and CPU tensors take the host path, CUDA tensors the HIP path.  A Python float."""
    for i in (img1, img2):
        if len(i.shape) != 3:
            raise ValueError('calculate_identity takes one image pair (identity_batch takes batches)')
    return float(identity_batch(img1, img2, net, input_order)[0].item())


def load_arcface(path=None, device=None):
    """ResNetArcFace('IRBlock', [2, 2, 2, 2], use_se=False) in eval mode -- the configuration identity scoring uses -- with the checkpoint at
    `path` loaded if one is given ('params_ema' / 'params' wrappers and a leading 'module.' of the keys are removed).  Nothing is
    downloaded: a missing file raises FileNotFoundError.  Without a path the weights are the seeded-by-the-caller random initialisation."""
    import os
    from .archs.arcface_arch import ResNetArcFace
    net = ResNetArcFace('IRBlock', [2, 2, 2, 2], use_se=False)
    if path is not None:
        if not os.path.isfile(path):
            raise FileNotFoundError(f'ArcFace checkpoint {path} not found (nothing is downloaded)')
        state = torch.load(path, map_location='cpu', weights_only=True)
        for k in ('params_ema', 'params'):
            if isinstance(state, dict) and k in state:
                state = state[k]
                break
        net.load_state_dict({(k[7:] if k.startswith('module.') else k): v for k, v in state.items()}, strict=True)
    net.eval()
    return net.to(device) if device is not None else net


# ---- perceptual / style score -------------------------------------------------------------------------------------------------------------
def perceptual_batch(a, b, net, order='HWC', criterion='l1', style=False):
    """The perceptual distance of every image pair of two batches under `net`, a losses.PerceptualLoss (load_vgg): per image
    sum_k w_k mean|f_k(a) - f_k(b)| over its layer_weights ('mse': the mean square, 'fro': the Frobenius norm, every image as a batch of
    one), with style=True the same on the Gram matrices F F^T / (c h w).  Its vgg_type and norm flags apply; perceptual_weight and
    style_weight do not.  Inputs as for identity_batch: uint8 BGR (B,H,W,3) -- what CodeFormer.restore_u8 returns -- or float32 RGB in
    [0, 1], 'HWC' or 'CHW', read through their strides.  A (B,) float64 tensor on the inputs' device; on the device both batches pass the
    network in one call (row r is bitwise the call on r alone), nothing is copied to the host and nothing synchronises."""
    from .losses import CRITERIA, gram_host, reduce_dist
    if criterion not in CRITERIA:
        raise NotImplementedError(f'{criterion} criterion has not been supported.')
    ta, tb = (t if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t)) for t in (a, b))
    va, vb = _identity_view(ta, order, 'perceptual_batch'), _identity_view(tb, order, 'perceptual_batch')
    if va.shape != vb.shape or va.device != vb.device or va.dtype != vb.dtype:
        raise ValueError(f'two batches of one size and type on one device are needed, got {va.dtype} {tuple(va.shape)} on {va.device} and {vb.dtype} {tuple(vb.shape)} on {vb.device}')
    bgr = va.dtype == torch.uint8
    if va.is_cuda:
        from . import ops
        ops.L.ensure_device(va.device)
        with torch.no_grad(), torch.cuda.device(va.device):
            return net.score(net.features([va, vb], bgr), style=style, criterion=criterion, per_image=True)
    with torch.no_grad():
        n = va.shape[0]
        x = torch.cat([va, vb], 0)
        x = x.to(torch.float32) / torch.tensor(255., dtype=torch.float32) if bgr else x
        x = (x.flip(3) if bgr else x).permute(0, 3, 1, 2)
        total = torch.zeros(n, dtype=torch.float64)
        for k, f in net.vgg.forward_host(x).items():
            t = gram_host(f) if style else f
            d = (t[:n] - t[n:]).double().reshape(n, -1)
            total = total + reduce_dist(torch.stack([d.abs().sum(1), (d * d).sum(1)], 1), d.shape[1], criterion, True) * float(net.layer_weights[k])
        return total


@METRIC_REGISTRY.register()
def calculate_perceptual(img1, img2, net, input_order='HWC', criterion='l1', style=False):
    """The perceptual distance of one image pair ((h,w,3) or (3,h,w); uint8 BGR or float32 RGB in [0, 1]) under `net` (load_vgg).  numpy
    arrays and CPU tensors take the host path, CUDA tensors the HIP path.  A Python float."""
    for i in (img1, img2):
        if len(i.shape) != 3:
            raise ValueError('calculate_perceptual takes one image pair (perceptual_batch takes batches)')
    return float(perceptual_batch(img1, img2, net, input_order, criterion, style)[0].item())


VGG_LAYER_WEIGHTS = {'conv1_2': 0.1, 'conv2_2': 0.1, 'conv3_4': 1., 'conv4_4': 1., 'conv5_4': 1.}   # the weights of the reference's training options


def load_vgg(path=None, vgg_type='vgg19', layer_weights=None, use_input_norm=True, range_norm=False, device=None):
    """A losses.PerceptualLoss on `vgg_type` for perceptual_batch, with the torchvision state dict at `path` loaded if one is given
    (`features.<i>.*` by position; `classifier.*` and layers past the last requested one are ignored).  Nothing is downloaded: a missing
    file raises FileNotFoundError.  Without a path the weights are the seeded-by-the-caller random initialisation (or
    vgg_arch.VGG_PRETRAIN_PATH, where that file exists)."""
    import os
    from .archs.vgg_arch import FeaturesOnly
    from .losses import PerceptualLoss
    net = PerceptualLoss(dict(layer_weights or VGG_LAYER_WEIGHTS), vgg_type=vgg_type, use_input_norm=use_input_norm, range_norm=range_norm)
    if path is not None:
        if not os.path.isfile(path):
            raise FileNotFoundError(f'VGG checkpoint {path} not found (nothing is downloaded)')
        full = FeaturesOnly(vgg_type)
        full.load_state_dict(torch.load(path, map_location='cpu', weights_only=True))
        with torch.no_grad():
            for dst, src in zip(net.vgg.names, full.features):
                if dst in net.vgg.vgg_net._modules and list(src.state_dict()):
                    net.vgg.vgg_net._modules[dst].load_state_dict(src.state_dict())
    net.eval()
    return net.to(device) if device is not None else net


# ---- the LPIPS form, by its published definition ---------------------------------------------------------------------------------------------
# The reference trains with LPIPSLoss, a wrapper of the external `lpips` package; that package is not installed, so no fixture of it can exist
# and this is the definition of Zhang et al. 2018 restated: vgg16 taps relu1_2 .. relu5_3 of an image in [-1, 1] behind the scaling layer
# (x - shift) / scale, features divided per pixel by sqrt(sum_c f^2) + 1e-10, squared differences weighted by non-negative `lin` vectors,
# averaged over the pixels, summed over the layers.  No LPIPS weights (neither the VGG nor the lin layers) ship with or were run through this code.
LPIPS_TAPS = ('relu1_2', 'relu2_2', 'relu3_3', 'relu4_3', 'relu5_3')
LPIPS_SHIFT = (-.030, -.088, -.188)
LPIPS_SCALE = (.458, .448, .450)


def load_lpips_vgg(device=None):
    """A vgg16 VGGFeatureExtractor on LPIPS_TAPS whose input normalisation is the LPIPS scaling layer (mean = shift, std = scale; inputs in
    [-1, 1]); weights as for VGGFeatureExtractor (seeded by the caller when no checkpoint file exists).  Nothing is downloaded."""
    from .archs.vgg_arch import VGGFeatureExtractor
    net = VGGFeatureExtractor(list(LPIPS_TAPS), vgg_type='vgg16', use_input_norm=True, range_norm=False)
    with torch.no_grad():
        net.mean.copy_(torch.tensor(LPIPS_SHIFT).view(1, 3, 1, 1))
        net.std.copy_(torch.tensor(LPIPS_SCALE).view(1, 3, 1, 1))
    return net.to(device) if device is not None else net


def lpips_batch(a, b, net, lin, order='HWC'):
    """The LPIPS distance of every image pair of two device batches of float32 RGB images in [-1, 1] ((B,H,W,3), or (B,3,H,W) with 'CHW';
    strides only) under `net` (load_lpips_vgg) and `lin`: one non-negative float32 weight vector per tap of `net`, in tap order.  A (B,)
    float64 tensor on the device: sum over the taps of cf_lpips_head; no copy to the host, no synchronisation.  Device only."""
    va, vb = _identity_view(a, order, 'lpips_batch'), _identity_view(b, order, 'lpips_batch')
    if not va.is_cuda or va.dtype != torch.float32 or vb.dtype != torch.float32:
        raise ValueError('lpips_batch takes float32 CUDA (ROCm) tensors with values in [-1, 1]')
    if va.shape != vb.shape or va.device != vb.device:
        raise ValueError(f'two batches of one size on one device are needed, got {tuple(va.shape)} on {va.device} and {tuple(vb.shape)} on {vb.device}')
    if len(lin) != len(net.layer_name_list):
        raise ValueError(f'lin: one weight vector per tap ({len(net.layer_name_list)}), got {len(lin)}')
    from . import ops
    ops.L.ensure_device(va.device)
    n = va.shape[0]
    with torch.no_grad(), torch.cuda.device(va.device):
        feats = net.features_from_views([va, vb])
        total = 0
        for (k, f), w in zip(feats.items(), lin):
            total = total + ops.lpips_head(f[:n], f[n:], w)
    return total
