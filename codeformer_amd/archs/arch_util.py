"""The reference's basicsr/archs/arch_util.py on this library: the helpers every BasicSR architecture file imports -- weight
initialisation, `make_layer`, the EDSR-style blocks, `flow_warp` / `resize_flow`, `pixel_unshuffle`, `DCNv2Pack` and the tuple helpers --
with the reference's names, signatures, defaults, parameter names and state_dict keys.  No registered arch of this repository uses
them (rrdbnet_arch.py keeps its own); the module exists so that code written against BasicSR imports and runs.

GPU tensors run the HIP kernels, CPU tensors a float32 torch formula of the same definition:
  * `flow_warp`           cf_flow_warp (cf_warp.hip).  The definition (include/codeformer_hip.h) is the reference's arithmetic -- mesh grid
                          plus flow, normalised by n - 1, through F.grid_sample -- with the normalise / un-normalise round trip cancelled.  The
                          CPU path `flow_warp_host` states that definition in torch ops rather than calling F.grid_sample: grid_sample
                          leaves NaN positions undefined (here they give 0) and its round trip rounds the position three more times.
                          Wherever the round trip is exact the two agree bit for bit (tests/test_arch_util_host.py).
  * `pixel_unshuffle`     cf_pixel_unshuffle_nhwc, then back to NCHW; the view / permute formula on the CPU.  Pure data movement.
  * `ResidualBlockNoBN`   ops.conv2d, ReLU as cf_fused_bias_act (slope 0, scale 1), ops.conv2d with the CF_EPI_AXPY epilogue.
  * `Upsample`            ops.conv2d whose output stays channels-last, cf_pixel_shuffle_nhwc.
  * `DCNv2Pack`           the deformable convolution of codeformer_amd/dcn.py; the torchvision branch of the reference is not mirrored
                          (the offset layout is the same in both branches).
The two blocks cover 3x3 convolutions with num_feat % 16 == 0 -- the general-geometry fp32 implicit GEMM, as dcn._conv_offset_forward --
and run F.conv2d for any other width.  Everything on the device is inference-only: `flow_warp` and `DCNv2Pack` raise RuntimeError for a
tensor that requires grad under enabled grad (the rule of dcn.py); the two blocks run under torch.no_grad() like every HipModule.
"""
import collections.abc
import math
import warnings
from itertools import repeat

import torch
from torch import nn
from torch.nn import functional as F
from torch.nn.modules.batchnorm import _BatchNorm

from .. import ops
from ..dcn import ModulatedDeformConvPack, _no_grad_only, modulated_deform_conv
from ..utils.logger import get_root_logger
from .hip_module import HipModule
from .rrdbnet_arch import _unshuffle_host

__all__ = ['default_init_weights', 'make_layer', 'ResidualBlockNoBN', 'Upsample', 'flow_warp', 'resize_flow', 'pixel_unshuffle',
           'DCNv2Pack', 'trunc_normal_', 'to_1tuple', 'to_2tuple', 'to_3tuple', 'to_4tuple', 'to_ntuple']


@torch.no_grad()
def default_init_weights(module_list, scale=1, bias_fill=0, **kwargs):
    """Kaiming-normal weights times `scale` and biases filled with `bias_fill` for every Conv2d and Linear of the module (or list of
    modules); batch norms get weight 1 and the same bias fill.  kwargs go to nn.init.kaiming_normal_."""
    for module in (module_list if isinstance(module_list, list) else [module_list]):
        for m in module.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                nn.init.kaiming_normal_(m.weight, **kwargs)
                m.weight.data *= scale
            elif isinstance(m, _BatchNorm):
                nn.init.constant_(m.weight, 1)
            else:
                continue
            if m.bias is not None:
                m.bias.data.fill_(bias_fill)


def make_layer(basic_block, num_basic_block, **kwarg):
    """nn.Sequential of `num_basic_block` instances of `basic_block(**kwarg)`."""
    return nn.Sequential(*[basic_block(**kwarg) for _ in range(num_basic_block)])


def _covered(conv, x):
    """Whether ops.conv2d's general-geometry fp32 kernel takes this 3x3 / stride 1 / padding 1 layer (the rule of dcn._conv_offset_forward)."""
    return x.is_cuda and x.dtype == torch.float32 and conv.weight.shape[1] % 16 == 0 and conv.weight.shape[0] % 4 == 0


class ResidualBlockNoBN(HipModule):
    """identity + conv2(relu(conv1(x))) * res_scale, two 3x3 convolutions of num_feat channels without batch norm.
    pytorch_init=False: default_init_weights at scale 0.1.  On the device: num_feat % 16 == 0 runs the HIP path (module docstring), any
    other width F.conv2d."""

    def __init__(self, num_feat=64, res_scale=1, pytorch_init=False):
        super().__init__()
        self.res_scale = res_scale
        self.conv1 = nn.Conv2d(num_feat, num_feat, 3, 1, 1, bias=True)
        self.conv2 = nn.Conv2d(num_feat, num_feat, 3, 1, 1, bias=True)
        self.relu = nn.ReLU(inplace=True)
        if not pytorch_init:
            default_init_weights([self.conv1, self.conv2], 0.1)

    def forward_nhwc(self, x):
        t = ops.conv2d(x, self._pw_conv('conv1'))
        t = ops.fused_bias_act(t, None, negative_slope=0.0, scale=1.0)    # ReLU; elementwise, so the layout does not matter
        return ops.conv2d(t, self._pw_conv('conv2'), epilogue=ops.EPI_AXPY, res=x, sft_w=float(self.res_scale))

    def forward_host(self, x):
        return x + self.conv2(F.relu(self.conv1(x))) * self.res_scale

    def forward(self, x):
        if x.is_cuda and not _covered(self.conv1, x.float()):
            with torch.no_grad():
                return self.forward_host(x)
        return super().forward(x)


class Upsample(nn.Sequential, HipModule):
    """Conv2d(num_feat, s*s*num_feat, 3, 1, 1) + PixelShuffle(s) per stage: log2(scale) stages of s = 2 for scale = 2^n, one of s = 3 for
    scale = 3 (keys 0.weight, 0.bias, 2.weight, ...).  On the device the conv output stays channels-last and goes through
    cf_pixel_shuffle_nhwc (num_feat % 16 == 0; any other width runs the torch modules)."""

    def __init__(self, scale, num_feat):
        stages = []
        if (scale & (scale - 1)) == 0:
            stages = [2] * int(math.log(scale, 2))
        elif scale == 3:
            stages = [3]
        else:
            raise ValueError(f'scale {scale} is not supported. Supported scales: 2^n and 3.')
        m = []
        for s in stages:
            m += [nn.Conv2d(num_feat, s * s * num_feat, 3, 1, 1), nn.PixelShuffle(s)]
        super().__init__(*m)

    def forward(self, x):
        mods = list(self)
        if not x.is_cuda or not all(_covered(c, x.float()) for c in mods[0::2]):
            with torch.set_grad_enabled(torch.is_grad_enabled() and not x.is_cuda):
                return nn.Sequential.forward(self, x)
        ops.L.ensure_device(x.device)
        with torch.no_grad(), torch.cuda.device(x.device):
            t = ops.to_nhwc(x.float())
            for conv, shuffle in zip(mods[0::2], mods[1::2]):
                t = ops.pixel_shuffle_nhwc(ops.conv2d(t, self._pw_conv(conv)), shuffle.upscale_factor)
            return ops.to_nchw(t)


def _warp_coord(p, n, padding, align_corners):
    """Sample coordinate of position p (float32 tensor) on an axis of n pixels: cf_flow_warp's rule, one float32 operation per step."""
    num = torch.tensor(float(n - 1 if align_corners else n), dtype=torch.float32, device=p.device)
    i = p * (num / float(max(n - 1, 1)))
    if not align_corners:
        i = i - 0.5
    hi = float(n - 1)
    if padding == 2:
        lo, span = (0.0, hi) if align_corners else (-0.5, float(n))
        if span > 0:
            r = torch.fmod((i - lo).abs(), 2 * span)
            i = torch.where(r <= span, r, 2 * span - r) + lo
    if padding != 0:
        i = torch.where(i < 0, torch.zeros_like(i), torch.where(i > hi, torch.full_like(i, hi), i))     # (a NaN stays a NaN)
    return i


def flow_warp_host(x, flow, interp_mode='bilinear', padding_mode='zeros', align_corners=True):
    """The definition of cf_flow_warp in float32 torch ops (CPU tensors): the in-range test on the float32 coordinate before anything
    becomes an index (a NaN position gives 0 in every padding mode), corners outside the image +0, the four terms added in order."""
    interp, padding = ops.flow_warp_check(x, flow, interp_mode, padding_mode)
    B, C, H, W = x.shape
    dev = x.device
    px = torch.arange(W, device=dev, dtype=torch.float32)[None, None, :] + flow[..., 0]
    py = torch.arange(H, device=dev, dtype=torch.float32)[None, :, None] + flow[..., 1]
    ix, iy = _warp_coord(px, W, padding, align_corners), _warp_coord(py, H, padding, align_corners)
    xf = x.reshape(B, C, H * W)
    zero = torch.zeros_like(ix)

    def take(inside, cy, cx):
        idx = torch.where(inside, cy * W + cx, torch.zeros_like(cy)).reshape(B, 1, H * W).expand(B, C, H * W)
        return torch.gather(xf, 2, idx).reshape(B, C, H, W)

    if interp == 1:
        rx, ry = torch.round(ix), torch.round(iy)                      # half to even
        ok = (rx >= 0) & (ry >= 0) & (rx <= W - 1) & (ry <= H - 1)     # False for NaN
        v = take(ok, torch.where(ok, ry, zero).long(), torch.where(ok, rx, zero).long())
        return torch.where(ok[:, None], v, torch.zeros_like(v))
    ok = (ix > -1) & (iy > -1) & (ix < W) & (iy < H)
    ix, iy = torch.where(ok, ix, zero), torch.where(ok, iy, zero)
    x0f, y0f = torch.floor(ix), torch.floor(iy)
    lw, lh = ix - x0f, iy - y0f
    hw, hh = 1 - lw, 1 - lh
    x0, y0 = x0f.long(), y0f.long()
    out = None
    for cy, cx, cw in ((y0, x0, hh * hw), (y0, x0 + 1, hh * lw), (y0 + 1, x0, lh * hw), (y0 + 1, x0 + 1, lh * lw)):
        inside = ok & (cy >= 0) & (cy <= H - 1) & (cx >= 0) & (cx <= W - 1)
        v = take(inside, cy, cx)
        t = torch.where(inside[:, None], cw[:, None] * v, torch.zeros_like(v))
        out = t if out is None else out + t
    return out


def flow_warp(x, flow, interp_mode='bilinear', padding_mode='zeros', align_corners=True):
    """Warp an image or a feature map x (n, c, h, w) with the optical flow (n, h, w, 2), in pixels: the output at (y, x) is the sample of x
    at (x + flow[..., 0], y + flow[..., 1]).  interp_mode 'bilinear' | 'nearest', padding_mode 'zeros' | 'border' | 'reflection'."""
    assert x.size()[-2:] == flow.size()[1:3]
    _no_grad_only(x, flow)
    fn = flow_warp_host if x.device.type == 'cpu' else ops.flow_warp
    return fn(x, flow, interp_mode, padding_mode, align_corners)


def resize_flow(flow, size_type, sizes, interp_mode='bilinear', align_corners=False):
    """Resize a flow (n, 2, h, w) and rescale its vectors with it.  size_type 'ratio': sizes = [ratio_h, ratio_w]; 'shape': sizes =
    [out_h, out_w].  F.interpolate on either device: not a hot path."""
    if size_type not in ('ratio', 'shape'):
        raise ValueError(f'Size type should be ratio or shape, but got type {size_type}.')
    h, w = flow.shape[2:]
    out_h, out_w = (int(h * sizes[0]), int(w * sizes[1])) if size_type == 'ratio' else (sizes[0], sizes[1])
    scaled = flow * flow.new_tensor([out_w / w, out_h / h]).reshape(1, 2, 1, 1)     # channel 0 is horizontal, channel 1 vertical
    return F.interpolate(scaled, size=(out_h, out_w), mode=interp_mode, align_corners=align_corners)


def pixel_unshuffle(x, scale):
    """(b, c, h*s, w*s) -> (b, c*s*s, h, w), output channel (c*s + dy)*s + dx."""
    b, c, hh, hw = x.size()
    assert hh % scale == 0 and hw % scale == 0
    if x.is_cuda and x.dtype == torch.float32:
        _no_grad_only(x)
        t = ops.pixel_unshuffle_nhwc(x.detach(), scale)        # channels zero-padded to a multiple of 16
        cu = c * scale * scale
        return ops.to_nchw(t if t.shape[3] == cu else t[..., :cu].contiguous())
    return _unshuffle_host(x, scale)


class DCNv2Pack(ModulatedDeformConvPack):
    """Modulated deformable convolution for feature alignment: offsets and mask come from a second feature map `feat`, not from x
    (Delving Deep into Deformable Alignment in Video Super-Resolution).  Warns through the root logger when the mean |offset| exceeds
    50 -- one read-back per call, as in the reference."""

    def forward(self, x, feat):
        _no_grad_only(x, feat, self.weight, self.bias, self.conv_offset.weight, self.conv_offset.bias)
        offset, mask = self.offset_mask(feat)
        offset_absmean = torch.mean(torch.abs(offset))
        if offset_absmean > 50:
            get_root_logger().warning(f'Offset abs mean is {offset_absmean}, larger than 50.')
        return modulated_deform_conv(x, offset, mask, self.weight, self.bias, self.stride, self.padding, self.dilation, self.groups,
                                     self.deformable_groups)


def _no_grad_trunc_normal_(tensor, mean, std, a, b):
    """Inverse-CDF sampling: uniform on [cdf(a), cdf(b)] mapped through the normal quantile function, then clamped."""

    def cdf(v):
        return 0.5 * (1.0 + math.erf(v / math.sqrt(2.0)))

    if mean < a - 2 * std or mean > b + 2 * std:
        warnings.warn('mean is more than 2 std from [a, b] in nn.init.trunc_normal_. The distribution of values may be incorrect.',
                      stacklevel=2)
    with torch.no_grad():
        lo, hi = cdf((a - mean) / std), cdf((b - mean) / std)
        tensor.uniform_(2 * lo - 1, 2 * hi - 1)
        tensor.erfinv_()
        tensor.mul_(std * math.sqrt(2.0))
        tensor.add_(mean)
        tensor.clamp_(min=a, max=b)
    return tensor


def trunc_normal_(tensor, mean=0., std=1., a=-2., b=2.):
    """Fill `tensor` from N(mean, std^2) truncated to [a, b] (works best with a <= mean <= b)."""
    return _no_grad_trunc_normal_(tensor, mean, std, a, b)


def _ntuple(n):

    def parse(x):
        return x if isinstance(x, collections.abc.Iterable) else tuple(repeat(x, n))

    return parse


to_1tuple = _ntuple(1)
to_2tuple = _ntuple(2)
to_3tuple = _ntuple(3)
to_4tuple = _ntuple(4)
to_ntuple = _ntuple
