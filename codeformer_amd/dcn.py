"""Python surface of the reference's third bundled extension, basicsr/ops/dcn (deform_conv.py:182-377), on the HIP C ABI; forward only.

`deform_conv` / `modulated_deform_conv` and the four modules keep the reference's positional signatures, constructor arguments, parameter
names and shapes, initialisation and state_dict keys, so code and checkpoints written against `basicsr.ops.dcn` import, load and run.
No registered arch reaches the op; it exists for the same reason as fused_act and upfirdn2d (bundled.py).

The reference's extension is CUDA-only (deform_conv.py:55-56, :137-138 raise for CPU tensors), so no golden output of it exists here:
parity is BY THE OP'S DEFINITION, restated in include/codeformer_hip.h (cf_deform_conv2d) and, independently, in tests/dcn_ref.py.

  * GPU tensors run cf_deform_conv2d: the bilinear gather fused into an fp32-MFMA implicit GEMM where the shape allows, a general
    vector-ALU kernel otherwise (ops.deform_conv2d_route) -- never a torch fallback.
  * CPU tensors run a float32 torch formula of the same definition (`deform_conv2d_host`).  A deliberate superset: the reference raises
    NotImplementedError there.
  * float32 only: half / bfloat16 tensors raise TypeError.
  * Inference only, like upfirdn2d: a tensor that requires grad, under enabled grad, raises RuntimeError -- call under torch.no_grad().
  * `im2col_step` is accepted and its divisibility assert kept; there is no column buffer for it to size.
"""
import math

import torch
import torch.nn.functional as F
from torch import nn

from . import ops


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def _no_grad_only(*tensors):
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise RuntimeError('codeformer_amd deformable convolution is inference-only: call under torch.no_grad()')


def deform_conv2d_host(x, offset, weight, mask=None, bias=None, stride=1, padding=0, dilation=1, groups=1, deformable_groups=1):
    """The definition in float32 torch ops (CPU tensors): positions and the four corner weights one fp32 operation each, the in-range test
    on the fp32 position before anything is converted to an index (NaN / inf / huge offsets sample nothing), corners outside the image 0."""
    Ho, Wo = ops.deform_conv2d_check(x, offset, weight, mask, bias, stride, padding, dilation, groups, deformable_groups)
    (sh, sw), (ph, pw), (dh, dw) = _pair(stride), _pair(padding), _pair(dilation)
    B, C, H, W = x.shape
    cout, cin_g, kh, kw = weight.shape
    K, DG, G = kh * kw, deformable_groups, groups
    dev = x.device
    ki = torch.arange(kh, device=dev).repeat_interleave(kw)   # tap k = i*kw + j
    kj = torch.arange(kw, device=dev).repeat(kh)
    base_h = (torch.arange(Ho, device=dev)[None, :] * sh - ph + ki[:, None] * dh).to(torch.float32)   # (K, Ho): summed in int, converted once
    base_w = (torch.arange(Wo, device=dev)[None, :] * sw - pw + kj[:, None] * dw).to(torch.float32)   # (K, Wo)
    off = offset.reshape(B, DG, K, 2, Ho, Wo)
    h = base_h[None, None, :, :, None] + off[:, :, :, 0]      # (B, DG, K, Ho, Wo)
    w = base_w[None, None, :, None, :] + off[:, :, :, 1]
    ok = (h > -1) & (w > -1) & (h < H) & (w < W)              # False for NaN
    h = torch.where(ok, h, torch.zeros_like(h))
    w = torch.where(ok, w, torch.zeros_like(w))
    h0f, w0f = torch.floor(h), torch.floor(w)
    lh, lw = h - h0f, w - w0f
    hh, hw = 1 - lh, 1 - lw
    h0, w0 = h0f.long(), w0f.long()
    m = torch.ones_like(h) if mask is None else mask.reshape(B, DG, K, Ho, Wo)
    cpdg = C // DG
    xf = x.reshape(B, DG, cpdg, H * W)
    val = torch.zeros(B, DG, cpdg, K, Ho, Wo, dtype=torch.float32, device=dev)
    for cy, cx, cw in ((h0, w0, hh * hw), (h0, w0 + 1, hh * lw), (h0 + 1, w0, lh * hw), (h0 + 1, w0 + 1, lh * lw)):
        inside = ok & (cy >= 0) & (cy <= H - 1) & (cx >= 0) & (cx <= W - 1)
        idx = torch.where(inside, cy * W + cx, torch.zeros_like(cy)).reshape(B, DG, 1, K * Ho * Wo).expand(B, DG, cpdg, K * Ho * Wo)
        v = torch.gather(xf, 3, idx).reshape(B, DG, cpdg, K, Ho, Wo)
        cwm = torch.where(inside, cw * m, torch.zeros_like(cw))[:, :, None]
        val = val + torch.where(inside[:, :, None], cwm * v, torch.zeros_like(v))   # (an excluded corner is 0 whatever the pixel holds)
    col = val.reshape(B, G, cin_g * K, Ho * Wo)
    out = torch.einsum('gok,bgkp->bgop', weight.reshape(G, cout // G, cin_g * K), col).reshape(B, cout, Ho, Wo)
    return out if bias is None else out + bias.reshape(1, cout, 1, 1)


def _run(x, offset, weight, mask, bias, stride, padding, dilation, groups, deformable_groups):
    _no_grad_only(x, offset, weight, mask, bias)
    if x is None or x.dim() != 4:
        raise ValueError(f'Expected 4D tensor as input, got {None if x is None else x.dim()}D tensor instead.')
    fn = deform_conv2d_host if x.device.type == 'cpu' else ops.deform_conv2d
    return fn(x, offset, weight, mask, bias, stride, padding, dilation, groups, deformable_groups)


def deform_conv(input, offset, weight, stride=1, padding=0, dilation=1, groups=1, deformable_groups=1, im2col_step=64):
    """Plain (v1) deformable convolution: no mask, no bias; stride / padding / dilation an int or a (vertical, horizontal) pair."""
    if input is not None and input.dim() == 4:
        step = min(im2col_step, input.shape[0])
        assert input.shape[0] % step == 0, 'im2col step must divide batchsize'
    return _run(input, offset, weight, None, None, stride, padding, dilation, groups, deformable_groups)


def modulated_deform_conv(input, offset, mask, weight, bias=None, stride=1, padding=0, dilation=1, groups=1, deformable_groups=1):
    """Modulated (v2) deformable convolution; stride / padding / dilation are one integer for both axes."""
    return _run(input, offset, weight, mask, bias, stride, padding, dilation, groups, deformable_groups)


class _Apply:
    """`DeformConvFunction.apply(...)` / `ModulatedDeformConvFunction.apply(...)` of the reference's `__all__`: the same calls as the two
    functions above.  They are not autograd Functions here -- the op has no backward pass."""

    def __init__(self, fn):
        self.apply = fn


DeformConvFunction = _Apply(deform_conv)
ModulatedDeformConvFunction = _Apply(modulated_deform_conv)


def _uniform_init(weight, in_channels, kernel_size):
    n = in_channels
    for k in kernel_size:
        n *= k
    bound = 1.0 / math.sqrt(n)
    weight.data.uniform_(-bound, bound)


def _conv_offset_forward(conv, x):
    """`conv(x)` of an nn.Conv2d held by its parameters: on the library's general-geometry fp32 implicit GEMM (ops.conv2d) where that covers
    the layer -- a CUDA float32 input, 3x3, stride 1, padding 1, dilation 1, one group, cin % 16 == 0, cout % 4 == 0 -- else F.conv2d."""
    w = conv.weight
    covered = x.is_cuda and x.dtype == torch.float32 and tuple(w.shape[2:]) == (3, 3) and conv.stride == (1, 1) and conv.padding == (1, 1) and \
        conv.dilation == (1, 1) and conv.groups == 1 and w.shape[1] % 16 == 0 and w.shape[0] % 4 == 0
    if not covered:
        return F.conv2d(x, w, conv.bias, conv.stride, conv.padding, conv.dilation, conv.groups)
    ver = ops.tensor_version(w)
    key = (w.data_ptr(), ver, None if conv.bias is None else (conv.bias.data_ptr(), ops.tensor_version(conv.bias)), str(w.device))
    ent = conv.__dict__.get('_cf_packed')
    if ent is None or ver is None or ent[0] != key:
        ent = (key, ops.pack_weight(w, conv.bias))
        conv.__dict__['_cf_packed'] = ent
    return ops.to_nchw(ops.conv2d(ops.to_nhwc(x), ent[1]))


class DeformConv(nn.Module):

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, deformable_groups=1, bias=False):
        super().__init__()
        assert not bias
        assert in_channels % groups == 0, f'in_channels {in_channels} is not divisible by groups {groups}'
        assert out_channels % groups == 0, f'out_channels {out_channels} is not divisible by groups {groups}'
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride, self.padding, self.dilation = _pair(kernel_size), _pair(stride), _pair(padding), _pair(dilation)
        self.groups, self.deformable_groups = groups, deformable_groups
        self.transposed, self.output_padding = False, (0,)   # (nn.Conv2d's attributes, as the reference keeps them)
        self.weight = nn.Parameter(torch.Tensor(out_channels, in_channels // groups, *self.kernel_size))
        self.reset_parameters()

    def reset_parameters(self):
        _uniform_init(self.weight, self.in_channels, self.kernel_size)

    def forward(self, x, offset):
        # an input smaller than the kernel is zero-padded at the bottom / right up to the kernel's size, and the output cropped back
        pad_h, pad_w = max(self.kernel_size[0] - x.size(2), 0), max(self.kernel_size[1] - x.size(3), 0)
        if pad_h or pad_w:
            x = F.pad(x, (0, pad_w, 0, pad_h), 'constant', 0).contiguous()
            offset = F.pad(offset, (0, pad_w, 0, pad_h), 'constant', 0).contiguous()
        out = deform_conv(x, offset, self.weight, self.stride, self.padding, self.dilation, self.groups, self.deformable_groups)
        if pad_h or pad_w:
            out = out[:, :, :out.size(2) - pad_h, :out.size(3) - pad_w].contiguous()
        return out


class DeformConvPack(DeformConv):
    """DeformConv that predicts its own offsets with `conv_offset`, an nn.Conv2d of the layer's geometry, zero-initialised."""

    _version = 2

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.conv_offset = nn.Conv2d(self.in_channels, self.deformable_groups * 2 * self.kernel_size[0] * self.kernel_size[1],
                                     kernel_size=self.kernel_size, stride=_pair(self.stride), padding=_pair(self.padding),
                                     dilation=_pair(self.dilation), bias=True)
        self.init_offset()

    def init_offset(self):
        self.conv_offset.weight.data.zero_()
        self.conv_offset.bias.data.zero_()

    def offset_mask(self, x):
        """(offset,): what `conv_offset` predicts for x."""
        return (_conv_offset_forward(self.conv_offset, x),)

    def forward(self, x):
        _no_grad_only(x, self.weight, self.conv_offset.weight, self.conv_offset.bias)
        offset, = self.offset_mask(x)
        return deform_conv(x, offset, self.weight, self.stride, self.padding, self.dilation, self.groups, self.deformable_groups)


class ModulatedDeformConv(nn.Module):

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, deformable_groups=1, bias=True):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size = _pair(kernel_size)
        self.stride, self.padding, self.dilation = stride, padding, dilation
        self.groups, self.deformable_groups = groups, deformable_groups
        self.with_bias = bias
        self.transposed, self.output_padding = False, (0,)
        self.weight = nn.Parameter(torch.Tensor(out_channels, in_channels // groups, *self.kernel_size))
        if bias:
            self.bias = nn.Parameter(torch.Tensor(out_channels))
        else:
            self.register_parameter('bias', None)
        self.init_weights()

    def init_weights(self):
        _uniform_init(self.weight, self.in_channels, self.kernel_size)
        if self.bias is not None:
            self.bias.data.zero_()

    def forward(self, x, offset, mask):
        return modulated_deform_conv(x, offset, mask, self.weight, self.bias, self.stride, self.padding, self.dilation, self.groups,
                                     self.deformable_groups)


class ModulatedDeformConvPack(ModulatedDeformConv):
    """ModulatedDeformConv that predicts offsets and mask with `conv_offset` (3 * DG * kh * kw channels, zero-initialised): the first two
    thirds are the offsets, the sigmoid of the last third is the mask -- so a fresh module computes 0.5 * conv(x) + bias."""

    _version = 2

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.conv_offset = nn.Conv2d(self.in_channels, self.deformable_groups * 3 * self.kernel_size[0] * self.kernel_size[1],
                                     kernel_size=self.kernel_size, stride=_pair(self.stride), padding=_pair(self.padding),
                                     dilation=_pair(self.dilation), bias=True)
        self.init_weights()

    def init_weights(self):
        super().init_weights()
        if hasattr(self, 'conv_offset'):
            self.conv_offset.weight.data.zero_()
            self.conv_offset.bias.data.zero_()

    def offset_mask(self, x):
        """(offset, mask) that `conv_offset` predicts for x."""
        o1, o2, m = torch.chunk(_conv_offset_forward(self.conv_offset, x), 3, dim=1)
        return torch.cat((o1, o2), dim=1), torch.sigmoid(m)

    def forward(self, x):
        _no_grad_only(x, self.weight, self.bias, self.conv_offset.weight, self.conv_offset.bias)
        offset, mask = self.offset_mask(x)
        return modulated_deform_conv(x, offset, mask, self.weight, self.bias, self.stride, self.padding, self.dilation, self.groups,
                                     self.deformable_groups)
