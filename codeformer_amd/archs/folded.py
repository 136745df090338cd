"""The BatchNorm-folded convolution layer of ResNetArcFace, VGGFeatureExtractor, BiSeNet / ResNet18 and the RetinaFace ResNet-50 detector (ParseNet
shares bn_deps and need_eval): how such a layer is folded, packed, cached and launched, written once.
  * an eval-mode BatchNorm AFTER a conv goes into the conv's weight and bias: on the device paths in float64, rounded once to float32; in the
    networks' `forward_folded` restatements in the parameters' dtype;
  * a layer is a pair (fold, deps): fold(dtype=float64) -> (weight, bias or None), deps the tensors its cached pack is keyed on (HipModule._packed
    rebuilds the pack when one of them is modified, replaced or moved).  `folded_layer` makes one of (conv, bn);
  * 3x3 layers run through `conv_hip` on the general fp32 kernel, the detector's 1x1 layers on cf_pointwise (`pointwise_hip`), the 7x7 / stride-2
    stems through `stem7x7_hip`: no BatchNorm, ReLU, PReLU or residual add is a launch of its own, except ReLU after the nearest-x2 form.
"""
import torch

from .. import ops


def bn_affine(bn, dtype=None):
    """(scale, shift) of an eval-mode BatchNorm: y = x * scale + shift."""
    dtype = dtype or bn.weight.dtype
    g = bn.weight.detach().to(dtype) * torch.rsqrt(bn.running_var.detach().to(dtype) + bn.eps)
    return g, bn.bias.detach().to(dtype) - bn.running_mean.detach().to(dtype) * g


def bn_deps(bn):
    return [bn.weight, bn.bias, bn.running_mean, bn.running_var]


def need_eval(mod):
    if mod.training:
        raise RuntimeError(f'{type(mod).__name__} on HIP folds BatchNorm and drops Dropout: call .eval() first')


def prelu_slope(mod, prelu):
    """The one slope of an nn.PReLU() as a Python float, read back once per parameter version."""
    if prelu.weight.numel() != 1:
        raise NotImplementedError('HIP path: nn.PReLU() with one slope')
    return mod._packed(('slope', id(prelu)), lambda: float(prelu.weight.detach().reshape(-1)[0]), prelu.weight)


def centre_tap(w):
    """A (cout,cin,1,1) weight as the centre tap of a (cout,cin,3,3) one: the eight other taps add 0 * x = 0 to a finite sum."""
    w3 = w.new_zeros(w.shape[0], w.shape[1], 3, 3)
    w3[:, :, 1, 1] = w[:, :, 0, 0]
    return w3


def fold_conv_bn(conv, bn, dtype=None, embed3=False):
    """(weight, bias or None) of bn(conv(x)); bn None: of conv(x).  embed3: a 1x1 weight as the centre tap of a 3x3 one."""
    dtype = dtype or conv.weight.dtype
    w = conv.weight.detach().to(dtype)
    b = None if conv.bias is None else conv.bias.detach().to(dtype)
    if bn is not None:
        g, t = bn_affine(bn, dtype)
        w = w * g.view(-1, 1, 1, 1)
        b = t if b is None else t + g * b
    if embed3:
        w = centre_tap(w)
    return w.contiguous(), None if b is None else b.contiguous()


def folded_layer(conv, bn, embed3=False):
    """The layer (fold, deps) of bn(conv(x)) (bn None: of conv(x))."""
    deps = [p for p in (conv.weight, conv.bias) if p is not None] + ([] if bn is None else bn_deps(bn))
    return (lambda dtype=torch.float64: fold_conv_bn(conv, bn, dtype, embed3)), deps


def epilogue_of(has_res, has_slope, up2x):
    """(conv epilogue, whether cf_relu follows) of act(conv + bias [+ res]).  The PReLU epilogues (alpha = sft_w; ReLU is alpha 0.0: x > 0 ? x :
    0 * x) exist on the plain instantiations only: after the sub-pixel form the activation is a launch of its own."""
    if has_slope and not up2x:
        return (ops.EPI_RES_PRELU if has_res else ops.EPI_PRELU), False
    return (ops.EPI_RESIDUAL if has_res else ops.EPI_NONE), has_slope


def conv_hip(mod, key, layer, x, *, stride=1, up2x=False, res=None, slope=None, out=None, x2=None, **conv2d_kw):
    """act(conv 3x3(x) + bias [+ res]) of the channels-last x on the general fp32 kernel, one launch; the packed weight is cached on `mod` under
    `key`.  slope: None no activation, 0.0 ReLU, else the PReLU slope.  stride 2: one padded row / column on every side; up2x: nearest x2 first
    (the folded sub-pixel form; ReLU only); x2: a second tensor concatenated after x; conv2d_kw: further ops.conv2d arguments (a prologue)."""
    if stride not in (1, 2) or (up2x and stride != 1):
        raise NotImplementedError(f'HIP path: stride 1 or 2 (nearest x2 first: 1), got {stride}')
    if up2x and slope:
        raise NotImplementedError(f'HIP path: ReLU or no activation after the nearest-x2 form, got slope {slope}')

    def build():
        w, b = layer[0]()
        return ops.pack_weight(w.float().contiguous(), None if b is None else b.float(), up2x=up2x)
    epi, relu_after = epilogue_of(res is not None, slope is not None, up2x)
    alpha = 0.0 if slope is None else slope   # (cf_conv_desc.sft_w; read by the PReLU epilogues only)
    kw = dict(conv2d_kw, epilogue=epi, res=res, out=out, x2=x2, sft_w=alpha)
    if up2x:
        kw.update(upsample=True, pad_mode=ops.PAD_ZERO)
    elif stride == 2:
        kw.update(stride=2, pad_lo=1)
    y = ops.conv2d(x, mod._packed(key, build, *layer[1]), **kw)
    return ops.relu(y, inplace=True) if relu_after else y


def pointwise_hip(mod, key, layer):
    """The cached PackedPointwise (cf_pointwise) of a 1x1 layer."""
    def build():
        w, b = layer[0]()
        return ops.pack_pointwise(w.float(), b.float())
    return mod._packed(key, build, *layer[1])


def stem7x7_hip(mod, key, conv, bn, x):
    """(B,3,H,W) NCHW float32 -> relu(bn(conv 7x7 / stride 2 / pad 3 (x))), (B,ceil(H/2),ceil(W/2),64) channels-last (before the max-pool)."""
    fold, deps = folded_layer(conv, bn)

    def build():
        w, b = fold()
        return ops.pack_stem7x7(w.float()), b.float().contiguous()
    wp, b = mod._packed(key, build, *deps)
    return ops.stem7x7s2(x.contiguous(), wp, b)
