"""VGGFeatureExtractor -- the network behind the perceptual and style terms (reference: basicsr/archs/vgg_arch.py:9-161) -- on the HIP kernels.

Same public names, constructor arguments, `state_dict` keys (`vgg_net.<layer name>.weight` / `.bias`, the BatchNorm entries of the `_bn` types,
`mean` / `std`) and forward result (a dict of NCHW float32 tensors in layer order) as the reference.  The reference takes the layer stack
from torchvision.models.vgg; torchvision is not a dependency here, so the `features` stack of vgg11 / 13 / 16 / 19 and their `_bn` forms is
stated below from the published configuration (Simonyan & Zisserman 2015, tables A / B / D / E): 3x3 convolutions with padding 1, optional
BatchNorm, ReLU, 2x2 max-pool -- initialised as torchvision initialises it (kaiming_normal_(fan_out, relu), zero bias, BatchNorm 1 / 0) in the
same module order, so the same seed gives the same weights.  Weights: VGG_PRETRAIN_PATH (a torchvision state dict: `features.<i>.*` by
position, `classifier.*` ignored) when that file exists, else the seeded initialisation and one warning.  Nothing is ever downloaded, and no
trained VGG checkpoint ships with or was run through this code.

CPU tensors run `forward_host` (stock torch ops: the reference's forward).  CUDA tensors run the HIP path, value-only, under no_grad:
  * cf_vgg_input: (x + 1) / 2 and (x - mean) / std in the reference's order, one fp32 operation each, into NHWC with 16 channels (13 zero):
    the conv's zero padding then pads the NORMALISED tensor, as in the reference;
  * every conv asks ops.conv_code(ops.WINOGRAD, ...): exact-fp32 Winograd F(2x2,3x3) on whole 8x16 patches, the general fp32 kernel elsewhere
    (`winograd_f43 = True` requests ops.WINOGRAD_F43 instead: faster from 64x64 up, larger error -- opt-in, see profiles/NOTES.md); on the
    general kernel a layer of more than 128 input channels runs per 128 channels, the parts added by the residual epilogue (_conv);
  * a BatchNorm is folded into the packed weight and bias in float64, rounded once (folded.fold_conv_bn); a requested `convX_Y` of a
    `_bn` type (the value BEFORE the BatchNorm) is a second launch with the unfolded weight;
  * ReLU is cf_relu (in place unless the pre-ReLU tensor was requested) or rides in cf_relu_maxpool2, which also hands out the full-size
    ReLU tensor when `reluX_Y` in front of a pool was requested.
Refused before the first launch (check_device_call): vgg_net in training mode or parameters that require grad (RuntimeError), a
pooling_stride other than 2 (NotImplementedError), inputs that are not (B,3,H,W) or that a pool would take to zero (ValueError).
"""
import logging
import os
from collections import OrderedDict

import torch
from torch import nn

from .. import ops
from ..utils.registry import ARCH_REGISTRY
from .folded import folded_layer
from .hip_module import HipModule

VGG_PRETRAIN_PATH = 'experiments/pretrained_models/vgg19-dcbb9e9d.pth'
CHAIN_CIN = 128   # input channels per launch of the general fp32 kernel: 1152 products per accumulation chain (see VGGFeatureExtractor._conv)

# output channels per stage (the published configurations A, B, D, E); a pool follows every stage
_STAGES = {'vgg11': (1, 1, 2, 2, 2), 'vgg13': (2, 2, 2, 2, 2), 'vgg16': (2, 2, 3, 3, 3), 'vgg19': (2, 2, 4, 4, 4)}
_WIDTHS = (64, 128, 256, 512, 512)


def _names(vgg_type):
    out = []
    for s, n in enumerate(_STAGES[vgg_type], 1):
        for i in range(1, n + 1):
            out += [f'conv{s}_{i}', f'relu{s}_{i}']
        out.append(f'pool{s}')
    return out


NAMES = {t: _names(t) for t in _STAGES}


def insert_bn(names):
    """The layer names with a `bnX_Y` after every `convX_Y` (vgg_arch.py:36-51)."""
    names_bn = []
    for name in names:
        names_bn.append(name)
        if 'conv' in name:
            names_bn.append('bn' + name.replace('conv', ''))
    return names_bn


def make_features(vgg_type):
    """The full `features` stack of `vgg_type` ('vgg11' .. 'vgg19', optionally '_bn') as a list of modules, in torchvision's order and with
    torchvision's initialisation (drawn in module order from torch's global generator)."""
    base, bn = vgg_type.replace('_bn', ''), vgg_type.endswith('_bn')
    if base not in _STAGES:
        raise ValueError(f'unknown vgg_type {vgg_type}')
    layers, cin = [], 3
    for n, cout in zip(_STAGES[base], _WIDTHS):
        for _ in range(n):
            layers.append(nn.Conv2d(cin, cout, kernel_size=3, padding=1))
            if bn:
                layers.append(nn.BatchNorm2d(cout))
            layers.append(nn.ReLU(inplace=True))
            cin = cout
        layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
    for m in layers:
        if isinstance(m, nn.Conv2d):
            nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.BatchNorm2d):
            nn.init.constant_(m.weight, 1)
            nn.init.constant_(m.bias, 0)
    return layers


class FeaturesOnly(nn.Module):
    """`.features` of a torchvision VGG, without the classifier: what the reference's VGGFeatureExtractor reads of the model it builds.
    load_state_dict ignores `classifier.*`."""

    def __init__(self, vgg_type):
        super().__init__()
        self.features = nn.Sequential(*make_features(vgg_type))

    def load_state_dict(self, state_dict, strict=True):
        return super().load_state_dict({k: v for k, v in state_dict.items() if not k.startswith('classifier.')}, strict=strict)


@ARCH_REGISTRY.register()
class VGGFeatureExtractor(HipModule):
    """VGG network for feature extraction (vgg_arch.py:54-161).

    layer_name_list: names of the layers whose outputs forward returns; vgg_type: 'vgg11' | 'vgg13' | 'vgg16' | 'vgg19', optionally '_bn';
    use_input_norm: (x - mean) / std of an image in [0, 1]; range_norm: (x + 1) / 2 first, for an image in [-1, 1]; requires_grad: train
    the VGG parameters (host path only); remove_pooling: drop the max-pools; pooling_stride: their stride (HIP path: 2)."""

    def __init__(self, layer_name_list, vgg_type='vgg19', use_input_norm=True, range_norm=False, requires_grad=False, remove_pooling=False,
                 pooling_stride=2):
        super().__init__()
        self.layer_name_list = layer_name_list
        self.use_input_norm = use_input_norm
        self.range_norm = range_norm
        self.winograd_f43 = False

        self.names = NAMES[vgg_type.replace('_bn', '')]
        if 'bn' in vgg_type:
            self.names = insert_bn(self.names)
        max_idx = max([0] + [self.names.index(v) for v in layer_name_list])   # only the layers that are used

        vgg_net = FeaturesOnly(vgg_type)
        path = VGG_PRETRAIN_PATH
        if os.path.exists(path):
            vgg_net.load_state_dict(torch.load(path, map_location='cpu', weights_only=True))
        else:
            logging.getLogger('basicsr').warning(f'{path} not found and nothing is downloaded: VGGFeatureExtractor({vgg_type}) keeps its random '
                                                 'initialisation')
        modified_net = OrderedDict()
        for k, v in zip(self.names, vgg_net.features[:max_idx + 1]):
            if 'pool' in k:
                if remove_pooling:
                    continue
                modified_net[k] = nn.MaxPool2d(kernel_size=2, stride=pooling_stride)
            else:
                modified_net[k] = v
        self.vgg_net = nn.Sequential(modified_net)

        if not requires_grad:
            self.vgg_net.eval()
            for param in self.parameters():
                param.requires_grad = False
        else:
            self.vgg_net.train()
            for param in self.parameters():
                param.requires_grad = True

        if self.use_input_norm:
            self.register_buffer('mean', torch.Tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1))   # of an image in [0, 1]
            self.register_buffer('std', torch.Tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1))

    # -- host ------------------------------------------------------------------------------------------------------------------------------
    def forward_host(self, x):
        """The reference's forward on stock torch ops (on whatever device x lies)."""
        if self.range_norm:
            x = (x + 1) / 2
        if self.use_input_norm:
            x = (x - self.mean) / self.std
        output = {}
        for key, layer in self.vgg_net._modules.items():
            x = layer(x)
            if key in self.layer_name_list:
                output[key] = x.clone()
        return output

    # -- HIP -------------------------------------------------------------------------------------------------------------------------------
    def check_device_call(self, shape):
        """What the HIP path refuses, before it touches a device."""
        if self.vgg_net.training or any(p.requires_grad for p in self.parameters()):
            raise RuntimeError('VGGFeatureExtractor on HIP is value-only and folds BatchNorm: build it with requires_grad=False and keep vgg_net in eval mode')
        for m in self.vgg_net:
            if isinstance(m, nn.MaxPool2d) and (m.stride, m.kernel_size) not in ((2, 2), ((2, 2), (2, 2))):
                raise NotImplementedError(f'VGGFeatureExtractor on HIP: pooling_stride 2, got {m.stride}')
        if len(shape) != 4 or shape[1] != 3 or min(shape) < 1:
            raise ValueError(f'VGGFeatureExtractor on HIP takes (B,3,H,W), got {tuple(shape)}')
        h, w = shape[2], shape[3]
        for k, m in self.vgg_net._modules.items():
            if isinstance(m, nn.MaxPool2d):
                if h < 2 or w < 2:
                    raise ValueError(f'VGGFeatureExtractor: {k} would take a {h}x{w} map of the {shape[2]}x{shape[3]} input to zero')
                h, w = h // 2, w // 2

    def _norm_consts(self):
        if not self.use_input_norm:
            return None, None
        return self._packed('norm', lambda: (self.mean.detach().flatten().tolist(), self.std.detach().flatten().tolist()), self.mean, self.std)

    def _conv(self, name, conv, bn, x):
        """conv (with bn folded, when given) of the channels-last x on the route ops.conv_code names.  The general fp32 kernel adds all
        9 * cin products of an output in ONE chain of MFMA accumulations, and the error of such a chain grows several times faster than
        rounded additions in another order would (profiles/NOTES.md): on that kernel a layer of more than CHAIN_CIN input channels runs once
        per CHAIN_CIN channels (a channel slice of x, the matching slice of the weight) and the partial outputs are added in channel order
        by the residual epilogue.  The Winograd kernels' chains are cin long (one per transform position) and are left whole.  The rule is a
        function of the per-image shape only."""
        cout, cin = conv.weight.shape[:2]
        code = ops.conv_code(ops.WINOGRAD_F43 if self.winograd_f43 else ops.WINOGRAD, cin, cout, x.shape[1], x.shape[2])
        step = CHAIN_CIN if (code == 0 and cin > CHAIN_CIN and cin % CHAIN_CIN == 0) else cin

        fold, deps = folded_layer(conv, bn)

        def build(k0):
            w, b = fold()
            return ops.pack_weight(w.float()[:, k0:k0 + step].contiguous(), b.float() if k0 == 0 else None, bf16=code)
        y = None
        for k0 in range(0, cin, step):
            pw = self._packed((name, code, bn is not None, k0, step), lambda: build(k0), *deps)
            xs = x if step == cin else x[..., k0:k0 + step]
            y = ops.conv2d(xs, pw) if y is None else ops.conv2d(xs, pw, epilogue=ops.EPI_RESIDUAL, res=y)
        return y

    def features_from_views(self, views, bgr=False):
        """{layer name: (B,h,w,c) channels-last float32} of the images of `views`: (b,H,W,3) VIEWS (any strides) of uint8 or float32
        tensors of one size on one device, concatenated along the batch.  The caller holds no_grad and the device."""
        B = sum(v.shape[0] for v in views)
        H, W = views[0].shape[1:3]
        if any(v.dim() != 4 or tuple(v.shape[1:]) != (H, W, 3) for v in views):
            raise ValueError(f'VGGFeatureExtractor: (b,H,W,3) views of one size are needed, got {[tuple(v.shape) for v in views]}')
        self.check_device_call((B, 3, H, W))
        mean, std = self._norm_consts()
        h = torch.empty((B, H, W, ops.VGG_IN_CPAD), dtype=torch.float32, device=views[0].device)
        b0 = 0
        for v in views:
            ops.vgg_input(v, bgr, self.range_norm, mean, std, out=h[b0:b0 + v.shape[0]])
            b0 += v.shape[0]
        want = set(self.layer_name_list)
        out = {}
        items = list(self.vgg_net._modules.items())
        i, kept = 0, False     # kept: h is a requested tensor and must not be overwritten
        while i < len(items):
            name, m = items[i]
            nxt = items[i + 1] if i + 1 < len(items) else (None, None)
            if isinstance(m, nn.Conv2d):
                bn = nxt[1] if isinstance(nxt[1], nn.BatchNorm2d) else None
                x = h
                kept = False
                if bn is None or name in want:
                    h = self._conv(name, m, None, x)
                    if name in want:
                        out[name], kept = h, True
                if bn is not None:
                    h = self._conv(nxt[0], m, bn, x)
                    kept = nxt[0] in want
                    if kept:
                        out[nxt[0]] = h
                    i += 1
            elif isinstance(m, nn.ReLU):
                if isinstance(nxt[1], nn.MaxPool2d):
                    if name in want:
                        h, out[name] = ops.relu_maxpool2(h, full=True if kept else 'inplace')
                    else:
                        h = ops.relu_maxpool2(h)
                    if nxt[0] in want:
                        out[nxt[0]] = h
                    i += 1
                else:
                    h = ops.relu(h, inplace=not kept)
                    if name in want:
                        out[name] = h
                kept = False     # (a requested ReLU or pool output is only read from here on)
            else:
                raise NotImplementedError(f'VGGFeatureExtractor on HIP: layer {name} ({type(m).__name__}) in this position')
            i += 1
        return out

    def features_nhwc(self, x):
        """forward without the NCHW conversion: {layer name: (B,h,w,c) channels-last float32} of a (B,3,H,W) CUDA tensor."""
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f'VGGFeatureExtractor on HIP takes (B,3,H,W), got {tuple(x.shape)}')
        self.check_device_call(x.shape)
        ops.L.ensure_device(x.device)
        with torch.no_grad(), torch.cuda.device(x.device):
            x = x.detach()
            return self.features_from_views([(x if x.dtype == torch.float32 else x.float()).permute(0, 2, 3, 1)])

    def forward(self, x):
        if x.is_cuda:
            feats = self.features_nhwc(x)
            with torch.no_grad(), torch.cuda.device(x.device):
                return {k: ops.to_nchw(v) for k, v in feats.items()}
        return self.forward_host(x)
