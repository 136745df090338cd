"""ResNetArcFace -- the identity network behind the third full-reference score of face restoration (reference:
basicsr/archs/arcface_arch.py:5-245) -- on the HIP kernels.

Same classes, constructor arguments, attribute names, `state_dict` keys and initialisation as the reference, so a reference checkpoint
loads unchanged.  Nothing here is used by CodeFormer.forward.  Supported on the GPU: what the reference itself can instantiate, that is
block 'IRBlock' with use_se True or False and any `layers`, in eval mode, on (B,1,128,128) float32 (fc5 fixes the size).  BasicBlock and
Bottleneck are host-only: the reference's _make_layer passes `use_se=` to every block, so neither can be built through ResNetArcFace.

How the layers map (fp32 tensors, IEEE-fp32 MFMA operands; no BatchNorm, PReLU or residual add is a launch of its own):
  * a BatchNorm AFTER a conv (stem bn1, IRBlock bn1 / bn2, the shortcut's BN) is folded into the packed weight and bias, in float64,
    rounded once;
  * IRBlock.bn0 stands BEFORE conv1, and the reference zero-pads the NORMALISED tensor: its shift cannot go into the conv bias without
    being wrong on every border pixel.  It rides in conv1's gather (CF_PRO_AFFINE; the (B,C) tables repeat one row), padding stays zero;
  * nn.PReLU() has one learned slope of any sign or size: x > 0 ? x : a * x in the conv epilogues CF_EPI_PRELU / CF_EPI_RES_PRELU (alpha
    = cf_conv_desc.sft_w; CF_EPI_LEAKY could not be reused, its 0.2 is a constant of the kernel).  The slope is read on the host once per
    parameter version;
  * stem: conv 1 -> 64 at 128x128 (the <= 4-channel NCHW-input kernel), then cf_prelu_maxpool2 (PReLU first: not monotone for a < 0);
  * stride-2 conv2: the fp32 stride-2 form with one padded row / column on every side (pad_lo = 1);
  * the 1x1 stride-s shortcut conv runs as a 3x3 stride-s pad_lo = 1 conv whose only non-zero tap is the centre: the eight other taps add
    0 * x = 0 to a finite sum, so the restatement is exact (9x the multiplies of a layer that is a few percent of the block);
  * SEBlock: cf_se_pool -> cf_se_gate -> cf_se_scale_res_prelu, which also applies the block's residual add and PReLU;
  * tail: bn4, Dropout (identity in eval), the NCHW flatten, fc5 and bn5 are ONE matrix: fc5's columns are permuted from c*64 + h*8 + w to
    channels-last order, bn4 scales them (its shift adds to the bias) and bn5 scales the rows; cf_fc_rows runs it.
`forward_folded` evaluates exactly this dataflow with stock torch ops in the parameters' dtype (tests compare it in float64 with the
unfolded module).
"""
import torch
from torch import nn
from torch.nn import functional as F

from .. import ops
from ..utils.registry import ARCH_REGISTRY
from .folded import bn_affine, bn_deps, conv_hip, fold_conv_bn, folded_layer, need_eval, prelu_slope
from .hip_module import HipModule

IN_SIZE = 128   # fc5 = Linear(512 * 8 * 8, 512) after four halvings


def conv3x3(inplanes, outplanes, stride=1):
    """3x3 convolution, padding 1, no bias (arcface_arch.py:5-13)."""
    return nn.Conv2d(inplanes, outplanes, kernel_size=3, stride=stride, padding=1, bias=False)


class BasicBlock(nn.Module):
    """conv-bn-relu, conv-bn, add, relu (arcface_arch.py:16-53).  Host only."""
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = conv3x3(inplanes, planes, stride)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = conv3x3(planes, planes)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        if x.is_cuda:
            raise NotImplementedError('BasicBlock has no HIP path (ResNetArcFace cannot instantiate it); IRBlock has')
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        out = out + (x if self.downsample is None else self.downsample(x))
        return self.relu(out)


class Bottleneck(nn.Module):
    """1x1, 3x3, 1x1 with expansion 4 (arcface_arch.py:103-146).  Host only."""
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * self.expansion, kernel_size=1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        if x.is_cuda:
            raise NotImplementedError('Bottleneck has no HIP path (ResNetArcFace cannot instantiate it); IRBlock has')
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        out = out + (x if self.downsample is None else self.downsample(x))
        return self.relu(out)


class SEBlock(HipModule):
    """x * sigmoid(fc2(prelu(fc1(mean(x))))) (arcface_arch.py:149-168)."""

    def __init__(self, channel, reduction=16):
        super().__init__()
        self.avg_pool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Sequential(nn.Linear(channel, channel // reduction), nn.PReLU(), nn.Linear(channel // reduction, channel), nn.Sigmoid())

    def gate_hip(self, x):
        """(B,H,W,C) -> the (B,C) gate."""
        fc1, act, fc2 = self.fc[0], self.fc[1], self.fc[2]
        return ops.se_gate(ops.se_pool(x), fc1.weight.detach(), fc1.bias.detach(), prelu_slope(self, act), fc2.weight.detach(), fc2.bias.detach())

    def gate_host(self, x):
        b, c = x.shape[:2]
        return self.fc(self.avg_pool(x).view(b, c))

    def forward_host(self, x):
        b, c = x.shape[:2]
        return x * self.gate_host(x).view(b, c, 1, 1)

    def forward_nhwc(self, x):
        # alone, the block is the scale: no residual, and prelu(t, 1) is t
        return ops.se_scale_res_prelu(x, self.gate_hip(x), None, 1.0)


class IRBlock(HipModule):
    """bn0, conv1, bn1, prelu, conv2 (stride), bn2, [SE], + shortcut, prelu -- one PReLU module for both activations
    (arcface_arch.py:56-100)."""
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None, use_se=True):
        super().__init__()
        self.bn0 = nn.BatchNorm2d(inplanes)
        self.conv1 = conv3x3(inplanes, inplanes)
        self.bn1 = nn.BatchNorm2d(inplanes)
        self.prelu = nn.PReLU()
        self.conv2 = conv3x3(inplanes, planes, stride)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = downsample
        self.stride = stride
        self.use_se = use_se
        if self.use_se:
            self.se = SEBlock(planes)

    # -- folded parameters (dtype None: the parameters' own) -------------------------------------------------------------------------------
    def layer(self, which):
        """The folded.folded_layer 'conv1' | 'conv2' | 'shortcut' (the 1x1 as the centre tap of a 3x3)."""
        if which != 'shortcut':
            return folded_layer(getattr(self, which), getattr(self, 'bn' + which[-1]))
        conv, bn = self.downsample[0], self.downsample[1]
        if conv.kernel_size != (1, 1) or conv.bias is not None or conv.stride != (self.stride, self.stride):
            raise NotImplementedError('IRBlock shortcut: a bias-free 1x1 conv at the block stride, then BatchNorm2d')
        return folded_layer(conv, bn, embed3=True)

    def folded(self, dtype=None):
        """dict: pre (scale, shift) of bn0; conv1 / conv2 (weight, bias) with bn1 / bn2 folded; shortcut (3x3 centre-tap weight, bias) or None."""
        return {'pre': bn_affine(self.bn0, dtype), 'conv1': self.layer('conv1')[0](dtype), 'conv2': self.layer('conv2')[0](dtype),
                'shortcut': None if self.downsample is None else self.layer('shortcut')[0](dtype)}

    def forward_folded(self, x):
        """The device dataflow on stock torch ops (NCHW), in the parameters' dtype."""
        f = self.folded()
        a = self.prelu.weight.detach().reshape(-1)[0]
        s, t = f['pre']
        h = F.conv2d(x * s.view(1, -1, 1, 1) + t.view(1, -1, 1, 1), *f['conv1'], padding=1)
        h = torch.where(h > 0, h, a * h)
        h = F.conv2d(h, *f['conv2'], stride=self.stride, padding=1)
        res = x if f['shortcut'] is None else F.conv2d(x, *f['shortcut'], stride=self.stride, padding=1)
        if self.use_se:
            b, c = h.shape[:2]
            h = h * self.se.gate_host(h).view(b, c, 1, 1)
        h = h + res
        return torch.where(h > 0, h, a * h)

    # -- HIP -------------------------------------------------------------------------------------------------------------------------------
    def _pre_tables(self, batch):
        """bn0 as the (batch, C) scale / shift tables of CF_PRO_AFFINE.  Every row is the same: a table of 16 rows, or of the next power of
        two above a larger batch, is cached and the batch takes its first rows (a contiguous slice: no launch)."""
        rows = max(16, 1 << (batch - 1).bit_length())

        def build():
            s, t = bn_affine(self.bn0, torch.float64)
            return s.float().expand(rows, -1).contiguous(), t.float().expand(rows, -1).contiguous()
        s, t = self._packed(('pre', rows), build, *bn_deps(self.bn0))
        return s[:batch], t[:batch]

    def run_hip(self, x):
        need_eval(self)
        a = prelu_slope(self, self.prelu)
        s, t = self._pre_tables(x.shape[0])
        h = conv_hip(self, ('w', 'conv1'), self.layer('conv1'), x, slope=a, prologue=ops.PRO_AFFINE, scale=s, shift=t)
        res = x if self.downsample is None else conv_hip(self, ('w', 'shortcut'), self.layer('shortcut'), x, stride=self.stride)
        if not self.use_se:
            return conv_hip(self, ('w', 'conv2'), self.layer('conv2'), h, stride=self.stride, res=res, slope=a)
        h = conv_hip(self, ('w', 'conv2'), self.layer('conv2'), h, stride=self.stride)
        return ops.se_scale_res_prelu(h, self.se.gate_hip(h), res, a)

    def forward_host(self, x):
        out = self.prelu(self.bn1(self.conv1(self.bn0(x))))
        out = self.bn2(self.conv2(out))
        if self.use_se:
            out = self.se.forward_host(out)
        out = out + (x if self.downsample is None else self.downsample(x))
        return self.prelu(out)

    def forward_nhwc(self, x):
        return self.run_hip(x)


@ARCH_REGISTRY.register()
class ResNetArcFace(HipModule):
    """ArcFace embedding network: (B,1,128,128) gray in [-1,1] -> (B,512) (arcface_arch.py:171-245).

    block: 'IRBlock' (a block class is accepted as the reference accepts it); layers: blocks per stage; use_se: SEBlock in every block."""

    def __init__(self, block, layers, use_se=True):
        if block == 'IRBlock':
            block = IRBlock
        self.inplanes = 64
        self.use_se = use_se
        super().__init__()
        self.conv1 = nn.Conv2d(1, 64, kernel_size=3, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.prelu = nn.PReLU()
        self.maxpool = nn.MaxPool2d(kernel_size=2, stride=2)
        self.layer1 = self._make_layer(block, 64, layers[0])
        self.layer2 = self._make_layer(block, 128, layers[1], stride=2)
        self.layer3 = self._make_layer(block, 256, layers[2], stride=2)
        self.layer4 = self._make_layer(block, 512, layers[3], stride=2)
        self.bn4 = nn.BatchNorm2d(512)
        self.dropout = nn.Dropout()
        self.fc5 = nn.Linear(512 * 8 * 8, 512)
        self.bn5 = nn.BatchNorm1d(512)
        # the reference's initialisation, in its module order (same RNG consumption)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.xavier_normal_(m.weight)
            elif isinstance(m, (nn.BatchNorm2d, nn.BatchNorm1d)):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.Linear):
                nn.init.xavier_normal_(m.weight)
                nn.init.constant_(m.bias, 0)

    def _make_layer(self, block, planes, num_blocks, stride=1):
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(nn.Conv2d(self.inplanes, planes * block.expansion, kernel_size=1, stride=stride, bias=False),
                                       nn.BatchNorm2d(planes * block.expansion))
        blocks = [block(self.inplanes, planes, stride, downsample, use_se=self.use_se)]
        self.inplanes = planes
        blocks += [block(self.inplanes, planes, use_se=self.use_se) for _ in range(1, num_blocks)]
        return nn.Sequential(*blocks)

    def _blocks(self):
        return [b for layer in (self.layer1, self.layer2, self.layer3, self.layer4) for b in layer]

    # -- folded parameters -------------------------------------------------------------------------------------------------------------------
    def folded_tail(self, dtype=None):
        """(weight (512, 32768), bias) of bn5(fc5(flatten(bn4(x)))) on the CHANNELS-LAST flattening (h*8 + w)*512 + c of x."""
        dtype = dtype or self.fc5.weight.dtype
        s4, t4 = bn_affine(self.bn4, dtype)
        s5, t5 = bn_affine(self.bn5, dtype)
        n, c = self.fc5.out_features, self.bn4.num_features
        w = self.fc5.weight.detach().to(dtype).view(n, c, -1).permute(0, 2, 1)   # [n][h*8 + w][c]
        bias = self.fc5.bias.detach().to(dtype) + (w * t4).sum(dim=(1, 2))
        w = (w * s4).reshape(n, -1)
        return (w * s5.view(-1, 1)).contiguous(), (bias * s5 + t5).contiguous()

    def forward_folded(self, x):
        """The device dataflow on stock torch ops, in the parameters' dtype."""
        a = self.prelu.weight.detach().reshape(-1)[0]
        h = F.conv2d(x, *fold_conv_bn(self.conv1, self.bn1), padding=1)
        h = F.max_pool2d(torch.where(h > 0, h, a * h), 2, 2)
        for blk in self._blocks():
            h = blk.forward_folded(h)
        w, b = self.folded_tail()
        return F.linear(h.permute(0, 2, 3, 1).reshape(h.shape[0], -1), w, b)

    # -- HIP -------------------------------------------------------------------------------------------------------------------------------
    def check_device_call(self, shape):
        """What the HIP path refuses, before it touches a device: training mode (RuntimeError), any input but (B,1,128,128) (ValueError)."""
        need_eval(self)
        if len(shape) != 4 or tuple(shape[1:]) != (1, IN_SIZE, IN_SIZE) or shape[0] < 1:
            raise ValueError(f'ResNetArcFace on HIP takes (B,1,{IN_SIZE},{IN_SIZE}) (fc5 fixes the size), got {tuple(shape)}')
        for blk in self._blocks():
            if not isinstance(blk, IRBlock):
                raise NotImplementedError(f'HIP path: IRBlock stages, got {type(blk).__name__}')

    def forward_hip(self, x):
        self.check_device_call(x.shape)

        def tail():
            w, b = self.folded_tail(torch.float64)
            return ops.pack_fc_rows(w.float()), b.float().contiguous()
        h = conv_hip(self, 'stem', folded_layer(self.conv1, self.bn1), x.float().contiguous(), in_nchw=True)
        h = ops.prelu_maxpool2(h, prelu_slope(self, self.prelu))
        for blk in self._blocks():
            h = blk.run_hip(h)
        wp, bias = self._packed('tail', tail, self.fc5.weight, self.fc5.bias, *bn_deps(self.bn4), *bn_deps(self.bn5))
        return ops.fc_rows(h.view(h.shape[0], -1), wp, bias)

    def forward_host(self, x):
        x = self.maxpool(self.prelu(self.bn1(self.conv1(x))))
        for blk in self._blocks():   # (stock torch ops on whatever device x lies: a block's own forward would pick the HIP path there)
            x = blk.forward_host(x) if isinstance(blk, HipModule) else blk(x)
        x = self.dropout(self.bn4(x))
        return self.bn5(self.fc5(x.view(x.size(0), -1)))

    def forward(self, x):
        if x.is_cuda:
            ops.L.ensure_device(x.device)
            with torch.no_grad(), torch.cuda.device(x.device):
                return self.forward_hip(x)   # (refuses training mode and other input sizes before its first launch)
        return self.forward_host(x)
