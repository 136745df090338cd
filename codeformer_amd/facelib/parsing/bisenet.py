"""BiSeNet -- the face parser `init_parsing_model` names by default (reference: facelib/parsing/bisenet.py:8-140) -- on the HIP kernels.

Same classes, constructor arguments, module tree and `state_dict` keys as the reference (191 entries, 13 300 416 parameters), so a reference
checkpoint loads with strict=True.  forward(x, return_feat=False) returns what the reference returns: (out, out16, out32) -- three
(B,num_class,H,W) float32 logit maps -- and with return_feat also the three mid features at full size.  Nothing here is used by
CodeFormer.forward.  No trained `parsing_bisenet.pth` ships with or was run through this code: every figure quoted for it is on seeded random
weights.

CPU tensors run `forward_host` (stock torch ops: the reference's forward, any size).  CUDA tensors run the device dataflow, value-only, eval
mode, channels-last fp32 with IEEE-fp32 MFMA operands (ops.pack_weight defaults):
  * ResNet18: see resnet.py (7x7 stem kernel, 3x3 / stride-2 max-pool, BasicBlocks on ops.conv2d with BatchNorm folded);
  * AttentionRefinementModule: 3x3 conv + bn + ReLU (folded.conv_hip), cf_se_pool,
    then the single-layer gate sigmoid(W'p + b') with bn_atten folded (cf_pooled_fc).  arm32: feat * gate + the per-image conv_avg row
    (cf_scale_add_row; the nearest upsampling of a 1x1 map is a row broadcast); arm16: feat * gate + feat32_up (cf_se_scale_res_prelu, slope 1);
  * conv_avg: the 1x1 conv + bn + ReLU on the pooled feat32 is cf_pooled_fc with ReLU;
  * conv_head32 / conv_head16: nearest interpolation to the next level + 3x3 pad 1 is the folded sub-pixel form (ops.conv2d(upsample=True,
    pad_mode=PAD_ZERO) on an up2x packing; chains of 4 * 128 products), followed by cf_relu in place: the sub-pixel instantiations have no
    ReLU epilogue.  The form holds only when every level is exactly x2: the device path takes H % 32 == 0 and W % 32 == 0 (H, W >= 32) and
    raises ValueError otherwise;
  * FeatureFusionModule: convblk is a 1x1 conv over the two-pointer concat (x2=), cf_se_pool, cf_se_gate with zero biases and slope 0
    (conv1, ReLU, conv2, sigmoid), cf_se_scale_res_prelu(feat, gate, feat, 1): feat * gate + feat;
  * BiSeNetOutput: 3x3 + bn + ReLU, then the bias-free 1x1 to num_class channels padded with zero rows to a multiple of 4 (19 -> 20);
  * the two 1x1 convolutions (conv1x1_hip): the 1x1 kernel tiles an image's pixels by 128 or 256 and its channels by 64, so convblk runs on
    it (then cf_relu in place) when the 1/8 level has a multiple of 256 pixels -- a 512x512 face has 4096 -- and otherwise, like the 20 class
    maps always, as the centre tap of a 3x3 on the general kernel (ReLU in the epilogue there).  The rule reads the per-image shape only;
  * outputs: cf_resize_bilinear_ac (align_corners=True) writes NCHW from the channels-last maps, the padding channel left out.
`parse_labels(x)` runs the `out` head only and takes the argmax inside the resize kernel (cf_resize_bilinear_ac_argmax): the num_class x H x W
floats are never stored.  `forward_folded` restates the device dataflow with stock torch ops in the parameters' dtype.
The sub-modules (resnet.NetPart) run on the device inside the network only, channels-last through `run_hip`; called alone they take CPU
tensors and refuse CUDA tensors.
"""
import torch
from torch import nn
from torch.nn import functional as F

from ... import ops
from ...archs.folded import bn_deps, centre_tap, conv_hip, fold_conv_bn, folded_layer, need_eval
from ...archs.hip_module import HipModule
from .resnet import NetPart, ResNet18

LEVEL = 32   # the device path takes heights and widths that are multiples of it: every nearest interpolation is then exactly x2


def up2x_conv_folded(x, w, b):
    """conv3x3(pad 1)(nearest x2 (x)) as the four 2x2 sub-pixel convolutions the device runs (ops.fold_phase_taps), on stock torch ops."""
    B, _, H, W = x.shape
    xp = F.pad(x, (1, 1, 1, 1))
    out = x.new_empty(B, w.shape[0], 2 * H, 2 * W)
    for a in (0, 1):
        for c in (0, 1):
            out[:, :, a::2, c::2] = F.conv2d(xp[:, :, a:a + H + 1, c:c + W + 1], ops.fold_phase_taps(w, a, c), b)
    return out


def conv1x1_hip(mod, key, layer, x, x2=None, relu=False):
    """[relu](1x1 conv) of channels-last x (x2 concatenated after it); layer: a folded.folded_layer with a (cout,cin,1,1) weight, cout % 4 == 0.
    The 1x1 kernel tiles the pixels of an image by 128 or 256 and the channels by 64: it takes images of a multiple of 256 pixels and cout % 64
    == 0 (512x512 faces: 4096 pixels at 1/8); it has no activation epilogue (cf_relu follows, in place).  Anything else -- the 20 class maps,
    small or odd-sized levels -- runs on the general 3x3 kernel with the weight as the centre tap.  The rule reads the per-image shape only."""
    fold, deps = layer
    if (x.shape[1] * x.shape[2]) % 256 != 0 or deps[0].shape[0] % 64 != 0:
        def fold3():
            w, b = fold()
            return centre_tap(w), b
        return conv_hip(mod, (key, True), (fold3, deps), x, x2=x2, slope=0.0 if relu else None)

    def build():
        w, b = fold()
        return ops.pack_weight(w.float(), None if b is None else b.float())
    y = ops.conv2d(x, mod._packed((key, False), build, *deps), x2=x2)
    return ops.relu(y, inplace=True) if relu else y


class ConvBNReLU(NetPart):
    """conv (no bias) + BatchNorm + ReLU (bisenet.py:8-18)."""

    def __init__(self, in_chan, out_chan, ks=3, stride=1, padding=1):
        super().__init__()
        self.conv = nn.Conv2d(in_chan, out_chan, kernel_size=ks, stride=stride, padding=padding, bias=False)
        self.bn = nn.BatchNorm2d(out_chan)

    def layer(self):
        return folded_layer(self.conv, self.bn)

    def folded(self, dtype=None):
        return self.layer()[0](dtype)

    def forward_folded(self, x, up2x=False):
        w, b = self.folded()
        if up2x:
            return F.relu(up2x_conv_folded(x, w, b))
        return F.relu(F.conv2d(x, w, b, stride=self.conv.stride, padding=self.conv.padding))

    def run_hip(self, x, up2x=False, x2=None):
        """Channels-last.  up2x: nearest x2 first; x2: a second tensor concatenated after x (1x1 only)."""
        need_eval(self)
        ks, st, pad = self.conv.kernel_size, self.conv.stride, self.conv.padding
        if ks == (1, 1) and st == (1, 1) and pad == (0, 0) and not up2x:
            return conv1x1_hip(self, 'w1x1', self.layer(), x, x2=x2, relu=True)
        if ks != (3, 3) or pad != (1, 1) or st not in ((1, 1), (2, 2)) or x2 is not None or (up2x and st != (1, 1)):
            raise NotImplementedError(f'ConvBNReLU on HIP: 3x3 pad 1 at stride 1 or 2, or 1x1 pad 0 at stride 1; got ks {ks}, stride {st}, padding {pad}')
        return conv_hip(self, 'w', self.layer(), x, stride=st[0], up2x=up2x, slope=0.0)

    def fc_hip(self, pooled):
        """A 1x1 ConvBNReLU on a 1x1 map: (B,C) pooled rows -> (B,out_chan)."""
        need_eval(self)
        if self.conv.kernel_size != (1, 1):
            raise NotImplementedError('ConvBNReLU.fc_hip: a 1x1 convolution')

        def build():
            w, b = self.folded(torch.float64)
            return w.float().flatten(1).contiguous(), b.float().contiguous()
        return ops.pooled_fc(pooled, *self._packed('fc', build, *self.layer()[1]), act='relu')

    def forward_host(self, x):
        return F.relu(self.bn(self.conv(x)))


class BiSeNetOutput(NetPart):
    """3x3 ConvBNReLU, then a bias-free 1x1 to the classes; returns (logits, mid feature) (bisenet.py:21-31)."""

    def __init__(self, in_chan, mid_chan, num_class):
        super().__init__()
        self.conv = ConvBNReLU(in_chan, mid_chan, ks=3, stride=1, padding=1)
        self.conv_out = nn.Conv2d(mid_chan, num_class, kernel_size=1, bias=False)

    @property
    def num_class(self):
        return self.conv_out.out_channels

    def forward_folded(self, x):
        feat = self.conv.forward_folded(x)
        return F.conv2d(feat, self.conv_out.weight.detach()), feat

    def run_hip(self, x):
        """(logits (B,h,w,num_class padded to a multiple of 4 with zero channels), feat (B,h,w,mid_chan)), channels-last."""
        feat = self.conv.run_hip(x)

        def fold():
            w = self.conv_out.weight.detach().float()
            pad = (w.shape[0] + 3) // 4 * 4 - w.shape[0]
            return (torch.cat([w, w.new_zeros((pad,) + tuple(w.shape[1:]))], 0) if pad else w), None
        return conv1x1_hip(self, 'out', (fold, [self.conv_out.weight]), feat), feat

    def forward_host(self, x):
        feat = self.conv.forward_host(x)
        return self.conv_out(feat), feat

class AttentionRefinementModule(NetPart):
    """feat = ConvBNReLU(x); feat * sigmoid(bn_atten(conv_atten(mean(feat)))) (bisenet.py:34-50)."""

    def __init__(self, in_chan, out_chan):
        super().__init__()
        self.conv = ConvBNReLU(in_chan, out_chan, ks=3, stride=1, padding=1)
        self.conv_atten = nn.Conv2d(out_chan, out_chan, kernel_size=1, bias=False)
        self.bn_atten = nn.BatchNorm2d(out_chan)
        self.sigmoid_atten = nn.Sigmoid()

    def folded_gate(self, dtype=None):
        """(weight (out,out), bias) of bn_atten(conv_atten(.)) on a pooled row."""
        w, b = fold_conv_bn(self.conv_atten, self.bn_atten, dtype)
        return w.flatten(1).contiguous(), b

    def gate_host(self, feat):
        """The (B,C) gate of an NCHW feat, from the folded single layer, in the parameters' dtype."""
        return torch.sigmoid(F.linear(feat.mean(dim=(2, 3)), *self.folded_gate()))

    def forward_folded(self, x, add):
        """feat * gate + add (add: an NCHW tensor, or (B,C,1,1) rows)."""
        feat = self.conv.forward_folded(x)
        return feat * self.gate_host(feat)[:, :, None, None] + add

    def feat_gate_hip(self, x):
        """Channels-last x -> (feat (B,h,w,C), gate (B,C))."""
        need_eval(self)
        feat = self.conv.run_hip(x)

        def build():
            w, b = self.folded_gate(torch.float64)
            return w.float().contiguous(), b.float().contiguous()
        w, b = self._packed('gate', build, self.conv_atten.weight, *bn_deps(self.bn_atten))
        return feat, ops.pooled_fc(ops.se_pool(feat), w, b, act='sigmoid')

    def forward_host(self, x):
        feat = self.conv.forward_host(x)
        atten = F.avg_pool2d(feat, feat.size()[2:])
        atten = self.sigmoid_atten(self.bn_atten(self.conv_atten(atten)))
        return torch.mul(feat, atten)

class ContextPath(NetPart):
    """ResNet18, two attention refinements and the global-average row, merged top-down; returns (feat8, feat_cp8, feat_cp16)
    (bisenet.py:53-84)."""

    def __init__(self):
        super().__init__()
        self.resnet = ResNet18()
        self.arm16 = AttentionRefinementModule(256, 128)
        self.arm32 = AttentionRefinementModule(512, 128)
        self.conv_head32 = ConvBNReLU(128, 128, ks=3, stride=1, padding=1)
        self.conv_head16 = ConvBNReLU(128, 128, ks=3, stride=1, padding=1)
        self.conv_avg = ConvBNReLU(512, 128, ks=1, stride=1, padding=0)

    def forward_folded(self, x):
        feat8, feat16, feat32 = self.resnet.forward_folded(x)
        w, b = self.conv_avg.folded()
        avg = F.relu(F.linear(feat32.mean(dim=(2, 3)), w.flatten(1), b))
        feat32_up = self.conv_head32.forward_folded(self.arm32.forward_folded(feat32, avg[:, :, None, None]), up2x=True)
        feat16_up = self.conv_head16.forward_folded(self.arm16.forward_folded(feat16, feat32_up), up2x=True)
        return feat8, feat16_up, feat32_up

    def run_hip(self, x):
        """NCHW image -> the three tensors, channels-last."""
        feat8, feat16, feat32 = self.resnet.run_hip(x)
        avg = self.conv_avg.fc_hip(ops.se_pool(feat32))
        feat, gate = self.arm32.feat_gate_hip(feat32)
        feat32_up = self.conv_head32.run_hip(ops.scale_add_row(feat, gate, avg), up2x=True)
        feat, gate = self.arm16.feat_gate_hip(feat16)
        feat16_up = self.conv_head16.run_hip(ops.se_scale_res_prelu(feat, gate, feat32_up, 1.0), up2x=True)
        return feat8, feat16_up, feat32_up

    def forward_host(self, x):
        feat8, feat16, feat32 = self.resnet.forward_host(x)
        avg = self.conv_avg.forward_host(F.avg_pool2d(feat32, feat32.size()[2:]))
        avg_up = F.interpolate(avg, feat32.size()[2:], mode='nearest')
        feat32_sum = self.arm32.forward_host(feat32) + avg_up
        feat32_up = self.conv_head32.forward_host(F.interpolate(feat32_sum, feat16.size()[2:], mode='nearest'))
        feat16_sum = self.arm16.forward_host(feat16) + feat32_up
        feat16_up = self.conv_head16.forward_host(F.interpolate(feat16_sum, feat8.size()[2:], mode='nearest'))
        return feat8, feat16_up, feat32_up

class FeatureFusionModule(NetPart):
    """feat = ConvBNReLU 1x1 of cat(fsp, fcp); feat * sigmoid(conv2(relu(conv1(mean(feat))))) + feat (bisenet.py:87-107)."""

    def __init__(self, in_chan, out_chan):
        super().__init__()
        self.convblk = ConvBNReLU(in_chan, out_chan, ks=1, stride=1, padding=0)
        self.conv1 = nn.Conv2d(out_chan, out_chan // 4, kernel_size=1, stride=1, padding=0, bias=False)
        self.conv2 = nn.Conv2d(out_chan // 4, out_chan, kernel_size=1, stride=1, padding=0, bias=False)
        self.relu = nn.ReLU(inplace=True)
        self.sigmoid = nn.Sigmoid()

    def forward_folded(self, fsp, fcp):
        feat = self.convblk.forward_folded(torch.cat([fsp, fcp], dim=1))
        hid = F.relu(F.linear(feat.mean(dim=(2, 3)), self.conv1.weight.detach().flatten(1)))
        gate = torch.sigmoid(F.linear(hid, self.conv2.weight.detach().flatten(1)))
        return feat * gate[:, :, None, None] + feat

    def run_hip(self, fsp, fcp):
        feat = self.convblk.run_hip(fsp, x2=fcp)

        def build():
            w1, w2 = self.conv1.weight.detach().float().flatten(1).contiguous(), self.conv2.weight.detach().float().flatten(1).contiguous()
            return w1, w1.new_zeros(w1.shape[0]), w2, w2.new_zeros(w2.shape[0])
        w1, b1, w2, b2 = self._packed('gate', build, self.conv1.weight, self.conv2.weight)
        gate = ops.se_gate(ops.se_pool(feat), w1, b1, 0.0, w2, b2)
        return ops.se_scale_res_prelu(feat, gate, feat, 1.0)

    def forward_host(self, fsp, fcp):
        feat = self.convblk.forward_host(torch.cat([fsp, fcp], dim=1))
        atten = F.avg_pool2d(feat, feat.size()[2:])
        atten = self.sigmoid(self.conv2(self.relu(self.conv1(atten))))
        return torch.mul(feat, atten) + feat

def check_size(mod, shape):
    """What the device path refuses before it touches a device: training mode (RuntimeError), anything but (B,3,H,W) with H and W multiples
    of 32 (ValueError)."""
    need_eval(mod)
    if len(shape) != 4 or shape[1] != 3 or shape[0] < 1 or shape[2] < LEVEL or shape[3] < LEVEL or shape[2] % LEVEL or shape[3] % LEVEL:
        raise ValueError(f'BiSeNet on HIP takes (B,3,H,W) with H % {LEVEL} == 0 and W % {LEVEL} == 0 (H, W >= {LEVEL}: every level of the context '
                         f'path is then exactly x2 of the next), got {tuple(shape)}; forward_host takes any size')


class BiSeNet(HipModule):
    """(B,3,H,W) RGB, normalised as the caller's checkpoint expects -> (out, out16, out32) logits (B,num_class,H,W), and with return_feat the
    three mid features at full size as well (bisenet.py:110-140)."""

    def __init__(self, num_class):
        super().__init__()
        self.cp = ContextPath()
        self.ffm = FeatureFusionModule(256, 256)
        self.conv_out = BiSeNetOutput(256, 256, num_class)
        self.conv_out16 = BiSeNetOutput(128, 64, num_class)
        self.conv_out32 = BiSeNetOutput(128, 64, num_class)

    def check_device_call(self, shape):
        check_size(self, shape)

    def forward_folded(self, x, return_feat=False):
        """The device dataflow on stock torch ops, in the parameters' dtype."""
        size = x.shape[2:]
        feat_res8, feat_cp8, feat_cp16 = self.cp.forward_folded(x)
        heads = [self.conv_out.forward_folded(self.ffm.forward_folded(feat_res8, feat_cp8)), self.conv_out16.forward_folded(feat_cp8),
                 self.conv_out32.forward_folded(feat_cp16)]
        outs = [h[0] for h in heads] + ([h[1] for h in heads] if return_feat else [])
        return tuple(F.interpolate(t, size, mode='bilinear', align_corners=True) for t in outs)

    def _fuse_hip(self, x):
        """NCHW image -> (feat_fuse, feat_cp8, feat_cp16), channels-last."""
        self.check_device_call(x.shape)
        feat_res8, feat_cp8, feat_cp16 = self.cp.run_hip(x)
        return self.ffm.run_hip(feat_res8, feat_cp8), feat_cp8, feat_cp16

    def forward_hip(self, x, return_feat=False):
        size = x.shape[2:]
        fuse, feat_cp8, feat_cp16 = self._fuse_hip(x)
        heads = [self.conv_out.run_hip(fuse), self.conv_out16.run_hip(feat_cp8), self.conv_out32.run_hip(feat_cp16)]
        n = self.conv_out.num_class
        outs = [ops.resize_bilinear_ac(h[0], size, c=n) for h in heads]
        if return_feat:
            outs += [ops.resize_bilinear_ac(h[1], size) for h in heads]
        return tuple(outs)

    @torch.no_grad()
    def parse_labels(self, x):
        """argmax over the classes of `out` per pixel, (B,H,W) int64.  On CUDA tensors only the `out` head runs (out16 / out32 are not
        computed) and the argmax is taken inside the resize kernel: the (B,num_class,H,W) logits are never stored."""
        if not x.is_cuda:
            return self.forward_host(x)[0].argmax(dim=1)
        self.check_device_call(x.shape)
        ops.L.ensure_device(x.device)
        with torch.cuda.device(x.device):
            out, _ = self.conv_out.run_hip(self._fuse_hip(x)[0])
            return ops.resize_bilinear_ac_argmax(out, x.shape[2:], c=self.conv_out.num_class)

    def forward_host(self, x, return_feat=False):
        size = x.size()[2:]
        feat_res8, feat_cp8, feat_cp16 = self.cp.forward_host(x)
        heads = [self.conv_out.forward_host(self.ffm.forward_host(feat_res8, feat_cp8)), self.conv_out16.forward_host(feat_cp8),
                 self.conv_out32.forward_host(feat_cp16)]
        outs = [h[0] for h in heads] + ([h[1] for h in heads] if return_feat else [])
        return tuple(F.interpolate(t, size, mode='bilinear', align_corners=True) for t in outs)

    def forward(self, x, return_feat=False):
        if x.is_cuda:
            self.check_device_call(x.shape)   # (before anything touches the device)
            ops.L.ensure_device(x.device)
            with torch.no_grad(), torch.cuda.device(x.device):
                return self.forward_hip(x, return_feat)
        return self.forward_host(x, return_feat)
