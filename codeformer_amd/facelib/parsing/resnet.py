"""ResNet18 -- the context path's backbone of BiSeNet (reference: facelib/parsing/resnet.py:5-69) -- on the HIP kernels.

Same classes, constructor arguments, attribute names and `state_dict` keys as the reference: conv1 / bn1 / maxpool, layer1 .. layer4 of two
BasicBlocks each, `downsample` a Sequential(conv 1x1, BatchNorm) where the shape changes.  forward(x) returns (feat8, feat16, feat32), the
outputs of layer2 / layer3 / layer4, NCHW float32.

Device dataflow (channels-last, fp32 tensors, IEEE-fp32 MFMA operands; no BatchNorm, ReLU or residual add of this file is a launch of its
own):
  * stem: cf_stem7x7s2 (7x7 / stride 2 / pad 3 on the NCHW image, bn1 folded in float64 and rounded once, ReLU in the epilogue), then
    cf_maxpool3s2 (3x3 / stride 2 / pad 1, padding -inf);
  * BasicBlock: conv1 + bn1 + ReLU and conv2 + bn2 + shortcut + ReLU are one ops.conv2d launch each on the general fp32 kernel (stride 2:
    one padded row / column on every side); ReLU is the PReLU epilogue with slope 0.0 (CF_EPI_PRELU / CF_EPI_RES_PRELU: x > 0 ? x : 0 * x);
  * the 1x1 stride-s `downsample` conv runs as a 3x3 stride-s conv whose only non-zero tap is the centre (folded.fold_conv_bn(embed3=True)):
    the eight other taps add 0 * x = 0 to a finite sum;
  * long accumulation chains: the general fp32 kernel adds all 9 * cin products of an output in one chain of MFMA accumulations, and layer3 /
    layer4 reach K = 4608.  VGGFeatureExtractor had to run such layers per 128 input channels to meet the 8x gate; here the gate does not need
    it.  Measured on the three fixture cases over all nine taps: worst e(device) / e(float32 reference) 3.18 with every layer whole, 2.75 with
    layers of more than 128 input channels in parts (profiles/NOTES.md), so every convolution is one launch.
`forward_folded` evaluates this dataflow with stock torch ops in the parameters' dtype (tests compare it in float64 with the unfolded module).
"""
import torch
from torch import nn
from torch.nn import functional as F

from ... import ops
from ...archs.folded import conv_hip, fold_conv_bn, folded_layer, need_eval, stem7x7_hip
from ...archs.hip_module import HipModule


def conv3x3(in_planes, out_planes, stride=1):
    """3x3 convolution, padding 1, no bias (resnet.py:5-7)."""
    return nn.Conv2d(in_planes, out_planes, kernel_size=3, stride=stride, padding=1, bias=False)


class NetPart(HipModule):
    """A sub-module of ResNet18 / BiSeNet.  On the device it runs inside the network, channels-last, through its `run_hip`; its own forward
    takes CPU tensors (forward_host: the reference's forward) and refuses CUDA tensors: there is no standalone device forward."""

    def forward(self, *xs):
        if xs[0].is_cuda:
            raise NotImplementedError(f'{type(self).__name__} has no device forward of its own: it runs inside ResNet18 / BiSeNet (run_hip, '
                                      'channels-last); CPU tensors take forward_host')
        return self.forward_host(*xs)


class BasicBlock(NetPart):
    """conv-bn-relu, conv-bn, + shortcut, relu (resnet.py:10-38)."""

    def __init__(self, in_chan, out_chan, stride=1):
        super().__init__()
        self.conv1 = conv3x3(in_chan, out_chan, stride)
        self.bn1 = nn.BatchNorm2d(out_chan)
        self.conv2 = conv3x3(out_chan, out_chan)
        self.bn2 = nn.BatchNorm2d(out_chan)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = None
        if in_chan != out_chan or stride != 1:
            self.downsample = nn.Sequential(nn.Conv2d(in_chan, out_chan, kernel_size=1, stride=stride, bias=False), nn.BatchNorm2d(out_chan))

    def layers(self):
        """The folded.folded_layer of conv1, conv2 and the shortcut (the 1x1 as the centre tap of a 3x3), the last None without a `downsample`."""
        sc = None if self.downsample is None else folded_layer(self.downsample[0], self.downsample[1], embed3=True)
        return {'conv1': folded_layer(self.conv1, self.bn1), 'conv2': folded_layer(self.conv2, self.bn2), 'shortcut': sc}

    def forward_folded(self, x):
        """The device dataflow on stock torch ops (NCHW), in the parameters' dtype."""
        f = {k: None if v is None else v[0](None) for k, v in self.layers().items()}   # (weight, bias) in the parameters' dtype
        s = self.conv1.stride[0]
        h = F.relu(F.conv2d(x, *f['conv1'], stride=s, padding=1))
        res = x if f['shortcut'] is None else F.conv2d(x, *f['shortcut'], stride=s, padding=1)
        return F.relu(F.conv2d(h, *f['conv2'], padding=1) + res)

    def run_hip(self, x):
        need_eval(self)
        s, ly = self.conv1.stride[0], self.layers()
        h = conv_hip(self, 'conv1', ly['conv1'], x, stride=s, slope=0.0)
        res = x if self.downsample is None else conv_hip(self, 'shortcut', ly['shortcut'], x, stride=s)
        return conv_hip(self, 'conv2', ly['conv2'], h, res=res, slope=0.0)

    def forward_host(self, x):
        residual = F.relu(self.bn1(self.conv1(x)))
        residual = self.bn2(self.conv2(residual))
        shortcut = x if self.downsample is None else self.downsample(x)
        return self.relu(shortcut + residual)


def create_layer_basic(in_chan, out_chan, bnum, stride=1):
    """bnum BasicBlocks, the first at `stride` (resnet.py:41-45)."""
    return nn.Sequential(BasicBlock(in_chan, out_chan, stride=stride), *[BasicBlock(out_chan, out_chan, stride=1) for _ in range(bnum - 1)])


class ResNet18(HipModule):
    """(B,3,H,W) -> (feat8 (B,128,H/8,W/8), feat16 (B,256,H/16,W/16), feat32 (B,512,H/32,W/32)) (resnet.py:48-69)."""

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = create_layer_basic(64, 64, bnum=2, stride=1)
        self.layer2 = create_layer_basic(64, 128, bnum=2, stride=2)
        self.layer3 = create_layer_basic(128, 256, bnum=2, stride=2)
        self.layer4 = create_layer_basic(256, 512, bnum=2, stride=2)

    def _layers(self, x, method):
        """layer1 .. layer4 through every block's `method` (a block's own forward would pick its path by the device); the last three outputs."""
        feats = []
        for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
            for blk in layer:
                x = getattr(blk, method)(x)
            feats.append(x)
        return tuple(feats[1:])

    def forward_folded(self, x):
        """The device dataflow on stock torch ops, in the parameters' dtype."""
        h = F.max_pool2d(F.relu(F.conv2d(x, *fold_conv_bn(self.conv1, self.bn1), stride=2, padding=3)), 3, 2, 1)
        return self._layers(h, 'forward_folded')

    def stem_hip(self, x):
        """(B,3,H,W) NCHW -> the stem's ReLU output (B,ceil(H/2),ceil(W/2),64) channels-last, before the max-pool."""
        need_eval(self)
        return stem7x7_hip(self, 'stem', self.conv1, self.bn1, x.float())

    def run_hip(self, x):
        """NCHW image -> the three features, channels-last."""
        return self._layers(ops.maxpool3s2(self.stem_hip(x)), 'run_hip')

    def forward_host(self, x):
        x = self.maxpool(F.relu(self.bn1(self.conv1(x))))
        return self._layers(x, 'forward_host')

    def forward(self, x):
        if x.is_cuda:
            ops.L.ensure_device(x.device)
            with torch.no_grad(), torch.cuda.device(x.device):
                return tuple(ops.to_nchw(f) for f in self.run_hip(x))
        return self.forward_host(x)
