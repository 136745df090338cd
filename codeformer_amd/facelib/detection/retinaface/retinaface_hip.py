"""The RetinaFace ResNet-50 detector on the HIP kernels: the `backend='hip'` half of retinaface.RetinaFace.

Device dataflow (channels-last, fp32 tensors, IEEE-fp32 MFMA operands; BatchNorm folded in float64 and rounded once; no BatchNorm, ReLU,
residual add or concat is a launch of its own):
  * trunk: cf_stem7x7s2 + cf_maxpool3s2, then per Bottleneck at most four launches -- conv1 (1x1) + ReLU and conv3 (1x1) + shortcut + ReLU on
    cf_pointwise, conv2 (3x3, stride 1 or 2, any size) + ReLU on the general fp32 3x3 kernel, the `downsample` (1x1 at the block's stride) on
    cf_pointwise reading every second pixel;
  * FPN: the lateral 1x1 layers + ReLU on cf_pointwise, `o + nearest(coarser -> o's size)` in cf_nearest_add, merge1 / merge2 3x3 + ReLU;
  * SSH: the five 3x3 layers write channel slices of ONE 256-channel buffer (ops.conv2d(out=buf[..., a:b])); the final ReLU is each branch's
    epilogue (relu(cat) = cat(relu)); conv5X5_1 feeds two convolutions and keeps its own ReLU;
  * heads: per level the three 1x1 heads as ONE 32-column cf_pointwise launch, an anchor's 16 values (4 box, 2 class, 10 landmark) together;
  * cf_retina_decode: softmax, decode / decode_landm against the cached device priors, the scale / resize products and the score threshold;
    only the passing rows leave the device.  More passing anchors than HipDetector.CAP: the call takes the full tensors and the host code.
`forward_folded` evaluates the same dataflow on stock torch ops in the parameters' dtype (tests compare it in float64 with the module).
"""
import numpy as np
import torch
from torch.nn import functional as F

from .... import ops
from ....archs.folded import conv_hip, fold_conv_bn, folded_layer, pointwise_hip, stem7x7_hip
from ....archs.hip_module import HipModule
from .retinaface_utils import PriorBox

SSH_UNITS = ('conv3X3', 'conv5X5_1', 'conv5X5_2', 'conv7X7_2', 'conv7x7_3')


def hip_refusal(net):
    """Why `net` cannot run on the HIP backend (a sentence), or None."""
    if net.cfg['name'] != 'Resnet50':
        return f"the HIP detector is built for network_name='resnet50' (got {net.cfg['name']}: its depthwise convolutions have no kernel)"
    if net.half_inference:
        return 'the HIP detector computes in float32 (half=True asks for float16)'
    if net.phase == 'train' or net.training:
        return 'the HIP detector folds BatchNorm and applies the softmax: it needs eval mode and phase test'
    if net.device.type != 'cuda':
        return f'the HIP detector runs on a CUDA (ROCm) device, the module is on {net.device}'
    return None


def fold_heads(net, level, dtype=None):
    """(weight (32,cin), bias (32,)) of level `level`'s three heads as one layer: row 16 a + j of anchor a = box (j 0..3), class (4, 5), landmark (6..15)."""
    hb, hc, hl = (getattr(net, n)[level].conv1x1 for n in ('BboxHead', 'ClassHead', 'LandmarkHead'))
    dtype = dtype or hb.weight.dtype
    w, b = [], []
    for a in range(2):
        for conv, per in ((hb, 4), (hc, 2), (hl, 10)):
            w.append(conv.weight.detach().to(dtype)[a * per:(a + 1) * per, :, 0, 0])
            b.append(conv.bias.detach().to(dtype)[a * per:(a + 1) * per])
    return torch.cat(w).contiguous(), torch.cat(b).contiguous()


def _head_deps(net, level):
    return [p for n in ('BboxHead', 'ClassHead', 'LandmarkHead') for p in (getattr(net, n)[level].conv1x1.weight, getattr(net, n)[level].conv1x1.bias)]


def split_heads(heads):
    """Per-level (B,H,W,32) channels-last head outputs -> raw (bbox (B,n,4), class logits (B,n,2), landmarks (B,n,10))."""
    v = torch.cat([h.reshape(h.shape[0], -1, 16) for h in heads], dim=1)
    return v[..., 0:4], v[..., 4:6], v[..., 6:16]


def forward_folded(net, x):
    """The device dataflow on stock torch ops (NCHW), in the parameters' dtype: (bbox, softmax, landmarks) as RetinaFace.forward."""
    body, dt = net.body, x.dtype

    def cb(conv, bn, x, relu=True, res=None, **kw):
        y = F.conv2d(x, *fold_conv_bn(conv, bn, dt), **kw)
        y = y if res is None else y + res
        return F.relu(y) if relu else y

    def unit(u, x, relu):      # a ConvUnit through its own folded()
        y = F.conv2d(x, *u.folded(dt), padding=u[0].padding)
        return F.relu(y) if relu else y

    h = F.max_pool2d(cb(body.conv1, body.bn1, x, stride=2, padding=3), 3, 2, 1)
    taps = []
    for layer in (body.layer1, body.layer2, body.layer3, body.layer4):
        for blk in layer:
            s = blk.stride
            idt = h if blk.downsample is None else cb(blk.downsample[0], blk.downsample[1], h[:, :, ::s, ::s], relu=False)
            y = cb(blk.conv2, blk.bn2, cb(blk.conv1, blk.bn1, h), stride=s, padding=1)
            h = cb(blk.conv3, blk.bn3, y, res=idt)
        taps.append(h)
    fpn = net.fpn
    o1, o2, o3 = (unit(getattr(fpn, f'output{i + 1}'), t, True) for i, t in enumerate(taps[1:]))
    o2 = unit(fpn.merge2, o2 + F.interpolate(o3, size=o2.shape[2:], mode='nearest'), True)
    o1 = unit(fpn.merge1, o1 + F.interpolate(o2, size=o1.shape[2:], mode='nearest'), True)
    heads = []
    for lv, o in enumerate((o1, o2, o3)):
        ssh = getattr(net, f'ssh{lv + 1}')
        mid = unit(ssh.conv5X5_1, o, True)
        f = torch.cat([unit(ssh.conv3X3, o, True), unit(ssh.conv5X5_2, mid, True), unit(ssh.conv7x7_3, unit(ssh.conv7X7_2, mid, True), True)], dim=1)
        w, b = fold_heads(net, lv, dt)
        heads.append(F.conv2d(f, w[:, :, None, None], b).permute(0, 2, 3, 1))
    bbox, cls, ldm = split_heads(heads)
    return bbox.contiguous(), F.softmax(cls, dim=-1), ldm.contiguous()


class HipDetector(HipModule):
    """Runs a RetinaFace module's parameters through the HIP kernels.  Holds no parameter of its own (the module's `state_dict` is untouched);
    packed weights are cached per layer until a source parameter changes."""

    PRIOR_SIZES = 8   # image sizes whose priors stay cached (a clip of varying frame sizes must not grow the cache without bound)
    CAP = 1024   # rows of the compact buffer per image; more passing anchors than this take the full-tensor path

    def __init__(self, net):
        super().__init__()
        self.__dict__['net'] = net      # (not a registered child: the detector is an attribute of `net`)
        self.__dict__['_priors'] = {}

    # ---- layers: folded.folded_layer pairs, a ConvUnit's by its own layer() ---------------------------------------------------------------------
    def _block(self, key, blk, x):
        s = blk.stride
        idt = x
        if blk.downsample is not None:
            idt = ops.pointwise(x, pointwise_hip(self, (key, 'down'), folded_layer(blk.downsample[0], blk.downsample[1])), step=s)
        y = ops.pointwise(x, pointwise_hip(self, (key, 1), folded_layer(blk.conv1, blk.bn1)), relu=True)
        y = conv_hip(self, (key, 2), folded_layer(blk.conv2, blk.bn2), y, stride=s, slope=0.0)
        return ops.pointwise(y, pointwise_hip(self, (key, 3), folded_layer(blk.conv3, blk.bn3)), res=idt, relu=True)

    def _ssh(self, lv, x):
        ssh = getattr(self.net, f'ssh{lv + 1}')
        u = {n: getattr(ssh, n) for n in SSH_UNITS}
        for n, m in u.items():
            if m.slope not in (None, 0.0):
                raise NotImplementedError(f'HIP detector: SSH.{n} has LeakyReLU({m.slope}); the kernels fuse ReLU (out_channel > 64)')
        B, H, W, _ = x.shape
        c = u['conv3X3'][0].out_channels
        q = u['conv5X5_2'][0].out_channels
        buf = torch.empty((B, H, W, c + 2 * q), dtype=torch.float32, device=x.device)

        def run(n, x, out=None):
            return conv_hip(self, ('ssh', lv, n), u[n].layer(), x, slope=0.0, out=out)
        run('conv3X3', x, buf[..., :c])
        mid = run('conv5X5_1', x)
        run('conv5X5_2', mid, buf[..., c:c + q])
        run('conv7x7_3', run('conv7X7_2', mid), buf[..., c + q:])
        return buf

    def heads(self, x):
        """(B,3,H,W) mean-subtracted float32 image on the device -> the three levels' (B,H_l,W_l,32) head outputs."""
        net = self.net
        why = hip_refusal(net)
        if why:
            raise NotImplementedError(why)
        if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f'HIP detector: a float32 (B,3,H,W) CUDA tensor, got {x.dtype} {tuple(x.shape)} on {x.device}')
        body = net.body
        h = ops.maxpool3s2(stem7x7_hip(self, 'stem', body.conv1, body.bn1, x))
        taps = []
        for li, layer in enumerate((body.layer1, body.layer2, body.layer3, body.layer4)):
            for bi, blk in enumerate(layer):
                h = self._block(('body', li, bi), blk, h)
            taps.append(h)
        fpn = net.fpn
        for n in ('output1', 'output2', 'output3', 'merge1', 'merge2'):
            if getattr(fpn, n).slope != 0.0:
                raise NotImplementedError(f'HIP detector: FPN.{n} has LeakyReLU({getattr(fpn, n).slope}); the kernels fuse ReLU (out_channel > 64)')
        o1, o2, o3 = (ops.pointwise(t, pointwise_hip(self, ('fpn', i), getattr(fpn, f'output{i + 1}').layer()), relu=True) for i, t in enumerate(taps[1:]))
        o2 = conv_hip(self, ('fpn', 'merge2'), fpn.merge2.layer(), ops.nearest_add(o2, o3), slope=0.0)
        o1 = conv_hip(self, ('fpn', 'merge1'), fpn.merge1.layer(), ops.nearest_add(o1, o2), slope=0.0)
        out = []
        for lv, o in enumerate((o1, o2, o3)):
            head = (lambda lv=lv: fold_heads(net, lv, torch.float64)), _head_deps(net, lv)
            out.append(ops.pointwise(self._ssh(lv, o), pointwise_hip(self, ('heads', lv), head)))
        return out

    def priors(self, h, w, device):
        """(PriorBox(...).forward(), scale [w, h] * 2, scale1 [w, h] * 5) of an h x w image as device tensors; the last PRIOR_SIZES sizes are kept."""
        key = (int(h), int(w), str(device))
        ent = self._priors.pop(key, None)
        if ent is None:
            wh = [float(w), float(h)]
            ent = (PriorBox(self.net.cfg, image_size=(int(h), int(w))).forward().to(device).contiguous(),
                   torch.tensor(wh * 2, dtype=torch.float32, device=device), torch.tensor(wh * 5, dtype=torch.float32, device=device))
        self._priors[key] = ent                         # (a dict keeps insertion order: the entry used last sits at the end)
        while len(self._priors) > self.PRIOR_SIZES:
            del self._priors[next(iter(self._priors))]    # the one unused for longest
        return ent

    def forward(self, x):
        """What RetinaFace.forward returns: (bbox (B,n,4), softmax (B,n,2), landmarks (B,n,10))."""
        ops.L.ensure_device(x.device)
        with torch.no_grad(), torch.cuda.device(x.device):
            return ops.retina_decode(self.heads(x.float()), full=True)

    def detect(self, x, resize, conf_threshold):
        """Mean-subtracted (B,3,H,W) batch -> per image a float32 (k_b, 15) array of the rows with score > conf_threshold in anchor order
        [x1, y1, x2, y2, score, landmarks], in pixels of the original image (`* scale / resize` applied)."""
        from .retinaface_utils import batched_decode, batched_decode_landm
        net = self.net
        B, _, H, W = x.shape
        ops.L.ensure_device(x.device)
        with torch.no_grad(), torch.cuda.device(x.device):
            heads = self.heads(x.float())
            pri, net.scale, net.scale1 = self.priors(H, W, x.device)       # (the pixel scales, set as the torch backend's _run sets them)
            rows, counts = ops.retina_decode(heads, pri, variance=net.cfg['variance'], img_wh=(W, H), resize=resize, conf_threshold=conf_threshold, cap=self.CAP)
            counts = counts.cpu().numpy()
            if int(counts.max()) <= self.CAP:
                k = int(counts.max())
                host = rows[:, :k].cpu().numpy() if k else np.zeros((B, 0, 15), dtype=np.float32)
                return [host[b, :counts[b]] for b in range(B)]
            # more passing anchors than the compact buffer holds: the full tensors and the torch backend's own expressions
            loc, conf, ldm = ops.retina_decode(heads, full=True)
            boxes = batched_decode(loc, pri.unsqueeze(0), net.cfg['variance']) * net.scale / resize
            lands = batched_decode_landm(ldm, pri.unsqueeze(0), net.cfg['variance']) * net.scale1 / resize
            full = torch.cat((boxes, conf[:, :, 1:2], lands), dim=2)
            return [full[b][conf[b, :, 1] > conf_threshold].cpu().numpy() for b in range(B)]
