"""PerceptualLoss -- the perceptual and style terms on VGG features (reference: basicsr/losses/losses.py:144-253) -- as a SCORE.

Only this class of the reference's losses is built, and it is forward-only: the project has no backward for its convolutions, so the CUDA
path returns values without a graph and refuses an input that requires grad while grad is enabled.  The constructor and the return value
`(percep, style)` (0-dim float32 tensors, or None for a weight that is not positive) are the reference's.

Criteria, with the reference's batch reductions over features f(x), f(gt) of every layer k, weighted by layer_weights[k]:
  'l1' / 'mse'   the mean over ALL elements of the batch tensor of |d| / d^2
  'fro'          the Frobenius norm of the whole batch tensor of d
  style          the same on the Gram matrices G[b] = F F^T / (c h w) of the (c, h w) feature matrix F (_gram_mat)
'l2' raises NotImplementedError at construction: the reference maps it to torch.nn.L2loss, which does not exist (its constructor raises
AttributeError there); 'mse' is that criterion.

CPU tensors take stock torch ops: the reference's forward.  CUDA tensors take the device path: x and gt pass the extractor as one batch of
2B images (features stay channels-last; no reduction here depends on the layout), cf_feat_dist gives sum |d| and sum d^2 per image in
float64 (d one float32 subtraction), cf_gram the Gram matrices on the fp32 MFMA; the layer weights, the batch reduction and the cast to
float32 are a few device tensor ops -- nothing is copied to the host and nothing synchronises.
"""
import torch
from torch import nn

from .archs.vgg_arch import VGGFeatureExtractor
from .utils.registry import LOSS_REGISTRY

__all__ = ['PerceptualLoss']

CRITERIA = ('l1', 'mse', 'fro')


def reduce_dist(d, n, criterion, per_image=False):
    """d: (B,2) float64 (sum |d|, sum d^2) per image of n elements each -> the criterion's value: a 0-dim tensor over the batch (the
    reference's reduction), or with per_image a (B,) tensor (every image as a batch of one)."""
    if criterion == 'fro':
        return torch.sqrt(d[:, 1] if per_image else d[:, 1].sum())
    col = d[:, 0] if criterion == 'l1' else d[:, 1]
    return col / n if per_image else col.sum() / (n * d.shape[0])


def gram_host(x):
    """_gram_mat of the reference (losses.py:240-253): (n,c,h,w) -> (n,c,c)."""
    n, c, h, w = x.size()
    features = x.view(n, c, w * h)
    return features.bmm(features.transpose(1, 2)) / (c * h * w)


@LOSS_REGISTRY.register()
class PerceptualLoss(nn.Module):
    """Perceptual loss with the commonly used style loss (losses.py:144-253), forward-only.

    layer_weights: {layer name: weight}, e.g. {'conv5_4': 1.}; vgg_type / use_input_norm / range_norm: see VGGFeatureExtractor;
    perceptual_weight / style_weight: the term is computed and multiplied by the weight when it is > 0, else None is returned for it;
    criterion: 'l1' | 'mse' | 'fro'."""

    def __init__(self, layer_weights, vgg_type='vgg19', use_input_norm=True, range_norm=False, perceptual_weight=1.0, style_weight=0.,
                 criterion='l1'):
        super().__init__()
        if criterion == 'l2':
            raise NotImplementedError("criterion 'l2': the reference maps it to torch.nn.L2loss, which does not exist; use 'mse'")
        if criterion not in CRITERIA:
            raise NotImplementedError(f'{criterion} criterion has not been supported.')
        self.perceptual_weight = perceptual_weight
        self.style_weight = style_weight
        self.layer_weights = layer_weights
        self.vgg = VGGFeatureExtractor(layer_name_list=list(layer_weights.keys()), vgg_type=vgg_type, use_input_norm=use_input_norm,
                                       range_norm=range_norm)
        self.criterion_type = criterion
        self.criterion = {'l1': torch.nn.L1Loss(), 'mse': torch.nn.MSELoss(reduction='mean'), 'fro': None}[criterion]

    # -- host ------------------------------------------------------------------------------------------------------------------------------
    def _term_host(self, a, b):
        if self.criterion_type == 'fro':
            return torch.norm(a - b, p='fro')
        return self.criterion(a, b)

    def forward_host(self, x, gt):
        x_features = self.vgg.forward_host(x)
        gt_features = self.vgg.forward_host(gt.detach())
        percep_loss = style_loss = None
        if self.perceptual_weight > 0:
            percep_loss = 0
            for k in x_features.keys():
                percep_loss += self._term_host(x_features[k], gt_features[k]) * self.layer_weights[k]
            percep_loss *= self.perceptual_weight
        if self.style_weight > 0:
            style_loss = 0
            for k in x_features.keys():
                style_loss += self._term_host(gram_host(x_features[k]), gram_host(gt_features[k])) * self.layer_weights[k]
            style_loss *= self.style_weight
        return percep_loss, style_loss

    _gram_mat = staticmethod(gram_host)

    # -- HIP -------------------------------------------------------------------------------------------------------------------------------
    def features(self, views, bgr=False):
        """The extractor's channels-last features of `views` = [a views..., b views...] (an even number of images in all; see
        VGGFeatureExtractor.features_from_views).  Device only."""
        return self.vgg.features_from_views(views, bgr)

    def score(self, feats, style=False, criterion=None, per_image=False):
        """sum_k w_k criterion(f_k[:B], f_k[B:]) of features of 2B images, float64 on the device: 0-dim with the reference's batch reduction,
        or (B,) per image (every image as a batch of one); style: on the Gram matrices."""
        from . import ops
        total = 0
        for k, f in feats.items():
            t = ops.gram(f) if style else f
            half = t.shape[0] // 2
            d = ops.feat_dist(t[:half], t[half:])
            total = total + reduce_dist(d, t[0].numel(), criterion or self.criterion_type, per_image) * float(self.layer_weights[k])
        return total

    def forward_hip(self, x, gt):
        from . import ops
        if torch.is_grad_enabled() and (x.requires_grad or gt.requires_grad):
            raise RuntimeError('PerceptualLoss on HIP is value-only (no backward): detach the input or call it under torch.no_grad()')
        if tuple(x.shape) != tuple(gt.shape) or x.device != gt.device or x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f'PerceptualLoss: two (B,3,H,W) tensors of one shape on one device, got {tuple(x.shape)} and {tuple(gt.shape)}')
        self.vgg.check_device_call((2 * x.shape[0],) + tuple(x.shape[1:]))
        ops.L.ensure_device(x.device)
        with torch.no_grad(), torch.cuda.device(x.device):
            views = [t.detach().float().permute(0, 2, 3, 1) for t in (x, gt)]
            feats = self.features(views)
            percep = style = None
            if self.perceptual_weight > 0:
                percep = (self.score(feats) * float(self.perceptual_weight)).float()
            if self.style_weight > 0:
                style = (self.score(feats, style=True) * float(self.style_weight)).float()
        return percep, style

    def forward(self, x, gt):
        if x.is_cuda:
            return self.forward_hip(x, gt)
        return self.forward_host(x, gt)
