from copy import deepcopy

from codeformer_amd.utils.registry import METRIC_REGISTRY
from .psnr_ssim import calculate_psnr, calculate_ssim

__all__ = ['calculate_psnr', 'calculate_ssim']


def calculate_metric(data, opt):
    """The metric named by opt['type'] (a METRIC_REGISTRY entry), called with data and the other options as keywords."""
    opt = deepcopy(opt)
    return METRIC_REGISTRY.get(opt.pop('type'))(**data, **opt)


from codeformer_amd.metrics import calculate_identity, identity_batch, identity_input, load_arcface  # noqa: E402

__all__ += ['calculate_identity', 'identity_batch', 'identity_input', 'load_arcface']
from codeformer_amd.metrics import calculate_perceptual, load_lpips_vgg, load_vgg, lpips_batch, perceptual_batch  # noqa: E402

__all__ += ['calculate_perceptual', 'perceptual_batch', 'load_vgg', 'lpips_batch', 'load_lpips_vgg']
