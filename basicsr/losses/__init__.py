from .losses import PerceptualLoss  # noqa: F401
from codeformer_amd.utils.registry import LOSS_REGISTRY  # noqa: F401

__all__ = ['PerceptualLoss', 'LOSS_REGISTRY']
