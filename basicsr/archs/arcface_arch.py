from codeformer_amd.archs.arcface_arch import *  # noqa: F401,F403
from codeformer_amd.archs.arcface_arch import BasicBlock, Bottleneck, IRBlock, ResNetArcFace, SEBlock, conv3x3  # noqa: F401
