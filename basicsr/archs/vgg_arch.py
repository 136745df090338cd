from codeformer_amd.archs.vgg_arch import *  # noqa: F401,F403
from codeformer_amd.archs.vgg_arch import NAMES, VGG_PRETRAIN_PATH, VGGFeatureExtractor, insert_bn  # noqa: F401
