from codeformer_amd.archs.arch_util import *  # noqa: F401,F403
from codeformer_amd.archs.arch_util import (DCNv2Pack, ResidualBlockNoBN, Upsample, _no_grad_trunc_normal_, _ntuple,  # noqa: F401
                                            default_init_weights, flow_warp, make_layer, pixel_unshuffle, resize_flow, to_1tuple,
                                            to_2tuple, to_3tuple, to_4tuple, to_ntuple, trunc_normal_)
