from codeformer_amd.losses import *  # noqa: F401,F403
from codeformer_amd.losses import PerceptualLoss  # noqa: F401
