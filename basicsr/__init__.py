"""Drop-in shim: the reference's entrypoints import `basicsr.*`; every name resolves to codeformer_amd.

The modules an inference user reaches exist: archs, ops (dcn, fused_act, upfirdn2d), metrics (PSNR / SSIM, imported on demand:
`import basicsr.metrics` fills METRIC_REGISTRY) and utils.{registry,misc,img_util,logger,download_util,matlab_functions}; the other
training-side packages of the reference (data, losses, models, train) are out of scope.
"""
from codeformer_amd import __version__  # noqa: F401
from . import archs  # noqa: F401,E402  (the reference's basicsr/__init__.py:3 star-imports archs, which fills ARCH_REGISTRY)
from . import utils  # noqa: F401,E402
