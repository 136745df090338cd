"""What the conv checkers (split_check.py, wino_check.py, f43_check.py; the timing loop also gemm_split_check.py and the probes) share:
the seeded draw of one 3x3 layer's tensors, its fp64 reference, the conv2d argument assembly, the GroupNorm-partials check and the timing
loop.  A library: nothing in the package imports it, and only t_ms / launch_args' default device need a GPU."""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from codeformer_amd import ops  # noqa: E402


def t_ms(fn, n=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def draw(B, H, W, cin, cout, *, upsample=False, seed=0, wscale=1.0, xscale=1.0, device='cpu'):
    """x, w, b, sc, sh, res, ss of one layer (NHWC activations; res / ss at the output size) from one seeded generator.  The order and
    the expressions are the data of every recorded checker result: do not reorder.  (device='cuda': timing-only data.)"""
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.randn(B, H, W, cin, generator=g, device=device) * xscale
    w = torch.randn(cout, cin, 3, 3, generator=g, device=device) * (2.0 / (9 * cin)) ** 0.5 * wscale
    b = torch.randn(cout, generator=g, device=device) * 0.1
    sc = torch.rand(B, cin, generator=g, device=device) + 0.5
    sh = torch.randn(B, cin, generator=g, device=device) * 0.1
    Ho, Wo = (2 * H, 2 * W) if upsample else (H, W)
    res = torch.randn(B, Ho, Wo, cout, generator=g, device=device)
    ss = torch.randn(B, Ho, Wo, cout, generator=g, device=device) * 0.3
    return x, w, b, sc, sh, res, ss


def reference(x, w, b, *, prologue, epilogue, sc=None, sh=None, res=None, ss=None, upsample=False, sft_w=0.7):
    """fp64: prologue, optional nearest-x2 upsample, 3x3 convolution with zero padding, epilogue; NHWC in and out."""
    xd = x.double()
    if prologue in (ops.PRO_AFFINE, ops.PRO_AFFINE_SWISH):
        xd = xd * sc.double()[:, None, None, :] + sh.double()[:, None, None, :]
        if prologue == ops.PRO_AFFINE_SWISH:
            xd = xd * torch.sigmoid(xd)
    elif prologue == ops.PRO_LEAKY:
        xd = F.leaky_relu(xd, 0.2)
    xn = xd.permute(0, 3, 1, 2)
    if upsample:
        xn = F.interpolate(xn, scale_factor=2.0, mode='nearest')
    ref = F.conv2d(xn, w.double(), b.double(), padding=1).permute(0, 2, 3, 1)
    if epilogue == ops.EPI_RESIDUAL:
        ref = ref + res.double()
    elif epilogue == ops.EPI_SFT:
        ref = res.double() + sft_w * (res.double() * ss.double() + ref)
    return ref


def launch_args(x, sc, sh, res, ss, *, prologue, epilogue, stats, upsample=False, c_split=None, device='cuda'):
    """(x1, x2, kw) for ops.conv2d(x1, pw, x2=x2, **kw): the tensors the options read, on the device, the input split at c_split."""
    kw = dict(prologue=prologue, epilogue=epilogue, emit_stats=stats, upsample=upsample)
    if prologue in (ops.PRO_AFFINE, ops.PRO_AFFINE_SWISH):
        kw.update(scale=sc.to(device), shift=sh.to(device))
    if epilogue != ops.EPI_NONE:
        kw.update(res=res.to(device))
    if epilogue == ops.EPI_SFT:
        kw.update(sft_scale=ss.to(device), sft_w=0.7)
    xc = x.to(device)
    x1, x2 = (xc, None) if c_split is None else (xc[..., :c_split].contiguous(), xc[..., c_split:].contiguous())
    return x1, x2, kw


def stats_rel_err(y):
    """The epilogue's GroupNorm partials (y._cf_stats) must describe exactly the tensor that was written: the largest relative error of
    the 32 groups' sum and sum of squares against fp64 sums over y."""
    st = y._cf_stats
    B = y.shape[0]
    got = st.part.view(B, 32, st.parts, 2).sum(2)
    r = y.double().view(B, -1, 32, st.cpg)
    want = torch.stack([r.sum((1, 3)), (r * r).sum((1, 3))], -1)
    return float(((got - want).abs() / want.abs().clamp_min(1e-6)).max())
