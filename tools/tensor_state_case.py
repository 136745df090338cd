"""The one case tests/test_gpu_tensor_state.py and tests/test_tensor_state_host.py share: two contents of a 2 x 16 x 16 x 64 NHWC buffer whose
GroupNorm tables and range scales cannot be mistaken for one another, the weights that produce them, and their fp64 model.  Pure CPU torch
/ NumPy; the bound functions come from tests/test_gpu_norm_conditioning.py (passed in as `nc`), nothing here is a tolerance."""
import numpy as np
import torch
import torch.nn.functional as F

B, H, W, C = 2, 16, 16, 64
GROUPS = 32
BIG = 2.0 ** 21          # contents B: an exact power of two above contents A


def contents(which, cin=C):
    """The INPUT of the producing convolution.  'A': seeded randn.  'B': another seeded randn times 2^21 plus a per-channel bias of
    magnitude 2^21 (sign alternating with the channel), so that the written tensor is 2^21 larger and sits off zero."""
    g = torch.Generator().manual_seed({'A': 101, 'B': 202}[which])
    x = torch.randn(B, H, W, cin, generator=g)
    if which == 'B':
        sign = torch.where(torch.arange(cin) % 2 == 0, 1.0, -1.0)
        x = x * BIG + sign * BIG
    return x


def weight(cout, cin=C, taps=3, seed=7):
    """He-scaled (cout, cin, taps, taps) weight and a small bias: the convolution part of the output has the sigma of its input times sqrt(2)."""
    g = torch.Generator().manual_seed(seed + 1000 * cout + cin)
    return torch.randn(cout, cin, taps, taps, generator=g) * (2.0 / (taps * taps * cin)) ** 0.5, torch.randn(cout, generator=g) * 0.1


def affine(c, seed=5):
    rng = np.random.default_rng(seed)
    return (0.5 + rng.random(c)) * np.where(rng.random(c) < 0.3, -1.0, 1.0), rng.standard_normal(c)


def model(x, w, b):
    """fp64 3x3 stride-1 zero-padded convolution of an NHWC tensor -> NHWC float64."""
    return F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), padding=w.shape[2] // 2).permute(0, 2, 3, 1).contiguous()


def groups_of(ts, cpg):
    """[(B, H, W, Ci) float64] (a channel concatenation) -> (B, groups, hw * cpg) numpy."""
    full = torch.cat(ts, dim=3)
    b, h, w, c = full.shape
    return full.view(b, h * w, c // cpg, cpg).permute(0, 2, 1, 3).reshape(b, c // cpg, h * w * cpg).numpy()


def reference_tables(nc, ts, gamma, beta, nt):
    """fp64 tables of the concatenation of ts and their first-order bounds at n_t = nt -> (scale, shift, b_scale, b_shift, r_rstd), (B, groups, cpg)
    each (r_rstd (B, groups)): what nc._check_tables compares ops.groupnorm_tables with."""
    ctot = sum(t.shape[3] for t in ts)
    cpg = ctot // GROUPS
    g32 = gamma.astype(np.float32).astype(np.float64).reshape(GROUPS, cpg)[None]
    b32 = beta.astype(np.float32).astype(np.float64).reshape(GROUPS, cpg)[None]
    t = nc.group_terms(groups_of(ts, cpg))
    b = nc.stat_bounds(t, nt, nc.GN_EPS)
    return (*nc.table_bounds(t, b, g32, b32, nc.GN_EPS), b['r_rstd'])


def tight_scale(m):
    """The power of two that puts m = growth * max|x| into [2^13, 2^14): what the from-tensor route returns; the statistics route may
    return down to 2^-7 of it (tests/test_gpu_range.py::test_act_scale_kernels)."""
    return 2.0 ** (14 - int(np.frexp(np.float32(m))[1]))
