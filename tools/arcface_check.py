"""The kernels of csrc/cf_arcface.hip per element: recipes, float64 references, bounds derived from the order each kernel's comment states, and a
NumPy float32 emulation of that order.  Library of tests/test_gpu_arcface.py (GPU: the kernel within the bound) and tests/test_arcface_host.py (CPU:
the emulation within 0.5 of the bound and the exactness preconditions, so every bound is a statement about the reference).  u = 2^-24.  No constant
here was fitted to what a kernel returns.

fc_rows (M, N, K)   per (row, column): an fmaf chain in ascending k from zero over each quarter (64) of a chunk (256), the quarters added in order (3),
    the chunks added as FC_FIN = 8 interleaved chains (ceil(chunks / 8) additions each, the first to zero), the chains in order (7), the bias.
    bound = c u sum_k |w||x| + 2 u |out|,  c = 64 + 3 + ceil(chunks / 8) + 7: the roundings a product passes; the bias add at a whole ulp.
    families: int_coded (bitwise the float64 result: every partial sum is a whole number of units below 2^24), onehot (row m holds a single 1 at k_m:
    the output is fl(w[n, k_m] + b[n]), bitwise; onehot_ks() walks both sides of every quarter and chunk boundary), cancel_pairs (terms O(1), sums
    ~2^-9), row_scales (rows over 2^+-20, no bias: a row's error is bounded by the row's own magnitude).
se_gate (B, C, r)   layer 1: one wave per hidden unit, lane partials over c in stride 64 (fmaf), a butterfly of 6, the bias, PReLU; layer 2: an fmaf chain
    over r, the bias, 1 / (1 + expf(-s)).
    e1 = (C + 16) u sum |w1||p| + u |b1|;  through PReLU: max(1, |a|) e1 (the product's own rounding, u |h|, is one of layer 2's r + 16);
    e2 = (r + 16) u (sum |w2||h| + |b2|) + sum |w2| max(1, |a|) e1;  the sigmoid has slope <= 1 / 4:  bound = e2 / 4 + 4 m u sigmoid(s),
    m = the largest error of torch's CPU float32 sigmoid against float64 on the same float32 pre-activations in units of u sigmoid(s) (sigmoid_figure();
    never below 0.5, the rounding of the result itself), 4 for another expf and the division.
se_pool (B, H, W, C)   16 additions per thread, 15 in LDS, nrb = ceil(HW / 256) partials, one division:  bound = (31 + nrb + 2) u sum |x| / HW.
    families: normal (mean 0.5), cancel (pairs +-v plus a ripple of 2^-12 per channel: mean ~1e-4, |x| ~1), mixed (channel scales over 2^+-20), int_coded
    (HW a power of two: bitwise).
cosine_rows   float64 throughout: lane partials over n in stride 64, a butterfly of 6, two square roots, a product, a quotient:
    bound = 3 (ceil(n / 64) + 9) 2^-53 sum |x y| / max(|x||y|, 1e-8)   (|out| <= that sum, and each norm carries the chain's relative error).
identity_input   bitwise the host definition (codeformer_amd.metrics); the host definition against F.interpolate(bilinear, align_corners=False) of the
    gray image in float64.  The source coordinate (o + 0.5) (n / 128) - 0.5 is EXACT in float32 for n < 2^15 (n / 128 is a division by a power of two,
    o + 0.5 has eight bits), so both tap weights are exact (identity_weights_exact()); what is left are the three products and three sums on the way
    of a value, each rounding at most u G with G = max |gray| (convex combinations stay below G):  bound = 6 u G.
"""
import math

import numpy as np

U = 2.0 ** -24
SLOPES = (-0.5, 0.0, 0.25, 1.5)
FC_KC, FC_FIN, FC_ROWS = 256, 8, 16
FC_SHAPES = ((1, 4, 256), (16, 68, 2304), (17, 128, 1024))
FC_FAMILIES = ('int_coded', 'cancel_pairs', 'row_scales', 'normal')
SE_GATE_SHAPES = ((2, 68, 3), (1, 320, 20), (1, 4096, 256), (2, 128, 8))
SE_POOL_SHAPES = ((1, 1, 1, 4), (1, 16, 16, 68), (2, 17, 19, 132))
SE_POOL_FAMILIES = ('normal', 'cancel', 'mixed', 'int_coded')
F32 = np.float32


def _seed(name):
    return sum(ord(c) * (i + 1) for i, c in enumerate(name))


# ---- fc_rows -----------------------------------------------------------------------------------------------------------------------------------
def fc_family(name, shape):
    """-> x (M, K), w (N, K), b (N,) or None, float32."""
    M, N, K = shape
    rng = np.random.default_rng(_seed(name) + M + 3 * N + 7 * K)
    x, w, b = rng.normal(0., 1., (M, K)), rng.normal(0., 1., (N, K)) / math.sqrt(K), rng.normal(0., 1., (N,))
    if name == 'int_coded':      # |x| <= 3, |w| <= 3 units of 2^-5, |b| <= 4: sum |w x| <= 9 K units of 2^-5 < 2^24
        x, w, b = rng.integers(-3, 4, (M, K)), rng.integers(-3, 4, (N, K)) * 2.0 ** -5, rng.integers(-4, 5, (N,))
    elif name == 'cancel_pairs':
        x = np.repeat(rng.normal(0., 1., (M, K // 2)), 2, axis=1)
        w0 = rng.normal(0., 1., (N, K // 2))
        w = np.stack((w0, -(w0 + rng.normal(0., 2.0 ** -9, w0.shape))), axis=2).reshape(N, K)
        b = b * 2.0 ** -9
    elif name == 'row_scales':
        x = x * 2.0 ** np.round(np.linspace(-20, 20, M) if M > 1 else np.array([-20.]))[:, None]
        b = None
    return x.astype(F32), w.astype(F32), None if b is None else b.astype(F32)


def fc_onehot_ks(K):
    """Both sides of every quarter boundary and every chunk boundary, the first and the last k."""
    ks = {0, K - 1}
    for q in range(64, K, 64):
        ks |= {q - 1, q}
    return sorted(ks)


def fc_ref(x, w, b):
    out = x.astype(np.float64) @ w.astype(np.float64).T
    return out if b is None else out + b.astype(np.float64)


def fc_coef(K):
    return 64 + 3 + -(-(K // FC_KC) // FC_FIN) + 7


def fc_bound(x, w, b):
    S = np.abs(x.astype(np.float64)) @ np.abs(w.astype(np.float64)).T
    return fc_coef(x.shape[1]) * U * S + 2 * U * np.abs(fc_ref(x, w, b))


def _fma32(a, b, c):
    """fl32(a b + c) for float32 arrays: the product is exact in float64, the sum is rounded to 53 bits and then to 24 (a double rounding that can
    differ from the fused result by a float32 tie only)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def fc_emulate(x, w, b):
    M, K = x.shape
    N, chunks = w.shape[0], K // FC_KC
    part = np.zeros((chunks, M, N), F32)
    for s in range(chunks):
        quarters = []
        for q in range(4):
            acc = np.zeros((M, N), F32)
            for k in range(s * FC_KC + q * 64, s * FC_KC + q * 64 + 64):
                acc = _fma32(w[None, :, k], x[:, k, None], acc)
            quarters.append(acc)
        part[s] = ((quarters[0] + quarters[1]) + quarters[2]) + quarters[3]
    chains = []
    for j in range(FC_FIN):
        t = np.zeros((M, N), F32)
        for c in range(j, chunks, FC_FIN):
            t = t + part[c]
        chains.append(t)
    t = chains[0]
    for q in range(1, FC_FIN):
        t = t + chains[q]
    return t if b is None else t + b[None]


# ---- se_gate -----------------------------------------------------------------------------------------------------------------------------------
def prelu(t, a):
    return np.where(t > 0, t, np.asarray(a, t.dtype) * t)


def gate_inputs(shape, slope):
    """-> pooled (B, C), w1 (r, C), b1 (r,), w2 (C, r), b2 (C,): float32.  Channels 1 and 2 (mod 7) get a layer-2 bias of +-40: pre-activations of about +-40."""
    B, C, r = shape
    rng = np.random.default_rng(1000 + C + 5 * r + int(slope * 8))
    p, w1, b1 = rng.normal(0., 1., (B, C)), rng.normal(0., 1., (r, C)) / math.sqrt(C), rng.normal(0., 0.5, (r,))
    w2, b2 = rng.normal(0., 1., (C, r)) / math.sqrt(r), rng.normal(0., 0.5, (C,))
    b2[1::7], b2[2::7] = 40.0, -40.0
    return tuple(t.astype(F32) for t in (p, w1, b1, w2, b2))


def gate_ref(p, w1, b1, a, w2, b2):
    """float64 -> dict(pre1, h, s, out)."""
    p, w1, b1, w2, b2 = (t.astype(np.float64) for t in (p, w1, b1, w2, b2))
    pre1 = p @ w1.T + b1
    h = prelu(pre1, float(a))
    s = h @ w2.T + b2
    return dict(pre1=pre1, h=h, s=s, out=1.0 / (1.0 + np.exp(-s)))


def sigmoid_figure(s32):
    """torch's CPU float32 sigmoid against float64 on float32 pre-activations: the largest |error| in units of u sigmoid(s); at least 0.5."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(s32, dtype=F32))
    ref = torch.sigmoid(t.double())
    ok = ref > 1e-30
    err = ((torch.sigmoid(t).double() - ref).abs() / (U * ref))[ok]
    return max(0.5, float(err.max()))


def gate_bound(p, w1, b1, a, w2, b2, ref, figure):
    C, r = p.shape[1], w1.shape[0]
    pa, w1a, w2a = (np.abs(t.astype(np.float64)) for t in (p, w1, w2))
    amp = max(1.0, abs(float(a)))
    e1 = (C + 16) * U * (pa @ w1a.T) + U * np.abs(b1.astype(np.float64))
    e2 = (r + 16) * U * (np.abs(ref['h']) @ w2a.T + np.abs(b2.astype(np.float64))) + (amp * e1) @ w2a.T
    return e2 / 4 + 4 * figure * U * ref['out']


def gate_emulate(p, w1, b1, a, w2, b2):
    """The kernel's order in float32 (the sigmoid is torch's CPU float32 one) -> (gate, the float32 layer-2 pre-activations)."""
    import torch
    B, C = p.shape
    r = w1.shape[0]
    lanes = np.zeros((B, r, 64), F32)
    for i0 in range(0, C, 64):
        n = min(64, C - i0)
        lanes[:, :, :n] = _fma32(w1[None, :, i0:i0 + n], p[:, None, i0:i0 + n], lanes[:, :, :n])
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[:, :, np.arange(64) ^ o]
    h = prelu(lanes[:, :, 0] + b1[None], F32(a))
    s = np.zeros((B, C), F32)
    for j in range(r):
        s = _fma32(w2[None, :, j], h[:, j, None], s)
    s = s + b2[None]
    return torch.sigmoid(torch.from_numpy(s)).numpy(), s


# ---- se_pool -----------------------------------------------------------------------------------------------------------------------------------
def pool_family(name, shape):
    B, H, W, C = shape
    rng = np.random.default_rng(_seed(name) + H * W + 11 * C)
    hw = H * W
    x = rng.normal(0.5, 1., (B, hw, C))
    if name == 'cancel':      # pairs +-v (an odd last pixel: 0) plus a ripple of 2^-12: the mean is ~1e-4 where |x| is ~1
        v = rng.normal(0., 1., (B, hw // 2, C))
        x = np.zeros((B, hw, C))
        x[:, 0:2 * (hw // 2):2], x[:, 1:2 * (hw // 2):2] = v, -v
        x = rng.permuted(x, axis=1) + 2.0 ** -12 * (1.0 + rng.random((B, 1, C)))
    elif name == 'mixed':
        x = x * 2.0 ** np.round(np.linspace(-20, 20, C))[None, None, :]
    elif name == 'int_coded':
        x = rng.integers(-100, 101, (B, hw, C)).astype(np.float64)
    return x.reshape(B, H, W, C).astype(F32)


def pool_nrb(hw):
    return (hw + 255) // 256


def pool_ref(x):
    B, H, W, C = x.shape
    return x.astype(np.float64).reshape(B, H * W, C).mean(axis=1)


def pool_bound(x):
    B, H, W, C = x.shape
    return (31 + pool_nrb(H * W) + 2) * U * np.abs(x.astype(np.float64)).reshape(B, H * W, C).sum(axis=1) / (H * W)


def pool_emulate(x):
    B, H, W, C = x.shape
    hw, nrb = H * W, pool_nrb(H * W)
    xp = np.zeros((B, nrb * 256, C), F32)
    xp[:, :hw] = x.reshape(B, hw, C)
    xp = xp.reshape(B, nrb, 16, 16, C)      # pixel = rb 256 + 16 i + rl
    out = np.zeros((B, C), F32)
    for rb in range(nrb):
        s = np.zeros((B, 16, C), F32)
        for i in range(16):
            s = s + xp[:, rb, i]
        t = s[:, 0]
        for rl in range(1, 16):
            t = t + s[:, rl]
        out = out + t
    return out / F32(hw)


# ---- cosine_rows -------------------------------------------------------------------------------------------------------------------------------
def cosine_ref(x, y):
    x, y = x.astype(np.float64), y.astype(np.float64)
    den = np.maximum(np.sqrt((x * x).sum(1)) * np.sqrt((y * y).sum(1)), 1e-8)
    return (x * y).sum(1) / den


def cosine_bound(x, y):
    x, y = x.astype(np.float64), y.astype(np.float64)
    den = np.maximum(np.sqrt((x * x).sum(1)) * np.sqrt((y * y).sum(1)), 1e-8)
    return 3 * (-(-x.shape[1] // 64) + 9) * 2.0 ** -53 * np.abs(x * y).sum(1) / den


def cosine_emulate(x, y):
    """The kernel's order in float64: lane partials in stride 64, the butterfly, sqrt sqrt, the floor, the quotient."""
    rows, n = x.shape
    acc = np.zeros((3, rows, 64))
    for i0 in range(0, n, 64):
        m = min(64, n - i0)
        p, q = x[:, i0:i0 + m].astype(np.float64), y[:, i0:i0 + m].astype(np.float64)
        acc[0, :, :m] += p * q
        acc[1, :, :m] += p * p
        acc[2, :, :m] += q * q
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, :, np.arange(64) ^ o]
    den = np.sqrt(acc[1, :, 0]) * np.sqrt(acc[2, :, 0])
    return acc[0, :, 0] / np.where(den > 1e-8, den, 1e-8)


def cosine_rows_family(rows, n, norm):
    rng = np.random.default_rng(17 * rows + n)
    x, y = rng.normal(0., 1., (rows, n)), rng.normal(0., 1., (rows, n))
    x, y = (t / np.sqrt((t * t).sum(1, keepdims=True)) * norm for t in (x, y))
    return x.astype(F32), y.astype(F32)


# ---- identity_input ----------------------------------------------------------------------------------------------------------------------------
def identity_bound(gray):
    """gray (B, H, W) float64 -> the bound of the host definition against the float64 bilinear resize (one number per image)."""
    return 6 * U * np.abs(gray).reshape(gray.shape[0], -1).max(1)


def identity_weights_exact(n):
    """The float32 source coordinates of an axis of n pixels equal the float64 ones."""
    o = np.arange(128)
    s32 = np.maximum((o.astype(F32) + F32(0.5)) * (F32(n) / F32(128)) - F32(0.5), F32(0))
    s64 = np.maximum((o + 0.5) * (n / 128) - 0.5, 0.0)
    return bool(np.array_equal(s32.astype(np.float64), s64))


# ---- IRBlock without SE, per element -----------------------------------------------------------------------------------------------------------
def block_ref(blk, x):
    """The folded dataflow of an IRBlock (no SE) in float64 on the float32-ROUNDED folded parameters the device packs (so the fold's own rounding is
    not in the bound), and the per-element bound composed along it (u at a whole ulp, 2 u |value|, for every single rounding):
      prologue   p = x s + t: two roundings, ep = 2 u (|x s| + |t|)
      conv1      (9 cin + 16) u (S1 + |b1|) + sum |w1| ep,  S1 = sum |w1||p| under zero padding (the padding is NOT shifted)
      PReLU      h = pre1 > 0 ? pre1 : a pre1: max(1, |a|) e1 + 2 u |h|
      conv2      (9 cin + 16) u (sum |w2| (|h| + eh) + |b2|) + sum |w2| eh, at the block's stride
      shortcut   x itself (exact), or the 1x1 conv as the centre tap of a 3x3: (9 cin + 16) u (sum |wsc||x| + |bsc|)
      residual add and PReLU   t = pre2 + res: e2 + esc + 2 u |t|;  out: max(1, |a|) et + 2 u |out|
    x: (B, C, H, W) float32 CPU -> (out, bound), float64 NCHW."""
    import torch
    import torch.nn.functional as F
    f = {k: None if v is None else tuple(t.float().double() for t in v) for k, v in blk.folded(torch.float64).items()}
    a = float(np.float32(float(blk.prelu.weight.detach().reshape(-1)[0])))
    amp, st = max(1.0, abs(a)), blk.stride
    xd = x.double()
    s, t = (v.view(1, -1, 1, 1) for v in f['pre'])
    cin = x.shape[1]
    c = (9 * cin + 16) * U
    p, ep = xd * s + t, 2 * U * ((xd * s).abs() + t.abs())
    w1, b1 = f['conv1']
    pre1 = F.conv2d(p, w1, b1, padding=1)
    e1 = c * (F.conv2d(p.abs(), w1.abs(), padding=1) + b1.abs().view(1, -1, 1, 1)) + F.conv2d(ep, w1.abs(), padding=1)
    h = torch.where(pre1 > 0, pre1, a * pre1)
    eh = amp * e1 + 2 * U * h.abs()
    w2, b2 = f['conv2']
    pre2 = F.conv2d(h, w2, b2, stride=st, padding=1)
    e2 = c * (F.conv2d(h.abs() + eh, w2.abs(), stride=st, padding=1) + b2.abs().view(1, -1, 1, 1)) + F.conv2d(eh, w2.abs(), stride=st, padding=1)
    if f['shortcut'] is None:
        res, esc = xd, torch.zeros_like(pre2)
    else:
        ws, bs = f['shortcut']
        res = F.conv2d(xd, ws, bs, stride=st, padding=1)
        esc = c * (F.conv2d(xd.abs(), ws.abs(), stride=st, padding=1) + bs.abs().view(1, -1, 1, 1))
    tt = pre2 + res
    out = torch.where(tt > 0, tt, a * tt)
    return out, amp * (e2 + esc + 2 * U * tt.abs()) + 2 * U * out.abs()


def block_emulate(blk, x):
    """The same dataflow in torch float32 on the CPU."""
    import torch
    import torch.nn.functional as F
    f = {k: None if v is None else tuple(t.float() for t in v) for k, v in blk.folded(torch.float64).items()}
    a = torch.tensor(float(blk.prelu.weight.detach().reshape(-1)[0]), dtype=torch.float32)
    s, t = (v.view(1, -1, 1, 1) for v in f['pre'])
    h = F.conv2d(x * s + t, *f['conv1'], padding=1)
    h = torch.where(h > 0, h, a * h)
    h = F.conv2d(h, *f['conv2'], stride=blk.stride, padding=1)
    tt = h + (x if f['shortcut'] is None else F.conv2d(x, *f['shortcut'], stride=blk.stride, padding=1))
    return torch.where(tt > 0, tt, a * tt)
