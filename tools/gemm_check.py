"""The five token-GEMM kernels behind the Transformer's Linear layers on exact, cancelling and off-grid inputs: seeded input families, the fp64
reference, the per-element gate, the routes (which launch reaches which kernel) and a sequential fp32 CPU emulation of both operand schemes that
makes the gate a condition on the reference.  Library of tests/test_gpu_token_gemm.py (GPU) and tests/test_token_gemm_families_host.py (CPU).
usage (GPU box): python tools/gemm_check.py          one line per (family, shape, kernel): kernel error, emulation error, gate

Kernels (KERNELS) and the launch that reaches each (routes(): the rules of cf_gemm_split_launch / cf_gemm_f32_tile_try / conv_dispatch):
  f32_sk    fp32 64x64 split-K instantiation of igemm_kernel (cf_igemm.hip), fp32 weight: split_k 2.. always; split_k 1 when M % 128 != 0, or the
            weight is padded (N != cout_pad: N = 192), or 512 -> 512.  Rows per IMAGE % 64 == 0.
  f32_tile  gemm_f32_tile_kernel: fp32 weight, split_k 1, M % 128 == 0, N == cout_pad, not 512 -> 512.
  h_sk      gemm_split_kernel: GSPLIT weight, split_k >= 2 (workspace + counters), or split_k 1 with M % 128 != 0 (nsplit == 1: the direct epilogue).  M % 64 == 0.
  h_tile    gemm_split_tile_kernel<1>: GSPLIT, split_k 1, M % 128 == 0.
  h_wg      gemm_split_chunk_kernel<1, 1>: GSPLIT, split_k = SPLITK_IN_WORKGROUP, M % 32 == 0, K <= 1024.
A split count is legal when it divides V = K / 128 (SPLITS: up to ops.SPLITK_MAX).  M is formed as (B, h, w) images: IMAGES.

Families (all generated on the CPU from fixed seeds; family(name, M, K, N) -> A[M,K], W[N,K], bias, res, epilogue):
  int_coded     A[m,k] = ((5m + 3k + (mk mod 251)) mod 17) - 8, W[n,k] = ((7n + 11k + (nk mod 241)) mod 13) - 6, integer bias and residual: every
                operand, its hi half and its pack-scaled image are exact in IEEE half (lo = 0), every partial sum is an integer below 2^24 (largest K
                1152: <= 48 K = 55296; exactness_preconditions() asserts both), so EVERY kernel, split count and association returns the fp64 result
                exactly -- and any permutation of m, k or n changes it.
  onehot_rows   row m of A = e_k(m), k(m) = (37 m + 5) mod K; W ~ N(0,1)/sqrt(K): out[m,n] = W[n,k(m)] + b[n].  fp32 operands: bitwise fp32(W + b)
                (one rounding, the bias add).  Split halves: within the 22-bit split of W.  A sweep of 384 rows sees every k mod 32, every chunk, each row mod 128 in three
                chunks and 24 of the 32 (swizzle class (row >> 2) & 3, 16-byte slot) pairs (asserted on the CPU); all pairs are int_coded's part.
  perm_weight   W a signed permutation (W[n, p(n)] = +-1 for n < K, zero rows beyond), A ~ N(0,1): out[m,n] = +-A[m,p(n)], bitwise for fp32 operands,
                within the 22-bit split of A for split halves.
  cancel_chunks k = 128 c carries A = alpha_m, W = s_c beta_n with alpha beta in [2e4, 5.8e4) and integer chunk weights s_c summing to zero, of unequal
                size so that the chunk additions round and their ORDER shows (+16, -1, +1, .., -16; odd V ends -15, -1; V = 2: +1, -1; V = 1: +1 at
                k = 0, -1 at k = 64); the other k an O(1) signal (0.25 N(0,1) x N(0,1)/sqrt(K)).  The chunk sums are s_c S, S >= 2e4, the result
                O(1): sum|a w| / |ref| >= 1e4 for every element (asserted on the CPU).  A missing `acc = 0`, a chunk folded twice or another
                chunk order shows in the first digits.
  mixed_cols    W ~ N(0,1)/sqrt(K) with column n scaled by 2^-e(n), e linear in n from 0 to MIXED_SPAN = 15 + 14 + 3 = 32: under ops.pack_scale the
                largest columns fill the top binade of half (2^14 .. 2^15), columns below 2^-17 have subnormal lo halves, below 2^-29 subnormal hi
                halves (asserted on the CPU with the host's own rule).
  mixed_rows    A in (-2, 2) with row m scaled by 2^e(m), e from -30 to +14: cf_split_pair splits A in registers with NO scale; the header promises
                22 bits for 2^-3 <= |a| <= 65504 and an absolute 2^-25 per element below.
  gelu_edges    EPI_GELU on pre-activations that are EXACT in every kernel: A[m, k0(m)] = t(m), W[n, k0] = +-1 (sign by the parity of n), every other k
                in exactly cancelling integer pairs (A[m,k+1] = -A[m,k], W[n,k+1] = W[n,k]), bias 0; t cycles through GELU_TARGETS = +-0, +-2^-10,
                +-1, +-3, -6, -10, +10.  Expected: GELU of a known fp32 number; 1 + erf cancels at -3 and is exactly 0 at -6 and -10.
  big_epilogue  bias and residual of +-1e6 (1 .. 2) against an O(1) product, EPI_RESIDUAL.

Gate, against fp64, PER ELEMENT (u = 2^-24; S = sum_k |a_k w_k|, pre = the fp64 pre-activation, out = the fp64 result, V = K / 128):
    pre_err = c S + 2 u |pre| [bias present] + floor                                 gate = pre_err                       (no epilogue)
    c (fp32 operands)  = (128 + V) u                                                 gate = pre_err + 2 u |out|           (residual)
    c (split halves)   = (3 128 + V + 12) u                                          gate = 1.13 pre_err + 4 u |pre| + 3 u |out| + 1e-37   (GELU)
    floor (split halves) = 2^-25 (1 + 2^-10) (sum_k |a_k| / scale + sum_k |w_k|),    0 for fp32 operands
Derivation.  The kernels document ONE association (cf_common.h, cf_gemm_split.hip): a virtual chunk of 128 K values is accumulated from zero in k
order -- on v_mfma_f32_32x32x2_f32 a chain of fp32 FMAs, one rounding each; with split halves three f16 MFMAs per 16-wide step (lo hi, hi lo, hi hi),
whose products are exact in fp32 (11 x 11 bits) and whose 3 x 128 additions round --, then the V chunk sums are added in chunk order from zero,
acc_scale (a power of two: exact) is applied, the bias is added, then the epilogue.  Every rounding is at most u times the magnitude of its result,
and every partial result is at most S (the chunk additions: S; the bias add: |pre| to first order): (128 + V) u S resp. (384 + V) u S with NO
statistical discount, so an adversarial family (cancel_chunks: all 128 partial sums of a chunk have the size of the chunk's S) cannot exceed it.
The two single roundings of the epilogue (bias add, residual add) are entered at a whole ulp, 2 u |result|: half an ulp is ATTAINED by a correct
evaluation just above a power of two (big_epilogue, the small rows of mixed_rows), and the gate is held to twice the emulation.
Split halves add, per product: |a - hi - lo| <= 2^-22 |a| for both operands (two roundings to 11 bits) and the dropped lo lo term, <= 2^-11 |a| 2^-11 |w|:
3 2^-22 = 12 u.  floor: IEEE half has the spacing 2^-24 below 2^-14, so a lo half below 2^-14 (|x| < 2^-3) is rounded with an ABSOLUTE error of 2^-25
instead of 2^-22 |x|; weights are packed times `scale` (ops.pack_scale: one power of two per matrix), tokens with none: per product 2^-25 |a| / scale
resp. 2^-25 |w|, (1 + 2^-10) for the cross terms.  GELU = 0.5 v (1 + erf(v / sqrt 2)) has
|d GELU / dv| <= 1.13, erff and its argument product within 4 u absolute of erf (|x erf'(x)| <= 0.5), 1 + erf rounded once: 0.5 |v| 8 u, and two
products: 3 u |out| (1e-37: fp32 underflow of 0.5 v (1 + erf) at v = -10).  gelu_edges makes its pre-activations exact in every kernel (every partial sum is
a multiple of 2^-10 below 2^14), so its gate keeps the epilogue terms only: 4 u |pre| + 3 u |out| + 1e-37.
The emulation (emulate(): numpy float32, k strictly in order, chunks of 128, hi / lo halves through numpy float16, three products per step, the
epilogue in fp32 with a correctly rounded erf) is the condition on the gate: tests/test_token_gemm_families_host.py asserts its error within 0.5 of
the gate for every gate family at the largest shape the GPU test uses; the factor that remains is the allowance for what the emulation does not
know (how an f16 MFMA rounds its 16 internal additions).  No number here was tuned to what a kernel returns; the kernels' own figures are in the
docstring of tests/test_gpu_token_gemm.py.  Largest emulation error / gate over GATE_SHAPES (fp32 operands | split halves), and the largest |error|:
    cancel_chunks 0.058 (6.3e-1) | 0.019 (6.3e-1)    mixed_cols 0.007 (6.5e-7) | 0.086 (1.3e-6)    mixed_rows 0.493 (1.7e-2) | 0.144 (1.9e-2)
    gelu_edges    0.082 (8.4e-8) | 0.082 (8.4e-8)    big_epilogue 0.492 (1.9e-1) | 0.491 (1.9e-1)
(mixed_rows with fp32 operands and big_epilogue sit at the single bias / residual rounding, which a correct evaluation attains: 0.5 by construction.)
"""
import functools
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from codeformer_amd import ops  # noqa: E402

U = 2.0 ** -24
CHUNK = 128
HALF_SPACING = float(np.finfo(np.float16).smallest_subnormal)      # 2^-24
HALF_MIN_NORMAL = float(np.finfo(np.float16).tiny)                 # 2^-14
MIXED_SPAN = 15 + 14 + 3          # top exponent of the packed weights + |smallest normal exponent of half| + 3: the smallest columns have subnormal hi halves
ROW_EXP = (-30, 14)
GELU_TARGETS = (0.0, -0.0, 2.0 ** -10, -2.0 ** -10, 1.0, -1.0, 3.0, -3.0, -6.0, -10.0, 10.0)
EPI_NONE, EPI_RESIDUAL, EPI_GELU = ops.EPI_NONE, ops.EPI_RESIDUAL, ops.EPI_GELU
KERNELS = ('f32_sk', 'f32_tile', 'h_sk', 'h_tile', 'h_wg')
IMAGES = {32: (1, 4, 8), 96: (3, 4, 8), 64: (1, 8, 8), 192: (3, 8, 8), 128: (2, 8, 8), 384: (6, 8, 8), 256: (1, 16, 16), 48: (1, 6, 8)}
EXACT_FAMILIES = ('int_coded', 'onehot_rows', 'perm_weight')
GATE_FAMILIES = ('cancel_chunks', 'mixed_cols', 'mixed_rows', 'gelu_edges', 'big_epilogue')
# (M, K, N) of the gate families on the GPU: the first one reaches both tile kernels (M = 384: three tiles of 128 rows; K = 1152: V = 9, beyond the
# in-workgroup form), the second the nsplit == 1 epilogue of gemm_split_kernel (M = 192), the in-workgroup form at its largest K and ntn = 3
GATE_SHAPES = ((384, 1152, 64), (192, 1024, 192))


def splits(K):
    """The split counts the C ABI accepts for this K (they divide V = K / 128), up to ops.SPLITK_MAX."""
    return [n for n in range(1, ops.SPLITK_MAX + 1) if (K // CHUNK) % n == 0]


def routes(kernel, M, K, N):
    """-> the split_k values with which ops.conv2d on IMAGES[M] reaches `kernel` at this shape (empty: it cannot)."""
    B, h, w = IMAGES[M]
    V = K // CHUNK
    if K % CHUNK or N % 64:
        return []
    if kernel in ('f32_sk', 'f32_tile'):
        if (h * w) % 64:
            return []
        padded = ops._cout_pad(N) != N
        tile = M % 128 == 0 and not padded and not (K == 512 and N == 512)      # cf_gemm_f32_tile_try
        if kernel == 'f32_tile':
            return [1] if tile else []
        return [n for n in splits(K) if n > 1 or not tile]
    if kernel == 'h_wg':                                                          # cf_gemm_split_launch, split_k == CF_SPLITK_IN_WORKGROUP
        return [ops.SPLITK_IN_WORKGROUP] if M % 32 == 0 and V <= 8 else []
    if M % 64:
        return []
    if kernel == 'h_tile':                                                        # nsplit == 1 && M % 128 == 0
        return [1] if M % 128 == 0 else []
    return [n for n in splits(K) if n > 1 or M % 128]                             # h_sk: gemm_split_kernel


def rnd(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


# ---- the families ----------------------------------------------------------------------------------------------------------------------------
def _int_coded(M, K, N):
    m, n, k = torch.arange(M)[:, None], torch.arange(N)[:, None], torch.arange(K)[None, :]
    A = ((5 * m + 3 * k + (m * k) % 251) % 17 - 8).float()
    W = ((7 * n + 11 * k + (n * k) % 241) % 13 - 6).float()
    bias = (torch.arange(N) % 9 - 4).float()
    res = ((3 * torch.arange(M)[:, None] + 2 * torch.arange(N)[None, :]) % 11 - 5).float()
    return A, W, bias, res


def chunk_weights(V):
    """Integer weights of the big terms per chunk, summing to zero, of UNEQUAL size from V = 3 up: with equal sizes every chunk addition would be
    exact (all chunk sums multiples of one ulp, the partial sums small) and the order of the chunks invisible."""
    if V <= 2:
        return [1, -1][:V]
    mid = [(-1) ** (c + 1) for c in range(V - 2 - V % 2)]
    s = [16] + mid + ([-15, -1] if V % 2 else [-16])
    assert len(s) == V and sum(s) == 0
    return s


def onehot_k(M, K):
    return (37 * torch.arange(M) + 5) % K


def perm_of(N, K, seed=3):
    """-> (p (min(N, K)) int64: W[n, p[n]] = sign[n], sign)"""
    rng = np.random.default_rng(seed)
    p = torch.from_numpy(rng.permutation(K)[:min(N, K)].copy())
    sign = torch.from_numpy(rng.integers(0, 2, min(N, K)) * 2.0 - 1.0).float()
    return p, sign


@functools.lru_cache(maxsize=None)
def family(name, M, K, N):
    """-> dict(A, W, bias (or None), res (or None), epi): float32 CPU tensors, computed once per (name, shape), never modified."""
    V = K // CHUNK
    bias = res = None
    epi = EPI_NONE
    if name == 'int_coded':
        A, W, bias, res = _int_coded(M, K, N)
        epi = EPI_RESIDUAL
    elif name == 'onehot_rows':
        A = torch.zeros(M, K)
        A[torch.arange(M), onehot_k(M, K)] = 1.0
        W, bias = rnd((N, K), 11, K ** -0.5), rnd((N,), 12)
    elif name == 'perm_weight':
        A = rnd((M, K), 13)
        W = torch.zeros(N, K)
        p, sign = perm_of(N, K)
        W[torch.arange(len(p)), p] = sign
    elif name == 'cancel_chunks':
        A, W, bias = rnd((M, K), 14, 0.25), rnd((N, K), 15, K ** -0.5), rnd((N,), 16)
        alpha = 128.0 * (1.0 + (torch.arange(M) % 7).float() / 8.0)
        beta = 160.0 * (1.0 + (torch.arange(N) % 5).float() / 8.0)
        for c, s in enumerate(chunk_weights(V)):
            A[:, c * CHUNK], W[:, c * CHUNK] = alpha, s * beta
        if V == 1:
            A[:, 64], W[:, 64] = alpha, -beta
    elif name == 'mixed_cols':
        A, W = rnd((M, K), 17), rnd((N, K), 18, K ** -0.5)
        e = torch.round(torch.arange(N).float() * (MIXED_SPAN / (N - 1)))
        W = W * torch.pow(2.0, -e)[:, None]
    elif name == 'mixed_rows':
        A, W, bias = rnd((M, K), 19).clamp_(-1.99, 1.99), rnd((N, K), 20, K ** -0.5), rnd((N,), 21)
        e = torch.round(ROW_EXP[0] + torch.arange(M).float() * ((ROW_EXP[1] - ROW_EXP[0]) / (M - 1)))
        A = A * torch.pow(2.0, e)[:, None]
    elif name == 'gelu_edges':
        A, W, _, _ = _int_coded(M, K, N)
        A[:, 1::2], W[:, 1::2] = -A[:, 0::2], W[:, 0::2]                # exactly cancelling pairs (k, k + 1): a w + (-a) w = 0 in any order
        r, k0 = torch.arange(M), 2 * onehot_k(M, K // 2)                # the pair (k0, k0 + 1) of row m carries (t(m), 0) instead ...
        A[r, k0], A[r, k0 + 1] = torch.tensor(GELU_TARGETS)[r % len(GELU_TARGETS)], 0.0
        sgn = (1.0 - 2.0 * (torch.arange(N) % 2).float())[:, None]
        K0 = torch.unique(k0)                                            # ... against W[n, k0] = sign(n); the other rows keep a cancelling pair there
        W[:, K0], W[:, K0 + 1] = sgn.expand(-1, len(K0)), sgn.expand(-1, len(K0))
        bias, epi = torch.zeros(N), EPI_GELU
    elif name == 'big_epilogue':
        A, W = rnd((M, K), 22), rnd((N, K), 23, K ** -0.5)
        bias = 1e6 * (1.0 + torch.rand(N, generator=torch.Generator().manual_seed(24))) * (1.0 - 2.0 * (torch.arange(N) % 2).float())
        res = 1e6 * (1.0 + torch.rand(M, N, generator=torch.Generator().manual_seed(25))) * (1.0 - 2.0 * (torch.arange(M) % 3 == 0).float())[:, None]
        epi = EPI_RESIDUAL
    else:
        raise KeyError(name)
    return dict(A=A.contiguous(), W=W.contiguous(), bias=bias, res=res, epi=epi)


def gelu_pre(M, N):
    """The exact pre-activations of gelu_edges: t(m) * sign(n)."""
    t = torch.tensor(GELU_TARGETS, dtype=torch.float64)[torch.arange(M) % len(GELU_TARGETS)]
    return t[:, None] * (1.0 - 2.0 * (torch.arange(N) % 2).double())[None, :]


# ---- fp64 reference and gate -----------------------------------------------------------------------------------------------------------------
def gelu64(v):
    return 0.5 * v * torch.special.erfc(-v * 0.5 ** 0.5)       # (erfc: 1 + erf without the cancellation)


def reference(A, W, bias=None, res=None, epi=EPI_NONE):
    """-> dict(pre, out, S = sum_k |a w|, sa = sum_k |a| (M, 1), sw = sum_k |w| (1, N)) in fp64."""
    a, w = A.double(), W.double()
    pre = a @ w.t()
    if bias is not None:
        pre = pre + bias.double()
    out = pre
    if epi == EPI_GELU:
        out = gelu64(pre)
    elif epi == EPI_RESIDUAL:
        out = pre + res.double()
    return dict(pre=pre, out=out, S=a.abs() @ w.abs().t(), sa=a.abs().sum(1, keepdim=True), sw=w.abs().sum(1)[None, :])


def pack_scale_of(W):
    """The scale ops.pack_weight gives this matrix (the host's own rule, on the CPU)."""
    return ops.pack_scale(float(W.abs().max()))


def coef(scheme, K):
    V = K // CHUNK
    return (CHUNK + V) * U if scheme == 'f32' else (3 * CHUNK + V + 12) * U


def gate(ref, scheme, K, scale=1.0, bias=True, epi=EPI_NONE, exact_pre=False):
    """The tolerance per element.  scheme: 'f32' | 'half'; scale: pack_scale_of(W) (split halves); exact_pre: the family's pre-activation is
    exact in every kernel by construction (gelu_edges): only the epilogue terms remain."""
    floor = 0.0 if scheme == 'f32' else 2.0 ** -25 * (1.0 + 2.0 ** -10) * (ref['sa'] / scale + ref['sw'])
    pre_err = 0.0 if exact_pre else coef(scheme, K) * ref['S'] + (2 * U * ref['pre'].abs() if bias else 0.0) + floor
    if epi == EPI_GELU:
        return 1.13 * pre_err + 4 * U * ref['pre'].abs() + 3 * U * ref['out'].abs() + 1e-37
    if epi == EPI_RESIDUAL:
        return pre_err + 2 * U * ref['out'].abs()
    return pre_err


def gate_of(name, M, K, N, scheme):
    d, ref, scale = prepared(name, M, K, N)
    return gate(ref, scheme, K, scale, d['bias'] is not None, d['epi'], exact_pre=(name == 'gelu_edges'))


def scheme_of(kernel):
    return 'f32' if kernel.startswith('f32') else 'half'


# ---- sequential fp32 emulation of both operand schemes -----------------------------------------------------------------------------------------
def split_halves(x):
    """fp32 array -> (hi, lo) as float32 arrays holding IEEE-half values: hi = half(x), lo = half(x - hi) (x - hi is exact in fp32)."""
    with np.errstate(over='ignore', invalid='ignore'):
        hi = x.astype(np.float16).astype(np.float32)
        lo = (x - hi).astype(np.float16).astype(np.float32)
    return hi, lo


def emulate(A, W, bias=None, res=None, epi=EPI_NONE, scheme='f32'):
    """The documented association in numpy float32 -> (M, N) float32 tensor."""
    f = np.float32
    a, w = A.numpy(), W.numpy()
    M, K = a.shape
    N = w.shape[0]
    tot = np.zeros((M, N), f)
    if scheme == 'f32':
        aT, wT = np.ascontiguousarray(a.T).astype(np.float64), np.ascontiguousarray(w.T).astype(np.float64)
        for c in range(K // CHUNK):
            acc = np.zeros((M, N), f)
            for k in range(c * CHUNK, (c + 1) * CHUNK):           # an fp32 FMA chain: the product is exact in fp64, one rounding per step
                acc = (acc.astype(np.float64) + aT[k][:, None] * wT[k][None, :]).astype(f)
            tot = tot + acc
        v = tot
    else:
        scale = pack_scale_of(W)
        ah, al = (np.ascontiguousarray(t.T) for t in split_halves(a))
        wh, wl = (np.ascontiguousarray(t.T) for t in split_halves(w * f(scale)))
        for c in range(K // CHUNK):
            acc = np.zeros((M, N), f)
            for s in range(c * 8, c * 8 + 8):                     # 16-wide steps: lo hi, hi lo, hi hi (products of halves are exact in fp32)
                for x, y in ((al, wh), (ah, wl), (ah, wh)):
                    for k in range(s * 16, s * 16 + 16):
                        acc += x[k][:, None] * y[k][None, :]
            tot = tot + acc
        v = tot * f(1.0 / scale)
    assert v.dtype == f
    if bias is not None:
        v = v + bias.numpy()[None, :]
    if epi == EPI_GELU:
        x = v * f(0.70710678118654752440)
        e = torch.erf(torch.from_numpy(x).double()).float().numpy()
        v = (f(0.5) * v) * (f(1.0) + e)
    elif epi == EPI_RESIDUAL:
        v = v + res.numpy()
    assert v.dtype == f
    return torch.from_numpy(v)


def exactness_preconditions(K, M=384, N=1536):
    """int_coded at the largest K used: every partial sum an integer below 2^24 (bias and residual included), every operand and its pack-scaled image
    exact in half with a zero lo half.  -> the bound on the partial sums."""
    A, W, bias, res = _int_coded(M, K, N)
    bound = float(A.abs().max() * W.abs().max()) * K + float(bias.abs().max()) + float(res.abs().max())
    assert bound < 2.0 ** 24, bound
    assert float((A.double() @ W.double().t()).abs().max()) <= bound
    scale = pack_scale_of(W)
    for x in (A.numpy(), W.numpy() * np.float32(scale)):
        hi, lo = split_halves(x)
        assert np.array_equal(hi, x) and not lo.any()
    assert float(W.abs().max()) * scale * bound < 2.0 ** 24 * scale       # (the packed image is the integer matrix times a power of two: exact in fp32)
    return bound


# ---- the kernels -----------------------------------------------------------------------------------------------------------------------------
def as_images(t, M):
    B, h, w = IMAGES[M]
    return t.view(B, h, w, t.shape[-1])


@functools.lru_cache(maxsize=None)
def _packed(name, M, K, N, scheme, with_bias):
    d = family(name, M, K, N)
    b = d['bias'].cuda() if (with_bias and d['bias'] is not None) else None
    return ops.pack_weight(d['W'].cuda(), b, bf16=ops.GSPLIT if scheme == 'half' else 0)


def run(name, M, K, N, kernel, split_k, epi=None, with_bias=True, A=None, out=None):
    """One launch of `kernel` on a family (epi: the family's own unless given) -> (M, N) CUDA tensor."""
    d = family(name, M, K, N)
    epi = d['epi'] if epi is None else epi
    pw = _packed(name, M, K, N, scheme_of(kernel), with_bias)
    x = as_images((d['A'] if A is None else A).cuda(), M)
    r = as_images(d['res'].cuda(), M) if epi == EPI_RESIDUAL else None
    return ops.conv2d(x, pw, epilogue=epi, res=r, split_k=split_k, out=out).view(M, N)


def bits_equal(a, b):
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def ratio(got, ref, tol):
    """Largest |got - ref| / tol over the elements (inf where got is not finite) and the largest |error|."""
    d = (got.double().cpu() - ref['out']).abs()
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, float('inf')))
    return float((d / tol).max()), float(d.max())


@functools.lru_cache(maxsize=None)
def prepared(name, M, K, N):
    """The family, its fp64 reference and pack scale: once per (name, shape)."""
    d = family(name, M, K, N)
    return d, reference(d['A'], d['W'], d['bias'], d['res'], d['epi']), pack_scale_of(d['W'])


@functools.lru_cache(maxsize=None)
def emulated(name, M, K, N, scheme):
    """-> (largest error / gate, largest |error|) of the emulation."""
    d, ref, scale = prepared(name, M, K, N)
    tol = gate_of(name, M, K, N, scheme)
    return ratio(emulate(d['A'], d['W'], d['bias'], d['res'], d['epi'], scheme), ref, tol)


def case(name, M, K, N, kernel, emulate_too=True):
    """A gate family on one kernel, every split count that reaches it -> dict(ratio, err, emu_ratio, emu_err, splits) or None (no route)."""
    ks = routes(kernel, M, K, N)
    if not ks:
        return None
    d, ref, scale = prepared(name, M, K, N)
    sch = scheme_of(kernel)
    tol = gate_of(name, M, K, N, sch)
    worst = (0.0, 0.0)
    for sk in ks:
        worst = max(worst, ratio(run(name, M, K, N, kernel, sk), ref, tol))
    er = emulated(name, M, K, N, sch) if emulate_too else (math.nan, math.nan)
    return dict(ratio=worst[0], err=worst[1], emu_ratio=er[0], emu_err=er[1], splits=ks)


if __name__ == '__main__':
    bad = 0
    for fam in GATE_FAMILIES:
        for shape in GATE_SHAPES:
            for kern in KERNELS:
                r = case(fam, *shape, kern)
                if r is None:
                    continue
                ok = r['ratio'] <= 1.0
                bad += not ok
                print(f'[{"ok" if ok else "FAIL"}] {fam:13s} {shape} {kern:8s} split_k {r["splits"]}: kernel max|d| {r["err"]:.3e} = {r["ratio"]:.3f} of the gate'
                      f' | emulation {r["emu_err"]:.3e} = {r["emu_ratio"]:.3f}', flush=True)
    sys.exit(1 if bad else 0)
