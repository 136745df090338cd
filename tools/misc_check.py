#!/usr/bin/env python
"""The cases and references of the token-selection, layout and image-boundary kernels (cf_misc.hip): cf_argmax_rows / cf_argmax_rows_gap,
cf_row_sqnorm / cf_vq_argmin, cf_nchw_to_nhwc / cf_nhwc_to_nchw, cf_img_u8_to_tensor / cf_tensor_to_img_u8.

Everything here is numpy / torch on the CPU, in integers or fp64, written from the definition of the operation; nothing is imported from
codeformer_amd (the one exception is oracle.codeformer_oracle.tensor2img_u8, the restatement of the reference's tensor2img).  The fp32
emulations (`*_emulate`) restate the kernels' operation ORDER so that tests/test_misc_check_host.py can prove, without a GPU, that every bound
below leaves room for the arithmetic it bounds.  tests/test_gpu_misc_kernels.py runs the kernels against these references.

Bounds, each derived from the operation count and the operand magnitudes (u = 2^-24, the unit roundoff of fp32):

  cf_row_sqnorm.  A lane squares four elements (one rounding each), adds them as (a + b) + (c + d) (two more levels), adds that group to its
  running sum once per 256-column pass, and the wave sum is a 6-step butterfly.  Adding an exact zero rounds nothing, so a term goes through
  depth(dim) = 3 + (ceil(dim / 256) - 1) + ceil(log2(min(64, dim / 4))) roundings: 3 at dim 4, 12 at dim 1024.  Every term is >= 0, so
  |err| <= depth * u * sum x^2 (1 + O(u)).  The asserted bound is the issue's, (dim / 4 + 7) * u * sum x^2, which is >= the derived one at
  every dim (sqnorm_depth <= dim / 4 + 7: the host test checks all five); the ratios the GPU test prints are against the asserted bound.

  cf_vq_argmin, random family.  d_j = (zz + ee_j) - 2 s_j with zz, ee_j from cf_row_sqnorm and s_j from a dim-term fp32 dot product:
  |err(zz)| <= (dim / 4 + 7) u zz, |err(ee_j)| likewise, |err(2 s_j)| <= dim u 2 |z|.|e_j| whatever the order of the dot product's additions,
  and the add and the subtract round twice more on values no larger than zz + ee_j + 2 |z|.|e_j|.  Sum: <= (dim + 4) u (zz + ee_j + 2 |z|.|e_j|)
  =: bound[r][j] (dim / 4 + 7 + 2 <= dim + 4 for dim >= 4).  A row's winner is decided when the fp64 margin (second smallest minus smallest
  distance) exceeds 2 * max_j bound[r][j]; its dmin is within max_j bound[r][j] of the fp64 minimum on EVERY row (|min a - min b| <= max |a - b|).

  Everything else is bitwise: integers below 2^24 are exact in fp32, a layout change moves bits, a byte has 256 values.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

U = 2.0 ** -24
NO_INDEX = 0x7fffffff            # what both argmax forms return for a row without a single comparable element (all NaN)

# ------------------------------------------------------------------------------------------------------------------ row argmax
ARGMAX_N = (4, 8, 20, 252, 256, 260, 516, 1024)
ARGMAX_ROWS = (1, 3, 5, 8, 257)
ARGMAX_KINDS = ('random', 'ints', 'walking')
ROWS_PER_GROUP = {1: 1, 3: 3, 5: 1, 8: 4, 257: 257}
# column pairs that hold the same maximum: inside one 16-byte load; in two lanes; one 256-column pass apart in the SAME lane; lane 63 of pass 0
# against lane 0 of pass 1 (the lower index sits in the higher lane); the last column of a pass against the first of the next; both ends
TIE_PAIRS = ((1, 2), (2, 9), (3, 259), (252, 256), (255, 256), (0, -1), (5, 6, 7), (0, 1, 2, 3))


def walking_column(r, n):
    """The winner's column of row r: 0, n-1, 1, n-2, ... -- from both ends, so that a few rows reach the first and the last column and 257
    rows reach every lane of both the first and the last pass."""
    return (r // 2) % n if r % 2 == 0 else (n - 1 - r // 2) % n


def argmax_input(kind, rows, n):
    g = torch.Generator().manual_seed(1000 * n + rows)
    if kind == 'random':
        return torch.randn(rows, n, generator=g)
    if kind == 'ints':
        return torch.randint(-3, 4, (rows, n), generator=g).float()
    assert kind == 'walking'
    x = ((torch.arange(rows) % 7).float() - 3.0).view(rows, 1).repeat(1, n)
    for r in range(rows):
        x[r, walking_column(r, n)] += 1.0
    return x


def tie_rows(n):
    """One row per TIE_PAIRS entry that fits n: negative noise, and the same maximum at every column of the entry."""
    g = torch.Generator().manual_seed(77 + n)
    rows, pairs = [], []
    for cols in TIE_PAIRS:
        cols = tuple(sorted(c % n if c < 0 else c for c in cols))
        if cols[-1] >= n or len(set(cols)) != len(cols):
            continue
        x = -torch.rand(n, generator=g) - 1.0
        x[list(cols)] = 0.5
        rows.append(x)
        pairs.append(cols)
    return torch.stack(rows), pairs


def special_rows(n):
    """Rows holding -inf, +inf and NaN; names in order.  n >= 4."""
    g = torch.Generator().manual_seed(99 + n)
    inf, nan = float('inf'), float('nan')
    x = torch.randn(12, n, generator=g)
    names = []
    x[0, ::2] = -inf; names.append('every other -inf')
    x[1, :] = -inf; names.append('all -inf')                                  # every element ties: index 0, gap NaN
    x[2, :] = -inf; x[2, n - 1] = -3.0; names.append('one finite, last')       # second is -inf: gap +inf
    x[3, :] = -inf; x[3, n - 1], x[3, 1] = -3.0, -7.0; names.append('two finite')
    x[4, n - 2] = inf; names.append('one +inf')                               # gap +inf
    x[5, 1] = x[5, n - 1] = inf; names.append('two +inf')                     # gap inf - inf = NaN
    x[6, 2] = nan; names.append('one NaN')
    x[7, int(x[7].argmax())] = nan; names.append('NaN in place of the maximum')
    x[8, :] = nan; names.append('all NaN')
    x[9, :] = -inf; x[9, 0] = nan; names.append('NaN then -inf')               # the NaN is skipped: index 1, not 0
    x[10, :] = nan; x[10, n - 1] = -2.0; names.append('all NaN but the last')
    x[11, 0] = nan; x[11, 3] = inf; names.append('NaN and +inf')
    return x, names


def argmax_reference(x):
    """Lowest index of the largest comparable (non-NaN) element; NO_INDEX for a row that has none.  numpy.argmax where no NaN is present."""
    a = x.numpy()
    out = np.empty(a.shape[0], dtype=np.int64)
    for r, row in enumerate(a):
        ok = ~np.isnan(row)
        if not ok.any():
            out[r] = NO_INDEX
        elif ok.all():
            out[r] = int(np.argmax(row))
        else:
            m = row[ok].max()
            out[r] = int(np.flatnonzero(ok & (row == m))[0])
    return torch.from_numpy(out)


def gap_reference(x, per):
    """(gap, group minimum) as fp32 tensors: topk(2) difference in one fp32 subtraction; NaN for a row holding a NaN (topk would rank it first);
    a NaN gap makes its group's minimum NaN."""
    top = torch.topk(x, 2, dim=-1).values
    gap = top[:, 0] - top[:, 1]
    gap[torch.isnan(x).any(dim=1)] = float('nan')
    grp = gap.view(-1, per)
    gmin = grp.min(dim=1).values
    gmin[torch.isnan(grp).any(dim=1)] = float('nan')
    return gap, gmin


def same_bits(a, b):
    """fp32 tensors equal bit for bit, every NaN counted as one value."""
    a, b = a.detach().cpu().float().contiguous(), b.detach().cpu().float().contiguous()
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.shape == b.shape and torch.equal(na, nb) and torch.equal(a[~na].view(torch.int32), b[~nb].view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------ row sum of squares
SQ_DIMS = (4, 32, 256, 260, 1024)
SQ_ROWS = (1, 5, 256)


def sqnorm_depth(dim):
    lanes = min(64, dim // 4)
    return 3 + (-(-dim // 256) - 1) + int(np.ceil(np.log2(lanes))) if lanes > 1 else 3 + (-(-dim // 256) - 1)


def sqnorm_bound(x):
    """The asserted per-row bound, fp64: (dim / 4 + 7) u sum x^2."""
    dim = x.shape[1]
    return (dim / 4 + 7) * U * (x.double() ** 2).sum(dim=1)


def sqnorm_input(kind, rows, dim):
    g = torch.Generator().manual_seed(31 * dim + rows)
    if kind == 'ints':                    # |x| <= 7: the sum is at most 49 * 1024 < 2^24, every partial sum an integer below it
        return torch.randint(-7, 8, (rows, dim), generator=g).float()
    x = torch.randn(rows, dim, generator=g)
    if kind == 'mixed':                   # magnitudes over six decades: the large terms' roundings dwarf the small terms
        x = x * torch.pow(10.0, torch.randint(-3, 4, (rows, dim), generator=g).float())
    return x


def sqnorm_emulate(x):
    """fp32, in the kernel's order: per lane and pass (x0^2 + x1^2) + (x2^2 + x3^2), passes added in order, then the xor butterfly."""
    a = x.numpy().astype(np.float32)
    rows, dim = a.shape
    lane = np.zeros((rows, 64), dtype=np.float32)
    for c in range(0, dim, 4):
        v = a[:, c:c + 4]
        q = v * v
        lane[:, (c // 4) % 64] += (q[:, 0] + q[:, 1]) + (q[:, 2] + q[:, 3])
    o = 32
    while o:
        lane = lane + lane[:, np.arange(64) ^ o]
        o >>= 1
    return torch.from_numpy(lane[:, 0].copy())


# ------------------------------------------------------------------------------------------------------------------ nearest code, exact
VQ_NCODES = (4, 20, 256, 260, 1024)
VQ_ROWS = (1, 5, 256)
VQ_EXACT_KINDS = ('random', 'dups', 'ends')
VQ_EXACT_DIM, VQ_EXACT_MAX = 32, 60       # zz, ee, |s| <= 32 * 3600 = 115200; zz + ee and 2 s <= 230400; the distance <= 460800 < 2^24


def vq_exact_input(kind, rows, ncodes):
    """Integer-valued (scores, zz, ee) as fp32 plus the int64 distances they stand for.
    dups:  codebook rows duplicated at TIE_PAIRS; token r IS one of the duplicated codes, so its distance 0 occurs at every column of the entry.
    ends:  token r is code 0 (r even) or code ncodes - 1 (r odd), both unique."""
    g = torch.Generator().manual_seed(5000 + 7 * ncodes + rows)
    m = VQ_EXACT_MAX
    e = torch.randint(-m, m + 1, (ncodes, VQ_EXACT_DIM), generator=g)
    z = torch.randint(-m, m + 1, (rows, VQ_EXACT_DIM), generator=g)
    pairs = []
    if kind == 'dups':
        taken = set()
        for cols in TIE_PAIRS:
            cols = tuple(sorted(c % ncodes if c < 0 else c for c in cols))
            if cols[-1] >= ncodes or len(set(cols)) != len(cols) or taken & set(cols):
                continue
            taken |= set(cols)
            for c in cols[1:]:
                e[c] = e[cols[0]]
            pairs.append(cols)
        for r in range(rows):
            z[r] = e[pairs[r % len(pairs)][0]]
    elif kind == 'ends':
        for r in range(rows):
            z[r] = e[0 if r % 2 == 0 else ncodes - 1]
    s = z @ e.t()
    zz, ee = (z * z).sum(1), (e * e).sum(1)
    d = (zz.view(-1, 1) + ee.view(1, -1)) - 2 * s
    return dict(scores=s.float(), zz=zz.float(), ee=ee.float(), d=d, pairs=pairs, ints=(s, zz, ee))


def vq_exact_reference(d):
    """(idx int64, dmin fp32) of the int64 distance table: lowest index on ties."""
    idx = torch.from_numpy(np.argmin(d.numpy(), axis=1).astype(np.int64))
    return idx, d.gather(1, idx.view(-1, 1)).view(-1).float()


def vq_emulate(scores, zz, ee, order='reference'):
    """fp32 in the kernel's order ('reference': (zz + ee) - 2 s, vqgan_arch.py's) or in the other one ('folded': zz + (ee - 2 s))."""
    s, z, e = scores.numpy().astype(np.float32), zz.numpy().astype(np.float32)[:, None], ee.numpy().astype(np.float32)[None, :]
    two = np.float32(2.0)
    d = (z + e) - two * s if order == 'reference' else z + (e - two * s)
    assert d.dtype == np.float32
    idx = np.argmin(d, axis=1).astype(np.int64)
    return torch.from_numpy(idx), torch.from_numpy(d[np.arange(d.shape[0]), idx].copy())


# ------------------------------------------------------------------------------------------------------------------ nearest code, operation order
ORDER_SEED, ORDER_ROWS, ORDER_NCODES = 0, 256, 8          # the seed order_search() returns, kept as a literal (the host test repeats the search)


def _order_draw(seed):
    """zz + ee_j in [400, 600], where fp32 numbers are 2^-15 or 2^-14 apart, and scores that put the eight distances of a row within 2^-13 of
    one another: (zz + ee) rounds before the subtraction, zz + (ee - 2 s) after it, and the two pick different codes on some rows."""
    g = torch.Generator().manual_seed(seed)
    zz = 200.0 + 100.0 * torch.rand(ORDER_ROWS, generator=g)
    ee = 200.0 + 100.0 * torch.rand(ORDER_NCODES, generator=g)
    d = 1.0 + torch.rand(ORDER_ROWS, ORDER_NCODES, generator=g).double() * 2.0 ** -13
    s = ((zz.view(-1, 1).double() + ee.view(1, -1).double()) - d) / 2
    return s.float(), zz, ee


def order_search(first=0, last=200):
    """The first seed whose draw has at least 8 rows where the two orders pick different codes AND the reference order's winner is strict
    (its smallest fp32 distance occurs once), so that no tie rule is involved."""
    for seed in range(first, last):
        s, zz, ee = _order_draw(seed)
        if len(order_rows(s, zz, ee)) >= 8:
            return seed
    return None


def order_rows(s, zz, ee):
    a, _ = vq_emulate(s, zz, ee, 'reference')
    b, _ = vq_emulate(s, zz, ee, 'folded')
    z, e, sc = zz.numpy()[:, None], ee.numpy()[None, :], s.numpy()
    d = (z + e) - np.float32(2.0) * sc
    strict = (d == d.min(axis=1, keepdims=True)).sum(axis=1) == 1
    return [r for r in range(s.shape[0]) if a[r] != b[r] and strict[r]]


def order_case():
    s, zz, ee = _order_draw(ORDER_SEED)
    return dict(scores=s, zz=zz, ee=ee, rows=order_rows(s, zz, ee))


# ------------------------------------------------------------------------------------------------------------------ nearest code, random
# name: (rows, ncodes, dim, codebook scale, where the scores come from on the GPU)
VQ_RANDOM = {
    'r1024x256': (256, 1024, 256, 1.0, 'ops.linear'),
    'r512x32': (256, 512, 32, 1.0, 'cpu fp32 matmul'),          # K = 32: not a shape ops.linear takes (K % 128)
    'r20x260': (256, 20, 260, 1.0, 'cpu fp32 matmul'),          # N = 20, K = 260: likewise
    'r1024x256_small_codes': (256, 1024, 256, 0.05, 'ops.linear'),
}
VQ_EXCLUDED_CAP = 0.05


def vq_random_input(name):
    rows, ncodes, dim, scale, _ = VQ_RANDOM[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    return torch.randn(rows, dim, generator=g), torch.randn(ncodes, dim, generator=g) * scale


_VQ_REF = {}


def vq_random_reference(name):
    """fp64: (distance table, idx, dmin, row bound = max_j bound[r][j], decided rows (margin > 2 * row bound)); computed once per name."""
    if name not in _VQ_REF:
        z, e = (t.double() for t in vq_random_input(name))
        dim = z.shape[1]
        zz, ee = (z * z).sum(1), (e * e).sum(1)
        d = (zz.view(-1, 1) + ee.view(1, -1)) - 2 * (z @ e.t())
        bound = ((dim + 4) * U * (zz.view(-1, 1) + ee.view(1, -1) + 2 * (z.abs() @ e.abs().t()))).max(dim=1).values
        two = torch.topk(d, 2, dim=1, largest=False).values
        decided = (two[:, 1] - two[:, 0]) > 2 * bound
        _VQ_REF[name] = dict(d=d, idx=torch.argmin(d, dim=1), dmin=two[:, 0], bound=bound, decided=decided)
    return _VQ_REF[name]


# ------------------------------------------------------------------------------------------------------------------ layout
LAYOUT_B = (1, 3)
LAYOUT_C = (1, 3, 19, 20, 32, 33, 64)
LAYOUT_HW = ((1, 1), (5, 7), (8, 4), (33, 31))
SENTINEL = -7.0


def layout_input(B, C, H, W):
    """NCHW, every element its own flat index (< 2^24: exact in fp32), so a misplaced element names its source."""
    return torch.arange(B * C * H * W, dtype=torch.float32).view(B, C, H, W)


# ------------------------------------------------------------------------------------------------------------------ image boundary
# (B, H, W): every residue of h * w mod 4 ((2, 2, 3) is here for residue 2), second images whose first byte is not 4-byte aligned, both code paths
IMG_SHAPES = ((1, 1, 1), (2, 1, 3), (3, 5, 7), (2, 3, 3), (1, 2, 2), (2, 8, 4), (1, 16, 16), (2, 2, 3))


def u8_rounds(B, H, W):
    return -(-256 // (B * H * W))


def u8_input(B, H, W):
    """uint8 (rounds, B, H, W, 3): byte (round * npix + pixel + 85 * c) % 256 -- over the rounds every colour plane sees all 256 values."""
    n = B * H * W
    p = torch.arange(u8_rounds(B, H, W) * n).view(-1, B, H, W, 1)
    return ((p + 85 * torch.arange(3).view(1, 1, 1, 1, 3)) % 256).to(torch.uint8)


def u8_to_tensor_reference(img):
    """(..., H, W, 3) BGR bytes -> (..., 3, H, W) RGB fp32: float32(u / 255.0) in fp64 rounded once, then (v - 0.5f) / 0.5f in fp32."""
    u = img.numpy().astype(np.float64)
    v = (u / 255.0).astype(np.float32)
    v = (v - np.float32(0.5)) / np.float32(0.5)
    assert v.dtype == np.float32
    v = np.moveaxis(v[..., ::-1], -1, -3)
    return torch.from_numpy(np.ascontiguousarray(v))


def img_values():
    """fp32: every half-way point (k + 0.5) / 255 * 2 - 1, k = 0..254, with one fp32 spacing to each side; -1, 1 and one spacing outside
    both; +-inf; NaN last."""
    h = ((np.arange(255, dtype=np.float64) + 0.5) / 255.0 * 2.0 - 1.0).astype(np.float32)
    lo, hi = np.nextafter(h, np.float32(-2)), np.nextafter(h, np.float32(2))
    one = np.float32(1.0)
    ends = np.array([-one, one, np.nextafter(-one, np.float32(-2)), np.nextafter(one, np.float32(2)), -np.inf, np.inf, np.nan], dtype=np.float32)
    return torch.from_numpy(np.concatenate([np.stack([lo, h, hi], 1).reshape(-1), ends]))


NAN_BYTE = 0        # cf_tensor_to_img_u8 of a NaN: fmaxf(NaN, -1) is -1.  The oracle has no defined answer (a NaN -> uint8 cast)


def img_input(B, H, W):
    """fp32 (rounds, B, 3, H, W): value index (round + pixel + 257 * c) % nvals with rounds = nvals, so EVERY value visits every pixel of every
    colour plane: each position of a packed quad, each position of a one-at-a-time quad and of a partial last quad, each image base."""
    v = img_values()
    n = v.numel()
    p = torch.arange(B * H * W).view(1, B, 1, H, W) + torch.arange(n).view(n, 1, 1, 1, 1) + 257 * torch.arange(3).view(1, 1, 3, 1, 1)
    return v[p % n].contiguous()


def img_reference(t):
    """(rounds, B, 3, H, W) -> uint8 (rounds, B, H, W, 3) by oracle.codeformer_oracle.tensor2img_u8, NaN inputs pinned to NAN_BYTE."""
    from oracle.codeformer_oracle import tensor2img_u8
    R, B, _, H, W = t.shape
    flat = t.permute(2, 0, 1, 3, 4).reshape(3, R * B * H, W)
    nan = torch.isnan(flat)
    with np.errstate(invalid='ignore'):
        img = torch.from_numpy(np.ascontiguousarray(tensor2img_u8(torch.where(nan, torch.zeros_like(flat), flat))))
    img[nan.permute(1, 2, 0).flip(-1)] = NAN_BYTE
    return img.view(R, B, H, W, 3)


if __name__ == '__main__':
    print('argmax: n', ARGMAX_N, 'rows', ARGMAX_ROWS, 'kinds', ARGMAX_KINDS)
    print('row_sqnorm: dim', SQ_DIMS, 'rows', SQ_ROWS, 'depth', [sqnorm_depth(d) for d in SQ_DIMS])
    print('vq exact: ncodes', VQ_NCODES, 'rows', VQ_ROWS, 'kinds', VQ_EXACT_KINDS)
    print('vq order: seed', ORDER_SEED, 'rows that differ', order_case()['rows'])
    for k in VQ_RANDOM:
        r = vq_random_reference(k)
        print(f'vq random {k}: undecided rows {int((~r["decided"]).sum())} of {r["decided"].numel()} ({VQ_RANDOM[k][4]})')
    print('layout: B', LAYOUT_B, 'C', LAYOUT_C, 'HW', LAYOUT_HW)
    print('image: shapes', IMG_SHAPES, 'values', img_values().numel())
