"""CPU experiment (numpy, no GPU): which interpolation points to give Winograd F(4x4,2x2) for the Upsample blocks of precision 'fp32'.
Nearest-x2 + 3x3 is four 2x2 convolutions of the low-resolution image, one per output parity (a, b); each has a Winograd form with 5x5 = 25
products per 16 outputs (1.5625 per output) against the 36 (2.25) of F(4x4,3x3) on the virtually upsampled image.  For every candidate set of
four finite points (plus infinity) this prints the error of the fp32 pipeline of the kernel -- fp32 input transform, fp32 products summed
over the channels in order, fp32 output transform, weights transformed in fp64 and rounded once -- against an fp64 direct convolution, next
to the same emulation of F(4x4,3x3) with the points of cf_wf43.hip on the upsampled image.  Usage: python tools/winograd_f42_numerics.py [C] [H]"""
import sys
import numpy as np

C = int(sys.argv[1]) if len(sys.argv) > 1 else 128
H = int(sys.argv[2]) if len(sys.argv) > 2 else 16          # low-resolution size, multiple of 4


def toom(points, m, r):
    """Transforms of F(m, r) for the finite interpolation points `points` plus infinity (Toom-Cook), as tools/winograd_f43_numerics.py builds them."""
    n = m + r - 1
    p = np.array(points, np.float64)
    AT, G = np.zeros((m, n)), np.zeros((n, r))
    for j in range(n - 1):
        AT[:, j] = p[j] ** np.arange(m)
        G[j] = p[j] ** np.arange(r) / np.prod([p[j] - p[l] for l in range(n - 1) if l != j])
    AT[m - 1, n - 1] = G[n - 1, r - 1] = 1.0
    g0 = np.random.default_rng(1)
    rows, rhs = [], []
    for _ in range(80):
        d, g = g0.standard_normal(n), g0.standard_normal(r)
        for i in range(m):
            rows.append(np.outer(AT[i] * (G @ g), d).ravel())
            rhs.append(np.dot(d[i:i + r], g))
    BT = np.linalg.lstsq(np.array(rows), np.array(rhs), rcond=None)[0].reshape(n, n)
    BT[np.abs(BT) < 1e-12] = 0.0
    return BT, G, AT


def fold(w, a, axis):
    """Taps g0 g1 g2 along `axis` -> the two taps phase a sees: [g0, g1 + g2] (rows i-1, i) / [g0 + g1, g2] (rows i, i+1)."""
    g0, g1, g2 = (np.take(w, k, axis) for k in range(3))
    return np.stack((g0, g1 + g2) if a == 0 else (g0 + g1, g2), axis)


def chan_sum32(U, V):
    """sum_c U[i,m,k,c] V[i,m,c] in fp32, the channels in order (one rounding per product-accumulate, as an fp32 FMA chain)."""
    acc = np.zeros(U.shape[:3], np.float32)
    for c in range(U.shape[3]):
        acc = (acc.astype(np.float64) + U[..., c].astype(np.float64) * V[:, :, None, c].astype(np.float64)).astype(np.float32)
    return acc


def tiles32(xp, U, BT, AT, m, oy, ox, n):
    """fp32 Winograd over n x n tiles of m x m outputs; tile (ty, tx) reads the window of xp that starts at (m ty + oy, m tx + ox)."""
    a = BT.shape[0]
    U32, BT32, AT32 = U.astype(np.float32), BT.astype(np.float32), AT.astype(np.float32)
    out = np.zeros((U.shape[2], n * m, n * m), np.float32)
    for ty in range(n):
        for tx in range(n):
            d = xp[:, ty * m + oy:ty * m + oy + a, tx * m + ox:tx * m + ox + a].astype(np.float32)
            V = np.einsum('ij,cjl->cil', BT32, d).astype(np.float32)
            V = np.einsum('cil,ml->imc', V, BT32).astype(np.float32)
            M = chan_sum32(U32, V)
            Y = np.einsum('ij,jlk->ilk', AT32, M).astype(np.float32)
            Y = np.einsum('ilk,ml->kim', Y, AT32).astype(np.float32)
            out[:, ty * m:(ty + 1) * m, tx * m:(tx + 1) * m] = Y
    return out


def upsample_f42(x, w, BT, G, AT):
    """x: (C, H, H), w: (K, C, 3, 3) -> (K, 2H, 2H): four phases of F(4x4,2x2) on the image padded by one low-resolution pixel."""
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1)))
    out = np.zeros((w.shape[0], 2 * x.shape[1], 2 * x.shape[2]), np.float32)
    for a in range(2):
        for b in range(2):
            g = fold(fold(w.astype(np.float64), a, 2), b, 3)                     # (K, C, 2, 2), fp64
            U = np.einsum('ij,kcjl,ml->imkc', G, g, G)                            # fp64, rounded once in tiles32
            out[:, a::2, b::2] = tiles32(xp, U, BT, AT, 4, a, b, x.shape[1] // 4)
    return out


def upsample_f43(x, w, BT, G, AT):
    up = np.repeat(np.repeat(x, 2, 1), 2, 2)
    U = np.einsum('ij,kcjl,ml->imkc', G, w.astype(np.float64), G)
    return tiles32(np.pad(up, ((0, 0), (1, 1), (1, 1))), U, BT, AT, 4, 0, 0, up.shape[1] // 4)


def reference(x, w):
    up = np.pad(np.repeat(np.repeat(x, 2, 1), 2, 2), ((0, 0), (1, 1), (1, 1)))
    n = 2 * x.shape[1]
    ref = np.zeros((w.shape[0], n, n))
    for ky in range(3):
        for kx in range(3):
            ref += np.einsum('kc,chw->khw', w[:, :, ky, kx], up[:, ky:ky + n, kx:kx + n])
    return ref


if __name__ == '__main__':
    rng = np.random.default_rng(0)
    x = rng.standard_normal((C, H, H)).astype(np.float32).astype(np.float64)     # (the un-normalised residual stream: no activation in front)
    w = (rng.standard_normal((C, C, 3, 3)) * np.sqrt(2.0 / (9 * C))).astype(np.float32).astype(np.float64)
    ref = reference(x, w)
    e = np.abs(upsample_f43(x, w, *toom((0, 0.5, -0.5, 2, -2), 4, 3)) - ref)
    print(f'F(4x4,3x3) on the upsampled image, points 0 +-1/2 +-2 inf: max err {e.max():.2e}  mean err {e.mean():.2e}  (output max {np.abs(ref).max():.2f}, C = {C}, {H}x{H} -> {2 * H}x{2 * H})')
    for pts in ((0, 1, -1, 2), (0, 1, -1, 0.5), (0, 1, -1, -2), (0, 1, -1, -0.5), (0, 0.5, -0.5, 1), (0, 0.5, -0.5, 2), (0, 0.5, -0.5, -1), (0, 2, -2, 1), (0, 2, -2, 0.5),
                (0, 1, -0.5, 2), (0, -1, 0.5, 2), (0, 1, -0.5, -2)):
        BT, G, AT = toom(pts, 4, 2)
        e = np.abs(upsample_f42(x, w, BT, G, AT) - ref)
        print(f'four phases of F(4x4,2x2), points {pts} inf: max err {e.max():.2e}  mean err {e.mean():.2e}')
