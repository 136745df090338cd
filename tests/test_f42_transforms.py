"""No GPU: the Winograd F(4x4,2x2) transform set of the sub-pixel Upsample form (ops.B42T / G42 / A42T, ops.fold_phase_taps, ops.f42_weights;
the kernel is the UP form of cf_wf43.hip).  In float64 the four phases reproduce nearest-x2 + 3x3 of torch.nn.functional to 1e-12 relative --
random data, a single non-zero tap, a window on the zero border -- and a float32 emulation of the kernel's pipeline (fp32 transforms, fp32
FMA chain over 128 channels, weights transformed in fp64 and rounded once) is no further from fp64 than the same emulation of the form it
replaces, F(4x4,3x3) on the upsampled image."""
import torch
import torch.nn.functional as F

from codeformer_amd import ops

B42T = torch.tensor(ops.B42T, dtype=torch.float64)
G42 = torch.tensor(ops.G42, dtype=torch.float64)
A42T = torch.tensor(ops.A42T, dtype=torch.float64)
# F(4x4,3x3) as cf_wf43.hip evaluates it: points (0, +-1/2, +-2, inf), rows of B^T scaled by D = diag(1/4, 1/4, 1/4, 1/2, 1/2, 1/4), G by D^-1
B43T = torch.tensor([[.25, 0, -1.0625, 0, .25, 0], [0, -.5, -1, .125, .25, 0], [0, .5, -1, -.125, .25, 0], [0, -.25, -.125, 1, .5, 0],
                     [0, .25, -.125, -1, .5, 0], [0, .25, 0, -1.0625, 0, .25]], dtype=torch.float64)
G43 = torch.tensor([[4, 0, 0], [-32 / 15, -16 / 15, -8 / 15], [-32 / 15, 16 / 15, -8 / 15], [1 / 15, 2 / 15, 4 / 15], [1 / 15, -2 / 15, 4 / 15], [0, 0, 4]],
                   dtype=torch.float64)
A43T = torch.tensor([[1, 1, 1, 1, 1, 0], [0, .5, -.5, 2, -2, 0], [0, .25, .25, 4, 4, 0], [0, .125, -.125, 8, -8, 1]], dtype=torch.float64)


def phases_f64(P, g):
    """P: (6, 6) low-resolution rows / columns i0 - 1 .. i0 + 4 around four positions, g: (3, 3) -> (8, 8): the outputs (2 i + a, 2 j + b) of the four
    positions per axis, every phase through A42^T [(G42 g_p G42^T) (.) (B42^T d B42)] A42 on the window that starts at (a, b)."""
    out = torch.zeros(8, 8, dtype=torch.float64)
    for a in range(2):
        for b in range(2):
            U = G42 @ ops.fold_phase_taps(g, a, b) @ G42.T
            V = B42T @ P[a:a + 5, b:b + 5] @ B42T.T
            out[a::2, b::2] = A42T @ (U * V) @ A42T.T
    return out


def direct_f64(P, g):
    """The same 8 x 8 outputs from torch.nn.functional: nearest x2 of the 6 x 6 patch, valid 3x3 correlation, the rows / columns of positions 1..4."""
    up = F.interpolate(P[None, None], scale_factor=2.0, mode='nearest')
    return F.conv2d(up, g[None, None])[0, 0, 1:9, 1:9]


def test_f42_phases_equal_nearest_upsample_conv_in_float64():
    gen = torch.Generator().manual_seed(42)
    worst = 0.0
    for _ in range(200):
        P = torch.randn(6, 6, generator=gen, dtype=torch.float64)
        g = torch.randn(3, 3, generator=gen, dtype=torch.float64)
        ref = direct_f64(P, g)
        err = float((phases_f64(P, g) - ref).abs().max() / ref.abs().max())
        worst = max(worst, err)
        assert err <= 1e-12, err
    print(f'F(4,2) phases against nearest x2 + 3x3 in float64: worst relative error {worst:.2e} over 200 windows')


def test_f42_single_tap_selects_the_right_pixel_per_phase():
    gen = torch.Generator().manual_seed(7)
    P = torch.randn(6, 6, generator=gen, dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            g = torch.zeros(3, 3, dtype=torch.float64)
            g[ky, kx] = 1.0
            ref = direct_f64(P, g)
            # what the tap reads is known in closed form too: output (2 i + a) takes upsampled row 2 i + a + ky - 1 = low-resolution row (2 i + a + ky - 1) >> 1
            iy = (torch.arange(2, 10) + ky - 1) >> 1
            ix = (torch.arange(2, 10) + kx - 1) >> 1
            assert torch.equal(ref, P[iy][:, ix])
            got = phases_f64(P, g)
            assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), (ky, kx)


def test_f42_window_on_the_zero_border():
    """A 4 x 4 image is one tile: zero padding of the LOW-RESOLUTION image by one pixel is the padding=1 of the upsampled one."""
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(4, 4, generator=gen, dtype=torch.float64)
    g = torch.randn(3, 3, generator=gen, dtype=torch.float64)
    ref = F.conv2d(F.interpolate(x[None, None], scale_factor=2.0, mode='nearest'), g[None, None], padding=1)[0, 0]
    got = phases_f64(F.pad(x, (1, 1, 1, 1)), g)
    assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


def test_f42_weights_are_the_folded_taps_in_the_transform_domain():
    gen = torch.Generator().manual_seed(5)
    w = torch.randn(3, 2, 3, 3, generator=gen)
    U = ops.f42_weights(w)
    assert U.dtype == torch.float64 and tuple(U.shape) == (4, 3, 2, 5, 5)
    for p in range(4):
        g = ops.fold_phase_taps(w.double(), p >> 1, p & 1)
        assert float((U[p, 1, 0] - G42 @ g[1, 0] @ G42.T).abs().max()) < 1e-15      # (the einsum may add in another order)
    g = w.double()[0, 0]
    assert torch.equal(ops.fold_phase_taps(g, 0, 1), torch.stack([torch.stack([g[0, 0] + g[0, 1], g[0, 2]]), torch.stack([g[1, 0] + g[1, 1] + g[2, 0] + g[2, 1], g[1, 2] + g[2, 2]])]))


def _chain32(U, V):
    """sum_c U[.., c] * V[.., c] as an fp32 FMA chain in channel order (the product is exact in fp64; one rounding per step)."""
    acc = torch.zeros(torch.broadcast_shapes(U.shape[:-1], V.shape[:-1]), dtype=torch.float32)
    for c in range(U.shape[-1]):
        acc = (acc.double() + U[..., c].double() * V[..., c].double()).float()
    return acc


def _tiles32(xp, U, BT, AT, oy, ox, n):
    """fp32 Winograd over n x n tiles of 4 x 4 outputs: xp (C, H, W) padded input, U (K, C, s, s) fp64 transform-domain weights (rounded once here);
    tile (ty, tx) reads the window at (4 ty + oy, 4 tx + ox).  -> (K, 4 n, 4 n) fp32."""
    s = BT.shape[0]
    U32, BT32, AT32 = U.float().permute(2, 3, 0, 1), BT.float(), AT.float()            # (s, s, K, C)
    out = torch.zeros(U.shape[0], 4 * n, 4 * n, dtype=torch.float32)
    for ty in range(n):
        for tx in range(n):
            d = xp[:, 4 * ty + oy:4 * ty + oy + s, 4 * tx + ox:4 * tx + ox + s].float()
            V = torch.einsum('ij,cjl->cil', BT32, d)
            V = torch.einsum('cil,ml->imc', V, BT32)                                   # (s, s, C)
            M = _chain32(U32, V[:, :, None, :])                                         # (s, s, K)
            Y = torch.einsum('ij,jlk->ilk', AT32, M)
            out[:, 4 * ty:4 * ty + 4, 4 * tx:4 * tx + 4] = torch.einsum('ilk,ml->kim', Y, AT32)
    return out


def test_f42_float32_pipeline_is_no_worse_than_f43_on_the_upsampled_image():
    gen = torch.Generator().manual_seed(2024)
    C, K, H = 128, 16, 8
    x = torch.randn(C, H, H, generator=gen)
    w = torch.randn(K, C, 3, 3, generator=gen) * (2.0 / (9 * C)) ** 0.5
    up = F.interpolate(x[None].double(), scale_factor=2.0, mode='nearest')
    ref = F.conv2d(up, w.double(), padding=1)[0]
    # today's form: F(4x4,3x3) tiles of the upsampled image
    U43 = torch.einsum('xa,kcab,yb->kcxy', G43, w.double(), G43)
    y43 = _tiles32(F.pad(up[0], (1, 1, 1, 1)), U43, B43T, A43T, 0, 0, 2 * H // 4)
    # the sub-pixel form: per phase F(4x4,2x2) tiles of the low-resolution image padded by one pixel
    U42 = ops.f42_weights(w)
    xp = F.pad(x.double(), (1, 1, 1, 1))
    y42 = torch.zeros_like(y43)
    for p in range(4):
        y42[:, (p >> 1)::2, (p & 1)::2] = _tiles32(xp, U42[p], B42T, A42T, p >> 1, p & 1, H // 4)
    e43, e42 = (y43.double() - ref).abs(), (y42.double() - ref).abs()
    print(f'fp32 emulation, {C} channels, {H}x{H} -> {2 * H}x{2 * H}, max|ref| {float(ref.abs().max()):.2f}: F(4,3) on the upsampled image max err {float(e43.max()):.3e} '
          f'mean {float(e43.mean()):.3e}; four F(4,2) phases max err {float(e42.max()):.3e} mean {float(e42.mean()):.3e}')
    assert float(e42.max()) <= float(e43.max())
