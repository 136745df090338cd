"""-m gpu: nearest x2 + 3x3 in precision 'fp32' as four Winograd F(4x4,2x2) sub-pixel phases (the UP form of cf_wf43.hip, ops.WF42U; the
algebra is pinned on the CPU by tests/test_f42_transforms.py).

Shapes: B = 2, 32x32 -> 64x64 -- four 16x16 low-resolution blocks per image, so every image border, the interior block borders and all four
phases are in every launch (16 workgroups per image and channel tile) -- at 128 -> 128 channels (4 slabs, one channel tile) and 256 -> 256 (8
slabs, two channel tiles).  Every output element is compared with the fp64 reference (tools/conv_case.py) under the bound
tests/test_gpu_split.py::test_winograd_f43_fp32_upsampling_gather uses at |ref| > 4, 4e-5 max|ref| / 4.  That is one bound for the whole tensor at the
network's size; the per-element gate of this form (c u S + 2 u |pre|, c = cin + 15), on 1, 3 and 8 slabs, a non-square image and the mixed-scale,
cancelling, DC + ripple and single-channel families, is the route w42_up of tools/conv_check.py, run by tests/test_gpu_conv_families.py.

Impulses: a unit pixel at a corner, on an edge, on both sides of the interior block border and inside a block, each in an input channel of its
own and routed by a one-hot tap of value 81 to an output channel of its own.  The output is then 81 on the 2 x 2 footprint ((Y + ky - 1) >> 1,
(X + kx - 1) >> 1) == (i, j) -- one output of each phase -- and 0 everywhere else, BITWISE: G42 holds ninths, so with the tap 81 = 9^2 every entry of
U = G42 g_p G42^T is an integer (the one rounding at pack time is exact), B42^T d B42 of a unit impulse is a multiple of 1/4, every product is exact and
every partial sum of A42^T M A42 is a multiple of 1/256 below 2^18 / 256 -- far inside fp32's 24 bits, so no addition rounds in any order.

The packer: cf_pack_conv_weight_winograd42_up, taken apart by its documented layout, against ops.f42_weights (fp64, rounded once).
"""
import functools

import pytest

from _tools import load_script

pytestmark = pytest.mark.gpu

CASES = {'c128': (2, 32, 32, 128, 128, 101), 'c256': (2, 32, 32, 256, 256, 102)}   # B, H, W of the input, cin, cout, seed


@pytest.fixture(scope='module')
def up():
    import torch
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    from codeformer_amd import lib, ops
    lib.load()
    reference = load_script('tools/conv_case.py').reference

    @functools.lru_cache(maxsize=None)
    def case(key):
        """Inputs, the fp64 reference and ONE launch with statistics; computed once and shared, never modified."""
        B, H, W, cin, cout, seed = CASES[key]
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(B, H, W, cin, generator=g)
        w = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
        b = torch.randn(cout, generator=g) * 0.1
        ref = reference(x, w, b, prologue=ops.PRO_NONE, epilogue=ops.EPI_NONE, upsample=True)
        pw = ops.pack_weight(w.cuda(), b.cuda(), bf16=ops.WF42U)
        xc = x.cuda()
        y = ops.conv2d(xc, pw, upsample=True, emit_stats=True)
        return dict(x=xc, w=w, b=b, ref=ref, pw=pw, y=y)
    return case


@pytest.mark.parametrize('key', sorted(CASES))
def test_every_element_against_fp64(up, key):
    import torch
    from codeformer_amd import ops
    c = up(key)
    B, H, W, cin, cout, _ = CASES[key]
    y, ref = c['y'], c['ref']
    assert tuple(y.shape) == (B, 2 * H, 2 * W, cout) and y.dtype == torch.float32 and bool(torch.isfinite(y).all())
    err = (y.cpu().double() - ref).abs()
    scale = float(ref.abs().max())
    per_phase = [float(err[:, a::2, b::2].max()) for a in (0, 1) for b in (0, 1)]
    print(f'F(4,2) sub-pixel phases {H}x{W} -> {2 * H}x{2 * W} {cin}->{cout}: max err {float(err.max()):.3e} (phases {", ".join(f"{e:.2e}" for e in per_phase)}), '
          f'mean {float(err.mean()):.3e}, |ref| max {scale:.2f}, bound {4e-5 * scale / 4.0:.3e}')
    assert err.numel() == B * 4 * H * W * cout and float(err.max()) <= 4e-5 * scale / 4.0
    # the plain F(4,3) packing of the same weight keeps the form it had (F(4,3) on the upsampled image): another kernel, the same bound
    y43 = ops.conv2d(c['x'], ops.pack_weight(c['w'].cuda(), c['b'].cuda(), bf16=ops.WF43F), upsample=True)
    e43 = float((y43.cpu().double() - ref).abs().max())
    print(f'    F(4,3) upsampling gather on the same case: max err {e43:.3e}')
    assert e43 <= 4e-5 * scale / 4.0 and not torch.equal(y43, y)


def test_impulses_land_on_their_footprint_in_every_phase(up):
    import torch
    from codeformer_amd import ops
    H = W = 32
    C = 128
    TAP = 81.0                                                                                      # 9^2: U = G42 g_p G42^T is integral (see the module docstring)
    pixels = [(0, 0), (0, 17), (31, 31), (15, 15), (16, 15), (15, 16), (21, 9), (31, 4), (8, 31)]   # corners, edges, both sides of the block border, interior
    x = torch.zeros(1, H, W, C)
    for k, (i, j) in enumerate(pixels):
        x[0, i, j, 3 * k + 1] = 1.0
    xc = x.cuda()
    Y = torch.arange(2 * H)
    for ky in range(3):
        for kx in range(3):
            w = torch.zeros(C, C, 3, 3)
            want = torch.zeros(1, 2 * H, 2 * W, C)
            for k, (i, j) in enumerate(pixels):
                w[5 * k + 2, 3 * k + 1, ky, kx] = TAP
                rows, cols = ((Y + ky - 1) >> 1) == i, ((Y + kx - 1) >> 1) == j          # (a negative index is row -1: padding, never a pixel)
                want[0, :, :, 5 * k + 2] = (rows[:, None] & cols[None, :]).float() * TAP
                fp = want[0, :, :, 5 * k + 2].nonzero()
                if 0 < i < H - 1 and 0 < j < W - 1:                                      # an interior pixel: a 2 x 2 block with one output of each phase
                    assert len(fp) == 4 and {(int(p[0]) & 1, int(p[1]) & 1) for p in fp} == {(0, 0), (0, 1), (1, 0), (1, 1)}
            pw = ops.pack_weight(w.cuda(), None, bf16=ops.WF42U)
            assert torch.equal(pw.w, pw.w.round())                                       # every transform-domain weight is an integer
            got = ops.conv2d(xc, pw, upsample=True).cpu()
            bad = (got != want).nonzero()
            assert torch.equal(got, want), (ky, kx, len(bad), float((got - want).abs().max()), [tuple(int(v) for v in p) for p in bad[:8]])


def test_packed_weights_are_the_fp64_transform_rounded_once(up):
    """[4 phases][25 positions][cin / 32][cout / 16][64 lanes][8 k groups]: word j of a lane is U_p[n = 16 block + (lane & 15)][c = 32 slab + 4 j + (lane >> 4)].
    The kernel and ops.f42_weights both evaluate G42 g_p G42^T in fp64, in another order of additions: they may differ by an fp64 rounding before the one
    rounding to fp32, so an element may differ by one fp32 ulp -- or, where the sum cancels, by 2^-50 of the largest term (max |w| x 4 taps x (4/3)^2)."""
    import torch
    from codeformer_amd import ops
    c = up('c128')
    _, _, _, cin, cout, _ = CASES['c128']
    got = c['pw'].w.cpu().view(4, 5, 5, cin // 32, cout // 16, 4, 16, 8)           # phase, xi, nu, slab, block, lane >> 4, lane & 15, j
    got = got.permute(0, 4, 6, 3, 7, 5, 1, 2).reshape(4, cout, cin, 5, 5)          # phase, (block, lane & 15), (slab, j, lane >> 4), xi, nu
    want = ops.f42_weights(c['w'])
    assert got.dtype == torch.float32 and tuple(want.shape) == (4, cout, cin, 5, 5)
    err = (got.double() - want).abs()
    tol = 2.0 ** -23 * want.abs() + 2.0 ** -50 * float(c['w'].abs().max()) * 4 * (4 / 3) ** 2
    print(f'packed F(4,2) weights against fp64: {int((got != want.float()).sum())} of {got.numel()} elements differ from the fp64 value rounded once, largest |d| {float(err.max()):.3e}')
    assert bool((err <= tol).all()), float((err / tol).max())


def test_groupnorm_partials_batch_invariance_and_repeatability(up):
    import torch
    from codeformer_amd import ops
    c = up('c128')
    B, H, W, cin, cout, _ = CASES['c128']
    y, st = c['y'], c['y']._cf_stats
    assert st.parts == (2 * H // 16) * (2 * W // 16)          # one partial per workgroup = per 16x16 patch of the output, as the form it replaces
    got = st.part.view(B, 32, st.parts, 2).sum(2).cpu()
    r = y.cpu().double().view(B, 4 * H * W, 32, st.cpg)
    want = torch.stack([r.sum((1, 3)), (r * r).sum((1, 3))], -1)
    room = torch.stack([r.abs().sum((1, 3)), (r * r).sum((1, 3))], -1)      # (a group's sum may cancel: measure against the sum of magnitudes)
    assert float(((got - want).abs() / room).max()) < 1e-6
    y1 = ops.conv2d(c['x'][1:2].contiguous(), c['pw'], upsample=True, emit_stats=True)
    assert torch.equal(y1, y[1:2])
    assert torch.equal(y1._cf_stats.part.view(1, -1), st.part.view(B, -1)[1:2])
    y2 = ops.conv2d(c['x'], c['pw'], upsample=True, emit_stats=True)
    assert torch.equal(y2, y) and torch.equal(y2._cf_stats.part, st.part)
