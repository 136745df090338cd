"""-m gpu: the five token-GEMM kernels of the Transformer's Linear layers on exact, cancelling and off-grid inputs.

The families, the fp64 reference, the per-element gate with its derivation, the routes and the CPU emulation live in tools/gemm_check.py;
tests/test_token_gemm_families_host.py proves on the CPU that the emulation stays within 0.5 of the gate, so every condition here is a
condition on the reference.  Every launch goes through ops.conv2d with an explicit split_k; gemm_check.routes() says which split_k reaches which
kernel at a shape, by these rules of the C ABI:
  f32_sk    conv_dispatch (cf_igemm.hip): taps 1, fp32 operands, split_k >= 1 -> launch_sk<2,2,1,1>, unless cf_gemm_f32_tile_try takes it
  f32_tile  cf_gemm_f32_tile_try: split_k == 1, M % 128 == 0, cout_pad == cout, not 512 -> 512
  h_sk      cf_gemm_split_launch: its last launch -- nsplit >= 2, or nsplit == 1 with M % 128 != 0 (the workspace-free epilogue)
  h_tile    cf_gemm_split_launch: `nsplit == 1 && M % 128 == 0`
  h_wg      cf_gemm_split_launch: `split_k == CF_SPLITK_IN_WORKGROUP` (M % 32 == 0, K <= 1024)
M is formed as images: 4x8 -> 32, 8x8 -> 64, 16x16 -> 256 (gemm_check.IMAGES).  Nothing is larger than 384 x 1152 x 1536.

Measured on an MI355X, the whole file 3.4 s (48 cases).  Largest |error| / gate per family and kernel (the CPU emulation: fp32 | split halves):
                   f32_sk   f32_tile  h_sk     h_tile   h_wg       emulation
    cancel_chunks  0.0575   0.0575    0.0118   0.0118   0.0114     0.058 | 0.019
    mixed_cols     0.0074   0.0054    0.0861   0.0777   0.0861     0.007 | 0.086
    mixed_rows     0.4928   0.4920    0.1443   0.1257   0.1443     0.493 | 0.144
    gelu_edges     0.0820   0.0820    0.0820   0.0820   0.0820     0.082 | 0.082
    big_epilogue   0.4915   0.4890    0.4911   0.4885   0.4911     0.492 | 0.491
(the fp32 kernels return the emulation's FMA chain bit for bit on most cases; mixed_rows / big_epilogue sit at one bias / residual rounding.)
The kernels needed no change and the C ABI refuses every shape of the refusal list.  Scratch builds of cf_gemm_split.hip with one in-range edit
each (not committed), tests of this file that fail | of the four token-GEMM tests of test_gpu_split.py:
  (a) a0 / a1 reads swapped in compute of gemm_f32_tile_kernel        15 (int_coded, onehot, permutation, every f32_tile gate, bitwise, batch, counters) | 3
  (b) store_stage of gemm_f32_tile_kernel without (row >> 2) & 3       the same 15 | 3
  (c) gemm_split_tile_kernel skips tot += acc of the last chunk        18 | 2
  (d) in-workgroup kernel adds the chunk sums in reverse order         4: the bitwise contracts and batch invariance on cancel_chunks and mixed_cols; every accuracy
                                                                       case passes | 1 (test_split_half_token_gemm: its split-count bits on randn)
  (e) `>` for `>=` in gs_rows                                          2: the alt_from edges only | 1 (alt_from = 1024 is a tile boundary as well)
  (f) gemm_split_kernel without its lo hi MFMA (every nsplit)          9: permutation, mixed_cols / mixed_rows gates of h_sk, bitwise, batch, counters | 2
With chunk weights of EQUAL size (+S, -S, ..) edit (d) passed cancel_chunks: every chunk addition was exact; the weights are unequal for that reason.
"""
import pytest

from _tools import load_script

pytestmark = pytest.mark.gpu

KERNELS = ('f32_sk', 'f32_tile', 'h_sk', 'h_tile', 'h_wg')
# (M, K, N): V = 3 and 5 (odd, > 1), V = 1 (the tile kernels' prologue requests stages 0..2 of 4), V = 8 (the in-workgroup form's largest), V = 9 (beyond
# it); M tile counts 1, 3 (odd), M = 32 / 96 (in-workgroup only), 192 (nsplit == 1 of gemm_split_kernel); ntn = 1, 3, 24
EXACT_SHAPES = ((192, 384, 192), (64, 640, 64), (384, 128, 1536), (128, 1152, 64), (256, 1024, 192), (32, 384, 64), (96, 640, 192))


@pytest.fixture(scope='module')
def gc():
    import torch
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    from codeformer_amd import lib
    lib.load()
    m = load_script('tools/gemm_check.py')
    assert m.KERNELS == KERNELS
    return m


def _launches(gc, M, K, N, kernels=KERNELS):
    return [(k, sk) for k in kernels for sk in gc.routes(k, M, K, N)]


# ---- 1. exact families -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', EXACT_SHAPES)
def test_int_coded_is_the_fp64_result_bitwise(gc, shape):
    """Every kernel, every legal split count, the epilogues none / bias / residual: torch.equal with the fp64 result."""
    import torch
    d = gc.family('int_coded', *shape)
    ran = set()
    for epi, with_bias in ((gc.EPI_NONE, False), (gc.EPI_NONE, True), (gc.EPI_RESIDUAL, True)):
        want64 = gc.reference(d['A'], d['W'], d['bias'] if with_bias else None, d['res'], epi)['out']
        want = want64.float()
        assert torch.equal(want.double(), want64)
        want = want.cuda()
        for kern, sk in _launches(gc, *shape):
            got = gc.run('int_coded', *shape, kern, sk, epi=epi, with_bias=with_bias)
            bad = int((got != want).sum())
            assert bad == 0, (shape, kern, sk, epi, with_bias, bad, float((got - want).abs().max()))
            ran.add(kern)
    assert ran, shape
    if shape[0] in (32, 96):
        assert ran == {'h_wg'}


@pytest.mark.parametrize('shape', ((384, 640, 64), (256, 1024, 192), (128, 128, 64)))
def test_onehot_rows_select_the_weight(gc, shape):
    """out[m, n] = W[n, k(m)] + b[n]: bitwise fp32(W + b) with fp32 operands; within the 22-bit split of W (and the absolute 2^-25 / scale of a
    subnormal lo half, and the bias add) with split halves."""
    import torch
    M, K, N = shape
    d = gc.family('onehot_rows', *shape)
    k = gc.onehot_k(M, K)
    sel = d['W'][:, k].t().contiguous()
    want32 = (sel + d['bias'][None, :]).cuda()
    want64 = sel.double() + d['bias'].double()[None, :]
    scale = gc.pack_scale_of(d['W'])
    tol = 2.0 ** -22 * sel.double().abs() + 2.0 ** -25 / scale + 2 * gc.U * want64.abs()
    for kern, sk in _launches(gc, *shape):
        got = gc.run('onehot_rows', *shape, kern, sk)
        if gc.scheme_of(kern) == 'f32':
            assert gc.bits_equal(got, want32), (shape, kern, sk, float((got - want32).abs().max()))
        else:
            err = (got.double().cpu() - want64).abs()
            assert bool((err <= tol).all()), (shape, kern, sk, float((err / tol).max()))


@pytest.mark.parametrize('shape', ((256, 128, 192), (384, 1152, 64), (192, 640, 1536)))
def test_signed_permutation_weight_copies_the_tokens(gc, shape):
    """out[m, n] = +-A[m, p(n)] (zero columns where N > K): bitwise with fp32 operands, within the 22-bit split of A with split halves."""
    import torch
    M, K, N = shape
    d = gc.family('perm_weight', *shape)
    p, sign = gc.perm_of(N, K)
    want = torch.zeros(M, N)
    want[:, :len(p)] = d['A'][:, p] * sign[None, :]
    tol = (2.0 ** -22 + gc.U) * want.double().abs() + 2.0 ** -25
    for kern, sk in _launches(gc, *shape):
        got = gc.run('perm_weight', *shape, kern, sk).cpu()
        if gc.scheme_of(kern) == 'f32':
            assert bool((got == want).all()), (shape, kern, sk, float((got - want).abs().max()))
        else:
            err = (got.double() - want.double()).abs()
            assert bool((err <= tol).all()), (shape, kern, sk, float((err / tol).max()))


# ---- 2. gate families ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('family', ('cancel_chunks', 'mixed_cols', 'mixed_rows', 'gelu_edges', 'big_epilogue'))
def test_family_within_the_gate(gc, family, kernel):
    """The per-element gate on every kernel, every split count that reaches it; the measured / gate ratio is printed, may not exceed 1 and may not
    fall below 1e-3 of the emulation's (a gate that loose would check nothing)."""
    worst, emu = 0.0, 0.0
    for shape in gc.GATE_SHAPES:
        r = gc.case(family, *shape, kernel)
        if r is None:
            continue
        print(f'{family} {shape} {kernel} split_k {r["splits"]}: max|d| {r["err"]:.3e} = {r["ratio"]:.4f} of the gate | emulation {r["emu_err"]:.3e} = {r["emu_ratio"]:.4f}')
        worst, emu = max(worst, r['ratio']), max(emu, r['emu_ratio'])
    assert emu > 0.0                       # the kernel ran on at least one shape
    assert worst <= 1.0, (family, kernel, worst)
    assert worst >= 1e-3 * emu, (family, kernel, worst, emu)


# ---- 3. the bitwise contracts on the hard families -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', ('cancel_chunks', 'mixed_cols'))
def test_kernels_and_split_counts_agree_bitwise(gc, family):
    """Per operand scheme ONE result: every split count, fp32 tile kernel == fp32 split-K instantiation, split-half tile == cross-workgroup ==
    in-workgroup."""
    seen = set()
    for shape in ((256, 1024, 64), (128, 640, 64), (384, 384, 1536), (128, 512, 512)):      # (512 -> 512: split_k 1 stays on the split-K instantiation)
        for scheme, kernels in (('f32', ('f32_tile', 'f32_sk')), ('half', ('h_tile', 'h_sk', 'h_wg'))):
            outs = [(k, sk, gc.run(family, *shape, k, sk)) for k, sk in _launches(gc, *shape, kernels)]
            assert len(outs) >= 2 and (shape[1:] == (512, 512) or {k for k, _, _ in outs} == set(kernels)), (shape, [o[:2] for o in outs])
            seen |= {k for k, _, _ in outs}
            for k, sk, y in outs[1:]:
                assert gc.bits_equal(y, outs[0][2]), (family, shape, outs[0][:2], (k, sk), int((y != outs[0][2]).sum()))
    assert seen == set(KERNELS)


@pytest.mark.parametrize('family', ('cancel_chunks', 'mixed_cols'))
def test_an_image_alone_equals_the_image_inside_a_batch(gc, family):
    """Six 8x8 images (384 rows: the tile kernels), images 3..5 as a batch of three (192 rows: the split-K instantiation / gemm_split_kernel with
    nsplit == 1 / the in-workgroup form), image 4 alone (64 rows, a split): the same bits per row."""
    from codeformer_amd import ops
    M, K, N = 384, 640, 64
    d = gc.family(family, M, K, N)
    x6 = gc.as_images(d['A'].cuda(), M)
    for scheme, code in (('f32', 0), ('half', ops.GSPLIT)):
        pw = gc._packed(family, M, K, N, scheme, True)
        y6 = ops.conv2d(x6, pw, split_k=1)
        x3, x1 = x6[3:6].contiguous(), x6[4:5].contiguous()
        for sk in ([1, 5] + ([ops.SPLITK_IN_WORKGROUP] if code else [])):
            assert gc.bits_equal(ops.conv2d(x3, pw, split_k=sk), y6[3:6]), (family, scheme, sk)
            assert gc.bits_equal(ops.conv2d(x1, pw, split_k=sk), y6[4:5]), (family, scheme, sk)


@pytest.mark.parametrize('family', ('cancel_chunks', 'mixed_cols'))
def test_two_token_matrices_at_the_extreme_alt_from(gc, family):
    """x_alt with alt_from at its first (128) and last (N - 128) legal value: bitwise the two single-matrix launches, in the three split-half kernels."""
    import torch
    from codeformer_amd import ops
    M, K, N = 128, 384, 1536
    d = gc.family(family, M, K, N)
    pw = gc._packed(family, M, K, N, 'half', True)
    xa = gc.as_images(d['A'].cuda(), M)
    xb = gc.as_images(torch.flip(d['A'], dims=(0,)).contiguous().cuda() * 0.5, M)
    for sk in (1, 3, ops.SPLITK_IN_WORKGROUP):
        ya, yb = ops.conv2d(xa, pw, split_k=sk).view(M, N), ops.conv2d(xb, pw, split_k=sk).view(M, N)
        assert not torch.equal(ya, yb)
        for alt in (128, N - 128):
            both = ops.conv2d(xa, pw, x_alt=xb, alt_from=alt, split_k=sk).view(M, N)
            assert gc.bits_equal(both[:, :alt], ya[:, :alt]) and gc.bits_equal(both[:, alt:], yb[:, alt:]), (family, sk, alt)


# ---- 4. the split-K counters across shapes ---------------------------------------------------------------------------------------------------
def test_counters_stay_zero_across_shapes(gc):
    """One stream, one cached counter buffer: many tiles, then fewer, then more, then the first shape again -- each result the bits of split_k = 1,
    the counters all zero afterwards."""
    import torch
    from codeformer_amd import ops
    seq = (((256, 1024, 192), 8), ((64, 640, 64), 5), ((384, 384, 1536), 3), ((256, 1024, 192), 8))      # 12 (fp32: N padded to 256, 16), 1, 144, 12 tiles
    dev = torch.device('cuda', torch.cuda.current_device())
    key = (str(dev), torch.cuda.current_stream(dev).cuda_stream)
    cached = None
    for ktile, ksk in (('f32_tile', 'f32_sk'), ('h_tile', 'h_sk')):
        base = {}
        for shape, _ in seq:
            k1 = [k for k in (ktile, ksk) if 1 in gc.routes(k, *shape)]       # whichever kernel split_k = 1 reaches at this shape
            base[shape] = gc.run('cancel_chunks', *shape, k1[0], 1)
        for shape, ns in seq:
            assert ns in gc.routes(ksk, *shape)
            assert gc.bits_equal(gc.run('cancel_chunks', *shape, ksk, ns), base[shape]), (ksk, shape, ns)
            assert key in ops._COUNTERS and (cached is None or ops._COUNTERS[key] is cached)      # one buffer, under this device and stream
            cached = ops._COUNTERS[key]
    t = ops._counters(dev, 1)
    assert t is ops._COUNTERS[key] and t is cached and int(t.abs().sum()) == 0      # the buffer the launches used, not a fresh one


# ---- 5. containment --------------------------------------------------------------------------------------------------------------------------
# (M, K, N) and the kernels reached there: N = 192 is padded to 256 in the fp32 packing, which cf_gemm_f32_tile_try does not take, so the tile kernels
# get a shape of their own (N = 64 == cout_pad); every split_k comes from gemm_check.routes(), which must name a route for each kernel listed
@pytest.mark.parametrize('shape,kernels', (((192, 1024, 192), ('f32_sk', 'h_sk', 'h_wg')), ((128, 1024, 64), ('f32_tile', 'h_tile'))))
def test_non_finite_inputs_stay_in_their_row_and_column(gc, shape, kernels):
    """A NaN in one row of A: exactly that output row NaN.  An inf in one row of W: exactly that column non-finite.  GELU of a large negative finite
    pre-activation: 0, not NaN.  A token beyond the half range (1e5 > 65504): fp32 operands stay finite and right; split halves make exactly that row
    non-finite, never a wrong finite value (the header's statement on the token range)."""
    import torch
    from codeformer_amd import ops
    M, K, N = shape
    g = torch.Generator().manual_seed(31)
    A, W, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g)      # (no exact zero: an inf meets no 0)
    rn, ro, cn = 77, 50, 30
    An, Ao, Wi = A.clone(), A.clone(), W.clone()
    An[rn, 300], Ao[ro, 123], Wi[cn, 517] = float('nan'), 1e5, float('inf')
    big = torch.zeros(N)
    big[5], big[6] = -1e30, -3.0e38
    ref_o = Ao.double() @ W.double().t() + b.double()
    img = lambda t: gc.as_images(t.cuda(), M)
    for kern in kernels:
        sks = gc.routes(kern, M, K, N)
        assert sks, (kern, shape)
        code = ops.GSPLIT if gc.scheme_of(kern) == 'half' else 0
        pw, pwi, pwg = (ops.pack_weight(w.cuda(), bb.cuda(), bf16=code) for w, bb in ((W, b), (Wi, b), (W, big)))
        for sk in sks:
            y = ops.conv2d(img(An), pw, split_k=sk).view(M, N).cpu()
            rows = torch.isnan(y).all(1)
            assert bool(rows[rn]) and int(rows.sum()) == 1 and bool(torch.isfinite(y[~rows]).all()), (kern, sk)
            y = ops.conv2d(img(A), pwi, split_k=sk).view(M, N).cpu()
            cols = (~torch.isfinite(y)).all(0)
            assert bool(cols[cn]) and int(cols.sum()) == 1 and bool(torch.isfinite(y[:, ~cols]).all()), (kern, sk)
            y = ops.conv2d(img(A), pwg, epilogue=ops.EPI_GELU, split_k=sk).view(M, N).cpu()
            assert bool(torch.isfinite(y).all()) and bool((y[:, 5:7] == 0).all()), (kern, sk)
            y = ops.conv2d(img(Ao), pw, split_k=sk).view(M, N).cpu()
            if code:
                rows = (~torch.isfinite(y)).all(1)
                assert bool(rows[ro]) and int(rows.sum()) == 1, (kern, sk)
                keep = ~rows
            else:
                keep = torch.ones(M, dtype=torch.bool)
                assert bool(torch.isfinite(y).all()), (kern, sk)
            err = (y.double() - ref_o).abs()[keep]
            assert float(err.max()) <= 1e-4 * float(ref_o.abs().max()), (kern, sk, float(err.max()))     # (the other rows, and with fp32 operands all, are the product)


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_raise_and_leave_out_untouched(gc):
    import torch
    from codeformer_amd import ops

    def refused(x, pw, N, out=None, **kw):
        B, h, w, _ = x.shape
        o = torch.full((B, h, w, N), 7.0, device='cuda') if out is None else out
        with pytest.raises((RuntimeError, ValueError)):
            ops.conv2d(x, pw, out=o, **kw)
        torch.cuda.synchronize()
        assert bool((o == 7.0).all()), kw

    g = torch.Generator().manual_seed(41)
    w384, w1152, w1536 = (torch.randn(n, k, generator=g).cuda() / k ** 0.5 for n, k in ((64, 384), (64, 1152), (1536, 384)))
    f384, h384, h1152, h1536 = ops.pack_weight(w384), ops.pack_weight(w384, bf16=ops.GSPLIT), ops.pack_weight(w1152, bf16=ops.GSPLIT), ops.pack_weight(w1536, bf16=ops.GSPLIT)
    x48, x64, x128 = (torch.randn(*gc.IMAGES[m], 384, generator=g).cuda() for m in (48, 64, 128))
    for pw in (f384, h384):                                            # M = 48: no multiple of 64 (nor of 32)
        for sk in (1, 3):
            refused(x48, pw, 64, split_k=sk)
    refused(x48, h384, 64, split_k=ops.SPLITK_IN_WORKGROUP)
    with pytest.raises(ValueError):                                    # K = 192 with split-half operands: refused when the weight is packed
        ops.pack_weight(torch.zeros(64, 192, device='cuda'), bf16=ops.GSPLIT)
    from codeformer_amd import lib as L
    junk = torch.full((64 * 192,), 7.0, device='cuda')
    assert L.load().cf_pack_linear_weight_f16x2(L.ptr(torch.zeros(64, 192, device='cuda')), 64, 192, 1.0, L.ptr(junk, dtype=None), L.stream_ptr()) != 0
    torch.cuda.synchronize()
    assert bool((junk == 7.0).all())
    for pw in (f384, h384):                                            # split_k = 2 at V = 3
        refused(x64, pw, 64, split_k=2)
    refused(torch.randn(2, 8, 8, 1152, generator=g).cuda(), h1152, 64, split_k=ops.SPLITK_IN_WORKGROUP)       # in-workgroup at K = 1152
    wide = torch.full((1, 8, 8, 128), 7.0, device='cuda')
    for sk in (1, 3, ops.SPLITK_IN_WORKGROUP):                          # a strided `out` for split-half operands
        refused(x64, h384, 64, out=wide[..., :64], split_k=sk)
    assert bool((wide == 7.0).all())
    for sk in (1, 3, ops.SPLITK_IN_WORKGROUP):                          # alt_from 64: not a multiple of 128
        refused(x128, h1536, 1536, x_alt=x128.clone(), alt_from=64, split_k=sk)
    # and the same launches are accepted once the argument is legal
    assert bool(torch.isfinite(ops.conv2d(x128, h1536, x_alt=x128.clone(), alt_from=128, split_k=3)).all())
    assert bool(torch.isfinite(ops.conv2d(x64, h384, split_k=3)).all())
