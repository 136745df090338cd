"""-m gpu: the token-selection, layout and image-boundary kernels of cf_misc.hip per element.

The cases and the references (integers or fp64, written from the definitions) live in tools/misc_check.py; tests/test_misc_check_host.py proves on
the CPU that every exactness precondition, excluded-row cap and bound holds on the reference alone.  ops.* is called where a wrapper exists;
cf_row_sqnorm and cf_vq_argmin are called through the C ABI so that scores, zz and ee are supplied exactly, and every kernel is also launched
through the C ABI into a sentinel-filled buffer to show that nothing outside its result is written.  Nothing is larger than 1024 x 1024 or 3 x 64 x 64.

Measured on an MI355X: the whole file 3.0 s, 64 tests, none above 0.3 s (the first, which loads the library; every other below 0.03 s, the CPU references
included).  Largest |error| / bound (everything not listed is bitwise and was):
    cf_row_sqnorm   dim 4: 0.25   dim 32: 0.17   dim 256: 0.026   dim 260: 0.039   dim 1024: 0.010      (random and six-decade inputs; the bound is the issue's
                    (dim / 4 + 7) u sum x^2, the derived depth 3 .. 12 roundings: the ratios fall as the bound's dim / 4 outgrows the tree's log2)
    cf_vq_argmin    |dmin - fp64| / bound: r1024x256 0.0043, r512x32 0.034, r20x260 0.0048, r1024x256_small_codes 0.0098; undecided rows 1, 0, 0, 5 of 256
                    (the bound is a worst case over dim terms; random signs cancel), and idx equals the fp64 argmin on ALL 256 rows of every case
    scores: ops.linear on the packed codebook for the two 1024 x 256 cases, a CPU fp32 matmul for r512x32 and r20x260 (K % 128 != 0).

What the first run found.  No defect in a kernel: all 62 tests of the first run passed.  Three things the issue left open or had wrong are settled here:
  * an all-NaN row returns 0x7fffffff from both argmax forms.  Both callers treat that as out of range without reading through it (codebook_gather clamps
    to the last code, label_lut maps to entry 0), so the value stays; include/codeformer_hip.h now says so, and that a NaN element is skipped (numpy.argmax
    would name it).  A NaN pixel becomes byte 0 in cf_tensor_to_img_u8, where the oracle has no defined answer: stated in the header, pinned here.
  * the issue's seven image shapes have no h * w % 4 == 2; (2, 2, 3) is added for it.
  * one fp32 spacing to either side of a half-way point does not always change the byte: for 128 of the 255 points, all at byte 64 and above, the reference's own fp32
    (v + 1) / 2 * 255 rounds the neighbour back onto k + 0.5 and half-to-even decides.  The oracle is the reference either way; the host test states the count.
The comparisons of tools/gpu_check.py against permute stay there (test_gpu_parity.py::test_group[basic] runs them at one full-size shape).

Scratch builds with one in-range edit each (not committed; arithmetic, comparisons or a mask that narrows; no address, barrier or launch geometry), each run once
through this file, tests/test_gpu_conv_ends.py and the old tests of the same kernels (the kernel tests of test_gpu_logit_guard.py, the VectorQuantizer, tensor2img and
off-grid boundary tests of test_gpu_real_images.py, the first / last conv tests of test_gpu_u8_boundary.py, test_group[basic|blocks], the layout round trip and the
boundary test of test_gpu_parity.py).  Tests that fail here | old:
  (m1) argbest: ties to the HIGHER index                  30: argmax_rows_is_numpy_argmax, ties and infinities_and_nans at all eight n; vq_argmin_integer_inputs at all five
                                                          ncodes; the operation-order case | 2 (kernel_against_topk_bitwise, test_group[basic])
  (m2) argbest2: `second` not merged across lanes         14: argmax_rows_is_numpy_argmax and ties at the seven n > 4 (n = 4 has one busy lane and passes, as it should)
                                                          | 1 (kernel_against_topk_bitwise)
  (m3) vq_argmin: zz + (ee - 2 s)                         1: vq_argmin_keeps_the_reference_operation_order | 0 -- the vq_seed11 golden does not see the order
  (m4) transpose store mask: `r < R - 1`                  7: layout_each_direction at every C | 4 (layout_round_trip, test_group[basic], [blocks], vector_quantizer_statistics)
  (m5) tensor_to_img_u8 scalar tail: RGB for BGR          5: tensor_to_img_u8_at_every_rounding_boundary at the five shapes with h * w % 4 != 0 (the packed path's three
                                                          pass, as they should) | 5 (boundary_kernels_on_sizes_off_the_vector_grid, last_conv_writes_the_bytes x 4)
  (m6) first conv, fp32 fill: `ix < a.win - 1`            0 here; 40 in tests/test_gpu_conv_ends.py (see there) | 3 (first_conv_reads_the_bytes x 2, non_temporal_variant)
Plainly: five of the six are caught by an old test too (m5 by test_boundary_kernels_on_sizes_off_the_vector_grid, which already ran the one-pixel path at three
sizes); this file adds the localisation -- which n, which lane pattern, which shape.  m3 is caught by this file alone.
"""
import pytest

from _tools import load_script

pytestmark = pytest.mark.gpu

ARGMAX_N = (4, 8, 20, 252, 256, 260, 516, 1024)
ARGMAX_ROWS = (1, 3, 5, 8, 257)
SQ_DIMS = (4, 32, 256, 260, 1024)
VQ_NCODES = (4, 20, 256, 260, 1024)
VQ_RANDOM = ('r1024x256', 'r512x32', 'r20x260', 'r1024x256_small_codes')
LAYOUT_C = (1, 3, 19, 20, 32, 33, 64)
IMG_SHAPES = ((1, 1, 1), (2, 1, 3), (3, 5, 7), (2, 3, 3), (1, 2, 2), (2, 8, 4), (1, 16, 16), (2, 2, 3))
IDX_SENTINEL = -12345
PAD = 32           # elements of sentinel in front of and behind a result (a multiple of 4: the result keeps its 16-byte alignment)


@pytest.fixture(scope='module')
def mc():
    import torch
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    m = load_script('tools/misc_check.py')
    assert (m.ARGMAX_N, m.ARGMAX_ROWS, m.SQ_DIMS, m.VQ_NCODES, tuple(m.VQ_RANDOM), m.LAYOUT_C, m.IMG_SHAPES) == (
        ARGMAX_N, ARGMAX_ROWS, SQ_DIMS, VQ_NCODES, VQ_RANDOM, LAYOUT_C, IMG_SHAPES)
    return m


@pytest.fixture(scope='module')
def native():
    from codeformer_amd import lib
    return lib.load()


def _guarded(n, dtype, fill):
    """(whole buffer, the n-element result inside it) on the GPU, PAD sentinels on either side."""
    import torch
    buf = torch.full((n + 2 * PAD,), fill, dtype=dtype, device='cuda')
    return buf, buf[PAD:PAD + n]


def _untouched(buf, n, fill):
    import torch
    return bool(torch.all(buf[:PAD] == fill)) and bool(torch.all(buf[PAD + n:] == fill))


def _abi(native, name, *args):
    from codeformer_amd import lib as L
    L.check(getattr(native, name)(*args, L.stream_ptr()), name)


# ---- 1. row argmax ---------------------------------------------------------------------------------------------------------------------------
def _check_argmax(mc, native, x, per, what):
    """Both forms through ops.*, and both through the C ABI into guarded buffers, against the references."""
    import torch
    from codeformer_amd import ops
    rows, n = x.shape
    xd = x.cuda()
    want = mc.argmax_reference(x)
    wgap, wmin = mc.gap_reference(x, per)
    got = ops.argmax_rows(xd)
    gi, gg, gm = ops.argmax_rows_gap(xd, per)
    assert got.dtype == gi.dtype == torch.int64
    assert torch.equal(got.cpu(), want), (what, 'argmax_rows', got.cpu()[got.cpu() != want][:8], want[got.cpu() != want][:8])
    assert torch.equal(gi.cpu(), want), (what, 'argmax_rows_gap idx')
    assert mc.same_bits(gg, wgap), (what, 'gap', gg.cpu(), wgap)
    assert mc.same_bits(gm, wmin), (what, 'group minimum', gm.cpu(), wmin)
    ibuf, idx = _guarded(rows, torch.int64, IDX_SENTINEL)
    _abi(native, 'cf_argmax_rows', xd.data_ptr(), rows, n, idx.data_ptr())
    assert torch.equal(idx.cpu(), want) and _untouched(ibuf, rows, IDX_SENTINEL), (what, 'cf_argmax_rows wrote past its rows')
    ibuf, idx = _guarded(rows, torch.int64, IDX_SENTINEL)
    gbuf, gap = _guarded(rows, torch.float32, mc.SENTINEL)
    mbuf, gmin = _guarded(rows // per, torch.float32, mc.SENTINEL)
    _abi(native, 'cf_argmax_rows_gap', xd.data_ptr(), rows, n, per, idx.data_ptr(), gap.data_ptr(), gmin.data_ptr())
    assert torch.equal(idx.cpu(), want) and mc.same_bits(gap, wgap) and mc.same_bits(gmin, wmin), (what, 'cf_argmax_rows_gap (C ABI)')
    assert _untouched(ibuf, rows, IDX_SENTINEL) and _untouched(gbuf, rows, mc.SENTINEL) and _untouched(mbuf, rows // per, mc.SENTINEL), what


@pytest.mark.parametrize('n', ARGMAX_N)
def test_argmax_rows_is_numpy_argmax(mc, native, n):
    """Every rows x n, three inputs each: random fp32, integers in [-3, 3] (many exact ties), the walking winner."""
    import numpy as np
    for rows in ARGMAX_ROWS:
        for kind in mc.ARGMAX_KINDS:
            x = mc.argmax_input(kind, rows, n)
            assert np.array_equal(mc.argmax_reference(x).numpy(), x.numpy().argmax(axis=1))       # no NaN here: the reference IS numpy.argmax
            _check_argmax(mc, native, x, mc.ROWS_PER_GROUP[rows], (kind, rows, n))


@pytest.mark.parametrize('n', ARGMAX_N)
def test_argmax_ties_go_to_the_lowest_index(mc, native, n):
    """The same maximum inside one 16-byte load, in two lanes, across 256-column passes, in the first and the last column."""
    x, pairs = mc.tie_rows(n)
    assert mc.argmax_reference(x).tolist() == [p[0] for p in pairs]
    _check_argmax(mc, native, x, 1, ('ties', n, pairs))


@pytest.mark.parametrize('n', ARGMAX_N)
def test_argmax_rows_with_infinities_and_nans(mc, native, n):
    """Pins, for both forms: a NaN element is never the winner (the comparisons skip it); the gap form makes that row's gap and its group's minimum
    NaN; a row with no comparable element at all returns 0x7fffffff -- the callers' out-of-range case (codebook_gather clamps it to the last code,
    label_lut maps it to entry 0), as the header states."""
    import torch
    x, names = mc.special_rows(n)
    want = mc.argmax_reference(x)
    assert want[names.index('all NaN')] == mc.NO_INDEX == 0x7fffffff and want[names.index('NaN then -inf')] == 1
    assert want[names.index('all -inf')] == 0 and want[names.index('all NaN but the last')] == n - 1
    for per in (1, 4, 12):
        _check_argmax(mc, native, x, per, ('special', n, per))
    gap, gmin = mc.gap_reference(x, 4)                                      # the pinned values, spelled out
    for name, g in (('one finite, last', float('inf')), ('one +inf', float('inf'))):
        assert gap[names.index(name)] == g
    for name in ('all -inf', 'two +inf', 'one NaN', 'NaN in place of the maximum', 'all NaN', 'NaN then -inf', 'all NaN but the last', 'NaN and +inf'):
        assert torch.isnan(gap[names.index(name)]), name
    assert torch.isnan(gmin).tolist() == [True, True, True]                 # rows 1, 5..7, 8..11
    assert torch.isnan(mc.gap_reference(x[:4], 4)[1]).tolist() == [True] and not torch.isnan(mc.gap_reference(x[2:4], 2)[1]).any()


# ---- 2. row sum of squares -------------------------------------------------------------------------------------------------------------------
def _sqnorm(native, x):
    import torch
    rows, dim = x.shape
    xd = x.cuda()
    buf, out = _guarded(rows, torch.float32, -7.0)
    _abi(native, 'cf_row_sqnorm', xd.data_ptr(), rows, dim, out.data_ptr())
    assert _untouched(buf, rows, -7.0), 'cf_row_sqnorm wrote past its rows'
    return out.cpu()


@pytest.mark.parametrize('dim', SQ_DIMS)
def test_row_sqnorm_within_its_summation_tree(mc, native, dim):
    import torch
    worst = {}
    for rows in mc.SQ_ROWS:
        x = mc.sqnorm_input('ints', rows, dim)
        want = (x.double() ** 2).sum(1)
        assert float(want.max()) < 2 ** 24
        assert torch.equal(_sqnorm(native, x).double(), want), ('ints', rows, dim)
        for kind in ('random', 'mixed'):
            x = mc.sqnorm_input(kind, rows, dim)
            got = _sqnorm(native, x)
            ratio = float(((got.double() - (x.double() ** 2).sum(1)).abs() / mc.sqnorm_bound(x)).max())
            worst[kind] = max(worst.get(kind, 0.0), ratio)
            assert ratio <= 1.0, (kind, rows, dim, ratio)
    print(f'\nrow_sqnorm dim {dim}: |err| / bound {worst} (derived depth {mc.sqnorm_depth(dim)} of {dim / 4 + 7:g})')


# ---- 3. nearest code -------------------------------------------------------------------------------------------------------------------------
def _vq(native, scores, zz, ee, dmin=True):
    import torch
    rows, ncodes = scores.shape
    s, z, e = scores.cuda().contiguous(), zz.cuda().contiguous(), ee.cuda().contiguous()
    ibuf, idx = _guarded(rows, torch.int64, IDX_SENTINEL)
    dbuf, d = _guarded(rows, torch.float32, -7.0)
    _abi(native, 'cf_vq_argmin', s.data_ptr(), z.data_ptr(), e.data_ptr(), rows, ncodes, idx.data_ptr(), d.data_ptr() if dmin else None)
    assert _untouched(ibuf, rows, IDX_SENTINEL) and _untouched(dbuf, rows, -7.0), 'cf_vq_argmin wrote past its rows'
    if not dmin:
        assert bool(torch.all(d == -7.0))
    return idx.cpu(), d.cpu()


@pytest.mark.parametrize('ncodes', VQ_NCODES)
def test_vq_argmin_integer_inputs_bitwise(mc, native, ncodes):
    """idx and dmin are the integer reference's; duplicated codes (in one load, across lanes, across passes) go to the lowest index; the nearest
    code at column 0 and at column ncodes - 1; a null dmin changes no index."""
    import torch
    for rows in mc.VQ_ROWS:
        for kind in mc.VQ_EXACT_KINDS:
            c = mc.vq_exact_input(kind, rows, ncodes)
            widx, wmin = mc.vq_exact_reference(c['d'])
            idx, dmin = _vq(native, c['scores'], c['zz'], c['ee'])
            assert torch.equal(idx, widx), (kind, rows, ncodes, idx[idx != widx][:8], widx[idx != widx][:8])
            assert torch.equal(dmin.view(torch.int32), wmin.view(torch.int32)), (kind, rows, ncodes)
            if kind == 'dups':
                assert widx.tolist() == [c['pairs'][r % len(c['pairs'])][0] for r in range(rows)] and float(wmin.abs().max()) == 0.0
            if kind == 'ends':
                assert widx.tolist() == [0 if r % 2 == 0 else ncodes - 1 for r in range(rows)]
            idx0, _ = _vq(native, c['scores'], c['zz'], c['ee'], dmin=False)
            assert torch.equal(idx0, widx), (kind, rows, ncodes, 'null dmin')


def test_vq_argmin_keeps_the_reference_operation_order(mc, native):
    """(zz + ee) - 2 s, VectorQuantizer.forward's order: on the rows where zz + (ee - 2 s) picks another code the kernel returns the first form's."""
    import torch
    c = mc.order_case()
    a, da = mc.vq_emulate(c['scores'], c['zz'], c['ee'], 'reference')
    b, _ = mc.vq_emulate(c['scores'], c['zz'], c['ee'], 'folded')
    assert len(c['rows']) >= 8 and all(a[r] != b[r] for r in c['rows'])
    idx, dmin = _vq(native, c['scores'], c['zz'], c['ee'])
    assert torch.equal(idx[c['rows']], a[c['rows']]), (idx[c['rows']], a[c['rows']], b[c['rows']])
    assert torch.equal(idx, a) and torch.equal(dmin.view(torch.int32), da.view(torch.int32))


@pytest.mark.parametrize('name', VQ_RANDOM)
def test_vq_nearest_random_against_fp64(mc, native, name):
    """zz and ee from cf_row_sqnorm, scores from ops.linear on the packed codebook (the two 1024 x 256 cases, as ops.vq_nearest does) or from a CPU
    fp32 matmul (r512x32 and r20x260: K % 128 != 0 is no shape ops.linear takes).  idx is the fp64 argmin on every decided row; dmin is within the
    bound of the fp64 minimum on every row."""
    import torch
    from codeformer_amd import ops
    rows, ncodes, dim, _, source = mc.VQ_RANDOM[name]
    z, e = mc.vq_random_input(name)
    ref = mc.vq_random_reference(name)
    undecided = int((~ref['decided']).sum())
    assert undecided <= mc.VQ_EXCLUDED_CAP * rows
    zz, ee = _sqnorm(native, z), _sqnorm(native, e)
    if source == 'ops.linear':
        scores = ops.linear(z.cuda(), ops.pack_weight(e.cuda())).cpu()
    else:
        scores = z @ e.t()
    assert scores.shape == (rows, ncodes) and scores.dtype == torch.float32
    idx, dmin = _vq(native, scores, zz, ee)
    ok = ref['decided']
    assert torch.equal(idx[ok], ref['idx'][ok]), (name, int((idx[ok] != ref['idx'][ok]).sum()))
    ratio = float(((dmin.double() - ref['dmin']).abs() / ref['bound']).max())
    print(f'\nvq_argmin {name}: {undecided} of {rows} rows undecided, idx equal on all {rows} rows: {bool(torch.equal(idx, ref["idx"]))}, '
          f'|dmin err| / bound {ratio:.4f} (scores: {source})')
    assert ratio <= 1.0, (name, ratio)
    if source == 'ops.linear':           # the wrapper the network calls gives the same answer
        widx, wmin, _ = ops.vq_nearest(z.cuda(), e.cuda())
        assert torch.equal(widx.cpu(), idx) and torch.equal(wmin.cpu().view(torch.int32), dmin.view(torch.int32))


# ---- 4. layout -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', LAYOUT_C)
def test_layout_each_direction_against_permute(mc, native, C):
    """ops.to_nhwc and ops.to_nchw separately against permute().contiguous() (the two comparisons of tools/gpu_check.py, at shapes with partial
    32x32 tiles), then the C ABI into a guarded buffer: nothing outside B*C*H*W elements is written."""
    import torch
    from codeformer_amd import ops
    for B in mc.LAYOUT_B:
        for H, W in mc.LAYOUT_HW:
            x = mc.layout_input(B, C, H, W)
            y = x.permute(0, 2, 3, 1).contiguous()
            n = x.numel()
            got = ops.to_nhwc(x.cuda())
            assert got.shape == y.shape and torch.equal(got.cpu(), y), ('to_nhwc', B, C, H, W, got.cpu()[got.cpu() != y][:8])
            got = ops.to_nchw(y.cuda())
            assert got.shape == x.shape and torch.equal(got.cpu(), x), ('to_nchw', B, C, H, W, got.cpu()[got.cpu() != x][:8])
            for name, src, want in (('cf_nchw_to_nhwc', x, y), ('cf_nhwc_to_nchw', y, x)):
                buf, out = _guarded(n, torch.float32, mc.SENTINEL)
                _abi(native, name, src.cuda().data_ptr(), B, C, H * W, out.data_ptr())
                assert torch.equal(out.cpu(), want.reshape(-1)) and _untouched(buf, n, mc.SENTINEL), (name, B, C, H, W)


# ---- 5. image boundary -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', IMG_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_img_u8_to_tensor_every_byte_in_every_plane(mc, native, shape):
    import torch
    from codeformer_amd import ops
    B, H, W = shape
    img = mc.u8_input(B, H, W)
    want = mc.u8_to_tensor_reference(img)
    for c in range(3):
        assert len(set(img[..., c].reshape(-1).tolist())) == 256
    imd = img.cuda()
    got = torch.stack([ops.img_u8_to_tensor(imd[r]) for r in range(img.shape[0])]).cpu()
    assert got.shape == want.shape and torch.equal(got, want), (shape, int((got != want).sum()))
    n = B * 3 * H * W
    buf, out = _guarded(n, torch.float32, mc.SENTINEL)
    _abi(native, 'cf_img_u8_to_tensor', imd[0].data_ptr(), B, H, W, out.data_ptr())
    assert torch.equal(out.cpu(), want[0].reshape(-1)) and _untouched(buf, n, mc.SENTINEL), shape


@pytest.mark.parametrize('shape', IMG_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_tensor_to_img_u8_at_every_rounding_boundary(mc, native, shape):
    """Every half-way point and its two fp32 neighbours, the ends, +-inf and NaN, each at every pixel of every colour plane, against the oracle's
    tensor2img_u8.  NaN: the oracle has no defined answer (a NaN -> uint8 cast); the kernel's is byte 0, as the header states."""
    import torch
    from codeformer_amd import ops
    B, H, W = shape
    t = mc.img_input(B, H, W)
    want = mc.img_reference(t)
    td = t.cuda()
    got = torch.stack([ops.tensor_to_img_u8(td[r]) for r in range(t.shape[0])]).cpu()
    assert got.dtype == torch.uint8 and got.shape == want.shape
    bad = got != want
    assert not bool(bad.any()), (shape, int(bad.sum()), got[bad][:8], want[bad][:8])
    n = B * H * W * 3
    buf, out = _guarded(n, torch.uint8, 0x5a)
    _abi(native, 'cf_tensor_to_img_u8', td[0].data_ptr(), B, H, W, out.data_ptr())
    assert torch.equal(out.cpu(), want[0].reshape(-1)) and _untouched(buf, n, 0x5a), shape
