"""CPU: the cases of tests/paste_cases.py can see what tests/test_gpu_paste_kernels.py relies on them to see.

Everything here is computed with the numpy references alone (oracle/paste_oracle.py and the restatements of paste_cases.py): the
sampling grids visit all 32 x 32 sub-pixel fractions, all 5 x 5 in/out states of the taps and at least 100 exact ties of
(v + 2^14) >> 15; the float cases give different bits under a fused multiply-add in at least a tenth of their elements; the masks of the
whole geometry product lie inside DeviceFaceHelper._region and their area gives one feathering width however it is summed; the uint8
resize cases hold ties of (v + 2^21) >> 22.  A smooth image or a single matrix in place of a case list fails these conditions."""
import math

import numpy as np
import pytest

import paste_cases as C
from oracle import paste_oracle as P

MIN_FUSED_VISIBLE = 0.10


def _differs(a, b):
    return float((a != b).mean())


# ---- sampling grids --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,fwd,dsize', C.grid_matrices())
def test_sampling_grid_visits_every_fraction_tap_state_and_ties(name, fwd, dsize):
    sh, sw = C.GRID_SRC_HW
    assert C.fraction_pairs(fwd, dsize) == {(a, b) for a in range(32) for b in range(32)}
    assert C.tap_states(fwd, dsize, sh, sw) == {(x, y) for x in range(5) for y in range(5)}
    src = C.grid_source_u8()
    assert src.min() == 0 and src.max() == 255
    for border in C.BORDERS:
        acc = C.warp_u8_acc(src, fwd, dsize, border)
        assert np.array_equal(((acc + (1 << 14)) >> 15).astype(np.uint8), P.warp_affine_u8(src, fwd, dsize, border_value=border))
        assert C.warp_ties(acc) >= 100, (border, C.warp_ties(acc))


def test_origin_grid_visits_every_fraction_and_ties_but_not_every_tap_state():
    name, fwd, dsize = C.origin_grid()
    assert C.fraction_pairs(fwd, dsize) == {(a, b) for a in range(32) for b in range(32)}
    assert len(C.tap_states(fwd, dsize, *C.GRID_SRC_HW)) == 19
    assert all(C.warp_ties(C.warp_u8_acc(C.grid_source_u8(), fwd, dsize, border)) >= 100 for border in C.BORDERS)


def test_restatements_equal_the_oracle_on_the_further_matrices():
    src = C.further_source_u8()
    f = C.mixed_f32(C.FURTHER_SRC_HW, 13)
    for name, fwd in C.further_matrices():
        acc = C.warp_u8_acc(src, fwd, C.FURTHER_DSIZE, C.BORDERS[0])
        assert np.array_equal(((acc + (1 << 14)) >> 15).astype(np.uint8), P.warp_affine_u8(src, fwd, C.FURTHER_DSIZE, border_value=C.BORDERS[0])), name
        assert np.array_equal(C.warp_f32_sums(f, fwd, C.FURTHER_DSIZE)[0], P.warp_affine_f32(f, fwd, C.FURTHER_DSIZE)), name


def test_further_matrices_do_what_their_names_say():
    src = C.further_source_u8()
    mats = dict(C.further_matrices())
    dw, dh = C.FURTHER_DSIZE
    sh, sw = C.FURTHER_SRC_HW
    border = np.array(C.BORDERS[0], np.uint8)
    out = {k: P.warp_affine_u8(src, m, C.FURTHER_DSIZE, border_value=C.BORDERS[0]) for k, m in mats.items()}
    assert np.array_equal(out['identity'][:sh, :sw], src) and (out['identity'][sh:] == border).all() and (out['identity'][:, sw:] == border).all()
    assert np.array_equal(out['shift_+5_+3'][3:3 + sh, 5:5 + sw], src)
    assert np.array_equal(out['shift_-4_-6'][:sh - 6, :sw - 4], src[6:, 4:])
    assert np.array_equal(out['rot_90_exact'][2:2 + sw, 4:4 + sh], np.rot90(src, -1))
    assert np.array_equal(out['mirror'][4:4 + sh, 2:2 + sw], src[:, ::-1])
    assert (out['shift_1e6'] == border).all()
    assert (out['singular'] == src[0, 0]).all() and not P.invert_affine(mats['singular']).any()
    assert np.linalg.det(mats['mirror'][:, :2]) < 0
    assert src.min() == 0 and src.max() == 255


# ---- a fused multiply-add is visible ---------------------------------------------------------------------------------------------------
def test_fused_four_tap_sum_is_visible():
    """On the axis-aligned grid and on the magnifications that stay over the source, where most pixels sum several non-zero taps."""
    name, fwd, dsize = C.grid_matrices()[0]
    cases = [(name, C.mixed_f32(C.GRID_SRC_HW, 14), fwd, dsize)]
    cases += [(n, C.mixed_f32(C.FURTHER_SRC_HW, 13), m, C.FURTHER_DSIZE) for n, m in C.further_matrices() if n in C.FURTHER_DENSE]
    assert len(cases) == 1 + len(C.FURTHER_DENSE)
    for name, src, fwd, dsize in cases:
        sep, fused = C.warp_f32_sums(src, fwd, dsize)
        assert np.array_equal(sep, P.warp_affine_f32(src, fwd, dsize)), name
        assert _differs(sep, fused) >= MIN_FUSED_VISIBLE, (name, _differs(sep, fused))
    for seed in (13, 14):
        v = np.abs(C.mixed_f32(C.FURTHER_SRC_HW, seed))
        assert v.min() < 1e-2 and v.max() > 1e2 and (C.mixed_f32(C.FURTHER_SRC_HW, seed) < 0).any()


@pytest.mark.parametrize('ksize,sigma', [k for k in C.GAUSS_KSIZES if k[0] >= 9])
def test_fused_gaussian_row_sum_is_visible(ksize, sigma):
    """The fixed tables for ksize <= 7 are short dyadic fractions, whose products are mostly exact: fusion shows from ksize 9 on."""
    x = np.random.default_rng(15).random((53, 57)).astype(np.float32)
    sep, fused = C.gauss_row_sums(x, ksize, sigma)
    assert _differs(sep, fused) >= MIN_FUSED_VISIBLE, _differs(sep, fused)


@pytest.mark.parametrize('with_parse', [False, True])
def test_fused_blend_is_visible(with_parse):
    canvas, face, ero, soft, parse = C.blend_inputs()
    pm = parse if with_parse else None
    for m in (ero, soft, parse):
        assert (m == 0).any() and (m == 1).any() and ((m > 0) & (m < 1)).mean() > 0.7
    assert (parse == soft).any() and (parse < soft).any() and (parse > soft).any()
    assert (canvas != np.rint(canvas)).mean() > 0.99 and canvas.min() >= 0 and canvas.max() <= 255
    full = (0, 0, canvas.shape[1], canvas.shape[0])
    assert sum(dense for _, _, dense in C.blend_matrices()) >= 3
    for name, fwd, dense in C.blend_matrices():
        if dense:                                             # the face lies over most of the canvas
            sep = C.blend_ref(canvas, face, fwd, ero, soft, full, pm)
            for k, fused in enumerate(C.blend_fused(canvas, face, fwd, ero, soft, pm)):
                assert _differs(sep, fused) >= MIN_FUSED_VISIBLE, (name, k, _differs(sep, fused))


# ---- geometry product ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('u', C.UPSCALES)
def test_masks_of_the_geometry_product_lie_inside_the_region(u):
    """For every case of the product: the support of the warped mask, of both erosions and of the soft mask lies inside
    DeviceFaceHelper._region (all zero where it returns None), and int(sqrt(area)) // 20 is the same from the float32 np.sum the
    reference takes and from math.fsum, which the device's fp64 partials approach."""
    from codeformer_amd.facelib.paste import DeviceFaceHelper
    h_up, w_up = C.FRAME_HW[0] * u, C.FRAME_HW[1] * u
    cases = [c for c in C.geometry_product() if c[0] == u]
    assert len(cases) == 384
    none, edges = 0, set()
    for _, size, angle, (cx, cy) in cases:
        aff = C.face_affine(cx, cy, size, angle)
        masks = C.oracle_masks(aff, u)
        area32 = masks[4]
        w32, w64 = int(area32 ** 0.5) // 20, int(math.fsum(masks[1].reshape(-1).tolist()) ** 0.5) // 20
        assert w32 == w64, (size, angle, cx, cy, float(area32))
        edges.add(w32)
        region = DeviceFaceHelper._region(C.paste_matrix(aff, u), h_up, w_up, (C.FACE, C.FACE))
        outside = np.ones((h_up, w_up), bool)
        if region is None:
            none += 1
        else:
            x, y, w, h = region
            assert 0 <= x and 0 <= y and w > 0 and h > 0 and x + w <= w_up and y + h <= h_up
            outside[y:y + h, x:x + w] = False
        for k, m in enumerate(masks[:4]):
            assert not m[outside].any(), (size, angle, cx, cy, k)
    assert none >= 1                                          # faces wholly outside the frame are among the cases
    assert {0, 1, 2, 3, 4} <= edges                           # and several feathering widths, the empty one included


def test_overlapping_faces_overlap_and_have_one_feathering_width():
    for u in C.UPSCALES:
        soft = []
        for aff in C.overlap_affines():
            masks = C.oracle_masks(aff, u)
            assert int(masks[4] ** 0.5) // 20 == int(math.fsum(masks[1].reshape(-1).tolist()) ** 0.5) // 20
            soft.append(masks[3] > 0)
        assert all((soft[i] & soft[j]).any() for i, j in ((0, 1), (0, 2), (1, 2)))


def test_pipeline_cases_cover_every_size_angle_and_centre():
    for u in C.UPSCALES:
        cases = C.pipeline_cases(u)
        assert len(cases) >= 64 and len(set(cases)) == len(cases) and set(cases) <= set(C.geometry_product())
        for column, values in ((1, C.SIZES), (2, C.ANGLES), (3, C.CENTRES)):
            for v in values:
                assert sum(c[column] == v for c in cases) >= 3, (u, v)


# ---- resize ties -----------------------------------------------------------------------------------------------------------------------
def test_resize_cases_hold_ties():
    """Every source of more than one pixel holds a tie of (v + 2^21) >> 22 somewhere in its targets (a one-pixel source has none: its
    accumulator is v << 22), and the accumulator restated here is the oracle's."""
    total = 0
    for shape in C.RESIZE_SOURCES:
        src = C.resize_source_u8(shape)
        ties = 0
        for dh, dw in C.resize_targets(*shape):
            acc = C.resize_u8_acc(src, (dw, dh))
            assert np.array_equal(((acc + (1 << 21)) >> 22).astype(np.uint8), P.resize_linear_u8(src, (dw, dh))), (shape, dh, dw)
            ties += C.resize_ties(acc)
        assert ties >= 1 or shape == (1, 1), shape
        total += ties
    assert total >= 1
    assert all((s, s2) in C.resize_targets(s, s2) for s, s2 in C.RESIZE_SOURCES)       # identity is among the targets


# ---- the small references ----------------------------------------------------------------------------------------------------------------
def test_small_references():
    v = C.trunc_values()
    assert np.array_equal(C.trunc_ref(v), v.astype(np.uint8)) and len(v) == 770 and v.min() == 0 and v.max() < 256
    assert np.array_equal(C.trunc_ref(v)[256:512], np.arange(256)) and C.trunc_ref(v)[-2:].tolist() == [0, 0]
    for nlut in (19, 32):
        lut, labels = C.lut_table(nlut), C.lut_labels(nlut)
        want = [lut[l] if 0 <= l < nlut else 0.0 for l in labels.tolist()]
        assert C.label_lut_ref(labels, lut).tolist() == want and len(set(lut)) == nlut and 0.0 not in lut
    x = np.arange(70, dtype=np.float32).reshape(2, 5, 7) + 1
    assert not C.scale_clear_border_ref(x, 3, 0.5).any()
    assert np.array_equal(C.scale_clear_border_ref(x, 0, 0.5), x * np.float32(0.5))
    assert np.count_nonzero(C.scale_clear_border_ref(x, 2, 0.5)) == 2 * 1 * 3
    for n in C.SUM_LENGTHS:
        ch = C.sum_chunks(n)
        assert ch[0][0] == 0 and max(hi for _, hi in ch) == n and all(a[1] == b[0] or b[0] == n for a, b in zip(ch, ch[1:]))
