"""-m gpu: the paste-back and alignment kernels (cf_paste.hip, through codeformer_amd.ops) per element at their edges.

Every kernel is compared with oracle/paste_oracle.py or the numpy references of tests/paste_cases.py on the cases built there, which
tests/test_paste_cases_host.py proves sharp on the CPU: every 1/32-pixel fraction pair, every in/out state of the four taps, exact ties
of both fixed-point roundings, float sums a fused multiply-add would change, windows at every corner and edge, one-pixel axes, and the
host's region arithmetic over a product of face sizes, rotations, upscales and positions.  Everything is bitwise unless a test says
otherwise."""
import math

import numpy as np
import pytest

import paste_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def env():
    import torch
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    from codeformer_amd import lib, ops
    from oracle import paste_oracle as P
    lib.load()
    return torch, ops, P


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _d2s(fwd):
    from codeformer_amd.facelib.paste import invert_affine
    return invert_affine(fwd)


def _same(got, want):
    """Bitwise equality of two float32 / uint8 arrays (so that -0.0 and 0.0 differ and equal NaNs agree)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    return np.array_equal(got.view(np.uint8), want.view(np.uint8))


def _warp_u8(torch, ops, src, fwds, dsize, border=(0, 0, 0), region=None, fill=0):
    dw, dh = dsize
    inv = _dev(torch, np.stack([_d2s(m) for m in fwds]).reshape(-1, 6))
    dst = torch.full((len(fwds), dh, dw, 3), fill, dtype=torch.uint8, device='cuda')
    ops.warp_affine_u8(_dev(torch, src), inv, dst, region=region, border=border)
    return dst.cpu().numpy()


# ---- sampling ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('border', C.BORDERS)
@pytest.mark.parametrize('name,fwd,dsize', C.grid_matrices() + [C.origin_grid()])
def test_warp_u8_on_the_fraction_grids(env, name, fwd, dsize, border):
    torch, ops, P = env
    src = C.grid_source_u8()
    got = _warp_u8(torch, ops, src, [fwd], dsize, border)[0]
    assert np.array_equal(got, P.warp_affine_u8(src, fwd, dsize, border_value=border))


@pytest.mark.parametrize('name,fwd,dsize', C.grid_matrices() + [C.origin_grid()])
def test_warp_f32_on_the_fraction_grids(env, name, fwd, dsize):
    torch, ops, P = env
    src = C.mixed_f32(C.GRID_SRC_HW, 14)
    got = ops.warp_affine_f32(_dev(torch, src), _d2s(fwd), (0, 0) + dsize).cpu().numpy()
    assert _same(got, P.warp_affine_f32(src, fwd, dsize))


def test_warp_u8_further_matrices(env):
    torch, ops, P = env
    src = C.further_source_u8()
    names, fwds = zip(*C.further_matrices())
    for border in C.BORDERS:
        got = _warp_u8(torch, ops, src, fwds, C.FURTHER_DSIZE, border)                  # one launch, one shared source
        for i, name in enumerate(names):
            assert np.array_equal(got[i], P.warp_affine_u8(src, fwds[i], C.FURTHER_DSIZE, border_value=border)), (name, border)
    sh, sw = C.FURTHER_SRC_HW
    assert np.array_equal(got[names.index('identity')][:sh, :sw], src)
    assert (got[names.index('singular')] == src[0, 0]).all()


def test_warp_f32_further_matrices(env):
    torch, ops, P = env
    src = C.mixed_f32(C.FURTHER_SRC_HW, 13)
    sd = _dev(torch, src)
    for name, fwd in C.further_matrices():
        got = ops.warp_affine_f32(sd, _d2s(fwd), (0, 0) + C.FURTHER_DSIZE).cpu().numpy()
        assert _same(got, P.warp_affine_f32(src, fwd, C.FURTHER_DSIZE)), name
    dw, dh = C.FURTHER_DSIZE                                                            # a window equals that window of the whole
    fwd = dict(C.further_matrices())['magnify_rot_inside']
    want = P.warp_affine_f32(src, fwd, C.FURTHER_DSIZE)
    for x, y, w, h in C.corner_regions(dw, dh, 7, 5) + [(11, 9, 1, 1)]:
        assert _same(ops.warp_affine_f32(sd, _d2s(fwd), (x, y, w, h)).cpu().numpy(), want[y:y + h, x:x + w]), (x, y, w, h)


def test_warp_u8_per_item_sources(env):
    """src of shape (n, sh, sw, 3): every item samples its own source."""
    torch, ops, P = env
    srcs = C.further_source_u8(seed=16, n=3)
    assert not np.array_equal(srcs[0], srcs[1]) and not np.array_equal(srcs[1], srcs[2]) and not np.array_equal(srcs[0], srcs[2])
    fwds = C.batch_matrices()
    border = C.BORDERS[0]
    got = _warp_u8(torch, ops, srcs, fwds, C.FURTHER_DSIZE, border)
    for i in range(3):
        assert np.array_equal(got[i], P.warp_affine_u8(srcs[i], fwds[i], C.FURTHER_DSIZE, border_value=border)), i
    for k in range(3):                                       # the shared-source form agrees on the item whose source it was given
        shared = _warp_u8(torch, ops, srcs[k], fwds, C.FURTHER_DSIZE, border)
        assert np.array_equal(shared[k], got[k]), k
        assert all(not np.array_equal(shared[j], got[j]) for j in range(3) if j != k), k


def test_warp_u8_region_form(env):
    torch, ops, P = env
    src = C.further_source_u8()
    fwd = dict(C.further_matrices())['magnify_rot_inside']
    dw, dh = C.FURTHER_DSIZE
    want = P.warp_affine_u8(src, fwd, C.FURTHER_DSIZE)
    for x, y, w, h in C.corner_regions(dw, dh, 7, 5) + [(11, 9, 1, 1), (0, 0, dw, dh)]:
        got = _warp_u8(torch, ops, src, [fwd], C.FURTHER_DSIZE, region=(x, y, w, h), fill=7)[0]
        ref = np.full((dh, dw, 3), 7, np.uint8)
        ref[y:y + h, x:x + w] = want[y:y + h, x:x + w]
        assert np.array_equal(got, ref), (x, y, w, h)
    assert (want != 7).all(-1).mean() > 0.9                 # the sentinel is no value of the result
    inv = _dev(torch, _d2s(fwd).reshape(1, 6))
    dst = torch.zeros(1, dh, dw, 3, dtype=torch.uint8, device='cuda')
    for region in ((dw - 3, 0, 5, 5), (0, dh - 1, 2, 2), (dw, 0, 1, 1), (-1, 0, 2, 2), (0, 0, 0, 1)):
        with pytest.raises(RuntimeError):
            ops.warp_affine_u8(_dev(torch, src), inv, dst, region=region)
    with pytest.raises(ValueError):                          # two matrices, one destination item
        ops.warp_affine_u8(_dev(torch, src), torch.cat([inv, inv]), dst)
    with pytest.raises(ValueError):                          # two sources, one destination item
        ops.warp_affine_u8(_dev(torch, C.further_source_u8(n=2)), inv, dst)
    assert not dst.any()


# ---- paste_blend alone -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('with_parse', [False, True])
def test_paste_blend(env, with_parse):
    torch, ops, P = env
    canvas, face, ero, soft, parse = C.blend_inputs()
    fd = _dev(torch, face)
    for name, fwd, _ in C.blend_matrices():
        for region in C.blend_regions():
            x, y, w, h = region
            win = (slice(y, y + h), slice(x, x + w))
            cd = _dev(torch, canvas)
            ops.paste_blend(cd, fd, _d2s(fwd), _dev(torch, ero[win]), _dev(torch, soft[win]), region,
                            parse=_dev(torch, parse[win]) if with_parse else None)
            want = C.blend_ref(canvas, face, fwd, ero, soft, region, parse if with_parse else None)
            assert _same(cd.cpu().numpy(), want), (name, region)      # the canvas outside the region included


# ---- erode -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', C.ERODE_SHAPES)
def test_erode(env, shape):
    torch, ops, P = env
    ks = C.ERODE_KS + ((C.ERODE_K_LARGE,) if max(shape) < C.ERODE_K_LARGE else ())
    for name, x in C.erode_inputs(shape):
        xd = _dev(torch, x)
        for k in ks:
            assert _same(ops.erode(xd, k).cpu().numpy(), P.erode(x, k)), (name, k)


# ---- gaussian_blur -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ksize,sigma', C.GAUSS_KSIZES)
def test_gaussian_blur_whole_frame(env, ksize, sigma):
    torch, ops, P = env
    from codeformer_amd.facelib.paste import gaussian_taps
    taps = gaussian_taps(ksize, sigma)
    assert _same(taps, P.gaussian_kernel(ksize, sigma))
    ran = 0
    for frame in C.GAUSS_FRAMES:
        if not C.gauss_allowed(ksize, frame):
            continue
        x = np.random.default_rng(50 + frame[0]).random(frame).astype(np.float32)
        assert _same(ops.gaussian_blur(_dev(torch, x), _dev(torch, taps)).cpu().numpy(), P.gaussian_blur(x, ksize, sigma)), frame
        ran += 1
    assert ran >= 2


@pytest.mark.parametrize('ksize,sigma', C.GAUSS_KSIZES)
def test_gaussian_blur_window_of_a_frame(env, ksize, sigma):
    """A region of a frame whose outside is exactly zero equals the same window of the full-frame blur."""
    torch, ops, P = env
    from codeformer_amd.facelib.paste import gaussian_taps
    assert C.gauss_allowed(ksize, C.GAUSS_WINDOW_FRAME)
    td = _dev(torch, gaussian_taps(ksize, sigma))
    rng = np.random.default_rng(60)
    for x, y, w, h in C.gauss_windows():
        full = np.zeros(C.GAUSS_WINDOW_FRAME, np.float32)
        full[y:y + h, x:x + w] = rng.random((h, w)).astype(np.float32)
        got = ops.gaussian_blur(_dev(torch, full[y:y + h, x:x + w]), td, (x, y), C.GAUSS_WINDOW_FRAME).cpu().numpy()
        assert _same(got, P.gaussian_blur(full, ksize, sigma)[y:y + h, x:x + w]), (x, y, w, h)


# ---- resizes -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', C.RESIZE_SOURCES)
def test_resize_linear_u8(env, shape):
    torch, ops, P = env
    src = C.resize_source_u8(shape)
    sd = _dev(torch, src)
    for dh, dw in C.resize_targets(*shape):
        got = ops.resize_linear_u8(sd, dh, dw).cpu().numpy()
        assert _same(got, P.resize_linear_u8(src, (dw, dh)).astype(np.float32)), (dh, dw)
    assert _same(ops.resize_linear_u8(sd, *shape).cpu().numpy(), src.astype(np.float32))       # identity: the plain cast


def test_resize_linear_f32_one_pixel_axes(env):
    torch, ops, P = env
    for sh, sw in ((1, 9), (9, 1), (1, 1), (2, 2)):
        x = C.mixed_f32((2, sh, sw), 70 + sh)
        xd = _dev(torch, x)
        for dh, dw in ((2 * sh, 2 * sw), (3 * sh, 3 * sw), (5, 7), (1, 1), (sh, sw), (max(1, sh // 2), max(1, sw // 2)), (1, 4), (4, 1)):
            got = ops.resize_linear_f32(xd, dh, dw).cpu().numpy()
            for i in range(2):
                assert _same(got[i], C.resize_linear_f32(x[i], (dw, dh))), (sh, sw, dh, dw, i)


# ---- small kernels -----------------------------------------------------------------------------------------------------------------------
def test_f32_to_u8_trunc(env):
    torch, ops, P = env
    v = C.trunc_values()
    assert np.array_equal(ops.f32_to_u8_trunc(_dev(torch, v)).cpu().numpy(), C.trunc_ref(v))
    for n in (1, 255, 256, 257):
        for part in (v[:n], v[256:256 + n], v[-n:]):
            assert np.array_equal(ops.f32_to_u8_trunc(_dev(torch, part)).cpu().numpy(), C.trunc_ref(part)), n
    plane = v[:768].reshape(16, 16, 3)                       # the shape of the input is the shape of the result
    assert np.array_equal(ops.f32_to_u8_trunc(_dev(torch, plane)).cpu().numpy(), C.trunc_ref(plane))


@pytest.mark.parametrize('nlut', [19, 32])
def test_label_lut(env, nlut):
    torch, ops, P = env
    lut, labels = C.lut_table(nlut), C.lut_labels(nlut)
    want = C.label_lut_ref(labels, lut)
    assert _same(ops.label_lut(_dev(torch, labels), lut).cpu().numpy(), want)
    outside = (labels < 0) | (labels >= nlut)
    assert outside.sum() >= 5 and not want[outside].any() and want[~outside].all()
    big = np.resize(labels, (3, 11, 17))                     # more than one block
    assert _same(ops.label_lut(_dev(torch, big), lut).cpu().numpy(), C.label_lut_ref(big, lut))
    with pytest.raises(RuntimeError):
        ops.label_lut(_dev(torch, labels), [1.0] * 33)


@pytest.mark.parametrize('border', [0, 1, 2, 3])
def test_scale_clear_border(env, border):
    torch, ops, P = env
    x = C.mixed_f32((2, 5, 7), 80)
    x[0, 0, 0], x[0, 4, 6], x[1, 0, 3], x[1, 2, 0] = np.inf, np.nan, -np.inf, np.nan       # on the outermost ring
    for scale in (1.0 / 255.0, 1.0, -3.5):
        got = ops.scale_clear_border_(_dev(torch, x), border, scale).cpu().numpy()
        if border == 0:                                      # nothing is cleared: inf and NaN pass through the product
            assert np.array_equal(got, x * np.float32(scale), equal_nan=True) and np.isnan(got).sum() == 2
        else:
            assert _same(got, C.scale_clear_border_ref(x, border, scale)), scale
            assert np.isfinite(got).all() and bool(got.any()) == (border < 3)


@pytest.mark.parametrize('n', C.SUM_LENGTHS)
def test_sum_partials(env, n):
    torch, ops, P = env
    rng = np.random.default_rng(90 + n)
    part = torch.empty(64, dtype=torch.float64, device='cuda')

    def partials(x):
        part.fill_(float('nan'))
        ops.sum_partials(_dev(torch, x), part)
        return part.cpu().numpy()

    chunks = C.sum_chunks(n)
    ints = rng.integers(-1000, 1001, n).astype(np.float32)
    got = partials(ints)
    assert got.tolist() == [float(ints[lo:hi].astype(np.int64).sum()) for lo, hi in chunks]     # integer data sums exactly, chunk by chunk
    for lo, hi in (chunks[0], chunks[1], chunks[-1]):        # the first and the last element of a chunk are seen
        for i in ({lo, hi - 1} if hi > lo else ()):
            moved = ints.copy()
            moved[i] += 1
            assert float(partials(moved).sum()) == float(ints.astype(np.int64).sum()) + 1, i
    x = C.mixed_f32((n,), 91 + n)
    bound = n * 2.0 ** -53 * math.fsum(np.abs(x).tolist())
    assert abs(float(partials(x).sum()) - math.fsum(x.tolist())) <= bound


# ---- the pipeline over geometry ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def scene():
    rng = np.random.default_rng(100)
    frame = rng.integers(0, 256, C.FRAME_HW + (3,), dtype=np.uint8)
    faces = rng.integers(0, 256, (3, C.FACE, C.FACE, 3), dtype=np.uint8)
    return frame, faces


def _paste(torch, u, frame, faces, affs):
    from codeformer_amd.facelib.paste import DeviceFaceHelper
    h = DeviceFaceHelper(face_size=C.FACE, upscale_factor=u, device='cuda')
    h.read_image(frame)
    crops = h.align_warp_face(affs).cpu().numpy()
    h.add_restored_faces(_dev(torch, np.stack(faces)))
    return crops, h.paste_faces_to_input_image()


@pytest.mark.parametrize('u', C.UPSCALES)
def test_pipeline_over_the_geometry_product(env, scene, u):
    torch, ops, P = env
    from codeformer_amd.facelib.paste import DeviceFaceHelper
    frame, faces = scene
    fs = (C.FACE, C.FACE)
    h_up, w_up = C.FRAME_HW[0] * u, C.FRAME_HW[1] * u
    background = P.resize_linear_u8(frame, (w_up, h_up)) if u > 1 else frame
    cases = C.pipeline_cases(u)
    assert len(cases) >= 64
    empty = 0
    for k, (_, size, angle, (cx, cy)) in enumerate(cases):
        aff = C.face_affine(cx, cy, size, angle)
        face = faces[k % 3]
        crops, got = _paste(torch, u, frame, [face], [aff])
        assert np.array_equal(crops[0], P.align_warp_face(frame, aff, face_size=fs)), (size, angle, cx, cy)
        want = P.paste_faces(frame, [face], [aff], upscale=u, face_size=fs)
        assert got.shape == (h_up, w_up, 3) and np.array_equal(got, want), (size, angle, cx, cy, int((got != want).sum()))
        if DeviceFaceHelper._region(C.paste_matrix(aff, u), h_up, w_up, fs) is None:
            empty += 1
            assert np.array_equal(got, background), (size, angle, cx, cy)
    assert empty >= 1


@pytest.mark.parametrize('u', C.UPSCALES)
def test_overlapping_faces_in_two_orders(env, scene, u):
    torch, ops, P = env
    frame, faces = scene
    fs = (C.FACE, C.FACE)
    affs = C.overlap_affines()
    results = []
    for order in ((0, 1, 2), (2, 1, 0)):
        f, a = [faces[i] for i in order], [affs[i] for i in order]
        _, got = _paste(torch, u, frame, f, a)
        assert np.array_equal(got, P.paste_faces(frame, f, a, upscale=u, face_size=fs)), order
        results.append(got)
    assert not np.array_equal(results[0], results[1])
