"""-m gpu: the RetinaFace ResNet-50 detector's HIP backend (csrc/cf_retina.hip, the odd-size stride-2 3x3 convolution, RetinaFace(backend='hip')).

Kernels are checked per element: cf_pointwise and the stride-2 3x3 against float64 within the project's per-kernel 2e-5 + 1e-5 |ref|,
cf_nearest_add bitwise against the torch expression, cf_retina_decode's full mode within 1e-5 relative of the float64 formulas and its compact
rows against the full rows.  The network's gate is the one ArcFace, VGG and BiSeNet carry: e_dev = max|hip - f64| <= 8 e_ref, e_ref =
max|ref32 - f64|, with ref32 / f64 the reference module's own float32 / float64 forward (tests/golden/retinaface_hip_ref.npz).  Every measured
figure is printed before it is asserted.  All weights are seeded random ones: no released detector checkpoint was run.

Measured on an MI355X (profiles/NOTES.md, "RetinaFace on HIP"): network ratios 1.90 .. 2.98 over the nine outputs with every convolution one launch;
cf_pointwise |err| / bound at most 0.22 (K 2048), the odd-size stride-2 3x3 0.21 / 0.26; decode rows 7.7e-6 relative; end-to-end rows 3.2e-5 pixels
of 1e-3 at threshold 0.6634 (score gap 1.7e-2, smallest |IoU - nms| 1.1e-3, 100 e_ref 1.8e-4).
"""
import numpy as np
import pytest
import torch
from torch.nn import functional as F

import retinaface_hip_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    from codeformer_amd import build as cf_build
    cf_build.build()
    assert torch.cuda.is_available()
    from codeformer_amd import ops
    return ops


@pytest.fixture(scope='module')
def net(ops):
    from codeformer_amd.facelib.detection.retinaface.retinaface import RetinaFace
    return R.build(RetinaFace, device='cuda', backend='hip')


def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32) * scale


def _close(what, got, ref64):
    """per element: |got - ref| <= 2e-5 + 1e-5 |ref|"""
    got, ref64 = got.detach().cpu().double(), ref64.cpu().double()
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    worst = float(((got - ref64).abs() / (2e-5 + 1e-5 * ref64.abs())).max())
    print(f'{what}: worst |err| / (2e-5 + 1e-5 |ref|) = {worst:.4f}')
    assert worst <= 1.0, what


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---- cf_pointwise --------------------------------------------------------------------------------------------------------------------
def _pw_case(B, H, W, cin, cout, seed, step=1):
    x = _randn((B, H, W, cin), seed)
    w = _randn((cout, cin), seed + 1, cin ** -0.5)
    b = _randn((cout,), seed + 2)
    Ho, Wo = (H + step - 1) // step, (W + step - 1) // step
    res = _randn((B, Ho, Wo, cout), seed + 3)
    ref = torch.einsum('bhwk,nk->bhwn', x[:, ::step, ::step].double(), w.double()) + b.double()
    return x, w, b, res, ref


@pytest.mark.parametrize('with_res', [False, True])
@pytest.mark.parametrize('relu', [False, True])
def test_pointwise_64_to_256(ops, with_res, relu):
    x, w, b, res, ref = _pw_case(2, 38, 53, 64, 256, 100)
    if with_res:
        ref = ref + res.double()
    if relu:
        ref = ref.clamp(min=0)
    pp = ops.pack_pointwise(w.cuda(), b.cuda())
    xd, rd = x.cuda(), res.cuda() if with_res else None
    y = ops.pointwise(xd, pp, res=rd, relu=relu)
    _close(f'pointwise 2x38x53 64->256 res={with_res} relu={relu}', y, ref)
    assert torch.equal(_bits(y), _bits(ops.pointwise(xd, pp, res=rd, relu=relu))), 'a repeat is not bitwise'
    alone = ops.pointwise(xd[1:2].contiguous(), pp, res=None if rd is None else rd[1:2].contiguous(), relu=relu)
    assert torch.equal(_bits(alone), _bits(y[1:2])), 'image 1 alone differs from image 1 of the batch'


@pytest.mark.parametrize('shape', [(1, 19, 27, 1024, 256, 1), (1, 75, 105, 256, 512, 2), (1, 5, 7, 2048, 512, 1),
                                   (2, 9, 11, 40, 72, 1), (1, 13, 7, 100, 64, 2)])      # the last two: a K tail (cin % 32 != 0), cout off the 64-column tile
def test_pointwise_shapes(ops, shape):
    B, H, W, cin, cout, step = shape
    x, w, b, _, ref = _pw_case(B, H, W, cin, cout, 200 + cin, step)
    y = ops.pointwise(x.cuda(), ops.pack_pointwise(w.cuda(), b.cuda()), step=step)
    assert tuple(y.shape) == (B, (H + step - 1) // step, (W + step - 1) // step, cout)
    _close(f'pointwise {shape}', y, ref)


def test_pointwise_channel_slices(ops):
    """input, residual and output as channel slices of wider buffers; the floats around the output slice stay as they were"""
    x, w, b, res, ref = _pw_case(2, 9, 11, 64, 40, 300)
    xb, rb = _randn((2, 9, 11, 96), 310).cuda(), _randn((2, 9, 11, 48), 311).cuda()
    xb[..., 16:80] = x.cuda()
    rb[..., 4:44] = res.cuda()
    ob = torch.full((2, 9, 11, 64), 7.0, device='cuda')
    y = ops.pointwise(xb[..., 16:80], ops.pack_pointwise(w.cuda(), b.cuda()), res=rb[..., 4:44], relu=True, out=ob[..., 8:48])
    assert y.data_ptr() == ob[..., 8:48].data_ptr()
    _close('pointwise slices', ob[..., 8:48], (ref + res.double()).clamp(min=0))
    assert bool((ob[..., :8] == 7.0).all()) and bool((ob[..., 48:] == 7.0).all())
    dense = ops.pointwise(x.cuda(), ops.pack_pointwise(w.cuda(), b.cuda()), res=res.cuda(), relu=True)
    assert torch.equal(_bits(dense), _bits(ob[..., 8:48])), 'slices change the bits'


# ---- stride-2 3x3 at odd sizes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(128, 75, 105), (512, 19, 27)])
def test_conv3x3_stride2_odd_sizes(ops, shape):
    c, H, W = shape
    x = _randn((1, H, W, c), 400 + c)
    w = _randn((c, c, 3, 3), 401 + c, (9 * c) ** -0.5)
    b = _randn((c,), 402 + c)
    ref = F.relu(F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), b.double(), stride=2, padding=1)).permute(0, 2, 3, 1)
    y = ops.conv2d(x.cuda(), ops.pack_weight(w.cuda(), b.cuda()), stride=2, pad_lo=1, epilogue=ops.EPI_PRELU, sft_w=0.0)
    assert tuple(y.shape) == (1, (H + 1) // 2, (W + 1) // 2, c)       # every row / column, the ones that touch the padding included
    _close(f'conv3x3 s2 {shape}', y, ref)


def test_conv3x3_stride2_pad_lo0_keeps_even_sizes(ops):
    w = ops.pack_weight(_randn((128, 128, 3, 3), 450, 0.03).cuda(), None)
    with pytest.raises(RuntimeError, match='even input'):
        ops.conv2d(_randn((1, 7, 8, 128), 451).cuda(), w, stride=2)


# ---- cf_nearest_add ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sizes', [((5, 7), (10, 14)), ((10, 14), (19, 27)), ((3, 2), (7, 3))])
def test_nearest_add_bitwise(ops, sizes):
    (hb, wb), (ha, wa) = sizes
    a, b = _randn((2, ha, wa, 256), 500).cuda(), _randn((2, hb, wb, 256), 501).cuda()
    ref = a.permute(0, 3, 1, 2) + F.interpolate(b.permute(0, 3, 1, 2), size=[ha, wa], mode='nearest')
    assert torch.equal(_bits(ops.nearest_add(a, b)), _bits(ref.permute(0, 2, 3, 1)))


# ---- cf_retina_decode ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def decode_case(ops):
    from codeformer_amd.facelib.detection.retinaface.retinaface import generate_config
    from codeformer_amd.facelib.detection.retinaface.retinaface_hip import split_heads
    from codeformer_amd.facelib.detection.retinaface.retinaface_utils import PriorBox
    H, W, B = 150, 210, 2
    heads = [_randn((B, -(-H // s), -(-W // s), 32), 600 + s, 1.5) for s in (8, 16, 32)]
    priors = PriorBox(generate_config('resnet50'), image_size=(H, W)).forward()
    loc, cls, ldm = (t.double() for t in split_heads(heads))
    conf = torch.softmax(cls, dim=-1)
    return dict(H=H, W=W, B=B, heads=[h.cuda() for h in heads], priors=priors, loc=loc, conf=conf, ldm=ldm)


def _rel(what, got, ref64, tol=1e-5):
    """the compact rows' bound, in pixels: relative with a floor of one pixel, since x1 = cx - w / 2 can cancel to near 0"""
    got, ref64 = got.detach().cpu().double(), ref64.double()
    worst = float(((got - ref64).abs() / ref64.abs().clamp(min=1.0)).max())
    print(f'{what}: worst |err| / max(|ref|, 1) = {worst:.3e}')
    assert worst <= tol, what


def test_decode_full_mode(ops, decode_case):
    d = decode_case
    loc, conf, ldm = ops.retina_decode(d['heads'], full=True)
    n = d['priors'].shape[0]
    assert tuple(loc.shape) == (d['B'], n, 4) and tuple(conf.shape) == (d['B'], n, 2) and tuple(ldm.shape) == (d['B'], n, 10)
    for what, got, ref in (('loc', loc, d['loc']), ('conf', conf, d['conf']), ('ldm', ldm, d['ldm'])):
        err = (got.detach().cpu().double() - ref).abs()        # strictly relative, no floor: the smallest probability here is 7e-4
        worst = float((err / ref.abs()).max())
        print(f'decode full {what}: worst |err| / |ref| = {worst:.3e} (smallest |ref| {float(ref.abs().min()):.3e}, worst |err| {float(err.max()):.3e})')
        assert bool((err <= 1e-5 * ref.abs()).all()), what


def test_decode_takes_one_mode_per_call(ops, decode_case):
    d = decode_case
    with pytest.raises(ValueError, match='one mode'):
        ops.retina_decode(d['heads'], d['priors'].cuda(), conf_threshold=0.5, cap=8, full=True)
    with pytest.raises(ValueError, match='one mode'):
        ops.retina_decode(d['heads'])


@pytest.mark.parametrize('thr', [0.5, 0.9, -1.0])
def test_decode_compact_rows(ops, decode_case, thr):
    d = decode_case
    n = d['priors'].shape[0]
    _, conf, _ = ops.retina_decode(d['heads'], full=True)
    rows, counts = ops.retina_decode(d['heads'], d['priors'].cuda(), img_wh=(d['W'], d['H']), resize=1.25, conf_threshold=thr, cap=n)
    rows, counts, conf = rows.cpu(), counts.cpu(), conf.cpu()
    for b in range(d['B']):
        idx = torch.nonzero(conf[b, :, 1] > thr).reshape(-1)       # ascending anchors (a float32 comparison, as the kernel's)
        assert int(counts[b]) == idx.numel(), 'the count is not exact'
        if thr < 0:
            assert idx.numel() == n
        got = rows[b, :idx.numel()]
        assert torch.equal(_bits(got[:, 4]), _bits(conf[b, idx, 1])), 'scores / anchor order'
        boxes, pts = R.decode64(d['loc'][b].numpy(), d['ldm'][b].numpy(), d['priors'].numpy(), d['W'], d['H'], resize=1.25)
        _rel(f'compact boxes thr {thr} image {b}', got[:, :4], torch.from_numpy(boxes)[idx])
        _rel(f'compact landmarks thr {thr} image {b}', got[:, 5:], torch.from_numpy(pts)[idx])


def test_decode_cap_overflow_reports_the_true_count(ops, decode_case):
    d = decode_case
    _, conf, _ = ops.retina_decode(d['heads'], full=True)
    rows, counts = ops.retina_decode(d['heads'], d['priors'].cuda(), img_wh=(d['W'], d['H']), conf_threshold=0.5, cap=8)
    assert [int(c) for c in counts.cpu()] == [int((conf[b, :, 1] > 0.5).sum()) for b in range(d['B'])] and int(counts.min()) > 8
    full_rows, _ = ops.retina_decode(d['heads'], d['priors'].cuda(), img_wh=(d['W'], d['H']), conf_threshold=0.5, cap=d['priors'].shape[0])
    assert tuple(rows.shape) == (d['B'], 8, 15) and torch.equal(_bits(rows), _bits(full_rows[:, :8]))


# ---- the network ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def forwards(net):
    """Device forward of every case, computed once."""
    return {case: [t.cpu() for t in net(R.case_input(case).cuda())] for case in R.CASES}


@pytest.mark.parametrize('case', R.NET_CASES)
def test_network_against_the_reference(forwards, case):
    g = R.golden()
    for name, got in zip(R.OUTS, forwards[case]):
        f64, f32 = g[f'{case}_{name}64'], g[f'{case}_{name}32']
        assert got.dtype == torch.float32 and tuple(got.shape) == f64.shape
        e_dev = float(np.abs(got.numpy().astype(np.float64) - f64).max())
        e_ref = float(np.abs(f32.astype(np.float64) - f64).max())
        print(f'network {case} {name}: e_dev {e_dev:.3e}  e_ref {e_ref:.3e}  ratio {e_dev / e_ref:.2f}')
        assert e_dev <= 8 * e_ref, (case, name)


def test_network_image_alone_is_bitwise_the_batch(net, forwards):
    x = R.case_input('b2_150x210')[1:2].cuda()
    for got, ref in zip(net(x), forwards['b2_150x210']):
        assert torch.equal(_bits(got), _bits(ref[1:2]))


def test_torch_backend_agrees(net, forwards):
    net.backend = 'torch'
    try:
        with torch.no_grad():
            ref = net(R.case_input('b1_64x96').cuda())
    finally:
        net.backend = 'hip'
    for name, a, b in zip(R.OUTS, forwards['b1_64x96'], ref):
        assert float((a - b.cpu()).abs().max()) < 1e-3, name


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def _flow_reference():
    g, case = R.golden(), R.FLOW_CASE
    loc, conf, ldm, pri = (g[f'{case}_{k}'] for k in ('loc64', 'conf64', 'ldm64', 'priors'))
    e_ref = max(float(np.abs(g[f'{case}_{k}32'].astype(np.float64) - g[f'{case}_{k}64']).max()) for k in R.OUTS)
    thr, gap = R.pick_threshold(conf[:, :, 1])
    h, w = R.CASES[case]['shape'][1:3]
    flows = [R.flow64(loc[i], conf[i], ldm[i], pri, w, h, thr) for i in range(loc.shape[0])]
    margin = min(m for _, m in flows)
    print(f'flow {case}: threshold {thr:.6f}, gap {gap:.3e}, IoU margin {margin:.3e}, 100 e_ref {100 * e_ref:.3e}')
    assert thr == float(g['flow_thr']) and gap > 100 * e_ref and margin > 100 * e_ref
    for i, (rows, _) in enumerate(flows):
        assert rows.shape == g[f'flow_rows{i}'].shape and np.abs(rows - g[f'flow_rows{i}']).max() < 1e-9
    return thr, [rows for rows, _ in flows]


def _rows_close(what, got, ref):
    assert got.dtype == np.float32 and got.shape == ref.shape, (what, got.shape, ref.shape)
    err = float(np.abs(got.astype(np.float64) - ref).max()) if ref.size else 0.0
    print(f'{what}: {ref.shape[0]} rows, max |err| {err:.3e}')
    assert err <= 1e-3, what


def test_detect_faces_end_to_end(net):
    thr, ref = _flow_reference()
    frames = R.case_frames(R.FLOW_CASE)
    for i in range(frames.shape[0]):
        _rows_close(f'detect_faces image {i} (array)', net.detect_faces(frames[i], conf_threshold=thr, nms_threshold=R.NMS), ref[i])
    dev = torch.from_numpy(frames[0]).cuda()
    _rows_close('detect_faces image 0 (device tensor)', net.detect_faces(dev, conf_threshold=thr, nms_threshold=R.NMS), ref[0])


def test_batched_detect_faces_end_to_end(net):
    thr, ref = _flow_reference()
    frames = torch.from_numpy(R.case_frames(R.FLOW_CASE).astype(np.float32))
    boxes, lands = net.batched_detect_faces(frames, conf_threshold=thr, nms_threshold=R.NMS)
    for i in range(len(ref)):
        _rows_close(f'batched image {i}', np.concatenate((boxes[i], lands[i]), axis=1), ref[i])


def test_detect_with_a_small_cap_takes_the_full_tensor_path(net):
    thr, ref = _flow_reference()
    frames = torch.from_numpy(R.case_frames(R.FLOW_CASE).astype(np.float32))
    cap, net._hip.CAP = net._hip.CAP, 4
    try:
        boxes, lands = net.batched_detect_faces(frames, conf_threshold=thr, nms_threshold=R.NMS)
    finally:
        net._hip.CAP = cap
    for i in range(len(ref)):
        _rows_close(f'batched image {i}, cap 4', np.concatenate((boxes[i], lands[i]), axis=1), ref[i])
