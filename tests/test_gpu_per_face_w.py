"""-m gpu: one fidelity weight per face, network level (CodeFormer.forward / restore_u8 / restore_sweep with a vector w, graph replay, the logit
guard's second pass).  The forward is bitwise batch-invariant and the SFT epilogues form image b's weight by the expression of the scalar
launch, so every row of a call with a vector w has a scalar one-face call it must equal BIT FOR BIT, and logits, lq_feat and the code indices --
which do not depend on w -- are those of the scalar batch.  Seed-0 weights and four seeded faces, as the parity tests build them; every
`precision`, eager and under graph replay."""
import math

import numpy as np
import pytest

from _tools import load_script

pytestmark = pytest.mark.gpu

ALL_POSITIVE = (0.2, 0.5, 0.7, 1.0)
MIXED = (0.0, 0.5, -1.0, 1.0)
WITH_NAN = (0.7, float('nan'), 0.2, 0.0)
SWEEP = (0.0, 0.3, 0.7, 1.0)


@pytest.fixture(scope='module')
def chk():
    import torch
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    from codeformer_amd import lib
    lib.load()
    return load_script('tools/gpu_check.py')


@pytest.fixture(scope='module')
def net(chk):
    n = chk.build_net().cuda()
    assert n.use_hip_graphs == 'auto' and n.graph_max_batch >= 4 and n.logit_guard == 'off'
    return n


@pytest.fixture(scope='module')
def faces():
    from oracle.synth import seeded_input
    return seeded_input(4).cuda()


@pytest.fixture(scope='module')
def scalar(net, faces):
    """scalar(precision, b, w) -> (out, logits, lq_feat, indices) of the eager one-face call net(faces[b:b+1], w=w, adain=True), each computed
    once; b = None: the four-face batch.  The reference of every test below; never modified."""
    import torch
    memo = {}

    def get(precision, b, w):
        key = (precision, b, 'nan' if w != w else float(w))
        if key not in memo:
            keep = (net.precision, net.use_hip_graphs)
            net.precision, net.use_hip_graphs = precision, False
            try:
                with torch.no_grad():
                    r = net(faces if b is None else faces[b:b + 1], w=w, adain=True)
                memo[key] = tuple(t.clone() for t in r) + (net.last_indices.clone(),)
            finally:
                net.precision, net.use_hip_graphs = keep
        return memo[key]
    return get


def _call(net, precision, graphs, fn):
    import torch
    keep = (net.precision, net.use_hip_graphs)
    net.precision, net.use_hip_graphs = precision, graphs
    try:
        with torch.no_grad():
            r = fn()
        torch.cuda.synchronize()
        return r
    finally:
        net.precision, net.use_hip_graphs = keep


@pytest.mark.parametrize('mode', ['eager', 'graph'])
@pytest.mark.parametrize('precision', ['f16x2', 'fp32', 'bf16', 'fp16'])
def test_rows_are_the_scalar_one_face_calls(net, faces, scalar, precision, mode):
    import torch
    graphs = 'auto' if mode == 'graph' else False
    _, logits4, lq4, idx4 = scalar(precision, None, 0.5)
    # the three patterns, each in another of the forms forward accepts: a tuple, a numpy array, a tensor on the device
    forms = ((ALL_POSITIVE, ALL_POSITIVE), (MIXED, np.array(MIXED)), (WITH_NAN, torch.tensor(WITH_NAN).cuda()))
    for ws, given in forms:
        for rep in range(2 if mode == 'graph' else 1):      # (capture, then replay)
            out, logits, lq = _call(net, precision, graphs, lambda: net(faces, w=given, adain=True))
            assert torch.equal(logits, logits4) and torch.equal(lq, lq4) and torch.equal(net.last_indices, idx4), (ws, rep)
            for b, w in enumerate(ws):
                assert torch.equal(out[b], scalar(precision, b, w)[0][0]), (precision, mode, ws, b, rep)
    assert not torch.equal(scalar(precision, 0, 0.7)[0], scalar(precision, 0, 0.0)[0])       # fused and un-fused rows differ
    # bytes in, bytes out
    u8 = torch.randint(0, 256, (4, 512, 512, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(5)).cuda()
    got = _call(net, precision, graphs, lambda: net.restore_u8(u8, w=MIXED, adain=True))
    for b, w in enumerate(MIXED):
        one = _call(net, precision, False, lambda: net.restore_u8(u8[b:b + 1], w=w, adain=True))
        assert torch.equal(got[b], one[0]), (precision, mode, 'restore_u8', b)
    dst = torch.zeros(4, 512, 512, 3, dtype=torch.uint8, device='cuda')
    assert _call(net, precision, graphs, lambda: net.restore_u8(u8, w=list(MIXED), adain=True, out=dst)).data_ptr() == dst.data_ptr()
    assert torch.equal(dst, got)


@pytest.mark.parametrize('precision', ['f16x2', 'fp32', 'bf16', 'fp16'])
def test_restore_sweep_is_the_scalar_calls_with_one_encoder_pass(net, faces, scalar, precision, monkeypatch):
    import torch
    from codeformer_amd import ops
    x = faces[:2]
    real = ops.conv2d
    log = []

    def counted(x_, pw, **kw):
        log.append((bool(kw.get('in_nchw')), (kw['img_in'] if x_ is None else x_).shape[0]))
        return real(x_, pw, **kw)

    def launches(fn):
        log.clear()
        monkeypatch.setattr(ops, 'conv2d', counted)
        try:
            r = _call(net, precision, False, fn)
        finally:
            monkeypatch.setattr(ops, 'conv2d', real)
        return r, list(log)

    (outs, logits, lq), sweep = launches(lambda: net.restore_sweep(x, SWEEP, adain=True))
    idx = net.last_indices.clone()                      # (the scalar calls below leave their own)
    assert outs.shape == (4, 2, 3, 512, 512)
    for k, w in enumerate(SWEEP):
        for b in range(2):
            assert torch.equal(outs[k, b], scalar(precision, b, w)[0][0]), (precision, k, b)
    for b in range(2):
        assert torch.equal(logits[b], scalar(precision, b, 0.3)[1][0]) and torch.equal(lq[b], scalar(precision, b, 0.3)[2][0])
        assert torch.equal(idx[b], scalar(precision, b, 0.3)[3][0])
    # the encoder's launches are issued once, for the two faces: the image is read by one launch, and the sweep's convolution launches are
    # those of one code_only pass + one fused generator pass (six rows) + one un-fused generator pass (two rows)
    assert [n for first, n in sweep if first] == [2]
    _, enc = launches(lambda: net(x, w=0.5, adain=True, code_only=True))
    _, fused = launches(lambda: net(x, w=0.5, adain=True))
    _, unfused = launches(lambda: net(x, w=0.0, adain=True))
    assert len(sweep) == len(enc) + (len(fused) - len(enc)) + (len(unfused) - len(enc))
    assert sorted({n for _, n in sweep}) == [2, 6]
    # a sweep whose weights are all positive / all non-positive runs one generator pass
    (o1, _, _), only = launches(lambda: net.restore_sweep(x, (1.0, 0.3), adain=True))
    assert len(only) == len(fused) and torch.equal(o1[1], outs[1]) and torch.equal(o1[0], outs[3])
    (o2, _, _), none = launches(lambda: net.restore_sweep(x, (-2.0, float('nan')), adain=True))
    assert len(none) == len(unfused) and torch.equal(o2[0], outs[0]) and torch.equal(o2[1], outs[0])


def test_vectors_share_one_graph_and_scalars_keep_theirs(net, faces):
    import torch
    assert net.precision == 'f16x2' and net.use_hip_graphs == 'auto'
    x = faces[:2]
    net._graphs.clear()
    before = net.graph_captures
    outs = [_call(net, 'f16x2', 'auto', lambda: net(x, w=ws, adain=True))[0] for ws in ((0.2, 0.9), (0.5, 0.4), (1.0, 0.05))]
    assert net.graph_captures == before + 1 and len(net._graphs) == 1         # the key holds the pattern, not the values
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2])
    _call(net, 'f16x2', 'auto', lambda: net(x, w=(0.3, 0.0), adain=True))
    assert net.graph_captures == before + 2                                   # another pattern: another graph
    _call(net, 'f16x2', 'auto', lambda: net(x, w=(0.0, -1.0), adain=True))
    _call(net, 'f16x2', 'auto', lambda: net(x, w=0.0, adain=True))
    assert net.graph_captures == before + 3                                   # no face fused: the scalar call's un-fused graph, once
    before = net.graph_captures
    for w in (0.25, 0.5, 0.75):
        _call(net, 'f16x2', 'auto', lambda: net(faces[:1], w=w, adain=True))
    assert net.graph_captures == before + 3                                   # a scalar w is part of the key, as ever
    _call(net, 'f16x2', 'auto', lambda: net(faces[:1], w=0.5, adain=True))
    assert net.graph_captures == before + 3
    net._graphs.clear()


def test_logit_guard_rerun_keeps_every_face_its_own_weight(chk, faces):
    """The crafted tie of tests/test_gpu_logit_guard.py (two identical, dominant rows of the logits head: every face is flagged) with a vector
    w: 'rerun' reproduces, per face, the scalar call of the F(2x2,3x3)-encoder network with that face's weight -- forward and restore_sweep."""
    import torch

    def tied(f43):
        n = chk.build_net()
        with torch.no_grad():
            W = n.idx_pred_layer[1].weight
            W[700] = W[3]
            W[3] *= 1024.0
            W[700] *= 1024.0
        n = n.cuda()
        n.winograd_f43_encoder = f43
        return n
    net, f23 = tied(True), tied(False)
    ws = (0.2, 0.0, 1.0, 0.6)
    f23.use_hip_graphs = False
    with torch.no_grad():
        ref = [tuple(t.clone() for t in f23(faces[b:b + 1], w=w, adain=True)) + (f23.last_indices.clone(),) for b, w in enumerate(ws)]
    net.logit_guard = 'rerun'
    for graphs in (False, 'auto'):
        net.reset_guard_stats()
        out, logits, lq = _call(net, 'f16x2', graphs, lambda: net(faces, w=ws, adain=True))
        st = net.guard_stats
        assert (st['flagged'], st['rerun_faces'], st['min_gap']) == (4, 4, 0.0)
        for b in range(4):
            assert torch.equal(out[b], ref[b][0][0]) and torch.equal(logits[b], ref[b][1][0]) and torch.equal(lq[b], ref[b][2][0]), (graphs, b)
            assert torch.equal(net.last_indices[b], ref[b][3][0])
    net.reset_guard_stats()
    outs, logits, lq = _call(net, 'f16x2', False, lambda: net.restore_sweep(faces[:1], (0.0, 0.2), adain=True))
    assert net.guard_stats['rerun_faces'] == 1
    with torch.no_grad():
        want0 = f23(faces[:1], w=0.0, adain=True)[0]
    assert torch.equal(outs[1, 0], ref[0][0][0]) and torch.equal(outs[0, 0], want0[0]) and torch.equal(logits[0], ref[0][1][0])
    assert math.isfinite(float(outs.abs().max()))


def test_pipeline_takes_one_weight_per_path(net, tmp_path):
    """AlignedFacePipeline.restore(paths, out_paths, w=<one weight per path>) with batches of two over three PNGs: every written face is the
    bytes of restore_u8 on that face alone with its own weight (PNG is lossless), and a wrong count is refused."""
    import torch
    from codeformer_amd.pipeline import AlignedFacePipeline
    from codeformer_amd.utils.img_util import imread_bgr, imwrite
    rng = np.random.default_rng(9)
    faces = [rng.integers(0, 256, size=(512, 512, 3), dtype=np.uint8) for _ in range(3)]
    paths, outs = [str(tmp_path / f'in{i}.png') for i in range(3)], [str(tmp_path / f'out{i}.png') for i in range(3)]
    for f, p in zip(faces, paths):
        imwrite(f, p)
    ws = (0.7, 0.0, 0.3)
    pipe = AlignedFacePipeline(net, torch.device('cuda'), batch_size=2, workers=2, slots=2)
    st = pipe.restore(paths, outs, w=np.array(ws), adain=True, strict=True)
    assert st['faces'] == 3 and st['batches'] == 2 and st['failures'] == 0
    for f, o, w in zip(faces, outs, ws):
        want = _call(net, 'f16x2', False, lambda: net.restore_u8(torch.from_numpy(f).unsqueeze(0).cuda(), w=w, adain=True))[0].cpu().numpy()
        assert np.array_equal(imread_bgr(o), want), w
    with pytest.raises(ValueError, match='3 paths'):
        pipe.restore(paths, outs, w=[0.5, 0.5], strict=True)


def test_restore_sweep_with_some_faces_rerun(chk, net, faces):
    """restore_sweep under logit_guard='rerun' when only SOME faces are flagged (the two-group case): face 1 is the reference's crop 0342,
    whose smallest top-2 gap lies under the default threshold (tests/test_gpu_logit_guard.py), faces 0 and 2 are seeded ones, which are not
    flagged.  The kept faces -- selected with their encoder taps -- are bitwise the guard-off network's scalar calls, the flagged one the
    F(2x2,3x3)-encoder network's."""
    import os
    import torch
    from codeformer_amd import ops
    img = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'real_0342.npz'))['img']
    x = faces[:3].clone()
    x[1] = ops.img_u8_to_tensor(torch.from_numpy(img).unsqueeze(0).cuda())[0]
    f23 = chk.build_net().cuda()
    f23.winograd_f43_encoder, f23.use_hip_graphs = False, False
    ws = (0.0, 0.6)
    net.logit_guard = 'rerun'
    try:
        net.reset_guard_stats()
        outs, logits, lq = _call(net, 'f16x2', False, lambda: net.restore_sweep(x, ws, adain=True))
        idx, st = net.last_indices.clone(), net.guard_stats
    finally:
        net.logit_guard = 'off'
        net.reset_guard_stats()
    assert (st['faces'], st['flagged'], st['rerun_faces']) == (3, 1, 1)
    for b in range(3):
        ref_net = f23 if b == 1 else net
        for k, w in enumerate(ws):
            want = _call(ref_net, 'f16x2', False, lambda: ref_net(x[b:b + 1], w=w, adain=True))
            assert torch.equal(outs[k, b], want[0][0]), (b, k)
            assert torch.equal(logits[b], want[1][0]) and torch.equal(lq[b], want[2][0]) and torch.equal(idx[b], ref_net.last_indices[0]), b
