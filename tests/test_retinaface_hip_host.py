"""The RetinaFace HIP backend's host half: the folded dataflow against the module in float64, the fixture, the backend switch and the bindings.
No GPU is needed: the entry points validate their arguments before anything is launched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import retinaface_hip_ref as R

HEADER = os.path.join(R.ROOT, 'include', 'codeformer_hip.h')
NEW_EXPORTS = {'cf_pointwise_packed_elems': 2, 'cf_pack_pointwise': 5, 'cf_pointwise': 16, 'cf_nearest_add': 10, 'cf_retina_decode': 21}


@pytest.fixture(scope='module')
def RetinaFace():
    from codeformer_amd.facelib.detection.retinaface.retinaface import RetinaFace
    return RetinaFace


@pytest.mark.parametrize('case', ['b1_64x96', 'b1_97x33'])
def test_folded_dataflow_equals_the_module_in_float64(RetinaFace, case):
    net = R.build(RetinaFace).double()
    x = R.case_input(case).double()
    g = R.golden()
    with torch.no_grad():
        plain, folded = net(x), net.forward_folded(x)
    for name, a, b in zip(R.OUTS, plain, folded):
        assert a.shape == b.shape and float((a - b).abs().max()) < 1e-10, name
        assert float(np.abs(a.numpy() - g[f'{case}_{name}64']).max()) < 1e-10, f'{name}: the module is not the recorded reference'


def test_fixture_reference_error_is_positive():
    g = R.golden()
    for case in R.CASES:
        for name in R.OUTS:
            f32, f64 = g[f'{case}_{name}32'], g[f'{case}_{name}64']
            assert f32.dtype == np.float32 and f64.dtype == np.float64 and f32.shape == f64.shape
            assert np.abs(f32.astype(np.float64) - f64).max() > 0, (case, name)
        n = sum(-(-R.CASES[case]['shape'][1] // s) * -(-R.CASES[case]['shape'][2] // s) * 2 for s in (8, 16, 32))
        assert g[f'{case}_priors'].shape == (n, 4) and g[f'{case}_loc64'].shape == (R.CASES[case]['shape'][0], n, 4)


def test_flow_case_margins_hold_on_the_cpu():
    """the end-to-end case: the score gap and every candidate pair's IoU distance from the NMS threshold exceed 100 e_ref"""
    g, case = R.golden(), R.FLOW_CASE
    e_ref = max(float(np.abs(g[f'{case}_{k}32'].astype(np.float64) - g[f'{case}_{k}64']).max()) for k in R.OUTS)
    thr, gap = R.pick_threshold(g[f'{case}_conf64'][:, :, 1])
    assert thr == float(g['flow_thr']) and R.SCORE_BAND[0] < thr < R.SCORE_BAND[1]
    assert gap > 100 * e_ref and float(g['flow_margin']) > 100 * e_ref
    assert all(g[f'flow_rows{i}'].shape[0] > 1 for i in range(R.CASES[case]['shape'][0]))


def test_default_backend_is_torch(RetinaFace, monkeypatch):
    monkeypatch.delenv('CODEFORMER_HIP_DETECTOR', raising=False)
    net = RetinaFace('resnet50')
    assert net.backend == 'torch'
    assert not any('hip' in k for k in net.state_dict())
    monkeypatch.setenv('CODEFORMER_HIP_DETECTOR', 'hip')
    assert RetinaFace('resnet50').backend == 'hip'
    assert RetinaFace('resnet50', backend='torch').backend == 'torch'
    with pytest.raises(ValueError):
        RetinaFace('resnet50', backend='miopen')


def test_hip_is_refused_where_it_cannot_run(RetinaFace, monkeypatch):
    monkeypatch.delenv('CODEFORMER_HIP_DETECTOR', raising=False)
    with pytest.raises(NotImplementedError, match='resnet50'):
        RetinaFace('mobile0.25', backend='hip')
    with pytest.raises(NotImplementedError, match='half'):
        RetinaFace('resnet50', half=True, backend='hip')
    net = RetinaFace('resnet50', backend='hip')       # on the CPU
    x = torch.zeros(1, 3, 32, 32)
    with pytest.raises(NotImplementedError, match='CUDA'):
        net(x)
    with pytest.raises(NotImplementedError, match='CUDA'):
        net.detect_faces(np.zeros((32, 32, 3), dtype=np.uint8))
    with pytest.raises(NotImplementedError, match='CUDA'):
        net.batched_detect_faces(torch.zeros(1, 32, 32, 3))
    net.train()
    with pytest.raises(NotImplementedError, match='eval'):
        net(x)


def test_conv_unit_folded_is_the_shared_routine(RetinaFace):
    from codeformer_amd.archs.folded import fold_conv_bn
    net = R.build(RetinaFace)
    for u in (net.fpn.output2, net.fpn.merge1, net.ssh2.conv7x7_3):
        for dt in (None, torch.float64):
            for a, b in zip(u.folded(dt), fold_conv_bn(u[0], u[1], dt)):
                assert a.dtype == (dt or torch.float32) and torch.equal(a, b)
        assert len(u.fold_deps()) == 5 and u.fold_deps()[0] is u[0].weight


def test_priors_cache_is_bounded(RetinaFace):
    net = RetinaFace('resnet50')
    hip = net._hip
    sizes = [(32 + 8 * i, 40) for i in range(hip.PRIOR_SIZES + 3)]
    first = hip.priors(*sizes[0], 'cpu')
    assert hip.priors(*sizes[0], 'cpu')[0] is first[0]                       # a hit returns the cached tensors
    assert first[1].tolist() == [40., 32.] * 2 and first[2].tolist() == [40., 32.] * 5 and first[0].shape == (2 * (5 * 4 + 3 * 2 + 2 * 1), 4)
    for hw in sizes[1:]:
        hip.priors(*hw, 'cpu')
        hip.priors(*sizes[1], 'cpu')                                         # kept alive by use
    assert len(hip._priors) == hip.PRIOR_SIZES
    keys = [k[:2] for k in hip._priors]
    assert sizes[0] not in keys and sizes[1] in keys and sizes[-1] in keys


def test_entry_points_take_the_backend(monkeypatch):
    import inspect
    from codeformer_amd.facelib.detection import init_detection_model
    from codeformer_amd.facelib.utils.face_restoration_helper import FaceRestoreHelper
    assert inspect.signature(init_detection_model).parameters['backend'].default is None
    assert inspect.signature(FaceRestoreHelper.__init__).parameters['det_backend'].default is None
    import inference_codeformer
    assert inference_codeformer.parse_args([]).det_backend is None
    assert inference_codeformer.parse_args(['--det_backend', 'hip']).det_backend == 'hip'


def test_new_exports_are_declared_and_bound():
    from codeformer_amd import lib
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    for name, nargs in NEW_EXPORTS.items():
        m = re.search(r'(?:int|int64_t)\s+' + name + r'\s*\(([^)]*)\)', src)
        assert m, f'{name} is not declared in include/codeformer_hip.h'
        assert len(m.group(1).split(',')) == nargs == len(lib.SIGNATURES[name][1]), name
    assert lib.ABI_VERSION == 22 and re.search(r'#define\s+CF_ABI_VERSION\s+22\b', src)


@pytest.fixture(scope='module')
def native():
    from codeformer_amd import build as cf_build
    from codeformer_amd import lib
    cf_build.build()
    return lib._open()


def test_entry_points_validate_before_any_launch(native):
    from codeformer_amd import lib
    assert native.cf_version() == 22
    assert native.cf_pointwise_packed_elems(100, 70) == 128 * 128 and native.cf_pointwise_packed_elems(0, 4) == -1
    p = ctypes.c_void_p(256)     # never dereferenced: every call below is refused by its checks
    assert native.cf_pointwise(p, 64, p, None, None, 0, 1, 4, 4, 64, 64, 3, 0, p, 64, None) != 0 and 'step' in lib.last_error()
    assert native.cf_pointwise(p, 62, p, None, None, 0, 1, 4, 4, 62, 64, 1, 0, p, 64, None) != 0
    assert native.cf_pointwise(p, 64, p, None, None, 0, 1, 4, 4, 64, 64, 1, 0, p, 32, None) != 0 and 'stride' in lib.last_error()
    assert native.cf_nearest_add(p, p, 1, 4, 4, 2, 2, 6, p, None) != 0
    assert native.cf_retina_decode(p, p, p, 4, 1, 1, p, 1, 0.1, 0.2, 8.0, 8.0, 1.0, 0.5, None, None, None, None, 0, None, None) != 0
    assert native.cf_retina_decode(p, p, p, 4, 1, 1, p, 1, 0.1, 0.2, 8.0, 8.0, 1.0, 0.5, None, None, None, p, 0, p, None) != 0 and 'cap' in lib.last_error()
    assert native.cf_retina_decode(p, p, p, 4, 1, 1, p, 1, 0.1, 0.2, 8.0, 8.0, 1.0, 0.5, p, p, p, p, 8, p, None) != 0 and 'one mode' in lib.last_error()


def _s2_desc(lib, hin, win, hout, wout, pad_lo):
    return lib.ConvDesc(c0=128, batch=1, hin=hin, win=win, hout=hout, wout=wout, cout=128, cout_pad=128, taps=9, stride=2, epilogue=lib.EPI_PRELU,
                        pad_lo=pad_lo)


def test_stride2_accepts_odd_sizes_with_pad_lo_1_only(native):
    from codeformer_amd import lib
    query = native.cf_conv2d_stats_parts      # (runs every check of cf_conv2d and launches nothing)
    assert query(ctypes.byref(_s2_desc(lib, 75, 105, 38, 53, 1))) > 0, lib.last_error()
    assert query(ctypes.byref(_s2_desc(lib, 76, 106, 38, 53, 1))) > 0, lib.last_error()
    assert query(ctypes.byref(_s2_desc(lib, 75, 105, 37, 52, 1))) < 0 and 'expected 38x53' in lib.last_error()
    assert query(ctypes.byref(_s2_desc(lib, 75, 105, 37, 52, 0))) < 0 and 'even input' in lib.last_error()
    assert query(ctypes.byref(_s2_desc(lib, 76, 106, 38, 53, 0))) > 0, lib.last_error()
