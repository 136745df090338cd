"""CPU side of --face_upsample / --draw_box: the numpy restatement in tests/test_gpu_face_upsample.py agrees with itself and with the
oracle primitives, the CLI refuses scales the x2 face upsampler cannot paste at before it touches a device, and the new kernels are
declared in the header and bound in lib.SIGNATURES."""
import os
import re

import numpy as np
import pytest
import torch

import test_gpu_face_upsample as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('cf_box_overlay_u8', 'cf_resize_linear_f32', 'cf_esrgan_tile_gather_u8', 'cf_esrgan_tile_scatter_u8')


def test_border_band_rule():
    m = G.band_mask(12, 3)
    assert m.dtype == np.float32 and m[3:9, 3:9].sum() == 0 and m.sum() == 144 - 36
    assert not G.band_mask(12, 0).any()                      # border 0: no box
    assert G.band_mask(12, 6).all() and G.band_mask(12, 20).all()  # an empty interior slice leaves all ones
    from codeformer_amd.facelib.paste import box_border
    for area in (1.0, 400.0, 16900.0, 67600.0, 1960000.0, 1960001.0, 4e6):
        assert box_border(area) == int(1400 / np.sqrt(np.float32(area))), area
    assert box_border(4e6) == 0 and box_border(16900.0) == 10


def test_two_to_one_reduction_is_inter_linear():
    from oracle import paste_oracle as P
    img = np.random.default_rng(1).integers(0, 256, (64, 90, 3), dtype=np.uint8)
    assert np.array_equal(G.reduce_2to1_u8(img), P.resize_linear_u8(img, (45, 32)))
    img[:] = 255
    assert (G.reduce_2to1_u8(img) == 255).all()


def test_float_resize_restatement():
    import torch.nn.functional as F
    x = np.random.default_rng(2).random((40, 52)).astype(np.float32)
    up = G.resize_linear_f32(x, (104, 80))
    assert up.dtype == np.float32 and up.shape == (80, 104)
    ref = F.interpolate(torch.from_numpy(x).double()[None, None], size=(80, 104), mode='bilinear', align_corners=False)[0, 0].numpy()
    assert np.abs(up - ref).max() <= 1e-6
    assert np.array_equal(G.resize_linear_f32(x, (52, 40)), x)  # identity
    assert np.array_equal(up[0, 0], x[0, 0]) and np.array_equal(up[-1, -1], x[-1, -1])


def test_paste_oracle_without_the_new_flags_is_the_existing_one():
    from oracle import paste_oracle as P
    frame = G._img(120, 160, 3)
    affs = [G._affine(60, 50, 70, 0.2), G._affine(110, 70, 60, -0.1)]
    faces = [G._img(512, 512, 4 + i) for i in range(2)]
    for u in (1, 2):
        assert np.array_equal(G.paste_oracle(frame, faces, affs, u), P.paste_faces(frame, faces, affs, upscale=u))


def test_cli_rejects_face_upsample_at_other_scales_without_a_device(monkeypatch):
    import inference_codeformer as ic
    touched = []
    monkeypatch.setattr(ic, 'get_device', lambda *a, **k: touched.append(1))
    with pytest.raises(NotImplementedError, match='LANCZOS4'):
        ic.main(['-i', 'nowhere', '--face_upsample', '-s', '4'])
    with pytest.raises(NotImplementedError, match='LANCZOS4'):
        ic.main(['-i', 'nowhere', '--face_upsample', '-s', '1', '--device', 'cuda'])
    assert not touched
    ic.check_args(ic.parse_args(['--face_upsample', '-s', '2']))
    ic.check_args(ic.parse_args(['--draw_box', '-s', '4']))


def test_new_symbols_are_declared_and_bound():
    from codeformer_amd import lib
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'codeformer_hip.h')).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(rf'\b{name}\s*\(', src), name
        assert name in lib.SIGNATURES, name
    assert lib.ABI_VERSION == 22


def test_enhance_faces_refuses_other_output_scales():
    from codeformer_amd.utils.realesrgan_utils import RealESRGANer
    up = RealESRGANer(scale=2, model_path=None, model=G._net(), tile=0, device='cpu')
    with pytest.raises(NotImplementedError, match='LANCZOS4'):
        up.enhance_faces(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), outscale=4)
    with pytest.raises(ValueError):
        up.enhance_faces(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))       # device tensors only
