"""The uint8 image boundary (cf_conv2d_u8, ops.conv2d(img_in= / img_out=), CodeFormer.restore_u8), the parts that need no GPU: the C ABI
declaration and binding, the argument checks of cf_conv2d_u8 (they run before any launch), the refusals of restore_u8 and of the operator
layer, and the host path of restore_u8 against the converters of utils/img_util.py composed by hand."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'codeformer_hip.h')
FAKE = 0x1000   # a non-NULL "device pointer": every call below is refused before anything is launched


def test_symbol_is_declared_and_bound():
    from codeformer_amd import lib
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    m = re.search(r'int\s+cf_conv2d_u8\s*\(([^)]*)\)', src)
    assert m, 'cf_conv2d_u8 is not declared in include/codeformer_hip.h'
    params = [p.strip() for p in m.group(1).split(',')]
    assert len(params) == 4 and 'cf_conv_desc' in params[0] and 'const uint8_t' in params[1] and 'img_in' in params[1]
    assert 'uint8_t' in params[2] and 'const' not in params[2] and 'img_out' in params[2] and 'cf_stream_t' in params[3]
    res, args = lib.SIGNATURES['cf_conv2d_u8']
    assert res is ctypes.c_int and len(args) == 4 and lib.ABI_VERSION == 22


@pytest.fixture(scope='module')
def native():
    from codeformer_amd import build as cf_build
    from codeformer_amd import lib
    cf_build.build()
    n = lib.load()
    assert n.cf_version() == 22           # additive: the struct layout and the version stay
    return n


def _first(**kw):
    """The descriptor of the network's first conv (3 -> 64, NCHW in) at 32x32; in0 is left NULL: the image stands for it."""
    from codeformer_amd import lib
    d = dict(c0=3, c1=0, batch=1, hin=32, win=32, hout=32, wout=32, cout=64, cout_pad=64, taps=9, stride=1, in_nchw=1, out_nchw=0,
             weight=FAKE, bias=FAKE, out=FAKE, acc_scale=1.0)
    d.update(kw)
    return lib.ConvDesc(**d)


def _last(**kw):
    """The descriptor of the network's last conv (64 -> 3, NCHW out) at 24x40; out is left NULL."""
    from codeformer_amd import lib
    d = dict(in0=FAKE, c0=64, c1=0, batch=1, hin=24, win=40, hout=24, wout=40, cout=3, cout_pad=32, taps=9, stride=1, in_nchw=0, out_nchw=1,
             weight=FAKE, bias=FAKE, acc_scale=1.0)
    d.update(kw)
    return lib.ConvDesc(**d)


REFUSED = [
    ('both NULL', lambda: _first(), None, None, 'both NULL'),
    ('both set', lambda: _first(), FAKE, FAKE, 'both set'),
    ('img_in, in_nchw 0', lambda: _first(in_nchw=0), FAKE, None, 'in_nchw'),
    ('img_in, c0 4', lambda: _first(c0=4), FAKE, None, 'c0 = 3'),
    ('img_in, hout 24', lambda: _first(hin=24, hout=24), FAKE, None, 'multiples of 16'),
    ('img_out, out_nchw 0', lambda: _last(out_nchw=0), None, FAKE, 'out_nchw'),
    ('img_out, cout 4', lambda: _last(cout=4), None, FAKE, 'cout = 3'),
    ('img_out, epilogue', lambda: _last(epilogue=1, res=FAKE), None, FAKE, 'epilogue'),
    # refused by the checks cf_conv2d_u8 shares with cf_conv2d: the text still names the export that was called
    ('img_in, hout != hin', lambda: _first(hout=48), FAKE, None, 'hout/wout'),
    ('img_out, c0 24', lambda: _last(c0=24), None, FAKE, 'multiples of 16'),
]


@pytest.mark.parametrize('case', REFUSED, ids=[c[0] for c in REFUSED])
def test_entry_point_validates_before_any_launch(native, case):
    from codeformer_amd import lib
    _, desc, img_in, img_out, word = case
    assert native.cf_conv2d_u8(ctypes.byref(desc()), img_in, img_out, None) == -1
    err = lib.last_error()
    assert err.startswith('cf_conv2d_u8:') and word in err, err


def test_null_descriptor(native):
    assert native.cf_conv2d_u8(None, FAKE, None, None) == -1


@pytest.fixture(scope='module')
def small_net():
    import codeformer_amd.archs  # noqa: F401
    from codeformer_amd.utils.registry import ARCH_REGISTRY
    torch.manual_seed(0)
    return ARCH_REGISTRY.get('CodeFormer')(dim_embd=64, codebook_size=32, n_head=2, n_layers=1, connect_list=['32']).eval()


def test_restore_u8_refuses_what_is_not_a_byte_face_batch(small_net):
    with pytest.raises(ValueError):
        small_net.restore_u8(torch.zeros(1, 512, 512, 3))                                  # float
    with pytest.raises(ValueError):
        small_net.restore_u8(torch.zeros(1, 3, 512, 512, dtype=torch.uint8))               # NCHW
    with pytest.raises(ValueError):
        small_net.restore_u8(torch.zeros(1, 512, 512, 6, dtype=torch.uint8)[..., ::2])     # the right shape, not contiguous
    good = torch.zeros(1, 512, 512, 3, dtype=torch.uint8)
    with pytest.raises(ValueError):
        small_net.restore_u8(good, out=torch.zeros(1, 512, 512, 3))                        # float destination
    with pytest.raises(ValueError):
        small_net.restore_u8(good, out=torch.zeros(2, 512, 512, 3, dtype=torch.uint8))     # another batch size
    small_net.logit_guard = 'maybe'
    try:
        with pytest.raises(ValueError):
            small_net.restore_u8(good)
    finally:
        small_net.logit_guard = 'off'


def test_ops_refuse_cpu_tensors(native):
    from codeformer_amd import ops
    conv = torch.nn.Conv2d(3, 64, 3, padding=1)
    with pytest.raises(ValueError):
        ops.conv2d(None, ops.PackedWeight(conv.weight.detach(), conv.bias.detach(), 64, 3, 9, 64, 16), in_nchw=True,
                   img_in=torch.zeros(1, 16, 16, 3, dtype=torch.uint8))
    with pytest.raises(ValueError):
        ops.conv2d(torch.zeros(1, 16, 16, 64), ops.PackedWeight(torch.zeros(1), None, 3, 64, 9, 32, 64), out_nchw=True,
                   img_out=torch.zeros(1, 16, 16, 3, dtype=torch.uint8))


def test_host_path_equals_the_converters_composed_by_hand(small_net):
    """One CPU face: restore_u8 == tensor2img(net(normalize(img2tensor(face / 255.)))[0], min_max=(-1, 1)), `out=` included."""
    from codeformer_amd.utils.img_util import img2tensor, normalize_, tensor2img
    face = np.random.default_rng(7).integers(0, 256, size=(512, 512, 3), dtype=np.uint8)
    x = normalize_(img2tensor(face / 255., bgr2rgb=True, float32=True), (0.5, 0.5, 0.5), (0.5, 0.5, 0.5)).unsqueeze(0)
    with torch.no_grad():
        want = tensor2img(small_net(x, w=0.5, adain=True)[0][0], rgb2bgr=True, min_max=(-1, 1))
    dst = torch.full((2, 512, 512, 3), 7, dtype=torch.uint8)
    got = small_net.restore_u8(torch.from_numpy(face).unsqueeze(0), w=0.5, adain=True, out=dst[:1])
    assert got.dtype == torch.uint8 and got.data_ptr() == dst.data_ptr()
    assert np.array_equal(got[0].numpy(), want)
    assert len(np.unique(want)) > 8 and bool((dst[1] == 7).all())
