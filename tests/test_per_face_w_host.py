"""One fidelity weight per face (cf_conv2d_sft_w, ops.conv2d(sft_w=tensor), CodeFormer.forward / restore_u8 / restore_sweep with a vector w,
inference_codeformer.py --fidelity_sweep), the parts that need no GPU: the C ABI declaration and binding, the argument checks of the entry
point (they run before any launch), the refusals of the operator and module layers, the CPU forms against the scalar calls, the flag."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from _tools import load_script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'codeformer_hip.h')
FAKE = 0x1000   # a non-NULL "device pointer": every call below is refused before anything is launched


def test_symbol_is_declared_and_bound():
    from codeformer_amd import lib
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    m = re.search(r'int\s+cf_conv2d_sft_w\s*\(([^)]*)\)', src)
    assert m, 'cf_conv2d_sft_w is not declared in include/codeformer_hip.h'
    params = [p.strip() for p in m.group(1).split(',')]
    assert len(params) == 3 and 'cf_conv_desc' in params[0] and 'const float' in params[1] and 'w_img' in params[1] and 'cf_stream_t' in params[2]
    res, args = lib.SIGNATURES['cf_conv2d_sft_w']
    assert res is ctypes.c_int and len(args) == 3 and lib.ABI_VERSION == 22


@pytest.fixture(scope='module')
def native():
    from codeformer_amd import build as cf_build
    from codeformer_amd import lib
    cf_build.build()
    n = lib.load()
    assert n.cf_version() == 22           # additive: the struct layout and the version stay
    return n


def _sft(**kw):
    """The descriptor of a fusion block's last conv (128 -> 128 with the SFT epilogue) at 2 x 32x32."""
    from codeformer_amd import lib
    d = dict(in0=FAKE, c0=128, c1=0, batch=2, hin=32, win=32, hout=32, wout=32, cout=128, cout_pad=128, taps=9, stride=1,
             prologue=lib.PRO_LEAKY, epilogue=lib.EPI_SFT, weight=FAKE, bias=FAKE, res=FAKE, sft_scale=FAKE, out=FAKE, acc_scale=1.0)
    d.update(kw)
    return lib.ConvDesc(**d)


def test_entry_point_refuses_a_null_table_and_other_epilogues(native):
    from codeformer_amd import lib
    assert native.cf_conv2d_sft_w(ctypes.byref(_sft()), None, None) == -1
    err = lib.last_error()
    assert err.startswith('cf_conv2d_sft_w:') and 'w_img' in err and 'NULL' in err, err
    for epi in (lib.EPI_NONE, lib.EPI_RESIDUAL, lib.EPI_GELU, lib.EPI_AXPY):
        assert native.cf_conv2d_sft_w(ctypes.byref(_sft(epilogue=epi)), FAKE, None) == -1
        err = lib.last_error()
        assert err.startswith('cf_conv2d_sft_w:') and 'SFT' in err and f'epilogue {epi}' in err, err
    assert native.cf_conv2d_sft_w(None, FAKE, None) == -1
    # with the table and the epilogue in place the descriptor goes on to cf_conv2d's own checks: a bad one is still refused before a launch
    assert native.cf_conv2d_sft_w(ctypes.byref(_sft(hout=48)), FAKE, None) == -1
    assert 'hout/wout' in lib.last_error()


def test_ops_refuse_a_weight_tensor_that_is_not_one_float_per_image(native):
    """The checks of ops.conv2d on sft_w run before the device pointers are taken (which is where CPU tensors are refused)."""
    from codeformer_amd import ops
    pw = ops.PackedWeight(torch.zeros(1), None, 64, 64, 9, 64, 64)
    x, r = torch.zeros(2, 16, 16, 64), torch.zeros(2, 16, 16, 64)
    kw = dict(epilogue=ops.EPI_SFT, res=r, sft_scale=r)
    with pytest.raises(ValueError, match='one per image'):
        ops.conv2d(x, pw, sft_w=torch.ones(3), **kw)                            # three weights for two images
    with pytest.raises(ValueError, match='one per image'):
        ops.conv2d(x, pw, sft_w=torch.ones(2, 1), **kw)                         # not a vector
    with pytest.raises(TypeError, match='float32'):
        ops.conv2d(x, pw, sft_w=torch.ones(2, dtype=torch.float64), **kw)
    with pytest.raises(TypeError, match='float32'):
        ops.conv2d(x, pw, sft_w=torch.ones(2, dtype=torch.int64), **kw)
    with pytest.raises(ValueError, match='EPI_SFT'):
        ops.conv2d(x, pw, sft_w=torch.ones(2), epilogue=ops.EPI_RESIDUAL, res=r)   # a tensor is the SFT epilogue's
    with pytest.raises(ValueError, match='CUDA'):
        ops.conv2d(x, pw, sft_w=torch.ones(2), **kw)                            # well-formed: goes on, and CPU tensors are refused as ever


@pytest.fixture(scope='module')
def small_net():
    import codeformer_amd.archs  # noqa: F401
    from codeformer_amd.utils.registry import ARCH_REGISTRY
    torch.manual_seed(0)
    return ARCH_REGISTRY.get('CodeFormer')(dim_embd=64, codebook_size=32, n_head=2, n_layers=1, connect_list=['32']).eval()


def test_face_weights_reads_every_form_the_same_way():
    from codeformer_amd.archs.codeformer_arch import FaceWeights, face_weights
    vals = [0.2, 0.0, -1.0, float('nan')]
    forms = [vals, tuple(vals), np.array(vals), np.array(vals, dtype=np.float32), torch.tensor(vals), torch.tensor(vals, dtype=torch.float64)]
    for w in forms:
        fw = face_weights(w, 4)
        assert isinstance(fw, FaceWeights) and fw.fused == (True, False, False, False)       # a NaN is not fused: `if w > 0`
        assert fw.host[:3] == (float(np.float32(0.2)), 0.0, -1.0) and fw.host[3] != fw.host[3]
        assert fw.rows_fused == [0] and fw.rows_unfused == [1, 2, 3] and fw.mixed
    assert face_weights([1, 2], 2).all_fused and face_weights(np.array([0, -3]), 2).none_fused      # integers are real weights
    from codeformer_amd.archs.codeformer_arch import is_scalar_weight
    for scalar in (0.5, 1, True, np.float32(0.5), np.bool_(True), np.array(0.5), torch.tensor(0.5)):   # a number stays the scalar call
        assert not isinstance(face_weights(scalar, 4), FaceWeights) and is_scalar_weight(scalar)
    for vector in ([0.5], (0.5,), np.array([0.5]), torch.tensor([0.5])):
        assert not is_scalar_weight(vector)
    for bad in (np.str_('0.5'), [0.5, np.bool_(True)], [0.5, True], [torch.tensor(True), 0.5]):       # neither numbers nor real weights
        with pytest.raises(TypeError):
            face_weights(bad, 2)
    assert face_weights([0.7, 0.3, 1.0], 3).rows([2, 0]).host == (1.0, float(np.float32(0.7)))


def test_forward_refuses_wrong_lengths_and_dtypes(small_net):
    x = torch.zeros(2, 3, 512, 512)
    for bad in ([0.5], (0.5, 0.5, 0.5), np.ones(3), torch.ones(1), torch.ones(2, 1), np.ones((1, 2))):
        with pytest.raises(ValueError, match='one weight per face'):
            small_net(x, w=bad)
        with pytest.raises(ValueError, match='one weight per face'):
            small_net.restore_u8(torch.zeros(2, 512, 512, 3, dtype=torch.uint8), w=bad)
    for bad in (['a', 'b'], [0.5, None], np.array(['a', 'b']), np.array([True, False]), torch.tensor([True, False]),
                torch.ones(2, dtype=torch.complex64), 'half', {0.5, 0.7}):
        with pytest.raises(TypeError):
            small_net(x, w=bad)
    with pytest.raises(ValueError):
        small_net.restore_sweep(x, [])
    with pytest.raises(ValueError):
        small_net.restore_sweep(x, [[0.5, 0.7]])


def test_fuse_block_cpu_vector_is_the_broadcast_formula(small_net):
    """Fuse_sft_block.forward on CPU tensors with one weight per face == dec + w.view(B,1,1,1) * (dec * scale(e) + shift(e)) computed here
    from the block's own submodules on the same batch, bitwise."""
    blk = small_net.fuse_convs_dict['32']
    g = torch.Generator().manual_seed(3)
    enc, dec = torch.randn(3, 256, 8, 8, generator=g), torch.randn(3, 256, 8, 8, generator=g)
    w = torch.tensor([0.5, 1.0, 0.125])
    with torch.no_grad():
        got = blk(enc, dec, w)
        e = blk.encode_enc(torch.cat([enc, dec], dim=1))
        want = dec + w.view(3, 1, 1, 1) * (dec * blk.scale(e) + blk.shift(e))
        one = blk(enc, dec, 0.5)
    assert torch.equal(got, want)
    assert torch.equal(one, dec + 0.5 * (dec * blk.scale(e) + blk.shift(e)))     # the scalar call is what it was
    assert not torch.equal(got[1:], one[1:])
    with pytest.raises(ValueError, match='one weight per face'):
        blk(enc, dec, torch.ones(2))


@pytest.fixture(scope='module')
def two_faces():
    g = torch.Generator().manual_seed(11)
    return torch.rand(2, 3, 512, 512, generator=g) * 2 - 1


@pytest.fixture(scope='module')
def scalar_calls(small_net, two_faces):
    """The reference of the CPU tests: face 0 at w = 0.7, face 1 at w = 0 and face 0 at w = 0, each alone, computed once."""
    with torch.no_grad():
        return [small_net(two_faces[b:b + 1], w=w, adain=True) for b, w in ((0, 0.7), (1, 0.0), (0, 0.0))]


def test_cpu_forward_with_a_mixed_vector_matches_the_scalar_calls(small_net, two_faces, scalar_calls):
    """One positive and one zero weight on two faces: rows against the two scalar CPU calls at the suite's gates (pixels 1e-3, logits 1e-4;
    CPU convolutions are not batch-invariant, so bitwise equality is not asked here -- the GPU tests ask it)."""
    with torch.no_grad():
        out, logits, lq = small_net(two_faces, w=(0.7, 0.0), adain=True)
    assert out.shape == (2, 3, 512, 512)
    for b, (o1, l1, q1) in enumerate(scalar_calls[:2]):
        px, lg = float((out[b] - o1[0]).abs().max()), float((logits[b] - l1[0]).abs().max())
        print(f'face {b}: max |pixel diff| {px:.3g}, max |logit diff| {lg:.3g}')
        assert px < 1e-3 and lg < 1e-4
        assert float((lq[b] - q1[0]).abs().max()) < 1e-4
    # the fused and the un-fused row are different functions of their input: the partition is not a no-op
    assert float((out[0] - scalar_calls[2][0][0]).abs().max()) > 1e-2


def test_zero_dim_tensor_is_the_number_it_holds(small_net, two_faces, scalar_calls):
    """A 0-dim tensor w is a scalar w: `w > 0` decides, as it always did -- 0, -1 and NaN run un-fused and equal the float call bit for bit
    (one face: the same operations on the same batch); a positive one is fused."""
    x = two_faces[:1]
    unfused, fused = scalar_calls[2][0], scalar_calls[0][0]
    with torch.no_grad():
        for v in (0.0, -1.0, float('nan')):
            assert torch.equal(small_net(x, w=torch.tensor(v), adain=True)[0], unfused), v
        assert torch.equal(small_net(x, w=-1.0, adain=True)[0], unfused) and torch.equal(small_net(x, w=np.float32(-1.0), adain=True)[0], unfused)
        assert torch.equal(small_net(x, w=torch.tensor(0.7), adain=True)[0], fused)
        assert torch.equal(small_net.restore_sweep(x, torch.tensor([-1.0, float('nan')]), adain=True)[0][1], unfused)
    blk = small_net.fuse_convs_dict['32']
    g = torch.Generator().manual_seed(4)
    enc, dec = torch.randn(1, 256, 8, 8, generator=g), torch.randn(1, 256, 8, 8, generator=g)
    with torch.no_grad():
        assert torch.equal(blk(enc, dec, torch.tensor(0.25)), blk(enc, dec, 0.25))


def test_kernel_resources_tool_reads_the_build(native):
    """tools/kernel_resources.py on the objects of this build: every kernel of the library with its registers, and the statement DESIGN.md
    makes with it -- no F(4,3) instantiation above 128 vector registers (two 8-wave or one 16-wave workgroup per CU)."""
    from codeformer_amd import build as cf_build
    kr = load_script('tools/kernel_resources.py')
    table = kr.build_table(cf_build._cache_dir())
    wf43 = {k: v for k, v in table.items() if k[0] == 'cf_wf43' and 'wf43_kernel' in k[1]}
    assert len(table) > 200 and len(wf43) >= 60
    assert all(0 < v['v'] <= 128 and v['a'] == 0 for v in wf43.values())
    assert {v['kernarg'] for v in wf43.values()} == {424}            # F4Args (168 bytes) + the 256 hidden bytes


def test_cpu_restore_sweep_matches_the_scalar_calls(small_net, two_faces, scalar_calls):
    """The host form of restore_sweep: outs[k, b] against forward(x[b:b+1], w=ws[k]) at the same gates, for one face and (0.7, 0.0)."""
    with torch.no_grad():
        outs, logits, lq = small_net.restore_sweep(two_faces[:1], (0.7, 0.0), adain=True)
    assert outs.shape == (2, 1, 3, 512, 512) and logits.shape[0] == 1 and lq.shape[0] == 1
    assert float((outs[0, 0] - scalar_calls[0][0][0]).abs().max()) < 1e-3
    assert float((outs[1, 0] - scalar_calls[2][0][0]).abs().max()) < 1e-3
    assert float((logits[0] - scalar_calls[0][1][0]).abs().max()) < 1e-4


def test_fidelity_sweep_flag():
    cli = load_script('inference_codeformer.py')
    args = cli.parse_args(['--has_aligned', '-i', 'faces', '--fidelity_sweep', '0', '0.3', '0.75', '1'])
    assert args.fidelity_sweep == [0.0, 0.3, 0.75, 1.0] and args.fidelity_weight == 0.5     # -w keeps its default and its meaning
    cli.check_args(args)
    assert [cli.sweep_name('00', w) for w in args.fidelity_sweep] == ['00_w0.00.png', '00_w0.30.png', '00_w0.75.png', '00_w1.00.png']
    assert cli.sweep_name('face', 0.5, suffix='x') == 'face_w0.50_x.png'
    assert cli.parse_args(['--has_aligned']).fidelity_sweep is None
    with pytest.raises(NotImplementedError, match='--has_aligned'):
        cli.check_args(cli.parse_args(['-i', 'imgs', '--fidelity_sweep', '0.5', '0.7']))
    with pytest.raises(ValueError, match='file name'):
        cli.check_args(cli.parse_args(['--has_aligned', '--fidelity_sweep', '0.501', '0.499']))
    with pytest.raises(SystemExit):
        cli.parse_args(['--has_aligned', '--fidelity_sweep'])                                 # at least one weight


def test_fidelity_sweep_writes_one_file_per_face_and_weight(tmp_path, small_net, monkeypatch):
    """The CLI on the CPU with two small aligned faces and a stand-in network: restored_faces/<name>_w<W>.png for every face and weight,
    through restore_sweep (one call for both faces), nothing else in the folder."""
    cli = load_script('inference_codeformer.py')
    from codeformer_amd.utils.img_util import imwrite
    rng = np.random.default_rng(5)
    src = tmp_path / 'in'
    src.mkdir()
    for name in ('a', 'b'):
        imwrite(rng.integers(0, 256, size=(512, 512, 3), dtype=np.uint8), str(src / f'{name}.png'))
    calls = []

    class Net:
        logit_guard = 'off'

        def restore_sweep(self, x, ws, adain=False):
            calls.append((tuple(x.shape), list(ws), adain))
            return torch.stack([x * 0 + (2 * w - 1) for w in ws]), None, None

    monkeypatch.setattr(cli, 'build_net', lambda device, args: Net())
    out = tmp_path / 'out'
    rc = cli.main(['--has_aligned', '-i', str(src), '-o', str(out), '--device', 'cpu', '--batch_size', '6', '--fidelity_sweep', '0', '0.5', '1'])
    assert rc == 0 and calls == [((2, 3, 512, 512), [0.0, 0.5, 1.0], True)]
    assert sorted(os.listdir(out / 'restored_faces')) == [f'{n}_w{w}.png' for n in ('a', 'b') for w in ('0.00', '0.50', '1.00')]
    from codeformer_amd.utils.img_util import imread_bgr
    assert int(imread_bgr(str(out / 'restored_faces' / 'a_w0.00.png')).max()) == 0 and int(imread_bgr(str(out / 'restored_faces' / 'b_w1.00.png')).min()) == 255
