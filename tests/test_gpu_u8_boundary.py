"""-m gpu: the uint8 image boundary.  cf_conv2d_u8 reads the uint8 HWC BGR faces in the network's first conv and writes them from its last
one; CodeFormer.restore_u8 is the network on top of both.  Everything here is BITWISE against the path it replaces
(cf_img_u8_to_tensor -> cf_conv2d ... cf_conv2d -> cf_tensor_to_img_u8): output tensors, GroupNorm partials, bytes, code indices.  The
shapes are the smallest at which each kernel can go wrong; the network runs on the real crops of tests/golden.
"""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
pytestmark = pytest.mark.gpu
REAL = ('real_0143.npz', 'real_0342.npz', 'real_Solvay_conference_1927_0018.npz')
POISON = 0xA5


@pytest.fixture(scope='module')
def env():
    import torch
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    from codeformer_amd import lib, ops
    lib.load()
    return torch, ops


# ---------------------------------------------------------------------------------------------------------------- first conv
@pytest.fixture(scope='module')
def first_pw(env):
    torch, ops = env
    torch.manual_seed(11)
    conv = torch.nn.Conv2d(3, 64, 3, padding=1)
    return conv, ops.pack_weight(conv.weight.cuda(), conv.bias.cuda())


def _byte_image(B, H, W, seed):
    """Every byte value, 0 and 255 in the four corners of every image (where the zero halo meets lut(0) = -1 and lut(255) = 1)."""
    rng = np.random.default_rng(seed)
    img = rng.permutation(np.arange(B * H * W * 3) % 256).astype(np.uint8).reshape(B, H, W, 3)
    img[:, 0, 0], img[:, 0, -1], img[:, -1, 0], img[:, -1, -1] = (0, 255, 0), (255, 0, 255), (255, 255, 0), (0, 0, 255)
    assert len(np.unique(img)) == 256
    return img


# (1,16,16): one tile, every pixel on a border; (3,32,48): halos that cross tiles, the batch offset
@pytest.mark.parametrize('shape', [(1, 16, 16), (3, 32, 48)])
def test_first_conv_reads_the_bytes(env, first_pw, shape):
    torch, ops = env
    conv, pw = first_pw
    img = torch.from_numpy(_byte_image(*shape, seed=shape[2])).cuda()
    x = ops.img_u8_to_tensor(img)
    want = ops.conv2d(x, pw, in_nchw=True, emit_stats=True)
    got = ops.conv2d(None, pw, in_nchw=True, emit_stats=True, img_in=img)
    assert got.shape == want.shape == (shape[0], shape[1], shape[2], 64) and got.dtype == torch.float32
    assert torch.equal(got, want)
    sw, sg = want._cf_stats, got._cf_stats
    assert (sg.parts, sg.cpg) == (sw.parts, sw.cpg) and torch.equal(sg.part, sw.part) and float(sw.part.abs().sum()) > 0
    # the two-launch path itself is the convolution of the normalised image (not two equal wrong answers)
    ref = torch.nn.functional.conv2d(x.cpu(), conv.weight.detach(), conv.bias.detach(), padding=1).permute(0, 2, 3, 1)
    assert float((want.cpu() - ref).abs().max()) <= 1e-4
    with pytest.raises(TypeError):
        ops.conv2d(None, pw, in_nchw=True, img_in=img.float())      # a wrong dtype is refused, never reinterpreted


def test_first_conv_non_temporal_variant(env, first_pw):
    """Two 512x512 faces: 134 MB of output, above cf_nt_store's 100 MB threshold -- the launch takes the non-temporal store variant."""
    torch, ops = env
    _, pw = first_pw
    assert 2 * 512 * 512 * 64 * 4 >= 100 << 20
    img = torch.from_numpy(np.random.default_rng(5).integers(0, 256, size=(2, 512, 512, 3), dtype=np.uint8)).cuda()
    want = ops.conv2d(ops.img_u8_to_tensor(img), pw, in_nchw=True, emit_stats=True)
    got = ops.conv2d(None, pw, in_nchw=True, emit_stats=True, img_in=img)
    assert torch.equal(got, want) and torch.equal(got._cf_stats.part, want._cf_stats.part)


# ---------------------------------------------------------------------------------------------------------------- last conv
def _head_case(torch, shape, seed):
    """64 -> 3 with a GroupNorm affine prologue.  The weight gain is chosen HERE, on the CPU, so that the planes saturate on both sides:
    a convolution output of standard deviation 0.78 has about 10 % of its values below -1 and 10 % above 1."""
    B, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, 64, generator=g)
    scale = 1.0 + 0.1 * torch.randn(B, 64, generator=g)
    shift = 0.1 * torch.randn(B, 64, generator=g)
    w = torch.randn(3, 64, 3, 3, generator=g)
    bias = 0.05 * torch.randn(3, generator=g)
    xn = (x * scale.view(B, 1, 1, 64) + shift.view(B, 1, 1, 64)).permute(0, 3, 1, 2)
    w = w * (0.78 / float(torch.nn.functional.conv2d(xn, w, None, padding=1).std()))
    return x, scale, shift, w, bias


# (1,16,16): one full tile; (2,24,40): masked edge tiles; (1,17,19): rows of 57 bytes -- row starts and the edge dword off the 4-byte grid.
# pad 64 / 61: the image itself on / off the 4-byte grid inside its poisoned buffer.
@pytest.mark.parametrize('pad', [64, 61])
@pytest.mark.parametrize('bf16_in', [False, True], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('shape', [(1, 16, 16), (2, 24, 40), (1, 17, 19)])
def test_last_conv_writes_the_bytes(env, shape, bf16_in, pad):
    torch, ops = env
    B, H, W = shape
    x, scale, shift, w, bias = _head_case(torch, shape, seed=H * W)
    pw = ops.pack_weight(w.cuda(), bias.cuda())
    xd = x.cuda().to(torch.bfloat16) if bf16_in else x.cuda()      # (a bf16 tensor: cf_conv_desc.io_bf16, the 'bf16' mode's head)
    kw = dict(prologue=ops.PRO_AFFINE, scale=scale.cuda(), shift=shift.cuda(), out_nchw=True)
    want = ops.tensor_to_img_u8(ops.conv2d(xd, pw, **kw))
    frac0, frac255 = float((want == 0).float().mean()), float((want == 255).float().mean())
    print(f'{shape} {"bf16" if bf16_in else "fp32"}: bytes 0: {frac0:.3f}  255: {frac255:.3f}  between: {1 - frac0 - frac255:.3f}')
    assert frac0 >= 0.05 and frac255 >= 0.05 and 1 - frac0 - frac255 >= 0.50       # the comparison below is not between two constants
    n = B * H * W * 3
    big = torch.full((pad + n + 64,), POISON, dtype=torch.uint8, device='cuda')
    dst = big[pad:pad + n].view(B, H, W, 3)
    got = ops.conv2d(xd, pw, img_out=dst, **kw)
    assert got.data_ptr() == dst.data_ptr() and torch.equal(got, want)
    assert bool((big[:pad] == POISON).all()) and bool((big[pad + n:] == POISON).all())     # nothing outside the image
    with pytest.raises(TypeError):
        ops.conv2d(xd, pw, img_out=dst.view(torch.int8), **kw)


# ---------------------------------------------------------------------------------------------------------------- network
@pytest.fixture(scope='module')
def net(env):
    torch, ops = env
    import codeformer_amd.archs  # noqa: F401
    from codeformer_amd.utils.registry import ARCH_REGISTRY
    torch.manual_seed(0)
    return ARCH_REGISTRY.get('CodeFormer')(dim_embd=512, codebook_size=1024, n_head=8, n_layers=9, connect_list=['32', '64', '128', '256']).eval().cuda()


@pytest.fixture(scope='module')
def crops(env):
    torch, _ = env
    imgs = [np.load(os.path.join(GOLD, n))['img'] for n in REAL]
    imgs += [np.ascontiguousarray(imgs[0][::-1]), np.ascontiguousarray(imgs[1][:, ::-1])]
    return torch.from_numpy(np.stack(imgs)).cuda()          # (5,512,512,3)


def _composed(ops, net, faces, w):
    return ops.tensor_to_img_u8(net(ops.img_u8_to_tensor(faces), w=w, adain=True)[0])


def _check_u8(got, ref):   # the rule of tests/test_gpu_real_images.py: at most 1 LSB, on at most 0.1 % of the bytes
    d = np.abs(got.astype(np.int16) - ref.astype(np.int16))
    assert int(d.max()) <= 1 and float((d > 0).mean()) <= 1e-3, (int(d.max()), float((d > 0).mean()))


@pytest.mark.parametrize('w', [0.0, 0.5])
@pytest.mark.parametrize('B', [1, 5])        # 1: graph replay under use_hip_graphs = 'auto'; 5: eager
@pytest.mark.parametrize('precision', ['f16x2', 'fp32', 'bf16'])
def test_restore_u8_is_the_composed_path(env, net, crops, precision, B, w):
    torch, ops = env
    assert net.use_hip_graphs == 'auto' and net.graph_max_batch == 4 and net.logit_guard == 'off'
    faces = crops[:B].contiguous()
    net.precision = precision
    try:
        want = _composed(ops, net, faces, w)
        idx = net.last_indices.clone()
        buf = torch.full((16, 512, 512, 3), POISON, dtype=torch.uint8, device='cuda')
        got = net.restore_u8(faces, w=w, adain=True)
        assert got.dtype == torch.uint8 and got.shape == (B, 512, 512, 3) and torch.equal(got, want)
        assert torch.equal(net.last_indices, idx)
        dst = buf[2:2 + B]                                   # out=: a slice of a 16-face buffer; the other rows stay
        assert net.restore_u8(faces, w=w, adain=True, out=dst).data_ptr() == dst.data_ptr()
        assert torch.equal(dst, want) and bool((buf[:2] == POISON).all()) and bool((buf[2 + B:] == POISON).all())
        assert torch.equal(net.restore_u8(faces, w=w, adain=True), want)       # (B = 1: a replay of the captured graph)
        if w == 0.5 and precision in ('f16x2', 'fp32'):      # the modes and the w the golden bytes of the reference were gated for
            for i, name in enumerate(REAL[:B]):
                _check_u8(got[i].cpu().numpy(), np.load(os.path.join(GOLD, name))['out_u8'])
    finally:
        net.precision = 'f16x2'


def test_restore_u8_recaptures_after_load_state_dict(env, net, crops):
    torch, ops = env
    face = crops[:1].contiguous()
    before = net.restore_u8(face, w=0.5, adain=True)
    key = 'generator.blocks.%d.bias' % (len(net.generator.blocks) - 1)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    changed = dict(sd)
    changed[key] = sd[key] + 0.25
    try:
        net.load_state_dict(changed)
        got = net.restore_u8(face, w=0.5, adain=True)
        assert torch.equal(got, _composed(ops, net, face, 0.5)) and not torch.equal(got, before)
    finally:
        net.load_state_dict(sd)
    assert torch.equal(net.restore_u8(face, w=0.5, adain=True), before)


@pytest.mark.parametrize('B', [1, 5])
def test_guard_rerun_replaces_the_flagged_faces(env, net, crops, B):
    """logit_guard_gap so large that every face is flagged: the bytes are those of a network whose encoder runs F(2x2,3x3), and the
    counters are what forward reports on the same input."""
    torch, ops = env
    faces = crops[:B].contiguous()
    assert net.winograd_f43_encoder
    try:
        net.winograd_f43_encoder = False
        want = _composed(ops, net, faces, 0.5)
        idx = net.last_indices.clone()
        net.winograd_f43_encoder = True
        net.logit_guard, net.logit_guard_gap = 'rerun', 1e9
        net.reset_guard_stats()
        assert torch.equal(_composed(ops, net, faces, 0.5), want)
        st_forward, gap = net.guard_stats, net.last_min_gap.clone()
        net.reset_guard_stats()
        got = net.restore_u8(faces, w=0.5, adain=True)
        assert torch.equal(got, want) and torch.equal(net.last_indices, idx) and torch.equal(net.last_min_gap, gap)
        st = net.guard_stats
        assert st == st_forward and (st['calls'], st['faces'], st['flagged'], st['rerun_faces']) == (1, B, B, B)
        net.logit_guard = 'report'
        net.reset_guard_stats()
        plain = net.restore_u8(faces, w=0.5, adain=True)
        assert net.guard_stats['flagged'] == B and net.guard_stats['rerun_faces'] == 0
        net.logit_guard = 'off'
        assert torch.equal(plain, net.restore_u8(faces, w=0.5, adain=True))
    finally:
        net.winograd_f43_encoder, net.logit_guard, net.logit_guard_gap = True, 'off', 1.1e-4
        net.reset_guard_stats()


# ---------------------------------------------------------------------------------------------------------------- callers
class _Counting:
    """The real network behind its call signature and restore_u8, counting the calls of each."""

    def __init__(self, net):
        self.net, self.forward_calls, self.u8_calls = net, 0, 0

    def __call__(self, x, **kw):
        self.forward_calls += 1
        return self.net(x, **kw)

    def restore_u8(self, faces, **kw):
        self.u8_calls += 1
        return self.net.restore_u8(faces, **kw)


@pytest.fixture()
def converters(env, monkeypatch):
    """Counts the calls of the two stand-alone converters."""
    _, ops = env
    seen = {'in': 0, 'out': 0}
    to_t, to_u8 = ops.img_u8_to_tensor, ops.tensor_to_img_u8

    def count_in(img):
        seen['in'] += 1
        return to_t(img)

    def count_out(t):
        seen['out'] += 1
        return to_u8(t)

    monkeypatch.setattr(ops, 'img_u8_to_tensor', count_in)
    monkeypatch.setattr(ops, 'tensor_to_img_u8', count_out)
    return seen


def test_pipeline_uses_restore_u8(env, net, crops, converters, tmp_path):
    torch, ops = env
    from PIL import Image
    from codeformer_amd.pipeline import AlignedFacePipeline
    paths = []
    for i in range(3):
        Image.fromarray(crops[i].cpu().numpy()[:, :, ::-1]).save(tmp_path / f'in{i}.png')
        paths.append(str(tmp_path / f'in{i}.png'))

    def run(network, tag):
        outs = [str(tmp_path / tag / f'in{i}.png') for i in range(3)]
        st = AlignedFacePipeline(network, 'cuda', batch_size=2, workers=2, slots=2).restore(paths, outs, w=0.5)
        assert st['faces'] == 3 and st['batches'] == 2 and st['failures'] == 0
        return [np.asarray(Image.open(o)) for o in outs]

    real = _Counting(net)
    a = run(real, 'u8')
    assert (real.u8_calls, real.forward_calls) == (2, 0) and converters == {'in': 0, 'out': 0}
    b = run(lambda x, w=0.5, adain=True: net(x, w=w, adain=adain), 'stub')        # the call signature only: today's sequence
    assert converters == {'in': 2, 'out': 2}
    assert all(np.array_equal(p, q) for p, q in zip(a, b)) and len(np.unique(a[0])) > 8


def test_video_restorer_uses_restore_u8(env, net, converters):
    torch, ops = env
    from codeformer_amd.video import VideoRestorer
    rng = np.random.default_rng(3)
    frames = [rng.integers(0, 256, size=(96, 128, 3), dtype=np.uint8) for _ in range(2)]
    affs = [np.array([[[6.0, 0.0, -100.0 - 40 * i], [0.0, 6.0, -30.0]]]) for i in range(2)]     # one 85-pixel face per frame

    def run(network):
        vr = VideoRestorer(network, 'cuda', upscale=1, batch_size=4)
        out = vr.restore(frames, affs, w=0.5)
        assert vr.stats == {'frames': 2, 'faces': 2, 'forward_calls': 1}
        return out

    real = _Counting(net)
    a = run(real)
    assert (real.u8_calls, real.forward_calls) == (1, 0) and converters == {'in': 0, 'out': 0}
    b = run(lambda x, w=0.5, adain=True: net(x, w=w, adain=adain))
    assert converters == {'in': 1, 'out': 1}
    assert all(np.array_equal(p, q) for p, q in zip(a, b)) and any((p != f).any() for p, f in zip(a, frames))
