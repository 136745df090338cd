"""-m gpu: the HIP path on the reference's OWN input images against outputs of the reference (tests/golden/real_*.npz,
made by oracle/make_golden_real.py from inputs/cropped_faces and inputs/masked_faces), plus the network-level w=0.7 gate of
BASELINE config 3, the index-exactness sweep, VectorQuantizer.forward's statistics and the tensor-boundary known answers.

Tolerances (north star): pixels atol 1e-3, logits 1e-4, code indices exact -- except tokens whose REFERENCE top-1/top-2
logit gap is below 1e-5 (there the reference's own thread-count noise, 2.6e-6 on logits, decides the winner;
such a token must still pick one of the reference's top two).  uint8 images: at most 1 LSB, on at most 0.1 % of the bytes
(a float that sits within 1e-4 of a rounding boundary may land on either side).
"""
import os

import numpy as np
import pytest

from _tools import load_script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
pytestmark = pytest.mark.gpu

REAL = ('real_0143.npz', 'real_0342.npz', 'real_Solvay_conference_1927_0018.npz')
# precision modes of CodeFormer.precision and their pixel gates against the fp32 reference: (max |d|, mean |d|)
# (bf16: 1.65x / 1.32x the cost of bf16 operands for ANY implementation with these weights -- the CPU oracle with the same 58 convolutions'
# operands rounded to bf16 differs from the fp32 reference by 0.1094 / 0.01064: tools/bf16_gate_derivation.py, profiles/r05_bf16_gate_derivation.txt)
GATES = {'fp32': (1e-3, 1e-4), 'f16x2': (1e-3, 1e-4), 'fp16': (0.04, 0.003), 'bf16': (0.196, 0.0152)}


@pytest.fixture(scope='module')
def chk():
    import torch
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    from codeformer_amd import lib
    lib.load()
    return load_script('tools/gpu_check.py')


@pytest.fixture(scope='module')
def net(chk):
    return chk.build_net().cuda()


def _check_indices(got, g):
    got, ref, gap = got.reshape(-1), g['idx'].reshape(-1), g['gap'].reshape(-1)
    safe = gap >= 1e-5
    assert np.array_equal(got[safe], ref[safe]), f'{int((got[safe] != ref[safe]).sum())} code indices differ'
    return int((~safe).sum())


def _check_u8(got, ref):
    d = np.abs(got.astype(np.int16) - ref.astype(np.int16))
    assert int(d.max()) <= 1 and float((d > 0).mean()) <= 1e-3, (int(d.max()), float((d > 0).mean()))


@pytest.mark.parametrize('precision', ['fp32', 'f16x2'])
@pytest.mark.parametrize('name', REAL)
def test_real_aligned_faces_match_the_reference(net, name, precision):
    """uint8 crop -> cf_img_u8_to_tensor -> CodeFormer.forward(w=0.5, adain) -> cf_tensor_to_img_u8, every stage against
    what the reference produced for the same PNG."""
    import torch
    from codeformer_amd import ops
    g = np.load(os.path.join(GOLD, name))
    net.precision = precision
    x = ops.img_u8_to_tensor(torch.from_numpy(g['img']).unsqueeze(0).cuda())
    ref_x = ((torch.from_numpy(np.ascontiguousarray((g['img'][:, :, ::-1] / 255.).astype(np.float32).transpose(2, 0, 1))) - 0.5) / 0.5)
    assert torch.equal(x[0].cpu(), ref_x)
    out, logits, _ = net(x, w=0.5, adain=True)
    dl = float((logits.cpu() - torch.from_numpy(g['logits'])).abs().max())
    near = _check_indices(net.last_indices.cpu().numpy(), g)
    dp = float((out.cpu()[:, :, ::4, ::4] - torch.from_numpy(g['out_sub'])).abs().max())
    print(f'{name} [{precision}]: logits {dl:.2e}  pixels {dp:.2e}  near-tie tokens {near}  min gap {g["gap"].min():.2e}')
    assert dl <= 1e-4 and dp <= 1e-3
    _check_u8(ops.tensor_to_img_u8(out)[0].cpu().numpy(), g['out_u8'])
    net.precision = 'fp32'


@pytest.mark.parametrize('precision', ['f16x2', 'fp32'])
def test_encoder_logit_margin(chk, precision):
    """The gate behind Winograd F(4x4,3x3) in the ENCODER (CodeFormer.winograd_f43_encoder, on by default since round 5): over every
    golden with reference logits -- seeded face, three real crops, masked face (inpainting net), four range variants (full logits) and the
    32-face sweep (tests/golden/logit_sweep32.npz, the reference's top-8 codes per token) -- and every token whose reference top-2 gap is
    >= 1e-5:   (reference gap) / (2 x max |our logit - reference logit|)  >=  5,   no index differs, and no code outside the reference's
    top-8 comes anywhere near the winner.  Measured on MI355X: 7.0 ('f16x2') / 7.3 ('fp32') with the switch on, 9.9 / 8.7 with it off."""
    lm = load_script('tools/logit_margin.py')
    default_on = chk.build_net().winograd_f43_encoder
    r = lm.measure(lm.Nets(chk), chk, precision, default_on)
    rows = {k: v for k, v in r.items() if not k.startswith('_')}
    for k, v in rows.items():
        print(f'{k:40s} [{precision}, encoder F(4,3) {default_on}] min margin {v[0]:9.2f}  max logit error {v[1]:.2e}  near ties {v[2]}  indices differing {v[3]}')
    assert len(rows) == 10
    assert all(v[3] == 0 for v in rows.values())                       # every index on every safe token
    assert all(v[1] <= 1e-4 for v in rows.values())                    # the north-star logit tolerance
    assert min(v[0] for v in rows.values()) >= 5.0, min(v[0] for v in rows.values())
    assert r['_sweep32_outside_top8_distance'] >= 1e-2                 # (top-8 is enough: the ninth code is ~1e-1 below the winner)


def test_real_masked_face_inpainting_matches_the_reference(chk):
    """BASELINE config 5 on inputs/masked_faces/00105.png: codebook 512, 3 fuse levels, w=1, adain=False, then the white-brush
    composite (inference_inpainting.py:68-74) and tensor2img -- bytes against the reference's saved face."""
    import torch
    from codeformer_amd import cli, ops
    g = np.load(os.path.join(GOLD, 'real_masked_00105.npz'))
    net = chk.build_net(512, ('32', '64', '128')).cuda()
    x = ops.img_u8_to_tensor(torch.from_numpy(g['img']).unsqueeze(0).cuda())
    out, logits, _ = net(x, w=1, adain=False)
    assert float((logits.cpu() - torch.from_numpy(g['logits'])).abs().max()) <= 1e-4
    _check_indices(net.last_indices.cpu().numpy(), g)
    assert float((out.cpu()[:, :, ::4, ::4] - torch.from_numpy(g['out_sub'])).abs().max()) <= 1e-3
    comp = cli.inpaint_composite(x, out)
    m = torch.from_numpy(g['mask']).bool().cuda().expand_as(x)
    assert int(m.sum()) > 3000 and torch.equal(comp[m], out[m]) and torch.equal(comp[~m], x[~m])
    _check_u8(ops.tensor_to_img_u8(comp)[0].cpu().numpy(), g['comp_u8'])


def test_mask_composite_against_the_oracle(chk):
    """cf_mask_composite against the CPU restatement of inference_inpainting.py:68-74 (not against this package's own code)."""
    import torch
    from codeformer_amd import ops
    from oracle import codeformer_oracle as O
    x = torch.rand(2, 3, 32, 40, generator=torch.Generator().manual_seed(3)) * 2 - 1
    x[0, :, 4:9, 5:20] = 1.0
    x[1, 0, 0, 0] = 1.0  # only one channel white -> not masked
    y = torch.randn(2, 3, 32, 40, generator=torch.Generator().manual_seed(4))
    assert torch.equal(ops.mask_composite(x.cuda(), y.cuda()).cpu(), O.inpaint_composite(x, y))


@pytest.mark.parametrize('precision', ['fp32', 'f16x2', 'fp16', 'bf16'])
def test_config3_fidelity_weight_through_the_network(net, precision):
    """BASELINE config 3 (w=0.7) through the whole network; 16-bit operand modes against stated gates (measured: see print)."""
    import torch
    from oracle.synth import seeded_input
    g = np.load(os.path.join(GOLD, 'restoration_seed0_face0_w0.7.npz'))
    g0 = np.load(os.path.join(GOLD, 'restoration_seed0_face0.npz'))
    net.precision = precision
    out, logits, _ = net(seeded_input(1).cuda(), w=0.7, adain=True)
    net.precision = 'fp32'
    d = (out.cpu()[:, :, ::4, ::4] - torch.from_numpy(g['out_sub'])).abs()
    print(f'w=0.7 [{precision}]: max|d| {float(d.max()):.3e} mean|d| {float(d.mean()):.3e}')
    assert np.array_equal(net.last_indices.cpu().numpy(), g0['idx'])
    assert float((logits.cpu() - torch.from_numpy(g0['logits'])).abs().max()) <= 1e-4
    gmax, gmean = GATES[precision]
    assert float(d.max()) <= gmax and float(d.mean()) <= gmean
    if precision in ('fp32', 'f16x2'):
        from codeformer_amd import ops
        _check_u8(ops.tensor_to_img_u8(out)[0].cpu().numpy(), g['out_u8'])


def test_index_exactness_sweep(net):
    """Eight more seeded faces in one batch: every code index equals the reference's (tokens with a reference gap < 1e-5 must
    pick one of the reference's top two: face 6 holds a 4.8e-7 near-tie)."""
    from oracle.synth import seeded_input
    g = np.load(os.path.join(GOLD, 'index_sweep_seed2024.npz'))
    x = seeded_input(16, seed=2024)[:8].cuda()
    logits, _ = net(x, w=0.5, code_only=True)
    idx = logits.argmax(-1).cpu().numpy()
    safe = g['gap'] >= 1e-5
    assert np.array_equal(idx[safe], g['idx'][safe]), f'{int((idx[safe] != g["idx"][safe]).sum())} indices differ'
    top2 = logits.topk(2, dim=-1).indices.cpu().numpy()
    for b, t in zip(*np.nonzero(~safe)):
        assert g['idx'][b, t] in top2[b, t]
    print(f'index sweep: {int(safe.sum())}/2048 tokens gated exactly, {int((~safe).sum())} near-ties, min gap {g["gap"].min():.2e}')


def test_vector_quantizer_statistics_match_the_reference(chk):
    """VectorQuantizer.forward on the GPU: indices, z_q, loss, perplexity, mean_distance and the one-hot usage counts against
    the reference module's outputs (vqgan_arch.py:33-70)."""
    import torch
    import codeformer_amd.archs  # noqa: F401
    from codeformer_amd.archs.vqgan_arch import VectorQuantizer
    g = np.load(os.path.join(GOLD, 'vq_seed11.npz'))
    s = np.load(os.path.join(GOLD, 'vq_stats_seed11.npz'))
    q = VectorQuantizer(1024, 256, 0.25)
    q.embedding.weight.data.copy_(torch.from_numpy(g['codebook']))
    q = q.cuda().eval()
    zq, loss, st = q(torch.from_numpy(g['z']).cuda())
    assert np.array_equal(st['min_encoding_indices'].view(-1).cpu().numpy(), g['idx'])
    assert float((zq.cpu() - torch.from_numpy(g['zq'])).abs().max()) <= 1e-9
    assert np.array_equal(st['min_encodings'].sum(0).cpu().numpy(), s['counts'])
    for k, v in (('loss', loss), ('perplexity', st['perplexity']), ('mean_distance', st['mean_distance'])):
        rel = abs(float(v) - float(s[k])) / abs(float(s[k]))
        print(f'vq {k}: {float(v):.8e} vs reference {float(s[k]):.8e} (rel {rel:.1e})')
        assert rel <= 1e-5, k


def test_tensor2img_bytes_equal_the_reference(chk):
    import torch
    from codeformer_amd import ops
    k = np.load(os.path.join(GOLD, 'tensor2img_kat.npz'))
    got = ops.tensor_to_img_u8(torch.from_numpy(k['t']).unsqueeze(0).cuda())[0].cpu().numpy()
    assert np.array_equal(got, k['img'])


def test_overlapped_pipeline_writes_the_direct_path_bytes(net, tmp_path):
    """codeformer_amd.pipeline (pinned staging, copy streams, decode / encode workers, partial last batch) against the plain
    sequence decode -> cf_img_u8_to_tensor -> forward -> cf_tensor_to_img_u8 -> encode on the same files."""
    import torch
    from PIL import Image
    from codeformer_amd import ops
    from codeformer_amd.pipeline import AlignedFacePipeline
    imgs = [np.load(os.path.join(GOLD, n))['img'] for n in REAL]
    imgs += [np.ascontiguousarray(imgs[0][::-1]), np.repeat(imgs[1].mean(-1, keepdims=True).astype(np.uint8), 3, axis=2)]   # + a gray one
    paths, outs = [], []
    for i, a in enumerate(imgs):
        p = tmp_path / f'in{i}.png'
        Image.fromarray(a[:, :, ::-1]).save(p)
        paths.append(str(p))
        outs.append(str(tmp_path / 'out' / f'in{i}.png'))
    pipe = AlignedFacePipeline(net, 'cuda', batch_size=2, workers=3, slots=2)
    st = pipe.restore(paths, outs, w=0.5)
    assert st['faces'] == 5 and st['batches'] == 3 and st['failures'] == 0
    for a, o in zip(imgs, outs):
        x = ops.img_u8_to_tensor(torch.from_numpy(a).unsqueeze(0).cuda())
        want = ops.tensor_to_img_u8(net(x, w=0.5, adain=True)[0])[0].cpu().numpy()
        got = np.asarray(Image.open(o))[:, :, ::-1]
        assert np.array_equal(got, want), o


def test_boundary_kernels_on_sizes_off_the_vector_grid(chk):
    """cf_img_u8_to_tensor / cf_tensor_to_img_u8 convert four pixels per thread; sizes with h*w % 4 != 0 take the per-pixel tail."""
    import torch
    from codeformer_amd import ops
    from oracle import codeformer_oracle as O
    rng = np.random.default_rng(7)
    for h, w in ((5, 7), (3, 3), (16, 18)):
        img = rng.integers(0, 256, (3, h, w, 3), dtype=np.uint8)
        t = ops.img_u8_to_tensor(torch.from_numpy(img).cuda())
        ref = torch.from_numpy(((img[..., ::-1] / 255.).astype(np.float32).transpose(0, 3, 1, 2) - 0.5) / 0.5)
        assert torch.equal(t.cpu(), ref), (h, w)
        x = torch.randn(3, 3, h, w, generator=torch.Generator().manual_seed(h)) * 1.2
        got = ops.tensor_to_img_u8(x.cuda()).cpu().numpy()
        for b in range(3):
            assert np.array_equal(got[b], O.tensor2img_u8(x[b])), (h, w)


def test_dtype_mismatch_is_refused_not_reinterpreted(chk):
    import torch
    from codeformer_amd import ops
    cb = torch.randn(1024, 256, device='cuda')
    idx = torch.randint(0, 1024, (256,), device='cuda', dtype=torch.int32)
    with pytest.raises(TypeError):
        ops.codebook_gather(idx, cb, 1, 256)
    with pytest.raises(TypeError):
        ops.groupnorm_tables([torch.randn(1, 16, 16, 64, device='cuda')], torch.ones(64, device='cuda', dtype=torch.float16),
                             torch.zeros(64, device='cuda'))
