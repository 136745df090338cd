"""-m gpu: the per-image weight of the SFT epilogue (cf_conv2d_sft_w; ops.conv2d(sft_w=<float32 tensor of B values>)), kernel level.

Every kernel family forms the weight of image b by one expression -- w_img ? w_img[b] : sft_w -- in front of the same epilogue arithmetic, so
for every route that accepts EPI_SFT, bit for bit, on the output AND on the GroupNorm partials the epilogue writes:
  * the per-image launch equals the concatenation of single-image scalar launches with sft_w = w_b;
  * a per-image launch whose values are all equal equals the scalar batched launch.
Routes: those of tools/conv_check.py (d32, dsplit, w23_f32 and w23_h4 with their split-K forms, w23_h8 in its three operand types, w43_8,
w43_16k32, w43_16k16), the direct kernel on bf16 / IEEE-half operands, and the two bf16-STORAGE forms that take SFT (eight-wave Winograd and
the direct 64-channel kernel on bf16 tensors).  Shapes: conv_check's multi-image ones (b, c with its concatenated input, d), a three-image
16x16 one with 256 -> 128 channels (split-K counts 1 and 2: the last ticket's epilogue), and the one-face and two-face 32x32 256-channel SFT
layer of the network at the split count the host picks.  Operands: conv_check's exact integer-coded SFT variant and swish_leaky_edges_sft
(LeakyReLU prologue, range scale, epilogue operands 2^10 larger than the convolution).  Nothing here compares against a reference value:
what these launches compute is the subject of tests/test_gpu_conv_families.py."""
import pytest

from _tools import load_script

pytestmark = pytest.mark.gpu

WEIGHTS = {'int_coded': (0.5, 1.0, 0.125), 'swish_leaky_edges_sft': (0.7, 0.3, 1.0)}     # distinct per image; the first set keeps int_coded exact
VARIANT = {'int_coded': 2, 'swish_leaky_edges_sft': 0}                                    # int_coded: (affine prologue, SFT epilogue)
# key -> (B, H, W, cin, cout, c_split); b, c, d are conv_check.SHAPES' own
NEW_SHAPES = {'x3': (3, 16, 16, 256, 128, None), 'sft32_1': (1, 32, 32, 256, 256, None), 'sft32_2': (2, 32, 32, 256, 256, None)}
BF16_IO = {'wbf16_io': ((2, 64, 64, 128, 128, None), 'WBF16'), 'direct_bf16_io': ((2, 16, 32, 32, 64, None), 'BF16')}


@pytest.fixture(scope='module')
def env():
    import torch
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    from codeformer_amd import lib, ops
    lib.load()
    cc = load_script('tools/conv_check.py')
    assert cc.ROUTES == ('d32', 'dsplit', 'w23_f32', 'w23_h4', 'w23_h8', 'w43_8', 'w43_16k32', 'w43_16k16', 'w43_up')
    return ops, cc, {}


def _geom(cc, key):
    return cc.SHAPES[key][:6] if key in cc.SHAPES else NEW_SHAPES[key] if key in NEW_SHAPES else BF16_IO[key][0]


def _family(cc, name, key):
    if key in cc.SHAPES:
        return cc.family(name, key, VARIANT[name])
    B, H, W, cin, cout, _ = _geom(cc, key)
    return cc.family_at(name, (B, H, W, cin, cout, False), 7000 + 13 * sorted(list(NEW_SHAPES) + list(BF16_IO)).index(key), VARIANT[name])


def _launches(ops, cc, key):
    """[(label, pack code, split_k)]; split_k None: the host picks."""
    B, H, W, cin, cout, cs = _geom(cc, key)
    if key in BF16_IO:
        return [(BF16_IO[key][1], {'WBF16': ops.WBF16, 'BF16': 1}[BF16_IO[key][1]], 0)]
    rows = []
    for name, code in cc.CODES.items():
        sks = [0]
        if key.startswith('sft32'):
            sks = [None]
        elif code in (ops.WINOGRAD, ops.WSPLIT) and H * W <= 256 and cin % 128 == 0:
            sks += [n for n in (1, 2, 4) if (cin // 128) % n == 0]
        for sk in sks:
            r = cc.route_of(code, H, W, cin, cout, False, sk or 0, cs)
            if r is not None:
                rows.append((f'{r[0]}/{name}/{r[1]}' + (f'/sk{sk}' if sk else ''), code, sk))
    c0 = cin if cs is None else cs
    if cin % 32 == 0 and c0 % 32 == 0 and cout % 64 == 0:            # the direct kernel on single 16-bit operands (conv_validate's rule)
        rows += [('direct/BF16', 1, 0), ('direct/F16', 2, 0)]
    return rows


def _run(env, d, name, key, code, split_k, images, sft_w, io_bf16):
    import torch
    ops, cc, packs = env
    cs = _geom(cc, key)[5]
    pk = (name, key, code)      # (one packed weight per family, shape and code)
    if pk not in packs:
        packs[pk] = ops.pack_weight(d['w'].cuda(), d['b'].cuda(), bf16=code)
    sl = images
    x1, x2, kw = cc.launch_args(d['x'][sl].contiguous(), d['sc'][sl].contiguous(), d['sh'][sl].contiguous(), d['res'][sl].contiguous(),
                                d['ss'][sl].contiguous(), prologue=d['pro'], epilogue=d['epi'], stats=True, c_split=cs)
    kw['sft_w'] = sft_w
    if d['pro'] in (ops.PRO_NONE, ops.PRO_LEAKY):
        kw['act'] = ops.act_scale(x1, x2)
    if split_k is not None:
        kw['split_k'] = split_k
    if io_bf16:
        x1 = x1.to(torch.bfloat16)
        kw['res'], kw['sft_scale'] = kw['res'].to(torch.bfloat16), kw['sft_scale'].to(torch.bfloat16)
    y = ops.conv2d(x1, packs[pk], x2=x2, **kw)
    return y, y._cf_stats.part


def _bits(t):
    import torch
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int64 if t.dtype == torch.float64 else torch.int32)


@pytest.mark.parametrize('name', sorted(WEIGHTS))
@pytest.mark.parametrize('key', ['b', 'c', 'd', 'x3', 'sft32_1', 'sft32_2', 'wbf16_io', 'direct_bf16_io'])
def test_per_image_weight_is_the_scalar_launch_per_image(env, key, name):
    import torch
    ops, cc, _ = env
    d = _family(cc, name, key)
    assert d['epi'] == ops.EPI_SFT
    B = d['x'].shape[0]
    ws = WEIGHTS[name][:B]
    w_dev = torch.tensor(ws, dtype=torch.float32).cuda()
    rows = _launches(ops, cc, key)
    routes = {r[0].split('/')[0] for r in rows}
    if key in ('b', 'c', 'd', 'x3'):
        assert {'d32', 'w23_f32'} <= routes and routes & {'w23_h4', 'w23_h8'} and routes & {'w43_8', 'w43_16k32', 'w43_16k16'}, routes
    for label, code, sk in rows:
        y, part = _run(env, d, name, key, code, sk, slice(None), w_dev, key in BF16_IO)
        assert y.shape[0] == B and part.numel() % B == 0
        for b in range(B):
            y1, p1 = _run(env, d, name, key, code, sk, slice(b, b + 1), float(ws[b]), key in BF16_IO)
            assert torch.equal(_bits(y[b:b + 1]), _bits(y1)), (label, key, name, b, float((y[b:b + 1].float() - y1.float()).abs().max()))
            assert torch.equal(_bits(part.view(B, -1)[b]), _bits(p1.view(-1))), (label, key, name, b, 'statistics partials')
        same = torch.full((B,), ws[0], dtype=torch.float32).cuda()
        ye, pe = _run(env, d, name, key, code, sk, slice(None), same, key in BF16_IO)
        ys, ps = _run(env, d, name, key, code, sk, slice(None), float(ws[0]), key in BF16_IO)
        assert torch.equal(_bits(ye), _bits(ys)) and torch.equal(_bits(pe), _bits(ps)), (label, key, name, 'equal values against the scalar batched launch')
        if B > 1:
            assert not torch.equal(_bits(y[1:]), _bits(ys[1:])), (label, key, name, 'the weights of images 1.. were not read')
    print(f'{key} {name}: {len(rows)} launches bitwise: {[r[0] for r in rows]}')


def test_routes_cover_every_sft_kernel_family(env):
    """The union of the routes the cases above reach: every route of conv_check that accepts EPI_SFT, and the split-K forms."""
    ops, cc, _ = env
    seen = set()
    for key in ('b', 'c', 'd', 'x3', 'sft32_1', 'sft32_2'):
        seen |= {r[0].split('/')[0] for r in _launches(ops, cc, key)}
        seen |= {'split-K' for r in _launches(ops, cc, key) if r[2]}
    assert seen >= {'d32', 'dsplit', 'w23_f32', 'w23_h4', 'w23_h8', 'w43_8', 'w43_16k32', 'w43_16k16', 'direct', 'split-K'}, seen
