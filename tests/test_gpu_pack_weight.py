"""ops.pack_weight, layout by layout: the packed buffer is bitwise what a direct call to the C packer writes with the arguments spelled out
here (the power-of-two scale of the split-half layouts included, computed here as 2 ** (15 - frexp(max)[1])), and every PackedWeight field
equals a written-out table."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
G23 = [[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]]
G43 = [[4.0, 0.0, 0.0], [-32 / 15, -16 / 15, -8 / 15], [-32 / 15, 16 / 15, -8 / 15], [1 / 15, 2 / 15, 4 / 15], [1 / 15, -2 / 15, 4 / 15], [0.0, 0.0, 4.0]]


def _scale(wmax):
    return 1.0 if wmax == 0.0 else 2.0 ** (15 - math.frexp(wmax)[1])


def _domain_max(w, G):
    g = torch.tensor(G, dtype=torch.float64, device=w.device)
    return float(torch.einsum('xa,kcab,yb->kcxy', g, w.double(), g).abs().max())


def _wmax(w):
    return float(w.abs().max())


# id: (weight shape, pack_weight keywords, C packer, its arguments between the weight and the buffer as a function of (cout, cin, scale),
#      the maximum the scale is taken from (None: no scale), buffer elements as a function of (cout, cin), buffer dtype,
#      PackedWeight fields (cout_pad, cin_pad, taps, bf16, wino, up2x, s2, conv1))
def _cases():
    from codeformer_amd import ops as O
    c = {}
    for cout in (64, 128):
        s = (cout, 32, 3, 3)
        wino = lambda co, ci, sc: (co, ci, co, ci)                   # noqa: E731
        wino_s = lambda co, ci, sc: (co, ci, co, ci, sc)             # noqa: E731
        f23 = lambda w: _domain_max(w, G23)                          # noqa: E731
        f43 = lambda w: _domain_max(w, G43)                          # noqa: E731
        n16, n36, n9 = (lambda co, ci: 16 * ci * co), (lambda co, ci: 36 * ci * co), (lambda co, ci: 9 * ci * co)
        c[f'f23_fp32_{cout}'] = (s, dict(bf16=O.WINOGRAD), 'cf_pack_conv_weight_winograd', wino, None, n16, F32, (cout, 32, 9, 0, 1, 0, 0, 0))
        c[f'f23_split_{cout}'] = (s, dict(bf16=O.WSPLIT), 'cf_pack_conv_weight_winograd_f16x2', wino_s, f23, n16, F32, (cout, 32, 9, 3, 1, 0, 0, 0))
        c[f'f23_f16_{cout}'] = (s, dict(bf16=O.WF16), 'cf_pack_conv_weight_winograd_f16x2', wino_s, f23, n16, F32, (cout, 32, 9, 2, 1, 0, 0, 0))
        c[f'f23_bf16_{cout}'] = (s, dict(bf16=O.WBF16), 'cf_pack_conv_weight_winograd_bf16', wino_s, f23, n16, F32, (cout, 32, 9, 1, 1, 0, 0, 0))
        c[f'f43_fp32_{cout}'] = (s, dict(bf16=O.WF43F), 'cf_pack_conv_weight_winograd43', wino, None, n36, F32, (cout, 32, 9, 0, 2, 0, 0, 0))
        c[f'f43_split_{cout}'] = (s, dict(bf16=O.WF43), 'cf_pack_conv_weight_winograd43_f16x2', wino_s, f43, n36, F32, (cout, 32, 9, 3, 2, 0, 0, 0))
        c[f'split_{cout}'] = (s, dict(bf16=O.SPLIT), 'cf_pack_conv_weight_f16x2', lambda co, ci, sc: (co, ci, 0, co, ci, sc), _wmax, n9, F32,
                              (cout, 32, 9, 3, 0, 0, 0, 0))
        c[f'split_up2x_{cout}'] = (s, dict(bf16=O.SPLIT, up2x=True), 'cf_pack_conv_weight_f16x2', lambda co, ci, sc: (co, ci, 1, co, ci, sc),
                                   lambda w: 4.0 * _wmax(w), n16, F32, (cout, 32, 9, 3, 0, 1, 0, 0))
        c[f'split_s2_{cout}'] = ((cout, 16, 3, 3), dict(bf16=O.SPLIT, stride2=True), 'cf_pack_conv_weight_f16x2',
                                 lambda co, ci, sc: (co, ci, 2, co, ci, sc), _wmax, n16, F32, (cout, 16, 9, 3, 0, 0, 1, 0))
        c[f'split_1x1_{cout}'] = ((cout, 32, 1, 1), dict(bf16=O.SPLIT), 'cf_pack_conv_weight_f16x2', lambda co, ci, sc: (co, ci, 3, co, ci, sc),
                                  _wmax, lambda co, ci: ci * co, F32, (cout, 32, 1, 3, 0, 0, 0, 1))
        direct = lambda co, ci, sc, cp=cout: (co, ci, 9, cp, ci)       # noqa: E731
        folded = lambda co, ci, sc, cp=cout: (co, ci, cp, ci)          # noqa: E731
        nd, nf = (lambda co, ci, cp=cout: 9 * ci * cp), (lambda co, ci, cp=cout: 16 * ci * cp)
        c[f'plain_3x3_{cout}'] = (s, {}, 'cf_pack_conv_weight', direct, None, nd, F32, (cout, 32, 9, 0, 0, 0, 0, 0))
        c[f'bf16_{cout}'] = (s, dict(bf16=True), 'cf_pack_conv_weight_bf16', direct, None, nd, BF16, (cout, 32, 9, 1, 0, 0, 0, 0))
        c[f'f16_{cout}'] = (s, dict(f16=True), 'cf_pack_conv_weight_f16', direct, None, nd, F16, (cout, 32, 9, 2, 0, 0, 0, 0))
        c[f'up2x_fp32_{cout}'] = (s, dict(up2x=True), 'cf_pack_conv_weight_up2x', folded, None, nf, F32, (cout, 32, 9, 0, 0, 1, 0, 0))
        c[f'up2x_bf16_{cout}'] = (s, dict(bf16=True, up2x=True), 'cf_pack_conv_weight_up2x_bf16', folded, None, nf, BF16, (cout, 32, 9, 1, 0, 1, 0, 0))
        c[f'up2x_f16_{cout}'] = (s, dict(f16=True, up2x=True), 'cf_pack_conv_weight_up2x_f16', folded, None, nf, F16, (cout, 32, 9, 2, 0, 1, 0, 0))
    c['gemm_split_128_to_64'] = ((64, 128), dict(bf16=O.GSPLIT), 'cf_pack_linear_weight_f16x2', lambda co, ci, sc: (co, ci, sc), _wmax,
                                 lambda co, ci: co * ci, F32, (64, 128, 1, 3, 0, 0, 0, 0))
    # the plain layout pads: cout 3 -> 32, 96 -> 128, cin 24 -> 32; 1x1 and Linear weights have one tap
    c['plain_cout3'] = ((3, 32, 3, 3), {}, 'cf_pack_conv_weight', lambda co, ci, sc: (co, ci, 9, 32, 32), None, lambda co, ci: 9 * 32 * 32, F32,
                        (32, 32, 9, 0, 0, 0, 0, 0))
    c['plain_cout96_cin24'] = ((96, 24, 3, 3), {}, 'cf_pack_conv_weight', lambda co, ci, sc: (co, ci, 9, 128, 32), None, lambda co, ci: 9 * 32 * 128,
                               F32, (128, 32, 9, 0, 0, 0, 0, 0))
    c['plain_linear'] = ((64, 128), {}, 'cf_pack_conv_weight', lambda co, ci, sc: (co, ci, 1, 64, 128), None, lambda co, ci: 128 * 64, F32,
                         (64, 128, 1, 0, 0, 0, 0, 0))
    c['f16_cout32'] = ((32, 32, 3, 3), dict(f16=True), 'cf_pack_conv_weight_f16', lambda co, ci, sc: (co, ci, 9, 32, 32), None,
                       lambda co, ci: 9 * 32 * 32, F16, (32, 32, 9, 2, 0, 0, 0, 0))
    c['bf16_cout32'] = ((32, 32, 3, 3), dict(bf16=True), 'cf_pack_conv_weight_bf16', lambda co, ci, sc: (co, ci, 9, 64, 32), None,
                        lambda co, ci: 9 * 32 * 64, BF16, (64, 32, 9, 1, 0, 0, 0, 0))
    return c


CASE_IDS = [f'{k}_{co}' for co in (64, 128) for k in ('f23_fp32', 'f23_split', 'f23_f16', 'f23_bf16', 'f43_fp32', 'f43_split', 'split', 'split_up2x',
                                                       'split_s2', 'split_1x1', 'plain_3x3', 'bf16', 'f16', 'up2x_fp32', 'up2x_bf16', 'up2x_f16')] + \
    ['gemm_split_128_to_64', 'plain_cout3', 'plain_cout96_cin24', 'plain_linear', 'f16_cout32', 'bf16_cout32']


def _check(case, w):
    from codeformer_amd import lib as L, ops as O
    shape, kw, fn, args, maximum, numel, dtype, fields = case
    cout, cin = shape[:2]
    scale = 1.0 if maximum is None else _scale(maximum(w))
    pw = O.pack_weight(w, None, **kw)
    buf = torch.full((numel(cout, cin),), float('nan'), dtype=dtype, device='cuda')
    L.check(getattr(L.load(), fn)(L.ptr(w), *args(cout, cin, scale), L.ptr(buf, dtype=None), L.stream_ptr()), fn)
    torch.cuda.synchronize()
    assert pw.w.dtype == dtype and pw.w.numel() == buf.numel()
    assert torch.equal(pw.w.view(torch.uint8), buf.view(torch.uint8))        # bitwise, whatever the element type
    got = (pw.cout_pad, pw.cin_pad, pw.taps, int(pw.bf16), int(pw.wino), int(pw.up2x), int(pw.s2), int(pw.conv1))
    assert got == fields and (pw.cout, pw.cin) == (cout, cin) and pw.bias is None
    assert pw.scale == scale and (maximum is not None or pw.scale == 1.0)
    return pw


@pytest.mark.parametrize('name', CASE_IDS)
def test_layout_matches_the_c_packer(name):
    cases = _cases()
    assert sorted(cases) == sorted(CASE_IDS)
    g = torch.Generator().manual_seed(20 + CASE_IDS.index(name))
    w = (torch.randn(cases[name][0], generator=g) * 0.05).cuda()
    pw = _check(cases[name], w)
    if cases[name][4] is not None:      # max |w * scale| sits in the top binade below the IEEE-half maximum
        assert 2.0 ** 14 <= cases[name][4](w) * pw.scale < 2.0 ** 15


@pytest.mark.parametrize('name', ['f23_split_64', 'f43_split_64', 'split_64', 'split_up2x_64', 'split_s2_64', 'split_1x1_64', 'gemm_split_128_to_64',
                                  'plain_3x3_64'])
def test_all_zero_weight_has_scale_one(name):
    case = _cases()[name]
    pw = _check(case, torch.zeros(case[0], device='cuda'))
    assert pw.scale == 1.0 and not bool(pw.w.any())


def test_bias_is_a_private_copy():
    from codeformer_amd import ops as O
    w, b = torch.zeros(64, 32, 3, 3, device='cuda'), torch.arange(64, dtype=torch.float32, device='cuda')
    pw = O.pack_weight(w, b)
    assert torch.equal(pw.bias, b) and pw.bias.data_ptr() != b.data_ptr()


def test_refusals():
    from codeformer_amd import ops as O
    z = lambda *s: torch.zeros(*s, device='cuda')       # noqa: E731
    for code in (0, 1, 2):      # stride2 with a non-SPLIT code
        with pytest.raises(ValueError, match='stride2'):
            O.pack_weight(z(64, 32, 3, 3), None, bf16=code, stride2=True)
    with pytest.raises(ValueError, match='stride2'):
        O.pack_weight(z(64, 32, 3, 3), None, bf16=O.SPLIT, up2x=True, stride2=True)
    with pytest.raises(ValueError, match='kernel size'):
        O.pack_weight(z(64, 32, 5, 5), None)
    with pytest.raises(ValueError, match='2-D or 4-D'):
        O.pack_weight(z(64, 32, 3), None)
    for kw in (dict(bf16=True), dict(f16=True), dict(bf16=O.SPLIT)):
        with pytest.raises(ValueError, match='cin % 32'):
            O.pack_weight(z(64, 48, 3, 3), None, **kw)
    with pytest.raises(ValueError, match='cin % 16'):
        O.pack_weight(z(64, 24, 3, 3), None, up2x=True)
    for code in (O.WINOGRAD, O.WSPLIT, O.WF16, O.WBF16, O.WF43, O.WF43F):
        with pytest.raises(ValueError, match='winograd'):
            O.pack_weight(z(64, 32, 3, 3), None, bf16=code, up2x=True)
        with pytest.raises(ValueError, match='winograd'):
            O.pack_weight(z(96, 32, 3, 3), None, bf16=code)
    with pytest.raises(ValueError, match='1x1'):
        O.pack_weight(z(64, 48, 1, 1), None, bf16=O.SPLIT)
    with pytest.raises(ValueError, match='GEMM'):
        O.pack_weight(z(64, 64), None, bf16=O.GSPLIT)
