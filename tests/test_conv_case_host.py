"""CPU: tools/conv_case.py, the case builder of the conv checkers (split_check.py, wino_check.py, f43_check.py), and tests/_tools.py.

  * draw() is the sequence of generator calls the checkers made before they shared it, written out here as the specification: every
    recorded checker result and every gate of the GPU tests was taken on those bits;
  * reference() is the convolution: against an evaluation that shares no operation with it (unfold of the zero-padded, prologue-applied
    input, one einsum, the epilogue written out), to 1e-12 * max|ref| -- fp64 round-off of about 300 products, not a kernel tolerance;
  * launch_args() hands conv2d exactly the tensors its options read;
  * stats_rel_err() is ~0 for partials that are exact splits of the true sums and reports a 1% offset as 1e-2;
  * load_script() returns a fresh module on every call.
"""
import types

import pytest
import torch

from _tools import load_script
from codeformer_amd import ops

CASES = [dict(B=1, H=16, W=16, cin=32, cout=64),
         dict(B=1, H=16, W=16, cin=32, cout=64, upsample=True, seed=1),
         dict(B=1, H=16, W=16, cin=32, cout=64, wscale=300.0, seed=2),
         dict(B=1, H=16, W=16, cin=32, cout=64, wscale=1e-4, xscale=30.0, seed=3),
         dict(B=3, H=8, W=16, cin=32, cout=64, seed=4)]
PROLOGUES = (ops.PRO_NONE, ops.PRO_LEAKY, ops.PRO_AFFINE, ops.PRO_AFFINE_SWISH)
EPILOGUES = (ops.EPI_NONE, ops.EPI_RESIDUAL, ops.EPI_SFT)


@pytest.fixture(scope='module')
def cc():
    return load_script('tools/conv_case.py')


def _legacy_draw(B, H, W, cin, cout, upsample=False, seed=0, wscale=1.0, xscale=1.0):
    """The body of split_check.case before conv_case existed."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, cin, generator=g) * xscale
    w = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5 * wscale
    b = torch.randn(cout, generator=g) * 0.1
    sc = torch.rand(B, cin, generator=g) + 0.5
    sh = torch.randn(B, cin, generator=g) * 0.1
    Ho, Wo = (2 * H, 2 * W) if upsample else (H, W)
    res = torch.randn(B, Ho, Wo, cout, generator=g)
    ss = torch.randn(B, Ho, Wo, cout, generator=g) * 0.3
    return x, w, b, sc, sh, res, ss


@pytest.mark.parametrize('c', CASES, ids=lambda c: '-'.join(f'{k}{v}' for k, v in c.items()))
def test_draw_is_the_sequence_the_checkers_drew(cc, c):
    got, want = cc.draw(**c), _legacy_draw(**c)
    assert len(got) == len(want) == 7
    for name, a, e in zip(('x', 'w', 'b', 'sc', 'sh', 'res', 'ss'), got, want):
        assert a.dtype == torch.float32 and a.shape == e.shape and torch.equal(a, e), name
    if 'wscale' not in c:       # wino_check had no scales: a factor of 1.0 leaves its bits alone
        g = torch.Generator().manual_seed(c.get('seed', 0))
        x = torch.randn(c['B'], c['H'], c['W'], c['cin'], generator=g)
        w = torch.randn(c['cout'], c['cin'], 3, 3, generator=g) * (2.0 / (9 * c['cin'])) ** 0.5
        assert torch.equal(got[0], x) and torch.equal(got[1], w)


def _independent(x, w, b, sc, sh, res, ss, prologue, epilogue, upsample):
    v = x.double()
    if prologue in (ops.PRO_AFFINE, ops.PRO_AFFINE_SWISH):
        v = v * sc.double()[:, None, None, :] + sh.double()[:, None, None, :]
        if prologue == ops.PRO_AFFINE_SWISH:
            v = v / (1.0 + torch.exp(-v))
    elif prologue == ops.PRO_LEAKY:
        v = torch.where(v >= 0, v, 0.2 * v)
    if upsample:
        v = v.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    B, H, W, C = v.shape
    p = torch.zeros(B, H + 2, W + 2, C, dtype=torch.float64)
    p[:, 1:-1, 1:-1] = v
    patches = p.unfold(1, 3, 1).unfold(2, 3, 1)                    # (B, H, W, C, 3, 3)
    y = torch.einsum('bhwcij,ocij->bhwo', patches, w.double()) + b.double()
    if epilogue == ops.EPI_RESIDUAL:
        y = y + res.double()
    elif epilogue == ops.EPI_SFT:
        y = res.double() * (1.0 + 0.7 * ss.double()) + 0.7 * y
    return y


@pytest.mark.parametrize('c', CASES, ids=lambda c: '-'.join(f'{k}{v}' for k, v in c.items()))
def test_reference_is_the_convolution(cc, c):
    x, w, b, sc, sh, res, ss = cc.draw(**c)
    up = c.get('upsample', False)
    for prologue in PROLOGUES:
        for epilogue in EPILOGUES:
            ref = cc.reference(x, w, b, prologue=prologue, epilogue=epilogue, sc=sc, sh=sh, res=res, ss=ss, upsample=up)
            want = _independent(x, w, b, sc, sh, res, ss, prologue, epilogue, up)
            assert ref.dtype == torch.float64 and ref.shape == res.shape
            err, top = float((ref - want).abs().max()), float(ref.abs().max())
            assert err <= 1e-12 * top, (prologue, epilogue, err, top)


def test_reference_reads_only_what_the_options_name(cc):
    x, w, b, sc, sh, res, ss = cc.draw(**CASES[0])
    plain = cc.reference(x, w, b, prologue=ops.PRO_NONE, epilogue=ops.EPI_NONE)
    assert torch.equal(plain, cc.reference(x, w, b, prologue=ops.PRO_NONE, epilogue=ops.EPI_NONE, sc=sc, sh=sh, res=res, ss=ss))
    sft = cc.reference(x, w, b, prologue=ops.PRO_NONE, epilogue=ops.EPI_SFT, res=res, ss=ss, sft_w=0.25)
    assert float((sft - (res.double() + 0.25 * (res.double() * ss.double() + plain))).abs().max()) == 0.0


@pytest.mark.parametrize('c_split', (None, 16))
def test_launch_args_hold_what_the_options_read(cc, c_split):
    x, w, b, sc, sh, res, ss = cc.draw(**CASES[4])
    for prologue in PROLOGUES:
        for epilogue in EPILOGUES:
            for stats in (False, True):
                x1, x2, kw = cc.launch_args(x, sc, sh, res, ss, prologue=prologue, epilogue=epilogue, stats=stats, c_split=c_split,
                                            device='cpu')
                assert kw['prologue'] == prologue and kw['epilogue'] == epilogue and kw['emit_stats'] is stats and kw['upsample'] is False
                affine = prologue in (ops.PRO_AFFINE, ops.PRO_AFFINE_SWISH)
                assert ('scale' in kw) == ('shift' in kw) == affine
                assert ('res' in kw) == (epilogue != ops.EPI_NONE)
                assert ('sft_scale' in kw) == ('sft_w' in kw) == (epilogue == ops.EPI_SFT)
                assert set(kw) <= {'prologue', 'epilogue', 'emit_stats', 'upsample', 'scale', 'shift', 'res', 'sft_scale', 'sft_w'}
                if affine:
                    assert torch.equal(kw['scale'], sc) and torch.equal(kw['shift'], sh)
                if epilogue != ops.EPI_NONE:
                    assert torch.equal(kw['res'], res)
                if epilogue == ops.EPI_SFT:
                    assert torch.equal(kw['sft_scale'], ss) and kw['sft_w'] == 0.7
                assert (x2 is None) == (c_split is None)
                if c_split is None:
                    assert torch.equal(x1, x)
                else:
                    assert x1.shape[-1] == c_split and x1.is_contiguous() and x2.is_contiguous() and torch.equal(torch.cat([x1, x2], -1), x)
    assert cc.launch_args(x, sc, sh, res, ss, prologue=ops.PRO_NONE, epilogue=ops.EPI_NONE, stats=False, upsample=True, device='cpu')[2]['upsample'] is True


def test_stats_rel_err_on_a_stand_in(cc):
    B, H, W, C, parts = 2, 8, 12, 64, 4         # cpg 2; the pixels fall into four partials of 24
    g = torch.Generator().manual_seed(5)
    y = torch.randn(B, H, W, C, generator=g) + 1.0      # (the offset keeps every group's sum away from zero)
    r = y.double().view(B, parts, H * W // parts, 32, C // 32)
    part = torch.stack([r.sum((2, 4)), (r * r).sum((2, 4))], -1).permute(0, 2, 1, 3).contiguous()      # (B, 32, parts, 2)
    y._cf_stats = types.SimpleNamespace(part=part.clone().view(-1), parts=parts, cpg=C // 32)
    assert cc.stats_rel_err(y) < 1e-12
    total = part.sum(2)
    for which in (0, 1):        # the sum, the sum of squares: one partial off by 1% of its group's total
        bad = part.clone()
        bad[1, 7, 2, which] += 0.01 * total[1, 7, which]
        y._cf_stats = types.SimpleNamespace(part=bad.view(-1), parts=parts, cpg=C // 32)
        assert cc.stats_rel_err(y) == pytest.approx(1e-2, rel=1e-6)


def test_load_script_returns_a_fresh_module_each_call():
    import sys
    a, b = load_script('tools/conv_case.py'), load_script('tools/conv_case.py')
    assert a is not b and a.draw is not b.draw and a.__name__ == 'conv_case'
    assert sys.modules.get('conv_case') not in (a, b)
