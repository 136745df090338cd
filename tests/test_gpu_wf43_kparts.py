"""-m gpu: the K-part form of the fp32 Winograd F(4x4,3x3) kernel (ops.WF43K: cf_wf43.hip "KP" + cf_ksum.hip) -- one workgroup per (patch, 128 input
channels, 128 output channels) writes raw partial sums, a second launch adds them in part order from zero and applies bias, epilogue and statistics.

Cases, fp64 reference, loader and gate are those of tools/conv_check.py at five shapes of this form (B, H, W, cin, cout, concat boundary):
  zk1 (2, 16, 16, 256, 128)  2 parts          zk2 (2, 16, 16, 512, 128)  4 parts
  zk3 (1, 32, 32, 256, 256)  2 parts, 2 channel blocks, 4 patches (every patch has image-border and interior-border sides)
  zk4 (2, 16, 16, 256, 128, split at 128)     zk5 (1, 16, 16, 256, 512)  statistics with 16 channels per group
The bound is conv_check.gate for the route w43_16k32 with the code WF43F at split_k = 0: the per-element gate of the whole-K fp32 F(4,3) kernel, c = cin + 19.
The K-part form makes no more roundings on the way of an element than that count: 128 per part in the transform-domain chain and cin / 128 - 1 between
the parts (0 + P0 is exact) against cin in one chain.

The exact case.  F(4,3) has no exact family in general (conv_check: G' holds fifteenths).  Here the weights are +-225 on the CENTRE tap only and only
for one input channel per part, the inputs sparse in {-1, 0, 1}: U = 225 G'[:, 1] G'[:, 1]^T is an integer matrix (|entries| <= 256, rows / columns 0 and 5
zero), V holds multiples of 2^-6 of magnitude <= 3.6, every product is exact, a part's sum has ONE term, and the output is 225 * (+-x): what
remains to be exact are the additions of the output transform, which the test's own fp32 evaluation of A^T M A (conv_check.wino in float32) checks
on the host for the data used before the kernel is asked for the same bits.
"""
import pytest

from _tools import load_script

pytestmark = pytest.mark.gpu

KSHAPES = {'zk1': (2, 16, 16, 256, 128, None, False), 'zk2': (2, 16, 16, 512, 128, None, False), 'zk3': (1, 32, 32, 256, 256, None, False),
           'zk4': (2, 16, 16, 256, 128, 128, False), 'zk5': (1, 16, 16, 256, 512, None, False)}
ROUTE = 'w43_16k32'
# prologue none + bias | affine + bias | affine + swish, residual | LeakyReLU, SFT with a scalar weight | none, residual
FAMILIES = ('mixed_cin_act', 'cancel_pairs', 'swish_leaky_edges', 'swish_leaky_edges_sft', 'dc_plus_ripple')


@pytest.fixture(scope='module')
def cc():
    import torch
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    from codeformer_amd import lib
    lib.load()
    m = load_script('tools/conv_check.py')
    assert not set(KSHAPES) & set(m.SHAPES) and min(KSHAPES) > max(m.SHAPES)      # (appended behind the checker's own keys: their seeds stay)
    m.SHAPES.update(KSHAPES)
    return m


def gate(cc, family, key):
    from codeformer_amd import ops
    return cc.gate(family, key, ROUTE, ops.WF43F, 0)


def launch(cc, d, key, tag, *, x=None, w=None, images=None, stats=False, sft_w=None):
    """One K-part launch of the family's tensors (conv_check.run with statistics, a per-face SFT weight and another weight tensor)."""
    import torch
    from codeformer_amd import ops
    dd = d if w is None else dict(d, w=w)
    pw = cc.packed(dd, ops.WF43K, tag)
    assert pw.kparts == dd['w'].shape[1] // 128 and pw.wino == 2 and not pw.bf16
    sl = slice(None) if images is None else images
    xs = (d['x'] if x is None else x)[sl].contiguous()
    x1, x2, kw = cc.launch_args(xs, d['sc'][sl].contiguous(), d['sh'][sl].contiguous(), d['res'][sl].contiguous(), d['ss'][sl].contiguous(),
                                prologue=d['pro'], epilogue=d['epi'], stats=stats, upsample=False, c_split=cc.SHAPES[key][5])
    if d['epi'] == cc.EPI_SFT:
        kw['sft_w'] = d['sft_w'] if sft_w is None else sft_w
    y = ops.conv2d(x1, pw, x2=x2, **kw)
    assert bool(torch.isfinite(y).all())
    return y


# ---- per element against fp64 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', ('zk1', 'zk2', 'zk3', 'zk4'))
@pytest.mark.parametrize('family', FAMILIES)
def test_family_within_the_gate_of_the_whole_k_kernel(cc, family, key):
    d, ref = cc.prepared(family, key)
    y = cc.run(d, __import__('codeformer_amd').ops.WF43K, 0, (family, key))
    r, err = cc.ratio(y, ref, gate(cc, family, key))
    print(f'{family} {key}: max|d| {err:.3e} = {r:.4f} of the gate')
    assert r <= 1.0, (family, key, r, err)


def test_the_families_cover_the_prologues_and_epilogues(cc):
    got = {(cc.family(f, 'zk1')['pro'], cc.family(f, 'zk1')['epi']) for f in FAMILIES}
    assert {(cc.PRO_NONE, cc.EPI_NONE), (cc.PRO_AFFINE, cc.EPI_NONE), (cc.PRO_AFFINE_SWISH, cc.EPI_RESIDUAL), (cc.PRO_LEAKY, cc.EPI_SFT),
            (cc.PRO_NONE, cc.EPI_RESIDUAL)} <= got
    assert all(float(cc.family(f, 'zk1')['b'].abs().min()) > 0 for f in FAMILIES)       # every case carries a bias


def test_sft_with_one_weight_per_face(cc):
    """Image 0 under the family's own weight 0.7: its gate.  Image 1 under 0.25: the same gate with the SFT terms taken at 0.25, and bitwise the
    scalar launch on that image alone."""
    import torch
    family, key = 'swish_leaky_edges_sft', 'zk1'
    d, ref = cc.prepared(family, key)
    w_img = torch.tensor([d['sft_w'], 0.25], dtype=torch.float32)
    y = launch(cc, d, key, (family, key), sft_w=w_img.cuda())
    g = gate(cc, family, key)
    r0, _ = cc.ratio(y[:1], dict(out=ref['out'][:1]), g[:1])
    r0v, r1v, pre = d['res'].double(), d['ss'].double(), ref['pre']

    def sft_terms(w, out):
        return 2 * cc.U * ((w * r0v * r1v).abs() + 2 * (w * (r0v * r1v + pre)).abs() + out.abs())
    w1 = float(w_img[1])
    out1 = r0v + w1 * (r0v * r1v + pre)
    g1 = g - sft_terms(d['sft_w'], ref['out']) + sft_terms(w1, out1)
    r1, _ = cc.ratio(y[1:], dict(out=out1[1:]), g1[1:])
    print(f'per-face SFT: image 0 {r0:.4f}, image 1 {r1:.4f} of the gate')
    assert r0 <= 1.0 and r1 <= 1.0, (r0, r1)
    alone = launch(cc, d, key, (family, key), images=slice(1, 2), sft_w=w1)
    assert cc.bits_equal(y[1:2], alone), int((y[1:2] != alone).sum())


# ---- statistics --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', ('zk1', 'zk3', 'zk5'))
@pytest.mark.parametrize('family', ('mixed_cout', 'dc_plus_ripple'))
def test_statistics_describe_the_tensor_that_was_written(cc, family, key):
    """One partial per (image, group, 16x16 patch); conv_case.stats_rel_err <= 1e-4 and, through the normal finalize, the GroupNorm rows of the fp64
    statistics of the produced tensor within the bounds of test_gpu_split.py (rstd 1e-5 relative, shift 1e-4)."""
    import torch
    from codeformer_amd import ops
    case = load_script('tools/conv_case.py')
    d, _ = cc.prepared(family, key)
    B, H, W, _, cout = cc.SHAPES[key][:5]
    y = launch(cc, d, key, (family, key), stats=True)
    plain = launch(cc, d, key, (family, key))
    assert cc.bits_equal(y, plain)
    st = y._cf_stats
    assert st.parts == (H // 16) * (W // 16) and st.cpg == cout // 32 and st.part.numel() == B * 32 * st.parts * 2
    err = case.stats_rel_err(y)
    print(f'{family} {key}: statistics rel err {err:.3e}')
    assert err <= 1e-4, (family, key, err)
    sc_, sh_ = ops.groupnorm_tables([y], torch.ones(cout, device='cuda'), torch.zeros(cout, device='cuda'))
    yn = y.double().view(B, -1, 32, cout // 32)
    mean = yn.mean(dim=(1, 3))
    rstd = 1.0 / torch.sqrt(yn.var(dim=(1, 3), unbiased=False) + 1e-6)
    e_sc = float((sc_.double().view(B, 32, -1)[:, :, 0] - rstd).abs().max() / rstd.abs().max())
    e_sh = float((sh_.double().view(B, 32, -1)[:, :, 0] + mean * rstd).abs().max())
    print(f'{family} {key}: rstd rel err {e_sc:.3e}, shift err {e_sh:.3e}')
    assert e_sc <= 1e-5 and e_sh <= 1e-4 * max(1.0, float((mean * rstd).abs().max())), (family, key, e_sc, e_sh)


# ---- part order and isolation ------------------------------------------------------------------------------------------------------------------
def _exact_case(cc, key, last):
    """Sparse inputs in {-1, 0, 1} on ONE channel per part (its first, or with `last` its last), weights +-225 on the centre tap of those channels:
    out[n] = 225 sum_p s[n, p] x[.., c_p], small integers."""
    import torch
    B, H, W, cin, cout = cc.SHAPES[key][:5]
    g = torch.Generator().manual_seed(77 + int(last))
    chans = [128 * p + (127 if last else 0) for p in range(cin // 128)]
    x = torch.zeros(B, H, W, cin)
    w = torch.zeros(cout, cin, 3, 3)
    for c in chans:
        v = torch.randint(-1, 2, (B, H, W), generator=g).float()
        x[..., c] = v * (torch.rand(B, H, W, generator=g) < 0.5)
        w[:, c, 1, 1] = 225.0 * (torch.randint(0, 2, (cout,), generator=g).float() * 2 - 1)
    base = cc.family('mixed_cin_act', key)
    d = dict(base, x=x, w=w, b=torch.zeros(cout), pro=cc.PRO_NONE, epi=cc.EPI_NONE)
    want = torch.einsum('bhwc,nc->bhwn', x.double(), w[:, :, 1, 1].double())
    return d, want


@pytest.mark.parametrize('key,last', [('zk2', False), ('zk2', True), ('zk3', False), ('zk3', True)])
def test_small_integers_give_the_exact_result_bit_for_bit(cc, key, last):
    import torch
    d, want = _exact_case(cc, key, last)
    assert torch.equal(cc.reference(d)['out'], want) and torch.equal(want, want.float().double())
    # the precondition: per part (one channel), the algorithm in float32 on the host is exact, so no addition of it rounds on this data
    for c in [int(i) for i in torch.nonzero(d['w'][0, :, 1, 1]).flatten()]:
        xc, wc = torch.zeros_like(d['x']), torch.zeros_like(d['w'])
        xc[..., c], wc[:, c] = d['x'][..., c], d['w'][:, c]
        y32, _ = cc.wino(xc, wc, 4, dtype=torch.float32)
        assert y32.dtype == torch.float32 and torch.equal(y32.double(), torch.einsum('bhwc,nc->bhwn', xc.double(), wc[:, :, 1, 1].double()))
    y = launch(cc, d, key, ('exact', key, last))
    assert cc.bits_equal(y.cpu() + 0.0, want.float() + 0.0), (key, last, int((y.cpu() != want.float()).sum()), float((y.cpu().double() - want).abs().max()))


@pytest.mark.parametrize('key', ('zk2', 'zk3'))
def test_input_in_one_part_equals_the_layer_with_only_that_parts_weights(cc, key):
    """x zero outside the channels of part p, all weights  ==  all of x, weights zero outside part p: the other parts add exact zeros either way."""
    import torch
    d, _ = cc.prepared('mixed_cin_act', key)
    assert d['pro'] == cc.PRO_NONE
    cin = cc.SHAPES[key][3]
    full = cc.run(d, __import__('codeformer_amd').ops.WF43K, 0, ('mixed_cin_act', key))
    seen = 0
    for p in range(cin // 128):
        keep = torch.zeros(cin, dtype=torch.bool)
        keep[128 * p:128 * p + 128] = True
        xa = d['x'] * keep
        wb = d['w'] * keep[None, :, None, None]
        a = launch(cc, d, key, ('mixed_cin_act', key), x=xa)
        b = launch(cc, d, key, ('isolated', key, p), w=wb)
        assert cc.bits_equal(a + 0.0, b + 0.0), (key, p, int((a != b).sum()))
        assert not cc.bits_equal(a, full)
        seen += 1
    assert seen == cin // 128 >= 2


@pytest.mark.parametrize('key', ('zk2', 'zk3'))
def test_a_one_hot_channel_at_both_ends_of_every_part(cc, key):
    """The input lives in ONE channel, the first or the last of a part: per element against fp64 under the whole-K gate with the chain counted at one
    term (conv_check.coef(live=1): the other channels' products are exact zeros, as in its solo families)."""
    import torch
    from codeformer_amd import ops
    base, _ = cc.prepared('mixed_cin_act', key)
    cin = cc.SHAPES[key][3]
    for c in [128 * p + o for p in range(cin // 128) for o in (0, 127)]:
        keep = torch.zeros(cin)
        keep[c] = 1.0
        d = dict(base, x=base['x'] * keep)
        ref = cc.reference(d)
        p64, _ = cc.prologue64(d)
        S, _ = cc.wino(p64, d['w'], 4, absolute=True)
        tol = cc.coef(ROUTE, ops.WF43F, cin, 0, False, live=1) * cc.U * S + 2 * cc.U * ref['pre'].abs()
        y = launch(cc, d, key, ('mixed_cin_act', key), x=d['x'])
        r, err = cc.ratio(y, ref, tol)
        print(f'one-hot channel {c} {key}: max|d| {err:.3e} = {r:.4f} of the gate')
        assert r <= 1.0, (key, c, r, err)
        assert float((y.double().cpu() - d['b'].double()).abs().max()) > 0.0           # (the channel reached the output)


# ---- batch invariance --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', ('cancel_pairs', 'swish_leaky_edges_sft'))
def test_face_1_of_a_three_face_call_is_bitwise_the_one_face_call(cc, family):
    import torch
    for key in ('zk2', 'zk3'):
        d, _ = cc.prepared(family, key)
        x0 = d['x'][:1]
        first = lambda t: t[:1].expand(3, *t.shape[1:]).contiguous()
        d3 = dict(d, x=torch.cat((torch.roll(x0, 1, dims=2), x0, torch.flip(x0, dims=(1,)))), sc=first(d['sc']), sh=first(d['sh']), res=first(d['res']), ss=first(d['ss']))
        y3 = launch(cc, d3, key, (family, key), stats=True)
        y1 = launch(cc, d3, key, (family, key), images=slice(1, 2), stats=True)
        assert cc.bits_equal(y3[1:2], y1), (family, key, int((y3[1:2] != y1).sum()))
        assert torch.equal(y3._cf_stats.part.view(3, -1)[1:2], y1._cf_stats.part.view(1, -1))
        assert not cc.bits_equal(y3[0:1], y1)


# ---- dispatch ----------------------------------------------------------------------------------------------------------------------------------
def test_the_request_code_selects_the_form_exactly_on_its_rule():
    from codeformer_amd import ops
    n_k = 0
    for cin in (64, 128, 192, 256, 320, 384, 512, 640, 1024):
        for cout in (64, 128, 192, 256, 512):
            for (h, w) in ((8, 16), (16, 16), (16, 32), (24, 24), (32, 32), (32, 48), (48, 48), (64, 64), (128, 128)):
                for c_split in (None, 64, 128, 160, 256):
                    if c_split is not None and c_split >= cin:
                        continue
                    for up2x in (False, True):
                        for plain in (True, False):
                            rule = (cout % 128 == 0 and cin % 128 == 0 and 256 <= cin <= 512 and h % 16 == 0 and w % 16 == 0 and 256 <= h * w < 64 * 64
                                    and plain and not up2x and (c_split is None or c_split % 128 == 0)
                                    and (h // 16) * (w // 16) * (cin // 128) * (cout // 128) >= 16)      # (the measured narrowing: ops.f43k_ok)
                            got = ops.conv_code(ops.WINOGRAD_F43K, cin, cout, h, w, up2x=up2x, c_split=c_split, plain=plain)
                            want = ops.WF43K if rule else ops.conv_code(ops.WINOGRAD_F43, cin, cout, h, w, up2x=up2x, c_split=c_split, plain=plain)
                            assert got == want, (cin, cout, h, w, c_split, up2x, plain, got, want)
                            n_k += rule
                            assert ops.conv_code(ops.WINOGRAD_F43, cin, cout, h, w, up2x=up2x, c_split=c_split, plain=plain) != ops.WF43K
    assert n_k > 20
    # the layer classes of the network: 512 -> 512 @ 16x16, 256 -> 256 and 512 -> 256 @ 32x32 measured shorter and are adopted; 256 -> 512 and
    # 512 -> 256 @ 16x16 (8 workgroups per image) did not and stay on F(2,3)
    for cin, cout, h in ((512, 512, 16), (256, 256, 32), (512, 256, 32)):
        assert ops.conv_code(ops.WINOGRAD_F43K, cin, cout, h, h) == ops.WF43K
    for cin, cout, h in ((256, 512, 16), (512, 256, 16)):
        assert ops.conv_code(ops.WINOGRAD_F43K, cin, cout, h, h) == ops.WINOGRAD and ops.f43k_covers(cin, cout, h, h)
    assert ops.conv_code(ops.WINOGRAD_F43K, 512, 256, 32, 32, c_split=256) == ops.WF43K
    assert ops.conv_code(ops.WINOGRAD_F43K, 256, 256, 64, 64) == ops.WF43F and ops.conv_code(ops.WINOGRAD_F43K, 128, 128, 32, 32) == ops.WINOGRAD
    assert ops.WINOGRAD_F43K in ops.F43_FP32_CODES and ops.exact_code(ops.WINOGRAD_F43K) == ops.WINOGRAD_F43K


def test_a_k_part_weight_refuses_the_launches_the_form_does_not_cover(cc):
    import torch
    from codeformer_amd import ops
    w = torch.randn(128, 256, 3, 3).cuda() * 0.02
    pw = ops.pack_weight(w, None, bf16=ops.WF43K)
    assert pw.kparts == 2
    for shape in ((1, 64, 64, 256), (1, 8, 16, 256), (1, 24, 24, 256)):
        with pytest.raises(ValueError):
            ops.conv2d(torch.zeros(*shape, device='cuda'), pw)
    with pytest.raises(ValueError):
        ops.conv2d(torch.zeros(1, 16, 16, 64, device='cuda'), pw, x2=torch.zeros(1, 16, 16, 192, device='cuda'))      # a concat boundary inside a part
    for cout, cin in ((128, 128), (64, 256), (128, 640)):
        with pytest.raises(ValueError):
            ops.pack_weight(torch.zeros(cout, cin, 3, 3).cuda(), None, bf16=ops.WF43K)
