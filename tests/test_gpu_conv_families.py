"""-m gpu: the 3x3 stride-1 convolution kernels per element on exact, impulse and mixed-scale inputs.

The families, the fp64 reference, the routes, the per-element gate with its derivation and the CPU emulation live in tools/conv_check.py;
tests/test_conv_families_host.py proves on the CPU that the emulation stays within 0.5 of the gate and that the exactness preconditions hold, so every
condition here is a condition on the reference.  Weights are packed with the explicit code; conv_check.routes() says which code and shape reaches
which kernel form (d32, dsplit, w23_f32, w23_h4, w23_h8, w43_8, w43_16k32, w43_16k16, w43_up, w42_up), and the union of the cases below reaches all ten.
Nothing is larger than 48x48 pixels, batch 3 or 512 channels.

Measured on an MI355X, the whole file 16.9 s (125 cases; the slowest 1.2 s: tap_shift at zu1, nine taps on four routes, then 0.9 s: solo_cin_act on dsplit) against 13.0 s
of the 109 cases before the w42_up route and its shapes zu1 / zu2, in the same session: 3.9 s for all that the sub-pixel form adds.  Largest |error| / gate per family
and route, kernel | CPU emulation (test_family_within_the_gate prints every single ratio; onehot_pixels: the kernel's, d32 being the folded form):
                          d32             dsplit          w23_f32         w23_h4          w23_h8          w43_8           w43_16k32       w43_16k16       w43_up          w42_up
    mixed_cout            0.0301 | 0.0246 0.1806 | 0.2101 0.0094 | 0.0101 0.1301 | 0.1301 0.0795 | 0.0795 0.1338 | 0.1338 0.0728 | 0.0728 0.0751 | 0.0751 0.0058 | 0.0064 0.0066 | 0.0068
    mixed_cin             0.0573 | 0.0174 0.0056 | 0.0038 0.0181 | 0.0176 0.0112 | 0.0109 0.0852 | 0.0852 0.0119 | 0.0115 0.0043 | 0.0038 0.0084 | 0.0088 -               -
    mixed_cin_act         0.0656 | 0.0169 0.0061 | 0.0047 0.0172 | 0.0167 0.0128 | 0.0097 0.0884 | 0.0884 0.0111 | 0.0102 0.0038 | 0.0033 0.0061 | 0.0057 0.0075 | 0.0079 0.0116 | 0.0098
    cancel_pairs          0.0021 | 0.0044 0.0011 | 0.0009 0.0037 | 0.0039 0.0033 | 0.0034 0.0223 | 0.0223 0.0024 | 0.0030 0.0006 | 0.0005 0.0011 | 0.0011 0.0012 | 0.0014 0.0021 | 0.0021
    dc_plus_ripple        0.0109 | 0.0097 0.0015 | 0.0018 0.0043 | 0.0031 0.0015 | 0.0019 0.0082 | 0.0082 0.0022 | 0.0020 0.0011 | 0.0011 0.0013 | 0.0013 0.0017 | 0.0016 0.0021 | 0.0018
    swish_leaky_edges     0.4295 | 0.4295 0.2952 | 0.2952 0.3366 | 0.3366 0.2981 | 0.2981 0.2063 | 0.2063 0.2390 | 0.2390 0.1767 | 0.1767 0.2089 | 0.2089 -               -
    swish_leaky_edges_sft 0.2921 | 0.4235 0.2462 | 0.4148 0.2887 | 0.4238 0.2414 | 0.4038 0.2459 | 0.4160 0.2415 | 0.4018 0.2445 | 0.4108 0.2460 | 0.4119 -               -
    solo_cin              0.3338 | 0.3738 0.4544 | 0.4544 0.1214 | 0.1409 0.3117 | 0.3117 0.2653 | 0.2653 0.2746 | 0.2746 0.2612 | 0.2612 0.2693 | 0.2694 -               -
    solo_cin_act          0.4258 | 0.4258 0.4991 | 0.4990 0.1463 | 0.1352 0.2570 | 0.2570 0.2906 | 0.2906 0.2696 | 0.2696 0.2474 | 0.2474 0.2545 | 0.2545 0.0378 | 0.0406 0.0623 | 0.0803
    onehot_pixels         0.4026          0.3964          0.4667          0.4278          0.4920          0.3518          0.3503          0.2761          0.4161          0.4039
(equal pairs: the worst element is one whose error is a single rounding both evaluations make alike -- the residual add of swish_leaky_edges, the half
rounding of a small channel's U in mixed_cout, the half rounding of a subnormal activation half in the solo families, whose gate enters it at the whole
spacing; the w23_h8 column is its bf16 form, whose gate is the operand format's 2^-8.  The swish / leaky families sit at
the epilogue's own rounding by construction: their operands are 2^10 larger than the convolution.  The SFT epilogue is an FMA chain in the kernels.
Read the equal cells as what they are: they exercise the epilogue add (swish_leaky_edges, whole row) or the host-side packer's half rounding (the Winograd
columns of mixed_cout), NOT the MFMA accumulation, and meet the >= 1e-3 condition trivially; the evidence on the accumulation path is in the cells that differ,
in int_coded, tap_shift and onehot_pixels.)
The kernels needed no change: every exact, impulse, gate, bitwise and containment condition held on the first run.
The w42_up column (ops.WF42U at u1, zu1, zu2: 1, 3 and 8 slabs; per shape, kernel | emulation: mixed_cout 0.0066 | 0.0068, 0.0037 | 0.0037, 0.0011 | 0.0008;
mixed_cin_act 0.0116 | 0.0098, 0.0033 | 0.0033, 0.0008 | 0.0007; cancel_pairs 0.0021 | 0.0021, 0.0005 | 0.0005, 0.0001 | 0.0001; dc_plus_ripple 0.0021 | 0.0018,
0.0008 | 0.0010, 0.0004 | 0.0002; solo_cin_act 0.0623 | 0.0605, 0.0615 | 0.0803, 0.0581 | 0.0505; onehot_pixels 0.2375, 0.4039, 0.2113) was measured when the route was added:
the kernel stands where the float32 emulation of its own pipeline stands at every shape, and needed no change either.  Its dense cells are small because
c = cin + 15 counts a whole u S per channel of the chain; what holds the form to its arithmetic are the one-term sums (solo_cin_act, onehot_pixels, tap_shift)
and the two edits of the emulation that tests/test_conv_families_host.py shows at 2 x 10^5 .. 5 x 10^7 times the gate of the family that sees each best (cancel_pairs at cin 256 sees them at 2 times its gate only).  The older columns changed where zu1 / zu2
now reach them too (solo_cin_act on dsplit and w43_up, onehot_pixels on d32 and w43_up).

Scratch builds with one in-range edit each (not committed; addresses, barriers and launch geometry untouched), tests of this file that fail | of the
eight 3x3 tests of test_gpu_split.py that were run against each build (split_conv_against_fp64, split_conv_is_bitwise.., splitk_winograd.., winograd_single.., the four winograd_f43..):
  (e1) cf_split.hip: the lo hi MFMA left out                           7: tap_shift b / c / u1, the dsplit gates of mixed_cout, mixed_cin, mixed_cin_act, dc_plus_ripple
                                                                        | 1 (split_conv_against_fp64)
  (e2) cf_wf43.hip packer: lo half zeroed for positions 30..35         23: onehot_pixels on five shapes, tap_shift b / c / d, 15 F(4,3) gates of all seven families
                                                                        | 2 (winograd_f43_forms_against_fp64, winograd_f43_with_512_input_channels)
  (e3) cf_wsplit.hip: acc_scale applied after the bias                 10: int_coded c / d, onehot_pixels c / d, six w23_h8 gates | 3 (split_conv_against_fp64,
                                                                        split_conv_is_bitwise.., winograd_single_16bit_operands)
  (e4) cf_winograd.hip: gather pad test off by one, right border only   29: int_coded on the seven plain shapes, onehot_pixels on five, tap_shift b / c / d, every w23_f32 and
         (`ix < w - 1`: the last image column read as padding)           w23_h4 gate | 3 (split_conv_against_fp64, split_conv_is_bitwise.., splitk_winograd..)
  (e5) cf_wf43.hip packer: subnormal lo halves flushed to zero          2: mixed_cout on w43_8 and w43_16k16 | 0
  (e6) cf_split.hip gather: padding made by v * 0 instead of a select   3: the containment test on b, c, u1 (a NaN at the first image's pixel (0, 0) reaches every padded tile) | 0
         (with the (0, 0) pixel in the LAST image, as this test first had it, the edit passed everything: a clamped load reads the tensor's first pixel)
  (e7) cf_winograd.hip split halves: lo half of V dropped for nu = 3    6: tap_shift b, the w23_h4 gates of mixed_cout, mixed_cin, mixed_cin_act, dc_plus_ripple, swish_leaky_edges
                                                                        | 1 (split_conv_against_fp64)
  (e8) cf_winograd.hip packer: subnormal lo halves flushed to zero      2: mixed_cout on w23_h4 and w23_h8 | 0
  (e9) cf_split.hip packer: subnormal lo halves flushed to zero         1: mixed_cout on dsplit | 0
  (e10) cf_winograd.hip split-K: chunk sums parked in reverse order     2: every_split_count_gives_the_same_bits on both families; every accuracy case passes | 1 (splitk_winograd..)
  (e11) cf_winograd.hip split halves: the lo hi MFMA left out           7: tap_shift b, the w23_h4 gates of six families | 1 (split_conv_against_fp64)
Plainly: of eleven edits, four are caught by this file and by none of the old tests (e5, e6, e8, e9: subnormal lo halves flushed in each of the three packers, padding that lets a NaN through), errors confined to elements that are
small next to the tensor's largest, or to non-finite inputs -- the gap the per-element gates were built for.  The seven gross edits (a product or an operand half left out, a wrong
border, a misplaced scale, another chunk order) are caught by the old whole-tensor bounds as well; there this file adds only the localisation (which
route, which family, which tap).
The solo families (one input channel per output channel, channel scales over 32 binades; conv_check) were added for the edit the older families cannot
see: the lo half of an activation zeroed where it is a subnormal half, |a| < 2^-3 under the range scale.  In every dense family a small input channel
hides behind the large ones of the same sum -- tests/test_conv_families_host.py pins that on the CPU emulation (no older family's ratio at shape b moves
by 0.005 of its gate; the solo families' rises to 25 .. 103 times theirs).  Four scratch builds with exactly that edit, one kernel each, all four built
and run once; tests of this file that fail | of the eight 3x3 tests of test_gpu_split.py:
  (s1) cf_split.hip split2 (the gather's split)                         5: the dsplit gates of solo_cin and solo_cin_act, tap_shift b / c / u1 | 1 (split_conv_against_fp64)
         (in test_gpu_conv_geom.py: 11 -- the three solo gates of s2_dsplit / c1_dsplit, tap_shift on the seven split-half cases, mixed_cout on c1_dsplit)
  (s2) cf_winograd.hip, the V split of the split-half form              2: the w23_h4 gates of solo_cin and solo_cin_act | 1 (split_conv_against_fp64)
  (s3) cf_wsplit.hip, the V split                                       2: the w23_h8 gates of solo_cin and solo_cin_act | 2 (split_conv_against_fp64, split_conv_is_bitwise..)
  (s4) cf_wf43.hip, the V split (the edit once "tried on paper")        6: the w43_8, w43_16k32 and w43_16k16 gates of solo_cin and solo_cin_act
                                                                        | 2 (winograd_f43_forms_against_fp64, winograd_f43_with_512_input_channels)
Plainly: every one of the four is now caught here, by the solo gates on exactly the route that was edited, and on the three Winograd kernels by nothing
else in this file -- none of the seven older gate families, int_coded, onehot_pixels or (s2 - s4) tap_shift moves.  The old whole-tensor tests catch
each of the four as well: most of their cases put O(1) values behind an affine or swish prologue, with no range scale, so a large share of ALL their operands lies below 2^-3
and the edit is a gross one there (the split kernels' error is also held to 5x the fp32 kernels').  What they cannot see, and the solo gates can, is the same loss confined to the channels that are small next to the
image's largest under a range scale (the host test's figures): there this file is the only check.
"""
import pytest

from _tools import load_script

pytestmark = pytest.mark.gpu

ROUTES = ('d32', 'dsplit', 'w23_f32', 'w23_h4', 'w23_h8', 'w43_8', 'w43_16k32', 'w43_16k16', 'w43_up', 'w42_up')
UP_ROUTES = ('w43_up', 'w42_up')                  # prologue none, no epilogue operand, one input
GATE_FAMILIES = ('mixed_cout', 'mixed_cin', 'mixed_cin_act', 'cancel_pairs', 'dc_plus_ripple', 'swish_leaky_edges', 'swish_leaky_edges_sft')
SOLO_FAMILIES = ('solo_cin', 'solo_cin_act')      # one input channel per output channel, under conv_check's solo gate
PROLOGUE_ONLY = ('mixed_cin', 'swish_leaky_edges', 'swish_leaky_edges_sft', 'solo_cin')       # families that ARE their prologue: the upsampling forms take none
SHAPE_KEYS = ('a', 'b', 'c', 'd', 'e', 'f', 'g', 'u1', 'u2', 'zu1', 'zu2')
W42_KEYS = ('u1', 'zu1', 'zu2')                   # the shapes of the sub-pixel F(4,2) form: 1, 3 and 8 slabs; one block per phase, 2 x 3 blocks, one block


@pytest.fixture(scope='module')
def cc():
    import torch
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    from codeformer_amd import lib
    lib.load()
    m = load_script('tools/conv_check.py')
    m.with_f42()
    assert m.ROUTES == ROUTES and m.GATE_FAMILIES == GATE_FAMILIES and m.SOLO_FAMILIES == SOLO_FAMILIES and tuple(m.SHAPES) == SHAPE_KEYS
    return m


def test_the_cases_reach_every_route(cc):
    reached = {r for key in SHAPE_KEYS for _, _, _, r, _ in cc.launches(key)}
    assert reached == set(ROUTES)
    forms = {(r, f) for key in SHAPE_KEYS for _, _, _, r, f in cc.launches(key)}
    assert {('d32', '256x64'), ('d32', '128x128'), ('d32', 'narrow 128x64'), ('d32', 'folded 256x64'), ('d32', 'folded narrow 128x64'), ('dsplit', 'form 0 64-wide'),
            ('dsplit', 'form 1 64-wide'), ('w23_f32', 'split-K 1'), ('w23_f32', 'split-K 2'), ('w23_f32', 'split-K 4'), ('w23_h4', 'split-K 4'), ('w23_h8', 'f16x2'),
            ('w23_h8', 'f16'), ('w23_h8', 'bf16'), ('w43_8', 'ntn 3'), ('w43_up', 'k32 gather'), ('w42_up', 'sub-pixel phases')} <= forms
    assert tuple(key for key in SHAPE_KEYS if any(r == 'w42_up' for _, _, _, r, _ in cc.launches(key))) == W42_KEYS


# ---- 1. the exact family ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', SHAPE_KEYS)
def test_int_coded_is_the_fp64_result_bitwise(cc, key):
    """d32, dsplit (plain and folded), w23_f32 at every split count, w23_h4, w23_h8 in its three operand types; prologue none / affine, epilogue bias /
    residual / SFT: torch.equal with the fp64 result.  (F(4,3) cannot be exact: see conv_check.)"""
    import torch
    ran = set()
    for variant in range(1 if cc.SHAPES[key][6] else 4):
        d, ref = cc.prepared('int_coded', key, variant)
        want = ref['out'].float()
        assert torch.equal(want.double(), ref['out'])
        want = want.cuda()
        for cname, code, sk, route, form in cc.launches(key, cc.EXACT_ROUTES):
            got = cc.run(d, code, sk, ('int_coded', key))
            bad = int((got != want).sum())
            assert bad == 0, (key, variant, cname, sk, route, form, bad, float((got - want).abs().max()))
            ran.add(route)
    assert ran and ran <= set(cc.EXACT_ROUTES)


# ---- 2. the impulse families -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', ('a', 'b', 'c', 'd', 'g', 'u1', 'zu1', 'zu2'))
def test_onehot_pixels_select_the_flipped_weight(cc, key):
    """out = the flipped weight slice + bias around each pixel, the bias elsewhere: d32 bitwise fp32(w + b); every other route within the gate."""
    import torch
    d, ref = cc.prepared('onehot_pixels', key)
    want32 = ref['out'].float().cuda()
    for cname, code, sk, route, form in cc.launches(key):
        got = cc.run(d, code, sk, ('onehot_pixels', key))
        if route == 'd32' and not cc.SHAPES[key][6]:
            assert cc.bits_equal(got + 0.0, want32 + 0.0), (key, form, float((got - want32).abs().max()))
        else:
            if route == 'd32':          # folded: a tap is a sum of up to four weights (more than one rounding) -- except where ONE weight meets the pixel:
                p, _ = cc.prologue64(d)  # the outputs diagonal to a pixel's 2x2 block, and every output no pixel reaches: bitwise fp32(w + b) / b there
                one = (cc.conv64(p.abs(), torch.ones(1, p.shape[3], 3, 3))[..., 0] <= 1.0).cuda()
                assert int(one.sum()) > 8 * len(cc.onehot_positions(*cc.SHAPES[key][1:4])) and bool(((got + 0.0) == (want32 + 0.0))[one].all()), (key, form)
            r, err = cc.ratio(got, ref, cc.gate('onehot_pixels', key, route, code, sk))
            print(f'onehot_pixels {key} {route} {cname} {form}: max|d| {err:.3e} = {r:.4f} of the gate')
            assert r <= 1.0, (key, route, cname, form, r, err)


@pytest.mark.parametrize('key', ('b', 'c', 'd', 'u1', 'zu1', 'zu2'))
def test_tap_shift_moves_the_input_and_pads_each_border_with_zeros(cc, key):
    """Per tap a signed channel permutation: the input moved by one pixel.  d32 bitwise; dsplit within the 22-bit split of x (and the absolute 2^-25 / s of
    a subnormal lo half); the Winograd routes within the gate."""
    for tap in range(9):
        d, ref = cc.prepared('tap_shift', key, tap)
        want = ref['out']
        s = cc.act_scale_of(d)[:, None, None, None]
        for cname, code, sk, route, form in cc.launches(key):
            if sk > 1:
                continue
            got = cc.run(d, code, sk, ('tap_shift', key, tap))
            if route == 'd32':
                assert cc.bits_equal(got.cpu() + 0.0, want.float() + 0.0), (key, tap, form)
            elif route == 'dsplit':
                err = (got.double().cpu() - want).abs()
                tol = 2.0 ** -22 * want.abs() + 2.0 ** -25 * (1.0 + 2.0 ** -10) / s
                assert bool((err <= tol).all()), (key, tap, form, float((err / tol).max()))
            else:
                r, err = cc.ratio(got, ref, cc.gate('tap_shift', key, route, code, sk, tap))
                assert r <= 1.0, (key, tap, route, cname, form, r, err)


# ---- 3. the gate families --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family,route', [(f, r) for f in GATE_FAMILIES + SOLO_FAMILIES for r in ROUTES if not (r in UP_ROUTES and f in PROLOGUE_ONLY)])
def test_family_within_the_gate(cc, family, route):
    """The per-element gate on every shape, code and split count that reaches the route; the measured / gate ratio is printed, may not exceed 1 and may
    not fall below 1e-3 of the emulation's (a gate that loose would check nothing)."""
    worst, emu, n = 0.0, 0.0, 0
    for key in SHAPE_KEYS:
        if cc.SHAPES[key][6] and family in PROLOGUE_ONLY:
            continue
        for cname, code, sk, rt, form in cc.launches(key, (route,)):
            r = cc.case(family, key, code, sk, route)
            print(f'{family} {key} {route} {cname} {form}: max|d| {r["err"]:.3e} = {r["ratio"]:.4f} of the gate | emulation {r["emu_err"]:.3e} = {r["emu_ratio"]:.4f}')
            assert r['ratio'] <= 1.0, (family, key, route, cname, form, r)
            worst, emu, n = max(worst, r['ratio']), max(emu, r['emu_ratio']), n + 1
    assert n > 0 and emu > 0.0
    assert worst >= 1e-3 * emu, (family, route, worst, emu)
    print(f'TABLE {family} {route} {worst:.4f} {emu:.4f}')


@pytest.mark.parametrize('key', ('b', 'e'))
def test_a_single_unit_tap_moves_a_solo_input_bitwise(cc, key):
    """solo_cin_act's input (channel scales 2^-16 .. 2^16) against tap_shift's weight, one +-1 per output channel: d32 returns +- the moved input bit for
    bit, the smallest channels included (cout 64 reads 64 of the 256 channels at e)."""
    import torch
    base = cc.family('solo_cin_act', key)
    for tap in (0, 4, 8):
        d = dict(base, w=cc.tap_weight(*cc.SHAPES[key][3:5], tap), b=torch.zeros_like(base['b']))
        want = cc.reference(d)['out']
        assert torch.equal(want, want.float().double()) and float(want.abs().min()) < 2.0 ** -20 < 2.0 ** 16 < float(want.abs().max())
        got = cc.run(d, 0, 0, ('solo_tap', key, tap))
        assert cc.bits_equal(got.cpu() + 0.0, want.float() + 0.0), (key, tap, int((got.cpu() != want.float()).sum()))


# ---- 4. bitwise contracts and containment on the hard families ---------------------------------------------------------------------------------
@pytest.mark.parametrize('family', ('cancel_pairs', 'mixed_cout'))
def test_every_split_count_gives_the_same_bits(cc, family):
    """split_k 1, 2 (256 channels) and 1, 2, 4 (512 channels) of the split-K instantiation, fp32 operands and split halves."""
    from codeformer_amd import ops
    for key in ('e', 'f'):
        d, _ = cc.prepared(family, key)
        for code in (ops.WINOGRAD, ops.WSPLIT):          # w23_f32, w23_h4
            outs = [(sk, cc.run(d, code, sk, (family, key))) for sk in (1, 2, 4) if cc.route_of(code, 16, 16, d['w'].shape[1], d['w'].shape[0], split_k=sk)]
            assert len(outs) == (2 if key == 'e' else 3)
            for sk, y in outs[1:]:
                assert cc.bits_equal(y, outs[0][1]), (family, key, code, sk, int((y != outs[0][1]).sum()))


@pytest.mark.parametrize('family', ('cancel_pairs', 'mixed_cout'))
def test_an_image_alone_equals_the_image_inside_a_batch_of_three(cc, family):
    import torch
    reached = set()
    for key in ('b', 'c', 'd', 'e', 'g', 'u1', 'u2', 'zu1', 'zu2'):
        d, _ = cc.prepared(family, key)
        x0 = d['x'][:1]
        first = lambda t: t[:1].expand(3, *t.shape[1:]).contiguous()
        d3 = dict(d, x=torch.cat((torch.roll(x0, 1, dims=2), x0, torch.flip(x0, dims=(1,)))), sc=first(d['sc']), sh=first(d['sh']), res=first(d['res']), ss=first(d['ss']))
        for cname, code, sk, route, form in cc.launches(key):
            y3 = cc.run(d3, code, sk, (family, key))
            y1 = cc.run(d3, code, sk, (family, key), images=slice(1, 2))
            assert cc.bits_equal(y3[1:2], y1), (family, key, route, cname, form, int((y3[1:2] != y1).sum()))
            reached.add(route)
    assert reached == set(ROUTES)


@pytest.mark.parametrize('family', ('cancel_pairs', 'mixed_cout'))
def test_a_concatenated_input_equals_the_dense_tensor(cc, family):
    """x2 split at every legal boundary (multiples of 16, or of 32 where the route's slab is 32): the bits of the dense launch.  fp32 routes and split-half
    routes with an affine prologue (both families have one), so no range-scale table differs between the two launches."""
    reached = set()
    for key in ('b', 'c', 'd', 'g', 'e'):
        B, H, W, cin, cout, _, _ = cc.SHAPES[key]
        d, _ = cc.prepared(family, key)
        assert d['pro'] == cc.PRO_AFFINE
        for cname, code, sk, route, form in cc.launches(key):
            cuts = [c for c in range(16, cin, 16) if cc.route_of(code, H, W, cin, cout, False, sk, c) is not None]
            if not cuts:
                continue
            dense = cc.run(d, code, sk, (family, key), c_split=None)
            for c in cuts:
                y = cc.run(d, code, sk, (family, key), c_split=c)
                assert cc.bits_equal(y, dense), (family, key, route, cname, form, c, int((y != dense).sum()))
            reached.add(route)
    assert reached == set(ROUTES) - set(UP_ROUTES)        # (the upsampling forms take one input)


def _allowed(route, pixels, H, W):
    """The outputs that non-finite conv-input pixels may reach, from the tile geometry: direct routes the 3x3 neighbourhoods; F(m, 3) the m x m output
    tiles whose (m + 2) x (m + 2) input window (rows m t - 1 .. m t + m) holds a pixel.  (With upsampling the conv input is the upsampled image: one
    source pixel is four of its pixels.)"""
    import torch
    ok = torch.zeros(H, W, dtype=torch.bool)
    m = 1 if route in ('d32', 'dsplit') else 2 if route.startswith('w23') else 4
    for r, q in pixels:
        for t in range(H // m):
            for v in range(W // m):
                if m * t - 1 <= r <= m * t + m and m * v - 1 <= q <= m * v + m:
                    ok[m * t:m * t + m, m * v:m * v + m] = True
    return ok


def _allowed42(r, q, H, W):
    """Sub-pixel F(4,2) phases, (H, W) and the pixel (r, q) on the LOW-RESOLUTION grid: phase (a, b) of tile (t, v) reads the rows 4 t - 1 + a .. 4 t + 3 + a and the
    columns 4 v - 1 + b .. 4 v + 3 + b, and writes the outputs (2 i + a, 2 j + b) of its 4x4 positions.  -> (2 H, 2 W) bool."""
    import torch
    ok = torch.zeros(2 * H, 2 * W, dtype=torch.bool)
    for a in (0, 1):
        for b in (0, 1):
            for t in range(H // 4):
                for v in range(W // 4):
                    if 4 * t - 1 + a <= r <= 4 * t + 3 + a and 4 * v - 1 + b <= q <= 4 * v + 3 + b:
                        ok[8 * t + a:8 * t + 8:2, 8 * v + b:8 * v + 8:2] = True
    return ok


@pytest.mark.parametrize('key', ('b', 'c', 'd', 'u1', 'zu1', 'zu2'))
def test_a_non_finite_pixel_stays_inside_the_tiles_that_read_it(cc, key):
    """One NaN, then one +inf, in a single input pixel and channel, at a patch interior, at pixels whose 3x3 reach crosses the corner of an 8x16 and of a
    16x16 patch, at pixel (0, 0) of the FIRST image (the address every clamped out-of-image load reads) and in the last row.  Affine prologue with sc = 1, sh = 0: no range scale reads the tensor (the upsampling gather
    takes no prologue and has fp32 operands: no range scale either).  Outside the allowed set every output bit equals the clean run; inside the true
    3x3 neighbourhood every output channel is non-finite (the weights are dense, non-zero).  No statistics partials are read.
    w42_up: a low-resolution pixel is read by the 4x4 low-resolution tiles whose 5x5 window, moved by the phase, holds it, in all four phases: the allowed
    set is those tiles' outputs (2 i + a, 2 j + b), phase by phase -- within the 2x-scaled footprint of the tiles (_allowed42)."""
    import torch
    B, H, W, cin, cout, _, up = cc.SHAPES[key]
    Ho, Wo = (2 * H, 2 * W) if up else (H, W)
    base, _ = cc.prepared('cancel_pairs', key)
    assert bool((base['w'] != 0).all())
    affine = dict(base, pro=cc.PRO_AFFINE, sc=torch.ones_like(base['sc']), sh=torch.zeros_like(base['sh']))
    spots = [(4, 5), (7, 15), (15, 15), (0, 0), (H - 1, 9)]
    for cname, code, sk, route, form in cc.launches(key):
        d = base if route in UP_ROUTES else affine
        clean = cc.run(d, code, sk, ('cancel_pairs', key))
        assert bool(torch.isfinite(clean).all())
        for val in (float('nan'), float('inf')):
            for i, (r, q) in enumerate(spots):
                x = d['x'].clone()
                bi = 0 if (r, q) == (0, 0) else B - 1          # (the tensor's very first pixel is what a clamped out-of-image load reads)
                x[bi, r, q, (7 * i + 3) % cin] = val
                y = cc.run(d, code, sk, ('cancel_pairs', key), x=x)
                pixels = [(2 * r + a, 2 * q + b) for a in (0, 1) for b in (0, 1)] if up else [(r, q)]
                ok = (_allowed42(r, q, H, W) if route == 'w42_up' else _allowed(route, pixels, Ho, Wo)).cuda()
                assert route != 'w42_up' or (int(ok.sum()) <= 4 * 64 and bool(ok[2 * r:2 * r + 2, 2 * q:2 * q + 2].all()))     # (at most four tiles' footprints)
                same = (y.view(torch.int32) == clean.view(torch.int32)).all(dim=3)
                others = [b for b in range(B) if b != bi]
                assert bool(same[others].all()) and bool(same[bi][~ok].all()), (key, route, cname, form, val, (r, q), int((~same[bi][~ok]).sum()))
                near = torch.zeros(Ho, Wo, dtype=torch.bool)
                for pr, pq in pixels:
                    near[max(pr - 1, 0):pr + 2, max(pq - 1, 0):pq + 2] = True
                assert bool((~torch.isfinite(y[bi][near.cuda()])).all()), (key, route, cname, form, val, (r, q))


@pytest.mark.parametrize('key', W42_KEYS)
def test_the_sub_pixel_form_repeats_its_bits(cc, key):
    """w42_up, run to run, on the two families whose sums cancel; and the four phases are all written: no output keeps the fill of a fresh tensor."""
    import torch
    from codeformer_amd import ops
    for family in ('dc_plus_ripple', 'cancel_pairs'):
        d, ref = cc.prepared(family, key)
        y0 = cc.run(d, ops.WF42U, 0, (family, key))
        y1 = cc.run(d, ops.WF42U, 0, (family, key))
        assert cc.bits_equal(y0, y1), (family, key, int((y0 != y1).sum()))
        assert tuple(y0.shape) == tuple(ref['out'].shape) and bool(torch.isfinite(y0).all())
