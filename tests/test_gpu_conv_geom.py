"""-m gpu: the stride-2, 1x1 and general-geometry convolutions per element on exact, impulse and mixed-scale inputs.

The cases, the fp64 reference written from the definitions, the routes, the per-element gate with its derivation and the CPU emulation live in
tools/conv_geom_check.py; tests/test_conv_geom_host.py proves on the CPU that the emulation stays within 0.5 of the gate, that the exactness
preconditions hold and that the reference is the index-by-index convolution, so every condition here is a condition on the reference.  Weights are
packed with the explicit code (0, or ops.SPLIT with stride2=True / a 1x1 weight); fp32 1x1 launches pass split_k=0.  Nothing is larger than 128x128x32
in or 64x64x384 out.

Measured on an MI355X, the whole file 7.9 s (167 cases; none above 0.4 s, the CPU references included; every case runs every gate family
but mixed_cout at p1c, see conv_geom_check.families_of).  Largest |error| / gate per family and route,
kernel | CPU emulation (test_family_within_the_gate prints every single ratio; onehot_pixels: the kernel's; -: the route lacks the family's prologue or epilogue):
                          s2_d32          s2_dsplit       c1_d32          c1_dsplit       ext_d32         ext_up          d32_32          head
    mixed_cout            0.0262 | 0.0247 0.2748 | 0.2748 0.1149 | 0.1257 0.4679 | 0.4680 0.4939 | 0.4939 0.0117 | 0.0096 0.0231 | 0.0201 0.0114 | 0.0118
    mixed_cin             0.0542 | 0.0196 -               0.1032 | 0.0948 0.0661 | 0.0649 0.0426 | 0.0141 0.0180 | 0.0130 0.0619 | 0.0165 0.0181 | 0.0072
    mixed_cin_act         0.0572 | 0.0182 0.0105 | 0.0084 0.1118 | 0.0901 0.0699 | 0.0571 0.0342 | 0.0193 0.0200 | 0.0131 0.0539 | 0.0155 0.0190 | 0.0101
    cancel_pairs          0.0023 | 0.0058 0.0019 | 0.0023 0.0220 | 0.0123 0.0317 | 0.0288 0.0018 | 0.0041 0.0023 | 0.0022 0.0020 | 0.0047 0.0005 | 0.0017
    dc_plus_ripple        0.0124 | 0.0119 0.0038 | 0.0041 0.0558 | 0.0565 0.0205 | 0.0180 0.0116 | 0.0082 0.0046 | 0.0043 0.0138 | 0.0126 0.0023 | 0.0007
    swish_leaky_edges     0.4234 | 0.4234 -               0.4886 | 0.4886 0.4792 | 0.4792 0.4050 | 0.4050 0.3811 | 0.3811 0.4387 | 0.4387 -
    swish_leaky_edges_sft 0.3096 | 0.4366 0.2474 | 0.4363 0.4254 | 0.4254 0.4003 | 0.4218 -               -               0.2386 | 0.3863 -
    solo_cin              0.3512 | 0.3832 -               0.4747 | 0.4747 0.4995 | 0.4995 .               .               .               .
    solo_cin_act          0.4072 | 0.4072 0.4547 | 0.4547 0.4981 | 0.4981 0.4998 | 0.4995 .               .               .               .
    onehot_pixels         0.4220          0.3679          0.4273          0.4157          0.4741          0.4193          0.2292          0.2243
(the PReLU instantiations -- route `prelu` of conv_geom_check, merged in by with_prelu() -- have a file of their own, tests/test_gpu_conv_prelu.py, which calls the
tests of this file that fit; its column, kernel | emulation: mixed_cout 0.4333 | 0.4333, mixed_cin 0.0403 | 0.0162, mixed_cin_act 0.0440 | 0.0182, cancel_pairs
0.0020 | 0.0046, dc_plus_ripple 0.0109 | 0.0089, swish_leaky_edges 0.3609 | 0.3609, swish_leaky_edges_sft -, solo ., onehot_pixels 0.4312.)
(.: the solo families run on the two split-half routes and their fp32 partners only.  Their c1 cells sit at one half by construction: a 1x1 with one input
channel per output is ONE product, every rounding on its way is entered at a whole ulp and attains half of that -- see conv_geom_check.)
(equal pairs: one rounding both evaluations make alike -- the residual add of swish_leaky_edges, the half rounding of a small channel's weight in
mixed_cout on the split-half routes, and on ext_d32 the bias add of the 32-wide rung's smallest channel; they exercise the epilogue and the packer,
not the accumulation, whose evidence is in the cells that differ, in int_coded, tap_shift and onehot_pixels.)

What the first run found.  The split-half stride-2 form indexed its affine-prologue tables by the 4 c0 channels of the space-to-depth view and so
read a [batch][c0] table past its end: int_coded wrong in 32752 of 32768 elements at s2a, the gates of the four affine families missed by factors of
2e4 .. 6e6, NaN statistics.  No layer of the network asks for it; cf_split_launch now refuses it (test 9) and the families run there without it.
The containment question: at c0 = 16 the reach of a non-finite pixel is the 2x2 space-to-depth window, exactly; the arithmetic is kept and the
header and DESIGN.md state it (test 6 pins both sets).  Everything else held on the first run: slices and the dense launch agree bitwise, no
masked edge tile writes outside its tensor.

Scratch builds with one in-range edit each (not committed; addresses, barriers and launch geometry untouched, the one mask edit narrows), each run once
through this file and the four old tests that cover these forms (test_split_conv_stride2.., test_split_conv_1x1_streaming.. of test_gpu_split.py,
test_border_modes_and_symmetric_stride2 of test_parsenet.py, test_pixel_unshuffle_and_strided_conv_ops of test_rrdbnet.py).  Tests of this file that fail | old:
  (e1) cf_igemm.hip cf_border: reflection as a clamp                 32: int_coded, onehot_pixels, tap_shift on s2r e1r e2r e3r hd; 17 gates (every family on s2_d32,
                                                                      ext_d32 and head) | 1 (border_modes_and_symmetric_stride2)
  (e2) cf_igemm.hip EXT stride-2 gather: pad_lo read as 0             13: int_coded, onehot_pixels, tap_shift on s2z s2r; six s2_d32 gates; containment on s2_d32 | 1 (border_modes..)
  (e3) cf_pack.hip split halves: subnormal lo halves flushed to zero  2: mixed_cout on s2_dsplit and c1_dsplit | 0
  (e4) cf_split.hip 1x1 form: the lo hi MFMA left out                 9: tap_shift p1a p1b p1c; six c1_dsplit gates | 1 (split_conv_1x1_streaming..)
  (e5) cf_igemm.hip AXPY2: alpha applied once                         8: int_coded, onehot_pixels, tap_shift on epa2; five ext_d32 gates | 1 (pixel_unshuffle_and_strided_conv_ops)
  (e6) cf_igemm.hip EXT epilogue mask: `ox < wout - 1`                83: every test of the sixteen EXT cases, slices, edge tiles, containment and invariance on the
                                                                      three EXT routes | 2 (border_modes.., pixel_unshuffle..)
  (e7) cf_split.hip s2_skip: one block too many skipped               13: int_coded, onehot_pixels on s2b s2c s2d, tap_shift s2b s2d, five s2_dsplit gates | 1 (split_conv_stride2..)
         (tap 1 of parity (1, 0))                                     (s2a, c0 = 16, does not skip and passes, as it should; tap_shift at s2c runs taps 0, 4, 8 only)
Plainly: six of the seven edits are gross and the old whole-tensor bounds catch them too; there this file adds the localisation (which case, route and
family).  One (e3: subnormal lo halves flushed in the packer, an error confined to channels small next to the tensor's largest) is caught by this file
alone, as was the real defect above.  e1 does not move the containment sets: a clamp reads the border pixel where the reflection reads its neighbour,
and both windows belong to the same outputs.
  (s1) cf_split.hip split2: the lo half of an activation zeroed       11: the solo gates of s2_dsplit (solo_cin_act) and c1_dsplit (both), tap_shift on the seven split-half
         where it is a subnormal half, |a| < 2^-3                      cases, mixed_cout on c1_dsplit | 0 of the two split-half tests above (stride2.., 1x1_streaming..)
The solo families exist for this edit: see tests/test_gpu_conv_families.py, which lists it on all four split-half kernels.
"""
import pytest

from _tools import load_script

pytestmark = pytest.mark.gpu

ROUTES = ('s2_d32', 's2_dsplit', 'c1_d32', 'c1_dsplit', 'ext_d32', 'ext_up', 'd32_32', 'head')
FORMS = {('s2_d32', '64-wide'), ('s2_d32', '128-wide'), ('s2_d32', 'ext'), ('s2_dsplit', '64-wide skip'), ('s2_dsplit', '64-wide no-skip'),
         ('s2_dsplit', '128-wide'), ('c1_d32', '256x64'), ('c1_d32', '128x128'), ('c1_d32', 'narrow 128x64'), ('c1_dsplit', '64-wide'),
         ('c1_dsplit', '128-wide'), ('ext_d32', '128'), ('ext_d32', '64'), ('ext_d32', '32'), ('ext_up', '128'), ('ext_up', '64'),
         ('d32_32', '256x32'), ('head', 'few_cout reflect')}
CASE_KEYS = ('s2a', 's2b', 's2c', 's2d', 's2z', 's2r', 'p1a', 'p1b', 'p1c', 'p1d', 'e1z', 'e1r', 'e2z', 'e2r', 'e3z', 'e3r', 'sl', 'epl', 'epa', 'epa2',
             'u1z', 'u1e', 'u2z', 'u2e', 'd32', 'hd')
GATE_FAMILIES = ('mixed_cout', 'mixed_cin', 'mixed_cin_act', 'cancel_pairs', 'dc_plus_ripple', 'swish_leaky_edges', 'swish_leaky_edges_sft')
SOLO_FAMILIES = ('solo_cin', 'solo_cin_act')      # one input channel per output channel: the split-half routes and their fp32 partners
SOLO_ROUTES = ('s2_d32', 's2_dsplit', 'c1_d32', 'c1_dsplit')
SFT_ROUTES = ('s2_d32', 's2_dsplit', 'c1_d32', 'c1_dsplit', 'd32_32')       # routes with the SFT epilogue (the EXT instantiations and the head lack it)
NAN_BITS = 0x7fc00000


@pytest.fixture(scope='module')
def gc():
    import torch
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    from codeformer_amd import lib
    lib.load()
    m = load_script('tools/conv_geom_check.py')
    assert m.ROUTES == ROUTES and m.GATE_FAMILIES == GATE_FAMILIES and tuple(m.CASES) == CASE_KEYS
    assert m.SOLO_FAMILIES == SOLO_FAMILIES and m.SOLO_ROUTES == SOLO_ROUTES
    return m


def _taps(gc, key):
    return (0,) if gc.CASES[key].taps == 1 else (0, 4, 8) if key in gc.BIG else tuple(range(9))


# ---- 1. reach --------------------------------------------------------------------------------------------------------------------------------
def test_the_cases_reach_every_route_and_form(gc):
    forms = {(r, f) for key in CASE_KEYS for _, _, r, f in gc.launches(key)}
    assert forms == FORMS and {r for r, _ in forms} == set(ROUTES)


# ---- 2. the exact family ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', CASE_KEYS)
def test_int_coded_is_the_fp64_result_bitwise(gc, key):
    """Every route, every (prologue, epilogue) variant the route takes; AXPY / AXPY2 with alpha 0.5; LEAKY: float32(0.2) * pre rounded once."""
    import torch
    n = 0
    for cname, code, route, form in gc.launches(key):
        for variant in gc.int_coded_variants(key, route, form):
            d, ref, _ = gc.prepared('int_coded', key, route, form, variant)
            want = ref['out'].float()
            assert d['epi'] == gc.EPI_LEAKY or torch.equal(want.double(), ref['out'])
            got = gc.run(d, key, code, ('int_coded', key, variant, d['epi']))
            bad = int((got != want.cuda()).sum())
            assert bad == 0, (key, variant, cname, route, form, bad, float((got.cpu() - want).abs().max()))
            n += 1
    assert n >= 2


# ---- 3. the impulse families -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', CASE_KEYS)
def test_onehot_pixels_select_the_weight(gc, key):
    """fp32 routes: bitwise fp32(w + b) wherever at most ONE weight meets a pixel (no reflected second reading, no folded sum), the bias elsewhere;
    every output of every route within the gate."""
    import torch
    g = gc.CASES[key]
    for cname, code, route, form in gc.launches(key):
        d, ref, tol = gc.prepared('onehot_pixels', key, route, form)
        got = gc.run(d, key, code, ('onehot_pixels', key, 0, d['epi']))
        if route not in gc.SPLIT_ROUTES and g.epi is None:
            one = gc.conv64(gc.padded(d['x'].double().abs(), g), torch.ones_like(d['w'][:1]), g)[..., 0] <= 1.0
            assert int(one.sum()) > 4 * len(gc.onehot_positions(g, 0)) or g.taps == 1
            want32 = ref['out'].float()
            assert bool(((got.cpu() + 0.0) == (want32 + 0.0))[one].all()), (key, route, form, float((got.cpu() - want32)[one].abs().max()))
        r, err = gc.ratio(got, ref, tol)
        print(f'onehot_pixels {key} {route} {cname} {form}: max|d| {err:.3e} = {r:.4f} of the gate')
        assert r <= 1.0, (key, route, cname, form, r, err)


@pytest.mark.parametrize('key', CASE_KEYS)
def test_tap_shift_moves_decimates_or_permutes_the_input(gc, key):
    """Per tap a signed channel permutation of the shifted (stride 2: decimated; taps 1: unmoved) input under the case's padding rule.  fp32 routes
    bitwise (AXPY / AXPY2 round twice: within the gate); split-half routes within the 22-bit split of x and the absolute 2^-25 / s of a subnormal lo half."""
    g = gc.CASES[key]
    for tap in _taps(gc, key):
        for cname, code, route, form in gc.launches(key):
            d, ref, tol = gc.prepared('tap_shift', key, route, form, tap)
            want = ref['out']
            got = gc.run(d, key, code, ('tap_shift', key, tap, d['epi']))
            if route in gc.SPLIT_ROUTES:
                s = gc.act_scale_of(d)[:, None, None, None]
                err = (got.double().cpu() - want).abs()
                lim = 2.0 ** -22 * want.abs() + 2.0 ** -25 * (1.0 + 2.0 ** -10) / s
                assert bool((err <= lim).all()), (key, tap, form, float((err / lim).max()))
            elif g.epi in (gc.EPI_AXPY, gc.EPI_AXPY2):
                r, err = gc.ratio(got, ref, tol)
                assert r <= 1.0, (key, tap, route, form, r, err)
            else:
                assert gc.bits_equal(got.cpu() + 0.0, want.float() + 0.0), (key, tap, route, form)


# ---- 4. the gate families --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family,route', [(f, r) for f in GATE_FAMILIES for r in ROUTES
                                          if not (f == 'swish_leaky_edges_sft' and r not in SFT_ROUTES) and not (f == 'swish_leaky_edges' and r in ('head', 's2_dsplit'))
                                          and not (f == 'mixed_cin' and r == 's2_dsplit')])
def test_family_within_the_gate(gc, family, route):
    """The per-element gate on every case and form that reaches the route; the measured / gate ratio is printed, may not exceed 1 and may not fall
    below 1e-3 of the emulation's (a gate that loose would check nothing)."""
    worst, emu, n = 0.0, 0.0, 0
    for key in gc.cases_of(route):
        if family not in gc.families_of(key):
            continue
        for cname, code, rt, form in gc.launches(key, (route,)):
            r = gc.case(family, key, code, route, form)
            if r is None:
                continue
            print(f'{family} {key} {route} {cname} {form}: max|d| {r["err"]:.3e} = {r["ratio"]:.4f} of the gate | emulation {r["emu_err"]:.3e} = {r["emu_ratio"]:.4f}')
            assert r['ratio'] <= 1.0, (family, key, route, cname, form, r)
            worst, emu, n = max(worst, r['ratio']), max(emu, r['emu_ratio']), n + 1
    assert n > 0 and emu > 0.0
    assert worst >= 1e-3 * emu, (family, route, worst, emu)
    print(f'TABLE {family} {route} {worst:.4f} {emu:.4f}')


@pytest.mark.parametrize('family,route', [(f, r) for f in SOLO_FAMILIES for r in SOLO_ROUTES if not (f == 'solo_cin' and r == 's2_dsplit')])
def test_solo_family_within_the_gate(gc, family, route):
    """One input channel per output channel over 32 binades of channel scales, on every case and form of the split-half routes and their fp32 partners,
    under conv_geom_check's solo gate (c counts the one product chain that exists; the floor sums that channel alone, at the whole spacing)."""
    worst, emu, n = 0.0, 0.0, 0
    for key in gc.cases_of(route):
        for cname, code, rt, form in gc.launches(key, (route,)):
            r = gc.case(family, key, code, route, form)
            assert r is not None, (family, key, route, form)
            print(f'{family} {key} {route} {cname} {form}: max|d| {r["err"]:.3e} = {r["ratio"]:.4f} of the gate | emulation {r["emu_err"]:.3e} = {r["emu_ratio"]:.4f}')
            assert r['ratio'] <= 1.0, (family, key, route, cname, form, r)
            worst, emu, n = max(worst, r['ratio']), max(emu, r['emu_ratio']), n + 1
    assert n >= 3 and emu > 0.0
    assert worst >= 1e-3 * emu, (family, route, worst, emu)
    print(f'TABLE {family} {route} {worst:.4f} {emu:.4f}')


# ---- 5. slices and masked edge tiles -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', ('dc_plus_ripple', 'mixed_cout', 'int_coded'))
def test_channel_slices_equal_the_dense_launch_and_leave_their_surroundings_alone(gc, family):
    """x = buf[..., 16:48] of 80, x2 = buf2[..., :32] of 48, out = obuf[..., 32:96] of 128 (the residual in a slice of the same stride), every channel
    around them NaN before the launch: the out slice is bitwise the dense launch on contiguous copies, every other element of obuf keeps its bits."""
    import torch
    d, _, _ = gc.prepared(family, 'sl', 'ext_d32', '64', 1 if family == 'int_coded' else 0)
    keep = {}
    y = gc.run(d, 'sl', 0, (family, 'sl'), keep=keep)
    dense = gc.run(d, 'sl', 0, (family, 'sl'), dense=True)
    assert bool(torch.isfinite(dense).all()) and gc.bits_equal(y.contiguous(), dense), int((y != dense).sum())
    width, at = gc.SLICE['out']
    bits = keep['obuf'].view(torch.int32)
    assert y.data_ptr() == keep['obuf'][..., at:].data_ptr() and keep['obuf'].shape[3] == width
    assert bool((bits[..., :at] == NAN_BITS).all()) and bool((bits[..., at + y.shape[3]:] == NAN_BITS).all())
    for name, (w, a) in (('buf', gc.SLICE['x']), ('buf2', gc.SLICE['x2'])):        # (the inputs' surroundings are still NaN: nothing wrote there either)
        b = keep[name].view(torch.int32)
        c = 32
        assert bool((b[..., :a] == NAN_BITS).all()) and bool((b[..., a + c:] == NAN_BITS).all()), name


@pytest.mark.parametrize('key', ('e1z', 'e1r', 'e2z', 'e3r', 'u1z', 'u2e', 's2z', 's2r', 'hd'))
def test_masked_edge_tiles_write_inside_the_tensor_only(gc, key):
    """An off-grid output that is a view into a larger NaN-filled allocation with guard rows behind it: the bits of the launch into a tensor of its own,
    and the guard untouched."""
    import torch
    g = gc.CASES[key]
    cname, code, route, form = gc.launches(key)[0]
    d, _, _ = gc.prepared('mixed_cout', key, route, form)
    Ho, Wo = gc.out_hw(g)
    shape = (g.B, g.cout, Ho, Wo) if g.out_nchw else (g.B, Ho, Wo, g.cout)
    n, guard = g.B * Ho * Wo * g.cout, 4 * 16 * max(Wo, 16) * max(g.cout, 32)        # (four tile rows of the widest tile)
    big = torch.full((n + guard,), float('nan'), device='cuda')
    y = gc.run(d, key, code, ('mixed_cout', key), out=big[:n].view(shape))
    own = gc.run(d, key, code, ('mixed_cout', key))
    assert bool(torch.isfinite(own).all()) and gc.bits_equal(y.contiguous(), own.contiguous()), (key, route, form)
    assert bool((big[n:].view(torch.int32) == NAN_BITS).all()), (key, route, form, int((big[n:].view(torch.int32) != NAN_BITS).sum()))


# ---- 6. containment ----------------------------------------------------------------------------------------------------------------------------
CONTAIN = {'s2_d32': ('s2a', 's2z', 's2r', 's2c'), 's2_dsplit': ('s2a', 's2d', 's2c'), 'c1_d32': ('p1a', 'p1d', 'p1c'), 'c1_dsplit': ('p1a', 'p1c'), 'ext_d32': ('e1z', 'e1r', 'e3r'),
           'ext_up': ('u1z', 'u1e'), 'd32_32': ('d32',), 'head': ('hd',)}


@pytest.mark.parametrize('route', ROUTES)
def test_a_non_finite_pixel_reaches_exactly_the_outputs_whose_window_holds_it(gc, route):
    """One NaN, then one +inf, in a single pixel and channel of the FIRST image: at pixel (0, 0) (the address a clamped out-of-image load reads), at
    (1, 1) (read twice under reflection), at an odd column in the interior, on a tile boundary and in the last row.  Affine prologue with sc = 1,
    sh = 0, so no range scale reads the tensor (s2_dsplit takes no affine prologue: prologue none, with the CLEAN input's range-scale table).  The non-finite outputs are exactly conv_geom_check.expected_reach(): the window under the case's
    stride and padding rule -- and in the split-half stride-2 form at c0 = 16, where the structurally zero weight blocks are multiplied, the 2x2
    window of the space-to-depth view, as include/codeformer_hip.h states (c0 = 32: the window itself).  Every other output keeps the clean run's bits."""
    import torch
    forms = set()
    for key in CONTAIN[route]:
        g = gc.CASES[key]
        for cname, code, rt, form in gc.launches(key, (route,)):
            base = gc.family_of('cancel_pairs', key, route, form)
            assert bool((base['w'] != 0).all())
            d = dict(base, pro=gc.PRO_AFFINE, sc=torch.ones_like(base['sc']), sh=torch.zeros_like(base['sh'])) if route != 's2_dsplit' else base
            tag = ('contain', key, d['epi'])
            clean = gc.run(d, key, code, tag)
            assert bool(torch.isfinite(clean).all())
            spots = dict.fromkeys([(0, 0), (1, 1), (4, min(5, g.W - 2)), (min(7, g.H - 2), min(15, g.W - 2)), (g.H - 1, min(9, g.W - 1))])
            for val in (float('nan'), float('inf')):
                for i, (r, q) in enumerate(spots):
                    x = d['x'].clone()
                    x[0, r, q, (7 * i + 3) % g.cin] = val
                    y = gc.run(d, key, code, tag, x=x, act_x=d['x'])
                    reach = gc.expected_reach(g, route, form, r, q).cuda()
                    same = (y.contiguous().view(torch.int32) == clean.contiguous().view(torch.int32)).all(dim=3)
                    assert bool(same[1:].all()) and bool(same[0][~reach].all()), (key, route, form, val, (r, q), int((~same[0][~reach]).sum()))
                    assert bool((~torch.isfinite(y[0][reach])).all()), (key, route, form, val, (r, q), int(torch.isfinite(y[0][reach]).sum()))
            forms.add(form)
    if route == 's2_dsplit':
        assert {'64-wide no-skip', '64-wide skip'} <= forms and gc.CASES['s2a'].cin == 16 and gc.CASES['s2d'].cin == 32


# ---- 7. statistics -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', ('mixed_cout', 'dc_plus_ripple'))
def test_stride_2_statistics_describe_the_tensor_that_was_written(gc, family):
    """The three stride-2 forms that emit GroupNorm partials at the cases' shapes (fp32 64-wide, split-half 64-wide with and without the skip):
    conv_case.stats_rel_err <= 1e-4, the bound of test_gpu_split.py."""
    forms = set()
    for key in ('s2a', 's2b', 's2d'):                 # (s2c: 384 channels are 12 per group, and the partials want a power of two)
        for cname, code, route, form in gc.launches(key):
            d, _, _ = gc.prepared(family, key, route, form)
            y = gc.run(d, key, code, (family, key, 0, d['epi']), stats=True)
            err = gc.stats_rel_err(y)
            print(f'{family} {key} {route} {form}: statistics rel err {err:.3e}')
            assert err <= 1e-4, (family, key, route, form, err)
            forms.add((route, form))
    assert forms == {('s2_d32', '64-wide'), ('s2_dsplit', '64-wide skip'), ('s2_dsplit', '64-wide no-skip')}


# ---- 8. invariance -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('route', ROUTES)
def test_a_launch_repeats_bitwise_and_an_image_alone_equals_the_image_in_a_batch(gc, route):
    import torch
    for key in gc.cases_of(route):
        if gc.CASES[key].sliced:
            continue
        for cname, code, rt, form in gc.launches(key, (route,)):
            d = gc.family_of('cancel_pairs', key, route, form)
            if d is None:
                d = gc.family_of('mixed_cout', key, route, form)
            x0 = d['x'][:1]
            first = lambda t: t[:1].expand(2, *t.shape[1:]).contiguous()
            d2 = dict(d, x=torch.cat((torch.roll(x0, 1, dims=2), x0)), sc=first(d['sc']), sh=first(d['sh']), res=first(d['res']), ss=first(d['ss']))
            tag = ('inv', key, d['epi'])
            y2 = gc.run(d2, key, code, tag)
            assert gc.bits_equal(y2.contiguous(), gc.run(d2, key, code, tag).contiguous()), (key, route, form)
            y1 = gc.run(d2, key, code, tag, images=slice(1, 2))
            assert gc.bits_equal(y2[1:2].contiguous(), y1.contiguous()), (key, route, form, int((y2[1:2] != y1).sum()))


# ---- 9. the finding of this file ---------------------------------------------------------------------------------------------------------------
def test_the_split_half_stride_2_form_refuses_an_affine_prologue(gc):
    """The space-to-depth view has 4 c0 channels and the kernel indexes its prologue tables by them, so it read a [batch][c0] table past its end (the first
    run of this file: int_coded wrong in 32752 of 32768 elements at s2a, NaN statistics).  The network never asks for it (Downsample has no norm
    in front); cf_split_launch now says so instead of launching."""
    import torch
    from codeformer_amd import ops
    d = gc.family('mixed_cout', 's2a')
    assert d['pro'] == gc.PRO_AFFINE
    pw = gc.packed(d, gc.CASES['s2a'], ops.SPLIT, ('mixed_cout', 's2a', 0, d['epi']))
    with pytest.raises(RuntimeError, match='stride 2 takes prologue none / leaky'):
        ops.conv2d(d['x'].cuda(), pw, stride=2, prologue=d['pro'], scale=d['sc'].cuda(), shift=d['sh'].cuda())
    y = ops.conv2d(d['x'].cuda(), pw, stride=2, prologue=gc.PRO_LEAKY, act=ops.act_scale(d['x'].cuda()))
    assert bool(torch.isfinite(y).all())
