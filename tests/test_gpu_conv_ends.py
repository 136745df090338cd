"""-m gpu: the NCHW ends of cf_conv2d per element -- the first conv's three implementations (conv3x3_few_cin_kernel<3>, <0>, and the MFMA instantiation
launch<9,1,4,1,2,2,true>) and both instantiations of conv3x3_few_cout_kernel under zero padding -- on exact, impulse and mixed-scale inputs.

The 34 cases are END_CASES of tools/conv_geom_check.py, merged into a module object of its own (with_nchw_ends()); reference, families, gates and emulation are
that file's, the proofs on the reference alone are in tests/test_conv_ends_host.py, and the tests of tests/test_gpu_conv_geom.py that fit a case unchanged are
called from here.  What that file pins (ROUTES, FORMS, CASE_KEYS, its figures) is untouched.

Measured on an MI355X: the whole file 3.9 s, 138 tests, none above 0.3 s (the CPU references included).  Largest |error| / gate per family and route,
kernel | CPU emulation (test_family_within_the_gate prints every single ratio; onehot_pixels: the kernel's; -: the route lacks the family's prologue or epilogue):
                          head (24 zero-padded cases)   nchw_in
    mixed_cout            0.0280 | 0.0245               0.4979 | 0.4979
    mixed_cin             0.0523 | 0.0188               -
    mixed_cin_act         0.0488 | 0.0204               0.1926 | 0.2214
    cancel_pairs          0.0014 | 0.0047               0.1120 | 0.1152
    dc_plus_ripple        0.0123 | 0.0092               0.2151 | 0.2561
    onehot_pixels         0.3372                        0.4706
nchw_in is larger than the other fp32 routes because its gate is small: 9 to 36 terms.  Its 0.4979 and 0.4706 are the MFMA cases nm3a / nm3b, one rounding the
kernel and the emulation make alike: the bias add of mixed_cout's smallest channel, u |pre| against the gate's 2 u |pre|, and the SFT epilogue of a one-hot pixel.  The
vector kernel's own largest ratio is 0.36 (mixed_cout, n1b); its statistics partials come to 0.091 of their bound (17 u of the sums of magnitudes: sixteen fp32
additions per thread, then fp64).  int_coded and tap_shift are bitwise on every case (K <= 36 on the input end: exactness is trivial there, the family checks addressing).

What the first run found.  No defect in a kernel: every case passed at once except one line of the test's own (tap_shift compared nm3b's SFT epilogue bitwise; it
rounds more than once and goes against the gate).  The finding is about dispatch: NO in_nchw launch exists off the 16x16 tile grid.  The vector kernel owns whole
tiles, and the MFMA instantiation that takes every other in_nchw launch (cout < 64, an epilogue, statistics other than two channels per group) is not an EXT one, so its
tile check refuses 17x19 and 24x40 with a message before any launch.  The network's input is 512x512; nothing asks for those sizes, the refusal was already in place, and
the last test of this file pins it (the host test asks the library the same through a parts query).  The MFMA form is reached at 16x16 and 32x48 through a residual and
an SFT epilogue.  The vector and the MFMA form of the same launch each meet fp64 within their gates and are not bitwise equal (50 .. 97 % of the elements differ in
their last bits: the vector kernel starts its FMA chain at the bias, the MFMA form adds it last); on int_coded both are the fp64 result.  Both few_cout instantiations hold
at every (cout, size, chunk count); a NaN pixel at (0, 0) reaches the four outputs of its window in image 0 and nothing else.

Scratch build with one in-range edit (not committed; a mask that narrows), run once through this file and the old tests of the same kernel:
  cf_igemm.hip few_cin fp32 fill: `ix < a.win - 1`      40 tests of this file fail: int_coded, onehot_pixels, tap_shift and the statistics test on the eight few_cin cases,
                                                        the four nchw_in gates, the four vector-against-MFMA cases (nm3a / nm3b, the MFMA form, pass, as they should)
                                                        | old: 3 (first_conv_reads_the_bytes x 2 and first_conv_non_temporal_variant of test_gpu_u8_boundary.py: the uint8
                                                        form has a fill of its own and stops agreeing with the fp32 one)
The five scratch builds of the cf_misc.hip kernels are in the docstring of tests/test_gpu_misc_kernels.py.
"""
import pytest

import test_gpu_conv_geom as base
from _tools import load_script

pytestmark = pytest.mark.gpu

NCHW_KEYS = ('n3a', 'n3b', 'n1a', 'n1b', 'n2a', 'n2b', 'n4a', 'n4b', 'nm3a', 'nm3b')
HEAD_KEYS = tuple(f'h{n}{t}{c}' for n in (1, 2, 4, 3) for t in 'ab' for c in (16, 32, 64))
END_KEYS = NCHW_KEYS + HEAD_KEYS
END_ROUTES = ('head', 'nchw_in')
FORMS = {('nchw_in', 'few_cin 3'), ('nchw_in', 'few_cin n'), ('nchw_in', 'mfma'), ('head', 'few_cout 4'), ('head', 'few_cout 3')}
GATE_FAMILIES = base.GATE_FAMILIES
NAN_BITS = base.NAN_BITS


@pytest.fixture(scope='module')
def gc():
    import torch
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    from codeformer_amd import lib
    lib.load()
    m = load_script('tools/conv_geom_check.py')
    assert m.ROUTES == base.ROUTES and tuple(m.CASES) == base.CASE_KEYS and m.END_ROUTES == END_ROUTES
    m.with_nchw_ends()
    assert tuple(m.CASES) == base.CASE_KEYS + END_KEYS and m.ROUTES == base.ROUTES + ('nchw_in',) and m.GATE_FAMILIES == GATE_FAMILIES
    return m


# ---- 1. reach --------------------------------------------------------------------------------------------------------------------------------
def test_the_cases_reach_all_three_first_conv_implementations_and_both_few_cout_instantiations(gc):
    forms = {(r, f) for key in END_KEYS for _, _, r, f in gc.launches(key)}
    assert forms == FORMS and {r for r, _ in forms} == set(END_ROUTES)
    assert all(len(gc.launches(key)) == 1 for key in END_KEYS)


# ---- 2. the exact and the impulse families -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', END_KEYS)
def test_int_coded_is_the_fp64_result_bitwise(gc, key):
    base.test_int_coded_is_the_fp64_result_bitwise(gc, key)


@pytest.mark.parametrize('key', END_KEYS)
def test_onehot_pixels_select_the_weight(gc, key):
    base.test_onehot_pixels_select_the_weight(gc, key)


@pytest.mark.parametrize('key', END_KEYS)
def test_tap_shift_moves_the_input(gc, key):
    """Per tap a signed channel permutation of the shifted input under zero padding: bitwise, and with nm3b's SFT epilogue (which rounds more than
    once) within the gate."""
    g = gc.CASES[key]
    if g.epi != gc.EPI_SFT:
        return base.test_tap_shift_moves_decimates_or_permutes_the_input(gc, key)
    (cname, code, route, form), = gc.launches(key)
    for tap in range(9):
        d, ref, tol = gc.prepared('tap_shift', key, route, form, tap)
        r, err = gc.ratio(gc.run(d, key, code, ('tap_shift', key, tap, d['epi'])), ref, tol)
        assert r <= 1.0, (key, tap, route, form, r, err)


# ---- 3. the gate families --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family,route', [(f, r) for f in GATE_FAMILIES for r in END_ROUTES if not f.startswith('swish') and not (f == 'mixed_cin' and r == 'nchw_in')])
def test_family_within_the_gate(gc, family, route):
    """As tests/test_gpu_conv_geom.py, over the new cases of a route.  (in_nchw has no prologue: no mixed_cin; neither end has the swish families' point.)"""
    worst, emu, n = 0.0, 0.0, 0
    for key in END_KEYS:
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


# ---- 4. masked edge tiles ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', ('h1a16', 'h2a32', 'h4a64', 'h3a32'))
def test_masked_edge_tiles_write_inside_the_tensor_only(gc, key):
    """21x37 planes as a view into a larger NaN-filled allocation with guard rows behind it: the bits of the launch into a tensor of its own, the guard untouched."""
    import torch
    g = gc.CASES[key]
    (cname, code, route, form), = gc.launches(key)
    fam = 'mixed_cout' if gc.buildable('mixed_cout', g) else 'dc_plus_ripple'        # (one output channel has no exponents to spread)
    d, _, _ = gc.prepared(fam, key, route, form)
    n, guard = g.B * g.H * g.W * g.cout, 4 * 16 * g.W * 32
    big = torch.full((n + guard,), float('nan'), device='cuda')
    y = gc.run(d, key, code, (fam, key), out=big[:n].view(g.B, g.cout, g.H, g.W))
    own = gc.run(d, key, code, (fam, key))
    assert bool(torch.isfinite(own).all()) and gc.bits_equal(y.contiguous(), own.contiguous()), (key, route, form)
    assert bool((big[n:].view(torch.int32) == NAN_BITS).all()), (key, route, form)


# ---- 5. containment ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', ('n3a', 'n1b', 'n4a', 'nm3a', 'h1a16', 'h4b64', 'h3a32'))
def test_a_non_finite_pixel_reaches_exactly_the_outputs_whose_window_holds_it(gc, key):
    """One NaN, then one +inf, in a single pixel and channel of the FIRST image -- at (0, 0) first: it reaches exactly the outputs of the 3x3 window under zero
    padding and no other image; every other output keeps the clean run's bits.  The head runs with the affine prologue (sc = 1, sh = 0), the input end has none."""
    import torch
    g = gc.CASES[key]
    (cname, code, route, form), = gc.launches(key)
    base_d = gc.family_of('cancel_pairs', key, route, form) or gc.family_of('mixed_cout', key, route, form)       # (an odd channel count has no pairs)
    assert bool((base_d['w'] != 0).all())
    d = dict(base_d, pro=gc.PRO_AFFINE, sc=torch.ones_like(base_d['sc']), sh=torch.zeros_like(base_d['sh'])) if route == 'head' else base_d
    tag = ('contain', key, d['epi'])
    clean = gc.run(d, key, code, tag)
    assert bool(torch.isfinite(clean).all())
    for val in (float('nan'), float('inf')):
        for i, (r, q) in enumerate(((0, 0), (1, 1), (4, 5), (7, 15), (g.H - 1, 9))):
            x = d['x'].clone()
            x[0, r, q, (7 * i + 3) % g.cin] = val
            y = gc.run(d, key, code, tag, x=x)
            reach = gc.expected_reach(g, route, form, r, q).cuda()
            same = (y.contiguous().view(torch.int32) == clean.contiguous().view(torch.int32)).all(dim=3)
            assert bool(same[1:].all()) and bool(same[0][~reach].all()), (key, form, val, (r, q), int((~same[0][~reach]).sum()))
            assert bool((~torch.isfinite(y[0][reach])).all()), (key, form, val, (r, q), int(torch.isfinite(y[0][reach]).sum()))


# ---- 6. invariance -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('route', END_ROUTES)
def test_a_launch_repeats_bitwise_and_an_image_alone_equals_the_image_in_a_batch(gc, route):
    base.test_a_launch_repeats_bitwise_and_an_image_alone_equals_the_image_in_a_batch(gc, route)


# ---- 7. the input end: statistics, the two forms of one launch, the refusal ------------------------------------------------------------------------
@pytest.mark.parametrize('key', NCHW_KEYS[:8])
def test_first_conv_statistics_describe_the_tensor_that_was_written(gc, key):
    """The vector kernel with emit_stats (two channels per group): the tensor is bitwise the launch without statistics, and every group's sum and sum
    of squares is the fp64 sum over that tensor within conv_geom_check.stats_ratio's bound (sixteen fp32 additions per thread, then fp64)."""
    for family in ('mixed_cout', 'dc_plus_ripple'):
        (cname, code, route, form), = gc.launches(key)
        d, ref, tol = gc.prepared(family, key, route, form)
        y = gc.run(d, key, code, (family, key, 0, d['epi']), stats=True)
        plain = gc.run(d, key, code, (family, key, 0, d['epi']))
        st = y._cf_stats
        assert st.cpg == 2 and st.parts == 4 * (gc.CASES[key].H // 16) * (gc.CASES[key].W // 16)
        assert gc.bits_equal(y.contiguous(), plain.contiguous()) and gc.ratio(y, ref, tol)[0] <= 1.0
        r = gc.stats_ratio(y)
        print(f'{family} {key} {form}: statistics |error| / bound {r:.4f}')
        assert r <= 1.0, (family, key, form, r)


@pytest.mark.parametrize('key', ('n3a', 'n3b', 'n4a', 'n1b'))
def test_the_vector_and_the_mfma_form_of_the_first_conv_both_meet_fp64(gc, key):
    """The same tensors through conv3x3_few_cin_kernel (no epilogue) and through launch<9,1,4,1,2,2,true> (a residual of zeros sends the launch there and
    adds nothing): each within its gate of the fp64 result.  They are NOT required to agree bitwise -- the vector kernel starts its FMA chain at the bias,
    the MFMA form adds the bias last -- and the count of differing elements is printed."""
    import torch
    (cname, code, route, form), = gc.launches(key)
    assert form in ('few_cin 3', 'few_cin n')
    for family in ('mixed_cout', 'dc_plus_ripple', 'int_coded'):
        d, ref, tol = gc.prepared(family, key, route, form)
        vec = gc.run(d, key, code, (family, key, 0, d['epi']))
        dm = dict(d, epi=gc.EPI_RESIDUAL, res=torch.zeros_like(d['res']))
        mf = gc.run(dm, key, code, (family, key, 0, d['epi']))
        tol_m = gc.gate_of(dm, gc.CASES[key], route, gc.reference(dm, gc.CASES[key]), 'mfma')
        rv, rm = gc.ratio(vec, ref, tol)[0], gc.ratio(mf, ref, tol_m)[0]
        differ = int((vec != mf).sum())
        print(f'{family} {key}: vector {rv:.4f} of its gate, mfma {rm:.4f} of its gate, {differ} of {vec.numel()} elements differ between the two')
        assert rv <= 1.0 and rm <= 1.0, (family, key, rv, rm)
        if family == 'int_coded':
            assert differ == 0 and torch.equal(vec.cpu().double(), ref['out'])


def test_the_first_conv_off_the_16x16_tile_grid_is_refused(gc):
    """What the first run found: no in_nchw launch exists off the 16x16 tile grid.  The vector kernel owns whole tiles, and the MFMA instantiation that
    takes everything else is not an EXT one (EXT reads NHWC only), so 17x19 and 24x40 -- sizes the network never has at its input -- end in the tile
    check of launch<> with a message, before any launch.  The same weight on the next whole-tile size runs."""
    import torch
    from codeformer_amd import ops
    d = gc.family('mixed_cout', 'n3a')
    pw = gc.packed(d, gc.CASES['n3a'], 0, ('mixed_cout', 'n3a', 0, d['epi']))
    for g in gc.OFF_GRID_NCHW:
        x = torch.zeros(g.B, g.cin, g.H, g.W, device='cuda')
        with pytest.raises(RuntimeError, match='not divisible by the 16x16 tile'):
            ops.conv2d(x, pw, in_nchw=True)
        with pytest.raises(RuntimeError, match='not divisible by the 16x16 tile'):
            ops.conv2d(x, pw, in_nchw=True, epilogue=gc.EPI_RESIDUAL, res=torch.zeros(g.B, g.H, g.W, 64, device='cuda'))
    y = ops.conv2d(torch.zeros(2, 3, 32, 48, device='cuda'), pw, in_nchw=True)
    assert tuple(y.shape) == (2, 32, 48, 64) and bool(torch.isfinite(y).all())
