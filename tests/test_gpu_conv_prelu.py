"""-m gpu: the five PReLU convolution instantiations (igemm_kernel<.., PRELU = true> behind CF_EPI_PRELU / CF_EPI_RES_PRELU) per element.

The thirteen cases are PRELU_CASES of tools/conv_geom_check.py, merged into a module object of its own (with_prelu()); the route `prelu`, its forms `s2`,
`narrow`, `128`, `64`, `32`, the reference, the gate terms and the emulation are that file's, the proofs on the reference alone are in
tests/test_conv_prelu_host.py, and the tests of tests/test_gpu_conv_geom.py that fit a case unchanged are called from here.  What that file pins (ROUTES,
FORMS, CASE_KEYS, its figures) is untouched.  Slopes: arcface_ref.SLOPES, -0.5, 0, 0.25, 1.5; every form sees a negative one and one above one.

Measured on an MI355X: the whole file 3.5 s, 54 tests, none above 0.4 s (int_coded[q64a], which builds the 19x35 references first).  Largest |error| / gate per family, kernel | CPU emulation:
    mixed_cout 0.4333 | 0.4333   mixed_cin 0.0403 | 0.0162   mixed_cin_act 0.0440 | 0.0182   cancel_pairs 0.0020 | 0.0046   dc_plus_ripple 0.0109 | 0.0089
    swish_leaky_edges 0.3609 | 0.3609 (on the RES_PRELU cases, whose epilogue adds the family's residual)   swish_leaky_edges_sft - (EXT has no SFT)
    onehot_pixels 0.4312
(mixed_cout and swish_leaky_edges: the residual add of q64b / q128b, one rounding both evaluations make alike.)  int_coded is bitwise with prologue none and
affine, tap_shift bitwise the float32 definition on all nine taps.  Everything held on the first run; the `128` and `32` instantiations had never been
launched before (the network and the block tests reach `64`, `narrow` and `s2` only).  That the affine prologue's SHIFT does not reach the zero padding is
int_coded's (variant 1, sh != 0, bitwise) and the gates' to show: edit p3.

Scratch builds with one in-range edit each (not committed; addresses, barriers and launch geometry untouched), each run once through these tests and
tests/test_gpu_arcface.py.  Tests of this file that fail | old (the yardstick tests of tests/test_gpu_arcface.py):
  (p1) cf_igemm.hip PReLU epilogue written as max(t, a t)               21: int_coded, onehot_pixels, tap_shift on the five cases of slope 1.5 (q64b q32a qnb q128b qs0), the six
                                                                      gates | old: the network r18 and the five blocks at slope 1.5 (the max IS the select for a <= 1)
  (p2) cf_igemm.hip RES_PRELU: the residual added after the select     24: int_coded, onehot_pixels, tap_shift on the six RES_PRELU cases, the six gates | old: r18, 12 block cases
  (p3) cf_igemm.hip affine prologue: the padding takes the shift        19: int_coded on all thirteen cases, the six gates (and int_coded on fifteen cases, nine gates and a solo
         (y kept where the pixel is outside the image)                  gate of tests/test_gpu_conv_geom.py) | old: both networks, all 20 block cases
Plainly: all three are gross and the old yardstick tests of the network and the blocks catch them too, at the slopes and shapes they run; this file adds
which epilogue, form, case and slope -- and covers the `128` and `32` forms, which no old test launches.
"""
import pytest

import test_gpu_conv_geom as base
from _tools import load_script

pytestmark = pytest.mark.gpu

PRELU_KEYS = ('q64a', 'q64b', 'q64c', 'q32a', 'q32b', 'q32c', 'qna', 'qnb', 'q128a', 'q128b', 'qs0', 'qs1', 'qs1p')
FORMS = {('prelu', 's2'), ('prelu', 'narrow'), ('prelu', '128'), ('prelu', '64'), ('prelu', '32')}
GATE_FAMILIES = ('mixed_cout', 'mixed_cin', 'mixed_cin_act', 'cancel_pairs', 'dc_plus_ripple', 'swish_leaky_edges')      # (EXT has no SFT)
CONTAIN = ('q64c', 'q32b', 'qnb', 'q128b', 'qs0', 'qs1')


@pytest.fixture(scope='module')
def gc():
    import torch
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    from codeformer_amd import lib
    lib.load()
    m = load_script('tools/conv_geom_check.py')
    assert m.ROUTES == base.ROUTES and tuple(m.CASES) == base.CASE_KEYS
    m.with_prelu()
    assert tuple(m.CASES) == base.CASE_KEYS + PRELU_KEYS and m.ROUTES == base.ROUTES + ('prelu',) and set(GATE_FAMILIES) < set(m.GATE_FAMILIES)
    return m


# ---- 1. reach --------------------------------------------------------------------------------------------------------------------------------
def test_the_cases_reach_all_five_prelu_instantiations(gc):
    forms = {(r, f) for key in PRELU_KEYS for _, _, r, f in gc.launches(key)}
    assert forms == FORMS and all(len(gc.launches(key)) == 1 for key in PRELU_KEYS)
    for form in ('s2', 'narrow', '128', '64', '32'):      # every form sees a negative slope and one above one, and both epilogues
        mine = [gc.CASES[k] for k in PRELU_KEYS if gc.launches(k)[0][3] == form]
        assert min(g.alpha for g in mine) < 0 and max(g.alpha for g in mine) > 1 and {g.epi for g in mine} == set(gc.PRELU_EPIS), form


# ---- 2. the exact and the impulse families -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', PRELU_KEYS)
def test_int_coded_is_the_fp64_result_bitwise(gc, key):
    """Prologue none and affine (ArcFace's conv2 and conv1 pairings); the slopes have two significant bits, so a t is exact."""
    base.test_int_coded_is_the_fp64_result_bitwise(gc, key)


@pytest.mark.parametrize('key', PRELU_KEYS)
def test_onehot_pixels_select_the_weight(gc, key):
    base.test_onehot_pixels_select_the_weight(gc, key)


@pytest.mark.parametrize('key', PRELU_KEYS)
def test_tap_shift_is_bitwise_the_float32_definition(gc, key):
    """pre is +-x, exact: t = fl(pre + res) and fl(a t) are each what float32 does, so the output is conv_geom_check.prelu32 bit for bit, on every tap."""
    (cname, code, route, form), = gc.launches(key)
    for tap in range(9):
        d, ref, _ = gc.prepared('tap_shift', key, route, form, tap)
        assert bool((ref['pre'].float().double() == ref['pre']).all())
        got = gc.run(d, key, code, ('tap_shift', key, tap, d['epi']))
        assert gc.bits_equal(got.cpu() + 0.0, gc.prelu32(d, ref['pre'].float()) + 0.0), (key, tap, route, form)


# ---- 3. the gate families --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', GATE_FAMILIES)
def test_family_within_the_gate(gc, family):
    """As tests/test_gpu_conv_geom.py, over the cases of the route: every ratio printed, at most 1, and not below 1e-3 of the emulation's."""
    worst, emu, n = 0.0, 0.0, 0
    for key in PRELU_KEYS:
        (cname, code, route, form), = gc.launches(key)
        r = gc.case(family, key, code, route, form)
        if r is None:
            continue
        print(f'{family} {key} {route} {cname} {form}: max|d| {r["err"]:.3e} = {r["ratio"]:.4f} of the gate | emulation {r["emu_err"]:.3e} = {r["emu_ratio"]:.4f}')
        assert r['ratio'] <= 1.0, (family, key, route, cname, form, r)
        worst, emu, n = max(worst, r['ratio']), max(emu, r['emu_ratio']), n + 1
    assert n >= (6 if family == 'swish_leaky_edges' else 13) and emu > 0.0
    assert worst >= 1e-3 * emu, (family, worst, emu)
    print(f'TABLE {family} prelu {worst:.4f} {emu:.4f}')


# ---- 4. masked edge tiles ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', ('q64b', 'q32a', 'q128a', 'qs0', 'qs1'))
def test_masked_edge_tiles_write_inside_the_tensor_only(gc, key):
    base.test_masked_edge_tiles_write_inside_the_tensor_only(gc, key)


# ---- 5. containment ----------------------------------------------------------------------------------------------------------------------------
def test_a_non_finite_pixel_reaches_exactly_the_outputs_whose_window_holds_it(gc):
    """As tests/test_gpu_conv_geom.py (affine prologue with sc = 1, sh = 0; one NaN, then one +inf, at five spots of the first image), on every form.
    The PReLU epilogues launder nothing: NaN > 0 is false and a NaN is NaN; +inf passes; -inf gives a (-inf), which is +-inf for a != 0 and NaN for the
    slope 0 of q64c -- non-finite in every case, so the reach is the definition's window, and every other output keeps the clean run's bits."""
    import torch
    forms = set()
    for key in CONTAIN:
        g = gc.CASES[key]
        (cname, code, route, form), = gc.launches(key)
        base_d = gc.family_of('cancel_pairs', key, route, form)
        assert bool((base_d['w'] != 0).all())
        d = dict(base_d, pro=gc.PRO_AFFINE, sc=torch.ones_like(base_d['sc']), sh=torch.zeros_like(base_d['sh']))
        tag = ('contain', key, d['epi'])
        clean = gc.run(d, key, code, tag)
        assert bool(torch.isfinite(clean).all())
        spots = dict.fromkeys([(0, 0), (1, 1), (4, min(5, g.W - 2)), (min(7, g.H - 2), min(15, g.W - 2)), (g.H - 1, min(9, g.W - 1))])
        for val in (float('nan'), float('inf')):
            for i, (r, q) in enumerate(spots):
                x = d['x'].clone()
                x[0, r, q, (7 * i + 3) % g.cin] = val
                y = gc.run(d, key, code, tag, x=x)
                reach = gc.expected_reach(g, route, form, r, q).cuda()
                same = (y.contiguous().view(torch.int32) == clean.contiguous().view(torch.int32)).all(dim=3)
                assert bool(same[1:].all()) and bool(same[0][~reach].all()), (key, form, val, (r, q), int((~same[0][~reach]).sum()))
                assert bool((~torch.isfinite(y[0][reach])).all()), (key, form, val, (r, q), int(torch.isfinite(y[0][reach]).sum()))
        forms.add(form)
    assert forms == {'s2', 'narrow', '128', '64', '32'} and gc.CASES['q64c'].alpha == 0.0


# ---- 6. invariance -----------------------------------------------------------------------------------------------------------------------------
def test_a_launch_repeats_bitwise_and_an_image_alone_equals_the_image_in_a_batch(gc):
    assert gc.cases_of('prelu') == list(PRELU_KEYS)
    base.test_a_launch_repeats_bitwise_and_an_image_alone_equals_the_image_in_a_batch(gc, 'prelu')


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_the_prelu_epilogues_refuse_every_launch_without_an_instantiation(gc):
    """The two PReLU epilogues exist in five general fp32 3x3 instantiations and nowhere else: every other request is refused by conv_validate, before
    any launch, with the message cf_igemm.hip gives."""
    import torch
    from codeformer_amd import ops
    d = gc.family('mixed_cout', 'q64a')
    w, b, x = d['w'].cuda(), d['b'].cuda(), d['x'].cuda()
    kw = dict(epilogue=gc.EPI_PRELU, sft_w=0.25)
    general = 'strided slices / leaky.axpy epilogues / off-grid sizes'
    with pytest.raises(RuntimeError, match='the PReLU epilogues belong to the general fp32'):
        ops.conv2d(x, ops.pack_weight(w, b, bf16=ops.WINOGRAD), **kw)
    with pytest.raises(RuntimeError, match=general):
        ops.conv2d(x, ops.pack_weight(w, b, bf16=True), **kw)
    with pytest.raises(RuntimeError, match='the PReLU epilogues are built for plain 3x3 convs with fp32 operands'):
        ops.conv2d(x, ops.pack_weight(w, b, f16=True), **kw)
    with pytest.raises(RuntimeError, match='the PReLU epilogues are built for plain 3x3 convs with fp32 operands'):
        ops.conv2d(x, ops.pack_weight(w, b, up2x=True), upsample=True, **kw)
    pw = ops.pack_weight(w, b)
    with pytest.raises(RuntimeError, match='NCHW output supports no epilogue op or statistics'):
        ops.conv2d(x, pw, out_nchw=True, **kw)
    with pytest.raises(RuntimeError, match=general):
        ops.conv2d(torch.zeros(2, 3, 19, 35, device='cuda'), ops.pack_weight(w[:, :3].contiguous(), b), in_nchw=True, **kw)
    assert pw.cout_pad == 64
    with pytest.raises(RuntimeError, match=general):
        ops.conv2d(torch.zeros(2, 20, 36, 32, device='cuda'), pw, stride=2, pad_lo=1, **kw)
    y = ops.conv2d(x, pw, **kw)      # (the request itself is served)
    assert bool(torch.isfinite(y).all())
