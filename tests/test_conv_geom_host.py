"""CPU: the evidence that the conditions of tests/test_gpu_conv_geom.py are conditions on the REFERENCE, not on what a kernel returns.

For the cases of tools/conv_geom_check.py (stride 2, 1x1, the EXT instantiations, the dense 32-wide rung, the NCHW head):
  * route_of() against a literal table of (route, form) per case and code, every form of the issue's table reached; the library's own validation
    (cf_conv2d_stats_parts: a launch up to the point where a kernel would start) accepts every launch it can be asked about and refuses the named
    out-of-rule neighbours.  Two routes it cannot be asked about as launched: `head` -- a query passes the few-channel kernel by (it emits no
    statistics) and lands on the 32-wide rung, so the query is made at the next whole-tile size, 32x48, and shows conv_validate's part only -- and
    `c1_dsplit` -- conv_validate answers no query for the streaming 1x1, so the test asserts that refusal and the host rule ops.split_1x1_ok.  Which
    kernel template runs is route_of()'s restatement of the launchers, not something a query reports;
  * the fp64 reference against an index-by-index loop on the smallest case of every padding rule;
  * int_coded: the exactness preconditions on every route and variant, and the emulation returns the fp64 result bitwise;
  * every gate family's emulation within 0.5 of its gate, on every route and case the GPU test uses; onehot_pixels and tap_shift likewise;
  * cancel_pairs is ill-conditioned (median S / |pre| >= 100); the one-hot pixels sit where the docstring says.
"""
import ctypes

import pytest
import torch

from _tools import load_script


@pytest.fixture(scope='module')
def gc():
    return load_script('tools/conv_geom_check.py')


CASE_KEYS = ('s2a', 's2b', 's2c', 's2d', 's2z', 's2r', 'p1a', 'p1b', 'p1c', 'p1d', 'e1z', 'e1r', 'e2z', 'e2r', 'e3z', 'e3r', 'sl', 'epl', 'epa', 'epa2',
             'u1z', 'u1e', 'u2z', 'u2e', 'd32', 'hd')
EXPECTED = {
    's2a': {'F32': ('s2_d32', '64-wide'), 'SPLIT': ('s2_dsplit', '64-wide no-skip')},
    's2b': {'F32': ('s2_d32', '64-wide'), 'SPLIT': ('s2_dsplit', '64-wide skip')},
    's2c': {'F32': ('s2_d32', '128-wide'), 'SPLIT': ('s2_dsplit', '128-wide')},
    's2d': {'F32': ('s2_d32', '64-wide'), 'SPLIT': ('s2_dsplit', '64-wide skip')},
    's2z': {'F32': ('s2_d32', 'ext')}, 's2r': {'F32': ('s2_d32', 'ext')},
    'p1a': {'F32': ('c1_d32', '256x64'), 'SPLIT': ('c1_dsplit', '64-wide')},
    'p1b': {'F32': ('c1_d32', '128x128'), 'SPLIT': ('c1_dsplit', '64-wide')},
    'p1c': {'F32': ('c1_d32', '128x128'), 'SPLIT': ('c1_dsplit', '128-wide')},
    'p1d': {'F32': ('c1_d32', 'narrow 128x64')},
    'e1z': {'F32': ('ext_d32', '64')}, 'e1r': {'F32': ('ext_d32', '64')}, 'e2z': {'F32': ('ext_d32', '128')}, 'e2r': {'F32': ('ext_d32', '128')},
    'e3z': {'F32': ('ext_d32', '32')}, 'e3r': {'F32': ('ext_d32', '32')},
    'sl': {'F32': ('ext_d32', '64')}, 'epl': {'F32': ('ext_d32', '64')}, 'epa': {'F32': ('ext_d32', '64')}, 'epa2': {'F32': ('ext_d32', '64')},
    'u1z': {'F32': ('ext_up', '64')}, 'u1e': {'F32': ('ext_up', '64')}, 'u2z': {'F32': ('ext_up', '128')}, 'u2e': {'F32': ('ext_up', '128')},
    'd32': {'F32': ('d32_32', '256x32')},
    'hd': {'F32': ('head', 'few_cout reflect')},
}
ISSUE_FORMS = {('s2_d32', '64-wide'), ('s2_d32', '128-wide'), ('s2_d32', 'ext'), ('s2_dsplit', '64-wide skip'), ('s2_dsplit', '64-wide no-skip'),
               ('s2_dsplit', '128-wide'), ('c1_d32', '256x64'), ('c1_d32', '128x128'), ('c1_d32', 'narrow 128x64'), ('c1_dsplit', '64-wide'),
               ('c1_dsplit', '128-wide'), ('ext_d32', '128'), ('ext_d32', '64'), ('ext_d32', '32'), ('ext_up', '128'), ('ext_up', '64'),
               ('d32_32', '256x32'), ('head', 'few_cout reflect')}


def test_cases_are_the_issue_s_and_none_is_larger(gc):
    assert tuple(gc.CASES) == CASE_KEYS
    for key, g in gc.CASES.items():
        Ho, Wo = gc.out_hw(g)
        assert g.B * g.H * g.W * g.cin <= 128 * 128 * 32 and g.B * Ho * Wo * g.cout <= 64 * 64 * 384 and g.B <= 2, key
    assert tuple(gc.CASES['s2a'][:5]) == (2, 32, 32, 16, 64) and tuple(gc.CASES['s2c'][:5]) == (1, 128, 128, 32, 384)
    assert tuple(gc.CASES['p1b'][:6]) == (2, 32, 48, 96, 128, 64) and tuple(gc.CASES['hd'][:5]) == (2, 21, 37, 32, 3)
    assert gc.SLICE == dict(x=(80, 16), x2=(48, 0), out=(128, 32)) and gc.CASES['sl'].sliced


def test_routes_against_the_literal_table(gc):
    got = {key: {n: (r, f) for n, _, r, f in rows} for key, rows in gc.routes().items()}
    assert got == EXPECTED
    forms = {rf for rows in got.values() for rf in rows.values()}
    assert forms == ISSUE_FORMS and {r for r, _ in forms} == set(gc.ROUTES)
    # the concatenated 1x1 has an odd slab count, the single-input ones one slab
    assert (gc.CASES['p1b'].cin // 32) % 2 == 1 and gc.CASES['p1b'].c_split == 64
    # refusals: no route
    from codeformer_amd import ops
    G = gc.G
    assert gc.route_of(0, G(2, 20, 36, 32, 64, stride=2, pad_lo=1)) is None                           # stride 2 EXT at cout_pad 64
    assert gc.route_of(ops.SPLIT, G(2, 32, 32, 32, 128, stride=2, pad_lo=1)) is None                 # split-half stride 2 with pad_lo = 1
    assert gc.route_of(ops.SPLIT, G(2, 32, 32, 32, 64, taps=1)) is None                              # the streaming 1x1 at <= 1024 pixels
    assert gc.route_of(0, G(2, 16, 16, 32, 64, pad_mode=gc.PAD_EDGE)) is None                        # PAD_EDGE without upsample
    assert gc.route_of(0, G(2, 16, 16, 32, 64, epi=gc.EPI_SFT, sliced=True)) is None and gc.route_of(0, G(1, 24, 24, 16, 64, taps=1)) is None
    # a dense shape on whole tiles belongs to conv_check
    assert gc.route_of(0, G(2, 16, 32, 32, 64)) == ('d32', '256x64') and gc.route_of(ops.SPLIT, G(2, 16, 32, 32, 64)) == ('dsplit', 'form 0 64-wide')


def _desc(gc, g, code, **over):
    """The descriptor ops.conv2d builds for a case (a query dereferences nothing: every pointer the checks want present is a dummy)."""
    from test_conv_dispatch_host import D
    from codeformer_amd import lib, ops
    dummy = ctypes.create_string_buffer(64)
    p = ctypes.addressof(dummy)
    c0 = g.cin if g.c_split is None else g.c_split
    cp = g.cout if code == ops.SPLIT else max(64, ops._cout_pad(g.cout)) if g.up else ops._cout_pad(g.cout)
    epi = g.epi or 0
    kw = dict(taps=g.taps, stride=g.stride, upsample=int(g.up), bf16_mfma=ops.OPERAND_F16X2 if code == ops.SPLIT else 0, batch=g.B, stats_cpg=0, c1=g.cin - c0,
              acc_scale=1.0, in0=p, in1=p if g.cin - c0 else None, pad_mode=g.pad_mode, pad_lo=g.pad_lo, out_nchw=int(g.out_nchw), epilogue=epi,
              res=p if epi in (gc.EPI_AXPY, gc.EPI_AXPY2) else None, sft_scale=p if epi == gc.EPI_AXPY2 else None)
    if g.sliced:
        kw.update(ld_in0=gc.SLICE['x'][0], ld_in1=gc.SLICE['x2'][0], ld_out=gc.SLICE['out'][0])
    kw.update(over)
    d = lib.ConvDesc(**D(g.H, g.W, c0, g.cout, cp, **kw))
    d._keep = dummy
    return d


def test_the_library_accepts_every_launch_and_refuses_the_neighbours(gc):
    from codeformer_amd import build as cf_build
    from codeformer_amd import lib, ops
    cf_build.build()
    native = lib.load()
    dummy = ctypes.create_string_buffer(64)

    def query(g, code, **over):
        d = _desc(gc, g, code, **over)
        return native.cf_conv2d_stats_parts(ctypes.byref(d)), lib.last_error()

    for key, rows in gc.routes().items():
        g = gc.CASES[key]
        for cname, code, route, form in rows:
            if route == 'c1_dsplit':      # conv_validate answers no query for the streaming 1x1 (it emits no statistics); its own rules: below
                got, err = query(g, code)
                assert got <= 0 and 'no statistics epilogue' in err, (key, err)
                assert ops.split_1x1_ok(g.cin, g.cout, g.H, g.W, g.c_split)
                continue
            if route == 'head':           # a query passes the few-channel kernel by (no statistics) and lands on the 32-wide rung, which wants whole tiles:
                g = g._replace(H=32, W=48)      # conv_validate's part (reflect + out_nchw, cout_pad 32) is what the query can show, on the next whole-tile size
            got, err = query(g, code)
            assert got > 0, (key, cname, route, form, err)
    G = gc.G
    # the named out-of-rule neighbours
    got, err = query(G(2, 20, 36, 32, 64, stride=2, pad_lo=1), 0)
    assert got <= 0 and 'strided slices' in err, err
    got, err = query(G(2, 32, 32, 32, 128, stride=2), ops.SPLIT, pad_lo=1)
    assert got <= 0 and 'padding bottom / right' in err, err
    got, err = query(G(2, 32, 32, 16, 64, stride=2), ops.SPLIT, prologue=gc.PRO_AFFINE, pro_scale=ctypes.addressof(dummy), pro_shift=ctypes.addressof(dummy))
    assert got <= 0 and 'stride 2 takes prologue none / leaky' in err, err      # (its [batch][c0] tables would be indexed by the 4 c0 channels of the view)
    assert gc.int_coded_variants('s2a', 's2_dsplit', '64-wide no-skip') == (0, 3) and gc.prepared('mixed_cout', 's2a', 's2_dsplit', '64-wide no-skip')[0]['pro'] == gc.PRO_NONE
    got, err = query(G(2, 16, 16, 32, 64), 0, pad_mode=gc.PAD_EDGE)
    assert got <= 0 and 'edge padding belongs to the folded upsample' in err, err
    got, err = query(G(2, 16, 16, 32, 64, epi=gc.EPI_LEAKY), ops.SPLIT)
    assert got <= 0 and 'epilogues are none / residual / SFT' in err, err
    # the streaming 1x1 at <= 1024 pixels: the C ABI reads such a descriptor as a token GEMM, so the refusal is the host's, before any launch
    pw = ops.PackedWeight(None, None, 64, 32, 1, 64, 32, bf16=ops.OPERAND_F16X2, conv1=True)
    with pytest.raises(ValueError, match='1x1'):
        ops.conv2d(torch.zeros(2, 32, 32, 32), pw)
    assert not ops.split_1x1_ok(32, 64, 32, 32)


def _loop_reference(gc, d, g):
    """The convolution of a case index by index: every output pixel, every tap, the padding rule as a coordinate map written out here."""
    p, _ = gc.prologue64(dict(d, up=False))
    B, H, W, cin = p.shape
    Ho, Wo = gc.out_hw(g)
    n_h, n_w = (2 * H, 2 * W) if g.up else (H, W)          # the size of the image the 3x3 window moves over
    w = d['w'].double()
    out = d['b'].double().expand(B, Ho, Wo, g.cout).clone()
    pad = g.pad_lo if g.stride == 2 else 1

    def src(i, n):
        if i < 0 or i >= n:
            if g.pad_mode == gc.PAD_ZERO:
                return None
            i = -i if i < 0 else 2 * n - 2 - i           # reflection, without the border pixel
        return i // 2 if g.up else i
    for oy in range(Ho):
        for ox in range(Wo):
            for ky in range(3):
                for kx in range(3):
                    iy, ix = src(oy * g.stride - pad + ky, n_h), src(ox * g.stride - pad + kx, n_w)
                    if iy is not None and ix is not None:
                        out[:, oy, ox] += p[:, iy, ix] @ w[:, :, ky, kx].t()
    return out


@pytest.mark.parametrize('key', ('e3z', 'e3r', 's2a', 's2z', 's2r', 'u1z', 'u1e', 'hd'))
def test_reference_against_an_index_by_index_loop(gc, key):
    """The smallest case of every padding rule: zero and reflect at stride 1, bottom / right and both-sided zero and reflect at stride 2, zero and
    edge under the upsample, reflect on the head."""
    g = gc.CASES[key]
    for fam in ('dc_plus_ripple', 'onehot_pixels'):
        d = gc.family(fam, key)
        ref = gc.reference(d, g)
        want = _loop_reference(gc, d, g)
        S = gc._abs_eval(d, g)[0]
        assert bool(((ref['pre'] - want).abs() <= 1e-13 * S + 1e-300).all()), (key, fam, float((ref['pre'] - want).abs().max()))
    if g.taps == 9 and not g.up and g.stride == 1:
        # the border tells the rules apart: under reflect padding dc_plus_ripple's constant cancels at the border, under zero padding it does not
        d = gc.family('dc_plus_ripple', key)
        edge = gc.reference(d, g)['pre'][:, 0].abs().mean()
        inner = gc.reference(d, g)['pre'][:, 2:-2, 2:-2].abs().mean()
        assert (edge < 4 * inner) if g.pad_mode == gc.PAD_REFLECT else (edge > 20 * inner), (key, float(edge), float(inner))


def test_taps_1_is_a_matrix_product_and_the_epilogues_are_the_header_s(gc):
    d = gc.family('mixed_cout', 'p1b')
    p, _ = gc.prologue64(dict(d, up=False))
    want = torch.einsum('bhwc,nc->bhwn', p, d['w'].double()[:, :, 0, 0]) + d['b'].double()
    assert float((gc.reference(d, gc.CASES['p1b'])['pre'] - want).abs().max()) <= 1e-13 * float(want.abs().max())
    for key, f in (('epl', lambda v, a, r, q: torch.where(v > 0, v, gc.SLOPE * v)), ('epa', lambda v, a, r, q: v * a + r),
                   ('epa2', lambda v, a, r, q: (v * a + r) * a + q)):
        d = gc.family('mixed_cout', key)
        ref = gc.reference(d, gc.CASES[key])
        a = float(torch.tensor(d['sft_w'], dtype=torch.float32))
        assert torch.equal(ref['out'], f(ref['pre'], a, d['res'].double(), d['ss'].double())), key
    assert gc.SLOPE == float(torch.tensor(0.2, dtype=torch.float32))


def _launches(gc, key):
    return [(code, route, form) for _, code, route, form in gc.launches(key)]


@pytest.mark.parametrize('key', CASE_KEYS)
def test_int_coded_preconditions_and_exact_emulation(gc, key):
    g = gc.CASES[key]
    for code, route, form in _launches(gc, key):
        worst = gc.exactness_preconditions(key, route, form)
        print(f'int_coded {key} {route} {form}: largest accumulator {worst:.0f} units < 2^24')
        variants = gc.int_coded_variants(key, route, form)
        assert variants and worst < 2 ** 24
        for v in variants:
            d, ref, _ = gc.prepared('int_coded', key, route, form, v)
            assert gc.bits_equal(gc.emulate(d, g, route) + 0.0, ref['out'].float() + 0.0), (key, route, form, v)
    # position-coded: a shifted input or two exchanged channels change the result
    d = gc.family('int_coded', key, 0)
    ref = gc.reference(d, g)
    assert not torch.equal(gc.reference(dict(d, x=torch.roll(d['x'], 1, dims=2)), g)['out'], ref['out'])
    xs = d['x'].clone()
    xs[..., [0, 1]] = xs[..., [1, 0]]
    assert not torch.equal(gc.reference(dict(d, x=xs), g)['out'], ref['out'])


@pytest.mark.parametrize('key', CASE_KEYS)
def test_emulation_within_half_of_the_gate(gc, key):
    """Every gate family of the case, onehot_pixels and tap_shift (the taps the GPU test runs), on every route the case reaches."""
    g = gc.CASES[key]
    n = 0
    for code, route, form in _launches(gc, key):
        fams = [(f, 0) for f in gc.families_of(key) + ('onehot_pixels',)] + [('tap_shift', t) for t in gc_taps(gc, key)]
        for fam, v in fams:
            if gc.prepared(fam, key, route, form, v) is None:
                continue
            r, err = gc.emulated(fam, key, route, form, v)
            print(f'{fam} {v} {key} {route} {form}: emulation max|d| {err:.3e} = {r:.3f} of the gate')
            assert r <= 0.5, (fam, v, key, route, form, r, err)
            n += 1
    assert n >= 4


SOLO_FAMILIES = ('solo_cin', 'solo_cin_act')
SOLO_ROUTES = ('s2_d32', 's2_dsplit', 'c1_d32', 'c1_dsplit')


@pytest.mark.parametrize('route', SOLO_ROUTES)
def test_solo_emulation_within_half_of_the_gate_and_the_dropped_lo_halves_far_above_it(gc, route):
    """Every case and form the GPU test launches.  On the split-half routes the emulation with the small activations' lo halves dropped
    (conv_check.drop_small_lo) exceeds the gate at least 10 times."""
    assert gc.SOLO_FAMILIES == SOLO_FAMILIES and gc.SOLO_ROUTES == SOLO_ROUTES and not set(SOLO_FAMILIES) & set(gc.GATE_FAMILIES)
    n = 0
    for key in gc.cases_of(route):
        g = gc.CASES[key]
        for _, code, rt, form in gc.launches(key, (route,)):
            for fam in SOLO_FAMILIES:
                pr = gc.prepared(fam, key, route, form)
                assert (pr is None) == (fam == 'solo_cin' and route == 's2_dsplit'), (fam, key, route)      # (the split-half stride-2 form refuses affine prologues)
                if pr is None:
                    continue
                d, ref, tol = pr
                live = gc.cc.live_channels(d)
                assert bool((live.sum(1) == 1).all()) and torch.equal(live.nonzero()[:, 1], gc.cc.solo_perm(g.cin, g.cout)) and bool(live.any(0).all())
                lo_sub, hi_sub = gc.cc.solo_kinds(d)
                assert bool((lo_sub.sum(1) >= 2).all()) and bool((hi_sub.sum(1) >= 2).all()), (fam, key)
                r, err = gc.emulated(fam, key, route, form)
                print(f'{fam} {key} {route} {form}: emulation max|d| {err:.3e} = {r:.3f} of the gate')
                assert r <= 0.5, (fam, key, route, form, r, err)
                if route in gc.SPLIT_ROUTES:
                    rd, _ = gc.ratio(gc.emulate(d, g, route, gc.cc.drop_small_lo), ref, tol)
                    print(f'{fam} {key} {route} {form}: small lo halves dropped {rd:.1f} of the gate')
                    assert rd >= 10.0, (fam, key, route, form, rd)
                n += 1
    assert n >= 3


def gc_taps(gc, key):
    g = gc.CASES[key]
    return (0,) if g.taps == 1 else (0, 4, 8) if key in gc.BIG else tuple(range(9))


def test_gate_families_apply_where_the_issue_says(gc):
    """The swish / leaky families run only on routes that take their epilogue; every route keeps at least five gate families."""
    for route in gc.ROUTES:
        fams = {f for key in gc.cases_of(route) for _, code, r, form in gc.launches(key, (route,)) for f in gc.families_of(key)
                if gc.prepared(f, key, r, form) is not None}
        assert {'mixed_cout', 'mixed_cin_act', 'cancel_pairs', 'dc_plus_ripple'} <= fams, (route, fams)
        assert ('mixed_cin' in fams) == (route != 's2_dsplit'), route                       # (the split-half stride-2 form refuses affine prologues)
        assert ('swish_leaky_edges_sft' in fams) == (route in ('s2_d32', 's2_dsplit', 'c1_d32', 'c1_dsplit', 'd32_32')), route
        assert ('swish_leaky_edges' in fams) == (route not in ('head', 's2_dsplit')), route
    assert gc.prepared('swish_leaky_edges_sft', 's2z', 's2_d32', 'ext') is None and gc.prepared('swish_leaky_edges', 'epl', 'ext_d32', '64') is None
    assert gc.prepared('dc_plus_ripple', 'hd', 'head', 'few_cout reflect')[0]['epi'] == gc.EPI_NONE


def test_hard_families_are_hard(gc):
    for key in CASE_KEYS:
        if key in gc.BIG:
            continue
        g = gc.CASES[key]
        d = gc.family('cancel_pairs', key)
        ref = gc.reference(d, g)
        cond = float((gc._abs_eval(d, g)[0] / ref['pre'].abs()).median())
        print(f'cancel_pairs {key}: median S / |pre| {cond:.3g}')
        assert cond >= 100 and torch.equal(d['x'][..., 0::2], d['x'][..., 1::2]), (key, cond)
        d = gc.family('dc_plus_ripple', key)
        assert float(d['w'].sum((2, 3) if g.taps == 9 else 1).abs().max()) <= 1e-5 and 250 < float(d['x'].mean()) < 262


def test_onehot_pixels_are_where_the_docstring_says(gc):
    for key, g in gc.CASES.items():
        per_image = [gc.onehot_positions(g, bi) for bi in range(g.B)]
        for pos in per_image:
            assert len(pos) == len(set(pos)) >= min(g.cin, 6), key
            assert all(max(abs(p[0] - q[0]), abs(p[1] - q[1])) >= 3 for i, p in enumerate(pos) for q in pos[:i])
            assert all(0 <= r < g.H and 0 <= q < g.W for r, q in pos)
        allp = {p for pos in per_image for p in pos}
        assert (0, 0) in per_image[0] and (g.H - 1, g.W - 1) in per_image[0]
        if g.B > 1 and min(g.H, g.W) >= 7:
            assert {(1, 1), (g.H - 2, g.W - 2)} <= set(per_image[1]), key                    # rows and columns 1 and n - 2
        if g.stride == 2:
            b = 16
            for side in ((b - 2, b - 1), (b, b + 1)):                                        # both sides of the first tile boundary, rows ...
                assert {(r % 2, q % 2) for r, q in allp if r in side} == {(0, 0), (0, 1), (1, 0), (1, 1)}, (key, side)
            if g.W > 32 and g.B * g.cin >= 128:                                               # (s2c has 32 pixels in all: its rows only)
                for side in ((30, 31), (32, 33)):                                            # ... and columns
                    assert {(r % 2, q % 2) for r, q in allp if q in side} == {(0, 0), (0, 1), (1, 0), (1, 1)}, (key, side)
        elif g.taps == 9 and min(g.H, g.W) >= 7:                                              # (9x5: one tile, and no room 3 away from both corners)
            last_r, last_c = 8 * ((g.H - 1) // 8), 16 * ((g.W - 1) // 16)                    # the last (partial) tile's boundary
            rows, cols = {r for r, _ in allp}, {q for _, q in allp}
            assert last_r == 0 or {last_r - 1, last_r} <= rows, (key, last_r, sorted(rows))
            assert last_c == 0 or {last_c - 1, last_c} <= cols, (key, last_c, sorted(cols))
    # the fp64 result IS the weight slice + bias where one weight meets a pixel (stride 2: decimated)
    for key in ('s2a', 'e3r', 'p1a'):
        g = gc.CASES[key]
        d = gc.family('onehot_pixels', key)
        ref = gc.reference(d, g)
        count = gc.conv64(gc.padded(d['x'].double().abs(), g), torch.ones_like(d['w'][:1]), g)[..., 0]
        assert int((count == 1).sum()) >= len(gc.onehot_positions(g, 0))
        bias = d['b'].double().expand_as(ref['out'])
        assert torch.equal(ref['out'][count == 0], bias[count == 0])                          # no pixel in the window: the bias alone
        flat = {float(v) for v in d['w'].double().flatten()}
        got = (ref['out'] - bias)[count == 1]                                                  # one weight meets the pixel: that weight, exactly
        assert all(float(v) in flat for v in got.flatten()[::7][:500])


def test_tap_shift_is_the_decimated_shift_and_a_signed_permutation(gc):
    p, sign = gc.cc.tap_perm(16, 64)
    g = gc.CASES['s2a']
    for tap in range(9):
        d = gc.family('tap_shift', 's2a', tap)
        ky, kx = tap // 3, tap % 3
        xp = torch.nn.functional.pad(d['x'].double(), (0, 0, 0, 1, 0, 1))
        want = xp[:, ky:ky + g.H:2, kx:kx + g.W:2][:, :g.H // 2, :g.W // 2][..., p] * sign.double()
        assert torch.equal(gc.reference(d, g)['out'] + 0.0, want + 0.0), tap
    g = gc.CASES['p1a']
    d = gc.family('tap_shift', 'p1a', 0)
    p, sign = gc.cc.tap_perm(g.cin, g.cout)
    assert torch.equal(gc.reference(d, g)['out'] + 0.0, d['x'].double()[..., p] * sign.double() + 0.0)


def test_expected_reach_is_the_window_and_the_documented_wider_one(gc):
    g = gc.CASES['s2a']
    # an even pixel: rows / columns 2 oy .. 2 oy + 2 hold it for two outputs per axis -- in both forms
    assert gc.expected_reach(g, 's2_d32', '64-wide', 4, 6).nonzero().tolist() == [[1, 2], [1, 3], [2, 2], [2, 3]]
    assert torch.equal(gc.expected_reach(g, 's2_dsplit', '64-wide no-skip', 4, 6), gc.expected_reach(g, 's2_d32', '64-wide', 4, 6))
    # an odd pixel: one output by the definition, the 2x2 space-to-depth window where the zero blocks are multiplied
    assert gc.expected_reach(g, 's2_d32', '64-wide', 5, 7).nonzero().tolist() == [[2, 3]]
    assert gc.expected_reach(g, 's2_dsplit', '64-wide skip', 5, 7).nonzero().tolist() == [[2, 3]]
    assert gc.expected_reach(g, 's2_dsplit', '64-wide no-skip', 5, 7).nonzero().tolist() == [[1, 2], [1, 3], [2, 2], [2, 3]]
    assert gc.expected_reach(g, 's2_dsplit', '64-wide no-skip', 0, 1).nonzero().tolist() == [[0, 0]]
    # reflection widens the set at the border by the outputs that read the pixel a second time; edge replication of the upsample does not reach further than zero padding
    gz, gr = gc.CASES['e3z'], gc.CASES['e3r']
    assert int(gc.expected_reach(gr, 'ext_d32', '32', 1, 1).sum()) == 9 and int(gc.expected_reach(gz, 'ext_d32', '32', 0, 0).sum()) == 4
    assert torch.equal(gc.expected_reach(gr, 'ext_d32', '32', 1, 2), gc.expected_reach(gz, 'ext_d32', '32', 1, 2))
    assert int(gc.expected_reach(gc.CASES['u1e'], 'ext_up', '64', 0, 0).sum()) == int(gc.expected_reach(gc.CASES['u1z'], 'ext_up', '64', 0, 0).sum()) == 9
    assert gc.expected_reach(gc.CASES['p1a'], 'c1_d32', '256x64', 3, 5).nonzero().tolist() == [[3, 5]]
