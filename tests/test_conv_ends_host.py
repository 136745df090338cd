"""CPU: the evidence that the conditions of tests/test_gpu_conv_ends.py are conditions on the REFERENCE, not on what a kernel returns.

The NCHW ends of cf_conv2d are END_CASES of tools/conv_geom_check.py, merged into a module object of its own by with_nchw_ends(); CASES and ROUTES as
tests/test_conv_geom_host.py pins them are untouched (asserted here).  For the 34 cases:
  * they are the issue's: every (c0, size) of the input end, the two MFMA cases, every (cout, size, c0) of the zero-padded head; no earlier case's seed moved;
  * route_of() against a literal table, all five new forms reached; the library accepts every launch (a parts query) and refuses the neighbours -- among
    them the input end off the 16x16 tile grid (17x19, 24x40), which no kernel takes;
  * the reference against the index-by-index loop of test_conv_geom_host.py; int_coded's exactness preconditions and its exact emulation (K <= 36:
    accumulators below 2^12 units); every family's emulation within 0.5 of its gate;
  * which families apply where; cancel_pairs is ill-conditioned; the one-hot pixels of the input end sit at the corners, on every edge and on both sides of
    every 16-pixel tile border.
"""
import ctypes

import pytest
import torch

import test_conv_geom_host as base
from _tools import load_script

NCHW_KEYS = ('n3a', 'n3b', 'n1a', 'n1b', 'n2a', 'n2b', 'n4a', 'n4b', 'nm3a', 'nm3b')
HEAD_KEYS = tuple(f'h{n}{t}{c}' for n in (1, 2, 4, 3) for t in 'ab' for c in (16, 32, 64))
END_KEYS = NCHW_KEYS + HEAD_KEYS
EXPECTED = {k: {'F32': ('nchw_in', 'mfma' if k[1] == 'm' else 'few_cin 3' if k[1] == '3' else 'few_cin n')} for k in NCHW_KEYS}
EXPECTED.update({k: {'F32': ('head', 'few_cout 3' if k[1] == '3' else 'few_cout 4')} for k in HEAD_KEYS})
ISSUE_FORMS = {('nchw_in', 'few_cin 3'), ('nchw_in', 'few_cin n'), ('nchw_in', 'mfma'), ('head', 'few_cout 4'), ('head', 'few_cout 3')}


@pytest.fixture(scope='module')
def gc():
    m = load_script('tools/conv_geom_check.py')
    assert tuple(m.CASES) == base.CASE_KEYS and m.ROUTES == ('s2_d32', 's2_dsplit', 'c1_d32', 'c1_dsplit', 'ext_d32', 'ext_up', 'd32_32', 'head')
    assert all(m.SEED_INDEX[k] == sorted(base.CASE_KEYS).index(k) for k in base.CASE_KEYS)          # an added case moves no earlier case's seed
    m.with_nchw_ends()
    assert tuple(m.CASES) == base.CASE_KEYS + END_KEYS and tuple(m.END_CASES) == END_KEYS and m.ROUTES[-1] == 'nchw_in' and len(m.ROUTES) == 9
    return m


def test_cases_are_the_issue_s(gc):
    C = gc.CASES
    assert {(C[k].cin, C[k].H, C[k].W) for k in NCHW_KEYS[:8]} == {(c, *hw) for c in (1, 2, 3, 4) for hw in ((16, 16), (32, 48))}
    assert all(C[k].in_nchw and C[k].cout == 64 and C[k].B == 2 for k in NCHW_KEYS)
    assert C['nm3a'][:5] == (2, 16, 16, 3, 64) and C['nm3a'].epi == gc.EPI_RESIDUAL and C['nm3b'][:5] == (2, 32, 48, 3, 64) and C['nm3b'].epi == gc.EPI_SFT
    assert {(C[k].cout, C[k].H, C[k].W, C[k].cin) for k in HEAD_KEYS} == {(n, *hw, c) for n in (1, 2, 3, 4) for hw in ((21, 37), (16, 16)) for c in (16, 32, 64)}
    assert all(C[k].out_nchw and C[k].pad_mode == gc.PAD_ZERO and C[k].B == 2 for k in HEAD_KEYS)
    assert {(C[k].cin // 16) % 2 for k in HEAD_KEYS} == {0, 1}                 # the two-slab gather: odd and even chunk counts


def test_routes_against_the_literal_table(gc):
    from codeformer_amd import ops
    got = {key: {n: (r, f) for n, _, r, f in rows} for key, rows in gc.routes().items() if key in END_KEYS}
    assert got == EXPECTED and {rf for rows in got.values() for rf in rows.values()} == ISSUE_FORMS
    G = gc.G
    # the input end: no launch off the 16x16 tile grid (the issue's 17x19 and 24x40), an fp32 weight only, cout_pad 64 only, no EXT feature
    assert [gc.route_of(0, g) for g in gc.OFF_GRID_NCHW] == [None, None] and [tuple(g[:5]) for g in gc.OFF_GRID_NCHW] == [(2, 17, 19, 3, 64), (2, 24, 40, 3, 64)]
    assert gc.route_of(ops.SPLIT, gc.CASES['n3a']) is None and gc.route_of(0, G(2, 16, 16, 5, 64, in_nchw=True)) is None
    assert gc.route_of(0, G(2, 16, 16, 3, 128, in_nchw=True)) is None and gc.route_of(0, G(2, 16, 16, 3, 64, in_nchw=True, epi=gc.EPI_LEAKY)) is None
    assert gc.route_of(0, G(2, 16, 16, 3, 48, in_nchw=True)) == ('nchw_in', 'mfma')                   # (fewer than 64 channels: the MFMA form too)
    assert gc.route_of(0, gc.CASES['hd']) == ('head', 'few_cout reflect')


def _desc(gc, g, **over):
    from test_conv_dispatch_host import D
    from codeformer_amd import lib, ops
    dummy = ctypes.create_string_buffer(64)
    p = ctypes.addressof(dummy)
    epi = g.epi or 0
    kw = dict(batch=g.B, stats_cpg=0, acc_scale=1.0, in0=p, pad_mode=g.pad_mode, out_nchw=int(g.out_nchw), in_nchw=int(g.in_nchw), epilogue=epi,
              res=p if epi else None, sft_scale=p if epi == gc.EPI_SFT else None)
    kw.update(over)
    d = lib.ConvDesc(**D(g.H, g.W, g.cin, g.cout, ops._cout_pad(g.cout), **kw))
    d._keep = dummy
    return d


def test_the_library_accepts_every_launch_and_refuses_the_neighbours(gc):
    from codeformer_amd import build as cf_build
    from codeformer_amd import lib
    cf_build.build()
    native = lib.load()

    def query(g, **over):
        d = _desc(gc, g, **over)
        return native.cf_conv2d_stats_parts(ctypes.byref(d)), lib.last_error()

    for key in END_KEYS:
        g = gc.CASES[key]
        if g.out_nchw:           # (a query passes the few-channel kernel by and lands on the 32-wide rung, which wants whole tiles: test_conv_geom_host.py)
            g = g._replace(H=32, W=48)
        got, err = query(g)
        assert got > 0, (key, err)
    for g in gc.OFF_GRID_NCHW:   # refused by the MFMA form's tile check: no EXT instantiation reads NCHW
        got, err = query(g)
        assert got <= 0 and 'not divisible by the 16x16 tile' in err, err
    got, err = query(gc.CASES['n3a'], prologue=gc.PRO_LEAKY)
    assert got <= 0 and 'in_nchw has no prologue' in err, err
    got, err = query(gc.CASES['n3a'], pad_mode=gc.PAD_REFLECT)
    assert got <= 0 and 'strided slices' in err, err
    assert query(gc.CASES['n3a'], stats_cpg=2)[0] == 4 and query(gc.CASES['n3b'], stats_cpg=2)[0] == 24        # four partials per 16x16 tile


@pytest.mark.parametrize('key', ('n3a', 'n1a', 'h1b16', 'h3a16'))
def test_reference_against_an_index_by_index_loop(gc, key):
    base.test_reference_against_an_index_by_index_loop(gc, key)


@pytest.mark.parametrize('key', END_KEYS)
def test_int_coded_preconditions_and_exact_emulation(gc, key):
    g = gc.CASES[key]
    if g.cin > 1:
        base.test_int_coded_preconditions_and_exact_emulation(gc, key)        # (it also exchanges two channels)
    else:
        (_, code, route, form), = gc.launches(key)
        assert gc.exactness_preconditions(key, route, form) < 2 ** 24
        for v in gc.int_coded_variants(key, route, form):
            d, ref, _ = gc.prepared('int_coded', key, route, form, v)
            assert gc.bits_equal(gc.emulate(d, g, route) + 0.0, ref['out'].float() + 0.0), (key, v)
    if g.in_nchw:                                                              # K <= 36: trivially exact
        (_, code, route, form), = gc.launches(key)
        assert gc.exactness_preconditions(key, route, form) < 2 ** 12 and gc.int_coded_variants(key, route, form) == (0, 3)


@pytest.mark.parametrize('key', END_KEYS)
def test_emulation_within_half_of_the_gate(gc, key):
    base.test_emulation_within_half_of_the_gate(gc, key)


def test_gate_families_apply_where_the_issue_says(gc):
    fams = {}
    for key in END_KEYS:
        for _, code, r, form in gc.launches(key):
            fams.setdefault((r, form), set()).update(f for f in gc.families_of(key) if gc.prepared(f, key, r, form) is not None)
    assert fams[('nchw_in', 'few_cin 3')] == {'mixed_cout', 'mixed_cin_act', 'dc_plus_ripple'}                 # (three channels have no pairs)
    assert fams[('nchw_in', 'few_cin n')] == fams[('nchw_in', 'mfma')] | {'cancel_pairs'} == {'mixed_cout', 'mixed_cin_act', 'cancel_pairs', 'dc_plus_ripple'}
    for form in ('few_cout 3', 'few_cout 4'):                                                                  # (the head takes the affine prologue, no epilogue)
        assert fams[('head', form)] == {'mixed_cout', 'mixed_cin', 'mixed_cin_act', 'cancel_pairs', 'dc_plus_ripple'}
    C = gc.CASES
    assert not gc.buildable('mixed_cout', C['h1a16']) and not gc.buildable('mixed_cin_act', C['n1a']) and not gc.buildable('cancel_pairs', C['n3a'])
    assert gc.prepared('dc_plus_ripple', 'n3a', 'nchw_in', 'few_cin 3')[0]['epi'] == gc.EPI_NONE and gc.prepared('mixed_cout', 'n3a', 'nchw_in', 'few_cin 3')[0]['pro'] == gc.PRO_NONE
    assert gc.prepared('dc_plus_ripple', 'nm3b', 'nchw_in', 'mfma')[0]['epi'] == gc.EPI_SFT and gc.prepared('swish_leaky_edges', 'n3a', 'nchw_in', 'few_cin 3') is None


def test_hard_families_are_hard(gc):
    for key in END_KEYS:
        g = gc.CASES[key]
        if gc.buildable('cancel_pairs', g):
            d = gc.family('cancel_pairs', key)
            cond = float((gc._abs_eval(d, g)[0] / gc.reference(d, g)['pre'].abs()).median())
            # (the input end pairs up 2 or 4 channels, 18 or 36 products: there the bias, 0.1 randn, is what is left of |pre| and the ratio is lower)
            assert cond >= (30 if g.in_nchw else 100) and torch.equal(d['x'][..., 0::2], d['x'][..., 1::2]), (key, cond)
        else:
            assert g.in_nchw and g.cin in (1, 3)
        d = gc.family('dc_plus_ripple', key)
        assert float(d['w'].sum((2, 3)).abs().max()) <= 1e-5 and 250 < float(d['x'].mean()) < 262


def test_onehot_pixels_are_where_the_docstring_says(gc):
    for key in END_KEYS:
        g = gc.CASES[key]
        per_image = [gc.onehot_positions(g, bi) for bi in range(g.B)]
        for pos in per_image:
            assert len(pos) == len(set(pos)) >= min(g.cin, 6), key
            assert all(max(abs(p[0] - q[0]), abs(p[1] - q[1])) >= 3 for i, p in enumerate(pos) for q in pos[:i])
            assert all(0 <= r < g.H and 0 <= q < g.W for r, q in pos)
        allp = {p for pos in per_image for p in pos}
        corners = {(0, 0), (0, g.W - 1), (g.H - 1, 0), (g.H - 1, g.W - 1)}
        assert corners <= set(per_image[0]) and {(1, 1), (g.H - 2, g.W - 2)} <= set(per_image[1]), key
        rows, cols = {r for r, _ in allp}, {q for _, q in allp}
        if g.in_nchw:          # the four corners, a pixel on each edge, both sides of every 16-pixel tile border, several pixels per channel
            assert len(per_image[0]) > 4 * g.cin, key
            inner = allp - corners
            assert all(any(t(r, q) for r, q in inner) for t in (lambda r, q: r == 0, lambda r, q: r == g.H - 1, lambda r, q: q == 0, lambda r, q: q == g.W - 1)), key
            assert all({b - 1, b} <= rows for b in range(16, g.H, 16)) and all({b - 1, b} <= cols for b in range(16, g.W, 16)), (key, sorted(rows), sorted(cols))
        else:                  # the last (partial) tile's boundary, as test_conv_geom_host.py asks of every stride-1 case
            last_r, last_c = 8 * ((g.H - 1) // 8), 16 * ((g.W - 1) // 16)
            assert (last_r == 0 or {last_r - 1, last_r} <= rows) and (last_c == 0 or {last_c - 1, last_c} <= cols), (key, sorted(rows), sorted(cols))
    for key in ('n3a', 'h1a16'):       # the fp64 result IS the weight + bias where one weight meets a pixel
        g = gc.CASES[key]
        d = gc.family('onehot_pixels', key)
        ref = gc.reference(d, g)
        count = gc.conv64(gc.padded(d['x'].double().abs(), g), torch.ones_like(d['w'][:1]), g)[..., 0]
        bias = d['b'].double().expand_as(ref['out'])
        assert int((count == 1).sum()) >= len(gc.onehot_positions(g, 0)) and torch.equal(ref['out'][count == 0], bias[count == 0])


def test_expected_reach_of_the_corner_pixel(gc):
    """Zero padding at both ends: a pixel at (0, 0) is in the window of the four outputs around it, an interior one of nine."""
    for key, route, form in (('n3a', 'nchw_in', 'few_cin 3'), ('h1a16', 'head', 'few_cout 4')):
        g = gc.CASES[key]
        assert gc.expected_reach(g, route, form, 0, 0).nonzero().tolist() == [[0, 0], [0, 1], [1, 0], [1, 1]]
        assert int(gc.expected_reach(g, route, form, 4, 5).sum()) == 9
