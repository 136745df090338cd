"""CPU: the evidence that the conditions of tests/test_gpu_conv_prelu.py are conditions on the REFERENCE, not on what a kernel returns.

The thirteen cases are PRELU_CASES of tools/conv_geom_check.py, merged into a module object of its own by with_prelu(); CASES and ROUTES as
tests/test_conv_geom_host.py pins them stay, and its tests that fit a case unchanged are called from here:
  * route_of() against a literal table: the five forms, 32x32 to `narrow` and 25x41 to `128`, the refused neighbours; the library's own validation
    accepts every launch;
  * the reference is the definition (a select on the sign of t), the slopes are arcface_ref's, every form sees a negative slope and one above one;
  * int_coded: the exactness preconditions and the emulation bitwise the fp64 result, which is its own float32 rounding;
  * every gate family, onehot_pixels and tap_shift: the emulation within 0.5 of the gate.
"""
import ctypes

import pytest
import torch

import test_conv_geom_host as base
from _tools import load_script

PRELU_KEYS = ('q64a', 'q64b', 'q64c', 'q32a', 'q32b', 'q32c', 'qna', 'qnb', 'q128a', 'q128b', 'qs0', 'qs1', 'qs1p')
FORM_OF = {'q64': '64', 'q32': '32', 'qn': 'narrow', 'q128': '128', 'qs': 's2'}
EXPECTED = {k: {'F32': ('prelu', next(f for p, f in sorted(FORM_OF.items(), key=lambda t: -len(t[0])) if k.startswith(p)))} for k in PRELU_KEYS}
ISSUE_FORMS = {('prelu', 's2'), ('prelu', 'narrow'), ('prelu', '128'), ('prelu', '64'), ('prelu', '32')}


@pytest.fixture(scope='module')
def gc():
    m = load_script('tools/conv_geom_check.py')
    assert tuple(m.CASES) == base.CASE_KEYS and len(m.ROUTES) == 8 and 'prelu' not in m.ROUTES
    first = dict(m.SEED_INDEX)
    m.with_prelu()
    assert tuple(m.CASES) == base.CASE_KEYS + PRELU_KEYS and tuple(m.PRELU_CASES) == PRELU_KEYS and m.ROUTES[-1] == 'prelu' and len(m.ROUTES) == 9
    assert m.SEED_INDEX == first and all(m.SEED_INDEX[k] == 26 + len(m.END_CASES) + i for i, k in enumerate(PRELU_KEYS))      # an added case moves no earlier seed
    return m


def test_cases_are_the_issue_s(gc):
    C = gc.CASES
    P, RP = gc.EPI_PRELU, gc.EPI_RES_PRELU
    assert {(tuple(C[k][:5]), C[k].epi) for k in ('q64a', 'q64b')} == {((2, 19, 35, 32, 64), P), ((2, 19, 35, 32, 64), RP)}
    assert tuple(C['q32a'][:5]) == (1, 9, 5, 16, 32) and tuple(C['qna'][:5]) == (2, 8, 8, 64, 128) and tuple(C['qnb'][:5]) == (1, 32, 32, 32, 128)
    assert tuple(C['q128a'][:5]) == (1, 25, 41, 32, 128) and C['qnb'].H * C['qnb'].W == 1024 and C['q128a'].H * C['q128a'].W == 1025
    assert all(tuple(C[k][:5]) == (2, 20, 36, 32, 128) and C[k].stride == 2 for k in ('qs0', 'qs1', 'qs1p')) and (C['qs0'].pad_lo, C['qs1'].pad_lo) == (0, 1)
    from codeformer_amd import ops
    assert ops._cout_pad(96) == 128      # (the packer has no cout_pad of 96: the 32-wide form exists at cout <= 32 only)


def test_routes_against_the_literal_table(gc):
    got = {key: {n: (r, f) for n, _, r, f in rows} for key, rows in gc.routes().items() if key in PRELU_KEYS}
    assert got == EXPECTED
    assert {rf for rows in got.values() for rf in rows.values()} == ISSUE_FORMS


def test_the_prelu_route_its_predicates_reference_and_gate(gc):
    """route_of() on both sides of the `narrow` predicate and of every rung; the refused neighbours; the reference is the definition (a select on the
    sign of t, not max(t, a t)); the slopes are arcface_ref's and every form sees a negative one and one above one."""
    import arcface_ref
    G, P, RP = gc.G, gc.EPI_PRELU, gc.EPI_RES_PRELU
    assert gc.SLOPES == arcface_ref.SLOPES
    assert gc.route_of(0, G(1, 32, 32, 32, 128, epi=P, alpha=1.5)) == ('prelu', 'narrow')          # exactly 1024 pixels
    assert gc.route_of(0, G(1, 25, 41, 32, 128, epi=P, alpha=1.5)) == ('prelu', '128')             # 1025
    assert gc.route_of(0, G(1, 32, 32, 32, 64, epi=P, alpha=1.5)) == ('prelu', '64') and gc.route_of(0, G(1, 16, 16, 16, 32, epi=RP, alpha=0.0)) == ('prelu', '32')
    assert gc.route_of(0, G(1, 16, 16, 16, 96, epi=RP, alpha=0.0)) == ('prelu', 'narrow')          # (no cout_pad of 96: it packs to 128)
    assert gc.route_of(0, G(2, 20, 36, 32, 128, stride=2, epi=P, alpha=0.25)) == ('prelu', 's2')
    for bad in (G(2, 20, 36, 32, 64, stride=2, pad_lo=1, epi=P, alpha=0.25), G(2, 7, 11, 32, 64, up=True, epi=P, alpha=0.25),
                G(2, 16, 16, 32, 64, taps=1, epi=P, alpha=0.25), G(2, 16, 16, 32, 64, out_nchw=True, epi=P, alpha=0.25)):
        assert gc.route_of(0, bad) is None, bad
    from codeformer_amd import ops
    assert gc.route_of(ops.SPLIT, G(2, 16, 16, 32, 64, epi=P, alpha=0.25)) is None
    seen = {}
    assert gc.PRELU_KEYS == PRELU_KEYS
    for key in gc.PRELU_KEYS:
        g = gc.CASES[key]
        (_, code, route, form), = gc.launches(key)
        seen.setdefault(form, set()).add(g.alpha)
        assert g.cin // 16 >= 2 or key in ('q32a', 'q32c'), key                                        # two K slabs (the 9x5 PRELU pair: one)
        d, ref, tol = gc.prepared('mixed_cout', key, route, form)
        a = float(torch.tensor(g.alpha, dtype=torch.float32))
        t = ref['pre'] + d['res'].double() if g.epi == RP else ref['pre']
        assert torch.equal(ref['out'], torch.where(t > 0, t, a * t)) and bool((t < 0).any()) and bool((t > 0).any())
        if a > 1:
            assert not torch.equal(ref['out'], torch.maximum(t, a * t))                # (max(t, a t) is the select for a <= 1 only)
        assert d['pro'] == gc.PRO_AFFINE and gc.prepared('dc_plus_ripple', key, route, form)[0]['pro'] == gc.PRO_NONE
        assert bool((tol >= max(1.0, abs(a)) * gc.coef(route, g) * gc.U * gc._abs_eval(d, g)[0]).all())
    assert set(seen) == {'s2', 'narrow', '128', '64', '32'} and all(min(v) < 0 and max(v) > 1 for v in seen.values()), seen
    assert {a for v in seen.values() for a in v} == set(gc.SLOPES)
    assert {gc.CASES[k].epi for k in gc.PRELU_KEYS if gc.CASES[k].pad_lo} == {P, RP}               # pad_lo 1, ArcFace's stride-2 geometry, under both


def test_the_library_accepts_every_launch_and_refuses_the_neighbours(gc):
    """cf_conv2d_stats_parts: the library's own validation, up to the point where a kernel would start."""
    from codeformer_amd import build as cf_build
    from codeformer_amd import lib, ops
    cf_build.build()
    native = lib.load()
    dummy = ctypes.create_string_buffer(64)

    def query(g, code, **over):
        over.setdefault('res', ctypes.addressof(dummy) if g.epi == gc.EPI_RES_PRELU else None)
        d = base._desc(gc, g, code, **over)
        return native.cf_conv2d_stats_parts(ctypes.byref(d)), lib.last_error()

    for key in PRELU_KEYS:
        (cname, code, route, form), = gc.launches(key)
        got, err = query(gc.CASES[key], code)
        assert got > 0, (key, route, form, err)
    G, P = gc.G, gc.EPI_PRELU
    got, err = query(G(2, 20, 36, 32, 64, stride=2, pad_lo=1, epi=P, alpha=0.25), 0)                 # stride 2 at cout_pad 64
    assert got <= 0 and 'strided slices' in err, err
    got, err = query(G(2, 16, 16, 32, 64, epi=P, alpha=0.25), 0, bf16_mfma=2)                      # CF_OPERAND_F16: IEEE-half operands
    assert got <= 0 and 'PReLU epilogues are built for plain 3x3 convs with fp32 operands' in err, err
    got, err = query(G(2, 16, 16, 32, 64, epi=P, alpha=0.25), 0, winograd=1)
    assert got <= 0 and 'PReLU epilogues belong to the general fp32' in err, err
    got, err = query(G(2, 16, 16, 32, 64, epi=gc.EPI_RES_PRELU, alpha=0.25), 0, res=None)           # RES_PRELU without its residual
    assert got <= 0 and 'epilogue needs res' in err, err


@pytest.mark.parametrize('key', PRELU_KEYS)
def test_int_coded_preconditions_and_exact_emulation(gc, key):
    base.test_int_coded_preconditions_and_exact_emulation(gc, key)
    (_, code, route, form), = gc.launches(key)
    assert gc.int_coded_variants(key, route, form) == (0, 1)
    for v in (0, 1):      # the float32 reference IS the float64 one
        ref = gc.prepared('int_coded', key, route, form, v)[1]
        assert torch.equal(ref['out'].float().double(), ref['out'])


@pytest.mark.parametrize('key', PRELU_KEYS)
def test_emulation_within_half_of_the_gate(gc, key):
    base.test_emulation_within_half_of_the_gate(gc, key)


def test_gate_families_apply_where_the_issue_says(gc):
    fams = {f for key in PRELU_KEYS for _, code, r, form in gc.launches(key) for f in gc.families_of(key) if gc.prepared(f, key, r, form) is not None}
    assert fams == {'mixed_cout', 'mixed_cin', 'mixed_cin_act', 'cancel_pairs', 'dc_plus_ripple', 'swish_leaky_edges'}      # (EXT has no SFT)
    assert gc.prepared('swish_leaky_edges', 'q64a', 'prelu', '64') is None and gc.prepared('swish_leaky_edges', 'q64b', 'prelu', '64')[0]['epi'] == gc.EPI_RES_PRELU


def test_hard_families_are_hard_and_onehot_pixels_sit_on_the_borders(gc):
    for key in PRELU_KEYS:
        g = gc.CASES[key]
        d = gc.family('cancel_pairs', key)
        cond = float((gc._abs_eval(d, g)[0] / gc.reference(d, g)['pre'].abs()).median())
        assert cond >= 100, (key, cond)
        per_image = [gc.onehot_positions(g, bi) for bi in range(g.B)]
        for pos in per_image:
            # (an 8x8 image whose rows and columns 1 and 6 are taken has no pixel left 3 away from all four: the odd image of qna)
            assert len(pos) == len(set(pos)) >= min(g.cin, 4 if (g.H, g.W) == (8, 8) else 6), key
            assert all(max(abs(p[0] - q[0]), abs(p[1] - q[1])) >= 3 for i, p in enumerate(pos) for q in pos[:i])
        assert (0, 0) in per_image[0] and (g.H - 1, g.W - 1) in per_image[0]
        if g.stride == 1 and min(g.H, g.W) >= 7:
            allp = {p for pos in per_image for p in pos}
            last_r, last_c = 8 * ((g.H - 1) // 8), 16 * ((g.W - 1) // 16)                    # the last (partial) tile's boundary
            rows, cols = {r for r, _ in allp}, {q for _, q in allp}
            assert last_r == 0 or {last_r - 1, last_r} <= rows, (key, last_r, sorted(rows))
            assert last_c == 0 or {last_c - 1, last_c} <= cols, (key, last_c, sorted(cols))
