"""CPU: the evidence that the conditions of tests/test_gpu_conv_families.py are conditions on the REFERENCE, not on what a kernel returns.

For the input families of tools/conv_check.py:
  * int_coded at cin = 512 (and at the folded-upsample and concat shapes): every F(2,3) transform-domain value fits 8 significand bits, so it is exact in
    bf16 and in IEEE half with a zero lo half, with and without the pack scale; every accumulator's sum of |products| stays below 2^24 units; and the
    emulation of every exact route's operand scheme returns the fp64 result bitwise;
  * every gate family's emulation stays within 0.5 of its gate, per operand scheme (fp32, split halves, single half, bf16) and transform (direct,
    F(2,3), F(4,3)), at EVERY shape the GPU test uses (the largest: most pixels d, most channels f, most output channels g, folded u1);
  * the reference equals conv_case.reference; both Winograd evaluations in fp64 equal the convolution;
  * onehot_pixels / tap_shift: the fp64 result IS the flipped weight slice + bias / the shifted input, the pixels are >= 3 apart and sit where
    the docstring says; cancel_pairs is ill-conditioned, mixed_cout reaches subnormal lo and hi halves under the host's own scale rule;
  * routes() against a table of expected kernel forms for the issue's shapes, every route reached, and the C library's own validation
    (cf_conv2d_stats_parts: the code of a launch up to the point where a kernel would start) accepts every launch the GPU test makes;
  * the sub-pixel F(4,2) route w42_up at its shapes u1, zu1, zu2 (1, 3 and 8 slabs): its fp64 evaluation is conv_case.reference(upsample=True), its
    weights are ops.f42_weights, its S lies between the folded direct sum and 4556.25 sum_c max|g_p,c| max|p_c|; the float32 emulation stays within half
    the gate for every family the route admits, onehot_pixels and all nine tap_shift taps; the emulation with the taps of phase (b, a) given to phase
    (a, b), or with one position lost to the idle accumulator, stands at >= 10 times the gate on some family at every shape; and the older keys' data is
    what it was before zu1 / zu2 existed (digests).
"""
import ctypes

import numpy as np
import pytest
import torch

from _tools import load_script


@pytest.fixture(scope='module')
def cc():
    m = load_script('tools/conv_check.py')
    m.with_f42()          # (zu1, zu2 behind the older keys, whose data test_every_older_key_keeps_its_data pins)
    return m


LARGEST = ('d', 'f', 'g', 'u1')        # most pixels, most input channels, most output channels, folded
ALL_KEYS = ('a', 'b', 'c', 'd', 'e', 'f', 'g', 'u1', 'u2', 'zu1', 'zu2')
W42_KEYS = ('u1', 'zu1', 'zu2')        # the shapes of the sub-pixel F(4,2) form: 1, 3 and 8 slabs
GATE_FAMILIES = ('mixed_cout', 'mixed_cin', 'mixed_cin_act', 'cancel_pairs', 'dc_plus_ripple', 'swish_leaky_edges', 'swish_leaky_edges_sft')
PROLOGUE_ONLY = ('mixed_cin', 'swish_leaky_edges', 'swish_leaky_edges_sft', 'solo_cin')      # families that ARE their prologue: not on upsampling shapes
SOLO_FAMILIES = ('solo_cin', 'solo_cin_act')


def test_families_and_shapes_are_the_issue_s(cc):
    assert cc.GATE_FAMILIES == GATE_FAMILIES and cc.SOLO_FAMILIES == SOLO_FAMILIES
    assert {k: v[:5] for k, v in cc.SHAPES.items()} == {'a': (1, 16, 16, 16, 64), 'b': (2, 16, 32, 32, 64), 'c': (2, 32, 32, 64, 128), 'd': (3, 32, 48, 48, 128),
                                                        'e': (1, 16, 16, 256, 64), 'f': (1, 16, 16, 512, 128), 'g': (1, 48, 32, 192, 192),
                                                        'u1': (2, 16, 16, 32, 128), 'u2': (1, 16, 16, 64, 64), 'zu1': (1, 32, 48, 96, 256),
                                                        'zu2': (1, 16, 16, 256, 128)}
    assert tuple(cc.SHAPES) == ALL_KEYS and all(cc.SHAPES[k][6] for k in W42_KEYS)
    assert all(B <= 3 and H <= 48 and W <= 48 and cin <= 512 for B, H, W, cin, _, _, _ in cc.SHAPES.values())


def _schemes(cc, key):
    """One launch per (route, operand type) of a shape: the emulation does not depend on the split count."""
    seen = {}
    for cname, code, sk, route, form in cc.launches(key):
        seen.setdefault((route, cc.scheme_of(route, code)), (cname, code, route))
    return list(seen.values())


@pytest.mark.parametrize('family,key', [(f, k) for f in GATE_FAMILIES + SOLO_FAMILIES + ('onehot_pixels',) for k in ALL_KEYS if not ('u' in k and f in PROLOGUE_ONLY)])
def test_emulation_within_half_of_the_gate(cc, family, key):
    assert not (cc.SHAPES[key][6] and family in PROLOGUE_ONLY)            # (upsampling shapes take no prologue)
    for cname, code, route in _schemes(cc, key):
        r, err = cc.emulated(family, key, route, code)
        print(f'{family} {key} {route} {cname}: emulation max|d| {err:.3e} = {r:.3f} of the gate')
        assert r <= 0.5, (family, key, route, cname, r, err)


@pytest.mark.parametrize('key', ('b', 'c', 'd', 'u1', 'zu1', 'zu2'))            # the shapes of the GPU test's tap_shift cases
def test_tap_shift_emulation_within_half_of_the_gate(cc, key):
    for tap in range(9):
        for cname, code, route in _schemes(cc, key):
            r, err = cc.emulated('tap_shift', key, route, code, tap)
            assert r <= 0.5, (key, tap, route, cname, r, err)


@pytest.mark.parametrize('key', ('f', 'c', 'u1', 'u2', 'a'))
def test_int_coded_preconditions_and_exact_emulation(cc, key):
    worst = cc.exactness_preconditions(key)
    print(f'int_coded {key}: largest accumulator {worst:.0f} units < 2^24')
    assert worst < 2 ** 24
    for variant in range(4):
        d, ref = cc.prepared('int_coded', key, variant)
        want = ref['out'].float()
        assert torch.equal(want.double(), ref['out'])
        for cname, code, route in _schemes(cc, key):
            if route in cc.EXACT_ROUTES:
                assert cc.bits_equal(cc.emulate(d, route, code) + 0.0, want + 0.0), (key, variant, route, cname)
    # position-coded: a shifted input or two exchanged channels change the result
    d, ref = cc.prepared('int_coded', key, 0)
    alt = dict(d, x=torch.roll(d['x'], 1, dims=2))
    assert not torch.equal(cc.reference(alt)['out'], ref['out'])
    xs = d['x'].clone()
    xs[..., [0, 1]] = xs[..., [1, 0]]
    assert not torch.equal(cc.reference(dict(d, x=xs))['out'], ref['out'])


@pytest.mark.parametrize('key', ('b', 'c', 'u1'))
def test_reference_is_conv_case_reference_and_both_transforms_are_the_convolution(cc, key):
    for fam in GATE_FAMILIES + SOLO_FAMILIES + ('onehot_pixels', 'int_coded'):
        if cc.SHAPES[key][6] and fam in PROLOGUE_ONLY:
            continue
        d, ref = cc.prepared(fam, key)
        want = cc.case_ref(d)
        scale = float(want.abs().max())
        assert float((ref['out'] - want).abs().max()) <= 1e-12 * scale, fam
        p, _ = cc.prologue64(d)
        for m in (2, 4):
            y, _ = cc.wino(p, d['w'], m)
            S = cc._abs_eval(fam, key, 0, m)[0]
            assert bool(((y + d['b'].double() - ref['pre']).abs() <= 1e-13 * S + 1e-300).all()), (fam, m)
            assert bool((S >= cc._abs_eval(fam, key, 0, 0)[0] * (1 - 1e-12)).all())          # the Winograd S is never below the direct S
            # ... and never above (the product of the absolute row sums of A^T, G and B^T)^2 times sum_c max|g_c| max|p_c| over the tile's window: it
            # cannot quietly become a loose gate on a sparse family
            n, amp = m + 2, (3 * 1.5 * 2) ** 2 if m == 2 else (17.25 * 56 / 15 * 1.875) ** 2
            win = torch.nn.functional.pad(p.abs().permute(0, 3, 1, 2), (1, 1, 1, 1)).unfold(2, n, m).unfold(3, n, m).amax((4, 5))      # (B, C, th, tw)
            T = torch.einsum('bcyx,kc->byxk', win, d['w'].double().abs().amax((2, 3))).repeat_interleave(m, 1).repeat_interleave(m, 2)
            assert bool((S <= amp * T * (1 + 1e-12)).all()), (fam, m, float((S / T.clamp_min(1e-300)).max()))


def test_onehot_pixels_are_where_the_docstring_says_and_select_the_weight(cc):
    for key in ('a', 'b', 'd'):
        B, H, W, cin, cout, _, _ = cc.SHAPES[key]
        pos = cc.onehot_positions(H, W, cin)
        assert len(pos) == min(cin, len(pos)) >= 12 and len(set(pos)) == len(pos)
        assert all(max(abs(p[0] - q[0]), abs(p[1] - q[1])) >= 3 for i, p in enumerate(pos) for q in pos[:i])
        assert {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)} <= set(pos)
        rows, cols = {p[0] for p in pos}, {p[1] for p in pos}
        assert {7, 8} <= rows and (W == 16 or {15, 16} <= cols)                       # both sides of a patch boundary
        assert any(r % 4 == 3 for r in rows) and any(r % 4 == 0 for r in rows) and any(r % 2 for r in rows)
        d, ref = cc.prepared('onehot_pixels', key)
        want = d['b'].double().expand(B, H, W, cout).clone()
        for bi in range(B):
            for c, (r, q) in enumerate(pos):
                ch = (c + 5 * bi) % cin
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        if 0 <= r + dy < H and 0 <= q + dx < W:
                            want[bi, r + dy, q + dx] += d['w'][:, ch, 1 - dy, 1 - dx].double()
        assert torch.equal(ref['out'], want)
        route, code = 'd32', 0
        assert cc.bits_equal(cc.emulate(d, route, code) + 0.0, want.float() + 0.0)   # fp32(w + b): one rounding


def test_tap_shift_moves_the_input_by_one_pixel(cc):
    B, H, W, cin, cout, _, _ = cc.SHAPES['b']
    p, sign = cc.tap_perm(cin, cout)
    for tap in range(9):
        d, ref = cc.prepared('tap_shift', 'b', tap)
        dy, dx = tap // 3 - 1, tap % 3 - 1
        xp = torch.nn.functional.pad(d['x'].double(), (0, 0, 1, 1, 1, 1))
        want = xp[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W][..., p] * sign.double()
        assert torch.equal(ref['out'] + 0.0, want + 0.0), tap
        if dy:
            assert float(want[:, 0 if dy < 0 else H - 1].abs().max()) == 0.0
        if dx:
            assert float(want[:, :, 0 if dx < 0 else W - 1].abs().max()) == 0.0


def test_hard_families_are_hard(cc):
    from codeformer_amd import ops
    for key in LARGEST + W42_KEYS[1:]:
        d, ref = cc.prepared('cancel_pairs', key)
        S = cc._abs_eval('cancel_pairs', key, 0, 0)[0]
        cond = float((S / ref['pre'].abs()).median())
        print(f'cancel_pairs {key}: median S / |pre| {cond:.3g}')
        assert cond >= 100 and torch.equal(d['x'][..., 0::2], d['x'][..., 1::2])
        if key in W42_KEYS:          # the same two preconditions with the S of the sub-pixel form, whose operand is the folded tap (a sum of up to four weights)
            for fam in ('cancel_pairs', 'dc_plus_ripple'):
                pre, S42 = cc.prepared(fam, key)[1]['pre'], cc._abs_eval(fam, key, 0, cc.F42)[0]
                cond = float((S42 / pre.abs()).median())
                print(f'{fam} {key}: median S / |pre| {cond:.3g} with the F(4,2) S')
                assert cond >= 100, (fam, key, cond)
        assert not torch.equal(d['w'][:, 0::2].abs(), d['w'][:, 1::2].abs())
        d = cc.family('mixed_cout', key)
        for m in (0, 2, 4):
            scale = cc.pack_scale_of(d, m, d['up'])
            w = d['w'].double()
            if m:
                G = cc.mats(m)[1]
                w = torch.einsum('ia,kcab,jb->kcij', G, w, G)
            hi, lo = cc.split_halves((w * scale).float().numpy())
            top = np.abs(hi).max()
            top *= 4.0 if (d['up'] and not m) else 1.0              # (folded taps: the scale leaves room for a sum of four)
            assert 2.0 ** 14 <= top < 2.0 ** 15 and scale == ops.pack_scale(float(w.abs().max()) * (4.0 if (d['up'] and not m) else 1.0))
            ch_hi, ch_lo = np.abs(hi).reshape(hi.shape[0], -1).max(1), np.abs(lo).reshape(lo.shape[0], -1).max(1)
            assert ((ch_lo < 2.0 ** -14) & (ch_lo > 0)).sum() >= 4 and ((ch_hi < 2.0 ** -14) & (ch_hi > 0)).sum() >= 2 and ch_lo[0] >= 2.0 ** -14, (key, m)
        d = cc.family('dc_plus_ripple', key)
        assert float(d['w'].sum((2, 3)).abs().max()) <= 1e-6 and 250 < float(d['x'].mean()) < 262
        d = cc.family('mixed_cin_act', key)
        mx = d['x'].abs().amax((0, 1, 2))
        assert float(mx.max() / mx.min()) >= 2.0 ** 18
    d = cc.family('swish_leaky_edges', 'c')
    assert {float(v) for v in d['x'].flatten()[:4096]} == {float(v) for v in cc.EDGE_VALUES} and bool((d['x'] == 0).logical_and(torch.signbit(d['x'])).any())
    assert float(d['res'].abs().mean()) > 300 * float(cc.reference(d)['pre'].abs().mean())


@pytest.mark.parametrize('key', ALL_KEYS)
def test_solo_families_read_small_and_large_channels_each_alone_in_its_sum(cc, key):
    B, H, W, cin, cout, _, up = cc.SHAPES[key]
    p = cc.solo_perm(cin, cout)
    read = sorted(set(p.tolist()))
    assert 0 in read and cin - 1 in read and {c // 16 for c in read} == set(range(cin // 16)), (key, read)
    assert cout >= cin or len(read) == cout                                    # (fewer outputs than inputs: no channel read twice)
    for fam in SOLO_FAMILIES:
        if up and fam in PROLOGUE_ONLY:
            continue
        d = cc.family(fam, key)
        live = cc.live_channels(d)
        assert torch.equal(live.nonzero()[:, 1], p) and bool((live.sum(1) == 1).all())
        assert bool((d['w'][live] != 0).all()) and not bool((d['w'][live].abs() == 1).any()) and d['epi'] == cc.EPI_NONE and bool((d['b'] != 0).all())
        e = cc.solo_exponents(fam, cin)
        assert float(e[read].min()) == float(e.min()) and float(e[read].max()) == float(e.max()) and float(e.max() - e.min()) == 2 * cc.SOLO_EXP
        assert d['pro'] == (cc.PRO_AFFINE if fam == 'solo_cin' else cc.PRO_NONE)
        s = cc.act_scale_of(d)
        assert bool((s == 1).all()) if fam == 'solo_cin' else bool((s < 2.0 ** -4).all())       # (the range scale brings 2^16 N(0, 1) below 2^12)
        hw = cc.emulate(d, 'd32', 0)
        assert bool(torch.isfinite(hw).all())
        lo_sub, hi_sub = cc.solo_kinds(d)
        print(f'{fam} {key}: read channels with subnormal lo halves {lo_sub.sum(1).tolist()}, with subnormal hi halves {hi_sub.sum(1).tolist()} (per image)')
        assert bool((lo_sub.sum(1) >= 2).all()) and bool((hi_sub.sum(1) >= 2).all()), (fam, key)
        # under the prologue no operand leaves the IEEE half range: the largest channel is normal and finite as a half
        top = (d['x'] * d['sc'][:, None, None, :] + d['sh'][:, None, None, :] if fam == 'solo_cin' else d['x'] * s.float()[:, None, None, None]).abs().max()
        assert 2.0 ** 10 <= float(top) < 2.0 ** 14, (fam, key, float(top))


@pytest.mark.parametrize('key', ALL_KEYS)
def test_dropped_small_lo_halves_exceed_the_solo_gate_and_no_other(cc, key):
    """conv_check.drop_small_lo: the lo half of an activation (of V on the Winograd routes) zeroed where it is a subnormal half, |a| < 2^-3 under the
    range scale.  Every split-half scheme of every shape the GPU test launches, cin 256 and 512 included: the solo families' emulation then stands at
    >= 10 times their gate.  At shape b every older gate family's ratio stays where it was (within 0.005 of the gate, and below 0.5): with one gate per
    output element a small input channel hides behind the large ones of the same sum -- the gap the solo families close."""
    half2 = [(cname, code, route) for cname, code, route in _schemes(cc, key) if cc.scheme_of(route, code)[1] == 'half2']
    assert half2
    for fam in SOLO_FAMILIES:
        if cc.SHAPES[key][6] and fam in PROLOGUE_ONLY:
            continue
        d, ref = cc.prepared(fam, key)
        for cname, code, route in half2:
            r, err = cc.ratio(cc.emulate(d, route, code, cc.drop_small_lo), ref, cc.gate(fam, key, route, code))
            print(f'{fam} {key} {route} {cname}: small lo halves dropped {r:.1f} of the gate (unedited {cc.emulated(fam, key, route, code)[0]:.3f})')
            assert r >= 10.0, (fam, key, route, cname, r)
            r_all, _ = cc.ratio(cc.emulate(d, route, code, cc.drop_every_lo), ref, cc.gate(fam, key, route, code))
            assert r_all >= r, (fam, key, route, cname, r_all, r)              # (every activation lo half dropped: no less)
    if key == 'e':      # the second gap, pinned: at cin 256 an evaluation with NO activation lo half at all stays inside every older family's gate
        for fam in GATE_FAMILIES:
            d, ref = cc.prepared(fam, key)
            for cname, code, route in half2:
                r, _ = cc.ratio(cc.emulate(d, route, code, cc.drop_every_lo), ref, cc.gate(fam, key, route, code))
                print(f'{fam} {key} {route} {cname}: every activation lo half dropped {r:.3f} of the gate')
                assert r < 1.0, (fam, route, r)
    if key == 'b':
        assert {route for _, _, route in half2} == {'dsplit', 'w23_h4', 'w43_8'}
        for fam in GATE_FAMILIES:
            d, ref = cc.prepared(fam, key)
            for cname, code, route in half2:
                r0 = cc.emulated(fam, key, route, code)[0]
                r, _ = cc.ratio(cc.emulate(d, route, code, cc.drop_small_lo), ref, cc.gate(fam, key, route, code))
                print(f'{fam} {key} {route} {cname}: unedited {r0:.4f}, small lo halves dropped {r:.4f} of the gate')
                assert abs(r - r0) <= 0.005 and r <= 0.5, (fam, route, r0, r)


def test_the_activation_hook_defaults_to_the_unedited_split(cc):
    d, _ = cc.prepared('solo_cin_act', 'b')
    for cname, code, route in _schemes(cc, 'b'):
        assert cc.bits_equal(cc.emulate(d, route, code), cc.emulate(d, route, code, lambda a, hi, lo: (hi, lo))), route


EXPECTED_FORMS = {
    'a': {('F32', 0): ('d32', '256x64'), ('WINOGRAD', 0): ('w23_f32', 'four-wave'), ('WSPLIT', 0): ('w23_h4', 'four-wave'), ('WF43', 0): ('w43_8', 'ntn 1'),
          ('WF43F', 0): ('w43_8', 'ntn 1')},
    'b': {('F32', 0): ('d32', '256x64'), ('SPLIT', 0): ('dsplit', 'form 0 64-wide'), ('WINOGRAD', 0): ('w23_f32', 'four-wave'), ('WSPLIT', 0): ('w23_h4', 'four-wave'),
          ('WF43', 0): ('w43_8', 'ntn 1'), ('WF43F', 0): ('w43_8', 'ntn 1')},
    'c': {('F32', 0): ('d32', 'narrow 128x64'), ('SPLIT', 0): ('dsplit', 'form 0 64-wide'), ('WINOGRAD', 0): ('w23_f32', 'four-wave'), ('WSPLIT', 0): ('w23_h8', 'f16x2'),
          ('WF16', 0): ('w23_h8', 'f16'), ('WBF16', 0): ('w23_h8', 'bf16'), ('WF43', 0): ('w43_16k32', 'ntn 1'), ('WF43F', 0): ('w43_16k32', 'ntn 1')},
    'd': {('F32', 0): ('d32', '128x128'), ('WINOGRAD', 0): ('w23_f32', 'four-wave'), ('WSPLIT', 0): ('w23_h8', 'f16x2'), ('WF43', 0): ('w43_16k16', 'ntn 1'), ('WF43F', 0): ('w43_16k16', 'ntn 1')},
    'e': {('F32', 0): ('d32', '256x64'), ('SPLIT', 0): ('dsplit', 'form 0 64-wide'), ('WINOGRAD', 0): ('w23_f32', 'four-wave'), ('WINOGRAD', 1): ('w23_f32', 'split-K 1'),
          ('WINOGRAD', 2): ('w23_f32', 'split-K 2'), ('WSPLIT', 0): ('w23_h4', 'four-wave'), ('WSPLIT', 1): ('w23_h4', 'split-K 1'), ('WSPLIT', 2): ('w23_h4', 'split-K 2'),
          ('WF43', 0): ('w43_8', 'ntn 1'), ('WF43F', 0): ('w43_8', 'ntn 1')},
    'f': {('F32', 0): ('d32', 'narrow 128x64'), ('SPLIT', 0): ('dsplit', 'form 0 64-wide'), ('WINOGRAD', 0): ('w23_f32', 'four-wave'), ('WINOGRAD', 1): ('w23_f32', 'split-K 1'),
          ('WINOGRAD', 2): ('w23_f32', 'split-K 2'), ('WINOGRAD', 4): ('w23_f32', 'split-K 4'), ('WSPLIT', 0): ('w23_h4', 'four-wave'), ('WSPLIT', 1): ('w23_h4', 'split-K 1'),
          ('WSPLIT', 2): ('w23_h4', 'split-K 2'), ('WSPLIT', 4): ('w23_h4', 'split-K 4'), ('WF43', 0): ('w43_16k32', 'ntn 1'), ('WF43F', 0): ('w43_16k32', 'ntn 1')},
    'g': {('F32', 0): ('d32', '128x128'), ('SPLIT', 0): ('dsplit', 'form 0 64-wide'), ('WINOGRAD', 0): ('w23_f32', 'four-wave'), ('WSPLIT', 0): ('w23_h4', 'four-wave'),
          ('WF43', 0): ('w43_8', 'ntn 3'), ('WF43F', 0): ('w43_8', 'ntn 3')},
    'u1': {('F32', 0): ('d32', 'folded narrow 128x64'), ('SPLIT', 0): ('dsplit', 'form 1 64-wide'), ('WF43F', 0): ('w43_up', 'k32 gather'), ('WF42U', 0): ('w42_up', 'sub-pixel phases')},
    'u2': {('F32', 0): ('d32', 'folded 256x64'), ('SPLIT', 0): ('dsplit', 'form 1 64-wide')},
    'zu1': {('F32', 0): ('d32', 'folded 128x128'), ('SPLIT', 0): ('dsplit', 'form 1 64-wide'), ('WF43F', 0): ('w43_up', 'k32 gather'), ('WF42U', 0): ('w42_up', 'sub-pixel phases')},
    'zu2': {('F32', 0): ('d32', 'folded narrow 128x64'), ('SPLIT', 0): ('dsplit', 'form 1 64-wide'), ('WF43F', 0): ('w43_up', 'k32 gather'), ('WF42U', 0): ('w42_up', 'sub-pixel phases')},
}


def test_routes_against_the_table_of_expected_forms(cc):
    got = {key: {(n, sk): (r, f) for n, sk, r, f in rows} for key, rows in cc.routes().items()}
    assert got == EXPECTED_FORMS
    reached = {r for rows in got.values() for r, _ in rows.values()}
    assert reached == set(cc.ROUTES)
    forms = {(r, f) for rows in got.values() for r, f in rows.values()}
    assert {('d32', '256x64'), ('d32', '128x128'), ('d32', 'narrow 128x64'), ('w43_8', 'ntn 3'), ('w23_f32', 'split-K 4'), ('w23_h4', 'split-K 4')} <= forms
    # refusals: no route
    from codeformer_amd import ops
    assert cc.route_of(ops.SPLIT, 16, 16, 16, 64) is None and cc.route_of(ops.WF16, 16, 16, 16, 64) is None
    assert cc.route_of(ops.WF43, 16, 16, 512, 64) is None and cc.route_of(ops.WF43, 16, 16, 32, 128, up=True) is None
    assert cc.route_of(ops.WINOGRAD, 16, 16, 256, 64, split_k=4) is None and cc.route_of(ops.WF43F, 32, 32, 64, 128, c_split=16) is None
    # the sub-pixel form, by the rule of cf_wf43_launch: an upsampling launch of one input on whole slabs, channel tiles and 16x16 input blocks -- and
    # nothing of the ops.f43_up_ok policy (no smallest size: 16x16 inputs are launched)
    up42 = lambda H, W, cin, cout, **kw: cc.route_of(ops.WF42U, H, W, cin, cout, **{'up': True, **kw})
    assert up42(16, 16, 32, 128) == ('w42_up', 'sub-pixel phases') and not ops.f43_up_ok(32, 128, 32, 32)
    assert up42(16, 16, 32, 128, up=False) is None and up42(16, 16, 48, 128) is None and up42(16, 16, 32, 64) is None and up42(16, 24, 32, 128) is None
    assert up42(8, 16, 32, 128) is None and up42(16, 16, 64, 128, c_split=32) is None and up42(16, 16, 128, 128, split_k=1) is None and up42(16, 16, 544, 128) is None


def test_the_library_accepts_every_launch_of_the_table(cc):
    """cf_conv2d_stats_parts runs a launch's validation and routing without starting a kernel: every (shape, code, split_k) of routes() passes it.
    Descriptors as tests/test_conv_dispatch_host.py builds them; operand and winograd fields from the packers' own table (ops._WINO)."""
    from test_conv_dispatch_host import D
    from codeformer_amd import build as cf_build
    from codeformer_amd import lib, ops
    cf_build.build()
    native = lib.load()
    dummy = ctypes.create_string_buffer(64)       # (a query dereferences nothing; it only wants in1 present where c1 > 0)
    for key, rows in cc.routes().items():
        B, H, W, cin, cout, cs, up = cc.SHAPES[key]
        for cname, sk, route, form in rows:
            code = cc.CODES[cname]
            operand, wino = (int(ops._WINO[code][4]), int(ops._WINO[code][5])) if code in ops._WINO else (ops.OPERAND_F16X2 if code == ops.SPLIT else 0, 0)
            cp = max(64, ops._cout_pad(cout)) if (code == 0 and up) else ops._cout_pad(cout) if code == 0 else cout
            c0 = cin if cs is None else cs
            fields = D(H, W, c0, cout, cp, upsample=int(up), bf16_mfma=operand, batch=B, stats_cpg=0, c1=cin - c0, winograd=wino, acc_scale=1.0, split_k=sk,
                       in0=ctypes.addressof(dummy), in1=ctypes.addressof(dummy) if cin - c0 else None)
            if code == ops.WF42U:
                fields['upsample'] = 2            # (what ops.conv2d enters for this packing: the sub-pixel phases; the output stays twice the input)
            d = lib.ConvDesc(**fields)
            got = native.cf_conv2d_stats_parts(ctypes.byref(d))
            assert got > 0, (key, cname, sk, route, lib.last_error())
            assert code != ops.WF42U or got == 4 * (H // 16) * (W // 16)      # one workgroup per phase and 16x16 input block


# ---- the sub-pixel F(4,2) form (w42_up) -------------------------------------------------------------------------------------------------------------
W42_FAMILIES = tuple(f for f in GATE_FAMILIES + SOLO_FAMILIES if f not in PROLOGUE_ONLY) + ('onehot_pixels',)
OLD_X = {'a': '92582c1860532c58', 'b': '247dff1910251f45', 'c': 'd9de3fb100fab667', 'd': '3acc8fffa4c2da42', 'e': '7b7c0985824c2d86', 'f': 'e5678036f11c7a23',
         'g': '377c9f00e12e59b2', 'u1': 'bf66bd9fba02b991', 'u2': '3c1397b9212ba5fc', 'zk1': '126bce5b0f6f9209', 'zk2': '9505c16f12c2f75b',
         'zk3': '57d428bd35acd34c', 'zk4': 'fa82475c09373db7', 'zk5': '5e2c471f9338ab85'}


def test_every_older_key_keeps_its_data(cc):
    """family() seeds by the sorted position of a key.  sha256 of family('mixed_cout', key)['x'] (the seeded draw itself), taken before zu1 / zu2
    existed: the checker's nine keys with the new ones behind them, and the zk* keys as tests/test_gpu_wf43_kparts.py appends them."""
    import hashlib
    from test_gpu_wf43_kparts import KSHAPES
    digest = lambda m, k: hashlib.sha256(m.family('mixed_cout', k)['x'].numpy().tobytes()).hexdigest()[:16]
    got = {k: digest(cc, k) for k in ALL_KEYS[:9]}
    plain = load_script('tools/conv_check.py')                  # as the K-part test loads it
    assert tuple(plain.SHAPES) == ALL_KEYS[:9] and min(KSHAPES) > max(plain.SHAPES) and min(plain.UP_SHAPES) > max(KSHAPES)
    plain.SHAPES.update(KSHAPES)
    got.update({k: digest(plain, k) for k in KSHAPES})
    print(got)
    assert got == OLD_X


def test_f42_evaluation_is_the_convolution_and_its_weights_are_the_packer_s(cc):
    """fp64 through wino42 == conv_case.reference(upsample=True) at every w42_up shape: the tiling, the phases and the interleave (the algebra on
    windows is pinned by tests/test_f42_transforms.py).  S is never below the folded direct sum and never above 4556.25 sum_c max|g_p,c| max|p_c|."""
    from codeformer_amd import ops
    for key in W42_KEYS:
        for fam in W42_FAMILIES + ('int_coded',):
            d, ref = cc.prepared(fam, key)
            assert d['pro'] == cc.PRO_NONE and d['epi'] == cc.EPI_NONE and d['up']
            want = cc.case_ref(d)
            S = cc._abs_eval(fam, key, 0, cc.F42)[0]
            y, _ = cc.wino42(d['x'].double(), d['w'])
            err = float(((y + d['b'].double() - want).abs() / (S + 1e-300)).max())
            assert tuple(y.shape) == tuple(want.shape) and err <= 1e-13, (fam, key, err)
            x = d['x'].double().abs()
            xp = torch.nn.functional.pad(x.permute(0, 3, 1, 2), (1, 1, 1, 1))
            H, W = x.shape[1:3]
            gmax = torch.zeros(d['w'].shape[:2], dtype=torch.float64)
            for p in range(4):
                a, b = p >> 1, p & 1
                g = ops.fold_phase_taps(d['w'].double(), a, b).abs()
                direct = torch.nn.functional.conv2d(xp[:, :, a:a + H + 1, b:b + W + 1], g).permute(0, 2, 3, 1)
                assert bool((S[:, a::2, b::2] >= direct * (1 - 1e-12)).all()), (fam, key, p)
                gmax = torch.maximum(gmax, g.amax((2, 3)))
            win = xp.unfold(2, 6, 4).unfold(3, 6, 4).amax((4, 5))                # (B, C, H / 4, W / 4): the union of a tile's four phase windows
            T = torch.einsum('bcyx,kc->byxk', win, gmax).repeat_interleave(8, 1).repeat_interleave(8, 2)
            assert bool((S <= (10.125 * 4 / 3 * 5) ** 2 * T * (1 + 1e-12)).all()), (fam, key, float((S / T.clamp_min(1e-300)).max()))
        w = cc.family('mixed_cout', key)['w']
        BT, G, AT = cc.mats(cc.F42)
        mine = torch.stack([torch.einsum('ia,kcab,jb->kcij', G, ops.fold_phase_taps(w.double(), p >> 1, p & 1), G) for p in range(4)])
        assert torch.equal(mine, ops.f42_weights(w))
        assert [float(m.abs().sum(1).max()) for m in (AT, G, BT)] == [10.125, 12 / 9, 5.0]


@pytest.mark.parametrize('key', W42_KEYS)
def test_f42_edits_exceed_the_gate_and_the_unedited_emulation_does_not(cc, key):
    """Two subtly wrong kernels, as edits of the emulation: (a) phase (a, b) multiplied with the taps folded for (b, a); (b) the products of one
    transform-domain position lost to the idle accumulator -- position 12, the thirteenth of the lower wave half, or position 24, the last of the upper.
    Each stands at >= 10 times the gate on some family at every shape; unedited, every family stays within half."""
    from codeformer_amd import ops
    route, code = 'w42_up', ops.WF42U
    edits = {'swapped fold': dict(fold=cc.swapped_fold), 'position 12 lost': dict(zero_positions=cc.IDLE_LOWER), 'position 24 lost': dict(zero_positions=cc.IDLE_UPPER)}
    worst = {name: (0.0, None) for name in edits}
    for fam in W42_FAMILIES:
        d, ref = cc.prepared(fam, key)
        tol = cc.gate(fam, key, route, code)
        r0, _ = cc.emulated(fam, key, route, code)
        assert r0 <= 0.5 and cc.bits_equal(cc.emulate(d, route, code), cc.emulate(d, route, code, fold=lambda a, b: (a, b), zero_positions=())), (fam, key, r0)
        for name, kw in edits.items():
            r, _ = cc.ratio(cc.emulate(d, route, code, **kw), ref, tol)
            print(f'{fam} {key} w42_up: {name} {r:.1f} of the gate (unedited {r0:.4f})')
            worst[name] = max(worst[name], (r, fam))
    for name, (r, fam) in worst.items():
        print(f'{key}: {name} is seen best by {fam}, {r:.1f} of the gate')
        assert r >= 10.0, (key, name, fam, r)
