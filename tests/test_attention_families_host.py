"""CPU only: what makes the gate of tests/test_gpu_attention.py a condition on the reference and not on the kernels.

For every input family of tools/attn_check.py and both flavours (8 heads x 64, 1 head x 512):
  * the committed fp32 emulation of attention (every product rounded, the head_dim products and the 256 keys accumulated strictly one
    after another) stays within 0.5 of the gate  5e-6 + 1e-5 |ref| + COEF 2^-24 sqrt(head_dim) L_r max|v|  against the fp64 reference,
    with COEF = 0.5 for every family (the issue's ceiling for a per-family raise is 2: none needed one), is finite, and meets the family's
    exact condition (ones: within 2^-16 of 1; dup: duplicated P columns bitwise equal);
  * onehot: the fp64 gap between the best and the second-best logit exceeds 104 in every row, and the emulation returns v[pi] bitwise;
  * the offset families carry a largest |logit| above 88.7 (where expf overflows / underflows to 0 without the max subtraction) from
    +90 on, in every row;
  * the peak families' largest logits and probabilities lie where the tool's docstring says.
"""
import pytest

from _tools import load_script


@pytest.fixture(scope='module')
def ac():
    return load_script('tools/attn_check.py')


def test_the_family_table_is_what_the_issue_lists(ac):
    assert ac.FLAVOURS == {'8x64': dict(heads=8, head_dim=64, scale=0.125, seed=1), '1x512': dict(heads=1, head_dim=512, scale=512 ** -0.5, seed=5)}
    assert ac.FAMILIES == ('uniform', 'peak4', 'peak12', 'peak40', 'onehot', 'offset+30', 'offset+90', 'offset-300', 'offset+3000', 'big',
                           'allsame', 'P uniform', 'P peak4', 'P offset+90', 'ones', 'dup')
    assert all(ac.COEF[f] == 0.5 for f in ac.FAMILIES) and ac.U == 2.0 ** -24 and ac.ONEHOT_GAP == 104.0
    # the duplicated keys: distinct targets, in other 32-key (attn512 waves), 64-key (attn64 waves / key groups) and 128-key (V halves) ranges
    targets = [j + s for j in ac.DUP_KEYS for s in ac.DUP_STEPS]
    assert len(set(targets) | set(ac.DUP_KEYS)) == len(targets) + len(ac.DUP_KEYS) and max(targets) < 256
    # the P readback of head_dim 512: four identities inside the 512 columns, on both sides of the chunk split and across it
    assert all(0 <= c and c + 64 <= 512 for c in ac.P512_COLS) and any(c < 256 < c + 64 for c in ac.P512_COLS)
    assert any(c + 64 <= 256 for c in ac.P512_COLS) and any(c >= 256 for c in ac.P512_COLS)


@pytest.mark.parametrize('flavour', ['8x64', '1x512'])
def test_fp32_sequential_emulation_is_within_half_the_gate(ac, flavour):
    for family in ac.FAMILIES:
        res = ac.case(flavour, family, kernel=False)
        print(ac.line(res))
        e = res['emu']
        assert e['finite'], (flavour, family)
        assert e['ratio'] <= 0.5, (flavour, family, e)
        assert e['special'] is not False, (flavour, family)
        assert (e['special'] is not None) == (family in ('onehot', 'ones', 'dup')), (flavour, family)


@pytest.mark.parametrize('flavour', ['8x64', '1x512'])
def test_onehot_gap_and_bitwise_gather(ac, flavour):
    import torch
    fl = ac.FLAVOURS[flavour]
    H, dh = fl['heads'], fl['head_dim']
    inp, P, L = ac._prepared(flavour, 'onehot')
    s = ac.heads_view(inp['q'], H, dh).double() @ ac.heads_view(inp['k'], H, dh).double().transpose(-1, -2) * fl['scale']
    top = s.topk(2, -1)
    gap = top.values[..., 0] - top.values[..., 1]
    print(f'{flavour} onehot: smallest fp64 gap {float(gap.min()):.1f}')
    assert float(gap.min()) > 104.0
    assert torch.equal(top.indices[..., 0], inp['pi'])                       # the best key of row r is pi(r)
    assert len({tuple(p.tolist()) for p in inp['pi'].reshape(-1, 256)}) == 2 * H   # a different permutation for every (image, head)
    want = ac.rows_view(torch.gather(ac.heads_view(inp['v'], H, dh), 2, inp['pi'][..., None].expand(-1, -1, -1, dh)))
    got = ac.emulate_out(ac._emulated_probs(flavour, 'onehot'), inp['v'], H, dh)
    assert ac.bits_equal(got, want)
    p = ac._emulated_probs(flavour, 'onehot')
    assert ((p == 0) | (p == 1)).all() and (p.sum(-1) == 1).all()             # exp underflowed to exactly 0 for every other key


@pytest.mark.parametrize('flavour', ['8x64', '1x512'])
def test_offset_families_cross_the_exp_range(ac, flavour):
    for c in ac.OFFSETS:
        inp, P, L = ac._prepared(flavour, f'offset{c:+d}')
        s_min, s_max = float(L.min()), float(L.max())
        print(f'{flavour} offset{c:+d}: largest |logit| per row {s_min:.1f} .. {s_max:.1f}')
        assert abs(s_min - abs(c)) <= 4.0 and abs(s_max - abs(c)) <= 4.0       # the common term c, plus the uniform family's |logit| <= ~3
        if abs(c) >= 90:
            assert s_min > 88.7
        # the answer is the uniform family's with channel 0 taken out of the dot product: probabilities stay spread out
        assert float(P.amax(-1).max()) < 0.1
    inp, P, L = ac._prepared(flavour, 'big')
    fl = ac.FLAVOURS[flavour]
    s = ac.heads_view(inp['q'], fl['heads'], fl['head_dim']).double() @ ac.heads_view(inp['k'], fl['heads'], fl['head_dim']).double().transpose(-1, -2) * fl['scale']
    print(f'{flavour} big: logits {float(s.min()):.1f} .. {float(s.max()):.1f}')
    assert float(s.max()) > 60.0 and float(s.min()) < -60.0                    # both signs


# (largest logit of a row, largest probability of a row): smallest and largest over the rows, as in the docstring of tools/attn_check.py
PEAK_RANGES = {
    ('8x64', 4): ((2.0, 7.0), (0.026, 0.77)),
    ('8x64', 12): ((5.9, 21.0), (0.46, 0.999998)),
    ('8x64', 40): ((20.0, 70.0), (0.9998, 1.0)),
    ('1x512', 4): ((3.3, 4.9), (0.096, 0.33)),
    ('1x512', 12): ((9.9, 15.0), (0.986, 0.99986)),
    ('1x512', 40): ((33.0, 49.0), (1.0 - 1e-12, 1.0)),
}


@pytest.mark.parametrize('flavour', ['8x64', '1x512'])
def test_peak_families_lie_where_the_docstring_says(ac, flavour):
    fl = ac.FLAVOURS[flavour]
    H, dh = fl['heads'], fl['head_dim']
    inp, P, L = ac._prepared(flavour, 'uniform')
    print(f'{flavour} uniform: largest |logit| {float(L.max()):.2f}, largest probability {float(P.max()):.4f} (median over the rows {float(P.amax(-1).median()):.4f})')
    assert float(L.max()) < 4.0 and float(P.max()) < 0.1 and float(P.amax(-1).median()) < 0.03      # what the old gate saw: every output an average
    for beta in ac.PEAKS:
        inp, P, L = ac._prepared(flavour, f'peak{beta}')
        s = ac.heads_view(inp['q'], H, dh).double() @ ac.heads_view(inp['k'], H, dh).double().transpose(-1, -2) * fl['scale']
        top, pm = s.amax(-1), P.amax(-1)
        (l_lo, l_hi), (p_lo, p_hi) = PEAK_RANGES[(flavour, beta)]
        print(f'{flavour} peak{beta}: largest logit {float(top.min()):.2f} .. {float(top.max()):.2f}, largest probability {float(pm.min()):.6f} .. {float(pm.max()):.6f}')
        assert l_lo * 0.97 <= float(top.min()) <= l_lo * 1.03 and l_hi * 0.97 <= float(top.max()) <= l_hi * 1.03
        assert p_lo * 0.97 <= float(pm.min()) <= min(1.0, p_lo * 1.03) and p_hi * 0.97 <= float(pm.max()) <= min(1.0, p_hi * 1.03)
        assert len({tuple(p.tolist()) for p in inp['pi'].reshape(-1, 256)}) == 2 * H
    # the duplicated keys of 'dup' are copies, and the query rows are those of peak4
    a, b = ac._prepared(flavour, 'dup')[0], ac._prepared(flavour, 'peak4')[0]
    assert ac.bits_equal(a['q'], b['q']) and ac.bits_equal(a['v'], b['v'])
    k = a['k'].view(2, 256, -1)
    assert all(ac.bits_equal(k[:, j], k[:, j + s]) for j in ac.DUP_KEYS for s in ac.DUP_STEPS)
