"""CPU: the evidence that the conditions of tests/test_gpu_misc_kernels.py are conditions on the REFERENCE, not on what a kernel returns.

For the cases of tools/misc_check.py:
  * row argmax: the shapes are the issue's; the integer inputs do hold exact ties of the maximum; the walking winner reaches every lane, every
    element of a 16-byte load and the first and last column; the tie rows put the tie where their comment says (one load, two lanes, two passes,
    lane 63 against lane 0 of the next pass); the NaN-aware reference is numpy.argmax wherever no NaN is present;
  * cf_row_sqnorm: the derived depth is at most the asserted dim / 4 + 7 at every dim; the integer input's sum is below 2^24; an fp32 emulation in
    the kernel's order stays within half the bound;
  * cf_vq_argmin: the integer family's every intermediate is below 2^24 and its duplicated and end codes are the unique minimum where claimed; the
    operation-order seed is the search's result and the two orders differ on its rows; the random family excludes at most 5 % of a case's rows
    (the issue's four cases: 0, 0, 0 and about 2 %), the fp32 emulation agrees with fp64 on every decided row and its dmin stays within half
    the bound;
  * layout: every element distinct and exact in fp32;
  * image boundary: all 256 bytes in every colour plane of every shape, every residue of hw mod 4, an image base that is not 4-byte aligned;
    the half-way values do sit between two bytes (the oracle gives k or k + 1 one fp32 spacing to either side), and every value reaches every pixel.
"""
import numpy as np
import pytest
import torch

from _tools import load_script


@pytest.fixture(scope='module')
def mc():
    return load_script('tools/misc_check.py')


# ---- row argmax ------------------------------------------------------------------------------------------------------------------------------
def test_argmax_cases_are_the_issue_s(mc):
    assert mc.ARGMAX_N == (4, 8, 20, 252, 256, 260, 516, 1024) and mc.ARGMAX_ROWS == (1, 3, 5, 8, 257) and mc.ARGMAX_KINDS == ('random', 'ints', 'walking')
    assert all(n % 4 == 0 for n in mc.ARGMAX_N) and all(r % mc.ROWS_PER_GROUP[r] == 0 for r in mc.ARGMAX_ROWS)
    assert any(r % 4 for r in mc.ARGMAX_ROWS) and min(mc.ARGMAX_N) == 4          # rows that do not fill a workgroup; the smallest legal row


def test_integer_rows_tie_and_the_walking_winner_walks(mc):
    for n in mc.ARGMAX_N:
        x = mc.argmax_input('ints', 257, n)
        assert int(((x == x.max(dim=1, keepdim=True).values).sum(dim=1) > 1).sum()) >= (200 if n >= 20 else 20), n
        cols = [mc.walking_column(r, n) for r in range(257)]
        w = mc.argmax_input('walking', 257, n)
        assert mc.argmax_reference(w).tolist() == cols
        assert ((w == w.max(dim=1, keepdim=True).values).sum(dim=1) == 1).all()
        assert {(c // 4) % 64 for c in cols} == set(range(min(64, n // 4))) and {c % 4 for c in cols} == {0, 1, 2, 3}, n
        assert {0, n - 1} <= set(cols[:3]) and {c // 256 for c in cols} >= {0, (n - 1) // 256}, n      # first and last pass
    assert [mc.walking_column(r, 20) for r in range(3)] == [0, 19, 1]


def test_tie_rows_sit_where_they_claim(mc):
    x, pairs = mc.tie_rows(1024)
    assert pairs == [(1, 2), (2, 9), (3, 259), (252, 256), (255, 256), (0, 1023), (5, 6, 7), (0, 1, 2, 3)]
    lane, load, pas = (lambda c: (c // 4) % 64), (lambda c: c // 4), (lambda c: c // 256)
    assert load(1) == load(2) and lane(2) != lane(9) and pas(2) == pas(9)
    assert lane(3) == lane(259) and pas(3) != pas(259)
    assert lane(252) == 63 and lane(256) == 0 and pas(252) < pas(256)              # the lower index sits in the higher lane
    for row, cols in zip(x, pairs):
        assert (row == row.max()).nonzero().view(-1).tolist() == list(cols)
    assert mc.tie_rows(4)[1] == [(1, 2), (0, 3), (0, 1, 2, 3)] and len(mc.tie_rows(260)[1]) == 8 and (3, 259) not in mc.tie_rows(256)[1]


def test_argmax_reference_is_numpy_argmax_and_skips_nan(mc):
    for n in (4, 20, 260):
        x = mc.argmax_input('ints', 8, n)
        assert np.array_equal(mc.argmax_reference(x).numpy(), x.numpy().argmax(axis=1))
        s, names = mc.special_rows(n)
        want = mc.argmax_reference(s)
        for r in range(6):                                                          # the rows without a NaN
            assert want[r] == int(s[r].numpy().argmax()), names[r]
        assert want[names.index('all NaN')] == 0x7fffffff and want[names.index('NaN then -inf')] == 1
        assert want[names.index('one NaN')] == int(torch.nan_to_num(s[6], nan=-float('inf')).argmax())
        gap, gmin = mc.gap_reference(s, 4)
        assert torch.isnan(gap).tolist() == [False, True, False, False, False, True] + [True] * 6 and torch.isnan(gmin).all()
        assert gap[2] == float('inf') and gap[3] == 4.0 and gap[4] == float('inf')


# ---- row sum of squares ----------------------------------------------------------------------------------------------------------------------
def test_sqnorm_bound_covers_the_derived_depth_and_the_emulation(mc):
    assert mc.SQ_DIMS == (4, 32, 256, 260, 1024) and mc.SQ_ROWS == (1, 5, 256)
    assert [mc.sqnorm_depth(d) for d in mc.SQ_DIMS] == [3, 6, 9, 10, 12]
    for dim in mc.SQ_DIMS:
        assert mc.sqnorm_depth(dim) <= dim / 4 + 7
        x = mc.sqnorm_input('ints', 256, dim)
        want = (x.double() ** 2).sum(1)
        assert float(want.max()) <= 49 * dim < 2 ** 24 and torch.equal(mc.sqnorm_emulate(x).double(), want)
        for kind in ('random', 'mixed'):
            x = mc.sqnorm_input(kind, 256, dim)
            ratio = float(((mc.sqnorm_emulate(x).double() - (x.double() ** 2).sum(1)).abs() / mc.sqnorm_bound(x)).max())
            assert ratio <= 0.5, (kind, dim, ratio)
    x = mc.sqnorm_input('mixed', 256, 1024)
    assert float(x.abs().max() / x.abs().median()) > 100


# ---- nearest code ----------------------------------------------------------------------------------------------------------------------------
def test_vq_exact_family_is_exact_in_fp32(mc):
    assert mc.VQ_NCODES == (4, 20, 256, 260, 1024) and mc.VQ_ROWS == (1, 5, 256)
    for ncodes in mc.VQ_NCODES:
        for kind in mc.VQ_EXACT_KINDS:
            c = mc.vq_exact_input(kind, 256, ncodes)
            s, zz, ee = c['ints']
            for t in (s.abs(), zz, ee, zz.view(-1, 1) + ee.view(1, -1), 2 * s.abs(), c['d'].abs()):
                assert int(t.max()) < 2 ** 24
            assert torch.equal(c['scores'].long(), s) and torch.equal(c['zz'].long(), zz) and torch.equal(c['ee'].long(), ee)
            widx, wmin = mc.vq_exact_reference(c['d'])
            eidx, emin = mc.vq_emulate(c['scores'], c['zz'], c['ee'])
            assert torch.equal(eidx, widx) and torch.equal(emin, wmin)
            if kind == 'dups':
                assert len(c['pairs']) >= (2 if ncodes == 4 else 3)
                for r in range(256):
                    cols = c['pairs'][r % len(c['pairs'])]
                    assert (c['d'][r] == 0).nonzero().view(-1).tolist() == list(cols) and widx[r] == cols[0]
            if kind == 'ends':
                assert widx.tolist() == [0 if r % 2 == 0 else ncodes - 1 for r in range(256)] and ((c['d'] == 0).sum(1) == 1).all()
    assert mc.vq_exact_input('dups', 5, 1024)['pairs'][:4] == [(1, 2), (3, 259), (252, 256), (0, 1023)]


def test_vq_order_case_separates_the_two_orders(mc):
    assert mc.order_search(0, mc.ORDER_SEED + 1) == mc.ORDER_SEED
    c = mc.order_case()
    a, _ = mc.vq_emulate(c['scores'], c['zz'], c['ee'], 'reference')
    b, _ = mc.vq_emulate(c['scores'], c['zz'], c['ee'], 'folded')
    assert len(c['rows']) >= 8 and all(a[r] != b[r] for r in c['rows'])
    assert float(2 * c['scores'].abs().max()) < 2 ** 127                            # 2 s is exact: a fused multiply-add cannot change (zz + ee) - 2 s


@pytest.mark.parametrize('name,excluded', [('r1024x256', 0.0), ('r512x32', 0.0), ('r20x260', 0.0), ('r1024x256_small_codes', 0.03)])
def test_vq_random_family_excludes_few_rows_and_the_emulation_holds(mc, name, excluded):
    rows, ncodes, dim, scale, source = mc.VQ_RANDOM[name]
    assert rows == 256 and (source == 'ops.linear') == (dim % 128 == 0 and ncodes % 64 == 0)
    ref = mc.vq_random_reference(name)
    frac = float((~ref['decided']).float().mean())
    assert frac <= mc.VQ_EXCLUDED_CAP == 0.05 and frac <= excluded + 0.005, (name, frac)
    z, e = mc.vq_random_input(name)
    idx, dmin = mc.vq_emulate(z @ e.t(), mc.sqnorm_emulate(z), mc.sqnorm_emulate(e))
    ok = ref['decided']
    assert torch.equal(idx[ok], ref['idx'][ok])
    assert float(((dmin.double() - ref['dmin']).abs() / ref['bound']).max()) <= 0.5
    assert mc.vq_random_reference(name) is ref                                      # computed once


# ---- layout ----------------------------------------------------------------------------------------------------------------------------------
def test_layout_inputs_are_distinct_and_exact(mc):
    assert mc.LAYOUT_B == (1, 3) and mc.LAYOUT_C == (1, 3, 19, 20, 32, 33, 64) and mc.LAYOUT_HW == ((1, 1), (5, 7), (8, 4), (33, 31))
    x = mc.layout_input(3, 64, 33, 31)
    assert x.numel() < 2 ** 24 and torch.equal(x.reshape(-1).long(), torch.arange(x.numel())) and mc.SENTINEL < 0


# ---- image boundary --------------------------------------------------------------------------------------------------------------------------
def test_image_cases_cover_both_paths_and_every_byte(mc):
    assert mc.IMG_SHAPES == ((1, 1, 1), (2, 1, 3), (3, 5, 7), (2, 3, 3), (1, 2, 2), (2, 8, 4), (1, 16, 16), (2, 2, 3))
    assert {h * w % 4 for _, h, w in mc.IMG_SHAPES} == {0, 1, 2, 3}          # (2, 2, 3) is here for residue 2: the issue's seven have none
    assert any(b > 1 and (h * w * 3) % 4 for b, h, w in mc.IMG_SHAPES)              # a second image whose first byte is not 4-byte aligned
    for B, H, W in mc.IMG_SHAPES:
        img = mc.u8_input(B, H, W)
        assert img.shape[1:] == (B, H, W, 3)
        for c in range(3):
            assert len(set(img[..., c].reshape(-1).tolist())) == 256
    img = mc.u8_input(1, 2, 2)[:1]
    want = mc.u8_to_tensor_reference(img)
    assert want.shape == (1, 1, 3, 2, 2) and want.dtype == torch.float32
    for (y, x, c) in ((0, 0, 0), (1, 1, 2), (0, 1, 1)):
        u = int(img[0, 0, y, x, c])
        assert float(want[0, 0, 2 - c, y, x]) == float((np.float32(u / 255.0) - np.float32(0.5)) / np.float32(0.5))
    full = mc.u8_to_tensor_reference(torch.arange(256, dtype=torch.uint8).view(256, 1, 1, 1).repeat(1, 1, 1, 3))
    assert float(full.min()) == -1.0 and float(full.max()) == 1.0 and (full[1:] > full[:-1]).all()


def test_image_values_straddle_every_rounding_boundary(mc):
    from oracle.codeformer_oracle import tensor2img_u8
    v = mc.img_values()
    assert v.numel() == 255 * 3 + 7 and torch.isnan(v[-1]) and not torch.isnan(v[:-1]).any()
    tri = v[:765].view(255, 3)
    assert (tri[:, 0] < tri[:, 1]).all() and (tri[:, 1] < tri[:, 2]).all()
    by = torch.from_numpy(tensor2img_u8(tri.reshape(1, 1, -1).repeat(3, 1, 1)).copy())[0, :, 0].view(255, 3).long()
    k = torch.arange(255)
    # each triple straddles byte k | k + 1 in exact arithmetic; in the reference's fp32 arithmetic (v + 1) / 2 * 255 may round a neighbour back onto
    # k + 0.5, where half-to-even decides -- which is what makes these the inputs at which a different evaluation order shows
    assert ((by == k.view(-1, 1)) | (by == k.view(-1, 1) + 1)).all() and (by[:, 0] <= by[:, 1]).all() and (by[:, 1] <= by[:, 2]).all()
    assert int((by[:, 0] != by[:, 2]).sum()) >= 120 and int((by[:, 0] == by[:, 2]).sum()) >= 16
    ends = torch.from_numpy(tensor2img_u8(v[765:771].reshape(1, 1, -1).repeat(3, 1, 1)).copy())[0, :, 0].tolist()
    assert ends == [0, 255, 0, 255, 0, 255]
    t = mc.img_input(3, 5, 7)
    assert t.shape == (772, 3, 3, 5, 7)
    idx = {float(x) for x in v[:-1].tolist()}
    for pix in ((0, 0, 0, 0), (2, 1, 4, 6), (1, 2, 4, 4)):                           # first pixel, the last of the partial quad, another plane
        col = t[:, pix[0], pix[1], pix[2], pix[3]]
        assert {float(x) for x in col[~torch.isnan(col)].tolist()} == idx and int(torch.isnan(col).sum()) == 1
    want = mc.img_reference(t[:2])
    assert want.shape == (2, 3, 5, 7, 3) and want.dtype == torch.uint8
    one = tensor2img_u8(torch.nan_to_num(t[1, 2], nan=0.0))
    keep = ~torch.isnan(t[1, 2]).permute(1, 2, 0).flip(-1)
    assert torch.equal(want[1, 2][keep], torch.from_numpy(one.copy())[keep]) and (want[1, 2][~keep] == mc.NAN_BYTE).all()
