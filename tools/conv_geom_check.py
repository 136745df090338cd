"""The stride-2, 1x1 and general-geometry convolutions per element: what tools/conv_check.py does for 3x3 stride 1 on whole tiles, for every other form
cf_conv2d dispatches to with fp32 or split-half operands.  Library of tests/test_gpu_conv_geom.py (GPU) and tests/test_conv_geom_host.py (CPU); the
families, rnd, prologue64, act_scale_of, _halves, ratio, bits_equal and U are conv_check's own (family_at: its recipes at another geometry).
usage (GPU box): python tools/conv_geom_check.py [--ends] [--prelu]    one line per (family, case, route): kernel error, emulation error, both as parts of the gate
(--prelu: with the PReLU instantiations, PRELU_CASES -- the library of tests/test_gpu_conv_prelu.py and tests/test_conv_prelu_host.py; see with_prelu())
(--ends: with the NCHW ends, END_CASES -- the library of tests/test_gpu_conv_ends.py and tests/test_conv_ends_host.py; see with_nchw_ends())
Out of scope: the single-16-bit direct forms (pack_weight(f16=True) / bf16 operands) and bf16 tensors (io_bf16).

Geometry (Geo; CASES: key -> Geo): B, H, W of the INPUT, cin, cout, c_split | taps 1 | 9, stride 1 | 2, up (nearest x2 first), pad_mode, pad_lo,
sliced (x = buf[..., 16:48] of an 80-wide buffer, x2 = buf2[..., :32] of a 48-wide one, out = obuf[..., 32:96] of a 128-wide one; res / res2 share the
output's stride), epi (LEAKY / AXPY / AXPY2 / PRELU / RES_PRELU, on the NCHW input end RESIDUAL / SFT: the case's own epilogue instead of the family's), alpha (the
PReLU slope of the case, one of SLOPES = tests/arcface_ref.SLOPES: -0.5, 0, 0.25, 1.5 -- negative, zero, ordinary, above one, two significant bits at most), out_nchw, in_nchw
(the family's NHWC input is handed over as its NCHW permutation; the reference is unchanged).  Nothing above 128x128x32 in or 64x64x384 out.
The fp64 reference is written from the definitions: padded() builds the image the definition convolves -- F.pad(.., (0, 1, 0, 1)) for stride 2 with
pad_lo = 0, one row / column of zeros (padding = 1) or mode='reflect' on every side for pad_lo = 1 and for stride 1, nearest x2 and THEN reflect padding
of the upsampled image for PAD_EDGE -- and an unpadded F.conv2d of the case's stride follows; taps 1 is a matrix product.  Epilogues as the header
writes them: LEAKY pre > 0 ? pre : 0.2f pre; AXPY pre alpha + res; AXPY2 (pre alpha + res) alpha + res2, alpha = sft_w as the float the descriptor
carries (0.2f and float(alpha) are the kernel's constants: the reference takes them as given, so they enter no gate); PRELU t = pre, RES_PRELU t = pre + res,
out = t > 0 ? t : a t -- a select on the sign of t, never max(t, a t).
tests/test_conv_geom_host.py holds the reference against an index-by-index loop for each padding rule.

Routes (ROUTES; route_of() restates conv_validate's `ext` predicate, launch_direct, launch_ladder, conv1x1_mtiles (cf_igemm.hip) and cf_split_launch;
weights are packed with the explicit code 0 or ops.SPLIT (stride2=True / a 1x1 weight), never through ops.conv_code; fp32 1x1 launches pass split_k=0):
  s2_d32     code 0   stride 2: `64-wide` launch<9,2,2,2,2,1> / `128-wide` <9,2,2,2,2,2> (cout_pad % 128 == 0 and (Ho Wo / 128) (cout_pad / 128) > 64) /
                      `ext` (pad_lo = 1 or reflect: any size, cout_pad % 128 == 0)
  s2_dsplit  SPLIT    the space-to-depth form: `128-wide` (more than 64 128-wide workgroups per image), else `64-wide skip` (c0 % 32 == 0: the structurally
                      zero (tap, parity) blocks are skipped) / `64-wide no-skip` (c0 % 32 == 16: they are multiplied)
  c1_d32     code 0   taps 1: `256x64` (cout_pad 64), `128x128`, `narrow 128x64` (cout_pad % 128 == 0, <= 1024 pixels); rows per image % tile rows == 0
  c1_dsplit  SPLIT    the streaming 1x1 form, > 1024 pixels: `64-wide`, `128-wide`
  ext_d32    code 0   the EXT instantiations of 3x3 stride 1 (off-grid size, reflect, channel slices, LEAKY / AXPY / AXPY2): rungs `128`, `64`, `32`
  ext_up     code 0   the EXT instantiations of the folded upsample (off-grid source, PAD_EDGE): rungs `128`, `64`
  d32_32     code 0   the dense 32-wide rung (cout_pad == 32 on whole 16x16 tiles)
  (the route below is PRELU_CASES', merged in by with_prelu())
  prelu      code 0   the five igemm_kernel<.., PRELU = true> instantiations behind CF_EPI_PRELU / CF_EPI_RES_PRELU (route_of() restates the `f.ext &&
                      d->epilogue >= CF_EPI_PRELU` branch of launch_direct and conv_validate's narrow = cout_pad % 128 == 0 && hout wout <= 1024): `s2` (stride 2,
                      pad_lo 0 and 1; the residual has the output's shape), `narrow` (8x8 and 32x32 = exactly 1024 pixels, the predicate's last size), `128` (25x41 =
                      1025 pixels, the first size past it, off-grid), `64` (19x35), `32` (9x5).  Thirteen cases q*: every form sees a negative slope and one above
                      one, slopes 0 and 0.25 on q64c, q32c, qs1p; every form has a case of cin 32 (two K slabs; qna: 64, four).  ArcFace's pairings are among the
                      families: prologue AFFINE + PRELU (conv1 with bn0: mixed_cout, mixed_cin, cancel_pairs on the PRELU cases) and prologue none + RES_PRELU
                      (conv2: dc_plus_ripple, mixed_cin_act, int_coded variant 0 on the RES_PRELU cases).  The packer has no cout_pad of 96
                      (ops._cout_pad(96) is 128), so the 32-wide form exists at cout <= 32 only.
  (the forms below that no case of CASES reaches -- `few_cout 4`, `few_cout 3` and the whole nchw_in route -- are END_CASES', merged in by with_nchw_ends())
  head       code 0   the few-channel NCHW head (cout <= 4, out_nchw): `few_cout reflect` (cout 3, reflect padding), and under zero padding `few_cout 4`
                      (cout 1, 2, 4: conv3x3_few_cout_kernel<4>) and `few_cout 3` (<3>), at 21x37 and 16x16 with c0 = 16, 32, 64 (1, 2, 4 chunks of the two-slab gather)
  nchw_in    code 0   the NCHW input end (c0 <= 4, cout_pad 64, no prologue, whole 16x16 tiles): `few_cin 3` (conv3x3_few_cin_kernel<3>), `few_cin n`
                      (<0>: c0 = 1, 2, 4) -- cout = 64 without an epilogue, statistics none or two channels per group -- and `mfma`, launch<9,1,4,1,2,2,true>,
                      for everything else: here an epilogue of the case's own (residual, SFT).  Off the 16x16 grid NO launch exists: the MFMA form is not an
                      EXT instantiation (EXT reads NHWC) and refuses the size by its tile check (OFF_GRID_NCHW; a test of the refusal on both sides).
A dense 3x3 stride-1 shape on whole tiles with cout_pad 64 / 128 is conv_check's: route_of() hands it there.

Families: conv_check.family_at at the case's geometry (seed 3000 + 17 * the case's index), with these additions:
  int_coded      variants 0..3 as conv_check (prologue none / affine, epilogue none / residual / SFT) where the route has them (s2_dsplit: 0, 3); the cases with an epilogue
                 of their own take it with alpha = 0.5 (AXPY / AXPY2 stay exact; LEAKY is ONE rounding of 0.2f pre).  nchw_in: variants 0 and 3; K is at most
                 36 there and every operand has three bits, so exactness is trivial (accumulators below 2^12 units) -- the family checks addressing, not rounding.
  onehot_pixels  onehot_positions(): per image the corners and edge midpoints (even images) or rows / columns 1 and n - 2 (odd images: a reflected border
                 doubles those, a replicated one does not), then both sides of every tile boundary of the route's grid (rows 8 s k, columns 16 s k, s the
                 stride; at stride 2 the coordinates b - 2 .. b + 1, each with an odd and an even partner coordinate, so all nine taps pass through all
                 four space-to-depth slots; the last, partial tile of an off-grid size has its boundary in the list like any other), then whatever fits.
                 At most cin pixels per image, one per channel -- on the NCHW input end up to 64, several per channel (channel (i + 5 image) % cin), which
                 puts the four corners, a pixel on each edge and both sides of every 16-pixel tile border into every case.
  tap_shift      at stride 2 the decimated shift, at taps 1 a signed channel permutation (one variant).
  mixed_cout, mixed_cin, mixed_cin_act, cancel_pairs, dc_plus_ripple (taps 1: the weights sum to ~0 over the input channels), swish_leaky_edges[_sft]:
                 unchanged recipes.  A family whose prologue or epilogue the route lacks is dropped where that is its point (mixed_cin and
                 swish_leaky_edges: the affine prologue, which s2_dsplit refuses; swish_leaky_edges: residual, _sft: SFT) and runs without it
                 otherwise (family_of() returns None / prologue none / epilogue none).  nchw_in has no prologue: mixed_cin and swish_leaky_edges are dropped,
                 the others run with prologue none.  A recipe that needs more channels than the case has is dropped too (buildable(): mixed_cout at
                 cout 1, mixed_cin_act at c0 1, cancel_pairs at c0 1 and 3).

  solo_cin, solo_cin_act   (SOLO_FAMILIES, on SOLO_ROUTES: the two split-half routes and their fp32 partners) conv_check's recipe: one input channel per output
                 channel over 32 binades of channel scales, every other weight an exact zero.  s2_dsplit refuses the affine prologue that solo_cin is about.
                 They are not in GATE_FAMILIES: the other routes have no split halves to lose.

Gate, against fp64, PER ELEMENT, the form of conv_check.gate (u = 2^-24):    gate = c u S + P + floor + epilogue terms
  S      the definition's own convolution with |w| and |p(x)| on the padded image: a reflected or replicated pixel counts as often as it is read.
  c      taps cin for the fp32 chains (the head's FMA chain included), + 3 with folded taps; 3 taps cin + 12 for split halves -- at stride 2 the
         space-to-depth form's structural zeros add exact zeros, so 27 cin + 12 stands.  nchw_in: 9 c0 (the MFMA form pads K to 16 per tap with exact
         zeros); the vector kernel starts its chain AT the bias, so every partial sum carries it: + c u |b| on `few_cin 3` / `few_cin n`.
  P      conv_check's prologue term through the same padded convolution with |w|.
  floor  the two split-half routes: 2^-25 (1 + 2^-10) (sum |p(x)| / scale + sum |w| / s), as conv_check.
  epilogue (g0 = the terms above + the bias rounding 2 u |pre|; every rounding at a whole ulp, 2 u |value|)
         residual 2 u |out|; SFT as conv_check.
         LEAKY   out = pre > 0 ? pre : fl(0.2f pre): the map has slope <= 1, so g0 passes unchanged; one product: g0 + 2 u |out|
         AXPY    out = fl(fl(pre a) + res): |a| g0 + 2 u |a pre| + 2 u |out|
         AXPY2   t = fl(fl(pre a) + res), out = fl(fl(t a) + res2): a^2 g0 + 2 u (a^2 |pre| + |a t|) + 2 u |a t| + 2 u |out|
         PRELU   out = t > 0 ? t : fl(a t), t = pre: the map has slope <= max(1, |a|); where the computed and the true t differ in sign, |t| + |t'| = |t - t'|
                 and the same factor holds; one product: max(1, |a|) g0 + 2 u |out|
         RES_PRELU   t = fl(pre + res): max(1, |a|) (g0 + 2 u |t|) + 2 u |out|
         (int_coded stays exact: a = m 2^e with m = 1 or 3, so a t is a whole number of units 2^e and exactness_preconditions() holds 3 |t| below 2^24 of
         them; tap_shift is bitwise the float32 definition prelu32(): pre = +-x is exact, fl(pre + res) and fl(a t) are what float32 does.  swish_leaky_edges
         runs on the RES_PRELU cases, whose epilogue still adds the family's residual; swish_leaky_edges_sft drops out: EXT has no SFT.)
  The solo families take conv_check's two changes: c counts the ONE channel whose product exists (taps instead of taps cin), and the floor sums |p(x)| over
  that channel alone and enters the subnormal half's spacing whole, 2^-24.  At taps 1 in fp32 the whole sum is one product: its rounding, and the affine
  prologue's two, are then single roundings that attain their u, and go in at a whole ulp each (c = 2, 2 P) -- found by the host test, whose emulation
  stood at 0.96 (prologue none) and 0.60 (affine) of the gate without them.
emulate() is the fp32 CPU emulation of each operand scheme on the padded image (stride 2: the plain weight on the padded image; the folded forms: the
unfolded weight on the upsampled one); tests/test_conv_geom_host.py asserts it within 0.5 of the gate for every gate family, route and case.  No
constant here was fitted to what a kernel returns.

Non-finite inputs (expected_reach()): an output is non-finite exactly where its window under the case's stride and padding rule holds the pixel --
except in the split-half stride-2 form where c0 % 32 != 0 (or under CF_S2_SKIP=0): there the structurally zero weight blocks are multiplied, 0 * NaN
is NaN, and the reach is the 2x2 window of the space-to-depth view, input rows 2 oy .. 2 oy + 3 and columns 2 ox .. 2 ox + 3 (include/codeformer_hip.h).
"""
import collections
import functools
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import conv_check as cc  # noqa: E402
from codeformer_amd import ops  # noqa: E402
from conv_check import U, _halves, act_scale_of, bits_equal, prologue64, ratio, rnd  # noqa: E402,F401
from conv_case import stats_rel_err  # noqa: E402,F401

PRO_NONE, PRO_AFFINE, PRO_AFFINE_SWISH, PRO_LEAKY = ops.PRO_NONE, ops.PRO_AFFINE, ops.PRO_AFFINE_SWISH, ops.PRO_LEAKY
EPI_NONE, EPI_RESIDUAL, EPI_SFT, EPI_LEAKY, EPI_AXPY, EPI_AXPY2 = ops.EPI_NONE, ops.EPI_RESIDUAL, ops.EPI_SFT, ops.EPI_LEAKY, ops.EPI_AXPY, ops.EPI_AXPY2
EPI_PRELU, EPI_RES_PRELU = ops.EPI_PRELU, ops.EPI_RES_PRELU
PRELU_EPIS = (EPI_PRELU, EPI_RES_PRELU)
SLOPES = (-0.5, 0.0, 0.25, 1.5)        # tests/arcface_ref.SLOPES: negative, zero, ordinary, above one; at most two significant bits each
PAD_ZERO, PAD_REFLECT, PAD_EDGE = ops.PAD_ZERO, ops.PAD_REFLECT, ops.PAD_EDGE
SLOPE = float(np.float32(0.2))
ROUTES = ('s2_d32', 's2_dsplit', 'c1_d32', 'c1_dsplit', 'ext_d32', 'ext_up', 'd32_32', 'head')
END_ROUTES = ('head', 'nchw_in')       # the routes of END_CASES (with_nchw_ends() appends the new one to ROUTES)
SPLIT_ROUTES = ('s2_dsplit', 'c1_dsplit')
CODES = {'F32': 0, 'SPLIT': ops.SPLIT}
SOLO_FAMILIES = cc.SOLO_FAMILIES        # one input channel per output channel: on the two split-half routes and their fp32 partners (SOLO_ROUTES)
SOLO_ROUTES = ('s2_d32', 's2_dsplit', 'c1_d32', 'c1_dsplit')
GATE_FAMILIES = cc.GATE_FAMILIES
SLICE = dict(x=(80, 16), x2=(48, 0), out=(128, 32))      # (buffer width, first channel) of the sliced case

Geo = collections.namedtuple('Geo', 'B H W cin cout c_split taps stride up pad_mode pad_lo sliced epi out_nchw in_nchw alpha')


def G(B, H, W, cin, cout, c_split=None, taps=9, stride=1, up=False, pad_mode=PAD_ZERO, pad_lo=0, sliced=False, epi=None, out_nchw=False, in_nchw=False, alpha=None):
    assert (alpha is not None) == (epi in PRELU_EPIS) and (alpha is None or alpha in SLOPES)
    return Geo(B, H, W, cin, cout, c_split, taps, stride, up, pad_mode, pad_lo, sliced, epi, out_nchw, in_nchw, alpha)


CASES = {
    's2a': G(2, 32, 32, 16, 64, stride=2), 's2b': G(2, 32, 64, 64, 128, stride=2), 's2c': G(1, 128, 128, 32, 384, stride=2),
    's2d': G(1, 32, 32, 32, 64, stride=2),
    's2z': G(2, 20, 36, 32, 128, stride=2, pad_lo=1), 's2r': G(2, 20, 36, 32, 128, stride=2, pad_lo=1, pad_mode=PAD_REFLECT),
    'p1a': G(2, 32, 48, 32, 64, taps=1), 'p1b': G(2, 32, 48, 96, 128, c_split=64, taps=1), 'p1c': G(1, 64, 64, 32, 384, taps=1),
    'p1d': G(2, 16, 32, 48, 128, taps=1),
    'e1z': G(2, 19, 35, 32, 64), 'e1r': G(2, 19, 35, 32, 64, pad_mode=PAD_REFLECT),
    'e2z': G(2, 24, 40, 64, 128), 'e2r': G(2, 24, 40, 64, 128, pad_mode=PAD_REFLECT),
    'e3z': G(1, 9, 5, 16, 32), 'e3r': G(1, 9, 5, 16, 32, pad_mode=PAD_REFLECT),
    'sl': G(2, 16, 16, 64, 64, c_split=32, sliced=True),
    'epl': G(2, 16, 16, 32, 64, epi=EPI_LEAKY), 'epa': G(2, 16, 16, 32, 64, epi=EPI_AXPY), 'epa2': G(2, 16, 16, 32, 64, epi=EPI_AXPY2),
    'u1z': G(2, 7, 11, 32, 64, up=True), 'u1e': G(2, 7, 11, 32, 64, up=True, pad_mode=PAD_EDGE),
    'u2z': G(1, 10, 18, 32, 128, up=True), 'u2e': G(1, 10, 18, 32, 128, up=True, pad_mode=PAD_EDGE),
    'd32': G(1, 16, 16, 16, 32),
    'hd': G(2, 21, 37, 32, 3, pad_mode=PAD_REFLECT, out_nchw=True),
}
# ---- the NCHW ends (tests/test_gpu_conv_ends.py, tests/test_conv_ends_host.py).  They live in END_CASES, beside CASES: ROUTES, CASES and everything derived from
# them are what tests/test_gpu_conv_geom.py and tests/test_conv_geom_host.py pin, and stay.  with_nchw_ends() merges them into THIS module object
# (tests/_tools.load_script gives every caller a fresh one), after which every function here serves both sets.
# the input end (the network's first layer): c0 = 3 and c0 in {1, 2, 4} on one and on six 16x16 tiles; the MFMA form through an epilogue of the case's own
END_CASES = {f'n{c}{t}': G(2, H, W, c, 64, in_nchw=True) for c in (3, 1, 2, 4) for t, (H, W) in (('a', (16, 16)), ('b', (32, 48)))}
END_CASES.update({'nm3a': G(2, 16, 16, 3, 64, in_nchw=True, epi=EPI_RESIDUAL), 'nm3b': G(2, 32, 48, 3, 64, in_nchw=True, epi=EPI_SFT)})
# the output end under zero padding: cout in {1, 2, 4} (conv3x3_few_cout_kernel<4>) and 3 (<3>), off and on the tile grid, one, two and four 16-channel
# chunks (the two-slab gather has an odd and an even count to get right)
END_CASES.update({f'h{n}{t}{c}': G(2, H, W, c, n, out_nchw=True) for n in (1, 2, 4, 3) for t, (H, W) in (('a', (21, 37)), ('b', (16, 16))) for c in (16, 32, 64)})
# ---- the PReLU instantiations (route `prelu`; tests/test_gpu_conv_prelu.py, tests/test_conv_prelu_host.py): like the NCHW ends they live beside CASES and
# are merged in by with_prelu(), so what the earlier test files pin stays.  The smallest shapes that reach each form and its edges; the slope is the case's own
PRELU_CASES = {
    'q64a': G(2, 19, 35, 32, 64, epi=EPI_PRELU, alpha=-0.5), 'q64b': G(2, 19, 35, 32, 64, epi=EPI_RES_PRELU, alpha=1.5),
    'q64c': G(2, 19, 35, 32, 64, epi=EPI_PRELU, alpha=0.0),
    'q32a': G(1, 9, 5, 16, 32, epi=EPI_PRELU, alpha=1.5), 'q32b': G(1, 9, 5, 32, 32, epi=EPI_RES_PRELU, alpha=-0.5),
    'q32c': G(1, 9, 5, 16, 32, epi=EPI_RES_PRELU, alpha=0.25),
    'qna': G(2, 8, 8, 64, 128, epi=EPI_RES_PRELU, alpha=-0.5), 'qnb': G(1, 32, 32, 32, 128, epi=EPI_PRELU, alpha=1.5),
    'q128a': G(1, 25, 41, 32, 128, epi=EPI_PRELU, alpha=-0.5), 'q128b': G(1, 25, 41, 32, 128, epi=EPI_RES_PRELU, alpha=1.5),
    'qs0': G(2, 20, 36, 32, 128, stride=2, epi=EPI_PRELU, alpha=1.5), 'qs1': G(2, 20, 36, 32, 128, stride=2, pad_lo=1, epi=EPI_RES_PRELU, alpha=-0.5),
    'qs1p': G(2, 20, 36, 32, 128, stride=2, pad_lo=1, epi=EPI_PRELU, alpha=0.25),
}
PRELU_KEYS = tuple(PRELU_CASES)
PRELU_ROUTES = ('prelu',)
SEED_INDEX = {k: i for i, k in enumerate(sorted(CASES) + list(END_CASES) + list(PRELU_CASES))}       # (a case of CASES keeps the seed of its place in sorted(CASES))
OFF_GRID_NCHW = (G(2, 17, 19, 3, 64, in_nchw=True), G(2, 24, 40, 3, 64, in_nchw=True))       # refused: see route_of()
BIG = ('s2c', 'p1c')      # the cases that exist for a 128-wide form: tap_shift runs three of its nine taps there


def with_nchw_ends():
    """CASES and ROUTES of this module object with the NCHW ends in them."""
    global ROUTES
    CASES.update(END_CASES)
    if 'nchw_in' not in ROUTES:
        ROUTES = ROUTES + ('nchw_in',)
    routes.cache_clear()


def with_prelu():
    """CASES and ROUTES of this module object with the PReLU instantiations in them."""
    global ROUTES
    CASES.update(PRELU_CASES)
    if 'prelu' not in ROUTES:
        ROUTES = ROUTES + PRELU_ROUTES
    routes.cache_clear()


def out_hw(g):
    return (g.H // 2, g.W // 2) if g.stride == 2 else (2 * g.H, 2 * g.W) if g.up else (g.H, g.W)


# ---- routes ----------------------------------------------------------------------------------------------------------------------------------
def route_of(code, g):
    """(route, form) the explicit pack code reaches at a geometry, or None where the host (ops.pack_weight / ops.conv2d) or the C ABI refuses."""
    Ho, Wo = out_hw(g)
    px = Ho * Wo
    c0 = g.cin if g.c_split is None else g.c_split
    c1 = g.cin - c0
    epi = g.epi or EPI_NONE
    if g.in_nchw:
        # conv_validate: 3x3 stride 1, c0 <= 4, no prologue, cout_pad 64; never `ext` (its predicate excludes in_nchw only for the size: a slice, a
        # reflection or a LEAKY / AXPY epilogue makes the launch ext, and ext refuses in_nchw).  launch_direct: the vector kernel for cout = 64 on whole
        # 16x16 tiles without an epilogue (statistics: none or two channels per group), else launch<9,1,4,1,2,2,true> -- which is not an EXT
        # instantiation either and refuses a size off its 16x16 tile grid.  So NO in_nchw launch exists off that grid.
        if code != 0 or not 1 <= g.cin <= 4 or g.c_split is not None or g.taps != 9 or g.stride != 1 or g.up or g.out_nchw or g.sliced:
            return None
        if g.pad_mode != PAD_ZERO or g.pad_lo or epi not in (EPI_NONE, EPI_RESIDUAL, EPI_SFT) or (g.cout % 4 and epi != EPI_NONE):
            return None
        if ops._cout_pad(g.cout) != 64 or g.H % 16 or g.W % 16:
            return None
        if g.cout == 64 and epi == EPI_NONE:
            return 'nchw_in', 'few_cin 3' if g.cin == 3 else 'few_cin n'
        return 'nchw_in', 'mfma'
    # conv_validate, the checks every route shares
    if g.taps not in (1, 9) or g.stride not in (1, 2) or (g.stride == 2 and (g.taps != 9 or g.H % 2 or g.W % 2)):
        return None
    if g.up and (g.stride != 1 or g.taps != 9 or g.out_nchw):
        return None
    if c0 <= 0 or c0 % 16 or c1 % 16 or ((g.out_nchw or g.cout % 4) and epi != EPI_NONE):
        return None
    if (g.pad_mode == PAD_REFLECT and (g.taps != 9 or g.up or g.H < 2 or g.W < 2)) or (g.pad_mode == PAD_EDGE and not g.up) or (g.pad_lo and g.stride != 2):
        return None
    if g.out_nchw and (g.taps != 9 or epi != EPI_NONE):
        return None
    few_cout = g.taps == 9 and g.stride == 1 and g.out_nchw and g.cout <= 4 and not g.up and c1 == 0
    if code == ops.SPLIT:                                                # cf_split_launch (and _pack_split / conv2d's weight-form checks)
        if g.out_nchw or g.sliced or g.pad_mode != PAD_ZERO or g.pad_lo or epi not in (EPI_NONE, EPI_RESIDUAL, EPI_SFT) or g.cout % 64:
            return None
        if g.taps == 1:
            if g.cin % 32 or c0 % 32 or c1 % 32 or px <= ops.TOKEN_IMAGE_MAX or g.H % 8 or g.W % 16:
                return None                                              # (<= 1024 pixels: that weight form belongs to the token GEMM; conv2d refuses)
            tiles = (g.H // 8) * (g.W // 16)
            return 'c1_dsplit', '128-wide' if (g.cout % 128 == 0 and tiles * (g.cout // 128) > 64) else '64-wide'
        if g.stride == 2:
            if c1 or c0 % 16 or Ho % 8 or Wo % 16:
                return None
            tiles = (Ho // 8) * (Wo // 16)
            if g.cout % 128 == 0 and tiles * (g.cout // 128) > 64:
                return 's2_dsplit', '128-wide'
            return 's2_dsplit', '64-wide skip' if c0 % 32 == 0 else '64-wide no-skip'
        return cc.route_of(ops.SPLIT, g.H, g.W, g.cin, g.cout, g.up, 0, g.c_split)
    if code != 0:
        return None
    cp = max(64, ops._cout_pad(g.cout)) if g.up else ops._cout_pad(g.cout)
    ext = g.sliced or epi >= EPI_LEAKY or ((g.pad_mode != PAD_ZERO or g.pad_lo) and not (g.out_nchw and g.cout <= 4)) or \
        (g.taps == 9 and g.stride == 1 and not few_cout and (Ho % 16 != 0 or Wo % 16 != 0))
    if epi >= EPI_PRELU:                                                 # conv_validate: ext (epilogue >= LEAKY), fp32 operands, no upsample, NHWC
        if not (g.taps == 9 and (g.stride == 1 or cp % 128 == 0) and not g.out_nchw and g.cout % 4 == 0 and not g.up):
            return None
        # launch_direct, the `f.ext && d->epilogue >= CF_EPI_PRELU` branch; narrow is conv_validate's cout_pad % 128 == 0 && hout * wout <= 1024
        narrow = cp % 128 == 0 and px <= 1024
        return 'prelu', 's2' if g.stride == 2 else 'narrow' if narrow else '128' if cp % 128 == 0 else '64' if cp % 64 == 0 else '32'
    if ext:
        if not (g.taps == 9 and (g.stride == 1 or cp % 128 == 0) and not g.out_nchw and g.cout % 4 == 0 and epi != EPI_SFT) or (g.up and cp % 64):
            return None
        if g.stride == 2:
            return 's2_d32', 'ext'
        rung = '128' if cp % 128 == 0 else '64' if cp % 64 == 0 else '32'
        return ('ext_up', rung) if g.up else ('ext_d32', rung)
    if g.taps == 1:                                                      # launch_ladder<1> + conv1x1_mtiles (split_k = 0)
        rung, bm = ('narrow 128x64', 128) if (cp % 128 == 0 and px <= 1024) else ('128x128', 128) if cp % 128 == 0 else ('256x64', 256) if cp == 64 else (None, 1)
        return ('c1_d32', rung) if rung and px % bm == 0 else None
    if g.stride == 2:
        if Ho % 8 or Wo % 16:
            return None
        if cp % 128 == 0 and (px // 128) * (cp // 128) > 64:
            return 's2_d32', '128-wide'
        return ('s2_d32', '64-wide') if cp % 64 == 0 else None
    if few_cout:                                                         # (the ladder has no rung for cout_pad 32)
        return ('head', 'few_cout reflect' if g.pad_mode == PAD_REFLECT else 'few_cout 3' if g.cout == 3 else 'few_cout 4') if cp == 32 else None
    if g.up or cp != 32:
        return cc.route_of(0, g.H, g.W, g.cin, g.cout, g.up, 0, g.c_split)
    return 'd32_32', '256x32'


@functools.lru_cache(maxsize=None)
def routes():
    """{case: [(code name, code, route, form)]}: every launch the GPU test makes."""
    return {key: [(n, c, *r) for n, c in CODES.items() for r in (route_of(c, g),) if r is not None] for key, g in CASES.items()}


def launches(key, only_routes=None):
    return [row for row in routes()[key] if only_routes is None or row[2] in only_routes]


def cases_of(route):
    return [key for key in CASES if any(r == route for _, _, r, _ in routes()[key])]


def epilogues_of(route, form):
    if route == 'head' or form in ('few_cin 3', 'few_cin n'):
        return (EPI_NONE,)
    if route == 'prelu':
        return PRELU_EPIS
    if route in ('ext_d32', 'ext_up') or form == 'ext':
        return (EPI_NONE, EPI_RESIDUAL, EPI_LEAKY, EPI_AXPY, EPI_AXPY2)
    return (EPI_NONE, EPI_RESIDUAL, EPI_SFT)


# ---- the families ----------------------------------------------------------------------------------------------------------------------------
def onehot_positions(g, image=0):
    """Up to cin pixels of one image (the NCHW input end, cin <= 4: up to 64, several per channel), Chebyshev distance >= 3 apart (see the docstring)."""
    H, W, s = g.H, g.W, g.stride
    limit = 64 if g.in_nchw else g.cin
    side = (-2, -1, 0, 1) if s == 2 else (-1, 0)
    rows_b = [8 * s * k + o for k in range(1, H // (8 * s) + 1) for o in side if 0 <= 8 * s * k + o < H]
    cols_b = [16 * s * k + o for k in range(1, W // (16 * s) + 1) for o in side if 0 <= 16 * s * k + o < W]
    corners = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2 + 1), (H // 2 + 4, 0), (H // 2 + 5, W - 1)]
    inner = [(1, 1), (1, W - 2), (H - 2, 1), (H - 2, W - 2), (1, W // 2), (H - 2, W // 2 + 1), (H // 2 + 4, 1), (H // 2 + 5, W - 2)]
    cand = corners[:4] + inner[4:] if image % 2 == 0 else inner[:4] + corners[4:]
    # (the coordinates around one boundary are neighbours: their partners sit 3 apart and move on by 6 from one to the next; the image's parity
    #  shifts the partners by one, so over two images every coordinate meets both parities twice)
    pairs = [(r, q) for i, r in enumerate(rows_b) for q in (3 + 6 * (i % len(side)) + image % 2, 6 + 6 * (i % len(side)) + image % 2)]
    pairs += [(r, q) for i, q in enumerate(cols_b) for r in (3 + 6 * (i % len(side)) + image % 2, 6 + 6 * (i % len(side)) + image % 2)]
    # (one partner each, 3 apart along the boundary: first at stride 1, where a small image has no room for the pairs of both sides)
    single = [(r, 3 + 3 * (i % len(side)) + image % 2) for i, r in enumerate(rows_b)] + [(3 + 3 * (i % len(side)) + image % 2, q) for i, q in enumerate(cols_b)]
    cand += pairs + single if s == 2 else single + pairs
    cand += [(r, q) for r in rows_b for q in cols_b] + [(3, 3), (4, 11), (11, 4)]
    cand += [(r, q) for r in range(H) for q in range(W)]
    got = []
    for p in cand:
        if len(got) < limit and 0 <= p[0] < H and 0 <= p[1] < W and all(max(abs(p[0] - q[0]), abs(p[1] - q[1])) >= 3 for q in got):
            got.append(p)
    return got


def buildable(name, g):
    """A recipe needs its channels: mixed_cout spreads exponents over >= 2 output channels, mixed_cin[_act] over >= 2 input channels, cancel_pairs
    pairs the input channels up."""
    if name in SOLO_FAMILIES:
        return g.cin >= 2 and g.cout >= 2
    return not ((name == 'mixed_cout' and g.cout < 2) or (name in ('mixed_cin', 'mixed_cin_act') and g.cin < 2) or (name == 'cancel_pairs' and g.cin % 2))


@functools.lru_cache(maxsize=None)
def family(name, key, variant=0):
    """conv_check's recipe at the case's geometry; the case's own epilogue (Geo.epi) replaces the family's."""
    g = CASES[key]
    assert buildable(name, g), (name, key)
    seed = 3000 + 17 * SEED_INDEX[key]
    d = cc.family_at(name, (g.B, g.H, g.W, g.cin, g.cout, g.up), seed, variant, k=3 if g.taps == 9 else 1, out_hw=out_hw(g),
                     positions=lambda bi: onehot_positions(g, bi), key=key, bare_up=False)
    if g.epi is not None:
        d['epi'] = g.epi
    if g.alpha is not None:
        d['sft_w'] = g.alpha
    return d


def prologues_of(route):
    """s2_dsplit: none / leaky -- cf_split_launch refuses an affine prologue at stride 2 (its tables would be indexed by the space-to-depth channel)."""
    if route == 'nchw_in':                                 # (conv_validate: in_nchw has no prologue)
        return (PRO_NONE,)
    return (PRO_NONE, PRO_LEAKY) if route == 's2_dsplit' else (PRO_NONE, PRO_AFFINE, PRO_AFFINE_SWISH, PRO_LEAKY)


# what a family is ABOUT: without that prologue / epilogue it is not run at all; any other prologue / epilogue a route lacks is simply left out
POINT = {'mixed_cin': ('pro',), 'solo_cin': ('pro',), 'swish_leaky_edges': ('pro', 'epi'), 'swish_leaky_edges_sft': ('epi',), 'int_coded': ('pro',)}


def family_of(name, key, route, form, variant=0):
    """The family as the route can run it, or None where the route (or a case with an epilogue of its own) lacks what the family is about (POINT)."""
    if not buildable(name, CASES[key]):
        return None
    d, point = family(name, key, variant), POINT.get(name, ())
    if 'epi' in point and CASES[key].epi is not None:          # (the case's epilogue has replaced the family's)
        if not (name == 'swish_leaky_edges' and CASES[key].epi == EPI_RES_PRELU):      # (RES_PRELU still adds the family's residual)
            return None
    for what, have, none in (('pro', prologues_of(route), PRO_NONE), ('epi', epilogues_of(route, form), EPI_NONE)):
        if d[what] not in have:
            if what in point:
                return None
            d = dict(d, **{what: none})
    return d


def int_coded_variants(key, route, form):
    """The (prologue, epilogue) variants of int_coded a route takes: all four, without the SFT one on the EXT instantiations, prologue none / affine
    without an epilogue operand on the head; the cases with an epilogue of their own: prologue none / affine."""
    if route == 'nchw_in':       # no prologue: variants 0 and 3 (prologue none; 3 asks for a residual, which the vector kernel drops: there it repeats 0)
        return (0, 3)
    if CASES[key].epi is not None or route == 'head':
        return (0, 1)
    return tuple(v for v in range(4) if family('int_coded', key, v)['epi'] in epilogues_of(route, form) and family('int_coded', key, v)['pro'] in prologues_of(route))


def families_of(key):
    """The gate families of a case: all of them, except mixed_cout at p1c -- the 1x1 routes run it at p1a, p1b and p1d.  At one tap and 32 channels
    the floor is a worst case over 32 subnormal lo halves, and over p1c's 4096 x 384 outputs the CPU emulation itself comes to 0.60 of it (few terms,
    many trials), so the half-gate condition of the host test, which is what makes a gate a statement about the reference, cannot hold there."""
    return tuple(f for f in GATE_FAMILIES if not (key == 'p1c' and f == 'mixed_cout') and buildable(f, CASES[key]))


# ---- fp64 reference and gate -----------------------------------------------------------------------------------------------------------------
def padded(t, g):
    """NHWC (B, H, W, C) -> NCHW, the image the definition convolves WITHOUT further padding at the case's stride."""
    t = t.permute(0, 3, 1, 2)
    if g.taps == 1:
        return t
    if g.up:
        t = t.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    if g.stride == 2 and g.pad_lo == 0:
        assert g.pad_mode == PAD_ZERO
        return F.pad(t, (0, 1, 0, 1))
    return F.pad(t, (1, 1, 1, 1), mode='reflect' if g.pad_mode in (PAD_REFLECT, PAD_EDGE) else 'constant')


def conv64(tp, w, g):
    """The unpadded convolution (taps 1: the matrix product) of a padded() image -> NHWC."""
    if g.taps == 1:
        return tp.permute(0, 2, 3, 1) @ w.double().reshape(w.shape[0], -1).t()
    return F.conv2d(tp, w.double(), stride=g.stride).permute(0, 2, 3, 1)


def alpha_of(d):
    return float(np.float32(d['sft_w']))


def epilogue64(d, pre):
    r0, r1, e = d['res'].double(), d['ss'].double(), d['epi']
    if e == EPI_RESIDUAL:
        return pre + r0
    if e == EPI_SFT:
        return r0 + d['sft_w'] * (r0 * r1 + pre)
    if e == EPI_LEAKY:
        return torch.where(pre > 0, pre, SLOPE * pre)
    if e == EPI_AXPY:
        return pre * alpha_of(d) + r0
    if e == EPI_AXPY2:
        return (pre * alpha_of(d) + r0) * alpha_of(d) + r1
    if e in PRELU_EPIS:
        t = pre + r0 if e == EPI_RES_PRELU else pre
        return torch.where(t > 0, t, alpha_of(d) * t)
    return pre


def prelu32(d, pre32):
    """The two PReLU epilogues in float32 on a float32 `pre`, as the definition orders them: t = fl(pre + res), out = t > 0 ? t : fl(a t).  Where pre is
    exact in float32 (tap_shift) this IS the float32 result; the fp64 reference rounds a (pre + res) once and differs from it by a double rounding."""
    t = pre32 + d['res'] if d['epi'] == EPI_RES_PRELU else pre32
    return torch.where(t > 0, t, torch.tensor(alpha_of(d), dtype=torch.float32) * t)


def reference(d, g):
    p, _ = prologue64(dict(d, up=False))
    pre = conv64(padded(p, g), d['w'], g) + d['b'].double()
    return dict(pre=pre, out=epilogue64(d, pre))


def coef(route, g, live=None):
    """live: the number of input channels with a non-zero weight, where that is fewer than cin (the solo families: 1) -- a product with an exact
    zero is an exact zero in every scheme, and adding it never rounds."""
    n = g.taps * (g.cin if live is None else live)
    if n == 1 and route not in SPLIT_ROUTES:      # a solo 1x1 in fp32: the chain IS one product.  A single rounding attains its u, so it is entered at a whole
        n = 2                                     # ulp, as the bias and residual roundings are (the rule of gemm_check.gate): the emulation then stays within half
    return (3 * n + 12 if route in SPLIT_ROUTES else n) + (3 if g.up else 0)


def pack_scale_of(d, g):
    return ops.pack_scale(float(d['w'].abs().max()) * (4.0 if g.up else 1.0))


def _abs_eval(d, g):
    """(S, P, sum |p| over the window, sum |w| over the window) in fp64, each through the definition's convolution on the padded image."""
    p, ep = prologue64(dict(d, up=False))
    wa = d['w'].abs()
    S = conv64(padded(p.abs(), g), wa, g)
    P = conv64(padded(ep, g), wa, g) if bool((ep != 0).any()) else torch.zeros_like(S)
    if d.get('solo'):          # sum |p| over the channels that have halves in this output channel's sum: per output channel
        fv = conv64(padded(p.abs(), g), cc.live_channels(d)[:, :, None, None].float() * torch.ones_like(d['w']), g)
    else:
        fv = conv64(padded(p.abs(), g), torch.ones_like(d['w'][:1]), g)
    fu = conv64(padded(torch.ones_like(p[:1, :, :, :]), g), wa, g)
    return S, P, fv, fu


def gate_of(d, g, route, ref, form=None):
    """The tolerance per element (B, Ho, Wo, cout), fp64."""
    S, P, fv, fu = _abs_eval(d, g)
    solo = bool(d.get('solo'))
    live = int(cc.live_channels(d).sum(1).max()) if solo else None
    assert live in (None, 1)
    if solo and g.taps * live == 1 and route not in SPLIT_ROUTES:
        P = 2 * P      # one product is the whole sum: the affine prologue's two roundings (x sc, + sh), which prologue64 enters at the u each can attain, are
        #                single roundings on the way of ONE term and go in at a whole ulp like the product itself (coef)
    g0 = coef(route, g, live) * U * S + P + 2 * U * ref['pre'].abs()
    if form in ('few_cin 3', 'few_cin n'):      # the vector kernel STARTS its FMA chain at the bias: every partial sum carries it
        g0 = g0 + coef(route, g) * U * d['b'].double().abs()
    if route in SPLIT_ROUTES:
        s = act_scale_of(d)[:, None, None, None]
        g0 = g0 + (2.0 ** -24 if solo else 2.0 ** -25) * (1.0 + 2.0 ** -10) * (fv / pack_scale_of(d, g) + fu / s)
    r0, r1, e, out, pre = d['res'].double(), d['ss'].double(), d['epi'], ref['out'], ref['pre']
    if e == EPI_RESIDUAL:
        return g0 + 2 * U * out.abs()
    if e == EPI_SFT:
        w = d['sft_w']
        return g0 + 2 * U * ((w * r0 * r1).abs() + 2 * (w * (r0 * r1 + pre)).abs() + out.abs())
    if e == EPI_LEAKY:
        return g0 + 2 * U * out.abs()
    a = abs(alpha_of(d))
    if e == EPI_PRELU:
        return max(1.0, a) * g0 + 2 * U * out.abs()
    if e == EPI_RES_PRELU:
        return max(1.0, a) * (g0 + 2 * U * (pre + r0).abs()) + 2 * U * out.abs()
    if e == EPI_AXPY:
        return a * g0 + 2 * U * (a * pre.abs() + out.abs())
    if e == EPI_AXPY2:
        t = pre * alpha_of(d) + r0
        return a * a * g0 + 2 * U * (a * a * pre.abs() + a * t.abs()) + 2 * U * (a * t.abs() + out.abs())
    return g0


@functools.lru_cache(maxsize=None)
def prepared(name, key, route, form, variant=0):
    """-> (d, ref, gate) of a family on a route, or None where the route cannot run it."""
    d = family_of(name, key, route, form, variant)
    if d is None:
        return None
    g = CASES[key]
    ref = reference(d, g)
    return d, ref, gate_of(d, g, route, ref, form)


# ---- fp32 emulation ------------------------------------------------------------------------------------------------------------------------------
def emulate(d, g, route, act_halves=None):
    """The route's arithmetic in torch float32 -> (B, Ho, Wo, cout) float32: fp32 products, or split halves lo hi + hi lo + hi hi under the pack-time
    and range scales; the convolution as ONE matrix product over the unfolded padded image."""
    f = torch.float32
    split = route in SPLIT_ROUTES
    x, sc, sh = d['x'], d['sc'][:, None, None, :], d['sh'][:, None, None, :]
    s = act_scale_of(d).float()[:, None, None, None] if split else torch.ones(x.shape[0], 1, 1, 1)
    if d['pro'] in (PRO_AFFINE, PRO_AFFINE_SWISH):
        p = x * sc + sh
        if d['pro'] == PRO_AFFINE_SWISH:
            p = p * torch.sigmoid(p)
    elif d['pro'] == PRO_LEAKY:
        p = x * torch.where(x > 0, s, 0.2 * s)
    else:
        p = x * s
    scale = pack_scale_of(d, g) if split else 1.0
    xp = padded(p, g)
    cols = xp.permute(0, 2, 3, 1).reshape(x.shape[0], -1, g.cin) if g.taps == 1 else F.unfold(xp, 3, stride=g.stride).transpose(1, 2)
    wm = (d['w'].reshape(d['w'].shape[0], -1).t() * scale).contiguous()
    if split:
        ah, al = _halves(cols.contiguous())
        if act_halves is not None:            # (an edit of the activation's split: conv_check.drop_small_lo)
            ah, al = act_halves(cols, ah, al)
        bh, bl = _halves(wm)
        v = (al @ bh + ah @ bl) + ah @ bh
    else:
        v = cols @ wm
    v = v.reshape(x.shape[0], *out_hw(g), -1) * (1.0 / scale) / s + d['b']
    r0, r1, e = d['res'], d['ss'], d['epi']
    a = torch.tensor(d['sft_w'], dtype=f)
    if e == EPI_RESIDUAL:
        v = v + r0
    elif e == EPI_SFT:
        v = r0 + d['sft_w'] * (r0 * r1 + v)
    elif e == EPI_LEAKY:
        v = torch.where(v > 0, v, torch.tensor(0.2, dtype=f) * v)
    elif e == EPI_AXPY:
        v = v * a + r0
    elif e == EPI_AXPY2:
        v = (v * a + r0) * a + r1
    elif e in PRELU_EPIS:
        t = v + r0 if e == EPI_RES_PRELU else v
        v = torch.where(t > 0, t, a * t)
    assert v.dtype == f
    return v


@functools.lru_cache(maxsize=None)
def emulated(name, key, route, form, variant=0):
    d, ref, tol = prepared(name, key, route, form, variant)
    return ratio(emulate(d, CASES[key], route), ref, tol)


def exactness_preconditions(key, route, form):
    """int_coded on a route, every variant it takes: the operands fit 8 significand bits (directly and under the pack scale: hi halves exact, lo halves
    zero), every intermediate of the epilogue is a whole number of units and the sum of |products| through the epilogue stays below 2^24 units.
    -> the largest such sum in units."""
    g, worst = CASES[key], 0.0
    for variant in int_coded_variants(key, route, form):
        d, ref, _ = prepared('int_coded', key, route, form, variant)
        p, _ = prologue64(dict(d, up=False))
        for t, unit in ((p, 0.5), (d['w'].double(), 2.0 ** -5)):
            q = t / unit
            assert torch.equal(q, q.round()) and float(q.abs().max()) < 256
        for t in (p.float().numpy(), (d['w'] * pack_scale_of(d, g)).numpy()):
            hi, lo = cc.split_halves(t)
            assert np.array_equal(hi, t) and not lo.any()
        a = alpha_of(d) if d['epi'] in (EPI_AXPY, EPI_AXPY2) else d['sft_w'] if d['epi'] == EPI_SFT else 1.0
        if d['epi'] in PRELU_EPIS:      # a slope m 2^e with m = 1 or 3 (two significant bits): a t is a whole number of units 2^e, and 3 |t| stays below 2^24 of them
            a = {-0.5: 0.5, 0.0: 1.0, 0.25: 0.25, 1.5: 0.5}[alpha_of(d)]
        unit = 0.5 * 2.0 ** -5 * (a * a if d['epi'] == EPI_AXPY2 else a)
        assert math.log2(unit) == round(math.log2(unit))
        S = _abs_eval(d, g)[0] * (4 if g.up else 1)                       # (a folded tap is a sum of up to four weights)
        epi = float(max(d['b'].abs().max(), d['res'].abs().max() * (1 + d['ss'].abs().max()), d['ss'].abs().max()))
        tot = (float(S.max()) + epi + float(ref['out'].abs().max())) / unit * (3 if d['epi'] in PRELU_EPIS else 1)
        assert tot < 2.0 ** 24, tot
        worst = max(worst, tot)
        if d['epi'] != EPI_LEAKY:                                         # (LEAKY: fl(0.2f pre) is one rounding of an exact pre)
            q = ref['out'] / unit
            assert torch.equal(q, q.round()) and torch.equal(ref['out'], ref['out'].float().double())
        assert torch.equal(ref['pre'], ref['pre'].float().double())
    return worst


def expected_reach(g, route, form, r, q):
    """(Ho, Wo) bool: the outputs a non-finite input pixel (r, q) reaches (see the docstring)."""
    ind = torch.zeros(1, g.H, g.W, 1, dtype=torch.float64)
    ind[0, r, q, 0] = 1.0
    if route == 's2_dsplit' and form == '64-wide no-skip':
        return F.conv2d(F.pad(ind.permute(0, 3, 1, 2), (0, 2, 0, 2)), torch.ones(1, 1, 4, 4, dtype=torch.float64), stride=2)[0, 0] > 0
    k = 3 if g.taps == 9 else 1
    return conv64(padded(ind, g), torch.ones(1, 1, k, k), g)[0, :, :, 0] > 0


# ---- the kernels -----------------------------------------------------------------------------------------------------------------------------
_PW = {}


def packed(d, g, code, tag):
    k = (tag, code)
    if k not in _PW:
        w, b = d['w'].cuda(), d['b'].cuda()
        _PW[k] = ops.pack_weight(w, b, bf16=ops.SPLIT, stride2=g.stride == 2) if code == ops.SPLIT else ops.pack_weight(w, b, up2x=g.up)
    return _PW[k]


def into_slice(t, width, at):
    """t (.., C) as the channel slice [at, at + C) of a NaN-filled buffer `width` channels wide -> (view, buffer)."""
    buf = torch.full((*t.shape[:-1], width), float('nan'), dtype=t.dtype, device=t.device)
    buf[..., at:at + t.shape[-1]] = t
    return buf[..., at:at + t.shape[-1]], buf


def run(d, key, code, tag, x=None, images=None, stats=False, out=None, dense=False, keep=None, act_x=None):
    """One launch of a family's tensors at a case's geometry with the explicit pack code -> (B, Ho, Wo, cout) CUDA tensor (the head's NCHW planes as an
    NHWC view).  x: another input; images: a slice of the batch; out: a destination; dense: the sliced case on contiguous copies; keep: a dict that
    receives the buffers of the sliced case ('obuf', 'buf', 'buf2'); act_x: the tensor the range scale is taken from (default: the input)."""
    g = CASES[key]
    pw = packed(d, g, code, tag)
    sl = slice(None) if images is None else images
    xs = (d['x'] if x is None else x)[sl].contiguous().cuda()
    c0 = g.cin if g.c_split is None else g.c_split
    x1, x2 = xs[..., :c0].contiguous(), (xs[..., c0:].contiguous() if c0 < g.cin else None)
    if g.in_nchw:
        x1 = xs.permute(0, 3, 1, 2).contiguous()
    kw = dict(in_nchw=g.in_nchw, stride=g.stride, upsample=g.up, prologue=d['pro'], epilogue=d['epi'], pad_mode=g.pad_mode, pad_lo=g.pad_lo, out_nchw=g.out_nchw,
              emit_stats=stats, split_k=0)
    if d['pro'] in (PRO_AFFINE, PRO_AFFINE_SWISH):
        kw.update(scale=d['sc'][sl].contiguous().cuda(), shift=d['sh'][sl].contiguous().cuda())
    res = d['res'][sl].contiguous().cuda() if d['epi'] in (EPI_RESIDUAL, EPI_SFT, EPI_AXPY, EPI_AXPY2, EPI_RES_PRELU) else None
    ss = d['ss'][sl].contiguous().cuda() if d['epi'] in (EPI_SFT, EPI_AXPY2) else None
    if d['epi'] in (EPI_SFT, EPI_AXPY, EPI_AXPY2) + PRELU_EPIS:
        kw['sft_w'] = d['sft_w']
    if g.sliced and not dense:
        (x1, buf), (x2, buf2) = into_slice(x1, *SLICE['x']), into_slice(x2, *SLICE['x2'])
        out, obuf = into_slice(torch.zeros(xs.shape[0], *out_hw(g), g.cout, device='cuda'), *SLICE['out'])
        obuf.fill_(float('nan'))
        res, ss = (None if t is None else into_slice(t, *SLICE['out'])[0] for t in (res, ss))
        if keep is not None:
            keep.update(obuf=obuf, buf=buf, buf2=buf2)
    if res is not None:
        kw['res'] = res
    if ss is not None:
        kw['sft_scale'] = ss
    if code == ops.SPLIT and d['pro'] in (PRO_NONE, PRO_LEAKY):
        kw['act'] = ops.act_scale(xs if act_x is None else act_x[sl].contiguous().cuda())
    y = ops.conv2d(x1, pw, x2=x2, out=out, **kw)
    return y.permute(0, 2, 3, 1) if g.out_nchw else y


STATS_TERMS = 16      # conv3x3_few_cin_kernel: a thread adds its sixteen pixels' values and squares in fp32; everything after that is fp64


def stats_ratio(y):
    """The GroupNorm partials of a launch (y._cf_stats) against fp64 sums over the tensor y that was written: the largest |error| of a group's sum and
    sum of squares as a part of (STATS_TERMS + 1) u x (sum |y|, sum y^2) -- sixteen fp32 additions, and one rounding of each square."""
    st = y._cf_stats
    B = y.shape[0]
    got = st.part.view(B, 32, st.parts, 2).sum(2).cpu()
    r = y.detach().cpu().double().reshape(B, -1, 32, st.cpg)
    want = torch.stack([r.sum((1, 3)), (r * r).sum((1, 3))], -1)
    room = torch.stack([r.abs().sum((1, 3)), (r * r).sum((1, 3))], -1)
    return float(((got - want).abs() / ((STATS_TERMS + 1) * U * room + 1e-300)).max())


def case(name, key, code, route, form, variant=0):
    pr = prepared(name, key, route, form, variant)
    if pr is None:
        return None
    d, ref, tol = pr
    r, err = ratio(run(d, key, code, (name, key, variant, d['epi'])), ref, tol)
    er = emulated(name, key, route, form, variant)
    return dict(ratio=r, err=err, emu_ratio=er[0], emu_err=er[1])


if __name__ == '__main__':
    if '--ends' in sys.argv:
        with_nchw_ends()
    if '--prelu' in sys.argv:
        with_prelu()
    bad = 0
    for key in CASES:
        for fam in families_of(key) + ('onehot_pixels',) + SOLO_FAMILIES:
            for cname, code, route, form in launches(key):
                if fam in SOLO_FAMILIES and route not in SOLO_ROUTES:
                    continue
                r = case(fam, key, code, route, form)
                if r is None:
                    continue
                ok = r['ratio'] <= 1.0
                bad += not ok
                print(f'[{"ok" if ok else "FAIL"}] {fam:21s} {key:4s} {tuple(CASES[key][:5])} {route:9s} {cname:5s} {form:16s}: kernel max|d| {r["err"]:.3e} = '
                      f'{r["ratio"]:.4f} of the gate | emulation {r["emu_err"]:.3e} = {r["emu_ratio"]:.4f}', flush=True)
    sys.exit(1 if bad else 0)
