"""The 3x3 stride-1 convolution kernels (dense NHWC, zero padding) per element on exact, impulse and mixed-scale inputs: seeded input families, the
fp64 reference, the routes (which pack code and shape reaches which kernel form), the per-element gate and a CPU emulation in fp32 of every operand
scheme and transform that makes the gate a condition on the reference.  Library of tests/test_gpu_conv_families.py (GPU) and
tests/test_conv_families_host.py (CPU).
usage (GPU box): python tools/conv_check.py          one line per (family, shape, route): kernel error, emulation error, both as parts of the gate

Routes (ROUTES; route_of() restates the rules of conv_dispatch / launch_direct / launch_ladder in cf_igemm.hip, cf_winograd_launch, cf_wsplit_covers,
cf_wf43_launch and cf_split_launch; weights are packed with the explicit code, never through the ops.conv_code policy):
  d32        code 0        cf_igemm.hip ladder: cout_pad % 128 == 0 and <= 1024 pixels -> narrow 128x64, cout_pad % 128 == 0 -> 128x128, cout_pad 64 -> 256x64;
                           up2x=True: the same ladder on the four folded 2x2 sub-pixel convolutions
  dsplit     SPLIT         cf_split.hip form 0 (plain) / form 1 (folded upsample): cin % 32, cout % 64, whole 16x16 tiles of the input grid
  w23_f32    WINOGRAD      four-wave F(2,3) on fp32 operands; split_k >= 1 (cin % 128 == 0, split_k | cin / 128): its split-K instantiation
  w23_h4     WSPLIT        four-wave F(2,3) on split halves where cf_wsplit_covers says no (cout % 128 != 0, fewer than 1024 pixels, or split_k >= 1)
  w23_h8     WSPLIT WF16 WBF16   eight-wave cf_wsplit.hip (cout % 128 == 0, at least 32x32 pixels, no split_k); WF16 / WBF16: single 16-bit operands, cin % 32 == 0
  w43_8      WF43 WF43F    eight-wave F(4,3), 64 channels per workgroup (cout % 128 != 0; cout 192: ntn = 3), cin <= 256
  w43_16k32  WF43 WF43F    sixteen-wave form on 32-channel slabs (cout % 128 == 0, cin % 32 == 0, c_split % 32 == 0), cin <= 512
  w43_16k16  WF43 WF43F    sixteen-wave form on 16-channel slabs (cout % 128 == 0, cin % 32 != 0), cin <= 256
  w43_up     WF43F + upsample    the upsampling gather of the sixteen-wave form (prologue none, no epilogue operand, one input)
  w42_up     WF42U + upsample    nearest x2 + 3x3 as four F(4x4,2x2) sub-pixel phases on the low-resolution image (cf_conv_desc.upsample == 2; what the
                           Upsample blocks of precision 'fp32' run): fp32 operands, prologue none, no epilogue operand, one input, cin % 32 == 0 and <= 512
                           (the 32-channel-slab form's limit; the 256 and the smallest size of ops.f43_up_ok are policy, not the form), cout % 128 == 0,
                           whole 16x16 blocks of the INPUT.  A packing of its own: ops.pack_weight(w, b, bf16=ops.WF42U), no up2x.  Route, code and
                           shapes enter ROUTES, CODES and SHAPES through with_f42() (the two families tests and this script's own listing call it)
Shapes (SHAPES: B, H, W of the INPUT, cin, cout, c_split, upsample): nothing above 48x48 pixels, batch 3 or 512 channels.  UP_SHAPES (zu1: three slabs,
32x48, two channel tiles; zu2: eight slabs on 16x16) join them through with_f42(); with u1 (one slab: fill and drain with no steady state, one
block per phase) they are the shapes of w42_up.

Families (CPU, fixed seeds; family(name, shape_key) -> dict x, w, b, sc, sh, res, ss, pro, epi, sft_w; computed once, never modified):
  int_coded      x in -3..3, w in (-3..3) 2^-5, bias / residual / SFT operands small integers, prologue none or affine with sc in {1/2, 1, 2} and
                 integer sh, epilogue none / bias / residual / SFT with sft_w = 0.5.  EXACT routes (d32, dsplit plain and folded, w23_f32 at every split
                 count, w23_h4, w23_h8 in its three operand types) return the fp64 result with torch.equal: B^T, G and A^T of F(2,3) hold only 0, +-1
                 and +-1/2, so U = G g G^T (multiples of 2^-7 of at most 27 units) and V = B^T d B (multiples of 1/2 of at most 56 units) fit 8
                 significand bits -- bf16, and IEEE half with a ZERO lo half, so the dropped lo lo product is zero -- and every accumulator's sum of
                 |products| stays below 2^24 units through the output transform, the folded taps and the epilogue (exactness_preconditions() asserts
                 both on the seeded data at cin = 512): the result does not depend on the order of any addition.
                 F(4,3) is NOT in this family and cannot be: G' has entries in fifteenths (cf_wf43.hip:18), so U is never exact; multiples of 225
                 do not rescue it, because the A^T pass (entries 1/8 .. 8) then spans too many binades for fp32.  F(4,3) stands under the gates.
  onehot_pixels  x zero except isolated unit pixels, Chebyshev distance >= 3 apart, each in a channel of its own, at the four image corners, on the
                 edges and on both sides of the 8x16 / 16x16 patch and the 2x2 / 4x4 tile boundaries; w, b dense random.  out = the flipped weight
                 slice + bias around a pixel, the bias elsewhere: d32 bitwise fp32(w + b) (plain form; a folded tap is a sum of up to four weights); every other
                 route under the gate (one product per element).
  tap_shift      per tap t: w[n, c, t] = +-1 for c = p(n), zero elsewhere: out = +-the input moved by one pixel with a zero row / column at the border it
                 left.  d32 bitwise; dsplit within the 22-bit split of x; the Winograd routes under the gate.  Zero padding per border, per route.
  mixed_cout     output channel n carries weights 2^-e(n), e = 0 .. MIXED_SPAN = 32: past subnormal lo halves and subnormal hi halves under the ONE
                 pack-time scale.  Affine prologue.
  mixed_cin      input channel c carries 2^e(c), e = -10 .. 10: through the affine prologue (sc) -- variant 'mixed_cin' -- and in the tensor itself with
                 the per-image range scale `act` -- variant 'mixed_cin_act' (prologue none).
  cancel_pairs   channels 2k, 2k + 1 carry EQUAL inputs and weights +w, -(w + delta) of unequal size (pair magnitudes 1 .. 16, delta 2^-9 of w): each
                 output is a small remainder of a large S (median S / |pre| >= 100 asserted on the CPU) and the additions round.  Affine prologue, bias.
  dc_plus_ripple x = 2^8 + N(0, 1) against weights whose nine taps sum to ~0 per (n, c): the classic Winograd amplification case; the image border
                 (zero padding: the constant does not cancel there) and the interior patch borders are both in every shape.  Prologue none + act, residual.
  solo_cin       output channel n reads exactly ONE input channel p(n): w[n, p(n)] is a dense random 3x3 tap set (not +-1: the weight's own lo halves take
                 part, lo hi + hi lo + hi hi), every other weight an exact 0; input channel c carries 2^e(c), e linear over 2 SOLO_EXP = 32 binades.  In
                 every dense family a small input channel hides behind the large ones of the same sum (S and c are set by all of them); here each
                 channel is alone in its sum and meets its own gate.  Variant 'solo_cin': the scale through the affine prologue, e = -22 .. 10 (the top
                 where mixed_cin has it: IEEE half ends at 65504 and an affine prologue has no range scale); 'solo_cin_act': in the tensor itself,
                 e = -16 .. 16, prologue none with the per-image range scale `act`.  p (solo_perm) reads the smallest and the largest channel and at
                 least one per 16-channel slab at every shape, cout < cin included; under the range scale the read channels include some whose lo
                 halves are all subnormal with normal hi halves (|a| < 2^-3) and some whose hi halves are subnormal too (|a| < 2^-14) -- both
                 asserted by the host test, per shape and image.  The bias is random at the scale of the channel it is added to; no epilogue operand.
                 The gate differs in two places that follow from the zeros (below).
  swish_leaky_edges  inputs cycling through 0, -0, +-2^-10, +-1, +-6, +-20: affine (sc 1, sh 0) + swish with a residual, and LeakyReLU with an SFT
                 epilogue (variant 'swish_leaky_edges_sft'), the epilogue operands 2^10 larger than the convolution.

Gate, against fp64, PER ELEMENT (u = 2^-24):
    gate = c u S + P + floor + epilogue terms
  S   direct routes: sum over taps and channels of |w| |p(x)|, p = the prologue, zero outside the image.  Winograd routes: the SAME evaluation the
      kernel makes with every matrix and operand replaced by its absolute value, |A^T| [ sum_c (|G| |g| |G^T|) (.) (|B^T| |p(x)| |B|) ] |A| -- it bounds
      every partial result of the algorithm, is never below the direct S, and is at most (the squared product of the absolute row sums of A^T, G
      and B^T) times sum_c max|g_c| max|p_c| over the tile's window (81 for F(2,3), 14581 for F(4,3), 4556.25 = (10.125 x 4/3 x 5)^2 for F(4,2) with g_c the
      FOLDED 2x2 taps of the phase, themselves sums of up to four weights and the operand of that form: all three bounds asserted by the host test).  The direct S cannot serve there: a Winograd tile's outputs read all of the tile's window, so an
      element whose own 3x3 neighbourhood is empty (onehot_pixels) still carries the rounding of its neighbours' products.
  c   the number of roundings on the way of one element, each at most u times a partial result <= S (no statistical discount):
        d32      9 cin (the fp32 FMA chain over taps and channels), + 3 with folded taps (a folded weight is a sum of up to four)
        dsplit   3 x 9 cin (three products per term) + 12 (|a - hi - lo| <= 2^-22 |a| per operand and the dropped lo lo <= 2^-22 |a w|: 3 2^-22 = 12 u), + 3 folded
        w23      cin (the transform-domain chain) + 2 (B^T d B: one addition per pass; every row of B^T has absolute sum 2) + 1 (U = G g G^T in fp64,
                 rounded once; rows of G: absolute sum 3/2) + 4 (A^T M A: rows of absolute sum 3, two additions per pass) = cin + 7; split-K: + cin / 128
                 chunk additions.  Split halves: 3 cin + 12 + 7.  Single IEEE half (WF16): cin + 7 + 2 x 2^-11 / u; single bf16: cin + 7 + 2 x 2^-8 / u.
        w43      cin + 10 (B'^T d B': rows of up to four terms with the factor 17/16: five roundings per pass; absolute row sum 1.875) + 1 (U; rows
                 of G': up to 56/15) + 8 (A^T M A: five terms per row, absolute sums up to 17.25) = cin + 19; split halves 3 cin + 12 + 19
        w42      (w42_up; S through |A42^T|, |G42| |g_p| |G42^T| with g_p the folded taps, |B42^T|: absolute row sums up to 10.125, 4/3, 5.)  Read off
                 the kernel's arithmetic, every operation counted that can round, the worst row of each pass:
                 cin (the fp32 MFMA chain over the slabs, one rounding per product added)
                 + 8  B42^T d B42, bt42 of cf_wf43.hip, 4 per pass.  Rows xi 0 and 4, (d0 + d3) - (d1 + d2) 1.5: two additions, the product by 1.5 and the
                      subtraction, four roundings (1.5 and 2.5 are not powers of two: their products round; where the compiler contracts product and
                      subtraction into one FMA there are three -- counted as four, the bound holds either way).  Row 1, (d1 + d3) - 2.5 d2: three.
                      Rows 2 and 3, (d3 - d2) - 2 d1 and .5 (d2 - d1) + d3: two, the products by 2 and .5 are exact.
                 + 1  U = G42 g_p G42^T with the fold in fp64, rounded once (cf_pack.hip; ops.f42_weights): the fold adds no fp32 rounding
                 + 6  A42^T M A42, 3 per pass; every factor (.5, 2, .25, 4, .125, 8) is a power of two, so only additions round.  xi pass (col()):
                      m1 + ca1 m2 + ca2 m3 and (cb1 m2 + cb2 m3) - m1 two additions, + m0 (rows 0, 1) or + m4 (rows 2, 3) a third.  nu pass: (t0 + t1) +
                      (t2 + t3) three, (.5 t2 + 2 t3) - t1 and (.25 t2 + 4 t3) + t1 two, ((.125 t2 + 8 t3) - t1) + t4 three.
                 = cin + 15.  acc_scale is 1 with fp32 operands (an exact product); the bias addition is the epilogue's 2 u |pre|.  No prologue term,
                 no epilogue operand, no floor.
  P   the prologue's own error taken through the same absolute evaluation as S: affine 2 u (|x sc| + |sh|); swish |swish'(y)| times that +
      (2 |y| + 8) u |swish(y)| (v_exp_f32 on y log2 e, 1 + e, v_rcp_f32, one product: whole ulps); leaky u |p|; none 0 (the range scale is a power of two)
  floor  split-half and single-half routes: IEEE half has the spacing 2^-24 below 2^-14, so a half of an operand that falls there carries an ABSOLUTE
      error of 2^-25: 2^-25 (1 + 2^-10) (sum |p(x)| / scale + sum |w| / s), scale = the pack-time power of two (ops.pack_scale of the domain maximum),
      s = the image's range scale (1 with an affine prologue); on Winograd routes both sums in the transform domain, sum_c |V| and sum_c |U|, taken
      through |A^T| . |A|.  (The form of gemm_check.gate.)  0 for fp32 and bf16 operands.
  epilogue  bias 2 u |pre| (entered ALWAYS, also where b = 0 (tap_shift): harmless next to c u S, and exact elements meet any gate); residual 2 u |out|; SFT out = r0 + w (r0 r1 + pre): 2 u (|w r0 r1| + 2 |w (r0 r1 + pre)| + |out|): single roundings at a whole ulp.
The solo families (SOLO_FAMILIES), two changes, both consequences of the exact zeros:
  c      counts the products that exist.  A term whose weight is an exact zero is an exact zero product in every scheme (hi = lo = 0; U = G 0 G^T = 0), and
         adding an exact zero never rounds: the chain over the channels has ONE term, so cin becomes 1 in every row above (d32 9, dsplit 27 + 12,
         w23 1 + 7, split halves 3 + 12 + 7, w43 1 + 19, ...).  The transform constants and the split-K chunk additions (cin / 128: every chunk IS
         added) stay as they are.
  floor  sums the channels that have halves in the sum: sum |p(x)| / scale runs over the input channels with a non-zero weight for THAT output channel
         (direct: the convolution of |p| with the 0 / 1 pattern of the weight; Winograd: sum over those channels of |V| through |A^T| . |A|, evaluated
         exactly, no bound); sum |w| / s needs no change, a zero weight adds zero.  And with one channel alone in the sum the absolute 2^-25 of a
         subnormal half is ATTAINED by a correct evaluation (in a dense sum it is a worst case over cin halves that never align), so it is entered at
         the whole spacing 2^-24: the rule gemm_check.gate applies to single roundings (bias, residual), which keeps the emulation within half.
  The fp32 routes have no floor term and take only the first change.
The emulation (emulate(): torch float32 on the CPU; transforms as two passes of fp32 einsums, U from fp64 rounded once, halves split as
gemm_check.split_halves does, three products lo hi + hi lo + hi hi, fp32 epilogue) is the condition on the gate: tests/test_conv_families_host.py asserts its
error within 0.5 of the gate for every gate family, operand scheme and transform at every shape the GPU test uses (the folded forms are emulated on
the upsampled image with the unfolded weight: the fold's additions are the + 3 of c; w42_up is emulated as it runs, wino42() in float32 on the
low-resolution image, and takes two edits of its own -- fold=swapped_fold, phase (a, b) given the taps folded for (b, a), and zero_positions=IDLE_LOWER /
IDLE_UPPER, the thirteenth position of the lower wave half or the last of the upper taken for the idle accumulator -- each of which the host test shows
at >= 10 times the gate on some family at every w42_up shape).  emulate(.., act_halves=) takes an edit of the activation's
split: with drop_small_lo (the lo half zeroed where it is subnormal, |a| < 2^-3) the solo families' emulation exceeds their gate 25 .. 103 times at
every shape and split-half scheme while no other family's ratio at shape b moves by 0.002 of its gate (the host test asserts >= 10 and <= 0.005).  No number here was fitted to
what a kernel returns; the kernels' figures are in the docstring of tests/test_gpu_conv_families.py.
"""
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
from codeformer_amd import ops  # noqa: E402
from conv_case import launch_args  # noqa: E402
from conv_case import reference as case_reference  # noqa: E402
from gemm_check import split_halves  # noqa: E402

U = 2.0 ** -24
MIXED_SPAN = 15 + 14 + 3
CIN_EXP = 10
EDGE_VALUES = (0.0, -0.0, 2.0 ** -10, -2.0 ** -10, 1.0, -1.0, 6.0, -6.0, 20.0, -20.0)
PRO_NONE, PRO_AFFINE, PRO_AFFINE_SWISH, PRO_LEAKY = ops.PRO_NONE, ops.PRO_AFFINE, ops.PRO_AFFINE_SWISH, ops.PRO_LEAKY
EPI_NONE, EPI_RESIDUAL, EPI_SFT = ops.EPI_NONE, ops.EPI_RESIDUAL, ops.EPI_SFT
ROUTES = ('d32', 'dsplit', 'w23_f32', 'w23_h4', 'w23_h8', 'w43_8', 'w43_16k32', 'w43_16k16', 'w43_up')
EXACT_ROUTES = ('d32', 'dsplit', 'w23_f32', 'w23_h4', 'w23_h8')
CODES = {'F32': 0, 'SPLIT': ops.SPLIT, 'WINOGRAD': ops.WINOGRAD, 'WSPLIT': ops.WSPLIT, 'WF16': ops.WF16, 'WBF16': ops.WBF16, 'WF43': ops.WF43, 'WF43F': ops.WF43F}
# The sub-pixel F(4,2) form joins ROUTES, CODES and SHAPES through with_f42() (as tools/conv_geom_check.py adds its NCHW ends): the module as loaded
# keeps the nine routes, eight codes and nine shapes that its other users pin (tests/test_gpu_sft_per_image.py, tests/test_gpu_wf43_kparts.py).
F42_ROUTE, F42_CODE = 'w42_up', 'WF42U'
# key -> (B, H, W of the input, cin, cout, c_split, upsample)
SHAPES = {'a': (1, 16, 16, 16, 64, None, False), 'b': (2, 16, 32, 32, 64, None, False), 'c': (2, 32, 32, 64, 128, 32, False),
          'd': (3, 32, 48, 48, 128, None, False), 'e': (1, 16, 16, 256, 64, None, False), 'f': (1, 16, 16, 512, 128, 256, False),
          'g': (1, 48, 32, 192, 192, None, False), 'u1': (2, 16, 16, 32, 128, None, True), 'u2': (1, 16, 16, 64, 64, None, True)}
# the further upsampling shapes of the sub-pixel F(4,2) form (w42_up; u1 is its first: one slab, one block per phase, every side an image border): an odd
# slab count (3) on a non-square image with interior block borders on both axes and two channel tiles; the slab maximum of the network (8) on the
# smallest image.  Not in SHAPES until with_f42(): family() seeds by the sorted position of a key, and tests/test_gpu_wf43_kparts.py appends
# its own keys behind SHAPES' -- these sort after both, so every older key keeps its data bit for bit either way.
UP_SHAPES = {'zu1': (1, 32, 48, 96, 256, None, True), 'zu2': (1, 16, 16, 256, 128, None, True)}
GATE_FAMILIES = ('mixed_cout', 'mixed_cin', 'mixed_cin_act', 'cancel_pairs', 'dc_plus_ripple', 'swish_leaky_edges', 'swish_leaky_edges_sft')
# one input channel per output channel: gate families too, under a gate that counts and sums the channels that HAVE a product.  A tuple of their own:
# GATE_FAMILIES is the list of the dense families, which tests and tools/conv_geom_check.py pin as it is
SOLO_FAMILIES = ('solo_cin', 'solo_cin_act')
SOLO_EXP = 16
LO_SUBNORMAL, HI_SUBNORMAL = 2.0 ** -3, 2.0 ** -14       # |a| below which the lo half / the hi half of an operand is a subnormal IEEE half
IMPULSE_FAMILIES = ('onehot_pixels', 'tap_shift')

# the transforms, as the kernels document them (cf_winograd.hip; cf_wf43.hip:16-19, B'^T = D B^T, G' = D^-1 G)
BT2 = [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]]
G2 = [[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]]
AT2 = [[1, 1, 1, 0], [0, 1, -1, -1]]
BT4 = [[.25, 0, -1.0625, 0, .25, 0], [0, -.5, -1, .125, .25, 0], [0, .5, -1, -.125, .25, 0], [0, -.25, -.125, 1, .5, 0], [0, .25, -.125, -1, .5, 0],
       [0, .25, 0, -1.0625, 0, .25]]
G4 = [[4, 0, 0], [-32 / 15, -16 / 15, -8 / 15], [-32 / 15, 16 / 15, -8 / 15], [1 / 15, 2 / 15, 4 / 15], [1 / 15, -2 / 15, 4 / 15], [0, 0, 4]]
AT4 = [[1, 1, 1, 1, 1, 0], [0, .5, -.5, 2, -2, 0], [0, .25, .25, 4, 4, 0], [0, .125, -.125, 8, -8, 1]]


F42 = 42       # the transform tag of F(4x4,2x2) on the sub-pixel phases (scheme_of); its matrices are ops.B42T, ops.G42, ops.A42T


def mats(m, dtype=torch.float64):
    """(B^T, G, A^T) of F(m x m, 3x3), m = 2 | 4, or of F(4x4, 2x2), m = F42."""
    return tuple(torch.tensor(t, dtype=dtype) for t in ((BT2, G2, AT2) if m == 2 else (ops.B42T, ops.G42, ops.A42T) if m == F42 else (BT4, G4, AT4)))


def with_f42():
    """ROUTES, CODES and SHAPES of this module object with the sub-pixel F(4,2) form in them: the route w42_up, the code WF42U, and UP_SHAPES behind
    the older keys (idempotent)."""
    global ROUTES
    assert min(UP_SHAPES) > max(k for k in SHAPES if k not in UP_SHAPES)
    SHAPES.update(UP_SHAPES)
    CODES[F42_CODE] = ops.WF42U
    if F42_ROUTE not in ROUTES:
        ROUTES = ROUTES + (F42_ROUTE,)


# ---- routes ----------------------------------------------------------------------------------------------------------------------------------
def route_of(code, H, W, cin, cout, up=False, split_k=0, c_split=None):
    """(route, kernel form) an explicit pack code reaches at a shape ((H, W): the INPUT size), or None where packing or the C ABI refuses."""
    Ho, Wo = (2 * H, 2 * W) if up else (H, W)
    px = Ho * Wo
    c0 = cin if c_split is None else c_split
    if code == 0:                                                        # launch_direct / launch_ladder
        if split_k or cin % 16 or Ho % 16 or Wo % 16:
            return None
        cp = max(64, ops._cout_pad(cout)) if up else ops._cout_pad(cout)
        rung = 'narrow 128x64' if (cp % 128 == 0 and px <= 1024) else '128x128' if cp % 128 == 0 else '256x64' if cp == 64 else None
        return rung and ('d32', ('folded ' if up else '') + rung)
    if code == ops.SPLIT:                                                # cf_split_launch
        if split_k or cin % 32 or c0 % 32 or cout % 64 or H % 16 or W % 16:
            return None
        tiles = (4 if up else 1) * (H // 16) * (W // 16)
        wide = cout % 128 == 0 and tiles * (cout // 128) > 64
        return 'dsplit', f'form {int(up)} {"128" if wide else "64"}-wide'
    if code in (ops.WINOGRAD, ops.WSPLIT, ops.WF16, ops.WBF16):          # cf_winograd_launch / cf_wsplit_covers
        if up or cin % 16 or c0 % 16 or cout % 64 or H % 8 or W % 16:
            return None
        if split_k and (cin % 128 or (cin // 128) % split_k):
            return None
        if code in (ops.WF16, ops.WBF16) and (cin % 32 or c0 % 32):         # conv_validate: single 16-bit operands take 32-channel slabs
            return None
        sk = f'split-K {split_k}' if split_k else 'four-wave'
        if code == ops.WINOGRAD:
            return 'w23_f32', sk
        if not split_k and cout % 128 == 0 and px >= 1024:
            return 'w23_h8', {ops.WSPLIT: 'f16x2', ops.WF16: 'f16', ops.WBF16: 'bf16'}[code]
        return ('w23_h4', sk) if code == ops.WSPLIT else None
    if code == ops.WF42U:                                                # cf_wf43_launch, cf_conv_desc.upsample == 2 (the packer: whole 32-channel slabs, 128 output channels)
        # fp32 operands, one input, cf_wf43_k32 (cout % 128 == 0, cin % 32 == 0), whole 16x16 blocks of the INPUT, no split_k; the channel limit is the
        # 32-channel-slab form's own (F4_TAB_32 = 512 -- the 256 of ops.f43_up_ok is policy, as is its smallest size)
        ok = up and not split_k and c_split is None and cin % 32 == 0 and cin <= 512 and cout % 128 == 0 and H % 16 == 0 and W % 16 == 0
        return ('w42_up', 'sub-pixel phases') if ok else None
    if code in (ops.WF43, ops.WF43F):                                    # cf_wf43_launch
        if split_k or cin % 16 or c0 % 16 or cout % 64 or Ho % 16 or Wo % 16:
            return None
        wide = cout % 128 == 0
        k32 = wide and cin % 32 == 0
        if up:
            return ('w43_up', 'k32 gather') if (code == ops.WF43F and c_split is None and k32) else None
        if cin > (512 if k32 else 256) or (k32 and c0 % 32):
            return None
        return ('w43_16k32' if k32 else 'w43_16k16' if wide else 'w43_8'), f'ntn {cout // (128 if wide else 64)}'
    return None


def routes():
    """{shape key: [(code name, split_k, route, form)]}: every launch the GPU test makes, by the rules above."""
    out = {}
    for key, (B, H, W, cin, cout, cs, up) in SHAPES.items():
        rows = []
        for name, code in CODES.items():
            sks = [0] + ([n for n in (1, 2, 4) if cin % 128 == 0 and (cin // 128) % n == 0] if code in (ops.WINOGRAD, ops.WSPLIT) and H * W <= 256 else [])
            for sk in sks:
                r = route_of(code, H, W, cin, cout, up, sk, cs)
                if r is not None:
                    rows.append((name, sk, *r))
        out[key] = rows
    return out


def scheme_of(route, code):
    """(transform 0 | 2 | 4 | F42, operands 'f32' | 'half2' | 'half' | 'bf16')."""
    m = 0 if route in ('d32', 'dsplit') else 2 if route.startswith('w23') else F42 if route == 'w42_up' else 4
    op = {0: 'f32', ops.WINOGRAD: 'f32', ops.WF43F: 'f32', ops.WF42U: 'f32', ops.WF16: 'half', ops.WBF16: 'bf16'}.get(code, 'half2')
    return m, op


# ---- the families ----------------------------------------------------------------------------------------------------------------------------
def rnd(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def onehot_positions(H, W, n):
    """Up to n pixels, Chebyshev distance >= 3 apart, in priority order: corners, both sides of the patch boundaries (rows 8k-1 | 8k, 16k-1 | 16k,
    columns 16k-1 | 16k) at and off the image edge, tile boundaries, edge midpoints, then whatever else fits."""
    rows_b = sorted({r for k in range(1, H // 8 + 1) for r in (8 * k - 1, 8 * k) if r < H})
    cols_b = sorted({c for k in range(1, W // 16 + 1) for c in (16 * k - 1, 16 * k) if c < W})
    cand = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    # (the two sides of a boundary are neighbours: they take columns / rows at least 3 apart)
    cand += [(r, c) for i, r in enumerate(rows_b) for c in ((0, W - 1, 6) if i % 2 == 0 else (3, W - 4, 10))]
    cand += [(r, c) for i, c in enumerate(cols_b) for r in ((0, H - 1, 6) if i % 2 == 0 else (3, H - 4, 10))] + [(r, c) for r in rows_b for c in cols_b]
    cand += [(0, W // 2), (H - 1, W // 2 + 1), (H // 2, 0), (H // 2 + 1, W - 1), (3, 3), (4, 11), (11, 4)]
    cand += [(r, c) for r in range(H) for c in range(W)]
    got = []
    for p in cand:
        if len(got) < n and p[0] < H and p[1] < W and all(max(abs(p[0] - q[0]), abs(p[1] - q[1])) >= 3 for q in got):
            got.append(p)
    return got


def tap_perm(cin, cout, seed=5):
    rng = np.random.default_rng(seed)
    p = torch.from_numpy(np.concatenate([rng.permutation(cin) for _ in range((cout + cin - 1) // cin)])[:cout].copy())
    sign = torch.from_numpy(rng.integers(0, 2, cout) * 2.0 - 1.0).float()
    return p, sign


def tap_weight(cin, cout, tap, k=3):
    p, sign = tap_perm(cin, cout)
    w = torch.zeros(cout, cin, k, k)
    w[torch.arange(cout), p, tap // k, tap % k] = sign
    return w


def solo_perm(cin, cout):
    """p: output channel -> the one input channel it reads.  cout >= cin: n -> (5 n + 3) mod cin, a bijection on every run of cin outputs (5 is coprime
    to every cin in use), so EVERY input channel is read; cout < cin: cout channels spread evenly from 0 to cin - 1, both ends included, less than 16
    apart where cin <= 16 (cout - 1) + 1.  tap_perm promises neither where cout < cin."""
    n = torch.arange(cout)
    if cout >= cin:
        assert math.gcd(5, cin) == 1
        return (5 * n + 3) % cin
    return torch.round(n.double() * ((cin - 1) / (cout - 1))).long()


def solo_exponents(name, cin):
    """e(c), linear from -SOLO_EXP to +SOLO_EXP; solo_cin: moved down by SOLO_EXP - CIN_EXP, so that the largest channel sits at 2^CIN_EXP as
    mixed_cin's does -- an affine prologue has no range scale, and 2^16 x 1.5 x 4.5 is past the largest IEEE half."""
    e = torch.round(-SOLO_EXP + torch.arange(cin).float() * (2.0 * SOLO_EXP / (cin - 1)))
    return e - (SOLO_EXP - CIN_EXP) if name == 'solo_cin' else e


def family_at(name, geom, seed, variant=0, k=3, out_hw=None, positions=None, key=None, bare_up=True):
    """The recipe of family() at any geometry: geom = (B, H, W of the input, cin, cout, upsample); k = 3 | 1 the kernel's side; out_hw the output
    size where it is neither the input's nor twice it (stride 2); positions(image) -> the one-hot pixels of an image (default: onehot_positions); bare_up: upsampling shapes take prologue none and no
    epilogue operand.
    family(name, key, variant) is this function at SHAPES[key] with the seed of the key, bit for bit (tools/conv_geom_check.py draws its cases here)."""
    B, H, W, cin, cout, up = geom
    Ho, Wo = out_hw if out_hw is not None else (2 * H, 2 * W) if up else (H, W)
    pro, epi, sft_w = PRO_AFFINE, EPI_NONE, 0.7
    sc, sh = torch.rand(B, cin, generator=torch.Generator().manual_seed(seed + 1)) + 0.5, rnd((B, cin), seed + 2, 0.1)
    x, w, b = rnd((B, H, W, cin), seed + 3), rnd((cout, cin, k, k), seed + 4, (2.0 / (k * k * cin)) ** 0.5), rnd((cout,), seed + 5, 0.1)
    res, ss = rnd((B, Ho, Wo, cout), seed + 6), rnd((B, Ho, Wo, cout), seed + 7, 0.3)
    if name == 'int_coded':
        i = torch.arange(B * H * W * cin).view(B, H, W, cin)
        x = ((i * 7 + (i // cin) * 3 + (i % 251)) % 7 - 3).float()
        j = torch.arange(cout * cin * k * k).view(cout, cin, k, k)
        w = ((j * 5 + (j // (k * k)) * 11 + (j % 241)) % 7 - 3).float() * 2.0 ** -5
        b = (torch.arange(cout) % 9 - 4).float()
        o = torch.arange(B * Ho * Wo * cout).view(B, Ho, Wo, cout)
        res, ss = ((o * 3 + o // cout) % 11 - 5).float(), ((o * 5 + o // cout) % 5 - 2).float()
        sc = torch.tensor([0.5, 1.0, 2.0])[(torch.arange(B * cin) % 3)].view(B, cin)
        sh = (torch.arange(B * cin) % 3 - 1).float().view(B, cin)
        pro, epi = ((PRO_NONE, EPI_NONE), (PRO_AFFINE, EPI_RESIDUAL), (PRO_AFFINE, EPI_SFT), (PRO_NONE, EPI_RESIDUAL))[variant]
        sft_w = 0.5
    elif name == 'onehot_pixels':
        x = torch.zeros(B, H, W, cin)
        for bi in range(B):
            for c, (r, q) in enumerate(onehot_positions(H, W, cin) if positions is None else positions(bi)):
                x[bi, r, q, (c + 5 * bi) % cin] = 1.0
        pro = PRO_NONE
    elif name == 'tap_shift':
        w, b, pro = tap_weight(cin, cout, variant, k), torch.zeros(cout), PRO_NONE
    elif name == 'mixed_cout':
        e = torch.round(torch.arange(cout).float() * (MIXED_SPAN / (cout - 1)))
        w = w * torch.pow(2.0, -e)[:, None, None, None]
        b = b * torch.pow(2.0, -e)
    elif name in ('mixed_cin', 'mixed_cin_act'):
        e = torch.round(-CIN_EXP + torch.arange(cin).float() * (2.0 * CIN_EXP / (cin - 1)))
        if name == 'mixed_cin':
            sc, sh = sc * torch.pow(2.0, e)[None, :], sh * torch.pow(2.0, e)[None, :]
        else:
            x, pro = x * torch.pow(2.0, e), PRO_NONE
    elif name in SOLO_FAMILIES:
        e, p = solo_exponents(name, cin), solo_perm(cin, cout)
        w = torch.zeros(cout, cin, k, k)
        w[torch.arange(cout), p] = rnd((cout, k, k), seed + 11, (2.0 / (k * k)) ** 0.5)
        b = b * torch.pow(2.0, e)[p]                      # (at the scale of the one channel it is added to: a bias of 0.1 would hide a channel of 2^-16)
        if name == 'solo_cin':
            sc, sh = sc * torch.pow(2.0, e)[None, :], sh * torch.pow(2.0, e)[None, :]
        else:
            x, pro = x * torch.pow(2.0, e), PRO_NONE
    elif name == 'cancel_pairs':
        half = cin // 2
        x = rnd((B, H, W, half), seed + 8).repeat_interleave(2, dim=3)
        sc, sh = sc[:, :half].repeat_interleave(2, dim=1), sh[:, :half].repeat_interleave(2, dim=1)
        w0 = rnd((cout, half, k, k), seed + 9, (2.0 / (k * k * cin)) ** 0.5) * (1.0 + (torch.arange(half) % 16).float())[None, :, None, None]
        delta = rnd((cout, half, k, k), seed + 10, (2.0 / (k * k * cin)) ** 0.5 * 2.0 ** -9) * (1.0 + (torch.arange(half) % 16).float())[None, :, None, None]
        w = torch.stack((w0, -(w0 + delta)), dim=2).reshape(cout, cin, k, k)
    elif name == 'dc_plus_ripple':
        x = 256.0 + x
        w = w - w.mean(dim=(2, 3) if k > 1 else 1, keepdim=True)                # (a 1x1's "taps" are its input channels)
        pro, epi = PRO_NONE, EPI_RESIDUAL
    elif name in ('swish_leaky_edges', 'swish_leaky_edges_sft'):
        i = torch.arange(B * H * W * cin).view(B, H, W, cin)
        x = torch.tensor(EDGE_VALUES)[(i * 7 + i // cin + i // (cin * W)) % len(EDGE_VALUES)]
        sc, sh = torch.ones(B, cin), torch.zeros(B, cin)
        w, res, ss = w * 0.125, res * 1024.0, ss * 1024.0                     # (|conv| ~ 1 with inputs up to 20)
        pro, epi = (PRO_AFFINE_SWISH, EPI_RESIDUAL) if name == 'swish_leaky_edges' else (PRO_LEAKY, EPI_SFT)
    else:
        raise KeyError(name)
    if up and bare_up:
        pro, epi = PRO_NONE, EPI_NONE
    return dict(x=x.contiguous(), w=w.contiguous(), b=b, sc=sc.contiguous(), sh=sh.contiguous(), res=res, ss=ss, pro=pro, epi=epi, sft_w=sft_w, up=up, key=key, solo=name in SOLO_FAMILIES)


@functools.lru_cache(maxsize=None)
def family(name, key, variant=0):
    """-> dict(x, w, b, sc, sh, res, ss, pro, epi, sft_w, acted): float32 CPU tensors.  Upsampling shapes take prologue none and no epilogue operand
    (the only form w43_up has).  variant: int_coded's (prologue, epilogue) pair; tap_shift's tap."""
    B, H, W, cin, cout, cs, up = SHAPES[key]
    return family_at(name, (B, H, W, cin, cout, up), 1000 + 17 * sorted(SHAPES).index(key), variant, key=key)


# ---- fp64 reference and gate -----------------------------------------------------------------------------------------------------------------
def prologue64(d):
    """-> (p(x), |p(x)|-magnitude for S, the prologue's own error bound) in fp64, NHWC at the conv's input size (upsampled if the shape says so)."""
    x = d['x'].double()
    sc, sh = d['sc'].double()[:, None, None, :], d['sh'].double()[:, None, None, :]
    if d['pro'] in (PRO_AFFINE, PRO_AFFINE_SWISH):
        y = x * sc + sh
        ey = 2 * U * ((x * sc).abs() + sh.abs())
        if d['pro'] == PRO_AFFINE:
            p, ep = y, ey
        else:
            s = torch.sigmoid(y)
            p = y * s
            ep = (s * (1 + y * (1 - s))).abs() * ey + (2 * y.abs() + 8) * U * p.abs()
    elif d['pro'] == PRO_LEAKY:
        p = F.leaky_relu(x, 0.2)
        ep = U * p.abs()
    else:
        p, ep = x, torch.zeros_like(x)
    if d['up']:
        p, ep = (t.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2) for t in (p, ep))
    return p, ep


def wino(p, w, m, dtype=torch.float64, absolute=False, products=None):
    """F(m x m, 3x3) of the NHWC tensor p (already through the prologue; zero padding) with the weight w (cout, cin, 3, 3), evaluated as the kernels do:
    V = B^T d B in two passes, U = G g G^T in fp64 rounded to `dtype`, the products over the channels per position, Y = A^T M A in two passes.
    absolute: every matrix and operand by its absolute value.  products(V, U) -> M replaces the channel contraction (the operand schemes).
    -> (Y (B, H, W, cout), sum_c |V| and sum_c |U| taken through |A^T| . |A| (absolute only))."""
    if m == F42:          # (p is the conv's input, the upsampled image: its even pixels are the low-resolution one)
        return wino42(p[:, ::2, ::2], w, dtype, absolute, products)
    BT, G, AT = mats(m)
    n = m + 2
    B, H, W, C = p.shape
    if absolute:
        BT, G, AT, p, w = BT.abs(), G.abs(), AT.abs(), p.abs(), w.abs()
    xp = F.pad(p.permute(0, 3, 1, 2), (1, 1, 1, 1))
    d = xp.unfold(2, n, m).unfold(3, n, m)                                     # (B, C, th, tw, n, n)
    Bt = BT.to(dtype)
    V = torch.einsum('ia,bcyxaj->bcyxij', Bt, d.to(dtype))                     # column pass
    V = torch.einsum('bcyxia,ja->bcyxij', V, Bt)                               # row pass
    Uw = torch.einsum('ia,kcab,jb->ijck', G, w.double(), G).to(dtype)          # (n, n, C, N)
    th, tw = V.shape[2], V.shape[3]
    Vm = V.permute(4, 5, 0, 2, 3, 1).reshape(n * n, B * th * tw, C)
    Um = Uw.reshape(n * n, C, -1)
    M = (torch.bmm(Vm, Um) if products is None else products(Vm, Um)).reshape(n, n, B, th, tw, -1)
    At = AT.to(M.dtype)

    def back(Mx):
        Y = torch.einsum('oi,ijbyxk->ojbyxk', At, Mx)
        Y = torch.einsum('ojbyxk,pj->opbyxk', Y, At)
        return Y.permute(2, 3, 0, 4, 1, 5).reshape(B, th * m, tw * m, -1)[:, :H, :W]
    if not absolute:
        return back(M), None
    fv = back(Vm.sum(2, keepdim=True).reshape(n, n, B, th, tw, 1))
    fu = back(Um.sum(1)[:, None, :].expand(-1, B * th * tw, -1).reshape(n, n, B, th, tw, -1))
    return back(M), (fv, fu)


def swapped_fold(a, b):
    """An edit of wino42 / emulate: phase (a, b) multiplied with the weights folded for phase (b, a) -- pa / pb exchanged in the weight only."""
    return b, a


# The other edit: one transform-domain position's products taken as zero.  The M interval of the kernel splits a phase's 25 positions 13 / 12 over two
# wave halves, and the upper half's thirteenth accumulator is idle; taking the wrong accumulator for the idle one loses position 12 (the thirteenth of
# the lower half) or position 24 (the twelfth, last, of the upper half).
IDLE_LOWER, IDLE_UPPER = (12,), (24,)


def wino42(x, w, dtype=torch.float64, absolute=False, products=None, fold=None, zero_positions=()):
    """nearest-x2 + 3x3 (zero padding) of the LOW-RESOLUTION NHWC tensor x with the weight w (cout, cin, 3, 3), evaluated as the UP form of cf_wf43.hip
    does: per output parity p = 2 a + b the folded 2x2 taps g_p (ops.fold_phase_taps, fp64), U = G42 g_p G42^T in fp64 rounded once to `dtype`
    (ops.f42_weights: the fold adds no fp32 rounding), V = B42^T d B42 in two passes on the 5x5 windows of the image padded by one pixel and moved by
    the phase (window of tile t: rows 4 t - 1 + a .. 4 t + 3 + a), the products over the channels per position, Y = A42^T M A42 in two passes, the
    4x4 outputs of a tile at (2 i + a, 2 j + b).  absolute / products: as wino().  fold(a, b) -> the parity whose taps phase (a, b) is given;
    zero_positions: positions xi * 5 + nu whose M is taken as zero (two edits for the host test that shows the gate notices them).
    -> (Y (B, 2 H, 2 W, cout), sum_c |V| and sum_c |U| taken through |A42^T| . |A42| (absolute only))."""
    BT, G, AT = mats(F42)
    B, H, W, C = x.shape
    N = w.shape[0]
    if absolute:
        BT, G, AT, x = BT.abs(), G.abs(), AT.abs(), x.abs()
    xp = F.pad(x.permute(0, 3, 1, 2), (1, 1, 1, 1))
    Bt = BT.to(dtype)
    th, tw = H // 4, W // 4
    out = [None, None, None]
    for ph in range(4):
        a, b = ph >> 1, ph & 1
        g = ops.fold_phase_taps(w.double(), *((a, b) if fold is None else fold(a, b)))      # (cout, cin, 2, 2), fp64: the operand of this phase
        d = xp[:, :, a:a + H + 1, b:b + W + 1].unfold(2, 5, 4).unfold(3, 5, 4)            # (B, C, th, tw, 5, 5)
        V = torch.einsum('ia,bcyxaj->bcyxij', Bt, d.to(dtype))                            # column pass
        V = torch.einsum('bcyxia,ja->bcyxij', V, Bt)                                      # row pass
        Uw = torch.einsum('ia,kcab,jb->ijck', G, g.abs() if absolute else g, G).to(dtype)  # (5, 5, C, N)
        Vm = V.permute(4, 5, 0, 2, 3, 1).reshape(25, B * th * tw, C)
        Um = Uw.reshape(25, C, N)
        M = torch.bmm(Vm, Um) if products is None else products(Vm, Um)
        if zero_positions:
            M = M.clone()
            M[list(zero_positions)] = 0
        At = AT.to(M.dtype)

        def back(Mx):
            Y = torch.einsum('oi,ijbyxk->ojbyxk', At, Mx.reshape(5, 5, B, th, tw, -1))
            Y = torch.einsum('ojbyxk,pj->opbyxk', Y, At)
            return Y.permute(2, 3, 0, 4, 1, 5).reshape(B, H, W, -1)
        parts = [back(M)]
        if absolute:
            parts += [back(Vm.sum(2, keepdim=True)), back(Um.sum(1)[:, None, :].expand(-1, B * th * tw, -1))]
        for i, y in enumerate(parts):
            if out[i] is None:
                out[i] = y.new_zeros(B, 2 * H, 2 * W, y.shape[3])
            out[i][:, a::2, b::2] = y
    return out[0], ((out[1], out[2]) if absolute else None)


def conv64(p, w):
    return F.conv2d(p.permute(0, 3, 1, 2), w.double(), padding=1).permute(0, 2, 3, 1)


def reference(d):
    """-> dict(pre, out) in fp64; out equals conv_case.reference on the same tensors (asserted by the host test)."""
    p, _ = prologue64(d)
    pre = conv64(p, d['w']) + d['b'].double()
    out = pre
    if d['epi'] == EPI_RESIDUAL:
        out = pre + d['res'].double()
    elif d['epi'] == EPI_SFT:
        out = d['res'].double() + d['sft_w'] * (d['res'].double() * d['ss'].double() + pre)
    return dict(pre=pre, out=out)


def case_ref(d):
    return case_reference(d['x'], d['w'], d['b'], prologue=d['pro'], epilogue=d['epi'], sc=d['sc'], sh=d['sh'], res=d['res'], ss=d['ss'], upsample=d['up'],
                          sft_w=d['sft_w'])


def act_scale_of(d):
    """(B,) the power of two ops.act_scale gives an un-normalised input (4 max|x_b| into [2^13, 2^14)); ones with an affine prologue."""
    B = d['x'].shape[0]
    if d['pro'] not in (PRO_NONE, PRO_LEAKY):
        return torch.ones(B, dtype=torch.float64)
    mx = d['x'].abs().reshape(B, -1).max(1).values.double() * 4.0
    return torch.tensor([1.0 if v == 0 else 2.0 ** (14 - math.frexp(float(v))[1]) for v in mx], dtype=torch.float64)


def pack_scale_of(d, m, up=False):
    w = d['w']
    return ops.pack_scale(ops._f23_max(w) if m == 2 else ops._f43_max(w) if m == 4 else float(w.abs().max()) * (4.0 if up else 1.0))


def coef(route, code, cin, split_k=0, up=False, live=None):
    """live: the number of input channels whose weight is not an exact zero, where that is fewer than cin (the solo families): the chains' length.
    (The split-K chunk additions stay cin / 128: every chunk is added.)"""
    m, op = scheme_of(route, code)
    n = cin if live is None else live
    if m == 0:
        return (9 * n if op == 'f32' else 27 * n + 12) + (3 if up else 0)
    t = 7 if m == 2 else 15 if m == F42 else 19
    if op == 'f32':
        return n + t + (cin // 128 if split_k else 0)
    if op == 'half2':
        return 3 * n + 12 + t + (cin // 128 if split_k else 0)
    return n + t + 2.0 * (2.0 ** -11 if op == 'half' else 2.0 ** -8) / U


def live_channels(d):
    """(cout, cin) bool: the input channels an output channel has a non-zero weight for."""
    return (d['w'] != 0).flatten(2).any(2)


def solo_kinds(d):
    """(B, cin) bool x 2, of the conv's input as the kernels split it (fp32, through the prologue or under the range scale), among the channels some
    output reads: channels whose EVERY lo half is a subnormal half (max |a| < 2^-3) while their hi halves are normal (median |a| >= 2^-14), and
    channels whose every hi half is subnormal too (0 < max |a| < 2^-14)."""
    s = act_scale_of(d).float()[:, None, None, None]
    a = (d['x'] * d['sc'][:, None, None, :] + d['sh'][:, None, None, :] if d['pro'] == PRO_AFFINE else d['x'] * s).abs().flatten(1, 2)
    mx, med, read = a.amax(1), a.median(1).values, live_channels(d).any(0)[None, :]
    return (mx < LO_SUBNORMAL) & (med >= HI_SUBNORMAL) & read, (mx < HI_SUBNORMAL) & (mx > 0) & read


@functools.lru_cache(maxsize=None)
def _abs_eval(name, key, variant, m):
    """(S, P / u-free prologue term, sum|p| term, sum|w| term) of a family at a shape for the transform m, fp64."""
    d = family(name, key, variant)
    p, ep = prologue64(d)
    live = live_channels(d).double() if name in SOLO_FAMILIES else None       # the solo families: sum |p| over the channels that have halves in the sum
    if m == 0:
        ones_w, ones_p = torch.ones_like(d['w']), torch.ones_like(p)
        fv = conv64(p.abs(), ones_w)[..., :1] if live is None else conv64(p.abs(), live[:, :, None, None] * ones_w)
        return conv64(p.abs(), d['w'].abs()), conv64(ep, d['w'].abs()), fv, conv64(ones_p, d['w'].abs())
    S, (fv, fu) = wino(p, d['w'], m, absolute=True)
    P, _ = wino(ep, d['w'], m, absolute=True)
    if live is not None:          # sum over the live channels of |V|, per output channel, through |A^T| . |A|: exact, no bound
        fv, _ = wino(p, d['w'], m, absolute=True, products=lambda Vm, Um: torch.matmul(Vm, live.t()))
    return S, P, fv, fu


@functools.lru_cache(maxsize=None)
def prepared(name, key, variant=0):
    d = family(name, key, variant)
    return d, reference(d)


def gate(name, key, route, code, split_k=0, variant=0):
    """The tolerance per element (B, Ho, Wo, cout), fp64."""
    d, ref = prepared(name, key, variant)
    m, op = scheme_of(route, code)
    cin = d['w'].shape[1]
    S, P, fv, fu = _abs_eval(name, key, variant, m)
    solo = name in SOLO_FAMILIES
    live = int(live_channels(d).sum(1).max()) if solo else None
    assert live in (None, 1)
    g = coef(route, code, cin, split_k, d['up'], live) * U * S + P + 2 * U * ref['pre'].abs()
    if op in ('half2', 'half'):
        s = act_scale_of(d)[:, None, None, None]
        g = g + (2.0 ** -24 if solo else 2.0 ** -25) * (1.0 + 2.0 ** -10) * (fv / pack_scale_of(d, m, d['up']) + fu / s)
    if d['epi'] == EPI_RESIDUAL:
        g = g + 2 * U * ref['out'].abs()
    elif d['epi'] == EPI_SFT:
        r0, r1, w = d['res'].double(), d['ss'].double(), d['sft_w']
        g = g + 2 * U * ((w * r0 * r1).abs() + 2 * (w * (r0 * r1 + ref['pre'])).abs() + ref['out'].abs())
    return g


# ---- fp32 emulation of every operand scheme and transform ---------------------------------------------------------------------------------------
def _halves(t):
    hi, lo = split_halves(t.numpy())
    return torch.from_numpy(hi), torch.from_numpy(lo)


def _round16(t, op):
    return t.to(torch.float16 if op == 'half' else torch.bfloat16).float()


def drop_small_lo(a, ah, al):
    """The edit the solo families exist for: the lo half of an activation zeroed wherever it is a subnormal half (|a| < 2^-3 under the range scale)."""
    return ah, torch.where(a.abs() < LO_SUBNORMAL, torch.zeros_like(al), al)


def drop_every_lo(a, ah, al):
    return ah, torch.zeros_like(al)


def emulate(d, route, code, act_halves=None, fold=None, zero_positions=()):
    """The route's arithmetic in torch float32 -> (B, Ho, Wo, cout) float32.  act_halves(a, hi, lo) -> (hi, lo): an edit of the activation's split
    (split halves only; default none), for the host test that shows which family notices it.  fold, zero_positions: wino42's two edits (w42_up only)."""
    m, op = scheme_of(route, code)
    f = torch.float32
    x, sc, sh = d['x'], d['sc'][:, None, None, :], d['sh'][:, None, None, :]
    s = act_scale_of(d).float()[:, None, None, None] if op != 'f32' else torch.ones(x.shape[0], 1, 1, 1)
    if d['pro'] in (PRO_AFFINE, PRO_AFFINE_SWISH):
        p = x * sc + sh
        if d['pro'] == PRO_AFFINE_SWISH:
            p = p * torch.sigmoid(p)
    elif d['pro'] == PRO_LEAKY:
        p = x * torch.where(x > 0, s, 0.2 * s)
    else:
        p = x * s
    if d['up']:
        p = p.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    scale = 1.0 if op == 'f32' else pack_scale_of(d, m, d['up'])

    def products(a, b):               # a: (.., M, C) activations, b: (.., C, N) weights times scale, both float32
        if op == 'f32':
            return a @ b
        if op == 'half2':
            ah, al = _halves(a)
            if act_halves is not None:
                ah, al = act_halves(a, ah, al)
            bh, bl = _halves(b)
            return (al @ bh + ah @ bl) + ah @ bh
        return _round16(a, op) @ _round16(b, op)

    if m == 0:
        cols = F.unfold(p.permute(0, 3, 1, 2), 3, padding=1).transpose(1, 2)      # (B, HW, cin * 9)
        wm = (d['w'].reshape(d['w'].shape[0], -1).t() * scale).contiguous()
        v = products(cols.contiguous(), wm).reshape(*p.shape[:3], -1)
    else:
        Um_scale = torch.tensor(scale, dtype=torch.float64)
        if m == F42:
            v, _ = wino42(p[:, ::2, ::2], d['w'].double() * Um_scale, f, products=products, fold=fold, zero_positions=zero_positions)
        else:
            v, _ = wino(p, d['w'].double() * Um_scale, m, dtype=f, products=products)
    assert v.dtype == f
    v = v * (1.0 / scale) / s + d['b']
    if d['epi'] == EPI_RESIDUAL:
        v = v + d['res']
    elif d['epi'] == EPI_SFT:
        v = d['res'] + d['sft_w'] * (d['res'] * d['ss'] + v)
    assert v.dtype == f
    return v


def ratio(got, ref, tol):
    """Largest |got - ref| / tol over the elements (inf where got is not finite) and the largest |error|."""
    e = (got.double().cpu() - ref['out']).abs()
    e = torch.where(torch.isfinite(e), e, torch.full_like(e, float('inf')))
    return float(torch.where(e == 0, torch.zeros_like(e), e / tol).max()), float(e.max())       # (an exact element meets any gate, a zero one included)


@functools.lru_cache(maxsize=None)
def emulated(name, key, route, code, variant=0):
    d, ref = prepared(name, key, variant)
    return ratio(emulate(d, route, code), ref, gate(name, key, route, code, 0, variant))


def exactness_preconditions(key='f'):
    """int_coded at a shape, every (prologue, epilogue) variant: every transform-domain value of F(2,3) fits 8 significand bits (bf16; IEEE half with a zero
    lo half), directly and under the pack scale; every accumulator's sum of |products|, through the output transform, the folded taps and the
    epilogue, stays below 2^24 units.  -> the largest such sum in units."""
    worst = 0.0
    for variant in range(4):
        d = family('int_coded', key, variant)
        p, _ = prologue64(d)
        BT, G, AT = mats(2)
        unit_v, unit_u = 0.5, 2.0 ** -7
        xp = F.pad(p.permute(0, 3, 1, 2), (1, 1, 1, 1)).unfold(2, 4, 2).unfold(3, 4, 2)
        V = torch.einsum('ia,bcyxaj,lj->bcyxil', BT, xp, BT)
        Uw = torch.einsum('ia,kcab,jb->ijck', G, d['w'].double(), G)
        for t, unit in ((V, unit_v), (Uw, unit_u), (p, unit_v), (d['w'].double(), 2.0 ** -5)):
            q = t / unit
            assert torch.equal(q, q.round()) and float(q.abs().max()) < 256, float(q.abs().max())     # at most 8 bits
        scale = pack_scale_of(d, 2)
        for t in (V.float().numpy(), (Uw * scale).float().numpy(), p.float().numpy(), (d['w'] * pack_scale_of(d, 0, d['up'])).numpy()):
            hi, lo = split_halves(t)
            assert np.array_equal(hi, t) and not lo.any()
            assert np.array_equal(torch.from_numpy(t).bfloat16().float().numpy(), t)
        unit = unit_v * unit_u
        ref = reference(d)
        epi = float(max(d['b'].abs().max(), d['res'].abs().max() * (1 + d['ss'].abs().max())))
        for S in (_abs_eval('int_coded', key, variant, 2)[0], _abs_eval('int_coded', key, variant, 0)[0] * (4 if d['up'] else 1)):
            tot = (float(S.max()) + epi + float(ref['out'].abs().max())) / unit
            assert tot < 2.0 ** 24, tot
            worst = max(worst, tot)
        assert torch.equal(ref['out'], ref['out'].float().double())
    return worst


# ---- the kernels -----------------------------------------------------------------------------------------------------------------------------
def bits_equal(a, b):
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


_PW = {}


def packed(d, code, name_key):
    k = (name_key, code)
    if k not in _PW:
        up2x = d['up'] and code not in (ops.WF43F, ops.WF42U)          # (both are packings of their own: ops.pack_weight(w, b, bf16=code) is the whole call)
        _PW[k] = ops.pack_weight(d['w'].cuda(), d['b'].cuda(), bf16=code, up2x=up2x)
    return _PW[k]


def run(d, code, split_k=0, name_key=None, x=None, images=None, c_split='shape'):
    """One launch of the family's tensors with the explicit pack code -> (B, Ho, Wo, cout) CUDA tensor.  x: another input tensor; images: a slice of
    the batch; c_split: 'shape' = the shape's own, None = dense."""
    key = d['key']
    cs = SHAPES[key][5] if c_split == 'shape' else c_split
    pw = packed(d, code, name_key or id(d))
    sl = slice(None) if images is None else images
    xs = (d['x'] if x is None else x)[sl].contiguous()
    x1, x2, kw = launch_args(xs, d['sc'][sl].contiguous(), d['sh'][sl].contiguous(), d['res'][sl].contiguous(), d['ss'][sl].contiguous(),
                             prologue=d['pro'], epilogue=d['epi'], stats=False, upsample=d['up'], c_split=cs)
    if d['epi'] == EPI_SFT:
        kw['sft_w'] = d['sft_w']
    if d['pro'] in (PRO_NONE, PRO_LEAKY):
        kw['act'] = ops.act_scale(x1, x2)
    if split_k:
        kw['split_k'] = split_k
    return ops.conv2d(x1, pw, x2=x2, **kw)


def launches(key, only_routes=None):
    """[(code name, code, split_k, route, form)] of a shape."""
    return [(n, CODES[n], sk, r, f) for n, sk, r, f in routes()[key] if only_routes is None or r in only_routes]


def case(name, key, code, split_k, route, variant=0, emulate_too=True):
    d, ref = prepared(name, key, variant)
    tol = gate(name, key, route, code, split_k, variant)
    r, err = ratio(run(d, code, split_k, (name, key, variant)), ref, tol)
    er = emulated(name, key, route, code, variant) if emulate_too else (math.nan, math.nan)
    return dict(ratio=r, err=err, emu_ratio=er[0], emu_err=er[1])


if __name__ == '__main__':
    with_f42()
    bad = 0
    for fam in GATE_FAMILIES + SOLO_FAMILIES + ('onehot_pixels',):
        for key in SHAPES:
            if SHAPES[key][6] and fam in ('mixed_cin', 'swish_leaky_edges', 'swish_leaky_edges_sft', 'solo_cin'):
                continue          # (upsampling shapes take no prologue: these families are their prologue)
            for cname, code, sk, route, form in launches(key):
                r = case(fam, key, code, sk, route)
                ok = r['ratio'] <= 1.0
                bad += not ok
                print(f'[{"ok" if ok else "FAIL"}] {fam:21s} {key:2s} {SHAPES[key][:5]} {route:9s} {cname:8s} {form:18s}: kernel max|d| {r["err"]:.3e} = '
                      f'{r["ratio"]:.4f} of the gate | emulation {r["emu_err"]:.3e} = {r["emu_ratio"]:.4f}', flush=True)
    sys.exit(1 if bad else 0)
