"""-m gpu: the ORDER of the fp64 sums of the scoring kernels (csrc/cf_score_parts.h), bitwise.

The other GPU tests hold these sums to float64 references within a tolerance, which an edit that reorders a sum still meets.  Here a NumPy float64
emulation of the order the header documents is compared bit for bit with the device:
  * a thread adds its items in ascending order, and the elements of an item in ascending order;
  * a wave: the xor butterfly 32, 16, .., 1 over its 64 lanes, v = v + v[lane ^ o];
  * a workgroup: its four waves as ((w0 + w1) + w2) + w3;
  * the finish: lane l adds the image's partials l, l + 64, .. in ascending order, then the butterfly.
Cases: ops.feat_dist (float32, 16-byte and scalar path, more than 64 chunks so that the finish wraps its lanes) and the sse output of ops.psnr
(float32 without y: 16-byte path; scalar path with a ragged group at every row end and 66 strips).  uint8 and Y inputs are left out (their sums
are exact: order cannot show), lpips_head too (a float32 divide and square root per element).  Inputs are mixed-scale, normal * 2^uniform(-8, 8),
each case under a seed at which every emulated sum differs in bits from np.sum of the same terms: on an input where order is invisible a reordered kernel
would pass.  The zero padding of the emulation is invisible: every sum here is of non-negative terms, and s + (+0) is s.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEEDS = {('feat', 'vec'): 220, ('feat', 'scalar_wrap'): 1, ('sse', 'vec'): 3, ('sse', 'scalar_wrap'): 19}  # the first that show the order, found on the CPU
FEAT_CHUNK, SSE_ROWS = 16384, 8
FEAT_N = {'vec': 2 * FEAT_CHUNK + 8, 'scalar_wrap': 65 * FEAT_CHUNK + 6}
SSE_SHAPES = {'vec': (24, 16, 3), 'scalar_wrap': (521, 13, 3)}
BATCH = 2
LANE = np.arange(64)


def _mixed(rng, shape):
    return (rng.standard_normal(shape) * 2.0 ** rng.uniform(-8, 8, shape)).astype(np.float32)


def _butterfly(v):
    """(.., 64) lanes -> what lane 0 holds after the xor tree."""
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., LANE ^ o]
    return v[..., 0]


def _block_sum(items):
    """items (m, G): item i goes to thread i % 256; the workgroup's sum."""
    m, g = items.shape
    pad = np.zeros((-(-m // 256) * 256, g))
    pad[:m] = items
    acc = np.zeros(256)
    for step in pad.reshape(-1, 256, g):
        for k in range(g):
            acc = acc + step[:, k]
    w = _butterfly(acc.reshape(4, 64))
    return ((w[0] + w[1]) + w[2]) + w[3]


def _finish(parts):
    pad = np.zeros(-(-len(parts) // 64) * 64)
    pad[:len(parts)] = parts
    acc = np.zeros(64)
    for row in pad.reshape(-1, 64):
        acc = acc + row
    return _butterfly(acc)


def _groups_of_4(row_terms):
    """(rows, n) -> (rows * ceil(n / 4), 4): every row cut into groups of 4, the last one padded."""
    rows, n = row_terms.shape
    pad = np.zeros((rows, -(-n // 4) * 4))
    pad[:, :n] = row_terms
    return pad.reshape(-1, 4)


def _feat_dist_emulated(a, b):
    """(B, 2) and the terms (B, 2, n) it adds."""
    d = (a - b).astype(np.float64)  # one float32 subtraction, then widened
    terms = np.stack([np.abs(d), d * d], axis=1)
    out = [[_finish(np.array([_block_sum(_groups_of_4(t[None, e0:e0 + FEAT_CHUNK])) for e0 in range(0, len(t), FEAT_CHUNK)])) for t in img] for img in terms]
    return np.array(out), terms


def _sse_emulated(a, b):
    """(B,) and the terms (B, H, W * C) it adds."""
    d = a.astype(np.float64) - b.astype(np.float64)
    terms = (d * d).reshape(a.shape[0], a.shape[1], -1)
    out = [_finish(np.array([_block_sum(_groups_of_4(t[y0:y0 + SSE_ROWS])) for y0 in range(0, len(t), SSE_ROWS)])) for t in terms]
    return np.array(out), terms


def _order_shows(emulated, terms):
    plain = terms.reshape(emulated.shape + (-1,)).sum(axis=-1)
    assert emulated.shape == plain.shape
    return bool(np.all(emulated.view(np.uint64) != plain.view(np.uint64)))


def _inputs(kind, case):
    rng = np.random.default_rng([SEEDS[kind, case], sorted(FEAT_N).index(case), kind == 'sse'])
    shape = (BATCH, FEAT_N[case]) if kind == 'feat' else (BATCH,) + SSE_SHAPES[case]
    return _mixed(rng, shape), _mixed(rng, shape)


@pytest.fixture(scope='module')
def ops():
    from codeformer_amd import build as cf_build
    cf_build.build()
    assert torch.cuda.is_available()
    from codeformer_amd import ops
    return ops


@pytest.mark.parametrize('case', sorted(FEAT_N))
def test_feat_dist_adds_in_the_documented_order(ops, case):
    a, b = _inputs('feat', case)
    want, terms = _feat_dist_emulated(a, b)
    assert _order_shows(want, terms), 'the input does not show the order: pick another seed'
    got = ops.feat_dist(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()).cpu().numpy()
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (got, want)


@pytest.mark.parametrize('case', sorted(SSE_SHAPES))
def test_sse_adds_in_the_documented_order(ops, case):
    a, b = _inputs('sse', case)
    want, terms = _sse_emulated(a, b)
    assert _order_shows(want, terms), 'the input does not show the order: pick another seed'
    got = ops.psnr(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), y_channel=False)[0].cpu().numpy()
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (got, want)
