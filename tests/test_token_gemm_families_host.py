"""CPU: the evidence that the conditions of tests/test_gpu_token_gemm.py are conditions on the REFERENCE, not on what a kernel returns.

For the input families of tools/gemm_check.py at the largest shapes the GPU test uses:
  * the sequential fp32 emulation of both operand schemes (fp32 FMA chain; hi / lo IEEE halves, three products; chunks of 128 summed in order)
    stays within 0.5 of the per-element gate for every gate family;
  * int_coded: every partial sum is an integer below 2^24, every operand and its pack-scaled image exact in half with a zero lo half -- and the
    emulation of both schemes returns the fp64 result bitwise, in every epilogue;
  * onehot_rows / perm_weight: the emulation with fp32 operands returns the selected weight (+ bias) / token bitwise;
  * cancel_chunks has sum|a w| / |ref| >= 1e4 for every element, the chunk weights sum to zero for every V used;
  * mixed_cols reaches subnormal lo AND subnormal hi halves under the scale the host's own rule (ops.pack_scale) chooses, the largest
    columns the top binade of half; mixed_rows crosses both edges of the range the header states for the tokens;
  * gelu_edges: the fp64 pre-activations are the targets exactly, and the emulation of both schemes reproduces them bitwise;
  * routes(): every kernel is reached by at least one of the shapes, the refusals have no route.
"""
import numpy as np
import pytest
import torch

from _tools import load_script


@pytest.fixture(scope='module')
def gc():
    return load_script('tools/gemm_check.py')


LARGEST = (384, 1152, 64)      # the larger of gemm_check.GATE_SHAPES (rows x K), and K = 1152 is the largest K any test uses


def test_shapes_are_the_gpu_tests_shapes(gc):
    assert LARGEST in gc.GATE_SHAPES and all(M * K <= LARGEST[0] * LARGEST[1] and K <= LARGEST[1] for M, K, _ in gc.GATE_SHAPES)
    assert all(M <= 384 and K <= 1152 and N <= 1536 for M, K, N in gc.GATE_SHAPES)


@pytest.mark.parametrize('scheme', ('f32', 'half'))
@pytest.mark.parametrize('family', ('cancel_chunks', 'mixed_cols', 'mixed_rows', 'gelu_edges', 'big_epilogue'))
def test_emulation_within_half_of_the_gate(gc, family, scheme):
    assert family in gc.GATE_FAMILIES
    for shape in gc.GATE_SHAPES:
        r, err = gc.emulated(family, *shape, scheme)
        print(f'{family} {shape} {scheme}: emulation max|d| {err:.3e} = {r:.3f} of the gate')
        assert r <= 0.5, (family, shape, scheme, r, err)


def test_int_coded_is_exact_in_every_association(gc):
    bound = gc.exactness_preconditions(LARGEST[1])
    print(f'int_coded K {LARGEST[1]}: partial sums <= {bound:.0f} < 2^24')
    assert bound < 2 ** 24
    d = gc.family('int_coded', 192, 1152, 64)
    for epi, b, r in ((gc.EPI_NONE, None, None), (gc.EPI_NONE, d['bias'], None), (gc.EPI_RESIDUAL, d['bias'], d['res'])):
        want = gc.reference(d['A'], d['W'], b, r, epi)['out']
        assert torch.equal(want, want.float().double())
        for scheme in ('f32', 'half'):
            assert gc.bits_equal(gc.emulate(d['A'], d['W'], b, r, epi, scheme), want.float()), (epi, scheme)
    # position-coded: exchanging two rows, two columns or two k changes the result
    A, W = d['A'], d['W']
    base = A.double() @ W.double().t()
    for i, j in ((0, 1), (3, 20), (5, 37), (17, 34)):
        Ak = A.clone()
        Ak[:, [i, j]] = Ak[:, [j, i]]
        assert not torch.equal(Ak.double() @ W.double().t(), base), (i, j)
        assert not torch.equal(base[i], base[j]) and not torch.equal(base[:, i], base[:, j])


def test_onehot_and_permutation_select_bitwise(gc):
    M, K, N = 384, 640, 64
    d = gc.family('onehot_rows', M, K, N)
    k = gc.onehot_k(M, K)
    # what the sweep of 384 rows covers (k(m) is the issue's; not every row residue against every k residue: that is int_coded's part): every k residue
    # mod 32 (the stage of the tile kernels), every chunk, every row residue mod 128 in three different chunks, and 24 of the 32 pairs
    # (swizzle class (row >> 2) & 3, 16-byte slot (k mod 32) >> 2) of store_stage / compute, every class and every slot among them
    kl = [int(kk) for kk in k]
    assert len({kk % 32 for kk in kl}) == 32 and len({kk // 128 for kk in kl}) == K // 128
    assert all(len({kl[m] // 128 for m in range(r, M, 128)}) == 3 for r in range(128))
    pairs = {((m >> 2) & 3, (kl[m] % 32) >> 2) for m in range(M)}
    assert len(pairs) == 24 and {a for a, _ in pairs} == set(range(4)) and {c for _, c in pairs} == set(range(8))
    want = d['W'][:, k].t() + d['bias'][None, :]                 # fp32: one rounding
    assert gc.bits_equal(gc.emulate(d['A'], d['W'], d['bias'], None, gc.EPI_NONE, 'f32'), want)
    d = gc.family('perm_weight', 128, 128, 192)
    p, sign = gc.perm_of(192, 128)
    want = torch.zeros(128, 192)
    want[:, :128] = d['A'][:, p] * sign[None, :]
    assert gc.bits_equal(gc.emulate(d['A'], d['W'], None, None, gc.EPI_NONE, 'f32') + 0.0, want + 0.0)
    assert float((gc.emulate(d['A'], d['W'], None, None, gc.EPI_NONE, 'half').double() - want.double()).abs().max()) <= \
        float((2.0 ** -22 + gc.U) * d['A'].abs().max() + 2.0 ** -25)


def test_cancel_chunks_conditioning(gc):
    for V in (1, 3, 5, 8, 9):
        assert sum(gc.chunk_weights(V)) == 0 or V == 1
        assert V < 3 or len(set(abs(w) for w in gc.chunk_weights(V))) >= 2        # unequal sizes: the order of the chunk additions is visible
    for shape in gc.GATE_SHAPES + ((64, 128, 64), (64, 640, 64)):
        d, ref, _ = gc.prepared('cancel_chunks', *shape)
        cond = float((ref['S'] / ref['out'].abs()).min())
        print(f'cancel_chunks {shape}: smallest sum|a w| / |ref| = {cond:.3g}, largest |ref| {float(ref["out"].abs().max()):.2f}')
        assert cond >= 1e4, (shape, cond)
        # the chunk sums really are +-S with S >= 2e4
        K = shape[1]
        part = torch.stack([d['A'][:, c:c + 128].double() @ d['W'][:, c:c + 128].double().t() for c in range(0, K, 128)])
        if K > 128:
            assert float(part.abs().min()) >= 2e4 - 10


def test_mixed_families_reach_the_subnormal_halves(gc):
    from codeformer_amd import ops
    for shape in gc.GATE_SHAPES:
        d = gc.family('mixed_cols', *shape)
        W = d['W']
        scale = ops.pack_scale(float(W.abs().max()))          # the host's own rule
        assert scale == gc.pack_scale_of(W)
        hi, lo = gc.split_halves(W.numpy() * np.float32(scale))
        top = np.abs(hi).max()
        assert 2.0 ** 14 <= top < 2.0 ** 15
        col_hi, col_lo = np.abs(hi).max(1), np.abs(lo).max(1)
        sub_lo = (col_lo < gc.HALF_MIN_NORMAL) & (col_lo > 0)
        sub_hi = (col_hi < gc.HALF_MIN_NORMAL) & (col_hi > 0)
        print(f'mixed_cols {shape}: scale 2^{int(np.log2(scale))}, columns with only subnormal lo halves {int(sub_lo.sum())}, with only subnormal hi halves {int(sub_hi.sum())}')
        assert sub_lo.sum() >= 4 and sub_hi.sum() >= 2 and col_lo[0] >= gc.HALF_MIN_NORMAL
        a = gc.family('mixed_rows', *shape)['A'].abs()
        rows = a.max(1).values
        assert float(a.max()) <= 65504.0 and float(rows.max()) >= 2.0 ** 14 and float(rows.min()) < 2.0 ** -25 and int(((rows < 2.0 ** -3) & (rows > 2.0 ** -14)).sum()) >= 4


def test_gelu_edges_preactivations_are_exact(gc):
    for shape in gc.GATE_SHAPES:
        M, K, N = shape
        d, ref, _ = gc.prepared('gelu_edges', *shape)
        want = gc.gelu_pre(M, N)
        assert torch.equal(ref['pre'], want)
        assert set(gc.GELU_TARGETS) <= set(float(v) for v in want[:, 0])
        for scheme in ('f32', 'half'):
            pre = gc.emulate(d['A'], d['W'], d['bias'], None, gc.EPI_NONE, scheme)
            assert torch.equal(pre.double(), want), scheme
        g = gc.gelu64(torch.tensor([-10.0, -6.0, -3.0, 0.0, 1.0], dtype=torch.float64))
        assert -1e-22 < float(g[0]) < 0 and abs(float(g[1]) + 5.92e-9) < 1e-10 and abs(float(g[4]) - 0.8413447460685429) < 1e-15


def test_routes_name_every_kernel_and_no_refused_shape(gc):
    shapes = gc.GATE_SHAPES + ((32, 384, 64), (96, 640, 192), (64, 640, 64), (384, 128, 1536), (256, 1024, 192), (128, 1152, 64), (192, 384, 192))
    for k in gc.KERNELS:
        assert any(gc.routes(k, *s) for s in shapes), k
    assert gc.routes('h_sk', 192, 1024, 192)[0] == 1 and 1 not in gc.routes('h_sk', 256, 1024, 192)       # nsplit == 1 only where M % 128 != 0
    assert gc.routes('f32_sk', 192, 384, 192) == [1, 3] and gc.routes('h_sk', 64, 640, 64) == [1, 5]
    assert not gc.routes('h_wg', 128, 1152, 64) and gc.routes('h_wg', 96, 640, 192) == [-1]
    assert not any(gc.routes(k, 48, 384, 64) for k in gc.KERNELS)
    assert not gc.routes('f32_sk', 32, 384, 64) and not gc.routes('h_tile', 32, 384, 64)
