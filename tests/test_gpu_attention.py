"""-m gpu: the two attention kernels (cf_attention.hip: attn64_kernel, attn512_kernel) beyond near-uniform softmax.

The families, the fp64 reference, the gate and its derivation live in tools/attn_check.py (runnable stand-alone: one report line per
case); tests/test_attention_families_host.py proves on the CPU that a sequential fp32 evaluation stays within 0.5 of the gate
    |got - ref| <= 5e-6 + 1e-5 |ref| + 0.5 2^-24 sqrt(head_dim) L_r max|v|        (L_r: the row's largest |logit| in fp64)
so the gate is a condition on the reference; no number here was tuned to what a kernel returns.

Beside the gate: onehot bitwise v[pi], ones within 2^-16 of 1, duplicated keys bitwise equal probabilities, other head counts and head
isolation, batch invariance (16 and 3 images), leading dimensions, the power-of-two scale claim of the kernel header, the output
stride of the C ABI, containment of non-finite inputs, and the refusals (misaligned base pointers among them).

Measured on an MI355X (largest |error| of the kernel = that fraction of the gate | the CPU emulation's), 8x64 then 1x512:
    uniform       1.6e-07 = 0.017 |  2.5e-07 = 0.031         2.3e-07 = 0.022 |  3.9e-07 = 0.034
    peak4         1.6e-06 = 0.075 |  2.1e-06 = 0.100         2.2e-06 = 0.089 |  2.1e-06 = 0.087
    peak12        3.8e-06 = 0.084 |  7.0e-06 = 0.158         4.3e-06 = 0.068 |  5.9e-06 = 0.096
    peak40        1.1e-06 = 0.014 |  2.3e-06 = 0.037         1.1e-11 = 0.000 |  1.1e-11 = 0.000
    onehot        0       (bitwise v[pi])  |  0              0       (bitwise v[pi])  |  0
    offset+30     1.6e-06 = 0.036 |  1.6e-06 = 0.038         6.0e-06 = 0.060 |  6.0e-06 = 0.060
    offset+90     6.3e-06 = 0.057 |  6.3e-06 = 0.057         1.9e-05 = 0.066 |  1.9e-05 = 0.067
    offset-300    2.3e-05 = 0.066 |  2.3e-05 = 0.066         4.8e-05 = 0.053 |  4.8e-05 = 0.053
    offset+3000   1.9e-04 = 0.057 |  1.9e-04 = 0.057         7.5e-04 = 0.082 |  7.5e-04 = 0.082
    big           2.0e-05 = 0.320 |  2.3e-05 = 0.330         5.8e-05 = 0.370 |  5.3e-05 = 0.345
    allsame       7.1e-08 = 0.014 |  1.5e-07 = 0.021         8.7e-08 = 0.013 |  1.2e-07 = 0.019
    P uniform     1.7e-08 = 0.003 |  3.5e-08 = 0.006         3.9e-08 = 0.006 |  3.1e-08 = 0.005
    P peak4       5.9e-07 = 0.054 |  5.1e-07 = 0.053         6.5e-07 = 0.065 |  6.8e-07 = 0.070
    P offset+90   1.2e-06 = 0.044 |  1.2e-06 = 0.043         4.8e-06 = 0.071 |  4.8e-06 = 0.071
    ones          4.8e-07 = 0.031 |  1.4e-06 = 0.088         7.2e-07 = 0.045 |  1.1e-06 = 0.061      (bound 2^-16 = 1.5e-5)
    dup           5.8e-07 = 0.052 |  6.0e-07 = 0.054         6.5e-07 = 0.064 |  6.8e-07 = 0.069      (duplicated columns bitwise equal)
Other head counts (peak4): 2 x 512 0.082, 1 x 64 0.058, 8 x 64 0.075 of the gate; batch 16: 0.094 / 0.117, batch 3: 0.084 / 0.103.
The kernels needed no change.  Scratch builds with one edit each (not committed): without `- m` in phase 2 of attn64_kernel 7 tests of
this file fail (onehot, offset+90 / -300 / +3000, big, P offset+90, ones), of attn512_kernel 5 (onehot, the three offsets, P offset+90),
and g_attn of tools/gpu_check.py passes both; with the V halves or the key groups of attn64_kernel's phase 3 swapped on the P side 19 fail.
"""
import pytest

from _tools import load_script

pytestmark = pytest.mark.gpu

FLAVOURS = ('8x64', '1x512')
FAMILIES = ('uniform', 'peak4', 'peak12', 'peak40', 'onehot', 'offset+30', 'offset+90', 'offset-300', 'offset+3000', 'big', 'allsame',
            'P uniform', 'P peak4', 'P offset+90', 'ones', 'dup')


@pytest.fixture(scope='module')
def ac():
    import torch
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    from codeformer_amd import lib
    lib.load()
    m = load_script('tools/attn_check.py')
    assert m.FAMILIES == FAMILIES and tuple(m.FLAVOURS) == FLAVOURS
    return m


def _run(inp, B, H, dh, scale):
    from codeformer_amd import ops
    return ops.attention(inp['q'].cuda(), inp['k'].cuda(), inp['v'].cuda(), B, H, dh, scale)


def _within_gate(ac, got, inp, H, dh, scale):
    P, L = ac.ref_probs(inp['q'], inp['k'], H, dh, scale)
    ref = ac.ref_out(P, inp['v'], H, dh)
    tol = ac.gate(ref, L, float(inp['v'].abs().max()), dh, 0.5)
    d = (got.double().cpu() - ref).abs()
    return bool(got.isfinite().all()) and bool((d <= tol).all()), float((d / tol).max())


# ---- 1. the families against the gate ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('flavour', FLAVOURS)
def test_family_within_the_gate(ac, flavour, family):
    res = ac.case(flavour, family, kernel=True, emulate=False)
    print(ac.line(res))
    k = res['kernel']
    assert k['finite'], res
    assert k['ratio'] <= 1.0, res
    assert (k['special'] is not None) == (family in ('onehot', 'ones', 'dup'))
    assert k['special'] is not False, res         # onehot: bitwise v[pi]; ones: within 2^-16 of 1; dup: duplicated P columns bitwise equal


# ---- 2. other head counts, and heads do not see each other -------------------------------------------------------------------------------
def _perturbed(ac, inp, H, dh, heads, seed):
    """A copy of the inputs with q, k and v of `heads` replaced by other data."""
    out = {}
    for i, n in enumerate('qkv'):
        t = inp[n].clone()
        new = ac.rnd(tuple(t.shape), seed + i, 3.0)
        for h in heads:
            t[:, h * dh:(h + 1) * dh] = new[:, h * dh:(h + 1) * dh]
        out[n] = t
    return out


@pytest.mark.parametrize('H,dh,groups', [(2, 512, ((0,), (1,))), (1, 64, ()), (8, 64, ((3,), (0, 1, 2, 4, 5, 6, 7)))])
def test_head_counts_and_head_isolation(ac, H, dh, groups):
    scale = dh ** -0.5
    inp = ac.inputs('peak4', H, dh, scale, seed=20 + H, batch=2)
    got = _run(inp, 2, H, dh, scale)
    ok, r = _within_gate(ac, got, inp, H, dh, scale)
    print(f'heads {H} x {dh} peak4: largest error / gate {r:.3f}')
    assert ok, (H, dh, r)
    for changed in groups:
        kept = [h for h in range(H) if h not in changed]
        got2 = _run(_perturbed(ac, inp, H, dh, changed, seed=50), 2, H, dh, scale)
        for h in kept:
            assert ac.bits_equal(got[:, h * dh:(h + 1) * dh], got2[:, h * dh:(h + 1) * dh]), (H, dh, changed, h)
        for h in changed:      # (the perturbation did reach the kernel)
            assert not ac.bits_equal(got[:, h * dh:(h + 1) * dh], got2[:, h * dh:(h + 1) * dh]), (H, dh, changed, h)


# ---- 3. batch ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('flavour', FLAVOURS)
@pytest.mark.parametrize('B,alone', [(16, (0, 7, 15)), (3, (1,))])
def test_batch_invariance_and_repeatability(ac, flavour, B, alone):
    fl = ac.FLAVOURS[flavour]
    H, dh, scale = fl['heads'], fl['head_dim'], fl['scale']
    inp = ac.inputs('peak4', H, dh, scale, seed=30 + B, batch=B)
    dev = {n: inp[n].cuda() for n in 'qkv'}
    from codeformer_amd import ops
    full = ops.attention(dev['q'], dev['k'], dev['v'], B, H, dh, scale)
    assert ac.bits_equal(full, ops.attention(dev['q'], dev['k'], dev['v'], B, H, dh, scale))
    ok, r = _within_gate(ac, full, inp, H, dh, scale)
    print(f'{flavour} batch {B} peak4: largest error / gate {r:.3f}')
    assert ok, (flavour, B, r)
    for i in alone:
        rows = slice(i * 256, (i + 1) * 256)
        one = ops.attention(dev['q'][rows].contiguous(), dev['k'][rows].contiguous(), dev['v'][rows].contiguous(), 1, H, dh, scale)
        assert ac.bits_equal(full[rows], one), (flavour, B, i)


# ---- 4. leading dimensions ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('flavour', FLAVOURS)
def test_leading_dimensions_do_not_change_the_bits(ac, flavour):
    """Dense operands, slices of one 3E-wide matrix, slices of matrices E + 4 and E + 64 wide (mixed: the MultiheadAttention call pattern has
    q | k in one buffer and v in another) and a slice that starts at column 4.  What lies beside a slice is NaN: it must not be read."""
    import torch
    from codeformer_amd import ops
    fl = ac.FLAVOURS[flavour]
    H, dh, scale = fl['heads'], fl['head_dim'], fl['scale']
    E, R = H * dh, 512
    inp = ac._prepared(flavour, 'peak12')[0]
    dense = _run(inp, 2, H, dh, scale)
    ok, _ = _within_gate(ac, dense, inp, H, dh, scale)
    assert ok

    def wide(t, width, at):
        m = torch.full((R, width), float('nan'), device='cuda')
        m[:, at:at + E] = t.cuda()
        return m[:, at:at + E]

    qkv = torch.cat([inp['q'], inp['k'], inp['v']], 1).cuda()
    layouts = {
        '3E slices': (qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:]),
        'E+4': tuple(wide(inp[n], E + 4, 0) for n in 'qkv'),
        'E+64': tuple(wide(inp[n], E + 64, 0) for n in 'qkv'),
        'mixed': (wide(inp['q'], E + 4, 0), wide(inp['k'], E + 64, 0), inp['v'].cuda()),
        'offset 4': tuple(wide(inp[n], E + 4, 4) for n in 'qkv'),
        'offset 4 of E+64': (wide(inp['q'], E + 64, 4), wide(inp['k'], E + 64, 60), wide(inp['v'], E + 64, 32)),
    }
    for name, (q, k, v) in layouts.items():
        assert all(t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0 for t in (q, k, v)), name
        assert ac.bits_equal(dense, ops.attention(q, k, v, 2, H, dh, scale)), (flavour, name)


# ---- 5. the header's claim: scaling the scores by 1/8 is bit-identical to scaling q -------------------------------------------------------
@pytest.mark.parametrize('family', ['uniform', 'peak12', 'big'])
def test_power_of_two_scale_is_bitwise_prescaled_q(ac, family):
    from codeformer_amd import ops
    inp = ac._prepared('8x64', family)[0]
    q, k, v = (inp[n].cuda() for n in 'qkv')
    assert ac.bits_equal(ops.attention(q * 0.125, k, v, 2, 8, 64, 1.0), ops.attention(q, k, v, 2, 8, 64, 0.125)), family


# ---- 6. the output stride of the C ABI -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('flavour', FLAVOURS)
def test_output_stride_leaves_the_padding_alone(ac, flavour):
    import torch
    from codeformer_amd import lib as L
    lib = L.load()
    fl = ac.FLAVOURS[flavour]
    H, dh, scale = fl['heads'], fl['head_dim'], fl['scale']
    E, R, SENTINEL = H * dh, 512, -1234.5
    inp = ac._prepared(flavour, 'peak4')[0]
    q, k, v = (inp[n].cuda() for n in 'qkv')
    dense = _run(inp, 2, H, dh, scale)
    out = torch.full((R, E + 8), SENTINEL, device='cuda')
    L.check(lib.cf_attention(q.data_ptr(), E, k.data_ptr(), E, v.data_ptr(), E, out.data_ptr(), E + 8, 2, H, dh, 256, float(scale), L.stream_ptr()),
            'cf_attention')
    torch.cuda.synchronize()
    assert ac.bits_equal(out[:, :E], dense)
    assert bool((out[:, E:] == SENTINEL).all())
    # an output stride below heads * head_dim is refused
    assert lib.cf_attention(q.data_ptr(), E, k.data_ptr(), E, v.data_ptr(), E, out.data_ptr(), E - 4, 2, H, dh, 256, float(scale), L.stream_ptr()) != 0
    assert 'cf_attention' in L.last_error()
    # and so is an output base that is not 16-byte aligned (ldo a multiple of 4), before any launch
    assert lib.cf_attention(q.data_ptr(), E, k.data_ptr(), E, v.data_ptr(), E, out.data_ptr() + 4, E + 8, 1, H, dh, 256, float(scale), L.stream_ptr()) != 0
    assert 'align' in L.last_error()
    torch.cuda.synchronize()
    assert bool((out[:, E:] == SENTINEL).all()) and ac.bits_equal(out[:, :E], dense)


# ---- 7. non-finite inputs stay where they are ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('flavour', FLAVOURS)
def test_non_finite_inputs_are_contained(ac, flavour):
    import torch
    fl = ac.FLAVOURS[flavour]
    H, dh, scale = fl['heads'], fl['head_dim'], fl['scale']
    E = H * dh
    h = H // 2                       # head 4 of 8; the only head of 1 x 512
    cols = slice(h * dh, (h + 1) * dh)
    inp = ac._prepared(flavour, 'uniform')[0]
    clean = _run(inp, 2, H, dh, scale)
    assert bool(clean.isfinite().all())

    def run_with(name, row, col, value):
        bad = {n: inp[n].clone() if n == name else inp[n] for n in 'qkv'}
        bad[name][row, col] = value
        return _run(bad, 2, H, dh, scale)

    def rest_is_clean(got, mask):
        return ac.bits_equal(torch.where(mask, torch.zeros_like(got), got), torch.where(mask, torch.zeros_like(clean), clean))

    # a NaN in one query row of (image 1, head h): exactly that output row of that head
    got = run_with('q', 256 + 37, h * dh + 5, float('nan'))
    mask = torch.zeros(512, E, dtype=torch.bool, device='cuda')
    mask[256 + 37, cols] = True
    assert bool(got[mask].isnan().all()) and rest_is_clean(got, mask), flavour
    # a NaN in one key row of (image 1, head h): all 256 rows of that (image, head)
    got = run_with('k', 256 + 201, h * dh + dh - 1, float('nan'))
    mask = torch.zeros(512, E, dtype=torch.bool, device='cuda')
    mask[256:, cols] = True
    assert bool(got[mask].isnan().all()) and rest_is_clean(got, mask), flavour
    # +inf in one element of V of (image 0, head h): that output column of that (image, head)
    c = h * dh + dh // 2 + 3
    got = run_with('v', 99, c, float('inf'))
    mask = torch.zeros(512, E, dtype=torch.bool, device='cuda')
    mask[:256, c] = True
    assert not bool(got[mask].isfinite().any()) and rest_is_clean(got, mask), flavour


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals(ac):
    import torch
    from codeformer_amd import ops
    z = lambda r, c: torch.zeros(r, c, device='cuda')   # noqa: E731
    with pytest.raises(RuntimeError, match='head_dim'):
        ops.attention(z(256, 128), z(256, 128), z(256, 128), 1, 1, 128, 128 ** -0.5)
    with pytest.raises((ValueError, RuntimeError)):        # rows != batch * 256
        ops.attention(z(255, 512), z(255, 512), z(255, 512), 1, 8, 64, 0.125)
    with pytest.raises((ValueError, RuntimeError)):
        ops.attention(z(512, 512), z(512, 512), z(512, 512), 1, 8, 64, 0.125)
    with pytest.raises((ValueError, RuntimeError)):        # columns != heads * head_dim
        ops.attention(z(256, 576), z(256, 576), z(256, 576), 1, 8, 64, 0.125)
    with pytest.raises((ValueError, RuntimeError)):
        ops.attention(z(256, 512), z(256, 512), z(256, 448), 1, 8, 64, 0.125)
    for E, H, dh in ((512, 8, 64), (512, 1, 512)):
        good = z(256, E)
        odd = z(256, E + 2)[:, :E]                     # a leading dimension that is no multiple of 4 (base aligned)
        for i in range(3):
            args = [good, good, good]
            args[i] = odd
            with pytest.raises(RuntimeError, match='cf_attention'):
                ops.attention(*args, 1, H, dh, dh ** -0.5)
        m = z(256, E + 4)
        shifted = m[:, 1:E + 1]                        # ld a multiple of 4, base 4 bytes off: refused before any launch
        assert shifted.stride(0) % 4 == 0 and shifted.data_ptr() % 16 == 4
        for i in range(3):
            args = [good, good, good]
            args[i] = shifted
            with pytest.raises(RuntimeError, match='align'):
                ops.attention(*args, 1, H, dh, dh ** -0.5)
        assert float(ops.attention(good, good, good, 1, H, dh, dh ** -0.5).abs().max()) == 0.0      # (and the next call is served)
