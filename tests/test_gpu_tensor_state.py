"""-m gpu: the state codeformer_amd/ops.py keeps BETWEEN launches -- the GroupNorm partials (`_cf_stats`) and range-scale tables (`_cf_act`,
`_cf_act_pair`) that ride on tensor objects, and the per-stream scratch words of the range-scale / split-K kernels -- when a tensor object is
written a second time.  The contract is stated at the head of "state kept on tensor objects" in ops.py; every test here writes twice into one
object (or grows the scratch under a captured graph) and compares with

  (i)  fp64 on the CPU of the tensor read back from the device: tests/test_gpu_norm_conditioning.py's `_check_tables` (its `table_bounds`, the
       NT entry of the producing family, FACTOR, the row inside ENVELOPE) -- no tolerance of this file's own;
  (ii) the same calls on a fresh tensor (out=None): bitwise.

Shapes: NHWC, batch 2, nothing above 2 x 16 x 16 x 64.  Producer P: 3x3 stride 1, 64 -> 64 on 16x16, packed as code 0 ('direct') and as
ops.WINOGRAD ('f23'), both with statistics at 2 channels per group.  Consumer C: 3x3 64 -> 64 packed with ops.SPLIT -> WSPLIT, which applies the
range scale.  Contents A / B (tools/tensor_state_case.py): the producer on seeded randn / on another randn times 2^21 plus a per-channel bias
of magnitude 2^21; tests/test_tensor_state_host.py shows on their fp64 model that a stale table misses (i) by more than 100 x the bound and
that a stale range scale leaves [2^7, 2^14), in both orders.

The pair test runs at 32 channels per member AND at 64: a 32-channel convolution has one channel per group and
emits no partials (conv2d: cout / 32 >= 2), so groupnorm_tables([a, b], act_growth=4.0) parks a pair table from 64 channels per member up only;
at 32 the table is the host-side combination of the two single tables, which are cached per member.  Each member is still 2 x 16 x 16 x 64 at most.

torch.inference_mode: inference tensors keep no version counter and record no `._base` (a slice cannot find its buffer), so there the
library's own write count of the storage (ops.tensor_stamp) is what retires the state of a buffer written through a slice; dead attributes
may stay on such an object, which is why test 3 asks for absent attributes only where PyTorch records the base, and elsewhere that what is
left carries a stamp that no longer matches.

Measured once on an MI355X.  "parent" = ops.py of the commit before the contract, "fix" = with it; "ratio" = largest table error over the
first-order bound ((i) allows FACTOR = 2); "m" = 4 max|x| s of the returned range scale, which must lie in [2^7, 2^14).
  test                                  parent                                                                      fix (largest ratio)
  1 out= reuse with statistics          8 / 8 fail: tables right (new partials), range scale stale in BOTH modes:      pass, 0.256
                                        m = 2^32.8 / 2^33.8 (A then B, direct / f23), 2^-9.4 (B then A)
  2 out= reuse without statistics       8 / 8 fail: tables of the old contents, ratio 1.75e13 (A then B), 4.19e6 (B then A)   pass, 0.807
  3 writing through a view              4 / 4 fail: ratio 1.80e13                                                      pass, 0.807
  4 pair table                          6 / 8 fail: m = 2^33 (64 channels, either member, both modes), 2^34.8 (32        pass, 0.865
                                        channels, normal mode); 32 channels under inference_mode pass (nothing is cached there)
  5 user in-place writes                4 / 4 fail: ratio 8.80e12 (mul_), 1.75e13 (copy_)                              pass, 0.728
  6 copies outlive their source         pass                                                                          pass, 0.246
  7 a refused call leaves state alone   pass                                                                          pass
  8 scratch growth under a graph        fails at the liveness assertion (both old tensors freed); not replayed again     pass
After the fix every m lies in [2^10.85, 2^12.62] for tables from partials and in [2^13.03, 2^13.85] for tables from the tensor.
Wall time: 39 tests in 3.0 s, of which 1.8 s are the module fixture (library load, packing); slowest call 0.24 s
(test_out_reuse_with_statistics[normal-AB-direct], the first launches of the process).

Each part of the fix, reverted alone on a scratch copy, fails these tests (checked once each; nothing else fails):
  popping the three attributes of conv2d's destination      test_out_reuse_with_statistics, test_out_reuse_without_statistics (all 16: what is left on buf)
  doing the same on `._base`                                test_writing_through_a_view[normal-*]
  the version counter in the stamp of `_cf_stats`           test_user_in_place_writes_retire_the_state (all 4)
  the write count (pair invalidation, aliases)              test_pair_table_after_one_member_is_rewritten[*-64-b], test_writing_through_a_view[inference-*]
  keeping replaced scratch tensors                          test_scratch_growth_under_a_captured_graph
"""
import contextlib
import gc
import time
import weakref

import numpy as np
import pytest

from _tools import load_script

pytestmark = pytest.mark.gpu

MODES = ('normal', 'inference')
FAMS = (('direct', 0), ('f23', 'WINOGRAD'))      # NT key of tests/test_gpu_norm_conditioning.py, operand code of the producer
ORDERS = ('AB', 'BA')
GROWTH = 4.0
STATE = ('_cf_stats', '_cf_act', '_cf_act_pair')


class Env:
    pass


@pytest.fixture(scope='module')
def env():
    import torch
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    from codeformer_amd import lib, ops
    lib.load()
    e = Env()
    e.torch, e.ops = torch, ops
    e.nc = load_script('tests/test_gpu_norm_conditioning.py')
    e.case = case = load_script('tools/tensor_state_case.py')
    e.x = {k: case.contents(k).cuda() for k in 'AB'}
    e.P = {}
    for fam, code in FAMS:
        w, b = case.weight(64)
        e.P[fam] = ops.pack_weight(w.cuda(), b.cuda(), bf16=getattr(ops, code) if code else 0)
    e.pair = {c: [ops.pack_weight(*(t.cuda() for t in case.weight(c, seed=s))) for s in (21, 22)] for c in (32, 64)}   # code 0, two different weights
    w, b = case.weight(32, seed=9)
    e.P32 = ops.pack_weight(w.cuda(), b.cuda())
    w, b = case.weight(64, seed=13)
    code = ops.conv_code(ops.SPLIT, 64, 64, 16, 16)
    assert code == ops.WSPLIT
    e.C = ops.pack_weight(w.cuda(), b.cuda(), bf16=code)
    assert ops.needs_act_scale(e.C)
    e.affine = {c: case.affine(c) for c in (64, 128)}
    e.affine_d = {c: tuple(torch.from_numpy(v).float().cuda() for v in ab) for c, ab in e.affine.items()}
    t0 = time.time()
    yield e
    torch.cuda.synchronize()
    print(f'\n  tests/test_gpu_tensor_state.py: {time.time() - t0:.1f} s after the fixture')
    for fam, r in e.nc.RATIOS.items():
        print(f'  largest table error / first-order bound (FACTOR = {e.nc.FACTOR} allowed) | {fam:40s} {r:.3g}')


def _mode(env, mode):
    return env.torch.inference_mode() if mode == 'inference' else contextlib.nullcontext()


def _produce(env, fam, which, out=None, emit_stats=True):
    y = env.ops.conv2d(env.x[which], env.P[fam], emit_stats=emit_stats, out=out)
    assert out is None or y is out
    return y


def _tables(env, xs, act_growth=None):
    g, b = env.affine_d[sum(t.shape[3] for t in xs)]
    return env.ops.groupnorm_tables(xs, g, b, act_growth=act_growth)


def _consume(env, t, act):
    return env.ops.conv2d(t, env.C, act=act)


def _check_i(env, label, xs, ts, ntk):
    """Reference (i): ops.groupnorm_tables(xs) against the fp64 tables of ts at the family's n_t, inside the envelope, within FACTOR."""
    ctot = sum(t.shape[3] for t in ts)
    env.nc._check_tables(label, 'tables', env.ops, xs, ts, *env.affine[ctot], env.nc.NT[ntk], True)


def _check_range(env, label, act, ts, lo):
    """s a power of two with s * (1 / s) == 1, and lo <= growth max|x_b| s_b < 2^14: lo = 2^7 for a table from partials (loose by < 2^6,
    tests/test_gpu_range.py::test_act_scale_kernels), 2^13 for one from the tensor itself."""
    amax = env.torch.cat(ts, dim=3).abs().amax(dim=(1, 2, 3)).numpy()
    a = act.double().cpu().numpy()
    for b in range(a.shape[0]):
        s, inv = a[b]
        m = GROWTH * amax[b] * s
        print(f'    {label} | image {b}: growth max|x| s = 2^{np.log2(m):.2f}')
        assert s * inv == 1.0 and np.frexp(s)[0] == 0.5, (label, b, s, inv)
        assert lo <= m < 2.0 ** 14, (label, b, m, s)


def _same_as(env, label, got, want, lo, ntk):
    """Everything a reader takes from `got` (a twice-written object) against `want` (a tensor that holds the same values and was written
    once or never carried state): values, tables, range scale, the range-scaled consumer -- (ii) bitwise -- and (i)."""
    torch, ops = env.torch, env.ops
    assert torch.equal(got, want), label
    t64 = got.double().cpu()
    _check_i(env, label, [got], [t64], ntk)
    sc, sh = _tables(env, [got])
    sc_w, sh_w = _tables(env, [want])
    assert torch.equal(sc, sc_w) and torch.equal(sh, sh_w), (label, 'tables differ from the fresh tensor\'s', float((sc - sc_w).abs().max()), float((sh - sh_w).abs().max()))
    act, act_w = ops.act_scale(got), ops.act_scale(want)
    _check_range(env, label, act, [t64], lo)
    assert torch.equal(act, act_w), (label, 'range scale differs from the fresh tensor\'s', act.tolist(), act_w.tolist())
    z, z_w = _consume(env, got, act), _consume(env, want, act_w)
    assert bool(torch.isfinite(z).all()), (label, 'the range-scaled consumer overflowed')
    assert torch.equal(z, z_w), label


def _use(env, t):
    """What a forward does with a fresh activation: tables and the parked range-scale table, then the consumer -- the state that can go stale."""
    _tables(env, [t], act_growth=GROWTH)
    _consume(env, t, env.ops.act_scale(t))


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fam', [f for f, _ in FAMS])
@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('mode', MODES)
def test_out_reuse_with_statistics(env, mode, order, fam):
    """conv2d(out=buf, emit_stats=True) into a buffer that carries partials and a parked table of other contents."""
    with _mode(env, mode):
        buf = _produce(env, fam, order[0])
        _use(env, buf)
        _produce(env, fam, order[1], out=buf)
        left = [n for n in STATE if getattr(buf, n, None) is not None]
        _same_as(env, f'test 1 | {mode} {order} {fam}', buf, _produce(env, fam, order[1]), 2.0 ** 7, fam)
        assert left == ['_cf_stats'], left          # the new launch's partials, and nothing of the old contents


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fam', [f for f, _ in FAMS])
@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('mode', MODES)
def test_out_reuse_without_statistics(env, mode, order, fam):
    """The second launch emits no partials: the buffer must not keep the first launch's."""
    with _mode(env, mode):
        buf = _produce(env, fam, order[0])
        _use(env, buf)
        _produce(env, fam, order[1], out=buf, emit_stats=False)
        left = [n for n in STATE if getattr(buf, n, None) is not None]
        _same_as(env, f'test 2 | {mode} {order} {fam}', buf, buf.clone(), 2.0 ** 13, 'standalone')
        assert left == [], left


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fam', [f for f, _ in FAMS])
@pytest.mark.parametrize('mode', MODES)
def test_writing_through_a_view(env, mode, fam):
    """out=y[..., :32]: the slice is a new object, the state sits on y."""
    ops = env.ops
    with _mode(env, mode):
        y = _produce(env, fam, 'A')
        _use(env, y)
        assert getattr(y, '_cf_stats', None) is not None and getattr(y, '_cf_act', None) is not None
        ops.conv2d(env.x['B'], env.P32, out=y[..., :32])
        left = [n for n in STATE if getattr(y, n, None) is not None]
        assert float(y[..., :32].abs().max()) > 2.0 ** 20 > 2.0 ** 10 > float(y[..., 32:].abs().max())       # half B, half A
        _same_as(env, f'test 3 | {mode} {fam}', y, y.clone(), 2.0 ** 13, 'standalone')
        if mode == 'normal':      # PyTorch records the base: the attributes themselves were dropped
            assert left == [], left
        else:                     # no `._base` on an inference tensor: what is left on y is dead
            assert '_cf_stats' not in left or y._cf_stats.stamp != ops.tensor_stamp(y)
            assert '_cf_act' not in left or y._cf_act[0][2] != ops.tensor_stamp(y)[1]


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rewritten', ('b', 'a'))
@pytest.mark.parametrize('channels', (32, 64))
@pytest.mark.parametrize('mode', MODES)
def test_pair_table_after_one_member_is_rewritten(env, mode, channels, rewritten):
    """groupnorm_tables([a, b], act_growth=4.0), then out= into one member: act_scale(a, b) describes what the two hold now."""
    torch, ops = env.torch, env.ops
    pa, pb = env.pair[channels]
    label = f'test 4 | {mode} {channels} {rewritten}'
    with _mode(env, mode):
        a, b = ops.conv2d(env.x['A'], pa, emit_stats=True), ops.conv2d(env.x['A'], pb, emit_stats=True)
        _tables(env, [a, b], act_growth=GROWTH)
        first = ops.act_scale(a, b)
        if channels == 64:       # (one channel per group at 32: no partials, no parked pair -- the single tables are cached instead)
            parked = getattr(a, '_cf_act_pair', None)
            assert parked is not None and first is parked[3]
        wa, wb = ('B', 'A') if rewritten == 'a' else ('A', 'B')
        if rewritten == 'a':
            ops.conv2d(env.x['B'], pa, emit_stats=True, out=a)
        else:
            ops.conv2d(env.x['B'], pb, emit_stats=True, out=b)
        fa, fb = ops.conv2d(env.x[wa], pa, emit_stats=True), ops.conv2d(env.x[wb], pb, emit_stats=True)
        assert torch.equal(a, fa) and torch.equal(b, fb)
        act, act_f = ops.act_scale(a, b), ops.act_scale(fa, fb)
        ts = [a.double().cpu(), b.double().cpu()]
        _check_range(env, label, act, ts, 2.0 ** 7 if channels == 64 else 2.0 ** 13)
        assert torch.equal(act, act_f), (label, act.tolist(), act_f.tolist())
        sc, sh = _tables(env, [a, b])
        sc_f, sh_f = _tables(env, [fa, fb])
        assert torch.equal(sc, sc_f) and torch.equal(sh, sh_f), label
        _check_i(env, label, [a, b], ts, 'direct' if channels == 64 else 'standalone')
        sc2, sh2 = _tables(env, [a, b], act_growth=GROWTH)       # parked again, from what the members hold now
        assert torch.equal(sc2, sc) and torch.equal(sh2, sh) and torch.equal(ops.act_scale(a, b), act_f), label


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fam', [f for f, _ in FAMS])
@pytest.mark.parametrize('write', ('mul_', 'copy_'))
def test_user_in_place_writes_retire_the_state(env, write, fam):
    """Normal mode only (inference tensors keep no version counter): y.mul_ / y.copy_ on a tensor with partials and a parked table."""
    y = _produce(env, fam, 'A')
    _use(env, y)
    assert getattr(y, '_cf_stats', None) is not None and getattr(y, '_cf_act', None) is not None
    if write == 'mul_':
        y.mul_(2.0 ** 21)
    else:
        y.copy_(_produce(env, fam, 'B'))
    _same_as(env, f'test 5 | {write} {fam}', y, y.clone(), 2.0 ** 13, 'standalone')
    assert y._cf_stats.stamp != env.ops.tensor_stamp(y)         # (still on the object, and known to be of the old contents)


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fam', [f for f, _ in FAMS])
@pytest.mark.parametrize('mode', MODES)
def test_copies_outlive_their_source(env, mode, fam):
    """to_bf16 / select_rows copies describe the values at copy time, whatever happens to the source afterwards."""
    torch, ops = env.torch, env.ops
    label = f'test 6 | {mode} {fam}'
    sel = torch.tensor([1, 1, 0], device='cuda')
    with _mode(env, mode):
        y = _produce(env, fam, 'A')
        _tables(env, [y], act_growth=GROWTH)
        before = y.double().cpu()
        act_before = ops.act_scale(y).clone()
        yb, ys = ops.to_bf16(y), ops.select_rows(y, sel)
        assert getattr(ys, '_cf_act', None) is None and getattr(ys, '_cf_act_pair', None) is None
        _produce(env, fam, 'B', out=y)
        torch.cuda.synchronize()
        assert float(y.abs().max()) > 2.0 ** 20
        assert yb.dtype == torch.bfloat16 and torch.equal(yb.cpu(), before.float().to(torch.bfloat16)) and torch.equal(ys.double().cpu(), before[sel.cpu()])
        # the partials of a bf16 copy describe the fp32 values it was rounded from (tests/test_gpu_norm_conditioning.py, bf16 storage)
        _check_i(env, label + ' to_bf16', [yb], [before], fam)
        _check_i(env, label + ' select_rows', [ys], [before[sel.cpu()]], fam)
        a_b, a_s = ops.act_scale(yb), ops.act_scale(ys)
        _check_range(env, label + ' to_bf16', a_b, [before], 2.0 ** 7)
        _check_range(env, label + ' select_rows', a_s, [before[sel.cpu()]], 2.0 ** 7)
        assert torch.equal(a_b, act_before) and torch.equal(a_s, act_before[sel]), label


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
def test_a_refused_call_leaves_the_state_alone(env, mode):
    """State goes only once conv2d's own checks have passed."""
    torch, ops = env.torch, env.ops
    with _mode(env, mode):
        y = _produce(env, 'f23', 'A')
        sc, sh = _tables(env, [y], act_growth=GROWTH)
        y._cf_act_pair = ('a pair entry',)
        held = {n: getattr(y, n) for n in STATE}
        key = ops._act_key(y, GROWTH)
        with pytest.raises(ValueError, match='out: expected'):
            ops.conv2d(env.x['B'][:1], env.P['f23'], out=y, emit_stats=True)               # batch 1 into a batch-2 destination
        with pytest.raises(ValueError, match='epilogue operand shape'):
            ops.conv2d(env.x['B'], env.P['f23'], out=y, epilogue=ops.EPI_RESIDUAL, res=env.x['B'][:1])
        with pytest.raises(ValueError, match='input channels'):
            ops.conv2d(env.x['B'][..., :32], env.P['f23'], out=y)
        assert all(getattr(y, n, None) is held[n] for n in STATE)
        assert ops._act_key(y, GROWTH) == key and ops.act_scale(y) is held['_cf_act'][1]          # ... and still answers
        sc2, sh2 = _tables(env, [y])
        assert torch.equal(sc, sc2) and torch.equal(sh, sh2)


# ---- 8 ---------------------------------------------------------------------------------------------------------------------------------------
def test_scratch_growth_under_a_captured_graph(env):
    """A captured graph holds the raw address of the range-scale cells and split-K counters of its stream: growing either must not free them.
    The liveness of the old tensors is asserted on the host BEFORE the graph is replayed again -- a graph whose scratch was freed is never replayed."""
    torch, ops = env.torch, env.ops
    dev = env.x['A'].device
    g0 = torch.Generator().manual_seed(3)
    x256 = torch.randn(1, 16, 16, 256, generator=g0).cuda()
    w, b = env.case.weight(64, cin=256, seed=17)
    pw = ops.pack_weight(w.cuda(), b.cuda(), bf16=ops.WINOGRAD)
    assert ops.splitk_for(pw, 16, 16, 256, 1) >= 2                 # the launch takes workspace and counters
    xs = env.x['B'][:1].clone()
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        cells, counters = ops._act_cells(dev, 2), ops._counters(dev, 1)     # outside the capture, as the network's graphed forward does
        for _ in range(2):                                                 # warm-up: kernel attributes, the allocator
            ops.act_scale(xs.clone())
            ops.conv2d(x256, pw)
    s.synchronize()
    graph = torch.cuda.CUDAGraph()
    gc_on = gc.isenabled()
    gc.disable()                                                           # (no collection while capturing, as the network's capture)
    try:
        with torch.cuda.graph(graph, stream=s):
            assert ops._act_cells(dev, 2) is cells and ops._counters(dev, 1) is counters
            act = ops.act_scale(xs)
            y = ops.conv2d(x256, pw)
    finally:
        if gc_on:
            gc.enable()
    graph.replay()
    torch.cuda.synchronize()
    act1, y1 = act.clone(), y.clone()
    assert torch.equal(y1, ops.conv2d(x256, pw)) and torch.equal(act1, ops.act_scale(xs.clone()))      # the graph ran both launches: bitwise the eager ones
    _check_range(env, 'test 8', act1, [xs.double().cpu()], 2.0 ** 13)
    refs = weakref.ref(cells), weakref.ref(counters)
    with torch.cuda.stream(s):
        grown = ops._act_cells(dev, 1 << 16), ops._counters(dev, 1 << 20)
    assert grown[0] is not cells and grown[1] is not counters and grown[0].numel() >= 2 << 16 and grown[1].numel() >= 1 << 20
    addr = cells.data_ptr(), counters.data_ptr()
    del cells, counters
    gc.collect()
    old = refs[0](), refs[1]()
    assert old[0] is not None and old[1] is not None, 'scratch that a captured graph addresses was freed: the graph is not replayed'
    assert (old[0].data_ptr(), old[1].data_ptr()) == addr
    act.zero_()
    y.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(act, act1) and torch.equal(y, y1)
    assert not old[0].any() and not old[1].any() and not grown[0].any() and not grown[1].any()
