"""CPU only, no library: what tests/test_gpu_tensor_state.py relies on, shown on the fp64 model of its two contents and on the pure-Python
pieces of ops.py that keep the state on tensor objects honest.

  * A stale table cannot pass by accident: on the fp64 model of contents A and B (tools/tensor_state_case.py) every element of the scale
    table of one differs from the other's by at least 100 x the bound the GPU test asserts (FACTOR x the first-order bound at the largest
    n_t it uses), in both orders, and so does the largest element of the shift table; the range scale of one puts 4 max|x| of the other
    outside [2^7, 2^14) for every scale the statistics route may return (the tight one down to 2^-7 of it).
  * The stamp (version counter, library write count) moves when it must; state is dropped from an object and from its `._base`; copies
    carry state of their own; replaced scratch tensors stay referenced.
"""
import gc
import types
import weakref

import numpy as np
import pytest
import torch

from _tools import load_script


@pytest.fixture(scope='module')
def nc():
    return load_script('tests/test_gpu_norm_conditioning.py')


@pytest.fixture(scope='module')
def case():
    return load_script('tools/tensor_state_case.py')


@pytest.fixture()
def ops(monkeypatch):
    from codeformer_amd import ops as o
    monkeypatch.setattr(o, '_WRITE_EPOCH', {})
    monkeypatch.setattr(o, '_RETIRED_SCRATCH', [])
    return o


@pytest.fixture(scope='module')
def written(case):
    """fp64 model of the buffer's two contents: the 64 -> 64 producer on inputs A and B."""
    w, b = case.weight(64)
    return {k: case.model(case.contents(k), w, b) for k in 'AB'}


def test_stale_tables_miss_the_bound_by_two_orders_of_magnitude(nc, case, written):
    gamma, beta = case.affine(64)
    nt = max(nc.NT['direct'], nc.NT['f23'], nc.NT['standalone'])     # the widest bound the GPU test uses
    ref = {k: case.reference_tables(nc, [written[k]], gamma, beta, nt) for k in 'AB'}
    for fresh, stale in (('A', 'B'), ('B', 'A')):
        sc, sh, b_sc, b_sh, r = ref[fresh]
        assert float(r.max()) <= nc.ENVELOPE
        d_sc, d_sh = np.abs(ref[stale][0] - sc), np.abs(ref[stale][1] - sh)
        assert (d_sc >= 100 * nc.FACTOR * b_sc).all(), (fresh, float((d_sc / b_sc).min()))
        assert float((d_sh / b_sh).max()) >= 100 * nc.FACTOR, (fresh, float((d_sh / b_sh).max()))


def test_a_stale_range_scale_leaves_the_operand_range(case, written):
    amax = {k: written[k].abs().amax(dim=(1, 2, 3)).numpy() for k in 'AB'}
    for fresh, stale in (('A', 'B'), ('B', 'A')):
        for b in range(case.B):
            tight = case.tight_scale(4.0 * amax[stale][b])
            for s in (tight, tight / 2.0 ** 7):                      # every scale act_scale may have returned for the stale contents
                assert 2.0 ** 13 / 2.0 ** 7 <= 4.0 * amax[stale][b] * s < 2.0 ** 14       # ... is in range for them
                m = 4.0 * amax[fresh][b] * s
                assert not (2.0 ** 7 <= m < 2.0 ** 14), (fresh, b, m)
    assert (amax['B'] > amax['A'] * 2.0 ** 18).all()


def test_contents_b_is_contents_of_another_scale_and_offset(case):
    a, b = case.contents('A'), case.contents('B')
    assert a.shape == b.shape == (2, 16, 16, 64) and case.BIG == 2.0 ** 21
    assert float(a.abs().max()) < 8.0 and float(b.abs().min()) >= 0.0 and float(b.abs().max()) > 2.0 ** 22
    assert float((b.mean(dim=(0, 1, 2)).abs() / case.BIG - 1.0).abs().max()) < 0.2      # the per-channel bias of magnitude 2^21


def test_stamp_records_version_and_library_writes(ops):
    y = torch.zeros(2, 4, 4, 8)
    s0 = ops.tensor_stamp(y)
    assert s0 == (y._version, 0)
    y.mul_(2.0)
    assert ops.tensor_stamp(y) == (s0[0] + 1, 0)
    v = y[..., :4]
    ops._drop_state(v)                     # a library write through a slice
    assert ops.tensor_stamp(y)[1] == 1 and ops.tensor_stamp(v)[1] == 1 and ops.tensor_stamp(y[1:])[1] == 1
    assert ops.tensor_stamp(torch.zeros(3))[1] == 0
    with torch.inference_mode():
        z = torch.zeros(2, 4, 4, 8)
        assert ops.tensor_version(z) is None and ops.tensor_stamp(z) == (None, 0)
        assert z[..., :4]._base is None                # why the write count exists: the buffer behind a slice cannot be found here
        ops._drop_state(z[..., :4])
        assert ops.tensor_stamp(z) == (None, 1)


def test_statistics_are_ignored_once_the_stamp_moved(ops):
    y = torch.zeros(2, 4, 4, 64)
    part = torch.zeros(2 * 32 * 2, dtype=torch.float64)
    y._cf_stats = ops.GNStats(part, 1, 2, ops.tensor_stamp(y))
    assert y._cf_stats.stamp == (y._version, 0) and ops.live_stats(y) is y._cf_stats
    y.mul_(2.0)
    assert ops.live_stats(y) is None and y._cf_stats is not None
    y._cf_stats = ops.GNStats(part, 1, 2, ops.tensor_stamp(y))
    assert ops.live_stats(y) is not None
    ops._WRITE_EPOCH[y.untyped_storage().data_ptr()] = 5          # a library write the object did not see (through another alias)
    assert ops.live_stats(y) is None
    y._cf_stats = types.SimpleNamespace(part=part, parts=1, cpg=2)    # attached by hand, no stamp: trusted
    assert ops.live_stats(y) is y._cf_stats
    assert ops.live_stats(torch.zeros(1)) is None


def test_act_key(ops):
    y = torch.zeros(2, 4, 4, 64)
    k = ops._act_key(y, 4)
    assert k == (4.0, y._version, 0) and isinstance(k[0], float)
    assert ops._act_key(y, 2.0) != k
    y.add_(1.0)
    assert ops._act_key(y, 4.0) == (4.0, k[1] + 1, 0)
    ops._drop_state(y)
    assert ops._act_key(y, 4.0) == (4.0, k[1] + 1, 1)
    with torch.inference_mode():
        z = torch.zeros(2, 4, 4, 64)
        assert ops._act_key(z, 4.0) is None                  # nothing shows a write to z: nothing is cached for it
        z._cf_stats = ops.GNStats(None, 1, 2, ops.tensor_stamp(z))
        assert ops._act_key(z, 4.0) == (4.0, 'inference', 0)
        ops._drop_state(z[..., :32])
        assert ops._act_key(z, 4.0) is None                  # the statistics died with the write, and the key with them
        z._cf_stats = ops.GNStats(None, 1, 2, ops.tensor_stamp(z))
        assert ops._act_key(z, 4.0) == (4.0, 'inference', 1)


def test_parked_tables_are_found_only_while_both_members_are_unwritten(ops, monkeypatch):
    def miss():
        raise LookupError('act_scale found no valid table and went on to launch')
    monkeypatch.setattr(ops.L, 'load', miss)
    a, b = torch.zeros(2, 4, 4, 64), torch.zeros(2, 4, 4, 64)
    table, single = torch.ones(2, 2), torch.full((2, 2), 2.0)
    ops._park_act([a, b], 4.0, table)
    ops._park_act([a], 4.0, single)
    assert ops.act_scale(a, b) is table and ops.act_scale(a) is single and ops.act_scale(a, growth=4) is single
    assert a._cf_act_pair[2]() is b
    b.mul_(2.0)                            # the SECOND member written: the entry on `a` no longer answers
    with pytest.raises(LookupError):
        ops.act_scale(a, b)
    ops._park_act([a, b], 4.0, table)
    assert ops.act_scale(a, b) is table
    ops._drop_state(b)
    assert getattr(a, '_cf_act_pair', None) is not None
    with pytest.raises(LookupError):
        ops.act_scale(a, b)
    assert ops.act_scale(a) is single
    ops._drop_state(a)
    assert all(getattr(a, n, None) is None for n in ops._STATE_ATTRS)


def test_drop_state_clears_the_object_and_its_base(ops):
    buf = torch.zeros(2, 4, 4, 8)
    other = torch.zeros(2, 4, 4, 8)
    for t in (buf, other):
        t._cf_stats, t._cf_act, t._cf_act_pair, t.mine = 'stats', 'act', 'pair', 'kept'
    view = buf[..., 2:6]
    assert view._base is buf and getattr(view, '_cf_stats', None) is None      # a slice is a new object and carries nothing
    view._cf_act = 'act of the view'
    ops._drop_state(view)
    assert all(getattr(buf, n, None) is None and getattr(view, n, None) is None for n in ops._STATE_ATTRS)
    assert buf.mine == 'kept' and other._cf_stats == 'stats' and other._cf_act == 'act' and other._cf_act_pair == 'pair'
    ops._drop_state(other)
    assert all(getattr(other, n, None) is None for n in ops._STATE_ATTRS) and other.mine == 'kept'
    ops._drop_state(torch.zeros(3))        # nothing to drop: no error
    assert ops._STATE_ATTRS == ('_cf_stats', '_cf_act', '_cf_act_pair')


def test_select_rows_copies_live_statistics_only(ops):
    y = torch.arange(3 * 4 * 4 * 64, dtype=torch.float32).view(3, 4, 4, 64)
    part = torch.arange(3 * 32 * 2 * 2, dtype=torch.float64)
    y._cf_stats = ops.GNStats(part, 2, 2, ops.tensor_stamp(y))
    y._cf_act = (ops._act_key(y, 4.0), 'table')
    sel = torch.tensor([1, 1, 0])
    ys = ops.select_rows(y, sel)
    assert torch.equal(ys, y[sel]) and getattr(ys, '_cf_act', None) is None
    assert torch.equal(ys._cf_stats.part, part.view(3, -1)[sel].reshape(-1)) and (ys._cf_stats.parts, ys._cf_stats.cpg) == (2, 2)
    assert ops.live_stats(ys) is ys._cf_stats
    y.mul_(3.0)                            # the source rewritten: the copy is untouched, a new selection carries nothing
    assert ops.live_stats(ys) is ys._cf_stats and torch.equal(ys._cf_stats.part, part.view(3, -1)[sel].reshape(-1))
    assert getattr(ops.select_rows(y, sel), '_cf_stats', None) is None


def test_replaced_scratch_tensors_stay_allocated(ops, monkeypatch):
    monkeypatch.setattr(torch.cuda, 'current_stream', lambda device=None: types.SimpleNamespace(cuda_stream=0))
    for fn, table, floor, per in ((ops._act_cells, '_ACT_CELLS', 256, 2), (ops._counters, '_COUNTERS', 4096, 1)):
        monkeypatch.setattr(ops, table, {})
        t0 = fn('cpu', 1)
        assert t0.dtype == torch.int32 and t0.numel() == floor and not t0.any()
        assert fn('cpu', floor // per) is t0                      # large enough: the same tensor
        ref, n_retired = weakref.ref(t0), len(ops._RETIRED_SCRATCH)
        t1 = fn('cpu', 4 * floor)
        assert t1 is not t0 and t1.numel() >= per * 4 * floor and getattr(ops, table)[('cpu', 0)] is t1
        del t0
        gc.collect()
        assert ref() is not None and any(t is ref() for t in ops._RETIRED_SCRATCH)
        assert len(ops._RETIRED_SCRATCH) >= n_retired + 1
