"""-m gpu: the logit guard (CodeFormer.logit_guard) on an MI355X -- cf_argmax_rows_gap against torch.topk bit for bit, and the guard's
contract on whole forwards: every unflagged face is bitwise the face a guard-off network returns, every flagged face bitwise the face a
winograd_f43_encoder=False network returns (the forward is bitwise batch-invariant), in every precision mode, eagerly and under graph
replay.  Assertions on which golden face is flagged use only faces more than ten times the 1e-5 logit error away from the threshold:
real_0342 (reference minimum gap 5.5e-6: flagged) and the seeded face 0 (1.37e-3: not flagged)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from _tools import load_script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
pytestmark = pytest.mark.gpu
DEFAULT_GAP = 1.1e-4


@pytest.fixture(scope='module')
def chk():
    import torch
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    from codeformer_amd import lib
    lib.load()
    return load_script('tools/gpu_check.py')


@pytest.fixture(scope='module')
def nets(chk):
    """(network under test, the same seed-0 weights with the encoder on F(2x2,3x3))."""
    net, f23 = chk.build_net().cuda(), chk.build_net().cuda()
    assert net.winograd_f43_encoder is True and net.logit_guard == 'off' and net.logit_guard_gap == DEFAULT_GAP
    f23.winograd_f43_encoder = False
    return net, f23


@pytest.fixture(scope='module')
def faces16():
    """Face 0: the seeded face of restoration_seed0_face0.npz; face 1: the reference's crop 0342; faces 2..15: seeded noise."""
    import torch
    from codeformer_amd import ops
    from oracle.synth import seeded_input
    x = seeded_input(16).cuda()
    img = np.load(os.path.join(GOLD, 'real_0342.npz'))['img']
    x[1] = ops.img_u8_to_tensor(torch.from_numpy(img).unsqueeze(0).cuda())[0]
    return x


def _run(net, x, mode='off', gap=DEFAULT_GAP, graphs=None, code_only=False, w=0.5):
    """One forward under the given guard mode; every result as a fresh tensor, and the network left at its defaults."""
    import torch
    keep = (net.logit_guard, net.logit_guard_gap, net.use_hip_graphs)
    net.logit_guard, net.logit_guard_gap = mode, gap
    if graphs is not None:
        net.use_hip_graphs = graphs
    try:
        net.reset_guard_stats()
        if hasattr(net, 'last_min_gap'):
            del net.last_min_gap
        outs = net(x, w=w, adain=True, code_only=code_only)
        torch.cuda.synchronize()
        r = dict(zip(('logits', 'lq_feat') if code_only else ('out', 'logits', 'lq_feat'), outs))
        if not code_only or mode != 'off':
            r['idx'] = net.last_indices
        if mode != 'off':
            r['gap'] = net.last_min_gap
        else:
            assert not hasattr(net, 'last_min_gap')
        r['stats'] = net.guard_stats
        return r
    finally:
        net.logit_guard, net.logit_guard_gap, net.use_hip_graphs = keep


def _flags(gmin, thr=DEFAULT_GAP):
    return ~(gmin >= thr)


def _assert_mix(got, off, f23, flag, keys):
    """Rows of `got`: bitwise f23's where flagged, bitwise off's elsewhere."""
    import torch
    for k in keys:
        assert torch.equal(got[k][flag], f23[k][flag]), f'{k}: a flagged face is not the F(2,3) network\'s'
        assert torch.equal(got[k][~flag], off[k][~flag]), f'{k}: an unflagged face is not the guard-off network\'s'


# ---------------------------------------------------------------------------------------------------- 1. kernel
def _logit_cases():
    import torch
    g = torch.Generator().manual_seed(11)
    cases = []
    for rows, n, per in ((6, 512, 3), (10, 1024, 5), (512, 1024, 256), (7, 512, 7), (1, 1024, 1)):
        x = torch.randn(rows, n, generator=g)
        cases.append((f'random {rows}x{n}', x, per))
    x = torch.randn(12, 1024, generator=g)
    x[0, 5] = x[0, 900] = x[0].max() + 1                 # the maximum duplicated: gap exactly 0, lowest index wins
    x[1, :] = 0.25                                       # a whole row of ties
    x[2, 1023] = x[2, 0] = x[2, 511] = 9.0               # three-way tie across lanes
    x[3] = -x[3].abs() - 1                               # all negative
    x[4] = -x[4].abs() - 1
    x[4, 17] = x[4, 18] = -0.5                           # all negative with a tie inside one 16-byte load
    x[5, ::2] = float('-inf')                            # rows holding -inf
    x[6, :] = float('-inf')
    x[6, 1000], x[6, 3] = -3.0, -7.0                     # two finite values only
    x[7, 1:] = float('-inf')                             # one finite value: second is -inf, gap +inf
    x[8, 100] = x[8].max() + 1e-6                        # a near tie
    x[9] = torch.arange(1024, dtype=torch.float32)       # ascending: the winner is the last element of the last lane
    x[10] = -torch.arange(1024, dtype=torch.float32)
    cases.append(('crafted 12x1024', x, 4))
    cases.append(('crafted 12x1024, one group', x, 12))
    y = torch.randn(6, 512, generator=g).round()         # integers: many exact ties
    cases.append(('integer 6x512', y, 2))
    return cases


def test_kernel_against_topk_bitwise():
    import torch
    from codeformer_amd import ops
    for name, x, per in _logit_cases():
        xd = x.cuda()
        idx, gap, gmin = ops.argmax_rows_gap(xd, per)
        idx2, gap2, gmin2 = ops.argmax_rows_gap(xd, per)
        torch.cuda.synchronize()
        assert torch.equal(idx, ops.argmax_rows(xd)), name
        top = torch.topk(x, 2, dim=-1).values
        want = top[:, 0] - top[:, 1]
        assert torch.equal(gap.cpu().view(torch.int32), want.view(torch.int32)), (name, gap.cpu(), want)
        assert torch.equal(gmin.cpu().view(torch.int32), want.view(-1, per).min(dim=1).values.view(torch.int32)), name
        assert torch.equal(gmin.view(torch.int32), gap.view(-1, per).min(dim=1).values.view(torch.int32)), name
        assert torch.equal(idx, idx2) and torch.equal(gap.view(torch.int32), gap2.view(torch.int32)) and torch.equal(
            gmin.view(torch.int32), gmin2.view(torch.int32)), name
        assert idx.dtype == torch.int64 and gap.dtype == gmin.dtype == torch.float32 and gmin.shape == (x.shape[0] // per,)
        # lowest index on ties, against a plain statement of the rule
        assert torch.equal(idx.cpu(), torch.from_numpy(x.numpy().argmax(axis=1))), name


def test_kernel_nan_flags_its_group():
    """A NaN element makes its row's gap, and so its group's minimum, NaN: `not (min >= threshold)` flags it for every threshold."""
    import torch
    from codeformer_amd import ops
    x = torch.randn(8, 512, generator=torch.Generator().manual_seed(3))
    x[5, 77] = float('nan')
    idx, gap, gmin = ops.argmax_rows_gap(x.cuda(), 4)
    gap, gmin = gap.cpu(), gmin.cpu()
    assert torch.isnan(gap[5]) and not torch.isnan(gap[[0, 1, 2, 3, 4, 6, 7]]).any()
    assert not torch.isnan(gmin[0]) and torch.isnan(gmin[1])
    assert _flags(gmin, 0.0).tolist() == [False, True]
    with pytest.raises(ValueError):
        ops.argmax_rows_gap(x.cuda(), 3)


# ---------------------------------------------------------------------------------------------------- 2. off / report
def test_off_launches_the_plain_argmax_and_report_changes_no_result(nets, faces16, monkeypatch):
    import torch
    from codeformer_amd import lib
    from codeformer_amd.utils.diagnostics import top2_gap
    net, _ = nets
    native = lib.load()
    calls = {'cf_argmax_rows': 0, 'cf_argmax_rows_gap': 0}

    def counted(name):
        fn = getattr(native, name)

        def wrapper(*a):
            calls[name] += 1
            return fn(*a)
        return wrapper
    for name in calls:
        monkeypatch.setattr(native, name, counted(name))
    off = _run(net, faces16, 'off')                       # 16 faces: eager, so every call launches
    assert calls == {'cf_argmax_rows': 1, 'cf_argmax_rows_gap': 0}
    assert off['stats']['calls'] == 0
    rep = _run(net, faces16, 'report')
    assert calls == {'cf_argmax_rows': 1, 'cf_argmax_rows_gap': 1}
    for k in ('out', 'logits', 'lq_feat', 'idx'):
        assert torch.equal(rep[k], off[k]), k
    want = top2_gap(rep['logits'])[0].min(dim=1).values
    assert rep['gap'].shape == (16,) and rep['gap'].dtype == torch.float32 and torch.equal(rep['gap'], want)
    st = rep['stats']
    assert (st['calls'], st['faces'], st['rerun_faces'], st['index_changes']) == (1, 16, 0, 0)
    assert st['flagged'] == int(_flags(want).sum()) and st['min_gap'] == float(want.min())
    # code_only: the launch runs as well, so the gap is there without the generator
    rc = _run(net, faces16, 'report', code_only=True)
    assert calls == {'cf_argmax_rows': 1, 'cf_argmax_rows_gap': 2}
    assert torch.equal(rc['logits'], off['logits']) and torch.equal(rc['gap'], want) and torch.equal(rc['idx'], off['idx'])
    _run(net, faces16, 'off', code_only=True)
    assert calls == {'cf_argmax_rows': 1, 'cf_argmax_rows_gap': 2}       # as today: no argmax at all


# ---------------------------------------------------------------------------------------------------- 3. goldens
@pytest.mark.parametrize('precision', ['f16x2', 'fp32', 'bf16'])
def test_rerun_on_the_goldens(nets, faces16, precision):
    import torch
    net, f23 = nets
    net.precision = f23.precision = precision
    try:
        off = _run(net, faces16, 'off')
        rep = _run(net, faces16, 'report')
        ref = _run(f23, faces16, 'report')
        flag = _flags(rep['gap'])
        print(f'[{precision}] min gaps {rep["gap"].tolist()}  flagged {flag.nonzero().flatten().tolist()}')
        assert bool(flag[1]) and not bool(flag[0])        # crop 0342 / the seeded face (see the module docstring)
        got = _run(net, faces16, 'rerun')
        _assert_mix(got, off, ref, flag, ('out', 'logits', 'lq_feat', 'idx'))
        assert torch.equal(got['gap'][flag], ref['gap'][flag]) and torch.equal(got['gap'][~flag], rep['gap'][~flag])
        n = int(flag.sum())
        st = got['stats']
        assert (st['calls'], st['faces'], st['flagged'], st['rerun_faces']) == (1, 16, n, n)
        assert st['index_changes'] == int((off['idx'][flag] != ref['idx'][flag]).sum())
        assert st['min_gap'] == float(rep['gap'].min())
        print(f'[{precision}] flagged {n} of 16, index changes {st["index_changes"]}')
        if precision == 'f16x2':
            gc = _run(net, faces16, 'rerun', code_only=True)
            _assert_mix(gc, off, ref, flag, ('logits', 'lq_feat', 'idx'))
            assert 'out' not in gc and gc['stats']['rerun_faces'] == n
            assert torch.equal(gc['gap'][flag], ref['gap'][flag]) and torch.equal(gc['gap'][~flag], rep['gap'][~flag])
            # threshold 0: nothing finite is flagged, nothing is run again
            g0 = _run(net, faces16, 'rerun', gap=0.0)
            assert (g0['stats']['flagged'], g0['stats']['rerun_faces']) == (0, 0)
            for k in ('out', 'logits', 'lq_feat', 'idx'):
                assert torch.equal(g0[k], off[k]), k
    finally:
        net.precision = f23.precision = 'f16x2'


# ---------------------------------------------------------------------------------------------------- 4. a certain tie
def test_crafted_tie_flags_every_face(chk, faces16):
    """Two identical, dominant rows of the logits head (it has no bias): some token of every face is led by the pair, whose two logits
    are the same number -- minimum gap exactly 0.0 on every face, whatever the weights are."""
    import torch

    def tied(f43):
        n = chk.build_net()
        with torch.no_grad():
            W = n.idx_pred_layer[1].weight
            W[700] = W[3]
            W[3] *= 1024.0
            W[700] *= 1024.0
        n = n.cuda()
        n.winograd_f43_encoder = f43
        return n
    net, f23 = tied(True), tied(False)
    for x in (faces16[1:2], faces16):                     # one face per call: graph replay; sixteen: eager
        assert net.use_hip_graphs == 'auto'
        ref = _run(f23, x, 'off')
        for rep in range(2 if x.shape[0] == 1 else 1):    # (the second one-face call replays the captured graph)
            got = _run(net, x, 'rerun')
            assert got['gap'].tolist() == [0.0] * x.shape[0]
            for k in ('out', 'logits', 'lq_feat', 'idx'):
                assert torch.equal(got[k], ref[k]), (k, x.shape[0], rep)
            st = got['stats']
            assert (st['flagged'], st['rerun_faces'], st['min_gap']) == (x.shape[0], x.shape[0], 0.0)
        off = _run(net, x, 'off')
        g0 = _run(net, x, 'rerun', gap=0.0)               # 0.0 >= 0.0: not flagged
        assert (g0['stats']['flagged'], g0['stats']['rerun_faces']) == (0, 0)
        for k in ('out', 'logits', 'lq_feat', 'idx'):
            assert torch.equal(g0[k], off[k]), k


# ---------------------------------------------------------------------------------------------------- 5. graphs
@pytest.mark.parametrize('B', [1, 2, 4])
def test_graph_replay(nets, faces16, B):
    import torch
    net, f23 = nets
    assert net.use_hip_graphs == 'auto' and B <= net.graph_max_batch
    x = faces16[1:1 + B]                                  # face 0 of the slice is crop 0342: the second pass is triggered
    eager = {m: _run(net, x, m, graphs=False) for m in ('report', 'rerun')}
    assert eager['rerun']['stats']['rerun_faces'] >= 1
    net._graphs.clear()
    for m in ('report', 'rerun'):
        for _ in range(2):                                # capture, then replay
            got = _run(net, x, m)
            for k in ('out', 'logits', 'lq_feat', 'idx', 'gap'):
                assert torch.equal(got[k], eager[m][k]), (m, k)
            assert got['stats'] == eager[m]['stats']
    assert len(net._graphs) == 1                          # 'report' and 'rerun' capture the same launches
    before = [(k, id(e['graph'])) for k, e in net._graphs.items()]
    got = _run(net, x, 'rerun')
    assert got['stats']['rerun_faces'] >= 1
    assert [(k, id(e['graph'])) for k, e in net._graphs.items()] == before
    _run(net, x, 'off')
    assert len(net._graphs) == 2                          # the guard mode is part of the key
    # an earlier call's last_min_gap belongs to the caller: a later replay does not overwrite it
    first = _run(net, x, 'report')['gap']
    kept = first.clone()
    second = _run(net, faces16[8:8 + B], 'report')['gap']
    assert torch.equal(first, kept) and not torch.equal(first, second)


# ---------------------------------------------------------------------------------------------------- 6. nothing to fall back to
def test_rerun_without_f43_encoder_counts_only(nets, faces16):
    import torch
    _, f23 = nets
    off = _run(f23, faces16, 'off')
    got = _run(f23, faces16, 'rerun')
    st = got['stats']
    assert st['flagged'] >= 1 and st['flagged'] == int(_flags(got['gap']).sum()) and st['rerun_faces'] == 0 and st['index_changes'] == 0
    for k in ('out', 'logits', 'lq_feat', 'idx'):
        assert torch.equal(got[k], off[k]), k


# ---------------------------------------------------------------------------------------------------- 7. entry point
def test_entry_point_rerun(nets, tmp_path):
    import torch
    from PIL import Image
    from codeformer_amd import ops
    net, _ = nets
    src = tmp_path / 'crops'
    os.makedirs(src)
    rng = np.random.default_rng(7)
    imgs = {'a_0342': np.load(os.path.join(GOLD, 'real_0342.npz'))['img'],
            'b_0143': np.load(os.path.join(GOLD, 'real_0143.npz'))['img'],
            'c_noise': rng.integers(0, 256, (512, 512, 3), dtype=np.uint8)}
    for name, img in imgs.items():
        Image.fromarray(np.ascontiguousarray(img[:, :, ::-1])).save(src / f'{name}.png')
    names = sorted(imgs)
    x = ops.img_u8_to_tensor(torch.from_numpy(np.stack([imgs[n] for n in names])).cuda())
    flag = _flags(_run(net, x, 'report', code_only=True)['gap']).tolist()      # seed-0 weights: what --random_init_seed 0 builds
    assert flag[0]                                        # crop 0342

    def run(tag, extra, env=None):
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'inference_codeformer.py'), '--has_aligned', '-i', str(src), '-o',
                            str(tmp_path / tag), '--device', 'cuda', '--random_init_seed', '0'] + extra, capture_output=True, text=True,
                           timeout=900, cwd=str(tmp_path), env=dict(os.environ, **(env or {})))
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout, {n: open(tmp_path / tag / 'restored_faces' / f'{n}.png', 'rb').read() for n in names}
    out_d, png_d = run('default', [])
    out_g, png_g = run('guard', ['--logit_guard', 'rerun'])
    out_f, png_f = run('f23', [], {'CODEFORMER_HIP_F43_ENCODER': '0'})
    assert 'logit guard' not in out_d and 'logit guard' not in out_f      # auto: off for seeded random weights
    m = re.search(r'logit guard \(rerun, gap < 0.00011\): (\d+) faces, (\d+) flagged, (\d+) re-run, (\d+) indices changed, smallest gap (\S+)',
                  out_g)
    assert m, out_g
    assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (3, sum(flag), sum(flag))
    for n, f in zip(names, flag):
        assert png_g[n] == (png_f[n] if f else png_d[n]), (n, f)
