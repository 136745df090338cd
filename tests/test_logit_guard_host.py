"""Logit guard (CodeFormer.logit_guard), the parts that need no GPU: the gap rule restated in numpy against diagnostics.top2_gap on the
reference's logits, the C ABI declaration / binding of cf_argmax_rows_gap, the --logit_guard flag of the three entry points and the
function that resolves it, and the host path's `last_min_gap` / `guard_stats`."""
import os
import re

import numpy as np
import pytest
import torch

from _tools import load_script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
HEADER = os.path.join(ROOT, 'include', 'codeformer_hip.h')
DEFAULT_GAP = 1.1e-4

# smallest top-2 gap of the reference's own logits per golden face, as the issue that introduced the guard lists them
TABLE = {
    'real_0342': 5.5e-6, 'range_big_seed': 1.08e-4, 'real_Solvay_conference_1927_0018': 1.12e-4, 'real_0143': 1.13e-4,
    'restoration_seed0_b16_face1': 1.27e-4, 'real_masked_00105': 1.28e-4, 'range_heavy_seed': 1.81e-4, 'inpaint_seed0_face0': 9.0e-4,
    'range_heavy_real0143': 1.25e-3, 'restoration_seed0_face0': 1.37e-3,
}


def _gap_rule(logits):
    """The rule in numpy: the winner is the LOWEST index holding the maximum; `second` is the largest value at any other index;
    gap = best - second in one fp32 subtraction."""
    flat = logits.reshape(-1, logits.shape[-1]).astype(np.float32)
    idx = flat.argmax(axis=1)                           # (numpy returns the first occurrence)
    rest = flat.copy()
    rest[np.arange(flat.shape[0]), idx] = -np.inf
    gap = flat[np.arange(flat.shape[0]), idx] - rest.max(axis=1)
    return idx.reshape(logits.shape[:-1]), gap.astype(np.float32).reshape(logits.shape[:-1])


def _flagged(min_gap, thr):
    return not (min_gap >= thr)


@pytest.mark.parametrize('name', sorted(TABLE))
def test_gap_rule_agrees_with_top2_gap_on_the_goldens(name):
    from codeformer_amd.utils.diagnostics import top2_gap
    g = np.load(os.path.join(GOLD, name + '.npz'))
    idx, gap = _gap_rule(g['logits'])
    gaps, smallest = top2_gap(torch.from_numpy(g['logits']))
    assert np.array_equal(gaps.numpy().view(np.uint32), gap.view(np.uint32))          # bit for bit
    assert np.array_equal(idx, g['idx']) and smallest == float(gap.min())
    assert gap.min() == pytest.approx(TABLE[name], rel=0.01), (name, float(gap.min()))


def test_default_threshold_on_the_goldens():
    mins = {n: float(_gap_rule(np.load(os.path.join(GOLD, n + '.npz'))['logits'])[1].min()) for n in TABLE}
    assert _flagged(mins['real_0342'], DEFAULT_GAP) and not _flagged(mins['restoration_seed0_face0'], DEFAULT_GAP)
    assert not any(_flagged(m, 0.0) for m in mins.values())            # threshold 0 flags nothing finite
    assert _flagged(float('nan'), 0.0) and _flagged(float('nan'), DEFAULT_GAP)


def test_gap_rule_on_ties():
    row = np.array([[1.0, 3.0, 3.0, -np.inf], [-2.0, -5.0, -2.5, -np.inf], [0.0, 0.0, 0.0, 0.0]], dtype=np.float32)
    idx, gap = _gap_rule(row)
    assert idx.tolist() == [1, 0, 0] and gap.tolist() == [0.0, 0.5, 0.0]
    top = torch.topk(torch.from_numpy(row), 2, dim=-1).values
    assert torch.equal(top[:, 0] - top[:, 1], torch.from_numpy(gap))


def test_symbol_is_declared_and_bound():
    from codeformer_amd import lib
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    m = re.search(r'int\s+cf_argmax_rows_gap\s*\(([^)]*)\)', src)
    assert m, 'cf_argmax_rows_gap is not declared in include/codeformer_hip.h'
    params = [p.strip() for p in m.group(1).split(',')]
    assert len(params) == 8 and 'rows_per_group' in params[3] and 'group_min_gap' in params[6] and 'cf_stream_t' in params[7]
    res, args = lib.SIGNATURES['cf_argmax_rows_gap']
    assert len(args) == 8 and lib.ABI_VERSION == 22
    assert 'cf_argmax_rows' in lib.SIGNATURES                         # the plain argmax keeps its entry point (ParseNet, guard off)


def test_entry_point_validates_before_any_launch():
    from codeformer_amd import build as cf_build
    from codeformer_amd import lib
    cf_build.build()
    native = lib.load()
    assert native.cf_version() == 22
    assert native.cf_argmax_rows_gap(1, 256, 1024, 100, 1, 1, 1, None) == -1 and 'rows_per_group' in lib.last_error()
    assert native.cf_argmax_rows_gap(1, 256, 1022, 256, 1, 1, 1, None) == -1 and 'multiple of 4' in lib.last_error()
    assert native.cf_argmax_rows_gap(1, 256, 1024, 256, 1, 1, None, None) == -1


def _script(name):
    return load_script(name + '.py')


def test_flag_parses_in_inference_codeformer():
    m = _script('inference_codeformer')
    assert m.parse_args([]).logit_guard == 'auto'
    for v in ('off', 'report', 'rerun', 'auto'):
        assert m.parse_args(['--logit_guard', v]).logit_guard == v
    with pytest.raises(SystemExit):
        m.parse_args(['--logit_guard', 'maybe'])


@pytest.mark.parametrize('script', ['inference_inpainting', 'inference_colorization'])
def test_flag_parses_in_the_other_entry_points(script, monkeypatch):
    """These two parse inside main(): stop at build_codeformer and look at what it was handed."""
    from codeformer_amd import cli
    m = _script(script)
    seen = {}

    class Stop(Exception):
        pass

    def fake(*args, **kw):
        seen['args'], seen['kw'] = args, kw
        raise Stop
    monkeypatch.setattr(cli, 'build_codeformer', fake)
    for argv, want in (([], 'auto'), (['--logit_guard', 'rerun'], 'rerun'), (['--logit_guard', 'report'], 'report')):
        with pytest.raises(Stop):
            m.main(['-i', os.path.join(ROOT, 'tests'), '--device', 'cpu', '--random_init_seed', '0'] + argv)
        assert want in seen['args'] or want in seen['kw'].values()
    with pytest.raises(SystemExit):
        m.main(['--logit_guard', 'maybe'])


def test_resolving_function():
    from codeformer_amd import cli
    assert cli.resolve_logit_guard('auto', False) == 'off'            # seeded random weights: what the encoder gate was measured with
    assert cli.resolve_logit_guard('auto', True) == 'rerun'           # weights from a checkpoint file
    for v in ('off', 'report', 'rerun'):
        assert cli.resolve_logit_guard(v, False) == v and cli.resolve_logit_guard(v, True) == v
    with pytest.raises(ValueError):
        cli.resolve_logit_guard('maybe', True)


@pytest.fixture(scope='module')
def small_net():
    import codeformer_amd.archs  # noqa: F401
    from codeformer_amd.utils.registry import ARCH_REGISTRY
    torch.manual_seed(0)
    return ARCH_REGISTRY.get('CodeFormer')(dim_embd=64, codebook_size=32, n_head=2, n_layers=1, connect_list=['32']).eval()


def test_defaults(small_net, monkeypatch):
    from codeformer_amd.archs.codeformer_arch import CodeFormer
    assert small_net.logit_guard == 'off' and small_net.logit_guard_gap == DEFAULT_GAP
    assert small_net.guard_stats == {'calls': 0, 'faces': 0, 'flagged': 0, 'rerun_faces': 0, 'index_changes': 0, 'min_gap': float('inf')}
    monkeypatch.setenv('CODEFORMER_HIP_LOGIT_GUARD', 'report')
    monkeypatch.setenv('CODEFORMER_HIP_LOGIT_GUARD_GAP', '2.5e-3')
    n = CodeFormer(dim_embd=64, codebook_size=32, n_head=2, n_layers=1, connect_list=['32'])
    assert n.logit_guard == 'report' and n.logit_guard_gap == 2.5e-3


def test_bad_mode_raises(small_net):
    small_net.logit_guard = 'maybe'
    try:
        with pytest.raises(ValueError):
            small_net(torch.zeros(1, 3, 512, 512), w=0, code_only=True)
    finally:
        small_net.logit_guard = 'off'


def test_host_path_reports(small_net):
    from codeformer_amd.utils.diagnostics import top2_gap
    x = torch.rand(2, 3, 512, 512, generator=torch.Generator().manual_seed(5)) * 2 - 1
    net = small_net
    with torch.no_grad():
        ref_logits, ref_lq = net(x, w=0, code_only=True)
    assert not hasattr(net, 'last_min_gap') and net.guard_stats['calls'] == 0       # 'off' touches nothing
    want = top2_gap(ref_logits)[0].min(dim=1).values
    try:
        net.reset_guard_stats()
        net.logit_guard = 'report'
        net.logit_guard_gap = float(want.max())          # flags exactly the faces below the larger of the two minima
        with torch.no_grad():
            logits, lq = net(x, w=0, code_only=True)
        assert torch.equal(logits, ref_logits) and torch.equal(lq, ref_lq)
        assert net.last_min_gap.shape == (2,) and torch.equal(net.last_min_gap, want)
        st = net.guard_stats
        assert (st['calls'], st['faces'], st['rerun_faces'], st['index_changes']) == (1, 2, 0, 0)
        assert st['flagged'] == int((~(want >= net.logit_guard_gap)).sum()) and st['min_gap'] == float(want.min())
        net.logit_guard, net.logit_guard_gap = 'rerun', 0.0            # no second encoder on the host: counted, nothing run again
        with torch.no_grad():
            net(x[:1], w=0, code_only=True)
        st = net.guard_stats
        assert (st['calls'], st['faces'], st['rerun_faces']) == (2, 3, 0)
        net.reset_guard_stats()
        assert net.guard_stats['calls'] == 0 and net.guard_stats['min_gap'] == float('inf')
    finally:
        net.logit_guard, net.logit_guard_gap = 'off', DEFAULT_GAP
        net.reset_guard_stats()
