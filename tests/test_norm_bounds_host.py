"""CPU only: the error budget that tests/test_gpu_norm_conditioning.py asserts on the GPU, proved on the host.

For every row of that file's case table (its own `synth_written` stand-in for the tensor a convolution writes: the row's bias, residual and
outlier on a normal convolution part of sigma sqrt(2)) and every channels-per-group the network has:
  * a NumPy emulation of "n_t fp32 additions into one accumulator, then fp64" -- plain float32 accumulation, the group's values taken in
    three orders (as written, ascending and descending magnitude) and the worst of them kept, at n_t = the largest value of the NT table --
    stays within the first-order bounds on (sum, sumsq) for every row, and within FACTOR x the bounds on the scale / shift tables for every
    strict row;
  * the fp64 reference the GPU test compares with is itself stable: its mean and two-pass variance match a long double evaluation to 1e-12;
  * the rows whose bound on the relative rstd error stays inside ENVELOPE at the largest n_t are exactly the STRICT list, asserted
    literally: the GPU test cannot reclassify a row.
"""
import numpy as np
import pytest

from _tools import load_script


@pytest.fixture(scope='module')
def m():
    return load_script('tests/test_gpu_norm_conditioning.py')


NPIX = 1024
COUTS = (64, 128, 256, 512)     # cpg 2, 4, 8, 16


def _groups(v, cout):
    cpg = cout // 32
    return v.reshape(NPIX, 32, cpg).transpose(1, 0, 2).reshape(32, NPIX * cpg)


def _emulate(v32, nt):
    """(groups, n) float32 -> (sum, sumsq) as the epilogues form them: accumulators of nt consecutive values in fp32 (the square rounded to
    fp32 as well), the accumulators added in fp64."""
    G, n = v32.shape
    pad = (-n) % nt
    a = np.concatenate([v32, np.zeros((G, pad), np.float32)], axis=1).reshape(G, -1, nt)
    s = np.zeros(a.shape[:2], np.float32)
    q = np.zeros(a.shape[:2], np.float32)
    for k in range(nt):
        s = (s + a[..., k]).astype(np.float32)
        q = (q + (a[..., k] * a[..., k]).astype(np.float32)).astype(np.float32)
    return s.astype(np.float64).sum(1), q.astype(np.float64).sum(1)


def _orders(v32):
    mag = np.abs(v32)
    asc = np.take_along_axis(v32, np.argsort(mag, axis=1), axis=1)
    return (v32, asc, asc[:, ::-1].copy())


def test_nt_table_and_case_table_are_what_the_bound_assumes(m):
    assert m.U == 2.0 ** -24 and m.FACTOR == 2.0 and m.ENVELOPE == 1e-2
    assert m.NT_MAX == 16 and m.NT['standalone'] == 0 and m.NT['adain'] == 0 and all(isinstance(v, int) and v >= 0 for v in m.NT.values())
    names = tuple(n for n, _ in m.ROWS)
    assert len(set(names)) == len(names)
    assert set(m.STRICT) | set(m.WEAK) == set(names) and not set(m.STRICT) & set(m.WEAK)
    # range edges: the fp32 square of every written value stays normal
    for row in ('mag1e-12', 'mag1e12'):
        v = np.abs(m.synth_written(row, NPIX, 128).astype(np.float64))
        sq = (v[v > 0] ** 2)
        assert sq.min() > 2.0 ** -126 and sq.max() < 2.0 ** 127


def test_the_strict_set_is_the_envelope_at_the_largest_nt(m):
    inside = []
    for row, _ in m.ROWS:
        worst = 0.0
        for cout in COUTS:
            t = m.group_terms(_groups(m.synth_written(row, NPIX, cout).astype(np.float64), cout))
            worst = max(worst, float(m.stat_bounds(t, m.NT_MAX, m.GN_EPS)['r_rstd'].max()))
        print(f'{row:12s} bound on the relative rstd error at n_t = {m.NT_MAX}: {worst:.3g}')
        if worst <= m.ENVELOPE:
            inside.append(row)
    assert tuple(inside) == ('kappa0', 'kappa1', 'kappa10', 'kappa100', 'zero_input', 'outlier', 'residual', 'mag1e-12', 'mag1e12')
    assert tuple(inside) == m.STRICT
    assert m.WEAK == ('kappa1000', 'sigma0')


def test_fp32_accumulation_emulation_stays_within_the_bound(m):
    nt = m.NT_MAX
    rng = np.random.default_rng(3)
    for row, _ in m.ROWS:
        for cout in COUTS:
            cpg = cout // 32
            v32 = _groups(m.synth_written(row, NPIX, cout), cout)
            t = m.group_terms(v32.astype(np.float64))
            b = m.stat_bounds(t, nt, m.GN_EPS)
            gamma = ((0.5 + rng.random((32, cpg))) * np.where(rng.random((32, cpg)) < 0.3, -1.0, 1.0)).astype(np.float32)
            beta = rng.standard_normal((32, cpg)).astype(np.float32)
            sc, sh, b_sc, b_sh = m.table_bounds(t, b, gamma.astype(np.float64), beta.astype(np.float64), m.GN_EPS)
            r_sum = r_sq = r_sc = r_sh = 0.0
            for o in _orders(v32):
                s, q = _emulate(o, nt)
                e_s, e_q = np.abs(s - t['s']), np.abs(q - t['q'])
                assert (e_s[b['d_sum'] == 0] == 0).all() and (e_q[b['d_sq'] == 0] == 0).all()
                r_sum = max(r_sum, float((e_s / np.maximum(b['d_sum'], 1e-300)).max()))
                r_sq = max(r_sq, float((e_q / np.maximum(b['d_sq'], 1e-300)).max()))
                # the finalize arithmetic (cf_norm.hip gn_finalize_kernel) on the emulated sums
                mean = s / t['n']
                var = np.maximum(q / t['n'] - mean * mean, 0.0)
                rstd = (1.0 / np.sqrt(var + np.float64(np.float32(m.GN_EPS)))).astype(np.float32)
                sck = (rstd[:, None] * gamma).astype(np.float32)
                shk = ((-sck * mean.astype(np.float32)[:, None]).astype(np.float32) + beta).astype(np.float32)
                assert np.isfinite(sck).all() and np.isfinite(shk).all()
                assert (sck * np.sign(gamma) >= 0).all() and (np.abs(sck) <= np.abs(gamma) / np.sqrt(m.GN_EPS) * (1 + 4 * m.U)).all()
                r_sc = max(r_sc, float((np.abs(sck - sc) / b_sc).max()))
                r_sh = max(r_sh, float((np.abs(shk - sh) / b_sh).max()))
            print(f'{row:12s} cpg {cpg:2d}: emulated / bound  sum {r_sum:.3g}  sumsq {r_sq:.3g}  scale {r_sc:.3g}  shift {r_sh:.3g}')
            assert r_sum <= 1.0 and r_sq <= 1.0, (row, cout, r_sum, r_sq)          # first order alone holds these two with room
            if row in m.STRICT:
                assert r_sc <= m.FACTOR and r_sh <= m.FACTOR, (row, cout, r_sc, r_sh)


def test_fp64_throughout_leaves_only_the_final_roundings(m):
    """n_t = 0 (the stand-alone pass, AdaIN): fp64 sums in any order, then the fp32 table arithmetic, within FACTOR x the n_t = 0 bound --
    on every row, the weak ones included (the property the stand-alone pass's header promises for any |mean| / std)."""
    rng = np.random.default_rng(4)
    for row, _ in m.ROWS:
        cout = 128
        v = _groups(m.synth_written(row, NPIX, cout), cout).astype(np.float64)
        t = m.group_terms(v)
        b = m.stat_bounds(t, 0, m.GN_EPS)
        assert (b['d_sum'] == 0).all() and (b['d_sq'] == 0).all() and (b['d_var'] == 0).all() and np.allclose(b['r_rstd'], 2 * m.U)
        gamma = (0.5 + rng.random((32, 4))).astype(np.float32)
        beta = rng.standard_normal((32, 4)).astype(np.float32)
        sc, sh, b_sc, b_sh = m.table_bounds(t, b, gamma.astype(np.float64), beta.astype(np.float64), m.GN_EPS)
        s, q = v[:, ::-1].sum(1), (v[:, ::-1] ** 2).sum(1)
        mean = s / t['n']
        var = np.maximum(q / t['n'] - mean * mean, 0.0)
        rstd = (1.0 / np.sqrt(var + np.float64(np.float32(m.GN_EPS)))).astype(np.float32)
        sck = (rstd[:, None] * gamma).astype(np.float32)
        shk = ((-sck * mean.astype(np.float32)[:, None]).astype(np.float32) + beta).astype(np.float32)
        r_sc, r_sh = float((np.abs(sck - sc) / b_sc).max()), float((np.abs(shk - sh) / b_sh).max())
        print(f'{row:12s} n_t = 0: emulated / bound  scale {r_sc:.3g}  shift {r_sh:.3g}')
        assert r_sc <= m.FACTOR and r_sh <= m.FACTOR, (row, r_sc, r_sh)


def test_the_fp64_reference_is_stable(m):
    for row, _ in m.ROWS:
        for cout in COUTS:
            v = _groups(m.synth_written(row, NPIX, cout), cout).astype(np.float64)
            t = m.group_terms(v)
            vl = v.astype(np.longdouble)
            n = v.shape[1]
            mu = vl.sum(1) / n
            var = ((vl - mu[:, None]) ** 2).sum(1) / n
            q = (vl * vl).sum(1)
            assert float((np.abs(t['mu'] - mu) / (np.abs(vl).sum(1) / n + np.longdouble(1e-300))).max()) <= 1e-12, row
            assert float((np.abs(t['q'] - q) / (q + np.longdouble(1e-300))).max()) <= 1e-12, row
            scale = float(np.abs(vl).max()) ** 2 + 1e-300       # (sigma = 0 rows: the variance against the magnitude of the data, not against itself)
            assert float((np.abs(t['var'] - var) / np.maximum(var, np.longdouble(1e-12) * scale)).max()) <= 1e-12, row
            for eps in (m.GN_EPS,):
                r64, rl = 1.0 / np.sqrt(t['var'] + eps), 1.0 / np.sqrt(var + np.longdouble(eps))
                assert float((np.abs(r64 - rl) / rl).max()) <= 1e-12, row


def test_layernorm_and_adain_bounds_hold_on_an_fp32_emulation(m):
    """The two other derivations: a float32 two-pass LayerNorm (sequential in-row sums: more additions per element than the kernel's tree)
    and a float32 AdaIN tail on fp64 statistics, against the bounds the GPU test uses."""
    rng = np.random.default_rng(5)
    for C in (256, 1024):
        x = rng.standard_normal((9, C)).astype(np.float32)
        x += np.array([0, 10, 1000] * 3, np.float32)[:, None]
        x[4] = np.float32(1.2345)
        x[8, C // 3] = 1e4
        gamma, beta = (0.5 + rng.random(C)).astype(np.float32), rng.standard_normal(C).astype(np.float32)
        ref, bound, r_rstd = m.ln_bound(x.astype(np.float64), gamma.astype(np.float64), beta.astype(np.float64), m.LN_EPS)
        assert float(r_rstd.max()) <= m.ENVELOPE
        # pairwise float32 sums (numpy's): a tree, as the kernel's quad + butterfly
        mean = (x.sum(1, dtype=np.float32) * np.float32(1.0 / C)).astype(np.float32)
        d = (x - mean[:, None]).astype(np.float32)
        var = ((d * d).astype(np.float32).sum(1, dtype=np.float32) * np.float32(1.0 / C)).astype(np.float32)
        rstd = (np.float32(1.0) / np.sqrt((var + np.float32(m.LN_EPS)).astype(np.float32))).astype(np.float32)
        y = (((d * rstd[:, None]).astype(np.float32) * gamma).astype(np.float32) + beta).astype(np.float32)
        r = float((np.abs(y - ref) / bound).max())
        print(f'LayerNorm C {C}: emulated / bound {r:.3g}')
        assert r <= m.FACTOR
    c = rng.standard_normal((255, 48))
    c[:, 1] = 0.37
    s = rng.standard_normal((255, 48)) * 0.5 + 0.1
    s[:, 2] += 500.0
    c, s = c.astype(np.float32).astype(np.float64), s.astype(np.float32).astype(np.float64)
    ref, bound = m.adain_bound(c, s, m.ADAIN_EPS)
    n = c.shape[0]
    m1, m2 = c.mean(0), s.mean(0)
    v1, v2 = ((c * c).sum(0) - c.sum(0) * m1) / (n - 1), ((s * s).sum(0) - s.sum(0) * m2) / (n - 1)
    f = np.float32
    cs = np.sqrt((np.maximum(v1, 0).astype(f) + f(m.ADAIN_EPS)).astype(f)).astype(f)
    ss = np.sqrt((np.maximum(v2, 0).astype(f) + f(m.ADAIN_EPS)).astype(f)).astype(f)
    out = ((((c.astype(f) - m1.astype(f)).astype(f) / cs).astype(f) * ss).astype(f) + m2.astype(f)).astype(f)
    r = float((np.abs(out - ref) / bound).max())
    print(f'AdaIN: emulated / bound {r:.3g}')
    assert r <= m.FACTOR
