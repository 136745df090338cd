"""-m gpu: the normalisation kernels (GroupNorm statistics of every convolution epilogue and of the stand-alone pass, the finalize
launches, LayerNorm, codebook gather + AdaIN) on ill-conditioned and off-grid inputs.

Reference: fp64 torch on the CPU of the tensor the kernel actually WROTE, read back from the device (F.group_norm, F.layer_norm, the
oracle's adain) -- convolution error never enters a check here.

Bound (derived, not tuned; DESIGN.md "Accuracy envelope of the GroupNorm statistics").  u = 2^-24; n_t = the number of fp32 additions
that reach one accumulator element before its conversion to fp64 (table NT below, one value per kernel family, read from the kernels).
Per (image, group) with mean mu, variance s2 and M2 = s2 + mu^2 of the written tensor, to first order:
    |d sum|   <= n_t u sum|v|              |d sumsq| <= (n_t + 1) u sum v^2            |d var| <= (3 n_t + 1) u M2
    rel. error of rstd  <=  |d var| / (2 (s2 + eps)) + 2u
The table entries add the (float)mean cast, the two fp32 roundings of scale = rstd * gamma and the two of shift = beta - scale * mean.
n_t = 0 stands for "fp64 from the load on" (the stand-alone pass, AdaIN): the three statistic terms vanish and only the final fp32
roundings remain; the fp64 roundings of such a pass (< 2^-53 N (1 + kappa^2) relative on the variance: below 1e-4 u for every strict
case here) and of the host reference are covered by FACTOR.
Every assertion allows FACTOR = 2 over the first-order bound, for the second-order terms and the host's own fp64 arithmetic; that is
justified only where the bound on the relative rstd error is at most ENVELOPE = 1e-2, and a row belongs to the STRICT set only if the
bound stays below it at the largest n_t of the table.  tests/test_norm_bounds_host.py proves the bound on a NumPy emulation of every row,
and asserts the STRICT / WEAK split literally -- nothing here moves a row between the sets at run time.  WEAK rows (kappa ~ 1000 and
sigma = 0 exactly) assert finiteness, sign, the 1 / sqrt(eps) cap and the mean only.

Apart from u, the kernels' eps values, FACTOR and ENVELOPE no kernel tolerance here is a literal (the 1e-9 / 1e-300 of the checks that the
host's own fp64 reference agrees with F.group_norm / F.layer_norm / adain, and the count of GroupNorm calls of a forward, bound no kernel).
"""
import os

import numpy as np
import pytest

from _tools import load_script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
pytestmark = pytest.mark.gpu

U = 2.0 ** -24       # unit roundoff of fp32
FACTOR = 2.0         # over the first-order bound (second-order terms, the host's fp64 arithmetic)
ENVELOPE = 1e-2      # largest bound on the relative rstd error for which FACTOR is justified
GN_EPS = 1e-6        # ops.GN_EPS
LN_EPS = 1e-5        # ops.layernorm's default, the transformer layers' eps
ADAIN_EPS = 1e-5     # codeformer_arch.py:12 (calc_mean_std)
GROUPS = 32

# n_t per kernel family: fp32 additions into one ssum[e] / ssq[e] (rs / rq) element before cf_gn_partials' (double) conversions.
NT = {
    'direct': 16,        # cf_igemm.hip epilogue_vec: `for mi < MI` x `for p < PASSES`, MI = 2, PASSES = 32 / (64 / (8 NI)) = 4 NI, NI <= 2; conv3x3_few_cin_kernel: `for round < 16`
    'direct_splitk': 4,  # cf_igemm.hip launch_sk<2, 2, 1, 1>: the same loops with MI = 1, NI = 1
    'split': 16,         # cf_split.hip epilogue: `for mi < MI` x `for p < PASSES`, MI = 2, PASSES = 4 NI, NI <= 2
    'f23': 4,            # cf_winograd.hip epilogue: `for i < 4` inside one `pass` (ssum / ssq are re-zeroed per pass); split-K: the same loop on `tot`
    'f23_8w': 4,         # cf_wsplit.hip epilogue: `for i < 4` inside one `pass`
    'f43': 4,            # cf_wf43.hip: `rs += v; rq += v * v` over `for c < 4`, widened per `aa`
    'standalone': 0,     # cf_norm.hip gn_stats_kernel: `accum` converts the loaded float4 to double first
    'adain': 0,          # cf_misc.hip gather_adain_kernel: `const double v1 = cb[...]`
}
NT_MAX = max(NT.values())

# ---- the case table of the conditioning sweep ------------------------------------------------------------------------------------------------
# kappa: per-channel bias of magnitude kappa (the convolution part of the written tensor has sigma ~ sqrt(2): He-scaled weights on randn
# inputs, so the realised group ratio |mu| / sigma is ~ 0.7 kappa); every channel j of a group gets the bias (kappa + 0.1 j), groups
# alternate in sign.  zero: all-zero input (every channel constant = its bias); flat: the bias is also constant inside a group.
# outlier: one pixel of 1e4 (through the residual operand; through the input where a form has no residual epilogue).
# res: a constant residual of that value.  mag: everything (input, bias, residual) times this factor.
ROWS = (
    ('kappa0', dict(kappa=0.0)),
    ('kappa1', dict(kappa=1.0)),
    ('kappa10', dict(kappa=10.0)),
    ('kappa100', dict(kappa=100.0)),
    ('kappa1000', dict(kappa=1000.0)),                 # weak
    ('zero_input', dict(kappa=1.1, zero=True)),
    ('sigma0', dict(kappa=1.1, zero=True, flat=True)),  # weak
    ('outlier', dict(kappa=0.0, outlier=1e4)),
    ('residual', dict(kappa=0.0, res=50.0)),
    ('mag1e-12', dict(kappa=1.0, mag=1e-12)),
    ('mag1e12', dict(kappa=1.0, mag=1e12)),
)
WEAK = ('kappa1000', 'sigma0')
STRICT = ('kappa0', 'kappa1', 'kappa10', 'kappa100', 'zero_input', 'outlier', 'residual', 'mag1e-12', 'mag1e12')
ROW = dict(ROWS)
CONV_SIGMA = 2.0 ** 0.5


def row_bias(row, cout):
    """Per-output-channel bias of a row (float64 numpy; the launch gets its float32 rounding)."""
    r = ROW[row]
    cpg = cout // GROUPS
    j = np.arange(cout) % cpg
    sign = np.where((np.arange(cout) // cpg) % 2 == 0, 1.0, -1.0)
    off = 0.0 if r.get('flat') else 0.1 * j
    return sign * (r['kappa'] + off) * r.get('mag', 1.0)


def synth_written(row, npix, cout, seed=0):
    """Host stand-in for the tensor a convolution writes on a row: (npix, cout) float32 with the row's bias, residual and outlier and a
    normal convolution part of sigma sqrt(2).  What the host test classifies and emulates."""
    r = ROW[row]
    rng = np.random.default_rng(seed)
    mag = r.get('mag', 1.0)
    z = np.zeros((npix, cout)) if r.get('zero') else rng.standard_normal((npix, cout)) * CONV_SIGMA * mag
    v = (z.astype(np.float32) + row_bias(row, cout).astype(np.float32)[None, :]).astype(np.float32)
    if r.get('res'):
        v = (v + np.float32(r['res'] * mag)).astype(np.float32)
    if r.get('outlier'):
        v[npix // 3] = (v[npix // 3] + np.float32(r['outlier'])).astype(np.float32)
    return v


# ---- the bound -------------------------------------------------------------------------------------------------------------------------------
def group_terms(v):
    """v: float64 array (..., n) of the n values of each group -> dict of the per-group quantities the bound is made of."""
    n = v.shape[-1]
    s, q, sabs = v.sum(-1), (v * v).sum(-1), np.abs(v).sum(-1)
    mu = s / n
    var = ((v - mu[..., None]) ** 2).sum(-1) / n        # two-pass: stable for any |mu| / sigma
    return dict(n=n, s=s, q=q, sabs=sabs, mu=mu, var=var, m2=var + mu * mu)


def stat_bounds(t, nt, eps):
    """First-order bounds of the module docstring from group_terms(); nt == 0: fp64 from the load on."""
    d_sum = nt * U * t['sabs']
    d_sq = (nt + 1) * U * t['q'] if nt else 0.0 * t['q']
    d_var = (3 * nt + 1) * U * t['m2'] if nt else 0.0 * t['m2']
    r_rstd = 0.5 * d_var / (t['var'] + eps) + 2 * U
    return dict(d_sum=d_sum, d_sq=d_sq, d_var=d_var, d_mean=d_sum / t['n'], r_rstd=r_rstd)


def table_bounds(t, b, gamma, beta, eps):
    """gamma, beta: (..., cpg) per group.  -> reference tables and their bounds.  scale = fl(fl(rstd) * gamma): r_rstd + 2u relative;
    shift = fl(fl(-scale * fl(mean)) + beta): the scale error and the mean's (d_mean + the cast u |mu|) through the product, then the
    product's and the sum's rounding."""
    rstd = 1.0 / np.sqrt(t['var'] + eps)
    sc = rstd[..., None] * gamma
    sh = beta - sc * t['mu'][..., None]
    r_sc = (b['r_rstd'] + 2 * U)[..., None]
    amu = np.abs(t['mu'])[..., None]
    b_sc = np.abs(sc) * r_sc
    b_sh = np.abs(sc) * (amu * (r_sc + U) + b['d_mean'][..., None]) + U * np.abs(sc) * amu + U * (np.abs(sc) * amu + np.abs(beta))
    return sc, sh, b_sc, b_sh


def ln_bound(x, gamma, beta, eps):
    """cf_norm.hip layernorm_kernel, C = 256 NV: two-pass fp32.  x (rows, C), gamma, beta (C,) float64 -> (reference, bound).
    mean: a value passes the quad tree (2 additions), the in-lane chain (NV), the 6-step butterfly, the product with the rounded 1 / C (2):
    |d mean| <= (10 + NV) u mean|x|.  d = fl(x - mean) carries -d mean (common to the row: first-order neutral in sum d^2, second order
    d mean^2) and u |d|; sum d^2: the square (1), the in-lane chain (4 NV), the butterfly (6), the product with 1 / C (2):
    |d var| <= (4 NV + 11) u s2 + d mean^2.  rstd = 1 / sqrtf(fl(var + eps)): 4u more (sum, root, division).
    y = fl(fl(fl(d rstd) gamma) + beta):  |dy| <= |gamma| rstd |d mean| + |t| (r_rstd + 3u) + u |y|,  t = (x - mu) rstd gamma
    (the first term is 'the eps term' of a constant row: there rstd = 1 / sqrt(eps) and t = 0)."""
    C = x.shape[-1]
    nv = C // 256
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    d_mean = (10 + nv) * U * np.abs(x).mean(-1, keepdims=True)
    d_var = (4 * nv + 11) * U * var + d_mean ** 2
    r_rstd = 0.5 * d_var / (var + eps) + 4 * U
    rstd = 1.0 / np.sqrt(var + eps)
    t = (x - mu) * rstd * gamma
    y = t + beta
    return y, np.abs(gamma) * rstd * d_mean + np.abs(t) * (r_rstd + 3 * U) + U * np.abs(y), r_rstd


def adain_bound(c, s, eps):
    """cf_misc.hip gather_adain_kernel.  c, s: (ntok, dim) float64 content (gathered codebook rows) / style.  Statistics in fp64 (n_t = 0);
    fp32 from there: cm, sm = (float)mean (u each); cs, ss = sqrtf((float)var + eps) (cast, sum, root: 2u relative each);
    out = fl(fl(fl(fl(v - cm) / cs) ss) + sm):   |d out| <= u (|m1| ss / cs + 7 |t| + |sm| + |out|),  t = (v - m1) ss / cs."""
    n = c.shape[0]
    m1, m2 = c.mean(0), s.mean(0)
    cs = np.sqrt(((c - m1) ** 2).sum(0) / (n - 1) + eps)
    ss = np.sqrt(((s - m2) ** 2).sum(0) / (n - 1) + eps)
    t = (c - m1) / cs * ss
    out = t + m2
    return out, U * (np.abs(m1) * ss / cs + 7 * np.abs(t) + np.abs(m2) + np.abs(out))


# ---- fixtures --------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def ops():
    import torch
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    from codeformer_amd import lib, ops as o
    lib.load()
    return o


RATIOS = {}   # family -> largest measured-error / first-order-bound ratio of a strict assertion (a report: every ratio is asserted where it is taken)


@pytest.fixture(scope='module', autouse=True)
def _report_ratios():
    """Prints, when the module's last test has run (whichever tests were selected, in whatever order), the largest ratio per family."""
    yield
    for fam, r in RATIOS.items():
        print(f'  largest measured / bound ratio | {fam:32s} {r:.3g}')


def _ratio(label, what, err, bound):
    """Largest err / bound over the elements with a non-zero bound; elements with a zero bound must have zero error."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    assert np.isfinite(err).all() and np.isfinite(bound).all(), (label, what)
    zero = bound == 0
    assert (err[zero] == 0).all(), (label, what, 'error where the bound is zero')
    r = float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0
    fam = label.split(' | ')[0]
    RATIOS[fam] = max(RATIOS.get(fam, 0.0), r)
    print(f'    {label} | {what}: measured / bound = {r:.3g}')
    return r


def _groups_of(ts, cpg):
    """List of (B, H, W, Ci) float64 CPU tensors (a channel concatenation) -> (B, groups, hw * cpg) numpy."""
    import torch
    full = torch.cat(ts, dim=3)
    B, H, W, C = full.shape
    return full.view(B, H * W, C // cpg, cpg).permute(0, 2, 1, 3).reshape(B, C // cpg, H * W * cpg).numpy()


def _check_reference_is_group_norm(ts, sc, sh, gamma, beta):
    """The reference tables ARE fp64 F.group_norm of the written tensor: x * scale + shift against it, to fp64 accuracy."""
    import torch
    import torch.nn.functional as F
    full = torch.cat(ts, dim=3).permute(0, 3, 1, 2)
    B, C = full.shape[:2]
    want = F.group_norm(full, GROUPS, torch.from_numpy(gamma), torch.from_numpy(beta), GN_EPS)
    sct, sht = torch.from_numpy(sc).view(B, C, 1, 1), torch.from_numpy(sh).view(B, C, 1, 1)
    got = full * sct + sht
    room = (full * sct).abs() + sht.abs() + 1e-300
    assert float(((got - want).abs() / room).max()) <= 1e-9


def _check_tables(label, what, ops_mod, xs, ts, gamma, beta, nt, strict, fused=None):
    """ops.groupnorm_tables(xs) against the fp64 tables of ts (the same tensors read back) at n_t = nt."""
    import torch
    ctot = sum(t.shape[3] for t in ts)
    cpg = ctot // GROUPS
    B = ts[0].shape[0]
    old = ops_mod.FINALIZE_FUSED
    try:
        if fused is not None:
            ops_mod.FINALIZE_FUSED = fused
        sc_k, sh_k = ops_mod.groupnorm_tables(xs, torch.from_numpy(gamma).float().cuda(), torch.from_numpy(beta).float().cuda())
    finally:
        ops_mod.FINALIZE_FUSED = old
    sc_k, sh_k = sc_k.double().cpu().numpy().reshape(B, GROUPS, cpg), sh_k.double().cpu().numpy().reshape(B, GROUPS, cpg)
    g32 = gamma.astype(np.float32).astype(np.float64).reshape(GROUPS, cpg)[None]
    b32 = beta.astype(np.float32).astype(np.float64).reshape(GROUPS, cpg)[None]
    t = group_terms(_groups_of(ts, cpg))
    b = stat_bounds(t, nt, GN_EPS)
    sc, sh, b_sc, b_sh = table_bounds(t, b, g32, b32, GN_EPS)
    assert np.isfinite(sc_k).all() and np.isfinite(sh_k).all(), (label, what, 'non-finite tables')
    rstd_err = float((np.abs(sc_k / g32 * np.sqrt(t['var'] + GN_EPS)[..., None] - 1.0)).max())
    if not strict:
        print(f'    {label} | {what} [weak]: relative rstd error {rstd_err:.3g} (bound {float(b["r_rstd"].max()):.3g}, outside the envelope)')
        assert (sc_k * np.sign(g32) >= 0).all(), (label, what, 'scale with the wrong sign')
        assert (np.abs(sc_k) <= np.abs(g32) / np.sqrt(GN_EPS) * (1 + 4 * U)).all(), (label, what, 'scale above |gamma| / sqrt(eps)')
        return
    assert float(b['r_rstd'].max()) <= ENVELOPE, (label, what, 'a strict row outside the envelope', float(b['r_rstd'].max()))
    _check_reference_is_group_norm(ts, sc.reshape(B, -1), sh.reshape(B, -1), g32.reshape(-1), b32.reshape(-1))
    r1 = _ratio(label, what + ' scale', np.abs(sc_k - sc), b_sc)
    r2 = _ratio(label, what + ' shift', np.abs(sh_k - sh), b_sh)
    assert r1 <= FACTOR and r2 <= FACTOR, (label, what, r1, r2, rstd_err)


def _check_partials(label, y, t64, nt, strict):
    """(sum, sumsq) per (image, fine group), the parts added on the host in fp64, against the tensor read back."""
    st = y._cf_stats
    B, C = t64.shape[0], t64.shape[3]
    got = st.part.view(B, C // st.cpg, st.parts, 2).sum(2).cpu().numpy()
    assert np.isfinite(got).all(), (label, 'non-finite partials')
    t = group_terms(_groups_of([t64], st.cpg))
    b = stat_bounds(t, nt, GN_EPS)
    e_s, e_q = np.abs(got[..., 0] - t['s']), np.abs(got[..., 1] - t['q'])
    if strict:
        r1 = _ratio(label, 'partial sum', e_s, b['d_sum'])
        r2 = _ratio(label, 'partial sumsq', e_q, b['d_sq'])
        if not (r1 <= FACTOR and r2 <= FACTOR):     # distinct per-channel means: the residual names the channel that went astray
            i = np.unravel_index(np.argmax(e_q / np.maximum(b['d_sq'], 1e-300)), e_q.shape)
            print(f'    residual at (image, group) {i}: d sum {got[i][0] - t["s"][i]:.6g}  d sumsq {got[i][1] - t["q"][i]:.6g}  mu {t["mu"][i]:.6g}  n {t["n"]}')
        assert r1 <= FACTOR and r2 <= FACTOR, (label, r1, r2)
    else:   # weak rows: the mean within its bound
        r = _ratio(label, 'partial mean [weak]', e_s / t['n'], b['d_mean'])
        assert r <= FACTOR, (label, r)


def _check_act_scale(label, ops_mod, ys, ts, growth=4.0):
    """What ops.act_scale promises on partials: s a power of two with s * inv == 1, growth max|x| s < 2^14, s at most 2^7 below the tight scale.
    The scale comes from the square root of the largest partial sumsq, which exceeds max|x| by at most the root of the number of values in a
    partial: the 2^7 holds for partials of at most 2^14 values, which is asserted here from the partials' own layout (every shape of this
    file is a whole number of tiles, so a group's hw * cpg values are spread evenly over its `parts` partials)."""
    import torch
    for y, t in zip(ys, ts):
        st = y._cf_stats
        assert t.shape[1] * t.shape[2] * st.cpg <= st.parts * 2 ** 14, (label, tuple(t.shape), st.cpg, st.parts)
    act = ops_mod.act_scale(ys[0], ys[1] if len(ys) > 1 else None, growth=growth).cpu().double().numpy()
    amax = torch.cat(ts, dim=3).abs().amax(dim=(1, 2, 3)).numpy()
    for b in range(act.shape[0]):
        s, inv = act[b]
        m = growth * amax[b]
        assert s * inv == 1.0 and np.frexp(s)[0] == 0.5, (label, s, inv)
        assert m * s < 2.0 ** 14, (label, b, m, s)
        tight = 2.0 ** (14 - np.frexp(np.float32(m))[1])       # growth max|x| tight in [2^13, 2^14)
        assert s >= tight / 2.0 ** 7, (label, b, m, s, tight)


# ---- 2. conditioning sweep of the epilogue statistics ---------------------------------------------------------------------------------------
# name, NT key, operand code (an attribute of ops; None: the exact direct kernel, code 0), input (B, H, W, cin), cout, options
FAMILIES = (
    ('direct 3x3', 'direct', None, (2, 32, 32, 64), 128, {}),
    ('direct 3x3 cpg2', 'direct', None, (2, 32, 32, 64), 64, {}),
    ('direct 1x1', 'direct', None, (2, 64, 64, 128), 64, dict(taps=1)),
    ('direct stride 2', 'direct', None, (2, 64, 64, 64), 64, dict(stride=2)),
    ('direct upsample', 'direct', None, (2, 16, 16, 64), 64, dict(up=True)),
    ('split 3x3', 'split', 'SPLIT', (3, 32, 48, 128), 128, {}),
    ('split stride 2', 'split', 'SPLIT', (2, 64, 64, 64), 64, dict(stride=2)),
    ('split upsample', 'split', 'SPLIT', (3, 32, 48, 128), 128, dict(up=True)),
    ('F(2,3) fp32', 'f23', 'WINOGRAD', (2, 16, 16, 64), 128, {}),
    ('F(2,3) fp32 cpg2', 'f23', 'WINOGRAD', (3, 32, 48, 64), 64, {}),
    ('F(2,3) split', 'f23', 'WSPLIT', (3, 32, 48, 64), 64, {}),
    ('F(2,3) 8-wave', 'f23_8w', 'WSPLIT', (3, 32, 48, 128), 128, {}),
    ('F(4,3) split', 'f43', 'WF43', (3, 32, 48, 64), 64, {}),
    ('F(4,3) split 16-wave', 'f43', 'WF43', (3, 32, 48, 128), 128, {}),
    ('F(4,3) fp32', 'f43', 'WF43F', (3, 32, 48, 128), 128, {}),
    ('F(4,3) upsampling gather', 'f43', 'WF43F', (2, 32, 32, 128), 128, dict(up=True, no_res=True)),
    ('F(2,3) split-K', 'f23', 'WINOGRAD', (1, 16, 16, 512), 512, dict(split_k=2)),
    ('token GEMM split-K residual', 'direct_splitk', None, (1, 16, 16, 512), 512, dict(taps=1, split_k=2, always_res=True)),
)
FAMILY = {f[0]: f for f in FAMILIES}
assert len(FAMILY) == len(FAMILIES) and all(f[1] in NT for f in FAMILIES)


def _family(ops_mod, name):
    """One row of FAMILIES with its operand code resolved on ops."""
    name, ntk, code, shape, cout, opt = FAMILY[name]
    return name, ntk, (0 if code is None else getattr(ops_mod, code)), shape, cout, opt


def _produce(o, code, shape, cout, opt, row, seed, storage=None):
    """One launch of a family on a row -> the output tensor(s) with `._cf_stats`.  storage='bf16': also the same launch on bf16 tensors."""
    import torch
    r = ROW[row]
    mag = r.get('mag', 1.0)
    B, H, W, cin = shape
    taps = opt.get('taps', 3)
    stride, up = opt.get('stride', 1), opt.get('up', False)
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(shape) if r.get('zero') else torch.randn(shape, generator=g) * mag
    w = torch.randn(cout, cin, taps, taps, generator=g) * (2.0 / (taps * taps * cin)) ** 0.5     # He: the convolution part has sigma ~ sqrt(2)
    bias = torch.from_numpy(row_bias(row, cout)).float()
    Ho, Wo = (H // 2, W // 2) if stride == 2 else ((2 * H, 2 * W) if up else (H, W))
    res = None
    if (r.get('res') or r.get('outlier') or opt.get('always_res')) and not opt.get('no_res'):
        res = torch.full((B, Ho, Wo, cout), float(r.get('res', 0.0) * mag))
        if r.get('outlier'):
            res[0, Ho // 3, Wo // 3, :] = r['outlier']
    elif r.get('outlier'):        # a form without a residual epilogue: the outlier enters through one input pixel
        x[0, H // 3, W // 3, :] = r['outlier'] / 3.0
    if storage == 'bf16':
        x = x.to(torch.bfloat16).float()
        res = None if res is None else res.to(torch.bfloat16).float()
    pw = o.pack_weight(w.cuda(), bias.cuda(), bf16=code, up2x=up and code != o.WF43F, stride2=(stride == 2 and code == o.SPLIT))
    kw = dict(stride=stride, upsample=up, emit_stats=True)
    if res is not None:
        kw.update(epilogue=o.EPI_RESIDUAL)
    if 'split_k' in opt:
        kw.update(split_k=opt['split_k'])
    xc = x.cuda()
    if o.needs_act_scale(pw):
        kw.update(act=o.act_scale(xc))
    y = o.conv2d(xc, pw, res=None if res is None else res.cuda(), **kw)
    assert getattr(y, '_cf_stats', None) is not None, 'the launch attached no statistics'
    if storage != 'bf16':
        return y
    y16 = o.conv2d(xc.to(torch.bfloat16), pw, res=None if res is None else res.cuda().to(torch.bfloat16), **kw)
    return y, y16


def _affine(cout, seed):
    rng = np.random.default_rng(seed)
    gamma = (0.5 + rng.random(cout)) * np.where(rng.random(cout) < 0.3, -1.0, 1.0)      # both signs: the weak rows check scale * sign(gamma)
    return gamma, rng.standard_normal(cout)


@pytest.mark.parametrize('family', [f[0] for f in FAMILIES])
def test_epilogue_statistics_over_the_conditioning_rows(ops, family):
    """Every row of the case table through one kernel family: partials, the tables of both FINALIZE_FUSED settings at the family's n_t, the
    tables of the stand-alone pass on the same tensor at n_t = 0, and the range scale act_scale takes from the partials."""
    name, ntk, code, shape, cout, opt = _family(ops, family)
    nt = NT[ntk]
    gamma, beta = _affine(cout, 5)
    for i, (row, _) in enumerate(ROWS):
        strict = row in STRICT
        assert strict != (row in WEAK)
        label = f'{name} | {row}'
        y = _produce(ops, code, shape, cout, opt, row, seed=100 + i)
        t64 = y.double().cpu()
        assert bool(t64.isfinite().all()), label
        _check_partials(label, y, t64, nt, strict)
        for fused in (True, False):
            _check_tables(label, f'tables fused={int(fused)}', ops, [y], [t64], gamma, beta, nt, strict, fused=fused)
        plain = y.clone()                   # (no `._cf_stats`: groupnorm_tables runs the stand-alone pass)
        assert getattr(plain, '_cf_stats', None) is None
        _check_tables(label, 'tables stand-alone pass', ops, [plain], [t64], gamma, beta, NT['standalone'], strict)
        _check_act_scale(label, ops, [y], [t64])


def test_streaming_1x1_emits_no_statistics(ops):
    """The 1x1 streaming form of the split-half kernel is the one convolution form without a statistics epilogue: the C ABI says so."""
    import torch
    pw = ops.pack_weight(torch.randn(64, 128, 1, 1).cuda() * 0.1, None, bf16=ops.SPLIT)
    x = torch.randn(1, 64, 64, 128).cuda()
    with pytest.raises(RuntimeError, match='statistics'):
        ops.conv2d(x, pw, act=ops.act_scale(x), emit_stats=True)


def test_concatenated_pair_over_the_conditioning_rows(ops):
    """gmerge = 2: two 128-channel convolution outputs normalised as one 256-channel tensor (cpg 8 from two tensors of fine cpg 4)."""
    _, ntk, code, shape, cout, opt = _family(ops, 'direct 3x3')
    gamma, beta = _affine(2 * cout, 6)
    for i, (row, _) in enumerate(ROWS):
        strict = row in STRICT
        label = f'concatenated pair | {row}'
        ya = _produce(ops, code, shape, cout, opt, row, seed=300 + i)
        yb = _produce(ops, code, shape, cout, opt, row, seed=400 + i)
        ts = [ya.double().cpu(), yb.double().cpu()]
        assert ya._cf_stats.cpg * 2 == 2 * cout // GROUPS
        for half, (yh, th) in enumerate(zip((ya, yb), ts)):      # each half's own partials (fine groups), the weak rows' mean among them
            _check_partials(f'{label} | half {half}', yh, th, NT[ntk], strict)
        for fused in (True, False):
            _check_tables(label, f'tables fused={int(fused)}', ops, [ya, yb], ts, gamma, beta, NT[ntk], strict, fused=fused)
        _check_tables(label, 'tables stand-alone pass', ops, [ya.clone(), yb.clone()], ts, gamma, beta, NT['standalone'], strict)
        _check_act_scale(label, ops, [ya, yb], ts)


def test_bf16_storage_partials_describe_the_fp32_values(ops):
    """bf16 storage (the eight-wave F(2,3) kernel on bf16 tensors): the statistics are taken before the store rounding, so the reference is
    the fp64 of the fp32 value -- the same launch with fp32 storage.  Partials only (and the range scale act_scale takes from them)."""
    import torch
    code = ops.conv_code(1, 128, 128, 64, 64)
    assert code == ops.WBF16
    for i, (row, _) in enumerate(ROWS):
        label = f'bf16 storage | {row}'
        y32, y16 = _produce(ops, code, (1, 64, 64, 128), 128, {}, row, seed=500 + i, storage='bf16')
        assert y16.dtype == torch.bfloat16 and torch.equal(y16, y32.to(torch.bfloat16)), label
        y16f = y16.float()          # (a carrier for the check: its values are not used, its partials are)
        y16f._cf_stats = y16._cf_stats
        t32 = y32.double().cpu()
        _check_partials(label, y16f, t32, NT['f23_8w'], row in STRICT)
        _check_act_scale(label, ops, [y16], [t32])      # (the range scale of the bf16 tensor, from the same partials: a bound on the fp32 values)


# ---- 3. off-grid shapes of the stand-alone kernels, through the C ABI --------------------------------------------------------------------------
def _offset_input(shape, kappa, seed, j_mod):
    """randn + kappa + 0.1 * (channel index mod j_mod): sigma ~ 1, |mu| / sigma ~ kappa, distinct per-channel means."""
    import torch
    g = torch.Generator().manual_seed(seed)
    c = torch.arange(shape[-1]) % j_mod
    return torch.randn(shape, generator=g) + kappa + 0.1 * c


def test_groupnorm_stats_kernel_off_grid_shapes(ops):
    """cf_groupnorm_stats + cf_groupnorm_finalize: C = 16 (64 row lanes), 32, 64, 1024 (one row lane), cpg 2 (a quad straddles two groups) .. 64,
    ragged hw, parts that leave the tail loop, blocks past hw; against fp64 group_norm at n_t = 0, bitwise repeatable and batch invariant."""
    import torch
    from codeformer_amd import lib as L
    lib = L.load()
    B = 3
    worst = 0.0
    for C in (16, 32, 64, 1024):
        for hw in (1, 7, 255, 257, 40 * 48):
            for kappa in (0.0, 100.0):
                x = _offset_input((B, hw, C), kappa, seed=C + hw, j_mod=8)
                xc = x.cuda()
                x64 = x.double().view(B, hw, 1, C)
                for cpg in (2, 4, 32, 64):
                    if C % cpg or C // cpg > 64:
                        continue
                    G = C // cpg
                    rng = np.random.default_rng(C + cpg)
                    gamma, beta = (0.5 + rng.random(C)).astype(np.float32), rng.standard_normal(C).astype(np.float32)
                    g_d, b_d = torch.from_numpy(gamma).cuda(), torch.from_numpy(beta).cuda()
                    v = x64.view(B, hw, G, cpg).permute(0, 2, 1, 3).reshape(B, G, hw * cpg).numpy()
                    t = group_terms(v)
                    sc, sh, b_sc, b_sh = table_bounds(t, stat_bounds(t, NT['standalone'], GN_EPS), gamma.astype(np.float64).reshape(1, G, cpg),
                                                      beta.astype(np.float64).reshape(1, G, cpg), GN_EPS)
                    import torch.nn.functional as F
                    want = F.group_norm(x64.view(B, hw, C).permute(0, 2, 1), G, torch.from_numpy(gamma).double(), torch.from_numpy(beta).double(), GN_EPS)
                    mine = x64.view(B, hw, C).permute(0, 2, 1) * torch.from_numpy(sc).view(B, C, 1) + torch.from_numpy(sh).view(B, C, 1)
                    assert float(((mine - want).abs() / (want.abs() + torch.from_numpy(np.abs(sh)).view(B, C, 1) + 1e-300)).max()) <= 1e-9

                    def tables(xin, nb, parts):
                        part = torch.full((nb * G * parts * 2,), float('nan'), dtype=torch.float64, device='cuda')
                        L.check(lib.cf_groupnorm_stats(L.ptr(xin), nb, hw, C, cpg, L.ptr(part, dtype=torch.float64), parts, L.stream_ptr()), 'cf_groupnorm_stats')
                        s, h = torch.empty(nb, C, device='cuda'), torch.empty(nb, C, device='cuda')
                        L.check(lib.cf_groupnorm_finalize(L.ptr(part, dtype=torch.float64), nb, parts, C, cpg, 1, hw * cpg, L.ptr(g_d), L.ptr(b_d), GN_EPS,
                                                          L.ptr(s), L.ptr(h), C, L.stream_ptr()), 'cf_groupnorm_finalize')
                        return part, s, h

                    for parts in (1, 3, 256, hw + 5):
                        part, s_k, h_k = tables(xc, B, parts)
                        part2, s_k2, h_k2 = tables(xc, B, parts)
                        assert torch.equal(part, part2) and torch.equal(s_k, s_k2) and torch.equal(h_k, h_k2), (C, cpg, hw, parts)
                        p1, s_1, h_1 = tables(xc[1:2].contiguous(), 1, parts)
                        assert torch.equal(part.view(B, -1)[1:2], p1.view(1, -1)) and torch.equal(s_k[1:2], s_1) and torch.equal(h_k[1:2], h_1), (C, cpg, hw, parts)
                        assert bool(torch.isfinite(part).all()), (C, cpg, hw, parts)          # every (group, part) cell is written, blocks past hw too
                        e_sc = np.abs(s_k.double().cpu().numpy().reshape(B, G, cpg) - sc)
                        e_sh = np.abs(h_k.double().cpu().numpy().reshape(B, G, cpg) - sh)
                        r = max(float((e_sc / b_sc).max()), float((e_sh / b_sh).max()))
                        worst = max(worst, r)
                        assert r <= FACTOR, (C, cpg, hw, parts, kappa, r)
    print(f'  stand-alone GroupNorm pass: largest measured / bound ratio {worst:.3g}')
    assert worst > 0.0
    x = torch.zeros(1, 64, 256, device='cuda')
    part = torch.empty(1 * 128 * 2, dtype=torch.float64, device='cuda')
    for (C, cpg) in ((48, 4), (64, 3), (256, 2)):       # C does not divide 1024; odd cpg; 128 groups -- refused before any launch
        assert lib.cf_groupnorm_stats(L.ptr(x), 1, 64, C, cpg, L.ptr(part, dtype=torch.float64), 1, L.stream_ptr()) != 0
        assert 'cf_groupnorm_stats' in L.last_error(), L.last_error()


def test_layernorm_kernel_every_width_ragged_rows_and_offsets(ops):
    """cf_layernorm: all four instantiations, row counts that leave waves of the last workgroup idle (the `row >= rows` exit, checked by a NaN
    guard row behind y and ypos), pos tables with rows % npos != 0, row offsets up to kappa = 1000, a constant row, a 1e4 outlier."""
    import torch
    import torch.nn.functional as F
    from codeformer_amd import lib as L
    lib = L.load()
    worst = 0.0
    for C in (256, 512, 768, 1024):
        rng = np.random.default_rng(C)
        gamma, beta = (0.5 + rng.random(C)).astype(np.float32), rng.standard_normal(C).astype(np.float32)
        g_d, b_d = torch.from_numpy(gamma).cuda(), torch.from_numpy(beta).cuda()
        for rows in (1, 3, 4, 5, 509):
            g = torch.Generator().manual_seed(C + rows)
            x = torch.randn(rows, C, generator=g)
            kap = torch.tensor([0.0, 10.0, 1000.0])[torch.arange(rows) % 3]
            x = x + kap[:, None]
            x[rows // 2] = 1.2345                       # a constant row: sigma = 0
            if rows >= 4:
                x[rows - 1, C // 3] = 1e4                 # one outlier in an otherwise kappa-offset row
            y_ref, bound, r_rstd = ln_bound(x.double().numpy(), gamma.astype(np.float64), beta.astype(np.float64), LN_EPS)
            assert float(r_rstd.max()) <= ENVELOPE
            want = F.layer_norm(x.double(), (C,), torch.from_numpy(gamma).double(), torch.from_numpy(beta).double(), LN_EPS).numpy()
            assert float((np.abs(y_ref - want) / (np.abs(want) + np.abs(beta) + 1e-300)).max()) <= 1e-9       # the reference is fp64 F.layer_norm
            xc = x.cuda()
            for npos in (None, 1, 3, 4, 256):
                y = torch.full((rows + 1, C), float('nan'), device='cuda')
                yp = torch.full((rows + 1, C), float('nan'), device='cuda') if npos else None
                pos = torch.randn(npos, C, generator=g).cuda() if npos else None
                L.check(lib.cf_layernorm(L.ptr(xc), rows, C, L.ptr(g_d), L.ptr(b_d), LN_EPS, L.ptr(pos), npos or 0, L.ptr(y), L.ptr(yp), L.stream_ptr()),
                        'cf_layernorm')
                assert bool(torch.isnan(y[rows]).all()) and (yp is None or bool(torch.isnan(yp[rows]).all())), (C, rows, npos, 'guard row written')
                yk = y[:rows].double().cpu().numpy()
                assert np.isfinite(yk).all()
                r = float((np.abs(yk - want) / bound).max())
                worst = max(worst, r)
                assert r <= FACTOR, (C, rows, npos, r, np.unravel_index(np.argmax(np.abs(yk - want) / bound), yk.shape))
                if npos:        # ypos = fl(y + pos[row % npos]): one fp32 addition of the value that was stored as y
                    idx = torch.arange(rows, device='cuda') % npos
                    assert torch.equal(yp[:rows], y[:rows] + pos[idx]), (C, rows, npos)
    print(f'  LayerNorm: largest measured / bound ratio {worst:.3g}')
    x = torch.zeros(4, 384, device='cuda')
    assert lib.cf_layernorm(L.ptr(x), 4, 384, L.ptr(x), L.ptr(x), LN_EPS, None, 0, L.ptr(torch.empty_like(x)), None, L.stream_ptr()) != 0
    assert 'cf_layernorm' in L.last_error() and '384' in L.last_error()


def test_gather_adain_kernel_partial_channel_blocks_clamps_and_constant_channels(ops):
    """cf_codebook_gather_adain: dim 48 (the `c >= dim` lanes of the second 32-channel block), ntok 2 and 255, indices -1 and ncodes (clamped),
    a codebook channel constant over the gathered tokens (var = 0: only eps under the root), a style channel at kappa = 1000; against the
    oracle's adain in fp64; without a style tensor bitwise plain indexing."""
    import torch
    from oracle import codeformer_oracle as O
    ncodes, B = 64, 2
    worst = 0.0
    for dim in (32, 48, 256):
        for ntok in (2, 255, 256):
            g = torch.Generator().manual_seed(dim + ntok)
            cb = torch.randn(ncodes, dim, generator=g)
            cb[:, 1] = 0.37                                           # constant over any choice of tokens
            idx = torch.randint(0, ncodes, (B * ntok,), generator=g)
            idx[0], idx[-1] = -1, ncodes                               # clamp to 0 / ncodes - 1
            lq = torch.randn(B, ntok, dim, generator=g) * 0.5 + 0.1
            lq[:, :, 2] += 500.0                                       # kappa = 1000 in the style
            ic = idx.clamp(0, ncodes - 1)
            plain = ops.codebook_gather(idx.cuda(), cb.cuda(), B, ntok)
            assert torch.equal(plain.cpu(), cb[ic].view(B, ntok, dim)), (dim, ntok)
            got = ops.codebook_gather(idx.cuda(), cb.cuda(), B, ntok, lq=lq.cuda(), eps=ADAIN_EPS).double().cpu()
            q = cb[ic].view(B, ntok, dim).double()
            for b in range(B):
                ref, bound = adain_bound(q[b].numpy(), lq[b].double().numpy(), ADAIN_EPS)
                # the reference is the oracle's adain in fp64 ((B, C, H, W) tensors: the tokens as a 1 x ntok image)
                want = O.adain(q[b].t().reshape(1, dim, 1, ntok), lq[b].double().t().reshape(1, dim, 1, ntok)).reshape(dim, ntok).t().numpy()
                assert float((np.abs(ref - want) / (np.abs(want) + 1e-300)).max()) <= 1e-9
                r = float((np.abs(got[b].numpy() - want) / bound).max())
                worst = max(worst, r)
                assert r <= FACTOR, (dim, ntok, b, r)
    print(f'  gather + AdaIN: largest measured / bound ratio {worst:.3g}')


# ---- 4. what the network actually sees ---------------------------------------------------------------------------------------------------------
def test_network_operating_point_is_inside_the_strict_envelope(ops, monkeypatch):
    """The seeded network on the four real goldens, default mode: per GroupNorm call the largest group kappa = |mu| / sigma and the smallest
    sigma^2 / eps, recovered from the statistics partials the call was handed (from the tensor itself where it carries none), and the bound on
    the relative rstd error they imply at the largest n_t of the table -- every call must lie inside the strict envelope."""
    import torch
    chk = load_script('tools/gpu_check.py')
    calls = []
    real = ops.groupnorm_tables

    def hooked(xs, gamma, beta, eps=ops.GN_EPS, groups=ops.GN_GROUPS, act_growth=None):
        B, H, W, _ = xs[0].shape
        ctot = sum(t.shape[3] for t in xs)
        cpg = ctot // groups
        sums, route = [], 'epilogue'
        for t in xs:
            st = getattr(t, '_cf_stats', None)
            c = t.shape[3]
            if st is None or cpg % st.cpg:
                route = 'stand-alone'
                v = t.double().view(B, H * W, c // cpg, cpg)
                sums.append(torch.stack([v.sum((1, 3)), (v * v).sum((1, 3))], -1))
            else:
                sums.append(st.part.view(B, c // cpg, (cpg // st.cpg) * st.parts, 2).sum(2))
        s = torch.cat(sums, dim=1).cpu().numpy()
        n = H * W * cpg
        mu = s[..., 0] / n
        var = np.maximum(s[..., 1] / n - mu * mu, 0.0)
        kappa = np.abs(mu) / np.sqrt(np.maximum(var, 1e-300))
        nt = NT_MAX if route == 'epilogue' else NT['standalone']
        r = 0.5 * ((3 * nt + 1) * U if nt else 0.0) * (var + mu * mu) / (var + eps) + 2 * U
        calls.append((len(calls), route, (H, W, ctot), float(kappa.max()), float((var / eps).min()), float(r.max())))
        return real(xs, gamma, beta, eps, groups, act_growth=act_growth)

    monkeypatch.setattr(ops, 'groupnorm_tables', hooked)
    worst = []
    for name, cfg in (('real_0143.npz', None), ('real_0342.npz', None), ('real_Solvay_conference_1927_0018.npz', None), ('real_masked_00105.npz', (512, ('32', '64', '128')))):
        net = (chk.build_net() if cfg is None else chk.build_net(*cfg)).cuda()
        net.use_hip_graphs = False          # (a captured forward cannot be observed call by call)
        g = np.load(os.path.join(GOLD, name))
        x = ops.img_u8_to_tensor(torch.from_numpy(g['img']).unsqueeze(0).cuda())
        del calls[:]
        if cfg is None:
            net(x, w=0.5, adain=True)
        else:
            net(x, w=1, adain=False)
        torch.cuda.synchronize()
        assert len(calls) >= 40, len(calls)
        print(f'  {name}: {len(calls)} GroupNorm calls (seeded weights)')
        for (i, route, shp, k, ve, r) in calls:
            print(f'    call {i:3d} {route:11s} {shp[0]:4d}x{shp[1]:<4d} C{shp[2]:<4d} max kappa {k:9.3f}  min sigma^2/eps {ve:10.3g}  rstd bound {r:.3g}')
        worst.append((name, max(c[3] for c in calls), min(c[4] for c in calls), max(c[5] for c in calls)))
    for w in worst:
        print(f'  operating point | {w[0]:40s} largest kappa {w[1]:.3f}  smallest sigma^2/eps {w[2]:.3g}  largest rstd bound {w[3]:.3g}')
    assert max(w[3] for w in worst) <= ENVELOPE, worst
