"""The two attention kernels (cf_attention.hip: attn64_kernel, attn512_kernel) beyond near-uniform softmax: seeded input families, the
fp64 reference softmax(q k^T scale) v, the gate, and a CPU emulation of fp32 attention that makes the gate a condition on the reference.
Library of tests/test_gpu_attention.py (GPU) and tests/test_attention_families_host.py (CPU).
usage (GPU box): python tools/attn_check.py          one line per case: kernel error, emulation error, gate

Flavours (batch 2, different data per image and head):  '8x64' = 8 heads x 64, scale 0.125;  '1x512' = 1 head x 512, scale 512^-0.5.

Families (all generated on the CPU from fixed seeds):
  uniform      q, k ~ 0.7 N(0,1), v ~ N(0,1): the inputs of tools/gpu_check.py:g_attn (same seeds), passed as column slices of one
               (B 256, 3E) matrix as there.  Largest |logit| 2.9 / 2.3, largest probability of a row 0.014 in the median (0.059 / 0.035 at
               most): every output is an average.
  peak4/12/40  k ~ N(0,1), q_r = beta k_pi(r) / (scale dh) with a random permutation pi per (image, head): logit(r, j) =
               beta k_pi(r).k_j / dh, peaked at j = pi(r).  Measured on the CPU (fp64), smallest .. largest over the rows:
                   8x64    peak4  largest logit 2.0 .. 7.0   largest probability 0.026 .. 0.77
                           peak12               5.9 .. 21                         0.46  .. 0.999998
                           peak40               20  .. 70                         0.9998 .. 1
                   1x512   peak4                3.3 .. 4.9                        0.096 .. 0.33
                           peak12               9.9 .. 15                         0.986 .. 0.99986
                           peak40               33  .. 49                         1 - 1e-12 .. 1
               (tests/test_attention_families_host.py asserts these ranges.)
  onehot       peak with beta = ONEHOT_BETA (600 for 8x64, 400 for 1x512): the fp64 gap between the best and the second-best logit of every
               row exceeds 104 (asserted in inputs(); measured smallest gap 132 / 279; beta = 400 leaves 88 for 8x64), so expf underflows
               to exactly 0 for every other key -- fp32 denormals end at e^-103.3 -- and the output is BITWISE v[pi(r)].
  offset c     c in +30, +90, -300, +3000: the uniform inputs with channel 0 of every head of q set to sign(c) sqrt(|c| / scale) and channel 0
               of k to sqrt(|c| / scale): every logit of a row carries the common term c.  Without the max subtraction: inf / inf from
               +90 up, 0 / 0 at -300.
  big          the uniform q and k times 6: logits reach +-90 with both signs (cancellation inside the score sum).
  allsame      every key of an (image) equals its key 0: the output is the column mean of V.
  P ...        P readback on the uniform, peak4 and offset+90 inputs: V holds a 64 x 64 identity in keys [64 j, 64 j + 64) and zeros
               elsewhere, one launch per j = 0..3; the four outputs together are the probability matrix of every head.  For head_dim 512
               the identity of launch j sits at column P512_COLS[j] = 0, 224, 300, 448: the second one straddles the 256-column chunk
               split of attn512_kernel.  max|v| = 1 in the gate.
  ones         V = 1 everywhere (on the uniform, peak4 and big q, k): every output within 2^-16 of 1 (256 correctly rounded probabilities
               summed in fp32: at worst 256 2^-24).
  dup          peak4 with key j copied over keys j + 32, j + 64, j + 128 for j in DUP_KEYS (other waves' key ranges in both kernels, and
               the other V half / key group of attn64_kernel's phase 3): P read back as above, the duplicated columns BITWISE equal
               (same products in the same order).

Gate, against fp64, per output row r of an (image, head) with L_r = the largest |logit| of the row in fp64:
    |got - ref| <= 5e-6 + 1e-5 |ref| + COEF 2^-24 sqrt(head_dim) L_r max|v|
The first two terms are the gate of tools/gpu_check.py:g_attn; the third is the growth of the score rounding with the size of what is
summed: a score is a sum of head_dim products whose partial sums are of the size of L_r, each rounded to 2^-24 relative; the errors add
like a random walk (sqrt(head_dim)); an absolute score error d changes a probability by at most a factor e^d, the output by at most
~d max|v|.  COEF = 0.5 for every family.  The emulation (emulate_probs / emulate_out: fp32, the dh products and the 256 keys accumulated
strictly one after another, each product rounded) is the condition on the gate: tests/test_attention_families_host.py asserts its
error within 0.5 of the gate for every family and both flavours; the factor that remains is the allowance for the kernels' other
association (four key groups, MFMA blocks of two).  Measured emulation error / gate (COEF = 0.5), largest over the elements, and the
emulation's largest |error| -- 8x64 first, 1x512 second:
    uniform      0.031 (2.5e-7)   0.034 (3.9e-7)        big          0.330 (2.3e-5)   0.345 (5.3e-5)
    peak4        0.100 (2.1e-6)   0.087 (2.1e-6)        allsame      0.021 (1.5e-7)   0.019 (1.2e-7)
    peak12       0.158 (7.0e-6)   0.096 (5.9e-6)        P uniform    0.006 (3.5e-8)   0.005 (3.1e-8)
    peak40       0.037 (2.3e-6)   0.000 (1.1e-11)       P peak4      0.053 (5.1e-7)   0.070 (6.8e-7)
    onehot       0     (0)        0     (0)             P offset+90  0.043 (1.2e-6)   0.071 (4.8e-6)
    offset+30    0.038 (1.6e-6)   0.060 (6.0e-6)        ones         0.088 (1.4e-6)   0.061 (1.1e-6)
    offset+90    0.057 (6.3e-6)   0.067 (1.9e-5)        dup          0.054 (6.0e-7)   0.069 (6.8e-7)
    offset-300   0.066 (2.3e-5)   0.053 (4.8e-5)
    offset+3000  0.057 (1.9e-4)   0.082 (7.5e-4)
No number here was tuned to what a kernel returns; the kernels' own figures are in the docstring of tests/test_gpu_attention.py.
"""
import functools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NKEY = 256
U = 2.0 ** -24
FLAVOURS = {
    '8x64': dict(heads=8, head_dim=64, scale=0.125, seed=1),            # the seeds of g_attn's two cases
    '1x512': dict(heads=1, head_dim=512, scale=512 ** -0.5, seed=5),
}
PEAKS = (4, 12, 40)
ONEHOT_BETA = {64: 600, 512: 400}
ONEHOT_GAP = 104.0
OFFSETS = (30, 90, -300, 3000)
BIG = 6.0
P512_COLS = (0, 224, 300, 448)
DUP_KEYS = (0, 5, 17, 31, 100)
DUP_STEPS = (32, 64, 128)
P_ON = ('uniform', 'peak4', 'offset+90')
ONES_ON = ('uniform', 'peak4', 'big')
QK_FAMILIES = ('uniform',) + tuple(f'peak{b}' for b in PEAKS) + ('onehot',) + tuple(f'offset{c:+d}' for c in OFFSETS) + ('big', 'allsame')
FAMILIES = QK_FAMILIES + tuple(f'P {f}' for f in P_ON) + ('ones', 'dup')
COEF = {f: 0.5 for f in FAMILIES}      # (a family whose emulation exceeded 0.5 of the gate would be raised here, to at most 2: none did)


def rnd(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def heads_view(t, heads, dh):
    """(B 256, heads dh) -> (B, heads, 256, dh)"""
    return t.view(-1, NKEY, heads, dh).transpose(1, 2)


def rows_view(t):
    """(B, heads, 256, dh) -> (B 256, heads dh)"""
    B, H, _, dh = t.shape
    return t.transpose(1, 2).reshape(B * NKEY, H * dh)


def peak_q(k, heads, dh, scale, beta, seed):
    """q_r = beta k_pi(r) / (scale dh), a permutation per (image, head) -> (q, pi (B, heads, 256) int64)."""
    B = k.shape[0] // NKEY
    rng = np.random.default_rng(seed)
    pi = torch.from_numpy(np.stack([np.stack([rng.permutation(NKEY) for _ in range(heads)]) for _ in range(B)]))
    kh = heads_view(k, heads, dh)
    q = torch.gather(kh, 2, pi[..., None].expand(-1, -1, -1, dh)) * (beta / (scale * dh))
    return rows_view(q).contiguous(), pi


def inputs(family, heads, head_dim, scale, seed, batch=2):
    """One of QK_FAMILIES or 'dup' -> dict(q, k, v (batch 256, E) float32 CPU tensors, pi or None)."""
    dh, E, R = head_dim, heads * head_dim, batch * NKEY
    q, k, v = rnd((R, E), seed, 0.7), rnd((R, E), seed + 1, 0.7), rnd((R, E), seed + 2)
    pi = None
    if family.startswith('peak') or family in ('onehot', 'dup'):
        beta = ONEHOT_BETA[dh] if family == 'onehot' else (4 if family == 'dup' else int(family[4:]))
        k = rnd((R, E), seed + 1)
        q, pi = peak_q(k, heads, dh, scale, beta, seed + 100)
        if family == 'dup':
            kh = k.view(batch, NKEY, E)
            for j in DUP_KEYS:
                for s in DUP_STEPS:
                    kh[:, j + s] = kh[:, j]
        if family == 'onehot':
            top = (heads_view(q, heads, dh).double() @ heads_view(k, heads, dh).double().transpose(-1, -2) * scale).topk(2, -1).values
            gap = float((top[..., 0] - top[..., 1]).min())
            assert gap > ONEHOT_GAP, (head_dim, gap)
    elif family.startswith('offset'):
        c = int(family[6:])
        a = (abs(c) / scale) ** 0.5
        q.view(R, heads, dh)[:, :, 0] = a if c > 0 else -a
        k.view(R, heads, dh)[:, :, 0] = a
    elif family == 'big':
        q, k = q * BIG, k * BIG
    elif family == 'allsame':
        k = k.view(batch, NKEY, E)[:, :1].expand(-1, NKEY, -1).reshape(R, E).contiguous()
    else:
        assert family == 'uniform', family
    return dict(q=q, k=k, v=v, pi=pi)


def identity_v(j, batch, heads, head_dim):
    """V of launch j of the P readback."""
    v = torch.zeros(batch, NKEY, heads, head_dim)
    col = P512_COLS[j] if head_dim == 512 else 0
    i = torch.arange(64)
    v[:, 64 * j + i, :, col + i] = 1.0
    return v.view(batch * NKEY, heads * head_dim)


def assemble_p(outs, heads, head_dim):
    """The four outputs of the P readback -> (B, heads, 256, 256)."""
    return torch.cat([heads_view(o, heads, head_dim)[..., (P512_COLS[j] if head_dim == 512 else 0):][..., :64] for j, o in enumerate(outs)], -1)


# ---- fp64 reference and gate -------------------------------------------------------------------------------------------------------------
def ref_probs(q, k, heads, head_dim, scale):
    """-> (P (B, heads, 256, 256) float64, L (B, heads, 256): largest |logit| per row)"""
    s = heads_view(q, heads, head_dim).double() @ heads_view(k, heads, head_dim).double().transpose(-1, -2) * scale
    return torch.softmax(s, -1), s.abs().amax(-1)


def ref_out(P, v, heads, head_dim):
    return rows_view(P @ heads_view(v, heads, head_dim).double())


def gate(ref, L, vmax, head_dim, coef=0.5):
    """ref (B 256, E) float64, L (B, heads, 256) -> the tolerance per element."""
    Lr = L.transpose(1, 2).repeat_interleave(head_dim, dim=-1).reshape(ref.shape)
    return 5e-6 + 1e-5 * ref.abs() + coef * U * head_dim ** 0.5 * Lr * vmax


# ---- fp32 emulation: every product rounded, the dh products and the 256 keys accumulated one after another ----------------------------
def emulate_probs(q, k, heads, head_dim, scale):
    f = np.float32
    qT = np.ascontiguousarray(heads_view(q, heads, head_dim).numpy().transpose(3, 0, 1, 2))   # (dh, B, H, 256)
    kT = np.ascontiguousarray(heads_view(k, heads, head_dim).numpy().transpose(3, 0, 1, 2))
    s = np.zeros(qT.shape[1:] + (NKEY,), f)
    for c in range(head_dim):
        s += qT[c][..., :, None] * kT[c][..., None, :]
    s *= f(scale)
    e = np.exp(s - s.max(-1, keepdims=True))
    assert e.dtype == f
    tot = np.zeros(e.shape[:-1], f)
    for j in range(NKEY):
        tot += e[..., j]
    return e / tot[..., None]


def emulate_out(p, v, heads, head_dim):
    vh = np.ascontiguousarray(heads_view(v, heads, head_dim).numpy())
    o = np.zeros(vh.shape, np.float32)
    for j in range(NKEY):
        o += p[..., j, None] * vh[:, :, j, None, :]
    return rows_view(torch.from_numpy(o)).contiguous()


# ---- the kernel --------------------------------------------------------------------------------------------------------------------------
def run_kernel(q, k, v, heads, head_dim, scale, slices=False):
    from codeformer_amd import ops
    B, E = q.shape[0] // NKEY, heads * head_dim
    if slices:
        qkv = torch.cat([q, k, v], 1).cuda()
        q, k, v = qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:]
    else:
        q, k, v = q.cuda(), k.cuda(), v.cuda()
    return ops.attention(q, k, v, B, heads, head_dim, scale).cpu()


def bits_equal(a, b):
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


@functools.lru_cache(maxsize=None)
def _prepared(flavour, qk_family):
    """Inputs, fp64 probabilities and L of a (flavour, q / k family): computed once, shared by every case that uses them, never modified."""
    fl = FLAVOURS[flavour]
    inp = inputs(qk_family, **fl)
    P, L = ref_probs(inp['q'], inp['k'], fl['heads'], fl['head_dim'], fl['scale'])
    return inp, P, L


@functools.lru_cache(maxsize=None)
def _emulated_probs(flavour, qk_family):
    fl = FLAVOURS[flavour]
    inp = _prepared(flavour, qk_family)[0]
    return emulate_probs(inp['q'], inp['k'], fl['heads'], fl['head_dim'], fl['scale'])


def launches(flavour, family):
    """-> list of (q / k family, V, max|v| of the gate) of a family."""
    fl = FLAVOURS[flavour]
    H, dh = fl['heads'], fl['head_dim']
    if family.startswith('P ') or family == 'dup':
        qk = family[2:] if family.startswith('P ') else 'dup'
        return [(qk, identity_v(j, 2, H, dh), 1.0) for j in range(4)]
    if family == 'ones':
        return [(qk, torch.ones(2 * NKEY, H * dh), 1.0) for qk in ONES_ON]
    v = _prepared(flavour, family)[0]['v']
    return [(family, v, float(v.abs().max()))]


def _special(family, flavour, outs):
    """The family's own exact condition on the outputs of its launches (None: the family has none)."""
    fl = FLAVOURS[flavour]
    H, dh = fl['heads'], fl['head_dim']
    if family == 'onehot':
        inp = _prepared(flavour, 'onehot')[0]
        want = rows_view(torch.gather(heads_view(inp['v'], H, dh), 2, inp['pi'][..., None].expand(-1, -1, -1, dh)))
        return bits_equal(outs[0], want)
    if family == 'ones':
        return all(float((o.double() - 1.0).abs().max()) <= 2.0 ** -16 for o in outs)
    if family == 'dup':
        P = assemble_p(outs, H, dh)
        return all(bits_equal(P[..., j], P[..., j + s]) for j in DUP_KEYS for s in DUP_STEPS)
    return None


def case(flavour, family, kernel=True, emulate=True):
    """One family on one flavour -> dict: per side ('kernel', 'emu') the largest |error|, the largest error / gate, finiteness and the
    family's exact condition; 'gate' = the gate at the element of the kernel's (else the emulation's) largest error / gate."""
    fl = FLAVOURS[flavour]
    H, dh, scale = fl['heads'], fl['head_dim'], fl['scale']
    res = dict(flavour=flavour, family=family)
    sides = (['kernel'] if kernel else []) + (['emu'] if emulate else [])
    acc = {s: dict(err=0.0, ratio=0.0, finite=True, outs=[], gate=0.0) for s in sides}
    for qk, v, vmax in launches(flavour, family):
        inp, P, L = _prepared(flavour, qk)
        ref = ref_out(P, v, H, dh)
        tol = gate(ref, L, vmax, dh, COEF[family])
        got = {}
        if kernel:
            got['kernel'] = run_kernel(inp['q'], inp['k'], v, H, dh, scale, slices=(family == 'uniform'))
        if emulate:
            got['emu'] = emulate_out(_emulated_probs(flavour, qk), v, H, dh)
        for s, o in got.items():
            a = acc[s]
            a['outs'].append(o)
            a['finite'] = a['finite'] and bool(torch.isfinite(o).all())
            d = (o.double() - ref).abs()
            d = torch.where(torch.isfinite(d), d, torch.full_like(d, float('inf')))
            r = d / tol
            i = int(r.argmax())
            if float(r.view(-1)[i]) >= a['ratio']:
                a['ratio'], a['gate'] = float(r.view(-1)[i]), float(tol.view(-1)[i])
            a['err'] = max(a['err'], float(d.max()))
    for s in sides:
        a = acc[s]
        res[s] = dict(err=a['err'], ratio=a['ratio'], finite=a['finite'], special=_special(family, flavour, a['outs']))
    res['gate'] = acc[sides[0]]['gate']
    return res


def line(res):
    msg = f'{res["flavour"]:6s} {res["family"]:12s}'
    for s in ('kernel', 'emu'):
        if s in res:
            r = res[s]
            ex = '' if r['special'] is None else (' exact:ok' if r['special'] else ' exact:FAIL')
            msg += f' | {s} max|d| {r["err"]:.3e} = {r["ratio"]:.3f} of the gate{ex}{"" if r["finite"] else " NON-FINITE"}'
    return msg + f' | gate there {res["gate"]:.3e}'


if __name__ == '__main__':
    bad = 0
    for flavour in FLAVOURS:
        for family in FAMILIES:
            res = case(flavour, family)
            k = res['kernel']
            ok = k['finite'] and k['ratio'] <= 1.0 and k['special'] is not False
            bad += not ok
            print(f'[{"ok" if ok else "FAIL"}] ' + line(res), flush=True)
    sys.exit(1 if bad else 0)
