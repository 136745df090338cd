"""Host-side operator layer: torch tensors in, HIP kernels through the C ABI, torch tensors out.

Activations are fp32 channels-last tensors of shape (B, H, W, C) ("NHWC"); token matrices are (rows, cols).
PyTorch only provides device memory (torch.empty) and the current stream; every FLOP runs in
libcodeformer_hip.so.  Nothing here has a CPU/eager fallback.
"""
import ctypes
import math
import os
import weakref

import torch

from . import lib as L
from .lib import (EPI_AXPY, EPI_AXPY2, EPI_GELU, EPI_LEAKY, EPI_NONE, EPI_PRELU, EPI_RES_PRELU, EPI_RESIDUAL, EPI_SFT, PRO_AFFINE, PRO_AFFINE_SWISH,
                  PAD_EDGE, PAD_REFLECT, PAD_ZERO, PRO_LEAKY, PRO_NONE)

GN_GROUPS = 32
GN_EPS = 1e-6

# Optional per-launch timing for bench.py's roofline leg: when a list is installed here, conv2d brackets every
# kernel launch with events on the launch stream and appends (kind, algorithmic_flops, algorithmic_bytes, start, end).
PROFILE = None


def _f32(t):
    if t.dtype != torch.float32:
        raise TypeError(f'expected float32, got {t.dtype}')
    return t


def _act_dtype(t, what='activation'):
    """dtype of a conv activation: float32, or bfloat16 (bf16 STORAGE, cf_conv_desc.io_bf16 -- precision 'bf16' from 64x64 pixels up)."""
    if t.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f'{what}: expected float32 or bfloat16, got {t.dtype}')
    return t.dtype


# ---- state kept on tensor objects ---------------------------------------------------------------------------------------------------
# Three attributes travel on a tensor OBJECT from the launch that wrote it to the launches that read it: `_cf_stats` (GNStats: the GroupNorm
# partials of a conv epilogue), `_cf_act` (a cached range-scale table) and `_cf_act_pair` (the table of a concatenated pair, on its first
# member).  The contract (tests/test_gpu_tensor_state.py):
#   1. they describe the values the object holds NOW, or they are absent;
#   2. every ops.* call that writes into a caller-supplied tensor drops all three from that object, and from its `._base` where PyTorch
#      records one, before it attaches anything new -- after its own validation, so a refused call leaves the state alone;
#   3. state carries the STAMP of its tensor at attach and is ignored once the stamp has moved.  The stamp is (PyTorch's version counter,
#      the library's own write count of the tensor's storage): the first sees a user's y.mul_() / y.copy_() -- outside torch.inference_mode,
#      where tensors keep no counter and such a write cannot be seen --, the second sees the library's writes, which go through raw
#      pointers and never move the version.  The write count is what reaches the state of `buf` when a slice buf[..., a:b] is written
#      under inference_mode (inference tensors record no `._base`), of any other alias, and of a pair's second member;
#   4. the copies to_bf16 / select_rows make carry state of their own (their own stamp, the partials of copy time): rewriting the source
#      does not touch them.
_STATE_ATTRS = ('_cf_stats', '_cf_act', '_cf_act_pair')
_WRITE_EPOCH = {}    # storage address -> library writes into a caller-supplied destination there (a recycled address just goes on counting)


def tensor_version(t):
    """Version counter of a tensor, or None for inference tensors (torch.inference_mode), which do not track one -- reading
    `._version` there raises.  Callers skip their version-keyed caches for None."""
    return None if t.is_inference() else t._version


def tensor_stamp(t):
    """(version counter or None, library writes into t's storage): equal stamps <=> no write to t that the library can see."""
    return (tensor_version(t), _WRITE_EPOCH.get(t.untyped_storage().data_ptr(), 0) if _WRITE_EPOCH else 0)


def _drop_state(t):
    """Rule 2: `t` is about to be overwritten through its raw pointer.  Its state goes, its base's state goes, and whatever other object
    shares the storage finds its stamp moved."""
    for o in (t, t._base):
        if o is not None:
            for a in _STATE_ATTRS:
                o.__dict__.pop(a, None)
    p = t.untyped_storage().data_ptr()
    _WRITE_EPOCH[p] = _WRITE_EPOCH.get(p, 0) + 1


def live_stats(t):
    """t's `_cf_stats` if it still describes t (rule 3), else None.  Statistics without a stamp (attached by hand) are trusted."""
    st = getattr(t, '_cf_stats', None)
    if st is None:
        return None
    stamp = getattr(st, 'stamp', None)
    return st if stamp is None or stamp == tensor_stamp(t) else None


def to_bf16(x):
    """fp32 NHWC activation -> its bf16 copy (round to nearest even, cf_f32_to_bf16): the tensors that ENTER the bf16-storage part of the
    generator (the decoder feature in front of the first bf16 Upsample, the encoder taps of the fusion blocks).  The GroupNorm partials /
    range-scale table the producer attached travel with the copy: they were taken from the fp32 values, as the bf16 epilogues take theirs.
    State that no longer describes x (rule 3 above) is not copied; what is copied describes x at copy time and stays valid for the copy
    when x is rewritten afterwards (a rewrite takes fresh partials, it does not touch the ones the copy holds)."""
    if x.dtype == torch.bfloat16:
        return x
    _f32(x)
    if not x.is_contiguous() or x.numel() % 8:
        raise ValueError('to_bf16: expected a dense tensor with a multiple of 8 elements')
    y = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    L.check(L.load().cf_f32_to_bf16(L.ptr(x), x.numel(), L.ptr(y, dtype=torch.bfloat16), L.stream_ptr()), 'cf_f32_to_bf16')
    st = live_stats(x)
    if st is not None:
        y._cf_stats = GNStats(st.part, st.parts, st.cpg, tensor_stamp(y)) if isinstance(st, GNStats) else st
    cached = getattr(x, '_cf_act', None)
    if cached is not None and cached[0] == _act_key(x, cached[0][0]):
        key = _act_key(y, cached[0][0])
        if key is not None:
            y._cf_act = (key, cached[1])
    return y


class GNStats:
    """fp64 (sum, sumsq) partials of one NHWC tensor: [batch][channels/cpg][parts][2] (see cf_groupnorm_finalize).
    Produced by a conv epilogue (attached to the conv's output tensor as `._cf_stats`) or by the stand-alone pass.
    stamp: tensor_stamp() of the carrying tensor when the partials were attached (None: not attached to a tensor)."""

    __slots__ = ('part', 'parts', 'cpg', 'stamp')

    def __init__(self, part, parts, cpg, stamp=None):
        self.part, self.parts, self.cpg, self.stamp = part, parts, cpg, stamp


def select_rows(x, sel):
    """x.index_select(0, sel) for an activation of the network (sel: int64 indices on x's device; an index may repeat): the images `sel`
    names, as a batch of their own.  The GroupNorm partials the producing conv attached (`._cf_stats`, [image][group][part][2]) travel with
    their images, so the consumers of the selection compute per image exactly what they compute for the whole batch; a parked range-scale
    table is not carried -- act_scale() rebuilds it from those partials, per image.  The selection is a copy with partials of its own:
    they describe x at the time of the call and stay valid when x is rewritten; partials that no longer describe x are not carried."""
    y = x.index_select(0, sel)
    st = live_stats(x)
    if st is not None:
        y._cf_stats = GNStats(st.part.view(x.shape[0], -1).index_select(0, sel).reshape(-1), st.parts, st.cpg, tensor_stamp(y))
    return y


class PackedWeight:
    """A conv / linear weight in the kernel layout [tap][cin_pad/16][cout_pad][16] (+ bias).
    `bf16` is the operand code of cf_conv_desc.bf16_mfma: 0 / False fp32, 1 / True bf16, 2 IEEE half."""

    __slots__ = ('w', 'bias', 'cout', 'cin', 'taps', 'cout_pad', 'cin_pad', 'bf16', 'up2x', 'wino', 'scale', 's2', 'conv1', 'kparts')

    def __init__(self, w, bias, cout, cin, taps, cout_pad, cin_pad, bf16=False, up2x=False, wino=False, scale=1.0, s2=False, conv1=False, kparts=0):
        self.w, self.bias, self.cout, self.cin, self.taps = w, bias, cout, cin, taps
        self.kparts = kparts  # fp32 F(4,3) packing that runs the K-part form: cin / 128 parts (WF43K), else 0
        self.cout_pad, self.cin_pad, self.bf16, self.up2x, self.wino = cout_pad, cin_pad, bf16, up2x, wino
        self.s2 = s2         # f16x2 packing in the stride-2 (space-to-depth) form: only conv2d(stride=2) takes it
        self.conv1 = conv1   # f16x2 1x1 weight in the convolution kernel's layout (images of more than TOKEN_IMAGE_MAX pixels), not the token GEMM's
        self.scale = scale   # f16x2 packing: the power of two the weights were multiplied by (cf_conv_desc.acc_scale = 1 / scale)


def _cout_pad(cout):
    if cout <= 32:
        return 32
    if cout <= 64:
        return 64
    return (cout + 127) // 128 * 128


WINOGRAD = 3   # value of the operand-code argument that selects the Winograd F(2x2,3x3) fp32 evaluation
SPLIT = 4      # ... the split-half evaluation: fp32 operands as hi + lo IEEE halves, 3 f16 MFMAs per product (cf_split.hip)
WSPLIT = 6     # ... Winograd F(2x2,3x3) with split-half operands in the 16 transform-domain GEMMs (cf_winograd.hip, H2)
GSPLIT = 7     # ... a Linear / 1x1 weight for the split-half token GEMM (cf_gemm_split.hip)
WF16 = 8       # ... Winograd F(2x2,3x3) with SINGLE IEEE-half operands (eight-wave kernel of cf_wsplit.hip; precision 'fp16')
WBF16 = 9      # ... the same with single bf16 operands (precision 'bf16')
SPLIT_F43 = 10  # ... REQUEST: SPLIT, with Winograd F(4x4,3x3) where its kernel applies (~5x the error of F(2,3): generator / CFT layers, and the encoder behind its margin gate)
WF43 = 11      # ... Winograd F(4x4,3x3) with split-half operands (cf_wf43.hip; cf_conv_desc.winograd = 2)
WINOGRAD_F43 = 12   # ... REQUEST: WINOGRAD (exact fp32), with Winograd F(4x4,3x3) on fp32 operands where its kernel applies (generator / CFT only)
WF43F = 13     # ... Winograd F(4x4,3x3) with IEEE-fp32 operands (cf_wf43.hip on v_mfma_f32_16x16x4_f32; winograd = 2, operand fp32)
WF42U = 14     # ... nearest x2 + 3x3 as four Winograd F(4x4,2x2) sub-pixel phases with IEEE-fp32 operands (cf_wf43.hip; winograd = 2 + upsample)
WINOGRAD_F43K = 15  # ... REQUEST: WINOGRAD_F43, and the K-part form of the fp32 F(4,3) kernel on the 16x16 .. 32x32 layers it covers (f43k_ok)
WF43K = 16     # ... the WF43F packing, launched in K parts of 128 input channels + a sum-and-epilogue launch (cf_wf43.hip "KP", cf_ksum.hip)
F43_FP32_CODES = (WINOGRAD_F43, WINOGRAD_F43K)   # the requests for exact-fp32 operands with F(4,3) where it applies
OPERAND_F16X2 = 3   # enum cf_operand value behind SPLIT / WSPLIT / GSPLIT / WF43
SPLIT_CODES = (SPLIT, SPLIT_F43)   # requested codes that put un-normalised inputs / stride-2 / 1x1 layers on the split-half kernels


def split_ok(cin, cout, hin, win, c_split=None):
    """Shapes the split-half kernel covers (3x3 stride-1 dense NHWC, plain or folded upsample): 32-channel K slabs (also at a
    concat boundary), 64-wide channel tiles, whole 16x16 tiles of the conv's INPUT grid."""
    return cin % 32 == 0 and cout % 64 == 0 and hin % 16 == 0 and win % 16 == 0 and (c_split is None or c_split % 32 == 0)


def split_s2_ok(cin, cout, hin, win):
    """Shapes the split-half kernel covers at stride 2 (Downsample: one dense input, zero row / column bottom / right): 32-channel
    slabs of the space-to-depth view (2 * cin % 32 == 0), 64-wide channel tiles, whole 8x16 tiles of the OUTPUT grid."""
    return cin % 16 == 0 and cout % 64 == 0 and hin % 16 == 0 and win % 32 == 0


def split_1x1_ok(cin, cout, h, w, c_split=None):
    """1x1 convolutions the split-half kernel streams (ResBlock skips on images): 32-channel slabs, 64-wide channel tiles, 8x16 tiles."""
    return cin % 32 == 0 and cout % 64 == 0 and h % 8 == 0 and w % 16 == 0 and h * w > TOKEN_IMAGE_MAX and (c_split is None or c_split % 32 == 0)


def winograd_ok(cin, cout, hout, wout):
    """Shapes the Winograd kernel covers (3x3 stride-1 dense NHWC): whole 8x16 output patches, 64-wide channel tiles."""
    return cin % 16 == 0 and cout % 64 == 0 and hout % 8 == 0 and wout % 16 == 0


# Which layers a SPLIT_F43 / WINOGRAD_F43 request puts on the F(4x4,3x3) kernel: the shapes where it pays
# (profiles/r04_f43_per_shape.txt, r04_f43_fp32_check_time.txt, r04_latency_minpix.txt): every covered layer with 64 output channels (the
# 8-wave form, two workgroups per CU: x1.0-1.17 at sixteen faces) and the layers with a multiple of 128 output channels (the 16-wave form)
# from F43_WIDE_MIN_PIXELS up.  Split-half operands: 128x128 -- at 64x64 the form wins x1.11 at sixteen faces (0.15 ms of a 36 ms step) but a
# 64x64 image has 16 patches, and at one face per call its 9 launches cost 0.5 ms of 7.1 (140 -> 150 faces/s with the limit at 128x128);
# fp32 operands: 64x64 (x1.75 there: the fp32 MFMA work itself is the bound).  Below 64x64 the WHOLE-K form loses at any batch (x0.6 at 32x32: 4
# patches per image, a K chain of 8 - 16 slabs per workgroup); with fp32 operands those layers run the K-PART form instead (WINOGRAD_F43K ->
# f43k_ok below: x1.3 - 1.5 against F(2,3) on the three adopted classes at sixteen faces, 0.8 ms of the 45 ms step; at one face per call the
# fp32 forward is 8 % slower, 8.63 -> 9.33 ms -- the rule cannot follow the batch).
# The rule is a function of the per-image shape only: results do not depend on the batch.
F43_WIDE_MIN_PIXELS = 128 * 128        # smallest image of the 16-wave form, split-half operands
F43_WIDE_MIN_PIXELS_FP32 = 64 * 64     # ... fp32 operands


def f43_ok(cin, cout, hout, wout, fp32=False):
    """Shapes the F(4x4,3x3) kernel covers (3x3 stride-1 dense NHWC): whole 16x16 output patches, 64-wide channel tiles, at most 256
    input channels (512 in the 16-wave form on 32-channel slabs: the GroupNorm rows of an image sit in LDS) -- narrowed to where it
    pays (fp32: the operand type)."""
    if cout != 64 and (cout % 128 or hout * wout < (F43_WIDE_MIN_PIXELS_FP32 if fp32 else F43_WIDE_MIN_PIXELS)):
        return False
    cin_max = 512 if (cout % 128 == 0 and cin % 32 == 0) else 256     # GroupNorm rows in LDS: 512 in the 16-wave form on 32-channel slabs (round 6), else 256
    return cin % 16 == 0 and cin <= cin_max and cout % 64 == 0 and hout % 16 == 0 and wout % 16 == 0


F43K_MIN_WORKGROUPS = 16               # K-part form: fewest workgroups an image must give (256 CUs / 16 faces)


def f43k_ok(cin, cout, hout, wout, c_split=None):
    """Shapes a WINOGRAD_F43K request puts on the K-part form of the fp32 F(4x4,3x3) kernel (3x3 stride-1 dense NHWC): the 16x16 .. 32x32 layers
    with whole 128-channel parts on both sides.  An image of these sizes has 1 or 4 patches, too few workgroups for the whole-K form; one
    workgroup per (patch, 128 input channels, 128 output channels) fills the chip at sixteen faces and shortens the K chain to 4 slabs.  A
    function of the per-image shape only: the number of parts is cin / 128 whatever the batch.  (cin = 128 is one part: the whole-K form plus
    a pass over the output, so it stays where WINOGRAD_F43 puts it.)
    Narrowed to where the pair of launches measured shorter than the F(2,3) launch it replaces (sixteen faces, profiles/NOTES.md): an image must
    give at least F43K_MIN_WORKGROUPS (patch, part, channel block) workgroups, so that sixteen faces fill the 256 CUs in one round.  512 -> 512 @
    16x16 (16 per image: 117 -> 77 us), 256 -> 256 @ 32x32 (16: 91 -> 69 us) and 512 -> 256 @ 32x32 (32: 183 -> 130 us) pass; 256 -> 512 and
    512 -> 256 @ 16x16 (8 per image, half the chip: 59 -> 65 us and 70 -> 69 us, together longer) stay on F(2,3)."""
    return f43k_covers(cin, cout, hout, wout, c_split) and (hout // 16) * (wout // 16) * (cin // 128) * (cout // 128) >= F43K_MIN_WORKGROUPS


def f43k_covers(cin, cout, hout, wout, c_split=None):
    """Shapes a weight packed with bf16=WF43K can be launched on (the form itself; f43k_ok is the policy): 2 .. 4 whole parts of 128 input
    channels, 128-wide channel blocks, whole 16x16 patches, images of 16x16 up to (not including) 64x64 pixels, a concat boundary between parts."""
    return cout % 128 == 0 and cin % 128 == 0 and 256 <= cin <= 512 and hout % 16 == 0 and wout % 16 == 0 and 256 <= hout * wout < F43_WIDE_MIN_PIXELS_FP32 and \
        (c_split is None or c_split % 128 == 0)


# precision 'fp32': the Upsample blocks (nearest x2 + 3x3) as four Winograd F(4x4,2x2) sub-pixel phases on the fp32 F(4,3) kernel's stages
# (cf_wf43.hip: 25 transform-domain products per 16 outputs = 1.5625 per output) instead of the folded sub-pixel form on the direct fp32
# kernel, which executes every one of its 4 products per output (0.82 of the fp32 MFMA peak: nothing left to schedule).


def f43_up_ok(cin, cout, hout, wout):
    """Shapes the sub-pixel F(4x4,2x2) form of the fp32 Winograd kernel covers ((hout, wout) = the OUTPUT size): the 16-wave workgroup on
    32-channel slabs, at most 256 input channels, whole 16x16 blocks of the INPUT grid, from the size where the 16-wave form pays."""
    return cin % 32 == 0 and cin <= 256 and cout % 128 == 0 and hout % 32 == 0 and wout % 32 == 0 and \
        hout * wout >= F43_WIDE_MIN_PIXELS_FP32


# Smallest per-image input of the DIRECT split-half kernel and of the eight-wave Winograd kernel.  The 16x16 latents are below it: with
# SPLIT they run the four-wave Winograd kernel on split halves with split-K (conv_code -> WSPLIT: measured on the reference's crops
# before it became the default, profiles/r02_encoder_split_check.txt).
SPLIT_MIN_PIXELS = 32 * 32
TOKEN_IMAGE_MAX = 1024   # CF_TOKEN_IMAGE_MAX of cf_common.h: f16x2 1x1 layers on larger images run the streaming convolution kernel


def wsingle_ok(cin, cout, h, w):
    """Shapes the eight-wave Winograd kernel covers (the rule of cf_wsplit_covers): 128-wide channel tiles from 32x32 pixels up."""
    return winograd_ok(cin, cout, h, w) and cout % 128 == 0 and h * w >= SPLIT_MIN_PIXELS


def c_split_ok(c_split, slab):
    return c_split is None or c_split % slab == 0


def conv_code(code, cin, cout, h, w, up2x=False, c_split=None, plain=True):
    """Operand code a 3x3 stride-1 convolution really runs with, given the requested one and its shape ((h, w) = INPUT size).
    SPLIT falls back to WINOGRAD and WINOGRAD to the direct fp32 kernel where their kernels do not apply; the decision depends
    on the per-image shape only (never on the batch), so results stay batch-invariant."""
    code = int(code)
    f43_slab = 32 if (cout % 128 == 0 and cin % 32 == 0) else 16   # slab of the form cf_conv2d runs: a concat boundary must not cut one
    if code == WINOGRAD_F43K:
        if plain and not up2x and f43k_ok(cin, cout, h, w, c_split):
            return WF43K
        code = WINOGRAD_F43
    if code == WINOGRAD_F43:
        if plain and not up2x and c_split_ok(c_split, f43_slab) and f43_ok(cin, cout, h, w, fp32=True):
            return WF43F
        code = WINOGRAD
    if code == SPLIT_F43:
        if plain and not up2x and c_split_ok(c_split, f43_slab) and f43_ok(cin, cout, h, w):
            return WF43
        code = SPLIT
    if code == SPLIT:
        if plain and not up2x and winograd_ok(cin, cout, h, w):
            return WSPLIT
        if plain and split_ok(cin, cout, h, w, c_split) and (up2x or h * w >= SPLIT_MIN_PIXELS):   # (the folded upsample has no Winograd form: the direct split kernel beats the fp32 one from 16x16 up, tools/up16_probe.py)
            return SPLIT
        code = WINOGRAD
    if code == WINOGRAD:
        return WINOGRAD if (plain and not up2x and winograd_ok(cin, cout, h, w)) else 0
    if code and not (plain and cin % 32 == 0 and cout % 4 == 0):
        return 0
    if code in (1, 2) and plain and not up2x and wsingle_ok(cin, cout, h, w):
        # single 16-bit operands ('bf16' / 'fp16'): the eight-wave Winograd kernel where it covers the layer (one MFMA per
        # transform-domain product), else the direct 16-bit instantiations of cf_igemm.hip
        return WBF16 if code == 1 else WF16
    return code


# ---- range of the 16-bit MFMA operands --------------------------------------------------------------------------------------------
# An IEEE-half operand overflows above 65504 (16376 in the Winograd domain: the input transform sums four activations) and its lo half goes
# subnormal below 2^-3.  Weights are scaled into [2^14, 2^15) when they are packed.  Activations:
#   * inputs that pass a GroupNorm prologue are bounded by |gamma| * sqrt(n - 1) + |beta| (n = elements of a group); the arch modules check
#     that bound against HALF_LIMIT when they choose a layer's kernel (gn_range_ok) and fall back to exact fp32 where it fails;
#   * UN-NORMALISED inputs (the residual stream into Upsample.conv, the quantised feature, the CFT branch) get a per-image power-of-two
#     scale (act_scale -> cf_conv_desc.act_scale): exact, any fp32 magnitude.  CODEFORMER_HIP_RANGE_SCALE=0 switches it off (A/B only).
RANGE_SCALE = os.environ.get('CODEFORMER_HIP_RANGE_SCALE', '1') != '0'
HALF_LIMIT = 65504.0 / 4.0    # largest |activation| a Winograd-domain IEEE-half operand can carry


def switches():
    """The module-level switches a captured forward depends on (part of the graph-replay key of the arch modules)."""
    return (RANGE_SCALE, FINALIZE_FUSED)


def needs_act_scale(pw):
    """True when `pw` runs on a kernel with 16-bit MFMA operands that applies cf_conv_desc.act_scale."""
    if pw.conv1:
        return RANGE_SCALE
    return RANGE_SCALE and pw.taps == 9 and int(pw.bf16) in (1, 2, OPERAND_F16X2) and (bool(pw.wino) or int(pw.bf16) == OPERAND_F16X2)


_ACT_CELLS = {}
_RETIRED_SCRATCH = []   # replaced _act_cells / _counters tensors: a captured graph keeps their raw address and runs atomics on it for as long as it is replayed


def _scratch(table, device, n, floor):
    """n zero-initialised int32 words per (device, stream).  A tensor too small for a later caller is replaced by a larger one and kept
    allocated for the life of the process: the graphs that captured its address are not tracked."""
    key = (str(device), torch.cuda.current_stream(device).cuda_stream)
    t = table.get(key)
    if t is None or t.numel() < n:
        if t is not None:
            _RETIRED_SCRATCH.append(t)
        t = table[key] = torch.zeros(max(n, floor), dtype=torch.int32, device=device)
    return t


def _act_cells(device, batch):
    """2 * batch zero-initialised words per (device, stream) for cf_act_scale_fused; every launch leaves them at zero."""
    return _scratch(_ACT_CELLS, device, 2 * batch, 256)


def act_scale(x, x2=None, growth=4.0):
    """(B, 2) float32 table (s_b, 1 / s_b): power-of-two scale that puts growth * max|x_b| into [2^13, 2^14) -- from the statistics
    partials the producing conv wrote (no pass over x; the bound is loose by a few bits, which is harmless) or, for tensors without
    them, from x itself; one launch (cf_act_scale_fused).  x2: the second half of a concatenated input -- the table then covers both.
    Cached on the tensor under (growth, tensor_stamp(x)): one table serves every conv that reads the tensor; another growth factor, a
    write by this library (conv2d(out=x), also through a slice of x or into x as the second member of a parked pair) and, outside
    torch.inference_mode, a user's in-place write (x.mul_(), x.copy_()) get a fresh table -- and the partials such a write made stale are
    not used for it: the table then comes from x itself.  Under inference_mode a USER's in-place write cannot be seen (inference tensors
    keep no version counter): a tensor that carries statistics must not be written there except through this library."""
    key = _act_key(x, growth)
    # key is None for a user-held inference tensor (no version counter, no statistics attached): its table is computed on every call.  A
    # tensor that carries its producer's statistics is a conv2d output: keyed on the object and the library's own write count, one table
    # serves all its consumers under inference_mode too (else every consumer relaunched the kernel, and captured graphs baked that in).
    if x2 is None and key is not None:
        cached = getattr(x, '_cf_act', None)
        if cached is not None and cached[0] == key:
            return cached[1]
    if x2 is not None:      # a table groupnorm_tables([x, x2], act_growth=...) wrote in its own launch: valid while BOTH members are unwritten
        cached = getattr(x, '_cf_act_pair', None)
        if cached is not None and cached[2]() is x2 and cached[0] == key and cached[1] == _act_key(x2, growth):
            return cached[3]
    lib = L.load()
    B = x.shape[0]
    act = torch.empty(B, 2, dtype=torch.float32, device=x.device)
    cells = L.ptr(_act_cells(x.device, B), dtype=torch.int32)
    st = live_stats(x)
    st2 = None if x2 is None else live_stats(x2)
    if x2 is not None and (st is None or st2 is None):
        # a half without statistics partials: two single tables combined on the host side of the stream (rare: every conv that feeds a
        # concatenation writes partials)
        a1, a2 = act_scale(x, growth=growth), act_scale(x2, growth=growth)
        return torch.stack((torch.minimum(a1[:, 0], a2[:, 0]), torch.maximum(a1[:, 1], a2[:, 1])), dim=1)
    if st is not None:
        nper = st.part.numel() // (2 * B)
        p2, n2 = (L.ptr(st2.part, dtype=torch.float64), st2.part.numel() // (2 * B)) if st2 is not None else (None, 0)
        L.check(lib.cf_act_scale_fused(L.ptr(st.part, dtype=torch.float64), nper, p2, n2, None, 0, B, float(growth), cells, L.ptr(act), L.stream_ptr()),
                'cf_act_scale_fused')
    else:
        if not x.is_contiguous() or (x.numel() // B) % 4:
            raise ValueError('act_scale: expected a dense tensor with a multiple of 4 elements per image')
        L.check(lib.cf_act_scale_fused(None, 0, None, 0, L.ptr(_f32(x)), x.numel() // B, B, float(growth), cells, L.ptr(act), L.stream_ptr()),
                'cf_act_scale_fused')
    if x2 is None and key is not None:
        x._cf_act = (key, act)
    return act


class StatsPair:
    """Shared statistics buffer of TWO sibling convolutions of equal shape (the scale.0 / shift.0 convolutions of a fusion block,
    codeformer_arch.py:153-154): conv2d(..., stats_into=pair) places each launch's partials in one half, and act_scale_pair(pair, batch)
    turns both into their range-scale tables with ONE cf_act_scale_fused launch over 2 x batch "images"."""

    def __init__(self):
        self.buf, self.n, self.used = None, 0, 0

    def take(self, n, device):
        if self.buf is None:
            self.buf, self.n = torch.empty(2 * n, dtype=torch.float64, device=device), n
        if n != self.n or self.used >= 2:
            raise ValueError('StatsPair: two launches of equal statistics size')
        self.used += 1
        return self.buf[(self.used - 1) * n:self.used * n]


def act_scale_pair(pair, batch, growth=4.0):
    """((B, 2), (B, 2)) range-scale tables of the two tensors whose statistics share `pair` -- bitwise act_scale() of each, one launch."""
    if pair.used != 2:
        raise ValueError('act_scale_pair: the pair has not been filled by two launches')
    lib = L.load()
    act = torch.empty(2 * batch, 2, dtype=torch.float32, device=pair.buf.device)
    cells = L.ptr(_act_cells(pair.buf.device, 2 * batch), dtype=torch.int32)
    L.check(lib.cf_act_scale_fused(L.ptr(pair.buf, dtype=torch.float64), pair.n // (2 * batch), None, 0, None, 0, 2 * batch, float(growth), cells, L.ptr(act),
                                   L.stream_ptr()), 'cf_act_scale_fused')
    return act[:batch], act[batch:]


def gn_range_ok(gmax, bmax, n):
    """GroupNorm output bound |gamma| * sqrt(n - 1) + |beta| (n elements per group) against the IEEE-half operand range."""
    return gmax * math.sqrt(max(n - 1, 1)) + bmax < HALF_LIMIT


def exact_code(code):
    """Operand code of the exact-fp32 evaluation that replaces a 16-bit-operand code (range fallback); bf16 has fp32's exponent."""
    code = int(code)
    return {SPLIT: WINOGRAD, SPLIT_F43: WINOGRAD, 2: WINOGRAD}.get(code, code)


def pack_scale(wmax):
    """The power of two a split-half packing multiplies its weights by: max|w * scale| lands in [2^14, 2^15), the top binade of IEEE half
    below its largest finite value, so the lo halves of the largest weights are normal numbers.  ONE scale per matrix: a weight of less
    than 2^-3 / scale (2^-17 .. 2^-18 of the largest) has a subnormal lo half, one below 2^-14 / scale a subnormal hi half.  1.0 for an
    all-zero or non-finite matrix."""
    return 1.0 if wmax == 0.0 or not math.isfinite(wmax) else 2.0 ** (14 - math.frexp(wmax)[1] + 1)


# The weight-side Winograd matrices (what cf_pack.hip evaluates in fp64): G of F(2x2,3x3); G' = D^-1 G of F(4x4,3x3) for the points (0, +-1/2, +-2, inf),
# the matrix cf_wf43.hip documents; G42 of the sub-pixel F(4x4,2x2) form below.
G23 = ((1.0, 0.0, 0.0), (0.5, 0.5, 0.5), (0.5, -0.5, 0.5), (0.0, 0.0, 1.0))
G43 = ((4.0, 0.0, 0.0), (-32 / 15, -16 / 15, -8 / 15), (-32 / 15, 16 / 15, -8 / 15), (1 / 15, 2 / 15, 4 / 15), (1 / 15, -2 / 15, 4 / 15), (0.0, 0.0, 4.0))
G42 = ((1.0, 0.0), (-2 / 9, 2 / 9), (-8 / 9, -4 / 9), (1 / 9, 2 / 9), (0.0, 1.0))


def _domain_max(w, G):
    """max |G g G^T| over a (cout, cin, 3, 3) weight in fp64: every position in one tensor, ONE reduction / host read-back per weight."""
    Gm = torch.tensor(G, dtype=torch.float64, device=w.device)
    return float(torch.einsum('xa,kcab,yb->kcxy', Gm, w.double(), Gm).abs().max())


def _f23_max(w):
    return _domain_max(w, G23)


def _f43_max(w):
    return _domain_max(w, G43)


# Winograd F(4,2) for the sub-pixel phases of nearest x2 + 3x3 (conv2d(upsample=True) in precision 'fp32'): output parity a along an axis is the
# 2-tap correlation [g0, g1 + g2] of rows i - 1, i (a = 0) or [g0 + g1, g2] of rows i, i + 1 (a = 1) of the low-resolution image, and
#   Y = A42^T [ (G42 g_p G42^T) (.) (B42^T d B42) ] A42      d: 5x5 window, g_p: the folded 2x2 kernel of phase p, Y: 4x4 outputs of that phase
# with the interpolation points (0, -1, 1/2, 2, inf): of the twelve sets tools/winograd_f42_numerics.py compares (0, +-1 / +-1/2 / +-2 with a
# fourth point, and the mixed sets) the one with the smallest fp64-measured error of the fp32 pipeline -- 128 channels, 16x16 -> 32x32, |out| <=
# 6.65: max 1.90e-5, mean 7.7e-7 (its mirror (0, 1, -1/2, -2) measures the same), against max 2.69e-5, mean 1.25e-6 of F(4x4,3x3) on the
# upsampled image and mean 1.2e-6 of the symmetric sets (0, +-1, x).  Every entry of B42^T and A42^T is exact in fp32, so no row scaling is needed.
B42T = ((1.0, -1.5, -1.5, 1.0, 0.0), (0.0, 1.0, -2.5, 1.0, 0.0), (0.0, -2.0, -1.0, 1.0, 0.0), (0.0, -0.5, 0.5, 1.0, 0.0), (0.0, 1.0, -1.5, -1.5, 1.0))
A42T = ((1.0, 1.0, 1.0, 1.0, 0.0), (0.0, -1.0, 0.5, 2.0, 0.0), (0.0, 1.0, 0.25, 4.0, 0.0), (0.0, -1.0, 0.125, 8.0, 1.0))


def fold_phase_taps(w, a, b):
    """(.., 3, 3) -> (.., 2, 2): the taps output parity (a, b) of nearest x2 + 3x3 sees on the low-resolution image (in w's dtype; fp64 for packing)."""
    def fold(t, p, dim):
        g0, g1, g2 = t.unbind(dim)
        return torch.stack((g0, g1 + g2) if p == 0 else (g0 + g1, g2), dim)
    return fold(fold(w, a, -2), b, -1)


def f42_weights(w):
    """(cout, cin, 3, 3) -> (4 phases p = 2a + b, cout, cin, 5, 5) fp64: G42 g_p G42^T, what cf_pack_conv_weight_winograd42_up evaluates and rounds once."""
    G = torch.tensor(G42, dtype=torch.float64, device=w.device)
    return torch.stack([torch.einsum('xa,kcab,yb->kcxy', G, fold_phase_taps(w.double(), p >> 1, p & 1), G) for p in range(4)])


def _require_3x3(w, cin_mult, cout_mult, what, up2x):
    """The shape rule of the 3x3 layouts: whole K slabs and channel tiles; up2x is refused (pass False for a layout with a folded form)."""
    if up2x or w.dim() != 4 or tuple(w.shape[2:]) != (3, 3) or w.shape[1] % cin_mult or w.shape[0] % cout_mult:
        raise ValueError(f'{what} packing needs a 3x3 weight with cin % {cin_mult} == 0 and cout % {cout_mult} == 0 (and has no up2x form)')


def _packed(name, n, w, *args, dtype=torch.float32):
    """An n-element buffer that the C packer `name`(w, *args, buffer, stream) fills."""
    packed = torch.empty(n, dtype=dtype, device=w.device)
    L.check(getattr(L.load(), name)(L.ptr(w), *args, L.ptr(packed, dtype=None), L.stream_ptr()), name)
    return packed


# One packer per layout: (w contiguous fp32, bias, code, up2x, stride2) -> PackedWeight.  The Winograd-domain layouts differ in this row only:
# code -> (name in messages, C packer, transform-domain positions, domain maximum (None: fp32 operands, no scale), operand, wino)
_WINO = {WINOGRAD: ('winograd', 'cf_pack_conv_weight_winograd', 16, None, False, True),
         WSPLIT: ('winograd f16x2', 'cf_pack_conv_weight_winograd_f16x2', 16, _f23_max, OPERAND_F16X2, True),
         WF16: ('winograd f16x2', 'cf_pack_conv_weight_winograd_f16x2', 16, _f23_max, 2, True),   # (reads the hi slot)
         WBF16: ('winograd f16x2', 'cf_pack_conv_weight_winograd_bf16', 16, _f23_max, 1, True),
         WF43F: ('winograd F(4,3)', 'cf_pack_conv_weight_winograd43', 36, None, False, 2),
         WF43K: ('winograd F(4,3) K parts', 'cf_pack_conv_weight_winograd43', 36, None, False, 2),   # (the WF43F packing; PackedWeight.kparts selects the launch form)
         WF42U: ('winograd F(4,2) sub-pixel', 'cf_pack_conv_weight_winograd42_up', 100, None, False, 2),   # (4 phases x 25 positions)
         WF43: ('winograd F(4,3) f16x2', 'cf_pack_conv_weight_winograd43_f16x2', 36, _f43_max, OPERAND_F16X2, 2)}


def _pack_winograd(w, b, code, up2x, stride2):
    what, fn, npos, domain_max, operand, wino = _WINO[code]
    up = code == WF42U
    kp = code == WF43K
    _require_3x3(w, 128 if kp else 32 if up else 16, 128 if (up or kp) else 64, what, up2x)
    cout, cin = w.shape[:2]
    if kp and not 256 <= cin <= 512:
        raise ValueError(f'{what} packing needs 2 .. 4 parts of 128 input channels (got cin {cin})')
    scale = () if domain_max is None else (pack_scale(domain_max(w)),)
    return PackedWeight(_packed(fn, npos * cin * cout, w, cout, cin, cout, cin, *scale), b, cout, cin, 9, cout, cin, bf16=operand, up2x=up, wino=wino, scale=(*scale, 1.0)[0],
                        kparts=cin // 128 if kp else 0)


def _pack_split(w, b, code, up2x, stride2):
    """Split-half convolution kernel, form 0 plain 3x3 / 1 folded upsample / 2 stride 2 (a 2x2 convolution of the space-to-depth input) / 3 streaming 1x1 on images."""
    cout, cin, conv1 = w.shape[0], w.shape[1], w.dim() == 2 or tuple(w.shape[2:]) == (1, 1)
    if conv1 and (up2x or cin % 32 or cout % 64):
        raise ValueError('f16x2 1x1 packing needs cin % 32 == 0 and cout % 64 == 0')
    if not conv1:
        _require_3x3(w, 16 if stride2 else 32, 64, 'f16x2', False)
    form = 3 if conv1 else 2 if stride2 else int(bool(up2x))
    scale = pack_scale(float(w.abs().max()) * (4.0 if up2x else 1.0))   # (folded taps: at most 4 summed)
    packed = _packed('cf_pack_conv_weight_f16x2', (9, 16, 16, 1)[form] * cin * cout, w, cout, cin, form, cout, cin, scale)
    return PackedWeight(packed, b, cout, cin, 1 if conv1 else 9, cout, cin, bf16=OPERAND_F16X2, up2x=bool(up2x), scale=scale, s2=bool(stride2) and not conv1, conv1=conv1)


def _pack_gemm_split(w, b, code, up2x, stride2):
    cout, cin = w.shape[:2]
    w2 = w.reshape(cout, cin)
    if w.dim() not in (2, 4) or w.numel() != cout * cin or cout % 64 or cin % 128:
        raise ValueError('f16x2 GEMM packing needs a Linear / 1x1 weight with cout % 64 == 0 and cin % 128 == 0')
    scale = pack_scale(float(w2.abs().max()))
    return PackedWeight(_packed('cf_pack_linear_weight_f16x2', cout * cin, w2, cout, cin, scale), b, cout, cin, 1, cout, cin, bf16=OPERAND_F16X2, scale=scale)


def _pack_plain(w, b, code, up2x, stride2):
    if w.dim() not in (2, 4):
        raise ValueError('weight must be 2-D or 4-D')
    if w.dim() == 4 and (w.shape[2] != w.shape[3] or w.shape[2] not in (1, 3)):
        raise ValueError(f'unsupported kernel size {tuple(w.shape[2:])}')
    cout, cin, taps = w.shape[0], w.shape[1], 1 if w.dim() == 2 else w.shape[2] * w.shape[3]
    cout_pad, cin_pad = _cout_pad(cout), (cin + 15) // 16 * 16
    packed = _packed('cf_pack_conv_weight', L.load().cf_packed_weight_elems(cin_pad, taps, cout_pad), w, cout, cin, taps, cout_pad, cin_pad)
    return PackedWeight(packed, b, cout, cin, taps, cout_pad, cin_pad)


def _pack_16_or_folded(w, b, code, up2x, stride2):
    """bf16 / IEEE-half operands and the folded upsample (of any of the three operand types): 3x3 convs whose channels fill whole K slabs."""
    cout, cin, slab = w.shape[0], w.shape[1], 32 if code else 16
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3) or cin % slab:
        raise ValueError(f"{('fp32', 'bf16', 'f16')[code]}{' up2x' if up2x else ''} packing needs a 3x3 weight with cin % {slab} == 0")
    # bf16 kernels and every upsample kernel have N tiles of at least 64; the f16 general instantiation also has a 32-wide one
    cout_pad = _cout_pad(cout) if (code == 2 and not up2x) else max(64, _cout_pad(cout))
    name = 'cf_pack_conv_weight' + ('_up2x' if up2x else '') + ('', '_bf16', '_f16')[code]
    packed = _packed(name, (16 if up2x else 9) * cin * cout_pad, w, cout, cin, *(() if up2x else (9,)), cout_pad, cin, dtype=(torch.float32, torch.bfloat16, torch.float16)[code])
    return PackedWeight(packed, b, cout, cin, 9, cout_pad, cin, bf16=code, up2x=bool(up2x))


def pack_weight(weight, bias=None, bf16=False, up2x=False, f16=False, stride2=False):
    """weight: (cout, cin, 3, 3) | (cout, cin, 1, 1) | (cout, cin) CUDA fp32 -> PackedWeight.
    bf16=True (3x3 only, cin % 32 == 0): bf16 operands for the v_mfma_f32_32x32x16_bf16 path of cf_conv2d.
    f16=True (3x3 only, cin % 32 == 0): IEEE-half operands (general instantiations; RRDBNet's half mode).
    up2x=True (3x3 only): taps folded for conv2d(upsample=True) -- nearest x2 + 3x3 as four 2x2 sub-pixel convolutions.
    stride2=True (code SPLIT only): the stride-2 form of the split-half kernel -- a 2x2 convolution of the space-to-depth input."""
    code = 2 if f16 else int(bf16)   # callers may pass the operand code (0 fp32 / 1 bf16 / 2 f16 / 3 winograd) through `bf16`
    w = _f32(weight.detach()).contiguous()
    b = None if bias is None else _f32(bias.detach()).contiguous().clone()
    if stride2 and (code != SPLIT or up2x) and code != GSPLIT and code not in _WINO:   # (those two never looked at the flag)
        raise ValueError('stride2 packing exists for the split-half kernel (bf16=SPLIT) only')
    packer = _pack_gemm_split if code == GSPLIT else _pack_winograd if code in _WINO else _pack_split if code == SPLIT else \
        _pack_16_or_folded if (code or up2x) else _pack_plain
    return packer(w, b, code, up2x, stride2)


def pack_weight_cat(weights, biases):
    """Row-concatenate several (cout_i, cin[,1,1]) weights into one GEMM (e.g. q|k|v)."""
    w = torch.cat([x.detach().reshape(x.shape[0], x.shape[1]) for x in weights], dim=0)
    b = None if biases is None else torch.cat([x.detach() for x in biases], dim=0)
    return pack_weight(w, b)


def _nhwc_ld(t, what):
    """Channel stride (floats per pixel) of an NHWC tensor that is dense or a channel slice `buf[..., a:b]` of a dense one."""
    B, H, W, C = t.shape
    ld = t.stride(2) if W > 1 else (t.stride(1) if H > 1 else max(C, t.stride(0) // max(H * W, 1)))
    ok = t.stride(3) == 1 and ld >= C and (W == 1 or t.stride(2) == ld) and (H == 1 or t.stride(1) == W * ld) and \
        (B == 1 or t.stride(0) == H * W * ld)
    if not ok:
        raise ValueError(f'{what}: expected a dense NHWC tensor or a channel slice of one, got shape {tuple(t.shape)} '
                         f'strides {t.stride()}')
    return ld


# Split-K (cf_conv_desc.split_k) for 1x1 / Linear layers on small token images: WHETHER a layer takes the split-K kernel (64x64
# tiles, K cut into virtual chunks of 128 added in a fixed order) depends on its per-image shape only, so a face's bits are the same
# alone and inside any batch; HOW MANY workgroups then share a tile's chunks is chosen from the number of tiles in flight and does
# not change the result (see cf_common.h).  SPLITK_MAX = largest split count.
SPLITK_MAX = 8
SPLITK_IN_WORKGROUP = -1    # CF_SPLITK_IN_WORKGROUP of the header (ABI v21): split-half token GEMMs of one to a few faces
# Token GEMMs (split-half operands) of at most this many OUTPUTS (rows x columns) take the in-workgroup split: one to four faces (256 tokens
# each) for every layer, eight faces for the 512-column layers.  Measured per launch inside a captured graph (tools/gemm_chunk_probe.py):
# 256 x 512 x 512: 5.6 us against 15.0 (cross-workgroup split), 1024 x 512 x 1024: 13.9 / 17.2, 2048 x 1024 x 512: 22.3 / 30.2 -- and 4096 x 512 x
# 1024: 34.1 against 26.7 for the token-tile kernel, which keeps the large launches.  In the network (tools/latency.py, graph replay, one
# box): one face 6.71 -> 6.35 ms, two 8.34 -> 7.93, four 11.66 -> 11.38.
GEMM_IN_WG_MAX_OUTPUTS = 1 << 20
_COUNTERS = {}


def splitk_for(pw, ho, wo, cin, batch=1):
    """Split count for a 1x1 / Linear or a Winograd 3x3 on `batch` images of ho x wo pixels; 0: the layer is not a split-K layer."""
    if (pw.bf16 and not pw.wino and pw.taps != 1) or ho * wo > 1024 or cin % 128:
        return 0
    if pw.wino == 2:
        return 0   # (F(4x4,3x3) has no split-K form)
    if pw.wino:
        if ho % 8 or wo % 16 or ho * wo > 256:   # the 16x16 latents only: from 32x32 up a batch fills the CUs without splitting
            return 0
        tiles = batch * (ho // 8) * (wo // 16) * (pw.cout_pad // 64)
    elif pw.taps == 1 and (ho * wo) % 64 == 0 and pw.cout_pad % 64 == 0:
        if int(pw.bf16) == OPERAND_F16X2 and not pw.conv1 and batch * ho * wo * pw.cout_pad <= GEMM_IN_WG_MAX_OUTPUTS and cin <= 1024:
            return SPLITK_IN_WORKGROUP   # few tokens: the chunks of a 32x32 tile shared by the waves of one workgroup (cf_gemm_split.hip: same bits)
        tiles = batch * (ho * wo // 64) * (pw.cout_pad // 64)
    else:
        return 0
    # Workgroups a split launch may occupy (tools/sk_probe2.py, MI355X): the four-wave Winograd kernel runs two workgroups per CU, but
    # a second round of chain + finish costs more than the shorter chain saves (16 faces: 1 workgroup per tile 73 us, 2 -> 99 us);
    # the Linear kernel's finish outweighs its short K chain beyond 128 workgroups (8 faces, 512 -> 512: 1 -> 21 us, 2 -> 34 us).
    cap = 256 if pw.wino else 128
    v = cin // 128
    for ns in (8, 4, 2):
        if ns <= SPLITK_MAX and v % ns == 0 and tiles * ns <= cap:
            return ns
    return 1


def _counters(device, n):
    """n zero-initialised tile counters per (device, stream); every split-K launch leaves its counters at zero again."""
    return _scratch(_COUNTERS, device, n, 4096)


_KPART_WS = {}


def _kpart_ws(device, n):
    """n words per (device, stream) for the partial sums of a K-part F(4,3) launch (conv2d, pw.kparts): written by its first launch and read by its
    second, so every such layer of a stream shares one buffer.  The retired-scratch rule of _scratch holds: a captured graph keeps the raw address,
    so a buffer that a larger layer replaces stays allocated for the life of the process."""
    return _scratch(_KPART_WS, device, n, 1 << 22)


def _roofline_kind(pw, io, stride, upsample, c0, in_nchw, out_nchw, out_pixels, split_k):
    """The name bench.py's roofline leg books a conv2d launch under."""
    kind = ('conv3x3_s2' if stride == 2 else ('conv_up2x' if upsample else ('conv3x3_wino' if pw.wino else 'conv3x3'))) if pw.taps == 9 else 'gemm1x1'
    if pw.taps == 9 and stride == 1 and ((in_nchw and c0 <= 4) or (out_nchw and pw.cout <= 4)):
        kind = 'conv3x3_io'   # the network's first / last conv: vector-ALU kernels, HBM-bound (conv3x3_few_cin / few_cout)
    if pw.bf16:
        kind += ('', '_bf16', '_f16', '_f16x2')[int(pw.bf16)]
    if io == torch.bfloat16 and not pw.bf16:
        kind += '_bf16io'     # fp32 operands on bf16 tensors (the 1x1 skips and the RGB head of the bf16 mode)
    if pw.conv1:
        kind = 'conv1x1_stream_f16x2'   # 1x1 on images through the split-half convolution kernel (HBM-bound), not the token GEMM
    if pw.wino == 2:
        return 'conv3x3_wino43_f16x2' if pw.bf16 else 'conv3x3_wino43'   # F(4x4,3x3) on split halves / on fp32 operands (cf_wf43.hip)
    # the eight-wave 128-channel kernel (cf_wsplit.hip; the rule of cf_wsplit_covers)
    return kind + ('_8w' if pw.wino and pw.bf16 and pw.cout % 128 == 0 and out_pixels >= 1024 and not split_k else '')


def conv2d(x, pw, *, x2=None, stride=1, upsample=False, prologue=PRO_NONE, scale=None, shift=None,
           epilogue=EPI_NONE, res=None, sft_scale=None, sft_w=0.0, in_nchw=False, out_nchw=False, emit_stats=False,
           out=None, pad_mode=PAD_ZERO, pad_lo=0, split_k=None, act=None, x_alt=None, alt_from=0, stats_into=None,
           img_in=None, img_out=None):
    """Implicit-GEMM conv (3x3 / 1x1).  x: (B,H,W,C0) [x2: (B,H,W,C1) concatenated after x]; returns (B,Ho,Wo,cout)
    (or (B,cout,Ho,Wo) when out_nchw).  With in_nchw, x is (B,C<=4,H,W).
    emit_stats: also write the GroupNorm(32) partial statistics of the output in the epilogue and attach them to the
    returned tensor (`._cf_stats`), so a following groupnorm_tables() does not re-read the tensor.
    x, x2 and `out` (optional destination) may be channel slices `buf[..., a:b]` of wider NHWC buffers -- the dense-block
    pattern of RRDBNet, where torch.cat never materialises; res / sft_scale (= res2 of EPI_AXPY2) then share out's stride.
    A caller-supplied destination (`out`, `img_out` -- the only destination arguments of this module that take an activation) loses what
    earlier launches left on it: `_cf_stats`, `_cf_act` and `_cf_act_pair` are dropped from the object and from its `._base`, and the
    write is counted against its storage (tensor_stamp), so state held by any other object on that memory -- the buffer behind a slice
    under torch.inference_mode, the first member of a pair parked by groupnorm_tables -- is ignored from then on.  That happens once every
    check of this function has passed: a call refused with ValueError / TypeError leaves the state alone.  Statistics attached here
    carry the stamp of `out`; outside inference_mode a later in-place write by the caller (y.mul_(), y.copy_()) retires them, under
    inference_mode such a write cannot be seen.
    EPI_AXPY / EPI_AXPY2 / EPI_PRELU / EPI_RES_PRELU use sft_w as alpha (see cf_epilogue in the header; EPI_LEAKY's slope is the constant 0.2).
    sft_w with EPI_SFT: a float, or a contiguous float32 tensor of B values on x's device -- one weight per image (cf_conv2d_sft_w); image b
    is then bitwise the launch on that image alone with sft_w = float(sft_w[b]).
    pad_mode: PAD_ZERO, PAD_REFLECT (ReflectionPad2d(1) + unpadded 3x3) or PAD_EDGE (with upsample: reflection padding of the
    upsampled image); pad_lo=1 with stride 2: one padded row / column on every side instead of right / bottom only, at any
    input size (Ho = (H + 1) // 2: nn.Conv2d(3, 2, 1)); pad_lo=0 needs even H and W.
    act: (B, 2) range-scale table of an un-normalised input (act_scale(x)); dropped when the layer's kernel has fp32 operands.
    stats_into: a StatsPair -- the statistics partials of this launch go into its shared buffer (two sibling convolutions whose range-scale
    tables are then ONE launch: act_scale_pair).
    x_alt / alt_from (split-half token GEMMs only): output columns >= alt_from read their rows from x_alt (same shape as x) -- two Linear
    layers on two token matrices in one launch (q|k on LN(x) + pos, v on LN(x)).
    img_in / img_out (cf_conv2d_u8): the uint8 (B,H,W,3) BGR image at one end of the network.  img_in stands for x (pass x=None): the
    launch is the in_nchw one on img_u8_to_tensor(img_in), bitwise, statistics included.  img_out is the destination and is returned:
    the bytes tensor_to_img_u8 makes of the out_nchw launch's planes.  Both are contiguous CUDA tensors; any other dtype is refused."""
    lib = L.load()
    u8_in = u8_out = None
    if img_in is not None and img_out is not None:
        raise ValueError('conv2d: img_in and img_out belong to two different layers (the first and the last conv)')
    for t, what in ((img_in, 'img_in'), (img_out, 'img_out')):
        if t is not None and (t.dim() != 4 or t.shape[3] != 3):
            raise ValueError(f'{what}: expected a uint8 (B,H,W,3) BGR image, got shape {tuple(t.shape)}')
    if img_in is not None:
        if x is not None or not in_nchw:
            raise ValueError('img_in stands for the NCHW input: pass x=None and in_nchw=True')
        u8_in = L.ptr(img_in, dtype=torch.uint8)
        B, H, W, c0 = img_in.shape
        io, ld0, dev = torch.float32, 0, img_in.device
    elif in_nchw:
        io, dev = _act_dtype(x, 'x'), x.device
        _f32(x)
        B, c0, H, W = x.shape
        ld0 = 0
        if not x.is_contiguous():
            raise ValueError('in_nchw input must be contiguous')
    else:
        io, dev = _act_dtype(x, 'x'), x.device            # float32, or bfloat16 = bf16 storage of every activation of the launch (io_bf16)
        B, H, W, c0 = x.shape
        ld0 = _nhwc_ld(x, 'x')
    c1 = ld1 = 0
    if x2 is not None:
        if img_in is not None or x2.shape[:3] != x.shape[:3]:
            raise ValueError('x2 spatial shape mismatch')
        c1 = x2.shape[3]
        if x2.dtype != io:
            raise TypeError(f'x2 is {x2.dtype}, x is {io}: both halves of a concatenated input share the storage type (ops.to_bf16)')
        ld1 = _nhwc_ld(x2, 'x2')
    if c0 + c1 != pw.cin and not (c1 == 0 and c0 == pw.cin_pad):
        raise ValueError(f'input channels {c0}+{c1} != weight cin {pw.cin}')
    f43_up = bool(upsample) and pw.wino == 2 and not pw.bf16 and not pw.up2x   # a PLAIN fp32 F(4,3) packing (WF43F): F(4,3) on the upsampled image through the upsampling gather
    f42_up = bool(upsample) and pw.wino == 2 and not pw.bf16 and bool(pw.up2x)  # the WF42U packing: four F(4,2) sub-pixel phases (what the network runs)
    if bool(upsample) != bool(pw.up2x) and not f43_up:
        raise ValueError('conv2d(upsample=True) needs a weight packed with up2x=True, or the fp32 F(4,3) / F(4,2) sub-pixel packing (and vice versa)')
    if pw.taps == 1 and int(pw.bf16) == OPERAND_F16X2 and bool(pw.conv1) != (H * W > TOKEN_IMAGE_MAX):
        raise ValueError(f'1x1 with f16x2 operands: images of more than {TOKEN_IMAGE_MAX} pixels take a weight packed with bf16=SPLIT, '
                         'token matrices one packed with bf16=GSPLIT')
    if bool(pw.s2) != (stride == 2 and int(pw.bf16) == OPERAND_F16X2):
        raise ValueError('a weight packed with stride2=True serves conv2d(stride=2) only (and f16x2 operands at stride 2 need it)')
    if stride == 2:
        Ho, Wo = ((H + 1) // 2, (W + 1) // 2) if pad_lo == 1 else (H // 2, W // 2)   # (pad_lo 1: nn.Conv2d(3, 2, 1) at any size; pad_lo 0 needs even sizes)
    else:
        Ho, Wo = (H * 2, W * 2) if upsample else (H, W)
    shape = (B, pw.cout, Ho, Wo) if out_nchw else (B, Ho, Wo, pw.cout)
    ldo = 0
    odt = torch.float32 if out_nchw else io      # (the NCHW network output stays fp32)
    caller_out = out is not None or img_out is not None
    if img_out is not None:
        if not out_nchw or out is not None or tuple(img_out.shape) != (B, Ho, Wo, pw.cout) or img_out.device != dev:
            raise ValueError(f'img_out stands for the NCHW output: pass out_nchw=True, no out, and a uint8 {(B, Ho, Wo, 3)} image on {dev}')
        u8_out = L.ptr(img_out, dtype=torch.uint8)
        out = img_out
    elif out is None:
        out = torch.empty(shape, dtype=odt, device=dev)
    else:
        if tuple(out.shape) != shape or out.dtype != odt or out.device != dev:
            raise ValueError(f'out: expected {odt} {shape} on {dev}')
        if out_nchw:
            if not out.is_contiguous():
                raise ValueError('out_nchw destination must be contiguous')
        else:
            ldo = _nhwc_ld(out, 'out')
    for t in (res, sft_scale):
        if t is not None and tuple(t.shape) != (B, Ho, Wo, pw.cout):
            raise ValueError(f'epilogue operand shape {tuple(t.shape)} != {(B, Ho, Wo, pw.cout)}')
        if t is not None and t.dtype != io:
            raise TypeError(f'epilogue operand is {t.dtype}, the launch stores {io}')
        if t is not None and _nhwc_ld(t, 'epilogue operand') != (ldo or pw.cout):
            raise ValueError('epilogue operands must have the channel stride of the output')
    for t in (scale, shift):
        if t is not None and tuple(t.shape) != (B, c0 + c1):
            raise ValueError(f'prologue table shape {tuple(t.shape)} != {(B, c0 + c1)}')
    w_img = None
    if torch.is_tensor(sft_w):
        if epilogue != EPI_SFT or u8_in is not None or u8_out is not None:
            raise ValueError('sft_w: a tensor (one weight per image) belongs to epilogue=EPI_SFT; the other epilogues take a float')
        if sft_w.dtype != torch.float32:
            raise TypeError(f'sft_w: expected a float32 tensor of {B} values, got {sft_w.dtype}')
        if sft_w.dim() != 1 or sft_w.shape[0] != B or sft_w.device != dev:
            raise ValueError(f'sft_w: expected {B} values (one per image) on {dev}, got shape {tuple(sft_w.shape)} on {sft_w.device}')
        w_img, sft_w = L.ptr(sft_w), 0.0
    d = L.ConvDesc(
        in0=None if img_in is not None else L.ptr(x, not in_nchw, dtype=io), in1=L.ptr(x2, True, dtype=io), c0=c0, c1=c1, batch=B, hin=H, win=W, hout=Ho, wout=Wo, cout=pw.cout,
        cout_pad=pw.cout_pad, taps=pw.taps, stride=stride, upsample=2 if f42_up else int(bool(upsample)), in_nchw=int(bool(in_nchw)),
        out_nchw=int(bool(out_nchw)), prologue=prologue, epilogue=epilogue, pro_scale=L.ptr(scale),
        pro_shift=L.ptr(shift), weight=L.ptr(pw.w, dtype=None), bias=L.ptr(pw.bias), res=L.ptr(res, True, dtype=io),
        sft_scale=L.ptr(sft_scale, True, dtype=io), sft_w=float(sft_w), out=None if img_out is not None else L.ptr(out, not out_nchw, dtype=odt), bf16_mfma=int(pw.bf16),
        ld_in0=ld0, ld_in1=ld1, ld_out=ldo, pad_mode=int(pad_mode), pad_lo=int(pad_lo), winograd=int(pw.wino),
        acc_scale=1.0 / pw.scale, io_bf16=int(io == torch.bfloat16))
    if x_alt is not None:
        if tuple(x_alt.shape) != tuple(x.shape) or x_alt.dtype != torch.float32 or int(pw.bf16) != OPERAND_F16X2 or pw.taps != 1 or pw.conv1 or x2 is not None:
            raise ValueError('x_alt: a second float32 token matrix of the same shape, for a split-half token GEMM (bf16=GSPLIT weight)')
        d.in0_alt, d.alt_cout0 = L.ptr(x_alt), int(alt_from)
    if act is not None and needs_act_scale(pw):
        if tuple(act.shape) != (B, 2) or prologue not in (PRO_NONE, PRO_LEAKY):
            raise ValueError('act: expected a (B, 2) table and a none / leaky prologue')
        d.act_scale = L.ptr(act)
    if pw.kparts:
        # the K-part form of the fp32 F(4,3) kernel: cin / 128 planes of raw partial sums in the per-stream workspace, then the sum-and-epilogue launch
        dense = not in_nchw and not out_nchw and ld0 == c0 and (c1 == 0 or ld1 == c1) and ldo in (0, pw.cout)
        if split_k or upsample or stride != 1 or not dense or io != torch.float32 or not f43k_covers(c0 + c1, pw.cout, Ho, Wo, c0 if c1 else None):
            raise ValueError('a weight packed with bf16=WF43K serves dense fp32 3x3 stride-1 launches of the shapes f43k_covers names (conv_code decides: pack with its answer)')
        d.split_k = pw.kparts
        d.workspace = L.ptr(_kpart_ws(dev, pw.kparts * B * Ho * Wo * pw.cout), dtype=torch.int32)
        split_k = 0
    elif split_k is None:
        dense = not in_nchw and not out_nchw and ld0 == c0 and (c1 == 0 or ld1 == c1) and ldo in (0, pw.cout)
        split_k = splitk_for(pw, Ho, Wo, c0 + c1, B) if (stride == 1 and dense) else 0
    if split_k:
        d.split_k = int(split_k)
        if split_k > 1:
            nbytes, tiles = lib.cf_conv2d_workspace_bytes(ctypes.byref(d)), lib.cf_conv2d_tiles(ctypes.byref(d))
            if nbytes < 0 or tiles <= 0:
                raise RuntimeError(f'cf_conv2d_workspace_bytes failed: {L.last_error()}')
            ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
            d.workspace, d.counters = L.ptr(ws), L.ptr(_counters(dev, tiles), dtype=torch.int32)
    stats = None
    if emit_stats and not out_nchw and pw.cout % GN_GROUPS == 0 and pw.cout // GN_GROUPS >= 2:
        d.stats_cpg = pw.cout // GN_GROUPS
        parts = lib.cf_conv2d_stats_parts(ctypes.byref(d))
        if parts <= 0:
            raise RuntimeError(f'cf_conv2d_stats_parts failed ({parts}): {L.last_error()}')
        n_part = B * GN_GROUPS * parts * 2
        part = torch.empty(n_part, dtype=torch.float64, device=dev) if stats_into is None else stats_into.take(n_part, dev)
        d.stats_out = L.ptr(part, dtype=torch.float64)
        stats = (part, parts, d.stats_cpg)
    if caller_out:
        _drop_state(out)      # every check of this function has passed: from here on `out` is written
    if stats is not None:
        out._cf_stats = GNStats(*stats, tensor_stamp(out))

    def launch():
        if w_img is not None:
            L.check(lib.cf_conv2d_sft_w(ctypes.byref(d), w_img, L.stream_ptr()), 'cf_conv2d_sft_w')
        elif u8_in is None and u8_out is None:
            L.check(lib.cf_conv2d(ctypes.byref(d), L.stream_ptr()), 'cf_conv2d')
        else:      # the same descriptor; the image pointer takes the place of in0 / out
            L.check(lib.cf_conv2d_u8(ctypes.byref(d), u8_in, u8_out, L.stream_ptr()), 'cf_conv2d_u8')
    if PROFILE is None:
        launch()
        return out
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    launch()
    e1.record()
    x = img_in if img_in is not None else x
    cin = c0 + c1
    flops = 2.0 * B * Ho * Wo * pw.cout * cin * (4 if (upsample and not pw.wino) else pw.taps)   # executed MACs (folded taps for up2x); Winograd
    # launches are booked at the direct convolution's 9 taps (the algorithmic work), not at their 4 MFMA multiplies per output
    esz = x.element_size()
    nbytes = float(esz * (x.numel() + (0 if x2 is None else x2.numel()) + (0 if res is None else res.numel()) + (0 if sft_scale is None else sft_scale.numel()))
                   + 4 * pw.cout * cin * pw.taps + out.element_size() * out.numel())
    kind = _roofline_kind(pw, io, stride, upsample, c0, in_nchw, out_nchw, Ho * Wo, split_k)
    PROFILE.append((kind, flops, nbytes, e0, e1, (B, H, W, cin, pw.cout)))
    return out


def linear(x, pw, *, epilogue=EPI_NONE, res=None, x_alt=None, alt_from=0):
    """x: (M, K) -> (M, N) through the 1x1 path of the same kernel (M must be a multiple of 256).
    x_alt / alt_from: see conv2d (columns >= alt_from are x_alt @ W^T: two Linear layers, two inputs, one launch).
    M % 256 is THIS function's rule (it presents the rows as 16x16 token images, the unit splitk_for decides by).  The kernels behind
    conv2d(split_k=...) take less (K % 128 == 0 and N % 64 == 0 for all of them):
      fp32 weight    split_k 1, M % 128 == 0, N == cout_pad, not 512 -> 512: gemm_f32_tile_kernel; otherwise the 64x64 split-K instantiation
                     of igemm_kernel (rows per image % 64 == 0; split_k any divisor of K / 128)
      GSPLIT weight  split_k 1, M % 128 == 0: gemm_split_tile_kernel; split_k 1 otherwise or split_k >= 2 (a divisor of K / 128): gemm_split_kernel
                     (M % 64 == 0); split_k SPLITK_IN_WORKGROUP: gemm_split_chunk_kernel (M % 32 == 0, K <= 1024)
    All of one operand scheme return the same bits (tests/test_gpu_token_gemm.py)."""
    M, K = x.shape
    if M % 256:
        raise ValueError(f'linear: rows {M} must be a multiple of 256')
    # present the token matrix as (M/256) "images" of 16x16 tokens: tile selection keys on the per-image shape only
    r4 = None if res is None else res.view(M // 256, 16, 16, pw.cout)
    y = conv2d(x.view(M // 256, 16, 16, K), pw, epilogue=epilogue, res=r4, x_alt=None if x_alt is None else x_alt.view(M // 256, 16, 16, K), alt_from=alt_from)
    return y.view(M, pw.cout)


FINALIZE_FUSED = os.environ.get('CODEFORMER_HIP_FINALIZE_FUSED', '1') != '0'   # 0: one cf_groupnorm_finalize per tensor + separate range-scale launches (A/B; same bits)


def groupnorm_tables(xs, gamma, beta, eps=GN_EPS, groups=GN_GROUPS, act_growth=None):
    """GroupNorm(groups) statistics of the channel-concatenation of xs (each (B,H,W,Ci)) folded with the affine
    parameters into per-(b,c) scale / shift tables (B, sum Ci), to be applied by a conv prologue.

    Tensors that carry epilogue statistics (`._cf_stats`, see conv2d(emit_stats=True)) are not read again; the others
    go through the stand-alone statistics pass -- and so do tensors whose statistics no longer describe them (live_stats): written since
    by this library (conv2d(out=t), also through a slice of t) or, outside torch.inference_mode, in place by the caller (t.mul_(),
    t.copy_()).  Under inference_mode a caller's in-place write cannot be seen: there, write such tensors through this library only.
    act_growth: the caller will also ask act_scale(*xs, growth=act_growth) (the block input that feeds both norm1 and the 1x1 skip
    convolution): when every tensor carries statistics the SAME launch writes that table (cf_groupnorm_finalize2) and parks it where
    act_scale finds it -- bitwise the table of the separate launch."""
    lib = L.load()
    B, H, W, _ = xs[0].shape
    ctot = sum(t.shape[3] for t in xs)
    if ctot % groups:
        raise ValueError(f'{ctot} channels not divisible by {groups} groups')
    cpg = ctot // groups
    hw = H * W
    dev = xs[0].device
    scale = torch.empty(B, ctot, dtype=torch.float32, device=dev)
    shift = torch.empty_like(scale)
    g_ptr, b_ptr, sc_ptr, sh_ptr = L.ptr(gamma), L.ptr(beta), L.ptr(scale), L.ptr(shift)
    stats = []
    for t in xs:
        _act_dtype(t)
        c = t.shape[3]
        if c % cpg:
            raise ValueError('concat boundary splits a group')
        st = live_stats(t)
        if st is None or cpg % st.cpg:
            # ~128 KB of input per block, enough blocks to cover 256 CUs several times, at most 256 partials per group
            nblk = max(1, min(256, (hw * c * 4 + (1 << 17) - 1) >> 17))
            part = torch.empty(B * (c // cpg) * nblk * 2, dtype=torch.float64, device=dev)
            _f32(t)   # (the stand-alone pass reads fp32 tensors; bf16 tensors always carry the partials of their producer)
            L.check(lib.cf_groupnorm_stats(L.ptr(t), B, hw, c, cpg, L.ptr(part, dtype=torch.float64), nblk, L.stream_ptr()), 'cf_groupnorm_stats')
            st = GNStats(part, nblk, cpg)
            stats.append((st, False))
        else:
            stats.append((st, True))
    if FINALIZE_FUSED and len(xs) <= 2:
        # one launch for the tensor (or both halves of the concatenation), and the range-scale table with it when every half carries
        # its producer's statistics (that is where act_scale would take the bound from as well)
        want_act = act_growth is not None and RANGE_SCALE and all(own for _, own in stats)
        act = torch.empty(B, 2, dtype=torch.float32, device=dev) if want_act else None
        cells = L.ptr(_act_cells(dev, B), dtype=torch.int32) if want_act else None
        sa, ca = stats[0][0], xs[0].shape[3]
        sb, cb = (stats[1][0], xs[1].shape[3]) if len(xs) == 2 else (None, 0)
        L.check(lib.cf_groupnorm_finalize2(L.ptr(sa.part, dtype=torch.float64), sa.parts, ca, sa.cpg, cpg // sa.cpg,
                                           None if sb is None else L.ptr(sb.part, dtype=torch.float64), 0 if sb is None else sb.parts, cb,
                                           1 if sb is None else sb.cpg, 1 if sb is None else cpg // sb.cpg, B, hw * cpg, g_ptr, b_ptr, float(eps),
                                           sc_ptr, sh_ptr, ctot, float(act_growth or 0.0), cells, L.ptr(act), L.stream_ptr()), 'cf_groupnorm_finalize2')
        if want_act:
            _park_act(xs, float(act_growth), act)
        return scale, shift
    coff = 0
    for t, (st, _) in zip(xs, stats):
        c = t.shape[3]
        L.check(lib.cf_groupnorm_finalize(L.ptr(st.part, dtype=torch.float64), B, st.parts, c, st.cpg, cpg // st.cpg, hw * cpg,
                                          g_ptr + 4 * coff, b_ptr + 4 * coff, float(eps), sc_ptr + 4 * coff,
                                          sh_ptr + 4 * coff, ctot, L.stream_ptr()), 'cf_groupnorm_finalize')
        coff += c
    return scale, shift


def _act_key(x, growth):
    """What a range-scale table of x is cached under: the growth factor and x's stamp.  None: x shows no writes at all (an inference tensor
    without statistics of this library), so nothing is cached for it."""
    ver, epoch = tensor_stamp(x)
    if ver is None:
        if live_stats(x) is None:
            return None
        ver = 'inference'     # (see act_scale: a conv output, written through this library only)
    return (float(growth), ver, epoch)


def _park_act(xs, growth, act):
    """Leave a range-scale table computed elsewhere (groupnorm_tables) where act_scale(x[, x2]) looks first."""
    k0 = _act_key(xs[0], growth)
    if k0 is None:
        return
    if len(xs) == 1:
        xs[0]._cf_act = (k0, act)
    else:
        k1 = _act_key(xs[1], growth)
        if k1 is not None:
            xs[0]._cf_act_pair = (k0, k1, weakref.ref(xs[1]), act)    # (a weak reference, not an id: ids are recycled)


def layernorm(x, gamma, beta, eps=1e-5, pos=None):
    """x: (rows, C).  Returns LN(x) and, when pos (npos, C) is given, also LN(x)+pos[row % npos]."""
    lib = L.load()
    rows, C = x.shape
    y = torch.empty_like(x)
    ypos = torch.empty_like(x) if pos is not None else None
    npos = 0 if pos is None else pos.shape[0]
    L.check(lib.cf_layernorm(L.ptr(_f32(x)), rows, C, L.ptr(gamma), L.ptr(beta), float(eps), L.ptr(pos), npos, L.ptr(y),
                             L.ptr(ypos), L.stream_ptr()), 'cf_layernorm')
    return (y, ypos) if pos is not None else y


def attention(q, k, v, batch, heads, head_dim, scale):
    """q,k,v: 2-D views (batch*256, >= heads*head_dim) that may be column slices of wider row-major matrices
    (row stride taken from .stride(0)).  Returns (batch*256, heads*head_dim)."""
    lib = L.load()
    rows = batch * 256
    for t in (q, k, v):
        if t.shape[0] != rows or t.stride(1) != 1 or t.shape[1] != heads * head_dim:
            raise ValueError('attention operand must be (batch*256, heads*head_dim) with unit column stride')
    out = torch.empty(rows, heads * head_dim, dtype=torch.float32, device=q.device)
    L.check(lib.cf_attention(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0),
                             L.ptr(out), out.stride(0), batch, heads, head_dim, 256, float(scale), L.stream_ptr()),
            'cf_attention')
    return out


def argmax_rows(logits):
    lib = L.load()
    rows, n = logits.shape
    idx = torch.empty(rows, dtype=torch.int64, device=logits.device)
    L.check(lib.cf_argmax_rows(L.ptr(_f32(logits)), rows, n, L.ptr(idx, dtype=torch.int64), L.stream_ptr()), 'cf_argmax_rows')
    return idx


def argmax_rows_gap(logits, rows_per_group):
    """argmax_rows plus the top-2 gap of every row and its minimum over groups of `rows_per_group` consecutive rows (a face: 256
    tokens).  Returns (idx int64 (rows,), gap fp32 (rows,), group_min_gap fp32 (rows / rows_per_group,)); a NaN gap makes its group NaN."""
    lib = L.load()
    rows, n = logits.shape
    rows_per_group = int(rows_per_group)
    if rows_per_group <= 0 or rows % rows_per_group:
        raise ValueError(f'argmax_rows_gap: {rows} rows are not a multiple of rows_per_group={rows_per_group}')
    idx = torch.empty(rows, dtype=torch.int64, device=logits.device)
    gap = torch.empty(rows, dtype=torch.float32, device=logits.device)
    gmin = torch.empty(rows // rows_per_group, dtype=torch.float32, device=logits.device)
    L.check(lib.cf_argmax_rows_gap(L.ptr(_f32(logits)), rows, n, rows_per_group, L.ptr(idx, dtype=torch.int64), L.ptr(gap), L.ptr(gmin),
                                   L.stream_ptr()), 'cf_argmax_rows_gap')
    return idx, gap, gmin


def codebook_gather(idx, codebook, batch, ntok, lq=None, eps=1e-5):
    """idx: (batch*ntok,) int64 -> (batch, ntok, dim); AdaIN against lq (batch, ntok, dim) when given."""
    lib = L.load()
    ncodes, dim = codebook.shape
    out = torch.empty(batch, ntok, dim, dtype=torch.float32, device=codebook.device)
    L.check(lib.cf_codebook_gather_adain(L.ptr(idx, dtype=torch.int64), L.ptr(_f32(codebook)), ncodes, L.ptr(lq), batch, ntok, dim,
                                         int(lq is not None), float(eps), L.ptr(out), L.stream_ptr()),
            'cf_codebook_gather_adain')
    return out


def vq_nearest(z_tokens, codebook, pw_codebook=None):
    """z_tokens: (rows, dim), rows % 256 == 0.  Returns (idx int64 (rows,), dmin (rows,), (scores, zz, ee))."""
    lib = L.load()
    rows, dim = z_tokens.shape
    ncodes = codebook.shape[0]
    pw = pw_codebook or pack_weight(codebook)
    scores = linear(z_tokens, pw)
    zz = torch.empty(rows, dtype=torch.float32, device=z_tokens.device)
    ee = torch.empty(ncodes, dtype=torch.float32, device=z_tokens.device)
    L.check(lib.cf_row_sqnorm(L.ptr(z_tokens), rows, dim, L.ptr(zz), L.stream_ptr()), 'cf_row_sqnorm')
    L.check(lib.cf_row_sqnorm(L.ptr(_f32(codebook)), ncodes, dim, L.ptr(ee), L.stream_ptr()), 'cf_row_sqnorm')
    idx = torch.empty(rows, dtype=torch.int64, device=z_tokens.device)
    dmin = torch.empty(rows, dtype=torch.float32, device=z_tokens.device)
    L.check(lib.cf_vq_argmin(L.ptr(scores), L.ptr(zz), L.ptr(ee), rows, ncodes, L.ptr(idx, dtype=torch.int64), L.ptr(dmin), L.stream_ptr()),
            'cf_vq_argmin')
    return idx, dmin, (scores, zz, ee)


def to_nhwc(x):
    """(B,C,H,W) -> (B,H,W,C) by the HIP transpose kernel."""
    lib = L.load()
    B, C, H, W = x.shape
    x = _f32(x).contiguous()
    y = torch.empty(B, H, W, C, dtype=torch.float32, device=x.device)
    L.check(lib.cf_nchw_to_nhwc(L.ptr(x), B, C, H * W, L.ptr(y), L.stream_ptr()), 'cf_nchw_to_nhwc')
    return y


def pixel_unshuffle_nhwc(x, scale, c_pad=None):
    """(B,C,H*s,W*s) NCHW -> (B,H,W,c_pad) channels-last pixel-unshuffle (arch_util.py:190-206), channels zero-padded to a
    multiple of 16 so the result feeds conv2d directly.  scale=1 is a padded layout change."""
    lib = L.load()
    B, C, Hs, Ws = x.shape
    if Hs % scale or Ws % scale:
        raise ValueError(f'pixel_unshuffle: {Hs}x{Ws} not divisible by {scale}')
    cu = C * scale * scale
    c_pad = (cu + 15) // 16 * 16 if c_pad is None else c_pad
    x = _f32(x).contiguous()
    y = torch.empty(B, Hs // scale, Ws // scale, c_pad, dtype=torch.float32, device=x.device)
    L.check(lib.cf_pixel_unshuffle_nhwc(L.ptr(x), B, C, Hs // scale, Ws // scale, scale, c_pad, L.ptr(y), L.stream_ptr()),
            'cf_pixel_unshuffle_nhwc')
    return y


def pixel_shuffle_nhwc(x, scale):
    """(B,H,W,C*s*s) channels-last -> (B,H*s,W*s,C) channels-last: nn.PixelShuffle(s) on a conv output that stays NHWC (NCHW indices:
    out[b, c, h*s+i, w*s+j] = x[b, c*s*s + i*s + j, h, w]).  ValueError for a shape that does not fit, TypeError for anything but float32."""
    scale = int(scale)
    if x.dim() != 4 or scale < 1 or scale > 16 or x.shape[3] % (scale * scale):
        raise ValueError(f'pixel_shuffle_nhwc: expected (B,H,W,C*{scale}*{scale}) with 1 <= scale <= 16, got shape {tuple(x.shape)}')
    if x.dtype != torch.float32:
        raise TypeError(f'pixel_shuffle_nhwc: x is {x.dtype}; the op is float32 only')
    lib = L.load()
    B, H, W, Cs = x.shape
    C = Cs // (scale * scale)
    x = x.detach().contiguous()
    y = torch.empty(B, H * scale, W * scale, C, dtype=torch.float32, device=x.device)
    L.check(lib.cf_pixel_shuffle_nhwc(L.ptr(x), B, C, H, W, scale, L.ptr(y), L.stream_ptr()), 'cf_pixel_shuffle_nhwc')
    return y


def to_nchw(x):
    """(B,H,W,C) -> (B,C,H,W)."""
    lib = L.load()
    B, H, W, C = x.shape
    y = torch.empty(B, C, H, W, dtype=torch.float32, device=x.device)
    L.check(lib.cf_nhwc_to_nchw(L.ptr(_f32(x)), B, C, H * W, L.ptr(y), L.stream_ptr()), 'cf_nhwc_to_nchw')
    return y


def img_u8_to_tensor(img):
    """uint8 (B,H,W,3) BGR on device -> fp32 (B,3,H,W) RGB in [-1,1]."""
    lib = L.load()
    B, H, W, _ = img.shape
    out = torch.empty(B, 3, H, W, dtype=torch.float32, device=img.device)
    L.check(lib.cf_img_u8_to_tensor(L.ptr(img, dtype=torch.uint8), B, H, W, L.ptr(out), L.stream_ptr()), 'cf_img_u8_to_tensor')
    return out


def tensor_to_img_u8(t):
    """fp32 (B,3,H,W) RGB -> uint8 (B,H,W,3) BGR with tensor2img(min_max=(-1,1)) rounding."""
    lib = L.load()
    B, _, H, W = t.shape
    img = torch.empty(B, H, W, 3, dtype=torch.uint8, device=t.device)
    L.check(lib.cf_tensor_to_img_u8(L.ptr(_f32(t).contiguous()), B, H, W, L.ptr(img, dtype=torch.uint8), L.stream_ptr()), 'cf_tensor_to_img_u8')
    return img


def mask_composite(x, y):
    """Inpainting composite: where the normalised input pixel is pure white (x0+x1+x2 == 3) take y, else keep x."""
    lib = L.load()
    B, _, H, W = x.shape
    out = torch.empty_like(x)
    L.check(lib.cf_mask_composite(L.ptr(_f32(x).contiguous()), L.ptr(_f32(y).contiguous()), B, H, W, L.ptr(out), L.stream_ptr()),
            'cf_mask_composite')
    return out


_FBA_DTYPES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


def fused_bias_act(x, bias, negative_slope=0.2, scale=math.sqrt(2.0), ref=None, act=3, grad=0):
    """x: (N,C,...) NCHW-style; every mode of the reference op (fused_bias_act_kernel.cu:20-50): act 1 linear | 3 leaky ReLU; grad 0
    forward y = act(x + bias[c]) * scale, 1 first derivative gated by the sign of `ref` (the forward output), 2 zeros.
    float32 / float16 / bfloat16; bias / ref may be None (or empty, as the reference passes them)."""
    lib = L.load()
    if x.dtype not in _FBA_DTYPES:
        raise TypeError(f'fused_bias_act: float32 / float16 / bfloat16 tensors (got {x.dtype})')
    x = x.contiguous()
    bias = None if bias is None or bias.numel() == 0 else bias.detach().to(x.dtype).contiguous()
    ref = None if ref is None or ref.numel() == 0 else ref.detach().to(x.dtype).contiguous()
    if ref is not None and ref.shape != x.shape:
        raise ValueError('fused_bias_act: ref must have the shape of x')
    if bias is not None and bias.numel() != x.shape[1]:
        raise ValueError('fused_bias_act: bias must have one value per channel (dim 1)')
    hw = 1
    for s in x.shape[2:]:
        hw *= s
    y = torch.empty_like(x)
    L.check(lib.cf_fused_bias_act_ex(x.data_ptr(), 0 if bias is None else bias.data_ptr(), 0 if ref is None else ref.data_ptr(),
                                     x.numel(), x.shape[1] if x.dim() > 1 else 1, hw, int(act), int(grad), float(negative_slope),
                                     float(scale), _FBA_DTYPES[x.dtype], y.data_ptr(), L.stream_ptr()), 'cf_fused_bias_act_ex')
    return y


def upfirdn2d(x, kernel, up=1, down=1, pad=(0, 0)):
    """x: (N,C,H,W); kernel: (kh,kw)."""
    lib = L.load()
    x = _f32(x).contiguous()
    n, c, h, w = x.shape
    kh, kw = kernel.shape
    p0, p1 = pad
    oh = (h * up + p0 + p1 - kh) // down + 1
    ow = (w * up + p0 + p1 - kw) // down + 1
    y = torch.empty(n, c, oh, ow, dtype=torch.float32, device=x.device)
    L.check(lib.cf_upfirdn2d(L.ptr(x), n * c, h, w, L.ptr(_f32(kernel).contiguous()), kh, kw, up, up, down, down, p0, p1,
                             p0, p1, L.ptr(y), L.stream_ptr()), 'cf_upfirdn2d')
    return y


# ---- deformable convolution (cf_dcn.hip; codeformer_amd/dcn.py is the basicsr.ops.dcn surface on top) --------------------------------
DCN_MAX_TAPS = 49   # CF_DCN_MAX_TAPS of cf_dcn.h


def _pair(v):
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


def deform_conv2d_route(x_shape, weight_shape, groups=1, deformable_groups=1):
    """'mfma' | 'general': the kernel deform_conv2d runs for an input (B, Cin, H, W) and a weight (Cout, Cin/G, kh, kw).  The MFMA route
    takes every shape in which a float4 of channels lies in one deformable group and a 16-channel K slab in one group:
    (Cin/DG) % 4 == 0, (Cin/G) % 16 == 0, kh*kw <= 49, Cin < 65536 and an image (H*W*Cin floats) below 2^31 bytes (cf_dcn_mfma_covers of cf_dcn.h);
    stride, padding and dilation do not matter."""
    cin, (kh, kw) = int(x_shape[1]), (int(weight_shape[2]), int(weight_shape[3]))
    ok = cin % groups == 0 and cin % deformable_groups == 0 and (cin // deformable_groups) % 4 == 0 and (cin // groups) % 16 == 0 and \
        kh * kw <= DCN_MAX_TAPS and cin < 65536 and int(x_shape[2]) * int(x_shape[3]) * cin * 4 < 2 ** 31
    return 'mfma' if ok else 'general'


def deform_conv2d_out_hw(h, w, kh, kw, stride, padding, dilation):
    (sh, sw), (ph, pw), (dh, dw) = _pair(stride), _pair(padding), _pair(dilation)
    return (h + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1, (w + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1


def deform_conv2d_check(x, offset, weight, mask, bias, stride, padding, dilation, groups, deformable_groups):
    """The shape and dtype rules of the op, for GPU and CPU tensors alike: TypeError for anything but float32, ValueError for a shape that
    does not fit.  Returns (Ho, Wo)."""
    for t, what in ((x, 'input'), (offset, 'offset'), (weight, 'weight'), (mask, 'mask'), (bias, 'bias')):
        if t is not None and t.dtype != torch.float32:
            raise TypeError(f'deform_conv2d: {what} is {t.dtype}; the op is float32 only')
    if x.dim() != 4 or weight.dim() != 4 or offset.dim() != 4 or (mask is not None and mask.dim() != 4):
        raise ValueError('deform_conv2d: input, offset, mask and weight are 4-D tensors')
    (sh, sw), (ph, pw), (dh, dw) = _pair(stride), _pair(padding), _pair(dilation)
    if min(sh, sw, dh, dw) < 1 or min(ph, pw) < 0:
        raise ValueError('deform_conv2d: stride and dilation must be positive, padding non-negative')
    B, cin, H, W = x.shape
    cout, cin_g, kh, kw = weight.shape
    G, DG = int(groups), int(deformable_groups)
    if G < 1 or cin % G or cout % G or cin_g != cin // G:
        raise ValueError(f'deform_conv2d: groups {G} must divide cin {cin} and cout {cout}, and the weight hold cin/groups = {cin // max(G, 1)} input channels (it has {cin_g})')
    if DG < 1 or cin % DG:
        raise ValueError(f'deform_conv2d: deformable_groups {DG} must divide cin {cin}')
    Ho, Wo = deform_conv2d_out_hw(H, W, kh, kw, stride, padding, dilation)
    if H + 2 * ph < dh * (kh - 1) + 1 or W + 2 * pw < dw * (kw - 1) + 1:
        raise ValueError(f'deform_conv2d: the input ({H}x{W}) is smaller than the dilated kernel')
    if tuple(offset.shape) != (B, DG * 2 * kh * kw, Ho, Wo):
        raise ValueError(f'deform_conv2d: offset shape {tuple(offset.shape)}, expected {(B, DG * 2 * kh * kw, Ho, Wo)}')
    if mask is not None and tuple(mask.shape) != (B, DG * kh * kw, Ho, Wo):
        raise ValueError(f'deform_conv2d: mask shape {tuple(mask.shape)}, expected {(B, DG * kh * kw, Ho, Wo)}')
    if bias is not None and tuple(bias.shape) != (cout,):
        raise ValueError(f'deform_conv2d: bias shape {tuple(bias.shape)}, expected {(cout,)}')
    return Ho, Wo


def _dcn_packed(weight, groups):
    """The MFMA route's packing of `weight`, kept on the tensor object until its version, storage or device moves (as the arch modules keep
    theirs: an edit of `weight.data` in place is not versioned -- delete `weight._cf_dcn` after one).  Inference tensors keep no version
    and are packed per call."""
    ver = tensor_version(weight)
    key = (weight.data_ptr(), ver, str(weight.device), int(groups))
    ent = weight.__dict__.get('_cf_dcn') if ver is not None else None
    if ent is not None and ent[0] == key:
        return ent[1]
    lib = L.load()
    cout, cin_g, kh, kw = weight.shape
    w = weight.detach().contiguous()
    n = lib.cf_deform_conv2d_packed_elems(cout, cin_g * groups, kh * kw, groups)
    if n <= 0:
        raise RuntimeError(f'cf_deform_conv2d_packed_elems failed ({n})')
    packed = torch.empty(n, dtype=torch.float32, device=w.device)
    L.check(lib.cf_pack_deform_conv_weight(L.ptr(w), cout, cin_g * groups, kh * kw, groups, L.ptr(packed), L.stream_ptr()), 'cf_pack_deform_conv_weight')
    if ver is not None:
        weight._cf_dcn = (key, packed)
    return packed


def _is_channels_last(x):
    """Dense (B,C,H,W) tensor whose memory is [b][h][w][c] (torch.channels_last), 16-byte aligned: read in place as NHWC."""
    B, C, H, W = x.shape
    return x.stride() == (H * W * C, 1, W * C, C) and x.data_ptr() % 16 == 0


def deform_conv2d(x, offset, weight, mask=None, bias=None, stride=1, padding=0, dilation=1, groups=1, deformable_groups=1, route=None):
    """Deformable convolution, forward, float32: x (B,Cin,H,W), offset (B,DG*2*kh*kw,Ho,Wo), weight (Cout,Cin/G,kh,kw), mask (B,DG*kh*kw,Ho,Wo)
    or None (the plain op: mask == 1), bias (Cout) or None -> (B,Cout,Ho,Wo); the definition stands in include/codeformer_hip.h
    (cf_deform_conv2d).  stride / padding / dilation: an int or a (vertical, horizontal) pair.
    A torch.channels_last x is read in place; any other x is brought to channels-last by to_nhwc for the MFMA route and read as NCHW by
    the general one.  route: None (deform_conv2d_route decides), 'general' (any shape) or 'mfma' (ValueError where it does not cover)."""
    Ho, Wo = deform_conv2d_check(x, offset, weight, mask, bias, stride, padding, dilation, groups, deformable_groups)
    lib = L.load()
    auto = deform_conv2d_route(x.shape, weight.shape, groups, deformable_groups)
    if route not in (None, 'mfma', 'general'):
        raise ValueError(f"deform_conv2d: route {route!r} (None, 'mfma' or 'general')")
    if route == 'mfma' and auto != 'mfma':
        raise ValueError('deform_conv2d: the mfma route needs (Cin/DG) % 4 == 0, (Cin/G) % 16 == 0 and kh*kw <= 49')
    route = route or auto
    (sh, sw), (ph, pw), (dh, dw) = _pair(stride), _pair(padding), _pair(dilation)
    B, cin, H, W = x.shape
    cout, _, kh, kw = weight.shape
    x = x.detach()
    if _is_channels_last(x):
        xin, nhwc = x.permute(0, 2, 3, 1), 1
    elif route == 'mfma':
        xin, nhwc = to_nhwc(x), 1
    else:
        xin, nhwc = x.contiguous(), 0
    w = _dcn_packed(weight, groups) if route == 'mfma' else weight.detach().contiguous()
    offset = offset.detach().contiguous()
    mask = None if mask is None else mask.detach().contiguous()
    bias = None if bias is None else bias.detach().contiguous()
    out = torch.empty(B, cout, Ho, Wo, dtype=torch.float32, device=x.device)
    L.check(lib.cf_deform_conv2d(L.ptr(xin), L.ptr(offset), L.ptr(mask), L.ptr(w), L.ptr(bias), L.ptr(out), B, cin, H, W, cout, kh, kw,
                                 sh, sw, ph, pw, dh, dw, int(groups), int(deformable_groups), nhwc, int(route == 'mfma'), L.stream_ptr()),
            'cf_deform_conv2d')
    return out


# ---- optical-flow warp (cf_warp.hip; codeformer_amd/archs/arch_util.py is the basicsr.archs.arch_util surface on top) -----------------
WARP_INTERP = {'bilinear': 0, 'nearest': 1}
WARP_PADDING = {'zeros': 0, 'border': 1, 'reflection': 2}


def flow_warp_check(x, flow, interp_mode, padding_mode):
    """The shape, dtype and mode rules of flow_warp, for GPU and CPU tensors alike: ValueError for a shape or a mode string that does not
    fit, TypeError for anything but float32.  Returns (interp, padding) as the kernel's codes."""
    if not isinstance(interp_mode, str) or interp_mode not in WARP_INTERP:
        raise ValueError(f"flow_warp: interp_mode {interp_mode!r} ('bilinear' or 'nearest')")
    if not isinstance(padding_mode, str) or padding_mode not in WARP_PADDING:
        raise ValueError(f"flow_warp: padding_mode {padding_mode!r} ('zeros', 'border' or 'reflection')")
    if x.dim() != 4 or flow.dim() != 4:
        raise ValueError('flow_warp: x is (B,C,H,W) and flow (B,H,W,2)')
    B, C, H, W = x.shape
    if tuple(flow.shape) != (B, H, W, 2) or min(B, C, H, W) < 1:
        raise ValueError(f'flow_warp: flow shape {tuple(flow.shape)}, expected {(B, H, W, 2)} for x {tuple(x.shape)}')
    if H >= 1 << 24 or W >= 1 << 24 or H * W >= 1 << 31:
        raise ValueError(f'flow_warp: image too large ({H}x{W})')
    for t, what in ((x, 'x'), (flow, 'flow')):
        if t.dtype != torch.float32:
            raise TypeError(f'flow_warp: {what} is {t.dtype}; the op is float32 only')
    return WARP_INTERP[interp_mode], WARP_PADDING[padding_mode]


def flow_warp(x, flow, interp_mode='bilinear', padding_mode='zeros', align_corners=True):
    """Warp x (B,C,H,W) by the optical flow (B,H,W,2) = (dx, dy), float32: out[b, c, y, x] = the sample of x[b, c] at (x + dx, y + dy); the
    definition stands in include/codeformer_hip.h (cf_flow_warp).  A torch.channels_last x with C % 4 == 0 is read in place and the result
    is channels_last too; any other x is read as contiguous NCHW planes (after a copy where it is not contiguous)."""
    interp, padding = flow_warp_check(x, flow, interp_mode, padding_mode)
    lib = L.load()
    B, C, H, W = x.shape
    x, flow = x.detach(), flow.detach().contiguous()
    nhwc = C % 4 == 0 and not x.is_contiguous() and _is_channels_last(x)
    if nhwc:
        out = torch.empty_like(x)     # (channels_last, like x)
        nhwc = _is_channels_last(out)
    if nhwc:
        xin, dst = x.permute(0, 2, 3, 1), out.permute(0, 2, 3, 1)
    else:
        xin = x.contiguous()
        out = dst = torch.empty(B, C, H, W, dtype=torch.float32, device=x.device)
    L.check(lib.cf_flow_warp(L.ptr(xin), L.ptr(flow), L.ptr(dst), B, C, H, W, interp, padding, int(bool(align_corners)), int(nhwc),
                             L.stream_ptr()), 'cf_flow_warp')
    return out


# ---- alignment warp / paste-back primitives (cf_paste.hip) -- see codeformer_amd/facelib/paste.py for the orchestration --------------
def _c6(m):
    """6 doubles in host memory for the ctypes call (a 2x3 destination->source matrix)."""
    vals = [float(v) for v in (m.reshape(-1).tolist() if hasattr(m, 'reshape') else m)]
    if len(vals) != 6:
        raise ValueError('affine matrix must have 6 elements')
    return (ctypes.c_double * 6)(*vals)


def warp_affine_u8(src, inv_dev, dst, region=None, border=(0, 0, 0)):
    """src: uint8 (sh,sw,3) (shared) or (n,sh,sw,3); inv_dev: float64 CUDA (n,6) destination->source matrices; dst: uint8 (n,dh,dw,3)
    written inside region = (rx, ry, rw, rh) (default: everything)."""
    lib = L.load()
    n, dh, dw, _ = dst.shape
    shared = src.dim() == 3
    sh, sw = (src.shape[0], src.shape[1]) if shared else (src.shape[1], src.shape[2])
    if (not shared and src.shape[0] != n) or tuple(inv_dev.shape) != (n, 6):
        raise ValueError('warp_affine_u8: batch mismatch')
    rx, ry, rw, rh = region or (0, 0, dw, dh)
    L.check(lib.cf_warp_affine_u8(L.ptr(src, dtype=torch.uint8), 0 if shared else sh * sw * 3, sh, sw, L.ptr(inv_dev, dtype=torch.float64), n,
                                  L.ptr(dst, dtype=torch.uint8), dh, dw, rx, ry, rw, rh, int(border[0]), int(border[1]), int(border[2]),
                                  L.stream_ptr()), 'cf_warp_affine_u8')
    return dst


def warp_affine_f32(src, inv, region):
    lib = L.load()
    rx, ry, rw, rh = region
    out = torch.empty(rh, rw, dtype=torch.float32, device=src.device)
    L.check(lib.cf_warp_affine_f32(L.ptr(src), src.shape[0], src.shape[1], _c6(inv), L.ptr(out), rx, ry, rw, rh, L.stream_ptr()),
            'cf_warp_affine_f32')
    return out


def erode(x, k):
    lib = L.load()
    tmp, out = torch.empty_like(x), torch.empty_like(x)
    L.check(lib.cf_erode_f32(L.ptr(x), L.ptr(tmp), L.ptr(out), x.shape[0], x.shape[1], int(k), L.stream_ptr()), 'cf_erode_f32')
    return out


def gaussian_blur(x, taps_dev, region_xy=(0, 0), frame_hw=None):
    """x: (rh,rw) float32 region at (rx, ry) of a frame of size frame_hw (default: the region is the frame); taps_dev: CUDA float32."""
    lib = L.load()
    ch, cw = frame_hw or (x.shape[0], x.shape[1])
    tmp, out = torch.empty_like(x), torch.empty_like(x)
    L.check(lib.cf_gaussian_blur_f32(L.ptr(x), L.ptr(tmp), L.ptr(out), x.shape[0], x.shape[1], int(region_xy[0]), int(region_xy[1]), ch, cw,
                                     L.ptr(taps_dev), taps_dev.numel(), L.stream_ptr()), 'cf_gaussian_blur_f32')
    return out


def sum_partials(x, out64):
    """64 fp64 partial sums of x into out64 (CUDA float64, 64 elements); the caller adds them after its read-back."""
    lib = L.load()
    L.check(lib.cf_sum_f32(L.ptr(x), x.numel(), L.ptr(out64, dtype=torch.float64), L.stream_ptr()), 'cf_sum_f32')


def paste_blend(canvas, face, inv, ero, soft, region, parse=None):
    lib = L.load()
    rx, ry, rw, rh = region
    L.check(lib.cf_paste_blend(L.ptr(canvas), canvas.shape[0], canvas.shape[1], L.ptr(face, dtype=torch.uint8), face.shape[0], face.shape[1],
                               _c6(inv), L.ptr(ero), L.ptr(soft), L.ptr(parse), rx, ry, rw, rh, L.stream_ptr()), 'cf_paste_blend')


def resize_linear_u8(src, dh, dw):
    lib = L.load()
    out = torch.empty(dh, dw, 3, dtype=torch.float32, device=src.device)
    L.check(lib.cf_resize_linear_u8(L.ptr(src, dtype=torch.uint8), src.shape[0], src.shape[1], L.ptr(out), dh, dw, L.stream_ptr()),
            'cf_resize_linear_u8')
    return out


def resize_area_u8(src, dh, dw):
    """cv2.resize(src uint8 (sh, sw, 3) on the device, (dw, dh), INTER_AREA) -> uint8 (dh, dw, 3); shrinking only."""
    lib = L.load()
    if src.dim() != 3 or src.shape[2] != 3 or not src.is_contiguous():
        raise ValueError('resize_area_u8 expects a contiguous uint8 (H, W, 3) image')
    out = torch.empty(dh, dw, 3, dtype=torch.uint8, device=src.device)
    L.check(lib.cf_resize_area_u8(L.ptr(src, dtype=torch.uint8), src.shape[0], src.shape[1], L.ptr(out, dtype=torch.uint8), dh, dw, L.stream_ptr()),
            'cf_resize_area_u8')
    return out


def f32_to_u8_trunc(x):
    lib = L.load()
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    L.check(lib.cf_f32_to_u8_trunc(L.ptr(x), x.numel(), L.ptr(out, dtype=torch.uint8), L.stream_ptr()), 'cf_f32_to_u8_trunc')
    return out


def box_overlay_u8(canvas, faces_dev, face_hw):
    """The final uint8 frame of a draw_box paste: truncation of `canvas` (float32 (H,W,3)) and, face by face, the green blend through the
    warped border band.  faces_dev: float64 CUDA (n, 11) = dst->src matrix, border, x0, y0, x1, y1 (None / n == 0: truncation only)."""
    lib = L.load()
    out = torch.empty(canvas.shape, dtype=torch.uint8, device=canvas.device)
    n = 0 if faces_dev is None else faces_dev.shape[0]
    if n and tuple(faces_dev.shape) != (n, 11):
        raise ValueError('box_overlay_u8: faces_dev must be (n, 11)')
    L.check(lib.cf_box_overlay_u8(L.ptr(canvas), canvas.shape[0], canvas.shape[1], L.ptr(faces_dev, dtype=torch.float64) if n else None, n,
                                  int(face_hw[0]), int(face_hw[1]), L.ptr(out, dtype=torch.uint8), L.stream_ptr()), 'cf_box_overlay_u8')
    return out


def resize_linear_f32(x, dh, dw):
    """cv2.resize(float32 plane, (dw, dh), INTER_LINEAR) of every plane of x (n, sh, sw) -> (n, dh, dw)."""
    lib = L.load()
    if x.dim() != 3:
        raise ValueError('resize_linear_f32 expects (n, H, W) planes')
    out = torch.empty(x.shape[0], dh, dw, dtype=torch.float32, device=x.device)
    if x.shape[0]:
        L.check(lib.cf_resize_linear_f32(L.ptr(x), x.shape[0], x.shape[1], x.shape[2], L.ptr(out), dh, dw, L.stream_ptr()),
                'cf_resize_linear_f32')
    return out


def esrgan_tile_gather(faces, pre_pad, mod, window):
    """uint8 BGR faces (n, h, w, 3) -> float32 RGB NCHW (n, 3, th, tw) in [0, 1]: window (py0, px0, th, tw) of the reflect-padded view."""
    lib = L.load()
    n, h, w, _ = faces.shape
    py0, px0, th, tw = window
    out = torch.empty(n, 3, th, tw, dtype=torch.float32, device=faces.device)
    L.check(lib.cf_esrgan_tile_gather_u8(L.ptr(faces, dtype=torch.uint8), n, h, w, int(pre_pad), int(mod), py0, px0, th, tw, L.ptr(out),
                                         L.stream_ptr()), 'cf_esrgan_tile_gather_u8')
    return out


def esrgan_tile_scatter(up, core, out, dst_yx):
    """The core (oy, ox, ch, cw) of the model output up (n, 3, uh, uw) into the uint8 BGR faces out (n, oh, ow, 3) at dst_yx (dy, dx)."""
    lib = L.load()
    n, _, uh, uw = up.shape
    oy, ox, ch, cw = core
    if out.shape[0] != n:
        raise ValueError('esrgan_tile_scatter: batch mismatch')
    L.check(lib.cf_esrgan_tile_scatter_u8(L.ptr(up), n, uh, uw, oy, ox, ch, cw, L.ptr(out, dtype=torch.uint8), out.shape[1], out.shape[2],
                                          int(dst_yx[0]), int(dst_yx[1]), L.stream_ptr()), 'cf_esrgan_tile_scatter_u8')


def label_lut(labels, lut):
    lib = L.load()
    out = torch.empty(labels.shape, dtype=torch.float32, device=labels.device)
    arr = (ctypes.c_float * len(lut))(*[float(v) for v in lut])
    L.check(lib.cf_label_lut_f32(L.ptr(labels, dtype=torch.int64), labels.numel(), arr, len(lut), L.ptr(out), L.stream_ptr()), 'cf_label_lut_f32')
    return out


def scale_clear_border_(x, border, scale):
    lib = L.load()
    B, H, W = x.shape
    L.check(lib.cf_scale_clear_border_f32(L.ptr(x), B, H, W, int(border), float(scale), L.stream_ptr()), 'cf_scale_clear_border_f32')
    return x


# ---- quality metrics (cf_metrics.hip) -- see codeformer_amd/metrics.py for the public surface -----------------------------------------
METRIC_DTYPES = {torch.uint8: 0, torch.float32: 1}


def _image_view(t, what, channels):
    """The check of a strided (B,H,W,C) image VIEW (cf_img_view in csrc/cf_score_parts.h): uint8 or float32, C one of `channels`, no empty
    dimension, non-negative strides, largest element offset below 2^31.  Returns (its element strides as ctypes, its dtype code)."""
    if t.dim() != 4 or t.shape[3] not in channels or min(t.shape) < 1 or t.dtype not in METRIC_DTYPES:
        raise ValueError(f'{what}: a uint8 or float32 (B,H,W,C) view with C in {channels} and no empty dimension is needed, got {t.dtype} {tuple(t.shape)}')
    if min(t.stride()) < 0 or sum((n - 1) * s for n, s in zip(t.shape, t.stride())) >= 1 << 31:
        raise ValueError(f'{what}: strides must be non-negative and the largest element offset below 2^31')
    return (ctypes.c_int64 * 4)(*t.stride()), METRIC_DTYPES[t.dtype]


def _metric_call(a, b, y_channel, ssim_):
    """The checks and scratch shared by psnr / ssim.  a, b: (B,H,W,C) VIEWS (any strides: a crop, a permuted CHW tensor, a slice)."""
    if not (a.is_cuda and b.is_cuda):
        raise ValueError('codeformer_amd ops need CUDA (ROCm) tensors')
    if a.device != b.device:
        raise ValueError(f'metrics: the images lie on different devices ({a.device}, {b.device})')
    if a.dim() != 4 or tuple(a.shape) != tuple(b.shape):
        raise ValueError(f'metrics: two (B,H,W,C) views of one shape are needed, got {tuple(a.shape)} and {tuple(b.shape)}')
    if a.dtype not in METRIC_DTYPES or b.dtype != a.dtype:
        raise TypeError(f'metrics: both images must be uint8 or both float32, got {a.dtype} and {b.dtype}')
    (sa, dt), (sb, _) = (_image_view(t, 'metrics', (1, 3)) for t in (a, b))
    B, H, W, C = a.shape
    if ssim_ and (H < 11 or W < 11):
        raise ValueError(f'ssim: the image ({H}x{W}) is smaller than the 11x11 window')
    lib = L.ensure_device(a.device)
    planes = 1 if y_channel else C
    nparts = lib.cf_metric_parts(H, W, planes)
    if nparts < 0:
        raise RuntimeError(f'cf_metric_parts failed: {L.last_error()}')
    parts = torch.empty(B * nparts, dtype=torch.float64, device=a.device)
    return lib, parts, (sa, sb), dt


def psnr(a, b, y_channel=False):
    """(sse, psnr): two (B,) float64 tensors -- the squared-error sum of every image pair of the (B,H,W,C) views a, b (uint8 or float32,
    values in [0, 255]) and its PSNR; the definition stands at cf_psnr in include/codeformer_hip.h.  No copy, no synchronisation."""
    lib, parts, (sa, sb), dt = _metric_call(a, b, y_channel, False)
    B, H, W, C = a.shape
    with torch.cuda.device(a.device):
        out = torch.empty(2, B, dtype=torch.float64, device=a.device)
        L.check(lib.cf_psnr(a.data_ptr(), b.data_ptr(), B, H, W, C, sa, sb, dt, int(bool(y_channel)), L.ptr(parts, dtype=torch.float64),
                            out[0].data_ptr(), out[1].data_ptr(), L.stream_ptr()), 'cf_psnr')
    return out[0], out[1]


def ssim(a, b, y_channel=False):
    """(B,) float64: the SSIM of every image pair of the (B,H,W,C) views a, b (cf_ssim in include/codeformer_hip.h).  No copy, no
    synchronisation."""
    lib, parts, (sa, sb), dt = _metric_call(a, b, y_channel, True)
    B, H, W, C = a.shape
    with torch.cuda.device(a.device):
        out = torch.empty(B, dtype=torch.float64, device=a.device)
        L.check(lib.cf_ssim(a.data_ptr(), b.data_ptr(), B, H, W, C, sa, sb, dt, int(bool(y_channel)), L.ptr(parts, dtype=torch.float64),
                            L.ptr(out, dtype=torch.float64), L.stream_ptr()), 'cf_ssim')
    return out


# ---- ResNetArcFace and the identity metric (cf_arcface.hip) -- definitions at "ArcFace / identity metric" in include/codeformer_hip.h ------
def _nhwc_dense(x, what):
    _f32(x)
    if x.dim() != 4 or not x.is_contiguous() or x.shape[3] % 4:
        raise ValueError(f'{what}: expected a dense float32 (B,H,W,C) tensor with C % 4 == 0, got {tuple(x.shape)}')
    return x.shape


def prelu_maxpool2(x, alpha):
    """MaxPool2d(2, 2) of prelu(x, alpha): (B,2h,2w,C) -> (B,h,w,C), PReLU first (they do not commute for alpha < 0)."""
    B, H, W, C = _nhwc_dense(x, 'prelu_maxpool2')
    if H % 2 or W % 2:
        raise ValueError(f'prelu_maxpool2: even height and width, got {H}x{W}')
    out = torch.empty((B, H // 2, W // 2, C), dtype=torch.float32, device=x.device)
    L.check(L.load().cf_prelu_maxpool2(L.ptr(x), B, H // 2, W // 2, C, float(alpha), L.ptr(out), L.stream_ptr()), 'cf_prelu_maxpool2')
    return out


def se_pool(x):
    """(B,H,W,C) -> the (B,C) mean over the pixels, in one fixed order per image."""
    B, H, W, C = _nhwc_dense(x, 'se_pool')
    lib = L.load()
    parts = torch.empty(B * lib.cf_se_pool_parts(H * W) * C, dtype=torch.float32, device=x.device)
    out = torch.empty((B, C), dtype=torch.float32, device=x.device)
    L.check(lib.cf_se_pool(L.ptr(x), B, H * W, C, L.ptr(parts), L.ptr(out), L.stream_ptr()), 'cf_se_pool')
    return out


def se_gate(pooled, w1, b1, alpha, w2, b2):
    """sigmoid(Linear(prelu(Linear(pooled)))) on (B,C) rows; w1 (r,C), w2 (C,r) in torch's Linear layout."""
    B, C = _f32(pooled).shape
    r = w1.shape[0]
    if tuple(w1.shape) != (r, C) or tuple(w2.shape) != (C, r) or tuple(b1.shape) != (r,) or tuple(b2.shape) != (C,):
        raise ValueError(f'se_gate: weights {tuple(w1.shape)}, {tuple(w2.shape)} do not fit {C} channels')
    out = torch.empty((B, C), dtype=torch.float32, device=pooled.device)
    L.check(L.load().cf_se_gate(L.ptr(pooled), L.ptr(w1), L.ptr(b1), float(alpha), L.ptr(w2), L.ptr(b2), B, C, r, L.ptr(out), L.stream_ptr()), 'cf_se_gate')
    return out


def se_scale_res_prelu(x, y, res, alpha):
    """prelu(x * y[b][c] + res, alpha): x, res (B,H,W,C), y (B,C); res None: prelu(x * y[b][c], alpha), no add."""
    B, H, W, C = _nhwc_dense(x, 'se_scale_res_prelu')
    if (res is not None and tuple(res.shape) != tuple(x.shape)) or tuple(y.shape) != (B, C):
        raise ValueError(f'se_scale_res_prelu: x {tuple(x.shape)}, y {tuple(y.shape)}, res {None if res is None else tuple(res.shape)}')
    out = torch.empty_like(x)
    L.check(L.load().cf_se_scale_res_prelu(L.ptr(x), L.ptr(y), L.ptr(res), B, H * W, C, float(alpha), L.ptr(out), L.stream_ptr()), 'cf_se_scale_res_prelu')
    return out


FC_ROWS = 16   # rows per cf_fc_rows launch


def pack_fc_rows(weight):
    """(N,K) Linear weight -> the [K/4][N][4] layout cf_fc_rows reads (a lane owns an output column)."""
    N, K = _f32(weight).shape
    if K % 256 or N % 4:
        raise ValueError(f'pack_fc_rows: K % 256 == 0 and N % 4 == 0, got {(N, K)}')
    return weight.detach().reshape(N, K // 4, 4).permute(1, 0, 2).contiguous()


def fc_rows(x, wp, bias=None):
    """x (M,K) @ W^T + bias for a handful of rows, W packed by pack_fc_rows; row m never depends on the other rows (more than FC_ROWS rows
    are that many launches, each reading the weight once)."""
    M, K = _f32(x).shape
    N = wp.shape[1]
    if tuple(wp.shape) != (K // 4, N, 4) or not x.is_contiguous():
        raise ValueError(f'fc_rows: x {tuple(x.shape)} (dense) does not fit the packed weight {tuple(wp.shape)}')
    lib = L.load()
    out = torch.empty((M, N), dtype=torch.float32, device=x.device)
    for m0 in range(0, M, FC_ROWS):
        m = min(FC_ROWS, M - m0)
        ws = torch.empty(lib.cf_fc_rows_workspace_elems(m, N, K), dtype=torch.float32, device=x.device)
        L.check(lib.cf_fc_rows(L.ptr(x[m0:m0 + m]), L.ptr(wp), L.ptr(bias), m, N, K, L.ptr(ws), L.ptr(out[m0:m0 + m]), L.stream_ptr()), 'cf_fc_rows')
    return out


def identity_input(view, bgr):
    """(B,H,W,3) VIEW (any non-negative strides), uint8 or float32 in [0, 1] -> (B,1,128,128) float32: RGB in [-1, 1], gray, bilinear resize."""
    st, dt = _image_view(view, 'identity_input', (3,))
    lib = L.ensure_device(view.device)
    B, H, W, _ = view.shape
    with torch.cuda.device(view.device):
        out = torch.empty((B, 1, 128, 128), dtype=torch.float32, device=view.device)
        L.check(lib.cf_identity_input(view.data_ptr(), B, H, W, st, dt, int(bool(bgr)), L.ptr(out), L.stream_ptr()), 'cf_identity_input')
    return out


def cosine_rows(x, y):
    """(B,) float64: x_r . y_r / max(|x_r| |y_r|, 1e-8) of the float32 rows of x and y, in float64."""
    if x.dim() != 2 or tuple(x.shape) != tuple(y.shape) or x.device != y.device:
        raise ValueError(f'cosine_rows: two (B,N) tensors of one shape on one device, got {tuple(x.shape)} and {tuple(y.shape)}')
    lib = L.ensure_device(x.device)
    with torch.cuda.device(x.device):
        out = torch.empty(x.shape[0], dtype=torch.float64, device=x.device)
        L.check(lib.cf_cosine_rows(L.ptr(_f32(x)), L.ptr(_f32(y)), x.shape[0], x.shape[1], L.ptr(out, dtype=torch.float64), L.stream_ptr()), 'cf_cosine_rows')
    return out


# ---- VGGFeatureExtractor and the perceptual / style score (cf_vgg.hip) -- definitions at "VGG / perceptual" in include/codeformer_hip.h ------
VGG_IN_CPAD = 16    # channels of vgg_input's output: one K slab of the general 3x3 kernel (pack_weight pads conv1_1's three to the same)
GRAM_CHUNK = 1024   # CF_GRAM_CHUNK
FEAT_CHUNK = 16384  # CF_FEAT_CHUNK


def vgg_input(view, bgr, range_norm=False, mean=None, std=None, c_pad=VGG_IN_CPAD, out=None):
    """(B,H,W,3) VIEW (any non-negative strides), uint8 (v / 255) or float32 -> dense (B,H,W,c_pad) float32, channels R, G, B then zeros:
    (x + 1) / 2 with range_norm, then (x - mean[c]) / std[c] when mean / std (three Python floats each) are given.  out: a dense
    destination (a batch slice of a larger buffer)."""
    st, dt = _image_view(view, 'vgg_input', (3,))
    if (mean is None) != (std is None) or (mean is not None and (len(mean) != 3 or len(std) != 3)):
        raise ValueError('vgg_input: mean and std are three floats each, or both None')
    if c_pad < 4 or c_pad > 64 or c_pad % 4:
        raise ValueError(f'vgg_input: c_pad {c_pad} (4 .. 64, a multiple of 4)')
    lib = L.ensure_device(view.device)
    B, H, W, _ = view.shape
    f3 = ctypes.c_float * 3
    if out is not None:
        if tuple(out.shape) != (B, H, W, c_pad) or out.dtype != torch.float32 or out.device != view.device or not out.is_contiguous():
            raise ValueError(f'vgg_input: out must be a dense float32 {(B, H, W, c_pad)} tensor on {view.device}')
        _drop_state(out)
    with torch.cuda.device(view.device):
        if out is None:
            out = torch.empty((B, H, W, c_pad), dtype=torch.float32, device=view.device)
        L.check(lib.cf_vgg_input(view.data_ptr(), B, H, W, st, dt, int(bool(bgr)), int(bool(range_norm)), int(mean is not None),
                                 None if mean is None else f3(*mean), None if std is None else f3(*std),
                                 int(c_pad), L.ptr(out), L.stream_ptr()), 'cf_vgg_input')
    return out


def relu(x, inplace=False):
    """x > 0 ? x : +0 on a dense float32 tensor with a multiple of 4 elements (NaN stays NaN); inplace: x is overwritten and returned."""
    _f32(x)
    if not x.is_contiguous() or x.numel() % 4 or x.numel() == 0:
        raise ValueError(f'relu: expected a dense tensor with a multiple of 4 elements, got {tuple(x.shape)}')
    out = x if inplace else torch.empty_like(x)
    if inplace:
        _drop_state(x)
    L.check(L.load().cf_relu(L.ptr(x), x.numel(), L.ptr(out), L.stream_ptr()), 'cf_relu')
    return out


def relu_maxpool2(x, full=False):
    """MaxPool2d(2, 2) of relu(x): (B,H,W,C) -> (B,H//2,W//2,C), an odd last row / column dropped; a NaN wins the max.
    full=True: (pooled, relu(x) at full size) from the one launch; full='inplace': the full-size ReLU overwrites x."""
    B, H, W, C = _nhwc_dense(x, 'relu_maxpool2')
    if H < 2 or W < 2:
        raise ValueError(f'relu_maxpool2: the pool would take {H}x{W} to zero')
    out = torch.empty((B, H // 2, W // 2, C), dtype=torch.float32, device=x.device)
    fl = None
    if full == 'inplace':
        fl = x
        _drop_state(x)
    elif full:
        fl = torch.empty_like(x)
    L.check(L.load().cf_relu_maxpool2(L.ptr(x), B, H, W, C, L.ptr(out), L.ptr(fl), L.stream_ptr()), 'cf_relu_maxpool2')
    return (out, fl) if full else out


def _features(f, what):
    """(B,H,W,C) or (B,HW,C) dense float32 features -> (B, HW, C)."""
    _f32(f)
    if f.dim() not in (3, 4) or not f.is_contiguous() or min(f.shape) < 1:
        raise ValueError(f'{what}: expected dense (B,H,W,C) or (B,HW,C) features, got {tuple(f.shape)}')
    B, C = f.shape[0], f.shape[-1]
    return B, f.numel() // (B * C), C


def gram(f):
    """(B,H,W,C) or (B,HW,C) dense float32 features -> (B,C,C): F^T F / (float)(C * HW) per image on the fp32 MFMA, C % 64 == 0, C <= 512.
    Bitwise symmetric, bitwise repeatable, image b bitwise the call on it alone."""
    B, hw, C = _features(f, 'gram')
    if C % 64 or C > 512 or B > 65535:
        raise ValueError(f'gram: C % 64 == 0, C <= 512 and B <= 65535, got B {B}, C {C}')
    lib = L.load()
    n = lib.cf_gram_workspace_elems(B, hw, C)
    if n < 0:
        raise ValueError(f'gram: unsupported shape {tuple(f.shape)}')
    ws = torch.empty(n, dtype=torch.float32, device=f.device)
    g = torch.empty((B, C, C), dtype=torch.float32, device=f.device)
    L.check(lib.cf_gram(L.ptr(f), B, hw, C, L.ptr(ws), L.ptr(g), L.stream_ptr()), 'cf_gram')
    return g


def feat_dist(a, b):
    """(B,2) float64: per image (sum |a - b|, sum (a - b)^2) of two dense float32 tensors of one shape (B, ...); each difference is one
    float32 subtraction, widened before use; partial sums per chunk of FEAT_CHUNK elements, added in one fixed order (cf_feat_dist in the header)."""
    _f32(a), _f32(b)
    if tuple(a.shape) != tuple(b.shape) or a.dim() < 2 or a.device != b.device or not (a.is_contiguous() and b.is_contiguous()) or a.numel() == 0:
        raise ValueError(f'feat_dist: two dense tensors of one shape (B, ...) on one device, got {tuple(a.shape)} and {tuple(b.shape)}')
    B = a.shape[0]
    n = a.numel() // B
    if B > 65535:
        raise ValueError(f'feat_dist: at most 65535 images, got {B}')
    lib = L.load()
    nparts = lib.cf_feat_dist_parts(n)
    if nparts < 0:
        raise ValueError(f'feat_dist: unsupported size {n}')
    parts = torch.empty(B * nparts * 2, dtype=torch.float64, device=a.device)
    out = torch.empty((B, 2), dtype=torch.float64, device=a.device)
    L.check(lib.cf_feat_dist(L.ptr(a), L.ptr(b), B, n, L.ptr(parts, dtype=torch.float64), L.ptr(out, dtype=torch.float64), L.stream_ptr()), 'cf_feat_dist')
    return out


def lpips_head(fa, fb, lin):
    """(B,) float64: one layer of the LPIPS distance of dense channels-last float32 features fa, fb (B,H,W,C) or (B,HW,C), C % 4 == 0, C <= 512,
    under the non-negative channel weights lin (C,): the pixel mean of sum_c lin[c] (fa_c / (|fa| + 1e-10) - fb_c / (|fb| + 1e-10))^2."""
    _f32(lin)
    (B, hw, C), _ = _features(fa, 'lpips_head'), _features(fb, 'lpips_head')
    if tuple(fa.shape) != tuple(fb.shape) or fa.device != fb.device:
        raise ValueError(f'lpips_head: two feature tensors of one shape on one device, got {tuple(fa.shape)} and {tuple(fb.shape)}')
    if C % 4 or C > 512 or B > 65535 or tuple(lin.shape) != (C,) or lin.device != fa.device or not lin.is_contiguous():
        raise ValueError(f'lpips_head: C % 4 == 0, C <= 512, B <= 65535 and lin of shape ({C},) on {fa.device}, got B {B}, C {C}, lin {tuple(lin.shape)}')
    lib = L.load()
    parts = torch.empty(B * lib.cf_lpips_parts(hw), dtype=torch.float64, device=fa.device)
    out = torch.empty(B, dtype=torch.float64, device=fa.device)
    L.check(lib.cf_lpips_head(L.ptr(fa), L.ptr(fb), L.ptr(lin), B, hw, C, L.ptr(parts, dtype=torch.float64), L.ptr(out, dtype=torch.float64), L.stream_ptr()), 'cf_lpips_head')
    return out


# ---- BiSeNet (cf_bisenet.hip) -- definitions at "BiSeNet / face parsing" in include/codeformer_hip.h --------------------------------------
STEM_K = 148        # K of the 7x7 stem: 3 * 7 * 7 = 147 padded to a multiple of 4
FC_MAX_C, FC_MAX_N = 4096, 512
FC_ACT = {None: 0, 'none': 0, 'relu': 1, 'sigmoid': 2}


def pack_stem7x7(weight):
    """(64,3,7,7) float32 -> the (148,64) layout cf_stem7x7s2 reads: K ascending in (c, ky, kx), the last row zero."""
    if tuple(_f32(weight).shape) != (64, 3, 7, 7):
        raise ValueError(f'pack_stem7x7: a (64,3,7,7) weight, got {tuple(weight.shape)}')
    w = weight.detach().contiguous()
    wp = torch.empty((STEM_K, 64), dtype=torch.float32, device=w.device)
    L.check(L.load().cf_pack_stem7x7(L.ptr(w), L.ptr(wp), L.stream_ptr()), 'cf_pack_stem7x7')
    return wp


def stem7x7s2(x, wp, bias):
    """relu(conv 7x7 / stride 2 / pad 3 + bias) of a dense (B,3,H,W) float32 image -> (B,(H-1)//2+1,(W-1)//2+1,64) channels-last, on the
    fp32 MFMA; wp from pack_stem7x7, bias (64,)."""
    _f32(x)
    if x.dim() != 4 or x.shape[1] != 3 or min(x.shape) < 1 or not x.is_contiguous():
        raise ValueError(f'stem7x7s2: expected a dense float32 (B,3,H,W) image, got {tuple(x.shape)}')
    if tuple(wp.shape) != (STEM_K, 64) or tuple(bias.shape) != (64,):
        raise ValueError(f'stem7x7s2: wp {tuple(wp.shape)} / bias {tuple(bias.shape)} are not a pack_stem7x7 weight and 64 biases')
    B, _, H, W = x.shape
    out = torch.empty((B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 64), dtype=torch.float32, device=x.device)
    L.check(L.load().cf_stem7x7s2(L.ptr(x), L.ptr(wp), L.ptr(bias), B, H, W, L.ptr(out), L.stream_ptr()), 'cf_stem7x7s2')
    return out


def maxpool3s2(x):
    """MaxPool2d(3, 2, 1) of (B,H,W,C) channels-last -> (B,(H-1)//2+1,(W-1)//2+1,C); padding is -inf, a NaN wins."""
    B, H, W, C = _nhwc_dense(x, 'maxpool3s2')
    out = torch.empty((B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C), dtype=torch.float32, device=x.device)
    L.check(L.load().cf_maxpool3s2(L.ptr(x), B, H, W, C, L.ptr(out), L.stream_ptr()), 'cf_maxpool3s2')
    return out


def pooled_fc(pooled, weight, bias, act=None):
    """act(pooled @ weight^T + bias) on (B,C) rows: weight (N,C), bias (N,), act None | 'relu' | 'sigmoid'; one fmaf chain per output in
    ascending c.  C <= FC_MAX_C with C % 4 == 0, N <= FC_MAX_N."""
    B, C = _f32(pooled).shape
    N = weight.shape[0]
    if act not in FC_ACT:
        raise ValueError(f'pooled_fc: act {act!r} (None, relu, sigmoid)')
    if tuple(_f32(weight).shape) != (N, C) or tuple(_f32(bias).shape) != (N,) or C % 4 or C > FC_MAX_C or N > FC_MAX_N:
        raise ValueError(f'pooled_fc: weight {tuple(weight.shape)} / bias {tuple(bias.shape)} do not fit {C} channels (C % 4 == 0, C <= {FC_MAX_C}, N <= {FC_MAX_N})')
    out = torch.empty((B, N), dtype=torch.float32, device=pooled.device)
    L.check(L.load().cf_pooled_fc(L.ptr(pooled), L.ptr(weight), L.ptr(bias), B, C, N, FC_ACT[act], L.ptr(out), L.stream_ptr()), 'cf_pooled_fc')
    return out


def scale_add_row(x, g, r):
    """x * g[b][c] + r[b][c]: x (B,H,W,C), g and r (B,C); multiply and add rounded separately."""
    B, H, W, C = _nhwc_dense(x, 'scale_add_row')
    if tuple(g.shape) != (B, C) or tuple(r.shape) != (B, C):
        raise ValueError(f'scale_add_row: x {tuple(x.shape)}, g {tuple(g.shape)}, r {tuple(r.shape)}')
    out = torch.empty_like(x)
    L.check(L.load().cf_scale_add_row(L.ptr(x), L.ptr(g), L.ptr(r), B, H * W, C, L.ptr(out), L.stream_ptr()), 'cf_scale_add_row')
    return out


def _resize_ac_args(x, c, size, what):
    B, H, W, ld = _nhwc_dense(x, what)
    c = ld if c is None else int(c)
    oh, ow = int(size[0]), int(size[1])
    if not 1 <= c <= ld or oh < 1 or ow < 1:
        raise ValueError(f'{what}: the first {c} of {ld} channels to {oh}x{ow}')
    return B, H, W, ld, c, oh, ow


def resize_bilinear_ac(x, size, c=None):
    """F.interpolate(mode='bilinear', align_corners=True) of the first c channels of (B,h,w,ld) channels-last -> (B,c,H,W) NCHW."""
    B, H, W, ld, c, oh, ow = _resize_ac_args(x, c, size, 'resize_bilinear_ac')
    out = torch.empty((B, c, oh, ow), dtype=torch.float32, device=x.device)
    L.check(L.load().cf_resize_bilinear_ac(L.ptr(x), B, H, W, ld, c, L.ptr(out), oh, ow, L.stream_ptr()), 'cf_resize_bilinear_ac')
    return out


def resize_bilinear_ac_argmax(x, size, c=None):
    """(B,H,W) int64: the per-pixel argmax over the first c channels of what resize_bilinear_ac would write (lowest index among equal
    maxima); the resized values are never stored and channels >= c are never read."""
    B, H, W, ld, c, oh, ow = _resize_ac_args(x, c, size, 'resize_bilinear_ac_argmax')
    out = torch.empty((B, oh, ow), dtype=torch.int64, device=x.device)
    L.check(L.load().cf_resize_bilinear_ac_argmax(L.ptr(x), B, H, W, ld, c, L.ptr(out, dtype=torch.int64), oh, ow, L.stream_ptr()), 'cf_resize_bilinear_ac_argmax')
    return out


# ---- RetinaFace (cf_retina.hip) -- definitions at "RetinaFace ResNet-50 detector" in include/codeformer_hip.h ------------------------------
class PackedPointwise:
    """A 1x1 convolution's weight in the layout cf_pointwise reads (pack_pointwise) and its bias (or None)."""

    def __init__(self, w, bias, cin, cout):
        self.w, self.bias, self.cin, self.cout = w, bias, cin, cout


def pack_pointwise(weight, bias=None):
    """(cout,cin) or (cout,cin,1,1) float32 -> PackedPointwise: rows padded to a multiple of 64, columns to a multiple of 32, with zeros."""
    w = _f32(weight).detach()
    if w.dim() == 4 and tuple(w.shape[2:]) == (1, 1):
        w = w.reshape(w.shape[0], w.shape[1])
    if w.dim() != 2 or w.shape[1] % 4:
        raise ValueError(f'pack_pointwise: a (cout,cin[,1,1]) weight with cin % 4 == 0, got {tuple(weight.shape)}')
    cout, cin = w.shape
    lib = L.load()
    n = lib.cf_pointwise_packed_elems(cin, cout)
    if n <= 0:
        raise ValueError(f'pack_pointwise: bad dims cin {cin}, cout {cout}')
    w = w.contiguous()
    wp = torch.empty(n, dtype=torch.float32, device=w.device)
    L.check(lib.cf_pack_pointwise(L.ptr(w), cin, cout, L.ptr(wp), L.stream_ptr()), 'cf_pack_pointwise')
    if bias is not None and tuple(_f32(bias).shape) != (cout,):
        raise ValueError(f'pack_pointwise: bias {tuple(bias.shape)} for {cout} outputs')
    return PackedPointwise(wp, None if bias is None else bias.detach().contiguous(), cin, cout)


def pointwise(x, pp, *, res=None, relu=False, step=1, out=None):
    """[relu](x @ W^T + bias [+ res]) over the pixels of a channels-last (B,H,W,cin) float32 tensor -> (B,Ho,Wo,cout), one launch on the fp32
    MFMA.  step 2 reads pixel (2y, 2x): Ho = ceil(H / 2), the 1x1 stride-2 convolution.  x, res and `out` may be channel slices
    `buf[..., a:b]` of wider channels-last buffers (x is read four channels at a time: a % 4 == 0 and a buffer width % 4 == 0; res and out are free).  One fixed K order, no split-K: image b is bitwise the call on it alone."""
    _f32(x)
    if x.dim() != 4 or x.shape[3] != pp.cin:
        raise ValueError(f'pointwise: x {tuple(x.shape)} for a weight of {pp.cin} input channels')
    if step not in (1, 2):
        raise ValueError(f'pointwise: step {step} (1 or 2)')
    B, H, W, _ = x.shape
    Ho, Wo = (H + step - 1) // step, (W + step - 1) // step
    shape = (B, Ho, Wo, pp.cout)
    ldx = _nhwc_ld(x, 'x')
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != x.device:
        raise ValueError(f'pointwise: out expected float32 {shape} on {x.device}')
    else:
        _drop_state(out)
    ldo = _nhwc_ld(out, 'out')
    ldr = 0
    if res is not None:
        if tuple(_f32(res).shape) != shape or res.device != x.device:
            raise ValueError(f'pointwise: res {tuple(res.shape)} != {shape}')
        ldr = _nhwc_ld(res, 'res')
    L.check(L.load().cf_pointwise(L.ptr(x, True), ldx, L.ptr(pp.w), L.ptr(pp.bias), L.ptr(res, True), ldr, B, H, W, pp.cin, pp.cout, step,
                                  1 if relu else 0, L.ptr(out, True), ldo, L.stream_ptr()), 'cf_pointwise')
    return out


def nearest_add(a, b):
    """a + F.interpolate(b, size=a's, mode='nearest') on dense channels-last (B,H,W,C) float32 tensors, bitwise the torch expression."""
    B, H, W, C = _nhwc_dense(a, 'nearest_add')
    Bb, Hb, Wb, Cb = _nhwc_dense(b, 'nearest_add')
    if (Bb, Cb) != (B, C):
        raise ValueError(f'nearest_add: a {tuple(a.shape)}, b {tuple(b.shape)}')
    out = torch.empty_like(a)
    L.check(L.load().cf_nearest_add(L.ptr(a), L.ptr(b), B, H, W, Hb, Wb, C, L.ptr(out), L.stream_ptr()), 'cf_nearest_add')
    return out


def retina_decode(heads, priors=None, *, variance=(0.1, 0.2), img_wh=(1.0, 1.0), resize=1.0, conf_threshold=None, cap=0, full=False):
    """The detector's tail.  heads: three dense (B,H_l,W_l,32) float32 tensors, an anchor's 16 values together (4 box, 2 class, 10 landmark).
    full=True: (bbox (B,n,4), softmax (B,n,2), landmarks (B,n,10)), what RetinaFace.forward returns.  conf_threshold given: (rows (B,cap,15),
    counts (B,) int32) -- the decoded, scaled rows [x1, y1, x2, y2, score, 5 x (lx, ly)] of the anchors with score > conf_threshold in
    ascending anchor order and their TRUE number per image (a count above cap: take the full tensors).  One mode per call."""
    if len(heads) != 3:
        raise ValueError('retina_decode: three pyramid levels')
    B, dev = heads[0].shape[0], heads[0].device
    nps = []
    for h in heads:
        b, hh, ww, c = _nhwc_dense(h, 'retina_decode')
        if b != B or c != 32:
            raise ValueError(f'retina_decode: heads of shape {tuple(h.shape)} (B,H,W,32)')
        nps.append(hh * ww)
    n = 2 * sum(nps)
    compact = conf_threshold is not None
    if bool(full) == compact:
        raise ValueError('retina_decode: one mode per call, full=True or a conf_threshold')
    outs = []
    bbox = conf = ldm = rows = counts = None
    if full:
        bbox, conf, ldm = (torch.empty((B, n, k), dtype=torch.float32, device=dev) for k in (4, 2, 10))
        outs += [bbox, conf, ldm]
    if compact:
        if priors is None or tuple(_f32(priors).shape) != (n, 4) or priors.device != dev or cap < 1:
            raise ValueError(f'retina_decode: the compact rows need ({n},4) priors on {dev} and cap >= 1')
        rows = torch.empty((B, cap, 15), dtype=torch.float32, device=dev)
        counts = torch.empty((B,), dtype=torch.int32, device=dev)
        outs += [rows, counts]
    L.check(L.load().cf_retina_decode(L.ptr(heads[0]), L.ptr(heads[1]), L.ptr(heads[2]), nps[0], nps[1], nps[2], L.ptr(priors), B,
                                      float(variance[0]), float(variance[1]), float(img_wh[0]), float(img_wh[1]), float(resize),
                                      float(conf_threshold) if compact else 0.0, L.ptr(bbox), L.ptr(conf), L.ptr(ldm), L.ptr(rows), int(cap),
                                      L.ptr(counts, dtype=torch.int32), L.stream_ptr()), 'cf_retina_decode')
    return tuple(outs)
