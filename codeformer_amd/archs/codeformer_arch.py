"""CodeFormer network, MI355X-native.

API mirror of the reference's basicsr/archs/codeformer_arch.py: `ARCH_REGISTRY.get('CodeFormer')(dim_embd=512,
codebook_size=1024, n_head=8, n_layers=9, connect_list=[...])`, identical state_dict keys / init order, and
`net(x, w=..., adain=...)` -> `(out, logits, lq_feat)` (`code_only=True` -> `(logits, lq_feat)`).

On ROCm tensors `CodeFormer.forward` (reference: codeformer_arch.py:223-280) runs entirely on the HIP kernels of
codeformer_amd/csrc with channels-last activations:
  encoder (fused GN/swish/conv stacks, taps kept by reference instead of .clone())
  -> 9 pre-LN Transformer layers on (B*256, 512) token matrices (LayerNorm kernel, fp32-MFMA GEMMs with bias/GELU/
     residual epilogues, 8-head attention kernel)
  -> logits GEMM -> wavefront-shuffle argmax (== softmax+topk(1), lowest index on ties) -> codebook gather (+AdaIN)
  -> generator with the controllable feature transform fused into conv gathers / epilogues.
"""
import gc
import os
import threading

import math
import numbers

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from .. import ops
from ..ops import EPI_GELU, EPI_RESIDUAL, EPI_SFT, PRO_LEAKY
from ..utils.diagnostics import top2_gap
from ..utils.registry import ARCH_REGISTRY
from .hip_module import PACK_EPOCH, HipModule
from .vqgan_arch import ResBlock, VQAutoEncoder


# Graphed forwards share static input / output buffers per captured shape, so capture and replay are serialised (one lock for the
# process: module attributes must stay picklable / deep-copyable).  The eager path (more than `graph_max_batch` faces) is re-entrant.
_GRAPH_LOCK = threading.RLock()
_CAPTURE_STREAMS = {}    # device -> the stream every graph of this process is captured on (its scratch words exist before the first capture)


def _min_nan(a, b):
    """min of two floats that keeps a NaN once it has one (Python's min() does not)."""
    return b if (b < a or b != b) else a


class FaceWeights:
    """One fidelity weight per face of a batch, read on the host: `host` the B values as the float32 numbers the kernels see, `fused` the
    faces whose weight is > 0 (a NaN is not: the rule `if w > 0` of the scalar call).  With a CUDA `device`: `dev` the float32 (B,) tensor
    the SFT epilogues index by image, and -- for a mixed batch -- `sel_f` / `sel_u`, the int64 row indices of the fused and un-fused faces."""

    def __init__(self, values, device=None):
        values = [float(v) for v in values]
        self.host = tuple(float(np.float32(v)) for v in values)
        self.fused = tuple(v > 0 for v in values)
        self.device = None if device is None else torch.device(device)
        self.dev = self.sel_f = self.sel_u = None
        if self.device is not None and self.device.type == 'cuda':
            self.dev = torch.tensor(self.host, dtype=torch.float32).to(self.device)
            if self.mixed:
                self.sel_f = torch.tensor(self.rows_fused, dtype=torch.int64).to(self.device)
                self.sel_u = torch.tensor(self.rows_unfused, dtype=torch.int64).to(self.device)

    def __len__(self):
        return len(self.host)

    @property
    def rows_fused(self):
        return [i for i, f in enumerate(self.fused) if f]

    @property
    def rows_unfused(self):
        return [i for i, f in enumerate(self.fused) if not f]

    @property
    def all_fused(self):
        return all(self.fused)

    @property
    def none_fused(self):
        return not any(self.fused)

    @property
    def mixed(self):
        return not self.all_fused and not self.none_fused

    def rows(self, idx):
        """The weights of faces `idx` (a list of ints), as a batch of their own."""
        return FaceWeights([self.host[i] for i in idx], self.device)


def is_scalar_weight(w):
    """Whether face_weights() leaves w as it is: the scalar call."""
    return isinstance(w, (numbers.Real, np.number, np.bool_)) or ((torch.is_tensor(w) or isinstance(w, np.ndarray)) and w.ndim == 0)


def face_weights(w, batch, device=None):
    """Normalise the `w` of a call on `batch` faces.  A number (Python / numpy scalar, 0-dim array or tensor) is returned as it is: the
    scalar call.  A sequence, numpy array or tensor of `batch` real values becomes a FaceWeights; the values are read on the host, so a
    device tensor costs one synchronisation.  Another length raises ValueError, anything that is not real numbers TypeError."""
    if isinstance(w, FaceWeights):
        if len(w) != batch:
            raise ValueError(f'w holds {len(w)} weights for a batch of {batch} faces')
        return w
    if isinstance(w, (numbers.Real, np.number, np.bool_)):      # (what `w > 0` and float(w) take today; np.str_ and the like are no numbers)
        return w
    if torch.is_tensor(w):
        if w.dim() == 0:
            return w
        if w.dtype == torch.bool or w.is_complex():
            raise TypeError(f'w: expected real weights, got a {w.dtype} tensor')
        if w.dim() != 1 or w.numel() != batch:
            raise ValueError(f'w: expected one weight per face ({batch}), got a tensor of shape {tuple(w.shape)}')
        vals = w.detach().to('cpu', torch.float64).tolist()      # (a device tensor: the one synchronisation)
    elif isinstance(w, np.ndarray):
        if w.ndim == 0:
            return w.item()
        if w.dtype.kind not in 'fiu':
            raise TypeError(f'w: expected real weights, got a numpy array of {w.dtype}')
        if w.ndim != 1 or w.shape[0] != batch:
            raise ValueError(f'w: expected one weight per face ({batch}), got an array of shape {w.shape}')
        vals = w.astype(np.float64).tolist()
    elif isinstance(w, (list, tuple)):
        if len(w) != batch:
            raise ValueError(f'w: expected one weight per face ({batch}), got {len(w)} values')
        for v in w:
            if isinstance(v, (bool, np.bool_)) or not (isinstance(v, (numbers.Real, np.number)) or (torch.is_tensor(v) and v.dim() == 0 and v.dtype != torch.bool)):
                raise TypeError(f'w: expected real weights, got {type(v).__name__} in the sequence')
        vals = [float(v) for v in w]
    else:
        raise TypeError(f'w: expected a number or one weight per face (sequence, numpy array, tensor), got {type(w).__name__}')
    return FaceWeights(vals, device)


def calc_mean_std(feat, eps=1e-5):
    """Per-(b,c) mean and sqrt(unbiased var + eps) of a 4-D tensor (codeformer_arch.py:12-26); host helper."""
    assert feat.dim() == 4, 'The input feature should be 4D tensor.'
    b, c = feat.shape[:2]
    flat = feat.reshape(b, c, -1)
    std = (flat.var(dim=2) + eps).sqrt().view(b, c, 1, 1)
    mean = flat.mean(dim=2).view(b, c, 1, 1)
    return mean, std


def adaptive_instance_normalization(content_feat, style_feat):
    """AdaIN (codeformer_arch.py:29-43).  NCHW in/out; on GPU the statistics + re-normalisation run in
    cf_codebook_gather_adain only inside CodeFormer.forward -- this free function is the host helper."""
    size = content_feat.size()
    style_mean, style_std = calc_mean_std(style_feat)
    content_mean, content_std = calc_mean_std(content_feat)
    normalized = (content_feat - content_mean.expand(size)) / content_std.expand(size)
    return normalized * style_std.expand(size) + style_mean.expand(size)


class TransformerSALayer(HipModule):
    """Pre-LN self-attention + MLP layer (codeformer_arch.py:99-134).

    GPU path works on batch-major token matrices X[(b*256 + t), 512] (the NHWC view of the 16x16 latent), i.e.
    the reference's (T, B, C) sequence-first tensor with the first two axes swapped.
    """

    def __init__(self, embed_dim, nhead=8, dim_mlp=2048, dropout=0.0, activation='gelu'):
        super().__init__()
        if activation != 'gelu':
            raise RuntimeError(f'activation should be gelu for the MI355X path, not {activation}.')
        self.self_attn = nn.MultiheadAttention(embed_dim, nhead, dropout=dropout)
        self.linear1 = nn.Linear(embed_dim, dim_mlp)
        self.dropout = nn.Dropout(dropout)
        self.linear2 = nn.Linear(dim_mlp, embed_dim)
        self.norm1 = nn.LayerNorm(embed_dim)
        self.norm2 = nn.LayerNorm(embed_dim)
        self.dropout1 = nn.Dropout(dropout)
        self.dropout2 = nn.Dropout(dropout)
        self.embed_dim, self.nhead = embed_dim, nhead

    def with_pos_embed(self, tensor, pos):
        return tensor if pos is None else tensor + pos

    def forward_tokens(self, X, pos, batch, code=0, code_ln=None):
        """X: (batch*256, E) tokens, pos: (256, E) or None.  Returns the layer output, same shape.
        code: operand code of the five GEMMs (0 exact fp32 MFMA, ops.GSPLIT split-half operands); code_ln: the code of the three that
        read a LayerNorm output (q|k, v, MLP-up; default: `code`) -- their inputs are bounded by the norm's parameters (ln_code)."""
        E, H = self.embed_dim, self.nhead
        sa = self.self_attn
        w, b = sa.in_proj_weight, sa.in_proj_bias
        code_ln = code if code_ln is None else code_ln
        c1 = ln_code(self, self.norm1, code_ln, pos)
        c2 = ln_code(self, self.norm2, code_ln)
        # out-proj reads convex combinations of v = Wv LN1(x) + bv, MLP-down reads GELU(W1 LN2(x) + b1) with |GELU(h)| <= |h|: both inherit
        # a bound from the norm's parameters and one weight matrix (bounded_code); `code` (gemm_precision='f16x2') overrides the check
        c_o = code or bounded_code(self, 'o', code_ln, self.norm1, w[2 * E:], b[2 * E:])
        c_d = code or bounded_code(self, 'd', code_ln, self.norm2, self.linear1.weight, self.linear1.bias)
        pw_o = self._pw_conv(sa.out_proj, bf16=c_o)
        if pos is not None:
            t2, t2p = ops.layernorm(X, self.norm1.weight, self.norm1.bias, self.norm1.eps, pos=pos)
        else:
            t2 = t2p = ops.layernorm(X, self.norm1.weight, self.norm1.bias, self.norm1.eps)
        if c1 == ops.GSPLIT and (2 * E) % 128 == 0:
            # split-half token GEMM: the whole in_proj (3 E rows) in ONE launch -- the q | k columns contract LN(x) + pos, the v columns LN(x)
            # (cf_conv_desc.in0_alt; per output element the arithmetic of the two launches below -- with ONE power-of-two pack scale for the whole
            #  in_proj instead of one per part, so q, k, v agree with the two-launch form to the last bits of the 22-bit operands, not bitwise)
            pw_qkv = self._packed(('qkv', c1), lambda: ops.pack_weight(w, b, bf16=c1), w, b)
            qkv = ops.linear(t2p, pw_qkv, x_alt=t2, alt_from=2 * E)
            q, k, v = qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:]
        else:
            pw_qk = self._packed(('qk', c1), lambda: ops.pack_weight(w[:2 * E], b[:2 * E], bf16=c1), w, b)
            pw_v = self._packed(('v', c1), lambda: ops.pack_weight(w[2 * E:], b[2 * E:], bf16=c1), w, b)
            qk = ops.linear(t2p, pw_qk)                      # q | k share the (LN(x)+pos) input
            v = ops.linear(t2, pw_v)                         # v = LN(x) without pos (codeformer_arch.py:125-126)
            q, k = qk[:, :E], qk[:, E:]
        hd = E // H
        a = ops.attention(q, k, v, batch, H, hd, float(hd) ** -0.5)
        X = ops.linear(a, pw_o, epilogue=EPI_RESIDUAL, res=X)
        t2 = ops.layernorm(X, self.norm2.weight, self.norm2.bias, self.norm2.eps)
        h = ops.linear(t2, self._pw_conv('linear1', bf16=c2), epilogue=EPI_GELU)
        return ops.linear(h, self._pw_conv('linear2', bf16=c_d), epilogue=EPI_RESIDUAL, res=X)

    def forward(self, tgt, tgt_mask=None, tgt_key_padding_mask=None, query_pos=None):
        """tgt: (T=256, B, E) sequence-first like the reference."""
        if tgt.is_cuda:
            if tgt_mask is not None or tgt_key_padding_mask is not None:
                raise NotImplementedError('attention masks are not part of the CodeFormer inference path')
            with torch.no_grad():
                T, B, E = tgt.shape
                X = tgt.float().transpose(0, 1).contiguous().view(B * T, E)
                pos = None
                if query_pos is not None:
                    pos = query_pos.float()[:, 0, :].contiguous()   # the reference broadcasts one table over the batch
                Y = self.forward_tokens(X, pos, B)
                return Y.view(B, T, E).transpose(0, 1).contiguous()
        tgt2 = self.norm1(tgt)
        q = k = self.with_pos_embed(tgt2, query_pos)
        tgt2 = self.self_attn(q, k, value=tgt2, attn_mask=tgt_mask, key_padding_mask=tgt_key_padding_mask)[0]
        tgt = tgt + self.dropout1(tgt2)
        tgt2 = self.norm2(tgt)
        tgt2 = self.linear2(self.dropout(F.gelu(self.linear1(tgt2))))
        return tgt + self.dropout2(tgt2)


def ln_code(module, norm, code, pos=None):
    """Operand code of a Linear layer that reads LayerNorm `norm`'s output (+ the position table): `code`, or 0 (exact fp32) when the bound
    max_i(|gamma_i| sqrt(C - 1) + |beta_i|) + max|pos| could leave the IEEE-half range of the split-half token GEMM, which has no range
    scale.  The maxima are read back once per parameter version (HipModule._packed)."""
    if int(code) != ops.GSPLIT:
        return int(code)
    params = (norm.weight, norm.bias) + (() if pos is None else (pos,))
    bound = module._packed(('ln_range', id(norm), pos is not None),
                           lambda: float((norm.weight.detach().abs() * math.sqrt(norm.weight.numel() - 1) + norm.bias.detach().abs()).max())
                           + (0.0 if pos is None else float(pos.detach().abs().max())), *params)
    return ops.GSPLIT if bound < 32768.0 else 0


def bounded_code(module, tag, code, norm, weight, bias):
    """Operand code of a Linear layer whose input is bounded by max_n(|W| L + |b|)_n with L = |gamma| sqrt(C - 1) + |beta| the bound of
    LayerNorm `norm`'s output and (W, b) the Linear layer in between (out-proj: the value projection -- attention outputs are convex
    combinations of values; MLP-down: the MLP-up layer -- |GELU(h)| <= |h|): `code` while that stays inside the IEEE-half range of the
    split-half token GEMM, else 0 (exact fp32).  One matrix-vector product per parameter version."""
    if int(code) != ops.GSPLIT:
        return int(code)

    def bound():
        L = norm.weight.detach().abs().float() * math.sqrt(norm.weight.numel() - 1) + norm.bias.detach().abs().float()
        v = weight.detach().abs().float() @ L
        if bias is not None:
            v = v + bias.detach().abs().float()
        return float(v.max())
    params = (norm.weight, norm.bias, weight) + (() if bias is None else (bias,))
    return ops.GSPLIT if module._packed(('lin_range', tag), bound, *params) < 32768.0 else 0


class Fuse_sft_block(HipModule):
    """Controllable feature transform (codeformer_arch.py:136-157):
    e = ResBlock(cat[enc, dec]); out = dec + w * (dec * scale(e) + shift(e)).

    GPU: the concat is two base pointers in the conv gather; LeakyReLU(0.2) is the gather prologue of the second
    conv of each branch; the SFT combine is the epilogue of the last `shift` conv.
    """

    def __init__(self, in_ch, out_ch):
        super().__init__()
        self.encode_enc = ResBlock(2 * in_ch, out_ch)
        self.scale = nn.Sequential(nn.Conv2d(in_ch, out_ch, kernel_size=3, padding=1), nn.LeakyReLU(0.2, True),
                                   nn.Conv2d(out_ch, out_ch, kernel_size=3, padding=1))
        self.shift = nn.Sequential(nn.Conv2d(in_ch, out_ch, kernel_size=3, padding=1), nn.LeakyReLU(0.2, True),
                                   nn.Conv2d(out_ch, out_ch, kernel_size=3, padding=1))

    def forward_nhwc(self, enc, dec, w=1, bf16=False):
        e = self.encode_enc.forward_nhwc(enc, dec, bf16=bf16)
        hw = e.shape[1:3]
        if int(bf16) == 2 and not ops.wsingle_ok(e.shape[3], e.shape[3], hw[0], hw[1]):
            bf16 = ops.SPLIT   # (single IEEE halves on the direct kernel have no range scaling; un-normalised inputs need it)
        # The four convs below read UN-NORMALISED tensors (e; the outputs of scale.0 / shift.0): on the 16-bit-operand kernels each
        # gets a per-image power-of-two range scale derived from the statistics its producer wrote (ops.act_scale).
        pws = [self._pw_conv(m, bf16, hw=hw) for m in (self.scale[0], self.scale[2], self.shift[0], self.shift[2])]
        rs = [ops.needs_act_scale(p) for p in pws]
        act_e = ops.act_scale(e) if (rs[0] or rs[2]) else None
        if rs[1] and rs[3]:
            # both second convolutions want a table: the two first convolutions write their statistics into one buffer and ONE launch turns
            # them into both tables (bitwise act_scale of each) -- 4 launches fewer per forward
            pair = ops.StatsPair()
            s0 = ops.conv2d(e, pws[0], act=act_e, emit_stats=True, stats_into=pair)
            h = ops.conv2d(e, pws[2], act=act_e, emit_stats=True, stats_into=pair)
            act_s, act_h = ops.act_scale_pair(pair, e.shape[0])
        else:
            s0 = ops.conv2d(e, pws[0], act=act_e, emit_stats=rs[1])
            h = ops.conv2d(e, pws[2], act=act_e, emit_stats=rs[3])
            act_s, act_h = (ops.act_scale(s0) if rs[1] else None), (ops.act_scale(h) if rs[3] else None)
        s = ops.conv2d(s0, pws[1], prologue=PRO_LEAKY, act=act_s)
        # w: a number, or a float32 (B,) tensor on the device -- one weight per face, indexed by image in the epilogue (cf_conv2d_sft_w)
        per_face = torch.is_tensor(w) and w.dim() == 1
        return ops.conv2d(h, pws[3], prologue=PRO_LEAKY, epilogue=EPI_SFT, res=dec, sft_scale=s, sft_w=w if per_face else float(w), emit_stats=True, act=act_h)

    def forward(self, enc_feat, dec_feat, w=1):
        """w: a number, or a tensor of B values -- one weight per face (GPU: float32 on the inputs' device)."""
        if torch.is_tensor(w) and w.dim() == 1 and w.shape[0] != dec_feat.shape[0]:
            raise ValueError(f'w: expected one weight per face ({dec_feat.shape[0]}), got {w.shape[0]}')
        if enc_feat.is_cuda:
            with torch.no_grad():
                out = self.forward_nhwc(ops.to_nhwc(enc_feat.float()), ops.to_nhwc(dec_feat.float()), w)
                return ops.to_nchw(out)
        enc = self.encode_enc(torch.cat([enc_feat, dec_feat], dim=1))
        if torch.is_tensor(w) and w.dim() == 1:
            w = w.to(dec_feat.dtype).view(-1, 1, 1, 1)
        return dec_feat + w * (dec_feat * self.scale(enc) + self.shift(enc))


@ARCH_REGISTRY.register()
class CodeFormer(VQAutoEncoder):

    def __init__(self, dim_embd=512, n_head=8, n_layers=9, codebook_size=1024, latent_size=256,
                 connect_list=['32', '64', '128', '256'], fix_modules=['quantize', 'generator'], vqgan_path=None):
        super().__init__(512, 64, [1, 2, 2, 4, 4, 8], 'nearest', 2, [16], codebook_size)
        if vqgan_path is not None:
            self.load_state_dict(torch.load(vqgan_path, map_location='cpu')['params_ema'])
        if fix_modules is not None:
            for name in fix_modules:
                for p in getattr(self, name).parameters():
                    p.requires_grad = False

        # Operand format of the convolutions (3x3 stride 1 / 2 / folded upsample and, for the split-half codes, the 1x1 skips on images).
        # Tensors, accumulation, attention, statistics and the code argmax are fp32 in every mode; the Transformer's Linear layers: see
        # gemm_precision.
        #   'f16x2' (default): fp32 operands split into hi + lo IEEE halves (22 significant bits), three f16 MFMAs per product, fp32
        #            accumulation, in the Winograd F(2x2,3x3) domain where the layer allows it (cf_wsplit.hip / cf_winograd.hip H2; folded
        #            upsample, stride-2 and image-sized 1x1 convs: cf_split.hip), for generator, CFT and -- see encoder_precision -- the encoder.  Per layer at or below
        #            the fp64-error of the exact kernels; whole network vs the reference on real crops: pixels 7.2e-5 (exact path
        #            7.1e-5; tolerance 1e-3), logits 6.7e-6 (exact: 7.6e-6; tolerance 1e-4), code indices identical.  1.5x the exact
        #            path's faces/s.
        #   'fp32':  everything on exact fp32 MFMA operands (Winograd where eligible: F(2x2,3x3), and F(4x4,3x3) in generator / CFT, see below).
        #   'bf16' (BASELINE configs 3/5) / 'fp16': single 16-bit operands with fp32 accumulate in generator + CFT -- in the Winograd domain
        #            (one MFMA per transform-domain product, cf_wsplit.hip) for the 128-channel-tile layers from 32x32 up, the direct 16-bit
        #            kernel elsewhere; the encoder runs as in the default mode (split halves, fp32-grade), so logits and code indices are
        #            bitwise those of 'f16x2' (pixel gates in tests/test_gpu_real_images.py).
        self.precision = os.environ.get('CODEFORMER_HIP_PRECISION', 'f16x2')
        # precision 'bf16' as BASELINE configs 3 / 5 define it: "bf16 storage + fp32 accumulate in generator + CFT" (round 6).  With the
        # switch on (default) every generator / fusion-block activation of more than 1024 pixels per image -- the 64x64 .. 512x512 levels,
        # 99.6 % of the decoder's bytes -- lives in HBM as bf16: the producing epilogue rounds once, after its GroupNorm partials were taken
        # from the fp32 accumulators; consumers widen on load; the four encoder taps the fusion blocks read get a bf16 copy.  Encoder,
        # Transformer, argmax, the 16x16 / 32x32 latents (AttnBlocks, AdaIN) stay fp32, so logits and code indices are bitwise those of the
        # default mode.  CODEFORMER_HIP_BF16_STORAGE=0 / False: bf16 OPERANDS on fp32 tensors (rounds 2-5).
        self.bf16_storage = os.environ.get('CODEFORMER_HIP_BF16_STORAGE', '1') != '0'
        # Exact-fp32 convolutions (precision='fp32', and in every mode the layers the split kernel does not take) evaluate 3x3 stride-1
        # convolutions with Winograd F(2x2,3x3) where the shape allows -- the same function in fp32 with 2.25x fewer multiplies
        # (cf_winograd.hip); the encoder too, in every precision mode.  Precision 'f16x2' and 'fp32': generator / CFT layers the F(4x4,3x3)
        # kernel covers (ops.f43_ok) run there (split-half / IEEE-fp32 operands) -- 2.25 instead of 4 transform-domain products per output.
        # Its error against fp64 is ~5x that of F(2x2,3x3): far inside the pixel tolerance; the encoder's use of it has its own switch and
        # gate (next attribute).
        # The same kernel for the ENCODER's covered layers (the 64-channel 512^2, 128-channel 256^2 / 128^2 stages and, for fp32 operands, the
        # 256-channel 64^2 stage): on by default since round 5 (CODEFORMER_HIP_F43_ENCODER=0 / False: F(2x2,3x3) there, the round-2..4 encoder).
        # The encoder decides the code indices and F(4x4,3x3) carries ~5x the per-layer error of F(2x2,3x3), so the switch was admitted on
        # a measured margin, not on "no index changed": for every golden token whose reference top-2 gap is >= 1e-5 the ratio
        # (reference gap) / (2 x max |our logit - reference logit|) must stay >= 5 (review of round 4) -- measured 7.0 (split halves) /
        # 7.3 (fp32 operands) with the switch on against 9.9 / 8.7 with it off, over the seeded face, the three real crops, the masked face,
        # the four range variants and the 32-face sweep; no index differs anywhere; logits move by 5-11e-6 (tolerance 1e-4).  It buys 4 % of
        # the step in the default mode and 9 % in 'fp32'.  With fp32 operands the switch also puts the 512-channel 16^2 and 256-channel 32^2 latent
        # layers on the K-part form of F(4x4,3x3) (ops.WINOGRAD_F43K): the smallest fp32 margin is then 6.3, no index differs, the largest logit
        # error on those goldens stays at 1.0e-5 (profiles/NOTES.md).  Gate: tests/test_gpu_real_images.py::test_encoder_logit_margin (tools/logit_margin.py,
        # profiles/r05_logit_margin.txt).
        self.winograd_f43_encoder = os.environ.get('CODEFORMER_HIP_F43_ENCODER', '1') == '1'
        # Logit guard (CODEFORMER_HIP_LOGIT_GUARD): the gate above was measured with random-init weights only, so the network can watch the
        # quantity it was about.  'off' (default): nothing changes.  'report': the launch that takes the code argmax also writes every
        # token's top-2 logit gap and its minimum per face (cf_argmax_rows_gap) -> `last_min_gap` (B,), no host synchronisation.
        # 'rerun': the B minima are read back once per call, and every face with `not (min gap >= logit_guard_gap)` (a NaN flags) runs
        # again, eagerly and in one batch, with the encoder on F(2x2,3x3); its rows of every returned tensor, of `last_indices` and of
        # `last_min_gap` are replaced.  The forward is bitwise batch-invariant, so an unflagged face is bitwise the guard-off face and a
        # flagged one bitwise the face of a winograd_f43_encoder=False network.  Totals: `guard_stats` / reset_guard_stats().
        # logit_guard_gap (CODEFORMER_HIP_LOGIT_GUARD_GAP) is an ABSOLUTE logit difference and comes from that gate, not from a new
        # measurement: required margin 5 x 2 x the largest F(4x4,3x3) logit error recorded for it (1.1e-5, profiles/r06_logit_margin.txt)
        # = 1.1e-4 -- an error measured with random-init weights; a trained checkpoint may want another value.
        self.logit_guard = os.environ.get('CODEFORMER_HIP_LOGIT_GUARD', 'off')
        self.logit_guard_gap = float(os.environ.get('CODEFORMER_HIP_LOGIT_GUARD_GAP', '1.1e-4'))
        self.reset_guard_stats()
        # Operand format of the ENCODER's 3x3 stride-1 convolutions: 'fp32' (exact fp32 MFMA, Winograd where eligible), 'f16x2' (split
        # halves on every layer but the first conv -- the 16x16 latents included, on the four-wave Winograd kernel with split-K) or
        # 'auto' = 'fp32' when precision is 'fp32', 'f16x2' otherwise (a 16-bit generator does not ask for an exact-fp32 encoder at 0.54 of the fp32 MFMA peak).  The code indices hang on the encoder, so this was measured before it became the
        # default (tools/encoder_split_check.py, profiles/r02_encoder_split_check.txt): against the reference's logits on its own
        # crops the split encoder is as close as the exact one (max 6.7e-6 / 5.4e-6 / 5.7e-6 vs 7.6e-6 / 5.5e-6 / 6.0e-6; the
        # reference's own 1-vs-8-thread noise is 2.6e-6), the smallest (reference top-2 gap) / (2 x our logit error) over all tokens
        # is 9.1 (exact: 8.8), and every index of every golden agrees.  Set 'fp32' to keep logits bitwise equal across precisions.
        self.encoder_precision = os.environ.get('CODEFORMER_HIP_ENCODER_PRECISION', 'auto')
        # Operand format of the Transformer's Linear layers (feat_emb, q|k / v / out projections, MLP, logits head): 'fp32' = exact fp32
        # MFMA GEMM; 'f16x2' = split-half operands (cf_gemm_split.hip) everywhere -- opt-in: the token GEMM has no range scale and the
        # inputs of out-proj / MLP-down / feat_emb are not bounded by anything the host can check; 'auto' (default) = split halves for the
        # Linear layers whose input the host can bound from parameters -- those behind a LayerNorm (q|k, v, MLP-up, the logits head:
        # |gamma| sqrt(C - 1) + |beta| (+ |pos|), ln_code) and those one Linear layer further (out-proj, MLP-down: bounded_code), 46 of 47
        # launches -- while the bound stays inside the half range and neither `precision` nor `encoder_precision` is 'fp32' (so that
        # encoder_precision = 'fp32' alone keeps the logits bitwise identical across modes); exact fp32 elsewhere (feat_emb reads the
        # un-normalised encoder feature).
        # Against fp64 the split-half GEMM is closer than the fp32-MFMA one (1.2e-6 vs 2.0e-6); logits / indices vs the reference unchanged.
        self.gemm_precision = os.environ.get('CODEFORMER_HIP_GEMM_PRECISION', 'auto')
        # Optional HIP-graph replay of the whole forward (one graph per input shape / w / flags): takes the ~250 host launches
        # per call off the critical path.  Measured: no gain at B=1..16 on an otherwise idle host (the kernels, not the launches,
        # bound even B=1), so it is off by default; useful when the host thread is busy (decode / encode of PNGs).
        # Round 3 re-measurement: with the faster kernels a one-face call is host-bound in places when run eagerly (the Transformer section:
        # 1.6 ms of host enqueue for 0.9 ms of GPU work), and replay takes the whole call from 6.76 to 6.55 ms on a box where the host is the
        # slower side.  Round 4: 'auto' (default) replays a graph for batches of at most `graph_max_batch` faces -- the reference's own call
        # pattern is one face per call (inference_codeformer.py:197-206) -- behind a parameter signature (sum of the parameters' versions
        # and storage addresses, ~70 us per call): a versioned in-place update, load_state_dict, .to() or invalidate_packed_weights() all
        # re-capture; only an un-versioned `.data` edit needs the explicit invalidate_packed_weights() the packed-weight cache needs too.
        # '1': every batch size; '0': never.  At most four captured graphs are kept (each pins the activations of its shape).
        # A scalar w is part of the key (each value its own graph); one weight per face is a static device buffer of the graph and the key
        # holds only which faces are fused, so every all-positive vector of a batch size replays one graph.  `graph_captures` counts captures.
        self.use_hip_graphs = {'0': False, '1': True}.get(os.environ.get('CODEFORMER_HIP_GRAPHS', 'auto'), 'auto')
        self.graph_max_batch = 4
        self._graphs = {}
        self.graph_captures = 0
        self.connect_list = connect_list
        self.n_layers = n_layers
        self.n_head = n_head
        self.dim_embd = dim_embd
        self.dim_mlp = dim_embd * 2
        self.latent_size = latent_size

        self.position_emb = nn.Parameter(torch.zeros(latent_size, self.dim_embd))
        self.feat_emb = nn.Linear(256, self.dim_embd)
        self.ft_layers = nn.Sequential(*[
            TransformerSALayer(embed_dim=dim_embd, nhead=n_head, dim_mlp=self.dim_mlp, dropout=0.0)
            for _ in range(self.n_layers)])
        self.idx_pred_layer = nn.Sequential(nn.LayerNorm(dim_embd), nn.Linear(dim_embd, codebook_size, bias=False))

        self.channels = {'16': 512, '32': 256, '64': 256, '128': 128, '256': 128, '512': 64}
        # encoder tap after the 2nd ResBlock of a level; generator fusion after the 1st ResBlock of a level
        self.fuse_encoder_block = {'512': 2, '256': 5, '128': 8, '64': 11, '32': 14, '16': 18}
        self.fuse_generator_block = {'16': 6, '32': 9, '64': 12, '128': 15, '256': 18, '512': 21}
        self.fuse_convs_dict = nn.ModuleDict()
        for f_size in self.connect_list:
            ch = self.channels[f_size]
            self.fuse_convs_dict[f_size] = Fuse_sft_block(ch, ch)

    # ------------------------------------------------------------------ GPU (HIP) path
    def _encode_hip(self, x, code_only, adain, f43_encoder=None, guard=False, u8=False):
        """Everything of the forward that does not depend on w: encoder, Transformer, code argmax, codebook gather (+ AdaIN).  Returns a
        dict: logits, lq_feat, idx (B, T), quant (B,16,16,256; None with code_only), enc_feat (the encoder taps by size).
        f43_encoder: the encoder's F(4x4,3x3) choice of THIS call (None: self.winograd_f43_encoder; the logit guard's second pass
        hands False down instead of flipping the attribute -- two threads may share a network).  guard: take the argmax on
        cf_argmax_rows_gap and leave the per-face minimum top-2 gap in `last_min_gap` (with code_only too).
        u8 (restore_u8, which checked the tensors): x is the uint8 (B,512,512,3) BGR batch, read by the first conv."""
        if u8:
            B = x.shape[0]
        else:
            B, _, Himg, Wimg = x.shape
            if (Himg, Wimg) != (512, 512):
                raise ValueError(f'CodeFormer expects aligned 512x512 faces, got {Himg}x{Wimg}')
            x = x.float().contiguous()
        enc_feat = {}
        enc_taps = {self.fuse_encoder_block[f]: (lambda t: enc_feat.__setitem__(str(t.shape[2]), t))
                    for f in self.connect_list}
        if self.encoder_precision not in ('auto', 'fp32', 'f16x2'):
            raise ValueError(f"encoder_precision must be 'auto', 'fp32' or 'f16x2', got {self.encoder_precision!r}")
        enc_code = ops.SPLIT if self.encoder_precision == 'f16x2' or (self.encoder_precision == 'auto' and self.precision != 'fp32') else ops.WINOGRAD
        if self.winograd_f43_encoder if f43_encoder is None else f43_encoder:
            enc_code = {ops.SPLIT: ops.SPLIT_F43, ops.WINOGRAD: ops.WINOGRAD_F43K}[enc_code]
        lq = self.encoder.forward_nhwc(x, enc_taps, bf16=enc_code, img_u8=u8)        # (B,16,16,256) channels-last
        T = lq.shape[1] * lq.shape[2]
        tokens = lq.view(B * T, lq.shape[3])

        if self.gemm_precision not in ('auto', 'fp32', 'f16x2'):
            raise ValueError(f"gemm_precision must be 'auto', 'fp32' or 'f16x2', got {self.gemm_precision!r}")
        gcode = ops.GSPLIT if self.gemm_precision == 'f16x2' else 0
        # 'auto' follows the encoder: encoder_precision = 'fp32' alone keeps logits bitwise identical across the precision modes
        gcode_ln = ops.GSPLIT if (self.gemm_precision == 'f16x2' or (self.gemm_precision == 'auto' and self.precision != 'fp32' and self.encoder_precision != 'fp32')) else 0
        X = ops.linear(tokens, self._pw_conv('feat_emb', bf16=gcode))
        for layer in self.ft_layers:
            X = layer.forward_tokens(X, self.position_emb, B, code=gcode, code_ln=gcode_ln)
        ln, head = self.idx_pred_layer[0], self.idx_pred_layer[1]
        logits2d = ops.linear(ops.layernorm(X, ln.weight, ln.bias, ln.eps), self._pw_conv(head, bf16=ln_code(self, ln, gcode_ln)))
        res = {'logits': logits2d.view(B, T, -1), 'lq_feat': ops.to_nchw(lq), 'idx': None, 'quant': None, 'enc_feat': enc_feat}
        if guard:
            idx, _, self.last_min_gap = ops.argmax_rows_gap(logits2d, T)   # the same indices + each face's smallest top-2 logit gap
            res['idx'] = idx.view(B, T)
        if code_only:
            return res

        if not guard:
            idx = ops.argmax_rows(logits2d)                                 # == topk(softmax(logits), 1)
            res['idx'] = idx.view(B, T)
        quant = ops.codebook_gather(idx, self.quantize.embedding.weight, B, T,
                                    lq=tokens.view(B, T, -1) if adain else None)
        res['quant'] = quant.view(B, lq.shape[1], lq.shape[2], -1)
        if self.precision not in ('fp32', 'f16x2', 'bf16', 'fp16'):
            raise ValueError(f"precision must be 'fp32', 'f16x2', 'bf16' or 'fp16', got {self.precision!r}")
        return res

    def _generate_hip(self, quant, enc_feat, w, u8=False, out_u8=None):
        """The generator on `quant` (B,16,16,256) with the fusion blocks reading `enc_feat`.  w: a number (a 0-dim tensor included) -- fused iff w > 0 -- or a float32
        (B,) device tensor, one weight per face, all of them fused.  u8: the last conv writes the uint8 (B,512,512,3) image (into out_u8
        when given), which is returned in place of the NCHW tensor."""
        B = quant.shape[0]
        # operand code of the generator + CFT 3x3 convs; 'fp32': F(4x4,3x3) on fp32 operands (four v_mfma_f32_16x16x4_f32 per 16 channels
        # instead of three f16 MFMAs), in K parts of 128 input channels on the 16x16 / 32x32 layers (ops.f43k_ok; the encoder's latent layers take the
        # same code under winograd_f43_encoder, _encode_hip); 'f16x2': the encoder gets SPLIT_F43 through winograd_f43_encoder only (_encode_hip)
        bf16 = {'fp32': ops.WINOGRAD_F43K,'f16x2': ops.SPLIT_F43, 'bf16': 1, 'fp16': 2}[self.precision]
        gen_taps = None
        if (torch.is_tensor(w) and w.dim() == 1) or w > 0:      # (a 0-dim tensor is a number: `w > 0` decides, as ever)
            def fuse(t):
                f = str(t.shape[2])
                enc = enc_feat[f]
                if t.dtype == torch.bfloat16:    # bf16 storage: the fusion block concatenates [enc, dec] -- the tap gets its bf16 copy
                    enc = ops.to_bf16(enc)
                return self.fuse_convs_dict[f].forward_nhwc(enc, t, w, bf16=bf16)
            gen_taps = {self.fuse_generator_block[f]: fuse for f in self.connect_list}
        if u8 and out_u8 is None:
            out_u8 = torch.empty((B, 512, 512, 3), dtype=torch.uint8, device=quant.device)
        return self.generator.forward_nhwc(quant, gen_taps, bf16=bf16, storage_bf16=bool(self.bf16_storage) and bf16 == 1,
                                           img_out=out_u8 if u8 else None)      # (B,3,512,512) NCHW, or the uint8 (B,512,512,3) image

    def _generate_rows_hip(self, e, w, u8=False, out_u8=None):
        """The generator for the faces of _encode_hip's result `e` under w, a number or a FaceWeights.  A mixed FaceWeights runs it twice --
        the fused faces with their weights, the others un-fused, each selected with ops.select_rows from quant and the encoder taps --
        and scatters the rows back into place; the forward is bitwise batch-invariant, so every row is bitwise its own scalar call."""
        quant, enc_feat = e['quant'], e['enc_feat']
        if not isinstance(w, FaceWeights):
            return self._generate_hip(quant, enc_feat, w, u8, out_u8)
        if w.none_fused:
            return self._generate_hip(quant, enc_feat, 0.0, u8, out_u8)
        if w.all_fused:
            return self._generate_hip(quant, enc_feat, w.dev, u8, out_u8)
        B = quant.shape[0]
        out = out_u8 if out_u8 is not None else torch.empty((B, 512, 512, 3) if u8 else (B, 3, 512, 512), dtype=torch.uint8 if u8 else torch.float32, device=quant.device)
        taps = {f: ops.select_rows(t, w.sel_f) for f, t in enc_feat.items()}
        out.index_copy_(0, w.sel_f, self._generate_hip(ops.select_rows(quant, w.sel_f), taps, w.dev.index_select(0, w.sel_f), u8))
        out.index_copy_(0, w.sel_u, self._generate_hip(ops.select_rows(quant, w.sel_u), None, 0.0, u8))
        return out

    def _forward_hip(self, x, w, code_only, adain, f43_encoder=None, guard=False, u8=False, out_u8=None):
        """w: a number or a FaceWeights (one weight per face).  f43_encoder / guard / u8: see _encode_hip; with u8 the first returned
        tensor is the uint8 (B,512,512,3) image the last conv wrote -- into out_u8 when given."""
        e = self._encode_hip(x, code_only, adain, f43_encoder, guard, u8)
        if code_only:
            if guard:
                self.last_indices = e['idx']
            return e['logits'], e['lq_feat']
        out = self._generate_rows_hip(e, w, u8, out_u8)
        self.last_indices = e['idx']
        return out, e['logits'], e['lq_feat']

    # ------------------------------------------------------------------ host (CPU tensors) path
    def _encode_host(self, x, detach_16, code_only, adain):
        """The part of the host forward that does not depend on w -> (logits, lq_feat, quant or None, enc_feat)."""
        enc_feat = {}
        out_list = [self.fuse_encoder_block[f] for f in self.connect_list]
        for i, block in enumerate(self.encoder.blocks):
            x = block(x)
            if i in out_list:
                enc_feat[str(x.shape[-1])] = x.clone()
        lq_feat = x
        pos_emb = self.position_emb.unsqueeze(1).repeat(1, x.shape[0], 1)
        query = self.feat_emb(lq_feat.flatten(2).permute(2, 0, 1))
        for layer in self.ft_layers:
            query = layer(query, query_pos=pos_emb)
        logits = self.idx_pred_layer(query).permute(1, 0, 2)
        if self.logit_guard != 'off':   # the host path has one encoder: the gap is reported and counted, nothing is run again
            self.last_min_gap = top2_gap(logits)[0].min(dim=1).values
            self._guard_count(self.last_min_gap)
        if code_only:
            return logits, lq_feat, None, enc_feat
        _, top_idx = torch.topk(F.softmax(logits, dim=2), 1, dim=2)
        quant = self.quantize.get_codebook_feat(top_idx, shape=[x.shape[0], 16, 16, 256])
        if detach_16:
            quant = quant.detach()
        if adain:
            quant = adaptive_instance_normalization(quant, lq_feat)
        return logits, lq_feat, quant, enc_feat

    def _generate_host(self, x, enc_feat, w):
        """The generator on the host; w: a number (fused iff w > 0) or a (B,) tensor of positive weights, one per face."""
        fused = (torch.is_tensor(w) and w.dim() == 1) or w > 0      # (a 0-dim tensor is a number: `w > 0` decides, as ever)
        fuse_list = [self.fuse_generator_block[f] for f in self.connect_list]
        for i, block in enumerate(self.generator.blocks):
            x = block(x)
            if i in fuse_list and fused:
                f = str(x.shape[-1])
                x = self.fuse_convs_dict[f](enc_feat[f].detach(), x, w)
        return x

    def _generate_rows_host(self, quant, enc_feat, w):
        """_generate_rows_hip on the host: a FaceWeights partitions the rows the same way."""
        if not isinstance(w, FaceWeights):
            return self._generate_host(quant, enc_feat, w)
        if w.none_fused:
            return self._generate_host(quant, enc_feat, 0.0)
        wt = torch.tensor(w.host, dtype=torch.float32)
        if w.all_fused:
            return self._generate_host(quant, enc_feat, wt)
        rf, ru = w.rows_fused, w.rows_unfused
        of = self._generate_host(quant[rf], {f: t[rf] for f, t in enc_feat.items()}, wt[rf])
        ou = self._generate_host(quant[ru], None, 0.0)
        out = of.new_empty((quant.shape[0],) + tuple(of.shape[1:]))
        out[rf] = of
        out[ru] = ou
        return out

    def _forward_host(self, x, w, detach_16, code_only, adain):
        logits, lq_feat, quant, enc_feat = self._encode_host(x, detach_16, code_only, adain)
        if code_only:
            return logits, lq_feat
        return self._generate_rows_host(quant, enc_feat, w), logits, lq_feat

    def _forward_graphed(self, x, w, code_only, adain, guard=False, u8=False, out_u8=None):
        """Capture-once / replay-many execution of _forward_hip on the current stream.  Outputs are copies, so callers may
        keep them across calls.  A graph is re-captured when any packed weight was rebuilt since its capture.
        u8: the uint8 form of _forward_hip -- the static input is the uint8 batch, the boundary form is part of the key, and the image
        is copied into out_u8 when given.
        w: a number -- part of the key, as ever -- or a FaceWeights: the key then holds which faces are fused, not the values; the weights
        are a static device buffer of the graph (the FaceWeights of the capturing call), copied into before each replay."""
        with _GRAPH_LOCK:   # static buffers per shape: two threads replaying one graph would race on them
            per_face = isinstance(w, FaceWeights)
            key = (tuple(x.shape), ('per-face', w.fused) if per_face else float(w), bool(code_only), bool(adain), self.precision, bool(self.bf16_storage), self.encoder_precision, self.gemm_precision, bool(self.winograd_f43_encoder), str(x.device), ops.switches(), bool(guard), bool(u8))
            ent = self._graphs.get(key)
            sig = self._param_signature()
            if ent is None or ent['epoch'] != PACK_EPOCH[0] or ent['sig'] != sig:
                static_x = x.clone() if u8 else x.float().contiguous().clone()
                for _ in range(2):                      # warm-up: packs weights, sets kernel attributes, primes the allocator
                    self._forward_hip(static_x, w, code_only, adain, guard=guard, u8=u8)
                torch.cuda.synchronize(x.device)
                graph = torch.cuda.CUDAGraph()
                # The zero-initialised scratch words of the range-scale / split-K kernels are kept per (device, stream).  Created inside the
                # capture they would be two fill launches of every replay (three with the workspace of the K-part F(4,3) layers, which comes
                # from the same pool): create them for the capture stream first, outside the capture.
                cap = _CAPTURE_STREAMS.get(str(x.device))
                if cap is None:
                    cap = _CAPTURE_STREAMS[str(x.device)] = torch.cuda.Stream(device=x.device)
                with torch.cuda.stream(cap):
                    ops._act_cells(x.device, 4 * max(int(x.shape[0]), 1))
                    ops._counters(x.device, 4096)
                    if self.precision == 'fp32':    # the K-part F(4,3) layers' partial sums: this network's largest layer is 512 -> 256 @ 32x32, 2^20 words per face
                        ops._kpart_ws(x.device, max(int(x.shape[0]), 1) << 20)
                cap.synchronize()
                # No garbage collection while capturing: a dead network (each one holds itself in _sig_modules, so it waits for the
                # cyclic collector) takes its captured graphs with it, and tearing a graph down during a capture aborts the process.
                gc_on = gc.isenabled()
                gc.disable()
                try:
                    with torch.cuda.graph(graph, stream=cap):
                        outs = self._forward_hip(static_x, w, code_only, adain, guard=guard, u8=u8)
                finally:
                    if gc_on:
                        gc.enable()
                ent = {'graph': graph, 'x': static_x, 'outs': outs, 'epoch': PACK_EPOCH[0], 'sig': sig, 'idx': getattr(self, 'last_indices', None),
                       'gap': self.last_min_gap if guard else None, 'w': w if per_face else None}
                self.graph_captures += 1
                self._graphs.pop(key, None)
                while len(self._graphs) >= 4:           # oldest first: a graph pins the activations of its shape
                    self._graphs.pop(next(iter(self._graphs)))
                self._graphs[key] = ent
            ent['x'].copy_(x)
            if per_face and ent['w'] is not w:
                ent['w'].dev.copy_(w.dev)
            ent['graph'].replay()
            if ent['idx'] is not None:
                self.last_indices = ent['idx'].clone()   # (a fresh tensor per call, as the eager path returns: the next replay overwrites the graph's own)
            if ent['gap'] is not None:
                self.last_min_gap = ent['gap'].clone()   # (the same ownership rule)
            if out_u8 is not None:
                return (out_u8.copy_(ent['outs'][0]),) + tuple(o.clone() for o in ent['outs'][1:])
            return tuple(o.clone() for o in ent['outs'])

    def _param_signature(self):
        """(sum of versions, sum of storage addresses, sum of object ids) over the parameters and buffers CURRENTLY registered in the
        module tree: changes with every versioned in-place update, every re-allocation and every replaced Parameter object
        (`m.weight = nn.Parameter(...)`, parametrize, an EMA swap).  The list of modules is cached (rebuilt by load_state_dict / _apply /
        invalidate_packed_weights, and here when a sub-module was replaced: the ids of all children are part of the walk); their
        `_parameters` / `_buffers` dictionaries are read on every call (~0.15 ms)."""
        for _ in range(2):
            mods = self.__dict__.get('_sig_modules')
            if mods is None:
                mods = list(self.modules())
                self.__dict__['_sig_modules'] = mods
                self.__dict__['_sig_children'] = sum(id(c) for m in mods for c in m._modules.values() if c is not None)
            ver = ptr = ident = kids = 0
            for m in mods:
                for t in m._parameters.values():
                    if t is not None:
                        ver += ops.tensor_version(t) or 0
                        ptr += t.data_ptr()
                        ident += id(t)
                for t in m._buffers.values():
                    if t is not None:
                        ver += ops.tensor_version(t) or 0
                        ptr += t.data_ptr()
                        ident += id(t)
                for c in m._modules.values():
                    if c is not None:
                        kids += id(c)
            if kids == self.__dict__['_sig_children']:
                break
            self.__dict__.pop('_sig_modules', None)   # a sub-module was replaced or added: walk the new tree
        return (ver, ptr, ident)

    def load_state_dict(self, *args, **kwargs):
        self._graphs.clear()                       # captured graphs point at the old packed weights
        self.__dict__.pop('_sig_modules', None)
        return super().load_state_dict(*args, **kwargs)

    def _apply(self, fn, *args, **kwargs):         # .to() / .cuda() / .float(): parameters move, graphs are stale
        if getattr(self, '_graphs', None):
            self._graphs.clear()
        self.__dict__.pop('_sig_modules', None)
        return super()._apply(fn, *args, **kwargs)

    def invalidate_packed_weights(self):
        self._graphs.clear()
        self.__dict__.pop('_sig_modules', None)
        super().invalidate_packed_weights()

    # ------------------------------------------------------------------ logit guard
    def reset_guard_stats(self):
        """Zero the running totals of the logit guard (`guard_stats`)."""
        self._guard_totals = {'calls': 0, 'faces': 0, 'flagged': 0, 'rerun_faces': 0, 'index_changes': 0, 'min_gap': float('inf')}
        self._guard_pending = []   # 'report' on the device: (last_min_gap, threshold, None) of calls not read back yet

    @property
    def guard_stats(self):
        """Running totals of the logit guard: `calls`, `faces`, `flagged` (faces with `not (min gap >= logit_guard_gap)`), `rerun_faces`,
        `index_changes` (tokens of re-run faces whose code index differs between the two passes) and `min_gap` (the smallest first-pass gap
        seen; NaN once a NaN was seen).  'report' adds no synchronisation to a call: its minima are read back here."""
        self._guard_fold(sync=True)
        return dict(self._guard_totals)

    def _guard_count(self, gmin, thr=None):
        """Add the faces of one call, given their minima on the host, to the totals; returns the flagged mask."""
        thr = self.logit_guard_gap if thr is None else thr
        flag = ~(gmin >= thr)
        st = self._guard_totals
        st['calls'] += 1
        st['faces'] += int(gmin.numel())
        st['flagged'] += int(flag.sum())
        st['min_gap'] = _min_nan(st['min_gap'], float(gmin.min()))
        return flag

    def _guard_fold(self, sync):
        """Reduce the pending 'report' minima to one (minimum, threshold, flagged count) entry on the device -- no synchronisation;
        sync=True: read it into the totals."""
        pend = self._guard_pending
        if not pend:
            return
        flagged = torch.stack([(~(g >= t)).sum() if f is None else f for g, t, f in pend]).sum()
        gmin = torch.cat([g.reshape(-1) for g, _, _ in pend]).min()           # (torch.min hands a NaN on)
        pend[:] = [(gmin, None, flagged)]
        if sync:
            st = self._guard_totals
            st['flagged'] += int(flagged)
            st['min_gap'] = _min_nan(st['min_gap'], float(gmin))
            pend.clear()

    def _guard_first_pass(self, faces):
        """The bookkeeping behind a first pass that ran with guard=True on `faces` faces (forward, restore_u8, restore_sweep) -> (flag, gmin):
        gmin that pass's last_min_gap; flag the host mask of the faces to run again, or None when nothing is ('report': the minima are
        queued, no read-back; 'rerun': the one read-back of the call -- no face flagged, or an F(2x2,3x3) encoder, which has nothing to
        fall back to: faces are counted only)."""
        gmin = self.last_min_gap
        if self.logit_guard == 'report':
            st = self._guard_totals
            st['calls'] += 1
            st['faces'] += int(faces)
            self._guard_pending.append((gmin, float(self.logit_guard_gap), None))
            if len(self._guard_pending) >= 64:
                self._guard_fold(sync=False)
            return None, gmin
        flag = self._guard_count(gmin.cpu())
        if not bool(flag.any()) or not self.winograd_f43_encoder:
            return None, gmin
        return flag, gmin

    def _guard_second_pass(self, sel, gmin, idx, idx2):
        """... and behind the second pass on the faces `sel`: the totals, and the flagged rows of last_min_gap (gmin: the first pass's,
        self.last_min_gap: the second's).  idx / idx2: the code indices of all faces in the first pass / of the flagged ones in the second."""
        st = self._guard_totals
        st['rerun_faces'] += int(sel.numel())
        st['index_changes'] += int((idx.index_select(0, sel) != idx2).sum())
        self.last_min_gap = gmin.index_copy_(0, sel, self.last_min_gap)

    def _forward_guarded(self, x, w, code_only, adain, graphed, u8=False, out_u8=None):
        outs = (self._forward_graphed if graphed else self._forward_hip)(x, w, code_only, adain, guard=True, u8=u8, out_u8=out_u8)
        flag, gmin = self._guard_first_pass(x.shape[0])
        if flag is None:
            return outs
        sel = flag.nonzero().flatten().to(x.device)
        idx = self.last_indices
        # second pass: the flagged faces as one batch, eagerly (it neither captures a graph nor evicts one)
        w2 = w.rows(flag.nonzero().flatten().tolist()) if isinstance(w, FaceWeights) else w    # (the flagged faces keep their own weights)
        outs2 = self._forward_hip(x.index_select(0, sel), w2, code_only, adain, f43_encoder=False, guard=True, u8=u8)
        self._guard_second_pass(sel, gmin, idx, self.last_indices)
        for o, o2 in zip(outs, outs2):
            o.index_copy_(0, sel, o2)
        self.last_indices = idx.index_copy_(0, sel, self.last_indices)
        return outs

    def _forward_cuda(self, x, w, code_only, adain, **u8):
        """The dispatch forward and restore_u8 share: graph replay by the use_hip_graphs / graph_max_batch rule, the logit guard, else eager."""
        ops.L.ensure_device(x.device)   # kernel attributes on the tensor's device, before (never inside) a capture
        with torch.no_grad(), torch.cuda.device(x.device):
            if torch.cuda.is_current_stream_capturing() and not is_scalar_weight(w):
                raise RuntimeError('w: one weight per face is read on the host and uploaded on every call, which a stream capture of the '
                                   "caller's does not allow; inside your own capture pass a number (or capture per fused pattern yourself "
                                   'around Fuse_sft_block / ops.conv2d with a device tensor)')
            w = face_weights(w, x.shape[0], x.device)
            if isinstance(w, FaceWeights) and w.none_fused:
                w = 0.0      # no face is fused: the scalar call's un-fused path, and its graph
            graphed = self.use_hip_graphs is True or (self.use_hip_graphs == 'auto' and x.shape[0] <= self.graph_max_batch)
            graphed = graphed and ops.PROFILE is None and not torch.cuda.is_current_stream_capturing()
            if self.logit_guard != 'off':
                return self._forward_guarded(x, w, code_only, adain, graphed, **u8)
            if graphed:
                return self._forward_graphed(x, w, code_only, adain, **u8)
            return self._forward_hip(x, w, code_only, adain, **u8)

    def forward(self, x, w=0, detach_16=True, code_only=False, adain=False):
        """w: the fidelity weight -- a number for the whole batch, or one weight per face (a sequence, numpy array or tensor of B values;
        they are read on the host and uploaded on every call: a device tensor costs one synchronisation, and neither form can be used while
        the caller is capturing a stream of their own -- a number can, as ever).  Face b is fused iff w_b > 0 (a NaN is not).  All fused:
        one generator pass with the weights on the device; none: the un-fused pass; mixed: encoder, Transformer and code lookup once for
        all faces, the generator once for the fused faces and once un-fused for the rest.  Every row is bitwise the one-face call with
        its own scalar w; logits, lq_feat, last_indices and last_min_gap do not depend on w."""
        if self.logit_guard not in ('off', 'report', 'rerun'):
            raise ValueError(f"logit_guard must be 'off', 'report' or 'rerun', got {self.logit_guard!r}")
        if x.is_cuda:
            return self._forward_cuda(x, w, code_only, adain)
        return self._forward_host(x, face_weights(w, x.shape[0]), detach_16, code_only, adain)

    def restore_sweep(self, x, ws, adain=False):
        """One batch at several fidelity weights: x (B,3,512,512), ws K weights -> (outs (K,B,3,512,512), logits, lq_feat), with
        outs[k, b] bitwise forward(x[b:b+1], w=ws[k], adain=adain)[0][0] on the GPU.  Encoder, Transformer, code argmax, gather and AdaIN run
        once for the B faces; the positive weights are ONE generator pass over B x (their number) rows (quant and the encoder taps repeated
        per weight, the weights per row on the device), all weights <= 0 (or NaN) share one un-fused pass.  Eager (no graph is captured or
        replayed); logit_guard is honoured ('rerun': the flagged faces take the encoder again before any generator pass and go through the
        generator as a batch of their own)."""
        if self.logit_guard not in ('off', 'report', 'rerun'):
            raise ValueError(f"logit_guard must be 'off', 'report' or 'rerun', got {self.logit_guard!r}")
        ws = np.asarray(ws.detach().cpu() if torch.is_tensor(ws) else ws)
        if ws.ndim != 1 or ws.shape[0] < 1:
            raise ValueError(f'restore_sweep: ws must hold K >= 1 weights, got shape {ws.shape}')
        wk = face_weights(ws, ws.shape[0])        # (K "faces": the same reading of the values and of what is fused)
        B, K = x.shape[0], len(wk)
        pos, neg = wk.rows_fused, wk.rows_unfused
        with torch.no_grad():
            if x.is_cuda:
                ops.L.ensure_device(x.device)
                with torch.cuda.device(x.device):
                    e, groups = self._encode_guarded_hip(x, adain)
                    outs = torch.empty((K, B, 3, 512, 512), dtype=torch.float32, device=x.device)
                    pos_idx = torch.tensor(pos, dtype=torch.int64).to(x.device)
                    for rows, quant, taps in groups:       # (one group -- all faces -- unless the logit guard re-ran some of them)
                        n = quant.shape[0]
                        rows = torch.arange(B, dtype=torch.int64).to(x.device) if rows is None else rows
                        if pos:
                            rep = torch.arange(n, dtype=torch.int64).repeat(len(pos)).to(x.device)
                            wv = torch.tensor([wk.host[k] for k in pos for _ in range(n)], dtype=torch.float32).to(x.device)
                            o = self._generate_hip(ops.select_rows(quant, rep), {f: ops.select_rows(t, rep) for f, t in taps.items()}, wv)
                            outs[pos_idx[:, None], rows[None, :]] = o.view(len(pos), n, 3, 512, 512)
                        if neg:
                            o = self._generate_hip(quant, None, 0.0)
                            for k in neg:
                                outs[k].index_copy_(0, rows, o)
                    self.last_indices = e['idx']
                    return outs, e['logits'], e['lq_feat']
            logits, lq_feat, quant, enc_feat = self._encode_host(x, True, False, adain)
            outs = None
            if pos:
                rep = list(range(B)) * len(pos)
                wv = torch.tensor([wk.host[k] for k in pos for _ in range(B)], dtype=torch.float32)
                o = self._generate_host(quant[rep], {f: t[rep] for f, t in enc_feat.items()}, wv)
                outs = o.new_empty((K, B) + tuple(o.shape[1:]))
                outs[pos] = o.view((len(pos), B) + tuple(o.shape[1:]))
            if neg:
                o = self._generate_host(quant, None, 0.0)
                outs = o.new_empty((K, B) + tuple(o.shape[1:])) if outs is None else outs
                for k in neg:
                    outs[k] = o
            return outs, logits, lq_feat

    def _encode_guarded_hip(self, x, adain):
        """_encode_hip under the logit guard, for restore_sweep -> (e, groups): e with the logits, lq_feat and indices of all faces, and
        groups = [(rows or None, quant, encoder taps)], what the generator reads, per group of faces.  One group (rows None: all faces)
        unless 'rerun' flagged some: those ran again, as a batch of their own, with the encoder on F(2x2,3x3) -- their rows of logits, lq_feat,
        indices and last_min_gap are replaced, and they form the second group (the taps of the two encoders carry statistics partials of
        different kernels: they are not merged).  'report' queues the minima as a forward does."""
        e = self._encode_hip(x, False, adain, guard=self.logit_guard != 'off')
        one = [(None, e['quant'], e['enc_feat'])]
        if self.logit_guard == 'off':
            return e, one
        flag, gmin = self._guard_first_pass(x.shape[0])
        if flag is None:
            return e, one
        sel, keep = flag.nonzero().flatten().to(x.device), (~flag).nonzero().flatten().to(x.device)
        e2 = self._encode_hip(x.index_select(0, sel), False, adain, f43_encoder=False, guard=True)
        self._guard_second_pass(sel, gmin, e['idx'], e2['idx'])
        groups = [(sel, e2['quant'], e2['enc_feat'])]
        if keep.numel():
            groups.append((keep, ops.select_rows(e['quant'], keep), {f: ops.select_rows(t, keep) for f, t in e['enc_feat'].items()}))
        for k in ('logits', 'lq_feat', 'idx'):
            e[k].index_copy_(0, sel, e2[k])
        return e, groups

    def restore_u8(self, faces, w=0.5, adain=True, out=None):
        """uint8 (B,512,512,3) BGR aligned faces -> the restored faces in the same form: the bytes of
        ops.tensor_to_img_u8(self(ops.img_u8_to_tensor(faces), w=w, adain=adain)[0]), with the conversions folded into the first and the
        last conv (cf_conv2d_u8) -- no fp32 image tensor exists at either end.  Dispatch (graph replay, logit guard: 'rerun' replaces the
        flagged faces' rows), `last_indices` and `last_min_gap` are those of forward.
        w: a number or one weight per face, as in forward.
        out: a contiguous uint8 (B,512,512,3) destination on faces' device (e.g. a `[:m]` slice of a larger buffer); it is returned.
        CPU tensors take the host path with the converters of utils/img_util.py."""
        if self.logit_guard not in ('off', 'report', 'rerun'):
            raise ValueError(f"logit_guard must be 'off', 'report' or 'rerun', got {self.logit_guard!r}")
        for t, what in ((faces, 'faces'), (out, 'out')):
            if t is None and what == 'out':
                continue
            if not torch.is_tensor(t) or t.dtype != torch.uint8 or t.dim() != 4 or tuple(t.shape[1:]) != (512, 512, 3) or not t.is_contiguous():
                raise ValueError(f'restore_u8: {what} must be a contiguous uint8 (B,512,512,3) BGR tensor, got '
                                 f'{(t.dtype, tuple(t.shape), t.stride()) if torch.is_tensor(t) else type(t)}')
        if out is not None and (out.shape[0] != faces.shape[0] or out.device != faces.device):
            raise ValueError(f'restore_u8: out is {tuple(out.shape)} on {out.device}, faces {tuple(faces.shape)} on {faces.device}')
        if faces.is_cuda:
            return self._forward_cuda(faces, w, False, adain, u8=True, out_u8=out)[0]
        from ..utils.img_util import img2tensor, normalize_, tensor2img
        with torch.no_grad():
            x = torch.stack([normalize_(img2tensor(f / 255., bgr2rgb=True, float32=True), (0.5, 0.5, 0.5), (0.5, 0.5, 0.5)) for f in faces.numpy()])
            y = self._forward_host(x, face_weights(w, x.shape[0]), True, False, adain)[0]
            res = torch.stack([torch.from_numpy(tensor2img(y[i], rgb2bgr=True, min_max=(-1, 1))) for i in range(y.shape[0])])
        return res if out is None else out.copy_(res)
