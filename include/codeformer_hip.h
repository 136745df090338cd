/*
 * codeformer_hip.h -- C ABI of libcodeformer_hip.so (gfx950 / MI355X).
 *
 * Drop-in boundary for the CodeFormer aligned-face hot path
 * (reference: basicsr/archs/codeformer_arch.py:223-280 CodeFormer.forward and the
 * VQGAN blocks of basicsr/archs/vqgan_arch.py).  The reference has no FFI on this
 * path: every arithmetic step is a PyTorch ATen call issued from Python.  Each
 * entry point below therefore cites the ATen call site(s) of the reference that
 * it replaces.  The Python host (codeformer_amd/lib.py) binds these with ctypes.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (torch.empty allocations);
 *   - every function only ENQUEUES work on `stream` (a hipStream_t passed as void*);
 *     nothing synchronises, nothing allocates, there is no global mutable state
 *     besides the thread-local last-error string (the table cf_device_init() walks is
 *     filled while the library loads and constant afterwards);
 *   - cf_device_init() is called once per device (with that device current) before the
 *     first launch there: kernels with more than 64 KB of dynamic LDS fail to launch without it;
 *   - return 0 on success, <0 on error (cf_last_error() describes it);
 *   - activations are fp32, channels-last ("NHWC": [batch][h][w][c]) unless a flag
 *     says NCHW; token matrices are row-major [rows][cols] (the same memory).
 */
#ifndef CODEFORMER_HIP_H
#define CODEFORMER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CF_ABI_VERSION 22
#define CF_SPLITK_IN_WORKGROUP (-1) /* cf_conv_desc.split_k: see there (ABI v21) */

typedef void* cf_stream_t; /* hipStream_t */

enum cf_status {
  CF_OK = 0,
  CF_ERR_ARG = -1,      /* unsupported shape / null pointer */
  CF_ERR_LAUNCH = -2,   /* HIP launch error */
};

int cf_version(void);
/* sha256 (first 16 hex digits) of the sources this library was compiled from (csrc + this header), passed by the build script
 * as -DCF_BUILD_ID; "unknown" for hand builds.  codeformer_amd/build.py rebuilds when it differs from the tree's hash. */
const char* cf_build_id(void);
const char* cf_last_error(void);
/* number of compute units of the current device (for host-side grid heuristics) */
int cf_device_cu_count(void);
/* Per-device setup (ABI v18): sets hipFuncAttributeMaxDynamicSharedMemorySize -- a per-device property of a function -- for every
 * kernel of the library that launches with more than 64 KB of dynamic LDS, on the CURRENT device.  Idempotent; call it once per
 * device before the first launch there (codeformer_amd/lib.py does, keyed by torch.cuda.current_device()).  Until v17 every launch
 * site kept a function-static bitmap of initialised devices instead -- mutable state this header promises not to have. */
int cf_device_init(void);

/* ---- convolution / linear as implicit GEMM on fp32 MFMA ------------------------------------
 * Replaces: F.conv2d 3x3 s1 p1 (vqgan_arch.py:132,147,149,243,266,292,314; codeformer_arch.py:142-149),
 *           pad(0,1,0,1)+conv 3x3 s2 (vqgan_arch.py:120-126), nearest x2 + conv (vqgan_arch.py:134-138),
 *           conv 1x1 (vqgan_arch.py:151,173-200), nn.Linear (codeformer_arch.py:104,106,183,192 and the
 *           MultiheadAttention in/out projections), with the surrounding elementwise work fused:
 *           GroupNorm-apply + swish (vqgan_arch.py:14-20), LeakyReLU(0.2) (codeformer_arch.py:143,148),
 *           torch.cat([enc,dec]) (codeformer_arch.py:152), residual adds, GELU (codeformer_arch.py:132),
 *           the SFT combine dec + w*(dec*scale+shift) (codeformer_arch.py:155-156).
 */
enum cf_prologue {
  CF_PRO_NONE = 0,
  CF_PRO_AFFINE = 1,        /* x*scale[b][c] + shift[b][c]                (GroupNorm apply)         */
  CF_PRO_AFFINE_SWISH = 2,  /* y = x*scale+shift ; y*sigmoid(y)           (GroupNorm apply + swish) */
  CF_PRO_LEAKY = 3,         /* x>0 ? x : 0.2*x                                                       */
};
enum cf_epilogue {
  CF_EPI_NONE = 0,      /* acc + bias                                      */
  CF_EPI_RESIDUAL = 1,  /* acc + bias + res                                */
  CF_EPI_SFT = 2,       /* res + sft_w*(res*sft_scale + (acc + bias))      */
  CF_EPI_GELU = 3,      /* gelu_erf(acc + bias)                            */
  /* dense-block family (Real-ESRGAN RRDBNet, basicsr/archs/rrdbnet_arch.py:32-62,111-119); alpha = sft_w */
  CF_EPI_LEAKY = 4,     /* leaky_relu_0.2(acc + bias)                      */
  CF_EPI_AXPY = 5,      /* (acc + bias) * alpha + res        (x5 * 0.2 + x, rrdbnet_arch.py:39)          */
  CF_EPI_AXPY2 = 6,     /* ((acc + bias) * alpha + res) * alpha + res2 ; res2 = sft_scale
                           (last conv of an RRDB: both residuals of rrdbnet_arch.py:39 and :62 in one pass) */
  /* nn.PReLU with ONE learned slope (ResNetArcFace, basicsr/archs/arcface_arch.py:73,87,98); alpha = sft_w, any real value (negative, zero,
     above 1): prelu(x, alpha) = x > 0 ? x : alpha * x -- a select, not max(x, alpha * x).  CF_EPI_LEAKY above is NOT this with alpha = 0.2
     passed in: its slope 0.2 is a constant of the kernel and sft_w is ignored there.  Enum values added without a version bump (no struct
     change); instantiations of their own beside the general ones of CF_EPI_LEAKY .. CF_EPI_AXPY2 -- which therefore keep their code --: plain 3x3,
     fp32 operands, stride 1, or stride 2 with pad_lo = 1 / cout_pad % 128 == 0; strided slices and off-grid sizes as there. */
  CF_EPI_PRELU = 7,     /* prelu(acc + bias, alpha)                        */
  CF_EPI_RES_PRELU = 8, /* prelu((acc + bias) + res, alpha)   (IRBlock: out += residual; prelu, :97-98) */
};

/* MFMA operand format (cf_conv_desc.bf16_mfma; the field keeps its ABI-v3 name) */
enum cf_operand {
  CF_OPERAND_F32 = 0,   /* v_mfma_f32_32x32x2_f32, exact fp32 */
  CF_OPERAND_BF16 = 1,  /* v_mfma_f32_32x32x16_bf16; weight from cf_pack_conv_weight[_up2x]_bf16 */
  CF_OPERAND_F16 = 2,   /* v_mfma_f32_32x32x16_f16; weight from cf_pack_conv_weight[_up2x]_f16.  The operand format of the
                           reference's half-precision Real-ESRGAN (inference_codeformer.py:23-27,44); same speed as bf16
                           with 3 more mantissa bits (conv inputs here are O(1): no range problem) */
  CF_OPERAND_F16X2 = 3, /* fp32-grade accuracy on the f16 MFMA pipe: every fp32 operand is split x = hi + lo into two IEEE halves
                           (22 significant bits) and a product is hi*hi + hi*lo + lo*hi -- three v_mfma_f32_32x32x16_f16 with fp32
                           accumulation (cf_split.hip).  Weight from cf_pack_conv_weight_f16x2, acc_scale = 1 / its scale.  3x3
                           stride-1 NHWC convolutions (plain or `upsample`), channels % 32 == 0, cout % 64 == 0, 16x16-tile sizes;
                           prologues as the fp32 kernels, epilogues none / residual / SFT, statistics supported.  Since ABI v17 also
                           stride 2 (Downsample, vqgan_arch.py:117-126: pad_lo == 0, one dense input, c0 % 16 == 0, output a multiple
                           of 8x16): a 2x2 convolution of the space-to-depth view of the input, weight packed with form 2; prologue none /
                           leaky only (an affine prologue is refused: its [batch][c0] tables would be indexed by the view's 4 c0 channels).
                           NON-FINITE INPUTS in that form: seven of its sixteen (tap, parity) weight blocks are zero by construction.
                           With c0 % 32 == 0 each is a whole 32-channel slab and is skipped, and a NaN / inf pixel reaches exactly the
                           outputs whose 3x3 window holds it.  With c0 % 32 == 16 (and under the A/B switch CF_S2_SKIP=0 at any c0) the
                           zeros are multiplied, 0 * NaN is NaN, and the pixel (r, q) reaches every output (oy, ox) with
                           2 oy <= r <= 2 oy + 3 and 2 ox <= q <= 2 ox + 3 -- the 2x2 window of the space-to-depth view, one output row /
                           column more than the 3x3 window for an odd r / q.  Finite inputs give the same bits either way; the network's
                           own stride-2 layers have c0 % 32 == 0 (tests/test_gpu_conv_geom.py pins both sets) */
};

/* Border handling of the 3x3 gather (general instantiations; CodeFormer itself only uses zero padding) */
enum cf_pad {
  CF_PAD_ZERO = 0,     /* F.conv2d(padding=1) / Downsample's F.pad(0,1,0,1) */
  CF_PAD_REFLECT = 1,  /* nn.ReflectionPad2d(1) before an unpadded conv (facelib/parsing/parsenet.py:99,107-109) */
  CF_PAD_EDGE = 2,     /* with `upsample`: reflection padding of the nearest-x2 image == edge replication of the source,
                          so the folded sub-pixel kernel clamps its 2x2 footprint (parsenet.py:96-97,105-109) */
};

typedef struct cf_conv_desc {
  const float* in0;       /* first input  [batch][hin][win][c0]  (or NCHW when in_nchw) */
  const float* in1;       /* optional second input, channel-concatenated after in0      */
  int32_t c0, c1;         /* channels of in0 / in1 (c1 = 0: none); both multiples of 16 unless in_nchw */
  int32_t batch, hin, win;
  int32_t hout, wout;     /* s1: hin<<upsample ; s2: hin/2 */
  int32_t cout;           /* valid output channels */
  int32_t cout_pad;       /* packed weight rows (multiple of the N tile: 32/64/128) */
  int32_t taps;           /* 1 or 9 */
  int32_t stride;         /* 1 or 2 (2: pad right/bottom only, vqgan_arch.py:123) */
  int32_t upsample;       /* 1: nearest x2 + 3x3 (vqgan_arch.py:134-138) computed as four 2x2 sub-pixel convolutions of the
                             SOURCE tensor (taps folded at pack time: 4 instead of 9 MACs per weight, mathematically
                             identical); `weight` must come from cf_pack_conv_weight_up2x[_bf16].  With winograd == 2 and
                             CF_OPERAND_F32 see there: 1 or 2 selects the form */
  int32_t in_nchw;        /* 1: in0 is NCHW with c0 <= 4 channels (network input) */
  int32_t out_nchw;       /* 1: write out as NCHW (network output) */
  int32_t prologue;       /* enum cf_prologue */
  int32_t epilogue;       /* enum cf_epilogue */
  const float* pro_scale; /* [batch][c0+c1] */
  const float* pro_shift; /* [batch][c0+c1] */
  const float* weight;    /* packed by cf_pack_conv_weight */
  const float* bias;      /* [cout] or NULL */
  const float* res;       /* [batch][hout][wout][cout] (RESIDUAL / SFT: the `dec` tensor) */
  const float* sft_scale; /* [batch][hout][wout][cout] (SFT) */
  float sft_w;            /* SFT: the weight w of every image (one per image: cf_conv2d_sft_w); LEAKY / AXPY family: alpha */
  float* out;
  double* stats_out;      /* optional: fp64 partial (sum, sumsq) of the OUTPUT per (image, group of stats_cpg channels,
                             tile part), layout [batch][cout/stats_cpg][parts][2], parts = cf_conv2d_stats_parts(d);
                             feeds cf_groupnorm_finalize so the next GroupNorm never re-reads the tensor */
  int32_t stats_cpg;      /* channels per statistics group: power of two in [2,32] dividing cout */
  int32_t bf16_mfma;      /* enum cf_operand.  1: `weight` was packed by cf_pack_conv_weight_bf16 and the contraction runs on
                             v_mfma_f32_32x32x16_bf16 (activations rounded to bf16 after the prologue, fp32 accumulate,
                             fp32 tensors in HBM); 3x3 stride-1 NHWC only.  Used by the bf16 configurations for the
                             generator / CFT convolutions -- never for encoder or Transformer (code indices stay exact) */
  /* Channel strides (floats per pixel) of in0 / in1 / out when they are channel SLICES of wider NHWC buffers; 0 = dense
   * (c0 / c1 / cout).  res and res2 share ld_out.  A dense block (rrdbnet_arch.py:32-39) keeps x1..x4 in one 128-channel
   * buffer: conv_k reads cat(x, growth[:, :32(k-1)]) through (in0, in1, ld_in1 = 128) and writes its 32 channels in place
   * at out = growth + 32(k-1), ld_out = 128 -- torch.cat never materialises.  Any stride other than dense, the epilogues
   * >= CF_EPI_LEAKY, and output sizes that are not a multiple of the 16x16 pixel tile (edge tiles are masked)
   * select the general instantiations: 3x3 stride-1 NHWC, cout_pad 32 or 64, no statistics, fp32 or f16 operands. */
  int32_t ld_in0, ld_in1, ld_out;
  int32_t pad_mode;       /* enum cf_pad */
  int32_t pad_lo;         /* stride 2 only: 0 = pad right/bottom only (vqgan_arch.py:123), 1 = one row/column on every side
                             (parsenet.py ConvLayer scale='down': ReflectionPad2d(1) + stride-2 conv); needs cout_pad % 128 == 0 */
  int32_t winograd;       /* 1: Winograd F(2x2,3x3) evaluation of a 3x3 stride-1 convolution: `weight` comes from
                             cf_pack_conv_weight_winograd (U = G g G^T), 16 instead of 36 multiplies per 2x2 outputs, all in fp32 --
                             the same function in a different summation order.  Dense NHWC
                             tensors, zero padding, hout % 8 == 0, wout % 16 == 0, cout_pad % 64 == 0; prologues as the direct
                             kernel, epilogues none / residual / SFT, statistics supported.  Measured against fp64 its error
                             is below the direct kernel's, so the host uses it for every eligible 3x3 stride-1 convolution.
                             With bf16_mfma == CF_OPERAND_F16X2 (`weight` from cf_pack_conv_weight_winograd_f16x2, acc_scale set)
                             the 16 Winograd-domain GEMMs run on split operands: U and V as hi + lo IEEE halves, three f16
                             MFMAs per product, fp32 accumulation -- 4/9 of the split-half MFMA work of the direct form.
                             With CF_OPERAND_F16 / CF_OPERAND_BF16 (cout % 128 == 0, >= 32x32 pixels): single rounded operands,
                             one MFMA per product (weight: see cf_pack_conv_weight_winograd_bf16).
                             2 (ABI v18; v19: 16x16 patches and the weight layout below): Winograd F(4x4,3x3) with CF_OPERAND_F16X2 operands only (`weight` from
                             cf_pack_conv_weight_winograd43_f16x2, acc_scale set): 36 transform-domain GEMMs per 4x4 outputs = 2.25
                             products per output and input channel instead of 4, interpolation points (0, +-1/2, +-2, inf).  Dense
                             NHWC, zero padding, hout % 16 == 0, wout % 16 == 0, cout == cout_pad, cout % 64 == 0, cin % 16 == 0,
                             cin <= 256, an image of any of its tensors below 2^31 bytes; prologues / epilogues / statistics / act_scale as winograd 1, no split_k.  Its error
                             against fp64 is ~5x that of F(2x2,3x3) (the conditioning of the larger transform), far inside the
                             1e-3 pixel gate; the host uses it for generator / CFT convolutions (vqgan_arch.py:296-323,
                             codeformer_arch.py:136-157) and -- behind a measured logit-margin gate, round 5 -- for the encoder's covered layers.
                             ABI v20: also with CF_OPERAND_F32 (`weight` from cf_pack_conv_weight_winograd43; acc_scale / act_scale
                             unused, act_scale must be null): the same kernel with IEEE-fp32 operands on v_mfma_f32_16x16x4_f32.
                             With CF_OPERAND_F32 and `upsample` (one input, c0 % 32 == 0, c0 <= 256, cout % 128 == 0, no prologue / epilogue
                             operand).  upsample == 1 (`weight` from the plain cf_pack_conv_weight_winograd43): F(4x4,3x3) on the virtually upsampled
                             image, the gather reading source pixel (y >> 1, x >> 1).  upsample == 2 (`weight` from cf_pack_conv_weight_winograd42_up;
                             hin % 16 == 0, win % 16 == 0): nearest x2 + 3x3 as four F(4x4,2x2) sub-pixel phases, 25 transform-domain GEMMs per 4x4
                             outputs = 1.5625 products per output and input channel instead of 2.25 */
  float acc_scale;        /* CF_OPERAND_F16X2 only (direct or winograd): the accumulator is multiplied by this before the bias is added -- the exact
                             inverse of the power-of-two scale given to cf_pack_conv_weight_f16x2 (> 0) */
  /* Deterministic split-K for layers with few output tiles (one face: 16x16 .. 64x64 pixels), where latency is the serial K loop of
   * a workgroup: split_k workgroups share an output tile, each contracting a contiguous K range; partial accumulators meet in
   * `workspace`, the workgroup drawing the last ticket on counters[tile] adds them in split order (bitwise reproducible, independent of
   * arrival order) and runs the epilogue.  0 = off.  Supported: taps == 1 (64x64 tiles; also selects them with split_k == 1),
   * winograd, CF_OPERAND_F16X2.  workspace: cf_conv2d_workspace_bytes(d) bytes; counters: one zero-initialised uint32 per output
   * tile (cf_conv2d_tiles(d)), left at zero by every launch.
   * ABI v21: CF_SPLITK_IN_WORKGROUP (-1), taps == 1 with CF_OPERAND_F16X2 only (token GEMMs of one to a few faces): the K chunks of a
   * 32 x 32 output tile are shared by the four waves of ONE workgroup and added in chunk order through LDS -- the same bits as every
   * other split count, no workspace / counters (K <= 1024, M % 32 == 0; N % 64 == 0 as for every form: the weight packing).
   * winograd == 2 with CF_OPERAND_F32 (additive, the ABI version stays): split_k == cin / 128 (2 .. 4) selects the K-part form of F(4x4,3x3) --
   * one workgroup per (patch, 128 input channels, 128 output channels) writes raw partial sums to `workspace`
   * ([split_k][batch][hout][wout][cout] floats, no counters), a second launch adds them in part order from zero and applies acc_scale,
   * bias, epilogue and statistics.  cout % 128 == 0, cin % 128 == 0, cin <= 512, c0 % 128 == 0, no upsample; any other split_k is refused. */
  int32_t split_k;
  float* workspace;
  uint32_t* counters;
  /* Range scaling of an UN-NORMALISED input for the 16-bit-operand kernels (CF_OPERAND_F16X2 / F16 / BF16; prologue NONE or LEAKY only):
   * [batch][2] floats (s_b, 1 / s_b) written by cf_act_scale_from_stats / cf_act_scale_from_tensor, or NULL.  The gather multiplies
   * image b's activations by s_b after the prologue and the epilogue multiplies the accumulator by 1 / s_b on top of acc_scale -- both
   * powers of two, so the result is the one an unscaled evaluation would give, for inputs of ANY fp32 magnitude: without it an IEEE-half
   * operand overflows above 65504 (16376 in the Winograd domain, whose input transform sums four activations) and loses its lo half
   * below 2^-3.  Inputs that went through a GroupNorm prologue need none (their range is bounded by gamma, beta and the group size; the
   * host checks that bound when it packs the layer).  Ignored by the exact fp32 kernels. */
  const float* act_scale;
  /* ABI v22: bf16 STORAGE of the activations of this launch (BASELINE configs 3 / 5: "bf16 = bf16 storage + fp32 accumulate in generator +
   * CFT", vqgan_arch.py:276-323, codeformer_arch.py:136-157).  0: fp32 tensors (every launch of rounds 1-5).  1: in0, in1, res, sft_scale
   * and out hold bf16 elements (2 bytes, dense NHWC; the float* fields are then typed loosely) -- consumers widen on load (exact),
   * the epilogue rounds to nearest even once, AFTER the GroupNorm partials (stats_out) were taken from the fp32 values; prologue tables,
   * bias, weights, accumulation and statistics are unchanged.  An NCHW output (the network's last conv) stays fp32.  Supported by the
   * kernels the bf16 mode runs from 64x64 pixels up: winograd == 1 with CF_OPERAND_BF16 (cout % 128 == 0), the direct CF_OPERAND_BF16
   * 3x3 (cout_pad 64) and folded upsample (cout_pad % 128 == 0) forms, fp32 1x1 on images (no split_k), the <= 4-channel NCHW head. */
  int32_t io_bf16;
  /* ABI v22: a second token matrix for the output columns >= alt_cout0 (taps == 1 with CF_OPERAND_F16X2 on token matrices only; NULL: none).
   * The q|k projections of nn.MultiheadAttention read LayerNorm(x) + pos and the v projection LayerNorm(x) (codeformer_arch.py:124-126):
   * with in0 = LN(x) + pos, in0_alt = LN(x), alt_cout0 = 2 E and the whole in_proj weight (3 E rows) they are ONE launch instead of two.
   * in0_alt has in0's shape; alt_cout0 is a multiple of 128.  Per output element the arithmetic is that of the separate launches. */
  const float* in0_alt;
  int32_t alt_cout0;
} cf_conv_desc;

int cf_conv2d(const cf_conv_desc* d, cf_stream_t stream);
/* cf_conv2d with a uint8 HWC BGR image at either end of the network: the image is read by the first conv / written by the last one,
   bitwise what cf_img_u8_to_tensor + cf_conv2d / cf_conv2d + cf_tensor_to_img_u8 give (output tensor, statistics partials, bytes).
   img_in  != NULL: replaces d->in0; needs in_nchw = 1, c0 = 3, taps 9, stride 1, fp32 operands, cout = cout_pad = 64,
                    hout, wout multiples of 16, no prologue / epilogue (the shapes conv3x3_few_cin takes today).
   img_out != NULL: replaces d->out; needs out_nchw = 1, cout = 3 (cout_pad 32), taps 9, stride 1, fp32 operands, no epilogue,
                    a dense input (io_bf16 0 or 1).
   Exactly one of the two is non-NULL.  Anything else: CF_ERR_ARG, nothing launched. */
int cf_conv2d_u8(const cf_conv_desc* d, const uint8_t* img_in, uint8_t* img_out, cf_stream_t stream);
/* cf_conv2d with d->epilogue == CF_EPI_SFT and one weight per image (entry point added, ABI version unchanged): w_img holds [batch]
   floats on the device and image b computes res + w_img[b] * (res * sft_scale + (acc + bias)); d->sft_w is ignored.  Every kernel family
   that has the SFT epilogue takes it (direct fp32 / bf16 / f16, split halves, F(2x2,3x3), F(4x4,3x3), their split-K and bf16-storage
   forms); the weight is one wave-uniform read per output patch, and the kernels form it by the same expression as the scalar launch, so
   image b's output and statistics partials are bitwise those of cf_conv2d on that image alone with sft_w = w_img[b] -- for any value,
   non-positive and non-finite ones included (whether a non-positive weight means "no fusion" is the caller's rule, not the kernel's).
   A NULL w_img or any other epilogue: CF_ERR_ARG with a message, nothing launched (checked before any device call). */
int cf_conv2d_sft_w(const cf_conv_desc* d, const float* w_img, cf_stream_t stream);
/* number of statistics partials per (image, group) the launch described by d will write (>0), or <0 on error */
int cf_conv2d_stats_parts(const cf_conv_desc* d);
/* split-K launches: bytes of workspace / number of output tiles (= counters) the launch described by d needs (0 when split_k <= 1) */
int64_t cf_conv2d_workspace_bytes(const cf_conv_desc* d);
int cf_conv2d_tiles(const cf_conv_desc* d);

/* ---- weight packers (every cf_pack_* below is defined in csrc/cf_pack.hip, whatever kernel file reads its layout) --------
 * Pack a PyTorch conv/linear weight [cout][cin][kh*kw] (taps = 1 or 9) into the kernel layout
 * [tap][cin_pad/16][cout_pad][16] (zero padded). */
int cf_pack_conv_weight(const float* w, int cout, int cin, int taps, int cout_pad, int cin_pad,
                        float* packed, cf_stream_t stream);
int64_t cf_packed_weight_elems(int cin_pad, int taps, int cout_pad);
/* Winograd-domain weights for cf_conv_desc.winograd: [16 positions][cin_pad/16][cout_pad][16] fp32 (16*cin_pad*cout_pad values),
 * U[xi*4+nu] = (G g G^T)[xi][nu] evaluated in fp64 and rounded once; cout_pad % 64 == 0 */
int cf_pack_conv_weight_winograd(const float* w, int cout, int cin, int cout_pad, int cin_pad, float* packed, cf_stream_t stream);
/* The same for winograd + CF_OPERAND_F16X2: scale * U as hi + lo IEEE halves in MFMA-operand order (16*cin_pad*cout_pad 32-bit
 * words); `scale` is a power of two that puts max|scale * U| into [2^14, 2^15) (cf_conv_desc.acc_scale = 1 / scale) */
int cf_pack_conv_weight_winograd_f16x2(const float* w, int cout, int cin, int cout_pad, int cin_pad, float scale, void* packed,
                                       cf_stream_t stream);
/* winograd == 2 (F(4x4,3x3)) + CF_OPERAND_F16X2: scale * U', U' = G' g G'^T with the rows of G scaled by (4, 4, 4, 2, 2, 4) (the input
 * transform carries the inverse powers of two), as hi + lo IEEE halves in MFMA-operand order [36 positions][cin_pad/16][cout_pad/16]
 * [64 lanes][hi 2 words | lo 2 words] (ABI v19: the 16x16x16 MFMA's B operand) = 36*cin_pad*cout_pad 32-bit words; cout_pad % 64 == 0; `scale` a power of two that puts
 * max|scale * U'| into [2^14, 2^15) (cf_conv_desc.acc_scale = 1 / scale) */
int cf_pack_conv_weight_winograd43_f16x2(const float* w, int cout, int cin, int cout_pad, int cin_pad, float scale, void* packed,
                                         cf_stream_t stream);
/* winograd == 2 + CF_OPERAND_F32 (ABI v20): U' in fp32, same tensor order with a lane's 16 (32) bytes = the four (eight) k groups
 * c = slab * KS + 4 j + (lane >> 4) of output channel block * 16 + (lane & 15) (the 16x16x4 fp32 MFMA's B operand); KS = 32 when
 * cout_pad % 128 == 0 and cin_pad % 32 == 0 (the form cf_conv2d runs for that shape), else 16.  36*cin_pad*cout_pad floats. */
int cf_pack_conv_weight_winograd43(const float* w, int cout, int cin, int cout_pad, int cin_pad, void* packed, cf_stream_t stream);
/* winograd == 2 + CF_OPERAND_F32 + upsample (entry point added, ABI version unchanged): nearest x2 + 3x3 as four Winograd F(4x4,2x2) sub-pixel
 * phases.  Phase p = 2 a + b (output parity (a, b)) folds the 3x3 taps to 2x2 -- along an axis [g0, g1 + g2] for parity 0, [g0 + g1, g2] for
 * parity 1 -- and U_p = G42 g_p G42^T, points (0, -1, 1/2, 2, inf), is evaluated in fp64 and rounded once: [4 phases][25 positions xi * 5 + nu]
 * [cin_pad/32][cout_pad/16][64 lanes][8 k groups] fp32 in the fragment order of the 32-channel-slab form above = 100*cin_pad*cout_pad floats;
 * cout_pad == cout, cout % 128 == 0, cin_pad == cin, cin % 32 == 0. */
int cf_pack_conv_weight_winograd42_up(const float* w, int cout, int cin, int cout_pad, int cin_pad, void* packed, cf_stream_t stream);
/* winograd + SINGLE 16-bit operands (cout % 128 == 0, at least 32x32 pixels per image: the eight-wave kernel of cf_wsplit.hip; the
 * network's 'fp16' / 'bf16' modes, BASELINE configs 3 and 5): one MFMA per transform-domain product.  CF_OPERAND_F16 reads the hi slot of
 * the split packing above as it is; CF_OPERAND_BF16 takes this buffer: bf16(scale * U) in the hi slot of the same layout, zeros in the
 * lo slot (same size; scale a power of two, acc_scale = 1 / scale) */
int cf_pack_conv_weight_winograd_bf16(const float* w, int cout, int cin, int cout_pad, int cin_pad, float scale, void* packed,
                                      cf_stream_t stream);
/* taps == 1 + CF_OPERAND_F16X2 (Linear / 1x1 on token matrices, codeformer_arch.py:104-106,126,132,183,192): w[n][k] -> scale * w as
 * hi + lo IEEE halves in MFMA-operand order (n*k 32-bit words); n % 64 == 0, k % 128 == 0.  The launch needs M = batch*hout*wout % 64 == 0
 * (split_k == CF_SPLITK_IN_WORKGROUP: M % 32 == 0 and k <= 1024), a dense single input and a dense output (ld_out 0 or cout), no prologue /
 * statistics, epilogue none | GELU | residual; split_k any divisor of k / 128 (same bits for every count, as for the fp32 GEMM).
 * Operand range the split-half token GEMM is accurate on (derived in tools/gemm_check.py, tested by tests/test_gpu_token_gemm.py):
 *   weights: ONE power-of-two scale per matrix puts max|scale * w| into [2^14, 2^15).  A weight carries 22 bits while |scale * w| >= 2^-3,
 *     i.e. down to 2^-17 .. 2^-18 of the largest weight of the matrix; below that its lo half is a subnormal half and the weight carries an
 *     ABSOLUTE error of up to 2^-25 / scale (below 2^-14 / scale the hi half is subnormal too; below 2^-25 / scale the weight is zero).
 *   tokens: split in registers with NO scale.  22 bits for 2^-3 <= |a| <= 65504; below 2^-3 an absolute error of up to 2^-25 per element;
 *     beyond 65504 the hi half is infinite and the outputs of that row are non-finite, never wrong finite values.
 *   per output element: |error| <= (396 + k / 128) 2^-24 sum|a w| + 2^-25 (sum|a| / scale + sum|w|) before bias and epilogue.  The host keeps
 *   a layer whose inputs may leave the token range on fp32 operands (bounded_code, codeformer_arch.py). */
int cf_pack_linear_weight_f16x2(const float* w, int n, int k, float scale, void* packed, cf_stream_t stream);
/* bf16 layout [tap][cin_pad/32][cout_pad][32] (round-to-nearest-even); cin_pad % 32 == 0, cout_pad % 64 == 0; the buffer
 * holds cf_packed_weight_elems(cin_pad, taps, cout_pad) bf16 values (half the bytes of the fp32 packing). */
int cf_pack_conv_weight_bf16(const float* w, int cout, int cin, int taps, int cout_pad, int cin_pad, void* packed,
                             cf_stream_t stream);
/* Folded weights for cf_conv_desc.upsample: [class 4][tap 4][cin_pad/16][cout_pad][16] fp32 (16*cin_pad*cout_pad values), or the
 * bf16 analogue with 32-channel slabs.  class = (oy&1)*2 + (ox&1); each entry is the fp32 sum of the 3x3 taps that read the same
 * source pixel for that output parity. */
int cf_pack_conv_weight_up2x(const float* w, int cout, int cin, int cout_pad, int cin_pad, float* packed, cf_stream_t stream);
int cf_pack_conv_weight_up2x_bf16(const float* w, int cout, int cin, int cout_pad, int cin_pad, void* packed,
                                  cf_stream_t stream);
/* IEEE-half analogues of the two bf16 packers (same layouts; cout_pad % 32 == 0), for CF_OPERAND_F16 */
int cf_pack_conv_weight_f16(const float* w, int cout, int cin, int taps, int cout_pad, int cin_pad, void* packed,
                            cf_stream_t stream);
int cf_pack_conv_weight_up2x_f16(const float* w, int cout, int cin, int cout_pad, int cin_pad, void* packed,
                                 cf_stream_t stream);
/* Split-half weights for CF_OPERAND_F16X2: [slab][cin_pad/32][cout_pad][hi 32 | lo 32] IEEE halves (4 bytes per weight, slab = 9
 * taps or, with up2x == 1, the 16 folded class x tap slabs of cf_pack_conv_weight_up2x; up2x == 2 (ABI v17) selects the STRIDE-2
 * form for cf_conv_desc.stride == 2: 4 taps x 4*cin channels, W'[ty][tx][(p, q, c)] = w[2ty + p][2tx + q][c] or 0 -- 16 * cin *
 * cout_pad words, cin % 16 == 0, cin_pad == cin); up2x == 3 (ABI v17): a 1x1 weight [cout][cin] for cf_conv_desc.taps == 1 on images of
 * more than 1024 pixels (the streaming 1x1 form of the same kernel: the ResBlock skip convolutions, vqgan_arch.py:150-164; two-pointer
 * concat, act_scale, epilogues none / residual / SFT, no statistics) -- token matrices of at most 1024 rows per image keep
 * cf_pack_linear_weight_f16x2 and the token GEMM.  Each (folded) fp32 weight is multiplied
 * by `scale` -- a power of two, exact; choose it so that max|w*scale| lies in [2^14, 2^15) -- then hi = half(w'), lo = half(w' - hi)
 * (round-to-nearest-even).  cin_pad % 32 == 0, cout_pad % 64 == 0; cf_conv_desc.acc_scale must be 1 / scale. */
int cf_pack_conv_weight_f16x2(const float* w, int cout, int cin, int up2x, int cout_pad, int cin_pad, float scale, void* packed,
                              cf_stream_t stream);

/* ---- GroupNorm statistics (vqgan_arch.py:14-15: 32 groups, eps 1e-6, biased variance) --------
 * Partials are fp64 (sum, sumsq) tables [batch][groups][parts][2] over an NHWC tensor with c channels whose (fine)
 * groups are cpg channels wide.  They come from a conv epilogue (cf_conv_desc.stats_out) or from
 * cf_groupnorm_stats (stand-alone pass, `parts` blocks per image).
 * finalize: fixed-order sum of the partials; `gmerge` adjacent fine groups form one GroupNorm group (the CFT block
 *           normalises cat[enc, dec]: its groups are pairs of each tensor's own 32 groups); writes, for the c
 *           channels of THIS tensor, scale[b*ld + i] = gamma[i]*rstd, shift[b*ld + i] = beta[i] - mean*scale
 *           (callers pre-offset gamma/beta/scale/shift to the tensor's first channel inside a concatenation;
 *           ld = row stride of the tables = total channels).  count = elements per merged group.
 */
int cf_groupnorm_stats(const float* x, int batch, int hw, int c, int cpg, double* partial, int parts,
                       cf_stream_t stream);
/* ---- per-image power-of-two range scale for cf_conv_desc.act_scale ------------------------------------------------------------
 * act[b] = (s_b, 1 / s_b) with s_b = 2^k such that growth * A_b * s_b lies in [2^13, 2^14), A_b >= max |x| over image b
 * (s_b = 1 for an all-zero or non-finite image; k clamped to [-100, 100]).  growth = 4 covers the Winograd input transform.
 * from_stats:  A_b = sqrt(max over the image's `nper` = groups * parts statistics partials of sumsq) -- a rigorous bound on max |x|
 *              (each partial covers at most a few hundred elements, so it is loose by at most ~5 bits: harmless, the split operands
 *              keep 22 bits over 18 binades) that costs no pass over the tensor: the partials are the ones cf_conv_desc.stats_out
 *              of the PRODUCING launch wrote, layout [batch][nper][2] doubles.
 * from_tensor: A_b = max |x| exactly, one pass over x [batch][n_per_image] (small tensors: the 16x16 quantised feature).
 * scratch: batch * 32 floats (32 partial maxima per image: the reduction runs on 32 workgroups per image, then one wave per image). */
int cf_act_scale_from_stats(const double* partial, int batch, int nper, float growth, float* scratch, float* act, cf_stream_t stream);
int cf_act_scale_from_tensor(const float* x, int batch, int64_t n_per_image, float growth, float* scratch, float* act, cf_stream_t stream);
/* The same table in ONE launch (ABI v17), for the statistics partials of one or two tensors -- the halves of a concatenated input share
 * one scale: A_b = the larger bound -- or (partial_a == NULL) for a tensor x.  cells: 2 * batch zero-initialised uint32 that every launch
 * leaves at zero again (an atomic maximum and a ticket per image: the workgroup drawing the last of the 32 tickets writes act[b]). */
int cf_act_scale_fused(const double* partial_a, int nper_a, const double* partial_b, int nper_b, const float* x, int64_t n_per_image, int batch,
                       float growth, uint32_t* cells, float* act, cf_stream_t stream);
int cf_groupnorm_finalize(const double* partial, int batch, int parts, int c, int cpg, int gmerge, int64_t count,
                          const float* gamma, const float* beta, float eps, float* scale, float* shift, int ld,
                          cf_stream_t stream);
/* ABI v22: the same for up to TWO tensors in one launch -- the halves [enc, dec] of a concatenated GroupNorm input (codeformer_arch.py:152;
 * partial_b NULL: one tensor) -- whose tables land side by side (tensor b's channels start at c_a; gamma / beta / scale / shift address the
 * concatenated channel axis, ld >= c_a + c_b), bitwise the tables of two cf_groupnorm_finalize launches.  With `act` set ([batch][2], and
 * `cells` as for cf_act_scale_fused) the launch also writes the range-scale table of the same tensor(s) -- bitwise cf_act_scale_fused's on the
 * same partials: the ResBlock input that feeds both norm1 and the 1x1 skip convolution (vqgan_arch.py:153-164) needs one launch, not three. */
int cf_groupnorm_finalize2(const double* partial_a, int parts_a, int c_a, int cpg_a, int gmerge_a, const double* partial_b, int parts_b, int c_b,
                           int cpg_b, int gmerge_b, int batch, int64_t count, const float* gamma, const float* beta, float eps, float* scale,
                           float* shift, int ld, float act_growth, uint32_t* cells, float* act, cf_stream_t stream);

/* ---- LayerNorm over the last dim (codeformer_arch.py:108-109,124,131,191; eps 1e-5) ----------
 * y = LN(x)*gamma+beta ; optional ypos = y + pos[row % npos]   (with_pos_embed, codeformer_arch.py:113-116) */
int cf_layernorm(const float* x, int rows, int c, const float* gamma, const float* beta, float eps,
                 const float* pos, int npos, float* y, float* ypos, cf_stream_t stream);

/* ---- attention over 256 keys (vqgan_arch.py:207-221 AttnBlock bmm/softmax/bmm, and the
 *      nn.MultiheadAttention core called at codeformer_arch.py:126) --------------------------------
 * q,k,v: row (b*256 + i), columns [h*head_dim, (h+1)*head_dim) of matrices with leading dimensions
 * ldq/ldk/ldv; out likewise with ldo.  softmax over keys of (q.k^T * scale).  head_dim in {64, 512}.
 * q, k, v and out must be 16-byte aligned and ldq/ldk/ldv multiples of 4 (the kernels read float4); ldo >= heads*head_dim
 * (columns past heads*head_dim of an out row are not written).  Anything else is CF_ERR_ARG before any launch. */
int cf_attention(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, float* out, int ldo,
                 int batch, int heads, int head_dim, int nkeys, float scale, cf_stream_t stream);

/* ---- code prediction (codeformer_arch.py:257-258 softmax+topk(1)) ------------------------------
 * argmax over each fp32 row, lowest index wins ties; idx is int64 like the reference's top_idx.  n % 4 == 0, any n >= 4 and any row count.
 * NaN: the comparisons skip a NaN element, so idx is the lowest index of the largest NON-NaN element (numpy.argmax would name the NaN).  A row
 * without a single comparable element -- every element NaN -- has no such index and gets 0x7fffffff, which is out of range for every caller:
 * cf_codebook_gather_adain clamps it to the last code, cf_label_lut_f32 maps it to entry 0.  Nothing reads memory through it; a row of -inf
 * only ties at index 0.  (tests/test_gpu_misc_kernels.py pins all of this for both entry points.) */
int cf_argmax_rows(const float* logits, int rows, int n, int64_t* idx, cf_stream_t stream);
/* The same argmax plus the top-2 logit gap (the logit guard of CodeFormer.forward; entry point added, ABI version unchanged):
 * idx[row]  bitwise cf_argmax_rows';
 * gap[row]  = best - second in one fp32 subtraction, `second` the largest value of the row at any index other than idx[row] (a second element
 *             equal to the maximum gives exactly 0.0f) == torch.topk(row, 2).values[0] - values[1];
 * group_min_gap[g] = min of gap over rows [g*rows_per_group, (g+1)*rows_per_group) (a face: 256 tokens); rows % rows_per_group == 0.
 * NaN: a row that holds a NaN element, or whose two largest values are the same infinity, gets gap = NaN, and a NaN gap makes its group's
 * minimum NaN -- so `!(group_min_gap >= threshold)` flags the group for every threshold.
 * Two launches on `stream` (the row scan, then one wave per group), no host synchronisation, nothing to initialise, capturable. */
int cf_argmax_rows_gap(const float* logits, int rows, int n, int rows_per_group, int64_t* idx, float* gap, float* group_min_gap,
                       cf_stream_t stream);

/* ---- codebook lookup (+ AdaIN) (vqgan_arch.py:72-84, codeformer_arch.py:12-43,266) -------------
 * out[b][p][:] = codebook[idx[b][p]][:]; when adain != 0 the per-(b,c) statistics over the ntok positions
 * (unbiased variance + eps) of `out` are replaced by those of lq (NHWC [batch][ntok][dim]). */
int cf_codebook_gather_adain(const int64_t* idx, const float* codebook, int codebook_size, const float* lq,
                             int batch, int ntok, int dim, int adain, float eps, float* out, cf_stream_t stream);

/* ---- nearest-code L2 quantisation (vqgan_arch.py:33-49 VectorQuantizer.forward) ----------------
 * The z.E^T product runs on cf_conv2d (taps=1, the packed codebook as weight); these two finish it:
 * cf_row_sqnorm: out[r] = sum_k x[r][k]^2                      ((z**2).sum(1) and (E**2).sum(1), :40)
 * cf_vq_argmin:  idx[r] = argmin_j (zz[r] + ee[j]) - 2*scores[r][j]   (:40-45; lowest index on ties) */
int cf_row_sqnorm(const float* x, int rows, int dim, float* out, cf_stream_t stream);
int cf_vq_argmin(const float* scores, const float* zz, const float* ee, int rows, int ncodes, int64_t* idx,
                 float* dist_min, cf_stream_t stream);

/* ---- layout converters at the NCHW module boundary ---------------------------------------------- */
int cf_nchw_to_nhwc(const float* x, int batch, int c, int hw, float* y, cf_stream_t stream);
int cf_nhwc_to_nchw(const float* x, int batch, int c, int hw, float* y, cf_stream_t stream);

/* pixel-unshuffle into channels-last (basicsr/archs/arch_util.py:190-206 + the NCHW->NHWC change): x [batch][c][h*s][w*s]
 * -> out [batch][h][w][c_pad], channel (ci*s + dy)*s + dx = x[ci][y*s+dy][x*s+dx], channels >= c*s*s zero (c_pad % 16 == 0).
 * s = 1 is a plain NCHW -> zero-padded NHWC conversion. */
int cf_pixel_unshuffle_nhwc(const float* x, int batch, int c, int h, int w, int s, int c_pad, float* out, cf_stream_t stream);
/* its inverse with channels-last on both sides (nn.PixelShuffle(s) behind a conv whose output stays NHWC; arch_util.py:95-114 Upsample):
 * x [batch][h][w][c*s*s] -> out [batch][h*s][w*s][c], out[b][y*s+i][x*s+j][k] = x[b][y][x][(k*s + i)*s + j].  Pure data movement. */
int cf_pixel_shuffle_nhwc(const float* x, int batch, int c, int h, int w, int s, float* out, cf_stream_t stream);

/* ---- tensor boundary (basicsr/utils/img_util.py:9-35 img2tensor + normalize, :38-94 tensor2img) ---
 * u8 HWC BGR [batch][h][w][3] -> fp32 NCHW RGB in [-1,1] ((x/255 - 0.5)/0.5), and back
 * (clamp[-1,1], (x+1)/2*255, round-half-even, RGB->BGR).  +-inf clamp to bytes 255 / 0.  A NaN gives byte 0 (fmaxf(NaN, -1) is -1): the
 * reference's tensor2img has no defined answer there (a NaN -> uint8 cast), this one is pinned by tests/test_gpu_misc_kernels.py.
 * Images with h * w % 4 == 0 are converted four pixels per thread through aligned 4-byte words, every other size pixel by pixel. */
int cf_img_u8_to_tensor(const uint8_t* img, int batch, int h, int w, float* out, cf_stream_t stream);
int cf_tensor_to_img_u8(const float* t, int batch, int h, int w, uint8_t* img, cf_stream_t stream);
/* inpainting composite (inference_inpainting.py:68-74): x, y, out are [batch][3][h][w]; mask = (x0+x1+x2 == 3);
 * out = (1-mask)*x + mask*y */
int cf_mask_composite(const float* x, const float* y, int batch, int h, int w, float* out, cf_stream_t stream);
/* ABI v22: fp32 -> bf16 copy (round to nearest even) of `numel` elements (a multiple of 8): the fp32 activations that enter the
 * bf16-storage part of the generator (cf_conv_desc.io_bf16) -- the decoder feature in front of the first bf16 Upsample
 * (vqgan_arch.py:129-138) and the encoder taps the fusion blocks concatenate (codeformer_arch.py:152, :228-230). */
int cf_f32_to_bf16(const float* x, int64_t numel, void* out, cf_stream_t stream);

/* ---- bundled StyleGAN2 ops of basicsr/ops (unused by the hot path) ---------------
 * cf_fused_bias_act: basicsr/ops/fused_act/src/fused_bias_act_kernel.cu:20-50 forward (act=3, grad=0):
 *    y = leaky_relu(x + bias[(i / hw) % c], slope) * scale                     (x is NCHW)
 * cf_fused_bias_act_ex: every mode of the op (:36-46, the switch on act*10 + grad): act 1 linear | 3 leaky ReLU(alpha); grad 0 forward,
 *    1 first derivative (y = ref > 0 ? x : x*alpha, ref = the forward OUTPUT, fused_act.py:33,47), 2 second derivative (0); bias
 *    and ref may be NULL; dtype 0 float | 1 IEEE half | 2 bf16 for x / bias / ref / y alike (AT_DISPATCH_FLOATING_TYPES_AND_HALF, :80)
 * cf_upfirdn2d: basicsr/ops/upfirdn2d/src/upfirdn2d_kernel.cu:50-208: planes [nplanes][in_h][in_w].  The reference's six tiled
 *    configurations (:251-291: (up, down) in {(1,1), (2,1), (1,2)}, taps <= 4 / <= 3 or 2) run an LDS-tiled kernel, everything else
 *    the general polyphase kernel (:50-106). */
int cf_fused_bias_act(const float* x, const float* bias, int64_t numel, int c, int hw, float slope, float scale,
                      float* y, cf_stream_t stream);
int cf_fused_bias_act_ex(const void* x, const void* bias, const void* ref, int64_t numel, int c, int hw, int act, int grad, float alpha,
                         float scale, int dtype, void* y, cf_stream_t stream);
int cf_upfirdn2d(const float* x, int nplanes, int in_h, int in_w, const float* kernel, int kh, int kw, int up_x,
                 int up_y, int down_x, int down_y, int pad_x0, int pad_x1, int pad_y0, int pad_y1, float* y,
                 cf_stream_t stream);

/* ---- deformable convolution, forward (basicsr/ops/dcn; no registered arch uses it) ------------------------------------------
 * One definition for the modulated (v2) and the plain (v1: mask == NULL, bias == NULL) op, K = kh*kw, tap k = i*kw + j, d = c / (cin /
 * deform_groups) the deformable group of input channel c:
 *   out[b][o][y][x] = bias[o] + sum_{c in the group of o, k} weight[o][c_local][i][j] * mask[b][d*K + k][y][x] * val
 *   val = bilinear sample of x[b][c], zeros outside the image, at
 *     h = (float)(y*stride_h - pad_h + i*dil_h) + offset[b][(d*K + k)*2][y][x],  w likewise with offset channel (d*K + k)*2 + 1;
 *   val = 0 unless h > -1 && w > -1 && h < hin && w < win on those fp32 values (so a NaN offset samples nothing).
 * hout = (hin + 2 pad_h - (dil_h (kh-1) + 1)) / stride_h + 1, wout likewise.  offset [batch][deform_groups*2*K][hout][wout], mask
 * [batch][deform_groups*K][hout][wout], out [batch][cout][hout][wout], all fp32.
 * route 1: the bilinear gather fused into an implicit GEMM on v_mfma_f32_32x32x2_f32 (exact fp32 operands).  x is channels-last
 *   [batch][hin][win][cin] (x_nhwc = 1), weight is packed by cf_pack_deform_conv_weight ([group][tap][cin_g/16][cout_pad_g][16] floats,
 *   cf_deform_conv2d_packed_elems of them); needs (cin/deform_groups) % 4 == 0, (cin/groups) % 16 == 0 and kh*kw <= 49 (and cin < 65536,
 *   one image below 2^31 bytes).  The image is read through a buffer descriptor of its own size: a corner that fails its bounds check
 *   gets an offset beyond it, for which the hardware makes no memory access.
 * route 0: one thread per output element, any shape.  weight is the plain [cout][cin/groups][kh][kw] tensor; x is channels-last
 *   (x_nhwc = 1) or [batch][cin][hin][win] (x_nhwc = 0).
 * Every argument is checked before anything is launched. */
int64_t cf_deform_conv2d_packed_elems(int cout, int cin, int taps, int groups); /* -1: groups does not divide the channels */
int cf_pack_deform_conv_weight(const float* w, int cout, int cin, int taps, int groups, float* packed, cf_stream_t stream);
int cf_deform_conv2d(const float* x, const float* offset, const float* mask, const float* weight, const float* bias, float* out,
                     int batch, int cin, int hin, int win, int cout, int kh, int kw, int stride_h, int stride_w, int pad_h,
                     int pad_w, int dil_h, int dil_w, int groups, int deform_groups, int x_nhwc, int route, cf_stream_t stream);

/* ---- optical-flow warp (basicsr/archs/arch_util.py:117-148 flow_warp; the alignment op next to DCNv2Pack) ---------------------
 * The reference adds the flow to a mesh grid, normalises by (n - 1) and calls torch's grid_sample, which un-normalises again; here the
 * round trip is cancelled algebraically.  x fp32 [batch][c][h][w] (x_nhwc = 0) or channels-last [batch][h][w][c] (x_nhwc = 1: c % 4 == 0,
 * x and out 16-byte aligned), flow fp32 [batch][h][w][2] = (dx, dy), out in the layout of x.  For output pixel (y, x), every step one
 * fp32 operation, none contracted:
 *   position    px = (float)x + dx,  py = (float)y + dy
 *   coordinate  align_corners = 1:  ix = px * ((w-1) / max(w-1, 1))          (px itself; px * 0 when w == 1)
 *               align_corners = 0:  ix = px * (w / max(w-1, 1)) - 0.5        (the reference normalises by w - 1 in both cases, and that
 *               quirk is part of the function); the ratio is one fp32 division per launch.  iy likewise with h.
 *   padding     0 zeros: nothing.   1 border: ix < 0 ? 0 : ix > w-1 ? w-1 : ix.
 *               2 reflection about [lo, lo + span], (lo, span) = (0, w-1) with align_corners, (-0.5, w) without:  a = |ix - lo|,
 *               r = fmod(a, span + span) (exact), ix = (r <= span ? r : (span + span) - r) + lo, then the border clamp (span == 0: the
 *               clamp alone).  It is torch's reflection with the parity of the fold count taken from the exact remainder.
 *   bilinear    in range when ix > -1 && iy > -1 && ix < w && iy < h; x0 = floor(ix), lw = ix - x0, hw = 1 - lw (lh, hh likewise); the
 *               corners top-left, top-right, bottom-left, bottom-right weigh hh*hw, hh*lw, lh*hw, lh*lw; a corner outside the image
 *               contributes +0 and is never read;  out = ((t0 + t1) + t2) + t3, t_i = weight_i * value_i, in that order.
 *   nearest     (rint(ix), rint(iy)), half to even; the pixel there, 0 when it lies outside the image.
 * Non-finite positions: every in-range test runs on the fp32 coordinate before any float -> int conversion, and no address is formed
 * from an unchecked value.  A NaN position samples nothing and gives 0 in EVERY padding mode -- a deliberate choice: torch's result
 * there is undefined.  +-inf follows the padding rule as written: 0 under zeros, the edge pixel under border, 0 under reflection (the
 * remainder of an infinite value is NaN); on an axis of one pixel with align_corners the coordinate is inf * 0 = NaN, hence 0.
 * h, w < 2^24 and h * w < 2^31.  Every argument is checked before anything is launched. */
int cf_flow_warp(const float* x, const float* flow, float* out, int batch, int c, int h, int w, int interp, int padding, int align_corners,
                 int x_nhwc, cf_stream_t stream);

/* ---- quality metrics: PSNR and SSIM of image batches (basicsr/metrics/psnr_ssim.py:9-128, metric_util.py:6-45) ------------------
 * Added without a version bump: the three exports are additive and CF_ABI_VERSION stays 22.
 * a and b are two images of the same shape, uint8 (dtype 0) or float32 (dtype 1) with values in [0, 255], `batch` of them, h x w pixels,
 * channels 1 or 3.  Element (n, y, x, ch) of image a lies at a[n*stride_a[0] + y*stride_a[1] + x*stride_a[2] + ch*stride_a[3]] (element
 * strides in HOST memory, 4 each, non-negative): HWC, CHW, a border crop and a slice of a larger tensor are all the same call, with no copy.
 * Values: without y_channel the element itself, in fp64.  With y_channel a 3-channel image is BGR and becomes ONE plane
 *   f = float32(v) / float32(255) per channel;  d = ((f_b*24.966 + f_g*128.553) + f_r*65.481) + 16.0 in fp64, each operation rounded on its
 *   own and in this order;  Y = float32(float32(d / 255.0) * float32(255))
 * (bgr2ycbcr(y_only) of basicsr/utils/matlab_functions.py as to_y_channel calls it), and a 1-channel image float32(float32(v)/255 * 255).
 * Everything after that is fp64.  planes = 1 with y_channel, else channels.
 *   cf_psnr   sse[n] = sum (a - b)^2 over pixels and planes; psnr[n] (may be NULL) = inf when sse == 0, else 20 log10(255 / sqrt(sse / N)),
 *             N = h*w*planes.  For uint8 inputs without y_channel sse is exact.
 *   cf_ssim   window g[i] = exp(-(i-5)^2 / (2 * 1.5^2)) / sum, applied along the rows and then along the columns, valid region only
 *             ((h-10) x (w-10) outputs: h, w >= 11); C1 = (0.01*255)^2, C2 = (0.03*255)^2; with mu = g*a etc.
 *             map = ((2 mu1 mu2 + C1)(2 s12 + C2)) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2)), s1 = g*a^2 - mu1^2, s2 likewise, s12 = g*ab - mu1 mu2;
 *             ssim[n] = the mean over planes of the mean of the plane's map.  fp64 throughout.
 * Reductions are deterministic and batch-invariant: every workgroup writes one fp64 partial to a slot of `parts` that depends only on
 * (image, plane, tile), a second launch adds an image's partials in a fixed order, the tiling depends on (h, w) only and there are no
 * floating-point atomics.  parts: batch * cf_metric_parts(h, w, planes) doubles of scratch (what either call needs at most; h, w below 11
 * count the squared-error strips alone).  The largest element offset of an image must stay below 2^31.
 * Every argument is checked before anything is launched. */
int cf_metric_parts(int h, int w, int channels); /* -1: bad arguments */
int cf_psnr(const void* a, const void* b, int batch, int h, int w, int channels, const int64_t* stride_a, const int64_t* stride_b, int dtype,
            int y_channel, double* parts, double* sse, double* psnr, cf_stream_t stream);
int cf_ssim(const void* a, const void* b, int batch, int h, int w, int channels, const int64_t* stride_a, const int64_t* stride_b, int dtype,
            int y_channel, double* parts, double* ssim, cf_stream_t stream);

/* ---- ArcFace / identity metric (basicsr/archs/arcface_arch.py ResNetArcFace; the identity score of face restoration) -------------------
 * Added without a version bump: the exports are additive and CF_ABI_VERSION stays 22.  fp32, channels-last, every pointer 16-byte aligned
 * where a kernel reads float4 (checked).  Every reduction has one fixed order given by the per-image shape: bitwise repeatable, and image /
 * row b of a batch is bitwise the call on it alone.  Every argument is checked before anything is launched.
 *   cf_prelu_maxpool2      x [batch][2h][2w][c] -> out [batch][h][w][c], c % 4 == 0: out = max over the 2x2 window of prelu(x, alpha), PReLU
 *                          FIRST (for alpha < 0 it is not monotone and the two do not commute; arcface_arch.py:232-233); a NaN wins the max.
 *   cf_se_pool             x [batch][hw][c] -> out [batch][c] = mean over the pixels (SEBlock's AdaptiveAvgPool2d(1), :159,166): fp32 partial
 *                          sums per (image, 64 channels, 256 pixels) in `parts` (batch * cf_se_pool_parts(hw) * c floats), added in block order,
 *                          one division by (float)hw.
 *   cf_se_gate             pooled [batch][c] -> out [batch][c] = sigmoid(w2 prelu(w1 p + b1, alpha) + b2), w1 [r][c], w2 [c][r] (torch's Linear
 *                          layout; :160-162), sigmoid(s) = 1 / (1 + expf(-s)); one workgroup per image; c <= 4096, r <= 256.
 *   cf_se_scale_res_prelu  out = prelu(x * y[b][c] + res, alpha), x / res / out [batch][hw][c], y [batch][c]; multiply and add rounded
 *                          separately (:168, :97-98).  res == NULL: no add, out = prelu(x * y[b][c], alpha) (SEBlock alone with alpha = 1).
 *   cf_fc_rows             out [m][n] = x [m][k] W^T + bias for 1 <= m <= 16 rows (fc5 of ResNetArcFace: k = 32768, n = 512 -- a 64 MiB weight
 *                          read once, a GEMV family).  wp is W [n][k] laid out [k/4][n][4] (a lane owns an output column and reads 16
 *                          contiguous bytes per 4 k); k % 256 == 0, n % 4 == 0.  K is cut into chunks of 256 across workgroups; a chunk is
 *                          four quarters of 64, each an fmaf chain in ascending k from zero, added in order; the chunk sums meet in ws
 *                          (cf_fc_rows_workspace_elems floats) and a second launch adds them -- chunks c = j mod 8 in ascending order for
 *                          j = 0 .. 7, those eight in order -- then the bias.  One order for every m.
 *   cf_identity_input      image -> [batch][1][128][128] fp32, the input of the identity network.  img: uint8 (dtype 0; f = (float)v / 255.0f)
 *                          or float32 in [0, 1] (dtype 1), 3 channels, element (n, y, x, ch) at img[n*stride[0] + y*stride[1] + x*stride[2] +
 *                          ch*stride[3]] (element strides in HOST memory, non-negative; largest offset below 2^31); bgr = 1: channel 0 is blue.
 *                          Every step one fp32 operation, none contracted:  v = f * 2 - 1 per channel;  gray = (0.2989 R + 0.5870 G) + 0.1140 B;
 *                          along an axis of n pixels, output index o:  src = (o + 0.5) * (n / 128) - 0.5 (the ratio one fp32 division per
 *                          launch), src = max(src, 0), i0 = floor(src), i1 = min(i0 + 1, n - 1), l = src - i0, h = 1 - l;
 *                          out = hy * (hx * g00 + lx * g01) + ly * (hx * g10 + lx * g11)  -- bilinear with half-pixel centres, edge clamp, no
 *                          antialiasing; gray first, resize second.  Indices are clamped to the image before any address is formed.
 *   cf_cosine_rows         out[r] = x_r . y_r / max(|x_r| |y_r|, 1e-8) in fp64 from fp32 rows [rows][n]; one wave per row (lane partials in
 *                          stride order, then a butterfly); a zero row gives 0. */
int cf_prelu_maxpool2(const float* x, int batch, int h, int w, int c, float alpha, float* out, cf_stream_t stream);
int cf_se_pool_parts(int hw); /* -1: bad argument */
int cf_se_pool(const float* x, int batch, int hw, int c, float* parts, float* out, cf_stream_t stream);
int cf_se_gate(const float* pooled, const float* w1, const float* b1, float alpha, const float* w2, const float* b2, int batch, int c, int r,
               float* out, cf_stream_t stream);
int cf_se_scale_res_prelu(const float* x, const float* y, const float* res, int batch, int hw, int c, float alpha, float* out, cf_stream_t stream);
int64_t cf_fc_rows_workspace_elems(int m, int n, int k); /* -1: bad arguments */
int cf_fc_rows(const float* x, const float* wp, const float* bias, int m, int n, int k, float* ws, float* out, cf_stream_t stream);
int cf_identity_input(const void* img, int batch, int h, int w, const int64_t* stride, int dtype, int bgr, float* out, cf_stream_t stream);
int cf_cosine_rows(const float* x, const float* y, int rows, int n, double* out, cf_stream_t stream);

/* ---- VGG / perceptual (basicsr/archs/vgg_arch.py VGGFeatureExtractor; basicsr/losses/losses.py PerceptualLoss) --------------------------
 * Additive exports, CF_ABI_VERSION stays 22.  fp32, channels-last; every reduction has one fixed order given by the per-image shape:
 * bitwise repeatable, image b of a batch is bitwise the call on it alone, no float atomics.  Every argument is checked before a launch.
 *   cf_vgg_input      image -> out [batch][h][w][c_pad] fp32, channels 3 .. c_pad - 1 zero (c_pad % 4 == 0, 4 <= c_pad <= 64: the K slab of the
 *                     first conv).  img / stride / dtype / bgr as cf_identity_input (uint8: f = (float)v / 255.0f; bgr = 1: channel 0 is
 *                     blue; output channel order is R, G, B).  Every step one fp32 operation, none contracted, as vgg_arch.py:150-153:
 *                     range_norm: f = (f + 1) / 2;  use_norm: f = (f - mean[c]) / std[c], mean / std three floats each in HOST memory.
 *   cf_relu           out = x > 0 ? x : +0 on n floats (n % 4 == 0), out == x allowed (in place).  NaN stays NaN, -inf gives 0.
 *   cf_relu_maxpool2  x [batch][h][w][c] -> out [batch][h/2][w/2][c], c % 4 == 0, h, w >= 2: max over the 2x2 window at stride 2 of relu(x);
 *                     an odd last row / column is dropped (nn.MaxPool2d(2, 2)); a NaN wins the max.  full != NULL: also writes relu(x) at
 *                     full resolution [batch][h][w][c] (full == x allowed: every element is read and written by the same thread).
 *   cf_gram           F [batch][hw][c] -> G [batch][c][c], G[b][i][j] = (sum_p F[b][p][i] F[b][p][j]) / (float)(c * hw), c % 64 == 0, c <= 512,
 *                     hw >= 1, on v_mfma_f32_32x32x2_f32 (IEEE-fp32 operands).  p is cut into chunks of CF_GRAM_CHUNK = 1024 pixels (the last
 *                     one zero-filled); a chunk's 64 x 64 tile is accumulated in ascending p with short chains: 16 pixels from zero on the
 *                     MFMA, those sums in order in groups of 8, the group sums in order; only tiles with j0 >= i0 are computed.  Chunk
 *                     products lie in ws (cf_gram_workspace_elems floats); a second launch adds them in ascending chunk order (groups of 16
 *                     chunks from zero, the group sums in order), divides once and writes G[i][j] and G[j][i] from the same value
 *                     (i <= j): G is bitwise symmetric.
 *   cf_feat_dist      a, b [batch][n] fp32 -> out [batch][2] fp64 = (sum |a - b|, sum (a - b)^2): the difference is one fp32 subtraction,
 *                     widened to fp64 before it is used.  One partial pair per (image, chunk of CF_FEAT_CHUNK = 16384 elements) in parts
 *                     (batch * cf_feat_dist_parts(n) * 2 doubles): a chunk is groups of 4 consecutive elements, thread t of 256 adds the
 *                     groups t, t + 256, .. in ascending order (elements 4t .. 4t + 3, 4t + 1024 .., each group in ascending order), then
 *                     the xor tree of each wave and the four waves in order.  The partials of an image are then added in ONE FIXED order,
 *                     which is not the ascending one: one wave per image, lane l adds chunks l, l + 64, .. in ascending order, then the
 *                     xor tree over the 64 lanes.
 *   cf_lpips_head     one layer of the LPIPS distance by its published definition (Zhang et al. 2018): a, b [batch][hw][c] fp32 (c % 4 == 0,
 *                     c <= 512), lin [c] -> out [batch] fp64 = mean over the pixels of  sum_c lin[c] (a_c / (sqrt(sum_c a_c^2) + 1e-10) -
 *                     b_c / (sqrt(sum_c b_c^2) + 1e-10))^2.  Per pixel everything is fp32, one operation per step, none contracted; channel
 *                     sums: a lane's elements in ascending order, then the xor tree of one wave.  Pixel values are widened to fp64; one
 *                     partial per (image, 256 pixels) in parts (batch * cf_lpips_parts(hw) doubles): wave w of a workgroup adds the pixels
 *                     w, w + 4, .. in ascending order, the four waves in order; the partials of an image are added as cf_feat_dist adds
 *                     its own (lane-strided, then the xor tree: fixed, not ascending), then one division by (double)hw. */
#define CF_GRAM_CHUNK 1024
#define CF_FEAT_CHUNK 16384
int cf_vgg_input(const void* img, int batch, int h, int w, const int64_t* stride, int dtype, int bgr, int range_norm, int use_norm,
                 const float* mean, const float* std, int c_pad, float* out, cf_stream_t stream);
int cf_relu(const float* x, int64_t n, float* out, cf_stream_t stream);
int cf_relu_maxpool2(const float* x, int batch, int h, int w, int c, float* out, float* full, cf_stream_t stream);
int64_t cf_gram_workspace_elems(int batch, int hw, int c); /* -1: bad arguments */
int cf_gram(const float* f, int batch, int hw, int c, float* ws, float* g, cf_stream_t stream);
int cf_feat_dist_parts(int64_t n); /* -1: bad argument */
int cf_feat_dist(const float* a, const float* b, int batch, int64_t n, double* parts, double* out, cf_stream_t stream);
int cf_lpips_parts(int hw); /* -1: bad argument */
int cf_lpips_head(const float* a, const float* b, const float* lin, int batch, int hw, int c, double* parts, double* out, cf_stream_t stream);

/* ---- BiSeNet / face parsing (facelib/parsing/bisenet.py BiSeNet; facelib/parsing/resnet.py ResNet18) -------------------------------------
 * Additive exports, CF_ABI_VERSION stays 22.  fp32; every pointer a kernel reads as float4 is 16-byte aligned (checked).  No reduction crosses
 * a thread but the stem's matrix instruction, whose order is fixed: bitwise repeatable, image / row b of a batch is bitwise the call on it
 * alone, no float atomics.  Every argument is checked before a launch.
 *   cf_pack_stem7x7    w [64][3][7][7] -> wp [148][64] (9472 floats): wp[k][n] = w[n][c][ky][kx] at k = (c * 7 + ky) * 7 + kx -- ascending
 *                      (c, ky, kx) -- and row 147, the padding of K = 147 to a multiple of 4, is zero.
 *   cf_stem7x7s2       x [batch][3][h][w] contiguous -> out [batch][ho][wo][64], ho = (h - 1) / 2 + 1, wo likewise, any h, w >= 1:
 *                      out = relu(bias[n] + sum_k wp[k][n] * x[c][2 oy - 3 + ky][2 ox - 3 + kx]), taps outside the image are zero (resnet.py:52,
 *                      :61-62 with bn1 folded into wp / bias by the caller).  An implicit GEMM on v_mfma_f32_32x32x2_f32 with IEEE-fp32
 *                      operands: the 148 products of an output are added in ONE accumulation chain from zero in ascending k, two k per
 *                      instruction; then one addition of the bias; relu(v) = v > 0 ? v : +0, a NaN stays.  A padded k multiplies the zero
 *                      weight by a stored zero, never by an image value.
 *   cf_maxpool3s2      x [batch][h][w][c], c % 4 == 0 -> out [batch][(h - 1) / 2 + 1][(w - 1) / 2 + 1][c]: the max over rows 2 oy - 1 .. 2 oy + 1
 *                      and columns 2 ox - 1 .. 2 ox + 1 that lie inside the image (nn.MaxPool2d(3, 2, 1), resnet.py:54: padding is -inf, not
 *                      zero); a NaN wins.
 *   cf_pooled_fc       pooled [batch][c], w [n][c], bias [n] -> out [batch][n] = act(s + bias[j]), s = one fmaf chain from zero over
 *                      i = 0 .. c - 1 in ascending order of w[j][i] * pooled[b][i]; the bias is one more addition.  act: CF_FC_NONE,
 *                      CF_FC_RELU (v > 0 ? v : +0, a NaN stays) or CF_FC_SIGMOID (1 / (1 + expf(-v)), as cf_se_gate).  c <= 4096, c % 4 == 0,
 *                      n <= 512.  The 1x1 convolutions on a 1x1 map of bisenet.py:45-48 and :70-71, BatchNorm folded by the caller.
 *   cf_scale_add_row   out[b][p][ch] = x[b][p][ch] * g[b][ch] + r[b][ch]; x / out [batch][hw][c], g / r [batch][c], c % 4 == 0; multiply and
 *                      add rounded separately (bisenet.py:49 then :72-75: the nearest upsampling of a 1x1 map is a row broadcast).
 *   cf_resize_bilinear_ac   x [batch][h][w][ld], the first c of ld channels (c <= ld, ld % 4 == 0) -> out [batch][c][oh][ow]:
 *                      F.interpolate(mode='bilinear', align_corners=True) (bisenet.py:130-137).  Per axis, source size n_in, output size
 *                      n_out, output index o:  scale = n_out > 1 ? (float)(n_in - 1) / (float)(n_out - 1) : 0 (once per launch);
 *                      src = scale * (float)o;  i0 = (int)src, clamped to 0 .. n_in - 1 before any address is formed;  i1 = i0 + (i0 < n_in - 1);
 *                      l1 = src - (float)i0;  l0 = 1 - l1.  Value = l0y * (l0x * a + l1x * b) + l1y * (l0x * c + l1x * d) with a, b the row-i0y
 *                      neighbours and c, d the row-i1y ones; every step is one fp32 operation, none contracted.
 *   cf_resize_bilinear_ac_argmax   the same values, compared and never stored: labels [batch][oh][ow] int64 = the index of the largest of the c
 *                      values, the lowest index among equal maxima, a NaN counting as the largest.  Channels >= c are never read. */
#define CF_FC_NONE 0
#define CF_FC_RELU 1
#define CF_FC_SIGMOID 2
int cf_pack_stem7x7(const float* w, float* wp, cf_stream_t stream);
int cf_stem7x7s2(const float* x, const float* wp, const float* bias, int batch, int h, int w, float* out, cf_stream_t stream);
int cf_maxpool3s2(const float* x, int batch, int h, int w, int c, float* out, cf_stream_t stream);
int cf_pooled_fc(const float* pooled, const float* w, const float* bias, int batch, int c, int n, int act, float* out, cf_stream_t stream);
int cf_scale_add_row(const float* x, const float* g, const float* r, int batch, int hw, int c, float* out, cf_stream_t stream);
int cf_resize_bilinear_ac(const float* x, int batch, int h, int w, int ld, int c, float* out, int oh, int ow, cf_stream_t stream);
int cf_resize_bilinear_ac_argmax(const float* x, int batch, int h, int w, int ld, int c, int64_t* labels, int oh, int ow, cf_stream_t stream);

/* ---- RetinaFace ResNet-50 detector (facelib/detection/retinaface/retinaface.py, retinaface_net.py, retinaface_utils.py) ------------------
 * Additive exports, CF_ABI_VERSION stays 22.  fp32, channels-last.  No split-K, no float atomics, one fixed summation order per output:
 * bitwise repeatable, and image b of a batch is bitwise the call on it alone.  Every argument is checked before a launch.
 *   cf_pointwise_packed_elems   floats of a packed pointwise weight: ceil64(cout) * ceil32(cin); -1: bad arguments.
 *   cf_pack_pointwise  w [cout][cin] -> wp [ceil64(cout)][ceil32(cin)], wp[n][k] = w[n][k], zero where n >= cout or k >= cin.
 *   cf_pointwise       a 1x1 convolution over pixels as one GEMM on v_mfma_f32_32x32x2_f32 with IEEE-fp32 operands:
 *                        out[b][oy][ox][n] = act(bias[n] + sum_k wp[n][k] * x[b][step * oy][step * ox][k] [+ res[b][oy][ox][n]])
 *                      x [batch][h][w] pixels of ld_x floats (the first cin are read; a channel slice of a wider buffer is ld_x > cin),
 *                      out / res [batch][ho][wo] pixels of ld_out / ld_res floats, ho = (h + step - 1) / step, wo likewise; step 1 or 2 (the
 *                      1x1 stride-2 `downsample` of a bottleneck: every second pixel of every second row).  M = batch * ho * wo is any value:
 *                      a workgroup owns 128 rows x 64 columns, edge rows and columns are masked on the store and read from a clamped address.
 *                      K order: slabs of 32 channels in ascending order; within a slab the instruction j (0 .. 15) of a wave multiplies
 *                      channels (8 (j / 4) + j % 4, 8 (j / 4) + 4 + j % 4); all of an output's products go down ONE accumulation chain
 *                      from zero, in that order whatever M, N and the batch are.  Then one addition of the bias, one of the residual, and
 *                      act: CF_PW_NONE, or CF_PW_RELU (v > 0 ? v : +0, a NaN stays).  cin % 4 == 0, ld_x % 4 == 0, x and wp 16-byte
 *                      aligned (x is read four channels at a time; res and out one float at a time: ld_res and ld_out are any value >= cout); bias may be NULL (zero), res may be NULL.  A padded k multiplies a stored zero by a stored zero.
 *   cf_nearest_add     out = a + nearest(b -> a's size): a / out [batch][ha][wa][c], b [batch][hb][wb][c], c % 4 == 0; the source index of
 *                      destination index d on an axis is min((int)floorf((float)d * scale), n_in - 1) with scale = (float)n_in / (float)n_out
 *                      computed once: F.interpolate(mode='nearest', size=...) as torch evaluates it (retinaface_net.py:94-99), followed by
 *                      one fp32 addition -- bitwise `a + F.interpolate(b, size=a's, mode='nearest')`.
 *   cf_retina_decode   the detector's tail on the fused head outputs.  Level l (0 .. 2) is heads[l]: [batch][np_l] pixels of 32 floats, anchor
 *                      a (0, 1) of a pixel at floats 16 a .. 16 a + 15: 4 box regressions, 2 class logits, 10 landmark regressions.  Anchor
 *                      i of an image (n = 2 (np_0 + np_1 + np_2), level-major, pixel-major, anchor-minor: the order of PriorBox) has
 *                      priors[i] = (cx, cy, w, h).  Softmax: m = max(l0, l1), e_j = expf(l_j - m), p_j = e_j / (e_0 + e_1).
 *                      Full mode (bbox != NULL): bbox [batch][n][4], conf [batch][n][2], ldm [batch][n][10] = the regressions as they are,
 *                      the softmax, the landmark regressions: what RetinaFace.forward returns.
 *                      Compact mode (rows != NULL): per anchor, score = p_1;  box (retinaface_utils.py:254-271): c = prior.xy + (loc.xy * var0)
 *                      * prior.wh, s = prior.wh * expf(loc.wh * var1), lo = c - s / 2, hi = s + lo;  landmarks (:274-294): prior.xy +
 *                      (pre * var0) * prior.wh;  each value then (v * scale) / resize with scale = img_w for x, img_h for y -- every step one
 *                      fp32 operation, none contracted.  The anchors with score > conf_threshold are written as rows of 15 floats (x1, y1,
 *                      x2, y2, score, 5 x (lx, ly)) to rows [batch][cap][15] in ASCENDING anchor order: one workgroup per image counts,
 *                      scans and writes chunk by chunk, no atomic append.  counts [batch] (int32) receives the TRUE number of passing
 *                      anchors; rows beyond cap are not written, and the caller that sees counts[b] > cap takes the full mode instead.
 *                      One mode per call: asking for both, or for neither, is refused.  np_l >= 0, n >= 1, batch <= 65535. */
#define CF_PW_NONE 0
#define CF_PW_RELU 1
int64_t cf_pointwise_packed_elems(int cin, int cout);
int cf_pack_pointwise(const float* w, int cin, int cout, float* wp, cf_stream_t stream);
int cf_pointwise(const float* x, int ld_x, const float* wp, const float* bias, const float* res, int ld_res, int batch, int h, int w, int cin,
                 int cout, int step, int act, float* out, int ld_out, cf_stream_t stream);
int cf_nearest_add(const float* a, const float* b, int batch, int ha, int wa, int hb, int wb, int c, float* out, cf_stream_t stream);
int cf_retina_decode(const float* heads0, const float* heads1, const float* heads2, int np0, int np1, int np2, const float* priors, int batch,
                     float var0, float var1, float img_w, float img_h, float resize, float conf_threshold, float* bbox, float* conf, float* ldm,
                     float* rows, int cap, int* counts, cf_stream_t stream);

/* ---- alignment warp and paste-back of the whole-image / video path ----------------------------------------------------------
 * Replaces the OpenCV calls of facelib/utils/face_restoration_helper.py: cv2.warpAffine of align_warp_face (:343-344) and of
 * paste_faces_to_input_image (:400, :428, :479), cv2.erode (:430-431, :447), cv2.GaussianBlur (:449), np.sum (:433), the soft-mask
 * blend (:485-492), cv2.resize of the background (:380) and the final astype(uint8) (:497).  OpenCV's fixed-point definitions are
 * followed bit for bit as restated in oracle/paste_oracle.py (OpenCV itself is not available to pin them).  Affine arguments are
 * the matrices that map DESTINATION pixels to SOURCE coordinates (what warpAffine obtains by inverting its M, in double).
 * Regions (rx, ry, rw, rh) are windows of the destination frame; *_region buffers are compact [rh][rw] float32 arrays. */
/* n warps in one launch: dst[i] (u8 [dh][dw][3]) region <- src + i*src_stride (u8 [sh][sw][3]; stride 0 = one source) through
 * inv_dev[i] (DEVICE array of n x 6 doubles); taps outside the source take (b0, b1, b2) */
int cf_warp_affine_u8(const uint8_t* src, int64_t src_stride, int sh, int sw, const double* inv_dev, int n, uint8_t* dst, int dh, int dw,
                      int rx, int ry, int rw, int rh, int b0, int b1, int b2, cf_stream_t stream);
/* float32 single-channel warp into a compact region buffer (border 0); inv_host: 6 doubles in HOST memory */
int cf_warp_affine_f32(const float* src, int sh, int sw, const double* inv_host, float* dst_region, int rx, int ry, int rw, int rh,
                       cf_stream_t stream);
/* cv2.erode with a k x k rectangle (anchor k/2; k == 0 -> OpenCV's 3x3 default); samples outside the region do not take part */
int cf_erode_f32(const float* in_region, float* tmp_region, float* out_region, int rh, int rw, int k, cf_stream_t stream);
/* cv2.GaussianBlur(ksize, 0) with the caller's taps (DEVICE, ksize floats), BORDER_REFLECT_101 at the borders of the ch x cw frame
 * the region (rx, ry) lies in; frame positions outside the region count as 0 */
int cf_gaussian_blur_f32(const float* in_region, float* tmp_region, float* out_region, int rh, int rw, int rx, int ry, int ch, int cw,
                         const float* taps_dev, int ksize, cf_stream_t stream);
/* 64 fp64 partial sums of x[0..n) in a fixed order (the caller adds them) */
int cf_sum_f32(const float* x, int64_t n, double* partials64, cf_stream_t stream);
/* canvas (f32 [ch][cw][3]) region <- m * (ero * warp(face)) + (1 - m) * canvas, m = soft (or min(parse, soft) when parse != NULL) */
int cf_paste_blend(float* canvas, int ch, int cw, const uint8_t* face, int fh, int fw, const double* inv_host, const float* ero_region,
                   const float* soft_region, const float* parse_region, int rx, int ry, int rw, int rh, cf_stream_t stream);
/* cv2.resize(src u8 [sh][sw][3], INTER_LINEAR) -> f32 [dh][dw][3] (a plain widening copy when the sizes are equal) */
int cf_resize_linear_u8(const uint8_t* src, int sh, int sw, float* dst, int dh, int dw, cf_stream_t stream);
/* cv2.resize(src u8 [sh][sw][3], (dw, dh), INTER_AREA) -> u8 [dh][dw][3], dh <= sh and dw <= sw: the reduction of a frame to the detector's
 * working size (facelib/utils/face_restoration_helper.py:208-215) */
int cf_resize_area_u8(const uint8_t* src, int sh, int sw, uint8_t* dst, int dh, int dw, cf_stream_t stream);
/* astype(np.uint8) of a float image in [0, 256): truncation */
int cf_f32_to_u8_trunc(const float* src, int64_t n, uint8_t* dst, cf_stream_t stream);
/* parse-map colouring out[i] = lut[labels[i]] (face_restoration_helper.py:468-471; lut_host: nlut <= 32 floats in HOST memory) */
int cf_label_lut_f32(const int64_t* labels, int64_t n, const float* lut_host, int nlut, float* out, cf_stream_t stream);
/* in place: x * scale inside the frame of `border` pixels, 0 on it (face_restoration_helper.py:476-481), x: [batch][h][w] */
int cf_scale_clear_border_f32(float* x, int batch, int h, int w, int border, float scale, cf_stream_t stream);
/* draw_box fused with the final astype(uint8) (face_restoration_helper.py:439-445, :497-509): out (u8 [ch][cw][3]) = imwrite's rint /
 * saturate of the truncated canvas (f32 [ch][cw][3]) blended, face by face in order, with green through the warp of each face's border
 * band (ones on the outer `border` pixels of the fh x fw face, zeros inside).  faces_dev: DEVICE array of nfaces x 11 doubles = the
 * dst->src matrix (6), border, and the band's bounding box x0, y0, x1, y1 in canvas pixels (outside it the warped band is 0).
 * nfaces == 0 is a plain truncation. */
int cf_box_overlay_u8(const float* canvas, int ch, int cw, const double* faces_dev, int nfaces, int fh, int fw, uint8_t* out,
                      cf_stream_t stream);
/* cv2.resize(float32 plane, (dw, dh), INTER_LINEAR) of `batch` planes [batch][sh][sw] -> [batch][dh][dw] (face_restoration_helper.py:482:
 * the 512^2 soft parse masks brought to the upsampled face size) */
int cf_resize_linear_f32(const float* src, int batch, int sh, int sw, float* dst, int dh, int dw, cf_stream_t stream);
/* Face upsampler tile I/O (RealESRGANer.enhance_faces).  Gather: u8 BGR faces [n][h][w][3] -> f32 RGB NCHW [n][3][th][tw] = window
 * (py0, px0) of the padded view pre_process builds (reflect pre-pad on the right / bottom, reflect pad to a multiple of mod), / 255 */
int cf_esrgan_tile_gather_u8(const uint8_t* faces, int n, int h, int w, int pre_pad, int mod, int py0, int px0, int th, int tw, float* out,
                             cf_stream_t stream);
/* Scatter: the ch x cw core at (oy, ox) of the model's f32 RGB NCHW output [n][3][uh][uw] -> (dy, dx) of u8 BGR faces [n][oh][ow][3],
 * rint(clamp(v, 0, 1) * 255.0f) */
int cf_esrgan_tile_scatter_u8(const float* up, int n, int uh, int uw, int oy, int ox, int ch, int cw, uint8_t* out, int oh, int ow, int dy,
                              int dx, cf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CODEFORMER_HIP_H */
