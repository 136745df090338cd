// What the convolution kernels behind cf_conv2d share (cf_igemm.hip, cf_split.hip, cf_winograd.hip, cf_wsplit.hip, cf_wf43.hip; the token
// GEMMs of cf_gemm_split.hip take the split-half product from here):
//   head   the XCD-contiguous workgroup order, the range scale of an un-normalised input, the gather prologue on a value or a quad, the
//          runtime -> compile-time dispatch of the prologue and of the epilogue triple, the three-MFMA split-half product;
//   tail   the swish of the GroupNorm prologue, the epilogue arithmetic on a quad of channels, the GroupNorm partials of the output;
//   host   the descriptor fields every argument struct has, the checks the launchers repeat, the prototypes by which the files call each other
//          (the weight packers of every family live in cf_pack.hip and take the F(4,3) slab-form rule from here).
// Pieces, all forceinline: a kernel keeps its own loops, staging and store order and calls these for the arithmetic, so that the order of
// every addition is written down once.
//
// A site uses a piece only where the compiled function stayed instruction-identical to the one with the text written out
// (tools/strip_experiment_macros.py --verify).  Sites that keep their own text, each with a comment naming the piece it spells out:
//   cf_act_scales     cf_winograd.hip, cf_wsplit.hip, cf_split.hip (the helper changed the branch structure around the null test; it
//                     serves cf_wf43.hip)
//   cf_pro_apply4     cf_split.hip convert_mode;  cf_pro_apply: cf_igemm.hip store_A_mode (another swish: see cf_swish)
//   cf_with_prologue  cf_split.hip, cf_igemm.hip;  cf_with_epilogue: cf_split.hip (device switches; the host ones all use the helpers)
//   cf_mma3_f16x2     cf_split.hip `mma` (each of the three products is taken over all mi / ni tiles before the next, so consecutive
//                     MFMAs go to different accumulators); cf_wf43.hip has other MFMA shapes and interleaves two positions
//   cf_gn_partials    cf_winograd.hip, cf_split.hip, cf_wf43.hip;  cf_epi_*: the vector epilogue of cf_igemm.hip, cf_wf43.hip (pairs)
// The halo index loop, the column pass and the nu-axis contraction that cf_winograd.hip and cf_wsplit.hip have in common are still two copies.
#pragma once
#include <type_traits>

#include "cf_common.h"

// ---- launchers and geometry queries of the kernel families (conv_dispatch / splitk_geometry in cf_igemm.hip call them) --------------------
// sft_w_img (cf_conv2d_sft_w; the families with an SFT epilogue): [batch] device floats, image b's weight of CF_EPI_SFT in place of d->sft_w.
int cf_winograd_launch(const cf_conv_desc* d, hipStream_t stream, int* parts_query, const float* sft_w_img = nullptr);  // cf_winograd.hip: F(2,3), fp32 or split-half operands
bool cf_wsplit_covers(const cf_conv_desc* d);                                         // cf_wsplit.hip: the eight-wave, 128-channel F(2,3) form,
int cf_wsplit_launch(const cf_conv_desc* d, hipStream_t stream, int* parts_query, const float* sft_w_img = nullptr);   // called by cf_winograd_launch for what it covers
int cf_wf43_launch(const cf_conv_desc* d, hipStream_t stream, int* parts_query, const float* sft_w_img = nullptr);      // cf_wf43.hip: F(4,3)
int cf_ksum_launch(const cf_conv_desc* d, hipStream_t stream, const float* sft_w_img);                                    // cf_ksum.hip: sum of the K parts of cf_wf43_launch + epilogue + statistics
bool cf_wf43_k32(int cout, int cin);                                                // cf_wf43.hip: F(4,3) / F(4,2) on 32-channel slabs? (cf_wf43_launch and the packers of cf_pack.hip)
int cf_split_launch(const cf_conv_desc* d, hipStream_t stream, int* parts_query, const float* sft_w_img = nullptr);     // cf_split.hip: direct, split-half operands
int cf_gemm_split_launch(const cf_conv_desc* d, hipStream_t stream, int* parts_query);  // cf_gemm_split.hip: split-half token GEMM
int cf_gemm_f32_tile_try(const cf_conv_desc* d, hipStream_t stream);                  // cf_gemm_split.hip: fp32 token tiles (CF_OK: launched, 1: not its shape)
// split-K geometry: output tiles of the launch and accumulator bytes one (tile, split) parks in the workspace
int cf_gemm_split_geometry(const cf_conv_desc* d, int* tiles, long* bytes_per_part);
int cf_winograd_splitk_geometry(const cf_conv_desc* d, int* tiles, long* bytes_per_part);
int cf_split_splitk_geometry(const cf_conv_desc* d, int* tiles, long* bytes_per_part);

// The descriptor fields that every kernel family's argument struct carries under the same name.  What differs per family stays in its
// launcher: K-slab count, image size fields, tiling, nparts, the stats_cpg default, acc_scale / act_scale, strides.  The structs keep
// their own members, order and size (the kernarg size feeds register allocation; each has a static_assert on its sizeof).
template <class A>
inline void cf_fill_conv_args(A& a, const cf_conv_desc* d, const float* sft_w_img = nullptr) {
  a.in0 = d->in0;
  a.in1 = d->in1;
  a.c0 = d->c0;
  a.c1 = d->c1;
  a.cin = d->c0 + d->c1;
  a.batch = d->batch;
  a.cout = d->cout;
  a.prologue = d->prologue;
  a.epilogue = d->epilogue;
  a.pro_scale = d->pro_scale;
  a.pro_shift = d->pro_shift;
  a.weight = d->weight;
  a.bias = d->bias;
  a.res = d->res;
  a.sft_scale = d->sft_scale;
  a.sft_w = d->sft_w;
  a.sft_w_img = sft_w_img;
  a.out = d->out;
  a.stats_out = d->stats_out;
}

// ---- host checks the launchers repeat --------------------------------------------------------------------------------------------------
// Each launcher keeps the place of a check among its other checks (the first failing one decides the message) and, where the families
// word a refusal differently, its text.
inline bool cf_epi_is_quad_triple(const cf_conv_desc* d) {  // the epilogues cf_epi_apply knows
  return d->epilogue == CF_EPI_NONE || d->epilogue == CF_EPI_RESIDUAL || d->epilogue == CF_EPI_SFT;
}
inline bool cf_dense_zero_pad(const cf_conv_desc* d) {  // dense NHWC tensors (no channel stride), zero padding
  return d->pad_mode == CF_PAD_ZERO && (d->ld_in0 == 0 || d->ld_in0 == d->c0) && (d->ld_in1 == 0 || d->ld_in1 == d->c1) &&
         (d->ld_out == 0 || d->ld_out == d->cout);
}
inline int cf_require_acc_scale(const cf_conv_desc* d, const char* family) {  // family: "cf_conv2d(f16x2)", ..
  CF_REQUIRE(d->acc_scale > 0.f, "%s: acc_scale must be the inverse of the pack-time weight scale (got %g)", family, (double)d->acc_scale);
  return CF_OK;
}

// ---- workgroup order -------------------------------------------------------------------------------------------------------------------
// Workgroup b runs on XCD b % 8 (observed dispatch order; speed only, never correctness).  Give every XCD a contiguous run of tile ids
// so neighbouring tiles -- which share halo rows / columns and the weight slabs -- hit the same L2.  Bijective for any grid size.
__device__ __forceinline__ int cf_xcd_tile(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, k = bid >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
}

// ---- runtime value -> template parameter -----------------------------------------------------------------------------------------------
// f(std::integral_constant<int, P>{}) for the prologue (enum cf_prologue) / for the epilogue triple of cf_epi_apply; host and device.
template <class F>
__host__ __device__ __forceinline__ void cf_with_prologue(int prologue, F&& f) {
  switch (prologue) {
    case CF_PRO_AFFINE: f(std::integral_constant<int, CF_PRO_AFFINE>{}); break;
    case CF_PRO_AFFINE_SWISH: f(std::integral_constant<int, CF_PRO_AFFINE_SWISH>{}); break;
    case CF_PRO_LEAKY: f(std::integral_constant<int, CF_PRO_LEAKY>{}); break;
    default: f(std::integral_constant<int, CF_PRO_NONE>{}); break;
  }
}
template <class F>
__host__ __device__ __forceinline__ void cf_with_epilogue(int epilogue, F&& f) {
  switch (epilogue) {
    case CF_EPI_RESIDUAL: f(std::integral_constant<int, CF_EPI_RESIDUAL>{}); break;
    case CF_EPI_SFT: f(std::integral_constant<int, CF_EPI_SFT>{}); break;
    default: f(std::integral_constant<int, CF_EPI_NONE>{}); break;
  }
}

// ---- prologue --------------------------------------------------------------------------------------------------------------------------
// x * sigmoid(x) on the hardware exp and the hardware reciprocal (v_exp_f32 / v_rcp_f32, ~1 ulp each): the GroupNorm-swish gather of the
// split-half and Winograd kernels.  cf_igemm.hip keeps two other forms (__frcp_rn in its MFMA gather, a true division in the vector-ALU
// first conv): the three differ in the last bits and are not interchangeable.
__device__ __forceinline__ float cf_swish(float y) { return y * __builtin_amdgcn_rcpf(1.0f + __expf(-y)); }

// Range scale of an un-normalised input of the 16-bit-operand kernels (cf_conv_desc.act_scale, [image][2] = (s, 1 / s), powers of two:
// x * s and acc / s are exact); 1 when unused.  s02 is the LeakyReLU slope folded with the scale: fl(y * (0.2 s)) == fl(0.2 y) * s,
// because s only moves the exponent.
template <bool USE>
__device__ __forceinline__ void cf_act_scales(const float* act_scale, int b, float& s, float& inv_s, float& s02) {
  s = 1.f;
  inv_s = 1.f;
  if (USE && act_scale) {
    s = act_scale[2 * b];
    inv_s = act_scale[2 * b + 1];
  }
  s02 = 0.2f * s;
}

// The gather prologue on one value: GroupNorm apply (sc, sh), the same with swish, LeakyReLU(0.2), none.  SCALED: the kernel multiplies
// an un-normalised input (LEAKY, NONE) by its range scale s (cf_act_scales); SCALED = false is the fp32 form -- no multiply for NONE.
template <int PRO, bool SCALED>
__device__ __forceinline__ float cf_pro_apply(float y, float sc, float sh, float s, float s02) {
  if (PRO == CF_PRO_AFFINE) y = y * sc + sh;
  if (PRO == CF_PRO_AFFINE_SWISH) {
    y = y * sc + sh;
    y = cf_swish(y);
  }
  if (PRO == CF_PRO_LEAKY) y = SCALED ? y * (y > 0.f ? s : s02) : (y > 0.f ? y : 0.2f * y);
  if (SCALED && PRO == CF_PRO_NONE) y = y * s;
  return y;
}
// ... on a quad of channels of one pixel.  Zero padding pads the conv INPUT, i.e. the post-activation tensor: an out-of-image value
// (`valid` false; its load came from a clamped address) is an exact zero whatever the prologue would make of it.
template <int PRO, bool SCALED>
__device__ __forceinline__ f32x4 cf_pro_apply4(f32x4 v, f32x4 sc, f32x4 sh, float s, float s02, bool valid) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float y = cf_pro_apply<PRO, SCALED>(v[e], sc[e], sh[e], s, s02);
    v[e] = valid ? y : 0.f;
  }
  return v;
}

// ---- split-half product ----------------------------------------------------------------------------------------------------------------
// a * b with both operands as hi + lo IEEE halves (8 per lane: the 32x32x16 shape): lo*hi, then hi*lo, then hi*hi into one fp32
// accumulator (the dropped lo*lo term is <= 2^-22 |a b|).  The order is part of every default-mode result.
typedef _Float16 cf_f16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ void cf_mma3_f16x2(f32x16& acc, f32x4 ah, f32x4 al, f32x4 bh, f32x4 bl) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(cf_f16x8, al), __builtin_bit_cast(cf_f16x8, bh), acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(cf_f16x8, ah), __builtin_bit_cast(cf_f16x8, bl), acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(cf_f16x8, ah), __builtin_bit_cast(cf_f16x8, bh), acc, 0, 0, 0);
}

// ---- epilogue on a quad of channels ----------------------------------------------------------------------------------------------------
// A thread owns four consecutive output channels of a pixel at element offset `off` (the same offset in res, sft_scale and out: dense
// NHWC tensors of cout channels).  Operand first: the residual / SFT operands of ALL of a thread's quads are requested before the
// accumulators are taken to the output layout (LDS transpose or Winograd output transform), so that their HBM latency overlaps it; then
// per quad  scale + bias -> residual / SFT -> store -> statistics.  BIO: the tensors hold bf16 (cf_common.h), the value is rounded
// once in the store, after the statistics operands were taken from the fp32 value.
//
// Two steps stay written out in the kernels, because as helpers they changed the code the compiler made of them (another register
// allocation; unpacked instead of packed fp32 arithmetic in the bf16-storage instantiations):
//   * which operands an epilogue reads -- r0 = res for RESIDUAL and SFT, r1 = sft_scale for SFT, zeros otherwise -- is three lines
//     around cf_epi_load4 at each fetch;
//   * the per-thread fp32 sums of what was written:  ssum[e] += v[e];  ssq[e] += v[e] * v[e].
template <bool BIO>
__device__ __forceinline__ f32x4 cf_epi_load4(const float* base, size_t off) {
  if constexpr (BIO) return cf_load4_bf16(base, off);
  else return *reinterpret_cast<const f32x4*>(base + off);
}
// acc * s + bias where the kernel has an accumulator scale (a power of two: exact), acc + bias where it has none.  The expression shapes
// here and in cf_epi_apply are part of the result: the compiler contracts them into FMAs as written.
template <bool SCALED>
__device__ __forceinline__ f32x4 cf_epi_bias(f32x4 v, float s, f32x4 bias4) {
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = SCALED ? v[e] * s + bias4[e] : v[e] + bias4[e];
  return v;
}
// RESIDUAL: v + r0.  SFT: r0 + w * (r0 * r1 + v), w = cf_sft_weight of the image the quad belongs to.  (The vector epilogue of cf_igemm.hip -- edge-tile mask, GELU / LEAKY / AXPY of the
// general instantiations -- keeps its own text: written with these helpers most of its instantiations compiled to other code.)
// The SFT weight of image b: the descriptor's scalar, or -- cf_conv2d_sft_w -- entry b of the per-image table.  One expression for both
// launches, so the arithmetic that follows (FMA contraction included) is the same instruction sequence; b is wave-uniform at every call
// site (a patch or tile lies in one image), so this is one scalar load per patch, like act_scale.
__device__ __forceinline__ float cf_sft_weight(const float* sft_w_img, float sft_w, int b) { return sft_w_img ? sft_w_img[b] : sft_w; }
__device__ __forceinline__ f32x4 cf_epi_apply(f32x4 v, int epi, f32x4 r0, f32x4 r1, float w) {
  if (epi == CF_EPI_RESIDUAL) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] += r0[e];
  } else if (epi == CF_EPI_SFT) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = r0[e] + w * (r0[e] * r1[e] + v[e]);
  }
  return v;
}
template <bool BIO>
__device__ __forceinline__ void cf_epi_store(float* out, size_t off, f32x4 v, bool nt = false) {
  if constexpr (BIO) cf_store4_bf16(out, off, v);   // (rounded here, once)
  else cf_store16(out + off, v, nt);
}

// ---- GroupNorm partials of the output --------------------------------------------------------------------------------------------------
// stats_out is [image][group][nparts][2] doubles: one (sum, sumsq) partial of the values just written per (image, group, part), where a
// part is the share of one wave (the direct and F(2,3) kernels: nparts = tiles per image x waves along M) or of one workgroup (F(4,3)).
// cf_groupnorm_finalize2 (cf_norm.hip) adds the parts of a group in index order, so the statistics -- and with them the bitwise batch
// invariance of the network -- are a function of the per-image shape only, provided the order below never depends on anything else.
__device__ __forceinline__ double* cf_gn_partial_ptr(double* stats_out, int b, int cout, int cpg, int n, int nparts, size_t part) {
  const int ng = cout / cpg;
  return stats_out + (((size_t)b * ng + n / cpg) * nparts + part) * 2;
}

// From a thread's sums over its quad (channels n .. n + 3 of image b) to the stores.  The order, the same at every call site:
//   1. fp32 -> fp64, the quad's channels pairwise: (s0 + s1) + (s2 + s3); with cpg == 2 the two pairs are two groups (d0 / d1);
//   2. __shfl_xor over the lanes that hold the same quad in other rows, distances first, 2 first, .. 32 (`first` = lanes per row);
//   3. __shfl_xor over the adjacent quads of one group, distances 1, 2, .. while 4 * distance < cpg;
//   4. the lane with `writes` whose quad opens a group stores the pair (cpg == 2: and the pair of group n / 2 + 1).
// PAIR says how a call site treats the second group of cpg == 2 -- the values stored are the same, the instructions are not:
//   CF_GN_QUAD  the kernel never sees cpg < 4 (cout >= 128);  CF_GN_PAIR_IF  d1 / q1 take step 2 in a loop of their own under cpg == 2;
//   CF_GN_PAIR  d1 / q1 ride through step 2 with d0 / q0 unconditionally.
enum { CF_GN_QUAD = 0, CF_GN_PAIR_IF = 1, CF_GN_PAIR = 2 };
template <int PAIR>
__device__ __forceinline__ void cf_gn_partials(const float (&ssum)[4], const float (&ssq)[4], double* stats_out, int cpg, int first, bool writes,
                                               size_t part, int nparts, int cout, int n, int b) {
  double d0, q0, d1 = 0, q1 = 0;
  if (PAIR != CF_GN_QUAD && cpg == 2) {  // two groups per lane
    d0 = (double)ssum[0] + ssum[1];
    q0 = (double)ssq[0] + ssq[1];
    d1 = (double)ssum[2] + ssum[3];
    q1 = (double)ssq[2] + ssq[3];
  } else {
    d0 = ((double)ssum[0] + ssum[1]) + ((double)ssum[2] + ssum[3]);
    q0 = ((double)ssq[0] + ssq[1]) + ((double)ssq[2] + ssq[3]);
  }
  for (int o = first; o < 64; o <<= 1) {
    d0 += __shfl_xor(d0, o, 64);
    q0 += __shfl_xor(q0, o, 64);
    if (PAIR == CF_GN_PAIR) {
      d1 += __shfl_xor(d1, o, 64);
      q1 += __shfl_xor(q1, o, 64);
    }
  }
  if (PAIR == CF_GN_PAIR_IF && cpg == 2) {  // (a wave-uniform branch)
    for (int o = first; o < 64; o <<= 1) {
      d1 += __shfl_xor(d1, o, 64);
      q1 += __shfl_xor(q1, o, 64);
    }
  }
  for (int o = 1; o * 4 < cpg; o <<= 1) {  // (cpg >= 8)
    d0 += __shfl_xor(d0, o, 64);
    q0 += __shfl_xor(q0, o, 64);
  }
  if (writes && (n % cpg) == 0) {
    double* op = cf_gn_partial_ptr(stats_out, b, cout, cpg, n, nparts, part);
    op[0] = d0;
    op[1] = q0;
    if (PAIR != CF_GN_QUAD && cpg == 2) {
      op[(size_t)nparts * 2] = d1;
      op[(size_t)nparts * 2 + 1] = q1;
    }
  }
}
