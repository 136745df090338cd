// Implicit-GEMM convolution / linear on fp32 MFMA (v_mfma_f32_32x32x2_f32) for gfx950.
//
// One kernel template covers every dense contraction of the CodeFormer hot path
// (reference call sites: include/codeformer_hip.h, cf_conv2d):
//   out[pixel][n] = epilogue( sum_{tap, c} prologue(in[pixel + tap][c]) * W[n][c][tap] + bias[n] )
// GEMM view: M = batch*hout*wout output pixels, N = cout, K = taps*cin.
//
// Data layout in HBM: activations channels-last fp32 ([b][h][w][c]); weights pre-packed as
// [tap][cin/16][cout_pad][16] so a (tap, k-slab, n-tile) weight slab is one contiguous block.
//
// Work decomposition: a 256-thread workgroup (4 waves) owns a BM x BN output tile; BM is a TH x 16
// spatial patch of ONE image.  For each 16-channel slab the (TH*s+2) x (16*s+2) input halo patch is
// gathered once into LDS -- with the GroupNorm-apply/swish (or LeakyReLU) prologue, the nearest-x2
// upsample, the channel concat of two inputs and the zero padding all resolved in that gather -- and
// is then reused by all 9 taps; the per-tap weight slab is double-buffered in LDS and prefetched
// through registers while the MFMAs of the previous tap run.  Each wave accumulates a
// (MI*32) x (NI*32) sub-tile in MI*NI*16 accumulator registers.
#include <string.h>
#include <type_traits>

#include "cf_conv_parts.h"

namespace {

struct ConvArgs {
  const float* in0;
  const float* in1;
  int c0, c1, cin, nchunks;
  int batch, hin, win, hout, wout;
  int cout, cout_pad;
  int upsample, out_nchw, prologue, epilogue;
  const float* pro_scale;
  const float* pro_shift;
  const float* weight;
  const float* bias;
  const float* res;
  const float* sft_scale;
  const float* sft_w_img;  // SFT: [batch] weights, one per image (cf_conv2d_sft_w), or null: sft_w for all of them
  float* out;
  double* stats_out;  // optional [batch][cout/stats_cpg][nparts][2] partial (sum, sumsq) of the OUTPUT
  int stats_cpg, nparts;
  int tiles_x, tiles_per_img, ntn;
  float sft_w;  // (behind ntn: the block keeps its size)
};
// The general (EXT) instantiations take a longer argument block; the CodeFormer kernels keep the exact ConvArgs layout
// (the kernarg size feeds register allocation: growing it perturbed every instantiation's code).
struct ConvArgsExt : ConvArgs {
  int ld0, ld1, ldo;  // channel strides of in0 / in1 / out (and res, res2)
  int pad_mode;       // CF_PAD_ZERO / CF_PAD_REFLECT (3x3) / CF_PAD_EDGE (folded upsample)
  int pad_lo;         // stride 2: rows / columns of padding on the top / left (0 = CodeFormer Downsample, 1 = symmetric)
  int nt_out;         // non-temporal output stores (the first conv; cf_common.h: cf_store16)
};
// border handling of the gather for the EXT instantiations: coordinate remap instead of zero fill
__device__ __forceinline__ int cf_border(int i, int n, int mode) {
  if (mode == CF_PAD_REFLECT) {
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * n - 2 - i : i;
  }
  return i < 0 ? 0 : (i >= n ? n - 1 : i);  // (also keeps the overhang of masked edge tiles addressable)
}
// Split-K instantiations (1x1 / Linear on small token matrices): workspace, ticket counters and the split count ride behind the
// ConvArgs fields, again in their own struct so the other instantiations keep their kernarg layout.
struct ConvArgsSK : ConvArgs {
  float* ws;
  unsigned* counters;
  int nsplit;
};
static_assert(sizeof(ConvArgs) == 176 && sizeof(ConvArgsExt) == 200 && sizeof(ConvArgsSK) == 200, "the kernarg blocks keep their size: it feeds the register allocation of every instantiation");
template <bool EXT, bool SK = false>
using ArgsOf = std::conditional_t<SK, ConvArgsSK, std::conditional_t<EXT, ConvArgsExt, ConvArgs>>;
template <bool EXT, bool SK = false>
__device__ __forceinline__ int ext_ld(const ArgsOf<EXT, SK>& a, int which, int dense) {
  if constexpr (EXT) return which == 0 ? a.ld0 : (which == 1 ? a.ld1 : a.ldo);
  return dense;
}

template <int TAPS, int STRIDE, int WM, int WN, int MI, int NI>
struct Cfg {
  static constexpr int BM = WM * MI * 32;
  static constexpr int BN = WN * NI * 32;
  static constexpr int TW = 16;
  static constexpr int TH = BM / 16;
  // TAPS: 9 = 3x3 ; 4 = nearest-x2 + 3x3 folded into four 2x2 sub-pixel convolutions (one output parity class per
  // workgroup, taps pre-summed at pack time: 4 instead of 9 MACs per weight) ; 1 = 1x1 / Linear
  static constexpr int HH = (TAPS == 9) ? (TH - 1) * STRIDE + 3 : (TAPS == 4 ? TH + 1 : TH);   // halo patch rows
  static constexpr int HWD = (TAPS == 9) ? (TW - 1) * STRIDE + 3 : (TAPS == 4 ? TW + 1 : TW);  // halo patch cols
  static constexpr int NPIX = (TAPS > 1) ? HH * HWD : BM;
  static constexpr int ABUF = (TAPS == 1) ? 3 : 1;    // 1x1: the A rows ride in a ring like the weights
  static constexpr int APT = (NPIX * 4 + 255) / 256;  // float4 gather items per thread
  static constexpr int BPT = (BN * 4 + 255) / 256;    // float4 weight items per thread
  static constexpr int BBUF = 3;                      // weight-slab ring depth in LDS
  static constexpr int LDS_MAIN = ABUF * NPIX * CF_LDK + BBUF * BN * CF_LDK;
  static constexpr int LDS_EPI = 4 * 32 * (NI * 32 + 4);  // per-wave 32-row transpose buffers of the epilogue
  static constexpr int LDS_FLOATS = LDS_MAIN > LDS_EPI ? LDS_MAIN : LDS_EPI;
};

// x * sigmoid(x) with sigmoid = 1/(1+exp(-x)), the operation order of vqgan_arch.py:18-20
__device__ __forceinline__ float swishf(float y) { return y * (1.0f / (1.0f + expf(-y))); }

// BF16 = true: the same schedule on v_mfma_f32_32x32x16_bf16 -- a K slab is 32 channels stored as bf16 (the LDS row is
// still 64 B + 16 B pad, so every LDS address below is unchanged), activations are rounded to bf16 (RNE) in the gather
// after the prologue, weights are pre-packed bf16, accumulation stays fp32.  Used for the generator / CFT convs of the
// bf16 configurations only; the fp32 instantiations are bit-for-bit what they were.
//
// EXT = true: the general variant used by dense-block networks (Real-ESRGAN RRDBNet): inputs / outputs are channel slices
// of wider NHWC buffers (ld0 / ld1 / ldo), image sizes need not be tile multiples (edge tiles are masked in the epilogue;
// the gather already zero-fills outside the image), and the epilogue set is {none, residual, leaky, axpy, axpy2}.  Kept
// behind a template flag so the CodeFormer instantiations stay instruction-for-instruction what they were.
// F16 = true: as BF16 but IEEE half operands on v_mfma_f32_32x32x16_f16 (3 more mantissa bits, same MFMA rate) -- the operand
// format of the reference's `half=True` Real-ESRGAN (inference_codeformer.py:23-27,44) and of CodeFormer's precision='fp16';
// fp32 accumulation and fp32 tensors in HBM.
// SK = true (1x1 / Linear only): `nsplit` workgroups share an output tile, each contracting a contiguous range of K slabs; the partial
// accumulators meet in a workspace and the last arriver adds them in split order (cf_splitk_combine) before the usual epilogue.
// BIO = true (round 6, cf_conv_desc.io_bf16): in0, in1, res, sft_scale and out are bf16 tensors (2 bytes per element); the gather widens on
// load, the vector epilogue rounds once (RNE) after the GroupNorm partials were taken.  Only the instantiations the bf16 mode runs from
// 64x64 pixels up exist (direct bf16 3x3 with 64 output channels, folded upsample, fp32 1x1 on images); every other one is untouched.
template <int TAPS, int STRIDE, int WM, int WN, int MI, int NI, bool IN_NCHW, bool BF16 = false, bool EXT = false, bool F16 = false,
          bool SK = false, bool BIO = false, bool PRELU = false>
__global__ __launch_bounds__(256, 3) void igemm_kernel(const ArgsOf<EXT, SK> a) {
  using C = Cfg<TAPS, STRIDE, WM, WN, MI, NI>;
  // PRELU: the general instantiations that carry the two PReLU epilogues and nothing else.  They are kernels of their own, so every other
  // instantiation is the code it was before those epilogues existed.
  static_assert(!PRELU || (EXT && TAPS == 9 && !BF16 && !F16), "PReLU epilogues: general fp32 3x3 instantiations");
  static_assert(!BIO || (!IN_NCHW && !EXT && !SK && !F16 && STRIDE == 1), "bf16 tensors: dense NHWC stride-1 instantiations only");
  static_assert(!SK || (TAPS == 1 && !EXT && !BF16 && !F16), "split-K: 1x1 / Linear fp32 instantiations");
  constexpr bool LP = BF16 || F16;  // 16-bit MFMA operands
  static_assert(!LP || (TAPS > 1 && STRIDE == 1 && !IN_NCHW), "16-bit operand path: 3x3 stride 1 NHWC only");
  static_assert(!(BF16 && F16), "one operand format");
  static_assert(!EXT || (TAPS > 1 && !IN_NCHW && !BF16), "EXT: 3x3 / folded 2x2, NHWC, fp32 or f16");
  constexpr int KC = LP ? 32 : CF_BK;  // channels per K slab
  constexpr int AV = LP ? 2 : 1;       // float4 fetched per gather item (8 / 4 channels)
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* const As = smem;
  float* const Bs = smem + C::ABUF * C::NPIX * CF_LDK;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WN;
  const int wn = wave % WN;
  const int half = lane >> 5;
  const int l31 = lane & 31;

  int bid = cf_xcd_tile(blockIdx.x, gridDim.x);
  [[maybe_unused]] int split = 0, sk_tile = 0;
  if constexpr (SK) {
    split = bid % a.nsplit;  // the splits of one tile are neighbours in the tile order
    bid /= a.nsplit;
    sk_tile = bid;
  }
  const int nt = bid % a.ntn;
  const int mt = bid / a.ntn;
  const int n0 = nt * C::BN;
  int b, y0 = 0, x0 = 0, m0 = 0;
  int sub_y = 0, sub_x = 0;  // TAPS == 4: output parity class (oy & 1, ox & 1) of this workgroup; y0/x0 are SOURCE coords
  if (TAPS > 1) {
    b = mt / a.tiles_per_img;
    int r = mt - b * a.tiles_per_img;
    if (TAPS == 4) {
      const int cls = r & 3;  // class-minor: the four parity classes of a source tile run side by side on one XCD and share its halo patch in L2 (cf_split.hip)
      r >>= 2;
      sub_y = cls >> 1;
      sub_x = cls & 1;
    }
    const int ty = r / a.tiles_x;
    y0 = ty * C::TH;
    x0 = (r - ty * a.tiles_x) * C::TW;
  } else {
    m0 = mt * C::BM;
    b = m0 / (a.hout * a.wout);
  }
  // SFT weight of the tile's image (a tile lies in one image), read before the kernel's first store so that it is a scalar load; the
  // general instantiations have no SFT epilogue
  [[maybe_unused]] const float sft_w = EXT ? 0.f : cf_sft_weight(a.sft_w_img, a.sft_w, b);

  // ---- gather geometry: item j of this thread is float4 #k4 of halo pixel p = (tid>>2) + 64*j ----
  const int k4 = tid & 3;
  int pix[C::APT];  // source pixel index (b*hin+sy)*win+sx (NCHW: sy*win+sx), -1 = zero padding / unused
#pragma unroll
  for (int j = 0; j < C::APT; ++j) {
    const int p = (tid >> 2) + 64 * j;
    int v = -1;
    if (p < C::NPIX) {
      if (TAPS == 4) {
        // parity 0 reads source rows (y-1, y), parity 1 reads (y, y+1): the 2x2 footprint of the folded taps
        const int hy = p / C::HWD;
        const int hx = p - hy * C::HWD;
        int iy = y0 - 1 + sub_y + hy;
        int ix = x0 - 1 + sub_x + hx;
        if constexpr (EXT) {
          if (a.pad_mode != CF_PAD_ZERO) {
            iy = cf_border(iy, a.hin, a.pad_mode);
            ix = cf_border(ix, a.win, a.pad_mode);
          }
        }
        if (iy >= 0 && iy < a.hin && ix >= 0 && ix < a.win) v = (b * a.hin + iy) * a.win + ix;
      } else if (TAPS == 9) {
        const int hy = p / C::HWD;
        const int hx = p - hy * C::HWD;
        int pad = (STRIDE == 1) ? 1 : 0;
        if constexpr (EXT && STRIDE == 2) pad = a.pad_lo;
        int iy = y0 * STRIDE - pad + hy;
        int ix = x0 * STRIDE - pad + hx;
        if constexpr (EXT) {
          if (a.pad_mode != CF_PAD_ZERO) {
            iy = cf_border(iy, a.hin, a.pad_mode);
            ix = cf_border(ix, a.win, a.pad_mode);
          }
        }
        if (iy >= 0 && iy < a.hin && ix >= 0 && ix < a.win) v = IN_NCHW ? (iy * a.win + ix) : ((b * a.hin + iy) * a.win + ix);
      } else {
        v = m0 + p;
      }
    }
    pix[j] = v;
  }

  // Loads are issued UNCONDITIONALLY from a clamped (always valid) address and zeroed by a select afterwards:
  // a load under a divergent branch makes hipcc wait for it on the spot, which would serialise the prefetch.
  auto load_A = [&](int chunk, f32x4(&ra)[C::APT * AV]) {
    const int c = chunk * KC + k4 * (KC / 4);
    if (IN_NCHW) {
      const size_t plane = (size_t)a.hin * a.win;
      const float* base = a.in0 + (size_t)b * a.c0 * plane;
      const int c1 = a.c0 > 1 ? 1 : 0, c2 = a.c0 > 2 ? 2 : 0, c3 = a.c0 > 3 ? 3 : 0;
#pragma unroll
      for (int j = 0; j < C::APT; ++j) {
        const int pj = pix[j] < 0 ? 0 : pix[j];
        f32x4 v;
        v[0] = base[pj];
        v[1] = base[c1 * plane + pj];
        v[2] = base[c2 * plane + pj];
        v[3] = base[c3 * plane + pj];
        const bool ok = pix[j] >= 0 && c == 0;
        v[0] = ok ? v[0] : 0.f;
        v[1] = (ok && a.c0 > 1) ? v[1] : 0.f;
        v[2] = (ok && a.c0 > 2) ? v[2] : 0.f;
        v[3] = (ok && a.c0 > 3) ? v[3] : 0.f;
        ra[j * AV] = v;
      }
    } else {
      const bool first = c < a.c0;
      const float* src = first ? a.in0 : a.in1;
      int cs = first ? a.c0 : a.c1;
      if constexpr (EXT) cs = first ? a.ld0 : a.ld1;
      const int cc = first ? c : c - a.c0;
#pragma unroll
      for (int j = 0; j < C::APT; ++j) {
        const int pj = pix[j] < 0 ? 0 : pix[j];
        if constexpr (BIO) {  // bf16 tensor: this item's KC / 4 channels are 8 (fp32 operands) or 16 (16-bit operands) bytes
          const unsigned short* sp = reinterpret_cast<const unsigned short*>(src) + (size_t)pj * cs + cc;
          if constexpr (AV == 2) {
            const cf_u32x4 q = *reinterpret_cast<const cf_u32x4*>(sp);
            ra[j * 2] = cf_bf16x4_widen(cf_u32x2{q[0], q[1]});
            ra[j * 2 + 1] = cf_bf16x4_widen(cf_u32x2{q[2], q[3]});
          } else {
            ra[j] = cf_bf16x4_widen(*reinterpret_cast<const cf_u32x2*>(sp));
          }
#pragma unroll
          for (int u = 0; u < AV; ++u)
            if (pix[j] < 0) ra[j * AV + u] = f32x4{0.f, 0.f, 0.f, 0.f};
        } else {
#pragma unroll
          for (int u = 0; u < AV; ++u) {
            f32x4 v = *reinterpret_cast<const f32x4*>(src + (size_t)pj * cs + cc + 4 * u);
            if (pix[j] < 0) v = f32x4{0.f, 0.f, 0.f, 0.f};
            ra[j * AV + u] = v;
          }
        }
      }
    }
  };

  // zero padding must stay exactly zero: it pads the conv INPUT, i.e. the post-activation tensor
  auto store_A_mode = [&](int buf, const f32x4(&ra)[C::APT * AV], int chunk, auto mode) {
    constexpr int PRO = decltype(mode)::value;
    f32x4 sc[AV], sh[AV];
#pragma unroll
    for (int u = 0; u < AV; ++u) {
      sc[u] = f32x4{1.f, 1.f, 1.f, 1.f};
      sh[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (PRO == CF_PRO_AFFINE || PRO == CF_PRO_AFFINE_SWISH) {
        const int c = chunk * KC + k4 * (KC / 4) + 4 * u;
        sc[u] = *reinterpret_cast<const f32x4*>(a.pro_scale + (size_t)b * a.cin + c);
        sh[u] = *reinterpret_cast<const f32x4*>(a.pro_shift + (size_t)b * a.cin + c);
      }
    }
    float* dst = As + buf * (C::NPIX * CF_LDK) + k4 * 4;
#pragma unroll
    for (int j = 0; j < C::APT; ++j) {
      const int p = (tid >> 2) + 64 * j;
      if ((j + 1) * 64 <= C::NPIX || p < C::NPIX) {
        const bool valid = pix[j] >= 0;
        f32x4 v[AV];
#pragma unroll
        for (int u = 0; u < AV; ++u) {
          v[u] = ra[j * AV + u];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float y = v[u][e];  // (cf_pro_apply<PRO, false> of cf_conv_parts.h written out: this gather has its own swish)
            if (PRO == CF_PRO_AFFINE) y = y * sc[u][e] + sh[u][e];
            if (PRO == CF_PRO_AFFINE_SWISH) {
              y = y * sc[u][e] + sh[u][e];
              y = y * __frcp_rn(1.0f + __expf(-y));  // v_exp_f32 / v_rcp_f32: ~3 ulp of x*sigmoid(x), +1.2..2.5 % on the GN-swish convs
            }
            if (PRO == CF_PRO_LEAKY) y = y > 0.f ? y : 0.2f * y;
            v[u][e] = valid ? y : 0.f;
          }
        }
        if constexpr (F16) {
          typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
          f32x4 packed;  // 8 channels -> 8 IEEE halves (v_cvt_f16_f32, round-to-nearest-even) in 16 bytes
#pragma unroll
          for (int h = 0; h < 4; ++h) {
            const float flo = v[h >> 1][(h & 1) * 2], fhi = v[h >> 1][(h & 1) * 2 + 1];
            const f16x2 pr = {(_Float16)flo, (_Float16)fhi};
            packed[h] = __builtin_bit_cast(float, pr);
          }
          *reinterpret_cast<f32x4*>(dst + p * CF_LDK) = packed;
        } else if constexpr (BF16) {
          f32x4 packed;  // 8 channels -> 8 bf16 (round-to-nearest-even) in 16 bytes, channel order preserved
#pragma unroll
          for (int h = 0; h < 4; ++h) {
            // (copy the lanes out first: __builtin_bit_cast on a vector-element lvalue reads element 0)
            const float flo = v[h >> 1][(h & 1) * 2], fhi = v[h >> 1][(h & 1) * 2 + 1];
            unsigned lo = __builtin_bit_cast(unsigned, flo);
            unsigned hi = __builtin_bit_cast(unsigned, fhi);
            lo += 0x7fffu + ((lo >> 16) & 1u);
            hi += 0x7fffu + ((hi >> 16) & 1u);
            packed[h] = __builtin_bit_cast(float, (lo >> 16) | (hi & 0xffff0000u));
          }
          *reinterpret_cast<f32x4*>(dst + p * CF_LDK) = packed;
        } else {
          *reinterpret_cast<f32x4*>(dst + p * CF_LDK) = v[0];
        }
      }
    }
  };
  auto store_A = [&](int buf, const f32x4(&ra)[C::APT * AV], int chunk) {
    switch (a.prologue) {  // (cf_with_prologue of cf_conv_parts.h written out: through the helper three 1x1 instantiations were scheduled differently)
      case CF_PRO_AFFINE: store_A_mode(buf, ra, chunk, std::integral_constant<int, CF_PRO_AFFINE>{}); break;
      case CF_PRO_AFFINE_SWISH: store_A_mode(buf, ra, chunk, std::integral_constant<int, CF_PRO_AFFINE_SWISH>{}); break;
      case CF_PRO_LEAKY: store_A_mode(buf, ra, chunk, std::integral_constant<int, CF_PRO_LEAKY>{}); break;
      default: store_A_mode(buf, ra, chunk, std::integral_constant<int, CF_PRO_NONE>{}); break;
    }
  };

  constexpr bool B_FULL = (C::BN * 4) % 256 == 0;  // every thread has BPT items (no tail guard)
  auto load_B = [&](int step, f32x4(&rb)[C::BPT]) {
    const int chunk = step / TAPS;
    const int tap = step - chunk * TAPS;
    const int cls_tap = (TAPS == 4) ? (sub_y * 2 + sub_x) * 4 + tap : tap;  // sub-pixel: [class][tap] slabs
    const float* src = a.weight + ((size_t)(cls_tap * a.nchunks + chunk) * a.cout_pad + n0) * CF_BK;
#pragma unroll
    for (int j = 0; j < C::BPT; ++j) {
      int f = tid + 256 * j;
      if (!B_FULL) f = f < C::BN * 4 ? f : 0;
      rb[j] = *reinterpret_cast<const f32x4*>(src + f * 4);
    }
  };
  auto store_B = [&](int buf, const f32x4(&rb)[C::BPT]) {
    float* dst = Bs + buf * (C::BN * CF_LDK);
#pragma unroll
    for (int j = 0; j < C::BPT; ++j) {
      const int f = tid + 256 * j;
      if (B_FULL || f < C::BN * 4) *reinterpret_cast<f32x4*>(dst + (f >> 2) * CF_LDK + (f & 3) * 4) = rb[j];
    }
  };

  // ---- MFMA operand rows of this lane ----
  int a_off[MI], b_off[NI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    const int row = wm * (MI * 32) + mi * 32 + l31;
    if (TAPS > 1) {
      const int py = row >> 4, px = row & 15;
      a_off[mi] = ((py * STRIDE) * C::HWD + px * STRIDE) * CF_LDK + half * 4;
    } else {
      a_off[mi] = row * CF_LDK + half * 4;
    }
  }
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) b_off[ni] = (wn * (NI * 32) + ni * 32 + l31) * CF_LDK + half * 4;

  f32x16 acc[MI][NI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

  const int nsteps = a.nchunks * TAPS;
  f32x4 ra[C::APT * AV];
  f32x4 rb[C::BPT];

  if constexpr (TAPS > 1) {
    // ---- software-pipelined schedule (3x3 / folded 2x2) -----------------------------------------------------------------
    // Weight slabs live in a 3-deep LDS ring: slab t is fetched from HBM/L2 at the start of step t-2, written to
    // LDS at the end of step t-2, made visible by the barrier that opens step t-1, and its first fragments are read
    // in the MIDDLE of step t-1 -- so no wave ever waits on an LDS round trip between two MFMA blocks:
    //     step s:  [barrier] issue loads B(s+2) | read frags(s, k 8..15) | 16 MFMA on frags(s, k 0..7)
    //                        read frags(s+1, k 0..7) | 16 MFMA on frags(s, k 8..15) | LDS write B(s+2)
    // RAW: B(s+1) was written before the barrier opening step s.  WAR: ring slot (s+2)%3 last held B(s-1), whose
    // reads every wave finished before arriving at the barrier opening step s.  The halo patch is single-buffered,
    // so the slab boundary (1 step in 9) drains: barrier, patch write, barrier, fragment read.
    auto read_frags = [&](f32x4(&af)[MI], f32x4(&bf)[NI], int tapoff, int bslot, int kg) {
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) af[mi] = *reinterpret_cast<const f32x4*>(As + a_off[mi] + tapoff + kg * 8);
#pragma unroll
      for (int ni = 0; ni < NI; ++ni)
        bf[ni] = *reinterpret_cast<const f32x4*>(Bs + bslot * (C::BN * CF_LDK) + b_off[ni] + kg * 8);
    };
    auto mma16 = [&](const f32x4(&af)[MI], const f32x4(&bf)[NI]) {
      if constexpr (F16) {
        typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
          for (int ni = 0; ni < NI; ++ni)
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, af[mi]),
                                                                 __builtin_bit_cast(f16x8, bf[ni]), acc[mi][ni], 0, 0, 0);
      } else if constexpr (BF16) {
        typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
          for (int ni = 0; ni < NI; ++ni)
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, af[mi]),
                                                                  __builtin_bit_cast(bf16x8, bf[ni]), acc[mi][ni], 0, 0, 0);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
              acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[mi][j], bf[ni][j], acc[mi][ni], 0, 0, 0);
      }
    };
    auto tap_off = [](int tap) { return (TAPS == 4 ? (tap >> 1) * C::HWD + (tap & 1) : (tap / 3) * C::HWD + (tap % 3)) * CF_LDK; };

    {
      f32x4 rb1[C::BPT];  // all three prologue fetches in flight together: one exposed HBM/L2 latency, not two
      load_A(0, ra);
      load_B(0, rb);
      load_B(1 < nsteps ? 1 : 0, rb1);
      store_A(0, ra, 0);
      store_B(0, rb);
      store_B(1, rb1);
    }
    __syncthreads();
    f32x4 ax[MI], bx[NI], ay[MI], by[NI];
    read_frags(ax, bx, tap_off(0), 0, 0);
    int slot = 0;  // ring slot of the current step's weight slab
    int step = 0;
    for (int chunk = 0; chunk < a.nchunks; ++chunk) {
#pragma unroll
      for (int tap = 0; tap < TAPS; ++tap, ++step) {
        const int slot1 = slot == 2 ? 0 : slot + 1;
        const int slot2 = slot1 == 2 ? 0 : slot1 + 1;
        constexpr int NM = LP ? MI * NI : MI * NI * 4;                      // MFMAs per half step
        constexpr int NA = C::APT * AV;                                     // halo-patch fetches riding in one step
        constexpr bool WEAVE = !LP && NM >= MI + NI + C::BPT + NA;
        // ---- first half: fetch slab s+2 (and, once per slab, the next halo patch), read frags(s, k 8..15), MFMA on frags(s, k 0..7)
        load_B(step + 2 < nsteps ? step + 2 : nsteps - 1, rb);  // clamped: the tail prefetches are harmless re-reads
        if (tap == 0) load_A(chunk + 1 < a.nchunks ? chunk + 1 : chunk, ra);
        read_frags(ay, by, tap_off(tap), slot, 1);
        if (!WEAVE) __builtin_amdgcn_sched_barrier(0);  // pin the fetches above the MFMA block (hipcc would sink them)
        mma16(ax, bx);
        if (WEAVE) {
          // MFMA-first weave: frags(s, k 0..7) are already in registers, so the block opens with an MFMA right behind the
          // barrier and every fetch / LDS read issues in the shadow of a 64-cycle MFMA instead of in front of the block.
#pragma unroll
          for (int i = 0; i < MI + NI; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // MFMA
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // DS read
          }
#pragma unroll
          for (int i = 0; i < C::BPT + (tap == 0 ? NA : 0); ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);  // VMEM read
          }
#pragma unroll
          for (int i = 0; i < NM - (MI + NI) - C::BPT - (tap == 0 ? NA : 0); ++i)
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        // ---- second half: read frags(s+1, k 0..7), MFMA on frags(s, k 8..15), LDS write of slab s+2
        if (tap != TAPS - 1) read_frags(ax, bx, tap_off(tap + 1), slot1, 0);
        if (!WEAVE) __builtin_amdgcn_sched_barrier(0);
        mma16(ay, by);
        if (!WEAVE) __builtin_amdgcn_sched_barrier(0);
        store_B(slot2, rb);
        if (WEAVE) {
#pragma unroll
          for (int i = 0; i < (tap != TAPS - 1 ? MI + NI : 0); ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
          }
#pragma unroll
          for (int i = 0; i < NM - (tap != TAPS - 1 ? MI + NI : 0) - C::BPT; ++i)
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
#pragma unroll
          for (int i = 0; i < C::BPT; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);  // DS write (waits for the slab fetched in the first half)
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();
        if (tap == TAPS - 1 && chunk + 1 < a.nchunks) {
          store_A(0, ra, chunk + 1);
          __syncthreads();
          read_frags(ax, bx, tap_off(0), slot1, 0);
        }
        slot = slot1;
      }
    }
  } else {
    // ---- 1x1 / Linear: the same ring + weave schedule with BOTH operands in 3-deep LDS rings -----------------------------
    // Slab t (A rows and weight rows) is fetched at the start of step t-2, written to LDS at the end of step t-2 (the
    // GroupNorm-apply prologue of the AttnBlock q|k|v GEMM runs in that write), made visible by the barrier opening step
    // t-1 and first read in the middle of step t-1; ring slot (t+3)%3 is rewritten only after the barrier that follows
    // every wave's last read of slab t.
    auto read_frags1 = [&](f32x4(&af)[MI], f32x4(&bf)[NI], int slot_, int kg) {
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
        af[mi] = *reinterpret_cast<const f32x4*>(As + slot_ * (C::NPIX * CF_LDK) + a_off[mi] + kg * 8);
#pragma unroll
      for (int ni = 0; ni < NI; ++ni)
        bf[ni] = *reinterpret_cast<const f32x4*>(Bs + slot_ * (C::BN * CF_LDK) + b_off[ni] + kg * 8);
    };
    auto mma16 = [&](const f32x4(&af)[MI], const f32x4(&bf)[NI]) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
          for (int ni = 0; ni < NI; ++ni)
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[mi][j], bf[ni][j], acc[mi][ni], 0, 0, 0);
    };
    int n = a.nchunks, kb = 0;  // this workgroup's K slabs: [kb, kb + n)
    [[maybe_unused]] f32x16 tot[MI][NI];  // SK: ordered sum of the finished virtual chunks (nsplit == 1)
    if constexpr (SK) {
      const int per = (a.nchunks / CF_SK_SLABS / a.nsplit) * CF_SK_SLABS;  // slabs of this workgroup: whole virtual chunks (host-checked)
      kb = split * per;
      n = per;
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
          for (int r = 0; r < 16; ++r) tot[mi][ni][r] = 0.f;
    }
    {
      f32x4 ra1[C::APT * AV];
      f32x4 rb1[C::BPT];
      load_A(kb, ra);
      load_B(kb, rb);
      load_A(kb + (1 < n ? 1 : 0), ra1);
      load_B(kb + (1 < n ? 1 : 0), rb1);
      store_A(0, ra, kb);
      store_B(0, rb);
      store_A(1, ra1, kb + (1 < n ? 1 : 0));
      store_B(1, rb1);
    }
    __syncthreads();
    f32x4 ax[MI], bx[NI], ay[MI], by[NI];
    read_frags1(ax, bx, 0, 0);
    int slot = 0;
    for (int chunk = 0; chunk < n; ++chunk) {
      const int slot1 = slot == 2 ? 0 : slot + 1;
      const int slot2 = slot1 == 2 ? 0 : slot1 + 1;
      const int nxt = kb + (chunk + 2 < n ? chunk + 2 : n - 1);  // clamped: the tail prefetches are harmless re-reads
      constexpr int NM = MI * NI * 4;
      constexpr bool WEAVE = NM >= MI + NI + C::BPT + C::APT * AV;
      load_B(nxt, rb);
      load_A(nxt, ra);
      read_frags1(ay, by, slot, 1);
      if (!WEAVE) __builtin_amdgcn_sched_barrier(0);
      mma16(ax, bx);
      if (WEAVE) {
#pragma unroll
        for (int i = 0; i < MI + NI; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
#pragma unroll
        for (int i = 0; i < C::BPT + C::APT * AV; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        }
#pragma unroll
        for (int i = 0; i < NM - (MI + NI) - C::BPT - C::APT * AV; ++i) __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
      read_frags1(ax, bx, slot1, 0);  // slab chunk+1 (on the last step: a harmless read of the clamped duplicate)
      mma16(ay, by);
      if (WEAVE) {
#pragma unroll
        for (int i = 0; i < MI + NI; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
#pragma unroll
        for (int i = 0; i < NM - (MI + NI); ++i) __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
      store_A(slot2, ra, nxt);
      store_B(slot2, rb);
      if constexpr (SK) {
        if ((chunk + 1) % CF_SK_SLABS == 0) {  // a virtual chunk is complete: fold it (one workgroup per tile) or park it (split)
          if (a.nsplit == 1) {
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
#pragma unroll
              for (int ni = 0; ni < NI; ++ni) {
                tot[mi][ni] += acc[mi][ni];
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;
              }
          } else {
            f32x4 v[MI * NI * 4];
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
#pragma unroll
              for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                  v[(mi * NI + ni) * 4 + q] = f32x4{acc[mi][ni][q * 4], acc[mi][ni][q * 4 + 1], acc[mi][ni][q * 4 + 2], acc[mi][ni][q * 4 + 3]};
#pragma unroll
                  for (int e = 0; e < 4; ++e) acc[mi][ni][q * 4 + e] = 0.f;
                }
            cf_splitk_park(v, a.ws, sk_tile, (kb + chunk) / CF_SK_SLABS, a.nchunks / CF_SK_SLABS, 256);
          }
        }
      }
      __syncthreads();
      slot = slot1;
    }
    // (the loop's closing barrier retired every LDS read before any wave reuses LDS in its epilogue)
    if constexpr (SK) {
      if (a.nsplit == 1) {
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
          for (int ni = 0; ni < NI; ++ni) acc[mi][ni] = tot[mi][ni];
      }
    }
  }

  if constexpr (SK) {
    if (a.nsplit > 1) {
      f32x4 v[MI * NI * 4];
      if (!cf_splitk_finish(v, a.ws, a.counters, sk_tile, a.nchunks / CF_SK_SLABS, a.nsplit, 256, smem)) return;
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
          for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[mi][ni][q * 4 + e] = v[(mi * NI + ni) * 4 + q][e];
      __syncthreads();  // the flag word lives in the LDS region the epilogue stages through
    }
  }

  // ---- epilogue ------------------------------------------------------------------------------------------
  // The accumulator layout (lane = one output channel, 16 rows per register file) would need 64 scalar stores
  // (+64 residual loads) per lane and the store tail is ISSUE-bound.  Instead each wave transposes its tile through
  // LDS (free after the main loop) 32 rows at a time and touches HBM with 16-byte accesses: lane -> 4 consecutive
  // channels of one pixel; bias / residual / SFT / GELU and the GroupNorm statistics are applied in that layout.
  constexpr int LDW = NI * 32 + 4;       // padded row of the per-wave transpose buffer
  constexpr int Q = NI * 8;              // float4 per tile row
  constexpr int RPP = 64 / Q;            // rows per pass
  constexpr int PASSES = 32 / RPP;
  const bool vec_ok = !(TAPS == 9 && a.out_nchw) && (a.cout % 4) == 0;

  auto epilogue_vec = [&](auto mode) {
    constexpr int EPI = decltype(mode)::value;
    float* stage = smem + wave * (32 * LDW);
    const int cq = lane % Q, rl = lane / Q;
    const int n = n0 + wn * (NI * 32) + cq * 4;
    const bool nvalid = n < a.cout;
    f32x4 bias4 = {0.f, 0.f, 0.f, 0.f};
    if (a.bias && nvalid) bias4 = *reinterpret_cast<const f32x4*>(a.bias + n);
    float ssum[4] = {0.f, 0.f, 0.f, 0.f}, ssq[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      size_t offs[PASSES];
      [[maybe_unused]] unsigned inside = 0;  // EXT: bit p = pass p's pixel lies inside the image (edge tiles)
#pragma unroll
      for (int p = 0; p < PASSES; ++p) {
        const int row = wm * (MI * 32) + mi * 32 + p * RPP + rl;
        size_t pixel;
        if (TAPS == 4)
          pixel = ((size_t)b * a.hout + (2 * (y0 + (row >> 4)) + sub_y)) * a.wout + (2 * (x0 + (row & 15)) + sub_x);
        else if (TAPS == 9)
          pixel = ((size_t)b * a.hout + (y0 + (row >> 4))) * a.wout + (x0 + (row & 15));
        else
          pixel = (size_t)m0 + row;
        offs[p] = pixel * ext_ld<EXT, SK>(a, 2, a.cout) + n;
        if constexpr (EXT) {
          const int oy = TAPS == 4 ? 2 * (y0 + (row >> 4)) + sub_y : y0 + (row >> 4);
          const int ox = TAPS == 4 ? 2 * (x0 + (row & 15)) + sub_x : x0 + (row & 15);
          if (oy < a.hout && ox < a.wout) inside |= 1u << p;
        }
      }
#define CF_LIVE(p) (nvalid && (!EXT || ((inside >> (p)) & 1u)))
      // Residual / SFT operands are requested BEFORE the transpose so their HBM latency overlaps it.  The transpose
      // buffer is private to the wave (LDS operations of one wave complete in issue order), so no workgroup barrier is
      // needed: the main loop's closing barrier already retired every read of this LDS region.
      f32x4 r0[PASSES], r1[PASSES];
#pragma unroll
      for (int p = 0; p < PASSES; ++p) {
        r0[p] = r1[p] = f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (BIO) {
          if (CF_LIVE(p) && (EPI == CF_EPI_RESIDUAL || EPI == CF_EPI_SFT)) r0[p] = cf_load4_bf16(a.res, offs[p]);
          if (CF_LIVE(p) && EPI == CF_EPI_SFT) r1[p] = cf_load4_bf16(a.sft_scale, offs[p]);
        } else {
        if (CF_LIVE(p) && (EPI == CF_EPI_RESIDUAL || EPI == CF_EPI_SFT || EPI == CF_EPI_AXPY || EPI == CF_EPI_AXPY2 || EPI == CF_EPI_RES_PRELU))
          r0[p] = *reinterpret_cast<const f32x4*>(a.res + offs[p]);
        if (CF_LIVE(p) && (EPI == CF_EPI_SFT || EPI == CF_EPI_AXPY2)) r1[p] = *reinterpret_cast<const f32x4*>(a.sft_scale + offs[p]);
        }
      }
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int ni = 0; ni < NI; ++ni)
#pragma unroll
        for (int r = 0; r < 16; ++r) stage[cf_acc_row(r, lane) * LDW + ni * 32 + l31] = acc[mi][ni][r];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
      for (int p = 0; p < PASSES; ++p) {
        const int trow = p * RPP + rl;
        f32x4 v = *reinterpret_cast<const f32x4*>(stage + trow * LDW + cq * 4);
        const size_t o = offs[p];
        if (CF_LIVE(p)) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] += bias4[e];
          if (EPI == CF_EPI_RESIDUAL) {
            const f32x4 rr = r0[p];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] += rr[e];
          } else if (EPI == CF_EPI_SFT) {
            const f32x4 dec = r0[p], sc = r1[p];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = dec[e] + sft_w * (dec[e] * sc[e] + v[e]);
          } else if (EPI == CF_EPI_GELU) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = 0.5f * v[e] * (1.0f + erff(v[e] * 0.70710678118654752440f));
          } else if (EPI == CF_EPI_LEAKY) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : 0.2f * v[e];
          } else if (EPI == CF_EPI_AXPY || EPI == CF_EPI_AXPY2) {
            // separately rounded multiply and add, the two ATen ops of `x5 * 0.2 + x` (rrdbnet_arch.py:39,62) -- no FMA contraction
            const f32x4 x = r0[p], xx = r1[p];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              v[e] = __fadd_rn(__fmul_rn(v[e], a.sft_w), x[e]);
              if (EPI == CF_EPI_AXPY2) v[e] = __fadd_rn(__fmul_rn(v[e], a.sft_w), xx[e]);
            }
          } else if (EPI == CF_EPI_PRELU || EPI == CF_EPI_RES_PRELU) {
            // nn.PReLU with one learned slope of any sign or size (arcface_arch.py:73,87,98): a select, never max(x, a * x)
            const f32x4 rr = r0[p];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float t = EPI == CF_EPI_RES_PRELU ? __fadd_rn(v[e], rr[e]) : v[e];
              v[e] = t > 0.f ? t : __fmul_rn(a.sft_w, t);
            }
          }
          if constexpr (BIO) cf_store4_bf16(a.out, o, v);   // (rounded here, once; the statistics below see the fp32 values)
          else *reinterpret_cast<f32x4*>(a.out + o) = v;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            ssum[e] += v[e];
            ssq[e] += v[e] * v[e];
          }
        }
      }
    }
    if (!EXT && a.stats_out) {
      // GroupNorm statistics of the values just written, for the NEXT norm: cf_gn_partials<CF_GN_PAIR> (cf_conv_parts.h) written out, one
      // partial per (image, group, tile, wave row).  This epilogue keeps its own text (edge-tile mask, dense-block epilogues): with
      // the shared quad helpers most instantiations compiled to other code.
      const int cpg = a.stats_cpg;
      double d0, q0, d1 = 0, q1 = 0;
      if (cpg == 2) {  // two groups per lane
        d0 = (double)ssum[0] + ssum[1];
        q0 = (double)ssq[0] + ssq[1];
        d1 = (double)ssum[2] + ssum[3];
        q1 = (double)ssq[2] + ssq[3];
      } else {
        d0 = ((double)ssum[0] + ssum[1]) + ((double)ssum[2] + ssum[3]);
        q0 = ((double)ssq[0] + ssq[1]) + ((double)ssq[2] + ssq[3]);
      }
      for (int o = Q; o < 64; o <<= 1) {  // lanes holding the same channels, different rows
        d0 += __shfl_xor(d0, o, 64);
        q0 += __shfl_xor(q0, o, 64);
        d1 += __shfl_xor(d1, o, 64);
        q1 += __shfl_xor(q1, o, 64);
      }
      for (int o = 1; o * 4 < cpg; o <<= 1) {  // adjacent channel quads of one group (cpg >= 8)
        d0 += __shfl_xor(d0, o, 64);
        q0 += __shfl_xor(q0, o, 64);
      }
      if (rl == 0 && nvalid && (n % cpg) == 0) {
        const int tile_in_img = (TAPS > 1) ? (mt - b * a.tiles_per_img) : (m0 - b * (a.hout * a.wout)) / C::BM;
        const size_t pidx = (size_t)tile_in_img * WM + wm;
        double* o = cf_gn_partial_ptr(a.stats_out, b, a.cout, cpg, n, a.nparts, pidx);
        o[0] = d0;
        o[1] = q0;
        if (cpg == 2) {
          o[(size_t)a.nparts * 2] = d1;      // group n/2 + 1
          o[(size_t)a.nparts * 2 + 1] = q1;
        }
      }
    }
  };

#undef CF_LIVE
  // scalar path: NCHW scatter of the 3-channel image (and any cout that is not a multiple of 4)
  auto epilogue_scalar = [&](auto mode) {
    constexpr int EPI = decltype(mode)::value;
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
      const int n = n0 + wn * (NI * 32) + ni * 32 + l31;
      const bool nvalid = n < a.cout;
      const float bias = (a.bias && nvalid) ? a.bias[n] : 0.f;
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = wm * (MI * 32) + mi * 32 + cf_acc_row(r, lane);
          size_t pixel;
          int oy = 0, ox = 0;
          if (TAPS == 9) {
            oy = y0 + (row >> 4);
            ox = x0 + (row & 15);
            pixel = ((size_t)b * a.hout + oy) * a.wout + ox;
          } else {
            pixel = (size_t)m0 + row;
          }
          const size_t o = pixel * a.cout + n;
          float v = acc[mi][ni][r] + bias;
          if (nvalid) {
            if (EPI == CF_EPI_RESIDUAL) {
              v += a.res[o];
            } else if (EPI == CF_EPI_SFT) {
              const float dec = a.res[o];
              v = dec + sft_w * (dec * a.sft_scale[o] + v);
            } else if (EPI == CF_EPI_GELU) {
              v = 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f));
            }
            if (TAPS == 9 && a.out_nchw)
              a.out[(((size_t)b * a.cout + n) * a.hout + oy) * a.wout + ox] = v;
            else
              a.out[o] = v;
          }
        }
      }
    }
  };
  if constexpr (PRELU) {  // host guarantees one of the two codes, NHWC output with cout % 4 == 0
    if (a.epilogue == CF_EPI_RES_PRELU) epilogue_vec(std::integral_constant<int, CF_EPI_RES_PRELU>{});
    else epilogue_vec(std::integral_constant<int, CF_EPI_PRELU>{});
  } else if constexpr (EXT) {  // host guarantees NHWC output with cout % 4 == 0
    switch (a.epilogue) {
      case CF_EPI_RESIDUAL: epilogue_vec(std::integral_constant<int, CF_EPI_RESIDUAL>{}); break;
      case CF_EPI_LEAKY: epilogue_vec(std::integral_constant<int, CF_EPI_LEAKY>{}); break;
      case CF_EPI_AXPY: epilogue_vec(std::integral_constant<int, CF_EPI_AXPY>{}); break;
      case CF_EPI_AXPY2: epilogue_vec(std::integral_constant<int, CF_EPI_AXPY2>{}); break;
      default: epilogue_vec(std::integral_constant<int, CF_EPI_NONE>{}); break;
    }
  } else if (vec_ok) {
    switch (a.epilogue) {
      case CF_EPI_RESIDUAL: epilogue_vec(std::integral_constant<int, CF_EPI_RESIDUAL>{}); break;
      case CF_EPI_SFT: epilogue_vec(std::integral_constant<int, CF_EPI_SFT>{}); break;
      case CF_EPI_GELU: epilogue_vec(std::integral_constant<int, CF_EPI_GELU>{}); break;
      default: epilogue_vec(std::integral_constant<int, CF_EPI_NONE>{}); break;
    }
  } else {
    epilogue_scalar(std::integral_constant<int, CF_EPI_NONE>{});  // host guarantees: no epilogue op, no statistics
  }
}

// ---- 3x3 convolution with <= 4 output channels written NCHW (the network's last conv, 64 -> 3 @ 512x512) -----------
// A 3-wide N would waste 29/32 of every MFMA tile (the MFMA instantiation spends 1.24 ms per 16 faces on padding), and the
// layer is HBM-bound anyway (reads 64 channels, writes 3): one thread per output pixel on the vector ALU, the same LDS
// halo patch + prologue as the MFMA kernel, weights fetched through the scalar cache (wave-uniform addresses), coalesced
// per-plane NCHW stores.  Accumulation order: slab, tap, channel (a plain fp32 FMA chain).
// NCO = output channels evaluated per pixel (3 for the RGB head: the zero padding row of the packed weight is not multiplied through)
// U8 (cf_conv2d_u8, NCO = 3): the output is the uint8 HWC BGR image -- byte 2 - co of a pixel is cf_to_u8(acc[co] + bias[co]), what
// cf_tensor_to_img_u8 makes of the NCHW planes.  A thread owns one pixel = three bytes: the tile's bytes go through `As` (free after the
// K loop's last barrier; no LDS is added -- `As` sets the six resident workgroups per CU) as one 24-bit word per pixel, and 192 threads
// write the sixteen 48-byte row segments as dwords.  `a.out` carries the image's address (the descriptor keeps float* fields).
template <int NCO, bool BIO = false, bool U8 = false>   // BIO: the input is a bf16 tensor (cf_conv_desc.io_bf16; the NCHW image stays fp32)
// (waves per SIMD: with the U8 epilogue the fp32-tensor instantiation needs 97 registers, one more than five waves allow; asked for five it
// keeps 96 and holds two values in scratch around the K loop -- one store before it, one load after.  DESIGN.md section 7 has both builds'
// timings.  1 is the default request: the instantiations without U8 are instruction for instruction what they were without the attribute.)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(U8 ? 5 : 1))) void conv3x3_few_cout_kernel(const ConvArgsExt a) {
  static_assert(!U8 || NCO == 3, "the uint8 image has three channels");
  constexpr int TH = 16, TW = 16, HWD = TW + 2, NPIX = (TH + 2) * HWD, APT = (NPIX * 4 + 255) / 256;
  __shared__ __attribute__((aligned(16))) float As[NPIX * CF_LDK];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / a.tiles_per_img;
  const int r = blockIdx.x - b * a.tiles_per_img;
  const int ty = r / a.tiles_x;
  const int y0 = ty * TH, x0 = (r - ty * a.tiles_x) * TW;
  const int k4 = tid & 3;
  int pix[APT];
#pragma unroll
  for (int j = 0; j < APT; ++j) {
    const int p = (tid >> 2) + 64 * j;
    int v = -1;
    if (p < NPIX) {
      const int hy = p / HWD, hx = p - hy * HWD;
      int iy = y0 - 1 + hy, ix = x0 - 1 + hx;
      if (a.pad_mode != CF_PAD_ZERO) {
        iy = cf_border(iy, a.hin, a.pad_mode);
        ix = cf_border(ix, a.win, a.pad_mode);
      }
      if (iy >= 0 && iy < a.hin && ix >= 0 && ix < a.win) v = (b * a.hin + iy) * a.win + ix;
    }
    pix[j] = v;
  }
  const int py = tid >> 4, px = tid & 15;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  const bool affine = a.prologue == CF_PRO_AFFINE || a.prologue == CF_PRO_AFFINE_SWISH;
  // Two 16-channel slabs per gather (round 5).  The slab of a pixel is 64 bytes -- half a 128-byte line -- and with one slab per pass the
  // other half was requested a whole tap loop later, when the line had left the L2 (counters: 2.2x the tensor's bytes from HBM); and the
  // loads sat under the per-item validity branch, so each was waited for before the next was issued.  Now both halves of a line are
  // requested together, unconditionally from clamped addresses (out-of-image items are zeroed at the store), the second slab waits in
  // registers while the first is multiplied: the LDS footprint -- what sets the six resident workgroups per CU -- is unchanged, and so is
  // the accumulation order (slab, tap, channel): bitwise the same output.
  for (int chunk = 0; chunk < a.nchunks; chunk += 2) {
    const bool two = chunk + 1 < a.nchunks;
    f32x4 raw[2][APT], sc[2], sh[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int c = (two || u == 0 ? chunk + u : chunk) * CF_BK + k4 * 4;
      sc[u] = f32x4{1.f, 1.f, 1.f, 1.f};
      sh[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (affine) {
        sc[u] = *reinterpret_cast<const f32x4*>(a.pro_scale + (size_t)b * a.cin + c);
        sh[u] = *reinterpret_cast<const f32x4*>(a.pro_shift + (size_t)b * a.cin + c);
      }
#pragma unroll
      for (int j = 0; j < APT; ++j) {
        const size_t pj = pix[j] < 0 ? (size_t)b * a.hin * a.win : (size_t)pix[j];   // (clamped: any pixel of this image)
        if constexpr (BIO) raw[u][j] = cf_load4_bf16(a.in0, pj * a.c0 + c);
        else raw[u][j] = *reinterpret_cast<const f32x4*>(a.in0 + pj * a.c0 + c);
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (u == 1 && !two) break;
#pragma unroll
      for (int j = 0; j < APT; ++j) {
        const int p = (tid >> 2) + 64 * j;
        if (p < NPIX) {
          f32x4 v = raw[u][j];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float y = v[e] * sc[u][e] + sh[u][e];
            if (a.prologue == CF_PRO_AFFINE_SWISH) y = swishf(y);
            if (a.prologue == CF_PRO_LEAKY) y = v[e] > 0.f ? v[e] : 0.2f * v[e];
            v[e] = pix[j] >= 0 ? y : 0.f;
          }
          *reinterpret_cast<f32x4*>(As + p * CF_LDK + k4 * 4) = v;
        }
      }
      __syncthreads();
#pragma unroll 1  // one tap's 64 weights fit the scalar registers; unrolling all nine spills them
      for (int tap = 0; tap < 9; ++tap) {
        const float* ap = As + ((py + tap / 3) * HWD + px + tap % 3) * CF_LDK;
        const float* wp = a.weight + (size_t)(tap * a.nchunks + chunk + u) * a.cout_pad * CF_BK;  // [cout_pad][16], wave-uniform
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4 av = *reinterpret_cast<const f32x4*>(ap + q * 4);
#pragma unroll
          for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int co = 0; co < NCO; ++co)  // (NCO = 4: rows >= cout of the packed weight are zero padding, no branch needed)
              acc[co] = fmaf(av[e], wp[co * CF_BK + q * 4 + e], acc[co]);
        }
      }
      __syncthreads();
    }
  }
  if constexpr (U8) {
    uint32_t* words = reinterpret_cast<uint32_t*>(As);   // [16 x 16 pixels]: B | G << 8 | R << 16
    uint32_t w = 0;
#pragma unroll
    for (int co = 0; co < 3; ++co) w |= cf_to_u8(acc[co] + (a.bias ? a.bias[co] : 0.f)) << (8 * (2 - co));
    words[tid] = w;
    __syncthreads();
    if (tid < 16 * 12) {   // dword d of tile row `row`: bytes 4 d .. 4 d + 3 of its 48, from the pixels (4 d) / 3 and the next one
      const int row = tid / 12, d = tid - row * 12, p = (4 * d) / 3, off = 4 * d - 3 * p;
      const int nb = (a.wout - x0 < TW ? a.wout - x0 : TW) * 3 - 4 * d;   // bytes of this dword inside the image row
      if (y0 + row < a.hout && nb > 0) {
        const uint32_t v = (words[row * TW + p] >> (8 * off)) | (words[row * TW + p + 1] << (24 - 8 * off));   // (d = 11: p + 1 = 15)
        uint8_t* g = reinterpret_cast<uint8_t*>(a.out) + (((size_t)b * a.hout + (y0 + row)) * a.wout + x0) * 3 + 4 * d;
        // a row starts on the 4-byte grid only where (image base + row * wout * 3) % 4 == 0: elsewhere, and on a dword the image's right
        // edge cuts, byte stores (as cf_tensor_to_img_u8 does for h * w % 4 != 0)
        if (nb >= 4 && (reinterpret_cast<uintptr_t>(g) & 3) == 0) {
          *reinterpret_cast<uint32_t*>(g) = v;
        } else {
          for (int k = 0; k < 4 && k < nb; ++k) g[k] = (uint8_t)(v >> (8 * k));
        }
      }
    }
  } else {
    const int oy = y0 + py, ox = x0 + px;
#pragma unroll
    for (int co = 0; co < 4; ++co)
      if (co < a.cout && oy < a.hout && ox < a.wout)
        a.out[(((size_t)b * a.cout + co) * a.hout + oy) * a.wout + ox] = acc[co] + (a.bias ? a.bias[co] : 0.f);
  }
}

// ---- 3x3 convolution of an NCHW input with <= 4 channels into 64 NHWC channels (the network's first conv, vqgan_arch.py:243) --------
// K = 27: on MFMA the layer pads K to 16 per tap and still moves 1.07 GB of output per 16 faces -- it is write-bound (AI = 13 FLOP/B),
// and the MFMA instantiation reached 1.0 TB/s.  Here a workgroup owns a 16x16 pixel tile: input patch (<= 4 x 18 x 18) and the 27 x 64
// weights sit in LDS, a thread computes FOUR channels of one pixel on the vector ALU (exact fp32 FMA chain: channel-major, then
// taps), and the 16 lanes that share a pixel store its 256 contiguous bytes.  GroupNorm partials as in the MFMA epilogue
// (fp64, fixed shuffle order): one per (image, group, tile, wave).
// C0 = the input channel count when it is known at compile time (3: the network input), 0 = any count <= 4 at run time.  With C0 known
// the thread keeps the 27 float4 weight rows of ITS channel quad in registers for all sixteen pixels it computes: the LDS-resident
// weights cost one ds_read_b128 per tap and pixel, 3456 LDS wave-instructions per tile = 0.31 of the kernel's 0.39 ms per 16 faces.
// The FMA chain (channel-major, then taps) and with it every bit of the output is unchanged.
// U8 (cf_conv2d_u8, C0 = 3): the input is the uint8 HWC BGR image, `a.in0` carries its address.  Only the fill of s_in differs: channel c
// (0 = R) of a pixel is cf_from_u8 of its byte 2 - c, through a 256-entry LDS table as in cf_img_u8_to_tensor -- the values that kernel
// would have written as fp32 NCHW, so output and statistics partials are bitwise those of the two launches.  Halo pixels outside the
// image are 0.f, not cf_from_u8(0).
template <int C0, bool NT = false, bool U8 = false>   // NT: non-temporal output stores (cf_common.h: cf_store16; a compile-time choice here -- sixteen stores per thread)
__global__ __launch_bounds__(256) void conv3x3_few_cin_kernel(const ConvArgsExt a) {
  static_assert(!U8 || C0 == 3, "the uint8 image has three channels");
  __shared__ float s_in[4][18 * 18];
  __shared__ __attribute__((aligned(16))) float s_w[36][64];  // [tap * 4 + c][n]
  const int tid = threadIdx.x;
  const int b = blockIdx.x / a.tiles_per_img;
  const int r = blockIdx.x - b * a.tiles_per_img;
  const int ty0 = r / a.tiles_x;
  const int y0 = ty0 * 16, x0 = (r - ty0 * a.tiles_x) * 16;
  const int quad = tid & 15, slot = tid >> 4;
  const int n = quad * 4;
  for (int i = tid; i < 36 * 64; i += 256) {
    const int nn = i & 63, tc = i >> 6, tap = tc >> 2, c = tc & 3;
    (&s_w[0][0])[i] = (c < a.c0 && nn < a.cout) ? a.weight[((size_t)tap * a.cout_pad + nn) * CF_BK + c] : 0.f;  // [tap][1 slab][cout_pad][16]
  }
  if constexpr (U8) {
    __shared__ float lut[256];
    lut[tid] = cf_from_u8(tid);
    __syncthreads();
    const uint8_t* img = reinterpret_cast<const uint8_t*>(a.in0);
    for (int i = tid; i < 18 * 18 * 3; i += 256) {   // the patch's bytes in image order: 18 row segments of 54 contiguous bytes
      const int hy = i / 54, j = i - hy * 54, hx = j / 3, k = j - hx * 3;
      const int iy = y0 - 1 + hy, ix = x0 - 1 + hx;
      float v = 0.f;
      if (iy >= 0 && iy < a.hin && ix >= 0 && ix < a.win) v = lut[img[(((size_t)b * a.hin + iy) * a.win + ix) * 3 + k]];
      s_in[2 - k][hy * 18 + hx] = v;   // (s_in[3] is never read with C0 = 3)
    }
  } else {
    const size_t plane = (size_t)a.hin * a.win;
    for (int i = tid; i < 4 * 18 * 18; i += 256) {
      const int c = i / (18 * 18), p = i - c * (18 * 18), hy = p / 18, hx = p - hy * 18;
      const int iy = y0 - 1 + hy, ix = x0 - 1 + hx;
      float v = 0.f;
      if (c < a.c0 && iy >= 0 && iy < a.hin && ix >= 0 && ix < a.win) v = a.in0[((size_t)b * a.c0 + c) * plane + (size_t)iy * a.win + ix];
      s_in[c][p] = v;
    }
  }
  __syncthreads();
  f32x4 wreg[C0 > 0 ? C0 * 9 : 1];
  if constexpr (C0 > 0) {  // this thread's 27 weight rows: read from LDS once, kept for its sixteen pixels
#pragma unroll
    for (int c = 0; c < C0; ++c)
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) wreg[c * 9 + tap] = *reinterpret_cast<const f32x4*>(&s_w[tap * 4 + c][n]);
  }
  f32x4 bias4 = {0.f, 0.f, 0.f, 0.f};
  if (a.bias) bias4 = *reinterpret_cast<const f32x4*>(a.bias + n);
  float ssum[4] = {0.f, 0.f, 0.f, 0.f}, ssq[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int round = 0; round < 16; ++round) {
    const int p = round * 16 + slot, py = p >> 4, px = p & 15;
    f32x4 acc = bias4;
    if constexpr (C0 > 0) {
#pragma unroll
      for (int c = 0; c < C0; ++c) {
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
          const float v = s_in[c][(py + tap / 3) * 18 + px + tap % 3];
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[e] = fmaf(v, wreg[c * 9 + tap][e], acc[e]);
        }
      }
    } else {
      for (int c = 0; c < a.c0; ++c) {
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
          const float v = s_in[c][(py + tap / 3) * 18 + px + tap % 3];
          const f32x4 w4 = *reinterpret_cast<const f32x4*>(&s_w[tap * 4 + c][n]);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[e] = fmaf(v, w4[e], acc[e]);
        }
      }
    }
    cf_store16(a.out + (((size_t)b * a.hout + (y0 + py)) * a.wout + (x0 + px)) * a.cout + n, acc, NT);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      ssum[e] += acc[e];
      ssq[e] += acc[e] * acc[e];
    }
  }
  if (a.stats_out) {  // cout = 64 -> 2 channels per group: a lane's four channels are two groups
    double d0 = (double)ssum[0] + ssum[1], q0 = (double)ssq[0] + ssq[1];
    double d1 = (double)ssum[2] + ssum[3], q1 = (double)ssq[2] + ssq[3];
    for (int o = 16; o < 64; o <<= 1) {  // the four pixel slots of the wave that share this channel quad
      d0 += __shfl_xor(d0, o, 64);
      q0 += __shfl_xor(q0, o, 64);
      d1 += __shfl_xor(d1, o, 64);
      q1 += __shfl_xor(q1, o, 64);
    }
    if ((tid & 63) < 16) {
      const size_t pidx = (size_t)r * 4 + (tid >> 6);
      double* o = a.stats_out + (((size_t)b * 32 + quad * 2) * a.nparts + pidx) * 2;
      o[0] = d0;
      o[1] = q0;
      o[(size_t)a.nparts * 2] = d1;
      o[(size_t)a.nparts * 2 + 1] = q1;
    }
  }
}

// 1x1 / Linear rows in tiles of `bm`: whole tiles, none across two images.  The tile count, or 0 with the error set.
int conv1x1_mtiles(const ConvArgsExt& a, int bm) {
  const long m = (long)a.batch * a.hout * a.wout;
  if (m % bm == 0 && (a.hout * a.wout) % bm == 0) return (int)(m / bm);
  cf_set_error("cf_conv2d: 1x1 rows %ld (per image %d) not divisible by %d", m, a.hout * a.wout, bm);
  return 0;
}

template <int TAPS, int STRIDE, int WM, int WN, int MI, int NI, bool IN_NCHW, bool BF16 = false, bool EXT = false, bool F16 = false, bool BIO = false, bool PRELU = false>
int launch(const ConvArgsExt& a, hipStream_t stream, int* parts_query) {
  using C = Cfg<TAPS, STRIDE, WM, WN, MI, NI>;
  ArgsOf<EXT> k = a;  // (slices the stride fields off for the CodeFormer instantiations)
  int mtiles;
  if (TAPS == 1) {
    k.tiles_x = k.tiles_per_img = 0;
    mtiles = conv1x1_mtiles(a, C::BM);
    if (!mtiles) return CF_ERR_ARG;
  } else {  // the folded upsample's tiles live on the SOURCE grid; each is computed once per output parity class
    const int gh = TAPS == 4 ? a.hin : a.hout, gw = TAPS == 4 ? a.win : a.wout;
    if (!EXT && (gh % C::TH != 0 || gw % C::TW != 0)) {  // (EXT: any image size, the grid is ceil-divided and edge tiles are masked)
      cf_set_error(TAPS == 4 ? "cf_conv2d: %dx%d upsample source not divisible by the %dx%d tile"
                             : "cf_conv2d: %dx%d output not divisible by the %dx%d tile", gh, gw, C::TH, C::TW);
      return CF_ERR_ARG;
    }
    k.tiles_x = (gw + C::TW - 1) / C::TW;
    k.tiles_per_img = (TAPS == 4 ? 4 : 1) * k.tiles_x * ((gh + C::TH - 1) / C::TH);
    mtiles = k.tiles_per_img * a.batch;
  }
  k.nparts = (mtiles / a.batch) * WM;  // statistics partials per (image, group): tiles per image x wave rows
  if (parts_query) {
    *parts_query = k.nparts;
    return CF_OK;
  }
  k.ntn = a.cout_pad / C::BN;
  constexpr auto kern = igemm_kernel<TAPS, STRIDE, WM, WN, MI, NI, IN_NCHW, BF16, EXT, F16, false, BIO, PRELU>;
  constexpr size_t lds = C::LDS_FLOATS * sizeof(float);
  CF_LDS_ATTR(kern, lds);  // (cf_device_init sets the dynamic-LDS attribute on each device)
  hipLaunchKernelGGL(kern, dim3(mtiles * k.ntn), dim3(256), lds, stream, k);
  CF_CHECK_LAUNCH("cf_conv2d");
  return CF_OK;
}

// 1x1 / Linear with split-K (small token matrices): 64x64 tiles, `nsplit` workgroups per tile.
template <int WM, int WN, int MI, int NI>
int launch_sk(const ConvArgsExt& a, float* ws, unsigned* counters, int nsplit, hipStream_t stream, int* parts_query) {
  using C = Cfg<1, 1, WM, WN, MI, NI>;
  ConvArgsSK k;
  static_cast<ConvArgs&>(k) = a;
  const int mtiles = conv1x1_mtiles(a, C::BM);
  if (!mtiles) return CF_ERR_ARG;
  k.tiles_x = k.tiles_per_img = 0;
  k.nparts = (mtiles / a.batch) * WM;
  if (parts_query) {
    *parts_query = k.nparts;
    return CF_OK;
  }
  k.ntn = a.cout_pad / C::BN;
  k.ws = ws;
  k.counters = counters;
  k.nsplit = nsplit;
  constexpr auto kern = igemm_kernel<1, 1, WM, WN, MI, NI, false, false, false, false, true>;
  constexpr size_t lds = C::LDS_FLOATS * sizeof(float);
  CF_LDS_ATTR(kern, lds);
  hipLaunchKernelGGL(kern, dim3(mtiles * k.ntn * nsplit), dim3(256), lds, stream, k);
  CF_CHECK_LAUNCH("cf_conv2d(split-K)");
  return CF_OK;
}

}  // namespace

// What conv_validate derives for the pieces below (ext: the general instantiations, narrow: 64-wide N tiles of a small-M layer).
struct ConvFacts { int ld0, ld1, ldo; bool ext, few_cout, narrow; };

// Every argument check of cf_conv2d; the first failing one decides the error text.  The direct kernels' own come last, each under its route.
static int conv_validate(const cf_conv_desc* d, const int* pq, ConvFacts& f) {
  CF_REQUIRE(d, "cf_conv2d: null descriptor");
  CF_REQUIRE(pq || (d->in0 && d->weight && d->out), "cf_conv2d: null in0/weight/out");
  CF_REQUIRE(d->taps == 1 || d->taps == 9, "cf_conv2d: taps must be 1 or 9 (got %d)", d->taps);
  CF_REQUIRE(d->stride == 1 || (d->stride == 2 && d->taps == 9), "cf_conv2d: unsupported stride %d", d->stride);
  CF_REQUIRE(d->batch > 0 && d->hin > 0 && d->win > 0 && d->cout > 0, "cf_conv2d: bad dims");
  CF_REQUIRE(!(d->upsample && (d->stride != 1 || d->taps != 9 || d->in_nchw || d->out_nchw)),
             "cf_conv2d: upsample needs a 3x3 stride-1 NHWC conv");
  // stride 2 with one padded row / column in front (pad_lo 1, nn.Conv2d(3, 2, 1)) takes any size: (h + 1) / 2 outputs, the last of which
  // reads row h of an odd image -- outside, refused by the gather like every padded pixel.  pad_lo 0 keeps its even sizes.
  const bool s2_sym = d->stride == 2 && d->pad_lo == 1;
  const int exp_h = d->stride == 2 ? (d->hin + (s2_sym ? 1 : 0)) / 2 : (d->hin << (d->upsample ? 1 : 0));
  const int exp_w = d->stride == 2 ? (d->win + (s2_sym ? 1 : 0)) / 2 : (d->win << (d->upsample ? 1 : 0));
  CF_REQUIRE(d->hout == exp_h && d->wout == exp_w, "cf_conv2d: hout/wout %dx%d, expected %dx%d", d->hout, d->wout,
             exp_h, exp_w);
  CF_REQUIRE(d->stride == 1 || s2_sym || (d->hin % 2 == 0 && d->win % 2 == 0), "cf_conv2d: stride 2 with pad_lo 0 needs even input");
  if (d->out_nchw || d->cout % 4 != 0)
    CF_REQUIRE(d->epilogue == CF_EPI_NONE && !d->stats_out, "cf_conv2d: cout %d / NCHW output supports no epilogue op or statistics",
               d->cout);
  if (d->stats_out || (pq && d->stats_cpg)) {
    const int g = d->stats_cpg;
    CF_REQUIRE(g >= 2 && g <= 32 && (g & (g - 1)) == 0 && d->cout % g == 0 && !d->out_nchw,
               "cf_conv2d: stats_cpg %d must be a power of two in [2,32] dividing cout %d (NHWC output)", g, d->cout);
  }
  if (d->in_nchw) {
    CF_REQUIRE(d->c0 >= 1 && d->c0 <= 4 && d->c1 == 0 && d->taps == 9 && d->stride == 1 && !d->upsample,
               "cf_conv2d: in_nchw supports 3x3 s1 with <=4 input channels");
    CF_REQUIRE(d->prologue == CF_PRO_NONE, "cf_conv2d: in_nchw has no prologue");
  } else {
    CF_REQUIRE(d->c0 % CF_BK == 0 && d->c1 % CF_BK == 0 && d->c0 > 0, "cf_conv2d: c0=%d c1=%d must be multiples of 16",
               d->c0, d->c1);
    CF_REQUIRE(d->c1 == 0 || d->in1, "cf_conv2d: c1 > 0 without in1");
  }
  CF_REQUIRE(d->bf16_mfma >= CF_OPERAND_F32 && d->bf16_mfma <= CF_OPERAND_F16X2, "cf_conv2d: bad operand format %d", d->bf16_mfma);
  if (d->bf16_mfma == CF_OPERAND_BF16 || d->bf16_mfma == CF_OPERAND_F16)
    CF_REQUIRE(d->taps == 9 && d->stride == 1 && !d->in_nchw && !d->out_nchw && d->c0 % 32 == 0 && d->c1 % 32 == 0 &&
                   d->cout_pad % (d->bf16_mfma == CF_OPERAND_F16 ? 32 : 64) == 0 && d->cout % 4 == 0,
               "cf_conv2d: bf16_mfma covers 3x3 stride-1 NHWC convs with channels %% 32 == 0 (c0=%d c1=%d cout_pad=%d)", d->c0,
               d->c1, d->cout_pad);
  CF_REQUIRE(d->prologue >= 0 && d->prologue <= 3 && d->epilogue >= 0 && d->epilogue <= CF_EPI_RES_PRELU, "cf_conv2d: bad pro/epilogue");
  if (d->prologue == CF_PRO_AFFINE || d->prologue == CF_PRO_AFFINE_SWISH)
    CF_REQUIRE(d->pro_scale && d->pro_shift, "cf_conv2d: affine prologue without scale/shift tables");
  if (d->epilogue == CF_EPI_RESIDUAL || d->epilogue == CF_EPI_SFT || d->epilogue == CF_EPI_AXPY || d->epilogue == CF_EPI_AXPY2 || d->epilogue == CF_EPI_RES_PRELU)
    CF_REQUIRE(d->res, "cf_conv2d: epilogue needs res");
  if (d->epilogue == CF_EPI_SFT) CF_REQUIRE(d->sft_scale, "cf_conv2d: SFT epilogue needs sft_scale");
  if (d->epilogue == CF_EPI_AXPY2) CF_REQUIRE(d->sft_scale, "cf_conv2d: AXPY2 epilogue needs res2 (sft_scale)");
  // general (EXT) instantiations: strided channel slices, dense-block epilogues, image sizes off the tile grid
  const int ld0 = d->ld_in0 > 0 ? d->ld_in0 : d->c0, ld1 = d->ld_in1 > 0 ? d->ld_in1 : d->c1,
            ldo = d->ld_out > 0 ? d->ld_out : d->cout;
  CF_REQUIRE(d->ld_in0 >= 0 && d->ld_in1 >= 0 && d->ld_out >= 0 && ld0 >= d->c0 && ld1 >= d->c1 && ldo >= d->cout,
             "cf_conv2d: channel strides (%d,%d,%d) smaller than the channel counts (%d,%d,%d)", ld0, ld1, ldo, d->c0, d->c1,
             d->cout);
  const bool few_cout = d->taps == 9 && d->stride == 1 && d->out_nchw && d->cout <= 4 && !d->upsample && d->c1 == 0 && !d->in_nchw;
  CF_REQUIRE(d->pad_mode >= CF_PAD_ZERO && d->pad_mode <= CF_PAD_EDGE && (d->pad_lo == 0 || d->pad_lo == 1),
             "cf_conv2d: bad pad_mode %d / pad_lo %d", d->pad_mode, d->pad_lo);
  CF_REQUIRE(d->pad_mode != CF_PAD_REFLECT || (d->taps == 9 && !d->upsample && d->hin >= 2 && d->win >= 2),
             "cf_conv2d: reflect padding is for plain 3x3 convs on images of at least 2x2");
  CF_REQUIRE(d->pad_mode != CF_PAD_EDGE || d->upsample, "cf_conv2d: edge padding belongs to the folded upsample conv");
  CF_REQUIRE(d->pad_lo == 0 || d->stride == 2, "cf_conv2d: pad_lo applies to stride 2");
  const bool ext = !d->winograd && d->bf16_mfma != CF_OPERAND_F16X2 && (ld0 != d->c0 || ld1 != d->c1 || ldo != d->cout || d->epilogue >= CF_EPI_LEAKY ||
                   ((d->pad_mode != CF_PAD_ZERO || d->pad_lo) && !(d->out_nchw && d->cout <= 4)) ||
                   (d->bf16_mfma == CF_OPERAND_F16 && d->cout_pad % 64 != 0) ||
                   (d->taps == 9 && d->stride == 1 && !d->in_nchw && !few_cout && (d->hout % 16 != 0 || d->wout % 16 != 0)) ||
                   // the folded upsample's dense tiles lie on the SOURCE grid (8 x 16 for 128-wide channel tiles): an 8x8 source gives an
                   // on-grid 16x16 output that only the general instantiation can tile (BiSeNet's conv_head16 on a 128x128 face)
                   (d->upsample && d->bf16_mfma == CF_OPERAND_F32 && d->cout_pad % 128 == 0 && (d->hin % 8 != 0 || d->win % 16 != 0)));
  if (ext) {
    CF_REQUIRE(d->taps == 9 && (d->stride == 1 || (d->bf16_mfma == CF_OPERAND_F32 && d->cout_pad % 128 == 0)) && !d->in_nchw &&
                   !d->out_nchw && d->bf16_mfma != CF_OPERAND_BF16 && !d->stats_out &&
                   !(pq && d->stats_cpg) && d->cout % 4 == 0 && d->epilogue != CF_EPI_SFT && d->epilogue != CF_EPI_GELU,
               "cf_conv2d: strided slices / leaky|axpy epilogues / off-grid sizes (%dx%d) need a 3x3 stride-1 fp32 / f16-operand NHWC conv with "
               "cout %% 4 == 0, no statistics, epilogue in {none, residual, leaky, axpy, axpy2, prelu, res_prelu}", d->hout, d->wout);
    CF_REQUIRE(ld0 % 4 == 0 && ld1 % 4 == 0 && ldo % 4 == 0, "cf_conv2d: channel strides must be multiples of 4 floats");
    CF_REQUIRE(d->epilogue < CF_EPI_PRELU || (d->bf16_mfma == CF_OPERAND_F32 && !d->upsample),
               "cf_conv2d: the PReLU epilogues are built for plain 3x3 convs with fp32 operands (operand %d, upsample %d)", d->bf16_mfma, d->upsample);
  } else {
    CF_REQUIRE(!few_cout || ld0 == d->c0, "cf_conv2d: the NCHW <=4-channel output conv reads a dense input");
    CF_REQUIRE(d->epilogue < CF_EPI_PRELU, "cf_conv2d: the PReLU epilogues belong to the general fp32 / f16-operand 3x3 instantiations (winograd %d, operand %d)",
               d->winograd, d->bf16_mfma);
  }
  CF_REQUIRE(!(d->out_nchw && (d->taps != 9 || d->epilogue != CF_EPI_NONE)), "cf_conv2d: out_nchw needs 3x3, no epilogue");
  CF_REQUIRE(d->cout_pad >= d->cout && d->cout_pad % 32 == 0, "cf_conv2d: cout_pad %d invalid for cout %d", d->cout_pad,
             d->cout);
  CF_REQUIRE(!d->in0_alt || (d->taps == 1 && d->bf16_mfma == CF_OPERAND_F16X2 && (long)d->hout * d->wout <= CF_TOKEN_IMAGE_MAX && !d->io_bf16),
             "cf_conv2d: in0_alt (a second token matrix for the columns >= alt_cout0) belongs to the split-half token GEMM");
  if (d->io_bf16) {   // bf16 tensors (ABI v22): exactly the launches the bf16 mode makes from 64x64 pixels up; anything else is refused, never reinterpreted
    const bool dense = ld0 == d->c0 && ld1 == d->c1 && ldo == d->cout && d->pad_mode == CF_PAD_ZERO && !d->in_nchw && d->stride == 1 && d->split_k < 1;
    const bool wino_bf16 = d->winograd == 1 && d->bf16_mfma == CF_OPERAND_BF16;
    const bool direct_bf16 = !d->winograd && d->bf16_mfma == CF_OPERAND_BF16 && d->taps == 9 && !d->out_nchw &&
                             (d->upsample ? (d->cout_pad % 128 == 0 && (long)d->hout * d->wout > 1024) : d->cout_pad == 64);
    const bool conv1 = !d->winograd && d->bf16_mfma == CF_OPERAND_F32 && d->taps == 1 && (d->cout_pad % 128 == 0 || d->cout_pad == 64) &&
                       (long)d->hout * d->wout > 1024;
    const bool conv1s = !d->winograd && d->bf16_mfma == CF_OPERAND_F16X2 && d->taps == 1 && (long)d->hout * d->wout > CF_TOKEN_IMAGE_MAX;   // streaming 1x1 (cf_split.hip)
    const bool head = few_cout && d->bf16_mfma == CF_OPERAND_F32 && !d->winograd && d->cout == 3;
    CF_REQUIRE(d->io_bf16 == 1 && dense && !ext && (head || d->cout % 4 == 0) && (wino_bf16 || direct_bf16 || conv1 || conv1s || head),
               "cf_conv2d: io_bf16 (bf16 tensors) is built for dense stride-1 launches of the bf16 mode: winograd + CF_OPERAND_BF16, direct CF_OPERAND_BF16 3x3 "
               "(cout_pad 64) / folded upsample (cout_pad %% 128 == 0), fp32 1x1 on images of more than 1024 pixels, the 3-channel NCHW head "
               "(taps %d operand %d winograd %d cout_pad %d upsample %d)", d->taps, d->bf16_mfma, d->winograd, d->cout_pad, d->upsample);
    CF_REQUIRE(d->epilogue == CF_EPI_NONE || d->epilogue == CF_EPI_RESIDUAL || d->epilogue == CF_EPI_SFT, "cf_conv2d: io_bf16 epilogues are none / residual / SFT");
  }
  if (d->act_scale) {
    CF_REQUIRE(d->prologue == CF_PRO_NONE || d->prologue == CF_PRO_LEAKY,
               "cf_conv2d: act_scale is for un-normalised inputs (prologue none / leaky), got prologue %d", d->prologue);
    const bool conv1x1_split = d->taps == 1 && d->bf16_mfma == CF_OPERAND_F16X2 && (long)d->hout * d->wout > CF_TOKEN_IMAGE_MAX;
    CF_REQUIRE((d->taps == 9 && (d->bf16_mfma == CF_OPERAND_F32 || d->winograd || d->bf16_mfma == CF_OPERAND_F16X2)) || conv1x1_split,
               "cf_conv2d: act_scale is applied by the Winograd / split-half convolution kernels only (operand %d, winograd %d, taps %d)",
               d->bf16_mfma, d->winograd, d->taps);
  }
  if (d->taps == 1 && d->bf16_mfma == CF_OPERAND_F16X2)  // (a query without statistics, stats_cpg 0, goes on through the token GEMM's checks)
    CF_REQUIRE(!pq || (!d->stats_cpg && (long)d->hout * d->wout <= CF_TOKEN_IMAGE_MAX), "cf_conv2d(1x1, f16x2): no statistics epilogue");
  else CF_REQUIRE(d->winograd >= 0 && d->winograd <= 2, "cf_conv2d: winograd must be 0, 1 (F(2x2,3x3)) or 2 (F(4x4,3x3)), got %d", d->winograd);
  const bool direct = !d->winograd && d->bf16_mfma != CF_OPERAND_F16X2;  // the kernels of this file (ext implies it)
  const int cp = d->cout_pad;
  CF_REQUIRE(!(ext && d->upsample) || cp % 64 == 0, "cf_conv2d: general upsample path needs cout_pad %% 64 == 0 (got %d)", cp);
  CF_REQUIRE(!(direct && d->in_nchw) || cp == 64, "cf_conv2d: in_nchw path is built for cout_pad 64 (got %d)", cp);
  if (direct && d->taps == 1 && d->split_k >= 1) {  // small token matrices: 64x64 tiles, split_k workgroups per tile
    const int K = d->c0 + d->c1, V = K / (CF_BK * CF_SK_SLABS);  // virtual chunks: the summation order is out = ((0 + P0) + P1) + ... whatever split_k is
    CF_REQUIRE(cp % 64 == 0 && K % (CF_BK * CF_SK_SLABS) == 0 && V >= 1 && V % d->split_k == 0,
               "cf_conv2d: split_k %d needs cout_pad %% 64 == 0, K %% 128 == 0 and split_k dividing K/128 = %d", d->split_k, V);
    CF_REQUIRE(pq || d->split_k == 1 || (d->workspace && d->counters), "cf_conv2d: split_k > 1 needs workspace and counters");
  }
  // narrow, for small-M layers (16x16 / 32x32 latents): at batch 16 a 128x128 tiling yields only 128-256 workgroups for 256 CUs; halving the N
  // tile doubles the count at the price of gathering the halo patch twice.  It depends on the per-image shape ONLY, never on the batch: tiling
  // (and with it the order of the statistics partials) must be the same for a face alone or inside any batch / shard: bitwise batch-invariant.
  f = {ld0, ld1, ldo, ext, few_cout, cp % 128 == 0 && (long)d->hout * d->wout <= 1024};
  return CF_OK;
}

static void conv_fill_args(ConvArgsExt& a, const cf_conv_desc* d, const ConvFacts& f, const float* sft_w_img = nullptr) {
  cf_fill_conv_args(a, d, sft_w_img);
  a.nchunks = d->bf16_mfma ? a.cin / 32 : (a.cin + CF_BK - 1) / CF_BK;
  a.hin = d->hin;
  a.win = d->win;
  a.hout = d->hout;
  a.wout = d->wout;
  a.cout_pad = d->cout_pad;
  a.upsample = d->upsample ? 1 : 0;
  a.out_nchw = d->out_nchw;
  a.stats_cpg = d->stats_cpg > 0 ? d->stats_cpg : 1;
  a.nparts = a.tiles_x = a.tiles_per_img = a.ntn = 0;
  a.ld0 = f.ld0;
  a.ld1 = f.ld1;
  a.ldo = f.ldo;
  a.pad_mode = d->pad_mode;
  a.pad_lo = d->pad_lo;
  a.nt_out = cf_nt_store((long)d->batch * d->hout * d->wout * d->cout * 4);
}

constexpr int CF_NOT_MINE = 1;  // (as cf_gemm_f32_tile_try: no rung takes the shape; the caller goes on or reports)
// The tile ladder of the direct stride-1 kernels: narrow -> 128x64 tiles, cout_pad % 128 == 0 -> 128x128, else 256x64 -- for cout_pad 64 only
// (exact64: fp32 operands) or for whatever is left (16-bit operands).  Instantiate it for the (TAPS, BF16, F16) that have all three shapes only.
template <int TAPS, bool BF16, bool F16>
static int launch_ladder(const ConvArgsExt& a, bool narrow, bool exact64, hipStream_t stream, int* pq) {
  if (narrow) return launch<TAPS, 1, 2, 2, 2, 1, false, BF16, false, F16>(a, stream, pq);
  if (a.cout_pad % 128 == 0) return launch<TAPS, 1, 2, 2, 2, 2, false, BF16, false, F16>(a, stream, pq);
  if (!exact64 || a.cout_pad == 64) return launch<TAPS, 1, 4, 1, 2, 2, false, BF16, false, F16>(a, stream, pq);
  return CF_NOT_MINE;
}

// The vector-ALU first conv (write-bound layer): 16x16 pixel tiles, four statistics partials per tile.
static int launch_few_cin(ConvArgsExt& a, const cf_conv_desc* d, hipStream_t stream, int* pq, bool u8 = false) {
  a.tiles_x = d->wout / 16;
  a.tiles_per_img = a.tiles_x * (d->hout / 16);
  a.nparts = a.tiles_per_img * 4;
  if (pq) {
    *pq = a.nparts;
    return CF_OK;
  }
  auto kern = d->c0 != 3 ? conv3x3_few_cin_kernel<0> : a.nt_out ? conv3x3_few_cin_kernel<3, true> : conv3x3_few_cin_kernel<3>;
  if (u8) kern = a.nt_out ? conv3x3_few_cin_kernel<3, true, true> : conv3x3_few_cin_kernel<3, false, true>;   // (c0 = 3: checked by cf_conv2d_u8)
  hipLaunchKernelGGL(kern, dim3(a.tiles_per_img * d->batch), dim3(256), 0, stream, a);
  CF_CHECK_LAUNCH(u8 ? "cf_conv2d_u8" : "cf_conv2d");
  return CF_OK;
}

// The vector-ALU NCHW <=4-channel output conv, any image size (edge tiles are masked).  No statistics: a parts query goes on to the next rung.
static int launch_few_cout(ConvArgsExt& a, const cf_conv_desc* d, hipStream_t stream, int* pq, bool u8 = false) {
  if (pq) return CF_NOT_MINE;
  a.tiles_x = (d->wout + 15) / 16;
  a.tiles_per_img = a.tiles_x * ((d->hout + 15) / 16);
  auto kern = d->cout != 3 ? conv3x3_few_cout_kernel<4> : d->io_bf16 ? conv3x3_few_cout_kernel<3, true> : conv3x3_few_cout_kernel<3>;
  if (u8) kern = d->io_bf16 ? conv3x3_few_cout_kernel<3, true, true> : conv3x3_few_cout_kernel<3, false, true>;   // (cout = 3: checked by cf_conv2d_u8)
  hipLaunchKernelGGL(kern, dim3(a.tiles_per_img * d->batch), dim3(256), 0, stream, a);
  CF_CHECK_LAUNCH(u8 ? "cf_conv2d_u8" : "cf_conv2d");
  return CF_OK;
}

// The direct kernels of this file.  Single-shape combinations are direct calls; the seven with three shapes go through launch_ladder.
static int launch_direct(ConvArgsExt& a, const cf_conv_desc* d, const ConvFacts& f, hipStream_t stream, int* pq) {
  const int cp = d->cout_pad;
  const bool f16 = d->bf16_mfma == CF_OPERAND_F16, bf16 = d->bf16_mfma == CF_OPERAND_BF16;
  if (f.ext && d->epilogue >= CF_EPI_PRELU) {  // the PReLU instantiations (fp32 operands, plain 3x3: checked); 64-wide channel tiles on small
    // images as in the dense kernels (`narrow`: per-image shape only), otherwise the tiles of the general rungs below
    if (d->stride == 2) return launch<9, 2, 2, 2, 2, 2, false, false, true, false, false, true>(a, stream, pq);  // cout_pad % 128 == 0 (checked)
    if (f.narrow) return launch<9, 1, 2, 2, 2, 1, false, false, true, false, false, true>(a, stream, pq);
    if (cp % 128 == 0) return launch<9, 1, 2, 2, 2, 2, false, false, true, false, false, true>(a, stream, pq);
    if (cp % 64 == 0) return launch<9, 1, 4, 1, 2, 2, false, false, true, false, false, true>(a, stream, pq);
    return launch<9, 1, 4, 1, 2, 1, false, false, true, false, false, true>(a, stream, pq);  // cout_pad % 32 == 0 (checked)
  }
  if (f.ext) {  // the general instantiations; their rungs follow no common ladder
    if (d->stride == 2) return launch<9, 2, 2, 2, 2, 2, false, false, true>(a, stream, pq);  // fp32, cout_pad % 128 == 0 (checked)
    if (d->upsample) {
      if (f16) return launch<4, 1, 4, 1, 2, 2, false, false, true, true>(a, stream, pq);
      if (cp % 128 == 0) return launch<4, 1, 2, 2, 2, 2, false, false, true>(a, stream, pq);
      return launch<4, 1, 4, 1, 2, 2, false, false, true>(a, stream, pq);
    }
    if (f16 && cp % 64 == 0) return launch<9, 1, 4, 1, 2, 2, false, false, true, true>(a, stream, pq);
    if (f16) return launch<9, 1, 4, 1, 2, 1, false, false, true, true>(a, stream, pq);
    if (cp % 128 == 0) return launch<9, 1, 2, 2, 2, 2, false, false, true>(a, stream, pq);
    if (cp % 64 == 0) return launch<9, 1, 4, 1, 2, 2, false, false, true>(a, stream, pq);
    return launch<9, 1, 4, 1, 2, 1, false, false, true>(a, stream, pq);  // cout_pad % 32 == 0 (checked)
  }
  int rc = CF_NOT_MINE;
  if (d->upsample) {  // nearest x2 + 3x3 as four 2x2 sub-pixel convolutions; weight packed by cf_pack_conv_weight_up2x[_bf16]
    if (f16) return launch_ladder<4, false, true>(a, f.narrow, false, stream, pq);
    if (bf16 && d->io_bf16) return launch<4, 1, 2, 2, 2, 2, false, true, false, false, true>(a, stream, pq);   // (cout_pad % 128 == 0, > 1024 pixels: checked)
    if (bf16) return launch_ladder<4, true, false>(a, f.narrow, false, stream, pq);
    rc = launch_ladder<4, false, false>(a, f.narrow, true, stream, pq);
    if (rc != CF_NOT_MINE) return rc;
    cf_set_error("cf_conv2d: upsample path needs cout_pad 64 or a multiple of 128 (got %d)", cp);
    return CF_ERR_ARG;
  }
  if (f16) return launch_ladder<9, false, true>(a, f.narrow, false, stream, pq);
  if (bf16 && d->io_bf16) return launch<9, 1, 4, 1, 2, 2, false, true, false, false, true>(a, stream, pq);   // (cout_pad == 64: checked)
  if (bf16) return launch_ladder<9, true, false>(a, f.narrow, false, stream, pq);
  if (d->taps == 9 && d->stride == 1) {
    if (d->in_nchw && d->cout == 64 && cp == 64 && d->hout % 16 == 0 && d->wout % 16 == 0 && (!d->stats_cpg || d->stats_cpg == 2) &&
        d->epilogue == CF_EPI_NONE)
      return launch_few_cin(a, d, stream, pq);
    if (d->in_nchw) return launch<9, 1, 4, 1, 2, 2, true>(a, stream, pq);  // (cout_pad == 64: checked)
    rc = launch_ladder<9, false, false>(a, f.narrow, true, stream, pq);
    if (rc == CF_NOT_MINE && f.few_cout) rc = launch_few_cout(a, d, stream, pq);
    if (rc == CF_NOT_MINE && cp == 32) rc = launch<9, 1, 4, 1, 2, 1, false>(a, stream, pq);
  } else if (d->taps == 9) {  // stride 2
    // 128-wide channel tiles unless the layer is small (at most 64 of them per image): 64-wide tiles double the workgroup count of a
    // small batch.  Per-image shape only: the two widths group the statistics partials differently (see cf_split_launch)
    const long wide_wgs = ((long)d->hout * d->wout / 128) * (cp / 128);
    if (cp % 128 == 0 && wide_wgs > 64) return launch<9, 2, 2, 2, 2, 2, false>(a, stream, pq);
    if (cp % 64 == 0) return launch<9, 2, 2, 2, 2, 1, false>(a, stream, pq);
  } else if (d->split_k >= 1) {  // small token matrices: 64x64 tiles, split_k workgroups per tile (its rules: checked)
    if (!pq && d->split_k == 1) {   // one workgroup per tile on a large token matrix: the 128-token tile kernel (bitwise the same result)
      rc = cf_gemm_f32_tile_try(d, stream);
      if (rc != 1) return rc;
    }
    return launch_sk<2, 2, 1, 1>(a, d->workspace, d->counters, d->split_k, stream, pq);
  } else if (d->io_bf16) {   // (images of more than 1024 pixels, cout_pad 64 or a multiple of 128: checked)
    if (cp % 128 == 0) return launch<1, 1, 2, 2, 2, 2, false, false, false, false, true>(a, stream, pq);
    return launch<1, 1, 4, 1, 2, 2, false, false, false, false, true>(a, stream, pq);
  } else {
    rc = launch_ladder<1, false, false>(a, f.narrow, true, stream, pq);
  }
  if (rc != CF_NOT_MINE) return rc;
  cf_set_error("cf_conv2d: no kernel for taps=%d stride=%d cout_pad=%d", d->taps, d->stride, cp);
  return CF_ERR_ARG;
}

static int conv_dispatch(const cf_conv_desc* d, hipStream_t stream, int* pq, const float* sft_w_img = nullptr) {
  ConvFacts f;
  if (const int rc = conv_validate(d, pq, f); rc != CF_OK) return rc;
  if (d->taps == 1 && d->bf16_mfma == CF_OPERAND_F16X2) {  // (the other four kernel families first)
    // images of more than CF_TOKEN_IMAGE_MAX pixels: the streaming 1x1 form of the split-half convolution kernel (weight: form 3 of
    // cf_pack_conv_weight_f16x2); token matrices (the Transformer's 16x16 "images"): the token GEMM (cf_pack_linear_weight_f16x2)
    if ((long)d->hout * d->wout > CF_TOKEN_IMAGE_MAX) return cf_split_launch(d, stream, pq, sft_w_img);
    return cf_gemm_split_launch(d, stream, pq);
  }
  if (d->winograd == 2) return cf_wf43_launch(d, stream, pq, sft_w_img);  // F(4x4,3x3), split-half operands (cf_wf43.hip)
  if (d->winograd) return cf_winograd_launch(d, stream, pq, sft_w_img);   // F(2x2,3x3), fp32 or split-half operands
  if (d->bf16_mfma == CF_OPERAND_F16X2) return cf_split_launch(d, stream, pq, sft_w_img);
  ConvArgsExt a;
  conv_fill_args(a, d, f, sft_w_img);
  return launch_direct(a, d, f, stream, pq);
}

extern "C" int cf_conv2d(const cf_conv_desc* d, cf_stream_t stream) { return conv_dispatch(d, (hipStream_t)stream, nullptr); }

// cf_conv2d with one SFT weight per image: every kernel family's SFT epilogue reads w_img[b] where the scalar launch reads d->sft_w (one
// expression, cf_sft_weight), so image b is bitwise the scalar launch with sft_w = w_img[b].  Checked before anything is launched.
extern "C" int cf_conv2d_sft_w(const cf_conv_desc* d, const float* w_img, cf_stream_t stream) {
  CF_REQUIRE(d, "cf_conv2d_sft_w: null descriptor");
  CF_REQUIRE(w_img, "cf_conv2d_sft_w: w_img is NULL (one float per image on the device; a scalar weight is cf_conv2d's sft_w)");
  CF_REQUIRE(d->epilogue == CF_EPI_SFT, "cf_conv2d_sft_w: the per-image weight belongs to the SFT epilogue (got epilogue %d)", d->epilogue);
  return conv_dispatch(d, (hipStream_t)stream, nullptr, w_img);
}

// cf_conv2d with the uint8 HWC BGR image at one end: the two vector-ALU boundary kernels in their U8 forms, nothing else.  The image
// pointer takes the place of d->in0 / d->out in a copy of the descriptor; the copy then passes every check of cf_conv2d, and the rules
// by which launch_direct would have sent it to the same kernel are REQUIRED here, so the fp32 launch it stands for exists.
// conv_validate for cf_conv2d_u8: the same checks, and a refusal of theirs names the export that was called.
static int conv_validate_u8(const cf_conv_desc* u, ConvFacts& f) {
  const int rc = conv_validate(u, nullptr, f);
  if (rc != CF_OK) {
    char msg[512];
    snprintf(msg, sizeof(msg), "%s", cf_last_error());
    if (!strncmp(msg, "cf_conv2d:", 10)) cf_set_error("cf_conv2d_u8:%s", msg + 10);
  }
  return rc;
}
extern "C" int cf_conv2d_u8(const cf_conv_desc* d, const uint8_t* img_in, uint8_t* img_out, cf_stream_t stream) {
  CF_REQUIRE(d, "cf_conv2d_u8: null descriptor");
  CF_REQUIRE(img_in || img_out, "cf_conv2d_u8: img_in and img_out are both NULL (exactly one of them is the image)");
  CF_REQUIRE(!(img_in && img_out), "cf_conv2d_u8: img_in and img_out are both set (exactly one of them is the image)");
  CF_REQUIRE(d->taps == 9 && d->stride == 1 && !d->upsample && d->bf16_mfma == CF_OPERAND_F32 && !d->winograd && d->c1 == 0 && d->split_k < 1,
             "cf_conv2d_u8: needs a plain 3x3 stride-1 conv with fp32 operands (taps %d stride %d upsample %d operand %d winograd %d c1 %d split_k %d)",
             d->taps, d->stride, d->upsample, d->bf16_mfma, d->winograd, d->c1, d->split_k);
  CF_REQUIRE(d->epilogue == CF_EPI_NONE, "cf_conv2d_u8: no epilogue op at the image boundary (got %d)", d->epilogue);
  cf_conv_desc u = *d;
  ConvFacts f;
  ConvArgsExt a;
  if (img_in) {
    CF_REQUIRE(d->in_nchw == 1 && !d->out_nchw, "cf_conv2d_u8: img_in stands for the NCHW input of an NHWC conv: needs in_nchw = 1 (got %d), out_nchw = 0 (got %d)",
               d->in_nchw, d->out_nchw);
    CF_REQUIRE(d->c0 == 3, "cf_conv2d_u8: img_in is a 3-channel BGR image: needs c0 = 3 (got %d)", d->c0);
    CF_REQUIRE(d->cout == 64 && d->cout_pad == 64, "cf_conv2d_u8: img_in needs cout = cout_pad = 64 (got %d / %d)", d->cout, d->cout_pad);
    CF_REQUIRE(d->hout % 16 == 0 && d->wout % 16 == 0, "cf_conv2d_u8: img_in needs hout, wout multiples of 16 (got %dx%d)", d->hout, d->wout);
    CF_REQUIRE(d->prologue == CF_PRO_NONE && !d->io_bf16 && d->pad_mode == CF_PAD_ZERO && (!d->stats_cpg || d->stats_cpg == 2),
               "cf_conv2d_u8: img_in takes no prologue, fp32 tensors, zero padding, stats_cpg 0 or 2 (prologue %d io_bf16 %d pad_mode %d stats_cpg %d)",
               d->prologue, d->io_bf16, d->pad_mode, d->stats_cpg);
    u.in0 = reinterpret_cast<const float*>(img_in);
    if (const int rc = conv_validate_u8(&u, f); rc != CF_OK) return rc;
    CF_REQUIRE(!f.ext, "cf_conv2d_u8: img_in needs a dense output (ld_out %d)", d->ld_out);
    conv_fill_args(a, &u, f);
    return launch_few_cin(a, &u, (hipStream_t)stream, nullptr, true);
  }
  CF_REQUIRE(d->out_nchw == 1 && !d->in_nchw, "cf_conv2d_u8: img_out stands for the NCHW output of an NHWC conv: needs out_nchw = 1 (got %d), in_nchw = 0 (got %d)",
             d->out_nchw, d->in_nchw);
  CF_REQUIRE(d->cout == 3 && d->cout_pad == 32, "cf_conv2d_u8: img_out is a 3-channel BGR image: needs cout = 3, cout_pad = 32 (got %d / %d)", d->cout, d->cout_pad);
  CF_REQUIRE((d->io_bf16 == 0 || d->io_bf16 == 1) && !d->stats_out, "cf_conv2d_u8: img_out needs io_bf16 0 or 1 (got %d) and no statistics", d->io_bf16);
  u.out = reinterpret_cast<float*>(img_out);
  if (const int rc = conv_validate_u8(&u, f); rc != CF_OK) return rc;
  CF_REQUIRE(f.few_cout && !f.ext, "cf_conv2d_u8: img_out needs a dense input (ld_in0 %d, c0 %d)", d->ld_in0, d->c0);
  conv_fill_args(a, &u, f);
  return launch_few_cout(a, &u, (hipStream_t)stream, nullptr, true);
}

// split-K geometry: output tiles of the launch and accumulator bytes one (tile, split) parks in the workspace
static int splitk_geometry(const cf_conv_desc* d, int* tiles, long* bytes_per_part) {
  *tiles = 0;
  *bytes_per_part = 0;
  if (!d || d->split_k < 1) return CF_OK;
  if (d->taps == 1 && d->bf16_mfma == CF_OPERAND_F16X2) return cf_gemm_split_geometry(d, tiles, bytes_per_part);
  if (d->winograd) return cf_winograd_splitk_geometry(d, tiles, bytes_per_part);
  if (d->bf16_mfma == CF_OPERAND_F16X2) return cf_split_splitk_geometry(d, tiles, bytes_per_part);
  CF_REQUIRE(d->taps == 1 && d->cout_pad % 64 == 0 && ((long)d->batch * d->hout * d->wout) % 64 == 0,
             "cf_conv2d: split_k covers 1x1 / Linear (64x64 tiles), winograd and f16x2 launches");
  *tiles = (int)((long)d->batch * d->hout * d->wout / 64) * (d->cout_pad / 64);
  *bytes_per_part = 64L * 64 * 4 * ((d->c0 + d->c1) / (16 * CF_SK_SLABS)) / (d->split_k > 0 ? d->split_k : 1);  // V chunk sums per tile in all
  return CF_OK;
}
extern "C" int64_t cf_conv2d_workspace_bytes(const cf_conv_desc* d) {
  int tiles = 0;
  long per = 0;
  const int rc = splitk_geometry(d, &tiles, &per);
  if (rc != CF_OK) return rc;
  return d && d->split_k > 1 ? (int64_t)tiles * d->split_k * per : 0;
}
extern "C" int cf_conv2d_tiles(const cf_conv_desc* d) {
  int tiles = 0;
  long per = 0;
  const int rc = splitk_geometry(d, &tiles, &per);
  return rc != CF_OK ? rc : tiles;
}

extern "C" int cf_conv2d_stats_parts(const cf_conv_desc* d) {
  int parts = 0;
  const int rc = conv_dispatch(d, nullptr, &parts);
  return rc == CF_OK ? parts : rc;
}
