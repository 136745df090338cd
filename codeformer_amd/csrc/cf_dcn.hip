// Deformable convolution, forward (basicsr/ops/dcn: modulated "v2" and plain "v1" -- v1 is mask == 1 without bias), for gfx950.
//
//   out[b][o][y][x] = bias[o] + sum_{c in group of o, tap k = i*kw + j} W[o][c_local][i][j] * mask[b][d*K + k][y][x] * val
//   val = bilinear sample, zeros outside the image, of x[b][c] at
//     h = float(y*sh - ph + i*dh) + offset[b][(d*K + k)*2][y][x],   w = float(x*sw - pw + j*dw) + offset[b][(d*K + k)*2 + 1][y][x]
//   with d = c / (Cin / DG) the deformable group of input channel c, K = kh*kw; val = 0 unless h > -1 && w > -1 && h < H && w < W.
//
// Two kernels:
//   dcn_mfma_kernel     the bilinear gather fused into an implicit GEMM on v_mfma_f32_32x32x2_f32 (exact fp32 operands, fp32 accumulation):
//                       M = a 4 x 16 patch of output pixels of one image, N = 64 output channels of one group, K = taps x 16-channel slabs.  The input is
//                       channels-last, so a corner of a sample is a contiguous channel vector (16-byte loads); the A tile is blended in
//                       registers and written to LDS -- no column buffer in HBM.  Weights: [group][tap][cin_g/16][cout_pad_g][16]
//                       (cf_pack_deform_conv_weight).
//   dcn_general_kernel  one thread per output element on the vector ALU: every shape the first refuses.
// Both evaluate a sample through dcn_sample below, and both form  sum_i (corner_i * mask) * x_i  before the product with the weight.
//
// Addresses: the in-range test runs on the fp32 position BEFORE any float -> int conversion (it is false for NaN, so any float bit
// pattern ends there), every corner is bounds-checked, and a corner that fails is never read: no address is formed from an unchecked
// offset.  The general kernel skips the load; the MFMA kernel reads the image through a buffer descriptor of exactly that image
// (hardware range check) and gives a failed corner the constant offset CF_DCN_NO_LOAD beyond it, for which the hardware makes no memory
// access and returns zeros -- the loads stay unconditional, so that all four corners and the weight slab are in flight behind the MFMAs.
#include "cf_conv_parts.h"
#include "cf_dcn.h"

namespace {

struct DcnArgs {
  const float* x;       // mfma: [b][h][w][cin];  general: that, or [b][cin][h][w] (x_cs / x_ps)
  const float* offset;  // [b][dg*2*taps][hout][wout]
  const float* mask;    // [b][dg*taps][hout][wout] or null (== 1)
  const float* weight;  // mfma: packed;  general: [cout][cin_g][taps]
  const float* bias;    // [cout] or null
  float* out;           // [b][cout][hout][wout]
  int batch, cin, hin, win, cout, hout, wout;
  int kh, kw, sh, sw, ph, pw, dh, dw;
  int groups, dg, cin_g, cout_g, cpdg;  // cpdg: input channels per deformable group
  int cout_pad_g, ntn_g, tiles_x, tiles_per_img;  // mfma: padded group width, N tiles per group, M tiles per row of tiles / per image
  long x_cs, x_ps;                       // general: element strides of a channel / of a pixel
  unsigned cpdg_magic;                   // mfma: 2^32 / cpdg + 1, so that c / cpdg == umulhi(c, magic) for c * cpdg < 2^32
};

// One sample: pix[i] = y*W + x of corner i (top-left, top-right, bottom-left, bottom-right), or -1 where the corner lies outside the
// image or the whole sample is out of range; cw[i] = its bilinear weight times the modulation m, 0 where pix[i] < 0.  Every operation
// is a single fp32 one (no contraction): the positions and the four weights are part of the op's definition.
__device__ __forceinline__ void dcn_sample(float h, float w, int H, int W, float m, int (&pix)[4], float (&cw)[4]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    pix[i] = -1;
    cw[i] = 0.f;
  }
  if (h > -1.f && w > -1.f && h < (float)H && w < (float)W) {  // false for NaN; from here on -1 < h < H, -1 < w < W
    const float h0f = floorf(h), w0f = floorf(w);
    const float lh = h - h0f, lw = w - w0f, hh = 1.f - lh, hw = 1.f - lw;
    const int h0 = (int)h0f, w0 = (int)w0f;  // in [-1, H-1] / [-1, W-1]
    const bool top = h0 >= 0, bot = h0 + 1 <= H - 1, left = w0 >= 0, right = w0 + 1 <= W - 1;
    if (top && left) {
      pix[0] = h0 * W + w0;
      cw[0] = (hh * hw) * m;
    }
    if (top && right) {
      pix[1] = h0 * W + w0 + 1;
      cw[1] = (hh * lw) * m;
    }
    if (bot && left) {
      pix[2] = (h0 + 1) * W + w0;
      cw[2] = (lh * hw) * m;
    }
    if (bot && right) {
      pix[3] = (h0 + 1) * W + w0 + 1;
      cw[3] = (lh * lw) * m;
    }
  }
}

constexpr int BM = CF_DCN_BM, BN = CF_DCN_BN;
constexpr int TH = 4, TW = 16;  // the M tile is a 4 x 16 patch of output pixels: the samples of neighbouring pixels fall on neighbouring
static_assert(TH * TW == BM);   // input pixels, so a compact patch re-reads far fewer cache lines than a 64-pixel row does
constexpr int LDS_TILE = BM * CF_LDK;                  // one A or B slab: 64 rows x 16 k, rows padded to 20 floats
constexpr int LDS_EPI = BN * (BM + 1);                 // the epilogue's [channel][pixel] transpose
constexpr int LDS_FLOATS = 4 * LDS_TILE > LDS_EPI ? 4 * LDS_TILE : LDS_EPI;
constexpr unsigned CF_DCN_NO_LOAD = 0x80000000u;       // byte offset past any image the route takes (cf_dcn_mfma_covers: < 2^31 bytes)

// The step counter of the K loop: tap-major, the 16-channel slabs of the group inside a tap.
struct Step {
  int tap, ti, tj, chunk;
  __device__ __forceinline__ void advance(int nchunks, int kw) {
    if (++chunk == nchunks) {
      chunk = 0;
      ++tap;
      if (++tj == kw) {
        tj = 0;
        ++ti;
      }
    }
  }
};

// 256 threads = 2 x 2 waves, each a 32 x 32 accumulator.  Gather item of a thread: float4 #k4 (4 channels) of tile pixel p = tid >> 2.
// A thread's sample (4 pixel indices, 4 weights x mask) is computed when the tap or the deformable group of its channels moves and reused
// for every slab in between.  Three stages run in one iteration, for three consecutive steps:
//   fetch   step s + 2: the two offsets and the modulation (three dwords; a pixel row of a plane is contiguous in the NCHW tensors)
//   gather  step s + 1: the sample from the values fetched one iteration earlier, then the four corner loads and the weight slab
//   mma     step s:     8 MFMAs on the LDS slabs; behind them the blend of step s + 1 and its LDS write (double buffer), one barrier
// so neither the offset -> address dependency nor the gather latency sits in front of the MFMAs.
template <bool MASK>
__global__ __launch_bounds__(256) void dcn_mfma_kernel(const DcnArgs a) {
  __shared__ __attribute__((aligned(16))) float smem[LDS_FLOATS];
  float* const As = smem;
  float* const Bs = smem + 2 * LDS_TILE;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, half = lane >> 5, l31 = lane & 31;

  const int bid = cf_xcd_tile(blockIdx.x, gridDim.x);
  const int ntn = a.groups * a.ntn_g;
  const int nt = bid % ntn, mt = bid / ntn;
  const int g = nt / a.ntn_g, n0 = (nt - g * a.ntn_g) * BN;  // n0: first channel of the tile inside its group
  const int b = mt / a.tiles_per_img, tm = mt - b * a.tiles_per_img;
  const int y0 = (tm / a.tiles_x) * TH, x0 = (tm - (tm / a.tiles_x) * a.tiles_x) * TW;
  const int npix = a.hout * a.wout, taps = a.kh * a.kw, nchunks = a.cin_g / CF_BK;

  const int p = tid >> 2, k4 = tid & 3;
  const bool live = y0 + p / TW < a.hout && x0 + p % TW < a.wout;  // edge tiles: a pixel past the image samples nothing and is not stored
  const int oy = live ? y0 + p / TW : 0, ox = live ? x0 + p % TW : 0;  // (its offset loads read pixel 0 of the plane instead and are dropped)
  const int mm = oy * a.wout + ox;
  const int c_thread = g * a.cin_g + k4 * 4;  // + chunk * 16: first channel of this thread's float4
  // image b through a descriptor of its own size: a byte offset at or beyond it -- CF_DCN_NO_LOAD -- reads nothing and yields zeros
  const __amdgpu_buffer_rsrc_t xr =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x + (size_t)b * a.hin * a.win * a.cin), 0, a.hin * a.win * a.cin * 4, 0x00020000);
  const float* const wg = a.weight + (size_t)g * taps * a.cin_g * a.cout_pad_g + tid * 4;
  const float* const offp = a.offset + (size_t)b * a.dg * taps * 2 * npix + mm;
  const float* const mskp = MASK ? a.mask + (size_t)b * a.dg * taps * npix + mm : nullptr;

  float r_oh, r_ow, r_m, r_hb, r_wb;  // fetched: offsets, modulation, and the integer part of the position converted once
  int r_d;                            // ... and the deformable group of the step's channels (c / cpdg by multiplication: cf_dcn_mfma_covers)
  auto fetch = [&](const Step& s) {
    r_d = (int)__umulhi((unsigned)(c_thread + s.chunk * CF_BK), a.cpdg_magic);
    const unsigned ch = (unsigned)r_d * taps + s.tap;  // (32-bit: the planes of one image hold fewer than 2^32 floats, checked by the host)
    r_oh = offp[ch * 2u * npix];
    r_ow = offp[(ch * 2u + 1u) * npix];
    r_m = MASK ? mskp[ch * (unsigned)npix] : 1.f;
    r_hb = (float)(oy * a.sh - a.ph + s.ti * a.dh);
    r_wb = (float)(ox * a.sw - a.pw + s.tj * a.dw);
  };

  // the sample in use: byte offsets of its four corners in the image (channel 0; CF_DCN_NO_LOAD for a corner that is not read) and weights
  unsigned boff[4] = {CF_DCN_NO_LOAD, CF_DCN_NO_LOAD, CF_DCN_NO_LOAD, CF_DCN_NO_LOAD};
  float cw[4] = {0.f, 0.f, 0.f, 0.f};
  int cur_tap = -1, cur_d = -1;
  auto gather = [&](const Step& s, f32x4(&ra)[4], f32x4& rb) {
    const int c = c_thread + s.chunk * CF_BK, d = r_d;
    // The fetched dwords are taken here on EVERY path (an empty statement that names them): were they read only inside the branch below,
    // the compiler would have to assume them still in flight on the other path and wait for this step's gathers before the next fetch may
    // overwrite the registers.
    asm volatile("" : "+v"(r_oh), "+v"(r_ow), "+v"(r_m));
    if (live && (d != cur_d || s.tap != cur_tap)) {
      int pix[4];
      dcn_sample(r_hb + r_oh, r_wb + r_ow, a.hin, a.win, r_m, pix, cw);
#pragma unroll
      for (int i = 0; i < 4; ++i) boff[i] = pix[i] >= 0 ? (unsigned)pix[i] * (unsigned)(a.cin * 4) : CF_DCN_NO_LOAD;  // (< 2^31: the image's size)
    }
    cur_d = d;
    cur_tap = s.tap;
#pragma unroll
    for (int i = 0; i < 4; ++i)  // (CF_DCN_NO_LOAD + c * 4 stays beyond the image: c * 4 < 2^31)
      ra[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xr, (int)(boff[i] + (unsigned)c * 4u), 0, 0));
    rb = *reinterpret_cast<const f32x4*>(wg + ((size_t)(s.tap * nchunks + s.chunk) * a.cout_pad_g + n0) * CF_BK);
  };
  auto store = [&](int buf, const f32x4(&ra)[4], const f32x4& rb) {
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = cw[0] * ra[0][e] + cw[1] * ra[1][e] + cw[2] * ra[2][e] + cw[3] * ra[3][e];
    *reinterpret_cast<f32x4*>(As + buf * LDS_TILE + p * CF_LDK + k4 * 4) = v;
    *reinterpret_cast<f32x4*>(Bs + buf * LDS_TILE + p * CF_LDK + k4 * 4) = rb;  // (weight row p of the slab, its float4 #k4)
  };

  f32x16 acc[1][1];
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[0][0][r] = 0.f;
  const int a_row = (wm * 32 + l31) * CF_LDK + half * 4, b_row = (wn * 32 + l31) * CF_LDK + half * 4;

  const int nsteps = taps * nchunks;
  Step sf{0, 0, 0, 0}, sg{0, 0, 0, 0};  // the steps the fetch / the gather stage works on
  f32x4 ra[4], rb;
  fetch(sf);
  gather(sg, ra, rb);
  if (nsteps > 1) {
    sf.advance(nchunks, a.kw);
    fetch(sf);
  }
  store(0, ra, rb);
  __syncthreads();
  auto mma = [&](int buf) {
    const float* const a_lds[1] = {As + buf * LDS_TILE + a_row};
    const float* const b_lds[1] = {Bs + buf * LDS_TILE + b_row};
    cf_mma_slab<1, 1>(acc, a_lds, b_lds);
  };
  // (the steady state has no condition in it, and the last two steps are written out: with `if (s + 1 < nsteps)` / `if (s + 2 < nsteps)` in
  // one loop body the compiler must assume the fetched dwords still in flight on the path that skips the gather, and waits for the
  // gathers before the next fetch)
  int s = 0;
  for (; s + 2 < nsteps; ++s) {
    sg.advance(nchunks, a.kw);
    gather(sg, ra, rb);
    sf.advance(nchunks, a.kw);
    fetch(sf);
    __builtin_amdgcn_sched_barrier(0);  // every load of the iteration is issued before the MFMAs, and the blend (which waits for the
    mma(s & 1);                         // gathers) stays behind them: the scheduler otherwise interleaves the two and the first MFMA waits
    __builtin_amdgcn_sched_barrier(0);
    store((s & 1) ^ 1, ra, rb);
    __syncthreads();
  }
  if (s + 1 < nsteps) {
    sg.advance(nchunks, a.kw);
    gather(sg, ra, rb);
    mma(s & 1);
    store((s & 1) ^ 1, ra, rb);
    __syncthreads();
    ++s;
  }
  mma(s & 1);
  __syncthreads();

  // ---- epilogue: accumulators -> LDS [channel][pixel] -> NCHW (a wave stores the patch's four 16-pixel rows of one channel), + bias; edges masked ----
  float bias[BN / 4];  // of the channels this thread stores (clamped inside the group: a masked channel reads the last one's)
#pragma unroll
  for (int j = 0; j < BN / 4; ++j) {
    const int n = n0 + (tid >> 6) + 4 * j;
    bias[j] = a.bias ? a.bias[g * a.cout_g + (n < a.cout_g ? n : a.cout_g - 1)] : 0.f;
  }
  float* const T = smem;  // (every wave is past the last barrier: the slabs are dead)
#pragma unroll
  for (int r = 0; r < 16; ++r) T[(wn * 32 + l31) * (BM + 1) + wm * 32 + cf_acc_row(r, lane)] = acc[0][0][r];
  __syncthreads();
  const int ep = tid & 63, ey = y0 + ep / TW, ex = x0 + ep % TW;
  if (ey < a.hout && ex < a.wout) {
#pragma unroll
    for (int j = 0; j < BN / 4; ++j) {
      const int n = (tid >> 6) + 4 * j;
      if (n0 + n < a.cout_g) a.out[((size_t)b * a.cout + g * a.cout_g + n0 + n) * npix + ey * a.wout + ex] = T[n * (BM + 1) + ep] + bias[j];
    }
  }
}

__global__ __launch_bounds__(256) void dcn_general_kernel(const DcnArgs a, long total) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int npix = a.hout * a.wout, taps = a.kh * a.kw;
  const int m = (int)(idx % npix);
  const int o = (int)((idx / npix) % a.cout), b = (int)(idx / ((long)npix * a.cout));
  const int oy = m / a.wout, ox = m - oy * a.wout;
  const int g = o / a.cout_g, c_lo = g * a.cin_g, c_hi = c_lo + a.cin_g;
  const float* const xb = a.x + (size_t)b * a.cin * a.hin * a.win;
  const float* const wo = a.weight + (size_t)o * a.cin_g * taps;
  float acc = 0.f;
  for (int k = 0; k < taps; ++k) {
    const int i = k / a.kw, j = k - i * a.kw;
    for (int d = c_lo / a.cpdg; d * a.cpdg < c_hi; ++d) {
      const size_t ch = ((size_t)b * a.dg + d) * taps + k;
      const float oh = a.offset[ch * 2 * npix + m], ow = a.offset[(ch * 2 + 1) * npix + m];
      const float mod = a.mask ? a.mask[ch * npix + m] : 1.f;
      int pix[4];
      float cw[4];
      dcn_sample((float)(oy * a.sh - a.ph + i * a.dh) + oh, (float)(ox * a.sw - a.pw + j * a.dw) + ow, a.hin, a.win, mod, pix, cw);
      if ((pix[0] & pix[1] & pix[2] & pix[3]) < 0) continue;  // all four are -1: nothing to sample
      const int c0 = d * a.cpdg > c_lo ? d * a.cpdg : c_lo, c1 = (d + 1) * a.cpdg < c_hi ? (d + 1) * a.cpdg : c_hi;
      for (int c = c0; c < c1; ++c) {
        const float* const xc = xb + (size_t)c * a.x_cs;
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          v[q] = 0.f;
          if (pix[q] >= 0) v[q] = xc[(size_t)pix[q] * a.x_ps];
        }
        const float val = cw[0] * v[0] + cw[1] * v[1] + cw[2] * v[2] + cw[3] * v[3];
        acc += wo[(size_t)(c - c_lo) * taps + k] * val;
      }
    }
  }
  a.out[idx] = acc + (a.bias ? a.bias[o] : 0.f);
}

}  // namespace

extern "C" int64_t cf_deform_conv2d_packed_elems(int cout, int cin, int taps, int groups) {
  if (cout <= 0 || cin <= 0 || taps <= 0 || groups <= 0 || cin % groups || cout % groups) return -1;
  return (int64_t)groups * taps * (cin / groups) * cf_dcn_cout_pad(cout / groups);
}

extern "C" int cf_deform_conv2d(const float* x, const float* offset, const float* mask, const float* weight, const float* bias, float* out,
                                int batch, int cin, int hin, int win, int cout, int kh, int kw, int stride_h, int stride_w, int pad_h,
                                int pad_w, int dil_h, int dil_w, int groups, int deform_groups, int x_nhwc, int route,
                                cf_stream_t stream) {
  CF_REQUIRE(x && offset && weight && out, "cf_deform_conv2d: null x/offset/weight/out");
  CF_REQUIRE(batch > 0 && cin > 0 && hin > 0 && win > 0 && cout > 0 && kh > 0 && kw > 0, "cf_deform_conv2d: bad dims");
  CF_REQUIRE(stride_h > 0 && stride_w > 0 && dil_h > 0 && dil_w > 0 && pad_h >= 0 && pad_w >= 0,
             "cf_deform_conv2d: stride and dilation must be positive, padding non-negative");
  CF_REQUIRE(groups > 0 && cin % groups == 0 && cout % groups == 0, "cf_deform_conv2d: groups %d must divide cin %d and cout %d", groups, cin, cout);
  CF_REQUIRE(deform_groups > 0 && cin % deform_groups == 0, "cf_deform_conv2d: deformable groups %d must divide cin %d", deform_groups, cin);
  CF_REQUIRE(route == 0 || route == 1, "cf_deform_conv2d: route %d (0 general, 1 mfma)", route);
  const long hout = ((long)hin + 2L * pad_h - ((long)dil_h * (kh - 1) + 1)) / stride_h + 1;
  const long wout = ((long)win + 2L * pad_w - ((long)dil_w * (kw - 1) + 1)) / stride_w + 1;
  CF_REQUIRE((long)hin + 2L * pad_h >= (long)dil_h * (kh - 1) + 1 && (long)win + 2L * pad_w >= (long)dil_w * (kw - 1) + 1 && hout > 0 && wout > 0,
             "cf_deform_conv2d: the input (%dx%d) is smaller than the dilated kernel", hin, win);
  const long lim = 1L << 31;
  const long taps = (long)kh * kw;
  // positions are formed in int and converted once, pixel indices are ints, the fp32 image bound must be exact
  CF_REQUIRE((long)hin * win < lim && hout * wout < lim && hin < (1 << 24) && win < (1 << 24) && taps < (1 << 16) &&
                 hout * stride_h + (long)kh * dil_h + pad_h < lim && wout * stride_w + (long)kw * dil_w + pad_w < lim,
             "cf_deform_conv2d: image or kernel too large");
  DcnArgs a;
  a.x = x;
  a.offset = offset;
  a.mask = mask;
  a.weight = weight;
  a.bias = bias;
  a.out = out;
  a.batch = batch, a.cin = cin, a.hin = hin, a.win = win, a.cout = cout, a.hout = (int)hout, a.wout = (int)wout;
  a.kh = kh, a.kw = kw, a.sh = stride_h, a.sw = stride_w, a.ph = pad_h, a.pw = pad_w, a.dh = dil_h, a.dw = dil_w;
  a.groups = groups, a.dg = deform_groups, a.cin_g = cin / groups, a.cout_g = cout / groups, a.cpdg = cin / deform_groups;
  a.cout_pad_g = cf_dcn_cout_pad(a.cout_g);
  a.ntn_g = a.cout_pad_g / BN;
  a.tiles_x = (int)((wout + TW - 1) / TW);
  const long tiles_per_img = (long)a.tiles_x * ((hout + TH - 1) / TH);
  a.tiles_per_img = (int)tiles_per_img;
  a.x_cs = x_nhwc ? 1 : (long)hin * win;
  a.x_ps = x_nhwc ? cin : 1;
  a.cpdg_magic = (unsigned)((1UL << 32) / (unsigned long)a.cpdg + 1);
  if (route == 1) {
    CF_REQUIRE(cf_dcn_mfma_covers(cin, cout, hin, win, (int)taps, groups, deform_groups),
               "cf_deform_conv2d: the mfma route needs (cin/deformable_groups) %% 4 == 0, (cin/groups) %% 16 == 0, kh*kw <= %d, cin < 65536 and an image "
               "below 2^31 bytes (cin %d groups %d deformable groups %d kernel %dx%d image %dx%d)", CF_DCN_MAX_TAPS, cin, groups, deform_groups, kh, kw, hin, win);
    CF_REQUIRE(x_nhwc, "cf_deform_conv2d: the mfma route reads a channels-last input");
    CF_REQUIRE((long)deform_groups * taps * 2 * hout * wout < (1L << 32), "cf_deform_conv2d: the offset planes of one image must hold fewer than 2^32 floats");
    CF_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)weight & 15) == 0, "cf_deform_conv2d: x and the packed weight must be 16-byte aligned");
    const long nwg = (long)batch * tiles_per_img * groups * a.ntn_g;
    CF_REQUIRE(tiles_per_img < lim && nwg < lim,"cf_deform_conv2d: too many tiles (%ld)", nwg);
    if (mask) hipLaunchKernelGGL(dcn_mfma_kernel<true>, dim3((unsigned)nwg), dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(dcn_mfma_kernel<false>, dim3((unsigned)nwg), dim3(256), 0, (hipStream_t)stream, a);
  } else {
    const long total = (long)batch * cout * hout * wout;
    CF_REQUIRE((total + 255) / 256 < lim, "cf_deform_conv2d: output too large");
    hipLaunchKernelGGL(dcn_general_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, total);
  }
  CF_CHECK_LAUNCH("cf_deform_conv2d");
  return CF_OK;
}
