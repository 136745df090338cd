// The pieces of BiSeNet (facelib/parsing/bisenet.py, facelib/parsing/resnet.py) that are not a 3x3 / 1x1 convolution, for gfx950.
// The definitions stand at "BiSeNet / face parsing" in include/codeformer_hip.h.
//
//   pack_stem7x7_kernel        (64,3,7,7) weight -> [148][64], K order ascending (c, ky, kx), row 147 zero
//   stem7x7s2_kernel           ResNet-18 stem: 7x7 / stride 2 / pad 3 on the NCHW image -> NHWC 64 with bias and ReLU, an implicit GEMM on
//                              v_mfma_f32_32x32x2_f32: M = a tile of 8 x 16 output pixels, N = 64, K = 148; the 21 x 37 x 3 input patch, the
//                              packed weight and the K -> patch offset table lie in LDS
//   maxpool3s2_kernel          MaxPool2d(3, 2, 1), channels-last, float4, padding -inf
//   pooled_fc_kernel           act(W p + b) on a pooled row: thread = one output, one fmaf chain in ascending c from zero
//   scale_add_row_kernel       x * g[b][c] + r[b][c], float4
//   resize_bilinear_ac_kernel<ARGMAX>   align_corners=True bilinear NHWC -> NCHW; thread = one output pixel, channels four at a time; with
//                              ARGMAX the values are compared instead of stored
//
// Only the stem has arithmetic worth a matrix instruction (2 * 147 * 64 FLOP per output); the rest is bandwidth.  No reduction crosses a
// thread except the MFMA's own, so results are bitwise repeatable and image b does not depend on the batch.
#include "cf_score_parts.h"

namespace {

// ---- stem -----------------------------------------------------------------------------------------------------------------------------
constexpr int ST_CIN = 3, ST_KS = 7, ST_COUT = 64;
constexpr int ST_K = ST_CIN * ST_KS * ST_KS, ST_KP = (ST_K + 3) / 4 * 4;  // 147 -> 148
constexpr int ST_TH = 8, ST_TW = 16;                                     // output pixels per workgroup: wave v owns rows 2v, 2v + 1
constexpr int ST_PH = (ST_TH - 1) * 2 + ST_KS, ST_PW = (ST_TW - 1) * 2 + ST_KS;  // 21 x 37 input patch
constexpr int ST_PATCH = ST_CIN * ST_PH * ST_PW;                         // 2331 floats; slot ST_PATCH holds the zero of the padded K rows
constexpr int ST_LDW = ST_COUT + 1;  // (the two half-waves read weight rows k and k + 1: an odd row length keeps them on different banks)

__global__ __launch_bounds__(256) void pack_stem7x7_kernel(const float* __restrict__ w, float* __restrict__ wp) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= ST_KP * ST_COUT) return;
  const int k = idx / ST_COUT, n = idx - k * ST_COUT;
  wp[idx] = k < ST_K ? w[n * ST_K + k] : 0.f;
}

__global__ __launch_bounds__(256) void stem7x7s2_kernel(const float* __restrict__ x, const float* __restrict__ wp, const float* __restrict__ bias,
                                                        float* __restrict__ out, int h, int w, int ho, int wo) {
  __shared__ float wl[ST_KP * ST_LDW];
  __shared__ float patch[ST_PATCH + 1];
  __shared__ int koff[ST_KP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.z;
  const int oy0 = blockIdx.y * ST_TH, ox0 = blockIdx.x * ST_TW;
  for (int i = tid; i < ST_KP * ST_COUT; i += 256) wl[(i / ST_COUT) * ST_LDW + (i % ST_COUT)] = wp[i];
  const int iy0 = oy0 * 2 - 3, ix0 = ox0 * 2 - 3;
  for (int i = tid; i < ST_PATCH; i += 256) {
    const int c = i / (ST_PH * ST_PW), r = i - c * (ST_PH * ST_PW);
    const int py = r / ST_PW, px = r - py * ST_PW;
    const int iy = iy0 + py, ix = ix0 + px;
    float v = 0.f;
    if (iy >= 0 && iy < h && ix >= 0 && ix < w) v = x[(((size_t)b * ST_CIN + c) * h + iy) * w + ix];
    patch[i] = v;
  }
  if (tid == 0) patch[ST_PATCH] = 0.f;
  if (tid < ST_KP) {
    const int c = tid / (ST_KS * ST_KS), r = tid - c * (ST_KS * ST_KS);
    koff[tid] = tid < ST_K ? (c * ST_PH + r / ST_KS) * ST_PW + r % ST_KS : ST_PATCH;
  }
  __syncthreads();
  // A[i][k] = patch[koff[k] + pix(i)], pixel i of the wave = (row 2 * wave + (i >> 4), column i & 15); a padded k reads the zero slot
  const int i = lane & 31, half = lane >> 5;
  const int pix = ((2 * wave + (i >> 4)) * 2) * ST_PW + (i & 15) * 2;
  f32x16 acc[2];
#pragma unroll
  for (int ni = 0; ni < 2; ++ni)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[ni][r] = 0.f;
#pragma unroll 2
  for (int s = 0; s < ST_KP / 2; ++s) {  // ascending k, two per instruction
    const int k = 2 * s + half;
    const int o = koff[k];
    const float a = patch[o == ST_PATCH ? o : o + pix];
    const float b0 = wl[k * ST_LDW + i], b1 = wl[k * ST_LDW + 32 + i];
    acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc[0], 0, 0, 0);
    acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc[1], 0, 0, 0);
  }
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const int ch = ni * 32 + i;
    const float bv = bias[ch];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int p = cf_acc_row(r, lane);
      const int oy = oy0 + 2 * wave + (p >> 4), ox = ox0 + (p & 15);
      if (oy < ho && ox < wo) {
        const float v = acc[ni][r] + bv;
        out[(((size_t)b * ho + oy) * wo + ox) * ST_COUT + ch] = (v > 0.f || v != v) ? v : 0.f;
      }
    }
  }
}

// ---- MaxPool2d(3, 2, 1) ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void maxpool3s2_kernel(const float* __restrict__ x, float* __restrict__ out, int h, int w, int ho, int wo, int c4n, long total) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int k = (int)(idx % c4n);
  const long p = idx / c4n;
  const int ox = (int)(p % wo);
  const long q = p / wo;
  const int oy = (int)(q % ho);
  const long b = q / ho;
  f32x4 m = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const int yy = 2 * oy - 1 + dy, xx = 2 * ox - 1 + dx;
      if (yy < 0 || yy >= h || xx < 0 || xx >= w) continue;
      const f32x4 v = reinterpret_cast<const f32x4*>(x)[(((size_t)b * h + yy) * w + xx) * c4n + k];
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (v[e] > m[e] || v[e] != v[e]) m[e] = v[e];  // torch's max_pool2d: a NaN wins
    }
  reinterpret_cast<f32x4*>(out)[idx] = m;
}

// ---- one Linear layer on a pooled row -------------------------------------------------------------------------------------------------
constexpr int FC_MAX_C = 4096, FC_MAX_N = 512;

__global__ __launch_bounds__(64) void pooled_fc_kernel(const float* __restrict__ pooled, const float* __restrict__ wt, const float* __restrict__ bias,
                                                       float* __restrict__ out, int c, int n, int act) {
#pragma clang fp contract(off)
  __shared__ float row[FC_MAX_C];
  const int b = blockIdx.y, j = blockIdx.x * 64 + threadIdx.x;
  for (int i = threadIdx.x; i < c; i += 64) row[i] = pooled[(size_t)b * c + i];
  __syncthreads();
  if (j >= n) return;
  const f32x4* const wr = reinterpret_cast<const f32x4*>(wt + (size_t)j * c);
  float s = 0.f;
  for (int i4 = 0; i4 < c / 4; ++i4) {
    const f32x4 wv = wr[i4];
#pragma unroll
    for (int e = 0; e < 4; ++e) s = fmaf(wv[e], row[i4 * 4 + e], s);
  }
  s = s + bias[j];
  if (act == CF_FC_RELU) s = (s > 0.f || s != s) ? s : 0.f;
  else if (act == CF_FC_SIGMOID) s = 1.0f / (1.0f + expf(-s));
  out[(size_t)b * n + j] = s;
}

__global__ __launch_bounds__(256) void scale_add_row_kernel(const float* __restrict__ x, const float* __restrict__ g, const float* __restrict__ r,
                                                            float* __restrict__ out, int c4n, long per_img, long total) {
#pragma clang fp contract(off)
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int k = (int)(idx % c4n);
  const long b = idx / per_img;
  const f32x4 xv = reinterpret_cast<const f32x4*>(x)[idx];
  const f32x4 gv = reinterpret_cast<const f32x4*>(g)[b * c4n + k], rv = reinterpret_cast<const f32x4*>(r)[b * c4n + k];
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float t = xv[e] * gv[e];
    o[e] = t + rv[e];
  }
  reinterpret_cast<f32x4*>(out)[idx] = o;
}

// ---- bilinear, align_corners=True -----------------------------------------------------------------------------------------------------
// source indices and weights of output index o along an axis of n source pixels
__device__ __forceinline__ void ac_axis(int o, float scale, int n, int& i0, int& i1, float& l0, float& l1) {
#pragma clang fp contract(off)
  const float src = scale * (float)o;
  int i = (int)src;
  i = i < 0 ? 0 : (i > n - 1 ? n - 1 : i);  // (0 <= src <= n - 1 up to rounding: clamped before any address is formed)
  i0 = i;
  i1 = i + (i < n - 1 ? 1 : 0);
  l1 = src - (float)i;
  l0 = 1.0f - l1;
}

// the first n (1 .. 4) of four consecutive floats; the others are not read
__device__ __forceinline__ f32x4 ac_load(const float* p, int n) {
  if (n == 4) return *reinterpret_cast<const f32x4*>(p);
  f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int e = 0; e < n; ++e) v[e] = p[e];
  return v;
}

template <bool ARGMAX>
__global__ __launch_bounds__(256) void resize_bilinear_ac_kernel(const float* __restrict__ x, float* __restrict__ out, int64_t* __restrict__ labels, int h, int w,
                                                                 int ld, int c, int oh, int ow, float sy, float sx, long total) {
#pragma clang fp contract(off)
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int ox = (int)(idx % ow);
  const long q = idx / ow;
  const int oy = (int)(q % oh);
  const long b = q / oh;
  int y0, y1, x0, x1;
  float l0y, l1y, l0x, l1x;
  ac_axis(oy, sy, h, y0, y1, l0y, l1y);
  ac_axis(ox, sx, w, x0, x1, l0x, l1x);
  const float* const img = x + (size_t)b * h * w * ld;
  const float* const pa = img + ((size_t)y0 * w + x0) * ld;
  const float* const pb = img + ((size_t)y0 * w + x1) * ld;
  const float* const pc = img + ((size_t)y1 * w + x0) * ld;
  const float* const pd = img + ((size_t)y1 * w + x1) * ld;
  const size_t plane = (size_t)oh * ow;
  float* const o = ARGMAX ? nullptr : out + (size_t)b * c * plane + (size_t)oy * ow + ox;
  float best = 0.f;
  int besti = 0;
  for (int c0 = 0; c0 < c; c0 += 4) {
    const int n = c - c0 < 4 ? c - c0 : 4;
    const f32x4 va = ac_load(pa + c0, n), vb = ac_load(pb + c0, n), vc = ac_load(pc + c0, n), vd = ac_load(pd + c0, n);
    for (int e = 0; e < n; ++e) {
      const float t0 = l0x * va[e], t1 = l1x * vb[e], t2 = l0x * vc[e], t3 = l1x * vd[e];
      const float top = t0 + t1, bot = t2 + t3;
      const float u0 = l0y * top, u1 = l1y * bot;
      const float v = u0 + u1;
      if (ARGMAX) {
        // the lowest index among equal maxima; a NaN counts as the largest value (torch.argmax)
        if (c0 + e == 0 || (best == best && (v > best || v != v))) best = v, besti = c0 + e;
      } else {
        o[(size_t)(c0 + e) * plane] = v;
      }
    }
  }
  if (ARGMAX) labels[idx] = besti;
}

}  // namespace

extern "C" int cf_pack_stem7x7(const float* w, float* wp, cf_stream_t stream) {
  CF_REQUIRE(w && wp, "cf_pack_stem7x7: null w/wp");
  hipLaunchKernelGGL(pack_stem7x7_kernel, dim3((ST_KP * ST_COUT + 255) / 256), dim3(256), 0, (hipStream_t)stream, w, wp);
  CF_CHECK_LAUNCH("cf_pack_stem7x7");
  return CF_OK;
}

extern "C" int cf_stem7x7s2(const float* x, const float* wp, const float* bias, int batch, int h, int w, float* out, cf_stream_t stream) {
  CF_REQUIRE(x && wp && bias && out, "cf_stem7x7s2: null x/wp/bias/out");
  CF_REQUIRE(batch > 0 && batch <= 65535 && h > 0 && w > 0, "cf_stem7x7s2: bad dims (batch %d (1 .. 65535), %dx%d)", batch, h, w);
  const int ho = (h - 1) / 2 + 1, wo = (w - 1) / 2 + 1;
  CF_REQUIRE((long)batch * ST_CIN * h * w < CF_GRID_LIM && (long)batch * ho * wo * ST_COUT < CF_GRID_LIM && (ho + ST_TH - 1) / ST_TH <= 65535,
             "cf_stem7x7s2: tensor too large");
  hipLaunchKernelGGL(stem7x7s2_kernel, dim3((wo + ST_TW - 1) / ST_TW, (ho + ST_TH - 1) / ST_TH, batch), dim3(256), 0, (hipStream_t)stream, x, wp, bias, out, h, w,
                     ho, wo);
  CF_CHECK_LAUNCH("cf_stem7x7s2");
  return CF_OK;
}

extern "C" int cf_maxpool3s2(const float* x, int batch, int h, int w, int c, float* out, cf_stream_t stream) {
  CF_REQUIRE(x && out, "cf_maxpool3s2: null x/out");
  CF_REQUIRE(batch > 0 && h > 0 && w > 0 && c > 0 && c % 4 == 0, "cf_maxpool3s2: bad dims (batch %d, %dx%d, c %d: c %% 4 == 0)", batch, h, w, c);
  CF_REQUIRE(cf_aligned16(x) && cf_aligned16(out), "cf_maxpool3s2: x and out must be 16-byte aligned");
  const int ho = (h - 1) / 2 + 1, wo = (w - 1) / 2 + 1;
  const long total = (long)batch * ho * wo * (c / 4);
  CF_REQUIRE((long)batch * h * w * (c / 4) < CF_GRID_LIM && (total + 255) / 256 < CF_GRID_LIM, "cf_maxpool3s2: tensor too large");
  hipLaunchKernelGGL(maxpool3s2_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, out, h, w, ho, wo, c / 4, total);
  CF_CHECK_LAUNCH("cf_maxpool3s2");
  return CF_OK;
}

extern "C" int cf_pooled_fc(const float* pooled, const float* w, const float* bias, int batch, int c, int n, int act, float* out, cf_stream_t stream) {
  CF_REQUIRE(pooled && w && bias && out, "cf_pooled_fc: null pooled/w/bias/out");
  CF_REQUIRE(batch > 0 && batch <= 65535 && c > 0 && c <= FC_MAX_C && c % 4 == 0 && n > 0 && n <= FC_MAX_N,
             "cf_pooled_fc: bad dims (batch %d (1 .. 65535), c %d <= %d with c %% 4 == 0, n %d <= %d)", batch, c, FC_MAX_C, n, FC_MAX_N);
  CF_REQUIRE(act == CF_FC_NONE || act == CF_FC_RELU || act == CF_FC_SIGMOID, "cf_pooled_fc: act %d (0 none, 1 relu, 2 sigmoid)", act);
  CF_REQUIRE(cf_aligned16(w), "cf_pooled_fc: w must be 16-byte aligned");
  hipLaunchKernelGGL(pooled_fc_kernel, dim3((n + 63) / 64, batch), dim3(64), 0, (hipStream_t)stream, pooled, w, bias, out, c, n, act);
  CF_CHECK_LAUNCH("cf_pooled_fc");
  return CF_OK;
}

extern "C" int cf_scale_add_row(const float* x, const float* g, const float* r, int batch, int hw, int c, float* out, cf_stream_t stream) {
  CF_REQUIRE(x && g && r && out, "cf_scale_add_row: null x/g/r/out");
  CF_REQUIRE(batch > 0 && hw > 0 && c > 0 && c % 4 == 0, "cf_scale_add_row: bad dims (batch %d, hw %d, c %d: c %% 4 == 0)", batch, hw, c);
  CF_REQUIRE(cf_aligned16(x) && cf_aligned16(g) && cf_aligned16(r) && cf_aligned16(out), "cf_scale_add_row: tensors must be 16-byte aligned");
  const long per_img = (long)hw * (c / 4), total = per_img * batch;
  CF_REQUIRE((total + 255) / 256 < CF_GRID_LIM, "cf_scale_add_row: tensor too large");
  hipLaunchKernelGGL(scale_add_row_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, g, r, out, c / 4, per_img, total);
  CF_CHECK_LAUNCH("cf_scale_add_row");
  return CF_OK;
}

static int resize_ac_launch(const char* who, const float* x, int batch, int h, int w, int ld, int c, float* out, int64_t* labels, int oh, int ow,
                            cf_stream_t stream) {
  CF_REQUIRE(x && (out || labels), "%s: null x/out", who);
  CF_REQUIRE(batch > 0 && h > 0 && w > 0 && oh > 0 && ow > 0 && c > 0 && c <= ld && ld % 4 == 0,
             "%s: bad dims (batch %d, %dx%d -> %dx%d, c %d of ld %d: c <= ld, ld %% 4 == 0)", who, batch, h, w, oh, ow, c, ld);
  CF_REQUIRE(cf_aligned16(x), "%s: x must be 16-byte aligned", who);
  CF_REQUIRE(h < (1 << 24) && w < (1 << 24) && oh < (1 << 24) && ow < (1 << 24), "%s: an axis of 2^24 or more pixels", who);
  const long total = (long)batch * oh * ow;
  CF_REQUIRE((total + 255) / 256 < CF_GRID_LIM, "%s: tensor too large", who);
  const float sy = oh > 1 ? (float)(h - 1) / (float)(oh - 1) : 0.f, sx = ow > 1 ? (float)(w - 1) / (float)(ow - 1) : 0.f;
  if (labels)
    hipLaunchKernelGGL(resize_bilinear_ac_kernel<true>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, out, labels, h, w, ld, c, oh, ow,
                       sy, sx, total);
  else
    hipLaunchKernelGGL(resize_bilinear_ac_kernel<false>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, out, labels, h, w, ld, c, oh,
                       ow, sy, sx, total);
  CF_CHECK_LAUNCH(who);
  return CF_OK;
}

extern "C" int cf_resize_bilinear_ac(const float* x, int batch, int h, int w, int ld, int c, float* out, int oh, int ow, cf_stream_t stream) {
  CF_REQUIRE(out, "cf_resize_bilinear_ac: null out");
  return resize_ac_launch("cf_resize_bilinear_ac", x, batch, h, w, ld, c, out, nullptr, oh, ow, stream);
}

extern "C" int cf_resize_bilinear_ac_argmax(const float* x, int batch, int h, int w, int ld, int c, int64_t* labels, int oh, int ow, cf_stream_t stream) {
  CF_REQUIRE(labels, "cf_resize_bilinear_ac_argmax: null labels");
  return resize_ac_launch("cf_resize_bilinear_ac_argmax", x, batch, h, w, ld, c, nullptr, labels, oh, ow, stream);
}
