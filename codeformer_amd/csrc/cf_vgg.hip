// The pieces of VGGFeatureExtractor (basicsr/archs/vgg_arch.py) and of PerceptualLoss (basicsr/losses/losses.py) that are not a convolution,
// for gfx950.  The definitions stand at "VGG / perceptual" in include/codeformer_hip.h.
//
//   vgg_input_kernel        image (uint8 / float32, any strides, BGR or RGB) -> normalised dense NHWC with zero-padded channels, thread = pixel
//   relu_kernel             x > 0 ? x : +0, float4, in place or not
//   cf_act_maxpool2_kernel<relu_act>   ReLU, then MaxPool2d(2, 2) with floor; optionally the full-size ReLU tensor too (cf_score_parts.h)
//   gram_kernel / gram_finish_kernel   F^T F per image on v_mfma_f32_32x32x2_f32: a workgroup owns one 64 x 64 tile (j0 >= i0) of one chunk of
//                           1024 pixels, four waves = 2 x 2 sub-tiles of 32 x 32; chunk products in a workspace, added in chunk order
//   feat_dist_kernel        per image sum |a - b| and sum (a - b)^2 in fp64, one partial per chunk of 16384 elements
//   lpips_head_kernel       the LPIPS layer term: channel-normalise both features per pixel, weighted squared difference, pixel mean
//   score_finish_kernel     one wave per image adds its partials of either in the finish order
//
// No float atomics; every order of summation is a function of the per-image shape only.
#include "cf_score_parts.h"

namespace {

__device__ __forceinline__ float relu1(float x) { return x > 0.f ? x : (x != x ? x : 0.f); }
struct relu_act {
  __device__ float operator()(float x) const { return relu1(x); }
};

// ---- input ----------------------------------------------------------------------------------------------------------------------------
struct VggInArgs {
  cf_img_view img;
  float* out;
  long pixels;
  int h, w, dtype, bgr, range_norm, use_norm, c4n;
  float mean[3], std[3];
};

__global__ __launch_bounds__(256) void vgg_input_kernel(const VggInArgs a) {
#pragma clang fp contract(off)
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= a.pixels) return;
  const int x = (int)(idx % a.w);
  const long q = idx / a.w;
  const int y = (int)(q % a.h);
  const long b = q / a.h;
  const long base = b * a.img.st[0] + y * a.img.st[1] + x * a.img.st[2];
  float v[4];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    float f = cf_img_unit(a.img.p, a.dtype, base + (a.bgr ? 2 - ch : ch) * a.img.st[3]);
    if (a.range_norm) {
      f = f + 1.0f;
      f = f / 2.0f;
    }
    if (a.use_norm) {
      f = f - a.mean[ch];
      f = f / a.std[ch];
    }
    v[ch] = f;
  }
  f32x4* const o4 = reinterpret_cast<f32x4*>(a.out) + idx * a.c4n;
  o4[0] = f32x4{v[0], v[1], v[2], 0.f};
  for (int k = 1; k < a.c4n; ++k) o4[k] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// ---- ReLU --------------------------------------------------------------------------------------------------------------------------------
// x and out are not __restrict__: cf_relu allows out == x (every element is read and written by the same thread)
__global__ __launch_bounds__(256) void relu_kernel(const float* x, float* out, long n4) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n4) return;
  const f32x4 v = reinterpret_cast<const f32x4*>(x)[idx];
  reinterpret_cast<f32x4*>(out)[idx] = f32x4{relu1(v[0]), relu1(v[1]), relu1(v[2]), relu1(v[3])};
}

// ---- Gram matrix ------------------------------------------------------------------------------------------------------------------------
// G = F^T F with F = [p][c]: the MFMA's A[i][k] = F[p0 + k][i0 + i] and B[k][j] = F[p0 + k][j0 + j] are both rows of F, contiguous along c.
// A slab is 16 pixels x 64 channels per operand tile, staged in LDS as [pixel][GR_LD]; MFMA step j of a slab contracts pixels 2 j and 2 j + 1
// (lane l: pixel 2 j + (l >> 5), channel l & 31 of the wave's half).  GR_LD = 96: the two half-waves of a read fall on disjoint banks.
constexpr int GR_T = 64, GR_KS = 16, GR_LD = 96, GR_MAXC = 512, GR_MID = 8, GR_FIN = 16;

__global__ __launch_bounds__(256) void gram_kernel(const float* __restrict__ f, float* __restrict__ ws, int hw, int c, int nchunks) {
  __shared__ __attribute__((aligned(16))) float As[2][GR_KS][GR_LD];
  __shared__ __attribute__((aligned(16))) float Bs[2][GR_KS][GR_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  const int T = c / GR_T;
  int t = blockIdx.x, ti = 0;
  while (t >= T - ti) {
    t -= T - ti;
    ++ti;
  }
  const int tj = ti + t, chunk = blockIdx.y, b = blockIdx.z;
  const bool diag = ti == tj;
  const int p0 = chunk * CF_GRAM_CHUNK;
  const int len = min(CF_GRAM_CHUNK, hw - p0), nslab = (len + GR_KS - 1) / GR_KS;
  const int lr = tid >> 4, lc = (tid & 15) * 4;  // this thread's (pixel, channel) of a slab
  const float* const fb = f + (size_t)b * hw * c;
  f32x4 ra, rb;
  auto gload = [&](int s) {
    const int p = p0 + s * GR_KS + lr;
    ra = rb = f32x4{0.f, 0.f, 0.f, 0.f};
    if (p < hw && p < p0 + CF_GRAM_CHUNK) {
      ra = *reinterpret_cast<const f32x4*>(fb + (size_t)p * c + ti * GR_T + lc);
      if (!diag) rb = *reinterpret_cast<const f32x4*>(fb + (size_t)p * c + tj * GR_T + lc);
    }
  };
  auto lstore = [&](int buf) {
    *reinterpret_cast<f32x4*>(&As[buf][lr][lc]) = ra;
    if (!diag) *reinterpret_cast<f32x4*>(&Bs[buf][lr][lc]) = rb;
  };
  // three levels of accumulation keep every chain short (fp32 rounding grows with the chain): a slab's 16 pixels on the MFMA from zero,
  // slab sums into `mid`, and `mid` into `acc` every GR_MID slabs -- chains of 16, 8 and 8 for a whole chunk
  f32x16 acc, mid;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = mid[r] = 0.f;
  gload(0);
  lstore(0);
  __syncthreads();
  const int kr = lane >> 5, ac = wm * 32 + (lane & 31), bc = wn * 32 + (lane & 31);
  for (int s = 0; s < nslab; ++s) {
    const int buf = s & 1;
    if (s + 1 < nslab) gload(s + 1);
    const float(*const Bt)[GR_LD] = diag ? As[buf] : Bs[buf];
    f32x16 sl;
#pragma unroll
    for (int r = 0; r < 16; ++r) sl[r] = 0.f;
#pragma unroll
    for (int j = 0; j < GR_KS / 2; ++j) sl = __builtin_amdgcn_mfma_f32_32x32x2f32(As[buf][2 * j + kr][ac], Bt[2 * j + kr][bc], sl, 0, 0, 0);
    mid += sl;
    if ((s & (GR_MID - 1)) == GR_MID - 1) {
      acc += mid;
#pragma unroll
      for (int r = 0; r < 16; ++r) mid[r] = 0.f;
    }
    if (s + 1 < nslab) lstore(buf ^ 1);
    __syncthreads();
  }
  acc += mid;
  float* const o = ws + (((size_t)b * nchunks + chunk) * c + ti * GR_T + wm * 32) * c + tj * GR_T + wn * 32 + (lane & 31);
#pragma unroll
  for (int r = 0; r < 16; ++r) o[(size_t)cf_acc_row(r, lane) * c] = acc[r];
}

__global__ __launch_bounds__(256) void gram_finish_kernel(const float* __restrict__ ws, float* __restrict__ g, int c, int nchunks, float denom, long total) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int j = (int)(idx % c), i = (int)((idx / c) % c);
  const long b = idx / ((long)c * c);
  if (i > j) return;
  const float* const p = ws + ((size_t)b * nchunks * c + i) * c + j;
  float s = 0.f, grp = 0.f;  // chunks in ascending order, in groups of GR_FIN: a group from zero, the group sums in order
  for (int k = 0; k < nchunks; ++k) {
    grp += p[(size_t)k * c * c];
    if ((k & (GR_FIN - 1)) == GR_FIN - 1) {
      s += grp;
      grp = 0.f;
    }
  }
  s += grp;
  s = s / denom;
  g[((size_t)b * c + i) * c + j] = s;
  g[((size_t)b * c + j) * c + i] = s;
}

// ---- feature distances ----------------------------------------------------------------------------------------------------------------
// A chunk is groups of 4 elements; group g belongs to thread g % 256, which adds its groups in ascending order and the elements of a
// group in ascending order.  VEC: 16-byte loads (n % 4 == 0, aligned pointers) -- the same elements in the same order as the scalar form.
template <bool VEC>
__global__ __launch_bounds__(256) void feat_dist_kernel(const float* __restrict__ a, const float* __restrict__ b, double* __restrict__ parts, long n, int nparts) {
#pragma clang fp contract(off)
  __shared__ double red[2][4];
  const int tid = threadIdx.x, chunk = blockIdx.x, img = blockIdx.y;
  const long e0 = (long)chunk * CF_FEAT_CHUNK, e1 = min(e0 + (long)CF_FEAT_CHUNK, n);
  const float* const pa = a + (size_t)img * n;
  const float* const pb = b + (size_t)img * n;
  double s1 = 0.0, s2 = 0.0;
  for (long e = e0 + tid * 4; e < e1; e += 1024) {
    float d[4] = {0.f, 0.f, 0.f, 0.f};
    if (VEC) {
      const f32x4 va = *reinterpret_cast<const f32x4*>(pa + e), vb = *reinterpret_cast<const f32x4*>(pb + e);
#pragma unroll
      for (int k = 0; k < 4; ++k) d[k] = va[k] - vb[k];
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (e + k < e1) d[k] = pa[e + k] - pb[e + k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double dd = (double)d[k];
      s1 += fabs(dd);
      s2 += dd * dd;
    }
  }
  s1 = cf_block_sum_f64(s1, red[0]);
  s2 = cf_block_sum_f64(s2, red[1]);
  if (tid == 0) parts[((size_t)img * nparts + chunk) * 2] = s1, parts[((size_t)img * nparts + chunk) * 2 + 1] = s2;
}

// out[img][j] = (the image's partials parts[img][..][j] in the finish order) / count, j < NV; a count of 1 leaves the sum as it is
template <int NV>
__global__ __launch_bounds__(64) void score_finish_kernel(const double* __restrict__ parts, int nparts, double count, double* __restrict__ out) {
  const size_t img = blockIdx.x;
  double s[NV];
  cf_finish_sum_f64(parts + img * nparts * NV, nparts, s);
  if (threadIdx.x == 0)
    for (int j = 0; j < NV; ++j) out[img * NV + j] = s[j] / count;
}

// ---- LPIPS head ---------------------------------------------------------------------------------------------------------------------------
// One wave per pixel: lane l holds float4 l and l + 64 of the pixel's channels (c <= 512).  Sums over channels: the lane's elements in
// ascending order, then the xor butterfly (every lane ends with the same value).  A workgroup owns LP_PIX pixels of one image, wave w the
// pixels w, w + 4, ..; a pixel's fp32 value is widened and added in that order, the four waves in order.
constexpr int LP_PIX = 256;

__global__ __launch_bounds__(256) void lpips_head_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ lin,
                                                         double* __restrict__ parts, int hw, int c, int nparts) {
#pragma clang fp contract(off)
  __shared__ double red[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, chunk = blockIdx.x, img = blockIdx.y, c4n = c >> 2;
  double acc = 0.0;
  for (int i = wave; i < LP_PIX; i += 4) {
    const int p = chunk * LP_PIX + i;
    if (p >= hw) break;  // (the same for every lane of the wave)
    const f32x4* const pa = reinterpret_cast<const f32x4*>(a + ((size_t)img * hw + p) * c);
    const f32x4* const pb = reinterpret_cast<const f32x4*>(b + ((size_t)img * hw + p) * c);
    f32x4 va[2], vb[2], vl[2];
    float sa = 0.f, sb = 0.f;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int k = lane + 64 * u;
      va[u] = vb[u] = vl[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (k < c4n) va[u] = pa[k], vb[u] = pb[k], vl[u] = reinterpret_cast<const f32x4*>(lin)[k];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float qa = va[u][e] * va[u][e], qb = vb[u][e] * vb[u][e];
        sa += qa;
        sb += qb;
      }
    }
    sa = cf_wave_sum(sa);
    sb = cf_wave_sum(sb);
    const float na = sqrtf(sa) + 1e-10f, nb = sqrtf(sb) + 1e-10f;
    float d = 0.f;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float xa = va[u][e] / na, xb = vb[u][e] / nb;
        const float x = xa - xb;
        const float t = x * x;
        const float wt = vl[u][e] * t;
        d += wt;
      }
    d = cf_wave_sum(d);
    acc += (double)d;
  }
  acc = cf_waves_sum_f64(acc, red);  // (every lane of a wave holds the wave's sum already)
  if (tid == 0) parts[(size_t)img * nparts + chunk] = acc;
}

}  // namespace

extern "C" int cf_vgg_input(const void* img, int batch, int h, int w, const int64_t* stride, int dtype, int bgr, int range_norm, int use_norm,
                            const float* mean, const float* std, int c_pad, float* out, cf_stream_t stream) {
  CF_REQUIRE(out, "cf_vgg_input: null out");
  CF_REQUIRE(batch > 0 && h > 0 && w > 0 && h < (1 << 24) && w < (1 << 24), "cf_vgg_input: bad dims (batch %d, %dx%d)", batch, h, w);
  CF_REQUIRE((bgr == 0 || bgr == 1) && (range_norm == 0 || range_norm == 1) && (use_norm == 0 || use_norm == 1), "cf_vgg_input: flags must be 0 or 1");
  CF_REQUIRE(!use_norm || (mean && std), "cf_vgg_input: use_norm needs mean and std");
  CF_REQUIRE(c_pad >= 4 && c_pad <= 64 && c_pad % 4 == 0, "cf_vgg_input: c_pad %d (4 .. 64, %% 4 == 0)", c_pad);
  CF_REQUIRE(cf_aligned16(out), "cf_vgg_input: out must be 16-byte aligned");
  const long pixels = (long)batch * h * w;
  CF_REQUIRE((pixels + 255) / 256 < CF_GRID_LIM, "cf_vgg_input: batch too large");
  VggInArgs a;
  if (int e = cf_img_view_fill("cf_vgg_input", img, stride, dtype, batch, h, w, 3, a.img)) return e;
  a.out = out;
  a.pixels = pixels, a.h = h, a.w = w, a.dtype = dtype, a.bgr = bgr, a.range_norm = range_norm, a.use_norm = use_norm, a.c4n = c_pad / 4;
  for (int i = 0; i < 3; ++i) a.mean[i] = use_norm ? mean[i] : 0.f, a.std[i] = use_norm ? std[i] : 1.f;
  hipLaunchKernelGGL(vgg_input_kernel, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  CF_CHECK_LAUNCH("cf_vgg_input");
  return CF_OK;
}

extern "C" int cf_relu(const float* x, int64_t n, float* out, cf_stream_t stream) {
  CF_REQUIRE(x && out, "cf_relu: null x/out");
  CF_REQUIRE(n > 0 && n % 4 == 0, "cf_relu: n %lld (> 0, %% 4 == 0)", (long long)n);
  CF_REQUIRE(cf_aligned16(x) && cf_aligned16(out), "cf_relu: x and out must be 16-byte aligned");
  CF_REQUIRE((n / 4 + 255) / 256 < CF_GRID_LIM, "cf_relu: tensor too large");
  hipLaunchKernelGGL(relu_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, out, (long)(n / 4));
  CF_CHECK_LAUNCH("cf_relu");
  return CF_OK;
}

extern "C" int cf_relu_maxpool2(const float* x, int batch, int h, int w, int c, float* out, float* full, cf_stream_t stream) {
  CF_REQUIRE(x && out, "cf_relu_maxpool2: null x/out");
  CF_REQUIRE(batch > 0 && h >= 2 && w >= 2 && c > 0 && c % 4 == 0, "cf_relu_maxpool2: bad dims (batch %d, input %dx%d >= 2x2, c %d: c %% 4 == 0)", batch, h, w, c);
  CF_REQUIRE(cf_aligned16(x) && cf_aligned16(out) && cf_aligned16(full), "cf_relu_maxpool2: tensors must be 16-byte aligned");
  CF_REQUIRE(out != x && out != full, "cf_relu_maxpool2: out must not alias x or full");
  return cf_act_maxpool2("cf_relu_maxpool2", x, batch, h, w, c, out, full, relu_act{}, stream);
}

static bool gram_dims_ok(int batch, int hw, int c) { return batch > 0 && batch <= 65535 && hw > 0 && c > 0 && c % GR_T == 0 && c <= GR_MAXC; }

extern "C" int64_t cf_gram_workspace_elems(int batch, int hw, int c) {
  if (!gram_dims_ok(batch, hw, c)) return -1;
  return (int64_t)batch * ((hw + CF_GRAM_CHUNK - 1) / CF_GRAM_CHUNK) * c * c;
}

extern "C" int cf_gram(const float* f, int batch, int hw, int c, float* ws, float* g, cf_stream_t stream) {
  CF_REQUIRE(f && ws && g, "cf_gram: null f/ws/g");
  CF_REQUIRE(gram_dims_ok(batch, hw, c), "cf_gram: bad dims (batch %d <= 65535, hw %d, c %d: c %% %d == 0, c <= %d)", batch, hw, c, GR_T, GR_MAXC);
  CF_REQUIRE(cf_aligned16(f), "cf_gram: f must be 16-byte aligned");
  const int nchunks = (hw + CF_GRAM_CHUNK - 1) / CF_GRAM_CHUNK, T = c / GR_T;
  CF_REQUIRE(nchunks <= 65535, "cf_gram: hw %d is more than 65535 chunks", hw);
  const long total = (long)batch * c * c;
  hipLaunchKernelGGL(gram_kernel, dim3(T * (T + 1) / 2, nchunks, batch), dim3(256), 0, (hipStream_t)stream, f, ws, hw, c, nchunks);
  CF_CHECK_LAUNCH("cf_gram");
  hipLaunchKernelGGL(gram_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ws, g, c, nchunks,
                     (float)((double)c * (double)hw), total);
  CF_CHECK_LAUNCH("cf_gram(finish)");
  return CF_OK;
}

extern "C" int cf_feat_dist_parts(int64_t n) { return n > 0 && (n + CF_FEAT_CHUNK - 1) / CF_FEAT_CHUNK < CF_GRID_LIM ? (int)((n + CF_FEAT_CHUNK - 1) / CF_FEAT_CHUNK) : -1; }

extern "C" int cf_feat_dist(const float* a, const float* b, int batch, int64_t n, double* parts, double* out, cf_stream_t stream) {
  CF_REQUIRE(a && b && parts && out, "cf_feat_dist: null a/b/parts/out");
  const int nparts = cf_feat_dist_parts(n);
  CF_REQUIRE(batch > 0 && batch <= 65535 && nparts > 0, "cf_feat_dist: bad dims (batch %d <= 65535, n %lld)", batch, (long long)n);
  const bool vec = n % 4 == 0 && cf_aligned16(a) && cf_aligned16(b);
  if (vec) hipLaunchKernelGGL(feat_dist_kernel<true>, dim3(nparts, batch), dim3(256), 0, (hipStream_t)stream, a, b, parts, (long)n, nparts);
  else hipLaunchKernelGGL(feat_dist_kernel<false>, dim3(nparts, batch), dim3(256), 0, (hipStream_t)stream, a, b, parts, (long)n, nparts);
  CF_CHECK_LAUNCH("cf_feat_dist");
  hipLaunchKernelGGL(score_finish_kernel<2>, dim3(batch), dim3(64), 0, (hipStream_t)stream, parts, nparts, 1.0, out);
  CF_CHECK_LAUNCH("cf_feat_dist(finish)");
  return CF_OK;
}

extern "C" int cf_lpips_parts(int hw) { return hw > 0 ? (hw + LP_PIX - 1) / LP_PIX : -1; }

extern "C" int cf_lpips_head(const float* a, const float* b, const float* lin, int batch, int hw, int c, double* parts, double* out, cf_stream_t stream) {
  CF_REQUIRE(a && b && lin && parts && out, "cf_lpips_head: null argument");
  CF_REQUIRE(batch > 0 && batch <= 65535 && hw > 0 && c > 0 && c % 4 == 0 && c <= 512, "cf_lpips_head: bad dims (batch %d <= 65535, hw %d, c %d: c %% 4 == 0, c <= 512)",
             batch, hw, c);
  CF_REQUIRE(cf_aligned16(a) && cf_aligned16(b) && cf_aligned16(lin), "cf_lpips_head: a, b and lin must be 16-byte aligned");
  const int nparts = cf_lpips_parts(hw);
  hipLaunchKernelGGL(lpips_head_kernel, dim3(nparts, batch), dim3(256), 0, (hipStream_t)stream, a, b, lin, parts, hw, c, nparts);
  CF_CHECK_LAUNCH("cf_lpips_head");
  hipLaunchKernelGGL(score_finish_kernel<1>, dim3(batch), dim3(64), 0, (hipStream_t)stream, parts, nparts, (double)hw, out);
  CF_CHECK_LAUNCH("cf_lpips_head(finish)");
  return CF_OK;
}
