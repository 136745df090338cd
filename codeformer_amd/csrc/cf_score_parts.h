// The pieces the scoring kernels share (cf_metrics.hip, cf_arcface.hip, cf_vgg.hip): host checks, the strided image view, the fp64 sums
// and activation + max-pool.  A new scoring kernel takes them from here.
//
// The order of every fp64 sum, fixed by the per-image shape alone (tests/test_gpu_score_order.py emulates it and compares bits):
//   a thread adds its items in ascending order; a wave: the xor butterfly 32, 16, .., 1 over 64 lanes, v = v + v[lane ^ o];
//   a workgroup: its four waves as ((w0 + w1) + w2) + w3; a finish: lane l adds partials l, l + 64, .. in ascending order, then the butterfly.
#pragma once
#include "cf_common.h"

inline bool cf_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
constexpr long CF_GRID_LIM = 1L << 31;  // workgroups per grid dimension, and the element offsets a kernel forms in 32 bits' reach

// ---- fp64 sums ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double cf_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// One value per wave of a workgroup of 256 (lane 0's counts) -> their sum in wave order; valid in thread 0.
__device__ __forceinline__ double cf_waves_sum_f64(double v, double* red) {
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}
// Sum over the 256 threads of a workgroup; valid in thread 0.  red: four doubles of LDS, one array per call.
__device__ __forceinline__ double cf_block_sum_f64(double v, double* red) { return cf_waves_sum_f64(cf_wave_sum(v), red); }
// The finish, by one wave: the n partials of an image, NV interleaved values each (p[i * NV + j]); v[j] = the sum of the j-th values.
template <int NV>
__device__ __forceinline__ void cf_finish_sum_f64(const double* __restrict__ p, int n, double (&v)[NV]) {
#pragma unroll
  for (int j = 0; j < NV; ++j) v[j] = 0.0;
  for (int i = threadIdx.x; i < n; i += 64)
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] += p[(size_t)i * NV + j];
#pragma unroll
  for (int j = 0; j < NV; ++j) v[j] = cf_wave_sum(v[j]);
}
__device__ __forceinline__ double cf_finish_sum_f64(const double* __restrict__ p, int n) {
  double v[1];
  cf_finish_sum_f64(p, n, v);
  return v[0];
}

// ---- the strided image view -----------------------------------------------------------------------------------------------------------
// A uint8 (dtype 0) or float32 (dtype 1) image batch (B,H,W,C) read through element strides, so HWC, CHW, a crop and a slice are one launch.
struct cf_img_view {
  const void* p;
  long st[4];  // element strides: image, row, column, channel
};

// Fills v after the checks every entry shares; the caller has checked that the dims are positive.
inline int cf_img_view_fill(const char* who, const void* p, const int64_t* stride, int dtype, int batch, int h, int w, int c, cf_img_view& v) {
  CF_REQUIRE(p && stride, "%s: null image or stride", who);
  CF_REQUIRE(dtype == 0 || dtype == 1, "%s: dtype %d (0 uint8, 1 float32)", who, dtype);
  const long dims[4] = {batch, h, w, c};
  long top = 0;  // the largest element offset of the tensor
  for (int i = 0; i < 4; ++i) {
    CF_REQUIRE(stride[i] >= 0, "%s: negative stride %ld", who, (long)stride[i]);
    top += dims[i] == 1 ? 0 : stride[i] < CF_GRID_LIM ? (dims[i] - 1) * stride[i] : CF_GRID_LIM;  // (no overflow, whatever the stride)
    CF_REQUIRE(top < CF_GRID_LIM, "%s: the largest element offset reaches 2^31", who);
  }
  v.p = p;
  for (int i = 0; i < 4; ++i) v.st[i] = stride[i];
  return CF_OK;
}

// the element as stored, as a float
template <int DT>
__device__ __forceinline__ float cf_img_elem(const void* p, long off) {
  if (DT == 0) return (float)static_cast<const uint8_t*>(p)[off];
  return static_cast<const float*>(p)[off];
}
// the element on the unit scale: a byte / 255.0f, a float as it is
__device__ __forceinline__ float cf_img_unit(const void* p, int dtype, long off) {
  return dtype == 0 ? cf_img_elem<0>(p, off) / 255.0f : cf_img_elem<1>(p, off);
}

// ---- activation, then MaxPool2d(2, 2) -------------------------------------------------------------------------------------------------
// Channels-last; thread = one float4 of one 2x2 cell of the ceil(h / 2) x ceil(w / 2) cells of an h x w input.  A cell that hangs over the
// last row / column gives no pooled output (floor) but its elements still reach `full`, the optional full-size activation.  x and full are
// not __restrict__: they may be the same tensor (each element belongs to one thread).  act: float -> float, bit-exact per element.
namespace {
template <class Act>
__global__ __launch_bounds__(256) void cf_act_maxpool2_kernel(const float* x, float* __restrict__ out, float* full, int h, int w, int c4n, long total,
                                                              const Act act) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int ch = (h + 1) >> 1, cw = (w + 1) >> 1, oh = h >> 1, ow = w >> 1;
  const int k = (int)(idx % c4n);
  const long p = idx / c4n;
  const int cx = (int)(p % cw);
  const long q = p / cw;
  const int cy = (int)(q % ch);
  const long b = q / ch;
  const bool pooled = cy < oh && cx < ow;
  if (!pooled && !full) return;
  f32x4 m = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
  for (int dy = 0; dy < 2; ++dy)
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      const int yy = 2 * cy + dy, xx = 2 * cx + dx;
      if (yy >= h || xx >= w) continue;
      const size_t o = (((size_t)b * h + yy) * w + xx) * c4n + k;
      const f32x4 v = reinterpret_cast<const f32x4*>(x)[o];
      f32x4 t;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        t[e] = act(v[e]);
        if (t[e] > m[e] || t[e] != t[e]) m[e] = t[e];  // torch's max_pool2d: a NaN wins
      }
      if (full) reinterpret_cast<f32x4*>(full)[o] = t;
    }
  if (pooled) reinterpret_cast<f32x4*>(out)[(((size_t)b * oh + cy) * ow + cx) * c4n + k] = m;
}
}  // namespace (a kernel of the including file, like its own)

// The launch both entries share; the caller has checked dims, alignment and aliasing.
template <class Act>
inline int cf_act_maxpool2(const char* who, const float* x, int batch, int h, int w, int c, float* out, float* full, const Act& act, cf_stream_t stream) {
  const long total = (long)batch * ((h + 1) / 2) * ((w + 1) / 2) * (c / 4);
  CF_REQUIRE((total + 255) / 256 < CF_GRID_LIM, "%s: tensor too large", who);
  hipLaunchKernelGGL(cf_act_maxpool2_kernel<Act>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, out, full, h, w, c / 4, total, act);
  CF_CHECK_LAUNCH(who);
  return CF_OK;
}
