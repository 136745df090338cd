// Quality metrics of image batches (basicsr/metrics/psnr_ssim.py: calculate_psnr, calculate_ssim) for gfx950: the definition stands at
// "quality metrics" in include/codeformer_hip.h.
//
//   sse_kernel<DT>        squared-error sum: a workgroup takes a strip of SSE_ROWS rows of one image pair, all channels, and writes ONE fp64
//                         partial.  Bandwidth-bound: 16-byte loads where the rows are contiguous and aligned, scalar loads otherwise -- the
//                         element -> thread map and every thread's order of additions are the same on both paths.
//   ssim_kernel<DT>       a workgroup takes a TH x TW tile of valid outputs of one plane of one image pair: it stages the tile plus the
//                         10-pixel halo of both images in LDS (fp32: uint8 and float32 inputs are exact there), filters the rows of the
//                         five planes x, y, x^2, y^2, xy into fp64 LDS, filters the columns, evaluates the map and writes ONE fp64 partial.
//   *_finalize_kernel     one wave per image adds that image's partials in a fixed order.
//
// Determinism and batch invariance: a partial's slot and value depend only on (image, plane, tile) and on (h, w): the tiling never looks at
// the batch size, the strides or the alignment, and there are no floating-point atomics.  An element is addressed through the element strides
// (batch, row, column, channel) of its image, so HWC, CHW, a border crop and a slice of a larger tensor are the same launch.
//
// This file is compiled without contraction: the Y conversion has to give the host's bits (a fused multiply-add can flip one float32 ulp of
// Y), and the SSIM map of two identical images has to be exactly 1.  The filter passes name their fused multiply-adds themselves (fma()).
#include "cf_score_parts.h"

#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int SSE_ROWS = 8;        // rows per squared-error strip
constexpr int TH = 16, TW = 32;    // SSIM outputs per tile
constexpr int TAPS = 11, HALO = TAPS - 1;
constexpr int IH = TH + HALO, IW = TW + HALO;  // staged inputs per tile: 26 x 42
constexpr int IS = 43;             // staged row stride in floats: 43 r + 4 g (r < 4, g < 8) hits 32 distinct banks in the row pass
static_assert(TH * TW == 512 && IH * (TW / 4) <= 256, "ssim_kernel: two outputs and at most one row item per thread of 256");
static_assert(2 * IH * IS * 4 + 5 * IH * TW * 8 + 64 <= 65536, "ssim_kernel: static LDS");

struct MetricArgs {
  cf_img_view a, b;
  int batch, h, w, c; // c: channels in memory (1 or 3)
  int y;              // 1: score the BT.601 Y of a BGR image (c == 3), or the float32 round trip of a grey one (c == 1)
  int planes;         // channels scored: 1 with y, else c
  int vec;            // sse_kernel: rows are contiguous in (column, channel) and every row starts on a 16-byte boundary
  int tiles_x, tiles; // ssim_kernel: tiles per row of tiles, tiles per plane
  double* parts;
  double g[TAPS];     // the normalised Gaussian window
};

// to_y_channel (basicsr/metrics/metric_util.py) of one BGR pixel with values in [0, 255]: every step one operation, in the host's order.
__device__ __forceinline__ float y_of_bgr(float b, float g, float r) {
  const float fb = b / 255.0f, fg = g / 255.0f, fr = r / 255.0f;
  const double d = (((double)fb * 24.966 + (double)fg * 128.553) + (double)fr * 65.481) + 16.0;
  return (float)(d / 255.0) * 255.0f;
}
__device__ __forceinline__ float y_of_grey(float v) { return (v / 255.0f) * 255.0f; }

// The value the metric sees at pixel `off` (an element offset that already holds batch, row and column) of plane p.
template <int DT>
__device__ __forceinline__ float load_plane(const void* img, long off, long sc, int c, int y, int p) {
  if (!y) return cf_img_elem<DT>(img, off + p * sc);
  if (c == 3) return y_of_bgr(cf_img_elem<DT>(img, off), cf_img_elem<DT>(img, off + sc), cf_img_elem<DT>(img, off + 2 * sc));
  return y_of_grey(cf_img_elem<DT>(img, off));
}

// ---- squared-error sum ----------------------------------------------------------------------------------------------------------------
// Without y a row is n = w * c logical elements e = x * c + channel, cut into groups of G = 16 (uint8) or 4 (float32); with y an element is
// a pixel and a group one pixel.  Item i of the strip = (row i / groups, group i % groups) goes to thread i % 256; a thread adds its items in
// ascending order and the elements of a group in ascending order.  uint8 without y: a group's sum is an exact integer.
template <int DT>
__global__ __launch_bounds__(256) void sse_kernel(const MetricArgs m) {
  __shared__ double red[4];
  constexpr int G = DT == 0 ? 16 : 4;
  const int strips = (m.h + SSE_ROWS - 1) / SSE_ROWS;
  const int img = blockIdx.x / strips, strip = blockIdx.x - img * strips;
  const int y0 = strip * SSE_ROWS, rows = m.h - y0 < SSE_ROWS ? m.h - y0 : SSE_ROWS;
  const long ba = img * m.a.st[0], bb = img * m.b.st[0];
  double acc = 0.0;
  if (m.y) {
    const int items = rows * m.w;
    for (int i = threadIdx.x; i < items; i += 256) {
      const int r = i / m.w, x = i - r * m.w;
      const float va = load_plane<DT>(m.a.p, ba + (y0 + r) * m.a.st[1] + x * m.a.st[2], m.a.st[3], m.c, 1, 0);
      const float vb = load_plane<DT>(m.b.p, bb + (y0 + r) * m.b.st[1] + x * m.b.st[2], m.b.st[3], m.c, 1, 0);
      const double d = (double)va - (double)vb;
      acc += d * d;
    }
  } else {
    const int n = m.w * m.c, groups = (n + G - 1) / G, items = rows * groups;
    for (int i = threadIdx.x; i < items; i += 256) {
      const int r = i / groups, e0 = (i - r * groups) * G;
      const int cnt = n - e0 < G ? n - e0 : G;
      const long ra = ba + (y0 + r) * m.a.st[1], rb = bb + (y0 + r) * m.b.st[1];
      float va[G], vb[G];
      if (m.vec && cnt == G) {  // 16 bytes per image: the logical elements e0 .. e0 + G - 1 are G consecutive elements of memory
        const cf_u32x4 qa = *reinterpret_cast<const cf_u32x4*>(static_cast<const char*>(m.a.p) + (ra + e0) * (DT == 0 ? 1 : 4));
        const cf_u32x4 qb = *reinterpret_cast<const cf_u32x4*>(static_cast<const char*>(m.b.p) + (rb + e0) * (DT == 0 ? 1 : 4));
#pragma unroll
        for (int k = 0; k < G; ++k) {
          if (DT == 0) {
            va[k] = (float)((qa[k >> 2] >> (8 * (k & 3))) & 255u);
            vb[k] = (float)((qb[k >> 2] >> (8 * (k & 3))) & 255u);
          } else {  // (through a copy: __builtin_bit_cast of a vector ELEMENT reads the vector's first dword whatever the index)
            const unsigned ua = qa[k & 3], ub = qb[k & 3];
            va[k] = __builtin_bit_cast(float, ua);
            vb[k] = __builtin_bit_cast(float, ub);
          }
        }
      } else {
#pragma unroll
        for (int k = 0; k < G; ++k) {
          va[k] = vb[k] = 0.f;
          if (k < cnt) {
            const int e = e0 + k, x = e / m.c, ch = e - x * m.c;
            va[k] = cf_img_elem<DT>(m.a.p, ra + x * m.a.st[2] + ch * m.a.st[3]);
            vb[k] = cf_img_elem<DT>(m.b.p, rb + x * m.b.st[2] + ch * m.b.st[3]);
          }
        }
      }
      if (DT == 0) {  // integers: at most 16 * 255^2 per group
        int s = 0;
#pragma unroll
        for (int k = 0; k < G; ++k) {
          const int d = (int)va[k] - (int)vb[k];
          s += d * d;
        }
        acc += (double)s;
      } else {
#pragma unroll
        for (int k = 0; k < G; ++k) {
          const double d = (double)va[k] - (double)vb[k];
          if (k < cnt) acc += d * d;
        }
      }
    }
  }
  acc = cf_block_sum_f64(acc, red);
  if (threadIdx.x == 0) m.parts[(size_t)img * strips + strip] = acc;
}

// sse[b] = the image's partials in strip order (lane l adds strips l, l + 64, .., then the xor tree); psnr[b] (optional) from it.
__global__ __launch_bounds__(64) void sse_finalize_kernel(const double* __restrict__ parts, int strips, double count, double* __restrict__ sse,
                                                          double* __restrict__ psnr) {
  const int img = blockIdx.x;
  const double s = cf_finish_sum_f64(parts + (size_t)img * strips, strips);
  if (threadIdx.x == 0) {
    sse[img] = s;
    if (psnr) {
      const double mse = s / count;
      psnr[img] = mse == 0.0 ? INFINITY : 20.0 * log10(255.0 / sqrt(mse));
    }
  }
}

// ---- SSIM -----------------------------------------------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(256) void ssim_kernel(const MetricArgs m) {
  __shared__ float s_a[IH * IS], s_b[IH * IS];
  __shared__ double s_row[5][IH][TW];  // the row-filtered planes x, y, x^2, y^2, xy
  __shared__ double red[4];
  const int tid = threadIdx.x;
  int blk = blockIdx.x;
  const int tile = blk % m.tiles;
  blk /= m.tiles;
  const int p = blk % m.planes, img = blk / m.planes;
  const int ty = tile / m.tiles_x, tx = tile - ty * m.tiles_x;
  const int y0 = ty * TH, x0 = tx * TW;  // the tile's first output = its first input row and column
  const long ba = img * m.a.st[0], bb = img * m.b.st[0];

  // stage: inputs outside the image are never read; they become 0 and reach only outputs that are masked below
  for (int i = tid; i < IH * IW; i += 256) {
    const int r = i / IW, c = i - r * IW;
    const int y = y0 + r, x = x0 + c;
    float va = 0.f, vb = 0.f;
    if (y < m.h && x < m.w) {
      va = load_plane<DT>(m.a.p, ba + y * m.a.st[1] + x * m.a.st[2], m.a.st[3], m.c, m.y, p);
      vb = load_plane<DT>(m.b.p, bb + y * m.b.st[1] + x * m.b.st[2], m.b.st[3], m.c, m.y, p);
    }
    s_a[r * IS + c] = va;
    s_b[r * IS + c] = vb;
  }
  __syncthreads();

  // rows: thread = (input row r, four adjacent outputs c0 .. c0 + 3); output j adds its taps k - j = 0 .. 10 in that order
  if (tid < IH * (TW / 4)) {
    const int r = tid / (TW / 4), c0 = (tid - r * (TW / 4)) * 4;
    double acc[4][5];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int q = 0; q < 5; ++q) acc[j][q] = 0.0;
#pragma unroll
    for (int k = 0; k < TAPS + 3; ++k) {
      const double x = (double)s_a[r * IS + c0 + k], y = (double)s_b[r * IS + c0 + k];
      const double v[5] = {x, y, x * x, y * y, x * y};  // exact products of 24-bit values
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (k - j >= 0 && k - j < TAPS) {
#pragma unroll
          for (int q = 0; q < 5; ++q) acc[j][q] = fma(m.g[k - j], v[q], acc[j][q]);
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 5; ++q)
#pragma unroll
      for (int j = 0; j < 4; ++j) s_row[q][r][c0 + j] = acc[j][q];
  }
  __syncthreads();

  // columns: thread = (column c, outputs 2 rp and 2 rp + 1), taps in ascending order again
  const int c = tid & (TW - 1), rp = tid / TW;
  double f[2][5];
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    double a0 = 0.0, a1 = 0.0;
#pragma unroll
    for (int k = 0; k < TAPS + 1; ++k) {
      const double v = s_row[q][2 * rp + k][c];
      if (k < TAPS) a0 = fma(m.g[k], v, a0);
      if (k >= 1) a1 = fma(m.g[k - 1], v, a1);
    }
    f[0][q] = a0;
    f[1][q] = a1;
  }
  const double C1 = (0.01 * 255) * (0.01 * 255), C2 = (0.03 * 255) * (0.03 * 255);
  const int oh = m.h - HALO, ow = m.w - HALO;
  double sum = 0.0;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const double mu1 = f[j][0], mu2 = f[j][1];
    const double mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
    const double sigma1_sq = f[j][2] - mu1_sq, sigma2_sq = f[j][3] - mu2_sq, sigma12 = f[j][4] - mu1_mu2;
    const double v = ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2));
    if (y0 + 2 * rp + j < oh && x0 + c < ow) sum += v;
  }
  sum = cf_block_sum_f64(sum, red);
  if (tid == 0) m.parts[((size_t)img * m.planes + p) * m.tiles + tile] = sum;
}

// ssim[b] = mean over planes of (the plane's partials in tile order / outputs per plane)
__global__ __launch_bounds__(64) void ssim_finalize_kernel(const double* __restrict__ parts, int planes, int tiles, double count,
                                                           double* __restrict__ ssim) {
  const int img = blockIdx.x;
  double total = 0.0;
  for (int p = 0; p < planes; ++p) total += cf_finish_sum_f64(parts + ((size_t)img * planes + p) * tiles, tiles) / count;
  if (threadIdx.x == 0) ssim[img] = total / (double)planes;
}

inline int ssim_tiles_x(int w) { return (w - HALO + TW - 1) / TW; }
inline int ssim_tiles_y(int h) { return (h - HALO + TH - 1) / TH; }

}  // namespace

// Checks shared by the entry points; fills the arguments that do not depend on the kernel.
static int metric_args(const char* who, const void* a, const void* b, int batch, int h, int w, int channels, const int64_t* stride_a,
                       const int64_t* stride_b, int dtype, int y_channel, double* parts, const void* out, MetricArgs& m) {
  CF_REQUIRE(parts && out, "%s: null parts/output", who);
  CF_REQUIRE(channels == 1 || channels == 3, "%s: channels %d (1 or 3)", who, channels);
  CF_REQUIRE(batch > 0 && h > 0 && w > 0, "%s: bad dims (batch %d, %dx%d)", who, batch, h, w);
  CF_REQUIRE(y_channel == 0 || y_channel == 1, "%s: y_channel %d (0 or 1)", who, y_channel);
  if (int e = cf_img_view_fill(who, a, stride_a, dtype, batch, h, w, channels, m.a)) return e;
  if (int e = cf_img_view_fill(who, b, stride_b, dtype, batch, h, w, channels, m.b)) return e;
  for (int i = 0; i < 4; ++i)  // (an axis of one element adds nothing to the largest offset, whatever its stride)
    CF_REQUIRE(stride_a[i] < CF_GRID_LIM && stride_b[i] < CF_GRID_LIM, "%s: stride above 2^31 - 1 elements", who);
  m.batch = batch, m.h = h, m.w = w, m.c = channels;
  m.y = y_channel;
  m.planes = y_channel ? 1 : channels;
  m.vec = 0, m.tiles_x = m.tiles = 0;
  m.parts = parts;
  double g[TAPS], sum = 0.0;  // cv2.getGaussianKernel(11, 1.5)
  for (int i = 0; i < TAPS; ++i) sum += g[i] = exp(-(double)((i - 5) * (i - 5)) / (2 * 1.5 * 1.5));
  for (int i = 0; i < TAPS; ++i) m.g[i] = g[i] / sum;
  return CF_OK;
}

extern "C" int cf_metric_parts(int h, int w, int channels) {
  CF_REQUIRE(h > 0 && w > 0 && (channels == 1 || channels == 3), "cf_metric_parts: %dx%d, channels %d", h, w, channels);
  const long strips = (h + SSE_ROWS - 1) / SSE_ROWS;
  const long tiles = h > HALO && w > HALO ? (long)channels * ssim_tiles_x(w) * ssim_tiles_y(h) : 0;
  const long n = strips > tiles ? strips : tiles;
  CF_REQUIRE(n < CF_GRID_LIM, "cf_metric_parts: image too large (%dx%d)", h, w);
  return (int)n;
}

extern "C" int cf_psnr(const void* a, const void* b, int batch, int h, int w, int channels, const int64_t* stride_a, const int64_t* stride_b,
                       int dtype, int y_channel, double* parts, double* sse, double* psnr, cf_stream_t stream) {
  MetricArgs m;
  if (int e = metric_args("cf_psnr", a, b, batch, h, w, channels, stride_a, stride_b, dtype, y_channel, parts, sse, m)) return e;
  const long strips = (h + SSE_ROWS - 1) / SSE_ROWS;
  CF_REQUIRE(strips * batch < CF_GRID_LIM, "cf_psnr: too many workgroups");
  if (!y_channel) {
    const long es = dtype == 0 ? 1 : 4;
    bool ok = true;
    for (int i = 0; i < 2; ++i) {
      const long* s = i ? m.b.st : m.a.st;
      ok = ok && (channels == 1 || s[3] == 1) && s[2] == channels && (s[0] * es) % 16 == 0 && (s[1] * es) % 16 == 0 && cf_aligned16(i ? b : a);
    }
    m.vec = ok;
  }
  const dim3 grid((unsigned)(strips * batch));
  if (dtype == 0) hipLaunchKernelGGL(sse_kernel<0>, grid, dim3(256), 0, (hipStream_t)stream, m);
  else hipLaunchKernelGGL(sse_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, m);
  CF_CHECK_LAUNCH("cf_psnr");
  hipLaunchKernelGGL(sse_finalize_kernel, dim3((unsigned)batch), dim3(64), 0, (hipStream_t)stream, parts, (int)strips,
                     (double)h * (double)w * (double)m.planes, sse, psnr);
  CF_CHECK_LAUNCH("cf_psnr (finalize)");
  return CF_OK;
}

extern "C" int cf_ssim(const void* a, const void* b, int batch, int h, int w, int channels, const int64_t* stride_a, const int64_t* stride_b,
                       int dtype, int y_channel, double* parts, double* ssim, cf_stream_t stream) {
  MetricArgs m;
  if (int e = metric_args("cf_ssim", a, b, batch, h, w, channels, stride_a, stride_b, dtype, y_channel, parts, ssim, m)) return e;
  CF_REQUIRE(h >= TAPS && w >= TAPS, "cf_ssim: the image (%dx%d) is smaller than the 11x11 window", h, w);
  m.tiles_x = ssim_tiles_x(w);
  m.tiles = m.tiles_x * ssim_tiles_y(h);
  const long blocks = (long)m.tiles * m.planes * batch;
  CF_REQUIRE(blocks < CF_GRID_LIM, "cf_ssim: too many workgroups");
  if (dtype == 0) hipLaunchKernelGGL(ssim_kernel<0>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, m);
  else hipLaunchKernelGGL(ssim_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, m);
  CF_CHECK_LAUNCH("cf_ssim");
  hipLaunchKernelGGL(ssim_finalize_kernel, dim3((unsigned)batch), dim3(64), 0, (hipStream_t)stream, parts, m.planes, m.tiles,
                     (double)(h - HALO) * (double)(w - HALO), ssim);
  CF_CHECK_LAUNCH("cf_ssim (finalize)");
  return CF_OK;
}
