// The pieces of ResNetArcFace (basicsr/archs/arcface_arch.py) and of the identity metric that are not a convolution, for gfx950.
// The definitions stand at "ArcFace / identity metric" in include/codeformer_hip.h.
//
//   cf_act_maxpool2_kernel<prelu_act>   stem: PReLU, then MaxPool2d(2, 2), channels-last (cf_score_parts.h)
//   se_pool_part_kernel / se_pool_finish_kernel   squeeze: fixed-order partial sums per (image, 64 channels, 256 pixels), then one
//                              thread per (image, channel) adds the partials in block order and divides once
//   se_gate_kernel             excitation: Linear -> PReLU -> Linear -> sigmoid on one pooled row, one workgroup per image
//   se_scale_res_prelu_kernel  prelu(x * y[b][c] + res), float4
//   fc_rows_kernel / fc_rows_finish_kernel   a Linear layer on at most 16 rows: lane = one output column, K cut into chunks of 256
//                              across workgroups, partials in a workspace, added in one fixed order
//   identity_input_kernel      image -> RGB in [-1, 1] -> gray -> bilinear 128 x 128, thread = one output pixel
//   cosine_rows_kernel         one wave per row pair, fp64
//
// Everything here is bandwidth-bound: no MFMA.  Reductions have one fixed order that depends on the per-image shape only (no float
// atomics), so results are bitwise repeatable and row b does not depend on the batch.
#include "cf_score_parts.h"

namespace {

__device__ __forceinline__ float prelu1(float x, float a) {
#pragma clang fp contract(off)
  return x > 0.f ? x : a * x;
}

struct prelu_act {
  float alpha;
  __device__ float operator()(float x) const { return prelu1(x, alpha); }
};

// ---- squeeze and excitation -------------------------------------------------------------------------------------------------------
constexpr int SE_PIX = 256;  // pixels per partial

__global__ __launch_bounds__(256) void se_pool_part_kernel(const float* __restrict__ x, float* __restrict__ parts, int hw, int c, int ncb, int nrb) {
  __shared__ f32x4 red[16][16];
  const int tid = threadIdx.x, cq = tid & 15, rl = tid >> 4;
  int blk = blockIdx.x;
  const int rb = blk % nrb;
  blk /= nrb;
  const int cb = blk % ncb, b = blk / ncb;
  const int ch = cb * 64 + cq * 4;
  f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
  if (ch < c) {
    for (int i = 0; i < 16; ++i) {
      const int p = rb * SE_PIX + rl + 16 * i;
      if (p < hw) s += *reinterpret_cast<const f32x4*>(x + ((size_t)b * hw + p) * c + ch);
    }
  }
  red[rl][cq] = s;
  __syncthreads();
  if (tid < 16 && ch < c) {
    f32x4 t = red[0][cq];
    for (int r = 1; r < 16; ++r) t += red[r][cq];
    *reinterpret_cast<f32x4*>(parts + ((size_t)b * nrb + rb) * c + ch) = t;
  }
}

__global__ __launch_bounds__(256) void se_pool_finish_kernel(const float* __restrict__ parts, float* __restrict__ out, int batch, int hw, int c, int nrb) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= batch * c) return;
  const int b = idx / c, ch = idx - b * c;
  float s = 0.f;
  for (int r = 0; r < nrb; ++r) s += parts[((size_t)b * nrb + r) * c + ch];
  out[idx] = s / (float)hw;
}

constexpr int SE_MAX_C = 4096, SE_MAX_R = 256;

__global__ __launch_bounds__(256) void se_gate_kernel(const float* __restrict__ pooled, const float* __restrict__ w1, const float* __restrict__ b1, float alpha,
                                                      const float* __restrict__ w2, const float* __restrict__ b2, float* __restrict__ out, int c, int r) {
  __shared__ float row[SE_MAX_C];
  __shared__ float hid[SE_MAX_R];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
  for (int i = tid; i < c; i += 256) row[i] = pooled[(size_t)b * c + i];
  __syncthreads();
  for (int j = wave; j < r; j += 4) {  // one wave per hidden unit: lane partials over c in stride order, then the butterfly
    float s = 0.f;
    for (int i = lane; i < c; i += 64) s = fmaf(w1[(size_t)j * c + i], row[i], s);
    s = cf_wave_sum(s);
    if (lane == 0) hid[j] = prelu1(s + b1[j], alpha);
  }
  __syncthreads();
  for (int i = tid; i < c; i += 256) {
    float s = 0.f;
    for (int j = 0; j < r; ++j) s = fmaf(w2[(size_t)i * r + j], hid[j], s);
    s += b2[i];
    out[(size_t)b * c + i] = 1.0f / (1.0f + expf(-s));
  }
}

__global__ __launch_bounds__(256) void se_scale_res_prelu_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ res,
                                                                 float* __restrict__ out, int c4n, long per_img, float alpha, long total) {
#pragma clang fp contract(off)
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int k = (int)(idx % c4n);
  const long b = idx / per_img;
  const f32x4 xv = reinterpret_cast<const f32x4*>(x)[idx];
  const f32x4 rv = res ? reinterpret_cast<const f32x4*>(res)[idx] : f32x4{0.f, 0.f, 0.f, 0.f};
  const f32x4 yv = reinterpret_cast<const f32x4*>(y)[b * c4n + k];
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float t = xv[e] * yv[e];
    o[e] = prelu1(res ? t + rv[e] : t, alpha);
  }
  reinterpret_cast<f32x4*>(out)[idx] = o;
}

// ---- Linear on a handful of rows ------------------------------------------------------------------------------------------------------
// A workgroup owns 64 output columns and one K chunk of 256; its four waves take a quarter of the chunk each (sixteen 16-byte weight loads
// per lane, all in flight at once: the layer is a stream of the weight) and meet in LDS, where the quarters are added in order.  Per (row,
// column): an fmaf chain in ascending k from zero per quarter, quarters in order, chunks in order -- whatever the number of rows.
constexpr int FC_ROWS = 16, FC_KC = 256, FC_Q = FC_KC / 16;  // rows per launch, K values per workgroup, float4 per wave and column
constexpr int FC_FIN = 8;                                   // the finish adds the chunks as FC_FIN interleaved chains, then those in order

__global__ __launch_bounds__(256) void fc_rows_kernel(const float* __restrict__ x, const float* __restrict__ wp, float* __restrict__ ws, int m_rows, int n_cols,
                                                      int k_len) {
  __shared__ f32x4 xs[FC_ROWS][FC_KC / 4];
  __shared__ float red[4][FC_ROWS][64];
  const int tid = threadIdx.x, nl = tid & 63, kq = tid >> 6, s = blockIdx.y, n = blockIdx.x * 64 + nl;
  for (int i = tid; i < FC_ROWS * (FC_KC / 4); i += 256) {
    const int m = i / (FC_KC / 4), k4 = i - m * (FC_KC / 4);
    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
    if (m < m_rows) v = *reinterpret_cast<const f32x4*>(x + (size_t)m * k_len + (size_t)s * FC_KC + k4 * 4);
    xs[m][k4] = v;
  }
  const int nc = n < n_cols ? n : n_cols - 1;  // (a column past the end computes a copy of the last one and stores nothing)
  const f32x4* const wcol = reinterpret_cast<const f32x4*>(wp) + ((size_t)s * (FC_KC / 4) + kq * FC_Q) * n_cols + nc;
  f32x4 wv[FC_Q];
#pragma unroll
  for (int u = 0; u < FC_Q; ++u) wv[u] = __builtin_nontemporal_load(wcol + (size_t)u * n_cols);
  __syncthreads();
  float acc[FC_ROWS];
#pragma unroll
  for (int m = 0; m < FC_ROWS; ++m) acc[m] = 0.f;
#pragma unroll
  for (int u = 0; u < FC_Q; ++u)
#pragma unroll
    for (int m = 0; m < FC_ROWS; ++m) {
      const f32x4 xv = xs[m][kq * FC_Q + u];  // the same address in every lane: an LDS broadcast
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[m] = fmaf(wv[u][e], xv[e], acc[m]);
    }
#pragma unroll
  for (int m = 0; m < FC_ROWS; ++m) red[kq][m][nl] = acc[m];
  __syncthreads();
#pragma unroll
  for (int i = 0; i < FC_ROWS / 4; ++i) {
    const int m = kq * (FC_ROWS / 4) + i;
    const float t = ((red[0][m][nl] + red[1][m][nl]) + red[2][m][nl]) + red[3][m][nl];
    if (m < m_rows && n < n_cols) ws[((size_t)s * m_rows + m) * n_cols + n] = t;
  }
}

// thread (j, output): chunks j, j + FC_FIN, ... in ascending order from zero; then the FC_FIN chains in order, then the bias
__global__ __launch_bounds__(256) void fc_rows_finish_kernel(const float* __restrict__ ws, const float* __restrict__ bias, float* __restrict__ out, int m_rows,
                                                             int n_cols, int nchunks) {
  __shared__ float part[FC_FIN][256 / FC_FIN];
  const int ol = threadIdx.x % (256 / FC_FIN), j = threadIdx.x / (256 / FC_FIN);
  const int idx = blockIdx.x * (256 / FC_FIN) + ol, total = m_rows * n_cols;
  float s = 0.f;
  if (idx < total)
    for (int c = j; c < nchunks; c += FC_FIN) s += ws[(size_t)c * total + idx];
  part[j][ol] = s;
  __syncthreads();
  if (j == 0 && idx < total) {
    float t = part[0][ol];
#pragma unroll
    for (int q = 1; q < FC_FIN; ++q) t += part[q][ol];
    out[idx] = bias ? t + bias[idx % n_cols] : t;
  }
}

// ---- identity metric ------------------------------------------------------------------------------------------------------------------
struct IdArgs {
  cf_img_view img;
  float* out;
  int batch, h, w, dtype, bgr;
  float sy, sx;  // h / 128, w / 128: one fp32 division each per launch
};

constexpr int ID_SIZE = 128;

// source rows / columns and weights of output index o along an axis of n pixels (half-pixel centres, edge clamp)
__device__ __forceinline__ void id_axis(int o, float scale, int n, int& i0, int& i1, float& lo, float& hi) {
#pragma clang fp contract(off)
  float src = ((float)o + 0.5f) * scale;
  src = src - 0.5f;
  src = src < 0.f ? 0.f : src;
  const float f = floorf(src);
  int i = (int)f;  // 0 <= src < n for every n >= 1: (o + 0.5) * n / 128 - 0.5 < n
  i = i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
  i0 = i;
  i1 = i + 1 > n - 1 ? n - 1 : i + 1;
  lo = src - f;
  hi = 1.0f - lo;
}

__device__ __forceinline__ float id_gray(const IdArgs& a, long base) {
#pragma clang fp contract(off)
  float v[3];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float f = cf_img_unit(a.img.p, a.dtype, base + ch * a.img.st[3]) * 2.0f;
    v[ch] = f - 1.0f;
  }
  const float r = a.bgr ? v[2] : v[0], g = v[1], bl = a.bgr ? v[0] : v[2];
  const float t0 = 0.2989f * r, t1 = 0.5870f * g, t2 = 0.1140f * bl;
  return (t0 + t1) + t2;
}

__global__ __launch_bounds__(256) void identity_input_kernel(const IdArgs a) {
#pragma clang fp contract(off)
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= a.batch * ID_SIZE * ID_SIZE) return;
  const int ox = idx % ID_SIZE, oy = (idx / ID_SIZE) % ID_SIZE, b = idx / (ID_SIZE * ID_SIZE);
  int y0, y1, x0, x1;
  float ly, hy, lx, hx;
  id_axis(oy, a.sy, a.h, y0, y1, ly, hy);
  id_axis(ox, a.sx, a.w, x0, x1, lx, hx);
  const long ib = (long)b * a.img.st[0];
  const float g00 = id_gray(a, ib + y0 * a.img.st[1] + x0 * a.img.st[2]), g01 = id_gray(a, ib + y0 * a.img.st[1] + x1 * a.img.st[2]);
  const float g10 = id_gray(a, ib + y1 * a.img.st[1] + x0 * a.img.st[2]), g11 = id_gray(a, ib + y1 * a.img.st[1] + x1 * a.img.st[2]);
  const float top = hx * g00 + lx * g01, bot = hx * g10 + lx * g11;
  a.out[idx] = hy * top + ly * bot;
}

__global__ __launch_bounds__(256) void cosine_rows_kernel(const float* __restrict__ x, const float* __restrict__ y, double* __restrict__ out, int rows, int n) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  double d = 0., xx = 0., yy = 0.;
  for (int i = lane; i < n; i += 64) {
    const double p = x[(size_t)row * n + i], q = y[(size_t)row * n + i];
    d += p * q;
    xx += p * p;
    yy += q * q;
  }
  d = cf_wave_sum(d), xx = cf_wave_sum(xx), yy = cf_wave_sum(yy);
  if (lane == 0) {
    const double den = sqrt(xx) * sqrt(yy);
    out[row] = d / (den > 1e-8 ? den : 1e-8);
  }
}

}  // namespace

extern "C" int cf_prelu_maxpool2(const float* x, int batch, int h, int w, int c, float alpha, float* out, cf_stream_t stream) {
  CF_REQUIRE(x && out, "cf_prelu_maxpool2: null x/out");
  CF_REQUIRE(batch > 0 && h > 0 && w > 0 && c > 0 && c % 4 == 0, "cf_prelu_maxpool2: bad dims (batch %d, output %dx%d, c %d: c %% 4 == 0)", batch, h, w, c);
  CF_REQUIRE(cf_aligned16(x) && cf_aligned16(out), "cf_prelu_maxpool2: x and out must be 16-byte aligned");
  CF_REQUIRE(h < (1 << 30) && w < (1 << 30), "cf_prelu_maxpool2: tensor too large");
  return cf_act_maxpool2("cf_prelu_maxpool2", x, batch, 2 * h, 2 * w, c, out, nullptr, prelu_act{alpha}, stream);  // (h, w: the output's)
}

extern "C" int cf_se_pool_parts(int hw) { return hw > 0 ? (hw + SE_PIX - 1) / SE_PIX : -1; }

extern "C" int cf_se_pool(const float* x, int batch, int hw, int c, float* parts, float* out, cf_stream_t stream) {
  CF_REQUIRE(x && parts && out, "cf_se_pool: null x/parts/out");
  CF_REQUIRE(batch > 0 && hw > 0 && c > 0 && c % 4 == 0, "cf_se_pool: bad dims (batch %d, hw %d, c %d: c %% 4 == 0)", batch, hw, c);
  CF_REQUIRE(cf_aligned16(x) && cf_aligned16(parts), "cf_se_pool: x and parts must be 16-byte aligned");
  const int ncb = (c + 63) / 64, nrb = (hw + SE_PIX - 1) / SE_PIX;
  const long blocks = (long)batch * ncb * nrb;
  CF_REQUIRE(blocks < CF_GRID_LIM && (long)batch * c < CF_GRID_LIM, "cf_se_pool: tensor too large");
  hipLaunchKernelGGL(se_pool_part_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, parts, hw, c, ncb, nrb);
  CF_CHECK_LAUNCH("cf_se_pool");
  hipLaunchKernelGGL(se_pool_finish_kernel, dim3((unsigned)(((long)batch * c + 255) / 256)), dim3(256), 0, (hipStream_t)stream, parts, out, batch, hw, c, nrb);
  CF_CHECK_LAUNCH("cf_se_pool(finish)");
  return CF_OK;
}

extern "C" int cf_se_gate(const float* pooled, const float* w1, const float* b1, float alpha, const float* w2, const float* b2, int batch, int c, int r,
                          float* out, cf_stream_t stream) {
  CF_REQUIRE(pooled && w1 && b1 && w2 && b2 && out, "cf_se_gate: null argument");
  CF_REQUIRE(batch > 0 && c > 0 && c <= SE_MAX_C && r > 0 && r <= SE_MAX_R, "cf_se_gate: bad dims (batch %d, c %d <= %d, r %d <= %d)", batch, c, SE_MAX_C, r,
             SE_MAX_R);
  hipLaunchKernelGGL(se_gate_kernel, dim3(batch), dim3(256), 0, (hipStream_t)stream, pooled, w1, b1, alpha, w2, b2, out, c, r);
  CF_CHECK_LAUNCH("cf_se_gate");
  return CF_OK;
}

extern "C" int cf_se_scale_res_prelu(const float* x, const float* y, const float* res, int batch, int hw, int c, float alpha, float* out, cf_stream_t stream) {
  CF_REQUIRE(x && y && out, "cf_se_scale_res_prelu: null x/y/out");
  CF_REQUIRE(batch > 0 && hw > 0 && c > 0 && c % 4 == 0, "cf_se_scale_res_prelu: bad dims (batch %d, hw %d, c %d: c %% 4 == 0)", batch, hw, c);
  CF_REQUIRE(cf_aligned16(x) && cf_aligned16(y) && cf_aligned16(res) && cf_aligned16(out), "cf_se_scale_res_prelu: tensors must be 16-byte aligned");
  const long per_img = (long)hw * (c / 4), total = per_img * batch;
  CF_REQUIRE((total + 255) / 256 < CF_GRID_LIM, "cf_se_scale_res_prelu: tensor too large");
  hipLaunchKernelGGL(se_scale_res_prelu_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, res, out, c / 4, per_img, alpha,
                     total);
  CF_CHECK_LAUNCH("cf_se_scale_res_prelu");
  return CF_OK;
}

extern "C" int64_t cf_fc_rows_workspace_elems(int m, int n, int k) {
  if (m < 1 || m > FC_ROWS || n < 1 || k < FC_KC || k % FC_KC) return -1;
  return (int64_t)(k / FC_KC) * m * n;
}

extern "C" int cf_fc_rows(const float* x, const float* wp, const float* bias, int m, int n, int k, float* ws, float* out, cf_stream_t stream) {
  CF_REQUIRE(x && wp && ws && out, "cf_fc_rows: null x/wp/ws/out");
  CF_REQUIRE(m >= 1 && m <= FC_ROWS, "cf_fc_rows: %d rows (1 .. %d per launch)", m, FC_ROWS);
  CF_REQUIRE(n >= 1 && n % 4 == 0 && k >= FC_KC && k % FC_KC == 0, "cf_fc_rows: n %d (%% 4 == 0), k %d (%% %d == 0)", n, k, FC_KC);
  CF_REQUIRE(cf_aligned16(x) && cf_aligned16(wp), "cf_fc_rows: x and wp must be 16-byte aligned");
  CF_REQUIRE(k / FC_KC <= 65535 && (long)m * n < CF_GRID_LIM, "cf_fc_rows: matrix too large");
  hipLaunchKernelGGL(fc_rows_kernel, dim3((n + 63) / 64, k / FC_KC), dim3(256), 0, (hipStream_t)stream, x, wp, ws, m, n, k);
  CF_CHECK_LAUNCH("cf_fc_rows");
  hipLaunchKernelGGL(fc_rows_finish_kernel, dim3((m * n + 256 / FC_FIN - 1) / (256 / FC_FIN)), dim3(256), 0, (hipStream_t)stream, ws, bias, out, m, n, k / FC_KC);
  CF_CHECK_LAUNCH("cf_fc_rows(finish)");
  return CF_OK;
}

extern "C" int cf_identity_input(const void* img, int batch, int h, int w, const int64_t* stride, int dtype, int bgr, float* out, cf_stream_t stream) {
  CF_REQUIRE(out, "cf_identity_input: null out");
  CF_REQUIRE(batch > 0 && h > 0 && w > 0 && h < (1 << 24) && w < (1 << 24), "cf_identity_input: bad dims (batch %d, %dx%d)", batch, h, w);
  CF_REQUIRE(bgr == 0 || bgr == 1, "cf_identity_input: bgr %d (0 or 1)", bgr);
  CF_REQUIRE((long)batch * ID_SIZE * ID_SIZE < CF_GRID_LIM, "cf_identity_input: batch too large");
  IdArgs a;
  if (int e = cf_img_view_fill("cf_identity_input", img, stride, dtype, batch, h, w, 3, a.img)) return e;
  a.out = out;
  a.batch = batch, a.h = h, a.w = w, a.dtype = dtype, a.bgr = bgr;
  a.sy = (float)h / (float)ID_SIZE;
  a.sx = (float)w / (float)ID_SIZE;
  hipLaunchKernelGGL(identity_input_kernel, dim3((batch * ID_SIZE * ID_SIZE + 255) / 256), dim3(256), 0, (hipStream_t)stream, a);
  CF_CHECK_LAUNCH("cf_identity_input");
  return CF_OK;
}

extern "C" int cf_cosine_rows(const float* x, const float* y, int rows, int n, double* out, cf_stream_t stream) {
  CF_REQUIRE(x && y && out, "cf_cosine_rows: null x/y/out");
  CF_REQUIRE(rows > 0 && n > 0, "cf_cosine_rows: bad dims (%d rows of %d)", rows, n);
  hipLaunchKernelGGL(cosine_rows_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, x, y, out, rows, n);
  CF_CHECK_LAUNCH("cf_cosine_rows");
  return CF_OK;
}
