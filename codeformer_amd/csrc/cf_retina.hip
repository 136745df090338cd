// The RetinaFace ResNet-50 detector's own kernels (facelib/detection/retinaface) for gfx950.  The definitions stand at "RetinaFace ResNet-50
// detector" in include/codeformer_hip.h.
//
//   pack_pointwise_kernel   (cout, cin) weight -> [ceil64(cout)][ceil32(cin)], zero padded
//   pointwise_kernel<STEP>  act(X W^T + b [+ res]) over pixels: a GEMM on v_mfma_f32_32x32x2_f32, workgroup tile 128 (M) x 64 (N), K slabs of
//                           32 channels staged through LDS; wave v owns rows 32 v .. 32 v + 31 and both 32-column halves (two accumulators).
//                           Both operands lie K-contiguous in LDS ([row][36]: the pad of 4 spreads the eight rows of a ds_read_b128 phase
//                           over all banks), so a lane fetches four k of its row with ONE 16-byte read and feeds four instructions from it.
//                           The next slab's global loads are issued before the current slab's MFMAs and land in LDS after them.
//   nearest_add_kernel      a + nearest(b -> a's size), float4
//   retina_decode_kernel    softmax, box / landmark decode and the score threshold: one workgroup of 1024 threads per image walks the anchors
//                           in chunks of 1024; per chunk a ballot prefix inside each wave and the 16 wave totals in LDS give every passing
//                           anchor its row, in ascending anchor order
//
// Half of a bottleneck trunk's products are 1x1 convolutions; everything else in this file is bandwidth.
#include "cf_score_parts.h"

namespace {

// ---- pointwise convolution ------------------------------------------------------------------------------------------------------------
constexpr int PW_BM = 128, PW_BN = 64, PW_BK = 32, PW_LD = PW_BK + 4;
constexpr int PW_AJ = PW_BM / 32, PW_BJ = PW_BN / 32;  // float4 loads per thread and slab: thread = (row tid >> 3 (+ 32 j), float4 tid & 7)

__global__ __launch_bounds__(256) void pack_pointwise_kernel(const float* __restrict__ w, float* __restrict__ wp, int cin, int cout, int kp, long total) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int n = (int)(idx / kp), k = (int)(idx - (long)n * kp);
  wp[idx] = (n < cout && k < cin) ? w[(size_t)n * cin + k] : 0.f;
}

struct PwArgs {
  const float* x;
  const float* wp;
  const float* bias;
  const float* res;
  float* out;
  int ld_x, ld_res, ld_out;
  int m, h, w, ho, wo;  // m = batch * ho * wo rows
  int cin, kp, cout, ntn, act;
};

template <int STEP>
__global__ __launch_bounds__(256) void pointwise_kernel(const PwArgs a) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float As[PW_BM * PW_LD];
  __shared__ __attribute__((aligned(16))) float Bs[PW_BN * PW_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nt = blockIdx.x % a.ntn, mt = blockIdx.x / a.ntn;  // N-minor: the workgroups that share an A tile run side by side
  const int m0 = mt * PW_BM, n0 = nt * PW_BN;
  const int kq = tid & 7, r0 = tid >> 3;

  // the source pixel of each A row this thread loads; a row past M reads the last row's address and is never stored
  size_t arow[PW_AJ];
#pragma unroll
  for (int j = 0; j < PW_AJ; ++j) {
    int m = m0 + r0 + 32 * j;
    m = m < a.m ? m : a.m - 1;
    size_t pix = (size_t)m;
    if (STEP == 2) {
      const int per = a.ho * a.wo;
      const int b = m / per, r = m - b * per;
      const int oy = r / a.wo, ox = r - oy * a.wo;
      pix = ((size_t)b * a.h + 2 * oy) * a.w + 2 * ox;
    }
    arow[j] = pix * a.ld_x;
  }
  const float* const wrow = a.wp + (size_t)(n0 + r0) * a.kp + kq * 4;

  f32x4 ra[PW_AJ], rb[PW_BJ];
  auto load = [&](int k0) {
    const int k = k0 + kq * 4;
    const bool live = k < a.cin;  // (cin % 4 == 0: a float4 is inside or outside as a whole; outside reads channel 0 and is zeroed)
    const int kc = live ? k : 0;
#pragma unroll
    for (int j = 0; j < PW_AJ; ++j) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(a.x + arow[j] + kc);
      ra[j] = live ? v : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int j = 0; j < PW_BJ; ++j) rb[j] = *reinterpret_cast<const f32x4*>(wrow + (size_t)32 * j * a.kp + k0);
  };

  f32x16 acc[2];
#pragma unroll
  for (int ni = 0; ni < 2; ++ni)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[ni][r] = 0.f;

  const int i = lane & 31, half = lane >> 5;
  const float* const ap = As + (32 * wave + i) * PW_LD + 4 * half;
  const float* const bp = Bs + i * PW_LD + 4 * half;

  load(0);
  for (int k0 = 0; k0 < a.kp; k0 += PW_BK) {
    __syncthreads();  // the previous slab's reads are done
#pragma unroll
    for (int j = 0; j < PW_AJ; ++j) *reinterpret_cast<f32x4*>(As + (r0 + 32 * j) * PW_LD + kq * 4) = ra[j];
#pragma unroll
    for (int j = 0; j < PW_BJ; ++j) *reinterpret_cast<f32x4*>(Bs + (r0 + 32 * j) * PW_LD + kq * 4) = rb[j];
    __syncthreads();
    if (k0 + PW_BK < a.kp) load(k0 + PW_BK);
#pragma unroll
    for (int g = 0; g < PW_BK / 8; ++g) {  // half 0 holds k = 8 g .. 8 g + 3 of its row, half 1 the next four: instruction e adds k pair (8 g + e, 8 g + 4 + e)
      const f32x4 av = *reinterpret_cast<const f32x4*>(ap + 8 * g);
      const f32x4 b0 = *reinterpret_cast<const f32x4*>(bp + 8 * g);
      const f32x4 b1 = *reinterpret_cast<const f32x4*>(bp + 32 * PW_LD + 8 * g);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[e], b0[e], acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[e], b1[e], acc[1], 0, 0, 0);
      }
    }
  }

#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const int n = n0 + ni * 32 + i;
    if (n >= a.cout) continue;
    const float bv = a.bias ? a.bias[n] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + 32 * wave + cf_acc_row(r, lane);
      if (m >= a.m) continue;
      float v = acc[ni][r] + bv;
      if (a.res) v = v + a.res[(size_t)m * a.ld_res + n];
      if (a.act == CF_PW_RELU) v = (v > 0.f || v != v) ? v : 0.f;
      a.out[(size_t)m * a.ld_out + n] = v;
    }
  }
}

// ---- a + nearest(b) -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void nearest_add_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, int ha, int wa, int hb,
                                                          int wb, int c4n, float sy, float sx, long total) {
#pragma clang fp contract(off)
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int k = (int)(idx % c4n);
  const long p = idx / c4n;
  const int x = (int)(p % wa);
  const long q = p / wa;
  const int y = (int)(q % ha);
  const long n = q / ha;
  int iy = (int)floorf((float)y * sy), ix = (int)floorf((float)x * sx);
  iy = iy < hb - 1 ? iy : hb - 1;
  ix = ix < wb - 1 ? ix : wb - 1;
  const f32x4 av = reinterpret_cast<const f32x4*>(a)[idx];
  const f32x4 bv = reinterpret_cast<const f32x4*>(b)[(((size_t)n * hb + iy) * wb + ix) * c4n + k];
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = av[e] + bv[e];
  reinterpret_cast<f32x4*>(out)[idx] = o;
}

// ---- decode ---------------------------------------------------------------------------------------------------------------------------
constexpr int RD_THREADS = 1024, RD_WAVES = RD_THREADS / 64;

struct RdArgs {
  const float* heads[3];
  int np[3];
  const float* priors;
  int n;
  float var0, var1, img_w, img_h, resize, thr;
  float* bbox;
  float* conf;
  float* ldm;
  float* rows;
  int cap;
  int* counts;
};

// the 16 head values of anchor i of image b
__device__ __forceinline__ const f32x4* rd_anchor(const RdArgs& a, int b, int i) {
  int l = 0, off = 0;
  if (i >= 2 * a.np[0]) {
    l = 1, off = 2 * a.np[0];
    if (i >= off + 2 * a.np[1]) l = 2, off += 2 * a.np[1];
  }
  const int j = i - off;  // = 2 * pixel + anchor: 16 floats each
  const float* const hp = l == 0 ? a.heads[0] : l == 1 ? a.heads[1] : a.heads[2];  // (selects, not an indexed read of the argument block)
  const int npl = l == 0 ? a.np[0] : l == 1 ? a.np[1] : a.np[2];
  return reinterpret_cast<const f32x4*>(hp + ((size_t)b * npl * 2 + j) * 16);
}

__device__ __forceinline__ void rd_softmax(float l0, float l1, float& p0, float& p1) {
#pragma clang fp contract(off)
  const float m = l0 > l1 ? l0 : l1;
  const float e0 = expf(l0 - m), e1 = expf(l1 - m);
  const float s = e0 + e1;
  p0 = e0 / s;
  p1 = e1 / s;
}

__device__ __forceinline__ void rd_full(const RdArgs& a, size_t row, const f32x4 v[4], float p0, float p1) {
  reinterpret_cast<f32x4*>(a.bbox)[row] = v[0];
  a.conf[row * 2] = p0;
  a.conf[row * 2 + 1] = p1;
  float* const l = a.ldm + row * 10;
  l[0] = v[1][2], l[1] = v[1][3];
#pragma unroll
  for (int e = 0; e < 4; ++e) l[2 + e] = v[2][e], l[6 + e] = v[3][e];
}

// grid (chunks, batch): the full tensors alone, no ordering between anchors
__global__ __launch_bounds__(256) void retina_full_kernel(const RdArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (i >= a.n) return;
  const f32x4* const hp = rd_anchor(a, b, i);
  const f32x4 v[4] = {hp[0], hp[1], hp[2], hp[3]};
  float p0, p1;
  rd_softmax(v[1][0], v[1][1], p0, p1);
  rd_full(a, (size_t)b * a.n + i, v, p0, p1);
}

// grid (batch): the compact rows
__global__ __launch_bounds__(RD_THREADS) void retina_decode_kernel(const RdArgs a) {
#pragma clang fp contract(off)
  __shared__ int wtot[RD_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
  int base = 0;  // passing anchors before this chunk (the same in every thread)
  for (int c0 = 0; c0 < a.n; c0 += RD_THREADS) {
    const int i = c0 + tid;
    const bool valid = i < a.n;
    f32x4 v[4];
    float p0 = 0.f, p1 = 0.f;
    if (valid) {
      const f32x4* const hp = rd_anchor(a, b, i);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = hp[e];
      rd_softmax(v[1][0], v[1][1], p0, p1);
    }
    const bool pass = valid && p1 > a.thr;
    const unsigned long long bal = __ballot(pass);
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wtot[wave] = __popcll(bal);
    __syncthreads();
    int slot = base + before, total = 0;
#pragma unroll
    for (int k = 0; k < RD_WAVES; ++k) {
      const int t = wtot[k];
      if (k < wave) slot += t;
      total += t;
    }
    base += total;
    __syncthreads();  // wtot is rewritten by the next chunk
    if (pass && slot < a.cap) {
      const f32x4 pr = reinterpret_cast<const f32x4*>(a.priors)[i];
      float* const o = a.rows + ((size_t)b * a.cap + slot) * 15;
      const float t0 = v[0][0] * a.var0, t1 = v[0][1] * a.var0;
      const float cx = pr[0] + t0 * pr[2], cy = pr[1] + t1 * pr[3];
      const float u0 = v[0][2] * a.var1, u1 = v[0][3] * a.var1;
      const float sw = pr[2] * expf(u0), sh = pr[3] * expf(u1);
      const float x1 = cx - sw / 2.f, y1 = cy - sh / 2.f;
      const float x2 = sw + x1, y2 = sh + y1;
      o[0] = (x1 * a.img_w) / a.resize;
      o[1] = (y1 * a.img_h) / a.resize;
      o[2] = (x2 * a.img_w) / a.resize;
      o[3] = (y2 * a.img_h) / a.resize;
      o[4] = p1;
      const float pre[10] = {v[1][2], v[1][3], v[2][0], v[2][1], v[2][2], v[2][3], v[3][0], v[3][1], v[3][2], v[3][3]};
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        const float lx = pr[0] + (pre[2 * k] * a.var0) * pr[2], ly = pr[1] + (pre[2 * k + 1] * a.var0) * pr[3];
        o[5 + 2 * k] = (lx * a.img_w) / a.resize;
        o[6 + 2 * k] = (ly * a.img_h) / a.resize;
      }
    }
  }
  if (tid == 0) a.counts[b] = base;
}

}  // namespace

extern "C" int64_t cf_pointwise_packed_elems(int cin, int cout) {
  if (cin <= 0 || cout <= 0 || cin > (1 << 20) || cout > (1 << 20)) return -1;
  return (int64_t)((cout + PW_BN - 1) / PW_BN * PW_BN) * ((cin + PW_BK - 1) / PW_BK * PW_BK);
}

extern "C" int cf_pack_pointwise(const float* w, int cin, int cout, float* wp, cf_stream_t stream) {
  CF_REQUIRE(w && wp, "cf_pack_pointwise: null w/wp");
  const long total = cf_pointwise_packed_elems(cin, cout);
  CF_REQUIRE(total > 0 && (total + 255) / 256 < CF_GRID_LIM, "cf_pack_pointwise: bad dims (cin %d, cout %d)", cin, cout);
  hipLaunchKernelGGL(pack_pointwise_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, wp, cin, cout,
                     (cin + PW_BK - 1) / PW_BK * PW_BK, total);
  CF_CHECK_LAUNCH("cf_pack_pointwise");
  return CF_OK;
}

extern "C" int cf_pointwise(const float* x, int ld_x, const float* wp, const float* bias, const float* res, int ld_res, int batch, int h, int w, int cin,
                            int cout, int step, int act, float* out, int ld_out, cf_stream_t stream) {
  CF_REQUIRE(x && wp && out, "cf_pointwise: null x/wp/out");
  CF_REQUIRE(batch > 0 && h > 0 && w > 0 && cin > 0 && cout > 0 && cin % 4 == 0 && cin <= (1 << 20) && cout <= (1 << 20),
             "cf_pointwise: bad dims (batch %d, %dx%d, cin %d (%% 4 == 0), cout %d)", batch, h, w, cin, cout);
  CF_REQUIRE(step == 1 || step == 2, "cf_pointwise: step %d (1 or 2)", step);
  CF_REQUIRE(act == CF_PW_NONE || act == CF_PW_RELU, "cf_pointwise: act %d (0 none, 1 relu)", act);
  CF_REQUIRE(ld_x >= cin && ld_x % 4 == 0 && ld_out >= cout && (!res || ld_res >= cout),
             "cf_pointwise: pixel strides (x %d, res %d, out %d) smaller than the channel counts (%d, %d) or ld_x %% 4 != 0", ld_x, ld_res, ld_out, cin, cout);
  CF_REQUIRE(cf_aligned16(x) && cf_aligned16(wp), "cf_pointwise: x and wp must be 16-byte aligned");
  const int ho = (h + step - 1) / step, wo = (w + step - 1) / step;
  const long m = (long)batch * ho * wo;
  CF_REQUIRE((long)batch * h * w < CF_GRID_LIM && m < CF_GRID_LIM, "cf_pointwise: tensor too large");
  PwArgs a;
  a.x = x, a.wp = wp, a.bias = bias, a.res = res, a.out = out;
  a.ld_x = ld_x, a.ld_res = ld_res, a.ld_out = ld_out;
  a.m = (int)m, a.h = h, a.w = w, a.ho = ho, a.wo = wo;
  a.cin = cin, a.kp = (cin + PW_BK - 1) / PW_BK * PW_BK, a.cout = cout, a.ntn = (cout + PW_BN - 1) / PW_BN, a.act = act;
  const long grid = ((m + PW_BM - 1) / PW_BM) * a.ntn;
  CF_REQUIRE(grid < CF_GRID_LIM, "cf_pointwise: too many tiles");
  if (step == 2) hipLaunchKernelGGL(pointwise_kernel<2>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(pointwise_kernel<1>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, a);
  CF_CHECK_LAUNCH("cf_pointwise");
  return CF_OK;
}

extern "C" int cf_nearest_add(const float* a, const float* b, int batch, int ha, int wa, int hb, int wb, int c, float* out, cf_stream_t stream) {
  CF_REQUIRE(a && b && out, "cf_nearest_add: null a/b/out");
  CF_REQUIRE(batch > 0 && ha > 0 && wa > 0 && hb > 0 && wb > 0 && c > 0 && c % 4 == 0, "cf_nearest_add: bad dims (batch %d, %dx%d <- %dx%d, c %d: c %% 4 == 0)",
             batch, ha, wa, hb, wb, c);
  CF_REQUIRE(ha < (1 << 24) && wa < (1 << 24) && hb < (1 << 24) && wb < (1 << 24), "cf_nearest_add: an axis of 2^24 or more pixels");
  CF_REQUIRE(cf_aligned16(a) && cf_aligned16(b) && cf_aligned16(out), "cf_nearest_add: tensors must be 16-byte aligned");
  const long total = (long)batch * ha * wa * (c / 4);
  CF_REQUIRE((total + 255) / 256 < CF_GRID_LIM && (long)batch * hb * wb * (c / 4) < CF_GRID_LIM, "cf_nearest_add: tensor too large");
  const float sy = (float)hb / (float)ha, sx = (float)wb / (float)wa;
  hipLaunchKernelGGL(nearest_add_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, b, out, ha, wa, hb, wb, c / 4, sy, sx, total);
  CF_CHECK_LAUNCH("cf_nearest_add");
  return CF_OK;
}

extern "C" int cf_retina_decode(const float* heads0, const float* heads1, const float* heads2, int np0, int np1, int np2, const float* priors, int batch,
                                float var0, float var1, float img_w, float img_h, float resize, float conf_threshold, float* bbox, float* conf, float* ldm,
                                float* rows, int cap, int* counts, cf_stream_t stream) {
  CF_REQUIRE(np0 >= 0 && np1 >= 0 && np2 >= 0 && (long)np0 + np1 + np2 >= 1 && (long)np0 + np1 + np2 < (1 << 28) && batch > 0 && batch <= 65535,
             "cf_retina_decode: bad dims (pixels %d + %d + %d, batch %d (1 .. 65535))", np0, np1, np2, batch);
  CF_REQUIRE((heads0 || !np0) && (heads1 || !np1) && (heads2 || !np2), "cf_retina_decode: null heads of a level with pixels");
  CF_REQUIRE(cf_aligned16(heads0) && cf_aligned16(heads1) && cf_aligned16(heads2), "cf_retina_decode: heads must be 16-byte aligned");
  const bool full = bbox || conf || ldm;
  CF_REQUIRE(full != (rows != nullptr), "cf_retina_decode: one mode per call: the full tensors (bbox, conf, ldm) or the compact rows");
  CF_REQUIRE(!full || (bbox && conf && ldm && cf_aligned16(bbox)), "cf_retina_decode: the full mode needs bbox (16-byte aligned), conf and ldm");
  CF_REQUIRE(!rows || (counts && priors && cf_aligned16(priors) && cap > 0), "cf_retina_decode: the compact mode needs rows, counts, priors (16-byte aligned) and cap > 0");
  CF_REQUIRE(!rows || resize != 0.f, "cf_retina_decode: resize 0");
  const int n = 2 * (np0 + np1 + np2);
  CF_REQUIRE((long)batch * n * 16 < CF_GRID_LIM && (long)batch * cap * 15 < CF_GRID_LIM, "cf_retina_decode: tensor too large");
  RdArgs a;
  a.heads[0] = heads0, a.heads[1] = heads1, a.heads[2] = heads2;
  a.np[0] = np0, a.np[1] = np1, a.np[2] = np2;
  a.priors = priors, a.n = n;
  a.var0 = var0, a.var1 = var1, a.img_w = img_w, a.img_h = img_h, a.resize = resize, a.thr = conf_threshold;
  a.bbox = bbox, a.conf = conf, a.ldm = ldm, a.rows = rows, a.cap = cap, a.counts = counts;
  if (rows) hipLaunchKernelGGL(retina_decode_kernel, dim3(batch), dim3(RD_THREADS), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(retina_full_kernel, dim3((n + 255) / 256, batch), dim3(256), 0, (hipStream_t)stream, a);
  CF_CHECK_LAUNCH("cf_retina_decode");
  return CF_OK;
}
