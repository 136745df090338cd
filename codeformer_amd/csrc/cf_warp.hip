// Optical-flow warp (basicsr/archs/arch_util.py flow_warp: a mesh grid plus the flow, normalised, through torch's grid_sample) for gfx950,
// with the normalise / un-normalise round trip cancelled: the definition stands at cf_flow_warp in include/codeformer_hip.h.
//
// The position and the four corner weights belong to the pixel, not to the channel: a thread computes them once and reuses them.
//   flow_warp_nchw_kernel  planes [b][c][h][w]: thread = pixel, a loop over a chunk of channels; blockIdx.y walks the chunks so that a
//                          small image still fills the chip.
//   flow_warp_nhwc_kernel  channels-last [b][h][w][c], c % 4 == 0: thread = pixel x float4 of channels (16-byte loads and stores).
// Bandwidth-bound (8 bytes of flow per pixel, one read and one write of the tensor): no LDS, no MFMA.
//
// Addresses: the in-range test runs on the fp32 position BEFORE any float -> int conversion (it is false for NaN, so any float bit pattern
// ends there), every corner is bounds-checked, and a corner that fails is never read: no address is formed from an unchecked value.
#include "cf_common.h"

namespace {

struct WarpArgs {
  const float* x;     // [b][c][h][w], or [b][h][w][c]
  const float* flow;  // [b][h][w][2]: (dx, dy)
  float* out;         // the layout of x
  int batch, c, h, w;
  int interp, padding, align;
  float rx, ry;       // position -> sample coordinate: (n-1) / max(n-1, 1) with align_corners, n / max(n-1, 1) without
  int cpc;            // nchw: channels per chunk
};

// Sample coordinate of position p along an axis of n pixels.  Every operation is a single fp32 one (no contraction).  A NaN stays a NaN
// through every branch (the clamp is written with comparisons, which are false for it).
__device__ __forceinline__ float warp_coord(float p, float ratio, int n, int padding, int align) {
#pragma clang fp contract(off)
  float i = p * ratio;
  if (!align) i = i - 0.5f;
  const float hi = (float)(n - 1);
  if (padding == 2) {  // reflect about [lo, lo + span]: exact, and with no quotient that would have to become an integer
    const float lo = align ? 0.f : -0.5f, span = align ? hi : (float)n;
    if (span > 0.f) {  // (one pixel with align_corners: i is p * 0 already)
      const float a = fabsf(i - lo);
      const float r = fmodf(a, span + span);  // NaN for an infinite position: it samples nothing
      i = (r <= span ? r : (span + span) - r) + lo;
    }
  }
  if (padding != 0) i = i < 0.f ? 0.f : (i > hi ? hi : i);
  return i;
}

// pix[i] = y*W + x of corner i (top-left, top-right, bottom-left, bottom-right) or -1 where it is not read; cw[i] its weight, 0 there.
// Nearest: corner 0 is the rounded point (half to even) with weight 1.
__device__ __forceinline__ void warp_sample(float ix, float iy, int H, int W, int interp, int (&pix)[4], float (&cw)[4]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    pix[i] = -1;
    cw[i] = 0.f;
  }
  if (interp == 1) {
    const float rx = rintf(ix), ry = rintf(iy);
    if (rx >= 0.f && ry >= 0.f && rx <= (float)(W - 1) && ry <= (float)(H - 1)) {  // false for NaN
      pix[0] = (int)ry * W + (int)rx;
      cw[0] = 1.f;
    }
    return;
  }
  if (iy > -1.f && ix > -1.f && iy < (float)H && ix < (float)W) {  // false for NaN; from here on -1 < iy < H, -1 < ix < W
    const float y0f = floorf(iy), x0f = floorf(ix);
    const float lh = iy - y0f, lw = ix - x0f, hh = 1.f - lh, hw = 1.f - lw;
    const int y0 = (int)y0f, x0 = (int)x0f;  // in [-1, H-1] / [-1, W-1]
    const bool top = y0 >= 0, bot = y0 + 1 <= H - 1, left = x0 >= 0, right = x0 + 1 <= W - 1;
    if (top && left) {
      pix[0] = y0 * W + x0;
      cw[0] = hh * hw;
    }
    if (top && right) {
      pix[1] = y0 * W + x0 + 1;
      cw[1] = hh * lw;
    }
    if (bot && left) {
      pix[2] = (y0 + 1) * W + x0;
      cw[2] = lh * hw;
    }
    if (bot && right) {
      pix[3] = (y0 + 1) * W + x0 + 1;
      cw[3] = lh * lw;
    }
  }
}

// The sample of output pixel (y, x) of image b.
__device__ __forceinline__ void warp_pixel(const WarpArgs& a, int b, int y, int x, int (&pix)[4], float (&cw)[4]) {
#pragma clang fp contract(off)
  const float* const f = a.flow + ((size_t)b * a.h * a.w + (size_t)y * a.w + x) * 2;
  const float px = (float)x + f[0], py = (float)y + f[1];
  warp_sample(warp_coord(px, a.rx, a.w, a.padding, a.align), warp_coord(py, a.ry, a.h, a.padding, a.align), a.h, a.w, a.interp, pix, cw);
}

// Four products and three sums, each rounded on its own and in this order, so that both kernels give the same bits.
__device__ __forceinline__ float warp_blend(const float (&cw)[4], float v0, float v1, float v2, float v3) {
#pragma clang fp contract(off)
  return ((cw[0] * v0 + cw[1] * v1) + cw[2] * v2) + cw[3] * v3;
}

__global__ __launch_bounds__(256) void flow_warp_nchw_kernel(const WarpArgs a) {
  const int npix = a.h * a.w, bpi = (npix + 255) / 256;  // blocks per image
  const int b = blockIdx.x / bpi, m = (blockIdx.x - b * bpi) * 256 + threadIdx.x;
  if (m >= npix) return;
  const int y = m / a.w;
  int pix[4];
  float cw[4];
  warp_pixel(a, b, y, m - y * a.w, pix, cw);
  const int c0 = blockIdx.y * a.cpc, c1 = c0 + a.cpc < a.c ? c0 + a.cpc : a.c;
  const float* xp = a.x + ((size_t)b * a.c + c0) * npix;
  float* op = a.out + ((size_t)b * a.c + c0) * npix + m;
  for (int c = c0; c < c1; ++c, xp += npix, op += npix) {
    float v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      v[q] = 0.f;
      if (pix[q] >= 0) v[q] = xp[pix[q]];
    }
    *op = a.interp == 1 ? v[0] : warp_blend(cw, v[0], v[1], v[2], v[3]);
  }
}

__global__ __launch_bounds__(256) void flow_warp_nhwc_kernel(const WarpArgs a, long total) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c4n = a.c / 4, npix = a.h * a.w;
  const int k = (int)(idx % c4n);
  const long p = idx / c4n;  // b * npix + m
  const int b = (int)(p / npix), m = (int)(p - (long)b * npix);
  const int y = m / a.w;
  int pix[4];
  float cw[4];
  warp_pixel(a, b, y, m - y * a.w, pix, cw);
  const f32x4* const xb = reinterpret_cast<const f32x4*>(a.x + (size_t)b * npix * a.c) + k;
  f32x4 v[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    v[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (pix[q] >= 0) v[q] = xb[(size_t)pix[q] * c4n];
  }
  f32x4 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) r[e] = a.interp == 1 ? v[0][e] : warp_blend(cw, v[0][e], v[1][e], v[2][e], v[3][e]);
  reinterpret_cast<f32x4*>(a.out)[idx] = r;
}

}  // namespace

extern "C" int cf_flow_warp(const float* x, const float* flow, float* out, int batch, int c, int h, int w, int interp, int padding,
                            int align_corners, int x_nhwc, cf_stream_t stream) {
  CF_REQUIRE(x && flow && out, "cf_flow_warp: null x/flow/out");
  CF_REQUIRE(batch > 0 && c > 0 && h > 0 && w > 0, "cf_flow_warp: bad dims");
  CF_REQUIRE(interp == 0 || interp == 1, "cf_flow_warp: interp %d (0 bilinear, 1 nearest)", interp);
  CF_REQUIRE(padding >= 0 && padding <= 2, "cf_flow_warp: padding %d (0 zeros, 1 border, 2 reflection)", padding);
  CF_REQUIRE(align_corners == 0 || align_corners == 1, "cf_flow_warp: align_corners %d (0 or 1)", align_corners);
  const long lim = 1L << 31;
  // pixel indices are ints, and the fp32 image bounds and pixel coordinates must be exact
  CF_REQUIRE(h < (1 << 24) && w < (1 << 24) && (long)h * w < lim, "cf_flow_warp: image too large (%dx%d)", h, w);
  WarpArgs a;
  a.x = x, a.flow = flow, a.out = out;
  a.batch = batch, a.c = c, a.h = h, a.w = w;
  a.interp = interp, a.padding = padding, a.align = align_corners;
  const float dw = (float)(w > 1 ? w - 1 : 1), dh = (float)(h > 1 ? h - 1 : 1);
  a.rx = (align_corners ? (float)(w - 1) : (float)w) / dw;  // one fp32 division per launch
  a.ry = (align_corners ? (float)(h - 1) : (float)h) / dh;
  a.cpc = c;
  if (x_nhwc) {
    CF_REQUIRE(c % 4 == 0, "cf_flow_warp: the channels-last form needs c %% 4 == 0 (c %d)", c);
    CF_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)out & 15) == 0, "cf_flow_warp: channels-last x and out must be 16-byte aligned");
    const long total = (long)batch * h * w * (c / 4);
    CF_REQUIRE((total + 255) / 256 < lim, "cf_flow_warp: tensor too large");
    hipLaunchKernelGGL(flow_warp_nhwc_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, total);
  } else {
    const long nbx = (long)batch * (((long)h * w + 255) / 256);
    CF_REQUIRE(nbx < lim, "cf_flow_warp: tensor too large");
    // channel chunks: enough workgroups for a few waves per SIMD of the whole chip, at most 65535 in y
    long chunks = (4096 + nbx - 1) / nbx;
    chunks = chunks < 1 ? 1 : (chunks > c ? c : chunks);
    a.cpc = (int)((c + chunks - 1) / chunks);
    if ((c + a.cpc - 1) / a.cpc > 65535) a.cpc = (c + 65534) / 65535;
    hipLaunchKernelGGL(flow_warp_nchw_kernel, dim3((unsigned)nbx, (unsigned)((c + a.cpc - 1) / a.cpc)), dim3(256), 0, (hipStream_t)stream, a);
  }
  CF_CHECK_LAUNCH("cf_flow_warp");
  return CF_OK;
}
