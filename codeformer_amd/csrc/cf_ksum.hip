// Sum of the K parts of the fp32 F(4x4,3x3) K-part form (cf_wf43.hip, "KP") + the epilogue of the convolution kernels + the GroupNorm partials.
//
//   out = epi( (((0 + P0) + P1) + ... + P(V-1)) * acc_scale + bias )          V = cin / 128 parts, ws = [V][B][H][W][cout] fp32
//
// The parts are added in part order starting from zero -- the association of cf_common.h (split-K) -- so the result is a function of the
// layer's shape only.  Epilogue arithmetic: cf_epi_bias / cf_epi_apply of cf_conv_parts.h (NONE, RESIDUAL, SFT with the scalar or the per-image
// weight), float4 NHWC stores.
//
// Work decomposition: a workgroup of 256 threads owns one 16x16 patch of one image x CB channels (CB = 32; 64 when a GroupNorm group has 64
// channels), thread = (pixel p0 = tid / (CB / 4), channel quad tid % (CB / 4)), pixels p0 + k * 1024 / CB: a wave reads whole 128- or 256-byte runs.
// HBM-bound: (V + 1 .. V + 3) x 4 bytes per output.
//
// Statistics (stats_out non-null): ONE fp64 (sum, sum of squares) partial per (image, group, 16x16 patch), the layout the F(4,3) kernel writes and
// cf_groupnorm_finalize2 reads (cf_gn_partial_ptr; nparts = patches per image).  Fixed order: a thread adds its pixels in ascending order in fp64
// (each value and its exact fp64 square), its quad's channels pairwise (c0 + c1) + (c2 + c3) -- with cpg == 2 the two pairs are two groups --,
// __shfl_xor over the lanes with the same quad (distances CB / 4 .. 32), over the adjacent quads of a group (1, 2, .. while 4 * distance < cpg), then
// the four waves in wave order through LDS.
#include "cf_conv_parts.h"

namespace {

struct KSumArgs {
  const float* ws;
  const float* bias;
  const float* res;
  const float* sft_scale;
  const float* sft_w_img;
  float* out;
  double* stats_out;
  float sft_w, acc_scale;
  int parts, batch, h, w, cout;
  int epilogue, stats_cpg;
  int tiles_x, tiles_per_img, nblk;   // nblk: channel blocks per patch = cout / CB
  int nt_out;
};

template <int CB>
__global__ __launch_bounds__(256) void ksum_kernel(const KSumArgs a) {
  constexpr int Q4 = CB / 4;          // quads per pixel
  constexpr int PSTEP = 256 / Q4;     // pixels between the items of a thread
  constexpr int NIT = 256 / PSTEP;    // items per thread
  __shared__ double sred[4][Q4][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bid = blockIdx.x;
  const int nb = bid % a.nblk;
  const int mt = bid / a.nblk;
  const int b = mt / a.tiles_per_img;
  const int rt = mt - b * a.tiles_per_img;
  const int ty = rt / a.tiles_x;
  const int y0 = ty * 16, x0 = (rt - ty * a.tiles_x) * 16;
  const int quad = tid % Q4, p0 = tid / Q4;
  const int n = nb * CB + quad * 4;
  const size_t plane = (size_t)a.batch * a.h * a.w * a.cout;
  f32x4 bias4 = {0.f, 0.f, 0.f, 0.f};
  if (a.bias) bias4 = *reinterpret_cast<const f32x4*>(a.bias + n);
  const float sft_w = a.epilogue == CF_EPI_SFT ? cf_sft_weight(a.sft_w_img, a.sft_w, b) : 0.f;
  const bool nt = a.nt_out != 0;
  double s01 = 0.0, s23 = 0.0, q01 = 0.0, q23 = 0.0;
#pragma unroll 4
  for (int k = 0; k < NIT; ++k) {
    const int p = p0 + k * PSTEP;
    const size_t off = (((size_t)b * a.h + (y0 + (p >> 4))) * a.w + (x0 + (p & 15))) * a.cout + n;
    f32x4 r0 = {0.f, 0.f, 0.f, 0.f}, r1 = {0.f, 0.f, 0.f, 0.f};
    if (a.epilogue == CF_EPI_RESIDUAL || a.epilogue == CF_EPI_SFT) r0 = *reinterpret_cast<const f32x4*>(a.res + off);
    if (a.epilogue == CF_EPI_SFT) r1 = *reinterpret_cast<const f32x4*>(a.sft_scale + off);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < a.parts; ++c) v += *reinterpret_cast<const f32x4*>(a.ws + (size_t)c * plane + off);
    v = cf_epi_bias<true>(v, a.acc_scale, bias4);
    v = cf_epi_apply(v, a.epilogue, r0, r1, sft_w);
    cf_store16(a.out + off, v, nt);
    const double d0 = v[0], d1 = v[1], d2 = v[2], d3 = v[3];
    s01 += d0 + d1;
    s23 += d2 + d3;
    q01 += d0 * d0 + d1 * d1;
    q23 += d2 * d2 + d3 * d3;
  }
  if (!a.stats_out) return;   // (uniform over the launch)
  const int cpg = a.stats_cpg;
  double d0 = s01, q0 = q01, d1 = s23, q1 = q23;
  if (cpg != 2) {
    d0 += d1;
    q0 += q1;
  }
  for (int o = Q4; o < 64; o <<= 1) {
    d0 += __shfl_xor(d0, o, 64);
    q0 += __shfl_xor(q0, o, 64);
    d1 += __shfl_xor(d1, o, 64);
    q1 += __shfl_xor(q1, o, 64);
  }
  for (int o = 1; o * 4 < cpg; o <<= 1) {
    d0 += __shfl_xor(d0, o, 64);
    q0 += __shfl_xor(q0, o, 64);
  }
  if (lane < Q4) {
    sred[wave][lane][0] = d0;
    sred[wave][lane][1] = q0;
    sred[wave][lane][2] = d1;
    sred[wave][lane][3] = q1;
  }
  __syncthreads();
  if (tid < Q4 && (n % cpg) == 0) {   // (cpg == 2: every quad opens a group, and holds a second one)
    double t[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int wv = 0; wv < 4; ++wv)
#pragma unroll
      for (int e = 0; e < 4; ++e) t[e] += sred[wv][tid][e];
    double* op = cf_gn_partial_ptr(a.stats_out, b, a.cout, cpg, n, a.tiles_per_img, rt);
    op[0] = t[0];
    op[1] = t[1];
    if (cpg == 2) {
      op[(size_t)a.tiles_per_img * 2] = t[2];
      op[(size_t)a.tiles_per_img * 2 + 1] = t[3];
    }
  }
}

}  // namespace

// Second launch of the K-part form; cf_wf43_launch has checked the descriptor (dense tensors, hout % 16 == 0, wout % 16 == 0, cout % 128 == 0,
// epilogue none / residual / SFT, stats_cpg a power of two in 2..64 or 0, workspace of split_k planes).
int cf_ksum_launch(const cf_conv_desc* d, hipStream_t stream, const float* sft_w_img) {
  CF_REQUIRE(d->workspace && d->split_k >= 2 && d->hout % 16 == 0 && d->wout % 16 == 0 && d->cout % 64 == 0 && cf_epi_is_quad_triple(d),
             "cf_conv2d(K-part sum): needs a workspace of split_k >= 2 planes, whole 16x16 patches, cout %% 64 == 0, epilogue none / residual / SFT");
  CF_REQUIRE(d->epilogue == CF_EPI_NONE || d->res, "cf_conv2d(K-part sum): the residual / SFT epilogue needs res");
  CF_REQUIRE(d->epilogue != CF_EPI_SFT || d->sft_scale, "cf_conv2d(K-part sum): the SFT epilogue needs sft_scale");
  KSumArgs a;
  a.ws = d->workspace;
  a.bias = d->bias;
  a.res = d->res;
  a.sft_scale = d->sft_scale;
  a.sft_w_img = sft_w_img;
  a.out = d->out;
  a.stats_out = d->stats_out;
  a.sft_w = d->sft_w;
  a.acc_scale = 1.f;   // (fp32 operands: no pack-time weight scale)
  a.parts = d->split_k;
  a.batch = d->batch;
  a.h = d->hout;
  a.w = d->wout;
  a.cout = d->cout;
  a.epilogue = d->epilogue;
  a.stats_cpg = d->stats_cpg > 0 ? d->stats_cpg : 2;
  a.tiles_x = d->wout / 16;
  a.tiles_per_img = a.tiles_x * (d->hout / 16);
  a.nt_out = cf_nt_store((long)d->batch * d->hout * d->wout * d->cout * 4);
  const bool wide = d->stats_out && a.stats_cpg == 64;   // a group must lie in one workgroup
  const int cb = wide ? 64 : 32;
  a.nblk = d->cout / cb;
  const dim3 grid(d->batch * a.tiles_per_img * a.nblk), block(256);
  if (wide) hipLaunchKernelGGL(ksum_kernel<64>, grid, block, 0, stream, a);
  else hipLaunchKernelGGL(ksum_kernel<32>, grid, block, 0, stream, a);
  CF_CHECK_LAUNCH("cf_conv2d(K-part sum)");
  return CF_OK;
}
