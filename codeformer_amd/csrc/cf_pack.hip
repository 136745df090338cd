// Every weight packer of the library: fp32 [cout][cin][taps] weights -> the operand layout a kernel family reads.
//
// One kernel, pack_kernel, writes one 32-bit word per thread from three pieces, each written once:
//   value     the real number a slot (slab or transform-domain position, n, c) holds before encoding; zero for n >= cout || c >= cin
//   layout    word index -> slot: (slab, n, the word's one or two channels, hi / lo part)
//   encoding  the value(s) of a word -> its bits
// and an entry point names its combination.  A new layout is a decoder here and a line in its entry point.
//
// Packed weights are cached per parameter version, so nothing here is on a measured path; what matters is that a word never changes:
// tests/test_gpu_pack_digest.py holds the SHA-256 of every layout's output.  The arithmetic of a value -- type, order of additions, where
// the one rounding to fp32 happens -- is part of that.
#include <math.h>

#include "cf_conv_parts.h"
#include "cf_dcn.h"

namespace {

// ---- values ----------------------------------------------------------------------------------------------------------------------------
// The weight tensor and the taps of (n, c); null in the zero padding.
struct Weight {
  const float* w;
  int cout, cin, taps;
  __device__ __forceinline__ const float* at(int n, int c) const { return n < cout && c < cin ? w + ((long)n * cin + c) * taps : nullptr; }
};

// Nearest x2 + 3x3 seen from the low-resolution image: output parity p along an axis reads two source pixels, and folded tap t of the two
// collects the 3x3 taps k0..k1 that land on it: parity 0 -> {0}, {1, 2}; parity 1 -> {0, 1}, {2}.
__device__ __forceinline__ void fold_taps(int parity, int t, int& k0, int& k1) {
  k0 = parity == 0 ? (t == 0 ? 0 : 1) : (t == 0 ? 0 : 2);
  k1 = parity == 0 ? (t == 0 ? 0 : 2) : (t == 0 ? 1 : 2);
}
// Folded tap (ty, tx) of output parity (sy, sx): the sum of its 3x3 taps, ky-major, one rounding per add in T, from zero.
template <class T>
__device__ __forceinline__ T folded_tap(const float* wk, int sy, int sx, int ty, int tx) {
  int ky0, ky1, kx0, kx1;
  fold_taps(sy, ty, ky0, ky1);
  fold_taps(sx, tx, kx0, kx1);
  T v = 0;
  for (int ky = ky0; ky <= ky1; ++ky)
    for (int kx = kx0; kx <= kx1; ++kx) v += wk[ky * 3 + kx];
  return v;
}

// Plain tap `slab` of a 3x3 (taps 9) or of a 1x1 / Linear weight (taps 1, slab 0).  `scale`, here and below: the power of two of a split-half
// layout (the fp32 product of the direct forms is exact), 1 where a layout has none.
struct TapValue {
  Weight g;
  float scale;
  __device__ __forceinline__ float operator()(int slab, int n, int c) const {
    const float* wk = g.at(n, c);
    return wk ? wk[slab] * scale : 0.f;
  }
};
// The direct kernels' nearest-x2 fold, 4 classes x 4 taps: slab = class*4 + tap2, class = (oy&1)*2 + (ox&1), tap2 = ty*2 + tx over the 2x2
// source footprint, summed in fp32.
struct FoldValue {
  Weight g;
  float scale;
  __device__ __forceinline__ float operator()(int slab, int n, int c) const {
    const float* wk = g.at(n, c);
    if (!wk) return 0.f;
    const int cls = slab >> 2, t2 = slab & 3;
    return folded_tap<float>(wk, cls >> 1, cls & 1, t2 >> 1, t2 & 1) * scale;
  }
};
// Stride-2 form (Downsample: zero row / column appended bottom / right, 3x3 stride 2 -- vqgan_arch.py:117-126): the input is read as the
// space-to-depth tensor X[i][j][(p, q, c)] = x[2i + p][2j + q][c] (4C channels, no copy: see the row-pair addressing of the gather) and
// the convolution becomes a 2x2 stride-1 one, out[i][j] = sum_{ty,tx} W'[ty][tx] . X[i + ty][j + tx], with
// W'[ty][tx][(p, q, c)] = w[2ty + p][2tx + q][c] where that tap exists and 0 elsewhere (7 of the 16 blocks are zero).
struct Stride2Value {
  Weight g;
  float scale;
  __device__ __forceinline__ float operator()(int tap, int n, int c4) const {
    if (c4 >= 4 * g.cin) return 0.f;
    const int p = c4 / (2 * g.cin), q = (c4 / g.cin) & 1;
    const int ky = 2 * (tap >> 1) + p, kx = 2 * (tap & 1) + q;
    const float* wk = g.at(n, c4 % g.cin);
    return wk && ky <= 2 && kx <= 2 ? wk[ky * 3 + kx] * scale : 0.f;
  }
};
// Winograd F(2x2,3x3): U = G g G^T at pos = xi*4 + nu, G's rows = g0, (g0 + g1 + g2)/2, (g0 - g1 + g2)/2, g2; fp64, rounded once.
struct F23Value {
  Weight g;
  float scale;
  __device__ __forceinline__ float operator()(int pos, int n, int c) const {
    const float* w = g.at(n, c);
    if (!w) return 0.f;
    const int xi = pos >> 2, nu = pos & 3;
    double row[3];  // row xi of G g: combination of the three kernel rows
#pragma unroll
    for (int x = 0; x < 3; ++x) {
      const double g0 = w[x], g1 = w[3 + x], g2 = w[6 + x];
      row[x] = xi == 0 ? g0 : (xi == 1 ? 0.5 * (g0 + g1 + g2) : (xi == 2 ? 0.5 * (g0 - g1 + g2) : g2));
    }
    const double u = nu == 0 ? row[0] : (nu == 1 ? 0.5 * (row[0] + row[1] + row[2]) : (nu == 2 ? 0.5 * (row[0] - row[1] + row[2]) : row[2]));
    return (float)(u * (double)scale);
  }
};
// Winograd F(4x4,3x3): U' = G' g G'^T at pos = xi*6 + nu; fp64 row sums, then the column sum, rounded once.
struct F43Value {
  Weight g;
  float scale;
  __device__ __forceinline__ float operator()(int pos, int n, int c) const {
    const float* w = g.at(n, c);
    if (!w) return 0.f;
    // rows of G' = D^-1 G for the points (0, 1/2, -1/2, 2, -2, inf), D = diag(1/4, 1/4, 1/4, 1/2, 1/2, 1/4)
    const double Gm[6][3] = {{4.0, 0.0, 0.0},           {-32.0 / 15.0, -16.0 / 15.0, -8.0 / 15.0}, {-32.0 / 15.0, 16.0 / 15.0, -8.0 / 15.0},
                             {1.0 / 15.0, 2.0 / 15.0, 4.0 / 15.0}, {1.0 / 15.0, -2.0 / 15.0, 4.0 / 15.0},  {0.0, 0.0, 4.0}};
    const int xi = pos / 6, nu = pos % 6;
    double u = 0.0;
#pragma unroll
    for (int y = 0; y < 3; ++y) {
      double rowv = 0.0;
#pragma unroll
      for (int x = 0; x < 3; ++x) rowv += (double)w[y * 3 + x] * Gm[nu][x];
      u += Gm[xi][y] * rowv;
    }
    return (float)(u * (double)scale);
  }
};
// The sub-pixel F(4x4,2x2) form: U_p = G42 g_p G42^T at slab = phase*25 + xi*5 + nu, phase p = 2 a + b the output parity, g_p the 3x3 taps
// folded to the 2x2 that parity sees (fp64 throughout, rounded once).
struct F42Value {
  Weight g;
  __device__ __forceinline__ float operator()(int slab, int n, int c) const {
    const float* w = g.at(n, c);
    if (!w) return 0.f;
    const double G[5][2] = {{1.0, 0.0}, {-2.0 / 9.0, 2.0 / 9.0}, {-8.0 / 9.0, -4.0 / 9.0}, {1.0 / 9.0, 2.0 / 9.0}, {0.0, 1.0}};
    const int pos = slab % 25, phase = slab / 25;
    const int xi = pos / 5, nu = pos % 5, pa = phase >> 1, pb = phase & 1;
    double f[2][2];
#pragma unroll
    for (int y = 0; y < 2; ++y)
#pragma unroll
      for (int x = 0; x < 2; ++x) f[y][x] = folded_tap<double>(w, pa, pb, y, x);
    double u = 0.0;
#pragma unroll
    for (int y = 0; y < 2; ++y) u += G[xi][y] * (f[y][0] * G[nu][0] + f[y][1] * G[nu][1]);
    return (float)u;
  }
};

// ---- layouts ---------------------------------------------------------------------------------------------------------------------------
// c is the word's channel, or the first of its two (c, c + 1: the 16-bit encodings); part: 0 = hi, 1 = lo half of the split pair.
struct Slot { int slab, n, c, part; };

// Rows: [slab][cin_pad/KC][cout_pad][KC channels], CPW channels per word.  fp32: KC = 16 (CF_BK) words; bf16 / IEEE half: KC = 32 values,
// two per word.
template <int KC, int CPW>
struct Rows {
  int cout_pad, nchunks;
  __device__ __forceinline__ Slot operator()(long i) const {
    constexpr int W = KC / CPW;
    const int k = (int)(i % W);
    long r = i / W;
    const int n = (int)(r % cout_pad);
    r /= cout_pad;
    return {(int)(r / nchunks), n, (int)(r % nchunks) * KC + k * CPW, 0};
  }
};
// Split-half rows of cf_split.hip: [class][cin/32][tap][cout_pad][32 words] (class = 1 plain / 4 folded / 1 stride-2 form with 4 cin
// channels / 1 for 1x1 with one tap): words 0..15 = hi halves of channels (2k, 2k+1), 16..31 = lo.  slab = class*4 + tap (class = 0 when
// not folded).
struct SplitRows {
  int cout_pad, nchunks, taps;
  __device__ __forceinline__ Slot operator()(long i) const {
    const int k2 = (int)(i & 15), part = (int)((i >> 4) & 1);
    long r = i >> 5;
    const int n = (int)(r % cout_pad);
    r /= cout_pad;
    const int tap = (int)(r % taps);
    r /= taps;
    return {(int)(r / nchunks) * 4 + tap, n, (int)(r % nchunks) * 32 + k2 * 2, part};
  }
};
// Fragments of the 32-row MFMA (v_mfma_f32_32x32x16_f16 B operand): [pos][cin_pad/16][cout_pad/32][part: hi, lo][lane 64][4 words]; a
// lane's 16 bytes are the 8 halves of [n = tile*32 + (lane&31)][c = chunk*16 + (lane>>5)*8 + 0..7].  F(2,3) split-half, F(2,3) with bf16 in
// the hi slot, and Linear ([K/16][N/32].., one position).
struct Frag32 {
  int ntiles, nchunks;
  __device__ __forceinline__ Slot operator()(long i) const {
    const int e = (int)(i & 3), ln = (int)((i >> 2) & 63), part = (int)((i >> 8) & 1);
    long r = i >> 9;
    const int n = (int)(r % ntiles) * 32 + (ln & 31);
    r /= ntiles;
    return {(int)(r / nchunks), n, (int)(r % nchunks) * CF_BK + (ln >> 5) * 8 + e * 2, part};
  }
};
// The fp32 F(2,3) fragment (v_mfma_f32_32x32x2_f32): [pos][cin_pad/16][cout_pad/32][kg 2][lane 64][4]: element =
// [n = tile*32 + (lane&31)][c = chunk*16 + kg*8 + (lane>>5)*4 + e].
struct Frag32F {
  int ntiles, nchunks;
  __device__ __forceinline__ Slot operator()(long i) const {
    const int e = (int)(i & 3), ln = (int)((i >> 2) & 63), kg = (int)((i >> 8) & 1);
    long r = i >> 9;
    const int n = (int)(r % ntiles) * 32 + (ln & 31);
    r /= ntiles;
    return {(int)(r / nchunks), n, (int)(r % nchunks) * CF_BK + kg * 8 + (ln >> 5) * 4 + e, 0};
  }
};
// Fragments of the 16-row MFMAs on KS = 16- or 32-channel slabs: [pos][cin_pad/KS][cout_pad/16][lane 64][KS/4 words], n = block*16 + (lane&15).
//   HALVES (v_mfma_f32_16x16x16_f16 / 16x16x32_f16 B operand, hi | lo in one dwordx4 / pair of them): a lane's words are [hi | lo] of
//          c = chunk*KS + (lane>>4)*KS/4 + 0..KS/4-1;
//   fp32   (v_mfma_f32_16x16x4_f32): word j = [n][c = chunk*KS + 4 j + (lane>>4)].
// F(4,3) in both operand types; the four F(4,2) phases (fp32, KS = 32, pos = phase*25 + xi*5 + nu).
template <bool HALVES>
struct Frag16 {
  int ks, ntiles, nchunks;
  __device__ __forceinline__ Slot operator()(long i) const {
    const int wpl = ks / 4, j = (int)(i % wpl), ln = (int)((i / wpl) & 63);
    long r = i / (wpl * 64);
    const int n = (int)(r % ntiles) * 16 + (ln & 15);
    r /= ntiles;
    const int slab = (int)(r / nchunks), c0 = (int)(r % nchunks) * ks;
    if (HALVES) return {slab, n, c0 + (ln >> 4) * wpl + (j % (wpl / 2)) * 2, j / (wpl / 2)};
    return {slab, n, c0 + 4 * j + (ln >> 4), 0};
  }
};

// ---- encodings -------------------------------------------------------------------------------------------------------------------------
// One fp32 word, or two 16-bit values (channel c in the low half): bf16 or IEEE half, round to nearest even; the split pair hi = f16(v),
// lo = f16(v - hi), of which a word holds the part its slot names; bf16 in the hi slot with a zero lo slot (the single-operand bf16 form of
// cf_wsplit.hip; its IEEE-half form reads the hi slot of the split packing as it is).
enum { ENC_F32, ENC_BF16, ENC_F16, ENC_SPLIT, ENC_BF16_HI };

__device__ __forceinline__ unsigned bf16_bits(float v) {
  unsigned u = __builtin_bit_cast(unsigned, v);
  u += 0x7fffu + ((u >> 16) & 1u);
  return u >> 16;
}
__device__ __forceinline__ unsigned f16_bits(float v) { return __builtin_bit_cast(unsigned short, (_Float16)v); }
template <int ENC>
__device__ __forceinline__ unsigned half_bits(float v, int part) {
  if (ENC == ENC_BF16) return bf16_bits(v);
  if (ENC == ENC_BF16_HI) return bf16_bits(part ? 0.f : v);
  if (ENC == ENC_F16) return f16_bits(v);
  const _Float16 hi = (_Float16)v;
  return part ? f16_bits(v - (float)hi) : f16_bits(v);
}

template <int ENC, class Value, class Layout>
__global__ void pack_kernel(Value value, Layout layout, unsigned* __restrict__ packed, long total) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const Slot s = layout(i);
  const float v = value(s.slab, s.n, s.c);
  if (ENC == ENC_F32) {
    packed[i] = __builtin_bit_cast(unsigned, v);
    return;
  }
  packed[i] = half_bits<ENC>(v, s.part) | half_bits<ENC>(value(s.slab, s.n, s.c + 1), s.part) << 16;
}

template <int ENC, class Value, class Layout>
int pack(const char* name, Value value, Layout layout, void* packed, long words, cf_stream_t stream) {
  hipLaunchKernelGGL((pack_kernel<ENC, Value, Layout>), dim3((unsigned)((words + 255) / 256)), dim3(256), 0, (hipStream_t)stream, value, layout,
                     reinterpret_cast<unsigned*>(packed), words);
  CF_CHECK_LAUNCH(name);
  return CF_OK;
}

// The padding rule of most layouts: whole K slabs of `kmul` channels and whole N tiles of `nmul`, no less than the weight has.
bool pads(int cout, int cin, int cout_pad, int cin_pad, int kmul, int nmul) {
  return cin_pad % kmul == 0 && cin_pad >= cin && cout_pad >= cout && cout_pad % nmul == 0;
}

// What the entry points check first, in this order: the pointers, the layout's padding rule (`padded`: evaluated by the caller; `rule`: its
// wording where the message spells one out), the scale of a scaled layout.
int pack_check(const char* name, const void* w, const void* packed, bool padded, int cout, int cin, int cout_pad, int cin_pad, float scale = 1.f,
               const char* rule = "") {
  CF_REQUIRE(w && packed, "%s: null pointer", name);
  CF_REQUIRE(padded, "%s: bad padding cin %d->%d cout %d->%d%s", name, cin, cin_pad, cout, cout_pad, rule);
  int ex = 0;
  CF_REQUIRE(scale > 0.f && frexpf(scale, &ex) == 0.5f, "%s: scale %g is not a power of two", name, (double)scale);
  return CF_OK;
}

// fp32 rows: the plain taps, or (fold) the 16 folded slabs of the nearest-x2 + 3x3 convolution
int pack_f32(const char* name, const float* w, int cout, int cin, int taps, int fold, int cout_pad, int cin_pad, float* packed, cf_stream_t stream) {
  if (const int e = pack_check(name, w, packed, pads(cout, cin, cout_pad, cin_pad, CF_BK, 32), cout, cin, cout_pad, cin_pad))
    return e;
  CF_REQUIRE(taps == 1 || taps == 9, "%s: taps must be 1 or 9 (got %d)", name, taps);
  const Weight g{w, cout, cin, taps};
  const Rows<CF_BK, 1> rows{cout_pad, cin_pad / CF_BK};
  const long words = (long)(fold ? 16 : taps) * cin_pad * cout_pad;
  return fold ? pack<ENC_F32>(name, FoldValue{g, 1.f}, rows, packed, words, stream) : pack<ENC_F32>(name, TapValue{g, 1.f}, rows, packed, words, stream);
}

// 16-bit rows, bf16 or (F16) IEEE half
template <int ENC>
int pack_16(const float* w, int cout, int cin, int fold, int cout_pad, int cin_pad, void* packed, cf_stream_t stream) {
  if (const int e = pack_check("cf_pack_conv_weight_bf16/f16", w, packed, pads(cout, cin, cout_pad, cin_pad, 32, ENC == ENC_F16 ? 32 : 64), cout, cin, cout_pad, cin_pad))
    return e;
  const Weight g{w, cout, cin, 9};
  const Rows<32, 2> rows{cout_pad, cin_pad / 32};
  const long words = (long)(fold ? 16 : 9) * cin_pad * cout_pad / 2;
  return fold ? pack<ENC>("cf_pack_conv_weight_bf16", FoldValue{g, 1.f}, rows, packed, words, stream)
              : pack<ENC>("cf_pack_conv_weight_bf16", TapValue{g, 1.f}, rows, packed, words, stream);
}

// F(2,3) on 16-bit operands: the split pair, or bf16 in the hi slot
template <int ENC>
int pack_winograd_halves(const float* w, int cout, int cin, int cout_pad, int cin_pad, float scale, void* packed, cf_stream_t stream) {
  const char* name = "cf_pack_conv_weight_winograd_f16x2";
  if (const int e = pack_check(name, w, packed, pads(cout, cin, cout_pad, cin_pad, CF_BK, 64), cout, cin, cout_pad, cin_pad, scale))
    return e;
  return pack<ENC>(name, F23Value{{w, cout, cin, 9}, scale}, Frag32{cout_pad / 32, cin_pad / CF_BK}, packed, 16L * cin_pad * cout_pad, stream);
}

// F(4,3): the layout follows the form cf_conv2d will run (cf_wf43_k32): 32-channel slabs for the 16-wave form where cin allows
template <int ENC>
int pack_winograd43(const char* name, const float* w, int cout, int cin, int cout_pad, int cin_pad, float scale, void* packed, cf_stream_t stream) {
  if (const int e = pack_check(name, w, packed, pads(cout, cin, cout_pad, cin_pad, CF_BK, 64), cout, cin, cout_pad, cin_pad, scale))
    return e;
  const int ks = cf_wf43_k32(cout_pad, cin_pad) ? 32 : CF_BK;
  return pack<ENC>(name, F43Value{{w, cout, cin, 9}, scale}, Frag16<ENC == ENC_SPLIT>{ks, cout_pad / 16, cin_pad / ks}, packed, 36L * cin_pad * cout_pad, stream);
}

}  // namespace

extern "C" int64_t cf_packed_weight_elems(int cin_pad, int taps, int cout_pad) {
  return (int64_t)taps * cin_pad * cout_pad;
}

extern "C" int cf_pack_conv_weight(const float* w, int cout, int cin, int taps, int cout_pad, int cin_pad,
                                   float* packed, cf_stream_t stream) {
  return pack_f32("cf_pack_conv_weight", w, cout, cin, taps, 0, cout_pad, cin_pad, packed, stream);
}

extern "C" int cf_pack_conv_weight_up2x(const float* w, int cout, int cin, int cout_pad, int cin_pad, float* packed,
                                        cf_stream_t stream) {
  return pack_f32("cf_pack_conv_weight_up2x", w, cout, cin, 9, 1, cout_pad, cin_pad, packed, stream);
}

extern "C" int cf_pack_conv_weight_bf16(const float* w, int cout, int cin, int taps, int cout_pad, int cin_pad, void* packed,
                                        cf_stream_t stream) {
  CF_REQUIRE(taps == 9, "cf_pack_conv_weight_bf16: the bf16 path covers 3x3 convolutions (taps=9)");
  return pack_16<ENC_BF16>(w, cout, cin, 0, cout_pad, cin_pad, packed, stream);
}

extern "C" int cf_pack_conv_weight_up2x_bf16(const float* w, int cout, int cin, int cout_pad, int cin_pad, void* packed,
                                             cf_stream_t stream) {
  return pack_16<ENC_BF16>(w, cout, cin, 1, cout_pad, cin_pad, packed, stream);
}

extern "C" int cf_pack_conv_weight_f16(const float* w, int cout, int cin, int taps, int cout_pad, int cin_pad, void* packed,
                                       cf_stream_t stream) {
  CF_REQUIRE(taps == 9, "cf_pack_conv_weight_f16: 3x3 weights only (taps=%d)", taps);
  return pack_16<ENC_F16>(w, cout, cin, 0, cout_pad, cin_pad, packed, stream);
}

extern "C" int cf_pack_conv_weight_up2x_f16(const float* w, int cout, int cin, int cout_pad, int cin_pad, void* packed,
                                            cf_stream_t stream) {
  return pack_16<ENC_F16>(w, cout, cin, 1, cout_pad, cin_pad, packed, stream);
}

extern "C" int cf_pack_conv_weight_f16x2(const float* w, int cout, int cin, int up2x, int cout_pad, int cin_pad, float scale,
                                         void* packed, cf_stream_t stream) {
  const char* name = "cf_pack_conv_weight_f16x2";
  const int kpad = up2x == 2 ? 4 * cin_pad : cin_pad;  // (the stride-2 form's K axis is the space-to-depth one)
  if (const int e = pack_check(name, w, packed, kpad % 32 == 0 && pads(cout, cin, cout_pad, cin_pad, 1, 64), cout, cin, cout_pad, cin_pad, scale))
    return e;
  CF_REQUIRE(up2x >= 0 && up2x <= 3, "cf_pack_conv_weight_f16x2: form %d (0 plain 3x3, 1 nearest-x2 folded, 2 stride 2, 3 1x1)", up2x);
  CF_REQUIRE(up2x != 2 || (cin_pad == cin && cin % 16 == 0), "cf_pack_conv_weight_f16x2: the stride-2 form needs cin %% 16 == 0, unpadded");
  const long words = (long)(up2x == 3 ? 1 : up2x ? 16 : 9) * cin_pad * cout_pad;  // two halves per word, hi + lo per channel: one word per weight
  const Weight g{w, cout, cin, up2x == 3 ? 1 : 9};
  const SplitRows rows{cout_pad, kpad / 32, up2x == 3 ? 1 : up2x ? 4 : 9};
  if (up2x == 1) return pack<ENC_SPLIT>(name, FoldValue{g, scale}, rows, packed, words, stream);
  if (up2x == 2) return pack<ENC_SPLIT>(name, Stride2Value{g, scale}, rows, packed, words, stream);
  return pack<ENC_SPLIT>(name, TapValue{g, scale}, rows, packed, words, stream);
}

extern "C" int cf_pack_linear_weight_f16x2(const float* w, int n, int k, float scale, void* packed, cf_stream_t stream) {
  const char* name = "cf_pack_linear_weight_f16x2";
  if (const int e = pack_check(name, w, packed, true, n, k, n, k, scale)) return e;  // (no padding in this layout)
  CF_REQUIRE(n > 0 && k > 0 && n % 64 == 0 && k % 128 == 0, "cf_pack_linear_weight_f16x2: N %d must be a multiple of 64, K %d of 128", n, k);
  return pack<ENC_SPLIT>(name, TapValue{{w, n, k, 1}, scale}, Frag32{n / 32, k / CF_BK}, packed, (long)n * k, stream);  // hi + lo half per weight
}

extern "C" int cf_pack_conv_weight_winograd(const float* w, int cout, int cin, int cout_pad, int cin_pad, float* packed,
                                            cf_stream_t stream) {
  const char* name = "cf_pack_conv_weight_winograd";
  if (const int e = pack_check(name, w, packed, pads(cout, cin, cout_pad, cin_pad, CF_BK, 64), cout, cin, cout_pad, cin_pad))
    return e;
  return pack<ENC_F32>(name, F23Value{{w, cout, cin, 9}, 1.f}, Frag32F{cout_pad / 32, cin_pad / CF_BK}, packed, 16L * cin_pad * cout_pad, stream);
}

extern "C" int cf_pack_conv_weight_winograd_f16x2(const float* w, int cout, int cin, int cout_pad, int cin_pad, float scale, void* packed,
                                                  cf_stream_t stream) {
  return pack_winograd_halves<ENC_SPLIT>(w, cout, cin, cout_pad, cin_pad, scale, packed, stream);
}

extern "C" int cf_pack_conv_weight_winograd_bf16(const float* w, int cout, int cin, int cout_pad, int cin_pad, float scale, void* packed,
                                                 cf_stream_t stream) {
  return pack_winograd_halves<ENC_BF16_HI>(w, cout, cin, cout_pad, cin_pad, scale, packed, stream);
}

extern "C" int cf_pack_conv_weight_winograd43_f16x2(const float* w, int cout, int cin, int cout_pad, int cin_pad, float scale, void* packed,
                                                    cf_stream_t stream) {
  return pack_winograd43<ENC_SPLIT>("cf_pack_conv_weight_winograd43_f16x2", w, cout, cin, cout_pad, cin_pad, scale, packed, stream);
}

extern "C" int cf_pack_conv_weight_winograd43(const float* w, int cout, int cin, int cout_pad, int cin_pad, void* packed, cf_stream_t stream) {
  return pack_winograd43<ENC_F32>("cf_pack_conv_weight_winograd43", w, cout, cin, cout_pad, cin_pad, 1.f, packed, stream);
}

extern "C" int cf_pack_conv_weight_winograd42_up(const float* w, int cout, int cin, int cout_pad, int cin_pad, void* packed, cf_stream_t stream) {
  const char* name = "cf_pack_conv_weight_winograd42_up";
  if (const int e = pack_check(name, w, packed, cin_pad == cin && cout_pad == cout && cin > 0 && cout > 0 && cin % 32 == 0 && cout % 128 == 0, cout, cin, cout_pad,
                               cin_pad, 1.f, " (cin % 32 == 0, cout % 128 == 0, no padding)"))
    return e;
  CF_REQUIRE(cf_wf43_k32(cout, cin), "cf_pack_conv_weight_winograd42_up: the sub-pixel form runs on 32-channel slabs (CF_F43_WIDE=k16 is set)");
  // fp32 words: 4 phases x 25 positions
  return pack<ENC_F32>(name, F42Value{{w, cout, cin, 9}}, Frag16<false>{32, cout / 16, cin / 32}, packed, 100L * cin * cout, stream);
}

// Deformable convolution (cf_dcn.hip): the fp32 rows of each group, [group][tap][cin_g/16][cout_pad_g][16] with cout_pad_g whole 64-wide
// channel tiles of the group (cf_dcn_cout_pad); any tap count up to CF_DCN_MAX_TAPS.
extern "C" int cf_pack_deform_conv_weight(const float* w, int cout, int cin, int taps, int groups, float* packed, cf_stream_t stream) {
  const char* name = "cf_pack_deform_conv_weight";
  CF_REQUIRE(w && packed, "%s: null pointer", name);
  CF_REQUIRE(cout > 0 && cin > 0 && groups > 0 && cin % groups == 0 && cout % groups == 0, "%s: groups %d must divide cin %d and cout %d", name, groups, cin, cout);
  CF_REQUIRE((cin / groups) % CF_BK == 0, "%s: cin per group %d must be a multiple of %d", name, cin / groups, CF_BK);
  CF_REQUIRE(taps >= 1 && taps <= CF_DCN_MAX_TAPS, "%s: taps must be in [1, %d] (got %d)", name, CF_DCN_MAX_TAPS, taps);
  const int cout_g = cout / groups, cin_g = cin / groups, cout_pad_g = cf_dcn_cout_pad(cout_g);
  const long words = (long)taps * cin_g * cout_pad_g;
  for (int g = 0; g < groups; ++g) {
    const Weight wg{w + (long)g * cout_g * cin_g * taps, cout_g, cin_g, taps};
    if (const int e = pack<ENC_F32>(name, TapValue{wg, 1.f}, Rows<CF_BK, 1>{cout_pad_g, cin_g / CF_BK}, packed + g * words, words, stream)) return e;
  }
  return CF_OK;
}
