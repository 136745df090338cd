// Deformable convolution (cf_dcn.hip): what its launcher and its weight packer (cf_pack.hip) both need to know.
#pragma once

constexpr int CF_DCN_BM = 64;         // output pixels of one image per workgroup tile (a 4 x 16 patch)
constexpr int CF_DCN_BN = 64;         // output channels of one group per workgroup tile
constexpr int CF_DCN_MAX_TAPS = 49;   // largest kh * kw the MFMA route takes

// A group's output channels are padded to whole N tiles: the packed weight is [group][tap][cin_g/16][cout_pad_g][16].
inline int cf_dcn_cout_pad(int cout_g) { return (cout_g + CF_DCN_BN - 1) / CF_DCN_BN * CF_DCN_BN; }

// The routing rule of the MFMA kernel (ops.deform_conv2d_route states the same one): a float4 of channels lies in one deformable group,
// a 16-channel K slab in one group, one image is addressed by a 31-bit byte offset (the kernel reads it through a buffer descriptor), and
// cin < 2^16 (the kernel divides a channel index by cin / dg with one multiplication, exact while the product of the two is below 2^32).
inline bool cf_dcn_mfma_covers(int cin, int cout, int hin, int win, int taps, int groups, int dg) {
  return groups > 0 && dg > 0 && cin % groups == 0 && cout % groups == 0 && cin % dg == 0 && (cin / dg) % 4 == 0 && (cin / groups) % 16 == 0 &&
         taps >= 1 && taps <= CF_DCN_MAX_TAPS && cin < 65536 && (long)hin * win * cin * 4 < (1L << 31);
}
