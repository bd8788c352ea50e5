// Device-side bf16 / matrix-core helpers shared by the kernels: vector typedefs of the MFMA operands, fp32 <-> bf16
// packing, the row reduction of the LayerNorm-shaped kernels, and the MFMA fragments read from LDS through the gfx950
// transposing read ds_read_b64_tr_b16.
// A helper lives here once a second kernel file needs it; what only one file uses stays in that file.
#pragma once
#include "basd_common.h"

namespace basd {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));      // 8 bf16 bit patterns: one A / B operand of a 16x16x32 MFMA
typedef short v4s __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) v4s lds_v4s;
typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// two fp32 -> packed bf16 (round to nearest even): one v_cvt_pk_bf16_f32
__device__ __forceinline__ unsigned int pack_bf16(float a, float b) {
  bf16x2 r = __builtin_convertvector((f32x2){a, b}, bf16x2);
  return *reinterpret_cast<unsigned int*>(&r);
}

// one fp32 -> bf16 bits (round to nearest even), and a pair of them in one word (first value in the low half)
__device__ __forceinline__ unsigned short f32_to_bf16_bits(float v) {
  return __builtin_bit_cast(unsigned short, (__bf16)v);
}
__device__ __forceinline__ unsigned int pack_bf16_bits(float lo, float hi) {
  return (unsigned int)f32_to_bf16_bits(lo) | ((unsigned int)f32_to_bf16_bits(hi) << 16);
}

// Rotary embedding of the attention kernels (attention.hip, attention_long.hip; ROPE): one word = the channel pair
// (2i, 2i + 1) in bf16 -> the pair rotated by (c, s) = (cos, sin) in fp32, rounded to bf16 once
__device__ __forceinline__ unsigned int rope_pair(unsigned int w, float c, float s) {
  const float a = __uint_as_float(w << 16), b = __uint_as_float(w & 0xffff0000u);
  return pack_bf16(fmaf(-b, s, a * c), fmaf(a, s, b * c));
}
// eight channels = four pairs; cs0 = (c, s) of the first two pairs, cs1 of the last two
__device__ __forceinline__ uint4 rope_chunk(const uint4& v, const float4& cs0, const float4& cs1) {
  return make_uint4(rope_pair(v.x, cs0.x, cs0.y), rope_pair(v.y, cs0.z, cs0.w), rope_pair(v.z, cs1.x, cs1.y),
                    rope_pair(v.w, cs1.z, cs1.w));
}

// 8 bf16 of a 16-byte word <-> fp32; the packing goes through __float2bfloat16
__device__ __forceinline__ void unpack8(const uint4& v, float (&f)[8]) {
  const unsigned int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = __uint_as_float(w[i] << 16);
    f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
}
__device__ __forceinline__ unsigned int pack2(float a, float b) {
  __hip_bfloat16 x = __float2bfloat16(a), y = __float2bfloat16(b);    // round to nearest even, NaN safe
  return (unsigned int)(*reinterpret_cast<unsigned short*>(&x)) |
         ((unsigned int)(*reinterpret_cast<unsigned short*>(&y)) << 16);
}
__device__ __forceinline__ uint4 pack8(const float (&f)[8]) {
  return make_uint4(pack2(f[0], f[1]), pack2(f[2], f[3]), pack2(f[4], f[5]), pack2(f[6], f[7]));
}

// ---- row helpers of the LayerNorm-shaped kernels (layernorm.hip, vit_embed.hip): their results are compared bit for
// bit, so both files reduce a row through this one summation order
typedef unsigned int ln_u32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float round_bf16(float a) {
  __hip_bfloat16 x = __float2bfloat16(a);
  return bf16_bits_to_f32(*reinterpret_cast<unsigned short*>(&x));
}

// sum over the G lanes of a row group, result in every lane of the group
template <int G>
__device__ __forceinline__ float group_allsum(float v) {
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, true));    // quad_perm [1,0,3,2]
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, true));    // quad_perm [2,3,0,1]
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xF, 0xF, true));   // row_half_mirror
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xF, 0xF, true));   // row_mirror
  ln_u32x2 r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = __uint_as_float(r.x) + __uint_as_float(r.y);                                                 // rows 0+1, 2+3
  if (G == 64) {
    r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = __uint_as_float(r.x) + __uint_as_float(r.y);
  }
  return v;
}

// Transposing LDS fragment reads from a row-major bf16 tile of row stride ld: two 4-row ds_read_b64_tr_b16.
// 8 rows {row0 .. row0+3, row0+16 .. row0+19} of column col0 + (lane & 15): the k order of two stacked 16-row
// accumulator tiles (4 (lane >> 4) + r in each)
__device__ __forceinline__ bf16x8 tr_split(const unsigned short* tile, int ld, int row0, int col0, int lane) {
  const int li = lane & 15, qq = li >> 2, pp = li & 3;
  const unsigned short* a0 = tile + (row0 + qq) * ld + col0 + 4 * pp;
  const v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)a0);
  const v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)(a0 + 16 * ld));
  return (bf16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}
// 8 CONSECUTIVE rows row0 .. row0+7 of column col0 + (lane & 15)
__device__ __forceinline__ bf16x8 tr_cons(const unsigned short* tile, int ld, int row0, int col0, int lane) {
  const int li = lane & 15, qq = li >> 2, pp = li & 3;
  const unsigned short* a0 = tile + (row0 + qq) * ld + col0 + 4 * pp;
  const v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)a0);
  const v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)(a0 + 4 * ld));
  return (bf16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

}  // namespace basd
