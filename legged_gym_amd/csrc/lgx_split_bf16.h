// The split-bf16 arithmetic of the "f32-accurate" kernels and the pre-split operand image, stated
// once (lgx_gemm_split / _x3p / _tn, lgx_mlp_x3, the Adam step's limb mirrors in lgx_ppo).
//
// Every f32 operand is split, round-to-nearest-even, into three bf16 limbs
//   x = x0 + x1 + x2 + e,   x0 = bf16(x), x1 = bf16(x - x0), x2 = bf16(x - x0 - x1),
//   |x1| <= 2^-8 |x0|, |x2| <= 2^-8 |x1|, |e| <= 2^-24 |x|   (both subtractions are exact in f32),
// and a * b is evaluated as the six limb products of order <= 2 on v_mfma_f32_32x32x16_bf16, each
// exact in the f32 accumulator.  The dropped terms (a1 b2, a2 b1, a2 b2) are <= 2.04 * 2^-24 |a b|
// and the accumulator's roundings of one product <= 5 * 2^-24 |a b|: a single product is within
// 2^-21 |a b| (tests/split_products_ref.py derives it; tests/test_gpu_split_products.py holds every
// kernel that calls lgx_split_mma to it, and their dense sums to 1.25x the exact-f32 MFMA's error).
// 6 MFMAs at 1/16 the cost of the f32 MFMA's 8 per 16 k: a 2.67x higher arithmetic roof.
//
// The layout part is plain C++ (tests/test_split_bf16_host.py compiles it with the host compiler).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define LGX_HD __host__ __device__
#else
#define LGX_HD
#endif

// Pre-split GEMM operand (lgx_split_bf16, the Adam limb mirrors; read by gemm_nt_x3_kernel and
// gemm_nt_x3p_kernel): the LDS image of every 128-column x 32-k block,
// [n / 128][k / 32][limb][n % 128][32 k], the four 16-byte k-chunks of a 64-byte row stored at
// chunk ^ ((n >> 2) & 3) so the 32x32x16 fragment reads (ds_read_b128) are bank-conflict free.
constexpr int LGX_X3_BN = 128, LGX_X3_BK = 32;         // columns and k of a block
constexpr int LGX_X3_PLANE = LGX_X3_BN * LGX_X3_BK;    // bf16 per limb plane of a block
constexpr int LGX_X3_BLOCK = 3 * LGX_X3_PLANE;         // bf16 per block (three planes)
constexpr int LGX_X3_UNIT = 3 * LGX_X3_BK;             // bf16 per (row, 32-k block)
// Offset (bf16 units) of element (n, k) limb `limb` within one batch entry; kb = ceil(K / 32).
// Limb l sits l planes after limb 0.
LGX_HD inline int64_t x3_limb_off(int n, int k, int limb, int kb) {
  const int nn = n & (LGX_X3_BN - 1), kk = k & (LGX_X3_BK - 1);
  return ((int64_t)((n >> 7) * kb + (k >> 5)) * 3 + limb) * LGX_X3_PLANE + nn * LGX_X3_BK +
         ((((kk >> 3) ^ ((nn >> 2) & 3))) << 3) + (kk & 7);
}
// bf16 elements of one batch entry (lgx_split_bf16_elems); n % 128 == 0
LGX_HD inline int64_t x3_image_elems(int n, int k) {
  return (int64_t)n * ((k + LGX_X3_BK - 1) / LGX_X3_BK) * LGX_X3_UNIT;
}

#ifdef __HIPCC__
typedef __bf16 lgx_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 lgx_bf16x2 __attribute__((ext_vector_type(2)));
typedef float lgx_fx2 __attribute__((ext_vector_type(2)));
typedef float lgx_f32x16 __attribute__((ext_vector_type(16)));

// The three limbs of two f32 values, packed (low half = first value): v_cvt_pk_bf16_f32 and exact
// f32 subtractions.  (Round 6 measured the residuals as v_dot2c_f32_bf16 with a -1 in the limb's
// half - 7 VALU per pair instead of 11, bitwise the same limbs - and the PPO update was slower,
// 10.83 vs 10.46 ms, same box, alternated: the dot instruction does not issue at the rate of the
// shift / subtract it replaces.)
__device__ __forceinline__ void lgx_split2(float x0, float x1, uint32_t& l0, uint32_t& l1, uint32_t& l2) {
  l0 = __builtin_bit_cast(uint32_t, __builtin_convertvector((lgx_fx2){x0, x1}, lgx_bf16x2));
  float r0 = x0 - __uint_as_float(l0 << 16), r1 = x1 - __uint_as_float(l0 & 0xffff0000u);
  l1 = __builtin_bit_cast(uint32_t, __builtin_convertvector((lgx_fx2){r0, r1}, lgx_bf16x2));
  r0 -= __uint_as_float(l1 << 16);
  r1 -= __uint_as_float(l1 & 0xffff0000u);
  l2 = __builtin_bit_cast(uint32_t, __builtin_convertvector((lgx_fx2){r0, r1}, lgx_bf16x2));
}
// The limbs of one value: the low halves of lgx_split2(x, 0), through the same conversion
__device__ __forceinline__ void lgx_split1(float x, uint16_t& l0, uint16_t& l1, uint16_t& l2) {
  auto rne = [](float v) {
    return (uint16_t)__builtin_bit_cast(uint32_t, __builtin_convertvector((lgx_fx2){v, 0.f}, lgx_bf16x2));
  };
  const uint16_t p0 = rne(x);
  const float r = x - __uint_as_float((uint32_t)p0 << 16);
  const uint16_t p1 = rne(r);
  const uint16_t p2 = rne(r - __uint_as_float((uint32_t)p1 << 16));
  l0 = p0;
  l1 = p1;
  l2 = p2;
}

// c += u * v over one 16-k step, from the limb fragments u[0..2], v[0..2] of the two operands:
// the six products u2 v0, u1 v1, u0 v2, u1 v0, u0 v1, u0 v0 in this order - small products first,
// they are the ones the accumulator's rounding would otherwise swamp last
// (tests/split_products_ref.py restates the order and bounds its error).  U_FIRST: u is the MFMA's
// first operand (the accumulator's lane = a row of v, registers = runs of 4 rows of u: the weights
// go first where a lane should hold runs of consecutive output columns), else v is.
template <bool U_FIRST>
__device__ __forceinline__ lgx_f32x16 lgx_limb_mma(lgx_f32x16 c, const lgx_bf16x8& u, const lgx_bf16x8& v) {
  if constexpr (U_FIRST) return __builtin_amdgcn_mfma_f32_32x32x16_bf16(u, v, c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_32x32x16_bf16(v, u, c, 0, 0, 0);
}
template <bool U_FIRST>
__device__ __forceinline__ lgx_f32x16 lgx_split_mma(lgx_f32x16 c, const lgx_bf16x8* u, const lgx_bf16x8* v) {
  c = lgx_limb_mma<U_FIRST>(c, u[2], v[0]);
  c = lgx_limb_mma<U_FIRST>(c, u[1], v[1]);
  c = lgx_limb_mma<U_FIRST>(c, u[0], v[2]);
  c = lgx_limb_mma<U_FIRST>(c, u[1], v[0]);
  c = lgx_limb_mma<U_FIRST>(c, u[0], v[1]);
  return lgx_limb_mma<U_FIRST>(c, u[0], v[0]);
}
#endif
