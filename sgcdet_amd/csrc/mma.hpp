// Arithmetic modes of the MFMA kernels (convolutions, Linears, the fused level tail).  Every such kernel is a template on
//   NP = 3   an fp32 multiply-add as THREE bf16 products, lo*hi + hi*lo + hi*hi with fp32 accumulation (operands split
//            v = hi + lo in bfloat16): fp32-faithful to ~5e-6 of the tensor scale -- the default and the headline;
//   NP = 1   ONE bf16 product (both operands rounded to bfloat16): opt-in, ~2^-8 relative per operand;
//   NP = 2   ONE fp16 product on v_mfma_f32_32x32x16_f16 (same rate as the bf16 instruction, 11 instead of 8 significant bits):
//            opt-in, the twin of the reference's fp16 operator (TU/multi_scale_3ddeformable_attn_function.py:353-428; BASELINE.json
//            config #5 "fp16").  Operands are rounded to IEEE half and SATURATED at +-65504 (an fp32 activation beyond the half
//            range becomes the largest half, not infinity); a NaN stays a NaN.
// The 16-bit operands travel in `__bf16`-typed containers whatever the mode (planes, fragments, LDS images are byte-identical in
// layout); only the rounding on the way in (op_hi) and the instruction that multiplies them (mma_hh) know the format.
// sgc_set_conv_products(3 | 1 | 2) selects the mode process-wide (include/sgcdet_amd.h).
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

namespace sgc {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// the operand (NP = 1, 2) or its high part (NP = 3)
template <int NP>
__device__ __forceinline__ __bf16 op_hi(float v) {
  if constexpr (NP == 2) {
    const float c = v != v ? v : fminf(fmaxf(v, -65504.f), 65504.f);
    return __builtin_bit_cast(__bf16, (_Float16)c);
  } else {
    return (__bf16)v;
  }
}
// the low part of the NP = 3 split; unused (zero bits) in the one-product modes.  An infinite v gives hi = v and lo = Inf - Inf = NaN:
// every MFMA kernel turns an Inf operand into NaN (bounded by the traced contract of DESIGN.md "Non-finite values"); a NaN stays NaN
template <int NP>
__device__ __forceinline__ __bf16 op_lo(float v, __bf16 hi) {
  if constexpr (NP == 3) return (__bf16)(v - (float)hi);
  else return __builtin_bit_cast(__bf16, (unsigned short)0);
}
// four consecutive floats as the 8-byte pieces of the hi and lo planes (built in locals: through the references every element
// store may alias v, and the packed conversions are lost)
template <int NP>
__device__ __forceinline__ void split4(const float (&v)[4], bf16x4 &h, bf16x4 &l) {
  bf16x4 h4, l4;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const __bf16 hb = op_hi<NP>(v[e]);
    h4[e] = hb;
    l4[e] = op_lo<NP>(v[e], hb);
  }
  h = h4;
  l = l4;
}
// 32x32 accumulator (lane = column): the row of element k within a lane half; lanes 32-63 sit 4 rows below.  (The epilogues of
// conv3d_halo.hpp, conv3d_igemm.hip, conv2d_image.hip and conv3d_wgrad.hip spell the sum out inside their address expressions: as
// a call it associates differently and their code changes -- profiles/r14_rows_core.md)
__host__ __device__ constexpr int acc_row(int k) { return (k & 3) + 8 * (k >> 2); }
// the hi * hi product (the only one of the one-product modes)
template <int NP>
__device__ __forceinline__ f32x16 mma_hh(bf16x8 a, bf16x8 b, f32x16 c) {
  if constexpr (NP == 2)
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
// one multiply-add of the mode on one accumulator chain, in THIS order: lo*hi, hi*lo, hi*hi (results are pinned bit for bit).
// The lo parts are references: the one-product modes never read them, and their callers never fill them.
template <int NP>
__device__ __forceinline__ f32x16 mma_split(const bf16x8 &ah, const bf16x8 &al, const bf16x8 &bh, const bf16x8 &bl, f32x16 c) {
  if constexpr (NP == 3) {
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, c, 0, 0, 0);
  }
  return mma_hh<NP>(ah, bh, c);
}

// The same on v_mfma_f32_16x16x32_bf16 / _f16 (the Winograd bricks of the halo kernel under `wz_mfma` = 16; conv3d_halo.hpp).
// Operands: lane l holds row (A) or column (B) l & 15 and the eight k = 8 (l >> 4) .. + 7 -- a 32-channel slice is ONE k-step, and
// a lane reads the 16-byte chunk l >> 4 of its row.  16x16 accumulator: 4 floats, lane = column l & 15, rows acc16_row(l) .. + 3.
// The instruction sums 32 products where the 32x32x16 form sums 16 twice: results differ from that form in the last bits.
typedef float f32x4 __attribute__((ext_vector_type(4)));
__host__ __device__ constexpr int acc16_row(int lane) { return 4 * (lane >> 4); }
template <int NP>
__device__ __forceinline__ f32x4 mma_hh(bf16x8 a, bf16x8 b, f32x4 c) {
  if constexpr (NP == 2)
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
// one product of the mode (0: lo*hi, 1: hi*lo, 2: hi*hi) -- the caller interleaves the accumulators of a tile row, so that none
// waits for its own previous MFMA, and keeps this order per accumulator; the one-product modes have product 2 only
template <int NP, int PROD>
__device__ __forceinline__ f32x4 mma_split_one(const bf16x8 &ah, const bf16x8 &al, const bf16x8 &bh, const bf16x8 &bl, f32x4 c) {
  if constexpr (PROD == 2) return mma_hh<NP>(ah, bh, c);
  else if constexpr (NP != 3) return c;
  else if constexpr (PROD == 0) return __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh, c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl, c, 0, 0, 0);
}
template <int NP>
__device__ __forceinline__ f32x4 mma_split(const bf16x8 &ah, const bf16x8 &al, const bf16x8 &bh, const bf16x8 &bl, f32x4 c) {
  c = mma_split_one<NP, 0>(ah, al, bh, bl, c);
  c = mma_split_one<NP, 1>(ah, al, bh, bl, c);
  return mma_split_one<NP, 2>(ah, al, bh, bl, c);
}

// host: the process-wide mode (g_conv_products) as the compile-time NP of a launch -- f(std::integral_constant<int, NP>)
template <class F>
inline auto with_products(int products, F &&f) {
  if (products == 1) return f(std::integral_constant<int, 1>{});
  if (products == 2) return f(std::integral_constant<int, 2>{});
  return f(std::integral_constant<int, 3>{});
}

}  // namespace sgc
