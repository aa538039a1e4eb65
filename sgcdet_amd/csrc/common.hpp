// Shared helpers of the gfx950 library (include/sgcdet_amd.h).  CDNA4 only: wave = 64.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <atomic>

#include "../../include/sgcdet_amd.h"
#include "sample_geom.hpp"

namespace sgc {

constexpr int kWave = 64;
constexpr int kXcd = 8;  // MI355X: 8 XCDs, blocks are dealt round-robin over them

int set_error(int code, const char *fmt, ...);

inline int check_launch(const char *what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_error(SGC_ELAUNCH, "%s: %s", what, hipGetErrorString(e));
  return SGC_OK;
}

inline int ceil_div(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// workgroups of a grid-stride kernel over `work` items: at most 16 per CU
inline int grid_for(int64_t work, int block) {
  int64_t g = (work + block - 1) / block;
  if (g > 256 * 16) g = 256 * 16;
  if (g < 1) g = 1;
  return (int)g;
}

// The ReLU of every epilogue.  torch.relu(NaN) is NaN and the oracle keeps it too (`v < 0 ? 0 : v`); fmaxf(NaN, 0) is 0, which
// turns a poisoned activation into a clean zero that no loss ever sees (DESIGN.md "Non-finite values").  Finite values are those
// of fmaxf up to the sign of a zero.  Running maxima, IoU terms and depth clamps keep fmaxf.
__device__ __forceinline__ float relu_nan(float v) { return v < 0.f ? 0.f : v; }
__device__ __forceinline__ float4 relu_nan(float4 v) { return make_float4(relu_nan(v.x), relu_nan(v.y), relu_nan(v.z), relu_nan(v.w)); }

// hipFuncAttributeMaxDynamicSharedMemorySize is a PER-DEVICE attribute: `done` is a bitmask over device ordinals
// (one static per call site), so a process that drives several GPUs sets it once on each of them; thread-safe
// (setting it twice is harmless, the mask only saves the driver call on the hot path).
inline void ensure_dynamic_lds(const void *fn, int bytes, std::atomic<uint64_t> &done) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  const uint64_t bit = 1ull << (dev & 63);
  if (done.load(std::memory_order_acquire) & bit) return;
  (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  done.fetch_or(bit, std::memory_order_release);
}

// XCD-aware, bijective block -> tile map: the blocks that share an XCD (equal
// blockIdx % 8 under round-robin dispatch) walk one contiguous chunk of the tile
// range, so tiles that touch the same camera's maps meet in one 4 MiB L2.  Placement
// is a speed assumption only; any dispatch order gives the same results.
__device__ __forceinline__ int xcd_tile(int bid, int ntiles) {
  const int x = bid % kXcd, j = bid / kXcd;
  const int base = ntiles / kXcd, rem = ntiles % kXcd;
  return x * base + (x < rem ? x : rem) + j;
}

// Butterfly exchange with lane ^ o.  o = 1, 2 stay on the VALU as DPP quad permutes (no trip through the
// LDS crossbar that ds_bpermute takes); larger strides fall back to __shfl_xor.
template <int CTRL>
__device__ __forceinline__ float dpp_move(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}
__device__ __forceinline__ float lane_xor(float v, int o) {
  if (o == 1) return dpp_move<0xB1>(v);    // quad_perm:[1,0,3,2]
  if (o == 2) return dpp_move<0x4E>(v);    // quad_perm:[2,3,0,1]
  return __shfl_xor(v, o);
}

// a / size, correctly rounded (== the IEEE division of the reference's `sampling_offsets / offset_normalizer`,
// TU/deformable_cross_attention.py:428-455), for a wave-uniform size and rcp = RN(1 / size): one Newton correction of
// the reciprocal product (Markstein): q0 = a * rcp is within 1.5 ulp, r = a - q0 * size is exact in an fma, RN(q0 + r * rcp)
// is the correctly rounded quotient (checked against `/` on 3e8 random operands for every map size in use; a * rcp alone
// differs from the quotient in the last bit for 20 % of the operands at size 80).  3 instructions instead of ~10.
__device__ __forceinline__ float div_by_size(float a, float size, float rcp) {
  const float q0 = a * rcp;
  const float r = __builtin_fmaf(-q0, size, a);
  return __builtin_fmaf(r, rcp, q0);
}

// ---- LayerNorm over one row of C = 64 * VPL channels held by ONE wave (rows.hip: layer_norm_rows_kernel; level_tail.hip uses the
// same functions on rows that live in LDS, so the fused level tail reproduces the stand-alone kernel bit for bit).  Lane l holds
// channels 4 l .. 4 l + 3 (VPL % 4 == 0: one 16-byte access) or l + 64 j. ----
template <int VPL>
__device__ __forceinline__ int ln_channel(int lane, int j) {
  return VPL % 4 == 0 ? ((j / 4) * 64 + lane) * 4 + (j & 3) : j * 64 + lane;
}
template <int VPL>
__device__ __forceinline__ void ln_row_load(const float *xr, int lane, float (&v)[VPL]) {
  if constexpr (VPL % 4 == 0) {
#pragma unroll
    for (int j = 0; j < VPL / 4; ++j) {
      const float4 t = *reinterpret_cast<const float4 *>(xr + (j * 64 + lane) * 4);
      v[4 * j] = t.x; v[4 * j + 1] = t.y; v[4 * j + 2] = t.z; v[4 * j + 3] = t.w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < VPL; ++j) v[j] = xr[j * 64 + lane];
  }
}
template <int VPL>
__device__ __forceinline__ void ln_row_store(float *yr, int lane, const float (&y)[VPL]) {
  if constexpr (VPL % 4 == 0) {
#pragma unroll
    for (int j = 0; j < VPL / 4; ++j)
      *reinterpret_cast<float4 *>(yr + (j * 64 + lane) * 4) = make_float4(y[4 * j], y[4 * j + 1], y[4 * j + 2], y[4 * j + 3]);
  } else {
#pragma unroll
    for (int j = 0; j < VPL; ++j) yr[j * 64 + lane] = y[j];
  }
}
template <int VPL>
__device__ __forceinline__ void ln_row_stats(const float (&v)[VPL], float eps, float &mean, float &rstd) {
  constexpr int C = 64 * VPL;
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < VPL; ++j) s += v[j];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  mean = s * (1.0f / (float)C);
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < VPL; ++j) { const float d = v[j] - mean; q += d * d; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
  rstd = rsqrtf(q * (1.0f / (float)C) + eps);
}
__device__ __forceinline__ float ln_apply(float v, float mean, float rstd, float g, float b) { return (v - mean) * rstd * g + b; }

}  // namespace sgc
