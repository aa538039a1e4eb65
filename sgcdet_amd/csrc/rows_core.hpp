// The weight-stationary row core: what rows_gemm_bf16x3_kernel, rows_gemm_gather_pc_kernel (rows_gemm.hip) and level_tail_kernel
// (level_tail.hip) share.
//
// A wave owns 32 output columns and keeps their weights -- hi and lo planes, KS 16-deep k-steps -- as MFMA B fragments in
// registers; 32-row A tiles stream through a bf16 hi | lo image in LDS (row pitch K + 8 bf16: conflict-free ds_read_b128).
// The core holds the scheme once, as free functions over the caller's registers:
//   rows_load_B         the resident fragments from row-major [N][K] planes
//   rows_multiply       the PD-ahead A-fragment ring, KS k-steps on ONE accumulator chain
//   rows_stage_chunk    four floats of a row, split, into the hi and lo planes
//   rows_gather_*       the gather tile: four corner rows per staged row, summed in the geometry sample's order (the producer waves
//                       of rows_gemm_gather_pc_kernel; the K = 128 gather form keeps a copy, see rows_gemm.hip)
//   rows_store_rowmajor the epilogue straight from the accumulator registers
// and on the host the LDS plan and the stripe count of a persistent launch.  It knows nothing of tile loops, barriers or who
// stages and who multiplies: those are the kernels'.
#pragma once
#include "conv_common.hpp"
#include "tuning.hpp"
#include "mma.hpp"

namespace sgc {

constexpr int RG_ROWS = 32;
constexpr unsigned RG_OOB = 0xfffffff0u;    // a byte offset no buffer of < 4 GiB reaches: the load returns 0, the store is dropped

// dynamic LDS of a row-GEMM workgroup: [2 buffers][hi | lo][32][K + 8] bf16
constexpr int rows_lds_bytes(int K) { return 2 * 2 * RG_ROWS * (K + 8) * 2; }

// Workgroups per column group of a persistent launch: per_cu workgroups on every CU (one 8-wave or two 4-wave), cut to the
// rows_cu_pct share (the kernels are memory-bound: with scenes in flight the CUs they leave serve MFMA kernels), at most one per
// tile, a multiple of 8 (the XCD-aware deal of rows_gemm_bf16x3_kernel; a stripe without a tile exits at once)
inline int persistent_stripes(int cap_tiles, int per_cu, int ncg) {
  int stripes = device_cus() * per_cu / ncg;
  if (g_tune_rows_cu_pct > 0 && g_tune_rows_cu_pct < 100) stripes = stripes * g_tune_rows_cu_pct / 100;
  if (stripes > cap_tiles) stripes = cap_tiles;
  return (stripes + 7) / 8 * 8;
}

__device__ __forceinline__ float4 as_float4(u32x4 v) {
  return make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3]));
}

// ---- weights: all KS k-steps of column `col` of row-major [N][KS * 16] planes, as B fragments in registers ----
template <int KS, int NP>
__device__ __forceinline__ void rows_load_B(const __bf16 *w_hi, const __bf16 *w_lo, int col, int fh, bf16x8 (&bh)[KS], bf16x8 (&bl)[KS]) {
  const __bf16 *wh = w_hi + (int64_t)col * (KS * 16) + fh * 8, *wl = w_lo + (int64_t)col * (KS * 16) + fh * 8;
#pragma unroll
  for (int kk = 0; kk < KS; ++kk) {
    bh[kk] = *reinterpret_cast<const bf16x8 *>(wh + kk * 16);
    if constexpr (NP == 3) bl[kk] = *reinterpret_cast<const bf16x8 *>(wl + kk * 16);
  }
}

// An LDS image is (hi, plane, pitch): the hi plane, the lo plane `plane` elements behind it, `pitch` elements per row.
// ---- acc += A[32 rows][koff .. koff + KS * 16) x B over an image ----
// A fragments are read PD k-steps ahead of the MFMAs that use them (ring of PD + 1 register slots, static indices after
// unrolling); the scheduling barrier per step keeps that distance in the emitted code (left alone, the compiler issues each read
// one step ahead: ~96 MFMA cycles of cover for an LDS round trip)
constexpr int ROWS_PD = 3;
template <int KS, int NP>
__device__ __forceinline__ void rows_multiply(const __bf16 *hi, int plane, int pitch, int koff, int fr, int fh,
                                              const bf16x8 (&bh)[KS], const bf16x8 (&bl)[KS], f32x16 &acc) {
  constexpr int PD = ROWS_PD;
  const __bf16 *a_hi = hi + fr * pitch + koff + fh * 8, *a_lo = a_hi + plane;
  bf16x8 ah[PD + 1], al[PD + 1];
#pragma unroll
  for (int kk = 0; kk < PD; ++kk) {
    ah[kk] = *reinterpret_cast<const bf16x8 *>(a_hi + kk * 16);
    if constexpr (NP == 3) al[kk] = *reinterpret_cast<const bf16x8 *>(a_lo + kk * 16);
  }
#pragma unroll
  for (int kk = 0; kk < KS; ++kk) {
    if (kk + PD < KS) {
      ah[(kk + PD) % (PD + 1)] = *reinterpret_cast<const bf16x8 *>(a_hi + (kk + PD) * 16);
      if constexpr (NP == 3) al[(kk + PD) % (PD + 1)] = *reinterpret_cast<const bf16x8 *>(a_lo + (kk + PD) * 16);
    }
    acc = mma_split<NP>(ah[kk % (PD + 1)], al[kk % (PD + 1)], bh[kk], bl[kk], acc);
    __builtin_amdgcn_sched_barrier(0);
  }
}

__device__ __forceinline__ void rows_zero(f32x16 &acc) {
#pragma unroll
  for (int k = 0; k < 16; ++k) acc[k] = 0.f;
}

// ---- stage floats [4 c4, 4 c4 + 4) of row `row`: split once, one 8-byte store per plane ----
template <int NP>
__device__ __forceinline__ void rows_stage_chunk(const float (&v)[4], __bf16 *hi, int plane, int pitch, int row, int c4) {
  bf16x4 h, l;
  split4<NP>(v, h, l);
  *reinterpret_cast<bf16x4 *>(hi + row * pitch + c4 * 4) = h;
  if constexpr (NP == 3) *reinterpret_cast<bf16x4 *>(hi + plane + row * pitch + c4 * 4) = l;
}

// ---- the gather tile (sgc_pairs_geometry_linear_bf16x3): staged row r = sum_k gw[r][k] * x[go[r][k]][:] ----
// A thread owns chunk c4 of rows row0 + i * RSTEP, i < CH.  request: the descriptor (four corner rows, four weights) and the
// corner rows' chunks, all in flight at once; `live` false (a tile past the last): every load returns zeros.
template <int CH, int RSTEP>
__device__ __forceinline__ void rows_gather_request(__amdgpu_buffer_rsrc_t xr, __amdgpu_buffer_rsrc_t gor, __amdgpu_buffer_rsrc_t gwr, bool live,
                                                    int row0, int c4, int64_t ldx, float4 (&rv)[4 * CH], float4 (&rw)[CH]) {
  int ldx4 = (int)ldx * 4;
  asm volatile("" : "+s"(ldx4));
#pragma unroll
  for (int i = 0; i < CH; ++i) {
    const unsigned doff = live ? (unsigned)(row0 + i * RSTEP) * 16u : RG_OOB;
    const u32x4 o = __builtin_amdgcn_raw_buffer_load_b128(gor, doff, 0, 0);
    rw[i] = as_float4(__builtin_amdgcn_raw_buffer_load_b128(gwr, doff, 0, 0));
#pragma unroll
    for (int k = 0; k < 4; ++k) rv[4 * i + k] = as_float4(__builtin_amdgcn_raw_buffer_load_b128(xr, o[k] * (unsigned)ldx4 + c4 * 16, 0, 0));
  }
}
// build: the geometry sample's arithmetic (dfa3d_fwd_kernel<kPairsGeom>: acc += w[k] * v[k] over the corners in order, contracted
// to fmas): the staged row is the value sgc_pairs_geometry_sample would have written, bit for bit
template <int NP, int CH, int RSTEP>
__device__ __forceinline__ void rows_gather_build(const float4 (&rv)[4 * CH], const float4 (&rw)[CH], __bf16 *hi, int plane, int pitch,
                                                  int row0, int c4) {
#pragma unroll
  for (int i = 0; i < CH; ++i) {
    const float wk[4] = {rw[i].x, rw[i].y, rw[i].z, rw[i].w};
    float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[0] = __builtin_fmaf(wk[k], rv[4 * i + k].x, v[0]); v[1] = __builtin_fmaf(wk[k], rv[4 * i + k].y, v[1]);
      v[2] = __builtin_fmaf(wk[k], rv[4 * i + k].z, v[2]); v[3] = __builtin_fmaf(wk[k], rv[4 * i + k].w, v[3]);
    }
    rows_stage_chunk<NP>(v, hi, plane, pitch, row0 + i * RSTEP, c4);
  }
}

// ---- row-major epilogue of the tile at row m0: acc * sc + sh; relu; + residual; relu (the order of epilogue4, igemm_tile.hpp) ----
// Row offsets are SCALAR multiples of the row pitch added to one per-lane base: the pitch is made opaque per call so that the 16
// offsets are not hoisted out of the tile loop into 16 long-lived VGPRs (the kernels sit at the 256-register limit of two waves
// per SIMD).  A store past the descriptor's range (rows past the live count) is dropped.
template <bool RESIDUAL>
__device__ __forceinline__ void rows_store_rowmajor(const f32x16 &acc, __amdgpu_buffer_rsrc_t yr, __amdgpu_buffer_rsrc_t rr, int m0, int fh, int col,
                                                    int N, float sc, float sh, bool relu_before, bool relu_after) {
  int n4 = N * 4;
  asm volatile("" : "+s"(n4));
  float res[16];
  const unsigned base = (unsigned)(m0 + 4 * fh) * (unsigned)n4 + col * 4;
  if constexpr (RESIDUAL) {
#pragma unroll
    for (int k = 0; k < 16; ++k) res[k] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rr, base + acc_row(k) * n4, 0, 0));
  }
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    float v = acc[k] * sc;                              // two roundings (product, then sum) like the staged epilogue of
    asm volatile("" : "+v"(v));                          // the tile kernel and the oracle's plain C: the empty asm keeps the
    v += sh;                                             // compiler from contracting them into one fma
    v = relu_before ? relu_nan(v) : v;
    if constexpr (RESIDUAL) {
      v += res[k];
      v = relu_after ? relu_nan(v) : v;
    }
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), yr, base + acc_row(k) * n4, 0, 0);
  }
}

}  // namespace sgc
