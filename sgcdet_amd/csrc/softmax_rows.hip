// Backward of a row softmax (sgc_softmax_rows_backward, include/sgcdet_amd_depth_train.h): the softmax that
// depth_reg's forward epilogue produces (sgc_conv2d_nhwc_ex_bf16x3, softmax_cols) has its gradient here,
//   g[r][c] = p[r][c] * (dp[r][c] - sum_c' p[r][c'] * dp[r][c']),
// written at the 32-column pitch the convolution kernels read their input gradient at.
//
// A streaming kernel: every value is read once and written once.  LG lanes own a row (LG = the power of two at or above C / 4, at
// most 32 for C <= 128), a lane one float4 of p and of dp (16-byte accesses, neighbouring lanes neighbouring addresses), the row sum
// is a butterfly over the LG lanes -- registers only, no LDS.  Rows are independent: a NaN stays in its row.
#include "common.hpp"
#include "../../include/sgcdet_amd_depth_train.h"

namespace sgc {

constexpr int SM_T = 256;

template <int LG>
__global__ __launch_bounds__(SM_T) void softmax_rows_backward_kernel(const float *__restrict__ p, const float *__restrict__ dp, float *__restrict__ g,
                                                                     int64_t rows, int C4, int ldp, int lddp, int ldg) {
  constexpr int RPB = SM_T / LG;                       // rows per workgroup and step
  const int l = threadIdx.x % LG, rl = threadIdx.x / LG;
  const int ldg4 = ldg >> 2;
  for (int64_t r0 = (int64_t)blockIdx.x * RPB; r0 < rows; r0 += (int64_t)gridDim.x * RPB) {    // r0 is uniform over the workgroup
    const int64_t r = r0 + rl;
    const bool live = r < rows && l < C4;
    float4 pv = make_float4(0.f, 0.f, 0.f, 0.f), dv = pv;
    if (live) {
      pv = *reinterpret_cast<const float4 *>(p + r * ldp + l * 4);
      dv = *reinterpret_cast<const float4 *>(dp + r * lddp + l * 4);
    }
    float s = pv.x * dv.x + pv.y * dv.y + pv.z * dv.z + pv.w * dv.w;
#pragma unroll
    for (int o = LG / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, LG);          // every lane of the wave takes part: no divergence above
    if (r < rows) {
      float *gr = g + r * ldg;
      if (l < C4)
        *reinterpret_cast<float4 *>(gr + l * 4) = make_float4(pv.x * (dv.x - s), pv.y * (dv.y - s), pv.z * (dv.z - s), pv.w * (dv.w - s));
      for (int c4 = (l < C4 ? l + LG : l); c4 < ldg4; c4 += LG)              // the padding columns [C, ldg): LG >= C4, so l + LG >= C4
        *reinterpret_cast<float4 *>(gr + c4 * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
}

template <int LG>
static int launch_softmax_backward(const float *p, const float *dp, float *g, int64_t rows, int C, int ldp, int lddp, int ldg, hipStream_t st) {
  const int64_t groups = (rows + SM_T / LG - 1) / (SM_T / LG);
  const int grid = (int)(groups < 8192 ? groups : 8192);
  hipLaunchKernelGGL(softmax_rows_backward_kernel<LG>, dim3(grid), dim3(SM_T), 0, st, p, dp, g, rows, C / 4, ldp, lddp, ldg);
  return check_launch("softmax_rows_backward_kernel");
}

}  // namespace sgc

using namespace sgc;

extern "C" int sgc_softmax_rows_backward(const float *p, const float *dp, float *g, int64_t rows, int C, int ldp, int lddp, int ldg,
                                         sgc_stream_t stream) {
  const char *who = "sgc_softmax_rows_backward";
  if (!p || !dp || !g) return set_error(SGC_EINVAL, "%s: null pointer", who);
  if (rows <= 0) return set_error(SGC_EINVAL, "%s: bad size", who);
  if (C < 4 || C > 128 || C % 4) return set_error(SGC_EUNSUP, "%s: needs C %% 4 == 0 and 4 <= C <= 128 (got %d)", who, C);
  if (ldp < C || lddp < C || ldg < C) return set_error(SGC_EUNSUP, "%s: a row pitch below C", who);
  if ((ldp | lddp | ldg) % 4) return set_error(SGC_EUNSUP, "%s: needs row pitches %% 4 == 0", who);
  if (((uintptr_t)p | (uintptr_t)dp | (uintptr_t)g) & 15) return set_error(SGC_EINVAL, "%s: pointers must be 16-byte aligned", who);
  hipStream_t st = (hipStream_t)stream;
  const int C4 = C / 4;
  if (C4 <= 1) return launch_softmax_backward<1>(p, dp, g, rows, C, ldp, lddp, ldg, st);
  if (C4 <= 2) return launch_softmax_backward<2>(p, dp, g, rows, C, ldp, lddp, ldg, st);
  if (C4 <= 4) return launch_softmax_backward<4>(p, dp, g, rows, C, ldp, lddp, ldg, st);
  if (C4 <= 8) return launch_softmax_backward<8>(p, dp, g, rows, C, ldp, lddp, ldg, st);
  if (C4 <= 16) return launch_softmax_backward<16>(p, dp, g, rows, C, ldp, lddp, ldg, st);
  return launch_softmax_backward<32>(p, dp, g, rows, C, ldp, lddp, ldg, st);
}
