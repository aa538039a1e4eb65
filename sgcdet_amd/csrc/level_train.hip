// Training a view-transform level (include/sgcdet_amd_level_train.h): the backward halves of what inference already
// runs in one launch each -- the row LayerNorm (rows.hip), the location / softmax arithmetic of the gather, the mean over views
// (view_pool.hip).  All streaming kernels, no float atomics: every sum runs in a fixed order, a repeated launch gives the same bits.
#include "common.hpp"
#include "../../include/sgcdet_amd_level_train.h"

namespace sgc {

// ---- LayerNorm backward ---------------------------------------------------------------------------------------------------------------
// Workgroup b walks the rows [b * R, min(b * R + R, rows)), R % 4 == 0: wave w takes the rows b * R + w, + 4, ...  A lane keeps the
// dgamma / dbeta terms of its channels in registers (added in row order), the four waves meet in LDS and are added in wave order:
// one partial [2, C] per workgroup.  ln_reduce_partials_kernel adds the partials.
constexpr int LN_MAX_PARTS = 256;       // one workgroup per CU at the largest levels
constexpr int LN_GENERIC_MAX_C = 2048;  // the generic form keeps 4 x [2, C] floats in LDS

struct LnBwdGeom {
  int P, R;
};

static LnBwdGeom ln_bwd_geom(int rows) {
  LnBwdGeom g;
  g.R = 4 * ceil_div(rows, 4 * LN_MAX_PARTS);
  g.P = ceil_div(rows, g.R);
  return g;
}

template <int VPL>     // C = 64 * VPL channels, VPL floats per lane (ln_channel's layout)
__global__ __launch_bounds__(256) void layer_norm_rows_backward_kernel(const float *__restrict__ x, const float *__restrict__ gamma, float eps,
                                                                       const float *__restrict__ dy, float *__restrict__ dx,
                                                                       float *__restrict__ part, int rows, int R) {
  constexpr int C = 64 * VPL;
  __shared__ float sm[4][2][C];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * R;
  const int64_t r1 = r0 + R < rows ? r0 + R : rows;
  float gm[VPL], dg[VPL], db[VPL];
#pragma unroll
  for (int j = 0; j < VPL; ++j) {
    gm[j] = gamma[ln_channel<VPL>(lane, j)];
    dg[j] = 0.f;
    db[j] = 0.f;
  }
  for (int64_t r = r0 + w; r < r1; r += 4) {                     // uniform over the wave
    float v[VPL], d[VPL];
    ln_row_load<VPL>(x + r * C, lane, v);
    ln_row_load<VPL>(dy + r * C, lane, d);
    float mean, rstd;
    ln_row_stats<VPL>(v, eps, mean, rstd);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
      v[j] = (v[j] - mean) * rstd;                               // xhat
      const float g = d[j] * gm[j];
      s1 += g;
      s2 += g * v[j];
      dg[j] += d[j] * v[j];
      db[j] += d[j];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      s1 += __shfl_xor(s1, o);
      s2 += __shfl_xor(s2, o);
    }
    const float m1 = s1 * (1.0f / (float)C), m2 = s2 * (1.0f / (float)C);
    float o[VPL];
#pragma unroll
    for (int j = 0; j < VPL; ++j) o[j] = rstd * (d[j] * gm[j] - m1 - v[j] * m2);
    ln_row_store<VPL>(dx + r * C, lane, o);
  }
#pragma unroll
  for (int j = 0; j < VPL; ++j) {
    const int c = ln_channel<VPL>(lane, j);
    sm[w][0][c] = dg[j];
    sm[w][1][c] = db[j];
  }
  __syncthreads();
  float *pb = part + (int64_t)blockIdx.x * 2 * C;
  for (int i = threadIdx.x; i < 2 * C; i += 256) {
    const int k = i / C, c = i - k * C;
    pb[i] = ((sm[0][k][c] + sm[1][k][c]) + sm[2][k][c]) + sm[3][k][c];
  }
}

// generic width (C <= LN_GENERIC_MAX_C): strided loops over the row as the forward's generic kernel, the terms of a wave in its
// own [2, C] slice of the dynamic LDS (a lane owns the columns lane, lane + 64, ...)
__global__ __launch_bounds__(256) void layer_norm_rows_backward_generic_kernel(const float *__restrict__ x, const float *__restrict__ gamma,
                                                                               float eps, const float *__restrict__ dy, float *__restrict__ dx,
                                                                               float *__restrict__ part, int rows, int R, int C) {
  extern __shared__ __attribute__((aligned(16))) float lsm[];    // [4][2][C]
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * R;
  const int64_t r1 = r0 + R < rows ? r0 + R : rows;
  float *mine = lsm + (int64_t)w * 2 * C;
  for (int c = lane; c < C; c += 64) mine[c] = mine[C + c] = 0.f;
  for (int64_t r = r0 + w; r < r1; r += 4) {
    const float *xr = x + r * C, *dr = dy + r * C;
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += xr[c];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const float mean = s / (float)C;
    float q = 0.f;
    for (int c = lane; c < C; c += 64) { const float d = xr[c] - mean; q += d * d; }
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
    const float rstd = rsqrtf(q / (float)C + eps);
    float s1 = 0.f, s2 = 0.f;
    for (int c = lane; c < C; c += 64) {
      const float xh = (xr[c] - mean) * rstd, d = dr[c], g = d * gamma[c];
      s1 += g;
      s2 += g * xh;
      mine[c] += d * xh;
      mine[C + c] += d;
    }
    for (int o = 32; o > 0; o >>= 1) {
      s1 += __shfl_xor(s1, o);
      s2 += __shfl_xor(s2, o);
    }
    const float m1 = s1 / (float)C, m2 = s2 / (float)C;
    for (int c = lane; c < C; c += 64) {
      const float xh = (xr[c] - mean) * rstd;
      dx[r * C + c] = rstd * (dr[c] * gamma[c] - m1 - xh * m2);
    }
  }
  __syncthreads();
  float *pb = part + (int64_t)blockIdx.x * 2 * C;
  for (int i = threadIdx.x; i < 2 * C; i += 256) pb[i] = ((lsm[i] + lsm[2 * C + i]) + lsm[4 * C + i]) + lsm[6 * C + i];
}

// part [P][2 * C] -> dgamma | dbeta.  64 columns by 4 partial lanes per workgroup: lane ty adds the partials ty, ty + 4, ..., the i-th
// of them into accumulator i % 4, then (a0 + a1) + (a2 + a3), then the four lanes in lane order -- a fixed order for a given P.
__global__ __launch_bounds__(256) void ln_reduce_partials_kernel(const float *__restrict__ part, int P, int C, float *__restrict__ dgamma,
                                                                 float *__restrict__ dbeta) {
  __shared__ float sm[4][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + tx, C2 = 2 * C;
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  if (col < C2) {
    int i = 0;
    for (int p = ty; p < P; p += 4, ++i) a[i & 3] += part[(int64_t)p * C2 + col];
  }
  sm[ty][tx] = (a[0] + a[1]) + (a[2] + a[3]);
  __syncthreads();
  if (ty == 0 && col < C2) {
    const float s = ((sm[0][tx] + sm[1][tx]) + sm[2][tx]) + sm[3][tx];
    if (col < C) dgamma[col] = s;
    else dbeta[col - C] = s;
  }
}

// ---- sampling locations and attention weights ----------------------------------------------------------------------------------------
// A lane owns one (pair, head): its 2 LP uv offsets, LP depth offsets and LP logits are three contiguous runs of its proj row, its
// 3 LP location floats and LP weights contiguous runs of loc / attn -- neighbouring lanes (heads, then pairs) neighbouring runs.  VEC:
// LP % 4 == 0 and aligned rows, the runs move as float4.  The arrays are indexed by unrolled loops only: registers, no scratch.
constexpr int SL_MAX_LP = 16;

template <bool VEC, int CAP>      // count <= CAP, the length of the array behind dst; VEC: count % 4 == 0
__device__ __forceinline__ void sl_load(const float *__restrict__ src, int count, float (&dst)[CAP]) {
  if constexpr (VEC) {
#pragma unroll
    for (int j = 0; j < CAP / 4; ++j)
      if (4 * j < count) {
        const float4 t = *reinterpret_cast<const float4 *>(src + 4 * j);
        dst[4 * j] = t.x; dst[4 * j + 1] = t.y; dst[4 * j + 2] = t.z; dst[4 * j + 3] = t.w;
      }
  } else {
#pragma unroll
    for (int j = 0; j < CAP; ++j)
      if (j < count) dst[j] = src[j];
  }
}

template <bool VEC, int CAP>
__device__ __forceinline__ void sl_store(float *__restrict__ dst, int count, const float (&src)[CAP]) {
  if constexpr (VEC) {
#pragma unroll
    for (int j = 0; j < CAP / 4; ++j)
      if (4 * j < count) *reinterpret_cast<float4 *>(dst + 4 * j) = make_float4(src[4 * j], src[4 * j + 1], src[4 * j + 2], src[4 * j + 3]);
  } else {
#pragma unroll
    for (int j = 0; j < CAP; ++j)
      if (j < count) dst[j] = src[j];
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void sampling_locations_forward_kernel(const float *__restrict__ ref, const float *__restrict__ proj,
                                                                         const float *__restrict__ normalizer, float *__restrict__ loc,
                                                                         float *__restrict__ attn, int64_t total, int M, int P, int LP, int ldp) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int64_t pair = idx / M;
  const int m = (int)(idx - pair * M);
  const float *row = proj + pair * ldp;
  const int MLP = M * LP;
  float uv[2 * SL_MAX_LP], dz[SL_MAX_LP], lg[SL_MAX_LP], o[3 * SL_MAX_LP];
  sl_load<VEC>(row + m * 2 * LP, 2 * LP, uv);
  sl_load<VEC>(row + 2 * MLP + m * LP, LP, dz);
  sl_load<VEC>(row + 3 * MLP + m * LP, LP, lg);
  const float ru = ref[pair * 3], rv = ref[pair * 3 + 1], rz = ref[pair * 3 + 2];
#pragma unroll
  for (int j = 0; j < SL_MAX_LP; ++j)
    if (j < LP) {
      const float *nz = normalizer + (j / P) * 3;
      o[3 * j] = ru + uv[2 * j] / nz[0];
      o[3 * j + 1] = rv + uv[2 * j + 1] / nz[1];
      o[3 * j + 2] = rz + dz[j] / nz[2];
    }
  sl_store<VEC>(loc + idx * 3 * LP, 3 * LP, o);
  float mx = lg[0];
#pragma unroll
  for (int j = 1; j < SL_MAX_LP; ++j)
    if (j < LP) mx = fmaxf(mx, lg[j]);                          // a NaN logit is skipped here and poisons the sum below
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < SL_MAX_LP; ++j)
    if (j < LP) {
      lg[j] = expf(lg[j] - mx);
      sum += lg[j];
    }
#pragma unroll
  for (int j = 0; j < SL_MAX_LP; ++j)
    if (j < LP) lg[j] = lg[j] / sum;
  sl_store<VEC>(attn + idx * LP, LP, lg);
}

template <bool VEC>
__global__ __launch_bounds__(256) void sampling_locations_backward_kernel(const float *__restrict__ attn, const float *__restrict__ grad_loc,
                                                                          const float *__restrict__ grad_attn,
                                                                          const float *__restrict__ normalizer, float *__restrict__ grad_proj,
                                                                          int64_t total, int M, int P, int LP, int ldp) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int64_t pair = idx / M;
  const int m = (int)(idx - pair * M);
  float *row = grad_proj + pair * ldp;
  const int MLP = M * LP;
  float gl[3 * SL_MAX_LP], a[SL_MAX_LP], ga[SL_MAX_LP], uv[2 * SL_MAX_LP], dz[SL_MAX_LP];
  sl_load<VEC>(grad_loc + idx * 3 * LP, 3 * LP, gl);
  sl_load<VEC>(attn + idx * LP, LP, a);
  sl_load<VEC>(grad_attn + idx * LP, LP, ga);
  float dot = 0.f;
#pragma unroll
  for (int j = 0; j < SL_MAX_LP; ++j)
    if (j < LP) {
      const float *nz = normalizer + (j / P) * 3;
      uv[2 * j] = gl[3 * j] / nz[0];
      uv[2 * j + 1] = gl[3 * j + 1] / nz[1];
      dz[j] = gl[3 * j + 2] / nz[2];
      dot += a[j] * ga[j];
    }
#pragma unroll
  for (int j = 0; j < SL_MAX_LP; ++j)
    if (j < LP) a[j] = a[j] * (ga[j] - dot);
  sl_store<VEC>(row + m * 2 * LP, 2 * LP, uv);
  sl_store<VEC>(row + 2 * MLP + m * LP, LP, dz);
  sl_store<VEC>(row + 3 * MLP + m * LP, LP, a);
  for (int c = 4 * MLP + m; c < ldp; c += M) row[c] = 0.f;      // the padding columns, dealt over the heads of the pair
}

// ---- mean over views, backward --------------------------------------------------------------------------------------------------------
// One lane per (valid voxel, T of its channels): counts the cameras that see the voxel as sgc_view_mean does, divides once, writes the
// quotient to the row of every such camera's pair.  Lanes of one voxel read the same slot column (broadcast loads).
template <typename T>
__device__ __forceinline__ T vm_div(T v, float c);
template <>
__device__ __forceinline__ float vm_div<float>(float v, float c) { return v / c; }
template <>
__device__ __forceinline__ float4 vm_div<float4>(float4 v, float c) { return make_float4(v.x / c, v.y / c, v.z / c, v.w / c); }

template <typename T>
__global__ __launch_bounds__(256) void view_mean_backward_kernel(const T *__restrict__ grad_mean, const int32_t *__restrict__ slot,
                                                                 const int32_t *__restrict__ valid_index, T *__restrict__ grad_feat, int N,
                                                                 int Nq, int CT, int n_valid, int n_pairs) {
  const int64_t total = (int64_t)n_valid * CT;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int i = (int)(idx / CT), c = (int)(idx - (int64_t)i * CT);
    const int q = valid_index[i];
    if (q < 0 || q >= Nq) continue;                              // no voxel of the grid: nothing to read, nothing to write
    int cnt = 0;
    for (int n = 0; n < N; ++n) cnt += slot[(int64_t)n * Nq + q] >= 0;
    const T g = vm_div<T>(grad_mean[idx], (float)cnt);
    for (int n = 0; n < N; ++n) {
      const int p = slot[(int64_t)n * Nq + q];
      if (p >= 0 && p < n_pairs) grad_feat[(int64_t)p * CT + c] = g;
    }
  }
}

static bool aligned16(const void *a, const void *b = nullptr, const void *c = nullptr, const void *d = nullptr) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) | reinterpret_cast<uintptr_t>(d)) & 15) == 0;
}

static int check_sampling(const char *who, const void *a, const void *b, const void *c, const void *d, const void *e, int n, int M, int L,
                          int P, int ldp) {
  if (!a || !b || !c || !d || !e) return set_error(SGC_EINVAL, "%s: null pointer", who);
  if (n <= 0 || M <= 0 || L <= 0 || P <= 0) return set_error(SGC_EINVAL, "%s: non-positive size", who);
  if ((int64_t)L * P > SL_MAX_LP) return set_error(SGC_EUNSUP, "%s: needs L * P <= %d (got %d * %d)", who, SL_MAX_LP, L, P);
  if ((int64_t)M * L * P * 4 > (int64_t)ldp) return set_error(SGC_EINVAL, "%s: ldp = %d is below 4 * M * L * P = %lld", who, ldp, (long long)M * L * P * 4);
  if ((int64_t)n * M > ((int64_t)1 << 31) * 255) return set_error(SGC_EUNSUP, "%s: too many (pair, head) items", who);
  return 0;
}

}  // namespace sgc

using namespace sgc;

extern "C" int64_t sgc_layer_norm_rows_backward_workspace_floats(int rows, int C) {
  if (rows <= 0 || C <= 0) {
    set_error(SGC_EINVAL, "sgc_layer_norm_rows_backward: needs rows >= 1 and C >= 1");
    return -1;
  }
  return (int64_t)ln_bwd_geom(rows).P * 2 * C;
}

extern "C" int sgc_layer_norm_rows_backward(const float *x, const float *gamma, float eps, const float *dy, float *dx, float *dgamma,
                                            float *dbeta, float *workspace, int64_t workspace_floats, int rows, int C, sgc_stream_t stream) {
  const char *who = "sgc_layer_norm_rows_backward";
  if (!x || !gamma || !dy || !dx || !dgamma || !dbeta || !workspace) return set_error(SGC_EINVAL, "%s: null pointer", who);
  if (rows <= 0 || C <= 0) return set_error(SGC_EINVAL, "%s: needs rows >= 1 and C >= 1", who);
  const LnBwdGeom g = ln_bwd_geom(rows);
  if (workspace_floats < (int64_t)g.P * 2 * C)
    return set_error(SGC_EINVAL, "%s: needs a workspace of sgc_layer_norm_rows_backward_workspace_floats(rows, C) floats", who);
  const bool vec = (C == 128 || C == 256) && aligned16(x, dy, dx, gamma);
  if (!vec && C > LN_GENERIC_MAX_C) return set_error(SGC_EUNSUP, "%s: the generic form needs C <= %d (got %d)", who, LN_GENERIC_MAX_C, C);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(g.P), block(256);
  if (vec && C == 256)
    hipLaunchKernelGGL(layer_norm_rows_backward_kernel<4>, grid, block, 0, st, x, gamma, eps, dy, dx, workspace, rows, g.R);
  else if (vec)
    hipLaunchKernelGGL(layer_norm_rows_backward_kernel<2>, grid, block, 0, st, x, gamma, eps, dy, dx, workspace, rows, g.R);
  else
    hipLaunchKernelGGL(layer_norm_rows_backward_generic_kernel, grid, block, (size_t)8 * C * sizeof(float), st, x, gamma, eps, dy, dx,
                       workspace, rows, g.R, C);
  if (int rc = check_launch("layer_norm_rows_backward_kernel")) return rc;
  hipLaunchKernelGGL(ln_reduce_partials_kernel, dim3(ceil_div(2 * (int64_t)C, 64)), block, 0, st, workspace, g.P, C, dgamma, dbeta);
  return check_launch("ln_reduce_partials_kernel");
}

extern "C" int sgc_sampling_locations_forward(const float *ref, const float *proj, const float *normalizer, float *loc, float *attn, int n,
                                              int M, int L, int P, int ldp, sgc_stream_t stream) {
  if (int rc = check_sampling("sgc_sampling_locations_forward", ref, proj, normalizer, loc, attn, n, M, L, P, ldp)) return rc;
  const int LP = L * P;
  const int64_t total = (int64_t)n * M;
  const dim3 grid(ceil_div(total, 256)), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (LP % 4 == 0 && ldp % 4 == 0 && aligned16(proj, loc, attn))
    hipLaunchKernelGGL(sampling_locations_forward_kernel<true>, grid, block, 0, st, ref, proj, normalizer, loc, attn, total, M, P, LP, ldp);
  else
    hipLaunchKernelGGL(sampling_locations_forward_kernel<false>, grid, block, 0, st, ref, proj, normalizer, loc, attn, total, M, P, LP, ldp);
  return check_launch("sampling_locations_forward_kernel");
}

extern "C" int sgc_sampling_locations_backward(const float *attn, const float *grad_loc, const float *grad_attn, const float *normalizer,
                                               float *grad_proj, int n, int M, int L, int P, int ldp, sgc_stream_t stream) {
  if (int rc = check_sampling("sgc_sampling_locations_backward", attn, grad_loc, grad_attn, normalizer, grad_proj, n, M, L, P, ldp)) return rc;
  const int LP = L * P;
  const int64_t total = (int64_t)n * M;
  const dim3 grid(ceil_div(total, 256)), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (LP % 4 == 0 && ldp % 4 == 0 && aligned16(grad_proj, grad_loc, grad_attn, attn))
    hipLaunchKernelGGL(sampling_locations_backward_kernel<true>, grid, block, 0, st, attn, grad_loc, grad_attn, normalizer, grad_proj, total,
                       M, P, LP, ldp);
  else
    hipLaunchKernelGGL(sampling_locations_backward_kernel<false>, grid, block, 0, st, attn, grad_loc, grad_attn, normalizer, grad_proj, total,
                       M, P, LP, ldp);
  return check_launch("sampling_locations_backward_kernel");
}

extern "C" int sgc_view_mean_backward(const float *grad_mean, const int32_t *slot, const int32_t *valid_index, float *grad_feat, int N,
                                      int Nq, int C, int n_valid, int n_pairs, sgc_stream_t stream) {
  const char *who = "sgc_view_mean_backward";
  if (!grad_mean || !slot || !valid_index || !grad_feat) return set_error(SGC_EINVAL, "%s: null pointer", who);
  if (N <= 0 || Nq <= 0 || C <= 0 || n_valid <= 0 || n_pairs <= 0) return set_error(SGC_EINVAL, "%s: non-positive size", who);
  hipStream_t st = (hipStream_t)stream;
  if (C % 4 == 0 && aligned16(grad_mean, grad_feat)) {
    const int64_t total = (int64_t)n_valid * (C / 4);
    const int grid = (int)(total / 256 + 1 < 65536 ? total / 256 + 1 : 65536);
    hipLaunchKernelGGL(view_mean_backward_kernel<float4>, dim3(grid), dim3(256), 0, st, reinterpret_cast<const float4 *>(grad_mean), slot,
                       valid_index, reinterpret_cast<float4 *>(grad_feat), N, Nq, C / 4, n_valid, n_pairs);
  } else {
    const int64_t total = (int64_t)n_valid * C;
    const int grid = (int)(total / 256 + 1 < 65536 ? total / 256 + 1 : 65536);
    hipLaunchKernelGGL(view_mean_backward_kernel<float>, dim3(grid), dim3(256), 0, st, grad_mean, slot, valid_index, grad_feat, N, Nq, C,
                       n_valid, n_pairs);
  }
  return check_launch("view_mean_backward_kernel");
}
