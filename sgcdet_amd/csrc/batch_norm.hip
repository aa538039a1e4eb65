// Training-mode BatchNorm over channels-last rows [rows, C]: nn.BatchNorm3d over [1, C, X, Y, Z] IS the
// per-channel statistics of the X*Y*Z rows (necks/imvoxelnet.py:36-64,146-173 -- every convolution of the neck is followed by one).
//
//   forward    batch mean / biased variance per channel (Welford per thread, Chan's merge across threads and workgroups in a
//              FIXED order: the same bits every run), the running-statistics update of nn.BatchNorm (unbiased variance,
//              momentum), y = tail((x - mean) * invstd * weight + bias).
//   backward   dweight = sum g * xhat, dbias = sum g, dx = weight * invstd * (g - dbias / rows - xhat * dweight / rows), g = the
//              incoming gradient behind the tail's gate.
//
// One set of kernels serves every entry: rows of pitch ld >= C, a tail 0 / 1 / 2.  sgc_bn_rows_forward / _backward and
// sgc_bn_rows_act_forward / _backward are these kernels at ld == C with tails 0 / 1; sgc_bn_rows_padded_forward / _backward
// (include/sgcdet_amd_depth_train.h: the regulation U-Nets of DepthNet_Fusion in training) pass pitch and tail through.
// sgc_bn_rows_sync_* (include/sgcdet_amd_syncbn.h) are the same passes cut where the caller of a SyncBatchNorm runs its
// collective: local statistics | merge of the ranks + apply, local sums | apply.
//
// Round 2 ran torch's channels-last batch-norm kernels here: 43 us (statistics) + 52 us (backward reduction) per layer for
// 26 MB tensors, 1.5 ms of a 25 ms training step.  These are plain column reductions: a workgroup walks a slab of rows with
// 16-byte loads (a thread owns 4 channels), partial results meet in a small workspace.
#include "common.hpp"
#include "../../include/sgcdet_amd_depth_train.h"
#include "../../include/sgcdet_amd_syncbn.h"

namespace sgc {

constexpr int BN_T = 256;          // threads per workgroup
constexpr int BN_MAXG = 256;       // slabs (workgroups of the partial kernels)

// merge (nb, mb, M2b) into (na, ma, M2a): Chan et al.
__device__ __forceinline__ void chan_merge(float &na, float &ma, float &M2a, float nb, float mb, float M2b) {
  if (nb == 0.f) return;
  const float n = na + nb, d = mb - ma, f = nb / n;
  ma += d * f;
  M2a += M2b + d * d * na * f;
  na = n;
}

// ---- pitch and tail -------------------------------------------------------------------------------------------------------------
// Rows of pitch ld >= C: columns [C, ld) of the inputs are never read, those of the outputs are written as +0.0.  Statistics,
// parameters and the workspace are [C] wide.  The pitch enters the addresses alone, never a value: the same rows give the same
// bits at every ld (tests/test_gpu_depth_unets_train.py pins ld == C against ld > C).
//   tail 0: y = bn(x) + residual?      tail 1: y = relu(bn(x) + residual?)      tail 2: y = relu(bn(x)) + residual

// bn(x) of one element with its rounding spelled out (subtract, multiply, one fused multiply-add), so that no choice of the
// compiler's can separate the forward from the tail-2 backward, which recomputes its gate from exactly this
__device__ __forceinline__ float bn_value(float v, float m, float s, float w, float b) {
  return __fmaf_rn(__fmul_rn(__fsub_rn(v, m), s), w, b);
}

// dx of one element, likewise spelled out:
// weight * invstd * (g - dbias / rows - xhat * dweight / rows) with the two subtractions as fused multiply-adds
__device__ __forceinline__ float bn_dx(float v, float g, float m, float is, float w, float db, float dw, float inv_rows) {
  const float xhat = __fmul_rn(__fsub_rn(v, m), is);
  const float t = __fmaf_rn(-inv_rows, __fmul_rn(xhat, dw), __fmaf_rn(-inv_rows, db, g));
  return __fmul_rn(__fmul_rn(w, is), t);
}

// partial statistics of slab g: ws[(g * 2 + 0) * C + c] = mean, ws[(g * 2 + 1) * C + c] = M2 (sum of squared deviations)
__global__ __launch_bounds__(BN_T) void bn_stats_partial_kernel(const float *__restrict__ x, float *__restrict__ ws, int rows, int C, int ld,
                                                                int rows_per_slab) {
  extern __shared__ float bn_lds[];                    // [RL][CG * 4][3]
  const int C4 = C >> 2;
  const int CG = C4 < BN_T ? C4 : BN_T;                // column groups (float4) handled at once
  const int RL = BN_T / CG;                            // row lanes
  const int tid = threadIdx.x, cg = tid % CG, rl = tid / CG;
  const int r_lo = blockIdx.x * rows_per_slab, r_hi = min(rows, r_lo + rows_per_slab);
  for (int c0 = 0; c0 < C4; c0 += CG) {
    const int c4 = c0 + cg;
    float n = 0.f, mean[4] = {0.f, 0.f, 0.f, 0.f}, M2[4] = {0.f, 0.f, 0.f, 0.f};
    if (c4 < C4 && rl < RL) {
      for (int r = r_lo + rl; r < r_hi; r += RL) {
        const float4 v4 = *reinterpret_cast<const float4 *>(x + (int64_t)r * ld + c4 * 4);
        const float v[4] = {v4.x, v4.y, v4.z, v4.w};
        n += 1.f;
        const float inv = __frcp_rn(n);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float d = v[e] - mean[e];
          mean[e] += d * inv;
          M2[e] += d * (v[e] - mean[e]);
        }
      }
    }
    // row lanes -> one partial per channel, merged in lane order by lane 0 of the column group
    if (rl < RL && c4 < C4) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        bn_lds[((rl * CG + cg) * 4 + e) * 3 + 0] = n;
        bn_lds[((rl * CG + cg) * 4 + e) * 3 + 1] = mean[e];
        bn_lds[((rl * CG + cg) * 4 + e) * 3 + 2] = M2[e];
      }
    }
    __syncthreads();
    if (rl == 0 && c4 < C4) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float na = n, ma = mean[e], Ma = M2[e];
        for (int l = 1; l < RL; ++l) {
          const float *q = bn_lds + ((l * CG + cg) * 4 + e) * 3;
          chan_merge(na, ma, Ma, q[0], q[1], q[2]);
        }
        ws[((int64_t)blockIdx.x * 2 + 0) * C + c4 * 4 + e] = ma;
        ws[((int64_t)blockIdx.x * 2 + 1) * C + c4 * 4 + e] = Ma;
      }
    }
    __syncthreads();
  }
}

// merge the slabs of one channel.  BN_FJ lanes per channel each merge a contiguous run of slabs in order, lane 0 merges the BN_FJ
// results in lane order: a fixed tree, the same bits every run.  True on the lane that then holds channel c's (count, mean, M2)
constexpr int BN_FJ = 8, BN_FC = BN_T / BN_FJ;       // lanes per channel, channels per workgroup
__device__ __forceinline__ bool bn_merge_slabs(const float *__restrict__ ws, int G, int rows, int rows_per_slab, int C, int &c, float &na, float &ma,
                                               float &Ma) {
  __shared__ float part[BN_FJ][BN_FC][3];
  const int cl = threadIdx.x % BN_FC, j = threadIdx.x / BN_FC;
  c = blockIdx.x * BN_FC + cl;
  const int per = (G + BN_FJ - 1) / BN_FJ;
  na = 0.f, ma = 0.f, Ma = 0.f;
  if (c < C) {
    for (int g = j * per; g < min(G, (j + 1) * per); ++g) {
      const int cnt = min(rows, (g + 1) * rows_per_slab) - g * rows_per_slab;
      if (cnt <= 0) break;
      chan_merge(na, ma, Ma, (float)cnt, ws[((int64_t)g * 2 + 0) * C + c], ws[((int64_t)g * 2 + 1) * C + c]);
    }
  }
  part[j][cl][0] = na; part[j][cl][1] = ma; part[j][cl][2] = Ma;
  __syncthreads();
  if (j != 0 || c >= C) return false;
  for (int l = 1; l < BN_FJ; ++l) chan_merge(na, ma, Ma, part[l][cl][0], part[l][cl][1], part[l][cl][2]);
  return true;
}

// batch statistics, running statistics (nn.BatchNorm: unbiased variance), invstd of the merged slabs
__global__ __launch_bounds__(BN_T) void bn_stats_final_kernel(const float *__restrict__ ws, int G, int rows, int rows_per_slab, int C, float eps,
                                                              float momentum, float *__restrict__ mean_out, float *__restrict__ invstd_out,
                                                              float *__restrict__ running_mean, float *__restrict__ running_var) {
  int c;
  float na, ma, Ma;
  if (!bn_merge_slabs(ws, G, rows, rows_per_slab, C, c, na, ma, Ma)) return;
  const float var = Ma / (float)rows;
  mean_out[c] = ma;
  invstd_out[c] = 1.0f / sqrtf(var + eps);
  if (running_mean) running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * ma;
  if (running_var) running_var[c] = (1.f - momentum) * running_var[c] + momentum * (rows > 1 ? Ma / (float)(rows - 1) : var);
}

// ---- the seam of SyncBatchNorm (include/sgcdet_amd_syncbn.h): local | collective | global ---------------------------
// The local half of the forward ends where bn_stats_final_kernel would turn (mean, M2) into a variance: this rank's merged slabs
// leave as packed [mean (C) | M2 (C) | count (1)], M2 the SUM of squared deviations, so that the ranks meet in the Chan step the
// slabs met in
__global__ __launch_bounds__(BN_T) void bn_sync_stats_final_kernel(const float *__restrict__ ws, int G, int rows, int rows_per_slab, int C,
                                                                   float *__restrict__ packed) {
  int c;
  float na, ma, Ma;
  if (!bn_merge_slabs(ws, G, rows, rows_per_slab, C, c, na, ma, Ma)) return;
  packed[c] = ma;
  packed[C + c] = Ma;
  if (c == 0) packed[2 * C] = (float)rows;
}

// The global half: the ranks of gathered [world, 2C + 1] merged in rank order (every rank computes the same bits; one rank is the
// identity: its own mean and M2 pass through untouched), then what bn_stats_final_kernel does with rows -> the total count, which
// stays on the device as 1 / N for the backward.  One thread per channel: the loop is world long
__global__ __launch_bounds__(BN_T) void bn_sync_merge_kernel(const float *__restrict__ gathered, int world, int C, float eps, float momentum,
                                                             float *__restrict__ mean_out, float *__restrict__ invstd_out,
                                                             float *__restrict__ inv_count_out, float *__restrict__ running_mean,
                                                             float *__restrict__ running_var) {
  const int c = blockIdx.x * BN_T + threadIdx.x;
  if (c >= C) return;
  const int64_t pitch = 2 * (int64_t)C + 1;
  float na = gathered[2 * C], ma = gathered[c], Ma = gathered[C + c];
  for (int r = 1; r < world; ++r) {
    const float *q = gathered + r * pitch;
    chan_merge(na, ma, Ma, q[2 * C], q[c], q[C + c]);
  }
  const float var = Ma / na;
  mean_out[c] = ma;
  invstd_out[c] = 1.0f / sqrtf(var + eps);
  if (running_mean) running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * ma;
  if (running_var) running_var[c] = (1.f - momentum) * running_var[c] + momentum * (na > 1.f ? Ma / (na - 1.f) : var);
  if (c == 0) inv_count_out[0] = 1.0f / na;
}

// the normalisation with its elementwise tail (round 5): the ResBlock tail `relu(norm2(conv2) + identity)` and the `relu(norm(conv))`
// pairs of the neck (necks/imvoxelnet.py:36-64) in this pass instead of two more elementwise kernels.  One float4 of a row of
// pitch ld4 (in float4) per step; the float4s at and beyond C4 are the padding
__global__ __launch_bounds__(BN_T) void bn_apply_kernel(const float4 *__restrict__ x, const float *__restrict__ mean, const float *__restrict__ invstd,
                                                        const float *__restrict__ w, const float *__restrict__ b, float4 *__restrict__ y,
                                                        int64_t total4, int C4, int ld4, const float4 *__restrict__ residual, int tail) {
  for (int64_t i = (int64_t)blockIdx.x * BN_T + threadIdx.x; i < total4; i += (int64_t)gridDim.x * BN_T) {
    const int c4 = (int)(i % ld4);
    if (c4 >= C4) { y[i] = make_float4(0.f, 0.f, 0.f, 0.f); continue; }
    const int c = c4 * 4;
    const float4 v = x[i];
    const float4 m = *reinterpret_cast<const float4 *>(mean + c), s = *reinterpret_cast<const float4 *>(invstd + c);
    const float4 ww = *reinterpret_cast<const float4 *>(w + c), bb = *reinterpret_cast<const float4 *>(b + c);
    float4 o = make_float4(bn_value(v.x, m.x, s.x, ww.x, bb.x), bn_value(v.y, m.y, s.y, ww.y, bb.y), bn_value(v.z, m.z, s.z, ww.z, bb.z),
                           bn_value(v.w, m.w, s.w, ww.w, bb.w));
    if (tail == 2) o = relu_nan(o);
    if (residual) { const float4 r = residual[i]; o.x += r.x; o.y += r.y; o.z += r.z; o.w += r.w; }
    if (tail == 1) o = relu_nan(o);
    y[i] = o;
  }
}

// the gated incoming gradient of one float4: tail 1 reads the gate off the saved output, tail 2 off bn(x) recomputed, tail 0 has none
// (a gate value of 1).  Selects: a NaN gate value lets the gradient pass, as torch's threshold_backward does; a closed gate drops a
// NaN gradient.
__device__ __forceinline__ float4 bnp_gate(float4 g4, int tail, const float *__restrict__ y, int64_t at, float4 v4, float4 m4, float4 i4,
                                           const float *__restrict__ w, const float *__restrict__ b, int c) {
  float t0 = 1.f, t1 = 1.f, t2 = 1.f, t3 = 1.f;
  if (tail == 1) {
    const float4 y4 = *reinterpret_cast<const float4 *>(y + at);
    t0 = y4.x; t1 = y4.y; t2 = y4.z; t3 = y4.w;
  } else if (tail == 2) {
    const float4 ww = *reinterpret_cast<const float4 *>(w + c), bb = *reinterpret_cast<const float4 *>(b + c);
    t0 = bn_value(v4.x, m4.x, i4.x, ww.x, bb.x); t1 = bn_value(v4.y, m4.y, i4.y, ww.y, bb.y);
    t2 = bn_value(v4.z, m4.z, i4.z, ww.z, bb.z); t3 = bn_value(v4.w, m4.w, i4.w, ww.w, bb.w);
  }
  return make_float4(t0 <= 0.f ? 0.f : g4.x, t1 <= 0.f ? 0.f : g4.y, t2 <= 0.f ? 0.f : g4.z, t3 <= 0.f ? 0.f : g4.w);
}

// partial sums of slab g: ws[(g * 2 + 0) * C + c] = sum g, ws[(g * 2 + 1) * C + c] = sum g * xhat, g = the gated gradient.
// The tail is a template parameter of the two backward kernels that gate: with a runtime tail the row loop keeps the gate's branches
// and the plain backward loses 1 - 4 us per layer of the neck (profiles/r23_bn_ab.txt)
template <int TAIL>
__global__ __launch_bounds__(BN_T) void bn_bwd_partial_kernel(const float *__restrict__ x, const float *__restrict__ dy, const float *__restrict__ mean,
                                                              const float *__restrict__ invstd, const float *__restrict__ w,
                                                              const float *__restrict__ b, float *__restrict__ ws, int rows, int C, int ld,
                                                              int rows_per_slab, const float *__restrict__ y_or_null) {
  extern __shared__ float bn_lds[];                    // [RL][CG * 4][2]
  const int C4 = C >> 2;
  const int CG = C4 < BN_T ? C4 : BN_T, RL = BN_T / CG;
  const int tid = threadIdx.x, cg = tid % CG, rl = tid / CG;
  const int r_lo = blockIdx.x * rows_per_slab, r_hi = min(rows, r_lo + rows_per_slab);
  for (int c0 = 0; c0 < C4; c0 += CG) {
    const int c4 = c0 + cg;
    float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
    if (c4 < C4 && rl < RL) {
      const float4 m4 = *reinterpret_cast<const float4 *>(mean + c4 * 4), i4 = *reinterpret_cast<const float4 *>(invstd + c4 * 4);
      const float m[4] = {m4.x, m4.y, m4.z, m4.w}, is[4] = {i4.x, i4.y, i4.z, i4.w};
      for (int r = r_lo + rl; r < r_hi; r += RL) {
        const int64_t at = (int64_t)r * ld + c4 * 4;
        const float4 v4 = *reinterpret_cast<const float4 *>(x + at);
        const float4 g4 = bnp_gate(*reinterpret_cast<const float4 *>(dy + at), TAIL, y_or_null, at, v4, m4, i4, w, b, c4 * 4);
        const float v[4] = {v4.x, v4.y, v4.z, v4.w}, g[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          s1[e] += g[e];
          s2[e] += g[e] * ((v[e] - m[e]) * is[e]);
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        bn_lds[((rl * CG + cg) * 4 + e) * 2 + 0] = s1[e];
        bn_lds[((rl * CG + cg) * 4 + e) * 2 + 1] = s2[e];
      }
    }
    __syncthreads();
    if (rl == 0 && c4 < C4) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float a = s1[e], bsum = s2[e];
        for (int l = 1; l < RL; ++l) {
          a += bn_lds[((l * CG + cg) * 4 + e) * 2 + 0];
          bsum += bn_lds[((l * CG + cg) * 4 + e) * 2 + 1];
        }
        ws[((int64_t)blockIdx.x * 2 + 0) * C + c4 * 4 + e] = a;
        ws[((int64_t)blockIdx.x * 2 + 1) * C + c4 * 4 + e] = bsum;
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(BN_T) void bn_bwd_final_kernel(const float *__restrict__ ws, int G, int C, float *__restrict__ dw, float *__restrict__ db) {
  __shared__ float part[BN_FJ][BN_FC][2];
  const int cl = threadIdx.x % BN_FC, j = threadIdx.x / BN_FC;
  const int c = blockIdx.x * BN_FC + cl;
  const int per = (G + BN_FJ - 1) / BN_FJ;
  float a = 0.f, b = 0.f;
  if (c < C) {
    for (int g = j * per; g < min(G, (j + 1) * per); ++g) {     // runs of slabs in order, then the runs in order: the same bits every run
      a += ws[((int64_t)g * 2 + 0) * C + c];
      b += ws[((int64_t)g * 2 + 1) * C + c];
    }
  }
  part[j][cl][0] = a; part[j][cl][1] = b;
  __syncthreads();
  if (j != 0 || c >= C) return;
  for (int l = 1; l < BN_FJ; ++l) { a += part[l][cl][0]; b += part[l][cl][1]; }
  db[c] = a;
  dw[c] = b;
}

// dres: the gradient of the added identity -- behind the gate for tails 0 / 1 (the add sits in front of the ReLU; tail 0 has no
// gate: the incoming gradient), the incoming gradient itself for tail 2 (the add sits behind it)
template <int TAIL>
__device__ __forceinline__ void bn_bwd_apply_rows(const float *__restrict__ x, const float *__restrict__ dy, const float *__restrict__ mean,
                                                  const float *__restrict__ invstd, const float *__restrict__ w, const float *__restrict__ b,
                                                  const float *__restrict__ dw, const float *__restrict__ db, float *__restrict__ dx,
                                                  int64_t total4, int C4, int ld4, float inv_rows, const float *__restrict__ y_or_null,
                                                  float *__restrict__ dres_or_null) {
  for (int64_t i = (int64_t)blockIdx.x * BN_T + threadIdx.x; i < total4; i += (int64_t)gridDim.x * BN_T) {
    const int c4 = (int)(i % ld4);
    float4 *dx4 = reinterpret_cast<float4 *>(dx) + i;
    if (c4 >= C4) {
      *dx4 = make_float4(0.f, 0.f, 0.f, 0.f);
      if (dres_or_null) reinterpret_cast<float4 *>(dres_or_null)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      continue;
    }
    const int c = c4 * 4;
    const float4 v4 = reinterpret_cast<const float4 *>(x)[i], raw = reinterpret_cast<const float4 *>(dy)[i];
    const float4 m4 = *reinterpret_cast<const float4 *>(mean + c), i4 = *reinterpret_cast<const float4 *>(invstd + c);
    const float4 g4 = bnp_gate(raw, TAIL, y_or_null, i * 4, v4, m4, i4, w, b, c);
    if (dres_or_null) {
      float4 *dres4 = reinterpret_cast<float4 *>(dres_or_null) + i;
      if (TAIL == 2) *dres4 = raw; else *dres4 = g4;
    }
    const float4 w4 = *reinterpret_cast<const float4 *>(w + c), db4 = *reinterpret_cast<const float4 *>(db + c);
    const float4 dw4 = *reinterpret_cast<const float4 *>(dw + c);
    *dx4 = make_float4(bn_dx(v4.x, g4.x, m4.x, i4.x, w4.x, db4.x, dw4.x, inv_rows), bn_dx(v4.y, g4.y, m4.y, i4.y, w4.y, db4.y, dw4.y, inv_rows),
                       bn_dx(v4.z, g4.z, m4.z, i4.z, w4.z, db4.z, dw4.z, inv_rows), bn_dx(v4.w, g4.w, m4.w, i4.w, w4.w, db4.w, dw4.w, inv_rows));
  }
}

template <int TAIL>
__global__ __launch_bounds__(BN_T) void bn_bwd_apply_kernel(const float *__restrict__ x, const float *__restrict__ dy, const float *__restrict__ mean,
                                                            const float *__restrict__ invstd, const float *__restrict__ w,
                                                            const float *__restrict__ b, const float *__restrict__ dw,
                                                            const float *__restrict__ db, float *__restrict__ dx, int64_t total4, int C4, int ld4,
                                                            float inv_rows, const float *__restrict__ y_or_null,
                                                            float *__restrict__ dres_or_null) {
  bn_bwd_apply_rows<TAIL>(x, dy, mean, invstd, w, b, dw, db, dx, total4, C4, ld4, inv_rows, y_or_null, dres_or_null);
}

// the same pass behind the all-reduce of SyncBatchNorm: sums = [sum g | sum g * xhat] over the rows of ALL ranks, and 1 / N of all
// ranks read from device memory (bn_sync_merge_kernel left it there: no host read-back between the passes).  Dense rows, tails 0 / 1
template <int TAIL>
__global__ __launch_bounds__(BN_T) void bn_sync_bwd_apply_kernel(const float *__restrict__ x, const float *__restrict__ dy,
                                                                 const float *__restrict__ mean, const float *__restrict__ invstd,
                                                                 const float *__restrict__ w, const float *__restrict__ sums,
                                                                 const float *__restrict__ inv_count, float *__restrict__ dx, int64_t total4,
                                                                 int C4, const float *__restrict__ y_or_null, float *__restrict__ dres_or_null) {
  bn_bwd_apply_rows<TAIL>(x, dy, mean, invstd, w, nullptr, sums + C4 * 4, sums, dx, total4, C4, C4, inv_count[0], y_or_null, dres_or_null);
}

static void bn_geometry(int rows, int &G, int &rows_per_slab) {
  G = ceil_div(rows, 64);
  if (G > BN_MAXG) G = BN_MAXG;
  rows_per_slab = ceil_div(rows, G);
  G = ceil_div(rows, rows_per_slab);
}

}  // namespace sgc

using namespace sgc;

extern "C" int64_t sgc_bn_rows_workspace_floats(int rows, int C) {
  if (rows <= 0 || C <= 0) return 0;
  int G, rps;
  bn_geometry(rows, G, rps);
  return (int64_t)G * 2 * C;
}

// ---- the two launchers: every entry below is an argument mapping onto one of them; `who` names the entry in the messages ----------
static int bn_check(const char *who, int rows, int C, int ld, int tail) {
  if (rows <= 0 || C <= 0) return set_error(SGC_EINVAL, "%s: bad size", who);
  if (C % 4) return set_error(SGC_EUNSUP, "%s: needs C %% 4 == 0", who);
  if (ld < C) return set_error(SGC_EUNSUP, "%s: row pitch %d below C = %d", who, ld, C);
  if (ld % 4) return set_error(SGC_EUNSUP, "%s: needs a row pitch %% 4 == 0 (got %d)", who, ld);
  if (tail < 0 || tail > 2) return set_error(SGC_EUNSUP, "%s: tail must be 0, 1 or 2", who);
  return SGC_OK;
}

static int bn_forward_launch(const char *who, const float *x, const float *weight, const float *bias, float *running_mean_or_null,
                             float *running_var_or_null, float momentum, float eps, const float *residual_or_null, int tail, float *y,
                             float *mean_out, float *invstd_out, float *workspace, int64_t workspace_floats, int rows, int C, int ld,
                             sgc_stream_t stream) {
  if (!x || !weight || !bias || !y || !mean_out || !invstd_out || !workspace) return set_error(SGC_EINVAL, "%s: null pointer", who);
  int rc = bn_check(who, rows, C, ld, tail);
  if (rc) return rc;
  if (tail == 2 && !residual_or_null) return set_error(SGC_EINVAL, "%s: tail 2 (relu, then add) needs a residual", who);
  if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)residual_or_null | (uintptr_t)weight | (uintptr_t)bias | (uintptr_t)mean_out |
       (uintptr_t)invstd_out) & 15)
    return set_error(SGC_EINVAL, "%s: pointers must be 16-byte aligned", who);
  int G, rps;
  bn_geometry(rows, G, rps);
  if (workspace_floats < (int64_t)G * 2 * C) return set_error(SGC_EINVAL, "%s: workspace too small", who);
  hipStream_t st = (hipStream_t)stream;
  const int C4 = C / 4, CG = C4 < BN_T ? C4 : BN_T, RL = BN_T / CG;
  const size_t smem = (size_t)RL * CG * 4 * 3 * sizeof(float);
  hipLaunchKernelGGL(bn_stats_partial_kernel, dim3(G), dim3(BN_T), smem, st, x, workspace, rows, C, ld, rps);
  rc = check_launch("bn_stats_partial_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(bn_stats_final_kernel, dim3(ceil_div(C, BN_FC)), dim3(BN_T), 0, st, (const float *)workspace, G, rows, rps, C, eps, momentum,
                     mean_out, invstd_out, running_mean_or_null, running_var_or_null);
  rc = check_launch("bn_stats_final_kernel");
  if (rc) return rc;
  const int64_t total4 = (int64_t)rows * (ld / 4);
  const int g = (int)((total4 + BN_T - 1) / BN_T < 4096 ? (total4 + BN_T - 1) / BN_T : 4096);
  hipLaunchKernelGGL(bn_apply_kernel, dim3(g), dim3(BN_T), 0, st, reinterpret_cast<const float4 *>(x), (const float *)mean_out,
                     (const float *)invstd_out, weight, bias, reinterpret_cast<float4 *>(y), total4, C4, ld / 4,
                     reinterpret_cast<const float4 *>(residual_or_null), tail);
  return check_launch("bn_apply_kernel");
}

static int bn_backward_launch(const char *who, const float *x, const float *dy, const float *y_or_null, const float *mean, const float *invstd,
                              const float *weight, const float *bias_or_null, float *dx, float *dweight, float *dbias,
                              float *dresidual_or_null, int tail, float *workspace, int64_t workspace_floats, int rows, int C, int ld,
                              sgc_stream_t stream) {
  if (!x || !dy || !mean || !invstd || !weight || !dx || !dweight || !dbias || !workspace) return set_error(SGC_EINVAL, "%s: null pointer", who);
  int rc = bn_check(who, rows, C, ld, tail);
  if (rc) return rc;
  if (tail == 1 && !y_or_null) return set_error(SGC_EINVAL, "%s: tail 1 reads its gate off the forward's output: y is null", who);
  if (tail == 2 && !bias_or_null) return set_error(SGC_EINVAL, "%s: tail 2 recomputes its gate from x: bias is null", who);
  // weight, dweight and dbias too, for every entry: the apply kernel reads them with 16-byte loads (include/sgcdet_amd.h asks for
  // 16-byte aligned pointers in all of these calls)
  if (((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dx | (uintptr_t)y_or_null | (uintptr_t)dresidual_or_null | (uintptr_t)mean |
       (uintptr_t)invstd | (uintptr_t)weight | (uintptr_t)bias_or_null | (uintptr_t)dweight | (uintptr_t)dbias) & 15)
    return set_error(SGC_EINVAL, "%s: pointers must be 16-byte aligned", who);
  int G, rps;
  bn_geometry(rows, G, rps);
  if (workspace_floats < (int64_t)G * 2 * C) return set_error(SGC_EINVAL, "%s: workspace too small", who);
  hipStream_t st = (hipStream_t)stream;
  const int C4 = C / 4, CG = C4 < BN_T ? C4 : BN_T, RL = BN_T / CG;
  const size_t smem = (size_t)RL * CG * 4 * 2 * sizeof(float);
  const auto partial = tail == 0 ? bn_bwd_partial_kernel<0> : tail == 1 ? bn_bwd_partial_kernel<1> : bn_bwd_partial_kernel<2>;
  const auto apply = tail == 0 ? bn_bwd_apply_kernel<0> : tail == 1 ? bn_bwd_apply_kernel<1> : bn_bwd_apply_kernel<2>;
  hipLaunchKernelGGL(partial, dim3(G), dim3(BN_T), smem, st, x, dy, mean, invstd, weight, bias_or_null, workspace, rows, C, ld, rps, y_or_null);
  rc = check_launch("bn_bwd_partial_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(bn_bwd_final_kernel, dim3(ceil_div(C, BN_FC)), dim3(BN_T), 0, st, (const float *)workspace, G, C, dweight, dbias);
  rc = check_launch("bn_bwd_final_kernel");
  if (rc) return rc;
  const int64_t total4 = (int64_t)rows * (ld / 4);
  const int g = (int)((total4 + BN_T - 1) / BN_T < 4096 ? (total4 + BN_T - 1) / BN_T : 4096);
  hipLaunchKernelGGL(apply, dim3(g), dim3(BN_T), 0, st, x, dy, mean, invstd, weight, bias_or_null, (const float *)dweight,
                     (const float *)dbias, dx, total4, C4, ld / 4, 1.0f / (float)rows, y_or_null, dresidual_or_null);
  return check_launch("bn_bwd_apply_kernel");
}

// ---- the entries: dense rows (ld == C, include/sgcdet_amd.h), then the padded form (include/sgcdet_amd_depth_train.h) -------------
extern "C" int sgc_bn_rows_forward(const float *x, const float *weight, const float *bias, float *running_mean_or_null,
                                   float *running_var_or_null, float momentum, float eps, float *y, float *mean_out,
                                   float *invstd_out, float *workspace, int64_t workspace_floats, int rows, int C,
                                   sgc_stream_t stream) {
  return bn_forward_launch("sgc_bn_rows_forward", x, weight, bias, running_mean_or_null, running_var_or_null, momentum, eps, nullptr, 0, y,
                           mean_out, invstd_out, workspace, workspace_floats, rows, C, C, stream);
}
// y = relu?(bn(x) + residual?)
extern "C" int sgc_bn_rows_act_forward(const float *x, const float *weight, const float *bias, float *running_mean_or_null,
                                       float *running_var_or_null, float momentum, float eps, const float *residual_or_null, int relu,
                                       float *y, float *mean_out, float *invstd_out, float *workspace, int64_t workspace_floats,
                                       int rows, int C, sgc_stream_t stream) {
  return bn_forward_launch("sgc_bn_rows_act_forward", x, weight, bias, running_mean_or_null, running_var_or_null, momentum, eps,
                           residual_or_null, relu ? 1 : 0, y, mean_out, invstd_out, workspace, workspace_floats, rows, C, C, stream);
}
extern "C" int sgc_bn_rows_backward(const float *x, const float *dy, const float *mean, const float *invstd, const float *weight,
                                    float *dx, float *dweight, float *dbias, float *workspace, int64_t workspace_floats, int rows,
                                    int C, sgc_stream_t stream) {
  return bn_backward_launch("sgc_bn_rows_backward", x, dy, nullptr, mean, invstd, weight, nullptr, dx, dweight, dbias, nullptr, 0, workspace,
                            workspace_floats, rows, C, C, stream);
}
// backward of sgc_bn_rows_act_forward: y_relu_or_null = its output when relu was set (the gradient passes where y > 0), dresidual_or_null
// = where to put the gradient of the added identity (the masked incoming gradient; null when there was none or nobody needs it)
extern "C" int sgc_bn_rows_act_backward(const float *x, const float *dy, const float *y_relu_or_null, const float *mean, const float *invstd,
                                        const float *weight, float *dx, float *dweight, float *dbias, float *dresidual_or_null,
                                        float *workspace, int64_t workspace_floats, int rows, int C, sgc_stream_t stream) {
  return bn_backward_launch("sgc_bn_rows_act_backward", x, dy, y_relu_or_null, mean, invstd, weight, nullptr, dx, dweight, dbias,
                            dresidual_or_null, y_relu_or_null ? 1 : 0, workspace, workspace_floats, rows, C, C, stream);
}

extern "C" int sgc_bn_rows_padded_forward(const float *x, const float *weight, const float *bias, float *running_mean_or_null,
                                          float *running_var_or_null, float momentum, float eps, const float *residual_or_null, int tail,
                                          float *y, float *mean_out, float *invstd_out, float *workspace, int64_t workspace_floats,
                                          int rows, int C, int ld, sgc_stream_t stream) {
  return bn_forward_launch("sgc_bn_rows_padded_forward", x, weight, bias, running_mean_or_null, running_var_or_null, momentum, eps,
                           residual_or_null, tail, y, mean_out, invstd_out, workspace, workspace_floats, rows, C, ld, stream);
}
extern "C" int sgc_bn_rows_padded_backward(const float *x, const float *dy, const float *y_or_null, const float *mean, const float *invstd,
                                           const float *weight, const float *bias_or_null, float *dx, float *dweight, float *dbias,
                                           float *dresidual_or_null, int tail, float *workspace, int64_t workspace_floats, int rows, int C,
                                           int ld, sgc_stream_t stream) {
  return bn_backward_launch("sgc_bn_rows_padded_backward", x, dy, y_or_null, mean, invstd, weight, bias_or_null, dx, dweight, dbias,
                            dresidual_or_null, tail, workspace, workspace_floats, rows, C, ld, stream);
}

// ---- SyncBatchNorm (include/sgcdet_amd_syncbn.h): the two launchers above cut at the collective ------------------------------------
static int bn_sync_check(const char *who, int rows, int C) {
  int rc = bn_check(who, rows, C, C, 0);
  if (rc) return rc;
  if (rows >= (1 << 24)) return set_error(SGC_EUNSUP, "%s: counts travel as fp32: rows = %d is not below 2^24", who, rows);
  return SGC_OK;
}

static int bn_apply_grid(int64_t total4) { return (int)((total4 + BN_T - 1) / BN_T < 4096 ? (total4 + BN_T - 1) / BN_T : 4096); }

extern "C" int sgc_bn_rows_sync_stats(const float *x, float *stats, float *workspace, int64_t workspace_floats, int rows, int C,
                                      sgc_stream_t stream) {
  const char *who = "sgc_bn_rows_sync_stats";
  if (!x || !stats || !workspace) return set_error(SGC_EINVAL, "%s: null pointer", who);
  int rc = bn_sync_check(who, rows, C);
  if (rc) return rc;
  if ((uintptr_t)x & 15) return set_error(SGC_EINVAL, "%s: pointers must be 16-byte aligned", who);
  int G, rps;
  bn_geometry(rows, G, rps);
  if (workspace_floats < (int64_t)G * 2 * C) return set_error(SGC_EINVAL, "%s: workspace too small", who);
  hipStream_t st = (hipStream_t)stream;
  const int C4 = C / 4, CG = C4 < BN_T ? C4 : BN_T, RL = BN_T / CG;
  const size_t smem = (size_t)RL * CG * 4 * 3 * sizeof(float);
  hipLaunchKernelGGL(bn_stats_partial_kernel, dim3(G), dim3(BN_T), smem, st, x, workspace, rows, C, C, rps);
  rc = check_launch("bn_stats_partial_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(bn_sync_stats_final_kernel, dim3(ceil_div(C, BN_FC)), dim3(BN_T), 0, st, (const float *)workspace, G, rows, rps, C, stats);
  return check_launch("bn_sync_stats_final_kernel");
}

extern "C" int sgc_bn_rows_sync_apply(const float *x, const float *gathered, int world, const float *weight, const float *bias,
                                      float *running_mean_or_null, float *running_var_or_null, float momentum, float eps,
                                      const float *residual_or_null, int relu, float *y, float *mean_out, float *invstd_out,
                                      float *inv_count_out, int rows, int C, sgc_stream_t stream) {
  const char *who = "sgc_bn_rows_sync_apply";
  if (!x || !gathered || !weight || !bias || !y || !mean_out || !invstd_out || !inv_count_out) return set_error(SGC_EINVAL, "%s: null pointer", who);
  int rc = bn_sync_check(who, rows, C);
  if (rc) return rc;
  if (world < 1 || world > SGC_SYNCBN_MAX_WORLD) return set_error(SGC_EUNSUP, "%s: world = %d outside 1 .. %d", who, world, SGC_SYNCBN_MAX_WORLD);
  if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)residual_or_null | (uintptr_t)weight | (uintptr_t)bias | (uintptr_t)mean_out |
       (uintptr_t)invstd_out) & 15)
    return set_error(SGC_EINVAL, "%s: pointers must be 16-byte aligned", who);
  if (((uintptr_t)gathered | (uintptr_t)inv_count_out) & 3) return set_error(SGC_EINVAL, "%s: gathered / inv_count_out must be 4-byte aligned", who);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(bn_sync_merge_kernel, dim3(ceil_div(C, BN_T)), dim3(BN_T), 0, st, gathered, world, C, eps, momentum, mean_out, invstd_out,
                     inv_count_out, running_mean_or_null, running_var_or_null);
  rc = check_launch("bn_sync_merge_kernel");
  if (rc) return rc;
  const int64_t total4 = (int64_t)rows * (C / 4);
  hipLaunchKernelGGL(bn_apply_kernel, dim3(bn_apply_grid(total4)), dim3(BN_T), 0, st, reinterpret_cast<const float4 *>(x), (const float *)mean_out,
                     (const float *)invstd_out, weight, bias, reinterpret_cast<float4 *>(y), total4, C / 4, C / 4,
                     reinterpret_cast<const float4 *>(residual_or_null), relu ? 1 : 0);
  return check_launch("bn_apply_kernel");
}

extern "C" int sgc_bn_rows_sync_backward_sums(const float *x, const float *dy, const float *y_relu_or_null, const float *mean,
                                              const float *invstd, float *sums, float *workspace, int64_t workspace_floats, int rows, int C,
                                              sgc_stream_t stream) {
  const char *who = "sgc_bn_rows_sync_backward_sums";
  if (!x || !dy || !mean || !invstd || !sums || !workspace) return set_error(SGC_EINVAL, "%s: null pointer", who);
  int rc = bn_sync_check(who, rows, C);
  if (rc) return rc;
  if (((uintptr_t)x | (uintptr_t)dy | (uintptr_t)y_relu_or_null | (uintptr_t)mean | (uintptr_t)invstd | (uintptr_t)sums) & 15)
    return set_error(SGC_EINVAL, "%s: pointers must be 16-byte aligned", who);
  int G, rps;
  bn_geometry(rows, G, rps);
  if (workspace_floats < (int64_t)G * 2 * C) return set_error(SGC_EINVAL, "%s: workspace too small", who);
  hipStream_t st = (hipStream_t)stream;
  const int C4 = C / 4, CG = C4 < BN_T ? C4 : BN_T, RL = BN_T / CG;
  const size_t smem = (size_t)RL * CG * 4 * 2 * sizeof(float);
  const auto partial = y_relu_or_null ? bn_bwd_partial_kernel<1> : bn_bwd_partial_kernel<0>;
  hipLaunchKernelGGL(partial, dim3(G), dim3(BN_T), smem, st, x, dy, mean, invstd, (const float *)nullptr, (const float *)nullptr, workspace, rows, C, C,
                     rps, y_relu_or_null);
  rc = check_launch("bn_bwd_partial_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(bn_bwd_final_kernel, dim3(ceil_div(C, BN_FC)), dim3(BN_T), 0, st, (const float *)workspace, G, C, sums + C, sums);
  return check_launch("bn_bwd_final_kernel");
}

extern "C" int sgc_bn_rows_sync_backward_apply(const float *x, const float *dy, const float *y_relu_or_null, const float *mean,
                                               const float *invstd, const float *weight, const float *sums, const float *inv_count, float *dx,
                                               float *dresidual_or_null, int rows, int C, sgc_stream_t stream) {
  const char *who = "sgc_bn_rows_sync_backward_apply";
  if (!x || !dy || !mean || !invstd || !weight || !sums || !inv_count || !dx) return set_error(SGC_EINVAL, "%s: null pointer", who);
  int rc = bn_sync_check(who, rows, C);
  if (rc) return rc;
  if (((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dx | (uintptr_t)y_relu_or_null | (uintptr_t)dresidual_or_null | (uintptr_t)mean |
       (uintptr_t)invstd | (uintptr_t)weight | (uintptr_t)sums) & 15)
    return set_error(SGC_EINVAL, "%s: pointers must be 16-byte aligned", who);
  if ((uintptr_t)inv_count & 3) return set_error(SGC_EINVAL, "%s: inv_count must be 4-byte aligned", who);
  const int64_t total4 = (int64_t)rows * (C / 4);
  const auto apply = y_relu_or_null ? bn_sync_bwd_apply_kernel<1> : bn_sync_bwd_apply_kernel<0>;
  hipLaunchKernelGGL(apply, dim3(bn_apply_grid(total4)), dim3(BN_T), 0, (hipStream_t)stream, x, dy, mean, invstd, weight, sums, inv_count, dx, total4,
                     C / 4, y_relu_or_null, dresidual_or_null);
  return check_launch("bn_sync_bwd_apply_kernel");
}
