// The parameter update of the TRAINING step: global-norm gradient clipping + AdamW over every parameter tensor of
// the model in three launches, no host read-back.
//
//   sgc_grad_sqnorm_batch   sum of squares of every gradient element -> norm_out[0] = sqrt(sum).  Launch 1: a workgroup reduces its
//                           chunk (registers -> wave butterfly -> LDS across the 4 waves) and stores ONE fp32 partial.  Launch 2 (one
//                           wave): lane l adds the partials of its contiguous index range in index order in fp64, the 64 lane sums
//                           meet in a fixed butterfly.  No float atomics anywhere: the order of every addition is a function of the
//                           item list alone, so the norm is bitwise reproducible run to run.
//                           (Stage two is a second launch and not "the last block by ticket": the ticket needs a counter that is
//                           zeroed every call -- a memset node, i.e. a launch of its own -- plus a device-scope fence in every block
//                           of stage one; the second launch costs the same queue slot and keeps stage one a pure read stream.)
//   sgc_adamw_step_batch    torch.optim.AdamW's single-tensor fp32 update (amsgrad = False, maximize = False) with
//                           torch.nn.utils.clip_grad_norm_'s scaling in front, the clip coefficient read from DEVICE memory.  A pure
//                           stream: 16 bytes per lane per array, four arrays in (param, grad, exp_avg, exp_avg_sq), three out;
//                           the clipped gradient exists only in registers (grad is not written).
//
// Both walk a device item list, one item per parameter tensor that has a gradient this step: block -> item by binary search over
// block_start (the pattern of sgc_pack_conv_weight_batch, csrc/weight_pack.hip), then block -> chunk of block_elems elements.
// The reference gets this step from torch / Lightning (main.py:71-72 gradient_clip_val = 35, LightningTools/pl_model.py:92-118).
#include "common.hpp"
#include "../../include/sgcdet_amd_train.h"

namespace sgc {

struct OptimItem {                // = sgc_optim_item of include/sgcdet_amd_train.h (64 bytes)
  float *param;
  const float *grad;
  float *exp_avg, *exp_avg_sq;
  int64_t numel;
  int32_t group, step, block_start, block_elems;
  float bias_correction1, bias_correction2_sqrt;
};
static_assert(sizeof(OptimItem) == 64, "sgc_optim_item is 64 bytes");
static_assert((sizeof(OptimItem) & (sizeof(OptimItem) - 1)) == 0, "sgc_optim_item size is a power of two");
static_assert(sizeof(sgc_optim_item) == sizeof(OptimItem), "header and kernel agree on the item");
static_assert(sizeof(sgc_optim_group) == 40, "sgc_optim_group is five doubles");

struct OptimGroups { sgc_optim_group g[SGC_OPTIM_MAX_GROUPS]; };   // by value: a kernel argument (320 bytes)

constexpr int kOptThreads = 256;
constexpr int kOptUnroll = 4;     // 16-byte loads in flight per lane and array before the first use

// last item with block_start <= b; the loads are uniform over the workgroup (scalar loads)
__device__ __forceinline__ int find_item(const OptimItem *__restrict__ items, int n, int b) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (items[mid].block_start <= b) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// this workgroup's element range [start, start + n) of item `it`; false when the block owns nothing
__device__ __forceinline__ bool block_range(const OptimItem &it, int b, int64_t &start, int &n) {
  if (it.block_elems <= 0 || (it.block_elems & 3)) return false;
  start = (int64_t)(b - it.block_start) * it.block_elems;
  if (start >= it.numel) return false;
  const int64_t left = it.numel - start;
  n = left < it.block_elems ? (int)left : it.block_elems;
  return true;
}

__device__ __forceinline__ bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// The tensors' pointers come out of the item list, so the compiler cannot know their address space and would emit flat_* accesses
// (which also count against lgkmcnt); they are device memory by contract: say so and get global_load / global_store_dwordx4.
typedef float f32x4 __attribute__((ext_vector_type(4)));
#define SGC_GLOBAL __attribute__((address_space(1)))
typedef SGC_GLOBAL float gfloat;
typedef SGC_GLOBAL f32x4 gf32x4;
__device__ __forceinline__ gfloat *as_global(float *p) { return (gfloat *)p; }
__device__ __forceinline__ const gfloat *as_global(const float *p) { return (const gfloat *)p; }

// ---------------------------------------------------------------------------------------------------------------------------
// gradient norm
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kOptThreads) void grad_sqnorm_partial_kernel(const OptimItem *__restrict__ items, int n_items,
                                                                         float *__restrict__ partials) {
  __shared__ float wave_sum[kOptThreads / kWave];
  const int b = blockIdx.x, tid = threadIdx.x;
  const OptimItem it = items[find_item(items, n_items, b)];
  int64_t start; int n = 0;
  float s = 0.f;
  if (block_range(it, b, start, n)) {
    const gfloat *g = as_global(it.grad + start);
    int done = 0;
    if (aligned16(it.grad)) {                       // start is a multiple of 4 elements: the chunk is aligned when the tensor is
      const int nvec = n >> 2;
      const gf32x4 *g4 = (const gf32x4 *)g;
      for (int i = tid; i < nvec; i += kOptThreads * kOptUnroll) {
        f32x4 v[kOptUnroll];
#pragma unroll
        for (int u = 0; u < kOptUnroll; ++u) {
          const int j = i + u * kOptThreads;
          v[u] = j < nvec ? g4[j] : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int u = 0; u < kOptUnroll; ++u) s += v[u].x * v[u].x + v[u].y * v[u].y + v[u].z * v[u].z + v[u].w * v[u].w;
      }
      done = nvec << 2;
    }
    for (int i = done + tid; i < n; i += kOptThreads) s += g[i] * g[i];     // unaligned tensors, and the < 4-element tail
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((tid & 63) == 0) wave_sum[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) partials[b] = (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
}

__global__ __launch_bounds__(kWave) void grad_sqnorm_final_kernel(const float *__restrict__ partials, int n, float *__restrict__ norm_out) {
  const int lane = threadIdx.x;
  const int seg = (n + kWave - 1) / kWave;
  const int i0 = lane * seg, i1 = i0 + seg < n ? i0 + seg : n;
  double s = 0.0;
  for (int i = i0; i < i1; ++i) s += (double)partials[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (lane == 0) norm_out[0] = (float)sqrt(s);
}

// ---------------------------------------------------------------------------------------------------------------------------
// AdamW
// ---------------------------------------------------------------------------------------------------------------------------
struct AdamCoef { float clip, decay, w1, beta2, w2, bc2_sqrt, eps, neg_step_size; };

// torch/optim/adamw.py -> adam.py _single_tensor_adam, in its order: param.mul_(1 - lr * wd); exp_avg.lerp_(grad, 1 - beta1);
// exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2); denom = exp_avg_sq.sqrt() / bias_correction2_sqrt + eps;
// param.addcdiv_(exp_avg, denom, value = -step_size).  Division and sqrt are the correctly rounded forms (hipcc's default).
__device__ __forceinline__ void adamw_one(float &p, float g, float &m, float &v, const AdamCoef &k) {
  g *= k.clip;
  p *= k.decay;
  m = m + (g - m) * k.w1;
  v = v * k.beta2 + (k.w2 * g) * g;
  const float denom = sqrtf(v) / k.bc2_sqrt + k.eps;
  p = p + k.neg_step_size * (m / denom);
}

__global__ __launch_bounds__(kOptThreads) void adamw_step_batch_kernel(const OptimItem *__restrict__ items, int n_items,
                                                                      const OptimGroups groups, int n_groups,
                                                                      const float *__restrict__ norm, float max_norm) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const OptimItem it = items[find_item(items, n_items, b)];
  int64_t start; int n = 0;
  if (!block_range(it, b, start, n) || it.group < 0 || it.group >= n_groups) return;
  const sgc_optim_group gr = groups.g[it.group];
  // the scalars torch computes in Python floats (double) and hands to fp32 tensor ops: same roundings here
  AdamCoef k;
  k.clip = 1.f;
  if (norm != nullptr && max_norm > 0.f) {           // clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max = 1)
    const float c = max_norm / (norm[0] + 1e-6f);
    k.clip = c > 1.f ? 1.f : c;                     // a NaN norm stays NaN, as torch.clamp(max = 1) keeps it: every gradient is poisoned
  }
  k.decay = (float)(1.0 - gr.lr * gr.weight_decay);
  k.w1 = (float)(1.0 - gr.beta1);
  k.beta2 = (float)gr.beta2;
  k.w2 = (float)(1.0 - gr.beta2);
  k.bc2_sqrt = it.bias_correction2_sqrt;
  k.eps = (float)gr.eps;
  k.neg_step_size = -(float)(gr.lr / (double)it.bias_correction1);

  gfloat *p = as_global(it.param + start), *m = as_global(it.exp_avg + start), *v = as_global(it.exp_avg_sq + start);
  const gfloat *g = as_global(it.grad + start);
  int done = 0;
  if (aligned16(it.param) && aligned16(it.grad) && aligned16(it.exp_avg) && aligned16(it.exp_avg_sq)) {
    const int nvec = n >> 2;
    gf32x4 *p4 = (gf32x4 *)p, *m4 = (gf32x4 *)m, *v4 = (gf32x4 *)v;
    const gf32x4 *g4 = (const gf32x4 *)g;
    for (int i = tid; i < nvec; i += kOptThreads * kOptUnroll) {
      f32x4 pp[kOptUnroll], gg[kOptUnroll], mm[kOptUnroll], vv[kOptUnroll];
#pragma unroll
      for (int u = 0; u < kOptUnroll; ++u) {           // 16 loads of 16 bytes in flight per lane before the first use
        const int j = i + u * kOptThreads;
        if (j < nvec) {
          pp[u] = p4[j];
          gg[u] = g4[j];
          mm[u] = m4[j];
          vv[u] = v4[j];
        }
      }
#pragma unroll
      for (int u = 0; u < kOptUnroll; ++u) {
        const int j = i + u * kOptThreads;
        if (j < nvec) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float pe = pp[u][e], me = mm[u][e], ve = vv[u][e];
            adamw_one(pe, gg[u][e], me, ve, k);
            pp[u][e] = pe; mm[u][e] = me; vv[u][e] = ve;
          }
          p4[j] = pp[u];
          m4[j] = mm[u];
          v4[j] = vv[u];
        }
      }
    }
    done = nvec << 2;
  }
  for (int i = done + tid; i < n; i += kOptThreads) {     // tensors that are not 16-byte aligned, and the < 4-element tail
    float pv = p[i], mv = m[i], vv = v[i];
    adamw_one(pv, g[i], mv, vv, k);
    p[i] = pv; m[i] = mv; v[i] = vv;
  }
}

}  // namespace sgc

using namespace sgc;

extern "C" int64_t sgc_grad_sqnorm_batch_workspace_bytes(int total_blocks) {
  if (total_blocks <= 0) return 0;
  return ((int64_t)total_blocks * (int64_t)sizeof(float) + 15) / 16 * 16;
}

extern "C" int sgc_grad_sqnorm_batch(const void *items, int n_items, int total_blocks, float *partials, float *norm_out,
                                     sgc_stream_t stream) {
  if (!items || !partials || !norm_out) return set_error(SGC_EINVAL, "sgc_grad_sqnorm_batch: null pointer");
  if (n_items <= 0 || total_blocks <= 0) return set_error(SGC_EINVAL, "sgc_grad_sqnorm_batch: bad size");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(grad_sqnorm_partial_kernel, dim3(total_blocks), dim3(kOptThreads), 0, st,
                     reinterpret_cast<const OptimItem *>(items), n_items, partials);
  if (int rc = check_launch("grad_sqnorm_partial_kernel")) return rc;
  hipLaunchKernelGGL(grad_sqnorm_final_kernel, dim3(1), dim3(kWave), 0, st, partials, total_blocks, norm_out);
  return check_launch("grad_sqnorm_final_kernel");
}

extern "C" int sgc_adamw_step_batch(const void *items, int n_items, int total_blocks, const sgc_optim_group *groups, int n_groups,
                                    const float *norm, float max_norm, sgc_stream_t stream) {
  if (!items || !groups) return set_error(SGC_EINVAL, "sgc_adamw_step_batch: null pointer");
  if (n_items <= 0 || total_blocks <= 0 || n_groups <= 0) return set_error(SGC_EINVAL, "sgc_adamw_step_batch: bad size");
  if (n_groups > SGC_OPTIM_MAX_GROUPS)
    return set_error(SGC_EUNSUP, "sgc_adamw_step_batch: %d parameter groups (at most %d)", n_groups, SGC_OPTIM_MAX_GROUPS);
  OptimGroups gs = {};
  for (int i = 0; i < n_groups; ++i) {
    gs.g[i] = groups[i];
    if (!(groups[i].beta1 >= 0.0 && groups[i].beta1 < 1.0 && groups[i].beta2 >= 0.0 && groups[i].beta2 < 1.0 && groups[i].eps >= 0.0))
      return set_error(SGC_EINVAL, "sgc_adamw_step_batch: group %d: betas must lie in [0, 1), eps >= 0", i);
  }
  hipLaunchKernelGGL(adamw_step_batch_kernel, dim3(total_blocks), dim3(kOptThreads), 0, (hipStream_t)stream,
                     reinterpret_cast<const OptimItem *>(items), n_items, gs, n_groups, norm, max_norm);
  return check_launch("adamw_step_batch_kernel");
}
