/*
 * sgcdet_amd_train.h -- training-only entry points of the MI355X (gfx950) library.
 *
 * The calls declared here have no twin in the CPU oracle (oracle/sgc_oracle.c mirrors include/sgcdet_amd.h only);
 * their checkers are float64 autograd of the reference formulation and fixtures made by the reference's own code
 * (tests/golden/plane_sweep_grad.npz).  Same conventions as include/sgcdet_amd.h: device pointers, dense row-major
 * fp32 unless stated, asynchronous on `stream`, no allocation (workspaces come from the caller, sized by the
 * matching *_workspace_bytes query), 0 or a negative SGC_E* code, sgc_last_error() describes a failure.
 * SGC_ABI_VERSION of include/sgcdet_amd.h covers these declarations too.
 */
#ifndef SGCDET_AMD_TRAIN_H_
#define SGCDET_AMD_TRAIN_H_

#include "sgcdet_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------- *
 * 9b. Backward of the plane-sweep matching cost (sgc_plane_sweep_corr, section 9 of sgcdet_amd.h)
 * ------------------------------------------------------------------------- */

/* grad_feat = d(sum corr * grad_corr) / d feat for the forward
 *   corr[n,d,p] = (1/K) sum_k ( sum_c S_{n,k,d,p}[c] * feat[n,p,c] ) / sqrt(C),
 * S = bilinear sample (zeros padding, align_corners = False) of view nbr[n,k] at the warped position of pixel p on plane
 * d, computed exactly as sgc_plane_sweep_corr computes it.  Equals autograd of homo_warping + the cost-volume loop of
 * DepthNet_Fusion.forward (mmdet3d_plugin/models/im2voxel/depth_utils/depth_est_fusion.py:87-126, :233-240) with
 * respect to f_mvs: the sampling grid is built under no_grad there, so positions get no gradient; feat receives its
 * reference-role term (gather) and its neighbour-role term (the grid_sample input gradient) in one tensor.
 *   feat [N, H*W, C] channels-last, C <= 256;  nbr [N,K] int32 in [0, N) (an id outside adds nothing: a guard,
 *   not checked on the host);  rt [N,K,12];  depth [D], D <= 32;
 *   grad_corr [N,D,H,W];  grad_feat [N, H*W, C] fully written (not accumulated);
 *   workspace >= sgc_plane_sweep_corr_backward_workspace_bytes(N, K, H, W, D) bytes, 16-byte aligned, contents
 *   irrelevant (about 8 * N*H*W*K*D*4 bytes: the destination-major list of the neighbour-role contributions).
 * SGC_EUNSUP for C > 256, D > 32 or N*H*W*K*D*4 >= 2^31.
 * Bitwise reproducible run to run while no destination row receives more than 512 corner contributions (every row
 * at the training shapes): each list is sorted by content before it is summed.  Rows of longer lists are summed in
 * atomic-fill order and their 512-entry chunks added by float atomics: they differ by fp32 reordering only
 * (csrc/plane_sweep_bwd.hip).                                                                       */
int sgc_plane_sweep_corr_backward(const float *feat, const int32_t *nbr, const float *rt, const float *depth,
                                  const float *grad_corr, float *grad_feat, void *workspace, int64_t workspace_bytes,
                                  int N, int K, int H, int W, int C, int D, sgc_stream_t stream);
int64_t sgc_plane_sweep_corr_backward_workspace_bytes(int N, int K, int H, int W, int D);

/* ------------------------------------------------------------------------- *
 * 10. The parameter update: global-norm gradient clipping + AdamW over a list of tensors (csrc/optim.hip)
 * ------------------------------------------------------------------------- */

/* Both calls walk a list of items in DEVICE memory, one per parameter tensor that has a gradient this step (the pattern of
 * sgc_pack_item): block_start ascending from 0, item i owning ceil(numel / block_elems) workgroups, total_blocks = their sum.
 * All four tensors are dense fp32 of numel elements (the raw pointers carry no type: a caller that holds anything else must
 * refuse it -- sgcdet_amd.optim raises TypeError); tensors that are not 16-byte aligned take a scalar path.
 *   step                    this tensor's own count of updates AFTER this one (torch's state["step"]; a parameter without a
 *                           gradient in some steps lags the others);
 *   bias_correction1        1 - beta1^step, bias_correction2_sqrt = sqrt(1 - beta2^step): computed by the host in double
 *                           as torch computes them, rounded to fp32;
 *   block_elems             elements per workgroup of this item, a positive multiple of 4 (a block whose item says otherwise
 *                           does nothing). */
typedef struct sgc_optim_item {
  float *param;
  const float *grad;
  float *exp_avg, *exp_avg_sq;
  int64_t numel;
  int32_t group, step, block_start, block_elems;
  float bias_correction1, bias_correction2_sqrt;
} sgc_optim_item;                 /* 64 bytes */

/* Hyper-parameters of one parameter group, as torch holds them (Python floats). */
typedef struct sgc_optim_group {
  double lr, weight_decay, beta1, beta2, eps;
} sgc_optim_group;                /* 40 bytes */
#define SGC_OPTIM_MAX_GROUPS 8

/* norm_out[0] = sqrt(sum of grad^2 over every item) == the total_norm of torch.nn.utils.clip_grad_norm_(norm_type = 2).
 * Two launches: one fp32 partial per workgroup (plain stores), then one wave adds the partials in index order in fp64.
 * No float atomics: bitwise reproducible run to run for a given item list.
 *   partials: >= sgc_grad_sqnorm_batch_workspace_bytes(total_blocks) bytes, contents irrelevant;  norm_out: 1 float (device). */
int sgc_grad_sqnorm_batch(const void *items, int n_items, int total_blocks, float *partials, float *norm_out,
                          sgc_stream_t stream);
int64_t sgc_grad_sqnorm_batch_workspace_bytes(int total_blocks);

/* One AdamW step (torch.optim.AdamW, amsgrad = False, maximize = False, fp32) of every item in ONE launch, per element:
 *   c = min(1, max_norm / (norm[0] + 1e-6))          (max_norm <= 0 or norm == NULL: c = 1, no clipping)
 *   g = grad * c                                     (registers only: grad is NOT written)
 *   p = p * (1 - lr * weight_decay)
 *   m = m + (g - m) * (1 - beta1)
 *   v = v * beta2 + (1 - beta2) * g * g
 *   p = p - (lr / bias_correction1) * (m / (sqrt(v) / bias_correction2_sqrt + eps))
 *   groups: n_groups <= SGC_OPTIM_MAX_GROUPS structs in HOST memory, copied into the kernel's arguments (no device copy of
 *   what a scheduler changes every step);  norm: 1 float in DEVICE memory (sgc_grad_sqnorm_batch's norm_out), read by the
 *   kernel -- the host never waits for it.  An item whose group is outside [0, n_groups) is left untouched.
 * SGC_EUNSUP for n_groups > SGC_OPTIM_MAX_GROUPS. */
int sgc_adamw_step_batch(const void *items, int n_items, int total_blocks, const sgc_optim_group *groups, int n_groups,
                         const float *norm, float max_norm, sgc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SGCDET_AMD_TRAIN_H_ */
