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

#ifdef __cplusplus
}
#endif
#endif /* SGCDET_AMD_TRAIN_H_ */
