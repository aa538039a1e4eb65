/*
 * sgcdet_amd_depth_train.h -- training DepthNet_Fusion's regulation U-Nets and depth_reg on the MI355X (gfx950) library
 * (DESIGN.md 4.14b): a live BatchNorm over zero-padded rows, and the backward of the softmax of depth_reg's epilogue.
 *
 * Training-only, like include/sgcdet_amd_train.h: no twin in the CPU oracle, checked against float64 torch.  Same
 * conventions as include/sgcdet_amd.h: device pointers, row-major fp32, asynchronous on `stream`, no allocation, 0 or a
 * negative SGC_E* code, sgc_last_error() describes a failure.  SGC_ABI_VERSION of include/sgcdet_amd.h covers these
 * declarations too.
 */
#ifndef SGCDET_AMD_DEPTH_TRAIN_H_
#define SGCDET_AMD_DEPTH_TRAIN_H_

#include "sgcdet_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------- *
 * 15. Live BatchNorm over rows whose pitch is wider than the channel count (csrc/batch_norm.hip)
 * ------------------------------------------------------------------------- */

/* sgc_bn_rows_act_forward (sgcdet_amd.h) for rows of pitch ld >= C: the convolutions of a layer with 12, 24, 48, 140 ... channels
 * work on planes zero-padded to a multiple of 32, the norm between them has the module's own C-long tensors.
 *   x, y, residual [rows, ld]: row r starts at r * ld; columns [C, ld) of x and residual are NEVER READ (a NaN there changes
 *   nothing), columns [C, ld) of y are written as +0.0;
 *   weight, bias, mean_out, invstd_out, running_mean, running_var [C]: dense, the module's tensors;
 *   tail 0: y = bn(x) + residual?     1: y = relu(bn(x) + residual?)     2: y = relu(bn(x)) + residual (residual required)
 *   the ReLU keeps a NaN (v < 0 ? 0 : v);
 *   workspace >= sgc_bn_rows_workspace_floats(rows, C) floats (the dense query: the partial statistics are [C] wide).
 * Statistics and the running-statistics update are those of sgc_bn_rows_forward (fixed-order Welford / Chan merge, unbiased
 * running variance): sgc_bn_rows_act_forward is the same kernels at ld == C (relu = tail 0 / 1), and the pitch changes no bit.
 * C % 4 == 0, ld % 4 == 0, ld >= C, tail in {0, 1, 2} (SGC_EUNSUP otherwise); 16-byte aligned row matrices, weight, bias, mean_out,
 * invstd_out; rows >= 1 (SGC_EINVAL otherwise). */
int sgc_bn_rows_padded_forward(const float *x, const float *weight, const float *bias, float *running_mean_or_null,
                               float *running_var_or_null, float momentum, float eps, const float *residual_or_null, int tail,
                               float *y, float *mean_out, float *invstd_out, float *workspace, int64_t workspace_floats, int rows,
                               int C, int ld, sgc_stream_t stream);

/* Its backward.  With gate = 1 (tail 0), y > 0 (tail 1, read off the saved output y) or t > 0 (tail 2: t = bn(x) recomputed from
 * x, mean, invstd, weight, bias by the very expression the forward evaluates -- the gate cannot be read off y = relu(t) + residual)
 * and g = gate ? dy : 0:
 *   dbias[c] = sum_r g[r][c];  dweight[c] = sum_r g[r][c] * xhat[r][c];
 *   dx = weight * invstd * (g - dbias / rows - xhat * dweight / rows);
 *   dresidual (when not null) = g for tails 0 / 1 (the add sits in front of the ReLU), dy for tail 2 (behind it).
 * The gate is a select on `value <= 0`: a NaN gate value lets dy pass, a closed gate drops a NaN of dy.
 *   x, dy, y, dx, dresidual [rows, ld]; columns [C, ld) of x, dy, y are never read, those of dx and dresidual are written as +0.0;
 *   y_or_null: required for tail 1, ignored otherwise;  bias_or_null: required for tail 2, ignored otherwise.
 * sgc_bn_rows_act_backward is the same kernels at ld == C (y_relu = tail 1's y; without it, tail 0).
 * Refusals as the forward's; mean, invstd, weight, bias, dweight, dbias 16-byte aligned too. */
int sgc_bn_rows_padded_backward(const float *x, const float *dy, const float *y_or_null, const float *mean, const float *invstd,
                                const float *weight, const float *bias_or_null, float *dx, float *dweight, float *dbias,
                                float *dresidual_or_null, int tail, float *workspace, int64_t workspace_floats, int rows, int C,
                                int ld, sgc_stream_t stream);

/* ------------------------------------------------------------------------- *
 * 16. Backward of a row softmax (csrc/softmax_rows.hip)
 * ------------------------------------------------------------------------- */

/* g[r][c] = p[r][c] * (dp[r][c] - sum over c' < C of p[r][c'] * dp[r][c'])  for c < C;  g[r][c] = +0.0 for C <= c < ldg.
 *   p [rows, ldp]: the softmax's OUTPUT (the softmax_cols epilogue of sgc_conv2d_nhwc_ex_bf16x3);  dp [rows, lddp]: its gradient;
 *   g [rows, ldg]: the gradient of the logits, fully written.  Columns at and beyond C of p and dp are never read.
 * Rows are independent: a NaN in a row makes that row NaN and no other.  One pass, each value read once; the row sum is added
 * in a fixed order (the same bits every run): |g - exact| <= (C + 4) * 2^-24 * max |dp| of the row.
 * C % 4 == 0 and 4 <= C <= 128 (the bound of softmax_cols), ldp, lddp, ldg % 4 == 0 and >= C (SGC_EUNSUP otherwise); 16-byte
 * aligned pointers, rows >= 1 (SGC_EINVAL otherwise). */
int sgc_softmax_rows_backward(const float *p, const float *dp, float *g, int64_t rows, int C, int ldp, int lddp, int ldg,
                              sgc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SGCDET_AMD_DEPTH_TRAIN_H_ */
