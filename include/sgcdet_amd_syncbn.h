/*
 * sgcdet_amd_syncbn.h -- SyncBatchNorm of the 3-D neck on the row kernels of the MI355X (gfx950) library: the
 * passes of sgc_bn_rows_act_forward / _backward (sgcdet_amd.h) cut at the seam between "this rank's rows" and "the rows of all
 * ranks", where the caller runs ONE collective per pass.
 *
 *   forward    sgc_bn_rows_sync_stats -> all_gather of 2C + 1 floats -> sgc_bn_rows_sync_apply
 *   backward   sgc_bn_rows_sync_backward_sums -> all_reduce (sum) of 2C floats -> sgc_bn_rows_sync_backward_apply
 *
 * The library runs no collective itself.  With world == 1 (no collective: `gathered` is the stats buffer, `sums` the local sums)
 * the four calls give bit for bit what sgc_bn_rows_act_forward / _backward give: they are the same kernels on the same slab
 * partition and the same fixed merge tree, and the merge of one rank is the identity.
 *
 * Training-only, like include/sgcdet_amd_train.h: no twin in the CPU oracle, checked against float64 torch.  Same conventions as
 * include/sgcdet_amd.h: device pointers, row-major fp32, asynchronous on `stream`, no allocation, no host synchronisation, 0 or a
 * negative SGC_E* code, sgc_last_error() describes a failure.  SGC_ABI_VERSION of include/sgcdet_amd.h covers these declarations
 * too.  Rows are dense channels-last [rows, C]; C % 4 == 0 (SGC_EUNSUP otherwise); x, dy, y, residual, dx, dresidual, weight, bias,
 * mean, invstd and sums 16-byte aligned, rows >= 1 (SGC_EINVAL otherwise).  workspace >= sgc_bn_rows_workspace_floats(rows, C)
 * floats.  Counts travel as fp32: rows < 2^24 per rank and world * rows < 2^24 in total (SGC_EUNSUP beyond the per-rank bound; the
 * total is the caller's to keep -- the library sees one rank).
 */
#ifndef SGCDET_AMD_SYNCBN_H_
#define SGCDET_AMD_SYNCBN_H_

#include "sgcdet_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The largest `world` sgc_bn_rows_sync_apply accepts: one thread per channel walks the ranks in a plain loop. */
#define SGC_SYNCBN_MAX_WORLD 1024

/* ------------------------------------------------------------------------- *
 * 20. SyncBatchNorm over rows: local and global halves of the BatchNorm passes (csrc/batch_norm.hip)
 * ------------------------------------------------------------------------- */

/* Local statistics of this rank's rows: stats [2C + 1] = [mean (C) | M2 (C) | count (1)], fully written.
 *   mean[c] = the mean of column c over the rows;  M2[c] = sum_r (x[r][c] - mean[c])^2 -- the SUM of squared deviations, not a
 *   variance: ranks merge by Chan's step (the step the slabs of one rank merge by), which is exact in M2 and needs no division
 *   by a count that differs between ranks;  count = (float) rows.
 * Welford per thread, the slab partition and the fixed merge tree of sgc_bn_rows_forward: the same bits every run. */
int sgc_bn_rows_sync_stats(const float *x, float *stats, float *workspace, int64_t workspace_floats, int rows, int C, sgc_stream_t stream);

/* gathered [world, 2C + 1]: the stats of every rank in rank order, this rank's own row included (what all_gather returns; with
 * world == 1 the stats buffer itself).  Every count >= 1.  Merges the ranks IN RANK ORDER starting from rank 0's values, so every
 * rank computes the same bits and one rank's statistics pass through untouched, then
 *   mean_out, invstd_out [C]: mean and 1 / sqrt(M2 / N + eps) over the N = sum of counts rows of all ranks;
 *   inv_count_out [1]: 1 / N as a device scalar, for sgc_bn_rows_sync_backward_apply;
 *   running_mean / running_var (either may be null): updated as nn.BatchNorm does, momentum and the UNBIASED variance M2 / (N - 1)
 *   (N == 1: the biased one);
 *   y [rows, C] = relu?(bn(x) + residual?) over this rank's rows, the apply pass of sgc_bn_rows_act_forward; the ReLU keeps a NaN.
 * 1 <= world <= SGC_SYNCBN_MAX_WORLD (SGC_EUNSUP otherwise).  gathered and inv_count_out need 4-byte alignment only. */
int sgc_bn_rows_sync_apply(const float *x, const float *gathered, int world, const float *weight, const float *bias,
                           float *running_mean_or_null, float *running_var_or_null, float momentum, float eps,
                           const float *residual_or_null, int relu, float *y, float *mean_out, float *invstd_out, float *inv_count_out,
                           int rows, int C, sgc_stream_t stream);

/* Local sums of the backward over this rank's rows: sums [2C] = [sum_r g[r][c] | sum_r g[r][c] * xhat[r][c]], fully written, with
 * g = dy, or (y_relu_or_null given: the forward ended in a ReLU) g = y_relu > 0 ? dy : 0 as in sgc_bn_rows_act_backward, and
 * xhat = (x - mean) * invstd with the GLOBAL mean / invstd of sgc_bn_rows_sync_apply.  Ordered reductions (the partition and tree of
 * sgc_bn_rows_backward).  These are also this rank's dbias | dweight: local sums, which the step's gradient all-reduce averages
 * like every other parameter gradient -- copy them before the all-reduce overwrites them. */
int sgc_bn_rows_sync_backward_sums(const float *x, const float *dy, const float *y_relu_or_null, const float *mean, const float *invstd,
                                   float *sums, float *workspace, int64_t workspace_floats, int rows, int C, sgc_stream_t stream);

/* dx [rows, C] = weight * invstd * (g - sums[c] * inv_count - xhat * sums[C + c] * inv_count) over this rank's rows, with sums
 * [2C] the all-reduced (summed over the ranks) output of sgc_bn_rows_sync_backward_sums and inv_count [1] the device scalar of
 * sgc_bn_rows_sync_apply (read on the device: no value crosses to the host between the passes).
 * dresidual_or_null [rows, C] (when not null) = g, the gradient of the added identity. */
int sgc_bn_rows_sync_backward_apply(const float *x, const float *dy, const float *y_relu_or_null, const float *mean, const float *invstd,
                                    const float *weight, const float *sums, const float *inv_count, float *dx, float *dresidual_or_null,
                                    int rows, int C, sgc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SGCDET_AMD_SYNCBN_H_ */
