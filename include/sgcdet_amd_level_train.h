/*
 * sgcdet_amd_level_train.h -- training a view-transform level on the MI355X (gfx950) library: the backward
 * of the row LayerNorm, the sampling locations / attention weights of the deformable attention with their backward, and the
 * backward of the mean over views.  Their forwards (sgc_layer_norm_rows, sgc_view_mean, sgc_scatter_rows) are in sgcdet_amd.h.
 *
 * Training-only, like include/sgcdet_amd_train.h: no twin in the CPU oracle, checked against float64 torch.  Same
 * conventions as include/sgcdet_amd.h: device pointers, row-major fp32, int32 indices, asynchronous on `stream`, no
 * allocation, 0 or a negative SGC_E* code, sgc_last_error() describes a failure; every refusal comes before any launch.
 * Row counts are host integers.  Every OUT buffer is written in full by every launch; no entry uses a float atomic, so a
 * launch repeated on the same inputs gives the same bits.  SGC_ABI_VERSION of include/sgcdet_amd.h covers these declarations too.
 */
#ifndef SGCDET_AMD_LEVEL_TRAIN_H_
#define SGCDET_AMD_LEVEL_TRAIN_H_

#include "sgcdet_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------- *
 * 17. Backward of the row LayerNorm (csrc/level_train.hip)
 * ------------------------------------------------------------------------- */

/* Floats of the workspace sgc_layer_norm_rows_backward sums its column partials through (-1 and an error text for a shape
 * the entry refuses). */
int64_t sgc_layer_norm_rows_backward_workspace_floats(int rows, int C);

/* Backward of sgc_layer_norm_rows (y = (x - mean) * rstd * gamma + beta over the C columns of a row).  A row's mean / rstd are
 * recomputed from x by the arithmetic of the forward.  With xhat = (x - mean) * rstd and g = dy * gamma:
 *   dx[r]     = rstd * (g - mean_c(g) - xhat * mean_c(g * xhat))
 *   dgamma[c] = sum_r dy[r][c] * xhat[r][c];      dbeta[c] = sum_r dy[r][c]
 *   x, dy, dx [rows, C];  gamma, dgamma, dbeta [C];  workspace >= sgc_layer_norm_rows_backward_workspace_floats(rows, C) floats.
 * One wave per row, four rows per workgroup and step; a workgroup walks a fixed range of rows, adds their dgamma / dbeta terms in
 * row order and writes one partial [2, C]; a second kernel adds the (at most 256) partials in a fixed order.
 * C = 128 and C = 256 take the register-resident forms of the forward (16-byte accesses: x, dy, dx, gamma 16-byte aligned, else
 * the generic form); any other C <= 2048 the generic form (SGC_EUNSUP beyond).  rows >= 1, C >= 1 (SGC_EINVAL otherwise). */
int sgc_layer_norm_rows_backward(const float *x, const float *gamma, float eps, const float *dy, float *dx, float *dgamma,
                                 float *dbeta, float *workspace, int64_t workspace_floats, int rows, int C, sgc_stream_t stream);

/* ------------------------------------------------------------------------- *
 * 18. Sampling locations and attention weights of the deformable attention (csrc/level_train.hip)
 * ------------------------------------------------------------------------- */

/* From the concatenated projection of a pair's geometry feature to what the DFA3D operator takes:
 *   ref [n, 3]: (u, v, zn) of every pair;
 *   proj [n, ldp]: columns [uv: 2 M L P, ordered (m, l, p, 2) | depth: M L P | logits: M L P]; ldp >= 4 M L P, the columns at and
 *   beyond 4 M L P are NEVER READ;
 *   normalizer [L, 3]: (W, H, D) of every level;
 *   loc [n, M, L, P, 3] = ref + (off_u / W, off_v / H, off_d / D)  (IEEE divisions);
 *   attn [n, M, L, P]: the softmax over the L P logits of a (pair, head), the maximum subtracted first.
 * A (pair, head) is independent of every other: a NaN logit makes the attn of its own (pair, head) NaN and nothing else.
 * A lane owns one (pair, head); L P <= 16 (SGC_EUNSUP beyond).  16-byte accesses when L P % 4 == 0, ldp % 4 == 0 and proj, loc,
 * attn are 16-byte aligned, scalar ones otherwise.  n >= 1, M, L, P >= 1, ldp >= 4 M L P (SGC_EINVAL otherwise). */
int sgc_sampling_locations_forward(const float *ref, const float *proj, const float *normalizer, float *loc, float *attn, int n,
                                   int M, int L, int P, int ldp, sgc_stream_t stream);

/* Its backward: grad_proj [n, ldp], every column written:
 *   uv columns     grad_loc_u / W, grad_loc_v / H;        depth columns   grad_loc_z / D;
 *   logit columns  a_j * (ga_j - sum_k a_k * ga_k) over the L P weights of the (pair, head), added in index order;
 *   columns [4 M L P, ldp)  +0.0 -- the row is a valid dy of the projection's input and weight gradients.
 *   attn [n, M, L, P]: the forward's output;  grad_loc [n, M, L, P, 3];  grad_attn [n, M, L, P].
 * ref takes no gradient.  Refusals as the forward's (the aligned pointers: grad_proj, grad_loc, grad_attn, attn). */
int sgc_sampling_locations_backward(const float *attn, const float *grad_loc, const float *grad_attn, const float *normalizer,
                                    float *grad_proj, int n, int M, int L, int P, int ldp, sgc_stream_t stream);

/* ------------------------------------------------------------------------- *
 * 19. Backward of the mean over views (csrc/level_train.hip)
 * ------------------------------------------------------------------------- */

/* Backward of sgc_view_mean: for every i < n_valid, v = valid_index[i], and every camera c with slot[c][v] >= 0:
 *   grad_feat[slot[c][v]] = grad_mean[i] / count(v),   count(v) = the number of cameras with slot[c][v] >= 0
 * (one IEEE division per element).  grad_mean [n_valid, C]; slot [N, Nq]; valid_index [n_valid]; grad_feat [n_pairs, C].
 * slot holds every pair row exactly once under a valid voxel (sgc_compact_pairs / sgc_bin_pairs), so every row of grad_feat is
 * written exactly once; the entry writes no other row, and skips a slot value at or beyond n_pairs.  16-byte accesses when C % 4 == 0
 * and the pointers are 16-byte aligned.  n_valid, n_pairs, N, Nq, C >= 1 (SGC_EINVAL otherwise). */
int sgc_view_mean_backward(const float *grad_mean, const int32_t *slot, const int32_t *valid_index, float *grad_feat, int N, int Nq,
                           int C, int n_valid, int n_pairs, sgc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SGCDET_AMD_LEVEL_TRAIN_H_ */
