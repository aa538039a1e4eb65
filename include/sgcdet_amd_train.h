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

/* ------------------------------------------------------------------------- *
 * 11. The loss of the detection head with its gradients (csrc/head_loss.hip)
 * ------------------------------------------------------------------------- */

/* The head tensors of one scale, for one image, read where the head produced them: element (channel c, point j) of a tensor is at
 * base[c * channel_stride + j * point_stride] (strides in elements, positive), j = (x * Y + y) * Z + z -- the order of get_points and
 * of the flattened point list.  [C, X, Y, Z] contiguous is (X*Y*Z, 1); the channels-last rows of the convolutions are (1, row length).
 *   centerness 1 channel (logit);  bbox_pred n_reg channels, already activated (6 face distances [+ the raw angle]);
 *   cls_score n_classes channels (logits);  valid [n_points] bytes, non-zero = inside some camera's view. */
typedef struct sgc_head_loss_level {
  const float *centerness, *bbox_pred, *cls_score;
  const uint8_t *valid;
  int64_t n_points;                                  /* X * Y * Z */
  int32_t centerness_point_stride, bbox_channel_stride, bbox_point_stride, cls_channel_stride, cls_point_stride, reserved;
} sgc_head_loss_level;            /* 64 bytes */
#define SGC_HEAD_LOSS_MAX_SCALES 4

/* ImVoxelHeadV2._loss_single (imvoxel_head_v2.py:147-235) for one image: pos = labels >= 0 & valid, n = max(count(pos), 1),
 *   losses[0] = lw_centerness * sum_pos BCEWithLogits(centerness, centerness_targets) / n
 *   losses[1] = lw_bbox * sum_pos w (1 - IoU(decode(point, bbox_pred), bbox_targets)) / sum_pos w,   w = centerness_targets
 *   losses[2] = lw_cls * sum_valid sum_c sigmoid_focal(cls_score, labels; gamma, alpha) / n
 * with log(max(p, FLT_MIN)) in the focal loss (zero gradient where the clamp is active), any label outside [0, n_classes) background
 * for every class; rotated = 0: n_reg = 6, boxes (x0,y0,z0,x1,y1,z1) = point -/+ distances, axis-aligned IoU with eps = 1e-6;
 * rotated = 1: n_reg = 7, boxes (cx,cy,cz,w,l,h,angle) with the centre shift rotated by the predicted angle, IoU of rotated boxes
 * (rectangle clipped against the four edges of the target, shoelace area, z overlap, inter / (vol - inter)).  Empty cases are decided
 * on the device: no valid point -> losses[2] = 0; no positive or sum w = 0 -> losses[0] = losses[1] = 0 (sum w = 0 alone: only
 * losses[1]); the corresponding gradients are 0.
 *   levels: n_scales <= SGC_HEAD_LOSS_MAX_SCALES structs in HOST memory, copied into the kernels' arguments;
 *   points [n_points, 3], centerness_targets [n_points], bbox_targets [n_points, n_reg], labels [n_points] int64: the flattened
 *   point list (level after level) and the outputs of sgc_assign_targets for it; targets of non-positive points are never read;
 *   gamma, alpha, lw_*: as torch holds them (Python floats);
 *   n_pos_override: NULL, or 1 float in DEVICE memory that replaces count(pos) in n (a distributed run's all-reduced mean);
 *   losses [3], n_pos [1] (the LOCAL count, whatever n_pos_override says): device floats, written;
 *   grads: the packed gradient buffer, (1 + n_reg + n_classes) * n_points floats, EVERY element written (nothing to pre-zero):
 *     level l starts at (1 + n_reg + n_classes) * (points of the levels before it) and holds the planes [1 + n_reg + n_classes,
 *     n_points_l] contiguous -- centerness, bbox_pred, cls_score, each a [C, X, Y, Z] contiguous tensor.  It holds the UNNORMALISED
 *     gradients; sgc_head_loss_scale_grads turns them into d (sum_k grad_k * losses[k]) / d tensor;
 *   workspace >= sgc_head_loss_workspace_bytes(n_points, n_scales) bytes, 8-byte aligned, contents irrelevant before; afterwards it
 *     holds the per-workgroup partial sums and the three scale factors that sgc_head_loss_finalize / sgc_head_loss_scale_grads read.
 * Two launches (three with rotated = 1), no host read-back, no float atomics: bitwise reproducible run to run.
 * SGC_EUNSUP for n_scales > SGC_HEAD_LOSS_MAX_SCALES, n_reg not 6 / 7, rotated not matching n_reg, levels whose n_points do not add
 * up to n_points, n_points * (1 + n_reg + n_classes) >= 2^31. */
int sgc_head_loss_forward(const sgc_head_loss_level *levels, int n_scales, const float *points, const float *centerness_targets,
                          const float *bbox_targets, const int64_t *labels, int n_points, int n_reg, int n_classes, int rotated,
                          double gamma, double alpha, double lw_centerness, double lw_bbox, double lw_cls, const float *n_pos_override,
                          float *losses, float *n_pos, float *grads, void *workspace, int64_t workspace_bytes, sgc_stream_t stream);
int64_t sgc_head_loss_workspace_bytes(int n_points, int n_scales);

/* The last launch of sgc_head_loss_forward again, on the workspace it left: losses, n_pos and the scale factors for another
 * n_pos_override.  A distributed run calls the forward without an override, all-reduces n_pos on the device and calls this.
 *   level_points: n_scales int64 in HOST memory, the n_points of the levels. */
int sgc_head_loss_finalize(void *workspace, int64_t workspace_bytes, const int64_t *level_points, int n_scales,
                           const float *n_pos_override, double lw_centerness, double lw_bbox, double lw_cls, float *losses, float *n_pos,
                           sgc_stream_t stream);

/* out = grads * (scale factor of the element's loss) * (upstream gradient of that loss), one launch over the packed gradient buffer;
 * out may be grads itself.  grad_centerness / grad_bbox / grad_cls: 1 float each in DEVICE memory (autograd's grad_outputs);
 * workspace: the one sgc_head_loss_forward (or _finalize) wrote last;  level_points as above. */
int sgc_head_loss_scale_grads(const float *grads, float *out, const int64_t *level_points, int n_scales, int n_reg, int n_classes,
                              const void *workspace, const float *grad_centerness, const float *grad_bbox, const float *grad_cls,
                              sgc_stream_t stream);

/* ------------------------------------------------------------------------- *
 * 12. Training the image backbone: the 2-D weight gradient and the backward of the frozen-norm epilogue
 *     (csrc/conv3d_wgrad.hip, csrc/frozen_norm.hip)
 * ------------------------------------------------------------------------- */

/* Weight gradient of nn.Conv2d(k, stride, padding = k / 2) over channels-last rows:
 *   dw[kh*k + kw][co][ci] = sum over (n, oh, ow) of dy[(n,oh,ow)][co] * x[(n, oh*s + kh - k/2, ow*s + kw - k/2)][ci]
 *   x [N*H*W, Cin], dy [N*OH*OW, Cout], OH = ceil(H / s), OW = ceil(W / s), dw [k*k, Cout, Cin] fully written
 *   (the layout sgc_unpack_conv_wgrad turns into the parameter's); a tap outside its image adds nothing.
 *   k in {1, 3}, s in {1, 2}, any H, W >= 1, Cin % 4 == 0, Cout % 4 == 0, 16-byte aligned pointers.
 * The tile kernel of sgc_conv3d_wgrad_bf16x3 with a reduction row decoded as (image, h, w): bf16x3 products (always three,
 * whatever sgc_set_conv_products says), fp32 accumulation, the reduction rows split over workgroups.  With a workspace of
 * sgc_conv2d_wgrad_workspace_floats(...) floats the partial sums are added in a fixed order (bit-identical run to run); without
 * one (null, or too small) one workgroup per tile walks the whole range.  The query returns 0 for a shape that is not split and
 * -1 for one the entry refuses.  SGC_EUNSUP for other k / s / channel counts, and for x or dy of 4 GiB or more. */
int sgc_conv2d_wgrad_bf16x3(const float *x, const float *dy, float *dw, int N, int H, int W, int Cin, int Cout, int ksize,
                            int stride, float *workspace_or_null, int64_t workspace_floats, sgc_stream_t stream);
int64_t sgc_conv2d_wgrad_workspace_floats(int N, int H, int W, int Cin, int Cout, int ksize, int stride);

/* Backward of the epilogue y = act(conv * scale + shift [+ residual]) of a layer whose norm is frozen, one pass over dy and y:
 *   gate       = relu ? (y[r][c] > 0) : 1
 *   g[r][c]    = gate ? dy[r][c] * scale[c] : 0      (scale null: 1)  -- feeds the input and weight gradients
 *   gres[r][c] = gate ? dy[r][c] : 0                 (gres null: not written) -- the residual's gradient when the ReLU sits behind the add
 * dy, y, g, gres [rows, C] dense;  y may be null with relu = 0.  The gate is a select: a NaN of dy goes through where the gate is
 * open and is dropped where it is closed; the product is a single fp32 multiply.  Needs C % 4 == 0 and 16-byte aligned pointers
 * (SGC_EUNSUP otherwise). */
int sgc_frozen_norm_act_backward(const float *dy, const float *y_or_null, const float *scale_or_null, float *g, float *gres_or_null,
                                 int64_t rows, int C, int relu, sgc_stream_t stream);

/* ------------------------------------------------------------------------- *
 * 13. Training the image FPN: the top-down step and the bias gradient (csrc/fpn_train.hip)
 * ------------------------------------------------------------------------- */

/* Top-down step of the FPN on channels-last maps: nearest upsampling of the coarse map to the fine map's size, added to it.
 *   out[n][h][w][:] = fine[n][h][w][:] + coarse[n][ih(h)][iw(w)][:],  ih(h) = min(h * Hs / Hd, Hs - 1) in integers, iw likewise
 *   fine, out [N, Hd, Wd, C], coarse [N, Hs, Ws, C];  out may be fine itself (the in-place form).
 * The index rule equals F.interpolate(mode = "nearest") for Hs in {ceil(Hd / 2), floor(Hd / 2)} (what a stride-2 stage produces);
 * any 1 <= Hs <= Hd, 1 <= Ws <= Wd is accepted.  Needs C % 4 == 0 and 16-byte aligned pointers (SGC_EUNSUP otherwise). */
int sgc_upsample_nearest_add_nhwc(const float *fine, const float *coarse, float *out, int N, int Hd, int Wd, int Hs, int Ws, int C,
                                  sgc_stream_t stream);

/* Its gradient with respect to the coarse map (the fine map's gradient is gout itself):
 *   gcoarse[n][hs][ws][:] = sum of gout[n][h][w][:] over h in [ceil(hs * Hd / Hs), ceil((hs + 1) * Hd / Hs)) below Hd, w likewise
 * -- the pixels whose ih / iw is (hs, ws); at most 2 x 2 of them for Hs = ceil(Hd / 2), 3 x 3 for the floor of an odd size.  One thread owns an output
 * element and adds h outer, w inner: no atomics, the same bits on every run; every element of gcoarse is written.
 * Same requirements as the forward. */
int sgc_upsample_nearest_add_backward_nhwc(const float *gout, float *gcoarse, int N, int Hd, int Wd, int Hs, int Ws, int C,
                                           sgc_stream_t stream);

/* out[c] = sum over r of x[r][c], x [rows, C] dense: the bias gradient of a convolution on rows.  Two stages in a fixed order --
 * per-workgroup partial sums of a row range into the workspace, then one workgroup adds the partial sums in index order -- so two
 * runs give the same bits, and no value passes through more than 160 dependent fp32 additions on its way into out[c] (75 at
 * rows = 192 000, C = 256): |out[c] - exact| <= 160 * 2^-24 * sum over r of |x[r][c]| to first order.
 * sgc_rows_colsum_workspace_floats(rows, C): the floats the workspace needs; 0: one workgroup row covers the input and writes
 * out directly (the workspace may be null); -1: a shape the entry refuses (C % 4 != 0, rows < 1, or so many rows -- beyond
 * about 600 000 -- that the chain bound would not hold).  16-byte aligned pointers; SGC_EUNSUP / SGC_EINVAL before any launch. */
int sgc_rows_colsum(const float *x, float *out, int64_t rows, int C, float *workspace, int64_t workspace_floats, sgc_stream_t stream);
int64_t sgc_rows_colsum_workspace_floats(int64_t rows, int C);

/* ------------------------------------------------------------------------- *
 * 14. Training DepthNet_Fusion's feature extractors: the weight gradient of the 7x7 stem (csrc/stem7_wgrad.hip)
 * ------------------------------------------------------------------------- */

/* Weight gradient of nn.Conv2d(3, 64, 7, stride = 2, padding = 3) -- the backward twin of sgc_conv2d_stem7_bf16x3 (sgcdet_amd_image.h):
 *   dw[co][ci][kh][kw] = sum over (n, oh, ow) of dy[(n,oh,ow)][co] * img[n][ci][2 oh + kh - 3][2 ow + kw - 3]
 *   img [N, 3, H, W] fp32 NCHW, H and W even;  dy [N * (H/2) * (W/2), 64] channels-last rows;
 *   dw [64, 3, 7, 7]: the PARAMETER's own layout (its flattened (ci * 7 + kh) * 7 + kw is the column of the forward kernel's
 *   [64][160] matrix), fully written; a tap outside the image adds nothing.
 * There is no input gradient: images do not need one.
 * bf16x3 products (always three, whatever sgc_set_conv_products says), fp32 accumulation.  The reduction rows are split over
 * workgroups by tiles of 8 x 32 output pixels.  With a workspace of sgc_conv2d_stem7_wgrad_workspace_floats(N, H, W) floats the
 * partial sums are added in a fixed order by a second launch (bit-identical run to run, no atomics); without one (null, or too
 * small) one workgroup walks the whole range.  The query answers on the host: 0 for a shape that is not split (one tile), -1 for
 * one the entry refuses (sgc_last_error() says why).
 * SGC_EINVAL for a null or misaligned (16 bytes) pointer and for a non-positive size; SGC_EUNSUP for an odd H or W and for img or
 * dy of 4 GiB or more. */
int sgc_conv2d_stem7_wgrad_bf16x3(const float *img, const float *dy, float *dw, int N, int H, int W, float *workspace_or_null,
                                  int64_t workspace_floats, sgc_stream_t stream);
int64_t sgc_conv2d_stem7_wgrad_workspace_floats(int N, int H, int W);

#ifdef __cplusplus
}
#endif
#endif /* SGCDET_AMD_TRAIN_H_ */
