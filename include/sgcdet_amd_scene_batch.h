/*
 * sgcdet_amd_scene_batch.h -- the 3-D convolution passes of the MI355X (gfx950) library on a BATCH of scenes in one launch
 * (DESIGN.md 4.20): what training on scene batches needs of the neck's and the head's convolutions.  The scene-less entries
 * sgc_conv3d_cl_bf16x3 / sgc_conv3d_wgrad_bf16x3 of include/sgcdet_amd.h are these entries with scenes = 1.
 *
 * Same conventions as include/sgcdet_amd.h: device pointers, row-major fp32, asynchronous on `stream`, no allocation, 0 or a
 * negative SGC_E* code, sgc_last_error() describes a failure; every refusal comes before any launch.  SGC_ABI_VERSION of
 * include/sgcdet_amd.h covers these declarations too.
 */
#ifndef SGCDET_AMD_SCENE_BATCH_H_
#define SGCDET_AMD_SCENE_BATCH_H_

#include "sgcdet_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* sgc_conv3d_cl_bf16x3 on `scenes` volumes of one grid:
 *   x [scenes * ix*iy*iz, Cin]: scene s occupies rows [s * IV, (s + 1) * IV); y and residual [scenes * OV, Cout] likewise;
 *   w_hi / w_lo, scale and shift are shared.  Every other argument as in sgc_conv3d_cl_bf16x3.
 * Isolation: every scene is convolved on its own.  A workgroup of the halo kernels works on one scene and its halo is zero
 *   padding at that scene's border; a 128-row tile of the tile kernel may span scenes (400 rows per scene at the coarsest
 *   scale), so the scene is decoded per row and a neighbour is looked up inside that row's scene.  No row of another scene is read.
 * Plan: the kernel family, the brick and the column tile are chosen from the per-scene grid, as sgc_conv3d_cl_bf16x3 chooses them:
 *   a layer stays in its numerical class whatever the batch.  The split count follows the workgroups of the whole launch, so a
 *   scene's rows agree with its own sgc_conv3d_cl_bf16x3 launch to summation order (tests: 1e-4 of the tensor scale), bit for bit
 *   where the splits coincide.  With a workspace of sgc_conv3d_batched_workspace_floats(...) floats a split launch is bit-identical
 *   from run to run; without one the partial tiles meet in y through float atomics (as sgc_conv3d_cl_bf16x3).
 * scenes = 1 launches exactly what sgc_conv3d_cl_bf16x3 launches.
 * scenes < 1: SGC_EINVAL.  scenes * ix*iy*iz * Cin * 4 must stay below 4 GiB, scenes * 8 * ix*iy*iz below 2^31, and with scenes > 1
 * the scene count and every extent of the grid below 2^15 (SGC_EUNSUP).
 * The masked form, the activation epilogue, the 2-D form, the Winograd stack, device-side row counts and the fp32 kernel have
 * no scene axis: their entries take one volume per launch.                                                                   */
int sgc_conv3d_cl_bf16x3_batched(const float *x, const uint16_t *w_hi, const uint16_t *w_lo, const float *scale,
                                 const float *shift, const float *residual_or_null, float *y,
                                 int ix, int iy, int iz, int Cin, int Cout, int ksize, int stride,
                                 int transposed, int relu, int scenes, float *workspace_or_null, int64_t workspace_floats,
                                 sgc_stream_t stream);
/* sgc_conv3d_workspace_floats for a batch; bf16x3 = 0 (the fp32 kernel) with scenes > 1 returns 0: that kernel has no scene axis. */
int64_t sgc_conv3d_batched_workspace_floats(int ix, int iy, int iz, int Cin, int Cout, int ksize, int stride,
                                            int transposed, int bf16x3, int scenes);

/* sgc_conv3d_wgrad_bf16x3 on `scenes` volumes: x [scenes * ix*iy*iz, Cin], dy [scenes * OV, Cout] (scene s first, as above);
 *   dw [ksize^3][Cout][Cin] is the SUM over the scenes, formed inside the launch: to the tile kernel the scene axis is more
 *   reduction rows, to the halo forms more bricks; no tap crosses a scene's border.  The form is chosen from the per-scene grid,
 *   the split count from the whole launch.  scenes = 1 launches exactly what sgc_conv3d_wgrad_bf16x3 launches.
 *   scenes < 1: SGC_EINVAL; x and dy must stay below 4 GiB each (SGC_EUNSUP).  The query returns -1 for a refused shape.      */
int sgc_conv3d_wgrad_bf16x3_batched(const float *x, const float *dy, float *dw, int ix, int iy, int iz, int Cin, int Cout,
                                    int ksize, int stride, int scenes, float *workspace_or_null, int64_t workspace_floats,
                                    sgc_stream_t stream);
int64_t sgc_conv3d_wgrad_batched_workspace_floats(int ix, int iy, int iz, int Cin, int Cout, int ksize, int stride, int scenes);

#ifdef __cplusplus
}
#endif
#endif  /* SGCDET_AMD_SCENE_BATCH_H_ */
