/*
 * sgcdet_amd_image.h -- image-side 2-D convolutions of the MI355X (gfx950) library: what DepthNet_Fusion's CNNs and the ResNet
 * backbone need beyond sgc_conv2d_nhwc_bf16x3 (csrc/conv2d_image.hip, csrc/maxpool2d.hip).
 *
 * The calls declared here have no twin in the CPU oracle (oracle/sgc_oracle.c mirrors include/sgcdet_amd.h only); their
 * checkers are torch's F.conv2d / F.conv_transpose2d in float64 and the reference class's own output
 * (tests/golden/depth_net.npz).  Same conventions as include/sgcdet_amd.h: device pointers, dense row-major fp32 unless
 * stated, asynchronous on `stream`, no allocation, 0 or a negative SGC_E* code, sgc_last_error() describes a failure.
 * Arithmetic: the bf16x3 split of section 7 of sgcdet_amd.h (weights pre-split into hi | lo planes, activations split while
 * they are staged), fp32 accumulation; sgc_set_conv_products selects the mode as for every MFMA kernel.  Observed error
 * ~1e-5 of the output scale, tests bound it at 1e-4.  SGC_ABI_VERSION of include/sgcdet_amd.h covers these declarations too.
 */
#ifndef SGCDET_AMD_IMAGE_H_
#define SGCDET_AMD_IMAGE_H_

#include "sgcdet_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SGC_CONV2D_RELU 1           /* v = max(v, 0) after scale / shift, BEFORE the residual is added */
#define SGC_CONV2D_RELU_AFTER_ADD 2 /* v = max(v, 0) after the residual is added (BasicBlock with a projection shortcut) */

/* Strided / transposed 2-D convolution over channels-last rows.
 *   x [N*H*W, Cin];  w_hi | w_lo [k*k][Cout][Cin] bf16 planes, tap = kh * k + kw;
 *   transposed == 0: ksize in {1, 3}, stride in {1, 2}, padding ksize / 2 (nn.Conv2d; weight[co][ci][kh][kw] at tap kh*k+kw);
 *                    OH = H / stride, OW = W / stride, a stride-2 layer needs even H and W;
 *   transposed == 1: nn.ConvTranspose2d(kernel 3, stride 2, padding 1, output_padding 1): OH = 2 H, OW = 2 W
 *                    (weight[ci][co][kh][kw] at tap kh*3+kw, row co, column ci; ksize = 3 and stride = 2 must be passed).
 *   Epilogue, in this order: v = acc * scale[co] + shift[co] (null: 1 / 0);  SGC_CONV2D_RELU;  + residual[row * ldr + co]
 *   (null: nothing);  SGC_CONV2D_RELU_AFTER_ADD;  softmax over columns [0, softmax_cols) of the row (0: none; needs
 *   Cout <= 128; columns behind them are stored as computed).
 *   y: row pitch ldy floats, the Cout columns start at column col0 -- columns outside [col0, col0 + Cout) are not touched,
 *   so two calls fill column ranges of one buffer (the channel concatenation).
 * Needs Cin % 32 == 0, Cout % 4 == 0, ldy % 4 == 0, col0 % 4 == 0, ldr % 4 == 0, 16-byte aligned pointers, x below 4 GiB;
 * SGC_EUNSUP otherwise, a misaligned pointer included (sgc_conv2d_nhwc_ex_supported answers the shape part of the question
 * without a launch). */
int sgc_conv2d_nhwc_ex_bf16x3(const float *x, const uint16_t *w_hi, const uint16_t *w_lo, const float *scale,
                              const float *shift, const float *residual_or_null, float *y, int N, int H, int W, int Cin,
                              int Cout, int ksize, int stride, int transposed, int flags, int ldy, int col0, int ldr,
                              int softmax_cols, sgc_stream_t stream);
int sgc_conv2d_nhwc_ex_supported(int N, int H, int W, int Cin, int Cout, int ksize, int stride, int transposed, int ldy,
                                 int col0, int ldr /* 0: no residual */, int softmax_cols);

/* The same kernel, arguments, epilogue and restrictions as sgc_conv2d_nhwc_ex_bf16x3 (transposed must be 0), for stride-2 layers
 * over maps of ANY size: OH = (H + 1) / 2, OW = (W + 1) / 2 at stride 2 -- nn.Conv2d with padding ksize / 2 for ksize 1 and 3 (the
 * ResNet stages: 15 x 20 -> 8 x 10).  y and residual have N*OH*OW rows.  On sizes both entries accept the results are
 * bit-identical; sgc_conv2d_nhwc_ex_bf16x3 and its _supported twin keep refusing odd sizes. */
int sgc_conv2d_nhwc_strided_bf16x3(const float *x, const uint16_t *w_hi, const uint16_t *w_lo, const float *scale,
                                   const float *shift, const float *residual_or_null, float *y, int N, int H, int W, int Cin,
                                   int Cout, int ksize, int stride, int transposed, int flags, int ldy, int col0, int ldr,
                                   int softmax_cols, sgc_stream_t stream);
int sgc_conv2d_nhwc_strided_supported(int N, int H, int W, int Cin, int Cout, int ksize, int stride, int transposed, int ldy,
                                      int col0, int ldr /* 0: no residual */, int softmax_cols);

/* nn.MaxPool2d(kernel_size=3, stride=2, padding=1) over channels-last rows (the pooling behind the ResNet stem):
 *   x [N*H*W, C] -> y [N*OH*OW, C], OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1, any H, W >= 1.
 * Padding takes no part in the maximum (a window always holds its centre pixel, so no -inf is stored); NaN propagates.
 * Needs C % 4 == 0 and 16-byte aligned pointers (SGC_EUNSUP otherwise). */
int sgc_maxpool2d_nhwc(const float *x, float *y, int N, int H, int W, int C, sgc_stream_t stream);

/* The ResNet stem: 7x7 stride-2 padding-3 convolution of fp32 NCHW images img [N, 3, H, W] to 64 channels,
 * v = acc * scale + shift (folded BatchNorm and bias), optional ReLU, written as channels-last rows y [N*(H/2)*(W/2), 64].
 *   w_hi | w_lo [64][160] bf16 planes: row co, column (ci * 7 + kh) * 7 + kw, columns 147..159 zero.
 * Needs even H and W and 16-byte aligned weight planes (SGC_EUNSUP otherwise). */
int sgc_conv2d_stem7_bf16x3(const float *img, const uint16_t *w_hi, const uint16_t *w_lo, const float *scale,
                            const float *shift, float *y, int N, int H, int W, int relu, sgc_stream_t stream);

/* src [N, C, H, W] -> dst [N*H*W, Cp] channels-last rows, columns C..Cp-1 written as zeros (Cp >= C, Cp % 4 == 0, dst 16-byte
 * aligned). */
int sgc_nchw_to_nhwc_padc(const float *src, float *dst, int N, int C, int H, int W, int Cp, sgc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SGCDET_AMD_IMAGE_H_ */
