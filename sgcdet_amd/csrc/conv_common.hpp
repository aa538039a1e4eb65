// What the convolution files share: the kernel parameter block, the tile constants, the plan that conv3d.hip makes of a call
// and the launchers of the kernel families (conv3d_igemm.hip, conv3d_halo.hip) that carry it out.
#pragma once
#include "common.hpp"

namespace sgc {
extern int g_conv_products;   // conv3d.hip (sgc_set_conv_products): the NP of mma.hpp in every bf16 MFMA kernel; not a tuning knob

// rows_gemm.hip: persistent weight-stationary form of the K <= 256 row GEMMs (every Linear of a level, the 1x1x1 layers)
bool rows_gemm_supported(int K, int N, int hm_cm, int hm_S, int64_t rows, int64_t ldx);
int device_cus();                // rows_gemm.hip: multiProcessorCount of the current device, cached
int rows_gemm_launch(const float *x, int64_t ldx, const uint16_t *w_hi, const uint16_t *w_lo, const float *scale,
                     const float *shift, const float *residual, void *y, const int32_t *m_dev, int M, int K, int N, int relu,
                     int hm_S, int hm_cm, int hm_bf16, hipStream_t st, float *zero_row = nullptr);
// its gather form (sgc_pairs_geometry_linear_bf16x3, dfa3d_fwd.hip): row r of the A operand is sum_k gw[r][k] * x[go[r][k]][:]
bool rows_gemm_gather_supported(int K, int N, int64_t x_rows, int64_t rows);
int rows_gemm_gather_launch(const float *x, int64_t x_rows, const float *gw, const int32_t *go, const uint16_t *w_hi, const uint16_t *w_lo,
                            const float *shift, float *y, const int32_t *m_dev, int M, int K, int N, hipStream_t st);

struct ConvParams {
  const float *x;         // [IV, Cin] channels-last input volume
  const float *w;         // [taps][Cout][Cin]
  const float *scale;     // [Cout] or null (= 1)
  const float *shift;     // [Cout] or null (= 0)
  const float *residual;  // [OV, Cout] or null
  float *y;               // [OV, Cout]
  int Cin, Cout;
  int ix, iy, iz;         // input grid
  int gx, gy, gz;         // GEMM-row grid (conv: output grid; transposed: input grid)
  int ksize, stride, pad; // conv geometry (transposed: ksize = 1 per parity)
  int transposed;         // 1: ConvTranspose3d k=2 s=2, parity = blockIdx.z % 8
  int relu;
  int taps;               // ksize^3
  int splitk;             // number of tap groups (divides taps); >1 -> atomic accumulate, no epilogue
  int steps_per;          // bf16x3 tile kernel, splitk > 1: K steps (32 channels of one tap) per split; the last split may hold fewer
  int M;                  // gx*gy*gz: GEMM rows of ONE scene
  int scenes;             // volumes of one launch (sgc_conv3d_cl_bf16x3_batched): x holds scenes * ix*iy*iz rows, y / residual / a workspace
                          // slab scenes * OV rows, scene s first; a workgroup's halo ends at its scene's border.  The tile kernel walks
                          // M * scenes GEMM rows and decodes the scene per row; the halo kernels launch scenes * bricks workgroups
  float *ws;              // optional split-K workspace [splitk][OV][Cout]: every split stores its partial tile there and
  int64_t ws_stride;      // the epilogue kernel sums them in split order (deterministic); null: float atomics into y
  int64_t ws_floats;      // capacity of ws
  const int32_t *m_dev;   // optional: the live row count lives on the device (sgc_linear_rows_*); rows >= *m_dev
                          // are neither read nor written and workgroups past it exit at once
  const uint8_t *out_mask; // optional [OV] {0,1}: OUTPUT mask of a 3x3x3 stride-1 layer on the halo kernel (sgc_conv3d_cl_bf16x3_masked):
                          // rows with mask 0 are not needed by the caller.  Tiles of 64 voxels (one wave) without a live row skip
                          // their MFMAs, bricks without one skip everything; what they store is the epilogue of a zero
                          // accumulator (finite, deterministic).  Live rows are bit-identical to the dense launch.
  int two_d;              // 2-D convolution over a stack of images: grid (x, y, z) = (image, row, column), the taps only span (y, z)
                          // (sgc_conv2d_nhwc_bf16x3: the FPN output convolutions)
  unsigned long long *stamps;  // diagnostic builds only (SGC_HALO_STAMPS)
  int xcd_deal;           // tile kernel: how workgroups are dealt to the 8 XCDs (hardware: linear id % 8).  0 = as launched;
                          // 1 = consecutive ROW tiles of one (column tile, split) on one XCD (they share a weight slab);
                          // 2 = consecutive COLUMN tiles of one (row tile, split) on one XCD (they share the gathered rows)
  int wz_Z;               // WZ kernels: z extent of the raw volume behind the virtual image stack (J = wz_Z / 2 pairs per position)
  int w_group_images;     // 2-D form only, > 0: the image stack is made of groups of this many images, group g convolves with the
                          // weight set w + g * taps * Cout * Cin (the four transform-domain positions of sgc_conv3d_winograd_z_bf16x3)
  float *zero_row;        // optional: Cout floats this launch sets to zero (workgroup (0, 0, 0); sgc_linear_rows_zrow_bf16x3)
  const float *act_scale; // optional: columns [act_c0, act_c1) leave as expf(v * *act_scale) -- the head's `exp(scale(reg))` (dense_heads/
  int act_c0, act_c1;     // imvoxel_head_v2.py:79,110: mmcv Scale then torch.exp) applied last in the epilogue (sgc_conv3d_cl_bf16x3_act)
  int hm_bf16;            // head-major output stored as bfloat16 (RNE of the fp32 result)
  int hm_S, hm_cm;        // hm_cm > 0: HEAD-MAJOR output of a row-list GEMM -- row r = n * hm_S + s, column c = h * hm_cm + j
                          // is stored at y[((n * (Cout / hm_cm) + h) * hm_S + s) * hm_cm + j] (sgc_linear_rows_headmajor_bf16x3)
};

// the optional output activation of a column range (ConvParams.act_*): applied after scale / shift / relu / residual
__device__ __forceinline__ float act_col(float v, int col, int c0, int c1, float s) { return (col >= c0 && col < c1) ? expf(v * s) : v; }
__device__ __forceinline__ float4 act_col4(float4 v, int col, int c0, int c1, float s) {
  if (c1 <= c0) return v;
  return make_float4(act_col(v.x, col, c0, c1, s), act_col(v.y, col + 1, c0, c1, s), act_col(v.z, col + 2, c0, c1, s), act_col(v.w, col + 3, c0, c1, s));
}

constexpr int BM = 128, BK = 32, LDK = BK + 4;

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
constexpr int LDKH = BK + 8;   // bf16 elements per LDS row (80 B): conflict-free ds_read_b128
// dynamic LDS of a bf16x3 tile workgroup (igemm_tile.hpp): two buffers of A_hi | A_lo [BM][LDKH] and B_hi | B_lo [bn][LDKH]
constexpr int igemm_tile_lds_bytes(int bn) { return 2 * (2 * BM + 2 * bn) * LDKH * 2; }

struct ConvParamsB : ConvParams {
  const __bf16 *w_hi, *w_lo;   // [taps][Cout][Cin]
};

// What plan_conv (conv3d.hip) decides for one call of the bf16x3 convolution -- the launch and the workspace query both read it
enum ConvFamily { kConvRowsGemm, kConvHalo, kConvHaloGrid, kConvHalo2D, kConvHaloWZ, kConvTile };
struct ConvPlan {
  ConvFamily family;        // row GEMM | halo bricks | whole-grid halo brick | 2-D halo form | its virtual Winograd stack | tile kernel
  int bx, by, bz;           // halo families: the brick
  int bn;                   // columns per workgroup tile: 32 | 64 | 128
  int mfma;                 // Winograd stack: the MFMA shape of its bricks, 32 (32x32x16, as every other family) | 16 (16x16x32)
  int splitk, steps_per;    // reduction splits; tile kernel: K steps per split (ConvParams.steps_per)
  int64_t ws_floats;        // split-K workspace this choice needs for a deterministic sum (0: one split)
  const char *unsupported;  // non-null: no kernel takes the call, and why
};

// conv3d_igemm.hip: the tile-per-workgroup kernels; grid.z carries parity x splits
int launch_igemm_f32(const ConvParams &p, bool narrow, dim3 grid, hipStream_t st);
void launch_igemm(const ConvParamsB &p, bool narrow, dim3 grid, size_t smem, hipStream_t st);
// conv3d_halo*.hip: the halo kernel of pl.family / brick / bn with p.splitk splits
int launch_halo(ConvParamsB &p, const ConvPlan &pl, hipStream_t st);
}  // namespace sgc
