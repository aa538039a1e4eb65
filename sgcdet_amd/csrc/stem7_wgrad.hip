// Weight gradient of the 7x7 stride-2 padding-3 stem (include/sgcdet_amd_train.h section 14): the backward twin of
// conv2d_stem7_kernel (conv2d_image.hip).
//
//   dw[co][(ci * 7 + kh) * 7 + kw] = sum over (n, oh, ow) of dy[(n, oh, ow)][co] * img[n][ci][2 oh + kh - 3][2 ow + kw - 3]
//
// i.e. the GEMM dy^T [64 x R] . patches [R x 147], the patches formed on the fly from the fp32 NCHW image.  The flattened column is
// the column of the forward kernel's [64][160] weight matrix, which is the parameter's own [64, 3, 7, 7] layout.
//
// Work unit = the forward's tile of 8 x 32 output pixels of one image; its 21 x 69 x 3 image patch is staged in LDS.  A workgroup
// (4 waves) walks a contiguous range of tiles; wave w owns tile rows 2w and 2w + 1, a K step is 16 consecutive output pixels of a row:
//   A (rows = output channels):  lane (co = lane & 31, half = lane >> 5) holds dy of pixels 8 half .. 8 half + 7 at channel co -- read
//                                straight from global memory (a wave load covers two pixels x 32 consecutive channels; every element
//                                of dy is read exactly once by exactly one lane, so it is not staged);
//   B (cols = patch elements):   lane (k = lane & 31, half) gathers patch[ci][2 r + kh][2 (q + e) + kw] for its 8 pixels from LDS.
// Every wave keeps the whole 64 x 160 result (2 x 5 accumulator blocks) over all its tiles; at the end the four waves' sums are
// added through LDS in wave order and wave 0 writes the 64 x 147 block -- to its slot of the workspace when the tile range is split
// over workgroups, else to dw.  A second kernel adds the slots in index order.  No atomics: the same bits on every run.
// The products are always three (bf16 hi / lo split of both operands), fp32 accumulation.
#include "common.hpp"
#include "mma.hpp"
#include "../../include/sgcdet_amd_train.h"

namespace sgc {

constexpr int SW_TH = 8, SW_TW = 32, SW_PH = 2 * SW_TH + 5, SW_PW = 2 * SW_TW + 5, SW_PWP = SW_PW + 1;   // patch 21 x 69 (+1 pad)
constexpr int SW_PATCH = 3 * SW_PH * SW_PWP;          // floats
constexpr int SW_K = 147, SW_KB = 5;                  // 147 columns in 5 blocks of 32
constexpr int SW_DW = 64 * SW_K;                      // floats of dw (and of one workspace slot)
constexpr int SW_RED = 2 * SW_KB * 16 * 64;           // floats of one wave's accumulators
constexpr int SW_MAX_SPLITS = 512;                    // workgroups the tiles are split over: the chip twice

struct Stem7WgradParams {
  const float *img;               // [N, 3, H, W]
  const float *dy;                // [N * OH * OW, 64]
  float *out;                     // dw, or the workspace [splits][64][147]
  int N, H, W, OH, OW, tiles_h, tiles_w, ntiles, splits;
};

// two waves per SIMD (160 accumulator registers + fragments fit 256, no spill): a second workgroup per CU hides the dy loads
__global__ __launch_bounds__(256, 2) void conv2d_stem7_wgrad_kernel(const Stem7WgradParams p) {
  // the patch while the tiles are walked, one wave's accumulators in the reduction behind them
  __shared__ __attribute__((aligned(16))) float smem[SW_RED > SW_PATCH ? SW_RED : SW_PATCH];
  float *patch = smem;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int fr = lane & 31, fh = lane >> 5;
  int koff[SW_KB];                                     // patch offset of this lane's column in block j; -1: a padding column
#pragma unroll
  for (int j = 0; j < SW_KB; ++j) {
    const int k = j * 32 + fr;
    const int c = k / 49, kh = (k % 49) / 7, kw = k % 7;
    koff[j] = k < SW_K ? (c * SW_PH + kh) * SW_PWP + kw : -1;
  }
  f32x16 acc[2][SW_KB];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < SW_KB; ++j)
#pragma unroll
      for (int k = 0; k < 16; ++k) acc[i][j][k] = 0.f;

  const int t0 = (int)((int64_t)blockIdx.x * p.ntiles / p.splits), t1 = (int)((int64_t)(blockIdx.x + 1) * p.ntiles / p.splits);
  for (int tile = t0; tile < t1; ++tile) {
    const int tw = tile % p.tiles_w, th = (tile / p.tiles_w) % p.tiles_h, n = tile / (p.tiles_w * p.tiles_h);
    const int oh0 = th * SW_TH, ow0 = tw * SW_TW;
    const int ih0 = 2 * oh0 - 3, iw0 = 2 * ow0 - 3;
    __syncthreads();                                   // the previous tile's fragment reads are done
    for (int e = tid; e < 3 * SW_PH * SW_PW; e += 256) {
      const int x = e % SW_PW, yy = (e / SW_PW) % SW_PH, c = e / (SW_PW * SW_PH);
      const int ih = ih0 + yy, iw = iw0 + x;
      const bool ok = ih >= 0 && ih < p.H && iw >= 0 && iw < p.W;
      patch[(c * SW_PH + yy) * SW_PWP + x] = ok ? p.img[(((int64_t)n * 3 + c) * p.H + ih) * p.W + iw] : 0.f;
    }
    __syncthreads();
#pragma unroll 1
    for (int s = 0; s < 4; ++s) {                      // K steps of the wave: tile row 2 wid + (s >> 1), pixels 16 (s & 1) .. + 15
      const int tr = 2 * wid + (s >> 1), q0 = 16 * (s & 1);
      const int oh = oh0 + tr;
      if (oh >= p.OH || ow0 + q0 >= p.OW) continue;    // wave-uniform: nothing of this step is inside the map
      const int ow = ow0 + q0 + fh * 8;                // the lane's first pixel
      const float *dyr = p.dy + (((int64_t)n * p.OH + oh) * p.OW + ow) * 64 + fr;
      bf16x8 ah[2], al[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = ow + e < p.OW ? dyr[e * 64 + i * 32] : 0.f;      // a pixel outside the map adds nothing
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const __bf16 hb = op_hi<3>(v[e]);
          ah[i][e] = hb;
          al[i][e] = op_lo<3>(v[e], hb);
        }
      }
      const int rbase = (2 * tr) * SW_PWP + 2 * (q0 + fh * 8);
#pragma unroll
      for (int j = 0; j < SW_KB; ++j) {
        bf16x8 bh, bl;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          // a pixel outside the map takes no patch element either: its dy is 0, but 0 * NaN would poison a tap that never reads that pixel
          const float v = koff[j] >= 0 && ow + e < p.OW ? patch[rbase + koff[j] + 2 * e] : 0.f;
          const __bf16 hb = op_hi<3>(v);
          bh[e] = hb;
          bl[e] = op_lo<3>(v, hb);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[i][j] = mma_split<3>(ah[i], al[i], bh, bl, acc[i][j]);
      }
    }
  }

  // the four waves' sums, added in wave order by wave 0
  float *red = smem;
  for (int w = 1; w < 4; ++w) {
    __syncthreads();                                   // the patch (w = 1) or the previous wave's sums have been read
    if (wid == w) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < SW_KB; ++j)
#pragma unroll
          for (int k = 0; k < 16; ++k) red[((i * SW_KB + j) * 16 + k) * 64 + lane] = acc[i][j][k];
    }
    __syncthreads();
    if (wid == 0) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < SW_KB; ++j)
#pragma unroll
          for (int k = 0; k < 16; ++k) acc[i][j][k] += red[((i * SW_KB + j) * 16 + k) * 64 + lane];
    }
  }
  if (wid != 0) return;
  // C layout: column = lane & 31 (patch element), row = (k & 3) + 8 (k >> 2) + 4 (lane >> 5) (output channel)
  float *out = p.out + (int64_t)blockIdx.x * SW_DW;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < SW_KB; ++j) {
      const int col = j * 32 + fr;
      if (col >= SW_K) continue;
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int co = i * 32 + (k & 3) + 8 * (k >> 2) + 4 * fh;
        out[co * SW_K + col] = acc[i][j][k];
      }
    }
}

// dw[i] = ws[0][i] + ws[1][i] + ... in index order.  A workgroup is 64 float4 columns x 4 slot lanes: lane g takes the slots
// g, g + 4, ... in order, then the four lane sums are added in lane order.
__global__ __launch_bounds__(256) void conv2d_stem7_wgrad_reduce_kernel(const float4 *__restrict__ ws, float4 *__restrict__ dw, int n4,
                                                                        int splits) {
  __shared__ float4 sm[256];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + tx;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  if (i < n4) {
#pragma unroll 4
    for (int s = ty; s < splits; s += 4) {
      const float4 b = ws[(int64_t)s * n4 + i];
      a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    }
  }
  sm[threadIdx.x] = a;
  __syncthreads();
  if (ty == 0 && i < n4) {
    for (int t = 1; t < 4; ++t) {
      const float4 b = sm[t * 64 + tx];
      a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    }
    dw[i] = a;
  }
}

// Sizes, tiles and the split of a shape; 0 or the error the entry returns for it.
static int stem7_wgrad_geometry(Stem7WgradParams &p, int N, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0) return set_error(SGC_EINVAL, "sgc_conv2d_stem7_wgrad_bf16x3: non-positive size");
  if ((H | W) & 1) return set_error(SGC_EUNSUP, "sgc_conv2d_stem7_wgrad_bf16x3: needs even H and W");
  if ((int64_t)N * 3 * H * W * 4 >= ((int64_t)1 << 32) || (int64_t)N * (H / 2) * (W / 2) * 64 * 4 >= ((int64_t)1 << 32))
    return set_error(SGC_EUNSUP, "sgc_conv2d_stem7_wgrad_bf16x3: img and dy must stay below 4 GiB each");
  p.N = N; p.H = H; p.W = W; p.OH = H / 2; p.OW = W / 2;
  p.tiles_h = ceil_div(p.OH, SW_TH); p.tiles_w = ceil_div(p.OW, SW_TW);
  p.ntiles = N * p.tiles_h * p.tiles_w;                // at most one tile per output pixel, and dy's 256-byte rows are below 2^24
  p.splits = p.ntiles < SW_MAX_SPLITS ? p.ntiles : SW_MAX_SPLITS;
  return SGC_OK;
}
}  // namespace sgc

using namespace sgc;

extern "C" int64_t sgc_conv2d_stem7_wgrad_workspace_floats(int N, int H, int W) {
  Stem7WgradParams p = {};
  if (stem7_wgrad_geometry(p, N, H, W)) return -1;
  return p.splits > 1 ? (int64_t)p.splits * SW_DW : 0;
}

extern "C" int sgc_conv2d_stem7_wgrad_bf16x3(const float *img, const float *dy, float *dw, int N, int H, int W,
                                             float *workspace_or_null, int64_t workspace_floats, sgc_stream_t stream) {
  if (!img || !dy || !dw) return set_error(SGC_EINVAL, "sgc_conv2d_stem7_wgrad_bf16x3: null pointer");
  if (((uintptr_t)img | (uintptr_t)dy | (uintptr_t)dw | (uintptr_t)workspace_or_null) & 15)
    return set_error(SGC_EINVAL, "sgc_conv2d_stem7_wgrad_bf16x3: pointers must be 16-byte aligned");
  Stem7WgradParams p = {};
  if (int rc = stem7_wgrad_geometry(p, N, H, W)) return rc;
  if (p.splits > 1 && !(workspace_or_null && workspace_floats >= (int64_t)p.splits * SW_DW)) p.splits = 1;   // one workgroup walks every tile
  p.img = img; p.dy = dy; p.out = p.splits > 1 ? workspace_or_null : dw;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(conv2d_stem7_wgrad_kernel, dim3(p.splits), dim3(256), 0, st, p);
  if (int rc = check_launch("conv2d_stem7_wgrad_kernel")) return rc;
  if (p.splits > 1) {
    const int n4 = SW_DW / 4;
    hipLaunchKernelGGL(conv2d_stem7_wgrad_reduce_kernel, dim3(ceil_div(n4, 64)), dim3(256), 0, st,
                       reinterpret_cast<const float4 *>(workspace_or_null), reinterpret_cast<float4 *>(dw), n4, p.splits);
    return check_launch("conv2d_stem7_wgrad_reduce_kernel");
  }
  return SGC_OK;
}
