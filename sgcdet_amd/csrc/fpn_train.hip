// Streaming kernels of the image FPN's training path (include/sgcdet_amd_train.h section 13): the top-down step
// (nearest upsample to the finer size + add) forward and backward on channels-last rows, and the column sum of a [rows, C]
// gradient (a convolution's bias gradient).  float4 per thread and step, 64-bit element offsets, every argument checked on the
// host before a launch.  None of them uses an atomic: each output element has one owner and a fixed summation order, so two runs
// give the same bits.
//
// Index rule of the two top-down kernels (plugin/fpn.py ``_nearest_index``, == F.interpolate(mode="nearest") for the sizes a
// stride-2 stage produces): source index of destination d is min(d * src / dst, src - 1) in integers; the destinations that read
// source s are the contiguous range [ceil(s * dst / src), ceil((s + 1) * dst / src)), cut at dst.
#include <algorithm>

#include "common.hpp"
#include "../../include/sgcdet_amd_train.h"

namespace sgc {

__device__ __forceinline__ float4 add4(float4 a, const float4 b) {
  a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
  return a;
}

// out may be fine itself (no __restrict__ on the two): an element is read and written by the same thread only.
__global__ __launch_bounds__(256) void upsample_nearest_add_kernel(const float4 *fine, const float4 *__restrict__ coarse, float4 *out,
                                                                   int Hd, int Wd, int Hs, int Ws, int C4, int64_t total) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int c4 = (int)(e % C4);
    int64_t pix = e / C4;
    const int w = (int)(pix % Wd);
    pix /= Wd;
    const int h = (int)(pix % Hd);
    const int64_t n = pix / Hd;
    const int ih = min((int)((int64_t)h * Hs / Hd), Hs - 1), iw = min((int)((int64_t)w * Ws / Wd), Ws - 1);
    out[e] = add4(fine[e], coarse[((n * Hs + ih) * Ws + iw) * C4 + c4]);
  }
}

// Gather form: one thread owns a float4 of gcoarse and adds its preimage rectangle of gout, h outer, w inner.
__global__ __launch_bounds__(256) void upsample_nearest_add_backward_kernel(const float4 *__restrict__ gout, float4 *__restrict__ gcoarse,
                                                                            int Hd, int Wd, int Hs, int Ws, int C4, int64_t total) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int c4 = (int)(e % C4);
    int64_t pix = e / C4;
    const int ws = (int)(pix % Ws);
    pix /= Ws;
    const int hs = (int)(pix % Hs);
    const int64_t n = pix / Hs;
    const int h0 = (int)(((int64_t)hs * Hd + Hs - 1) / Hs), h1 = min((int)(((int64_t)(hs + 1) * Hd + Hs - 1) / Hs), Hd);
    const int w0 = (int)(((int64_t)ws * Wd + Ws - 1) / Ws), w1 = min((int)(((int64_t)(ws + 1) * Wd + Ws - 1) / Ws), Wd);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int h = h0; h < h1; ++h)
      for (int w = w0; w < w1; ++w) acc = add4(acc, gout[((n * Hd + h) * Wd + w) * C4 + c4]);
    gcoarse[e] = acc;
  }
}

// Column sums of x [rows, C4 float4] over the row range [blockIdx.y * R, min(+R, rows)) -> part[blockIdx.y][C4].  A workgroup is
// TX = 1 << tx_log2 column lanes by TY = 256 / TX row lanes and walks the column tiles blockIdx.x, + gridDim.x, ...  Row lane ty takes
// the rows r0 + ty, + TY, ... of the range, the i-th of them into accumulator i % 4 (four loads in flight); then a0 + a1 + a2 + a3,
// then the TY lane sums are added in lane order by lane 0.  A value therefore passes through at most
//   ceil(ceil(R / TY) / 4) + 3 + (TY - 1)
// dependent fp32 adds (``colsum_chain``).  sgc_rows_colsum launches it twice: over x with one range per workgroup row, then with
// one workgroup over the partial sums.
__global__ __launch_bounds__(256) void rows_colsum_kernel(const float4 *__restrict__ x, float4 *__restrict__ part, int64_t rows, int C4,
                                                          int64_t R, int tx_log2) {
  __shared__ float4 sm[256];
  const int TX = 1 << tx_log2, TY = 256 >> tx_log2;
  const int tx = threadIdx.x & (TX - 1), ty = threadIdx.x >> tx_log2;
  const int64_t r0 = (int64_t)blockIdx.y * R, r1 = std::min<int64_t>(r0 + R, rows);
  for (int base = blockIdx.x * TX; base < C4; base += gridDim.x * TX) {          // uniform over the workgroup
    const int c4 = base + tx;
    float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0, a2 = a0, a3 = a0;
    if (c4 < C4) {
      int64_t r = r0 + ty;
      for (; r + 3 * (int64_t)TY < r1; r += 4 * TY) {
        const float4 v0 = x[r * C4 + c4], v1 = x[(r + TY) * C4 + c4], v2 = x[(r + 2 * TY) * C4 + c4], v3 = x[(r + 3 * TY) * C4 + c4];
        a0 = add4(a0, v0); a1 = add4(a1, v1); a2 = add4(a2, v2); a3 = add4(a3, v3);
      }
      if (r < r1) a0 = add4(a0, x[r * C4 + c4]);
      if (r + TY < r1) a1 = add4(a1, x[(r + TY) * C4 + c4]);
      if (r + 2 * (int64_t)TY < r1) a2 = add4(a2, x[(r + 2 * TY) * C4 + c4]);
    }
    sm[threadIdx.x] = add4(add4(add4(a0, a1), a2), a3);
    __syncthreads();
    if (ty == 0 && c4 < C4) {
      float4 s = sm[tx];
      for (int t = 1; t < TY; ++t) s = add4(s, sm[(t << tx_log2) + tx]);
      part[(int64_t)blockIdx.y * C4 + c4] = s;
    }
    __syncthreads();
  }
}

// Launch geometry of sgc_rows_colsum.  P row ranges of R rows: about 64 rows per range for small inputs, at most 256 ranges (one
// workgroup per CU) until a range would exceed 2048 rows.  ``chain`` is the longest run of dependent fp32 adds from an input element
// to its output over both stages; the entry refuses a shape whose chain exceeds 160 (the error bound the tests assert rests on it).
// At the largest shape of config 2, rows = 192 000 and C = 256 (TX 64, TY 4): P = 256, R = 750 -> 47 + 3 + 3 = 53 in the first
// stage and 16 + 3 + 3 = 22 in the second, 75 in all.  rows = 19 200, C = 256: R = 75 -> 11 + 22 = 33.
struct ColsumGeom {
  int tx_log2, P;
  int64_t R;
  int chain;
};

static int colsum_chain(int64_t n, int tx_log2) {          // n rows in one range
  const int64_t TY = 256 >> tx_log2;
  const int64_t per_lane = (n + TY - 1) / TY;
  return (int)((per_lane + 3) / 4 + 3 + (TY - 1));
}

static bool colsum_geom(int64_t rows, int C, ColsumGeom *g) {
  if (rows <= 0 || C <= 0 || C % 4 || rows > ((int64_t)1 << 31)) return false;
  const int C4 = C / 4;
  int t = 3;
  while (t < 6 && (1 << t) < C4) ++t;
  int64_t P = std::max<int64_t>(std::min<int64_t>((rows + 63) / 64, 256), (rows + 2047) / 2048);
  const int64_t R = (rows + P - 1) / P;
  P = (rows + R - 1) / R;                                   // no empty range
  g->tx_log2 = t; g->P = (int)P; g->R = R;
  g->chain = colsum_chain(R, t) + (P > 1 ? colsum_chain(P, t) : 0);
  return P <= 65535 && g->chain <= 160;
}

static bool elems_fit(int64_t a, int64_t b, int64_t c, int64_t d) {          // a * b * c * d below 2^46, every factor positive
  const int64_t lim = (int64_t)1 << 46;
  int64_t t = a;
  for (int64_t f : {b, c, d}) {
    if (t > lim / f) return false;
    t *= f;
  }
  return true;
}

static int check_top_down(const char *who, const void *a, const void *b, const void *c, int N, int Hd, int Wd, int Hs, int Ws, int C) {
  if (!a || !b || !c) return set_error(SGC_EINVAL, "%s: null pointer", who);
  if (N <= 0 || Hd <= 0 || Wd <= 0 || Hs <= 0 || Ws <= 0 || C <= 0) return set_error(SGC_EINVAL, "%s: non-positive size", who);
  if (Hs > Hd || Ws > Wd) return set_error(SGC_EINVAL, "%s: the coarse map must not be larger than the fine one", who);
  if (C % 4) return set_error(SGC_EUNSUP, "%s: needs C %% 4 == 0", who);
  if ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15)
    return set_error(SGC_EUNSUP, "%s: pointers must be 16-byte aligned", who);
  if (!elems_fit(N, Hd, Wd, C)) return set_error(SGC_EUNSUP, "%s: map too large", who);
  return 0;
}
}  // namespace sgc

using namespace sgc;

extern "C" int sgc_upsample_nearest_add_nhwc(const float *fine, const float *coarse, float *out, int N, int Hd, int Wd, int Hs, int Ws,
                                             int C, sgc_stream_t stream) {
  if (int rc = check_top_down("sgc_upsample_nearest_add_nhwc", fine, coarse, out, N, Hd, Wd, Hs, Ws, C)) return rc;
  const int64_t total = (int64_t)N * Hd * Wd * (C / 4);
  const int grid = (int)std::min<int64_t>((total + 255) / 256, 65536);
  hipLaunchKernelGGL(upsample_nearest_add_kernel, dim3(grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const float4 *>(fine), reinterpret_cast<const float4 *>(coarse), reinterpret_cast<float4 *>(out),
                     Hd, Wd, Hs, Ws, C / 4, total);
  return check_launch("upsample_nearest_add_kernel");
}

extern "C" int sgc_upsample_nearest_add_backward_nhwc(const float *gout, float *gcoarse, int N, int Hd, int Wd, int Hs, int Ws, int C,
                                                      sgc_stream_t stream) {
  if (int rc = check_top_down("sgc_upsample_nearest_add_backward_nhwc", gout, gcoarse, gcoarse, N, Hd, Wd, Hs, Ws, C)) return rc;
  const int64_t total = (int64_t)N * Hs * Ws * (C / 4);
  const int grid = (int)std::min<int64_t>((total + 255) / 256, 65536);
  hipLaunchKernelGGL(upsample_nearest_add_backward_kernel, dim3(grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const float4 *>(gout), reinterpret_cast<float4 *>(gcoarse), Hd, Wd, Hs, Ws, C / 4, total);
  return check_launch("upsample_nearest_add_backward_kernel");
}

extern "C" int64_t sgc_rows_colsum_workspace_floats(int64_t rows, int C) {
  ColsumGeom g;
  if (!colsum_geom(rows, C, &g)) {
    set_error(SGC_EUNSUP, "sgc_rows_colsum: needs rows >= 1, C >= 4, C %% 4 == 0 and a row count its 160-add chain bound covers");
    return -1;
  }
  return g.P > 1 ? (int64_t)g.P * C : 0;
}

extern "C" int sgc_rows_colsum(const float *x, float *out, int64_t rows, int C, float *workspace, int64_t workspace_floats,
                               sgc_stream_t stream) {
  if (!x || !out) return set_error(SGC_EINVAL, "sgc_rows_colsum: null pointer");
  if (rows <= 0 || C <= 0) return set_error(SGC_EINVAL, "sgc_rows_colsum: non-positive size");
  if (C % 4) return set_error(SGC_EUNSUP, "sgc_rows_colsum: needs C %% 4 == 0");
  ColsumGeom g;
  if (!colsum_geom(rows, C, &g)) return set_error(SGC_EUNSUP, "sgc_rows_colsum: too many rows for the 160-add chain bound");
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(workspace)) & 15)
    return set_error(SGC_EUNSUP, "sgc_rows_colsum: pointers must be 16-byte aligned");
  if (g.P > 1 && (!workspace || workspace_floats < (int64_t)g.P * C))
    return set_error(SGC_EINVAL, "sgc_rows_colsum: needs a workspace of sgc_rows_colsum_workspace_floats(rows, C) floats");
  const int C4 = C / 4, TX = 1 << g.tx_log2;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  float4 *first = reinterpret_cast<float4 *>(g.P > 1 ? workspace : out);
  hipLaunchKernelGGL(rows_colsum_kernel, dim3((C4 + TX - 1) / TX, g.P), dim3(256), 0, st, reinterpret_cast<const float4 *>(x), first,
                     rows, C4, g.R, g.tx_log2);
  if (int rc = check_launch("rows_colsum_kernel")) return rc;
  if (g.P > 1) {
    hipLaunchKernelGGL(rows_colsum_kernel, dim3(1, 1), dim3(256), 0, st, reinterpret_cast<const float4 *>(workspace),
                       reinterpret_cast<float4 *>(out), (int64_t)g.P, C4, (int64_t)g.P, g.tx_log2);
    return check_launch("rows_colsum_kernel (partials)");
  }
  return 0;
}
