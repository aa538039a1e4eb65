// nn.MaxPool2d(kernel_size=3, stride=2, padding=1) over channels-last rows (include/sgcdet_amd_image.h): the pooling between the
// ResNet stem and layer1 (mmdet ResNet.forward: conv1 / norm1 / relu / maxpool), DESIGN.md 4.11.
//
// A streaming kernel: 4 bytes read per byte written, no arithmetic to speak of.  Work split: one thread owns a channel quad of one
// output column and walks a strip of MP_ROWS output rows down the image.  Per input row it takes the maximum over the (up to) three
// columns of its window -- three float4 loads whose neighbours in the workgroup read the adjacent columns, so the column overlap
// of the windows is served by the vector cache -- and keeps the row maximum of the input row that two consecutive output rows
// share in registers: 2 MP_ROWS + 1 input rows per MP_ROWS output rows instead of 3 per row.  Lanes run over channel quads first,
// then output columns: every load and store instruction moves whole rows of C floats (256-byte runs at C = 64).
// Padding takes no part: a tap outside the image is skipped, and the centre tap (2 oh, 2 ow) always lies inside, so a window is
// never empty.  The maximum propagates NaN like torch's kernel (`v > m || isnan(v)`).
#include <algorithm>

#include "common.hpp"
#include "../../include/sgcdet_amd_image.h"

namespace sgc {

constexpr int MP_ROWS = 4;      // output rows per thread

__device__ __forceinline__ float max_nan(float m, float v) { return (v > m || v != v) ? v : m; }
__device__ __forceinline__ float4 max_nan4(float4 m, float4 v) {
  return make_float4(max_nan(m.x, v.x), max_nan(m.y, v.y), max_nan(m.z, v.z), max_nan(m.w, v.w));
}

__global__ __launch_bounds__(256) void maxpool2d_nhwc_kernel(const float *__restrict__ x, float *__restrict__ y, int H, int W, int C4,
                                                             int OH, int OW, int strips, int64_t total) {
  const int64_t C = (int64_t)C4 * 4;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int q = (int)(e % C4);
    int64_t r = e / C4;
    const int ow = (int)(r % OW); r /= OW;
    const int s = (int)(r % strips);
    const int64_t n = r / strips;
    const int oh0 = s * MP_ROWS, oh1 = min(oh0 + MP_ROWS, OH);
    const int iw = 2 * ow;
    const bool left = iw > 0, right = iw + 1 < W;
    // maximum over the window's columns of input row ih (0 <= ih < H)
    auto row_max = [&](int ih) -> float4 {
      const float *p = x + (((int64_t)n * H + ih) * W + iw) * C + q * 4;
      float4 m = *reinterpret_cast<const float4 *>(p);
      if (left) m = max_nan4(m, *reinterpret_cast<const float4 *>(p - C));
      if (right) m = max_nan4(m, *reinterpret_cast<const float4 *>(p + C));
      return m;
    };
    float4 above = make_float4(0.f, 0.f, 0.f, 0.f);
    bool has_above = oh0 > 0;
    if (has_above) above = row_max(2 * oh0 - 1);
    for (int oh = oh0; oh < oh1; ++oh) {
      float4 m = row_max(2 * oh);
      if (has_above) m = max_nan4(m, above);
      if (2 * oh + 1 < H) {
        above = row_max(2 * oh + 1);
        m = max_nan4(m, above);
      }
      has_above = true;
      *reinterpret_cast<float4 *>(y + (((int64_t)n * OH + oh) * OW + ow) * C + q * 4) = m;
    }
  }
}
}  // namespace sgc

using namespace sgc;

extern "C" int sgc_maxpool2d_nhwc(const float *x, float *y, int N, int H, int W, int C, sgc_stream_t stream) {
  if (!x || !y) return set_error(SGC_EINVAL, "sgc_maxpool2d_nhwc: null pointer");
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0) return set_error(SGC_EINVAL, "sgc_maxpool2d_nhwc: non-positive size");
  if (C % 4) return set_error(SGC_EUNSUP, "sgc_maxpool2d_nhwc: needs C %% 4 == 0");
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15)
    return set_error(SGC_EUNSUP, "sgc_maxpool2d_nhwc: pointers must be 16-byte aligned");
  const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
  const int strips = ceil_div(OH, MP_ROWS);
  const int64_t total = (int64_t)N * strips * OW * (C / 4);
  const int64_t blocks = (total + 255) / 256;
  const int grid = (int)std::min<int64_t>(blocks, 65536);
  hipLaunchKernelGGL(maxpool2d_nhwc_kernel, dim3(grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x, y, H, W, C / 4, OH, OW,
                     strips, total);
  return check_launch("maxpool2d_nhwc_kernel");
}
