// Backward of the frozen-norm epilogue of the image convolutions (include/sgcdet_amd_train.h): for a layer
// y = act(conv(x) * scale + shift [+ residual]) whose norm is frozen, the gradient that feeds the convolution's input and weight
// gradients is the incoming one, masked by the ReLU and multiplied by the folded scale; the residual's gradient is the masked
// one itself.  A streaming kernel: one pass over dy and y, one or two stores, a float4 per thread and step, 64-bit row offsets.
// The mask is a select (torch's threshold_backward): an element the ReLU closed gets 0 whatever dy holds there, everywhere else
// dy -- a NaN included -- goes through; the product with the scale is one fp32 multiply.
#include <algorithm>

#include "common.hpp"
#include "../../include/sgcdet_amd_train.h"

namespace sgc {

__global__ __launch_bounds__(256) void frozen_norm_act_backward_kernel(const float4 *__restrict__ dy, const float4 *__restrict__ y,
                                                                       const float4 *__restrict__ scale, float4 *__restrict__ g,
                                                                       float4 *__restrict__ gres, int C4, int64_t total) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    float4 d = dy[e];
    if (y) {
      const float4 v = y[e];
      d.x = v.x > 0.f ? d.x : 0.f; d.y = v.y > 0.f ? d.y : 0.f; d.z = v.z > 0.f ? d.z : 0.f; d.w = v.w > 0.f ? d.w : 0.f;
    }
    if (gres) gres[e] = d;
    if (scale) {
      const float4 s = scale[e % C4];
      d.x *= s.x; d.y *= s.y; d.z *= s.z; d.w *= s.w;
    }
    g[e] = d;
  }
}
}  // namespace sgc

using namespace sgc;

extern "C" int sgc_frozen_norm_act_backward(const float *dy, const float *y_or_null, const float *scale_or_null, float *g,
                                            float *gres_or_null, int64_t rows, int C, int relu, sgc_stream_t stream) {
  if (!dy || !g) return set_error(SGC_EINVAL, "sgc_frozen_norm_act_backward: null pointer");
  if (relu && !y_or_null) return set_error(SGC_EINVAL, "sgc_frozen_norm_act_backward: the ReLU gate needs y");
  if (rows <= 0 || C <= 0) return set_error(SGC_EINVAL, "sgc_frozen_norm_act_backward: non-positive size");
  if (C % 4) return set_error(SGC_EUNSUP, "sgc_frozen_norm_act_backward: needs C %% 4 == 0");
  if ((reinterpret_cast<uintptr_t>(dy) | reinterpret_cast<uintptr_t>(y_or_null) | reinterpret_cast<uintptr_t>(scale_or_null) |
       reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(gres_or_null)) & 15)
    return set_error(SGC_EUNSUP, "sgc_frozen_norm_act_backward: pointers must be 16-byte aligned");
  const int64_t total = rows * (C / 4);
  const int grid = (int)std::min<int64_t>((total + 255) / 256, 65536);
  hipLaunchKernelGGL(frozen_norm_act_backward_kernel, dim3(grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const float4 *>(dy), reinterpret_cast<const float4 *>(relu ? y_or_null : nullptr),
                     reinterpret_cast<const float4 *>(scale_or_null), reinterpret_cast<float4 *>(g),
                     reinterpret_cast<float4 *>(gres_or_null), C / 4, total);
  return check_launch("frozen_norm_act_backward_kernel");
}
