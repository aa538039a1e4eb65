// Voxel-mask utilities of the neck and head (not convolutions): 3x3x3 dilation and the valid-mask pyramid.
#include "common.hpp"

using namespace sgc;

// 3x3x3 dilation of a {0,1} voxel mask (what a 3x3x3 convolution must produce so that its consumer is exact on `in`)
__global__ void mask_dilate3_kernel(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, int X, int Y, int Z) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= (int64_t)X * Y * Z) return;
  const int z = (int)(v % Z), y = (int)((v / Z) % Y), x = (int)(v / ((int64_t)Z * Y));
  uint8_t any = 0;
  for (int dx = -1; dx <= 1; ++dx)
    for (int dy = -1; dy <= 1; ++dy)
      for (int dz = -1; dz <= 1; ++dz) {
        const int a = x + dx, b = y + dy, c = z + dz;
        if (a >= 0 && a < X && b >= 0 && b < Y && c >= 0 && c < Z) any |= in[((int64_t)a * Y + b) * Z + c];
      }
  out[v] = any ? 1 : 0;
}

extern "C" int sgc_mask_dilate3(const uint8_t *mask_in, uint8_t *mask_out, int X, int Y, int Z, sgc_stream_t stream) {
  if (!mask_in || !mask_out || mask_in == mask_out) return set_error(SGC_EINVAL, "sgc_mask_dilate3: null or aliased pointers");
  if (X <= 0 || Y <= 0 || Z <= 0) return set_error(SGC_EINVAL, "sgc_mask_dilate3: bad size");
  const int64_t n = (int64_t)X * Y * Z;
  hipLaunchKernelGGL(mask_dilate3_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, mask_in, mask_out, X, Y, Z);
  return check_launch("mask_dilate3_kernel");
}

// valid masks of the head's scales: nn.Upsample(size, mode='trilinear')(valid.float()).round().bool()
// (dense_heads/imvoxel_head_v2.py:123,258) for integer factors f = 2^s: align_corners=False puts every coarse voxel half-way
// between fine voxels f*d + f/2 - 1 and f*d + f/2 on each axis, i.e. the mean of 8 fine voxels; round() is half-to-even,
// so a coarse voxel is valid iff at least 5 of the 8 are.
__global__ void valid_pyramid_kernel(const int64_t *__restrict__ valid, uint8_t *__restrict__ out, int X, int Y, int Z, int f) {
  const int cx = X / f, cy = Y / f, cz = Z / f;
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= (int64_t)cx * cy * cz) return;
  const int z = (int)(v % cz), y = (int)((v / cz) % cy), x = (int)(v / ((int64_t)cz * cy));
  if (f == 1) { out[v] = valid[v] != 0; return; }
  const int o = f / 2 - 1;
  int cnt = 0;
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < 2; ++b)
      for (int c = 0; c < 2; ++c)
        cnt += valid[((int64_t)(x * f + o + a) * Y + (y * f + o + b)) * Z + (z * f + o + c)] != 0;
  out[v] = cnt >= 5;
}

extern "C" int sgc_valid_pyramid(const int64_t *valid, uint8_t *mask_out, int X, int Y, int Z, int factor, sgc_stream_t stream) {
  if (!valid || !mask_out) return set_error(SGC_EINVAL, "sgc_valid_pyramid: null pointer");
  if (X <= 0 || Y <= 0 || Z <= 0 || factor < 1 || (factor & (factor - 1)) || X % factor || Y % factor || Z % factor)
    return set_error(SGC_EUNSUP, "sgc_valid_pyramid: factor must be a power of two dividing the grid");
  const int64_t n = (int64_t)(X / factor) * (Y / factor) * (Z / factor);
  hipLaunchKernelGGL(valid_pyramid_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, valid, mask_out, X, Y, Z, factor);
  return check_launch("valid_pyramid_kernel");
}
