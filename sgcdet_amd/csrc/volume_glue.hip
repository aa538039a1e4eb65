// Volume and hand-over glue for gfx950: row scatters into the dense volume, the NCHW <-> channels-last transposes of the
// feature maps, the x2 trilinear upsample fused with the occupancy head and its adjoint.
#include "common.hpp"

namespace sgc {

__global__ void scatter_rows_kernel(const float *__restrict__ rows, const int32_t *__restrict__ idx,
                                    const int32_t *__restrict__ idx2, float *__restrict__ vol, int n, int C, int VEC,
                                    const int32_t *__restrict__ n_dev) {
  if (n_dev) n = min(n, *n_dev);
  const int CV = C / VEC;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < (int64_t)n * CV;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int i = (int)(t / CV), c = (int)(t - (int64_t)i * CV);
    int64_t d = idx[i];
    if (idx2) d = idx2[d];
    if (VEC == 4)
      reinterpret_cast<float4 *>(vol + d * C)[c] = reinterpret_cast<const float4 *>(rows + (int64_t)i * C)[c];
    else
      vol[d * C + c] = rows[(int64_t)i * C + c];
  }
}

// [N,C,Hs,Ws] -> [N,H*W,C] crop + transpose through a padded 32x33 LDS tile:
// reads coalesced along w, writes coalesced along c.
__global__ __launch_bounds__(256) void nchw_to_nhwc_kernel(const float *__restrict__ src, float *__restrict__ dst,
                                                           int C, int Hs, int Ws, int H, int W, int step) {
  __shared__ float tile[32][33];
  const int n = blockIdx.z;
  const int p0 = blockIdx.x * 32;  // pixel tile over the cropped H*W
  const int c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  const int HW = H * W;
  for (int j = ty; j < 32; j += 8) {
    const int c = c0 + j, px = p0 + tx;
    float v = 0.f;
    if (c < C && px < HW) {
      const int h = px / W, w = px - h * W;
      v = src[(((int64_t)n * C + c) * Hs + (int64_t)h * step) * Ws + (int64_t)w * step];
    }
    tile[j][tx] = v;
  }
  __syncthreads();
  for (int j = ty; j < 32; j += 8) {
    const int px = p0 + j, c = c0 + tx;
    if (c < C && px < HW) dst[((int64_t)n * HW + px) * C + c] = tile[tx][j];
  }
}


// Adjoint of the crop + transpose above (training: the gradient of the channels-last rows w.r.t. the NCHW map the producer holds):
// dst[n][c][h][w] = src[n][h * W + w][c] for h < H, w < W, written for the WHOLE [Hd, Wd] plane of dst (zero outside the crop when
// Hd > H or Wd > W).  32 x 32 tiles through LDS: 128-byte reads along c, 128-byte writes along the destination pixels.
__global__ __launch_bounds__(256) void nhwc_to_nchw_kernel(const float *__restrict__ src, float *__restrict__ dst,
                                                           int C, int H, int W, int Hd, int Wd) {
  __shared__ float tile[32][33];
  const int n = blockIdx.z;
  const int p0 = blockIdx.x * 32;                          // destination pixel tile over Hd * Wd
  const int c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  const int HWd = Hd * Wd;
  for (int j = ty; j < 32; j += 8) {                       // pixel p0 + j, channel c0 + tx
    const int pd = p0 + j, c = c0 + tx;
    float v = 0.f;
    if (pd < HWd && c < C) {
      const int h = pd / Wd, w = pd - h * Wd;
      if (h < H && w < W) v = src[((int64_t)n * H * W + (int64_t)h * W + w) * C + c];
    }
    tile[j][tx] = v;
  }
  __syncthreads();
  for (int j = ty; j < 32; j += 8) {                       // channel c0 + j, pixel p0 + tx
    const int c = c0 + j, pd = p0 + tx;
    if (c < C && pd < HWd) dst[((int64_t)n * C + c) * HWd + pd] = tile[tx][j];
  }
}

// Trilinear x2 upsample of a channels-last volume fused with the occupancy head:
//   up[v', :] = F.interpolate(vol, scale_factor=2, mode='trilinear', align_corners=False)   (AdaptiveSparseHead.py:64-69)
//   occ[v']   = sigmoid(dot(up[v', :], w) + b)                                               (:71, Sequential(Linear(C,1), Sigmoid))
// One group of C/4 lanes per OUTPUT voxel (a full wave at C = 256): up to 8 input rows are read as
// float4 lanes (L2-resident, the input is 1/8 of the output), the row is written once, and the dot
// product is reduced over the group with wave shuffles.  Source index / weights as torch's
// upsample_trilinear3d: t = max(0.5*(dst+0.5)-0.5, 0), i0 = floor(t), i1 = i0 + (i0 < n-1), l1 = t - i0.
__global__ __launch_bounds__(256) void upsample2x_occ_kernel(const float *__restrict__ vol, const float *__restrict__ w,
                                                             const float *__restrict__ b, float *__restrict__ up,
                                                             float *__restrict__ occ, int ix, int iy, int iz, int C, int G) {
  const int C4 = C >> 2;
  const int ox = 2 * ix, oy = 2 * iy, oz = 2 * iz;
  const int64_t nvox = (int64_t)ox * oy * oz;
  const int gpb = blockDim.x / G;                       // voxel groups per block
  const int g = threadIdx.x / G, l = threadIdx.x % G;
  for (int64_t v = (int64_t)blockIdx.x * gpb + g; v < nvox; v += (int64_t)gridDim.x * gpb) {
    const int z = (int)(v % oz), y = (int)((v / oz) % oy), x = (int)(v / ((int64_t)oz * oy));
    int i0[3], i1[3];
    float l0[3], l1[3];
    const int dst[3] = {x, y, z}, n[3] = {ix, iy, iz};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      float t = 0.5f * ((float)dst[a] + 0.5f) - 0.5f;
      t = t < 0.f ? 0.f : t;
      i0[a] = (int)t;
      i1[a] = i0[a] + (i0[a] < n[a] - 1 ? 1 : 0);
      l1[a] = t - (float)i0[a];
      l0[a] = 1.f - l1[a];
    }
    float dot = 0.f;
    for (int c4 = l; c4 < C4; c4 += G) {
      auto row = [&](int a, int bq, int c) {
        return reinterpret_cast<const float4 *>(vol + (((int64_t)a * iy + bq) * iz + c) * C)[c4];
      };
      const float4 v000 = row(i0[0], i0[1], i0[2]), v001 = row(i0[0], i0[1], i1[2]);
      const float4 v010 = row(i0[0], i1[1], i0[2]), v011 = row(i0[0], i1[1], i1[2]);
      const float4 v100 = row(i1[0], i0[1], i0[2]), v101 = row(i1[0], i0[1], i1[2]);
      const float4 v110 = row(i1[0], i1[1], i0[2]), v111 = row(i1[0], i1[1], i1[2]);
      float4 r;
#define SGC_TRI(f)                                                                                     \
  r.f = l0[0] * (l0[1] * (l0[2] * v000.f + l1[2] * v001.f) + l1[1] * (l0[2] * v010.f + l1[2] * v011.f)) + \
        l1[0] * (l0[1] * (l0[2] * v100.f + l1[2] * v101.f) + l1[1] * (l0[2] * v110.f + l1[2] * v111.f));
      SGC_TRI(x) SGC_TRI(y) SGC_TRI(z) SGC_TRI(w)
#undef SGC_TRI
      reinterpret_cast<float4 *>(up + v * C)[c4] = r;
      if (w) {
        const float4 ww = reinterpret_cast<const float4 *>(w)[c4];
        dot += r.x * ww.x + r.y * ww.y + r.z * ww.z + r.w * ww.w;
      }
    }
    if (w) {
      for (int o = 1; o < G; o <<= 1) dot += __shfl_xor(dot, o);
      if (l == 0) occ[v] = 1.f / (1.f + expf(-(dot + b[0])));
    }
  }
}

// vol[idx[i], :] += rows[i, :]  (volume = upsampled + DenseHead(selected voxels), AdaptiveSparseHead.py:77-82:
// the dense head's output is zero outside the selected voxels, so the full-volume add is a row scatter-add)
__global__ void scatter_add_rows_kernel(const float *__restrict__ rows, const int64_t *__restrict__ idx,
                                        float *__restrict__ vol, int n, int C4) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < (int64_t)n * C4;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int i = (int)(t / C4), c = (int)(t - (int64_t)i * C4);
    float4 *dst = reinterpret_cast<float4 *>(vol + idx[i] * (int64_t)C4 * 4) + c;
    const float4 a = reinterpret_cast<const float4 *>(rows + (int64_t)i * C4 * 4)[c];
    float4 d = *dst;
    d.x += a.x; d.y += a.y; d.z += a.z; d.w += a.w;
    *dst = d;
  }
}

}  // namespace sgc

using namespace sgc;

extern "C" int sgc_scatter_rows(const float *rows, const int32_t *idx, const int32_t *idx2_or_null,
                                float *vol, const int32_t *n_dev_or_null, int n, int C, sgc_stream_t stream) {
  if (!rows || !idx || !vol) return set_error(SGC_EINVAL, "sgc_scatter_rows: null pointer");
  if (n <= 0) return SGC_OK;
  const int vec = (C % 4 == 0 && !((uintptr_t)rows & 15) && !((uintptr_t)vol & 15)) ? 4 : 1;
  hipLaunchKernelGGL(scatter_rows_kernel, dim3(grid_for((int64_t)n * (C / vec), 256)), dim3(256), 0,
                     (hipStream_t)stream, rows, idx, idx2_or_null, vol, n, C, vec, n_dev_or_null);
  return check_launch("scatter_rows_kernel");
}

namespace sgc {
// The same through a 64 x 64 tile with 16-byte accesses on both sides (C % 64 == 0, W, Ws % 4 == 0, 16-byte aligned
// pointers: the feature maps): a float4 covers 4 pixels of one row on the way in and 4 channels of one pixel on the
// way out; tile[c][px] with a 65-float pitch keeps both LDS phases conflict-free.
__global__ __launch_bounds__(256) void nchw_to_nhwc_kernel64(const float *__restrict__ src, float *__restrict__ dst,
                                                             int C, int Hs, int Ws, int H, int W) {
  __shared__ float tile[64][65];
  const int n = blockIdx.z, p0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
  const int HW = H * W;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int e = threadIdx.x + 256 * i;
    const int c = e >> 4, q = e & 15;
    const int px = p0 + q * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (px < HW) {                                   // HW % 4 == 0: a group is in or out as a whole
      const int h = px / W, w = px - h * W;
      v = *reinterpret_cast<const float4 *>(src + (((int64_t)n * C + c0 + c) * Hs + h) * Ws + w);
    }
    tile[c][q * 4] = v.x; tile[c][q * 4 + 1] = v.y; tile[c][q * 4 + 2] = v.z; tile[c][q * 4 + 3] = v.w;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int e = threadIdx.x + 256 * i;
    const int px = e >> 4, g = e & 15;
    if (p0 + px < HW)
      *reinterpret_cast<float4 *>(dst + ((int64_t)n * HW + p0 + px) * C + c0 + g * 4) =
          make_float4(tile[g * 4][px], tile[g * 4 + 1][px], tile[g * 4 + 2][px], tile[g * 4 + 3][px]);
  }
}
}  // namespace sgc

extern "C" int sgc_nchw_to_nhwc_crop(const float *src, float *dst, int N, int C, int Hs, int Ws,
                                     int H, int W, int step, sgc_stream_t stream) {
  if (!src || !dst) return set_error(SGC_EINVAL, "sgc_nchw_to_nhwc_crop: null pointer");
  if (step < 1 || (int64_t)(H - 1) * step >= Hs || (int64_t)(W - 1) * step >= Ws || N <= 0 || C <= 0 || H <= 0 || W <= 0)
    return set_error(SGC_EINVAL, "sgc_nchw_to_nhwc_crop: bad sizes");
  if (N > 65535) return set_error(SGC_EUNSUP, "sgc_nchw_to_nhwc_crop: N > 65535");
  if (step == 1 && C % 64 == 0 && W % 4 == 0 && Ws % 4 == 0 && !(((uintptr_t)src | (uintptr_t)dst) & 15)) {
    hipLaunchKernelGGL(nchw_to_nhwc_kernel64, dim3(ceil_div(H * W, 64), C / 64, N), dim3(256), 0, (hipStream_t)stream, src,
                       dst, C, Hs, Ws, H, W);
    return check_launch("nchw_to_nhwc_kernel64");
  }
  hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3(ceil_div(H * W, 32), ceil_div(C, 32), N), dim3(256), 0,
                     (hipStream_t)stream, src, dst, C, Hs, Ws, H, W, step);
  return check_launch("nchw_to_nhwc_kernel");
}

extern "C" int sgc_nhwc_to_nchw_pad(const float *src, float *dst, int N, int C, int H, int W, int Hd, int Wd, sgc_stream_t stream) {
  if (!src || !dst) return set_error(SGC_EINVAL, "sgc_nhwc_to_nchw_pad: null pointer");
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || Hd < H || Wd < W) return set_error(SGC_EINVAL, "sgc_nhwc_to_nchw_pad: bad sizes");
  if (N > 65535) return set_error(SGC_EUNSUP, "sgc_nhwc_to_nchw_pad: N > 65535");
  hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3(ceil_div(Hd * Wd, 32), ceil_div(C, 32), N), dim3(256), 0, (hipStream_t)stream, src, dst,
                     C, H, W, Hd, Wd);
  return check_launch("nhwc_to_nchw_kernel");
}

extern "C" int sgc_upsample2x_occ(const float *vol, const float *w_or_null, const float *b_or_null, float *up,
                                  float *occ_or_null, int ix, int iy, int iz, int C, sgc_stream_t stream) {
  if (!vol || !up) return set_error(SGC_EINVAL, "sgc_upsample2x_occ: null pointer");
  if ((w_or_null != nullptr) != (occ_or_null != nullptr) || (w_or_null && !b_or_null))
    return set_error(SGC_EINVAL, "sgc_upsample2x_occ: w, b and occ go together");
  if (C % 4 || ix <= 0 || iy <= 0 || iz <= 0 || (((uintptr_t)vol | (uintptr_t)up | (uintptr_t)w_or_null) & 15))
    return set_error(SGC_EUNSUP, "sgc_upsample2x_occ: C %% 4 == 0 and 16-byte aligned pointers required");
  int G = 1;
  while (G < 64 && G < C / 4) G <<= 1;      // lanes per output voxel (power of two <= 64)
  const int64_t nvox = (int64_t)8 * ix * iy * iz;
  hipLaunchKernelGGL(upsample2x_occ_kernel, dim3(grid_for(nvox * G, 256)), dim3(256), 0, (hipStream_t)stream, vol,
                     w_or_null, b_or_null, up, occ_or_null, ix, iy, iz, C, G);
  return check_launch("upsample2x_occ_kernel");
}

// Adjoint of the x2 trilinear upsample on NCDHW planes as a gather: one thread per input voxel collects its <= 5 x 5 x 5
// outputs (per axis: 2i-1, 2i, 2i+1, 2i+2, and output 0 for i = 1) with the weights the forward's index rule gives them.  torch's backward
// scatters 8 float atomics per output element (5.2 ms per config-2 training step for the two upsamples of the path).
__device__ __forceinline__ float up2_weight(int o, int n, int i) {     // weight of input i in output o along one axis
  float t = 0.5f * ((float)o + 0.5f) - 0.5f;
  t = t < 0.f ? 0.f : t;
  const int i0 = (int)t;
  const int i1 = i0 + (i0 < n - 1 ? 1 : 0);
  const float l1 = t - (float)i0;
  return (i0 == i ? 1.f - l1 : 0.f) + (i1 == i ? l1 : 0.f);
}

__global__ __launch_bounds__(256) void upsample2x_backward_kernel(const float *__restrict__ go, float *__restrict__ gi, int C,
                                                                  int X, int Y, int Z) {
  const int64_t vin = (int64_t)X * Y * Z, total = vin * C;
  const int OY = 2 * Y, OZ = 2 * Z;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int c = (int)(e / vin);
    const int64_t v = e - (int64_t)c * vin;
    const int z = (int)(v % Z), y = (int)((v / Z) % Y), x = (int)(v / ((int64_t)Z * Y));
    const float *plane = go + (int64_t)c * vin * 8;
    float acc = 0.f;
    // input 1 also takes output 0, with weight exactly 0 (the forward clamps t to 0 there: i0 = 0, i1 = 1, l1 = 0): torch's scatter
    // adds that 0 * go, which is NaN for a non-finite go, and so does this gather
    for (int ox = x == 1 ? 0 : max(2 * x - 1, 0); ox <= min(2 * x + 2, 2 * X - 1); ++ox) {
      const float wx = up2_weight(ox, X, x);
      for (int oy = y == 1 ? 0 : max(2 * y - 1, 0); oy <= min(2 * y + 2, OY - 1); ++oy) {
        const float wxy = wx * up2_weight(oy, Y, y);
        const float *line = plane + ((int64_t)ox * OY + oy) * OZ;
        for (int oz = z == 1 ? 0 : max(2 * z - 1, 0); oz <= min(2 * z + 2, OZ - 1); ++oz) acc += wxy * up2_weight(oz, Z, z) * line[oz];
      }
    }
    gi[e] = acc;
  }
}

extern "C" int sgc_upsample2x_backward(const float *grad_out, float *grad_in, int C, int X, int Y, int Z, sgc_stream_t stream) {
  if (C <= 0 || X <= 0 || Y <= 0 || Z <= 0) return SGC_OK;
  if (!grad_out || !grad_in) return set_error(SGC_EINVAL, "sgc_upsample2x_backward: null pointer");
  const int64_t total = (int64_t)C * X * Y * Z;
  hipLaunchKernelGGL(upsample2x_backward_kernel, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, grad_out,
                     grad_in, C, X, Y, Z);
  return check_launch("upsample2x_backward_kernel");
}

extern "C" int sgc_scatter_add_rows(const float *rows, const int64_t *idx, float *vol, int n, int C, sgc_stream_t stream) {
  if (!rows || !idx || !vol) return set_error(SGC_EINVAL, "sgc_scatter_add_rows: null pointer");
  if (C % 4 || (((uintptr_t)rows | (uintptr_t)vol) & 15)) return set_error(SGC_EUNSUP, "sgc_scatter_add_rows: C %% 4 == 0 required");
  if (n <= 0) return SGC_OK;
  hipLaunchKernelGGL(scatter_add_rows_kernel, dim3(grid_for((int64_t)n * (C / 4), 256)), dim3(256), 0,
                     (hipStream_t)stream, rows, idx, vol, n, C / 4);
  return check_launch("scatter_add_rows_kernel");
}
