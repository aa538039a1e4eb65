// What the matrix pipe sustains under the package power limit: every SIMD issues bf16 MFMAs back to back on a 64 x 64 output
// tile per wave (random bf16 values, or zeros: argv[1] = 0) for a few seconds; prints TFLOP/s per interval.
//   argv: random data? (1) | seconds (4) | waves per SIMD (2) | operand order (0) | shape: 32 = 32x32x16, 16 = 16x16x32 (32) |
//         operands: 0 = register-resident, 1 = every fragment re-read from LDS by ds_read_b128 before each use (0)
// Both shapes cover the same tile with the same operand bytes per FLOP: four 32 x 32 accumulators over 2 + 2 fragments per
// 16-deep k-step, or sixteen 16 x 16 accumulators over 4 + 4 fragments per 32-deep k-step.  The LDS reads are one 16-byte chunk
// per lane at consecutive addresses, so they are conflict-free on either shape: the probe ranks the shapes, not an LDS layout.
// Run it next to `rocm-smi --showclocks --showpower` (tools/jobs/r04_mfma_power.sh).  Build: hipcc --offload-arch=gfx950 -O3
#include <hip/hip_runtime.h>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kFrags = 8;        // fragments per lane in the input buffer (the 32x32x16 loop uses the first four)
constexpr int kLanes = 4096;     // distinct lanes of input data

// ORDER 0: A and B alternate between consecutive MFMAs; 1: the same A and B for every MFMA; 2: A stationary, B alternates
template <int ORDER, bool LDS>
__global__ __launch_bounds__(512) void mfma_loop_32(const bf16x8 *in, float *out, int iters) {
  __shared__ bf16x8 sm[LDS ? 4 * 512 : 1];
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const bf16x8 *src = in + kFrags * (t & (kLanes - 1));
  bf16x8 a0 = src[0], a1 = src[1], b0 = src[2], b1 = src[3];
  if (LDS) {
    for (int k = 0; k < 4; ++k) sm[k * 512 + threadIdx.x] = src[k];
    __syncthreads();
  }
  f32x16 c0 = {}, c1 = {}, c2 = {}, c3 = {};
  for (int i = 0; i < iters; ++i) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (LDS) {
        asm volatile("" ::: "memory");   // the four fragments are read again for every k-step
        a0 = sm[threadIdx.x]; a1 = sm[512 + threadIdx.x]; b0 = sm[1024 + threadIdx.x]; b1 = sm[1536 + threadIdx.x];
      }
      c0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, c0, 0, 0, 0);
      c1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ORDER == 0 ? a1 : a0, b0, c1, 0, 0, 0);
      c2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, ORDER == 1 ? b0 : b1, c2, 0, 0, 0);
      c3 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ORDER == 0 ? a1 : a0, ORDER == 1 ? b0 : b1, c3, 0, 0, 0);
    }
  }
  float s = 0.f;
  for (int k = 0; k < 16; ++k) s += c0[k] + c1[k] + c2[k] + c3[k] + (float)a1[0] + (float)b1[0];
  out[t] = s;
}

template <int ORDER, bool LDS>
__global__ __launch_bounds__(512) void mfma_loop_16(const bf16x8 *in, float *out, int iters) {
  __shared__ bf16x8 sm[LDS ? 8 * 512 : 1];
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const bf16x8 *src = in + kFrags * (t & (kLanes - 1));
  bf16x8 a[4], b[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) { a[k] = src[k]; b[k] = src[4 + k]; }
  if (LDS) {
    for (int k = 0; k < 8; ++k) sm[k * 512 + threadIdx.x] = src[k];
    __syncthreads();
  }
  f32x4 c[4][4] = {};
  for (int i = 0; i < iters; ++i) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {   // one 32-deep k-step of the 64 x 64 tile: the FLOPs of two k-steps of the loop above
      if (LDS) {
        asm volatile("" ::: "memory");
#pragma unroll
        for (int k = 0; k < 4; ++k) { a[k] = sm[k * 512 + threadIdx.x]; b[k] = sm[(4 + k) * 512 + threadIdx.x]; }
      }
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n)
          c[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ORDER == 0 ? a[m] : a[0], ORDER == 1 ? b[0] : b[n], c[m][n], 0, 0, 0);
    }
  }
  float s = 0.f;
  for (int m = 0; m < 4; ++m)
    for (int n = 0; n < 4; ++n)
      for (int k = 0; k < 4; ++k) s += c[m][n][k] + (float)a[m][0] + (float)b[n][0];
  out[t] = s;
}

template <int ORDER, bool LDS>
static void launch(int shape, int blocks, int threads, const bf16x8 *din, float *dout, int iters) {
  if (shape == 16) hipLaunchKernelGGL((mfma_loop_16<ORDER, LDS>), dim3(blocks), dim3(threads), 0, 0, din, dout, iters);
  else hipLaunchKernelGGL((mfma_loop_32<ORDER, LDS>), dim3(blocks), dim3(threads), 0, 0, din, dout, iters);
}

int main(int argc, char **argv) {
  const int random_data = argc > 1 ? atoi(argv[1]) : 1;
  const float seconds = argc > 2 ? atof(argv[2]) : 4.f;
  const int waves_per_simd = argc > 3 ? atoi(argv[3]) : 2;
  const int order = argc > 4 ? atoi(argv[4]) : 0;
  const int shape = argc > 5 ? atoi(argv[5]) : 32;   // "32x32x16" and "16x16x32" parse to 32 and 16
  const int lds = argc > 6 ? atoi(argv[6]) : 0;
  if ((shape != 32 && shape != 16) || waves_per_simd < 1 || waves_per_simd > 2 || order < 0 || order > 2) {
    fprintf(stderr, "usage: mfma_power [random 0|1] [seconds] [waves per SIMD 1|2] [order 0|1|2] [shape 32x32x16|16x16x32] [lds 0|1]\n");
    return 2;
  }
  const int threads = 256 * waves_per_simd, blocks = 256, iters = 4096;
  std::vector<unsigned short> h((size_t)kLanes * kFrags * 8);
  srand(1);
  for (auto &v : h) {
    float f = random_data ? ((rand() % 2001) - 1000) * 1e-3f : 0.f;
    unsigned u; std::memcpy(&u, &f, 4);
    v = (unsigned short)(u >> 16);
  }
  bf16x8 *din; float *dout;
  if (hipMalloc(&din, h.size() * 2) != hipSuccess || hipMalloc(&dout, (size_t)blocks * threads * 4) != hipSuccess) return 1;
  if (hipMemcpy(din, h.data(), h.size() * 2, hipMemcpyHostToDevice) != hipSuccess) return 1;
  // either loop: 2 * 64 * 64 * 128 FLOP per wave and iteration (32 MFMAs of 32x32x16, or 64 of 16x16x32)
  const double flop = (double)blocks * (threads / 64) * iters * 2.0 * 64 * 64 * 128;
  printf("shape %s, operands from %s, %s data, %d waves per SIMD, order %d\n", shape == 16 ? "16x16x32" : "32x32x16",
         lds ? "LDS" : "registers", random_data ? "random" : "zero", waves_per_simd, order);
  auto t0 = std::chrono::steady_clock::now();
  for (;;) {
    auto a = std::chrono::steady_clock::now();
    for (int r = 0; r < 8; ++r) {
      if (lds) {
        if (order == 0) launch<0, true>(shape, blocks, threads, din, dout, iters);
        else if (order == 1) launch<1, true>(shape, blocks, threads, din, dout, iters);
        else launch<2, true>(shape, blocks, threads, din, dout, iters);
      } else {
        if (order == 0) launch<0, false>(shape, blocks, threads, din, dout, iters);
        else if (order == 1) launch<1, false>(shape, blocks, threads, din, dout, iters);
        else launch<2, false>(shape, blocks, threads, din, dout, iters);
      }
    }
    if (hipDeviceSynchronize() != hipSuccess) { fprintf(stderr, "kernel failed\n"); return 1; }
    auto b = std::chrono::steady_clock::now();
    const double dt = std::chrono::duration<double>(b - a).count();
    printf("%.2f s: %.1f TFLOP/s\n", std::chrono::duration<double>(b - t0).count(), 8 * flop / dt / 1e12);
    fflush(stdout);
    if (std::chrono::duration<double>(b - t0).count() > seconds) break;
  }
  return 0;
}
