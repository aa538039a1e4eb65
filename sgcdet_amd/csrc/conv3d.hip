// The convolution entry points of the library (sgc_conv3d_*, sgc_conv2d_*, sgc_linear_rows_*) and the ONE place that decides how
// a call runs: plan_conv picks the kernel family, the brick, the column tile and the reduction split, the launch and the workspace
// query both read its answer.  The kernels live with their launchers: conv3d_igemm.hip (tile-per-workgroup implicit GEMM, fp32 and
// bf16x3), conv3d_halo.hip (halo-resident 3x3x3 / 3x3 form), rows_gemm.hip (1x1x1 layers and Linears), conv3d_wgrad.hip (weight
// gradients).  Here: the geometry, the plan, the split-K plumbing (zero fill, epilogue kernel) and the Winograd-z output transform.
#include "conv_common.hpp"
#include "tuning.hpp"
#include "../../include/sgcdet_amd_scene_batch.h"

namespace sgc {
int g_conv_products = 3;     // NOT a tuning knob (it changes results; sgc_set_conv_products): the NP of csrc/mma.hpp -- 3 = fp32-faithful
                             // 3-way bf16 split (a_lo*b_hi + a_hi*b_lo + a_hi*b_hi), 1 = plain bf16 (a_hi*b_hi only: operands rounded
                             // to bf16, fp32 accumulate), 2 = plain fp16 (operands rounded to IEEE half): the opt-in reduced-precision
                             // modes of BASELINE.json configs #2 / #5

// Why the plan's knobs (tuning.hpp) stand where they do:
//   halo_brick    round 3, interleaved A/B of the three shapes on the 40x40x16 and 80x80x32 layers (bit-identical results): 8x8x4 is
//                 1.5 - 2.5 % faster than 4x4x16 (236 vs 241 us, 129.5 vs 133, 534 vs 546; 600 halo rows instead of 648) -> it is
//                 the choice wherever it tiles the grid exactly
//   wz_brick      Winograd-z stack, alternated with four scenes in flight (bit-identical results): 2 images x 10 x 10 on the three
//                 20x20x8 layers 526.8 against 515.8 scenes/s for 4 x 8 x 8, +7 .. +11 in three jobs (profiles/r15_wz_bricks.md)
//                 -> the brick with fewer matrix rows, 4 x 8 x 8 on a tie
//   wz_mfma       Winograd-z bricks on v_mfma_f32_16x16x32 (16) or 32x32x16 (32): the chip holds a higher clock on the 16x16x32 shape
//                 under load (bare loops on random data, 2 waves per SIMD: 2 107 against 1 906 TFLOP/s from registers, 1 755 against
//                 1 630 re-read from LDS).  Alone 176 against 181 us on the 90-GF layer, 141 against 151 on 512 -> 512 @ 20x20x8; with
//                 four scenes in flight, parent / 32 / 16 alternated: 541.9 / 545.9 / 551.8, 516.1 / 517.1 / 537.6 and 527.8 / 527.3 /
//                 542.2 scenes/s in three jobs (profiles/r21_wz_mfma_shape.md) -> 16 on every Winograd layer
//   split_target  interleaved A/B, tools/split_ab.py: 128 / 256 are 20-30 % slower on the stride-2 and 400-voxel layers, 1024+ no better
//   halo_narrow   1 = 64-column tiles for layers with <= 64 output channels and 32-column tiles (8 x 1 waves) for <= 32; 64 = never
//                 below 64 columns (the round-2..4 form, A/B); 0 = always 128
//   halo_min_cout the head's 28-channel convolutions run 105 -> 67 us on the halo kernel although 3/4 of the tile columns are padding
//   halo_wave_fix 1: latency geometry only -- one more split when the workgroups of a launch overflow the CUs by a small remainder
//                 (cfg3: 288 workgroups on 256 CUs took two full rounds); 2: in the throughput geometry too (A/B)

// Zero-fill of a split-K accumulation target as a KERNEL, not hipMemsetAsync: a memset captured into a large
// hipGraph (the whole-scene graph) is not ordered with the kernel nodes around it on ROCm 7.2 -- from the second
// replay on the accumulators started from whatever earlier nodes had left in the recycled pool memory
// (tools/scene_graph_check2.py); a kernel node is.
__global__ __launch_bounds__(256) void zero_fill_kernel(float4 *__restrict__ p, int64_t n4) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x)
    p[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}
static int zero_fill(float *y, int64_t n, hipStream_t st) {      // n floats, n % 4 == 0, y 16-byte aligned
  const int64_t n4 = n / 4;
  const int g = (int)((n4 + 255) / 256 < 2048 ? (n4 + 255) / 256 : 2048);
  hipLaunchKernelGGL(zero_fill_kernel, dim3(g > 0 ? g : 1), dim3(256), 0, st, reinterpret_cast<float4 *>(y), n4);
  return check_launch("zero_fill_kernel");
}

// (An XCD-aware tile order for the implicit-GEMM kernel -- 1-D launch decoded so that the n-blocks of an m tile, or the
//  m-blocks sharing a weight tile, run back to back on ONE XCD and its L2 serves the repeats -- was measured on the
//  Linears and on the 400-voxel 1024-channel layers: no change (162 vs 165 us, 140 vs 141 us).  The repeats are
//  served by the memory-side cache either way; the limiter is the load -> LDS -> MFMA latency chain, section 4.5.
//  A BK = 64 single-LDS-buffer form of the same kernel -- twice the bytes per thread in flight at the same LDS
//  footprint and occupancy, two barriers per step, half the steps -- was built and is correct but slower where it
//  matters: 203 vs 164 us on the 188,800-row Linear, 168 vs 140 us on the 400-voxel 1024-channel layer; it only wins
//  on the 6,400-row Linears (16 vs 20 us).  The exposed regs -> LDS phase between its two barriers costs more than
//  the deeper loads hide.)
// brick of the halo kernel for a grid: 0 = 4x4x16, 1 = 4x8x8, 2 = 8x8x4
static int halo_brick_shape(int gx, int gy, int gz) {
  if (g_tune_halo_brick == 2) return 2;
  if (g_tune_halo_brick == 0 && gz >= 16 && gx % 8 == 0 && gy % 8 == 0 && gz % 4 == 0) return 2;
  if (gz >= 16 && (g_tune_halo_brick == 0 || g_tune_halo_brick == 3)) return 0;
  if (gz >= 8) return 1;
  return 2;
}

// Whole-grid bricks for the coarsest scale of configs 2 / 3 (10 x 10 x 4 = 400 and 12 x 12 x 4 = 2 x 288 voxels; too few for 256-voxel
// bricks: 61 % of their rows would be padding, and on the tile kernel these weight-streaming layers -- 113 MB of weights for
// 400 voxels -- run at a quarter of the MFMA rate): 1 = one 10 x 10 x 4 brick, 2 = two 6 x 12 x 4 bricks, 0 = none.
// 64-column tiles (the 512 / 384 MFMA rows of such a brick leave the accumulators room for no more).
static int halo_small_grid(int gx, int gy, int gz, int Cout) {
  // measured (tools/small_grid_ab.py, alternated): 1024 -> 1024 109 -> 88 us at 10x10x4, 137 -> 119 at 12x12x4; with 128 output
  // channels (two column tiles x 32 splits) the tile kernel stays ahead (39 vs 47 / 40 us)
  if (!g_tune_halo_small || Cout < 512) return 0;
  if (gx == 10 && gy == 10 && gz == 4) return 1;
  if (gx == 12 && gy == 12 && gz == 4) return 2;
  return 0;
}

// channel-chunk splits of the halo kernel: enough workgroups for 3/4 of the CUs, and no empty split
static int halo_splitk(int bricks, int nb, int nchunks) {
  int splitk = 1;
  while (splitk < nchunks && (int64_t)bricks * nb * splitk < g_tune_halo_split_target) splitk *= 2;
  // Wave quantisation (round 5).  One workgroup per CU: W workgroups take ceil(W / CUs) rounds of (fixed + slices * per_slice).  When a
  // launch overflows the CUs by a small remainder -- 144 bricks x 2 column tiles = 288 workgroups on 256 CUs, BASELINE config 3's
  // 256 -> 256 layers at 48 x 48 x 16: two full rounds, 0.36 of the MFMA peak against 0.47 for config 2's 200 workgroups -- halving the
  // slices per workgroup (576 workgroups, three rounds of half the length) is faster alone although it adds a reduce pass.  Only in
  // the LATENCY geometry (halo_split_target >= 192): with scenes in flight the other streams fill the idle CUs of the second round and
  // what counts is CU-time, which a split only raises.  Cost model: 13.6 us fixed + 24.2 us per slice
  // (profiles/r04_halo_fixed_cost.txt), + 20 us for the workspace round trip of a split.
  if (g_tune_halo_wave_fix && (g_tune_halo_split_target >= 192 || g_tune_halo_wave_fix == 2) && splitk == 1 && nchunks >= 2) {
    const int cus = device_cus();                 // queried (a partitioned device or another SKU has another count)
    const int64_t w1 = (int64_t)bricks * nb, w2 = 2 * w1;
    const double t1 = (double)((w1 + cus - 1) / cus) * (13.6 + 24.2 * nchunks);
    const double t2 = (double)((w2 + cus - 1) / cus) * (13.6 + 24.2 * ((nchunks + 1) / 2)) + 20.0;
    if (t2 < 0.92 * t1) splitk = 2;
  }
  const int per = (nchunks + splitk - 1) / splitk;
  return (nchunks + per - 1) / per;
}

__global__ void conv_epilogue_kernel(float *__restrict__ y, const float *__restrict__ scale,
                                     const float *__restrict__ shift, const float *__restrict__ residual,
                                     int64_t total4, int C4, int relu, const float *__restrict__ ws, int splits,
                                     const float *__restrict__ act_scale, int act_c0, int act_c1) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C4);
    float4 v;
    if (ws) {                      // partial tiles of the splits, summed in split order: same bits every run
      v = reinterpret_cast<const float4 *>(ws)[i];
      for (int sidx = 1; sidx < splits; ++sidx) {
        const float4 t = reinterpret_cast<const float4 *>(ws)[(int64_t)sidx * total4 + i];
        v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w;
      }
    } else {
      v = reinterpret_cast<float4 *>(y)[i];
    }
    const float4 sc = scale ? reinterpret_cast<const float4 *>(scale)[c] : make_float4(1.f, 1.f, 1.f, 1.f);
    const float4 sh = shift ? reinterpret_cast<const float4 *>(shift)[c] : make_float4(0.f, 0.f, 0.f, 0.f);
    v.x = v.x * sc.x + sh.x; v.y = v.y * sc.y + sh.y; v.z = v.z * sc.z + sh.z; v.w = v.w * sc.w + sh.w;
    if (relu == 2) v = relu_nan(v);
    if (residual) {
      const float4 r = reinterpret_cast<const float4 *>(residual)[i];
      v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
    }
    if (relu == 1) v = relu_nan(v);
    if (act_scale) v = act_col4(v, c * 4, act_c0, act_c1, *act_scale);
    reinterpret_cast<float4 *>(y)[i] = v;
  }
}

// ---------------------------------------------------------------------------------------------
// Winograd F(2,3) along z for the 3x3x3 stride-1 layers (round 5).  With four scenes in flight the package sits at its power
// limit and the bf16 x 3 products of these layers are about half of a scene's joules: the only lever left on them
// is fewer multiply-adds.  Per (dx, dy) the z direction is a 1-D 3-tap convolution; for an output pair (z = 2j, 2j + 1) with the
// inputs d_k = x[.., 2j - 1 + k], k = 0..3 (zero outside the grid):
//     t0 = d0 - d2,  t1 = d1 + d2,  t2 = d2 - d1,  t3 = d1 - d3                    (input transform)
//     G0 = w0,  G1 = (w0 + w1 + w2) / 2,  G2 = (w0 - w1 + w2) / 2,  G3 = w2        (weight transform, once per module)
//     m_k = sum over (dx, dy, ci) of t_k G_k                                        (four 3 x 3 convolutions over (x, y))
//     y[2j] = m0 + m1 + m2,   y[2j + 1] = m1 - m2 - m3                              (output transform)
// 18 instead of 27 tap-GEMMs per output.  Two launches: the halo kernel's 2-D form convolves a VIRTUAL stack of 4 * Z/2 "images" of
// X x Y pixels (position-major; bricks of 4 images x 8 x 8 pixels, no halo along the image axis) with one weight set per position --
// the input transform is applied while the halo rows are staged (template flag WZ: two voxel rows per chunk, one add, then the
// hi / lo split; a transformed copy of the input never exists) -- and the output transform combines the four results and applies
// the epilogue (scale / shift / relu / residual -- the direct kernel's expressions in the direct kernel's order).
// The fused form does not fit: four accumulators per output pair and four weight tiles per tap need 164 - 189 KB of LDS.
// (The output transform in the TAIL of the convolution launch -- tiles to the scratch with sc1 stores, an arrival counter per brick, the
//  last of a brick's four position workgroups reads the four tiles back behind an agent-scope acquire and stores the output -- was
//  built, bit-identical, and measured: the convolution launch grows from 200-209 to 230-237 us, more than the 12.5 us launch it
//  removes; 557-560 against 563-572 scenes/s with four scenes in flight, 384-388 against 395-400 with one
//  (profiles/r05_wzfuse_ab.txt, also with the four positions adjacent on one XCD).  One CU moves the 1.25 MB of a brick's tiles,
//  residual and output at 50-100 GB/s; 256 CUs in a separate launch do it at the chip's rate.)
// Entries 0, +-1, +-1/2: every transform is exact up to one fp32 rounding per element; measured error against the direct form
// in tests/test_gpu_conv3d.py.  Deterministic (no atomics, fixed order).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void winograd_z_out_kernel(const float4 *__restrict__ m, float4 *__restrict__ y,
                                                             const float *__restrict__ scale, const float *__restrict__ shift,
                                                             const float4 *__restrict__ residual, int X, int Y, int Z, int C4, int relu,
                                                             const float *__restrict__ act_scale, int act_c0, int act_c1) {
  const int J = Z >> 1;
  const int64_t total = (int64_t)X * Y * J * C4, plane = (int64_t)X * Y * C4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C4);
    int64_t r = i / C4;
    const int j = (int)(r % J); r /= J;
    const int yy = (int)(r % Y), xx = (int)(r / Y);
    const float4 *mi = m + ((int64_t)j * X + xx) * Y * C4 + (int64_t)yy * C4 + c;
    const float4 m0 = mi[0], m1 = mi[(int64_t)J * plane], m2 = mi[(int64_t)2 * J * plane], m3 = mi[(int64_t)3 * J * plane];
    float4 v[2] = {make_float4((m0.x + m1.x) + m2.x, (m0.y + m1.y) + m2.y, (m0.z + m1.z) + m2.z, (m0.w + m1.w) + m2.w),
                   make_float4((m1.x - m2.x) - m3.x, (m1.y - m2.y) - m3.y, (m1.z - m2.z) - m3.z, (m1.w - m2.w) - m3.w)};
    const float4 sc = scale ? reinterpret_cast<const float4 *>(scale)[c] : make_float4(1.f, 1.f, 1.f, 1.f);
    const float4 sh = shift ? reinterpret_cast<const float4 *>(shift)[c] : make_float4(0.f, 0.f, 0.f, 0.f);
    const int64_t o0 = (((int64_t)xx * Y + yy) * Z + 2 * j) * C4 + c;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      float4 w = v[q];
      w.x = w.x * sc.x + sh.x; w.y = w.y * sc.y + sh.y; w.z = w.z * sc.z + sh.z; w.w = w.w * sc.w + sh.w;
      if (relu == 2) w = relu_nan(w);
      if (residual) {
        const float4 rr = residual[o0 + (int64_t)q * C4];
        w.x += rr.x; w.y += rr.y; w.z += rr.z; w.w += rr.w;
      }
      if (relu == 1) w = relu_nan(w);
      if (act_scale) w = act_col4(w, c * 4, act_c0, act_c1, *act_scale);
      y[o0 + (int64_t)q * C4] = w;
    }
  }
}

}  // namespace sgc

using namespace sgc;

// grids and taps of a call: ix, iy, iz in; the output grid and the GEMM-row grid (conv: the output grid; transposed: the input grid) out
static void conv_geometry(ConvParams &p, int ix, int iy, int iz, int Cin, int Cout, int ksize, int stride, int transposed,
                          int &ox, int &oy, int &oz) {
  p.Cin = Cin; p.Cout = Cout; p.ix = ix; p.iy = iy; p.iz = iz; p.transposed = transposed;
  if (p.scenes < 1) p.scenes = 1;
  if (transposed) {
    p.gx = ix; p.gy = iy; p.gz = iz; p.ksize = 1; p.stride = 1; p.pad = 0; p.taps = 1;
    ox = 2 * ix; oy = 2 * iy; oz = 2 * iz;
  } else {
    p.pad = ksize == 2 ? 0 : ksize / 2; p.ksize = ksize; p.stride = stride; p.taps = ksize * ksize * ksize;   // k2s2: no padding (the
                                                                                                       // dgrad of ConvTranspose3d k2s2)
    ox = (ix + 2 * p.pad - ksize) / stride + 1; oy = (iy + 2 * p.pad - ksize) / stride + 1;
    oz = (iz + 2 * p.pad - ksize) / stride + 1;
    p.gx = ox; p.gy = oy; p.gz = oz;
  }
  if (p.two_d) {                               // images are independent: no taps, no padding, no stride along x
    p.taps = ksize * ksize;
    ox = ix; p.gx = ox;
  }
  p.M = p.gx * p.gy * p.gz;
}

static int conv_setup(ConvParams &p, const char *who, const float *x, const void *w1, const void *w2, float *y,
                      int ix, int iy, int iz, int Cin, int Cout, int ksize, int stride, int transposed, int relu,
                      int &ox, int &oy, int &oz) {
  if (!x || !w1 || !w2 || !y) return set_error(SGC_EINVAL, "%s: null pointer", who);
  if (Cin <= 0 || Cout <= 0 || ix <= 0 || iy <= 0 || iz <= 0) return set_error(SGC_EINVAL, "%s: bad size", who);
  if (Cin % BK) return set_error(SGC_EUNSUP, "%s: Cin must be a multiple of %d", who, BK);
  if (((uintptr_t)x | (uintptr_t)w1 | (uintptr_t)w2 | (uintptr_t)y) & 15)
    return set_error(SGC_EINVAL, "%s: pointers must be 16-byte aligned", who);
  if (transposed && (ksize != 2 || stride != 2)) return set_error(SGC_EUNSUP, "%s: transposed supports k=2, s=2", who);
  if (!transposed && !((ksize == 3 || ksize == 1) && (stride == 1 || stride == 2)) && !(ksize == 2 && stride == 2))
    return set_error(SGC_EUNSUP, "%s: ksize in {1,3} with stride in {1,2}, or ksize 2 with stride 2", who);
  if (p.two_d && (transposed || stride != 1)) return set_error(SGC_EUNSUP, "%s: the 2-D form is stride 1, not transposed", who);
  // ksize 2 has no padding: an axis of extent 1 leaves no output ((1 - 2) / 2 + 1 truncates to 1 in C, floors to 0 in the callers)
  if (!transposed && ksize == 2 && (ix < 2 || iy < 2 || iz < 2)) return set_error(SGC_EINVAL, "%s: ksize 2 on an axis of extent 1 has no output", who);
  p.x = x; p.y = y; p.relu = relu;
  conv_geometry(p, ix, iy, iz, Cin, Cout, ksize, stride, transposed, ox, oy, oz);
  return SGC_OK;
}

static int pick_splitk(const ConvParams &p, int mb, int nb, int target_blocks) {
  int splitk = 1;
  if (!p.transposed && p.taps == 27) {
    const int64_t blocks = (int64_t)mb * nb;
    while (splitk < 27 && blocks * splitk < target_blocks) splitk *= 3;
  }
  return splitk;
}

// bf16x3 tile kernel (round 6): splits of whole K STEPS.  Groups of whole taps (above) only allow 3 / 9 / 27 splits and overshoot the
// target (100 tiles -> 300 or 900 workgroups on 256 CUs: some CUs carry twice the work of others); steps let a launch land on
// floor(target / tiles) splits of equal length.  split_free = 0 restores the tap groups (A/B), split_min_steps bounds how short a
// split may get (its prologue + the partial tile it stores are fixed costs), split_max the partial tiles the epilogue kernel re-reads.
static int pick_split_steps(const ConvParams &p, int mb, int nb, int target_blocks, int *steps_per) {
  const int total = (p.transposed ? 1 : p.taps) * (p.Cin / BK);
  *steps_per = total;
  if (p.two_d) return 1;                       // the 2-D entry point carries no workspace
  if (!p.transposed && p.taps == 1) return 1;  // 1x1x1 layers are plain GEMMs: one K order everywhere (sgc_level_tail and the row GEMM are
                                               // tested bit for bit against this kernel); splitting them bought 1 us of 18 alone
  if (!g_tune_split_free) {
    const int k = pick_splitk(p, mb, nb, target_blocks);
    *steps_per = total / k;
    return k;
  }
  const int64_t tiles = (int64_t)mb * nb * (p.transposed ? 8 : 1);
  int64_t want = target_blocks / (tiles > 0 ? tiles : 1);
  if (want > total / g_tune_split_min_steps) want = total / g_tune_split_min_steps;
  if (want > g_tune_split_max) want = g_tune_split_max;
  if (want <= 1) return 1;
  const int per = (total + (int)want - 1) / (int)want;
  *steps_per = per;
  return (total + per - 1) / per;
}

static int conv_finish(const ConvParams &p, int64_t OV, hipStream_t st) {
  if (p.splitk <= 1) return SGC_OK;
  if (p.Cout % 4) return set_error(SGC_EUNSUP, "conv3d: split-K path needs Cout %% 4 == 0");
  const int64_t total4 = OV * p.Cout / 4;
  const int g = (int)((total4 + 255) / 256 < 4096 ? (total4 + 255) / 256 : 4096);
  hipLaunchKernelGGL(conv_epilogue_kernel, dim3(g), dim3(256), 0, st, p.y, p.scale, p.shift, p.residual, total4,
                     p.Cout / 4, p.relu, (const float *)p.ws, p.splitk, p.act_scale, p.act_c0, p.act_c1);
  return check_launch("conv_epilogue_kernel");
}

// The plan of one bf16x3 call (p after conv_geometry; OV output rows of the launch, all scenes; masked: the caller passes an output
// mask).  A scene batch keeps the family, the brick and the column tile of its per-scene grid (p.M, p.gx ..: a layer stays in its
// numerical class whatever the batch); only the split count follows the workgroups of the whole launch.  Pure: the
// knobs and the CU count are its only other inputs.  What the launch may still change is not planning: without a (large enough)
// workspace a split launch accumulates with float atomics, and the 2-D forms, whose entry points carry none, take one split.
static ConvPlan plan_conv(const ConvParams &p, int64_t OV, bool masked) {
  ConvPlan pl = {};
  pl.family = kConvTile; pl.splitk = 1; pl.mfma = 32;
  const bool halo = g_tune_conv_halo && !p.transposed && p.ksize == 3 && p.stride == 1 && p.Cout >= g_tune_halo_min_cout;
  const bool narrow_n = g_tune_halo_narrow && p.Cout <= 64;          // 64-column tiles for layers with <= 64 output channels,
  const bool narrow_32 = g_tune_halo_narrow >= 1 && g_tune_halo_narrow != 64 && p.Cout <= 32;   // 32-column tiles (8 x 1 waves) for the head's 28 columns
  const auto brick = [&pl](ConvFamily f, int bx, int by, int bz, int bn) { pl.family = f; pl.bx = bx; pl.by = by; pl.bz = bz; pl.bn = bn; };
  int small = 0;
  if (!p.transposed && p.ksize == 1 && p.stride == 1 && !p.two_d && rows_gemm_supported(p.Cin, p.Cout, 0, 0, OV / p.scenes, p.Cin)) {
    // 1x1x1 stride-1 layers are row GEMMs (the FFN of a level, TU/encoder.py:311-338): persistent weight-stationary kernel
    // (asked with the rows of ONE scene: the family never depends on the batch)
    pl.family = kConvRowsGemm;
    return pl;
  } else if (halo && !p.two_d && p.M >= g_tune_halo_min_m) {
    // 3x3x3 stride-1 layers with enough voxels: halo-resident kernel (bricks of 256 voxels)
    const int shape = halo_brick_shape(p.gx, p.gy, p.gz), bn = narrow_32 ? 32 : narrow_n ? 64 : 128;
    if (shape == 0) brick(kConvHalo, 4, 4, 16, bn);
    else if (shape == 1) brick(kConvHalo, 4, 8, 8, bn);
    else brick(kConvHalo, 8, 8, 4, bn);
  } else if (halo && !p.two_d && !masked && (small = halo_small_grid(p.gx, p.gy, p.gz, p.Cout)) != 0) {
    if (small == 1) brick(kConvHaloGrid, 10, 10, 4, 64);
    else brick(kConvHaloGrid, 6, 12, 4, 64);
  } else if (halo && g_tune_halo_2d && p.two_d && p.wz_Z > 0 && p.gy >= 8 && p.gz >= 8) {
    // The virtual Winograd stack of sgc_conv3d_winograd_z_bf16x3: 4 positions x J = Z / 2 images of gy x gz pixels, weight set = position.
    // A brick's images belong to ONE position (the kernel derives the position and the transform from its first image), so the brick's
    // image count must divide J: 4 images x 8 x 8 pixels for J % 4 == 0, 2 images x 10 x 10 pixels for J = 2 and J % 4 == 0 (J = 6 would
    // fit the small brick, but no layer has it and nothing was measured there: it stays with the direct kernel).  Of the bricks that
    // fit, the one that issues fewer matrix rows for the grid (both pad to 256 rows; 20 x 20 pixels: 8 bricks of 10 x 10 against 9 of
    // 8 x 8 per two / four images); a tie keeps 4 x 8 x 8, so 40 x 40 and every grid it tiles exactly launch as they always have.
    // A stack of J % 4 == 0 needs halo_min_m rows as before; the J = 2 stacks (10 x 10 x 4: 800 rows) are what the small brick is for.
    const int J = p.wz_Z / 2;
    const bool stack = !narrow_n && p.w_group_images == J && p.gx == 4 * J && p.wz_Z % 4 == 0;
    const bool fit4 = stack && J % 4 == 0 && p.M >= g_tune_halo_min_m, fit2 = stack && (J == 2 || fit4);
    const auto rows = [&p](int bx, int by, int bz) { return (int64_t)ceil_div(p.gx, bx) * ceil_div(p.gy, by) * ceil_div(p.gz, bz) * 256; };
    const bool small = fit2 && (!fit4 || g_tune_wz_brick == 2 || (g_tune_wz_brick == 0 && rows(2, 10, 10) < rows(4, 8, 8)));
    if (small) brick(kConvHaloWZ, 2, 10, 10, 128);
    else if (fit4) brick(kConvHaloWZ, 4, 8, 8, 128);
    pl.mfma = g_tune_wz_mfma == 32 ? 32 : 16;
    if (pl.family == kConvHaloWZ && J % pl.bx != 0) pl.unsupported = "conv: a brick of the virtual Winograd stack must hold images of one position";
    else if (pl.family != kConvHaloWZ) pl.unsupported = "conv: the virtual Winograd stack needs Z / 2 = 2 or a multiple of 4 (and then halo_min_m stack rows) and > 64 output channels";
  } else if (halo && g_tune_halo_2d && p.two_d && p.wz_Z == 0 && p.M >= g_tune_halo_min_m && p.gy >= 8 && p.gz >= 8) {
    // 3 x 3 layers over a stack of images (the FPN's output convolutions): the 2-D form of the halo kernel, bricks of 16 x 16 pixels;
    // or bricks of 4 images x 8 x 8 pixels -- no halo along the image axis, 400 staged rows per 256 outputs: the geometry of the
    // transform-domain convolutions of sgc_conv3d_winograd_z_bf16x3 (image groups = positions: the branch above); halo_2d = 2 selects
    // it for any stack
    if ((g_tune_halo_2d == 2 || p.w_group_images > 0) && !narrow_n && p.gx % 4 == 0 && (p.w_group_images == 0 || p.w_group_images % 4 == 0))
      brick(kConvHalo2D, 4, 8, 8, 128);
    else if (p.w_group_images > 0) pl.unsupported = "conv: grouped 2-D form needs groups of a multiple of 4 images and > 64 output channels";
    else brick(kConvHalo2D, 1, 16, 16, narrow_n ? 64 : 128);
  } else if (p.w_group_images > 0 || p.wz_Z > 0) {
    pl.unsupported = "conv: the grouped 2-D form runs on the halo kernel only (stack too small?)";
  }
  if (pl.unsupported) return pl;
  if (pl.family == kConvTile) {
    pl.bn = p.Cout <= 64 ? 64 : 128;
    pl.splitk = pick_split_steps(p, ceil_div(p.M * p.scenes, BM), ceil_div(p.Cout, pl.bn), g_tune_split_target, &pl.steps_per);
  } else {
    pl.splitk = halo_splitk(p.scenes * ceil_div(p.gx, pl.bx) * ceil_div(p.gy, pl.by) * ceil_div(p.gz, pl.bz), ceil_div(p.Cout, pl.bn), p.Cin / BK);
    // a Winograd stack of halo_min_m rows or more launches unsplit, as it always has (its per-layer A/B lines were taken that way, and
    // with scenes in flight a split only adds CU-time); the few-brick launches of the small stacks split like every halo launch
    if (pl.family == kConvHaloWZ && p.M >= g_tune_halo_min_m) pl.splitk = 1;
  }
  pl.ws_floats = pl.splitk > 1 ? (int64_t)pl.splitk * OV * p.Cout : 0;
  return pl;
}

// where a split launch accumulates: partial tiles in the workspace, summed in split order by conv_finish, or -- without a
// workspace of the plan's size -- float atomics into a zeroed y
static int conv_split_begin(ConvParams &p, int64_t OV, hipStream_t st) {
  if (p.splitk <= 1) return SGC_OK;
  if (p.Cout % 4) return set_error(SGC_EUNSUP, "conv3d: split-K path needs Cout %% 4 == 0");
  if (p.ws && p.ws_floats >= (int64_t)p.splitk * OV * p.Cout) {
    p.ws_stride = OV * p.Cout;
    return SGC_OK;
  }
  p.ws = nullptr;
  return zero_fill(p.y, OV * p.Cout, st);
}

// x [ix*iy*iz, Cin] channels-last; wt [taps][Cout][Cin]; y [ox*oy*oz, Cout].
//   ksize 3 (pad 1) or 1 (pad 0), stride 1 or 2;  transposed = 1: ConvTranspose3d(k=2, s=2), wt [8][Cout][Cin]
//   with parity index (px*2+py)*2+pz.  Cin must be a multiple of 32 (zero-pad the channel dim otherwise).
extern "C" int sgc_conv3d_cl_f32(const float *x, const float *wt, const float *scale, const float *shift,
                                 const float *residual_or_null, float *y,
                                 int ix, int iy, int iz, int Cin, int Cout, int ksize, int stride,
                                 int transposed, int relu, float *workspace_or_null, int64_t workspace_floats,
                                 sgc_stream_t stream) {
  ConvParams p = {};
  int ox, oy, oz;
  int rc = conv_setup(p, "sgc_conv3d_cl_f32", x, wt, wt, y, ix, iy, iz, Cin, Cout, ksize, stride, transposed, relu, ox, oy, oz);
  if (rc) return rc;
  p.w = wt; p.scale = scale; p.shift = shift; p.residual = residual_or_null;
  p.ws = workspace_or_null; p.ws_floats = workspace_or_null ? workspace_floats : 0;
  const int64_t OV = (int64_t)ox * oy * oz;
  const bool narrow = Cout <= 32;
  const int mb = ceil_div(p.M, BM), nb = ceil_div(Cout, narrow ? 32 : 128);
  p.splitk = pick_splitk(p, mb, nb, g_tune_split_target);   // >= 2 workgroups per CU
  hipStream_t st = (hipStream_t)stream;
  rc = conv_split_begin(p, OV, st);
  if (rc) return rc;
  rc = launch_igemm_f32(p, narrow, dim3(mb, nb, (transposed ? 8 : 1) * p.splitk), st);
  if (rc) return rc;
  return conv_finish(p, OV, st);
}

// the tile kernel addresses its input and its weights with 32-bit byte offsets into buffer descriptors
static bool igemm_fits_32bit(const ConvParamsB &p) {
  const int64_t lim = 0xfffffff0ll - 65536;       // input: unsigned byte offsets; weights: the per-step offset is a signed scalar
  return (int64_t)p.scenes * p.ix * p.iy * p.iz * p.Cin * 4 < lim && (int64_t)(p.transposed ? 8 : p.taps) * p.Cout * p.Cin * 2 < 0x7fffffffll;
}

// Same contract with the weights pre-split on the host: w_hi = bf16(w), w_lo = bf16(w - float(w_hi)),
// both [taps][Cout][Cin] bf16 (raw 16-bit patterns).
static int conv3d_bf16x3(const float *x, const uint16_t *w_hi, const uint16_t *w_lo, const float *scale,
                         const float *shift, const float *residual_or_null, float *y,
                         int ix, int iy, int iz, int Cin, int Cout, int ksize, int stride,
                         int transposed, int relu, float *workspace_or_null, int64_t workspace_floats,
                         const uint8_t *out_mask_or_null, sgc_stream_t stream, int two_d = 0,
                         const float *act_scale = nullptr, int act_c0 = 0, int act_c1 = 0, int w_group_images = 0, int wz_Z = 0,
                         int scenes = 1) {
  if (scenes < 1) return set_error(SGC_EINVAL, "sgc_conv3d_cl_bf16x3_batched: scenes must be >= 1");
  // the scene axis exists in the plain 3-D forms only
  if (scenes > 1 && (out_mask_or_null || two_d || act_c1 > act_c0 || w_group_images || wz_Z))
    return set_error(SGC_EUNSUP, "sgc_conv3d_cl_bf16x3_batched: no scene axis in the masked, activation, 2-D and Winograd forms");
  if (scenes > 1 && ((int64_t)scenes * ix * iy * iz * 8 >= (1ll << 31) || scenes >= (1 << 15) || std::max(ix, std::max(iy, iz)) >= (1 << 15)))
    return set_error(SGC_EUNSUP, "sgc_conv3d_cl_bf16x3_batched: too many rows (scenes * 8 * ix*iy*iz < 2^31, scenes and every extent < 2^15)");
  ConvParamsB p = {};
  p.scenes = scenes;
  p.out_mask = out_mask_or_null;
  p.two_d = two_d;
  p.w_group_images = w_group_images;
  p.wz_Z = wz_Z;
  p.act_scale = act_c1 > act_c0 ? act_scale : nullptr; p.act_c0 = act_c0; p.act_c1 = act_c1;
  int ox, oy, oz;
  int rc = conv_setup(p, "sgc_conv3d_cl_bf16x3", x, w_hi, w_lo, y, ix, iy, iz, Cin, Cout, ksize, stride, transposed, relu, ox, oy, oz);
  if (rc) return rc;
  p.w_hi = reinterpret_cast<const __bf16 *>(w_hi); p.w_lo = reinterpret_cast<const __bf16 *>(w_lo);
  p.scale = scale; p.shift = shift; p.residual = residual_or_null;
  p.ws = workspace_or_null; p.ws_floats = workspace_or_null ? workspace_floats : 0;
  if (!igemm_fits_32bit(p)) return set_error(SGC_EUNSUP, "sgc_conv3d_cl_bf16x3: the input must stay below 4 GiB and the weights below 2 GiB");
  const int64_t OV = (int64_t)scenes * ox * oy * oz;         // output rows of the launch
  hipStream_t st = (hipStream_t)stream;
  const ConvPlan pl = plan_conv(p, OV, p.out_mask != nullptr);
  if (pl.unsupported) return set_error(SGC_EUNSUP, "%s", pl.unsupported);
  if (pl.family == kConvRowsGemm && scenes > 1 && !rows_gemm_supported(Cin, Cout, 0, 0, OV, Cin))
    return set_error(SGC_EUNSUP, "sgc_conv3d_cl_bf16x3_batched: the rows of the batch exceed the row GEMM's 4 GiB of x or y");
  if (pl.family == kConvRowsGemm)
    return rows_gemm_launch(x, Cin, w_hi, w_lo, scale, shift, residual_or_null, y, nullptr, (int)OV, Cin, Cout, relu, 0, 0, 0, st);
  p.splitk = pl.splitk; p.steps_per = pl.steps_per;
  // the 2-D entry point carries no workspace: one split rather than float atomics (the result must not depend on the run)
  // (the Winograd entry hands on what its caller gave beyond the transform-domain tensor: as many splits as that holds, none empty)
  if (p.two_d && !(p.ws && p.ws_floats >= pl.ws_floats)) {
    const int nchunks = Cin / BK, fit = p.ws ? (int)std::min<int64_t>(p.ws_floats / std::max<int64_t>(OV * Cout, 1), p.splitk) : 1;
    const int per = ceil_div(nchunks, std::max(fit, 1));
    p.splitk = ceil_div(nchunks, per);
  }
  rc = conv_split_begin(p, OV, st);
  if (rc) return rc;
  if (pl.family == kConvTile) {
    const dim3 grid(ceil_div(p.M * p.scenes, BM), ceil_div(Cout, pl.bn), (transposed ? 8 : 1) * p.splitk);
    const size_t smem = igemm_tile_lds_bytes(pl.bn);
    p.xcd_deal = (p.taps > 1 || transposed) && !p.two_d ? g_tune_igemm_xcd : 0;
    launch_igemm(p, pl.bn == 64, grid, smem, st);
    rc = check_launch("conv3d_igemm_bf16x3_kernel");
  } else {
    rc = launch_halo(p, pl, st);
  }
  if (rc) return rc;
  return conv_finish(p, OV, st);
}

// A batch of `scenes` volumes of one grid in ONE launch: x [scenes * ix*iy*iz, Cin], scene s in rows [s * IV, (s + 1) * IV); y and
// residual [scenes * OV, Cout]; weights, scale and shift shared.  Every scene is convolved on its own (zero padding at its border).
// The family, brick and column tile are those of the per-scene grid; the split count follows the whole launch, so the result agrees
// with per-scene launches to summation order (bitwise where the splits coincide).  scenes = 1 IS sgc_conv3d_cl_bf16x3.
extern "C" int sgc_conv3d_cl_bf16x3_batched(const float *x, const uint16_t *w_hi, const uint16_t *w_lo, const float *scale,
                                            const float *shift, const float *residual_or_null, float *y,
                                            int ix, int iy, int iz, int Cin, int Cout, int ksize, int stride,
                                            int transposed, int relu, int scenes, float *workspace_or_null, int64_t workspace_floats,
                                            sgc_stream_t stream) {
  return conv3d_bf16x3(x, w_hi, w_lo, scale, shift, residual_or_null, y, ix, iy, iz, Cin, Cout, ksize, stride, transposed, relu,
                       workspace_or_null, workspace_floats, nullptr, stream, 0, nullptr, 0, 0, 0, 0, scenes);
}

extern "C" int sgc_conv3d_cl_bf16x3(const float *x, const uint16_t *w_hi, const uint16_t *w_lo, const float *scale,
                                    const float *shift, const float *residual_or_null, float *y,
                                    int ix, int iy, int iz, int Cin, int Cout, int ksize, int stride,
                                    int transposed, int relu, float *workspace_or_null, int64_t workspace_floats,
                                    sgc_stream_t stream) {
  return sgc_conv3d_cl_bf16x3_batched(x, w_hi, w_lo, scale, shift, residual_or_null, y, ix, iy, iz, Cin, Cout, ksize, stride,
                                      transposed, relu, 1, workspace_or_null, workspace_floats, stream);
}

// 2-D convolution over a stack of channels-last images (the producer side of the hand-over -- the FPN's
// output convolutions, mmdet FPN.fpn_convs as configured by configs/SGCDet_ScanNet.py:84-88 and called at detectors/
// SGCDet.py:67, emitting the [N, H*W, C] rows the view transformation consumes, TU/transformer.py:151-170, without an
// NCHW round trip).  x [N*H*W, Cin] -> y [N*H*W, Cout], ksize 1 | 3 (pad k/2), stride 1; same bf16x3 arithmetic and
// epilogue (scale / shift / residual / relu) as the 3-D entry point, on the implicit-GEMM kernel with the taps confined to
// the (row, column) plane.
extern "C" int sgc_conv2d_nhwc_bf16x3(const float *x, const uint16_t *w_hi, const uint16_t *w_lo, const float *scale,
                                      const float *shift, const float *residual_or_null, float *y, int N, int H, int W,
                                      int Cin, int Cout, int ksize, int relu, sgc_stream_t stream) {
  if (ksize != 1 && ksize != 3) return set_error(SGC_EUNSUP, "sgc_conv2d_nhwc_bf16x3: ksize in {1,3}");
  return conv3d_bf16x3(x, w_hi, w_lo, scale, shift, residual_or_null, y, N, H, W, Cin, Cout, ksize, 1, 0, relu, nullptr, 0,
                       nullptr, stream, 1);
}

// Output-masked 3x3x3 stride-1 convolution (the decoder tail / head of the neck, where only voxels in -- or next to --
// the refined set are consumed, necks/imvoxelnet.py:47-64, dense_heads/imvoxel_head_v2.py:258,301): live rows are
// bit-identical to sgc_conv3d_cl_bf16x3.  Layers the halo kernel does not take run dense (the mask is a licence, not a
// duty).
extern "C" int sgc_conv3d_cl_bf16x3_masked(const float *x, const uint16_t *w_hi, const uint16_t *w_lo, const float *scale,
                                           const float *shift, const float *residual_or_null, float *y,
                                           const uint8_t *out_mask, int ix, int iy, int iz, int Cin, int Cout, int relu,
                                           float *workspace_or_null, int64_t workspace_floats, sgc_stream_t stream) {
  if (!out_mask) return set_error(SGC_EINVAL, "sgc_conv3d_cl_bf16x3_masked: null mask");
  return conv3d_bf16x3(x, w_hi, w_lo, scale, shift, residual_or_null, y, ix, iy, iz, Cin, Cout, 3, 1, 0, relu,
                       workspace_or_null, workspace_floats, out_mask, stream);
}

// 3x3x3 stride-1 convolution whose columns [act_c0, act_c1) leave as expf(v * *act_scale_dev) -- the head's fused
// centerness | reg | cls convolution with `torch.exp(scale(reg))` (dense_heads/imvoxel_head_v2.py:79,103-110: mmcv Scale, a
// learnable scalar, then exp) in the epilogue instead of two elementwise launches per scale.  out_mask_or_null as in
// sgc_conv3d_cl_bf16x3_masked.  The other columns are bit-identical to sgc_conv3d_cl_bf16x3.
extern "C" int sgc_conv3d_cl_bf16x3_act(const float *x, const uint16_t *w_hi, const uint16_t *w_lo, const float *scale,
                                        const float *shift, const float *residual_or_null, float *y,
                                        const uint8_t *out_mask_or_null, int ix, int iy, int iz, int Cin, int Cout, int relu,
                                        int act_c0, int act_c1, const float *act_scale_dev,
                                        float *workspace_or_null, int64_t workspace_floats, sgc_stream_t stream) {
  if (!act_scale_dev || act_c0 < 0 || act_c1 > Cout || act_c1 <= act_c0)
    return set_error(SGC_EINVAL, "sgc_conv3d_cl_bf16x3_act: needs 0 <= act_c0 < act_c1 <= Cout and a scale pointer");
  return conv3d_bf16x3(x, w_hi, w_lo, scale, shift, residual_or_null, y, ix, iy, iz, Cin, Cout, 3, 1, 0, relu,
                       workspace_or_null, workspace_floats, out_mask_or_null, stream, 0, act_scale_dev, act_c0, act_c1);
}

extern "C" int sgc_conv3d_winograd_z_supported(int ix, int iy, int iz, int Cin, int Cout) {
  // Z/2 images per position, in bricks of 4 or 2, more than 64 output channels; the rest is plan_conv's gate of the virtual stack of
  // 2 Z images of ix x iy pixels (slices of at least 8 x 8 pixels; Z = 4, or Z % 8 == 0 and halo_min_m rows in the stack)
  if (ix <= 0 || iy <= 0 || iz < 4 || iz % 4 || Cin % 32 || Cout % 4 || Cout <= 64) return 0;
  ConvParams p = {};
  p.two_d = 1; p.w_group_images = iz / 2; p.wz_Z = iz;
  int ox, oy, oz;
  conv_geometry(p, 2 * iz, ix, iy, Cin, Cout, 3, 1, 0, ox, oy, oz);
  return plan_conv(p, (int64_t)ox * oy * oz, false).family == kConvHaloWZ ? 1 : 0;
}
extern "C" int64_t sgc_conv3d_winograd_z_workspace_floats(int ix, int iy, int iz, int Cin, int Cout) {
  (void)Cin;
  return sgc_conv3d_winograd_z_supported(ix, iy, iz, Cin, Cout) ? (int64_t)2 * ix * iy * iz * Cout : 0;    // the four transform-domain outputs
}

// 3x3x3 stride-1 convolution through the Winograd F(2,3) transform along z (see the kernels above): wg_hi / wg_lo are the bf16 hi / lo
// planes of the TRANSFORMED weights [4][9][Cout][Cin] (position, (dx, dy) tap); workspace >= 2 V Cout floats (the four transform-domain
// outputs; the input transform is fused into the halo staging, so no transformed copy of the input exists): two launches.
extern "C" int sgc_conv3d_winograd_z_bf16x3(const float *x, const uint16_t *wg_hi, const uint16_t *wg_lo, const float *scale,
                                            const float *shift, const float *residual_or_null, float *y, int ix, int iy, int iz,
                                            int Cin, int Cout, int relu, float *workspace, int64_t workspace_floats,
                                            sgc_stream_t stream) {
  if (!x || !wg_hi || !wg_lo || !y || !workspace) return set_error(SGC_EINVAL, "sgc_conv3d_winograd_z_bf16x3: null pointer");
  if (!sgc_conv3d_winograd_z_supported(ix, iy, iz, Cin, Cout))
    return set_error(SGC_EUNSUP, "sgc_conv3d_winograd_z_bf16x3: needs ix, iy >= 8, iz == 4 or iz %% 8 == 0 with >= 2048 stack rows, Cin %% 32 == 0, Cout %% 4 == 0, Cout > 64");
  if (workspace_floats < sgc_conv3d_winograd_z_workspace_floats(ix, iy, iz, Cin, Cout))
    return set_error(SGC_EINVAL, "sgc_conv3d_winograd_z_bf16x3: workspace too small");
  if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)workspace | (uintptr_t)residual_or_null | (uintptr_t)scale | (uintptr_t)shift) & 15)
    return set_error(SGC_EINVAL, "sgc_conv3d_winograd_z_bf16x3: pointers must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int64_t V = (int64_t)ix * iy * iz;
  const int J = iz / 2;
  float *m = workspace;
  const int64_t n_out = V / 2 * (Cout / 4);
  // four 3 x 3 convolutions over (x, y) as ONE launch of the halo kernel's 2-D form on the VIRTUAL stack of 4 J images (the input
  // transform happens while the halo rows are staged: template flag WZ), weight set = image / J
  // what the caller passed beyond the transform-domain tensor holds the partial tiles of a split reduction (the few-brick launches of
  // the small stacks): summed in split order by conv_epilogue_kernel before the output transform reads m -- no atomics
  const int64_t m_floats = 2 * V * Cout, spare = workspace_floats - m_floats;
  int rc = conv3d_bf16x3(x, wg_hi, wg_lo, nullptr, nullptr, nullptr, m, 4 * J, ix, iy, Cin, Cout, 3, 1, 0, 0, spare > 0 ? m + m_floats : nullptr,
                         spare > 0 ? spare : 0, nullptr, stream, 1, nullptr, 0, 0, J, iz);
  if (rc) return rc;
  hipLaunchKernelGGL(winograd_z_out_kernel, dim3((unsigned)std::min<int64_t>((n_out + 255) / 256, 65536)), dim3(256), 0, st,
                     reinterpret_cast<const float4 *>(m), reinterpret_cast<float4 *>(y), scale, shift,
                     reinterpret_cast<const float4 *>(residual_or_null), ix, iy, iz, Cout / 4, relu, nullptr, 0, 0);
  return check_launch("winograd_z_out_kernel");
}

// Split-K workspace (floats) the convolution above would use for a deterministic reduction; 0 = the layer is not
// split.  The answer of the same dispatch as the launch: pick_splitk for sgc_conv3d_cl_f32 (bf16x3 = 0), plan_conv for
// sgc_conv3d_cl_bf16x3 (bf16x3 = 1).
extern "C" int64_t sgc_conv3d_batched_workspace_floats(int ix, int iy, int iz, int Cin, int Cout, int ksize, int stride,
                                                       int transposed, int bf16x3, int scenes) {
  if (ix <= 0 || iy <= 0 || iz <= 0 || Cin <= 0 || Cout <= 0 || scenes < 1 || (scenes > 1 && !bf16x3)) return 0;
  ConvParams p = {};
  p.scenes = scenes;
  int ox, oy, oz;
  conv_geometry(p, ix, iy, iz, Cin, Cout, ksize, stride, transposed, ox, oy, oz);
  const int64_t OV = (int64_t)scenes * ox * oy * oz;
  if (!bf16x3) {
    const int splitk = pick_splitk(p, ceil_div(p.M, BM), ceil_div(Cout, Cout <= 32 ? 32 : 128), g_tune_split_target);
    return splitk > 1 ? (int64_t)splitk * OV * Cout : 0;
  }
  const ConvPlan pl = plan_conv(p, OV, false);
  // a MASKED call on the whole-grid-brick grids takes the tile kernel (that brick carries no output mask): size for whichever
  // form splits further, so that neither ever falls back to float atomics for want of workspace
  return pl.family == kConvHaloGrid ? std::max(pl.ws_floats, plan_conv(p, OV, true).ws_floats) : pl.ws_floats;
}
extern "C" int64_t sgc_conv3d_workspace_floats(int ix, int iy, int iz, int Cin, int Cout, int ksize, int stride,
                                               int transposed, int bf16x3) {
  return sgc_conv3d_batched_workspace_floats(ix, iy, iz, Cin, Cout, ksize, stride, transposed, bf16x3, 1);
}

// y[rows, Cout] = x[rows, Cin] @ W^T + shift with the row count on the DEVICE: the pair-list stages size their
// GEMMs by the number of visible (camera, voxel) pairs, which sgc_compact_pairs leaves in totals[] -- reading it
// back costs a host round trip per level.  The grid covers rows_cap; workgroups past *rows_dev exit at once.
static int linear_rows(const float *x, const uint16_t *w_hi, const uint16_t *w_lo, const float *shift,
                       float *y, const int32_t *rows_dev_or_null, int rows_cap, int Cin, int Cout, int hm_S, int hm_cm,
                       int hm_bf16, sgc_stream_t stream, float *zero_row = nullptr) {
  if (!x || !w_hi || !w_lo || !y) return set_error(SGC_EINVAL, "sgc_linear_rows_bf16x3: null pointer");
  if (rows_cap <= 0) return SGC_OK;
  if (Cin % 32 || Cout % 4) return set_error(SGC_EUNSUP, "sgc_linear_rows_bf16x3: needs Cin %% 32 == 0 and Cout %% 4 == 0");
  // (a variant with the A operand resident in registers -- one wave owning 32 rows for the whole K = 256
  //  reduction, weights streamed through LDS in 32-column tiles -- was built, bit-identical, and measured:
  //  159 vs 175 us on 188,800 rows but 57 vs 41 us on 77,000 x 128 and 41 vs 18 us on 6,400 rows: its 10 us
  //  load-and-split prologue per workgroup is not amortised.  Not adopted.)
  if (((uintptr_t)x | (uintptr_t)w_hi | (uintptr_t)w_lo | (uintptr_t)y) & 15)
    return set_error(SGC_EINVAL, "sgc_linear_rows_bf16x3: pointers must be 16-byte aligned");
  if (rows_gemm_supported(Cin, Cout, hm_cm, hm_S, rows_cap, Cin))
    return rows_gemm_launch(x, Cin, w_hi, w_lo, nullptr, shift, nullptr, y, rows_dev_or_null, rows_cap, Cin, Cout, 0, hm_S, hm_cm,
                            hm_bf16, (hipStream_t)stream, zero_row);
  ConvParamsB p = {};
  p.zero_row = zero_row;
  p.x = x; p.w_hi = reinterpret_cast<const __bf16 *>(w_hi); p.w_lo = reinterpret_cast<const __bf16 *>(w_lo);
  p.y = y; p.shift = shift;
  p.Cin = Cin; p.Cout = Cout;
  p.ix = rows_cap; p.iy = 1; p.iz = 1; p.gx = rows_cap; p.gy = 1; p.gz = 1;
  p.ksize = 1; p.stride = 1; p.pad = 0; p.taps = 1; p.splitk = 1; p.M = rows_cap; p.scenes = 1; p.m_dev = rows_dev_or_null;
  p.hm_S = hm_S; p.hm_cm = hm_cm; p.hm_bf16 = hm_bf16;
  const bool narrow = Cout <= 64;
  const int bn = narrow ? 64 : 128;
  const dim3 grid(ceil_div(rows_cap, BM), ceil_div(Cout, bn), 1);
  const size_t smem = igemm_tile_lds_bytes(bn);
  hipStream_t st = (hipStream_t)stream;
  if (!igemm_fits_32bit(p)) return set_error(SGC_EUNSUP, "sgc_linear_rows_bf16x3: the input must stay below 4 GiB and the weights below 2 GiB");
  launch_igemm(p, narrow, grid, smem, st);
  return check_launch("conv3d_igemm_bf16x3_kernel (linear rows)");
}

extern "C" int sgc_linear_rows_bf16x3(const float *x, const uint16_t *w_hi, const uint16_t *w_lo, const float *shift,
                                      float *y, const int32_t *rows_dev_or_null, int rows_cap, int Cin, int Cout,
                                      sgc_stream_t stream) {
  return linear_rows(x, w_hi, w_lo, shift, y, rows_dev_or_null, rows_cap, Cin, Cout, 0, 0, 0, stream);
}

// ... with one extra all-zero row behind the result: y holds rows_cap + 1 rows and row rows_cap is set to zero by the SAME launch
// (the wave gather points out-of-image corners at that row, sgc_pairs_deform_gather's value_has_zero_row -- a separate fill was one
// more launch per level).  rows_cap > 0.
extern "C" int sgc_linear_rows_zrow_bf16x3(const float *x, const uint16_t *w_hi, const uint16_t *w_lo, const float *shift,
                                           float *y, const int32_t *rows_dev_or_null, int rows_cap, int Cin, int Cout,
                                           sgc_stream_t stream) {
  if (rows_cap <= 0 || !y) return set_error(SGC_EINVAL, "sgc_linear_rows_zrow_bf16x3: needs rows_cap > 0 and an output");
  return linear_rows(x, w_hi, w_lo, shift, y, rows_dev_or_null, rows_cap, Cin, Cout, 0, 0, 0, stream, y + (int64_t)rows_cap * Cout);
}

// The same GEMM with a HEAD-MAJOR result: x holds N * S rows (camera-major pixels), the Cout columns are M heads of
// Cm channels, and y is [N][M][S][Cm] -- the layout the LDS-tiled deformable gather stages one head's window from
// (dfa3d_tile.hip).  Same arithmetic per element as sgc_linear_rows_bf16x3: only the store address differs.
extern "C" int sgc_linear_rows_headmajor_bf16x3(const float *x, const uint16_t *w_hi, const uint16_t *w_lo,
                                                const float *shift, void *y, int y_bf16, int N, int S, int Cin, int M, int Cm,
                                                sgc_stream_t stream) {
  if (N <= 0 || S <= 0 || M <= 0 || Cm <= 0 || Cm % 4 || (int64_t)N * S >= (1ll << 31))
    return set_error(SGC_EINVAL, "sgc_linear_rows_headmajor_bf16x3: bad size (Cm %% 4 == 0 required)");
  // the head-major epilogues keep a head inside one column tile (128 columns on the tile kernel -- 64 when M * Cm <= 64 --,
  // 32 per wave on the persistent kernel, which also takes whole-wave multiples up to 128)
  const int tile_cols = M * Cm <= 64 ? 64 : 128;
  if (tile_cols % Cm)
    return set_error(SGC_EUNSUP, "sgc_linear_rows_headmajor_bf16x3: Cm must divide the %d-column tile (got %d)", tile_cols, Cm);
  return linear_rows(x, w_hi, w_lo, shift, reinterpret_cast<float *>(y), nullptr, N * S, Cin, M * Cm, S, Cm, y_bf16 ? 1 : 0, stream);
}

// Arithmetic mode of every bf16 MFMA kernel of the library (convolutions, Linears, the fused level tail): 3 = the
// fp32-faithful 3-way split (default), 1 = plain bf16 products.  Changes results (that is its purpose): not a tuning knob.
extern "C" int sgc_set_conv_products(int products) {
  if (products != 1 && products != 2 && products != 3)
    return set_error(SGC_EINVAL, "sgc_set_conv_products: 3 (bf16x3, fp32-faithful), 1 (one bf16 product) or 2 (one fp16 product)");
  sgc::g_conv_products = products;
  return SGC_OK;
}
extern "C" int sgc_get_conv_products(void) { return sgc::g_conv_products; }
