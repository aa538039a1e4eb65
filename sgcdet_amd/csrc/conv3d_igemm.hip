// Implicit-GEMM 3D convolution on MFMA for gfx950, channels-last volumes.
//
// Replaces the dense nn.Conv3d / ConvTranspose3d + BatchNorm3d(eval) + ReLU (+ residual) chains
// of FastIndoorImVoxelNeck (necks/imvoxelnet.py:36-64,146-173) and the three head convolutions
// (dense_heads/imvoxel_head_v2.py:75-78).  The reference runs them through cuDNN; on ROCm torch
// lowers them to MIOpen's Im3d2Col + GEMM (a 27x blown-up column buffer through HBM, measured
// 14.7 of 17.8 ms per scene at config 2).  Here:
//
//   GEMM view   out[v, co] = sum_{tap} sum_{ci} in[nbr(v, tap), ci] * W[tap][co][ci]
//               M = voxels, N = Cout, K = taps * Cin; no column buffer: the A tile of a K-step is
//               gathered straight from the channels-last volume (one tap, BK consecutive
//               channels, zero rows outside the volume) into LDS.
//   tile        128 voxels x BN channels x 32 (K) per 256-thread workgroup, 4 waves, each wave
//               (BM/WM x BN/WN) made of 32x32 MFMA tiles; fp32 operands on
//               v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulate).
//   LDS         A[128][32+4] and B[BN][32+4] floats, K contiguous, double buffered; the +4 pad
//               makes both the ds_write_b128 rows and the ds_read_b128 fragment reads
//               conflict-free (row stride 36 dwords -> 16 distinct 4-bank slots per lane group).
//   fragments   lane (r = l&31, h = l>>5) reads 16 B at [row r][8*kk + 4*h]: the 4 floats feed 4
//               consecutive MFMAs.  A and B use the same k permutation, so the sum is unchanged.
//   pipeline    global loads of K-step s+1 are issued into registers before the MFMAs of step s
//               and written to the other LDS buffer after them (one barrier per K-step).
//   split-K     layers with few voxels (400 / 3200) split the taps over blockIdx.z and add
//               partial tiles with float atomics into a zeroed output; a small epilogue kernel
//               applies BN/ReLU/residual.  Single-pass layers fuse the epilogue.
//   epilogue    y = acc * scale[co] + shift[co], then relu mode 1: relu(y + residual) (residual
//               block), mode 2: relu(y) + residual (decoder skip add); scale/shift carry the
//               folded eval-mode BatchNorm (or the conv bias).
#include "conv_common.hpp"
#include "mma.hpp"
#include "diag.hpp"
#include "tuning.hpp"

namespace sgc {

template <int BN, int WM, int WN>  // WM x WN waves; wave tile (BM/WM) x (BN/WN)
__global__ __launch_bounds__(256) void conv3d_igemm_f32_kernel(const ConvParams p) {
  constexpr int TM = BM / WM / 32, TN = BN / WN / 32;  // MFMA tiles per wave
  constexpr int BROWS = BN / 32;                       // B rows per thread (passes of 32 rows)
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float *As = smem;                      // [2][BM][LDK]
  float *Bs = smem + 2 * BM * LDK;       // [2][BN][LDK]

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid % WN;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  int zid = blockIdx.z;
  int parity = 0;
  if (p.transposed) { parity = zid % 8; zid /= 8; }
  const int taps_per = p.taps / p.splitk;
  const int tap_lo = zid * taps_per;
  const int ksteps_c = p.Cin / BK;
  const int nsteps = taps_per * ksteps_c;

  // --- this thread's load slots: 4 A rows and BROWS B rows, one float4 (c4) each ---
  const int c4 = tid & 7, r0 = tid >> 3;
  int ax[4], ay[4], az[4];
  bool arow_ok[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + r0 + 32 * i;
    arow_ok[i] = m < p.M;
    const int mm = arow_ok[i] ? m : 0;
    az[i] = mm % p.gz;
    ay[i] = (mm / p.gz) % p.gy;
    ax[i] = mm / (p.gz * p.gy);
  }

  float4 ra[4], rb[BROWS];
  auto load_step = [&](int s) {
    const int tap = p.transposed ? parity : tap_lo + s / ksteps_c;
    const int ci0 = (s % ksteps_c) * BK + c4 * 4;
    int dx = 0, dy = 0, dz = 0;
    if (!p.transposed && p.ksize > 1) {
      dx = tap / (p.ksize * p.ksize); dy = (tap / p.ksize) % p.ksize; dz = tap % p.ksize;
      if (p.two_d) { dx = p.pad; dy = tap / p.ksize; dz = tap % p.ksize; }      // k x k taps in the (y, z) plane of every x slice
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int xx = ax[i] * p.stride + dx - p.pad, yy = ay[i] * p.stride + dy - p.pad,
                zz = az[i] * p.stride + dz - p.pad;
      const bool ok = arow_ok[i] && xx >= 0 && xx < p.ix && yy >= 0 && yy < p.iy && zz >= 0 && zz < p.iz;
      ra[i] = ok ? *reinterpret_cast<const float4 *>(p.x + ((int64_t)(xx * p.iy + yy) * p.iz + zz) * p.Cin + ci0)
                 : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int i = 0; i < BROWS; ++i) {
      const int n = n0 + r0 + 32 * i;
      rb[i] = n < p.Cout ? *reinterpret_cast<const float4 *>(p.w + ((int64_t)tap * p.Cout + n) * p.Cin + ci0)
                         : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto store_step = [&](int buf) {
    float *a = As + buf * BM * LDK, *b = Bs + buf * BN * LDK;
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<float4 *>(a + (r0 + 32 * i) * LDK + c4 * 4) = ra[i];
#pragma unroll
    for (int i = 0; i < BROWS; ++i) *reinterpret_cast<float4 *>(b + (r0 + 32 * i) * LDK + c4 * 4) = rb[i];
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int k = 0; k < 16; ++k) acc[i][j][k] = 0.f;

  load_step(0);
  store_step(0);
  __syncthreads();
  const int fr = lane & 31, fh = lane >> 5;
  for (int s = 0; s < nsteps; ++s) {
    const int buf = s & 1;
    if (s + 1 < nsteps) load_step(s + 1);
    const float *a = As + buf * BM * LDK + (wm * (BM / WM) + fr) * LDK + fh * 4;
    const float *b = Bs + buf * BN * LDK + (wn * (BN / WN) + fr) * LDK + fh * 4;
#pragma unroll
    for (int kk = 0; kk < BK / 8; ++kk) {
      float4 af[TM], bf[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) af[i] = *reinterpret_cast<const float4 *>(a + i * 32 * LDK + kk * 8);
#pragma unroll
      for (int j = 0; j < TN; ++j) bf[j] = *reinterpret_cast<const float4 *>(b + j * 32 * LDK + kk * 8);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].x, bf[j].x, acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].y, bf[j].y, acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].z, bf[j].z, acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].w, bf[j].w, acc[i][j], 0, 0, 0);
        }
    }
    if (s + 1 < nsteps) {
      store_step(buf ^ 1);   // the other buffer was last read in step s-1, before the barrier below
    }
    __syncthreads();
  }

  // --- epilogue: C/D layout col = lane&31, row = (j&3) + 8*(j>>2) + 4*(lane>>5) ---
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int col = n0 + wn * (BN / WN) + j * 32 + (lane & 31);
      if (col >= p.Cout) continue;
      const float sc = p.scale ? p.scale[col] : 1.f, sh = p.shift ? p.shift[col] : 0.f;
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int m = m0 + wm * (BM / WM) + i * 32 + (k & 3) + 8 * (k >> 2) + 4 * (lane >> 5);
        if (m >= p.M) continue;
        int64_t orow = m;
        if (p.transposed) {
          const int z = m % p.gz, y = (m / p.gz) % p.gy, x = m / (p.gz * p.gy);
          const int px = parity >> 2, py = (parity >> 1) & 1, pz = parity & 1;
          orow = ((int64_t)(2 * x + px) * (2 * p.gy) + (2 * y + py)) * (2 * p.gz) + (2 * z + pz);
        }
        float *dst = p.y + orow * p.Cout + col;
        if (p.splitk > 1) {
          if (p.ws) p.ws[(int64_t)zid * p.ws_stride + orow * p.Cout + col] = acc[i][j][k];
          else atomicAdd(dst, acc[i][j][k]);
        } else {
          float v = acc[i][j][k] * sc + sh;
          if (p.relu == 2) v = fmaxf(v, 0.f);
          if (p.residual) v += p.residual[orow * p.Cout + col];
          if (p.relu == 1) v = fmaxf(v, 0.f);
          if (p.act_scale) v = act_col(v, col, p.act_c0, p.act_c1, *p.act_scale);
          *dst = v;
        }
      }
    }
}


// ---------------------------------------------------------------------------------------------
// bf16x3 variant: fp32 operands split as a = a_hi + a_lo (two bf16 each), products
// a_hi*b_hi + a_hi*b_lo + a_lo*b_hi on v_mfma_f32_32x32x16_bf16 with fp32 accumulation.  bf16 x bf16
// products are exact in fp32, the dropped a_lo*b_lo term is 2^-16 relative: the result agrees with
// the fp32 kernel to ~1e-5 (tests bound it at 1e-4 of the tensor scale, north-star bar 1e-3) at
// 3/16 of the fp32-MFMA cycles.  Activations stay fp32 in HBM and are split while they are staged
// into LDS; weights are split once on the host.
// ---------------------------------------------------------------------------------------------
// BMT: rows of the workgroup tile (128, or 256 = the tall tile of the split / transposed layers: wave tile 64 x 64, two thirds of the
// LDS fragment reads per MFMA of the 32 x 64 wave tile).  NP: bf16 products per multiply-add (3 = fp32-faithful split, 1 = hi * hi only)
template <int BN, int WM, int WN, int NP = 3, int BMT = 128>
__global__ __launch_bounds__(WM * WN * 64) void conv3d_igemm_bf16x3_kernel(const ConvParamsB p) {
  constexpr int NT = WM * WN * 64;                     // threads per workgroup (256 or 512)
  constexpr int TM = BMT / WM / 32, TN = BN / WN / 32;
  constexpr int ACH = BMT * 8 / NT;                     // float4 A chunks per thread (rows r0 + (NT/8) i)
  constexpr int AROWS = NT / 8;
  constexpr int BCH = BN * 4 / NT;                     // 16-byte weight chunks per thread per plane
  constexpr int BROWS_ = NT / 4;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_b[];
  // per buffer: A_hi[BMT][LDKH], A_lo[BMT][LDKH], B_hi[BN][LDKH], B_lo[BN][LDKH]
  constexpr int A_PLANE = BMT * LDKH, B_PLANE = BN * LDKH, BUF = 2 * A_PLANE + 2 * B_PLANE;
  __bf16 *base = reinterpret_cast<__bf16 *>(smem_b);

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid % WN;
  int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
  if (p.xcd_deal) {
    // the hardware deals workgroup L (x fastest) to XCD L % 8: XCD c holds L = c, c + 8, ...  Renumber so that the tiles an
    // XCD works on are CONSECUTIVE in the chosen order -- neighbours then find their shared operand in that XCD's L2
    const int total = gridDim.x * gridDim.y * gridDim.z;
    const int L = bx + gridDim.x * (by + gridDim.y * bz);
    const int q = total >> 3, r = total & 7, c = L & 7;
    int t = c * q + min(c, r) + (L >> 3);
    if (p.xcd_deal == 1) { bx = t % gridDim.x; t /= gridDim.x; by = t % gridDim.y; bz = t / gridDim.y; }
    else                 { by = t % gridDim.y; t /= gridDim.y; bx = t % gridDim.x; bz = t / gridDim.x; }
  }
  const int m0 = bx * BMT, n0 = by * BN;
  if (p.zero_row && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0)
    for (int c = threadIdx.x; c < p.Cout; c += NT) p.zero_row[c] = 0.f;
  const int Mrows = p.m_dev ? min(p.M, *p.m_dev) : p.M;
  if (m0 >= Mrows) return;
  int zid = bz;
  int parity = 0;
  if (p.transposed) { parity = zid % 8; zid /= 8; }
  // Split z of a split launch owns the K steps [zid * steps_per, ...) of the (tap, channel chunk) sequence: a split boundary may fall
  // inside a tap, so any number of splits balances a launch (round 6; groups of whole taps only allowed 3 / 9 / 27)
  const int ksteps_c = p.Cin / BK;
  const int total_steps = (p.transposed ? 1 : p.taps) * ksteps_c;
  const int step_lo = p.splitk > 1 ? zid * p.steps_per : 0;
  const int nsteps = p.splitk > 1 ? min(p.steps_per, total_steps - step_lo) : total_steps;
  if (nsteps <= 0) return;                              // (the host never launches an empty split)

  // Staging rows are dealt so that the lanes one LDS write pass covers (32 lanes x 8 B for A, 16 lanes x 16 B for B)
  // sit in rows {r, r+4, r+8, r+12}: with the 20-dword row pitch those start 16 banks apart and tile all 64 banks;
  // consecutive rows (the plain tid >> 3 deal) overlap by 12 banks and every pass took two turns.
  const int c4 = tid & 7, rs8 = (tid >> 3) & 7;
  const int r0 = 16 * (wid >> 1) + 2 * (wid & 1) + (rs8 >> 2) + 4 * (rs8 & 3);   // A: row r0 + AROWS i, 4 floats at c4*4
  const int bc = tid & 3, rs16 = (tid >> 2) & 15;
  const int br0 = 16 * wid + (rs16 >> 2) + 4 * (rs16 & 3);                        // B: row br0 + BROWS_ i, 8 bf16 at bc*8
  // Addressing is split by how often it changes.  Per TAP: the input row of each of this thread's A chunks (neighbour lookup,
  // padding test) -> a 32-bit byte offset, 0xfffffff0 for "no such row".  Per STEP: one uniform offset (the channel chunk, and
  // for the weights the tap's slab).  Loads go through buffer descriptors: an offset past the tensor returns zeros, so the loop
  // has no branch and no per-step index arithmetic in the vector unit (it used to spend 280 instructions per step, 100 of them
  // scalar divisions of the tap decode, on 12 MFMAs per wave).
  constexpr unsigned OOB = 0xfffffff0u;
  int ax[ACH], ay[ACH], az[ACH];
  bool arow_ok[ACH];
#pragma unroll
  for (int i = 0; i < ACH; ++i) {
    const int m = m0 + r0 + AROWS * i;
    arow_ok[i] = m < Mrows;
    const int mm = arow_ok[i] ? m : 0;
    az[i] = mm % p.gz;
    ay[i] = (mm / p.gz) % p.gy;
    ax[i] = mm / (p.gz * p.gy);
  }
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float *>(p.x), 0, (int)(unsigned)((int64_t)p.ix * p.iy * p.iz * p.Cin * 4), 0x00020000);
  const int w_bytes = (int)(unsigned)((int64_t)(p.transposed ? 8 : p.taps) * p.Cout * p.Cin * 2);
  const __amdgpu_buffer_rsrc_t whr = __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16 *>(p.w_hi), 0, w_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t wlr = __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16 *>(p.w_lo), 0, w_bytes, 0x00020000);
  unsigned boff[BCH];                                  // this thread's weight rows: fixed for the whole kernel
#pragma unroll
  for (int i = 0; i < BCH; ++i) {
    const int n = n0 + br0 + BROWS_ * i;
    boff[i] = n < p.Cout ? (unsigned)(n * p.Cin + bc * 8) * 2u : OOB;
  }
  unsigned aoff[ACH];                                  // this thread's input rows under the tap being loaded
  auto set_tap = [&](int tap) {
    int dx = 0, dy = 0, dz = 0;
    if (!p.transposed && p.ksize > 1) {
      dx = tap / (p.ksize * p.ksize); dy = (tap / p.ksize) % p.ksize; dz = tap % p.ksize;
      if (p.two_d) { dx = p.pad; dy = tap / p.ksize; dz = tap % p.ksize; }      // k x k taps in the (y, z) plane of every x slice
    }
#pragma unroll
    for (int i = 0; i < ACH; ++i) {
      const int xx = ax[i] * p.stride + dx - p.pad, yy = ay[i] * p.stride + dy - p.pad,
                zz = az[i] * p.stride + dz - p.pad;
      const bool ok = arow_ok[i] && xx >= 0 && xx < p.ix && yy >= 0 && yy < p.iy && zz >= 0 && zz < p.iz;
      aoff[i] = ok ? ((unsigned)((xx * p.iy + yy) * p.iz + zz) * (unsigned)p.Cin + c4 * 4) * 4u : OOB;
    }
  };
  // (a second register stage -- loads of step s + 2 issued before the MFMAs of step s -- was tried: 156 VGPRs and
  //  one workgroup per CU, or 128 with spills; 404 -> 507 us on the per-tap 90 GF layer, 143 -> 180-200 us on the
  //  split-K layers.  Two resident workgroups at 88 VGPRs hide more latency than the deeper prefetch.)
  float4 ra[ACH];
  uint4 rbh[BCH], rbl[BCH];
  if constexpr ((SGC_TILE_SKIP & 6) != 0) {               // timing builds: the registers the skipped loads would have filled
#pragma unroll
    for (int i = 0; i < ACH; ++i) ra[i] = make_float4(1.f + tid, 2.f, 3.f, 4.f);
#pragma unroll
    for (int i = 0; i < BCH; ++i) { rbh[i] = make_uint4(tid, 1, 2, 3); rbl[i] = make_uint4(3, 2, 1, tid); }
  }
  int ld_tap = p.transposed ? parity : step_lo / ksteps_c;       // (tap, channel chunk) of the NEXT load_step
  int ld_kc = p.transposed ? step_lo : step_lo % ksteps_c;
  set_tap(ld_tap);
  auto load_step = [&]() {
    const int soff_a = __builtin_amdgcn_readfirstlane(ld_kc * (BK * 4));
    const int soff_b = __builtin_amdgcn_readfirstlane((ld_tap * p.Cout * p.Cin + ld_kc * BK) * 2);
#pragma unroll
    for (int i = 0; i < ACH; ++i) {
      if constexpr ((SGC_TILE_SKIP & 2) != 0) break;      // timing builds (diag.hpp): no input loads
      const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(xr, aoff[i], soff_a, 0);
      ra[i] = make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3]));
    }
#pragma unroll
    for (int i = 0; i < BCH; ++i) {
      if constexpr ((SGC_TILE_SKIP & 4) != 0) break;      // timing builds: no weight loads
      const u32x4 h = __builtin_amdgcn_raw_buffer_load_b128(whr, boff[i], soff_b, 0);
      rbh[i] = make_uint4(h[0], h[1], h[2], h[3]);
      if constexpr (NP == 3) {
        const u32x4 l = __builtin_amdgcn_raw_buffer_load_b128(wlr, boff[i], soff_b, 0);
        rbl[i] = make_uint4(l[0], l[1], l[2], l[3]);
      } else {
        rbl[i] = make_uint4(0, 0, 0, 0);
      }
    }
    if (++ld_kc == ksteps_c) {                          // next tap: uniform branch, once per Cin / 32 steps
      ld_kc = 0;
      ++ld_tap;
      if (!p.transposed && ld_tap < p.taps) set_tap(ld_tap);
    }
  };
  auto store_step = [&](int buf) {
    if constexpr ((SGC_TILE_SKIP & 8) != 0) { if (p.relu != 77) return; }    // timing builds: no split, no LDS stores
    __bf16 *a_hi = base + buf * BUF, *a_lo = a_hi + A_PLANE, *b_hi = a_lo + A_PLANE, *b_lo = b_hi + B_PLANE;
#pragma unroll
    for (int i = 0; i < ACH; ++i) {
      const float v[4] = {ra[i].x, ra[i].y, ra[i].z, ra[i].w};
      bf16x4 h, l;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const __bf16 hb = op_hi<NP>(v[e]);
        h[e] = hb;
        l[e] = op_lo<NP>(v[e], hb);
      }
      const int o = (r0 + AROWS * i) * LDKH + c4 * 4;
      *reinterpret_cast<bf16x4 *>(a_hi + o) = h;
      if constexpr (NP == 3) *reinterpret_cast<bf16x4 *>(a_lo + o) = l;
    }
#pragma unroll
    for (int i = 0; i < BCH; ++i) {
      const int o = (br0 + BROWS_ * i) * LDKH + bc * 8;
      *reinterpret_cast<uint4 *>(b_hi + o) = rbh[i];
      if constexpr (NP == 3) *reinterpret_cast<uint4 *>(b_lo + o) = rbl[i];
    }
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int k = 0; k < 16; ++k) acc[i][j][k] = 0.f;

  load_step();
  store_step(0);
  __syncthreads();
  const int fr = lane & 31, fh = lane >> 5;
  for (int s = 0; s < nsteps; ++s) {
    const int buf = s & 1;
    if (s + 1 < nsteps) load_step();
    const __bf16 *a_hi = base + buf * BUF + (wm * (BMT / WM) + fr) * LDKH + fh * 8;
    const __bf16 *a_lo = a_hi + A_PLANE;
    const __bf16 *b_hi = base + buf * BUF + 2 * A_PLANE + (wn * (BN / WN) + fr) * LDKH + fh * 8;
    const __bf16 *b_lo = b_hi + B_PLANE;
#pragma unroll
    for (int kk = 0; kk < BK / 16; ++kk) {
      bf16x8 ah[TM], al[TM], bh[TN], bl[TN];
      if constexpr ((SGC_TILE_SKIP & 16) != 0) {           // timing builds: no fragment reads
#pragma unroll
        for (int i = 0; i < TM; ++i) { ah[i] = (bf16x8)(__bf16)(float)(lane + kk); al[i] = (bf16x8)(__bf16)(float)(lane + 2 * kk); }
#pragma unroll
        for (int j = 0; j < TN; ++j) { bh[j] = (bf16x8)(__bf16)(float)(wid + kk); bl[j] = (bf16x8)(__bf16)(float)(wid + 3 * kk); }
      } else {
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        ah[i] = *reinterpret_cast<const bf16x8 *>(a_hi + i * 32 * LDKH + kk * 16);
        if constexpr (NP == 3) al[i] = *reinterpret_cast<const bf16x8 *>(a_lo + i * 32 * LDKH + kk * 16);
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        bh[j] = *reinterpret_cast<const bf16x8 *>(b_hi + j * 32 * LDKH + kk * 16);
        if constexpr (NP == 3) bl[j] = *reinterpret_cast<const bf16x8 *>(b_lo + j * 32 * LDKH + kk * 16);
      }
      }
      if constexpr ((SGC_TILE_SKIP & 1) != 0) {            // timing builds: everything but the MFMAs
#pragma unroll
        for (int i = 0; i < TM; ++i) asm volatile("" ::"v"(ah[i]), "v"(al[i]));
#pragma unroll
        for (int j = 0; j < TN; ++j) asm volatile("" ::"v"(bh[j]), "v"(bl[j]));
        continue;
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          if constexpr (NP == 3) {
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
          }
          acc[i][j] = mma_hh<NP>(ah[i], bh[j], acc[i][j]);
        }
    }
    if (s + 1 < nsteps) store_step(buf ^ 1);
    if constexpr ((SGC_TILE_SKIP & 32) == 0) __syncthreads();     // timing builds: no barrier per step
  }
  if constexpr ((SGC_TILE_SKIP & 64) != 0) { if (p.relu != 77) return; }      // timing builds: no epilogue

  // Epilogue through LDS: in the MFMA layout a lane owns ONE column and 16 rows of a tile, i.e. 4-byte stores, 32 per
  // lane -- store-issue bound (PMC on the K = 256 Linears: waves parked 54 % of their cycles, matrix pipe busy 20 %).
  // The staging buffers are free now: the tile goes to LDS once and leaves as 16-byte row-contiguous stores (and the
  // partial tiles of a split reduction, the residual and the scale / shift vectors move 16 bytes at a time too).
  if ((p.Cout & 3) == 0 && (p.splitk == 1 || p.ws)) {
    constexpr int LDC = BN + 8;                              // floats per staged row: rows r and r + 4 (lane halves) 32 banks apart
    float *cs = reinterpret_cast<float *>(smem_b);           // [BMT][LDC] <= the 2 x (A + B) staging buffers
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int k = 0; k < 16; ++k)
          cs[(wm * (BMT / WM) + i * 32 + (k & 3) + 8 * (k >> 2) + 4 * (lane >> 5)) * LDC + wn * (BN / WN) + j * 32 + (lane & 31)] =
              acc[i][j][k];
    __syncthreads();
    constexpr int C4 = BN / 4;
    if (p.hm_cm > 0) {
      // head-major store: the lanes of a wave instruction walk ROWS of one head (a head's rows are hm_cm * 4 bytes apart in
      // its plane), so a wave writes one contiguous 1 KiB run instead of 8 head segments 1 plane apart
      const int cvh = p.hm_cm / 4, per_head = BMT * cvh, heads = p.Cout / p.hm_cm;
      const int ncam0 = m0 / p.hm_S, s0 = m0 - ncam0 * p.hm_S;
      for (int e = tid; e < BMT * C4; e += NT) {
        const int hl = e / per_head, rr = e - hl * per_head;
        const int rl = rr / cvh, c4 = hl * cvh + (rr - rl * cvh);
        const int m = m0 + rl, col = n0 + c4 * 4;
        if (m >= Mrows || col >= p.Cout) continue;
        float4 v = *reinterpret_cast<const float4 *>(cs + rl * LDC + c4 * 4);
        if (p.shift) {
          const float4 sh4 = *reinterpret_cast<const float4 *>(p.shift + col);
          v.x += sh4.x; v.y += sh4.y; v.z += sh4.z; v.w += sh4.w;
        }
        int ncam = ncam0, spx = s0 + rl;             // rows of one tile straddle at most a few cameras: no division per element
        while (spx >= p.hm_S) { spx -= p.hm_S; ++ncam; }
        const int head = (n0 / p.hm_cm) + hl;
        const int64_t o = (((int64_t)ncam * heads + head) * p.hm_S + spx) * p.hm_cm + (col - head * p.hm_cm);
        if (p.hm_bf16) {
          bf16x4 h;
          h[0] = (__bf16)v.x; h[1] = (__bf16)v.y; h[2] = (__bf16)v.z; h[3] = (__bf16)v.w;
          *reinterpret_cast<bf16x4 *>(reinterpret_cast<__bf16 *>(p.y) + o) = h;
        } else {
          *reinterpret_cast<float4 *>(p.y + o) = v;
        }
      }
      return;
    }
    for (int e = tid; e < BMT * C4; e += NT) {
      const int rl = e / C4, c4 = e - rl * C4;
      const int m = m0 + rl, col = n0 + c4 * 4;
      if (m >= Mrows || col >= p.Cout) continue;
      int64_t orow = m;
      if (p.transposed) {
        const int z = m % p.gz, y = (m / p.gz) % p.gy, x = m / (p.gz * p.gy);
        const int px = parity >> 2, py = (parity >> 1) & 1, pz = parity & 1;
        orow = ((int64_t)(2 * x + px) * (2 * p.gy) + (2 * y + py)) * (2 * p.gz) + (2 * z + pz);
      }
      float4 v = *reinterpret_cast<const float4 *>(cs + rl * LDC + c4 * 4);
      if (p.splitk > 1) {
        *reinterpret_cast<float4 *>(p.ws + (int64_t)zid * p.ws_stride + orow * p.Cout + col) = v;
        continue;
      }
      if (p.scale) {
        const float4 sc4 = *reinterpret_cast<const float4 *>(p.scale + col);
        v.x *= sc4.x; v.y *= sc4.y; v.z *= sc4.z; v.w *= sc4.w;
      }
      if (p.shift) {
        const float4 sh4 = *reinterpret_cast<const float4 *>(p.shift + col);
        v.x += sh4.x; v.y += sh4.y; v.z += sh4.z; v.w += sh4.w;
      }
      if (p.relu == 2) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
      if (p.residual) {
        const float4 r4 = *reinterpret_cast<const float4 *>(p.residual + orow * p.Cout + col);
        v.x += r4.x; v.y += r4.y; v.z += r4.z; v.w += r4.w;
      }
      if (p.relu == 1) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
      if (p.act_scale) v = act_col4(v, col, p.act_c0, p.act_c1, *p.act_scale);
      *reinterpret_cast<float4 *>(p.y + orow * p.Cout + col) = v;
    }
    return;
  }

#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int col = n0 + wn * (BN / WN) + j * 32 + (lane & 31);
      if (col >= p.Cout) continue;
      const float sc = p.scale ? p.scale[col] : 1.f, sh = p.shift ? p.shift[col] : 0.f;
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int m = m0 + wm * (BMT / WM) + i * 32 + (k & 3) + 8 * (k >> 2) + 4 * (lane >> 5);
        if (m >= Mrows) continue;
        int64_t orow = m;
        if (p.transposed) {
          const int z = m % p.gz, y = (m / p.gz) % p.gy, x = m / (p.gz * p.gy);
          const int px = parity >> 2, py = (parity >> 1) & 1, pz = parity & 1;
          orow = ((int64_t)(2 * x + px) * (2 * p.gy) + (2 * y + py)) * (2 * p.gz) + (2 * z + pz);
        }
        float *dst = p.y + orow * p.Cout + col;
        if (p.splitk > 1) {
          if (p.ws) p.ws[(int64_t)zid * p.ws_stride + orow * p.Cout + col] = acc[i][j][k];
          else atomicAdd(dst, acc[i][j][k]);
        } else {
          float v = acc[i][j][k] * sc + sh;
          if (p.relu == 2) v = fmaxf(v, 0.f);
          if (p.residual) v += p.residual[orow * p.Cout + col];
          if (p.relu == 1) v = fmaxf(v, 0.f);
          if (p.act_scale) v = act_col(v, col, p.act_c0, p.act_c1, *p.act_scale);
          *dst = v;
        }
      }
    }
}


int launch_igemm_f32(const ConvParams &p, bool narrow, dim3 grid, hipStream_t st) {
  const size_t smem = (size_t)2 * (BM + (narrow ? 32 : 128)) * LDK * sizeof(float);
  if (narrow) {
    hipLaunchKernelGGL((conv3d_igemm_f32_kernel<32, 4, 1>), grid, dim3(256), smem, st, p);
  } else {
    static std::atomic<uint64_t> attr_done{0};
    ensure_dynamic_lds((const void *)conv3d_igemm_f32_kernel<128, 2, 2>, (int)smem, attr_done);
    hipLaunchKernelGGL((conv3d_igemm_f32_kernel<128, 2, 2>), grid, dim3(256), smem, st, p);
  }
  return check_launch("conv3d_igemm_f32_kernel");
}

// one launch of the tile-per-workgroup implicit-GEMM kernel in the arithmetic mode of g_conv_products
template <int NP>
static void launch_igemm_np(const ConvParamsB &p, bool narrow, dim3 grid, size_t smem, hipStream_t st) {
  static std::atomic<uint64_t> done[2];
  const int big = (int)((size_t)2 * (2 * BM + 2 * 128) * LDKH * sizeof(uint16_t));
  ensure_dynamic_lds((const void *)conv3d_igemm_bf16x3_kernel<128, 2, 2, NP>, big, done[0]);
  ensure_dynamic_lds((const void *)conv3d_igemm_bf16x3_kernel<128, 4, 2, NP>, big, done[1]);
  if (narrow) hipLaunchKernelGGL((conv3d_igemm_bf16x3_kernel<64, 4, 1, NP>), grid, dim3(256), smem, st, p);
  else if (g_tune_conv_waves == 8) hipLaunchKernelGGL((conv3d_igemm_bf16x3_kernel<128, 4, 2, NP>), grid, dim3(512), smem, st, p);
  else hipLaunchKernelGGL((conv3d_igemm_bf16x3_kernel<128, 2, 2, NP>), grid, dim3(256), smem, st, p);
}
void launch_igemm(const ConvParamsB &p, bool narrow, dim3 grid, size_t smem, hipStream_t st) {
  if (g_conv_products == 1) launch_igemm_np<1>(p, narrow, grid, smem, st);
  else if (g_conv_products == 2) launch_igemm_np<2>(p, narrow, grid, smem, st);
  else launch_igemm_np<3>(p, narrow, grid, smem, st);
}
}  // namespace sgc
