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
#include "igemm_tile.hpp"
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
          if (p.relu == 2) v = relu_nan(v);
          if (p.residual) v += p.residual[orow * p.Cout + col];
          if (p.relu == 1) v = relu_nan(v);
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
// Three parts.  CORE (igemm_tile.hpp, shared with the image kernel of conv2d_image.hip): tile constants, LDS plan, staging deal, one K
// step's loads / split / stores, the double-buffered MFMA loop, the C scatter through LDS, the float4 epilogue arithmetic.
// ADDRESSING (here): XCD renumbering, m_dev / zero_row, split-step bookkeeping, GEMM row -> (x, y, z), tap -> byte offsets.
// STORE (here): float4 rows to the split workspace, head-major, transposed parity or with the activation columns; scalar fallback.
// ---------------------------------------------------------------------------------------------
// NP: bf16 products per multiply-add (3 = fp32-faithful split, 1 = hi * hi only).  The tile itself -- LDS plan, staging deal, K loop,
// MFMA group, C scatter -- is IgemmTile (igemm_tile.hpp); here are the addressing of volumes and the store paths.
// SC: the launch holds a batch of scenes (p.scenes > 1, sgc_conv3d_cl_bf16x3_batched).  An instantiation of its own, so that the
// scene-less kernel is the code it always was -- same registers, same spills -- and only a batch pays for the scene decode.
template <int BN, int WM, int WN, int NP = 3, bool SC = false>
__global__ __launch_bounds__(WM * WN * 64) void conv3d_igemm_bf16x3_kernel(const ConvParamsB p) {
  using Tile = IgemmTile<BN, WM, WN, NP>;
  constexpr int NT = Tile::NT, TM = Tile::TM, TN = Tile::TN, ACH = Tile::ACH;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_b[];
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
  const int m0 = bx * BM, n0 = by * BN;
  if (p.zero_row && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0)
    for (int c = threadIdx.x; c < p.Cout; c += NT) p.zero_row[c] = 0.f;
  const int Mall = SC ? p.M * p.scenes : p.M;            // GEMM rows of the launch: scene s owns [s * M, (s + 1) * M)
  const int Mrows = p.m_dev ? min(Mall, *p.m_dev) : Mall;
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

  // Addressing is split by how often it changes.  Per TAP: the input row of each of this thread's A chunks (neighbour lookup,
  // padding test) -> a 32-bit byte offset, 0xfffffff0 for "no such row".  Per STEP: one uniform offset (the channel chunk, and
  // for the weights the tap's slab).  Loads go through buffer descriptors: an offset past the tensor returns zeros, so the loop
  // has no branch and no per-step index arithmetic in the vector unit (it used to spend 280 instructions per step, 100 of them
  // scalar divisions of the tap decode, on 12 MFMAs per wave).
  Tile t(smem_b, threadIdx.x);
  const int tid = t.tid, lane = t.lane, wm = t.wm, wn = t.wn;
  // a tile of 128 rows may span scenes (400 rows per scene at the coarsest scale): the scene is decoded per row and the neighbour
  // test below is against that scene's grid.  A batch (SC) keeps the scene in the upper half of ax[] (the host checks every
  // extent of the grid and the scene count < 2^15): no register per chunk beyond the scene-less kernel's, unpacked once per TAP
  int ax[ACH], ay[ACH], az[ACH];
  bool arow_ok[ACH];
  const int IV = p.ix * p.iy * p.iz;
  constexpr bool batch = SC;
#pragma unroll
  for (int i = 0; i < ACH; ++i) {
    const int m = m0 + t.a_row(i);
    arow_ok[i] = m < Mrows;
    const int mg = arow_ok[i] ? m : 0, sc = batch ? mg / p.M : 0;
    const int mm = mg - sc * p.M;
    az[i] = mm % p.gz;
    ay[i] = (mm / p.gz) % p.gy;
    ax[i] = mm / (p.gz * p.gy) + (sc << 16);
  }
  t.bind(p.x, (int64_t)(SC ? p.scenes : 1) * IV * p.Cin * 4, p.w_hi, p.w_lo, (int64_t)(p.transposed ? 8 : p.taps) * p.Cout * p.Cin * 2,
         n0, p.Cout, p.Cin);
  auto set_tap = [&](int tap) {
    int dx = 0, dy = 0, dz = 0;
    if (!p.transposed && p.ksize > 1) {
      dx = tap / (p.ksize * p.ksize); dy = (tap / p.ksize) % p.ksize; dz = tap % p.ksize;
      if (p.two_d) { dx = p.pad; dy = tap / p.ksize; dz = tap % p.ksize; }      // k x k taps in the (y, z) plane of every x slice
    }
#pragma unroll
    for (int i = 0; i < ACH; ++i) {
      int axp = ax[i];
      if constexpr (SC) asm volatile("" : "+v"(axp));     // unpacked per tap: hoisted out of the K loop the scene's base costs a register per chunk
      const int sc = batch ? axp >> 16 : 0, axl = batch ? axp & 0xffff : axp;
      const int xx = axl * p.stride + dx - p.pad, yy = ay[i] * p.stride + dy - p.pad,
                zz = az[i] * p.stride + dz - p.pad;
      const bool ok = arow_ok[i] && xx >= 0 && xx < p.ix && yy >= 0 && yy < p.iy && zz >= 0 && zz < p.iz;
      t.aoff[i] = ok ? ((unsigned)(sc * IV + (xx * p.iy + yy) * p.iz + zz) * (unsigned)p.Cin + t.c4 * 4) * 4u : Tile::OOB;
    }
  };
  if constexpr ((SGC_TILE_SKIP & 6) != 0) {               // timing builds: the registers the skipped loads would have filled
#pragma unroll
    for (int i = 0; i < ACH; ++i) t.ra[i] = make_float4(1.f + tid, 2.f, 3.f, 4.f);
#pragma unroll
    for (int i = 0; i < Tile::BCH; ++i) { t.rbh[i] = make_uint4(tid, 1, 2, 3); t.rbl[i] = make_uint4(3, 2, 1, tid); }
  }
  int ld_tap = p.transposed ? parity : step_lo / ksteps_c;       // (tap, channel chunk) of the NEXT load
  int ld_kc = p.transposed ? step_lo : step_lo % ksteps_c;
  set_tap(ld_tap);
  t.template run<SGC_TILE_SKIP>(nsteps, [&]() {
    t.template load<SGC_TILE_SKIP>(__builtin_amdgcn_readfirstlane(ld_kc * (BK * 4)),
                                   __builtin_amdgcn_readfirstlane((ld_tap * p.Cout * p.Cin + ld_kc * BK) * 2));
    if (++ld_kc == ksteps_c) {                          // next tap: uniform branch, once per Cin / 32 steps
      ld_kc = 0;
      ++ld_tap;
      if (!p.transposed && ld_tap < p.taps) set_tap(ld_tap);
    }
  }, (SGC_TILE_SKIP & 8) == 0 || p.relu == 77);           // timing builds: no split, no LDS stores
  if constexpr ((SGC_TILE_SKIP & 64) != 0) { if (p.relu != 77) return; }      // timing builds: no epilogue

  auto out_row = [&](int m) -> int64_t {                  // transposed: GEMM row (input voxel) -> output voxel of this parity
    if (!p.transposed) return m;                          // (the output grid is the row grid: scene s starts at row s * M)
    const int sc = SC ? m / p.M : 0, ml = m - sc * p.M;
    const int z = ml % p.gz, y = (ml / p.gz) % p.gy, x = ml / (p.gz * p.gy);
    const int px = parity >> 2, py = (parity >> 1) & 1, pz = parity & 1;
    return (int64_t)sc * 8 * p.M + ((int64_t)(2 * x + px) * (2 * p.gy) + (2 * y + py)) * (2 * p.gz) + (2 * z + pz);
  };
  // Store paths.  Whole float4 columns and no atomics: through LDS (the partial tiles of a split reduction, the residual and
  // the scale / shift vectors move 16 bytes at a time too).
  if ((p.Cout & 3) == 0 && (p.splitk == 1 || p.ws)) {
    float *cs = t.scatter();
    constexpr int C4 = Tile::C4;
    if (p.hm_cm > 0) {
      // head-major store: the lanes of a wave instruction walk ROWS of one head (a head's rows are hm_cm * 4 bytes apart in
      // its plane), so a wave writes one contiguous 1 KiB run instead of 8 head segments 1 plane apart
      const int cvh = p.hm_cm / 4, per_head = BM * cvh, heads = p.Cout / p.hm_cm;
      const int ncam0 = m0 / p.hm_S, s0 = m0 - ncam0 * p.hm_S;
      for (int e = tid; e < BM * C4; e += NT) {
        const int hl = e / per_head, rr = e - hl * per_head;
        const int rl = rr / cvh, c4 = hl * cvh + (rr - rl * cvh);
        const int m = m0 + rl, col = n0 + c4 * 4;
        if (m >= Mrows || col >= p.Cout) continue;
        const float4 v = epilogue4(*Tile::c_quad(cs, rl, c4), col, nullptr, p.shift, false, nullptr, 0, false);
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
    for (int e = tid; e < BM * C4; e += NT) {
      const int rl = e / C4, c4 = e - rl * C4;
      const int m = m0 + rl, col = n0 + c4 * 4;
      if (m >= Mrows || col >= p.Cout) continue;
      const int64_t orow = out_row(m);
      float4 v = *Tile::c_quad(cs, rl, c4);
      if (p.splitk > 1) {
        *reinterpret_cast<float4 *>(p.ws + (int64_t)zid * p.ws_stride + orow * p.Cout + col) = v;
        continue;
      }
      v = epilogue4(v, col, p.scale, p.shift, p.relu == 2, p.residual, orow * p.Cout + col, p.relu == 1);
      if (p.act_scale) v = act_col4(v, col, p.act_c0, p.act_c1, *p.act_scale);
      *reinterpret_cast<float4 *>(p.y + orow * p.Cout + col) = v;
    }
    return;
  }

  // Cout % 4 or float atomics: scalar stores straight from the MFMA layout
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
        if (m >= Mrows) continue;
        const int64_t orow = out_row(m);
        float *dst = p.y + orow * p.Cout + col;
        if (p.splitk > 1) {
          if (p.ws) p.ws[(int64_t)zid * p.ws_stride + orow * p.Cout + col] = t.acc[i][j][k];
          else atomicAdd(dst, t.acc[i][j][k]);
        } else {
          float v = t.acc[i][j][k] * sc + sh;
          if (p.relu == 2) v = relu_nan(v);
          if (p.residual) v += p.residual[orow * p.Cout + col];
          if (p.relu == 1) v = relu_nan(v);
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
template <int NP, bool SC>
static void launch_igemm_np(const ConvParamsB &p, bool narrow, dim3 grid, size_t smem, hipStream_t st) {
  static std::atomic<uint64_t> done[2];
  constexpr int big = igemm_tile_lds_bytes(128);
  ensure_dynamic_lds((const void *)conv3d_igemm_bf16x3_kernel<128, 2, 2, NP, SC>, big, done[0]);
  ensure_dynamic_lds((const void *)conv3d_igemm_bf16x3_kernel<128, 4, 2, NP, SC>, big, done[1]);
  if (narrow) hipLaunchKernelGGL((conv3d_igemm_bf16x3_kernel<64, 4, 1, NP, SC>), grid, dim3(256), smem, st, p);
  else if (g_tune_conv_waves == 8) hipLaunchKernelGGL((conv3d_igemm_bf16x3_kernel<128, 4, 2, NP, SC>), grid, dim3(512), smem, st, p);
  else hipLaunchKernelGGL((conv3d_igemm_bf16x3_kernel<128, 2, 2, NP, SC>), grid, dim3(256), smem, st, p);
}
void launch_igemm(const ConvParamsB &p, bool narrow, dim3 grid, size_t smem, hipStream_t st) {
  with_products(g_conv_products, [&](auto np) {
    if (p.scenes > 1) launch_igemm_np<np(), true>(p, narrow, grid, smem, st);
    else launch_igemm_np<np(), false>(p, narrow, grid, smem, st);
  });
}
}  // namespace sgc
