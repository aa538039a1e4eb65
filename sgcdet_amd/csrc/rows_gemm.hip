// Persistent, weight-stationary row GEMM on the bf16 matrix cores (gfx950):  y[M, N] = x[M, K] @ W^T (+ epilogue)
// with the 3-way bf16 split of conv3d.hip (a = a_hi + a_lo, products a_lo*b_hi + a_hi*b_lo + a_hi*b_hi, fp32 accumulate).
//
// What it is for: every nn.Linear of a level of the view transformation (value_proj over N*S pixel rows,
// the fused offset / logit projection and the K|V in-projection over the visible pairs, the q / out projections and the
// FFN over the selected voxels -- TU/deformable_cross_attention.py:417-436,826-833 of the reference, mmcv's FFN) and the
// 1x1x1 layers of the neck (necks/imvoxelnet.py:36-64).  All of them have K <= 512 and 10^3 .. 10^5 rows: on the
// tile-per-workgroup implicit-GEMM kernel a K = 256 tile is a serial chain (weight + activation prologue, 8 short
// K-steps with one global-load latency each, store-heavy epilogue) and ran at 0.3 of its HBM floor on the large calls
// and at a 17 us latency floor on the small ones.
//
// Structure (CDNA4-first, nothing of it exists in the reference, which calls cuBLAS through torch):
//   * a WAVE owns 32 output columns for the whole kernel and keeps their weights -- hi and lo planes, all of K -- as
//     MFMA B fragments in REGISTERS (K = 256: 128 VGPRs).  No weight traffic after the prologue, no B fragment reads
//     from LDS, no weight staging barrier.
//   * a workgroup (NW waves = NW * 32 columns) walks 32-row tiles of x persistently (tile = stripe + i * stripes);
//     the tile is loaded fp32 (16 B per lane, one row = one contiguous wave access), split once into bf16 hi / lo and
//     written to a double-buffered LDS image; loads run DEPTH tiles ahead in registers so that the HBM latency of
//     tile i + DEPTH is hidden behind the MFMA phases of tiles i .. i + DEPTH - 1.
//   * A fragments: one ds_read_b128 per plane per 16-deep k-step (row pitch K + 8 bf16: conflict-free), 3 MFMAs per
//     k-step on ONE accumulator chain (v_mfma_f32_32x32x16_bf16 issues back to back on a single chain).
//   * epilogue straight from the accumulator registers: in the 32x32 C layout a store instruction covers two rows x
//     32 columns = two whole 128-byte lines, so neither LDS staging nor a second barrier is needed; the stores of
//     tile i drain while tile i + 1 computes (they are issued after the loads of the tiles ahead, so the counted
//     vmcnt of the next conversion does not wait for them).
//   * ONE barrier per tile.
// A row's result does not depend on the number of rows, the grid or the tile a row falls in (fixed k order, no split-K):
// the host-counted and the device-counted (m_dev) launches are bit-identical, and so are eager and graph replays.
// The k order and the product order are those of conv3d_igemm_bf16x3_kernel: both kernels give identical bits.
#include <stdlib.h>

#include "rows_core.hpp"

namespace sgc {

// rows_diag    TIMING EXPERIMENTS ONLY, honoured only with SGC_DIAG=1 in the environment (results are then
//              invalid): bit 0 = stores dropped by the range check, bit 1 = loads dropped (zeros), bit 2 = no MFMA
// rows_cu_pct  see persistent_stripes (rows_core.hpp)
// rows_depth   8-wave form: 2 = two tiles in flight ahead of the one being multiplied, anything else = one; the 4-wave
//              form (two workgroups per CU) and the one-product modes run one ahead.  A staggered-halves form (waves 4-7
//              half a period behind waves 0-3) is gone: interleaved on the 204,800 x 256 -> 256 Linear it took 96-100 us
//              row-major against 90-93 for one tile ahead and 92-93 for two; the memory-only form of the kernel (no
//              MFMA) takes 80 us = 5.2 TB/s

struct RowsGemmParams {
  const float *x;              // [M, K] rows, row stride ldx floats
  int64_t ldx;
  const __bf16 *w_hi, *w_lo;   // [N][K]
  const float *scale, *shift;  // [N] or null
  const float *residual;       // [M, N] or null
  void *y;                     // [M, N] fp32; head-major [cam][head][s][cm] fp32 / bf16 when hm_cm > 0
  const int32_t *m_dev;        // live row count on the device or null
  int M, N;
  int relu;                    // 0 none, 1 relu(y + residual), 2 relu(y) + residual (conv3d.hip's modes)
  int hm_S, hm_cm, hm_bf16;
  int ncg;                     // column groups of NW * 32 columns
  int diag;                    // see g_tune_rows_diag
  int64_t y_bytes;             // head-major output: bytes of the whole buffer (the range the stores are checked against)
  float *zero_row;             // optional: N floats the launch sets to zero (the all-zero row behind the value map the wave gather
                               // points out-of-image corners at, sgc_linear_rows_zrow_bf16x3) -- by workgroup 0, before its tiles
  // GATHER form (sgc_pairs_geometry_linear_bf16x3): row r of the A operand is sum_k gw[r][k] * x[go[r][k]][:] -- the geometry-aware
  // sample of a visible pair, built while the tile is staged instead of written to HBM by one kernel and read back by this one
  const float *gw;             // [M][4] corner weights (bilinear * depth score)
  const int32_t *go;           // [M][4] row of x of each corner (a valid row also where the weight is 0)
  int64_t x_rows;              // rows of x (the whole feature map), GATHER only
};

// EPI: 0 = y = acc * scale + shift (optional relu), row-major; 1 = head-major fp32 store (value_proj); 2 = row-major with
// residual; 3 = head-major bf16 store (opt-in storage mode)
template <int K, int NW, int DEPTH, int EPI, int NP = 3, bool GATHER = false>   // NP: bf16 products per multiply-add (conv3d.hip: g_conv_products)
__global__ __launch_bounds__(NW * 64, 2) void rows_gemm_bf16x3_kernel(const RowsGemmParams p) {
  static_assert(!GATHER || (DEPTH == 1 && EPI == 0), "the gather form runs the lockstep schedule with the plain epilogue");
  constexpr int NT = NW * 64;
  constexpr int KS = K / 16;                       // 16-deep k-steps
  constexpr int K4 = K / 4;                        // float4 chunks per row
  constexpr int CH = RG_ROWS * K4 / NT;            // float4 chunks per thread per tile
  constexpr int PITCH = K + 8;                     // bf16 per LDS row: 16-byte pad -> conflict-free ds_read_b128 fragments
  constexpr int PLANE = RG_ROWS * PITCH;
  static_assert(RG_ROWS * K4 % NT == 0, "tile must deal evenly");
  extern __shared__ __attribute__((aligned(16))) unsigned char rg_smem[];
  __bf16 *lds = reinterpret_cast<__bf16 *>(rg_smem);   // [2 buffers][hi | lo][32][PITCH]

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int fr = lane & 31, fh = lane >> 5;
  if (p.zero_row && blockIdx.x == 0)
    for (int c = tid; c < p.N; c += NT) p.zero_row[c] = 0.f;
  const int Mrows = p.m_dev ? min(p.M, *p.m_dev) : p.M;
  const int ntiles = (Mrows + RG_ROWS - 1) / RG_ROWS;
  // blocks that share an XCD (equal blockIdx % 8) take the column groups of the same stripes: the second group's
  // read of a tile hits the L2 the first one filled.  Speed only.
  const int xcd = blockIdx.x & 7, loc = blockIdx.x >> 3;
  const int cg = loc % p.ncg, stripe = (loc / p.ncg) * 8 + xcd, nstripes = gridDim.x / p.ncg;
  if (stripe >= ntiles) return;
  const int col = (cg * NW + wid) * 32 + fr;       // this lane's output column

  // Buffer descriptors over the LIVE rows: a load past them returns zeros and a store past them is dropped by the
  // range check, so the tile loop has no branch (every wave issues the same memory instructions every iteration:
  // the compiler's counted vmcnt stays exact and the loads of the tiles ahead stay in flight across the waits).
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float *>(p.x), 0, (p.diag & 2) ? 0 : (int)(unsigned)((int64_t)(GATHER ? p.x_rows : Mrows) * p.ldx * 4), 0x00020000);
  // gather descriptors over the LIVE rows: past them both loads return zeros (weights 0, row 0: a valid row)
  const __amdgpu_buffer_rsrc_t gwr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(GATHER ? p.gw : p.x), 0,
                                                                        GATHER ? (int)(unsigned)((int64_t)Mrows * 16) : 0, 0x00020000);
  const __amdgpu_buffer_rsrc_t gor = __builtin_amdgcn_make_buffer_rsrc(const_cast<int32_t *>(GATHER ? p.go : (const int32_t *)p.x), 0,
                                                                        GATHER ? (int)(unsigned)((int64_t)Mrows * 16) : 0, 0x00020000);
  const __amdgpu_buffer_rsrc_t yr = __builtin_amdgcn_make_buffer_rsrc(
      p.y, 0, (p.diag & 1) ? 0 : (int)(unsigned)((EPI == 1 || EPI == 3) ? p.y_bytes : (int64_t)Mrows * p.N * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float *>(EPI == 2 ? p.residual : p.x), 0, (int)(unsigned)(EPI == 2 ? (int64_t)Mrows * p.N * 4 : 0), 0x00020000);

  bf16x8 bh[KS], bl[KS];
  rows_load_B<KS, NP>(p.w_hi, p.w_lo, col, fh, bh, bl);
  const float sc = p.scale ? p.scale[col] : 1.f, sh = p.shift ? p.shift[col] : 0.f;
  // relu modes (conv3d.hip's): 1 = relu(y + residual), 2 = relu(y) + residual; without a residual both are relu(y)
  const bool relu_before = EPI == 2 ? p.relu == 2 : p.relu != 0, relu_after = p.relu == 1;

  // Staging deal: all NT threads cooperate on the 32 rows of a tile.  Chunk i of a thread: f = tid + i * NT -> (row, 16-byte
  // chunk) = (tid / K4 + i * (NT / K4), tid % K4): one per-lane offset plus a SCALAR multiple of the row pitch per chunk (made
  // opaque per call: not hoisted into CH long-lived VGPRs)
  static_assert(NT % K4 == 0, "chunks of a thread must share their column");
  constexpr int RSTEP = NT / K4;
  const int ld_row = tid / K4, ld_c4 = tid % K4;
  // A tile in flight: CH 16-byte chunks per thread -- or, GATHER, the four corner rows' chunks and their weights.  The gather
  // branches below are this kernel's own copy of rows_gather_request / rows_gather_build (rows_core.hpp): built from the helpers the
  // K = 128 gather form waited for its corner rows in coarser steps and ran 4.5 % slower (profiles/r14_rows_core.md)
  constexpr int TV = GATHER ? 4 * CH + CH : CH;
  auto load_tile = [&](int t, float4 (&ra)[TV]) {
    int ldx4 = (int)p.ldx * 4;
    asm volatile("" : "+s"(ldx4));
    if constexpr (GATHER) {
#pragma unroll
      for (int i = 0; i < CH; ++i) {
        const unsigned doff = t < ntiles ? (unsigned)(t * RG_ROWS + ld_row + i * RSTEP) * 16u : RG_OOB;
        const u32x4 o = __builtin_amdgcn_raw_buffer_load_b128(gor, doff, 0, 0);
        const u32x4 w = __builtin_amdgcn_raw_buffer_load_b128(gwr, doff, 0, 0);
        ra[4 * CH + i] = make_float4(__uint_as_float(w[0]), __uint_as_float(w[1]), __uint_as_float(w[2]), __uint_as_float(w[3]));
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(xr, o[k] * (unsigned)ldx4 + ld_c4 * 16, 0, 0);
          ra[4 * i + k] = make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3]));
        }
      }
      return;
    }
    const unsigned base = t < ntiles ? (unsigned)(t * RG_ROWS + ld_row) * (unsigned)ldx4 + ld_c4 * 16 : RG_OOB;
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(xr, t < ntiles ? base + i * RSTEP * ldx4 : RG_OOB, 0, 0);
      ra[i] = make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3]));
    }
  };
  auto split_tile = [&](const float4 (&ra)[TV], int buf) {
    __bf16 *a_hi = lds + buf * 2 * PLANE;
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      float v[4];
      if constexpr (GATHER) {
        // the geometry sample's arithmetic, corner by corner in order, as rows_gather_build has it
        const float wk[4] = {ra[4 * CH + i].x, ra[4 * CH + i].y, ra[4 * CH + i].z, ra[4 * CH + i].w};
        v[0] = v[1] = v[2] = v[3] = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          v[0] = __builtin_fmaf(wk[k], ra[4 * i + k].x, v[0]); v[1] = __builtin_fmaf(wk[k], ra[4 * i + k].y, v[1]);
          v[2] = __builtin_fmaf(wk[k], ra[4 * i + k].z, v[2]); v[3] = __builtin_fmaf(wk[k], ra[4 * i + k].w, v[3]);
        }
      } else {
        v[0] = ra[i].x; v[1] = ra[i].y; v[2] = ra[i].z; v[3] = ra[i].w;
      }
      rows_stage_chunk<NP>(v, a_hi, PLANE, PITCH, ld_row + i * RSTEP, ld_c4);
    }
  };
  auto multiply = [&](int buf, f32x16 &acc) {
    rows_zero(acc);
    if (p.diag & 4) return;
    rows_multiply<KS, NP>(lds + buf * 2 * PLANE, PLANE, PITCH, 0, fr, fh, bh, bl, acc);
  };
  // head-major constants: row m = cam * S + s, column = head * cm + j  ->  [cam][head][s][cm]
  constexpr bool HM = EPI == 1 || EPI == 3;
  const int hm_heads = HM ? p.N / p.hm_cm : 1, hm_head = HM ? col / p.hm_cm : 0;
  const int hm_j = HM ? col - hm_head * p.hm_cm : 0;
  auto store_tile = [&](int t, const f32x16 &acc) {
    const int m0 = t * RG_ROWS;
    if constexpr (HM) {
      // rows of a tile are consecutive pixels of a camera: byte offset = base(tile, lane) + row * cm * es, plus one
      // constant jump for the rows past a camera border (hm_S >= 32: at most one border per tile)
      constexpr int es = EPI == 3 ? 2 : 4;
      const int cam0 = m0 / p.hm_S, s0 = m0 - cam0 * p.hm_S;       // scalar: one division per tile
      int cme = p.hm_cm * es;
      asm volatile("" : "+s"(cme));
      const unsigned base = (unsigned)(((cam0 * hm_heads + hm_head) * p.hm_S + s0 + 4 * fh) * p.hm_cm + hm_j) * es;
      const unsigned jump = (unsigned)((hm_heads - 1) * p.hm_S) * (unsigned)cme;
      const int rows_left = p.hm_S - s0 - 4 * fh;                  // rows of camera cam0 from this lane's first row on
      const int live = Mrows - m0 - 4 * fh;
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int r = acc_row(k);                                  // row - 4 * fh
        unsigned off = base + r * cme;
        off += r >= rows_left ? jump : 0u;
        off = r < live ? off : RG_OOB;
        const float v = acc[k] + sh;
        if constexpr (EPI == 3) __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(unsigned short, (__bf16)v), yr, off, 0, 0);
        else __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), yr, off, 0, 0);
      }
    } else {
      rows_store_rowmajor<EPI == 2>(acc, yr, rr, m0, fh, col, p.N, sc, sh, relu_before, relu_after);
    }
  };

  // Loop shape.  The compiler's counted s_waitcnt vmcnt(N) in front of a split must leave the loads of the tiles ahead
  // (and the stores of the tiles behind) in flight; its count is exact only where every path into a block has issued
  // the same vector-memory operations.  Hence: the first iteration (pair) is peeled, the loop has ONE exit at its
  // bottom (a break in the middle leaves a structurizer edge from the break to the header on which the registers
  // being waited for were "just reloaded": the waits then degrade to "all but the last 16"), and an odd last tile
  // runs in a tail copy behind the loop.
  f32x16 acc;
  const int n = (ntiles - stripe + nstripes - 1) / nstripes;     // tiles of this workgroup, >= 1
  int t = stripe;                                                // tile multiplied in the current iteration
  if constexpr (DEPTH == 2) {
    float4 r0[TV], r1[TV];                 // tile j of this workgroup lives in set j & 1 until it is split
    load_tile(t, r0);
    load_tile(t + nstripes, r1);
    split_tile(r0, 0);
    load_tile(t + 2 * nstripes, r0);
    __syncthreads();
    // even iteration: tile t in buffer 0, t + ns in r1, t + 2 ns in r0 (in flight); odd: the mirror image
    auto even = [&]() {
      multiply(0, acc);
      split_tile(r1, 1);
      load_tile(t + 3 * nstripes, r1);
      store_tile(t, acc);
      t += nstripes;
    };
    auto odd = [&]() {
      multiply(1, acc);
      split_tile(r0, 0);
      load_tile(t + 3 * nstripes, r0);
      store_tile(t, acc);
      t += nstripes;
    };
    even();
    if (n == 1) return;
    __syncthreads();
    odd();
    if (n == 2) return;
    __syncthreads();
    const int pairs = (n - 2) >> 1;
    for (int i = 0; i < pairs; ++i) {
      even();
      __syncthreads();
      odd();
      __syncthreads();
    }
    if (n & 1) even();
  } else {
    float4 r0[TV];
    int buf = 0;
    load_tile(t, r0);
    split_tile(r0, 0);
    load_tile(t + nstripes, r0);
    __syncthreads();
    auto step = [&]() {
      multiply(buf, acc);
      split_tile(r0, buf ^ 1);
      load_tile(t + 2 * nstripes, r0);
      store_tile(t, acc);
      t += nstripes;
      buf ^= 1;
    };
    step();
    for (int i = 1; i < n; ++i) {
      __syncthreads();
      step();
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Gather form at K = 256 (round 6): PRODUCER and CONSUMER waves.  In the kernel above a wave stages its share of the next tile AND
// multiplies the current one: at K = 256 with the gather that is the resident weights of its 32 columns (128 registers) plus a tile in
// flight of 8 chunks x 4 corner rows (128 registers + weights of the corners) -- 388 bytes of scratch per lane.  Here the two jobs
// sit on different waves of an 8-wave workgroup, so neither register set meets the other:
//   waves 0-3 (consumers)  hold the weights of 32 columns each (N = 128) and multiply tile i from LDS buffer i & 1, then store it;
//   waves 4-7 (producers)  request the corner rows of tile i + 2, build tile i + 1's rows (the sample's fmas), split them to bf16 hi | lo
//                          and write LDS buffer (i + 1) & 1;
// ONE barrier per tile: behind barrier i buffer i & 1 holds tile i and every consumer is done with buffer (i + 1) & 1 (tile i - 1).
// Same A values (the fmas of the geometry sample), same k order and product order as the plain kernel: bit-identical results.
// ---------------------------------------------------------------------------------------------
template <int K, int NP>
__global__ __launch_bounds__(512) void rows_gemm_gather_pc_kernel(const RowsGemmParams p) {
  constexpr int KS = K / 16, K4 = K / 4, PITCH = K + 8, PLANE = RG_ROWS * PITCH;
  constexpr int NTP = 256;                          // producer threads
  constexpr int CH = RG_ROWS * K4 / NTP;            // chunks per producer thread and tile (8 at K = 256)
  static_assert(RG_ROWS * K4 % NTP == 0 && NTP % K4 == 0, "tile must deal evenly");
  extern __shared__ __attribute__((aligned(16))) unsigned char rg_smem[];
  __bf16 *lds = reinterpret_cast<__bf16 *>(rg_smem);   // [2 buffers][hi | lo][32][PITCH]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int fr = lane & 31, fh = lane >> 5;
  const int Mrows = p.m_dev ? min(p.M, *p.m_dev) : p.M;
  const int ntiles = (Mrows + RG_ROWS - 1) / RG_ROWS;
  const int stripe = blockIdx.x, nstripes = gridDim.x;           // N == 128: one column group
  if (stripe >= ntiles) return;
  const int n = (ntiles - stripe + nstripes - 1) / nstripes;    // tiles of this workgroup, >= 1
  const bool consumer = wid < 4;
  if (consumer) {
    const int col = wid * 32 + fr;
    const __amdgpu_buffer_rsrc_t yr = __builtin_amdgcn_make_buffer_rsrc(p.y, 0, (int)(unsigned)((int64_t)Mrows * p.N * 4), 0x00020000);
    bf16x8 bh[KS], bl[KS];
    rows_load_B<KS, NP>(p.w_hi, p.w_lo, col, fh, bh, bl);
    const float sc = p.scale ? p.scale[col] : 1.f, sh = p.shift ? p.shift[col] : 0.f;
    int t = stripe;
    for (int i = 0; i < n; ++i, t += nstripes) {
      __syncthreads();                                           // tile i is in buffer i & 1
      f32x16 acc;
      rows_zero(acc);
      rows_multiply<KS, NP>(lds + (i & 1) * 2 * PLANE, PLANE, PITCH, 0, fr, fh, bh, bl, acc);
      rows_store_rowmajor<false>(acc, yr, yr, t * RG_ROWS, fh, col, p.N, sc, sh, false, false);
    }
    __syncthreads();                                             // the producers' last barrier
    return;
  }
  // ---------------- producers ----------------
  const int pt = tid - 256;
  const int ld_row = pt / K4, ld_c4 = pt % K4;
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.x), 0, (int)(unsigned)(p.x_rows * p.ldx * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t gwr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.gw), 0, (int)(unsigned)((int64_t)Mrows * 16), 0x00020000);
  const __amdgpu_buffer_rsrc_t gor = __builtin_amdgcn_make_buffer_rsrc(const_cast<int32_t *>(p.go), 0, (int)(unsigned)((int64_t)Mrows * 16), 0x00020000);
  float4 rv[4 * CH], rw[CH];
  auto request = [&](int t) { rows_gather_request<CH, NTP / K4>(xr, gor, gwr, t < ntiles, t * RG_ROWS + ld_row, ld_c4, p.ldx, rv, rw); };
  auto build = [&](int buf) { rows_gather_build<NP, CH, NTP / K4>(rv, rw, lds + buf * 2 * PLANE, PLANE, PITCH, ld_row, ld_c4); };
  int t = stripe;
  request(t);
  build(0);
  request(t + nstripes);
  for (int i = 0; i < n; ++i) {
    __syncthreads();                                             // tile i published; buffer (i + 1) & 1 is free
    if (i + 1 < n) {
      build((i + 1) & 1);
      request(t + (i + 2) * nstripes);
    }
  }
  __syncthreads();
}

// host: f(std::integral_constant<int, V>) for the V of the list that equals v -- a run-time value as a template argument
template <int... Vs, class F>
static int with_value(int v, F &&f) {
  int rc = SGC_EUNSUP;
  ((v == Vs ? (rc = f(std::integral_constant<int, Vs>{}), 0) : 0), ...);
  return rc;
}

// One dispatch over (K, NW, DEPTH, EPI) and the arithmetic mode.  Two tiles ahead exists for the 8-wave three-product form only.
static int launch_rows_gemm(const RowsGemmParams &p, int K, int nw, int grid, hipStream_t st) {
  const int epi = p.hm_cm > 0 ? (p.hm_bf16 ? 3 : 1) : p.residual ? 2 : 0;
  const int depth = (nw == 8 && g_tune_rows_depth == 2 && g_conv_products == 3) ? 2 : 1;
  return with_value<128, 256>(K, [&](auto k) {
    return with_value<4, 8>(nw, [&](auto w) {
      return with_value<1, 2>(depth, [&](auto d) {
        return with_value<0, 1, 2, 3>(epi, [&](auto e) {
          return with_products(g_conv_products, [&](auto np) -> int {
            constexpr int KK = decltype(k)::value, NW = decltype(w)::value, DEPTH = decltype(d)::value, EPI = decltype(e)::value, NP = decltype(np)::value;
            if constexpr (DEPTH == 2 && (NW != 8 || NP != 3)) {
              return SGC_EUNSUP;                                   // not reached: see depth above
            } else {
              static std::atomic<uint64_t> attr_done{0};           // one per kernel: a static of the generic lambda's instantiation
              ensure_dynamic_lds((const void *)rows_gemm_bf16x3_kernel<KK, NW, DEPTH, EPI, NP>, rows_lds_bytes(KK), attr_done);
              hipLaunchKernelGGL((rows_gemm_bf16x3_kernel<KK, NW, DEPTH, EPI, NP>), dim3(grid), dim3(NW * 64), rows_lds_bytes(KK), st, p);
              return check_launch("rows_gemm_bf16x3_kernel");
            }
          });
        });
      });
    });
  });
}

// Can the persistent kernel take this GEMM?  K in {128, 256}; whole 128-column groups; 32-bit byte offsets into x and y;
// head-major: a camera holds at least one tile (the store handles one camera border per tile) and a wave's 32 columns
// are whole heads or part of one.
bool rows_gemm_supported(int K, int N, int hm_cm, int hm_S, int64_t rows, int64_t ldx) {
  if (!g_tune_rows_gemm) return false;
  if (K != 128 && K != 256) return false;
  if (N <= 0 || N % 128) return false;
  if (rows <= 0 || (rows + 64) * ldx * 4 >= (int64_t)RG_OOB || (rows + 64) * N * 4 >= (int64_t)RG_OOB) return false;
  if (hm_cm > 0 && (128 % hm_cm || hm_S < RG_ROWS)) return false;      // per-lane head / offset arithmetic: any hm_cm | 128
  return true;
}

int device_cus() {      // also conv3d.hip (the wave-quantisation model of the halo kernel)
  static std::atomic<int> cached{0};
  int c = cached.load(std::memory_order_relaxed);
  if (c > 0) return c;
  int dev = 0;
  hipDeviceProp_t prop;
  c = 256;
  if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
    c = prop.multiProcessorCount;
  cached.store(c, std::memory_order_relaxed);
  return c;
}

// Gather form (see RowsGemmParams): N == 128 columns; K == 128 on the kernel above (four waves, the lockstep schedule), K == 256 on
// the producer / consumer kernel (rows_gemm_gather_pc_kernel).
bool rows_gemm_gather_supported(int K, int N, int64_t x_rows, int64_t rows) {
  return rows_gemm_supported(K, N, 0, 0, rows, K) && N == 128 && x_rows > 0 && (x_rows + 1) * K * 4 < (int64_t)RG_OOB;
}

int rows_gemm_gather_launch(const float *x, int64_t x_rows, const float *gw, const int32_t *go, const uint16_t *w_hi, const uint16_t *w_lo,
                            const float *shift, float *y, const int32_t *m_dev, int M, int K, int N, hipStream_t st) {
  RowsGemmParams p = {};
  p.x = x; p.ldx = K; p.x_rows = x_rows; p.gw = gw; p.go = go;
  p.w_hi = reinterpret_cast<const __bf16 *>(w_hi); p.w_lo = reinterpret_cast<const __bf16 *>(w_lo);
  p.shift = shift; p.y = y; p.m_dev = m_dev; p.M = M; p.N = N;
  p.y_bytes = (int64_t)M * N * 4;
  p.ncg = 1;                                                    // N == 128: one column group
  const int cap_tiles = ceil_div(M, RG_ROWS);
  // K == 256: one 8-wave producer / consumer workgroup per CU; K == 128: two 4-wave workgroups of the lockstep kernel
  return with_products(g_conv_products, [&](auto np) {
    static std::atomic<uint64_t> attr_done[2];                  // per NP: statics of the generic lambda's instantiation
    if (K == 256) {
      ensure_dynamic_lds((const void *)rows_gemm_gather_pc_kernel<256, np()>, rows_lds_bytes(256), attr_done[0]);
      hipLaunchKernelGGL((rows_gemm_gather_pc_kernel<256, np()>), dim3(persistent_stripes(cap_tiles, 1, 1)), dim3(512), rows_lds_bytes(256), st, p);
      return check_launch("rows_gemm_gather_pc_kernel");
    }
    ensure_dynamic_lds((const void *)rows_gemm_bf16x3_kernel<128, 4, 1, 0, np(), true>, rows_lds_bytes(128), attr_done[1]);
    hipLaunchKernelGGL((rows_gemm_bf16x3_kernel<128, 4, 1, 0, np(), true>), dim3(persistent_stripes(cap_tiles, 2, 1)), dim3(256), rows_lds_bytes(128), st, p);
    return check_launch("rows_gemm_bf16x3_kernel (gather)");
  });
}

int rows_gemm_launch(const float *x, int64_t ldx, const uint16_t *w_hi, const uint16_t *w_lo, const float *scale,
                     const float *shift, const float *residual, void *y, const int32_t *m_dev, int M, int K, int N, int relu,
                     int hm_S, int hm_cm, int hm_bf16, hipStream_t st, float *zero_row) {
  RowsGemmParams p = {};
  p.zero_row = zero_row;
  p.x = x; p.ldx = ldx;
  p.w_hi = reinterpret_cast<const __bf16 *>(w_hi); p.w_lo = reinterpret_cast<const __bf16 *>(w_lo);
  p.scale = scale; p.shift = shift; p.residual = residual; p.y = y; p.m_dev = m_dev;
  p.M = M; p.N = N; p.relu = relu;
  p.hm_S = hm_S; p.hm_cm = hm_cm; p.hm_bf16 = hm_bf16;
  p.y_bytes = (int64_t)M * N * (hm_bf16 ? 2 : 4);
  {
    static const bool diag_ok = getenv("SGC_DIAG") && atoi(getenv("SGC_DIAG")) == 1;
    p.diag = diag_ok ? g_tune_rows_diag : 0;
  }
  const int nw = (N % 256 == 0) ? 8 : 4;                        // one 8-wave workgroup or two 4-wave workgroups per CU
  p.ncg = N / (nw * 32);
  const int stripes = persistent_stripes(ceil_div(M, RG_ROWS), nw == 8 ? 1 : 2, p.ncg);
  return launch_rows_gemm(p, K, nw, stripes * p.ncg, st);
}

}  // namespace sgc
