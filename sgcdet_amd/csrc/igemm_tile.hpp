// The bf16x3 implicit-GEMM tile core: what conv3d_igemm_bf16x3_kernel (volumes) and conv2d_ex_kernel (images) share.
//
// A workgroup of WM x WN waves owns a tile of 128 GEMM rows x BN columns and walks K in steps of 32: the A chunk of a step is
// gathered from a channels-last tensor, the B chunk from the [tap][Cout][Cin] weight planes, both through buffer descriptors (an
// offset past the tensor reads zeros, so the loop has no branch); fp32 activations are split hi | lo while they are staged into
// LDS, the weights were split on the host.  Loads of step s + 1 are issued before the MFMAs of step s and written to the other
// LDS buffer after them: one barrier per step.  The finished tile goes through LDS once and leaves as 16-byte row pieces.
//
// The core knows nothing of geometry.  A kernel supplies
//   addressing   aoff[i]: byte offset of the input row behind A chunk i under the tap being loaded (OOB: no such row), rewritten
//                per TAP; and per STEP the two uniform offsets of load() -- the channel chunk, and for the weights the tap's slab;
//   store policy where row rl, column quad q of the staged tile (c_quad) goes, with epilogue4() for the arithmetic on the way.
// Timing builds (diag.hpp) pass SGC_TILE_SKIP as SKIP; at SKIP = 0 none of that code is compiled.
#pragma once
#include "conv_common.hpp"
#include "mma.hpp"

namespace sgc {

__device__ __forceinline__ __amdgpu_buffer_rsrc_t tile_rsrc(const void *ptr, int64_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(ptr), 0, (int)(unsigned)bytes, 0x00020000);
}

__device__ __forceinline__ float4 relu4(float4 v) { return relu_nan(v); }

// v * scale[col ..] + shift[col ..]; relu; + residual[roff ..]; relu -- every vector optional, 16 bytes at a time
__device__ __forceinline__ float4 epilogue4(float4 v, int col, const float *scale, const float *shift, bool relu_before,
                                            const float *residual, int64_t roff, bool relu_after) {
  if (scale) {
    const float4 sc4 = *reinterpret_cast<const float4 *>(scale + col);
    v.x *= sc4.x; v.y *= sc4.y; v.z *= sc4.z; v.w *= sc4.w;
  }
  if (shift) {
    const float4 sh4 = *reinterpret_cast<const float4 *>(shift + col);
    v.x += sh4.x; v.y += sh4.y; v.z += sh4.z; v.w += sh4.w;
  }
  if (relu_before) v = relu4(v);
  if (residual) {
    const float4 r4 = *reinterpret_cast<const float4 *>(residual + roff);
    v.x += r4.x; v.y += r4.y; v.z += r4.z; v.w += r4.w;
  }
  if (relu_after) v = relu4(v);
  return v;
}

// NP: bf16 products per multiply-add (mma.hpp)
template <int BN, int WM, int WN, int NP>
struct IgemmTile {
  static constexpr int NT = WM * WN * 64;                       // threads per workgroup (256 or 512)
  static constexpr int TM = BM / WM / 32, TN = BN / WN / 32;    // MFMA tiles of a wave
  static constexpr int ACH = BM * 8 / NT, AROWS = NT / 8;       // float4 A chunks per thread: rows r0 + AROWS i
  static constexpr int BCH = (BN * 4 + NT - 1) / NT, BROWS = NT / 4;   // 16-byte weight chunks per thread per plane: rows br0 + BROWS i
  static constexpr bool B_PARTIAL = BCH * BROWS > BN;           // the 32-column tile: half the threads carry no weight chunk
  // per buffer: A_hi[BM][LDKH], A_lo[BM][LDKH], B_hi[BN][LDKH], B_lo[BN][LDKH]
  static constexpr int A_PLANE = BM * LDKH, B_PLANE = BN * LDKH, BUF = 2 * A_PLANE + 2 * B_PLANE;
  static constexpr int LDC = BN + 8;                            // floats per staged C row: rows r and r + 4 (lane halves) 32 banks apart
  static constexpr int C4 = BN / 4;
  // the 512-thread fp32-faithful form reads a column tile's B fragments right before its products (see compute()).  This answers
  // one compiler's register allocation, not the hardware: after a toolchain change, re-make the resource table of
  // profiles/r11_tile_core_resources.md and see whether the switch is still needed, or needed elsewhere
  static constexpr bool READS_STAY = NT == 512 && NP == 3;
  static constexpr unsigned OOB = 0xfffffff0u;
  static_assert(2 * BUF * 2 == igemm_tile_lds_bytes(BN) && BM * LDC * 4 <= igemm_tile_lds_bytes(BN), "LDS plan");

  __bf16 *const base;                                           // the workgroup's dynamic LDS
  const int tid, lane, wid, wm, wn;
  const int fr, fh;                                             // fragment row and k-half of this lane
  // Staging rows are dealt so that the lanes one LDS write pass covers (32 lanes x 8 B for A, 16 lanes x 16 B for B)
  // sit in rows {r, r+4, r+8, r+12}: with the 20-dword row pitch those start 16 banks apart and tile all 64 banks;
  // consecutive rows (the plain tid >> 3 deal) overlap by 12 banks and every pass took two turns.
  const int c4, r0;                                             // A: row r0 + AROWS i, 4 floats at c4 * 4
  const int bc, br0;                                            // B: row br0 + BROWS i, 8 bf16 at bc * 8
  __amdgpu_buffer_rsrc_t xr, whr, wlr;
  unsigned aoff[ACH];                                           // the caller's: input rows under the tap being loaded
  unsigned boff[BCH];                                           // this thread's weight rows: fixed for the whole kernel
  float4 ra[ACH];
  uint4 rbh[BCH], rbl[BCH];
  f32x16 acc[TM][TN];

  __device__ __forceinline__ IgemmTile(void *smem, int t)
      : base(reinterpret_cast<__bf16 *>(smem)), tid(t), lane(t & 63), wid(t >> 6), wm(wid / WN), wn(wid % WN), fr(lane & 31), fh(lane >> 5), c4(t & 7),
        r0(16 * (wid >> 1) + 2 * (wid & 1) + (((t >> 3) & 7) >> 2) + 4 * (((t >> 3) & 7) & 3)), bc(t & 3),
        br0(16 * wid + (((t >> 2) & 15) >> 2) + 4 * (((t >> 2) & 15) & 3)) {}

  __device__ __forceinline__ int a_row(int i) const { return r0 + AROWS * i; }
  __device__ __forceinline__ int b_row(int i) const { return br0 + BROWS * i; }
  __device__ __forceinline__ bool b_row_ok(int i) const { return !B_PARTIAL || b_row(i) < BN; }

  __device__ __forceinline__ void bind(const float *x, int64_t x_bytes, const __bf16 *w_hi, const __bf16 *w_lo, int64_t w_bytes,
                                       int n0, int Cout, int Cin) {
    xr = tile_rsrc(x, x_bytes);
    whr = tile_rsrc(w_hi, w_bytes);
    wlr = tile_rsrc(w_lo, w_bytes);
#pragma unroll
    for (int i = 0; i < BCH; ++i) {
      const int n = n0 + b_row(i);
      boff[i] = (b_row_ok(i) && n < Cout) ? (unsigned)(n * Cin + bc * 8) * 2u : OOB;
    }
  }

  // global loads of one K step into registers
  template <int SKIP = 0>
  __device__ __forceinline__ void load(int soff_a, int soff_b) {
#pragma unroll
    for (int i = 0; i < ACH; ++i) {
      if constexpr ((SKIP & 2) != 0) break;               // timing builds: no input loads
      const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(xr, aoff[i], soff_a, 0);
      ra[i] = make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3]));
    }
#pragma unroll
    for (int i = 0; i < BCH; ++i) {
      if constexpr ((SKIP & 4) != 0) break;               // timing builds: no weight loads
      const u32x4 h = __builtin_amdgcn_raw_buffer_load_b128(whr, boff[i], soff_b, 0);
      rbh[i] = make_uint4(h[0], h[1], h[2], h[3]);
      if constexpr (NP == 3) {
        const u32x4 l = __builtin_amdgcn_raw_buffer_load_b128(wlr, boff[i], soff_b, 0);
        rbl[i] = make_uint4(l[0], l[1], l[2], l[3]);
      } else {
        rbl[i] = make_uint4(0, 0, 0, 0);
      }
    }
  }

  // operand split and LDS stores of the loaded step
  __device__ __forceinline__ void store(int buf) {
    __bf16 *a_hi = base + buf * BUF, *a_lo = a_hi + A_PLANE, *b_hi = a_lo + A_PLANE, *b_lo = b_hi + B_PLANE;
#pragma unroll
    for (int i = 0; i < ACH; ++i) {
      const float v[4] = {ra[i].x, ra[i].y, ra[i].z, ra[i].w};
      bf16x4 h, l;
      split4<NP>(v, h, l);
      const int o = a_row(i) * LDKH + c4 * 4;
      *reinterpret_cast<bf16x4 *>(a_hi + o) = h;
      if constexpr (NP == 3) *reinterpret_cast<bf16x4 *>(a_lo + o) = l;
    }
#pragma unroll
    for (int i = 0; i < BCH; ++i) {
      if (!b_row_ok(i)) continue;
      const int o = b_row(i) * LDKH + bc * 8;
      *reinterpret_cast<uint4 *>(b_hi + o) = rbh[i];
      if constexpr (NP == 3) *reinterpret_cast<uint4 *>(b_lo + o) = rbl[i];
    }
  }

  // fragment reads and MFMAs of the step staged in buffer buf
  template <int SKIP = 0>
  __device__ __forceinline__ void compute(int buf) {
    const __bf16 *a_hi = base + buf * BUF + (wm * (BM / WM) + fr) * LDKH + fh * 8;
    const __bf16 *a_lo = a_hi + A_PLANE;
    const __bf16 *b_hi = base + buf * BUF + 2 * A_PLANE + (wn * (BN / WN) + fr) * LDKH + fh * 8;
    const __bf16 *b_lo = b_hi + B_PLANE;
#pragma unroll
    for (int kk = 0; kk < BK / 16; ++kk) {
      bf16x8 ah[TM], al[TM], bh[TN], bl[TN];
      auto read_b = [&](int j) {
        bh[j] = *reinterpret_cast<const bf16x8 *>(b_hi + j * 32 * LDKH + kk * 16);
        if constexpr (NP == 3) bl[j] = *reinterpret_cast<const bf16x8 *>(b_lo + j * 32 * LDKH + kk * 16);
      };
      if constexpr ((SKIP & 16) != 0) {                    // timing builds: no fragment reads
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
        if constexpr (!READS_STAY || (SKIP & 1) != 0) {           // (the no-MFMA timing build keeps every read at the top)
#pragma unroll
          for (int j = 0; j < TN; ++j) read_b(j);
        }
      }
      if constexpr ((SKIP & 1) != 0) {                     // timing builds: everything but the MFMAs
#pragma unroll
        for (int i = 0; i < TM; ++i) asm volatile("" ::"v"(ah[i]), "v"(al[i]));
#pragma unroll
        for (int j = 0; j < TN; ++j) asm volatile("" ::"v"(bh[j]), "v"(bl[j]));
        continue;
      }
      if constexpr (READS_STAY) {
        // one column tile at a time: its B fragments are read behind the products of the tile before it (16 fragment registers
        // instead of 36 with every read of the step hoisted to its top, which costs the 512-thread form a wave of occupancy)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          if constexpr ((SKIP & 16) == 0) read_b(j);
#pragma unroll
          for (int i = 0; i < TM; ++i) acc[i][j] = mma_split<NP>(ah[i], al[i], bh[j], bl[j], acc[i][j]);
          __builtin_amdgcn_sched_barrier(0);
        }
        continue;
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = mma_split<NP>(ah[i], al[i], bh[j], bl[j], acc[i][j]);
    }
  }

  // The double-buffered K loop over nsteps >= 1 steps.  load_step() is the caller's: it calls load() with the offsets of the
  // next step and moves on to the step after it.  `staged` is false only in timing builds that skip the split and the LDS stores.
  // (a second register stage -- loads of step s + 2 issued before the MFMAs of step s -- was tried: 156 VGPRs and
  //  one workgroup per CU, or 128 with spills; 404 -> 507 us on the per-tap 90 GF layer, 143 -> 180-200 us on the
  //  split-K layers.  Two resident workgroups at 88 VGPRs hide more latency than the deeper prefetch.)
  template <int SKIP = 0, class LoadStep>
  __device__ __forceinline__ void run(int nsteps, LoadStep &&load_step, bool staged = true) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int k = 0; k < 16; ++k) acc[i][j][k] = 0.f;
    load_step();
    if (staged) store(0);
    __syncthreads();
    for (int s = 0; s < nsteps; ++s) {
      const int buf = s & 1;
      if (s + 1 < nsteps) load_step();
      compute<SKIP>(buf);
      if (s + 1 < nsteps && staged) store(buf ^ 1);      // the other buffer was last read in step s - 1, before the barrier below
      if constexpr ((SKIP & 32) == 0) __syncthreads();     // timing builds: no barrier per step
    }
  }

  // Epilogue through LDS: in the MFMA layout a lane owns ONE column and 16 rows of a tile, i.e. 4-byte stores, 32 per
  // lane -- store-issue bound (PMC on the K = 256 Linears: waves parked 54 % of their cycles, matrix pipe busy 20 %).
  // The staging buffers are free after the loop's last barrier: the tile goes to LDS once, as [BM][LDC] floats, and
  // leaves as 16-byte row-contiguous stores.
  __device__ __forceinline__ float *scatter() {
    float *cs = reinterpret_cast<float *>(base);
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int k = 0; k < 16; ++k)
          cs[(wm * (BM / WM) + i * 32 + acc_row(k) + 4 * (lane >> 5)) * LDC + wn * (BN / WN) + j * 32 + (lane & 31)] =
              acc[i][j][k];
    __syncthreads();
    return cs;
  }
  // columns [4 q, 4 q + 4) of row rl of the staged tile
  static __device__ __forceinline__ float4 *c_quad(float *cs, int rl, int q) { return reinterpret_cast<float4 *>(cs + rl * LDC + q * 4); }
};

}  // namespace sgc
