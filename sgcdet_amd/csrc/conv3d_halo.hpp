// Halo-resident 3x3x3 / 3x3 stride-1 convolution on MFMA for gfx950 (bf16x3 arithmetic of mma.hpp): the kernel and the launcher of one
// instantiation.  The instantiations are spread over three translation units so that they compile side by side -- conv3d_halo.hip
// (deep 3-D bricks, and the dispatch on the plan), conv3d_halo_z4.hip (3-D bricks of depth 4), conv3d_halo_2d.hip (2-D and Winograd
// forms); every (brick, column tile, form) lives in exactly one of them.
#pragma once
#include "conv_common.hpp"
#include "mma.hpp"
#include "diag.hpp"
#include "tuning.hpp"

namespace sgc {

// ---------------------------------------------------------------------------------------------
// v2 for the 3x3x3 stride-1 layers (90 % of the neck's FLOPs): halo-resident A.
// A workgroup owns a brick of BX*BY*BZ = 256 output voxels.  For one 32-channel slice it stages the
// brick's input HALO ((BX+2)(BY+2)(BZ+2) rows, split to bf16 hi/lo once) in LDS and then walks the 27
// taps with the SAME staged rows: the A fragment of output row r at tap t is the halo row
// hr(r) + toff(t), a wave-uniform offset on a per-lane base.  Only the weights stream (16 KB hi+lo per
// tap, double buffered).  L2->LDS traffic per MAC drops 3.4x against the per-tap gather above, and the
// fp32->bf16 split runs once per halo element instead of 27 times.
// 512 threads = 8 waves as 4 (M) x 2 (N), wave tile 64 x 64, BN = 128 output channels.
// LDS: A 2 planes x HROWS x 80 B (<= 104 KB) + B 2 buffers x 2 planes x 128 x 80 B (41 KB).
// ---------------------------------------------------------------------------------------------
// z-pitch (in rows) of the halo image in LDS: the smallest pitch >= BZ + 2 for which every 32-row MFMA tile
// of the brick holds each halo-row residue mod 16 exactly twice (checked offline for the three brick shapes:
// 18 for BZ = 16, 12 for BZ = 8, 6 for BZ = 4) -- the precondition of the conflict-free lane assignment.
// BZ = 10 (the 2 images x 10 x 10 Winograd brick, 200 rows + 56 pad rows) has no such pitch: tools/halo_pitch_enum.py replays the
// kernel's greedy assignment for the pitches 12..16 and counts the 16-lane ds_read_b128 groups (of 16) that keep a two-way
// conflict -- 13, 7, 12, 13, 12 -- so 13 it is; the LDS plan is the 139 KB epilogue tile at every one of them.
// MF = 16 (the Winograd bricks on v_mfma_f32_16x16x32_bf16, see the kernel): rows of 96 bytes, on which a 16-lane read group is
// conflict-free iff each of its two 8-lane halves holds rows distinct mod 8.  A z run of 8 is that at any pitch (12 is kept);
// BZ = 10 keeps 12, 10, 6, 12, 12 conflicting groups of 32 at the pitches 12..16 (halo_pitch_enum.py --mfma16) -- 14.
__host__ __device__ constexpr int halo_pitch(int BZ, int MF = 32) { return BZ == 8 ? 12 : BZ == 10 ? (MF == 16 ? 14 : 13) : BZ + 2; }
__host__ __device__ constexpr int halo_ldk(int MF) { return MF == 16 ? BK + 16 : LDKH; }   // bf16 per LDS row
__host__ __device__ constexpr size_t halo_tab_offset(int lrows, int mrows = 256, int bnv = 128, int ldk = LDKH) {
  const size_t planes = (size_t)(2 * lrows + 2 * 2 * bnv) * ldk * sizeof(uint16_t);   // A hi|lo + 2 x B hi|lo
  const size_t stage = (size_t)mrows * (bnv + 8) * sizeof(float);                      // epilogue tile [MROWS][BNV + 8]
  return planes > stage ? planes : stage;
}

// BNV: output columns per workgroup, 128 (wave tile 64 x 64) or 64 (wave tile 64 x 32: the head's 28 / 32-column layers, which
// otherwise spend three quarters of their matrix work on padding columns).
// TD: 2-D form (sgc_conv2d_nhwc_bf16x3: the FPN's 3 x 3 output convolutions) -- the grid is (image, row, column),
// a brick is BX images x BY x BZ pixels, there is no halo and no tap along x: 9 taps, (BY + 2)(BZ + 2) halo rows per image.
// Bricks: 1 x 16 x 16 (324 halo rows) and 4 x 8 x 8 (400) of 256 pixels; 2 x 10 x 10 (288 halo rows, Winograd stack only) of 200 pixels
// in 256 matrix rows -- the 20 x 20 and 10 x 10 slices of the neck, which 8 x 8 pixel bricks cover with 576 pixels for 400 / not at all.
// STG: software-pipelined schedule with the barrier in the MIDDLE of a tap (round 4; the body explains the hazards).  The
// lockstep form (STG = false) put the barrier at the end of a tap: behind it every wave first had to fetch the freshly published
// weight fragments from LDS (MFMA pipe idle for an LDS round trip with 96 reads queued), and in front of it every wave waited
// for its two weight ds_write_b128 to drain.  Timing builds (tools/halo_skip.py, 90-GF layer, warm): 232 us as shipped, 195
// without the weight ds_writes, 215 without the barrier, 183 without the weight loads and writes, 179 with nothing but the MFMAs
// and the loop -- the weight path cost a fifth of the kernel although it moves 16 KB per tap.  With the barrier at mid-tap the
// operands of BOTH k-halves are in registers before the MFMAs that use them are reached, the weight tile is written a
// half-tap before the barrier that publishes it, and nothing but wave skew is left at the barrier.  Every accumulator still
// sees (tap, k-half, product) in the same order: bit-identical to the lockstep form.
// WZ (2-D form only): the image stack is VIRTUAL -- image k * J + j, pixel (xx, yy) is the Winograd F(2,3)-along-z input transform
// t_k of the raw volume p.x [rows][cols][Z = 2 J][Cin] at the output pair j (sgc_conv3d_winograd_z_bf16x3): every staged chunk is
// loaded from TWO voxel rows and combined (a - b, or a + b for k = 1) in front of the hi / lo split; no transformed copy exists.
// MF (Winograd bricks only, `wz_mfma`): the MFMA shape, 32 = v_mfma_f32_32x32x16 as everywhere else, 16 = v_mfma_f32_16x16x32.  Same
// waves, same 64 x 64 wave tile (4 x 4 tiles, sixteen 4-register accumulators), same staging, barriers and tap unrolling; a tap
// is ONE k-step, so the two operand sets of the pipelined schedule are the A fragments of row tiles 0-1 and 2-3 over one set of B
// fragments, refilled tile by tile behind the last MFMA that reads each.  What differs: the LDS rows are 96 bytes (halo_pitch), the
// lane -> voxel table deals rows by residue mod 8, the weight rows a thread stages, the fragment reads, the product loop and the
// accumulator -> LDS-tile store of the epilogue.  The instruction sums differently: last-bit differences against MF = 32.
// SC: the launch holds a batch of scenes (p.scenes > 1, sgc_conv3d_cl_bf16x3_batched; 3-D forms only).  An instantiation of its own:
// the scene-less kernel -- the one inference runs -- is the code it always was, only a batch pays for the scene decode.
template <int BX, int BY, int BZ, int BNV = 128, int NP = 3, bool TD = false, bool STG = true, bool WZ = false, int MF = 32, bool SC = false>
__global__ __launch_bounds__(512) void conv3d_halo_bf16x3_kernel(const ConvParamsB p) {
  static_assert(!WZ || TD, "the virtual Winograd stack is a 2-D form");
  static_assert(!SC || (!TD && !WZ), "the scene axis exists in the 3-D forms only");
  static_assert(MF == 32 || (MF == 16 && WZ && STG && BNV == 128 && BX * BY * BZ <= 256), "the 16x16x32 form: pipelined Winograd bricks only");
  constexpr int LDKH = halo_ldk(MF);                    // bf16 per LDS row (shadows the 80-byte rows of conv_common.hpp)
  constexpr int NTAP = TD ? 9 : 27, XO = TD ? 0 : 1;    // taps; halo width along x
  // MFMA rows of the brick: 256 for the standard bricks; a brick with another voxel count (a whole small grid: 10 x 10 x 4, the
  // coarsest config-2 scale) is padded to a multiple of 128 rows (4 wave rows x 32) -- pad rows work on voxel 0 and are dropped
  // wave layout: WMV (rows) x WNV (columns) = 8 waves.  4 x 2 for 128- and 64-column tiles; 8 x 1 for the 32-column tile of the
  // head's fused 28-column convolution (round 5: on 64 columns more than half of its matrix work was padding)
  constexpr int WNV = BNV >= 64 ? 2 : 1, WMV = 8 / WNV;
  constexpr int NVOX = BX * BY * BZ, MROWS = (NVOX + 32 * WMV - 1) / (32 * WMV) * (32 * WMV);
  constexpr int RT = MROWS / (32 * WMV);                // 32-row tiles per wave
  constexpr unsigned short kPadRow = 0x8000;            // vox_tab flag of a pad row
  static_assert(MROWS <= 512, "one table entry per thread");
  constexpr int TN = BNV / (32 * WNV), WCOL = BNV / WNV; // 32-column tiles per wave, columns per wave
  constexpr int HX = BX + 2 * XO, HY = BY + 2, HZ = BZ + 2, HROWS = HX * HY * HZ;
  constexpr int HZP = halo_pitch(BZ, MF), LROWS = HX * HY * HZP;   // z-pitch of the LDS image (see halo_pitch)
  constexpr int NT = 512;
  constexpr int NA = (HROWS * 8 + NT - 1) / NT;     // float4 halo chunks per thread
  constexpr int A_PLANE = LROWS * LDKH, B_PLANE = BNV * LDKH;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_h[];
  __bf16 *A_hi = reinterpret_cast<__bf16 *>(smem_h), *A_lo = A_hi + A_PLANE;
  __bf16 *Bbase = A_lo + A_PLANE;                   // [2][hi|lo][BNV][LDKH]
  // [8 tiles][32 lanes], behind both the staging planes and the epilogue's output tile that later overlays them
  unsigned short *vox_tab = reinterpret_cast<unsigned short *>(smem_h + halo_tab_offset(LROWS, MROWS, MROWS > 256 ? BNV : 128, LDKH));

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WNV, wn = wid % WNV;
  const int nby = (p.gy + BY - 1) / BY, nbz = (p.gz + BZ - 1) / BZ;
  // scene of this workgroup (sgc_conv3d_cl_bf16x3_batched launches scenes * bricks of them): its rows start at in0 / orow0, the
  // halo test below is against the scene's own grid, so rows of a neighbouring scene are never staged
  int bid = blockIdx.x;
  int in0 = 0;
  if constexpr (SC) {
    const int per_scene = ((p.gx + BX - 1) / BX) * nby * nbz;
    const int scene = bid / per_scene;
    bid -= scene * per_scene;
    in0 = scene * (p.ix * p.iy * p.iz);
  }
  const int bk = bid % nbz; bid /= nbz;
  const int bj = bid % nby; const int bi = bid / nby;
  const int X0 = bi * BX, Y0 = bj * BY, Z0 = bk * BZ;
  const int n0 = blockIdx.y * BNV;
  const int nchunks = p.Cin / BK;
  const int per = (nchunks + p.splitk - 1) / p.splitk;
  const int c_lo = blockIdx.z * per, c_hi = min(nchunks, c_lo + per);
  if (c_lo >= c_hi) return;

  // Which output voxel of the brick each MFMA row (= lane & 31 of a 32-row tile) works on.  ds_read_b128
  // serves a wave in four fixed 16-lane groups ({0-3,12-15,20-27}, {4-11,16-19,28-31}, +32) over 64 banks,
  // i.e. with the 80-byte row stride a group is conflict-free iff its halo rows are distinct mod 16.  The
  // natural order (lane = z-run position) is not: a tile spans several z-runs whose halo rows are HZP apart
  // (measured: 38 % of the LDS cycles of this kernel were bank-conflict cycles).  Every tile holds each
  // residue exactly twice (halo_pitch guarantees it), so lane l takes the first (l < 16) or second voxel of
  // the tile whose halo row is == l mod 16 -- any assignment works as long as the epilogue uses the same one.
  // (Other brick shapes -- a whole small grid -- do not keep that precondition for every tile: the greedy pass below IS the
  //  assignment above wherever it exists and degrades to a few two-way conflicts elsewhere, never to a wrong permutation.)
  // One wave per tile, lane j = row j of the tile (both wave halves compute the same; the upper half does not store): a row whose
  // residue it is the first / second to carry takes slot residue / 16 + residue; further rows of a crowded residue fill the
  // slots of the residues that came short, in order.
  // MF = 16: lane l of a 16-row tile reads chunk l >> 4 of row l & 15, so a 16-lane group holds eight rows at chunk c (lanes
  // 0-3, 12-15 of the tile) and the other eight at chunk c + 1 (lanes 4-11).  On 96-byte rows a lane sits at (6 row + chunk) mod 16
  // in 16-byte units -- the parity of its chunk -- so a group is conflict-free iff each half's rows are distinct mod 8, under any
  // tap offset.  (On 80-byte rows no assignment is: 5 row takes every residue over a tile, and the chunk-(c + 1) half would have to
  // map onto itself under + 1.)  The same greedy pass over 32 rows, then: residues mod 8, four halves (two 16-row tiles), the row
  // that is the k-th to carry its residue goes to half k.
  constexpr int RES = MF == 16 ? 8 : 16, RANKS = 32 / RES;           // residues; rows per residue a 32-row table segment seats
  const auto seat = [](int k, int q) {                               // slot of the k-th row with residue q
    if constexpr (MF == 16) return (k >> 1) * 16 + ((k & 1) ? 4 + q : q < 4 ? q : q + 8);
    else return k * 16 + q;
  };
  for (int t = wid; t < MROWS / 32; t += NT / 64) {
    const int j = lane & 31;
    const int r = t * 32 + j, rv = r < NVOX ? r : 0;
    const int x = rv / (BY * BZ), y = (rv / BZ) % BY, z = rv % BZ;
    const int res = (((x + XO) * HY + (y + 1)) * HZP + (z + 1)) & (RES - 1);
    // what slot j seats: residue sq, rank sk (MF = 32: j & 15, j >> 4)
    const int ji = j & 15, jb = MF == 16 && ji >= 4 && ji < 12;
    const int sq = MF == 16 ? (jb ? ji - 4 : ji < 4 ? ji : ji - 8) : ji, sk = MF == 16 ? 2 * (j >> 4) + jb : j >> 4;
    unsigned same = 0, mine = 0;                      // rows with this row's residue / with this SLOT's residue
#pragma unroll
    for (int q = 0; q < RES; ++q) {
      const unsigned m = (unsigned)__ballot(res == q);
      if (res == q) same = m;
      if (sq == q) mine = m;
    }
    const unsigned below = (1u << j) - 1u;
    const int rank = __popc(same & below);
    const bool slot_empty = __popc(mine) < sk + 1;
    const unsigned left = (unsigned)__ballot(rank >= RANKS), empty = (unsigned)__ballot(slot_empty);
    const unsigned short val = r < NVOX ? (unsigned short)r : kPadRow;
    unsigned short *tab = vox_tab + t * 32, *tmp = vox_tab + MROWS + (wid & 7) * 32;
    if (lane < 32) {
      if (rank < RANKS) tab[seat(rank, res)] = val;
      else tmp[__popc(left & below)] = val;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");        // one wave, LDS operations complete in order: its own stores are visible
    if (lane < 32 && slot_empty) tab[j] = tmp[__popc(empty & below)];
  }
  __syncthreads();
  const int fr = lane & 31, fh = lane >> 5;
  // MF = 16: RT16 row tiles and TN16 column tiles of 16 per wave; lane = row / column fr16 of a tile, chunk fq of its 32 channels
  constexpr int RT16 = 2 * RT, TN16 = BNV / (16 * WNV);
  const int fr16 = lane & 15, fq = lane >> 4;
  int arow[MF == 16 ? RT16 : RT];
#pragma unroll
  for (int i = 0; i < (MF == 16 ? RT16 : RT); ++i) {
    // pad rows read voxel 0's halo rows (valid LDS, result dropped)
    const int r = (MF == 16 ? vox_tab[wm * RT * 32 + i * 16 + fr16] : vox_tab[(wm * RT + i) * 32 + fr]) & 0x7fff;
    const int x = r / (BY * BZ), y = (r / BZ) % BY, z = r % BZ;
    arow[i] = ((x + XO) * HY + (y + 1)) * HZP + (z + 1);
  }
  // output mask: does this wave's 64-voxel tile / this brick hold a row the caller needs?
  bool wave_live = true;
  if (p.out_mask) {
    bool mine = false;
#pragma unroll
    for (int i = 0; i < RT; ++i) {
      const int r = vox_tab[(wm * RT + i) * 32 + fr];
      const int x = X0 + r / (BY * BZ), y = Y0 + (r / BZ) % BY, z = Z0 + r % BZ;
      if (!(r & kPadRow) && x < p.gx && y < p.gy && z < p.gz) mine |= p.out_mask[((int64_t)x * p.gy + y) * p.gz + z] != 0;
    }
    wave_live = __ballot(mine) != 0ull;
    if (!__syncthreads_or(wave_live ? 1 : 0)) {
      // dead brick: store the epilogue of a zero accumulator and leave (no staging, no taps)
      if (p.splitk > 1 && !p.ws) return;             // atomics path: y was zero-filled, the epilogue kernel finishes it
      for (int e = tid; e < NVOX * (BNV / 4); e += NT) {
        const int rl = e / (BNV / 4), c4 = e - rl * (BNV / 4);
        const int col = n0 + c4 * 4;
        if (col >= p.Cout) continue;
        const int x = X0 + rl / (BY * BZ), y = Y0 + (rl / BZ) % BY, z = Z0 + rl % BZ;
        if (x >= p.gx || y >= p.gy || z >= p.gz) continue;
        const int64_t orow = ((int64_t)x * p.gy + y) * p.gz + z;       // (the masked form is one scene)
        for (int q = 0; q < 4 && col + q < p.Cout; ++q) {
          float v = 0.f;
          if (p.splitk > 1) { p.ws[(int64_t)blockIdx.z * p.ws_stride + orow * p.Cout + col + q] = 0.f; continue; }
          v = v * (p.scale ? p.scale[col + q] : 1.f) + (p.shift ? p.shift[col + q] : 0.f);
          if (p.relu == 2) v = relu_nan(v);
          if (p.residual) v += p.residual[orow * p.Cout + col + q];
          if (p.relu == 1) v = relu_nan(v);
          if (p.act_scale) v = act_col(v, col + q, p.act_c0, p.act_c1, *p.act_scale);
          p.y[orow * p.Cout + col + q] = v;
        }
      }
      return;
    }
  }
  // B staging slot of this thread: 8 bf16 at (tid&3)*8 of row bn; the 16 lanes of one ds_write_b128 pass take rows
  // {r, r+4, r+8, r+12} (16 banks apart at the 20-dword pitch) instead of 4 consecutive rows that overlap by 12 banks
  const int bc = tid & 3, rs16 = (tid >> 2) & 15;
  // (96-byte rows, MF = 16: rows {r, r+2, r+4, r+6} are 16 banks apart at the 24-dword pitch)
  const int bn = MF == 16 ? 16 * wid + 2 * (rs16 & 3) + ((rs16 >> 2) & 1) + 8 * (rs16 >> 3) : 16 * wid + (rs16 >> 2) + 4 * (rs16 & 3);
  const bool bn_ok = tid < BNV * 4 && n0 + bn < p.Cout;     // BNV * 4 sixteen-byte chunks per plane and tap

  // MF = 32: acc; MF = 16: acc16 (the other is one unused element)
  f32x16 acc[MF == 16 ? 1 : RT][MF == 16 ? 1 : TN];
  f32x4 acc16[MF == 16 ? RT16 : 1][MF == 16 ? TN16 : 1];
#pragma unroll
  for (int i = 0; i < (MF == 16 ? 1 : RT); ++i)
#pragma unroll
    for (int j = 0; j < (MF == 16 ? 1 : TN); ++j)
#pragma unroll
      for (int k = 0; k < 16; ++k) acc[i][j][k] = 0.f;
#pragma unroll
  for (int i = 0; i < (MF == 16 ? RT16 : 1); ++i)
#pragma unroll
    for (int j = 0; j < (MF == 16 ? TN16 : 1); ++j)
#pragma unroll
      for (int k = 0; k < 4; ++k) acc16[i][j][k] = 0.f;
  SGC_HALO_STAMP(0);

  float4 ra[NA], rw[WZ ? NA : 1];      // rw: the second voxel row of a Winograd transform chunk
  uint4 rbh, rbl;
  // Addressing is fixed per thread for the whole kernel (the halo rows a thread stages and its weight row do not depend on the
  // channel slice or the tap): one 32-bit byte offset per chunk, 0xfffffff0 = "outside the volume / padding slot", computed once;
  // a slice / a tap then only moves a uniform offset.  Buffer loads return zeros past the tensor, so the loads carry no branch.
  constexpr unsigned OOB = 0xfffffff0u;
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float *>(p.x), 0, (int)(unsigned)((int64_t)(WZ ? p.wz_Z : SC ? p.scenes * p.ix : p.ix) * p.iy * p.iz * p.Cin * 4), 0x00020000);
  const int w_bytes = (int)(unsigned)((int64_t)NTAP * p.Cout * p.Cin * 2);
  // weight set of this brick: one for the whole launch, or -- 2-D form with image groups -- that of the group its images belong to
  const int64_t w_set = (TD && p.w_group_images > 0) ? (int64_t)(X0 / p.w_group_images) * NTAP * p.Cout * p.Cin : 0;
  const __amdgpu_buffer_rsrc_t whr = __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16 *>(p.w_hi + w_set), 0, w_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t wlr = __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16 *>(p.w_lo + w_set), 0, w_bytes, 0x00020000);
  unsigned aoff[NA], aoffb[WZ ? NA : 1];
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const int idx = i * NT + tid;
    const int row = idx >> 3, c4 = idx & 7;
    const int hz = row % HZ, hy = (row / HZ) % HY, hx = row / (HZ * HY);
    const int gx = X0 + hx - XO, gy = Y0 + hy - 1, gz = Z0 + hz - 1;
    const bool in = row < HROWS && gx >= 0 && gx < p.ix && gy >= 0 && gy < p.iy && gz >= 0 && gz < p.iz;
    if constexpr (WZ) {
      // image gx = kpos * J + j: the two voxel rows of the raw volume [iy][iz][Z] whose combination is this transform row
      const int J = p.wz_Z >> 1, kpos = X0 / J, j = gx - kpos * J;       // a brick's images belong to one position (J % BX == 0: plan_conv checks it)
      const int za = kpos == 0 ? 2 * j - 1 : kpos == 2 ? 2 * j + 1 : 2 * j;
      const int zb = kpos <= 1 ? 2 * j + 1 : kpos == 2 ? 2 * j : 2 * j + 2;
      const unsigned col = (unsigned)((gy * p.iz + gz) * p.wz_Z);
      aoff[i] = in && za >= 0 ? ((col + (unsigned)za) * (unsigned)p.Cin + c4 * 4) * 4u : OOB;
      aoffb[i] = in && zb < p.wz_Z ? ((col + (unsigned)zb) * (unsigned)p.Cin + c4 * 4) * 4u : OOB;
    } else {
      aoff[i] = in ? ((unsigned)((SC ? in0 : 0) + (gx * p.iy + gy) * p.iz + gz) * (unsigned)p.Cin + c4 * 4) * 4u : OOB;
    }
  }
  const float wz_sign = WZ && (X0 / max(p.wz_Z >> 1, 1)) == 1 ? 1.f : -1.f;      // t1 = d1 + d2; t0, t2, t3 are differences
  const unsigned boff = bn_ok ? (unsigned)((n0 + bn) * p.Cin + bc * 8) * 2u : OOB;
  auto load_A = [&](int cc) {
    const int soff = __builtin_amdgcn_readfirstlane(cc * (BK * 4));
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(xr, aoff[i], soff, 0);
      ra[i] = make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3]));
      if constexpr (WZ) {
        const u32x4 u = __builtin_amdgcn_raw_buffer_load_b128(xr, aoffb[i], soff, 0);
        rw[i] = make_float4(__uint_as_float(u[0]), __uint_as_float(u[1]), __uint_as_float(u[2]), __uint_as_float(u[3]));
      }
    }
  };
  // the split of a loaded halo chunk, in place: ra[i] = (hi.xy, hi.zw, lo.xy, lo.zw) as packed bf16 pairs.  Called under the
  // last tap of a slice (the loads went out three taps earlier), so that between the slice's last barrier and the next
  // slice's first tap only the ds_writes remain -- the vector work of the split overlaps the other wave's MFMAs instead of
  // sitting between two barriers.
  auto split_A = [&]() {
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      float v[4] = {ra[i].x, ra[i].y, ra[i].z, ra[i].w};
      if constexpr (WZ) {                       // the input transform: one fp32 rounding per element (sign * b is exact)
        v[0] += wz_sign * rw[i].x; v[1] += wz_sign * rw[i].y; v[2] += wz_sign * rw[i].z; v[3] += wz_sign * rw[i].w;
      }
      bf16x4 h, l;
      split4<NP>(v, h, l);
      const uint2 hu = __builtin_bit_cast(uint2, h), lu = __builtin_bit_cast(uint2, l);
      ra[i] = make_float4(__uint_as_float(hu.x), __uint_as_float(hu.y), __uint_as_float(lu.x), __uint_as_float(lu.y));
    }
  };
  auto store_A = [&]() {               // ra[] holds split chunks (split_A)
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      // LDS slot of the chunk, recomputed once per slice (two constant divisions) rather than held in NA registers
      const int idx = i * NT + tid;
      const int row = idx >> 3, c4 = idx & 7;
      if (row < HROWS) {
        const int o = ((row / HZ) * HZP + row % HZ) * LDKH + c4 * 4;
        *reinterpret_cast<uint2 *>(A_hi + o) = make_uint2(__float_as_uint(ra[i].x), __float_as_uint(ra[i].y));
        if constexpr (NP == 3) *reinterpret_cast<uint2 *>(A_lo + o) = make_uint2(__float_as_uint(ra[i].z), __float_as_uint(ra[i].w));
      }
    }
  };
  auto load_B = [&](int tap, int cc) {
    const int soff = __builtin_amdgcn_readfirstlane((tap * p.Cout * p.Cin + cc * BK) * 2);
    const u32x4 h = __builtin_amdgcn_raw_buffer_load_b128(whr, boff, soff, 0);
    rbh = make_uint4(h[0], h[1], h[2], h[3]);
    if constexpr (NP == 3) {
      const u32x4 l = __builtin_amdgcn_raw_buffer_load_b128(wlr, boff, soff, 0);
      rbl = make_uint4(l[0], l[1], l[2], l[3]);
    } else {
      rbl = make_uint4(0, 0, 0, 0);
    }
  };
  auto store_B = [&](int buf) {
    if (tid >= BNV * 4) return;
    __bf16 *b = Bbase + buf * 2 * B_PLANE + bn * LDKH + bc * 8;
    *reinterpret_cast<uint4 *>(b) = rbh;
    if constexpr (NP == 3) *reinterpret_cast<uint4 *>(b + B_PLANE) = rbl;
  };
  auto tap_off = [&](int tap) {
    const int dx = TD ? XO : tap / 9, dy = (tap / 3) % 3, dz = tap % 3;
    return ((dx - XO) * HY + (dy - 1)) * HZP + (dz - 1);
  };
  // one k-half (16 channels) of a tap: A fragments of the wave's two row tiles, B fragments of its TN column tiles
  struct Frag { bf16x8 ah[RT], al[RT], bh[TN], bl[TN]; };
  auto read_A = [&](Frag &f, int toff, int kk) {
#pragma unroll
    for (int i = 0; i < RT; ++i) {
      const int o = (arow[i] + toff) * LDKH + fh * 8 + kk * 16;
      f.ah[i] = *reinterpret_cast<const bf16x8 *>(A_hi + o);
      if constexpr (NP == 3) f.al[i] = *reinterpret_cast<const bf16x8 *>(A_lo + o);
    }
  };
  auto read_B = [&](Frag &f, int buf, int kk) {
    const __bf16 *b = Bbase + buf * 2 * B_PLANE + (wn * WCOL + fr) * LDKH + fh * 8 + kk * 16;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      f.bh[j] = *reinterpret_cast<const bf16x8 *>(b + j * 32 * LDKH);
      if constexpr (NP == 3) f.bl[j] = *reinterpret_cast<const bf16x8 *>(b + B_PLANE + j * 32 * LDKH);
    }
  };
  auto mfma_half = [&](const Frag &f) {
    if constexpr ((SGC_HALO_SKIP & 32) != 0) {          // timing / power builds: everything but the MFMAs
#pragma unroll
      for (int i = 0; i < RT; ++i) asm volatile("" ::"v"(f.ah[i]), "v"(f.al[i]));
#pragma unroll
      for (int j = 0; j < TN; ++j) asm volatile("" ::"v"(f.bh[j]), "v"(f.bl[j]));
      return;
    }
    // (s_setprio 2 around this cluster -- the wave that feeds the matrix pipe first at the issue arbiter -- or around everything else:
    //  181.9 / 181.7 against 182.7 us on the 90-GF Winograd layer, 149.7 / 150.1 against 151.3 on 512 -> 512, bit-identical: noise;
    //  profiles/r06_wz_prio.txt.  Not kept.)
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) acc[i][j] = mma_split<NP>(f.ah[i], f.al[i], f.bh[j], f.bl[j], acc[i][j]);
  };
  // MF = 16: a tap is one k-step.  A fragments of two of the wave's four row tiles (one half of the tap), B fragments of its column tiles
  struct FragA16 { bf16x8 h[2], l[2]; };
  struct FragB16 { bf16x8 h[TN16], l[TN16]; };
  auto read_A16 = [&](FragA16 &f, int toff, int half) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int o = (arow[MF == 16 ? 2 * half + i : 0] + toff) * LDKH + fq * 8;
      f.h[i] = *reinterpret_cast<const bf16x8 *>(A_hi + o);
      if constexpr (NP == 3) f.l[i] = *reinterpret_cast<const bf16x8 *>(A_lo + o);
    }
  };
  auto read_B16 = [&](FragB16 &f, int buf, int j) {
    const __bf16 *b = Bbase + buf * 2 * B_PLANE + (wn * WCOL + j * 16 + fr16) * LDKH + fq * 8;
    f.h[j] = *reinterpret_cast<const bf16x8 *>(b);
    if constexpr (NP == 3) f.l[j] = *reinterpret_cast<const bf16x8 *>(b + B_PLANE);
  };
  // one half of a tap: column tile by column tile, the three products interleaved over the two row tiles (no accumulator waits
  // on its own previous MFMA; each still sees lo*hi, hi*lo, hi*hi of a tap in this order).  next_buf >= 0: the fragments of
  // column tile j are refilled from that weight buffer behind the last MFMA that reads them
  auto mfma16_half = [&](const FragA16 &a, int half, FragB16 &b, int next_buf) {
#pragma unroll
    for (int j = 0; j < TN16; ++j) {
      f32x4 &c0 = acc16[MF == 16 ? 2 * half : 0][MF == 16 ? j : 0], &c1 = acc16[MF == 16 ? 2 * half + 1 : 0][MF == 16 ? j : 0];
      c0 = mma_split_one<NP, 0>(a.h[0], a.l[0], b.h[j], b.l[j], c0);
      c1 = mma_split_one<NP, 0>(a.h[1], a.l[1], b.h[j], b.l[j], c1);
      c0 = mma_split_one<NP, 1>(a.h[0], a.l[0], b.h[j], b.l[j], c0);
      c1 = mma_split_one<NP, 1>(a.h[1], a.l[1], b.h[j], b.l[j], c1);
      c0 = mma_split_one<NP, 2>(a.h[0], a.l[0], b.h[j], b.l[j], c0);
      c1 = mma_split_one<NP, 2>(a.h[1], a.l[1], b.h[j], b.l[j], c1);
      if (next_buf >= 0) read_B16(b, next_buf, j);
    }
  };
  const int steps_total = (c_hi - c_lo) * NTAP;
  auto step_tap = [&](int st) { return st % NTAP; };
  auto step_cc = [&](int st) { return c_lo + st / NTAP; };

  if constexpr (MF == 16) {
    // The pipelined schedule below with P / Q = the A fragments of row tiles 0-1 / 2-3 (16 registers each) and ONE set of B fragments
    // (32 registers).  Tap g, every wave:
    //   first half   issue the reads of Q(g); write the weight tile of tap g + 1, start the load of tap g + 2; multiply P(g) by B(g)
    //   BARRIER      publishes tile g + 1
    //   second half  issue the reads of P(g + 1); multiply Q(g) by B(g), refilling each column tile's fragments with B(g + 1)
    // Hazards as below: tile g + 1 overwrites tile g - 1, whose reads (the refills of tap g - 2's second half) completed before
    // barrier g - 1; the refills follow barrier g.  A slice's last tap reads neither the halo image nor the weights in its second half.
    load_A(c_lo);
    load_B(0, c_lo);
    split_A();
    store_A();
    store_B(0);
    if (steps_total > 1) load_B(step_tap(1), step_cc(1));
    __syncthreads();
    FragA16 P = {}, Q = {};
    FragB16 B = {};
    if (wave_live) {
      read_A16(P, tap_off(0), 0);
#pragma unroll
      for (int j = 0; j < TN16; ++j) read_B16(B, 0, j);
    }
    int g = 0;
    for (int cc = c_lo; cc < c_hi; ++cc) {
#pragma unroll
      for (int tap = 0; tap < NTAP; ++tap, ++g) {
        const bool last_tap = tap == NTAP - 1;
        if (wave_live) read_A16(Q, tap_off(tap), 1);
        if (g + 1 < steps_total) store_B((g + 1) & 1);
        if (g + 2 < steps_total) load_B(step_tap(g + 2), step_cc(g + 2));
        if (tap == NTAP - 3 && cc + 1 < c_hi) load_A(cc + 1);
        if (wave_live) mfma16_half(P, 0, B, -1);
        if (last_tap && cc + 1 < c_hi) split_A();
        __syncthreads();
        __builtin_amdgcn_sched_barrier(0);
        if (wave_live && !last_tap) read_A16(P, tap_off(tap + 1), 0);
        if (last_tap && cc + 1 < c_hi) store_A();
        if (wave_live) mfma16_half(Q, 1, B, last_tap ? -1 : (g + 1) & 1);
        __builtin_amdgcn_sched_barrier(0);
      }
      if (cc + 1 < c_hi) {
        __syncthreads();                                          // the new halo image is published
        if (wave_live) {
          read_A16(P, tap_off(0), 0);
#pragma unroll
          for (int j = 0; j < TN16; ++j) read_B16(B, g & 1, j);
        }
      }
    }
  } else if constexpr (STG) {
    // P: operands of a tap's first k-half, Q: of its second k-half (32 registers each).  Tap g, every wave:
    //   first half   issue the reads of Q(g); write the weight tile of tap g + 1 (registers loaded during tap g - 1) and
    //                start the load of tap g + 2; multiply P(g) -- in registers since the second half of tap g - 1
    //   BARRIER      publishes tile g + 1; its own waits (Q(g) reads, the tile's ds_writes) ended long before
    //   second half  issue the reads of P(g + 1); multiply Q(g)
    // Hazards: tile g + 1 overwrites tile g - 1, whose last reads (Q(g - 1)) completed before barrier g - 1; P(g + 1) is read
    // behind barrier g, which follows every wave's ds_writes of tile g + 1.  At a slice's last tap the second half reads
    // nothing from the halo image (P of the next slice needs the new image), so barrier g also ends the slice's halo reads:
    // the next slice's image is written under the MFMAs of that second half, one more barrier publishes it.
    // (Weight tiles by LDS-DMA instead of registers + ds_write_b128 -- unpadded swizzled rows, issued a whole tap ahead of the
    //  barrier that publishes them -- were built into this schedule and measured: 0.90 of the lockstep form's time against 0.83
    //  for the register-staged tiles, same box, bit-identical.  Two DMA pieces per wave cost more issue time than two ds_writes.)
    load_A(c_lo);
    load_B(0, c_lo);
    split_A();
    store_A();
    store_B(0);
    if (steps_total > 1) load_B(step_tap(1), step_cc(1));      // stays in registers until tap 0 publishes it
    __syncthreads();
    Frag P = {}, Q = {};
    constexpr int SKIP = SGC_HALO_SKIP;      // timing builds only (diag.hpp); 0 in the product
    if (wave_live) { read_A(P, tap_off(0), 0); read_B(P, 0, 0); }
    int g = 0;
    for (int cc = c_lo; cc < c_hi; ++cc) {
      // the taps are unrolled: a tap's halo offset, its place in the slice and (with the slice's parity) its weight buffer are
      // compile-time constants, so the fragment addresses are one register + an immediate and the tap decode -- ~50 scalar and
      // ~12 vector instructions per tap in the rolled loop (SQ_INSTS_SALU > SQ_INSTS_VALU in round 3's counters) -- is gone
#pragma unroll
      for (int tap = 0; tap < NTAP; ++tap, ++g) {
        const bool last_tap = tap == NTAP - 1;
        const bool more = g + 1 < steps_total;
        if (wave_live) {
          if (!(SKIP & 16) || g == 0) read_A(Q, tap_off(tap), 1);
          if (!(SKIP & 8) || g == 0) read_B(Q, g & 1, 1);
        }
        if (!(SKIP & 2) && more) store_B((g + 1) & 1);
        if (!(SKIP & 4) && g + 2 < steps_total) load_B(step_tap(g + 2), step_cc(g + 2));
        if (!(SKIP & 64) && tap == NTAP - 3 && cc + 1 < c_hi) load_A(cc + 1);    // next slice's halo rides under the last taps
        if (wave_live) mfma_half(P);
        if (!(SKIP & 64) && last_tap && cc + 1 < c_hi) split_A();
        if (!(SKIP & 1)) __syncthreads();
        // the fence keeps the refill of P behind the MFMAs that consumed it (hoisted above them it needs a second set of
        // registers) and behind the barrier that publishes the tile it reads
        __builtin_amdgcn_sched_barrier(0);
        if (wave_live && !last_tap) {
          if (!(SKIP & 16)) read_A(P, tap_off(tap + 1), 0);
          if (!(SKIP & 8)) read_B(P, (g + 1) & 1, 0);
        }
        if (!(SKIP & 64) && last_tap && cc + 1 < c_hi) store_A();                // every wave's halo reads of this slice are complete
        if (wave_live) mfma_half(Q);
        __builtin_amdgcn_sched_barrier(0);
      }
      if (cc + 1 < c_hi) {
        __syncthreads();                                          // the new halo image is published
        if (wave_live) { read_A(P, tap_off(0), 0); read_B(P, g & 1, 0); }
      }
    }
  } else {
    // lockstep form.  SGC_HALO_SKIP (diag.hpp; 0 in the product) removes parts of the tap loop in timing builds
    constexpr int SKIP = SGC_HALO_SKIP;
    int g = 0;                       // global step counter -> B buffer
    load_A(c_lo);
    load_B(0, c_lo);
    split_A();
    store_A();
    store_B(0);
    __syncthreads();
    // A fragments of the NEXT tap's first k-half are read before the barrier (the halo is static within a
    // channel slice), so after the barrier only the freshly written B tile has to come out of LDS
    Frag P = {}, Q = {};
    read_A(P, tap_off(0), 0);
    for (int cc = c_lo; cc < c_hi; ++cc) {
      for (int tap = 0; tap < NTAP; ++tap, ++g) {
        const bool last_tap = tap == NTAP - 1;
        if (!(SKIP & 4) && g + 1 < steps_total) load_B(step_tap(g + 1), step_cc(g + 1));
        if (tap == NTAP - 3 && cc + 1 < c_hi) load_A(cc + 1);      // next slice's halo rides under the last taps
        const int toff = tap_off(tap);
        if (wave_live) {
          if (!(SKIP & 8) || g == 0) read_B(P, g & 1, 0);
          if (!(SKIP & 16) || g == 0) read_A(Q, toff, 1);
          if (!(SKIP & 8) || g == 0) read_B(Q, g & 1, 1);
          mfma_half(P);
          mfma_half(Q);
          if (!last_tap && (!(SKIP & 16) || g == 0)) read_A(P, tap_off(tap + 1), 0);
        }
        if (!(SKIP & 2) && g + 1 < steps_total) store_B((g + 1) & 1);
        if (last_tap && cc + 1 < c_hi) split_A();
        if (!(SKIP & 1)) __syncthreads();
      }
      if (cc + 1 < c_hi) {            // every wave is past the last tap: the halo can be replaced
        store_A();
        __syncthreads();
        if (wave_live && (!(SKIP & 16))) read_A(P, tap_off(0), 0);
      }
    }
  }
  SGC_HALO_STAMP(2);
  if constexpr ((SGC_HALO_SKIP & 128) != 0) { if (p.relu != 77) return; }     // timing builds: no epilogue (the condition keeps the MFMAs alive)

  // first output row of this workgroup's scene: derived from the workgroup id again HERE (the empty asm keeps the compiler from
  // carrying the value of the prologue through the tap loop, where every register counts)
  int64_t orow0 = 0;
  if constexpr (SC) {
    int bid_e = blockIdx.x;
    asm volatile("" : "+s"(bid_e));
    orow0 = (int64_t)(bid_e / (((p.gx + BX - 1) / BX) * ((p.gy + BY - 1) / BY) * ((p.gz + BZ - 1) / BZ))) * p.gx * p.gy * p.gz;
  }
  // Epilogue through LDS (as in the implicit-GEMM kernel): the halo / weight buffers are free, the 256 x 128 tile
  // leaves as 16-byte row-contiguous stores instead of 64 four-byte stores per lane.
  if ((p.Cout & 3) == 0 && (p.splitk == 1 || p.ws)) {
    // (MF = 16: a lane quarter sits 4 rows below the previous one, and 4 rows of BNV + 4 floats are 16 banks)
    constexpr int LDC = MF == 16 ? BNV + 4 : BNV + 8;
    float *cs = reinterpret_cast<float *>(smem_h);           // [MROWS][LDC] floats (139 KB for 256 x 128; launch_halo sizes LDS for it)
    if constexpr (STG) __syncthreads();                      // the second half of the last tap ran after the loop's last barrier
    if constexpr (MF == 16) {
#pragma unroll
      for (int i = 0; i < RT16; ++i)
#pragma unroll
        for (int j = 0; j < TN16; ++j)
#pragma unroll
          for (int k = 0; k < 4; ++k)
            cs[(wm * (RT * 32) + i * 16 + acc16_row(lane) + k) * LDC + wn * WCOL + j * 16 + fr16] = acc16[i][j][k];
    } else {
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int k = 0; k < 16; ++k)
          cs[(wm * (RT * 32) + i * 32 + (k & 3) + 8 * (k >> 2) + 4 * (lane >> 5)) * LDC + wn * WCOL + j * 32 + (lane & 31)] = acc[i][j][k];
    }
    __syncthreads();
    constexpr int C4 = BNV / 4;
    for (int e = tid; e < MROWS * C4; e += NT) {
      const int rl = e / C4, c4 = e - rl * C4;
      const int col = n0 + c4 * 4;
      if (col >= p.Cout) continue;
      const int r = vox_tab[rl];
      if (r & kPadRow) continue;
      const int x = X0 + r / (BY * BZ), y = Y0 + (r / BZ) % BY, z = Z0 + r % BZ;
      if (x >= p.gx || y >= p.gy || z >= p.gz) continue;
      const int64_t orow = (SC ? orow0 : 0) + ((int64_t)x * p.gy + y) * p.gz + z;
      float4 v = *reinterpret_cast<const float4 *>(cs + rl * LDC + c4 * 4);
      if (p.splitk > 1) {
        *reinterpret_cast<float4 *>(p.ws + (int64_t)blockIdx.z * p.ws_stride + orow * p.Cout + col) = v;
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
      if (p.relu == 2) v = relu_nan(v);
      if (p.residual) {
        const float4 r4 = *reinterpret_cast<const float4 *>(p.residual + orow * p.Cout + col);
        v.x += r4.x; v.y += r4.y; v.z += r4.z; v.w += r4.w;
      }
      if (p.relu == 1) v = relu_nan(v);
      if (p.act_scale) v = act_col4(v, col, p.act_c0, p.act_c1, *p.act_scale);
      *reinterpret_cast<float4 *>(p.y + orow * p.Cout + col) = v;
    }
    return;
  }

  // element-wise stores (Cout % 4 != 0, or a split without a workspace): one accumulator element at a time, by the shape's map
  const auto store_one = [&](int tab_row, int col, float sc, float sh, float a) {
    const int r = vox_tab[tab_row];
    const int x = X0 + r / (BY * BZ), y = Y0 + (r / BZ) % BY, z = Z0 + r % BZ;
    if ((r & kPadRow) || x >= p.gx || y >= p.gy || z >= p.gz) return;
    const int64_t orow = (SC ? orow0 : 0) + ((int64_t)x * p.gy + y) * p.gz + z;
    float *dst = p.y + orow * p.Cout + col;
    if (p.splitk > 1) {
      if (p.ws) p.ws[(int64_t)blockIdx.z * p.ws_stride + orow * p.Cout + col] = a;
      else atomicAdd(dst, a);
    } else {
      float v = a * sc + sh;
      if (p.relu == 2) v = relu_nan(v);
      if (p.residual) v += p.residual[orow * p.Cout + col];
      if (p.relu == 1) v = relu_nan(v);
      if (p.act_scale) v = act_col(v, col, p.act_c0, p.act_c1, *p.act_scale);
      *dst = v;
    }
  };
  if constexpr (MF == 16) {
#pragma unroll
    for (int i = 0; i < RT16; ++i)
#pragma unroll
      for (int j = 0; j < TN16; ++j) {
        const int col = n0 + wn * WCOL + j * 16 + fr16;
        if (col >= p.Cout) continue;
        const float sc = p.scale ? p.scale[col] : 1.f, sh = p.shift ? p.shift[col] : 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) store_one(wm * RT * 32 + i * 16 + acc16_row(lane) + k, col, sc, sh, acc16[i][j][k]);
      }
  } else {
#pragma unroll
  for (int i = 0; i < RT; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int col = n0 + wn * WCOL + j * 32 + (lane & 31);
      if (col >= p.Cout) continue;
      const float sc = p.scale ? p.scale[col] : 1.f, sh = p.shift ? p.shift[col] : 0.f;
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int r = vox_tab[(wm * RT + i) * 32 + (k & 3) + 8 * (k >> 2) + 4 * (lane >> 5)];
        const int x = X0 + r / (BY * BZ), y = Y0 + (r / BZ) % BY, z = Z0 + r % BZ;
        if ((r & kPadRow) || x >= p.gx || y >= p.gy || z >= p.gz) continue;
        const int64_t orow = (SC ? orow0 : 0) + ((int64_t)x * p.gy + y) * p.gz + z;
        float *dst = p.y + orow * p.Cout + col;
        if (p.splitk > 1) {
          if (p.ws) p.ws[(int64_t)blockIdx.z * p.ws_stride + orow * p.Cout + col] = acc[i][j][k];
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
}

// Forms of this kernel that were built, bit-identical, and measured slower or equal (the code is in the
// history up to round 3): weights by LDS-DMA into a four-stage ring with swizzled unpadded rows (237 vs 230 us warm on the 90-GF
// layer); weights straight from L2 into registers, no barrier per tap (236 vs 229-240, 2-7 % slower elsewhere); three weight
// buffers staged two taps ahead (236 vs 232); v_mfma_f32_16x16x32_bf16 (234 vs 230: a timing build of round 2's lockstep kernel,
// one stream, ranked by wall alone -- measured again as a correct kernel on the Winograd bricks with scenes in flight, where it
// wins and is the default: MF = 16 above, profiles/r21_wz_mfma_shape.md); a one-wave-per-SIMD form with 512
// registers (309 vs 251).  Round 6, Winograd (2-D, 9 taps per slice) form: the next slice's halo loads issued at the slice's second tap
// and split two chunks per tap under the last four taps instead of one split under the last tap -- 191.5 vs 191.2 us on the 90-GF layer,
// 155.8 vs 151.8 on 512 -> 512 @ 20x20x8 (profiles/r06_wz_skip.txt: the 13 us the restaging costs are not vector-issue time).

// one launch of the form a plan names; p.splitk is the caller's (plan_conv and the launch-time downgrades of conv3d_bf16x3)
template <int BX, int BY, int BZ, int BNV, int NP, bool TD, bool STG, bool WZ = false, int MF = 32, bool SC = false>
static int launch_halo_k(ConvParamsB &p, hipStream_t st) {
  if constexpr (!SC && !TD && !WZ) {                    // a batch of volumes: the instantiation with the scene decode
    if (p.scenes > 1) return launch_halo_k<BX, BY, BZ, BNV, NP, TD, STG, WZ, MF, true>(p, st);
  }
#if defined(SGC_HALO_STAMPS)
  p.stamps = g_halo_stamp_buf;
#endif
  constexpr int LROWS = (TD ? BX : BX + 2) * (BY + 2) * halo_pitch(BZ, MF);
  constexpr int RGRAN = BNV >= 64 ? 128 : 256;          // rows per (wave rows x 32): see the kernel's wave layout
  constexpr int MROWS = (BX * BY * BZ + RGRAN - 1) / RGRAN * RGRAN;
  const size_t smem = halo_tab_offset(LROWS, MROWS, MROWS > 256 ? BNV : 128, halo_ldk(MF)) + (MROWS + 256) * sizeof(uint16_t);   // table + 8 x 32 scratch
  static_assert(halo_tab_offset(LROWS, MROWS, MROWS > 256 ? BNV : 128, halo_ldk(MF)) + (MROWS + 256) * sizeof(uint16_t) <= 160 * 1024, "brick does not fit the LDS");
  static std::atomic<uint64_t> attr_done{0};
  ensure_dynamic_lds((const void *)conv3d_halo_bf16x3_kernel<BX, BY, BZ, BNV, NP, TD, STG, WZ, MF, SC>, (int)smem, attr_done);
  const int bricks = (SC ? p.scenes : 1) * ceil_div(p.gx, BX) * ceil_div(p.gy, BY) * ceil_div(p.gz, BZ);
  const int nb = ceil_div(p.Cout, BNV);
  hipLaunchKernelGGL((conv3d_halo_bf16x3_kernel<BX, BY, BZ, BNV, NP, TD, STG, WZ, MF, SC>), dim3(bricks, nb, p.splitk), dim3(512), smem, st, p);
  return check_launch("conv3d_halo_bf16x3_kernel");
}

template <int BX, int BY, int BZ, int BNV = 128, bool TD = false, bool WZ = false, int MF = 32>
static int launch_halo(ConvParamsB &p, hipStream_t st) {
  // the one-product modes and the Winograd stack: the software-pipelined form only.  (sgc_set_conv_products admits 1, 2 and 3 and
  // nothing else: any other value would select the pipelined NP = 3 form here, where the old ladder fell through to the lines below.)
  // (a Winograd brick has no direct twin: `if constexpr` keeps the two direct forms of its shape out of the library)
  if constexpr (!WZ) {
    if (g_conv_products == 3) {
      // the lockstep form is kept for the fp32-faithful mode only: it is the reference of the schedule's bit-identity test, and the
      // form of the whole-grid bricks (four row tiles per wave: the unrolled pipelined loop spills 600 registers there)
      if (!g_tune_halo_stagger || BX * BY * BZ > 256) return launch_halo_k<BX, BY, BZ, BNV, 3, TD, false>(p, st);
      return launch_halo_k<BX, BY, BZ, BNV, 3, TD, true>(p, st);
    }
  }
  return with_products(g_conv_products, [&](auto np) { return launch_halo_k<BX, BY, BZ, BNV, np(), TD, true, WZ, MF>(p, st); });
}

int launch_halo_z4(ConvParamsB &p, const ConvPlan &pl, hipStream_t st);   // conv3d_halo_z4.hip
int launch_halo_2d(ConvParamsB &p, const ConvPlan &pl, hipStream_t st);   // conv3d_halo_2d.hip
}  // namespace sgc
