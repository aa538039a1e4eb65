// Weight gradient of the implicit-GEMM convolutions (training): the tile kernel (3-D, and 2-D over image rows by an addressing policy), the two
// halo forms of the 3-D entry, their reduction and the entry points.
#include "conv_common.hpp"
#include "mma.hpp"
#include "../../include/sgcdet_amd_scene_batch.h"
#include "diag.hpp"
#include "tuning.hpp"

using namespace sgc;

// ---------------------------------------------------------------------------------------------
// Weight gradient of the same convolutions (training): dW[tap][co][ci] = sum_o dy[o][co] * x[nbr(o, tap)][ci],
// a GEMM per tap with M = Cout, N = Cin and the OUTPUT VOXELS as the reduction dimension.  Both operands are stored
// voxel-major (rows = k), so the staging pass transposes: a thread loads a 4-voxel x 4-channel block (four 16-byte loads
// from four rows), splits it hi/lo and writes four 8-byte runs of 4 consecutive k into the [channel][k] LDS image the
// forward kernel's fragment reads expect.  128 x 128 tile, K-step 32 voxels, 4 waves (2 x 2, 64 x 64 each), register
// prefetch of step s + 1 under the MFMAs of step s, double-buffered LDS.  The voxel range is split over blockIdx.z
// (taps x splits); partial tiles go to a workspace and are summed in split order (deterministic), or straight to dW
// when there is one split.  ksize 1 | 3 (pad k/2, stride 1 | 2) or 2 (stride 2, no pad: the ConvTranspose3d k2s2 layers
// with x := the fine-grid tensor and dy := the coarse one).
// ---------------------------------------------------------------------------------------------
struct WgradParams {
  const float *x, *dy;
  float *out;               // dW [taps][Cout][Cin] (one split) or the workspace [splits][taps][Cout][Cin]
  int Cin, Cout;
  int ix, iy, iz, ox, oy, oz;
  int ksize, stride, pad, taps;
  int OV, ksteps, splits, steps_per_split;     // OV: reduction rows of the launch = scenes * ox * oy * oz
  int scenes;               // volumes of one grid behind x and dy (sgc_conv3d_wgrad_bf16x3_batched): the scene axis is more reduction rows
  int as, ax, by, cz;       // 32 = as * (ox * oy * oz) + ax * (oy * oz) + by * oz + cz: the per-step advance of a voxel's (scene, x, y, z)
};

// WM = 2: 4 waves (2 x 2, 64 x 64 each), every thread stages one block of BOTH operands; WM = 4: 8 waves (4 x 2, 32 x 64 each),
// threads 0-255 stage the dy tile and 256-511 the x tile (half the loads, conversions and registers per thread, twice the
// waves to hide them).
// IMG: the 2-D form (sgc_conv2d_wgrad_bf16x3).  A reduction row decodes as (image, h, w) = (x, y, z) of the carried coordinates,
// the taps are the k * k taps of (y, z) only and the leading coordinate is neither strided nor padded -- it picks the image, so
// no tap crosses one.  Staging, MMA and store are the 3-D kernel's.
// SC: x and dy hold a batch of scenes (p.scenes > 1): the carried coordinates get a scene digit.  An instantiation of its own: the
// scene-less kernel is the code it always was.
template <int WM, bool IMG = false, bool SC = false>
__global__ __launch_bounds__(WM * 128) void conv3d_wgrad_bf16x3_kernel(const WgradParams p) {
  constexpr int TMW = 4 / WM * 1;                           // 32-row tiles per wave along M: 2 (WM = 2) or 1 (WM = 4)
  constexpr int BMW = 128, BNW = 128;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_w[];
  constexpr int PLANE = 128 * LDKH, BUF = 4 * PLANE;        // per buffer: A_hi, A_lo, B_hi, B_lo of [128][LDKH]
  __bf16 *base = reinterpret_cast<__bf16 *>(smem_w);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  const int co0 = blockIdx.x * BMW, ci0 = blockIdx.y * BNW;
  const int tap = blockIdx.z % p.taps, split = blockIdx.z / p.taps;
  const int s_lo = split * p.steps_per_split, s_hi = min(p.ksteps, s_lo + p.steps_per_split);
  int dx = 0, dy_ = 0, dz = 0;
  if (p.ksize > 1) { dx = IMG ? 0 : tap / (p.ksize * p.ksize); dy_ = (tap / p.ksize) % p.ksize; dz = tap % p.ksize; }

  const int role = WM == 4 ? __builtin_amdgcn_readfirstlane(tid >> 8) : 2;   // 0: stages dy, 1: stages x, 2: both (wave-uniform)
  const int kb = tid & 7, cb = (tid & 255) >> 3;            // this thread's block: voxels 4 kb .. + 3 of the step, channels 4 cb .. + 3
  const bool a_ok = role != 1 && co0 + 4 * cb < p.Cout, b_ok = role != 0 && ci0 + 4 * cb < p.Cin;
  float4 ra[4], rb[4];
  // Addressing without a division in the loop: a thread's four voxels advance by 32 per step, so their (x, y, z) are carried
  // (32 = ax * oy * oz + by * oz + cz, uniform digits from the host: z += cz, y += by + carry, x += ax + carry) instead of decoded from the flat index with two runtime divisions per voxel and step; loads go
  // through buffer descriptors, an out-of-range offset (voxel past OV, neighbour outside the volume, channel block past the
  // tensor) returns zeros, so there is no branch either.
  constexpr unsigned OOB = 0xfffffff0u;
  const __amdgpu_buffer_rsrc_t dyr = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float *>(p.dy), 0, (int)(unsigned)((int64_t)p.OV * p.Cout * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float *>(p.x), 0, (int)(unsigned)((int64_t)(SC ? p.scenes : 1) * p.ix * p.iy * p.iz * p.Cin * 4), 0x00020000);
  int vs[SC ? 4 : 1], vx[4], vy[4], vz[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int o = s_lo * 32 + 4 * kb + j;                   // may be >= OV: `live` below is false then and the loads are OOB
    vz[j] = o % p.oz; vy[j] = (o / p.oz) % p.oy;
    const int xs = o / (p.oz * p.oy);
    if constexpr (SC) { vs[j] = xs / p.ox; vx[j] = xs - vs[j] * p.ox; }
    else vx[j] = xs;                                        // (one scene: the coordinates run past ox and the loads are OOB)
  }
  int o_base = s_lo * 32 + 4 * kb;
  auto load_step = [&]() {                                  // loads the step the carried coordinates stand at, then advances them
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int o = o_base + j;
      const bool live = o < p.OV;
      if (role != 1) {
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(dyr, live && a_ok ? (unsigned)(o * p.Cout + co0 + 4 * cb) * 4u : OOB, 0, 0);
        ra[j] = make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3]));
      }
      if (role != 0) {
        const int xx = IMG ? vx[j] : vx[j] * p.stride + dx - p.pad, yy = vy[j] * p.stride + dy_ - p.pad, zz = vz[j] * p.stride + dz - p.pad;
        const bool in = live && b_ok && xx >= 0 && xx < p.ix && yy >= 0 && yy < p.iy && zz >= 0 && zz < p.iz;
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(
            xr, in ? ((unsigned)((((SC ? vs[SC ? j : 0] * p.ix : 0) + xx) * p.iy + yy) * p.iz + zz) * (unsigned)p.Cin + ci0 + 4 * cb) * 4u : OOB, 0, 0);
        rb[j] = make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3]));
      }
    }
    if (role != 0) {                                        // carry the coordinates to the next step: selects only, no branch
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        vz[j] += p.cz;                                      // 32 = as * OV1 + ax * (oy * oz) + by * oz + cz: one carry per digit, always exact
        const int c1 = vz[j] >= p.oz ? 1 : 0;
        vz[j] -= c1 ? p.oz : 0;
        vy[j] += p.by + c1;
        const int c2 = vy[j] >= p.oy ? 1 : 0;
        vy[j] -= c2 ? p.oy : 0;
        vx[j] += p.ax + c2;
        if constexpr (SC) {
          const int c3 = vx[j] >= p.ox ? 1 : 0;             // past the scene's last voxel: the next scene's first (its rows follow in x and dy)
          vx[j] -= c3 ? p.ox : 0;
          vs[j] += p.as + c3;
        }
      }
    }
    o_base += 32;
  };
  auto store_block = [&](const float4 (&r)[4], __bf16 *hi, __bf16 *lo) {
    const float v[4][4] = {{r[0].x, r[0].y, r[0].z, r[0].w}, {r[1].x, r[1].y, r[1].z, r[1].w},
                           {r[2].x, r[2].y, r[2].z, r[2].w}, {r[3].x, r[3].y, r[3].z, r[3].w}};
#pragma unroll
    for (int c = 0; c < 4; ++c) {                           // channel 4 cb + c: its 4 consecutive k
      bf16x4 h, l;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const __bf16 hb = (__bf16)v[j][c];
        h[j] = hb;
        l[j] = (__bf16)(v[j][c] - (float)hb);
      }
      const int o = (4 * cb + c) * LDKH + 4 * kb;
      *reinterpret_cast<bf16x4 *>(hi + o) = h;
      *reinterpret_cast<bf16x4 *>(lo + o) = l;
    }
  };
  auto store_step = [&](int buf) {
    __bf16 *a_hi = base + buf * BUF;
    if (role != 1) store_block(ra, a_hi, a_hi + PLANE);
    if (role != 0) store_block(rb, a_hi + 2 * PLANE, a_hi + 3 * PLANE);
  };

  f32x16 acc[TMW][2];
#pragma unroll
  for (int i = 0; i < TMW; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int k = 0; k < 16; ++k) acc[i][j][k] = 0.f;

  if (s_lo < s_hi) {
    load_step();
    store_step(0);
    __syncthreads();
    const int fr = lane & 31, fh = lane >> 5;
    for (int s = s_lo; s < s_hi; ++s) {
      const int buf = (s - s_lo) & 1;
      if (s + 1 < s_hi) load_step();
      const __bf16 *a_hi = base + buf * BUF + (wm * (32 * TMW) + fr) * LDKH + fh * 8;
      const __bf16 *a_lo = a_hi + PLANE;
      const __bf16 *b_hi = base + buf * BUF + 2 * PLANE + (wn * 64 + fr) * LDKH + fh * 8;
      const __bf16 *b_lo = b_hi + PLANE;
#pragma unroll
      for (int kk = 0; kk < BK / 16; ++kk) {
        bf16x8 ah[TMW], al[TMW], bh[2], bl[2];
#pragma unroll
        for (int i = 0; i < TMW; ++i) {
          ah[i] = *reinterpret_cast<const bf16x8 *>(a_hi + i * 32 * LDKH + kk * 16);
          al[i] = *reinterpret_cast<const bf16x8 *>(a_lo + i * 32 * LDKH + kk * 16);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          bh[i] = *reinterpret_cast<const bf16x8 *>(b_hi + i * 32 * LDKH + kk * 16);
          bl[i] = *reinterpret_cast<const bf16x8 *>(b_lo + i * 32 * LDKH + kk * 16);
        }
#pragma unroll
        for (int i = 0; i < TMW; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = mma_split<3>(ah[i], al[i], bh[j], bl[j], acc[i][j]);
      }
      if (s + 1 < s_hi) store_step(buf ^ 1);
      __syncthreads();
    }
  }
  // a lane owns column ci = lane & 31 of a 32 x 32 tile: for a fixed register the 32 lanes of a half-wave store 128
  // contiguous bytes of one dW row
  float *out = p.out + ((int64_t)split * p.taps + tap) * p.Cout * p.Cin;
#pragma unroll
  for (int i = 0; i < TMW; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int ci = ci0 + wn * 64 + j * 32 + (lane & 31);
      if (ci >= p.Cin) continue;
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int co = co0 + wm * (32 * TMW) + i * 32 + (k & 3) + 8 * (k >> 2) + 4 * (lane >> 5);
        if (co < p.Cout) out[(int64_t)co * p.Cin + ci] = acc[i][j][k];
      }
    }
}

// ---------------------------------------------------------------------------------------------
// Halo form of the weight gradient for the 3x3x3 stride-1 layers (round 4).  The tile kernel above is one GEMM per tap: every
// (co, ci) tile streams dy AND the tap-shifted x for its voxel range, so a layer moves 27 x both operands (2.8 GB for
// 256 -> 256 at 40x40x16) and splits each element to bf16 27 times: it runs at 0.29 PF/s, bound by its staging.  Here a
// workgroup owns 32 output channels x 32 input channels and ALL 27 taps and walks bricks of 8 x 8 x 4 voxels: per brick it
// stages dy [256 voxels][32 co] and the brick's x halo [10 x 10 x 6 rows][32 ci] ONCE (split hi / lo once) and multiplies
// them 27 times.  Both operands are stored voxel-major -- rows = the reduction index -- which is what the MFMA wants
// transposed: the fragments come out of LDS through ds_read_b64_tr_b16 (a 4-row x 16-column block per 16 lanes, delivered
// column-major; lane map checked in tools/probe/tr16_probe.hip), so no transposing pass exists anywhere.  Wave w owns taps
// w, w + 8, w + 16 (, w + 24): its accumulators are 3 - 4 tiles of 32 x 32; the dy fragments of a k-step (16 voxels) are read
// once per wave and reused for its taps, the x fragments of a tap are the same LDS rows shifted by the tap's halo offset --
// with the k-steps unrolled every read is one register + an immediate.  The brick range is split over workgroups; partial
// sums go through the workspace and wgrad_reduce_kernel (fixed order: deterministic).
// ---------------------------------------------------------------------------------------------
struct WgradHaloParams {
  const float *x, *dy;
  float *out;               // dW [27][Cout][Cin] (one split) or the workspace [splits][27][Cout][Cin]
  int Cin, Cout;
  int gx, gy, gz;           // grid (input = output grid: stride 1, padding 1)
  int nbricks, bricks_per_split;   // nbricks = scenes * bricks_per_scene: brick b belongs to scene b / bricks_per_scene
  int scenes, bricks_per_scene;
};

typedef __bf16 bf16x4v __attribute__((ext_vector_type(4)));

// MT = 32-channel dy tiles per workgroup (2: 64 output channels x 32 input channels; every x fragment feeds two MFMA triples,
// which halves the LDS reads per MFMA -- with MT = 1 the k-loop is LDS-read-bound).  Rows are stored with NO padding (pitch
// 32 bf16 = 16 banks): a transposed read touches 4 rows x 16 banks per half-wave and the staging writes are contiguous, both
// conflict-free; a padded pitch of 40 makes row q = 3 alias row 0.
// NW = waves per workgroup (8: two per SIMD, 256 registers each).  Fragments are read right before their MFMAs: with two waves
// per SIMD the partner's MFMAs cover the LDS round trip (a one-wave-per-SIMD variant of THIS form with read-ahead was
// built and spilled 168 registers; the double-buffered kernel below is the form that uses one wave per SIMD).
template <int MT, int NW>
__global__ __launch_bounds__(64 * NW) void conv3d_wgrad_halo_kernel(const WgradHaloParams p) {
  constexpr int BX = 8, BY = 8, BZ = 4, HY = BY + 2, HZ = BZ + 2, HROWS = (BX + 2) * HY * HZ;      // 600 halo rows
  constexpr int PW = 32;                                                                            // row pitch (bf16)
  constexpr int NT = 64 * NW;
  constexpr int X_PLANE = HROWS * PW, D_IMG = 256 * PW, D_PLANE = MT * D_IMG;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_g[];
  __bf16 *X_hi = reinterpret_cast<__bf16 *>(smem_g), *X_lo = X_hi + X_PLANE;
  __bf16 *D_hi = X_lo + X_PLANE, *D_lo = D_hi + D_PLANE;
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  // workgroups go to the 8 XCDs round-robin by linear id: all (co, ci) tiles of one brick range are put on ONE XCD, so the
  // 2.3 x (Cout / 64) re-reads of x and the (Cin / 32) re-reads of dy are L2 hits (without it a 256 -> 256 layer at
  // 40 x 40 x 16 pulls 455 MB through the fabric and the loads, not the MFMAs, set the time).  gridDim.z is the split count
  // rounded up to a multiple of 8; the surplus workgroups leave at once.
  const int lin = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z), tiles = gridDim.x * gridDim.y;
  int split = blockIdx.z, tile = blockIdx.x + gridDim.x * blockIdx.y;
  if ((gridDim.z & 7) == 0) { split = (lin & 7) + 8 * ((lin >> 3) / tiles); tile = (lin >> 3) % tiles; }
  const int co0 = (tile % gridDim.x) * (32 * MT), ci0 = (tile / gridDim.x) * 32;
  const int b_lo = split * p.bricks_per_split, b_hi = min(p.nbricks, b_lo + p.bricks_per_split);
  if (b_lo >= b_hi) return;
  const int nby = (p.gy + BY - 1) / BY, nbz = (p.gz + BZ - 1) / BZ;
  constexpr unsigned OOB = 0xfffffff0u;
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float *>(p.x), 0, (int)(unsigned)((int64_t)p.scenes * p.gx * p.gy * p.gz * p.Cin * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t dr = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float *>(p.dy), 0, (int)(unsigned)((int64_t)p.scenes * p.gx * p.gy * p.gz * p.Cout * 4), 0x00020000);
  // staging assignment: the x halo goes slab by slab (hx = 0 .. 9; a slab is 60 rows (hy, hz) x 8 float4, APASS passes of
  // RPP rows), dy voxel-row by voxel-row: the x index of every global load is wave-uniform, (y, z) are per-thread constants
  constexpr int APASS = 512 / NT, RPP = HY * HZ / APASS, NA = (BX + 2) * APASS;
  constexpr int DCH = 8 * MT, DROWS = NT / DCH, ND = 256 / DROWS;      // float4 per dy row, dy rows per pass, passes
  const int a_r = tid >> 3, a_c4 = tid & 7;
  const int d_r = tid / DCH, d_c4 = tid % DCH;
  float4 ra[NA], rd[ND];
  auto load_brick = [&](int bg) {
    const int sc = bg / p.bricks_per_scene, b = bg - sc * p.bricks_per_scene, xs0 = sc * p.gx;     // the scene's first x slab in x and dy
    const int bk = b % nbz, bj = (b / nbz) % nby, bi = b / (nbz * nby);
    const int X0 = bi * BX, Y0 = bj * BY, Z0 = bk * BZ;
#pragma unroll
    for (int j = 0; j < APASS; ++j) {
      const int row = j * RPP + a_r, y = Y0 + row / HZ - 1, z = Z0 + row % HZ - 1;
      const bool in = a_r < RPP && y >= 0 && y < p.gy && z >= 0 && z < p.gz;
      const unsigned voff = in ? ((unsigned)(y * p.gz + z) * (unsigned)p.Cin + ci0 + a_c4 * 4) * 4u : OOB;
#pragma unroll
      for (int i = 0; i < BX + 2; ++i) {
        const int x = X0 + i - 1;                                                       // uniform
        const bool xin = x >= 0 && x < p.gx;
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(xr, xin ? voff : OOB, xin ? (int)((unsigned)(xs0 + x) * (unsigned)(p.gy * p.gz) * (unsigned)p.Cin * 4u) : 0, 0);
        ra[i * APASS + j] = make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3]));
      }
    }
#pragma unroll
    for (int i = 0; i < ND; ++i) {
      const int vx = i * DROWS + d_r, r = vx % (BY * BZ);                               // voxel of the brick, its (by, bz) row
      const int x = X0 + vx / (BY * BZ), y = Y0 + r / BZ, z = Z0 + r % BZ;
      const bool xin = x < p.gx, in = y < p.gy && z < p.gz;
      const unsigned voff = in && xin ? ((unsigned)(y * p.gz + z) * (unsigned)p.Cout + co0 + d_c4 * 4) * 4u : OOB;
      const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(dr, voff, xin ? (int)((unsigned)(xs0 + x) * (unsigned)(p.gy * p.gz) * (unsigned)p.Cout * 4u) : 0, 0);
      rd[i] = make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3]));
    }
  };
  auto split_store = [&](const float4 &r, __bf16 *hi, __bf16 *lo, int o) {
    const float v[4] = {r.x, r.y, r.z, r.w};
    bf16x4 h, l;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const __bf16 hb = (__bf16)v[e];
      h[e] = hb;
      l[e] = (__bf16)(v[e] - (float)hb);
    }
    *reinterpret_cast<bf16x4 *>(hi + o) = h;
    *reinterpret_cast<bf16x4 *>(lo + o) = l;
  };
  auto store_brick = [&]() {
    if (a_r < RPP) {
#pragma unroll
      for (int i = 0; i < NA; ++i)
        split_store(ra[i], X_hi, X_lo, ((i / APASS) * (HY * HZ) + (i % APASS) * RPP + a_r) * PW + a_c4 * 4);
    }
#pragma unroll
    for (int i = 0; i < ND; ++i)
      split_store(rd[i], D_hi, D_lo, (d_c4 >> 3) * D_IMG + (i * DROWS + d_r) * PW + (d_c4 & 7) * 4);
  };
  // transposed fragment reads: group g = lane >> 4 reads the block of rows (8 (g >> 1) + q [+ 4]) x columns 16 (g & 1) .. + 15;
  // lane 4 q + pp of the group supplies the address of row q, columns 4 pp .. 4 pp + 3
  const int g4 = lane >> 4, q = (lane & 15) >> 2, pp = lane & 3, hh = g4 >> 1;
  const int d_lane = (8 * hh + q) * PW + 16 * (g4 & 1) + 4 * pp;           // + (16 s + 4 rd) * PW
  const int x_lane = (12 * hh + q) * PW + 16 * (g4 & 1) + 4 * pp;          // + (row(s, rd) + toff(tap)) * PW, see below
  auto tr4 = [&](const __bf16 *ptr) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4v *)ptr);
  };
  auto frag = [&](const __bf16 *p0, const __bf16 *p1) {
    const bf16x4v a = tr4(p0), b = tr4(p1);
    bf16x8 f;
    f[0] = a[0]; f[1] = a[1]; f[2] = a[2]; f[3] = a[3]; f[4] = b[0]; f[5] = b[1]; f[6] = b[2]; f[7] = b[3];
    return f;
  };
  constexpr int TPW = (27 + NW - 1) / NW;              // tap slots of a wave: taps wid + NW t; the last slot may be empty
  const bool has_last = wid + NW * (TPW - 1) < 27;     // wave-uniform
  int toff[TPW];
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    const int tt = (t < TPW - 1 || has_last) ? wid + NW * t : 13;
    toff[t] = (((tt / 9 - 1) * HY + ((tt / 3) % 3 - 1)) * HZ + (tt % 3 - 1)) * PW;
  }
  f32x16 acc[TPW][MT];
#pragma unroll
  for (int t = 0; t < TPW; ++t)
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int k = 0; k < 16; ++k) acc[t][m][k] = 0.f;

  bf16x8 ah[1][MT], al[1][MT], bh[1], bl[1];
  auto read_A = [&](int s, int buf) {                  // dy fragments of k-step s: voxels 16 s .. 16 s + 15 of the brick
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const __bf16 *dp = D_hi + m * D_IMG + d_lane + 16 * s * PW;
      ah[buf][m] = frag(dp, dp + 4 * PW);
      al[buf][m] = frag(dp + D_PLANE, dp + D_PLANE + 4 * PW);
    }
  };
  auto read_B = [&](int s, int t, int buf) {           // x fragments of k-step s shifted by tap slot t
    // halo row of voxel 16 s + 8 hh + 4 rd + q:  ((s >> 1) + 1) * 60 + (4 (s & 1) + 2 hh + rd + 1) * 6 + q + 1
    const int r0 = ((s >> 1) + 1) * (HY * HZ) + (4 * (s & 1) + 1) * HZ + 1;
    const __bf16 *xp = X_hi + x_lane + r0 * PW + toff[t];
    bh[buf] = frag(xp, xp + HZ * PW);
    bl[buf] = frag(xp + X_PLANE, xp + X_PLANE + HZ * PW);
  };

  constexpr int WSKIP = SGC_WGRAD_SKIP;
  if (WSKIP & 6) {
#pragma unroll
    for (int m = 0; m < MT; ++m) ah[0][m] = al[0][m] = bf16x8{};
    bh[0] = bl[0] = bf16x8{};
  }
  if (WSKIP & 16) {
#pragma unroll
    for (int i = 0; i < NA; ++i) ra[i] = make_float4(1.f, 2.f, 3.f, 4.f);
#pragma unroll
    for (int i = 0; i < ND; ++i) rd[i] = make_float4(1.f, 2.f, 3.f, 4.f);
  }
  if (b_lo < b_hi && !(WSKIP & 16)) load_brick(b_lo);
  for (int b = b_lo; b < b_hi; ++b) {
    __syncthreads();                                   // every wave is done with the previous brick's images
    if (!(WSKIP & 8) || b == b_lo) store_brick();
    __syncthreads();
    if (b + 1 < b_hi && !(WSKIP & 16)) load_brick(b + 1);               // lands under this brick's MFMAs
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      if (!(WSKIP & 4)) read_A(s, 0);
#pragma unroll
      for (int t = 0; t < TPW; ++t) {
        if (!(WSKIP & 2) && (t < TPW - 1 || has_last)) read_B(s, t, 0);
        if (WSKIP & 1) {                               // keep the reads alive
          asm volatile("" ::"v"(bh[0]), "v"(bl[0]));
          if (t == 0) {
#pragma unroll
            for (int m = 0; m < MT; ++m) asm volatile("" ::"v"(ah[0][m]), "v"(al[0][m]));
          }
        } else if (t < TPW - 1 || has_last) {
#pragma unroll
          for (int m = 0; m < MT; ++m) acc[t][m] = mma_split<3>(ah[0][m], al[0][m], bh[0], bl[0], acc[t][m]);
        }
      }
    }
  }
  // a lane owns column ci = lane & 31 of its 32 x 32 tiles: the 32 lanes of a half-wave store 128 contiguous bytes of one dW row
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    if (t == TPW - 1 && !has_last) break;
    float *out = p.out + ((int64_t)split * 27 + (wid + NW * t)) * p.Cout * p.Cin;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int co = co0 + 32 * m + (k & 3) + 8 * (k >> 2) + 4 * (lane >> 5);
        out[(int64_t)co * p.Cin + ci0 + (lane & 31)] = acc[t][m][k];
      }
  }
}

// ---------------------------------------------------------------------------------------------
// Double-buffered form of the halo weight gradient (round 4, late).  Timing builds of the form above (SGC_WGRAD_SKIP) show its
// phases ADD: MFMAs alone 145 us, + fragment reads 186, + the split / LDS stores of a brick and its global loads 238 -- between
// the two barriers of a brick nothing multiplies.  Here a brick is 4 x 8 x 4 voxels (halo 6 x 10 x 6 = 360 rows), BOTH LDS images
// exist twice (154 KB), four waves (one per SIMD, 512 registers) own 7 taps x MT tiles each, and the staging of brick b + 1 is
// cut into four pieces that ride behind the MFMAs of k-steps 0 - 3 of brick b (register -> split -> LDS), the global loads of
// brick b + 2 behind k-steps 4 - 7: ONE barrier per brick, the matrix pipe never waits for staging.  Fragments of the next tap
// are read ahead of the MFMAs of the current one.  Same sums in the same order per workgroup as the form above is NOT
// guaranteed (bricks differ): the two forms agree to fp32 summation order.
// ---------------------------------------------------------------------------------------------
template <int MT>
__global__ __launch_bounds__(256) void conv3d_wgrad_halo2_kernel(const WgradHaloParams p) {
  constexpr int BX = 4, BY = 8, BZ = 4, NVB = BX * BY * BZ, HY = BY + 2, HZ = BZ + 2, HROWS = (BX + 2) * HY * HZ;   // 360 halo rows
  constexpr int PW = 32, NT = 256, NW = 4, KS = NVB / 16;
  constexpr int X_PLANE = HROWS * PW, D_IMG = NVB * PW, D_PLANE = MT * D_IMG;
  constexpr int X_BUF = 2 * X_PLANE, D_BUF = 2 * D_PLANE;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_g2[];
  __bf16 *Xb = reinterpret_cast<__bf16 *>(smem_g2);             // [2 buffers][hi | lo][HROWS][32]
  __bf16 *Db = Xb + 2 * X_BUF;                                  // [2 buffers][hi | lo][MT][128][32]
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lin = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z), tiles = gridDim.x * gridDim.y;
  int split = blockIdx.z, tile = blockIdx.x + gridDim.x * blockIdx.y;
  if ((gridDim.z & 7) == 0) { split = (lin & 7) + 8 * ((lin >> 3) / tiles); tile = (lin >> 3) % tiles; }   // a brick range on one XCD
  const int co0 = (tile % gridDim.x) * (32 * MT), ci0 = (tile / gridDim.x) * 32;
  const int b_lo = split * p.bricks_per_split, b_hi = min(p.nbricks, b_lo + p.bricks_per_split);
  if (b_lo >= b_hi) return;
  const int nby = (p.gy + BY - 1) / BY, nbz = (p.gz + BZ - 1) / BZ;
  constexpr unsigned OOB = 0xfffffff0u;
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float *>(p.x), 0, (int)(unsigned)((int64_t)p.scenes * p.gx * p.gy * p.gz * p.Cin * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t dr = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float *>(p.dy), 0, (int)(unsigned)((int64_t)p.scenes * p.gx * p.gy * p.gz * p.Cout * 4), 0x00020000);
  // staging: x halo slab by slab (hx = 0 .. 5; 60 rows x 8 float4 in two passes of 30 rows), dy in passes of DROWS voxels
  constexpr int RPP = HY * HZ / 2, NA = (BX + 2) * 2;
  constexpr int DCH = 8 * MT, DROWS = NT / DCH, ND = NVB / DROWS;
  constexpr int NCH = NA + ND;                                    // float4 chunks of a brick per thread: x halo, then dy
  static_assert(NCH <= 4 * 6, "one chunk per tap slot 0 .. 5 of four k-steps");
  // threads 240 .. 255 have no halo row of their own in a pass: they repeat row RPP - 1 (same loads, same values, same LDS
  // address -- a benign duplicate) so that the staging code has no predicate and can be interleaved with the MFMAs
  const int a_r = min(tid >> 3, RPP - 1), a_c4 = tid & 7;
  const int d_r = tid / DCH, d_c4 = tid % DCH;
  float4 rs[NCH];
  int X0 = 0, Y0 = 0, Z0 = 0, XS0 = 0;                            // origin of the brick being loaded; first x slab of its scene in x and dy
  unsigned a_voff[2];
  auto load_begin = [&](int bg) {
    const int sc = bg / p.bricks_per_scene, b = bg - sc * p.bricks_per_scene;
    XS0 = sc * p.gx;
    const int bk = b % nbz, bj = (b / nbz) % nby, bi = b / (nbz * nby);
    X0 = bi * BX; Y0 = bj * BY; Z0 = bk * BZ;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int row = j * RPP + a_r, y = Y0 + row / HZ - 1, z = Z0 + row % HZ - 1;
      const bool in = y >= 0 && y < p.gy && z >= 0 && z < p.gz;
      a_voff[j] = in ? ((unsigned)(y * p.gz + z) * (unsigned)p.Cin + ci0 + a_c4 * 4) * 4u : OOB;
    }
  };
  auto load_chunk = [&](int c) {
    u32x4 v;
    if (c < NA) {
      const int slab = c >> 1, j = c & 1;
      const int x = X0 + slab - 1;                                                      // uniform
      const bool xin = x >= 0 && x < p.gx;
      v = __builtin_amdgcn_raw_buffer_load_b128(xr, xin ? a_voff[j] : OOB, xin ? (int)((unsigned)(XS0 + x) * (unsigned)(p.gy * p.gz) * (unsigned)p.Cin * 4u) : 0, 0);
    } else {
      const int vx = (c - NA) * DROWS + d_r, r = vx % (BY * BZ);
      const int x = X0 + vx / (BY * BZ), y = Y0 + r / BZ, z = Z0 + r % BZ;
      const bool in = x < p.gx && y < p.gy && z < p.gz;
      const unsigned voff = in ? ((unsigned)(((XS0 + x) * p.gy + y) * p.gz + z) * (unsigned)p.Cout + co0 + d_c4 * 4) * 4u : OOB;
      v = __builtin_amdgcn_raw_buffer_load_b128(dr, voff, 0, 0);
    }
    rs[c] = make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3]));
  };
  auto store_chunk = [&](int c, int buf) {
    const float v[4] = {rs[c].x, rs[c].y, rs[c].z, rs[c].w};
    bf16x4 h, l;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const __bf16 hb = (__bf16)v[e];
      h[e] = hb;
      l[e] = (__bf16)(v[e] - (float)hb);
    }
    __bf16 *hi;
    int plane;
    if (c < NA) {
      hi = Xb + buf * X_BUF + ((c >> 1) * (HY * HZ) + (c & 1) * RPP + a_r) * PW + a_c4 * 4;
      plane = X_PLANE;
    } else {
      hi = Db + buf * D_BUF + (d_c4 >> 3) * D_IMG + ((c - NA) * DROWS + d_r) * PW + (d_c4 & 7) * 4;
      plane = D_PLANE;
    }
    *reinterpret_cast<bf16x4 *>(hi) = h;
    *reinterpret_cast<bf16x4 *>(hi + plane) = l;
  };
  const int g4 = lane >> 4, q = (lane & 15) >> 2, pp = lane & 3, hh = g4 >> 1;
  const int d_lane = (8 * hh + q) * PW + 16 * (g4 & 1) + 4 * pp;
  const int x_lane = (12 * hh + q) * PW + 16 * (g4 & 1) + 4 * pp;
  auto tr4 = [&](const __bf16 *ptr) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4v *)ptr);
  };
  auto frag = [&](const __bf16 *p0, const __bf16 *p1) {
    const bf16x4v a = tr4(p0), b = tr4(p1);
    bf16x8 f;
    f[0] = a[0]; f[1] = a[1]; f[2] = a[2]; f[3] = a[3]; f[4] = b[0]; f[5] = b[1]; f[6] = b[2]; f[7] = b[3];
    return f;
  };
  constexpr int TPW = 7;                               // tap slots of a wave: taps wid + 4 t; wave 3's last slot is empty
  const bool has_last = wid + NW * (TPW - 1) < 27;     // wave-uniform
  int toff[TPW];
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    const int tt = (t < TPW - 1 || has_last) ? wid + NW * t : 13;
    toff[t] = (((tt / 9 - 1) * HY + ((tt / 3) % 3 - 1)) * HZ + (tt % 3 - 1)) * PW;
  }
  f32x16 acc[TPW][MT];
#pragma unroll
  for (int t = 0; t < TPW; ++t)
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int k = 0; k < 16; ++k) acc[t][m][k] = 0.f;
  bf16x8 ah[2][MT], al[2][MT], bh[3], bl[3];      // x fragments two tap slots ahead of their MFMAs
  auto read_A = [&](int s, int fb, int buf) {
    const __bf16 *D_hi = Db + buf * D_BUF;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const __bf16 *dp = D_hi + m * D_IMG + d_lane + 16 * s * PW;
      ah[fb][m] = frag(dp, dp + 4 * PW);
      al[fb][m] = frag(dp + D_PLANE, dp + D_PLANE + 4 * PW);
    }
  };
  auto read_B = [&](int s, int t, int fb, int buf) {
    const int r0 = ((s >> 1) + 1) * (HY * HZ) + (4 * (s & 1) + 1) * HZ + 1;
    const __bf16 *xp = Xb + buf * X_BUF + x_lane + r0 * PW + toff[t];
    bh[fb] = frag(xp, xp + HZ * PW);
    bl[fb] = frag(xp + X_PLANE, xp + X_PLANE + HZ * PW);
  };

  constexpr int WSKIP = SGC_WGRAD_SKIP;                // timing builds only (diag.hpp); 0 in the product
  if (WSKIP & 6) {
#pragma unroll
    for (int i = 0; i < 3; ++i) bh[i] = bl[i] = bf16x8{};
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int m = 0; m < MT; ++m) ah[i][m] = al[i][m] = bf16x8{};
  }
  load_begin(b_lo);
#pragma unroll
  for (int c = 0; c < NCH; ++c) load_chunk(c);
#pragma unroll
  for (int c = 0; c < NCH; ++c) store_chunk(c, 0);
  load_begin(min(b_lo + 1, b_hi - 1));
#pragma unroll
  for (int c = 0; c < NCH; ++c) load_chunk(c);
  __syncthreads();
  for (int b = b_lo; b < b_hi; ++b) {
    const int buf = (b - b_lo) & 1;
    // the last brick(s) of the range restage themselves once more (into the buffer nobody reads): no condition, so the
    // staging chunks below sit in the same straight-line regions as the MFMAs
    const int b_load = min(b + 2, b_hi - 1);
    // slot n = s * TPW + t of the brick; its x fragments live in ring entry n % 3 and are read two slots ahead
    if (!(WSKIP & 4)) read_A(0, 0, buf);
    if (!(WSKIP & 2)) { read_B(0, 0, 0, buf); read_B(0, 1, 1, buf); }
#pragma unroll
    for (int s = 0; s < KS; ++s) {
#pragma unroll
      for (int t = 0; t < TPW; ++t) {
        const int n = s * TPW + t, n2 = n + 2, s2 = n2 / TPW, t2 = n2 % TPW;
        if (s2 < KS) {
          if (t2 == 0 && !(WSKIP & 4)) read_A(s2, s2 & 1, buf);        // dy fragments of the next k-step, two slots ahead as well
          if (!(WSKIP & 2)) read_B(s2, t2, n2 % 3, buf);
        }
        // one staging chunk per tap slot 0 .. 5: k-steps 0 - 3 split + store brick b + 1 (loaded during the previous brick),
        // k-steps 4 - 7 load brick b + 2.  The chunk's ~30 vector instructions go BETWEEN this slot's MFMAs (group fences):
        // a lone wave per SIMD issues in order, so a lump of staging code after the MFMAs would leave the pipe idle
        const int ch = (s & 3) * 6 + t;
        const bool stage = t < 6 && ch < NCH;
        if (WSKIP & 1) {
          asm volatile("" ::"v"(bh[n % 3]), "v"(bl[n % 3]));
          if (t == 0) {
#pragma unroll
            for (int m = 0; m < MT; ++m) asm volatile("" ::"v"(ah[s & 1][m]), "v"(al[s & 1][m]));
          }
        } else if (t < TPW - 1 || has_last) {
          // product-major: consecutive MFMAs go to different accumulators (the group fences below keep this order) -- not mma_split,
          // which would put a tile's three products back to back on one chain
#pragma unroll
          for (int m = 0; m < MT; ++m) acc[t][m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[s & 1][m], bh[n % 3], acc[t][m], 0, 0, 0);
#pragma unroll
          for (int m = 0; m < MT; ++m) acc[t][m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[s & 1][m], bl[n % 3], acc[t][m], 0, 0, 0);
#pragma unroll
          for (int m = 0; m < MT; ++m) acc[t][m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[s & 1][m], bh[n % 3], acc[t][m], 0, 0, 0);
        }
        if (stage) {
          if (s < 4) { if (!(WSKIP & 8)) store_chunk(ch, buf ^ 1); }
          else if (!(WSKIP & 16)) { if (ch == 0) load_begin(b_load); load_chunk(ch); }
        }
        // issue order of the slot: after every MFMA a share of the slot's LDS reads (they feed the slot after next) and of
        // the staging chunk's vector work.  A wave issues in order and an LDS instruction holds the issue port for several
        // cycles: four reads in a row, or a lump of staging code, let the matrix pipe run dry behind the one MFMA in flight
        {
          const bool two = s2 < KS && t2 == 0, st = stage && s < 4;       // 4 + 4 MT reads in the slot / a store chunk in it
#pragma unroll
          for (int i = 0; i < 3 * MT; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            if (two) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
            else __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            if (st) __builtin_amdgcn_sched_group_barrier(0x002, 6, 0);
          }
          if (st) __builtin_amdgcn_sched_group_barrier(0x200, 2, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    __syncthreads();                                   // publishes brick b + 1; every wave is done reading brick b
  }
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    if (t == TPW - 1 && !has_last) break;
    float *out = p.out + ((int64_t)split * 27 + (wid + NW * t)) * p.Cout * p.Cin;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int co = co0 + 32 * m + (k & 3) + 8 * (k >> 2) + 4 * (lane >> 5);
        out[(int64_t)co * p.Cin + ci0 + (lane & 31)] = acc[t][m][k];
      }
  }
}

// wgrad_halo: 3x3x3 stride-1 layers with Cin, Cout multiples of 32: 1 double-buffered halo form, 2 single-buffered, 0 tile kernel
// (the form is chosen from the per-scene grid; the bricks of all scenes are one range, split over the workgroups of the launch)
static bool wgrad_halo_geometry(WgradHaloParams &h, int &mt, int ix, int iy, int iz, int Cin, int Cout, int ksize, int stride, int scenes = 1) {
  if (!g_tune_wgrad_halo || ksize != 3 || stride != 1 || (Cin & 31) || (Cout & 31)) return false;
  if ((int64_t)scenes * ix * iy * iz * (Cin > Cout ? Cin : Cout) * 4 >= 0xfffffff0ll - 65536) return false;
  h.Cin = Cin; h.Cout = Cout; h.gx = ix; h.gy = iy; h.gz = iz;
  const bool db = g_tune_wgrad_halo == 1;                                       // double-buffered form (default): bricks of 4 x 8 x 4
  h.scenes = scenes;
  h.bricks_per_scene = ceil_div(ix, db ? 4 : 8) * ceil_div(iy, 8) * ceil_div(iz, 4);
  h.nbricks = scenes * h.bricks_per_scene;
  if ((int64_t)h.bricks_per_scene * (db ? 128 : 256) > (int64_t)2 * ix * iy * iz) return false;       // bricks mostly padding: the tile kernel wins
  mt = (Cout & 63) ? 1 : 2;
  const int tiles = (Cout / (32 * mt)) * (Cin / 32);
  const int splits = std::max(1, std::min(h.nbricks / 4, ceil_div(256, tiles)));      // fill the chip; >= 4 bricks per workgroup
  h.bricks_per_split = ceil_div(h.nbricks, splits);
  return true;
}

__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float4 *__restrict__ ws, float4 *__restrict__ dw, int64_t n4, int splits) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    float4 a = ws[i];
    for (int s = 1; s < splits; ++s) {                      // fixed order: deterministic
      const float4 b = ws[(int64_t)s * n4 + i];
      a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    }
    dw[i] = a;
  }
}

// Reduction rows, K steps, split count and the carried-coordinate digits of a geometry whose (ox, oy, oz), taps and channel counts are set.
static int wgrad_split_plan(WgradParams &p, const char *who) {
  const int Cin = p.Cin, Cout = p.Cout;
  if (p.scenes < 1) p.scenes = 1;
  const int OV1 = p.ox * p.oy * p.oz;
  if ((int64_t)p.scenes * OV1 >= ((int64_t)1 << 30)) return set_error(SGC_EUNSUP, "%s: too many rows", who);
  p.OV = p.scenes * OV1;
  p.ksteps = ceil_div(p.OV, 32);
  const int tiles = ceil_div(Cout, 128) * ceil_div(Cin, 128) * p.taps;
  int splits = 1;
  while (tiles * splits < 512 && p.ksteps / (splits * 2) >= 16) splits *= 2;     // fill the chip twice over; >= 16 K-steps per split
  // a layer that still leaves most CUs idle (the nn.Linear layers of a level: 800 rows, 4 tiles) is bound by the load latency
  // of its serial K-steps (~2.5 us each), not by flops: spread the steps over idle CUs, down to 3 per workgroup
  while (tiles * splits < 256 && p.ksteps / (splits * 2) >= 3) splits *= 2;
  p.steps_per_split = ceil_div(p.ksteps, splits);
  p.splits = ceil_div(p.ksteps, p.steps_per_split);
  p.by = (32 % (p.oy * p.oz)) / p.oz; p.cz = 32 % p.oz;
  if (p.scenes > 1) { p.as = 32 / OV1; p.ax = (32 % OV1) / (p.oy * p.oz); }      // a batch carries a scene digit above x
  else { p.as = 0; p.ax = 32 / (p.oy * p.oz); }
  if ((int64_t)p.OV * Cout * 4 >= 0xfffffff0ll - 65536 || (int64_t)p.scenes * p.ix * p.iy * p.iz * Cin * 4 >= 0xfffffff0ll - 65536)
    return set_error(SGC_EUNSUP, "%s: x and dy must stay below 4 GiB each", who);
  return SGC_OK;
}

static int wgrad_geometry(WgradParams &p, int ix, int iy, int iz, int Cin, int Cout, int ksize, int stride, int scenes = 1) {
  p.scenes = scenes;
  if (Cin <= 0 || Cout <= 0 || ix <= 0 || iy <= 0 || iz <= 0) return set_error(SGC_EINVAL, "sgc_conv3d_wgrad_bf16x3: bad size");
  if ((Cin & 3) || (Cout & 3)) return set_error(SGC_EUNSUP, "sgc_conv3d_wgrad_bf16x3: Cin and Cout must be multiples of 4");
  if (ksize == 2) {
    if (stride != 2 || (ix & 1) || (iy & 1) || (iz & 1)) return set_error(SGC_EUNSUP, "sgc_conv3d_wgrad_bf16x3: ksize 2 needs stride 2 and an even grid");
    p.pad = 0;
  } else if ((ksize == 1 || ksize == 3) && (stride == 1 || stride == 2)) {
    p.pad = ksize / 2;
  } else {
    return set_error(SGC_EUNSUP, "sgc_conv3d_wgrad_bf16x3: ksize in {1,2,3}, stride in {1,2}");
  }
  p.Cin = Cin; p.Cout = Cout; p.ix = ix; p.iy = iy; p.iz = iz; p.ksize = ksize; p.stride = stride;
  p.taps = ksize * ksize * ksize;
  p.ox = (ix + 2 * p.pad - ksize) / stride + 1; p.oy = (iy + 2 * p.pad - ksize) / stride + 1; p.oz = (iz + 2 * p.pad - ksize) / stride + 1;
  return wgrad_split_plan(p, "sgc_conv3d_wgrad_bf16x3");
}

// The 2-D form: (ix, iy, iz) = (N, H, W), the image index takes no part in the window (see the kernel's IMG policy).
static int wgrad2d_geometry(WgradParams &p, int N, int H, int W, int Cin, int Cout, int ksize, int stride) {
  if (Cin <= 0 || Cout <= 0 || N <= 0 || H <= 0 || W <= 0) return set_error(SGC_EINVAL, "sgc_conv2d_wgrad_bf16x3: bad size");
  if ((Cin & 3) || (Cout & 3)) return set_error(SGC_EUNSUP, "sgc_conv2d_wgrad_bf16x3: Cin and Cout must be multiples of 4");
  if ((ksize != 1 && ksize != 3) || (stride != 1 && stride != 2))
    return set_error(SGC_EUNSUP, "sgc_conv2d_wgrad_bf16x3: ksize in {1,3}, stride in {1,2}");
  if ((int64_t)N * H * W >= ((int64_t)1 << 30)) return set_error(SGC_EUNSUP, "sgc_conv2d_wgrad_bf16x3: too many rows");
  p.pad = ksize / 2;
  p.Cin = Cin; p.Cout = Cout; p.ix = N; p.iy = H; p.iz = W; p.ksize = ksize; p.stride = stride;
  p.taps = ksize * ksize;
  p.ox = N; p.oy = (H + 2 * p.pad - ksize) / stride + 1; p.oz = (W + 2 * p.pad - ksize) / stride + 1;      // ceil(H / s), ceil(W / s)
  return wgrad_split_plan(p, "sgc_conv2d_wgrad_bf16x3");
}

// The tile kernel (and the fixed-order reduction behind a split) on a prepared geometry: shared by the 3-D and the 2-D entry.
template <bool IMG>
static int wgrad_tile_launch(WgradParams &p, const float *x, const float *dy, float *dw, float *workspace_or_null, int64_t workspace_floats,
                             sgc_stream_t stream) {
  p.x = x; p.dy = dy;
  const int64_t n = (int64_t)p.taps * p.Cout * p.Cin;
  if (p.splits > 1 && !(workspace_or_null && workspace_floats >= p.splits * n)) {     // no workspace: one split (slower, same result class)
    p.splits = 1;
    p.steps_per_split = p.ksteps;
  }
  p.out = p.splits > 1 ? workspace_or_null : dw;
  hipStream_t st = (hipStream_t)stream;
  const size_t smem = (size_t)2 * 4 * 128 * LDKH * sizeof(uint16_t);
  static std::atomic<uint64_t> attr_done{0};
  static std::atomic<uint64_t> attr_done8{0};
  const dim3 wgrid(ceil_div(p.Cout, 128), ceil_div(p.Cin, 128), p.taps * p.splits);
  if (!IMG && p.scenes > 1) {                              // a batch of volumes: the kernels with the scene digit
    static std::atomic<uint64_t> attr_sc{0}, attr_sc8{0};
    ensure_dynamic_lds((const void *)conv3d_wgrad_bf16x3_kernel<2, false, true>, (int)smem, attr_sc);
    ensure_dynamic_lds((const void *)conv3d_wgrad_bf16x3_kernel<4, false, true>, (int)smem, attr_sc8);
    if (g_tune_wgrad_waves == 8) hipLaunchKernelGGL((conv3d_wgrad_bf16x3_kernel<4, false, true>), wgrid, dim3(512), smem, st, p);
    else hipLaunchKernelGGL((conv3d_wgrad_bf16x3_kernel<2, false, true>), wgrid, dim3(256), smem, st, p);
  } else {
    ensure_dynamic_lds((const void *)conv3d_wgrad_bf16x3_kernel<2, IMG>, (int)smem, attr_done);
    ensure_dynamic_lds((const void *)conv3d_wgrad_bf16x3_kernel<4, IMG>, (int)smem, attr_done8);
    if (g_tune_wgrad_waves == 8) hipLaunchKernelGGL((conv3d_wgrad_bf16x3_kernel<4, IMG>), wgrid, dim3(512), smem, st, p);
    else hipLaunchKernelGGL((conv3d_wgrad_bf16x3_kernel<2, IMG>), wgrid, dim3(256), smem, st, p);
  }
  int rc = check_launch("conv3d_wgrad_bf16x3_kernel");
  if (rc) return rc;
  if (p.splits > 1) {
    const int64_t n4 = n / 4;
    const int g = (int)((n4 + 255) / 256 < 4096 ? (n4 + 255) / 256 : 4096);
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(g), dim3(256), 0, st, reinterpret_cast<const float4 *>(workspace_or_null),
                       reinterpret_cast<float4 *>(dw), n4, p.splits);
    rc = check_launch("wgrad_reduce_kernel");
  }
  return rc;
}

extern "C" int64_t sgc_conv3d_wgrad_batched_workspace_floats(int ix, int iy, int iz, int Cin, int Cout, int ksize, int stride, int scenes) {
  if (scenes < 1) return -1;
  WgradHaloParams h = {};
  int mt = 1;
  if (wgrad_halo_geometry(h, mt, ix, iy, iz, Cin, Cout, ksize, stride, scenes)) {
    const int splits = ceil_div(h.nbricks, h.bricks_per_split);
    return splits > 1 ? (int64_t)splits * 27 * Cout * Cin : 0;
  }
  WgradParams p = {};
  if (wgrad_geometry(p, ix, iy, iz, Cin, Cout, ksize, stride, scenes)) return -1;
  return p.splits > 1 ? (int64_t)p.splits * p.taps * Cout * Cin : 0;
}
extern "C" int64_t sgc_conv3d_wgrad_workspace_floats(int ix, int iy, int iz, int Cin, int Cout, int ksize, int stride) {
  return sgc_conv3d_wgrad_batched_workspace_floats(ix, iy, iz, Cin, Cout, ksize, stride, 1);
}

// The weight gradient of a scene batch: x [scenes * ix*iy*iz, Cin] and dy [scenes * OV, Cout] (scene s first), dw summed over the
// scenes INSIDE the launch -- to the kernels the scene axis is more reduction rows (tile kernel) or more bricks (halo forms); no
// tap crosses a scene's border.  scenes = 1 IS sgc_conv3d_wgrad_bf16x3.
extern "C" int sgc_conv3d_wgrad_bf16x3_batched(const float *x, const float *dy, float *dw, int ix, int iy, int iz, int Cin, int Cout,
                                               int ksize, int stride, int scenes, float *workspace_or_null, int64_t workspace_floats,
                                               sgc_stream_t stream) {
  if (!x || !dy || !dw) return set_error(SGC_EINVAL, "sgc_conv3d_wgrad_bf16x3: null pointer");
  if (scenes < 1) return set_error(SGC_EINVAL, "sgc_conv3d_wgrad_bf16x3_batched: scenes must be >= 1");
  if (((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dw | (uintptr_t)workspace_or_null) & 15)
    return set_error(SGC_EINVAL, "sgc_conv3d_wgrad_bf16x3: pointers must be 16-byte aligned");
  hipStream_t st0 = (hipStream_t)stream;
  WgradHaloParams h = {};
  int mt = 1;
  if (wgrad_halo_geometry(h, mt, ix, iy, iz, Cin, Cout, ksize, stride, scenes)) {
    int splits = ceil_div(h.nbricks, h.bricks_per_split);
    const int64_t n27 = (int64_t)27 * Cout * Cin;
    if (splits > 1 && !(workspace_or_null && workspace_floats >= splits * n27)) { splits = 1; h.bricks_per_split = h.nbricks; }
    h.x = x; h.dy = dy; h.out = splits > 1 ? workspace_or_null : dw;
    const size_t smem_h = (size_t)2 * (600 + 256 * mt) * 32 * sizeof(uint16_t);
    static std::atomic<uint64_t> attr_h[4] = {};
    const dim3 grid_h(Cout / (32 * mt), Cin / 32, splits >= 8 ? (splits + 7) / 8 * 8 : splits);
    if (g_tune_wgrad_halo == 1) {                      // double-buffered bricks of 4 x 8 x 4 (default)
      const size_t smem2 = (size_t)2 * 2 * (360 + 128 * mt) * 32 * sizeof(uint16_t);
      if (mt == 2) {
        ensure_dynamic_lds((const void *)conv3d_wgrad_halo2_kernel<2>, (int)smem2, attr_h[0]);
        hipLaunchKernelGGL(conv3d_wgrad_halo2_kernel<2>, grid_h, dim3(256), smem2, st0, h);
      } else {
        ensure_dynamic_lds((const void *)conv3d_wgrad_halo2_kernel<1>, (int)smem2, attr_h[1]);
        hipLaunchKernelGGL(conv3d_wgrad_halo2_kernel<1>, grid_h, dim3(256), smem2, st0, h);
      }
    } else if (mt == 2) {                              // single-buffered bricks of 8 x 8 x 4, eight waves
      ensure_dynamic_lds((const void *)conv3d_wgrad_halo_kernel<2, 8>, (int)smem_h, attr_h[2]);
      hipLaunchKernelGGL((conv3d_wgrad_halo_kernel<2, 8>), grid_h, dim3(512), smem_h, st0, h);
    } else {
      ensure_dynamic_lds((const void *)conv3d_wgrad_halo_kernel<1, 8>, (int)smem_h, attr_h[3]);
      hipLaunchKernelGGL((conv3d_wgrad_halo_kernel<1, 8>), grid_h, dim3(512), smem_h, st0, h);
    }
    int rch = check_launch("conv3d_wgrad_halo_kernel");
    if (rch) return rch;
    if (splits > 1) {
      const int64_t n4 = n27 / 4;
      const int g = (int)((n4 + 255) / 256 < 4096 ? (n4 + 255) / 256 : 4096);
      hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(g), dim3(256), 0, st0, reinterpret_cast<const float4 *>(workspace_or_null),
                         reinterpret_cast<float4 *>(dw), n4, splits);
      rch = check_launch("wgrad_reduce_kernel");
    }
    return rch;
  }
  WgradParams p = {};
  int rc = wgrad_geometry(p, ix, iy, iz, Cin, Cout, ksize, stride, scenes);
  if (rc) return rc;
  return wgrad_tile_launch<false>(p, x, dy, dw, workspace_or_null, workspace_floats, stream);
}

extern "C" int sgc_conv3d_wgrad_bf16x3(const float *x, const float *dy, float *dw, int ix, int iy, int iz, int Cin, int Cout,
                                       int ksize, int stride, float *workspace_or_null, int64_t workspace_floats,
                                       sgc_stream_t stream) {
  return sgc_conv3d_wgrad_bf16x3_batched(x, dy, dw, ix, iy, iz, Cin, Cout, ksize, stride, 1, workspace_or_null, workspace_floats, stream);
}

extern "C" int64_t sgc_conv2d_wgrad_workspace_floats(int N, int H, int W, int Cin, int Cout, int ksize, int stride) {
  WgradParams p = {};
  if (wgrad2d_geometry(p, N, H, W, Cin, Cout, ksize, stride)) return -1;
  return p.splits > 1 ? (int64_t)p.splits * p.taps * Cout * Cin : 0;
}

extern "C" int sgc_conv2d_wgrad_bf16x3(const float *x, const float *dy, float *dw, int N, int H, int W, int Cin, int Cout, int ksize,
                                       int stride, float *workspace_or_null, int64_t workspace_floats, sgc_stream_t stream) {
  if (!x || !dy || !dw) return set_error(SGC_EINVAL, "sgc_conv2d_wgrad_bf16x3: null pointer");
  if (((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dw | (uintptr_t)workspace_or_null) & 15)
    return set_error(SGC_EINVAL, "sgc_conv2d_wgrad_bf16x3: pointers must be 16-byte aligned");
  WgradParams p = {};
  const int rc = wgrad2d_geometry(p, N, H, W, Cin, Cout, ksize, stride);
  if (rc) return rc;
  return wgrad_tile_launch<true>(p, x, dy, dw, workspace_or_null, workspace_floats, stream);
}
