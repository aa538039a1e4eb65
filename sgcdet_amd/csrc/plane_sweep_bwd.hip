// Backward of the fused plane-sweep matching cost (csrc/plane_sweep.hip): the gradient of
//   corr[n,d,p] = (1/K) sum_k ( sum_c S_{n,k,d,p}[c] * f[n,p,c] ) / sqrt(C)
// with respect to the matching features f, where S is the bilinear sample (zeros padding, align_corners = False) of
// view m = nbr[n,k] at the warped position of pixel p on plane d.  The reference builds the sampling grid under
// torch.no_grad() (depth_est_fusion.py homo_warping :87-126), so positions carry no gradient; f plays two roles and one
// grad_feat [N, H*W, C] receives both terms (scale s = 1 / (K sqrt(C))):
//   reference role  grad[n,p,:] += s * sum_k sum_d g[n,d,p] * S_{n,k,d,p}[:]                 -- a gather, as the forward
//   neighbour role  grad[m,q,:] += s * g[n,d,p] * w_corner * f[n,p,:]  for the 4 corners q     -- a scatter
// Sizing: at 40 views x 128 ch x 60x80 x 12 planes x 2 neighbours the scatter is 18.4 M contributions of
// one 512-B row (9.4 GB); as row atomics at the chip-wide float-atomic rate (~1.3 TB/s) that is ~7 ms.  Instead the
// scatter is inverted into a destination-major list of scalar coefficients (store-and-sum):
//   1. count   one thread per (n,k,p), all D planes: number of on-image corners landing on each destination row;
//   2. scan    exclusive scan of the counts -> list offsets; lists longer than PSB_CHUNK become chunk work items;
//   3. fill    the same walk again: (source row n*HW+p, coefficient g[n,d,p] * w_corner) at offset + slot;
//   4. final   one wave per row (n,p): the reference-role gather (the forward's loop) plus, for a list of at most
//              PSB_CHUNK entries, the neighbour-role sum sum_e coef_e * f[src_e,:] over the list sorted in LDS (a fixed
//              order); one plain store;
//   5. long    one wave per PSB_CHUNK-entry chunk of a longer list: its partial sum is added to the row with f32 row
//              atomics (256 contiguous bytes per wave instruction); only skewed lists take this path.
// Reproducibility: the slot of an entry inside its list is taken with an integer atomic in pass 3; pass 4 sorts each
// short list by its contents before summing, so grad_feat is bitwise reproducible run to run whenever no list is longer
// than PSB_CHUNK (every row at the measured shapes).  A longer list is summed in atomic-fill order and
// its chunks are added by float atomics: those rows differ from run to run by fp32 reordering only.
// Which corners count follows the forward exactly (both call plane_sweep_corners, sample_geom.hpp): a corner off the image
// or a non-finite position adds nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/sgcdet_amd_train.h"
#include "common.hpp"

#pragma clang fp contract(off)   // the sample position decides which pixels are read: keep the forward's op order

namespace sgc {

constexpr int PSB_MAXD = 32;
constexpr int PSB_CHUNK = 512;           // entries per wave of a split list (Appendix B: 512-row chunks measured)
constexpr int PSB_SCAN = 2048;           // counts per workgroup of the scan (256 threads x 8)

__global__ __launch_bounds__(256) void psb_zero_kernel(uint32_t *__restrict__ p, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = 0u;
}

// Passes 1 and 3: one thread per (n, k, p), planes in a loop.  FILL = false counts, FILL = true writes the entries.
template <bool FILL>
__global__ __launch_bounds__(256) void psb_route_kernel(const int32_t *__restrict__ nbr, const float *__restrict__ rt,
                                                        const float *__restrict__ depth, const float *__restrict__ grad_corr,
                                                        uint32_t *__restrict__ cnt, const uint32_t *__restrict__ off,
                                                        int2 *__restrict__ entries, int N, int K, int H, int W, int D) {
  const int HW = H * W;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)N * K * HW) return;
  const int p = (int)(t % HW), nk = (int)(t / HW), n = nk / K;
  const float fx = (float)(p % W), fy = (float)(p / W);
  const float *m = rt + (int64_t)nk * 12;
  const float rx = m[0] * fx + m[1] * fy + m[2], ry = m[4] * fx + m[5] * fy + m[6], rz = m[8] * fx + m[9] * fy + m[10];
  const int m_view = nbr[nk];
  if (m_view < 0 || m_view >= N) return;             // an id outside [0, N) adds nothing (no host sync to check it)
  const int64_t dst0 = (int64_t)m_view * HW;
  const int src = n * HW + p;
  for (int d = 0; d < D; ++d) {
    const PlaneSweepCorners c = plane_sweep_corners(rx, ry, rz, m, depth[d], H, W);
    const float g = FILL ? grad_corr[((int64_t)n * D + d) * HW + p] : 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (!c.ok[q]) continue;
      const int64_t dst = dst0 + c.idx[q];
      if (!FILL) {
        atomicAdd(&cnt[dst], 1u);
      } else {
        const uint32_t pos = off[dst] + atomicSub(&cnt[dst], 1u) - 1u;     // counts run back down to zero
        if (pos < off[dst + 1]) entries[pos] = make_int2(src, __float_as_int(g * c.w[q]));   // same walk as the count
      }
    }
  }
}

// Exclusive scan over the 256 threads of a workgroup (one value each): returns the prefix of `v` before this thread
// and writes the workgroup total to *total.  Every thread of the workgroup must call it.
__device__ __forceinline__ uint32_t psb_block_excl(uint32_t v, uint32_t *total) {
  __shared__ uint32_t wsum[4];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  uint32_t incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(incl, o);
    if (lane >= o) incl += y;
  }
  if (lane == 63) wsum[wid] = incl;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    before += w < wid ? wsum[w] : 0u;
    all += wsum[w];
  }
  __syncthreads();
  *total = all;
  return before + incl - v;
}

// Pass 2a: per-workgroup totals of PSB_SCAN counts.
__global__ __launch_bounds__(256) void psb_scan_reduce_kernel(const uint32_t *__restrict__ cnt, uint32_t *__restrict__ bsum,
                                                              int n) {
  const int64_t i0 = (int64_t)blockIdx.x * PSB_SCAN + threadIdx.x * 8;
  uint32_t s = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) s += i0 + j < n ? cnt[i0 + j] : 0u;
  uint32_t total;
  psb_block_excl(s, &total);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// Pass 2b: one workgroup, exclusive scan of the workgroup totals in place; off[n] = grand total.
__global__ __launch_bounds__(256) void psb_scan_top_kernel(uint32_t *__restrict__ bsum, uint32_t *__restrict__ off, int nb,
                                                           int n) {
  uint32_t carry = 0;
  for (int b0 = 0; b0 < nb; b0 += 256) {
    const int b = b0 + threadIdx.x;
    const uint32_t v = b < nb ? bsum[b] : 0u;
    uint32_t total;
    const uint32_t ex = psb_block_excl(v, &total);
    if (b < nb) bsum[b] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) off[n] = carry;
}

// Pass 2c: list offsets; every list longer than PSB_CHUNK appends its chunks (row, chunk) to the work list.
__global__ __launch_bounds__(256) void psb_scan_apply_kernel(const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ bsum,
                                                             uint32_t *__restrict__ off, uint32_t *__restrict__ n_work,
                                                             int2 *__restrict__ work, int n) {
  const int64_t i0 = (int64_t)blockIdx.x * PSB_SCAN + threadIdx.x * 8;
  uint32_t c[8], s = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    c[j] = i0 + j < n ? cnt[i0 + j] : 0u;
    s += c[j];
  }
  uint32_t total;
  uint32_t run = bsum[blockIdx.x] + psb_block_excl(s, &total);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (i0 + j >= n) break;
    off[i0 + j] = run;
    run += c[j];
    if (c[j] > (uint32_t)PSB_CHUNK) {
      const int nch = (int)((c[j] + PSB_CHUNK - 1) / PSB_CHUNK);
      const uint32_t w0 = atomicAdd(n_work, (uint32_t)nch);
      for (int h = 0; h < nch; ++h) work[w0 + h] = make_int2((int)(i0 + j), h);
    }
  }
}

// sum over entries [b, e) of coef * f[src, :], e - b arbitrary; lanes own channels v * 64 + lane.
template <int VPL>
__device__ __forceinline__ void psb_list_sum(const float *__restrict__ feat, const int2 *__restrict__ entries, uint32_t b,
                                             uint32_t e, int C, int lane, float acc[VPL]) {
  for (uint32_t base = b; base < e; base += 64) {
    const uint32_t nn = min(e - base, 64u);
    const int2 en = lane < (int)nn ? entries[base + lane] : make_int2(0, 0);   // padding: row 0 with weight 0
    constexpr int U = 8;
    for (int j0 = 0; j0 < (int)nn; j0 += U) {
      float coef[U], val[U][VPL];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int j = min(j0 + u, 63);
        const int src = __builtin_amdgcn_readlane(en.x, j);
        coef[u] = j0 + u < (int)nn ? __int_as_float(__builtin_amdgcn_readlane(en.y, j)) : 0.f;
        const float *row = feat + (int64_t)src * C;
#pragma unroll
        for (int v = 0; v < VPL; ++v) val[u][v] = v * 64 + lane < C ? row[v * 64 + lane] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int v = 0; v < VPL; ++v) acc[v] += coef[u] * val[u][v];
    }
  }
}

// Orders the entries [b, e) of one list (e - b <= PSB_CHUNK) by (source row, coefficient bits) into the wave's LDS
// slice `out`: the slots pass 3 took with atomics vary from run to run, the sorted order depends only on the list's
// contents (equal keys are equal entries), so the sum over it is bitwise reproducible.  Rank sort: each lane owns
// entries lane, lane + 64, ...; rank = keys below + equal keys at a lower index.
__device__ __forceinline__ void psb_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ void psb_sort_list(const int2 *__restrict__ entries, uint32_t b, uint32_t e, int lane,
                                              uint64_t *keys, int2 *out) {
  constexpr int T = PSB_CHUNK / 64;
  const int n = (int)(e - b);
  uint64_t mine[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int i = t * 64 + lane;
    mine[t] = ~0ull;
    if (i < n) {
      const int2 en = entries[b + i];
      mine[t] = ((uint64_t)(uint32_t)en.x << 32) | (uint32_t)en.y;
      keys[i] = mine[t];
    }
  }
  psb_wave_sync();
  int rank[T];
#pragma unroll
  for (int t = 0; t < T; ++t) rank[t] = 0;
  const int nt = (n + 63) / 64;                      // entries per lane in use: compare only those (uniform)
  for (int j = 0; j < n; ++j) {
    const uint64_t kj = keys[j];
#pragma unroll
    for (int t = 0; t < T; ++t)
      if (t < nt) rank[t] += (kj < mine[t] || (kj == mine[t] && j < t * 64 + lane)) ? 1 : 0;
  }
#pragma unroll
  for (int t = 0; t < T; ++t)
    if (t * 64 + lane < n) out[rank[t]] = make_int2((int)(uint32_t)(mine[t] >> 32), (int)(uint32_t)mine[t]);
  psb_wave_sync();
}

// Pass 4: one wave per row (n, p).  Reference role with the forward's loop (planes in groups of DG, all corner loads
// of a group issued together), then the neighbour-role list when it is short; one plain store of the row.
template <int VPL>
__global__ __launch_bounds__(256) void psb_final_kernel(const float *__restrict__ feat, const int32_t *__restrict__ nbr,
                                                        const float *__restrict__ rt, const float *__restrict__ depth,
                                                        const float *__restrict__ grad_corr, const uint32_t *__restrict__ off,
                                                        const int2 *__restrict__ entries, float *__restrict__ grad_feat, int N,
                                                        int K, int H, int W, int C, int D, float scale) {
  const int lane = threadIdx.x & 63;
  const int HW = H * W;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (int64_t)N * HW) return;
  const int n = (int)(row / HW), pix = (int)(row % HW);
  const float fx = (float)(pix % W), fy = (float)(pix / W);
  const float gl = lane < D ? grad_corr[((int64_t)n * D + lane) * HW + pix] : 0.f;   // g[n, lane, p]
  float acc[VPL];
#pragma unroll
  for (int v = 0; v < VPL; ++v) acc[v] = 0.f;
  constexpr int DG = 4;
  for (int k = 0; k < K; ++k) {
    const float *m = rt + ((int64_t)n * K + k) * 12;
    const float rx = m[0] * fx + m[1] * fy + m[2], ry = m[4] * fx + m[5] * fy + m[6], rz = m[8] * fx + m[9] * fy + m[10];
    const int m_view = nbr[n * K + k];
    if (m_view < 0 || m_view >= N) continue;          // as in the route kernel: nothing is read or added
    const float *src = feat + (int64_t)m_view * HW * C;
    for (int d0 = 0; d0 < D; d0 += DG) {
      int64_t idx[DG][4];
      float wg[DG][4];
#pragma unroll
      for (int j = 0; j < DG; ++j) {
        const int d = min(d0 + j, D - 1);
        const PlaneSweepCorners c = plane_sweep_corners(rx, ry, rz, m, depth[d], H, W);
        const float g = d0 + j < D ? __int_as_float(__builtin_amdgcn_readlane(__float_as_int(gl), d)) : 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          idx[j][q] = (int64_t)c.idx[q] * C;
          wg[j][q] = g * c.w[q];
        }
      }
      float val[DG][4][VPL];
#pragma unroll
      for (int j = 0; j < DG; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int v = 0; v < VPL; ++v) {
            const int c = v * 64 + lane;
            val[j][q][v] = c < C ? src[idx[j][q] + c] : 0.f;
          }
#pragma unroll
      for (int j = 0; j < DG; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int v = 0; v < VPL; ++v) acc[v] += wg[j][q] * val[j][q][v];
    }
  }
  const uint32_t b = off[row], e = off[row + 1];
  if (e - b <= (uint32_t)PSB_CHUNK) {
    __shared__ uint64_t keys_s[4][PSB_CHUNK];
    __shared__ int2 sorted_s[4][PSB_CHUNK];
    const int wid = threadIdx.x >> 6;
    psb_sort_list(entries, b, e, lane, keys_s[wid], sorted_s[wid]);
    psb_list_sum<VPL>(feat, sorted_s[wid], 0, e - b, C, lane, acc);
  }
  float *out = grad_feat + row * C;
#pragma unroll
  for (int v = 0; v < VPL; ++v)
    if (v * 64 + lane < C) out[v * 64 + lane] = acc[v] * scale;
}

// Pass 5: one wave per chunk of a long list (grid-stride over the work list), partial sum added to the row.
template <int VPL>
__global__ __launch_bounds__(256) void psb_long_kernel(const float *__restrict__ feat, const uint32_t *__restrict__ off,
                                                       const int2 *__restrict__ entries, const uint32_t *__restrict__ n_work,
                                                       const int2 *__restrict__ work, float *__restrict__ grad_feat, int C,
                                                       float scale) {
  const int lane = threadIdx.x & 63;
  const uint32_t nw = *n_work;
  for (uint32_t it = blockIdx.x * 4 + (threadIdx.x >> 6); it < nw; it += gridDim.x * 4) {
    const int2 wk = work[it];
    const uint32_t b = off[wk.x] + (uint32_t)wk.y * PSB_CHUNK, e = min(b + (uint32_t)PSB_CHUNK, off[wk.x + 1]);
    float acc[VPL];
#pragma unroll
    for (int v = 0; v < VPL; ++v) acc[v] = 0.f;
    psb_list_sum<VPL>(feat, entries, b, e, C, lane, acc);
    float *out = grad_feat + (int64_t)wk.x * C;
#pragma unroll
    for (int v = 0; v < VPL; ++v)
      if (v * 64 + lane < C) atomicAdd(&out[v * 64 + lane], acc[v] * scale);
  }
}

// Workspace layout (byte offsets, each region 256-B aligned).
struct PsbLayout {
  int64_t cnt, off, bsum, n_work, work, entries, total;
};

static inline int64_t psb_align(int64_t x) { return (x + 255) / 256 * 256; }

static PsbLayout psb_layout(int N, int K, int H, int W, int D) {
  const int64_t rows = (int64_t)N * H * W, e_max = rows * K * D * 4;
  const int64_t nb = (rows + PSB_SCAN - 1) / PSB_SCAN;
  PsbLayout L;
  L.cnt = 0;
  L.off = L.cnt + psb_align(4 * rows);
  L.bsum = L.off + psb_align(4 * (rows + 1));
  L.n_work = L.bsum + psb_align(4 * nb);
  L.work = L.n_work + 256;
  L.entries = L.work + psb_align(8 * (2 * e_max / PSB_CHUNK + 1));   // a list of len > CHUNK has < 2 len / CHUNK chunks
  L.total = L.entries + psb_align(8 * e_max);
  return L;
}

template <int VPL>
static void psb_launch_sums(const float *feat, const int32_t *nbr, const float *rt, const float *depth, const float *grad_corr,
                            const uint32_t *off, const int2 *entries, const uint32_t *n_work, const int2 *work,
                            float *grad_feat, int N, int K, int H, int W, int C, int D, float scale, hipStream_t st) {
  const int64_t rows = (int64_t)N * H * W;
  hipLaunchKernelGGL(psb_final_kernel<VPL>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, feat, nbr, rt, depth,
                     grad_corr, off, entries, grad_feat, N, K, H, W, C, D, scale);
  hipLaunchKernelGGL(psb_long_kernel<VPL>, dim3(1024), dim3(256), 0, st, feat, off, entries, n_work, work, grad_feat, C, scale);
}

}  // namespace sgc

using namespace sgc;

extern "C" int64_t sgc_plane_sweep_corr_backward_workspace_bytes(int N, int K, int H, int W, int D) {
  if (N <= 0 || K <= 0 || H <= 0 || W <= 0 || D <= 0) return 0;
  return psb_layout(N, K, H, W, D).total;
}

extern "C" int sgc_plane_sweep_corr_backward(const float *feat, const int32_t *nbr, const float *rt, const float *depth,
                                             const float *grad_corr, float *grad_feat, void *workspace,
                                             int64_t workspace_bytes, int N, int K, int H, int W, int C, int D,
                                             sgc_stream_t stream) {
  if (!feat || !nbr || !rt || !depth || !grad_corr || !grad_feat || !workspace)
    return set_error(SGC_EINVAL, "sgc_plane_sweep_corr_backward: null pointer");
  if (N <= 0 || K <= 0 || H <= 0 || W <= 0 || C <= 0 || D <= 0)
    return set_error(SGC_EINVAL, "sgc_plane_sweep_corr_backward: bad size");
  if (D > PSB_MAXD) return set_error(SGC_EUNSUP, "sgc_plane_sweep_corr_backward: at most %d depth planes", PSB_MAXD);
  if (C > 256) return set_error(SGC_EUNSUP, "sgc_plane_sweep_corr_backward: at most 256 channels");
  const int64_t rows = (int64_t)N * H * W;
  if (rows * K * D * 4 > INT32_MAX)
    return set_error(SGC_EUNSUP, "sgc_plane_sweep_corr_backward: N*H*W*K*D*4 corner entries must fit 31 bits");
  const PsbLayout L = psb_layout(N, K, H, W, D);
  if (workspace_bytes < L.total)
    return set_error(SGC_EINVAL, "sgc_plane_sweep_corr_backward: workspace of %lld bytes, %lld needed",
                     (long long)workspace_bytes, (long long)L.total);
  char *ws = (char *)workspace;
  uint32_t *cnt = (uint32_t *)(ws + L.cnt), *off = (uint32_t *)(ws + L.off), *bsum = (uint32_t *)(ws + L.bsum);
  uint32_t *n_work = (uint32_t *)(ws + L.n_work);
  int2 *work = (int2 *)(ws + L.work), *entries = (int2 *)(ws + L.entries);
  hipStream_t st = (hipStream_t)stream;
  const int n = (int)rows, nb = (int)((rows + PSB_SCAN - 1) / PSB_SCAN);
  const int64_t walkers = rows * K;
  const dim3 walk_grid((unsigned)((walkers + 255) / 256));
  // counts and the work counter sit back to back at the front of the workspace (cnt .. n_work): one zero-fill kernel
  // (a kernel, not hipMemsetAsync: see conv3d.hip zero_fill)
  const int64_t nz = (L.n_work + 4) / 4;
  hipLaunchKernelGGL(psb_zero_kernel, dim3((unsigned)std::min<int64_t>((nz + 255) / 256, 2048)), dim3(256), 0, st, cnt, nz);
  hipLaunchKernelGGL(psb_route_kernel<false>, walk_grid, dim3(256), 0, st, nbr, rt, depth, grad_corr, cnt, off, entries, N, K,
                     H, W, D);
  hipLaunchKernelGGL(psb_scan_reduce_kernel, dim3((unsigned)nb), dim3(256), 0, st, cnt, bsum, n);
  hipLaunchKernelGGL(psb_scan_top_kernel, dim3(1), dim3(256), 0, st, bsum, off, nb, n);
  hipLaunchKernelGGL(psb_scan_apply_kernel, dim3((unsigned)nb), dim3(256), 0, st, cnt, bsum, off, n_work, work, n);
  hipLaunchKernelGGL(psb_route_kernel<true>, walk_grid, dim3(256), 0, st, nbr, rt, depth, grad_corr, cnt, off, entries, N, K,
                     H, W, D);
  const float scale = (1.0f / sqrtf((float)C)) / (float)K;
  switch ((C + 63) / 64) {
    case 1: psb_launch_sums<1>(feat, nbr, rt, depth, grad_corr, off, entries, n_work, work, grad_feat, N, K, H, W, C, D, scale, st); break;
    case 2: psb_launch_sums<2>(feat, nbr, rt, depth, grad_corr, off, entries, n_work, work, grad_feat, N, K, H, W, C, D, scale, st); break;
    case 3: psb_launch_sums<3>(feat, nbr, rt, depth, grad_corr, off, entries, n_work, work, grad_feat, N, K, H, W, C, D, scale, st); break;
    default: psb_launch_sums<4>(feat, nbr, rt, depth, grad_corr, off, entries, n_work, work, grad_feat, N, K, H, W, C, D, scale, st); break;
  }
  return check_launch("plane_sweep_corr_backward");
}
