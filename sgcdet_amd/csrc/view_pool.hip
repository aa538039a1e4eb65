// Inter-view aggregation for gfx950.
//
// The reference scatters per-camera results into dense slots [N,1,Nq,C] (262 MB at
// config 2), projects K/V for every slot including the invisible ones and masks them
// with -inf (TU/deformable_cross_attention.py:815-833).  Here the visible (camera, query)
// pairs stay a compact list; `slot[n,q]` (pair index or -1) is the only dense object.
#include "common.hpp"
#include "tuning.hpp"

#include <type_traits>

namespace sgc {

// g_tune_pq_depth (key view_depth): pair rows in flight per lane in view_attend_pq_kernel (1 | 2 | 4 | 8) and in the
// group kernels of view_mean / view_attend (>= 4: four, else one) -- A/B; results identical

// The prefetch ring: PD rows in flight per lane (round 5: with one row ahead these kernels were chains of ~30 dependent loads per
// voxel and ran at a third of the HBM rate, although the projected-query kernel issues ~170 instructions per pair).  r[k] holds row
// j0 + k of the n rows of a sequence and is refilled with the row PD later as soon as it has been handed to `use`.  `next(j)` issues
// the load of row j and is called for j = 0, 1, ... n - 1 in that order, `use(j, row)` likewise: same order as a plain loop, same sums.
template <int PD, typename Row, typename Next, typename Use>
__device__ __forceinline__ void prefetch_ring(int n, Next &&next, Use &&use) {
  Row r[PD];
#pragma unroll
  for (int k = 0; k < PD; ++k) r[k] = k < n ? next(k) : Row{};
  for (int j0 = 0; j0 < n; j0 += PD) {
#pragma unroll
    for (int k = 0; k < PD; ++k) {
      const int j = j0 + k;
      if (j >= n) break;
      const Row v = r[k];
      if (j + PD < n) r[k] = next(j + PD);
      use(j, v);
    }
  }
}

// The visible-camera walk of a GROUP: the LG in {32, 64} lanes of a voxel inside one wave (lane gl of the group).  Round 3: the group
// reads the voxel's slot column 32 / 64 cameras at a time with ONE load per lane, and walks only the visible cameras (ballot +
// shuffle) through the ring -- instead of one dependent slot load per camera (28 of config 2's 40 cameras do not see a voxel)
// followed by a dependent row load.  `load(p)` issues the load of pair row p, `use(row)` consumes it: the cameras that see voxel q
// in ascending order, as the per-camera loops below take them.  Every lane of the wave must call this (shuffles).
template <int LG, int PD, typename Row, typename Load, typename Use>
__device__ __forceinline__ void walk_visible(const int32_t *__restrict__ slot, int N, int Nq, int q, int gl, Load &&load, Use &&use) {
  const int gbase = (threadIdx.x & 63) & ~(LG - 1);
  for (int nb = 0; nb < N; nb += LG) {
    const int pl = nb + gl < N ? slot[(int64_t)(nb + gl) * Nq + q] : -1;
    unsigned long long m = __ballot(pl >= 0);
    if (LG == 32) m = (m >> gbase) & 0xffffffffull;
    if (!m) continue;
    prefetch_ring<PD, Row>(
        __popcll(m),
        [&](int) {                                     // the next set bit of m: the pair index sits in that lane's pl
          const int pn = __shfl(pl, gbase + __builtin_ctzll(m));
          m &= m - 1;
          return load(pn);
        },
        [&](int, const Row &row) { use(row); });
  }
}

// One step of the online softmax over views: score d enters the running maximum mx and the running sum; the caller rescales
// what it has accumulated by corr and adds e times the new row.  exp(-inf) = 0 on the first visible view.
struct SoftmaxStep {
  float corr, e;
};
__device__ __forceinline__ SoftmaxStep online_softmax_step(float d, float &mx, float &sum) {
  const float nm = fmaxf(mx, d);
  const float corr = expf(mx - nm);
  const float e = expf(d - nm);
  sum = sum * corr + e;
  mx = nm;
  return {corr, e};
}

// mean over the cameras that see voxel valid_index[i]; LG = C/4 lanes per voxel (float4 rows) on walk_visible.  Same cameras in
// the same order, same sums as view_mean_kernel: bit-identical.
template <int LG, int PD = 4>
__global__ __launch_bounds__(256) void view_mean_group_kernel(const float *__restrict__ feat, const int32_t *__restrict__ slot,
                                                              const int32_t *__restrict__ valid_index, float *__restrict__ mean,
                                                              int N, int Nq, int n_valid, const int32_t *__restrict__ n_dev) {
  if (n_dev) n_valid = min(n_valid, *n_dev);
  constexpr int C = LG * 4;
  const int gl = threadIdx.x & (LG - 1);
  const int64_t total = (int64_t)n_valid * LG, span = ((total + 63) / 64) * 64;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < span; idx += (int64_t)gridDim.x * blockDim.x) {
    const bool live = idx < total;
    const int i = (int)((live ? idx : total - 1) / LG);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    int cnt = 0;
    walk_visible<LG, PD, float4>(
        slot, N, Nq, valid_index[i], gl, [&](int p) { return reinterpret_cast<const float4 *>(feat + (int64_t)p * C)[gl]; },
        [&](const float4 &v) {
          acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
          ++cnt;
        });
    if (live) {
      const float fc = (float)cnt;
      reinterpret_cast<float4 *>(mean + (int64_t)i * C)[gl] = make_float4(acc.x / fc, acc.y / fc, acc.z / fc, acc.w / fc);
    }
  }
}

// The per-camera loop: one lane per T (float4 when C % 4 == 0 and the rows are 16-byte aligned, else float) of a voxel's row.
template <typename T>
__global__ __launch_bounds__(256) void view_mean_kernel(const float *__restrict__ feat,
                                                        const int32_t *__restrict__ slot,
                                                        const int32_t *__restrict__ valid_index,
                                                        float *__restrict__ mean, int N, int Nq, int C, int n_valid,
                                                        const int32_t *__restrict__ n_dev) {
  if (n_dev) n_valid = min(n_valid, *n_dev);     // row count produced on the device (no host read-back)
  const int CT = C / (int)(sizeof(T) / sizeof(float));
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < (int64_t)n_valid * CT;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int i = (int)(idx / CT), c = (int)(idx - (int64_t)i * CT);
    const int q = valid_index[i];
    T acc{};
    int cnt = 0;
    for (int n = 0; n < N; ++n) {
      const int p = slot[(int64_t)n * Nq + q];
      if (p < 0) continue;
      acc += reinterpret_cast<const T *>(feat + (int64_t)p * C)[c];
      ++cnt;
    }
    reinterpret_cast<T *>(mean + (int64_t)i * C)[c] = acc / (float)cnt;     // per component
  }
}

// Group form of view_attend_kernel<4> for heads * G in {32, 64} lanes per voxel (C = 128 / 256 with 8 heads) on walk_visible: the
// next cameras' k | v rows are requested before the current one enters the online softmax.  Same cameras, same order, same
// arithmetic as the generic kernel below: bit-identical.
struct KvRow {
  float4 k, v;
};

template <int LG, int PD = 4>
__global__ __launch_bounds__(256) void view_attend_group_kernel(const float *__restrict__ q, const float *__restrict__ kv,
                                                                const int32_t *__restrict__ slot,
                                                                const int32_t *__restrict__ valid_index, float *__restrict__ ctx,
                                                                int N, int Nq, int heads, int n_valid, float scale,
                                                                const int32_t *__restrict__ n_dev) {
  if (n_dev) n_valid = min(n_valid, *n_dev);
  if (n_valid <= 0) return;
  constexpr int C = LG * 4;
  const int G = LG / heads;                          // lanes per head
  const int gl = threadIdx.x & (LG - 1);
  const int c0 = gl * 4;                             // == h * hd + g * 4 of the generic kernel
  const int64_t total = (int64_t)n_valid * LG, span = ((total + 63) / 64) * 64;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < span; idx += (int64_t)gridDim.x * blockDim.x) {
    const bool live = idx < total;
    const int i = (int)((live ? idx : total - 1) / LG);
    const float4 q4 = *reinterpret_cast<const float4 *>(q + (int64_t)i * C + c0);
    const float qv[4] = {q4.x * scale, q4.y * scale, q4.z * scale, q4.w * scale};
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    float mx = -INFINITY, sum = 0.f;
    walk_visible<LG, PD, KvRow>(
        slot, N, Nq, valid_index[i], gl,
        [&](int p) {
          const float *kp = kv + (int64_t)p * 2 * C + c0;
          return KvRow{*reinterpret_cast<const float4 *>(kp), *reinterpret_cast<const float4 *>(kp + C)};
        },
        [&](const KvRow &r) {
          const float kx[4] = {r.k.x, r.k.y, r.k.z, r.k.w}, vx[4] = {r.v.x, r.v.y, r.v.z, r.v.w};
          float d = 0.f;
#pragma unroll
          for (int v = 0; v < 4; ++v) d += qv[v] * kx[v];
          for (int o = 1; o < G; o <<= 1) d += __shfl_xor(d, o);
          const SoftmaxStep s = online_softmax_step(d, mx, sum);
          // view_attend_kernel<4>'s `acc * corr + e * v`, with the fma spelled out: hipcc is free to contract either product into
          // it, there it rounds e * v on its own, and inside this lambda it picked the other one (test_view_attend_forms_are_bit_identical)
#pragma unroll
          for (int v = 0; v < 4; ++v) acc[v] = __builtin_fmaf(acc[v], s.corr, s.e * vx[v]);
        });
    if (live) *reinterpret_cast<float4 *>(ctx + (int64_t)i * C + c0) = make_float4(acc[0] / sum, acc[1] / sum, acc[2] / sum, acc[3] / sum);
  }
}

// ---------------------------------------------------------------------------------------------
// Projected-query form of the same attention (round 5).  nn.MultiheadAttention over the views (query length 1,
// TU/deformable_cross_attention.py:826-833) in-projects K and V for EVERY visible (camera, voxel) pair: a [pairs, C] x
// [C, 2C] GEMM whose result (2 KB per pair at C = 256) is written, read back once by the softmax, and thrown away --
// at 100 views 2.1 M pairs per scene, the largest Linear of the path.  Both projections commute with the softmax:
//   score(n, h) = (scale q_h) . (W_k,h x_n + b_k,h) = (scale W_k,h^T q_h) . x_n + const(h)        (the constant
//                 is the same for every camera n and drops out of the softmax over n),
//   ctx_h       = sum_n a(n, h) (W_v,h x_n + b_v,h) = W_v,h (sum_n a(n, h) x_n) + b_v,h          (sum_n a = 1),
// so the per-pair work is the raw pair feature x_n against a PROJECTED QUERY qp_h = scale W_k,h^T q_h (C floats per voxel
// and head, one [n_valid, C] x [C, heads C] GEMM on the voxels), and V is applied once per voxel to the attention-weighted
// feature s_h = sum_n a(n, h) x_n ([n_valid, heads C] x block-diagonal [heads C, C]).  Same function of the inputs as
// sgc_view_attend on the in-projected tensors; sums are associated differently (~1e-6 relative).
//
// One group of LG = C / 4 lanes per voxel (one wave at C = 256, half a wave at C = 128), 8 heads.  Per visible camera
// the lane holds 4 channels of x_n and the same 4 channels of the 8 projected queries: 8 partial dot products, reduced
// over the group with a packed butterfly (the first three exchange steps halve the number of values a lane carries:
// 4 + 2 + 1 shuffles, then one value over the remaining lane bits), scores parked in LDS.  An exact two-pass softmax
// (max, expf, sum, true division -- torch's softmax) over the voxel's cameras, then a second walk over the same pair
// rows (L2 hits) accumulates the 8 weighted features.  Both walks run the ring over the voxel's pair list in LDS.
// No atomics, fixed order: the same bits every run.
// ---------------------------------------------------------------------------------------------
constexpr int kPqHeads = 8, kPqMaxViews = 128;

template <int LG, int PD = 4>
__global__ __launch_bounds__(256) void view_attend_pq_kernel(const float *__restrict__ qp, const float *__restrict__ x,
                                                             const int32_t *__restrict__ slot,
                                                             const int32_t *__restrict__ valid_index, float *__restrict__ s,
                                                             int N, int Nq, int n_valid, const int32_t *__restrict__ n_dev) {
  if (n_dev) n_valid = min(n_valid, *n_dev);
  if (n_valid <= 0) return;
  constexpr int C = LG * 4, H = kPqHeads, GPW = 64 / LG, GPB = 4 * GPW;      // groups per wave / per block
  __shared__ __attribute__((aligned(16))) float sc[GPB][kPqMaxViews][H];     // scores, then softmax weights: [camera][head]
  __shared__ int plist[GPB][kPqMaxViews];                                     // pair index of the voxel's j-th visible camera
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, gl = lane & (LG - 1), gbase = lane & ~(LG - 1);
  const int grp = wid * GPW + (lane / LG);
  float (*my_sc)[H] = sc[grp];
  int *my_pl = plist[grp];
  const bool b0 = gl & 1, b1 = gl & 2, b2 = gl & 4;
  const int hm = (b0 ? 4 : 0) + (b1 ? 2 : 0) + (b2 ? 1 : 0);                 // the head whose sum this lane holds after the butterfly
  const int64_t ngroups = n_valid, gstride = (int64_t)gridDim.x * GPB;
  // every lane of a wave runs the same number of iterations (shuffles need the whole wave): dead groups redo the last voxel
  const int64_t first = (int64_t)blockIdx.x * GPB + grp;
  const int64_t iters = (ngroups - (int64_t)blockIdx.x * GPB - wid * GPW + gstride - 1) / gstride;     // of this wave's first group
  const auto pair_row = [&](int j) { return *reinterpret_cast<const float4 *>(x + (int64_t)my_pl[j] * C + gl * 4); };
  int64_t i_raw = first;
  for (int64_t it = 0; it < iters; ++it, i_raw += gstride) {
    const bool live = i_raw < ngroups;
    const int i = (int)(live ? i_raw : ngroups - 1);
    const int vq = valid_index[i];
    // ---- the voxel's visible cameras, ascending camera index ----
    int cnt = 0;
    for (int nb = 0; nb < N; nb += LG) {
      const int pl = nb + gl < N ? slot[(int64_t)(nb + gl) * Nq + vq] : -1;
      unsigned long long m = __ballot(pl >= 0);
      if (LG == 32) m = (m >> gbase) & 0xffffffffull;
      if (pl >= 0) my_pl[cnt + __popcll(m & ((1ull << gl) - 1ull))] = pl;
      cnt += __popcll(m);
    }
    float4 q[H];
#pragma unroll
    for (int h = 0; h < H; ++h) q[h] = *reinterpret_cast<const float4 *>(qp + ((int64_t)i * H + h) * C + gl * 4);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // one wave: its LDS operations complete in order
    __builtin_amdgcn_wave_barrier();
    // ---- pass 1: scores ----
    prefetch_ring<PD, float4>(cnt, pair_row, [&](int j, const float4 &xv) {
      float v[H];
#pragma unroll
      for (int h = 0; h < H; ++h) v[h] = ((q[h].x * xv.x + q[h].y * xv.y) + q[h].z * xv.z) + q[h].w * xv.w;
      float t[4], u[2];
#pragma unroll
      for (int k = 0; k < 4; ++k) t[k] = (b0 ? v[4 + k] : v[k]) + __shfl_xor(b0 ? v[k] : v[4 + k], 1);
#pragma unroll
      for (int k = 0; k < 2; ++k) u[k] = (b1 ? t[2 + k] : t[k]) + __shfl_xor(b1 ? t[k] : t[2 + k], 2);
      float d = (b2 ? u[1] : u[0]) + __shfl_xor(b2 ? u[0] : u[1], 4);
#pragma unroll
      for (int o = 8; o < LG; o <<= 1) d += __shfl_xor(d, o);
      if (gl < 8) my_sc[j][hm] = d;
    });
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    // ---- softmax over the cameras, per head: lane = (head gl & 7, cameras (gl >> 3) + k LG / 8) ----
    {
      const int h = gl & 7, j0 = gl >> 3;
      constexpr int JS = LG / 8;
      float mx = -INFINITY;
      for (int j = j0; j < cnt; j += JS) mx = fmaxf(mx, my_sc[j][h]);
#pragma unroll
      for (int o = 8; o < LG; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
      float sum = 0.f;
      for (int j = j0; j < cnt; j += JS) {
        const float e = expf(my_sc[j][h] - mx);
        my_sc[j][h] = e;
        sum += e;
      }
#pragma unroll
      for (int o = 8; o < LG; o <<= 1) sum += __shfl_xor(sum, o);
      for (int j = j0; j < cnt; j += JS) my_sc[j][h] = my_sc[j][h] / sum;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    // ---- pass 2: the 8 attention-weighted features ----
    float4 acc[H];
#pragma unroll
    for (int h = 0; h < H; ++h) acc[h] = make_float4(0.f, 0.f, 0.f, 0.f);
    prefetch_ring<PD, float4>(cnt, pair_row, [&](int j, const float4 &xv) {
      const float4 a0 = *reinterpret_cast<const float4 *>(&my_sc[j][0]), a1 = *reinterpret_cast<const float4 *>(&my_sc[j][4]);
      const float a[H] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
      for (int h = 0; h < H; ++h) {
        acc[h].x += a[h] * xv.x; acc[h].y += a[h] * xv.y; acc[h].z += a[h] * xv.z; acc[h].w += a[h] * xv.w;
      }
    });
    if (live) {
#pragma unroll
      for (int h = 0; h < H; ++h) *reinterpret_cast<float4 *>(s + ((int64_t)i * H + h) * C + gl * 4) = acc[h];
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // the next voxel overwrites this group's LDS
    __builtin_amdgcn_wave_barrier();
  }
}

// Softmax over views for query length 1 (nn.MultiheadAttention, :829-833): one group of
// G = head_dim/VEC lanes per (voxel, head); the dot product is reduced over the group with
// wave shuffles, the softmax over views runs online (running max / sum) in registers.
template <int VEC>
__global__ __launch_bounds__(256) void view_attend_kernel(const float *__restrict__ q,
                                                          const float *__restrict__ kv,
                                                          const int32_t *__restrict__ slot,
                                                          const int32_t *__restrict__ valid_index,
                                                          float *__restrict__ ctx, int N, int Nq, int C,
                                                          int heads, int n_valid, int G, float scale,
                                                          const int32_t *__restrict__ n_dev) {
  if (n_dev) n_valid = min(n_valid, *n_dev);
  if (n_valid <= 0) return;
  const int hd = C / heads;
  const int64_t total = (int64_t)n_valid * heads * G;
  const int64_t span = (((int64_t)total + 63) / 64) * 64;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < span;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const bool live = idx < total;
    const int64_t id = live ? idx : total - 1;
    const int g = (int)(id % G);
    const int h = (int)((id / G) % heads);
    const int i = (int)(id / ((int64_t)G * heads));
    const int vq = valid_index[i];
    const int c0 = h * hd + g * VEC;
    float qv[VEC], acc[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      qv[v] = q[(int64_t)i * C + c0 + v] * scale;  // torch: q_scaled = q * sqrt(1/head_dim)
      acc[v] = 0.f;
    }
    float mx = -INFINITY, sum = 0.f;
    for (int n = 0; n < N; ++n) {
      const int p = slot[(int64_t)n * Nq + vq];
      if (p < 0) continue;  // uniform over the G lanes of a group
      const float *kp = kv + (int64_t)p * 2 * C + c0;
      float kx[VEC], vx[VEC];
      if (VEC == 4) {
        const float4 k4 = *reinterpret_cast<const float4 *>(kp);
        const float4 v4 = *reinterpret_cast<const float4 *>(kp + C);
        kx[0] = k4.x; kx[1 % VEC] = k4.y; kx[2 % VEC] = k4.z; kx[3 % VEC] = k4.w;
        vx[0] = v4.x; vx[1 % VEC] = v4.y; vx[2 % VEC] = v4.z; vx[3 % VEC] = v4.w;
      } else {
        kx[0] = kp[0]; vx[0] = kp[C];
      }
      float d = 0.f;
#pragma unroll
      for (int v = 0; v < VEC; ++v) d += qv[v] * kx[v];
      for (int o = 1; o < G; o <<= 1) d += __shfl_xor(d, o);
      const SoftmaxStep s = online_softmax_step(d, mx, sum);
#pragma unroll
      for (int v = 0; v < VEC; ++v) acc[v] = acc[v] * s.corr + s.e * vx[v];
    }
    if (live) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) ctx[(int64_t)i * C + c0 + v] = acc[v] / sum;
    }
  }
}

// Backward of view_attend_kernel (training over the pair list: no dense [N, L, C] slots, no full-size K/V projections --
// the reference back-propagates through nn.MultiheadAttention on the padded slots, TU/deformable_cross_attention.py:829-833).
// Same lane grouping as the forward: G lanes per (voxel, head).  With a_n the softmax weights, ctx = sum_n a_n v_n:
//   S = <d_ctx, ctx>;  da_n = <d_ctx, v_n>;  ds_n = a_n (da_n - S);
//   d_q = scale * sum_n ds_n k_n;  d_k_n = ds_n * scale * q;  d_v_n = a_n * d_ctx.
// Every pair belongs to exactly one voxel, so grad_kv rows are written once, without atomics.
template <int VEC>
__global__ __launch_bounds__(256) void view_attend_backward_kernel(const float *__restrict__ q, const float *__restrict__ kv,
                                                                   const int32_t *__restrict__ slot,
                                                                   const int32_t *__restrict__ valid_index,
                                                                   const float *__restrict__ ctx, const float *__restrict__ gctx,
                                                                   float *__restrict__ gq, float *__restrict__ gkv, int N, int Nq,
                                                                   int C, int heads, int n_valid, int G, float scale) {
  const int hd = C / heads;
  const int64_t total = (int64_t)n_valid * heads * G;
  const int64_t span = (((int64_t)total + 63) / 64) * 64;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < span; idx += (int64_t)gridDim.x * blockDim.x) {
    const bool live = idx < total;
    const int64_t id = live ? idx : total - 1;
    const int g = (int)(id % G);
    const int h = (int)((id / G) % heads);
    const int i = (int)(id / ((int64_t)G * heads));
    const int vq = valid_index[i];
    const int c0 = h * hd + g * VEC;
    float qv[VEC], dc[VEC], dq[VEC];
    float S = 0.f;
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      qv[v] = q[(int64_t)i * C + c0 + v] * scale;
      dc[v] = gctx[(int64_t)i * C + c0 + v];
      S += dc[v] * ctx[(int64_t)i * C + c0 + v];
      dq[v] = 0.f;
    }
    for (int o = 1; o < G; o <<= 1) S += __shfl_xor(S, o);
    float mx = -INFINITY, sum = 0.f;
    for (int n = 0; n < N; ++n) {                      // pass 1: the softmax normalisation (as the forward computes it)
      const int p = slot[(int64_t)n * Nq + vq];
      if (p < 0) continue;
      const float *kp = kv + (int64_t)p * 2 * C + c0;
      float d = 0.f;
#pragma unroll
      for (int v = 0; v < VEC; ++v) d += qv[v] * kp[v];
      for (int o = 1; o < G; o <<= 1) d += __shfl_xor(d, o);
      online_softmax_step(d, mx, sum);
    }
    for (int n = 0; n < N; ++n) {                      // pass 2: gradients
      const int p = slot[(int64_t)n * Nq + vq];
      if (p < 0) continue;
      const float *kp = kv + (int64_t)p * 2 * C + c0;
      float kx[VEC], vx[VEC];
#pragma unroll
      for (int v = 0; v < VEC; ++v) { kx[v] = kp[v]; vx[v] = kp[C + v]; }
      float d = 0.f, da = 0.f;
#pragma unroll
      for (int v = 0; v < VEC; ++v) { d += qv[v] * kx[v]; da += dc[v] * vx[v]; }
      for (int o = 1; o < G; o <<= 1) { d += __shfl_xor(d, o); da += __shfl_xor(da, o); }
      const float a = expf(d - mx) / sum;
      const float ds = a * (da - S);
      if (live) {
        float *gp = gkv + (int64_t)p * 2 * C + c0;
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          dq[v] += ds * kx[v];
          gp[v] = ds * qv[v];
          gp[C + v] = a * dc[v];
        }
      }
    }
    if (live) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) gq[(int64_t)i * C + c0 + v] = dq[v] * scale;
    }
  }
}

}  // namespace sgc

using namespace sgc;

// The <LG, PD> form of a kernel template: LG = `lanes` per voxel (64 | 32), PD = the first of the descending list PDS that the
// view_depth knob reaches, else the last of the list.  f(lg, pd) gets both as std::integral_constant.
template <int PD, int... REST, typename F>
static void for_depth(int knob, F &&f) {
  if constexpr (sizeof...(REST) == 0) f(std::integral_constant<int, PD>{});
  else if (knob >= PD) f(std::integral_constant<int, PD>{});
  else for_depth<REST...>(knob, f);
}
template <int... PDS, typename F>
static void for_form(int lanes, F &&f) {
  if (lanes == 64) for_depth<PDS...>(g_tune_pq_depth, [&](auto pd) { f(std::integral_constant<int, 64>{}, pd); });
  else for_depth<PDS...>(g_tune_pq_depth, [&](auto pd) { f(std::integral_constant<int, 32>{}, pd); });
}

// lanes per (voxel, head) of view_attend and its backward: head_dim / 4 (float4 accesses, where `vec4_ok`) when that is a power of
// two <= 64, else one lane per channel; G == 0: head_dim not supported
struct HeadLanes {
  int vec, G;
};
static HeadLanes head_lanes(int hd, bool vec4_ok) {
  int vec = 4, G = hd / 4;
  if (hd % 4 || (G & (G - 1)) || G > 64 || !vec4_ok) { vec = 1; G = hd; }
  if ((G & (G - 1)) || G > 64) G = 0;
  return {vec, G};
}

extern "C" int sgc_view_attend_pq_supported(int N, int C, int heads) {
  return heads == sgc::kPqHeads && (C == 128 || C == 256) && N > 0 && N <= sgc::kPqMaxViews ? 1 : 0;
}

extern "C" int sgc_view_mean(const float *feat, const int32_t *slot, const int32_t *valid_index,
                             float *mean, int N, int Nq, int C, const int32_t *n_valid_dev_or_null, int n_valid,
                             sgc_stream_t stream) {
  const int32_t *n_dev = n_valid_dev_or_null;
  if (!feat || !slot || !valid_index || !mean) return set_error(SGC_EINVAL, "sgc_view_mean: null pointer");
  if (n_valid <= 0) return SGC_OK;
  const bool al16 = !((uintptr_t)feat & 15) && !((uintptr_t)mean & 15);
  if ((C == 256 || C == 128) && al16 && g_tune_view_group)     // rows in flight per lane: 4 (default) | 1 (the round-3 form, A/B)
    for_form<4, 1>(C / 4, [&](auto lg, auto pd) {
      hipLaunchKernelGGL((view_mean_group_kernel<lg(), pd()>), dim3(grid_for((int64_t)n_valid * lg(), 256)), dim3(256), 0,
                         (hipStream_t)stream, feat, slot, valid_index, mean, N, Nq, n_valid, n_dev);
    });
  else if (C % 4 == 0 && al16)
    hipLaunchKernelGGL(view_mean_kernel<float4>, dim3(grid_for((int64_t)n_valid * (C / 4), 256)), dim3(256), 0,
                       (hipStream_t)stream, feat, slot, valid_index, mean, N, Nq, C, n_valid, n_dev);
  else
    hipLaunchKernelGGL(view_mean_kernel<float>, dim3(grid_for((int64_t)n_valid * C, 256)), dim3(256), 0,
                       (hipStream_t)stream, feat, slot, valid_index, mean, N, Nq, C, n_valid, n_dev);
  return check_launch("view_mean_kernel");
}

extern "C" int sgc_view_attend(const float *q, const float *kv, const int32_t *slot,
                               const int32_t *valid_index, float *ctx,
                               int N, int Nq, int C, int heads, const int32_t *n_valid_dev_or_null, int n_valid,
                               sgc_stream_t stream) {
  const int32_t *n_dev = n_valid_dev_or_null;
  if (!q || !kv || !slot || !valid_index || !ctx) return set_error(SGC_EINVAL, "sgc_view_attend: null pointer");
  if (heads <= 0 || C % heads) return set_error(SGC_EINVAL, "sgc_view_attend: C %% heads != 0");
  if (n_valid <= 0) return SGC_OK;
  const int hd = C / heads;
  const float scale = sqrtf(1.0f / (float)hd);
  const HeadLanes hl = head_lanes(hd, !(((uintptr_t)q | (uintptr_t)kv) & 15));
  const int vec = hl.vec, G = hl.G;
  if (!G) return set_error(SGC_EUNSUP, "sgc_view_attend: head_dim %d not supported", hd);
  const dim3 grid(grid_for((int64_t)n_valid * heads * G, 256));
  if (vec == 4 && (heads * G == 64 || heads * G == 32) && g_tune_view_group)
    for_form<4, 1>(heads * G, [&](auto lg, auto pd) {
      hipLaunchKernelGGL((view_attend_group_kernel<lg(), pd()>), grid, dim3(256), 0, (hipStream_t)stream, q, kv, slot, valid_index,
                         ctx, N, Nq, heads, n_valid, scale, n_dev);
    });
  else if (vec == 4)
    hipLaunchKernelGGL(view_attend_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, q, kv,
                       slot, valid_index, ctx, N, Nq, C, heads, n_valid, G, scale, n_dev);
  else
    hipLaunchKernelGGL(view_attend_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, q, kv,
                       slot, valid_index, ctx, N, Nq, C, heads, n_valid, G, scale, n_dev);
  return check_launch("view_attend_kernel");
}

extern "C" int sgc_view_attend_pq(const float *qp, const float *x, const int32_t *slot, const int32_t *valid_index, float *s,
                                  int N, int Nq, int C, int heads, const int32_t *n_valid_dev_or_null, int n_valid,
                                  sgc_stream_t stream) {
  if (!qp || !x || !slot || !valid_index || !s) return set_error(SGC_EINVAL, "sgc_view_attend_pq: null pointer");
  if (!sgc_view_attend_pq_supported(N, C, heads))
    return set_error(SGC_EUNSUP, "sgc_view_attend_pq: needs heads == %d, C in {128, 256}, N <= %d (got heads %d, C %d, N %d)",
                     kPqHeads, kPqMaxViews, heads, C, N);
  if (((uintptr_t)qp | (uintptr_t)x | (uintptr_t)s) & 15) return set_error(SGC_EINVAL, "sgc_view_attend_pq: pointers must be 16-byte aligned");
  if (n_valid <= 0) return SGC_OK;
  const int gpb = C == 256 ? 4 : 8;                                    // voxel groups per block
  const dim3 grid((unsigned)std::min<int64_t>(((int64_t)n_valid + gpb - 1) / gpb, 256 * 16));
  for_form<8, 4, 2, 1>(C / 4, [&](auto lg, auto pd) {
    hipLaunchKernelGGL((view_attend_pq_kernel<lg(), pd()>), grid, dim3(256), 0, (hipStream_t)stream, qp, x, slot, valid_index, s, N,
                       Nq, n_valid, n_valid_dev_or_null);
  });
  return check_launch("view_attend_pq_kernel");
}

extern "C" int sgc_view_attend_backward(const float *q, const float *kv, const int32_t *slot, const int32_t *valid_index,
                                        const float *ctx, const float *grad_ctx, float *grad_q, float *grad_kv,
                                        int N, int Nq, int C, int heads, int n_valid, sgc_stream_t stream) {
  if (!q || !kv || !slot || !valid_index || !ctx || !grad_ctx || !grad_q || !grad_kv)
    return set_error(SGC_EINVAL, "sgc_view_attend_backward: null pointer");
  if (heads <= 0 || C % heads) return set_error(SGC_EINVAL, "sgc_view_attend_backward: C %% heads != 0");
  if (n_valid <= 0) return SGC_OK;
  const int hd = C / heads;
  const float scale = sqrtf(1.0f / (float)hd);
  const HeadLanes hl = head_lanes(hd, true);           // the kernel reads scalars: no alignment condition
  const int vec = hl.vec, G = hl.G;
  if (!G) return set_error(SGC_EUNSUP, "sgc_view_attend_backward: head_dim %d not supported", hd);
  const dim3 grid(grid_for((int64_t)n_valid * heads * G, 256));
  if (vec == 4)
    hipLaunchKernelGGL(view_attend_backward_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, q, kv, slot,
                       valid_index, ctx, grad_ctx, grad_q, grad_kv, N, Nq, C, heads, n_valid, G, scale);
  else
    hipLaunchKernelGGL(view_attend_backward_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, q, kv, slot,
                       valid_index, ctx, grad_ctx, grad_q, grad_kv, N, Nq, C, heads, n_valid, G, scale);
  return check_launch("view_attend_backward_kernel");
}
