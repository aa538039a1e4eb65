// The loss of the detection head: ImVoxelHeadV2._loss_single (plugin/bbox_head.py over plugin/losses.py; reference
// imvoxel_head_v2.py:147-235) for one image -- sigmoid focal loss, BCE-with-logits on the centerness, IoU loss of the decoded boxes --
// with the gradients of the head tensors made in the same pass.  A loss is a leaf: its inputs' gradients do not need the upstream
// gradient until the very end, where it is one factor per loss.
//
//   head_loss_main_kernel<ROT>   one lane per point, adjacent lanes adjacent points; reads the head tensors where they are (any channel /
//                                point stride, no permuted or concatenated copy), writes the UNNORMALISED gradient of every element
//                                (zeros included: no memset, no atomics) into the packed gradient buffer and one partial of
//                                (sum focal, sum bce, sum w (1 - IoU), count(pos), sum w) per workgroup.
//   head_loss_riou_kernel        rotated head only: the positives' rotated IoU and its gradient.  The clip of the predicted rectangle
//                                against the four edges of the target runs on a dual number carrying the 5 BEV tangents, so the same code
//                                yields value and gradient; the 8-slot polygon of duals lives in scratch (see DESIGN.md for the resource
//                                report), which is why it is a kernel of its own: the common path keeps its occupancy.
//   head_loss_final_kernel       one workgroup adds the partials in a fixed order, applies max(., 1), n_pos_override and the empty-case
//                                rules on the device, writes the three losses, the local n_pos and the three scale factors.
//   head_loss_scale_kernel       gradient = unnormalised gradient * factor_k * grad_output_k, run by the autograd backward.
//
// Arithmetic: fp32 in, fp32 out, fp64 in registers.  The data is 3 MB and the chip's fp64 vector rate is not the limit of anything
// here; in return every loss and gradient is the correctly rounded value of the formula up to the last conversion, which is what a
// comparison of a SCALAR against torch's own fp32-vs-fp64 rounding needs (two equally noisy fp32 scalars miss a 4 x bound one time
// in six).  The focal loss keeps log(max(p, FLT_MIN)) with its zero gradient where the clamp is active, as losses.sigmoid_focal_loss
// and mmcv's operator have it: beyond |logit| = 87.3 the clamp acts exactly as in fp32.  Between 16.6 and 87.3, where fp32's 1 - p
// has already rounded to 0 and the fp32 formula reports log(FLT_MIN), this kernel follows the float64 evaluation of the same formula.
// No float atomics and a fixed summation order: bitwise reproducible run to run.
#include "common.hpp"
#include "../../include/sgcdet_amd_train.h"

namespace sgc {

constexpr int kHlThreads = 256;
constexpr int kHlSums = 5;             // focal, bce, w (1 - IoU), count(pos), w
constexpr int kHlHeader = 4;           // doubles in front of the partials: the three scale factors (+ 1 pad)
constexpr double kFltMin = 1.1754943508222875e-38;

struct HeadLevels {                    // by value: a kernel argument
  sgc_head_loss_level lv[SGC_HEAD_LOSS_MAX_SCALES];
  int point_start[SGC_HEAD_LOSS_MAX_SCALES + 1];      // first point of level l in the flattened point list
  int block_start[SGC_HEAD_LOSS_MAX_SCALES + 1];      // first workgroup of level l
  int n_scales;
};
static_assert(sizeof(sgc_head_loss_level) == 64, "sgc_head_loss_level is 64 bytes");

// workgroup -> level (wave-uniform: scalar loads from the argument block)
__device__ __forceinline__ int level_of_block(const HeadLevels &L, int b) {
  int l = 0;
  for (int k = 1; k < SGC_HEAD_LOSS_MAX_SCALES; ++k)
    if (k < L.n_scales && b >= L.block_start[k]) l = k;
  return l;
}

// sum over the workgroup, every addition in a fixed order; valid in thread 0
template <int N>
__device__ __forceinline__ void block_sum(double (&s)[N], double (*red)[N]) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < N; ++k)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s[k] += __shfl_xor(s[k], o);
  if ((tid & 63) == 0)
#pragma unroll
    for (int k = 0; k < N; ++k) red[tid >> 6][k] = s[k];
  __syncthreads();
  if (tid == 0)
#pragma unroll
    for (int k = 0; k < N; ++k) s[k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
}

// torch.maximum / torch.minimum hand an exact tie half of the gradient each
__device__ __forceinline__ double take_max(double mine, double other) { return mine > other ? 1.0 : (mine == other ? 0.5 : 0.0); }
__device__ __forceinline__ double take_min(double mine, double other) { return mine < other ? 1.0 : (mine == other ? 0.5 : 0.0); }

// ---------------------------------------------------------------------------------------------------------------------------
// main pass
// ---------------------------------------------------------------------------------------------------------------------------
template <bool ROT>
__global__ __launch_bounds__(kHlThreads) void head_loss_main_kernel(const HeadLevels L, const float *__restrict__ points,
                                                                    const float *__restrict__ ctr_t, const float *__restrict__ box_t,
                                                                    const int64_t *__restrict__ labels, int n_reg, int n_classes,
                                                                    double gamma, double alpha, float *__restrict__ grads,
                                                                    double *__restrict__ partials) {
  __shared__ double red[kHlThreads / kWave][kHlSums];
  const int b = blockIdx.x;
  const int l = level_of_block(L, b);
  const sgc_head_loss_level lv = L.lv[l];
  const int n_l = (int)lv.n_points;
  const int j = (b - L.block_start[l]) * kHlThreads + threadIdx.x;
  const int ch = 1 + n_reg + n_classes;
  double s[kHlSums] = {0.0, 0.0, 0.0, 0.0, 0.0};
  if (j < n_l) {
    const int i = L.point_start[l] + j;
    float *g_ctr = grads + (int64_t)ch * L.point_start[l] + j;     // [ch, n_l] planes of this level
    float *g_reg = g_ctr + n_l;
    float *g_cls = g_reg + (int64_t)n_reg * n_l;
    const bool valid = lv.valid[j] != 0;
    const int64_t lab = labels[i];
    const bool pos = valid && lab >= 0;

    // ---- classification: sigmoid focal loss over every class of a valid point ----
    const float *cls = lv.cls_score + (int64_t)j * lv.cls_point_stride;
    const bool square = gamma == 2.0;
    double focal = 0.0;
    for (int c = 0; c < n_classes; ++c) {
      double g = 0.0;
      if (valid) {
        const double x = (double)cls[(int64_t)c * lv.cls_channel_stride];
        const double p = 1.0 / (1.0 + exp(-x)), q = 1.0 - p;
        double val, dp;                                               // loss and d loss / d p
        if (lab == (int64_t)c) {
          const double pc = p > kFltMin ? p : kFltMin, lg = log(pc);
          const double qg = square ? q * q : pow(q, gamma), qg1 = square ? q : pow(q, gamma - 1.0);
          val = -alpha * qg * lg;
          dp = -alpha * (-gamma * qg1 * lg + (p >= kFltMin ? qg / pc : 0.0));
        } else {
          const double qc = q > kFltMin ? q : kFltMin, lg = log(qc);
          const double pg = square ? p * p : pow(p, gamma), pg1 = square ? p : pow(p, gamma - 1.0);
          val = -(1.0 - alpha) * pg * lg;
          dp = -(1.0 - alpha) * (gamma * pg1 * lg - (q >= kFltMin ? pg / qc : 0.0));
        }
        focal += val;
        g = dp * p * q;
      }
      g_cls[(int64_t)c * n_l] = (float)g;
    }
    s[0] = focal;

    // ---- centerness: BCE with logits against the soft target, positives only ----
    double gc = 0.0, w = 0.0;
    if (pos) {
      const double t = (double)ctr_t[i];
      if (t >= 0.0) {                                                 // mmdet's ignore mask (centerness targets are >= 0)
        const double x = (double)lv.centerness[(int64_t)j * lv.centerness_point_stride];
        const double ax = fabs(x);
        s[1] = (1.0 - t) * x + (x < 0.0 ? -x : 0.0) + log1p(exp(-ax));
        gc = 1.0 / (1.0 + exp(-x)) - t;
      }
      w = t;
      s[3] = 1.0;
      s[4] = w;
    }
    *g_ctr = (float)gc;

    // ---- boxes ----
    if (ROT) {
      if (!pos)                                                       // the positives' rows are head_loss_riou_kernel's
        for (int k = 0; k < n_reg; ++k) g_reg[(int64_t)k * n_l] = 0.f;
    } else {
      double g[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      if (pos) {
        // _bbox_pred_to_bbox (ScanNet head): point -/+ distances; axis_aligned_iou with its eps
        const float *reg = lv.bbox_pred + (int64_t)j * lv.bbox_point_stride;
        double lo[3], hi[3], tlo[3], thi[3], e[3], r[3], wh[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          const double pt = (double)points[(int64_t)i * 3 + a];
          lo[a] = pt - (double)reg[(int64_t)(2 * a) * lv.bbox_channel_stride];
          hi[a] = pt + (double)reg[(int64_t)(2 * a + 1) * lv.bbox_channel_stride];
          tlo[a] = (double)box_t[(int64_t)i * 6 + a];
          thi[a] = (double)box_t[(int64_t)i * 6 + 3 + a];
          e[a] = hi[a] - lo[a];
          r[a] = (hi[a] < thi[a] ? hi[a] : thi[a]) - (lo[a] > tlo[a] ? lo[a] : tlo[a]);
          wh[a] = r[a] > 0.0 ? r[a] : 0.0;
        }
        const double area1 = e[0] * e[1] * e[2];
        const double area2 = (thi[0] - tlo[0]) * (thi[1] - tlo[1]) * (thi[2] - tlo[2]);
        const double ov = wh[0] * wh[1] * wh[2];
        const double u0 = area1 + area2 - ov, eps = 1e-6;
        const double un = u0 > eps ? u0 : eps, um = take_max(u0, eps);
        const double iou = ov / un;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          const int a1 = (a + 1) % 3, a2 = (a + 2) % 3;
          const double dov = r[a] >= 0.0 ? wh[a1] * wh[a2] : 0.0;     // d overlap / d (rb - lt) of this axis (clamp passes 0)
          const double dov_lo = -dov * take_max(lo[a], tlo[a]), dov_hi = dov * take_min(hi[a], thi[a]);
          const double da = e[a1] * e[a2];                            // d area1 / d hi = -d area1 / d lo
          const double dun_lo = um * (-da - dov_lo), dun_hi = um * (da - dov_hi);
          const double diou_lo = (dov_lo * un - ov * dun_lo) / (un * un);
          const double diou_hi = (dov_hi * un - ov * dun_hi) / (un * un);
          g[2 * a] = w * diou_lo;                                     // lo = point - d: d (1 - iou) / d d = + d iou / d lo
          g[2 * a + 1] = -w * diou_hi;
        }
        s[2] = w * (1.0 - iou);
      }
#pragma unroll
      for (int k = 0; k < 6; ++k) g_reg[(int64_t)k * n_l] = (float)g[k];
    }
  }
  block_sum(s, red);
  if (threadIdx.x == 0) {
    double *out = partials + (int64_t)b * kHlSums;
    out[0] = s[0]; out[1] = s[1]; out[3] = s[3]; out[4] = s[4];
    if (!ROT) out[2] = s[2];                                          // the rotated head's comes from head_loss_riou_kernel
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// rotated IoU of the positives (losses.rotated_iou_3d: rectangle clipped against the four edges of the target on a fixed 8-slot
// polygon, shoelace area, z overlap, inter / (vol - inter)), value and gradient from one evaluation on dual numbers
// ---------------------------------------------------------------------------------------------------------------------------
struct Dual {                          // value + tangents with respect to the prediction's BEV (x, y, w, l, angle)
  double v, d[5];
};
__device__ __forceinline__ Dual operator+(const Dual &a, const Dual &b) {
  Dual r; r.v = a.v + b.v;
#pragma unroll
  for (int k = 0; k < 5; ++k) r.d[k] = a.d[k] + b.d[k];
  return r;
}
__device__ __forceinline__ Dual operator-(const Dual &a, const Dual &b) {
  Dual r; r.v = a.v - b.v;
#pragma unroll
  for (int k = 0; k < 5; ++k) r.d[k] = a.d[k] - b.d[k];
  return r;
}
__device__ __forceinline__ Dual operator*(const Dual &a, const Dual &b) {
  Dual r; r.v = a.v * b.v;
#pragma unroll
  for (int k = 0; k < 5; ++k) r.d[k] = a.d[k] * b.v + a.v * b.d[k];
  return r;
}
__device__ __forceinline__ Dual operator/(const Dual &a, const Dual &b) {
  Dual r; r.v = a.v / b.v;
  const double inv = 1.0 / b.v;
#pragma unroll
  for (int k = 0; k < 5; ++k) r.d[k] = (a.d[k] - r.v * b.d[k]) * inv;
  return r;
}
// e.x * (p.y - a.y) - e.y * (p.x - a.x): side of p relative to the edge a -> a + e (constants) -- positive on the left
__device__ __forceinline__ Dual edge_side(const Dual &px, const Dual &py, double ax, double ay, double ex, double ey) {
  Dual r; r.v = ex * (py.v - ay) - ey * (px.v - ax);
#pragma unroll
  for (int k = 0; k < 5; ++k) r.d[k] = ex * py.d[k] - ey * px.d[k];
  return r;
}

__global__ __launch_bounds__(kHlThreads) void head_loss_riou_kernel(const HeadLevels L, const float *__restrict__ points,
                                                                    const float *__restrict__ ctr_t, const float *__restrict__ box_t,
                                                                    const int64_t *__restrict__ labels, int n_classes,
                                                                    float *__restrict__ grads, double *__restrict__ partials) {
  __shared__ double red[kHlThreads / kWave][1];
  const int b = blockIdx.x;
  const int l = level_of_block(L, b);
  const sgc_head_loss_level lv = L.lv[l];
  const int n_l = (int)lv.n_points;
  const int j = (b - L.block_start[l]) * kHlThreads + threadIdx.x;
  double s[1] = {0.0};
  if (j < n_l) {
    const int i = L.point_start[l] + j;
    if (lv.valid[j] != 0 && labels[i] >= 0) {
      const double w = (double)ctr_t[i];
      const float *reg = lv.bbox_pred + (int64_t)j * lv.bbox_point_stride;
      double d[7], t[7];
#pragma unroll
      for (int k = 0; k < 7; ++k) {
        d[k] = (double)reg[(int64_t)k * lv.bbox_channel_stride];
        t[k] = (double)box_t[(int64_t)i * 7 + k];
      }
      // _bbox_pred_to_bbox (SunRgbd head): the centre shift rotated by the predicted angle
      const double ca = cos(d[6]), sa = sin(d[6]);
      const double sx = (d[1] - d[0]) * 0.5, sy = (d[3] - d[2]) * 0.5;
      const double cx = (double)points[(int64_t)i * 3] + (sx * ca - sy * sa);
      const double cy = (double)points[(int64_t)i * 3 + 1] + (sx * sa + sy * ca);
      const double cz = (double)points[(int64_t)i * 3 + 2] + (d[5] - d[4]) * 0.5;
      const double bw = d[0] + d[1], bl = d[2] + d[3], bh = d[4] + d[5];

      // _rect_corners: counter-clockwise corners of both rectangles
      const double sgx[4] = {-1.0, 1.0, 1.0, -1.0}, sgy[4] = {-1.0, -1.0, 1.0, 1.0};
      Dual px[8], py[8], qx[8], qy[8];
      double tx[4], ty[4];
      const double ct = cos(t[6]), st = sin(t[6]);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const double dx = sgx[k] * bw * 0.5, dy = sgy[k] * bl * 0.5;
        px[k].v = cx + dx * ca - dy * sa;
        px[k].d[0] = 1.0; px[k].d[1] = 0.0; px[k].d[2] = 0.5 * sgx[k] * ca; px[k].d[3] = -0.5 * sgy[k] * sa;
        px[k].d[4] = -dx * sa - dy * ca;
        py[k].v = cy + dx * sa + dy * ca;
        py[k].d[0] = 0.0; py[k].d[1] = 1.0; py[k].d[2] = 0.5 * sgx[k] * sa; py[k].d[3] = 0.5 * sgy[k] * ca;
        py[k].d[4] = dx * ca - dy * sa;
        const double ux = sgx[k] * t[3] * 0.5, uy = sgy[k] * t[4] * 0.5;
        tx[k] = t[0] + ux * ct - uy * st;
        ty[k] = t[1] + ux * st + uy * ct;
      }
      int cnt = 4;
      for (int k = 0; k < 4; ++k) {                                   // _clip_convex against the edge tx/ty[k] -> [k + 1]
        const double ax = tx[k], ay = ty[k], ex = tx[(k + 1) & 3] - ax, ey = ty[(k + 1) & 3] - ay;
        int m = 0;
        for (int v = 0; v < cnt; ++v) {
          const int nx = v + 1 < cnt ? v + 1 : 0;
          const Dual sp = edge_side(px[v], py[v], ax, ay, ex, ey), sq = edge_side(px[nx], py[nx], ax, ay, ex, ey);
          const bool p_in = sp.v >= 0.0, q_in = sq.v >= 0.0;
          if (p_in && m < 8) { qx[m] = px[v]; qy[m] = py[v]; ++m; }
          if (p_in != q_in && m < 8) {
            const Dual tt = sp / (sp - sq);
            qx[m] = px[v] + tt * (px[nx] - px[v]);
            qy[m] = py[v] + tt * (py[nx] - py[v]);
            ++m;
          }
        }
        for (int v = 0; v < m; ++v) { px[v] = qx[v]; py[v] = qy[v]; }
        cnt = m;
      }
      Dual sh; sh.v = 0.0;
#pragma unroll
      for (int k = 0; k < 5; ++k) sh.d[k] = 0.0;
      for (int v = 0; v < cnt; ++v) {
        const int nx = v + 1 < cnt ? v + 1 : 0;
        sh = sh + (px[v] * py[nx] - py[v] * px[nx]);
      }
      const double sgn = sh.v > 0.0 ? 0.5 : (sh.v < 0.0 ? -0.5 : 0.0);       // 0.5 * |.|
      const double area = sgn * sh.v;
      double ga[5];
#pragma unroll
      for (int k = 0; k < 5; ++k) ga[k] = sgn * sh.d[k];

      // z overlap and the IoU
      const double p_hi = cz + bh * 0.5, t_hi = t[2] + t[5] * 0.5, p_lo = cz - bh * 0.5, t_lo = t[2] - t[5] * 0.5;
      const double zr = (p_hi < t_hi ? p_hi : t_hi) - (p_lo > t_lo ? p_lo : t_lo);
      const double zo = zr > 0.0 ? zr : 0.0, zm = zr >= 0.0 ? 1.0 : 0.0;
      const double w_hi = take_min(p_hi, t_hi), w_lo = take_max(p_lo, t_lo);
      const double dzo_cz = zm * (w_hi - w_lo), dzo_h = zm * 0.5 * (w_hi + w_lo);
      const double inter = area * zo;
      const double vol = bw * bl * bh + t[3] * t[4] * t[5];
      const double den = vol - inter, iou = inter / den;
      // d iou / d (cx, cy, cz, w, l, h, angle) = (d inter * vol - inter * d vol) / den^2
      const double inv2 = 1.0 / (den * den);
      const double G_cx = zo * ga[0] * vol * inv2, G_cy = zo * ga[1] * vol * inv2, G_cz = area * dzo_cz * vol * inv2;
      const double G_w = (zo * ga[2] * vol - inter * bl * bh) * inv2, G_l = (zo * ga[3] * vol - inter * bw * bh) * inv2;
      const double G_h = (area * dzo_h * vol - inter * bw * bl) * inv2, G_a = zo * ga[4] * vol * inv2;
      double g[7];
      g[0] = -0.5 * ca * G_cx - 0.5 * sa * G_cy + G_w;
      g[1] = 0.5 * ca * G_cx + 0.5 * sa * G_cy + G_w;
      g[2] = 0.5 * sa * G_cx - 0.5 * ca * G_cy + G_l;
      g[3] = -0.5 * sa * G_cx + 0.5 * ca * G_cy + G_l;
      g[4] = -0.5 * G_cz + G_h;
      g[5] = 0.5 * G_cz + G_h;
      g[6] = G_cx * (-sx * sa - sy * ca) + G_cy * (sx * ca - sy * sa) + G_a;
      float *g_reg = grads + (int64_t)(8 + n_classes) * L.point_start[l] + n_l + j;
#pragma unroll
      for (int k = 0; k < 7; ++k) g_reg[(int64_t)k * n_l] = (float)(-w * g[k]);
      s[0] = w * (1.0 - iou);
    }
  }
  block_sum(s, red);
  if (threadIdx.x == 0) partials[(int64_t)b * kHlSums + 2] = s[0];
}

// ---------------------------------------------------------------------------------------------------------------------------
// finalise and scale
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kHlThreads) void head_loss_final_kernel(const double *__restrict__ partials, int n_blocks,
                                                                     const float *__restrict__ n_pos_override, double lw_ctr,
                                                                     double lw_box, double lw_cls, float *__restrict__ losses,
                                                                     float *__restrict__ n_pos, double *__restrict__ factors) {
  __shared__ double red[kHlThreads / kWave][kHlSums];
  double s[kHlSums] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < n_blocks; b += kHlThreads)
#pragma unroll
    for (int k = 0; k < kHlSums; ++k) s[k] += partials[(int64_t)b * kHlSums + k];
  block_sum(s, red);
  if (threadIdx.x == 0) {
    const double count = s[3];
    double norm = n_pos_override != nullptr ? (double)n_pos_override[0] : count;
    norm = norm > 1.0 ? norm : 1.0;
    const bool has_pos = count > 0.0;
    const double f_cls = lw_cls / norm;                               // no valid point: the sum and every gradient are 0 already
    const double f_ctr = has_pos ? lw_ctr / norm : 0.0;
    const double f_box = has_pos && s[4] > 0.0 ? lw_box / s[4] : 0.0;
    losses[0] = (float)(s[1] * f_ctr);
    losses[1] = (float)(s[2] * f_box);
    losses[2] = (float)(s[0] * f_cls);
    n_pos[0] = (float)count;
    factors[0] = f_ctr; factors[1] = f_box; factors[2] = f_cls;
  }
}

struct HeadSizes {
  int point_start[SGC_HEAD_LOSS_MAX_SCALES + 1];
  int n_scales;
};

__global__ __launch_bounds__(kHlThreads) void head_loss_scale_kernel(const float *__restrict__ stash, float *__restrict__ out,
                                                                     const HeadSizes S, int n_reg, int n_classes, int64_t total,
                                                                     const double *__restrict__ factors, const float *__restrict__ go_ctr,
                                                                     const float *__restrict__ go_box, const float *__restrict__ go_cls) {
  const int64_t e = (int64_t)blockIdx.x * kHlThreads + threadIdx.x;
  if (e >= total) return;
  const int ch = 1 + n_reg + n_classes;
  int l = 0;
  for (int k = 1; k < SGC_HEAD_LOSS_MAX_SCALES; ++k)
    if (k < S.n_scales && e >= (int64_t)ch * S.point_start[k]) l = k;
  const int n_l = S.point_start[l + 1] - S.point_start[l];
  const int c = (int)((e - (int64_t)ch * S.point_start[l]) / n_l);
  const double f = c == 0 ? factors[0] * (double)go_ctr[0] : (c <= n_reg ? factors[1] * (double)go_box[0] : factors[2] * (double)go_cls[0]);
  out[e] = (float)((double)stash[e] * f);
}

static int fill_levels(const char *who, const sgc_head_loss_level *levels, int n_scales, int n_reg, int n_classes, HeadLevels &L,
                       int &n_blocks) {
  if (n_scales > SGC_HEAD_LOSS_MAX_SCALES) return set_error(SGC_EUNSUP, "%s: %d scales (at most %d)", who, n_scales, SGC_HEAD_LOSS_MAX_SCALES);
  if (n_scales <= 0 || n_classes <= 0) return set_error(SGC_EINVAL, "%s: bad size", who);
  if (n_reg != 6 && n_reg != 7) return set_error(SGC_EUNSUP, "%s: n_reg = %d (6 or 7)", who, n_reg);
  int64_t pts = 0, blocks = 0;
  L = HeadLevels{};
  L.n_scales = n_scales;
  for (int l = 0; l < n_scales; ++l) {
    const sgc_head_loss_level &lv = levels[l];
    if (!lv.centerness || !lv.bbox_pred || !lv.cls_score || !lv.valid) return set_error(SGC_EINVAL, "%s: level %d: null pointer", who, l);
    if (lv.n_points <= 0) return set_error(SGC_EINVAL, "%s: level %d: n_points = %lld", who, l, (long long)lv.n_points);
    if (lv.centerness_point_stride <= 0 || lv.bbox_point_stride <= 0 || lv.cls_point_stride <= 0 || lv.bbox_channel_stride <= 0 ||
        lv.cls_channel_stride <= 0)
      return set_error(SGC_EINVAL, "%s: level %d: strides must be positive", who, l);
    L.lv[l] = lv;
    L.point_start[l] = (int)pts;
    L.block_start[l] = (int)blocks;
    pts += lv.n_points;
    blocks += (lv.n_points + kHlThreads - 1) / kHlThreads;
    if (pts * (1 + n_reg + n_classes) >= (int64_t)1 << 31) return set_error(SGC_EUNSUP, "%s: n * (1 + n_reg + n_classes) must fit 31 bits", who);
  }
  for (int l = n_scales; l <= SGC_HEAD_LOSS_MAX_SCALES; ++l) { L.point_start[l] = (int)pts; L.block_start[l] = (int)blocks; }
  n_blocks = (int)blocks;
  return SGC_OK;
}

}  // namespace sgc

using namespace sgc;

extern "C" int64_t sgc_head_loss_workspace_bytes(int n_points, int n_scales) {
  if (n_points <= 0 || n_scales <= 0) return 0;
  const int64_t blocks = ((int64_t)n_points + kHlThreads - 1) / kHlThreads + n_scales;      // every level rounds up on its own
  return (kHlHeader + blocks * kHlSums) * (int64_t)sizeof(double);
}

static int launch_final(void *workspace, int n_blocks, const float *n_pos_override, double lw_centerness, double lw_bbox, double lw_cls,
                        float *losses, float *n_pos, sgc_stream_t stream) {
  double *ws = (double *)workspace;
  hipLaunchKernelGGL(head_loss_final_kernel, dim3(1), dim3(kHlThreads), 0, (hipStream_t)stream, ws + kHlHeader, n_blocks, n_pos_override,
                     lw_centerness, lw_bbox, lw_cls, losses, n_pos, ws);
  return check_launch("head_loss_final_kernel");
}

extern "C" int sgc_head_loss_finalize(void *workspace, int64_t workspace_bytes, const int64_t *level_points, int n_scales,
                                      const float *n_pos_override, double lw_centerness, double lw_bbox, double lw_cls, float *losses,
                                      float *n_pos, sgc_stream_t stream) {
  const char *who = "sgc_head_loss_finalize";
  if (!workspace || !level_points || !losses || !n_pos) return set_error(SGC_EINVAL, "%s: null pointer", who);
  if (n_scales > SGC_HEAD_LOSS_MAX_SCALES) return set_error(SGC_EUNSUP, "%s: %d scales (at most %d)", who, n_scales, SGC_HEAD_LOSS_MAX_SCALES);
  if (n_scales <= 0) return set_error(SGC_EINVAL, "%s: bad size", who);
  int64_t pts = 0, blocks = 0;
  for (int l = 0; l < n_scales; ++l) {
    if (level_points[l] <= 0) return set_error(SGC_EINVAL, "%s: level %d: n_points = %lld", who, l, (long long)level_points[l]);
    pts += level_points[l];
    blocks += (level_points[l] + kHlThreads - 1) / kHlThreads;
  }
  if (pts >= (int64_t)1 << 31) return set_error(SGC_EUNSUP, "%s: too many points", who);
  if (workspace_bytes < sgc_head_loss_workspace_bytes((int)pts, n_scales))
    return set_error(SGC_EINVAL, "%s: workspace of %lld bytes is too small", who, (long long)workspace_bytes);
  return launch_final(workspace, (int)blocks, n_pos_override, lw_centerness, lw_bbox, lw_cls, losses, n_pos, stream);
}

extern "C" int sgc_head_loss_forward(const sgc_head_loss_level *levels, int n_scales, const float *points, const float *centerness_targets,
                                     const float *bbox_targets, const int64_t *labels, int n_points, int n_reg, int n_classes,
                                     int rotated, double gamma, double alpha, double lw_centerness, double lw_bbox, double lw_cls,
                                     const float *n_pos_override, float *losses, float *n_pos, float *grads, void *workspace,
                                     int64_t workspace_bytes, sgc_stream_t stream) {
  const char *who = "sgc_head_loss_forward";
  if (!levels || !points || !centerness_targets || !bbox_targets || !labels || !losses || !n_pos || !grads || !workspace)
    return set_error(SGC_EINVAL, "%s: null pointer", who);
  HeadLevels L;
  int n_blocks = 0;
  if (int rc = fill_levels(who, levels, n_scales, n_reg, n_classes, L, n_blocks)) return rc;
  if (L.point_start[n_scales] != n_points)
    return set_error(SGC_EUNSUP, "%s: the levels hold %d points, the point list %d", who, L.point_start[n_scales], n_points);
  if ((rotated != 0) != (n_reg == 7)) return set_error(SGC_EUNSUP, "%s: rotated = %d with n_reg = %d", who, rotated, n_reg);
  if (workspace_bytes < sgc_head_loss_workspace_bytes(n_points, n_scales))
    return set_error(SGC_EINVAL, "%s: workspace of %lld bytes, %lld needed", who, (long long)workspace_bytes,
                     (long long)sgc_head_loss_workspace_bytes(n_points, n_scales));
  hipStream_t st = (hipStream_t)stream;
  double *partials = (double *)workspace + kHlHeader;
  if (rotated) {
    hipLaunchKernelGGL(head_loss_main_kernel<true>, dim3(n_blocks), dim3(kHlThreads), 0, st, L, points, centerness_targets, bbox_targets,
                       labels, n_reg, n_classes, gamma, alpha, grads, partials);
    if (int rc = check_launch("head_loss_main_kernel<rotated>")) return rc;
    hipLaunchKernelGGL(head_loss_riou_kernel, dim3(n_blocks), dim3(kHlThreads), 0, st, L, points, centerness_targets, bbox_targets, labels,
                       n_classes, grads, partials);
    if (int rc = check_launch("head_loss_riou_kernel")) return rc;
  } else {
    hipLaunchKernelGGL(head_loss_main_kernel<false>, dim3(n_blocks), dim3(kHlThreads), 0, st, L, points, centerness_targets, bbox_targets,
                       labels, n_reg, n_classes, gamma, alpha, grads, partials);
    if (int rc = check_launch("head_loss_main_kernel")) return rc;
  }
  return launch_final(workspace, n_blocks, n_pos_override, lw_centerness, lw_bbox, lw_cls, losses, n_pos, stream);
}

extern "C" int sgc_head_loss_scale_grads(const float *grads, float *out, const int64_t *level_points, int n_scales, int n_reg, int n_classes,
                                         const void *workspace, const float *grad_centerness, const float *grad_bbox, const float *grad_cls,
                                         sgc_stream_t stream) {
  const char *who = "sgc_head_loss_scale_grads";
  if (!grads || !out || !level_points || !workspace || !grad_centerness || !grad_bbox || !grad_cls)
    return set_error(SGC_EINVAL, "%s: null pointer", who);
  if (n_scales > SGC_HEAD_LOSS_MAX_SCALES) return set_error(SGC_EUNSUP, "%s: %d scales (at most %d)", who, n_scales, SGC_HEAD_LOSS_MAX_SCALES);
  if (n_scales <= 0 || n_classes <= 0) return set_error(SGC_EINVAL, "%s: bad size", who);
  if (n_reg != 6 && n_reg != 7) return set_error(SGC_EUNSUP, "%s: n_reg = %d (6 or 7)", who, n_reg);
  HeadSizes S = {};
  S.n_scales = n_scales;
  int64_t pts = 0;
  for (int l = 0; l < n_scales; ++l) {
    if (level_points[l] <= 0) return set_error(SGC_EINVAL, "%s: level %d: n_points = %lld", who, l, (long long)level_points[l]);
    S.point_start[l] = (int)pts;
    pts += level_points[l];
    if (pts * (1 + n_reg + n_classes) >= (int64_t)1 << 31) return set_error(SGC_EUNSUP, "%s: n * (1 + n_reg + n_classes) must fit 31 bits", who);
  }
  for (int l = n_scales; l <= SGC_HEAD_LOSS_MAX_SCALES; ++l) S.point_start[l] = (int)pts;
  const int64_t total = pts * (1 + n_reg + n_classes);
  hipLaunchKernelGGL(head_loss_scale_kernel, dim3((unsigned)((total + kHlThreads - 1) / kHlThreads)), dim3(kHlThreads), 0, (hipStream_t)stream,
                     grads, out, S, n_reg, n_classes, total, (const double *)workspace, grad_centerness, grad_bbox, grad_cls);
  return check_launch("head_loss_scale_kernel");
}
