// Sample geometry of the deformable gather (DFA3D) and of the plane sweep: the ONE definition (three kernels keep a written-out
// copy and say so: phase 1 of dfa3d_fwd_tile_kernel, dfa3d_bwd_kernel, dfa3d_bwd_tile_kernel -- a fix here is a fix there too).
// DFA3D semantics: ms_depth_score_sample_cuda_kernel.cuh:24-148 and wms_deform_attn_cuda_kernel.cuh:24-80,286-294 of
// the reference.  Corners are in the GATHER order (h0,w0) (h0,w1) (h1,w0) (h1,w1) everywhere in this library; the
// reference's own order (h0,w0) (h0,w1) (h1,w1) (h1,w0) exists at its interfaces only (ref_order).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sgc {

typedef float float2_u __attribute__((ext_vector_type(2), aligned(4)));  // 4-byte aligned pair load
typedef float float4_u __attribute__((ext_vector_type(4), aligned(8)));

constexpr int kOutside = (int)0x80000000;
__device__ __forceinline__ int off_index(int off) { return off & 0x7fffffff; }

// Sample coordinate `loc * size - 0.5` with the REFERENCE's two roundings: `loc_h * spatial_h` is a float product
// (int promoted to float) and `- 0.5` a double subtraction rounded back to float on assignment
// (ms_depth_score_sample_cuda_kernel.cuh:133-135, wms_deform_attn_cuda_kernel.cuh:286-287) -- nvcc cannot contract
// that into an fma, so neither may hipcc: floor() of the result picks the pixel, a one-rounding fma flips it for
// ~1 sample in 1e7.  (float product exact in double, one rounding of the exact difference == float subtraction.)
__device__ __forceinline__ float sample_coord(float loc, float size) {
#pragma clang fp contract(off)
  const float prod = loc * size;
  return prod - 0.5f;
}

// One axis of a sample: t_im = loc * T - 0.5, the open gate -1 < t_im < T, floor, fraction, integer index.
// (int) of a huge float is undefined: the float is clamped first (the gate already holds the decision, taken on the
// floats), so i0 is in [-2, T] for every input, non-finite ones included.
struct Axis { float frac; int i0; bool in; };
__device__ __forceinline__ Axis sample_axis(float loc, float T) {
  const float t = sample_coord(loc, T), f = floorf(t);
  // bitwise & on purpose: with && the compiler may evaluate the later comparison under an exec mask (an s_and_saveexec / s_or
  // pair per chain); both operands are cheap and side-effect free.  Flags that are already VALUES (in2, in3, ok[k] below)
  // combine with &&: nothing is left to short-circuit, and & on stored bools went through 0 / 1 integers in vector registers
  // (v_and_b32 5 -> 25, v_cmp_eq 1 -> 13 in the wave kernel).
  return {t - f, (int)__builtin_amdgcn_fmed3f(f, -2.f, T), (bool)((t > -1.f) & (t < T))};
}

// Bilinear weights of the four corners and their derivatives by h and w (signs as wms_deform_attn_cuda_kernel.cuh:116-150).
struct Bilinear { float w[4], dh[4], dw[4]; };
__device__ __forceinline__ Bilinear bilinear(float lh, float lw) {
  const float hh = 1.f - lh, hw = 1.f - lw;
  return {{hh * hw, hh * lw, lh * hw, lh * lw}, {-hw, -lw, hw, lw}, {-hh, hh, -lh, lh}};
}

// Gather order <-> reference order: corners [2] and [3] trade places (its own inverse), for an index and for four values.
__device__ __forceinline__ int ref_corner(int k) { return k < 2 ? k : 5 - k; }
__device__ __forceinline__ float4 ref_order(float4 v) {
  const float a[4] = {v.x, v.y, v.z, v.w};
  return make_float4(a[ref_corner(0)], a[ref_corner(1)], a[ref_corner(2)], a[ref_corner(3)]);
}

// The four corners (h0 | h0 + 1, w0 | w0 + 1) of a 2-D sample.  `ok` is the in-map test alone, for a sample that passed
// its gate (h0 in [-1, H - 1] then, so one comparison per row and column decides); AND it with the gate.
struct Corners {
  int px[4];          // pixel index h * W + w: the corner's pixel where ok holds
  int cpx[4];         // the same from rows / columns clamped into the map: valid to read even where ok is false
  bool okh[2], ok[4];
};
__device__ __forceinline__ Corners sample_corners(int h0, int w0, int H, int W) {
  Corners c;
  c.okh[0] = h0 >= 0; c.okh[1] = h0 + 1 <= H - 1;
  const bool okw[2] = {w0 >= 0, w0 + 1 <= W - 1};
  const int ch[2] = {min(max(h0, 0), H - 1), min(max(h0 + 1, 0), H - 1)};
  const int cw[2] = {min(max(w0, 0), W - 1), min(max(w0 + 1, 0), W - 1)};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    c.ok[k] = c.okh[k >> 1] && okw[k & 1];
    c.px[k] = (h0 + (k >> 1)) * W + w0 + (k & 1);
    c.cpx[k] = ch[k >> 1] * W + cw[k & 1];
  }
  return c;
}

// The two depth taps d0, d0 + 1 of a corner, read as ONE pair at `base` (D >= 2): every depth load touches 64 different
// cache lines per wave instruction, so the instruction count is what the L1/TA path pays for.  The load itself stays with
// the caller (a global float2, a float4 of the pair-interleaved map); select() turns the loaded pair (a, b) =
// (dist[base], dist[base + 1]) into (tap d0, tap d0 + 1), 0 outside [0, D - 1].
struct DepthTaps {
  int base;           // min(max(d0, 0), D - 2)
  bool lo;            // d0 == base: false only at the two depth borders
  bool d0ok, d1ok;
  __device__ __forceinline__ void select(float a, float b, float &va, float &vb) const {
    va = d0ok ? (lo ? a : b) : 0.f;
    vb = d1ok ? (lo ? b : a) : 0.f;
  }
};
__device__ __forceinline__ DepthTaps depth_taps(int d0, int D) {
  const int base = min(max(d0, 0), D - 2);
  return {base, d0 == base, d0 >= 0, d0 + 1 <= D - 1};
}

// One trilinear sample, reduced to what the gather needs: 4 corner weights (bilinear * depth score * attention weight)
// and 4 pixel indices.
struct Sample {
  float w[4];
  int off[4];   // pixel index inside the level (h*W + w); corners outside the map (or of a gated-off sample) carry the sign
                // bit (kOutside) on top of a CLAMPED in-range index, so consumers can load unconditionally (no exec-mask
                // branch per load) and zero the value with a select
  float sg[4];  // depth scores
  float lh, lw, ld;   // pieces the backward needs
  int h0, w0, d0;
  bool in2, in3;
};

// 2-D part of a sample (gate, fractions, corner offsets), then the depth axis
__device__ __forceinline__ Corners sample_2d(Sample &sm, int H, int W, float x, float y) {
  const Axis ah = sample_axis(y, (float)H), aw = sample_axis(x, (float)W);
  sm.in2 = ah.in && aw.in;
  sm.lh = ah.frac; sm.lw = aw.frac; sm.h0 = ah.i0; sm.w0 = aw.i0;
  const Corners c = sample_corners(sm.h0, sm.w0, H, W);
#pragma unroll
  for (int k = 0; k < 4; ++k) sm.off[k] = (sm.in2 && c.ok[k]) ? c.px[k] : (c.cpx[k] | kOutside);
  return c;
}
__device__ __forceinline__ Corners sample_3d(Sample &sm, int H, int W, int D, float x, float y, float z) {
  const Corners c = sample_2d(sm, H, W, x, y);
  const Axis ad = sample_axis(z, (float)D);
  sm.in3 = sm.in2 && ad.in;
  sm.ld = ad.frac; sm.d0 = ad.i0;
  return c;
}
// common tail: scores of the corners (0 where the corner or the sample is gated off) -> weights
__device__ __forceinline__ void sample_weights(Sample &sm, const float (&sc)[4], float aw) {
  const Bilinear b = bilinear(sm.lh, sm.lw);
#pragma unroll
  for (int k = 0; k < 4; ++k) { sm.sg[k] = sc[k]; sm.w[k] = sm.in2 ? b.w[k] * sc[k] * aw : 0.f; }
}

__device__ __forceinline__ void make_sample(Sample &sm, const float *__restrict__ dist_px0, int64_t pix_stride, int H, int W,
                                            int D, float x, float y, float z, float aw) {
  const Corners c = sample_3d(sm, H, W, D, x, y, z);
  const DepthTaps t = depth_taps(sm.d0, D);
  const float hd = 1.f - sm.ld;
  float sc[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float v = 0.f;
    if (sm.in3 && c.ok[k]) {
      float va, vb;
      const float *p = dist_px0 + (int64_t)c.px[k] * pix_stride;
      if (D >= 2) {
        const float2_u pr = *reinterpret_cast<const float2_u *>(p + t.base);
        t.select(pr.x, pr.y, va, vb);
      } else {
        va = t.d0ok ? p[sm.d0] : 0.f; vb = t.d1ok ? p[sm.d0 + 1] : 0.f;
      }
      v = va * hd + vb * sm.ld;
    }
    sc[k] = v;
  }
  sample_weights(sm, sc, aw);
}

// Same sample from the PAIR-INTERLEAVED depth map dp[h][wq][d][2] (wq = w + 1 in [0, W]):
//   dp[h][wq][d] = (dist[h][wq-1][d] or 0, dist[h][wq][d] or 0)
// so the (w0, w1) x (d0, d1) taps of one image row are 16 contiguous bytes: 2 loads per sample
// instead of 4 (each depth load of a wave touches 64 different cache lines).  D >= 2 only (the pair at
// `base`): sgc_pairs_deform_gather ignores the pair map at D = 1.
__device__ __forceinline__ void make_sample_dp(Sample &sm, const float *__restrict__ dp_cam, int H, int W, int D,
                                               float x, float y, float z, float aw) {
  const Corners c = sample_3d(sm, H, W, D, x, y, z);
  const float hd = 1.f - sm.ld;
  float sc[4] = {0.f, 0.f, 0.f, 0.f};
  if (sm.in3) {
    const DepthTaps t = depth_taps(sm.d0, D);
    const int wq = sm.w0 + 1;                    // in [0, W] whenever in2 holds
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
      if (!c.okh[rr]) continue;
      const float4_u q = *reinterpret_cast<const float4_u *>(dp_cam + (((int64_t)(sm.h0 + rr) * (W + 1) + wq) * D + t.base) * 2);
      // q = (w0@base, w1@base, w0@base+1, w1@base+1)
      float a0, a1, b0, b1;
      t.select(q.x, q.z, a0, a1); t.select(q.y, q.w, b0, b1);
      sc[rr * 2] = a0 * hd + a1 * sm.ld;
      sc[rr * 2 + 1] = b0 * hd + b1 * sm.ld;
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (!c.ok[k]) sc[k] = 0.f;
  sample_weights(sm, sc, aw);
}

// LEFT OUT of the definition above: make_sample as it stood before this header (unclamped conversions, in range wherever the
// gates let an index be used; reduced to off, sg, lh / lw / ld, d0, in2 / in3), for dfa3d_bwd_kernel and
// dfa3d_bwd_tile_kernel.  Both sit at a register step, and built from the helpers -- the same operations -- the second measured
// 1.0 % slower and the scalar form of the first 0.1 % (profiles/r12_sample_geometry.md).  `taps` (optional, 8 floats): the two
// depth taps (d0, d0 + 1; 0 where gated off) of every corner.
__device__ __forceinline__ void make_sample_unclamped(Sample &sm, const float *__restrict__ dist_px0, int64_t pix_stride, int H,
                                                      int W, int D, float x, float y, float z, float *taps = nullptr) {
  const float h_im = sample_coord(y, (float)H), w_im = sample_coord(x, (float)W), d_im = sample_coord(z, (float)D);
  sm.in2 = h_im > -1.f && w_im > -1.f && h_im < (float)H && w_im < (float)W;
  sm.in3 = sm.in2 && d_im > -1.f && d_im < (float)D;
  const float hf = floorf(h_im), wf = floorf(w_im), df = floorf(d_im);
  const int h0 = (int)hf, w0 = (int)wf, d0 = (int)df;
  const int h1 = h0 + 1, w1 = w0 + 1, d1 = d0 + 1;
  sm.lh = h_im - hf; sm.lw = w_im - wf; sm.ld = d_im - df; sm.d0 = d0;
  const float hd = 1.f - sm.ld;
  const bool okh0 = h0 >= 0, okh1 = h1 <= H - 1, okw0 = w0 >= 0, okw1 = w1 <= W - 1;
  const bool ok[4] = {okh0 && okw0, okh0 && okw1, okh1 && okw0, okh1 && okw1};
  const int px[4] = {h0 * W + w0, h0 * W + w1, h1 * W + w0, h1 * W + w1};
  const int ch0 = min(max(h0, 0), H - 1), ch1 = min(max(h1, 0), H - 1), cw0 = min(max(w0, 0), W - 1), cw1 = min(max(w1, 0), W - 1);
  const int cpx[4] = {ch0 * W + cw0, ch0 * W + cw1, ch1 * W + cw0, ch1 * W + cw1};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    sm.off[k] = (sm.in2 && ok[k]) ? px[k] : (cpx[k] | kOutside);
    float v = 0.f;
    if (sm.in3 && ok[k]) {
      const float *p = dist_px0 + (int64_t)px[k] * pix_stride;
      float va, vb;
      if (D >= 2) {
        const int base = d0 < 0 ? 0 : (d0 > D - 2 ? D - 2 : d0);
        const float2_u pr = *reinterpret_cast<const float2_u *>(p + base);
        va = d0 < 0 ? 0.f : (d0 == base ? pr.x : pr.y);
        vb = d1 > D - 1 ? 0.f : (d0 == base ? pr.y : pr.x);
      } else {
        va = d0 >= 0 ? p[d0] : 0.f;
        vb = d1 <= D - 1 ? p[d1] : 0.f;
      }
      v = va * hd + vb * sm.ld;
      if (taps) { taps[2 * k] = va; taps[2 * k + 1] = vb; }
    } else if (taps) {
      taps[2 * k] = 0.f; taps[2 * k + 1] = 0.f;
    }
    sm.sg[k] = v;
  }
}

// Plane sweep (plane_sweep.hip, plane_sweep_bwd.hip): the warped position of a pixel on one depth plane and its four bilinear
// corners, with the arithmetic of the reference's homo_warping + F.grid_sample (depth_est_fusion.py:87-126).  Not the DFA3D axis:
// the formula differs.  The position decides which pixels are read, so the reference's op order is kept (no contraction).
struct PlaneSweepCorners {
  int idx[4];       // pixel index in the neighbour view (clamped: valid to read even where ok is false)
  float w[4];       // nw, ne, sw, se; 0 where ok is false
  bool ok[4];       // corner on the image (false for every corner of a non-finite / off-image position)
};
__device__ __forceinline__ PlaneSweepCorners plane_sweep_corners(float rx, float ry, float rz, const float *m, float dep, int H,
                                                                 int W) {
#pragma clang fp contract(off)
  const float half_w = (float)(W - 1) / 2.0f, half_h = (float)(H - 1) / 2.0f;
  const float px = rx * dep + m[3], py = ry * dep + m[7], pz = rz * dep + m[11];   // * depth + trans
  const float u = px / pz, v_ = py / pz;
  const float gx = u / half_w - 1.0f, gy = v_ / half_h - 1.0f;          // the reference's normalisation
  const float ix = ((gx + 1.0f) * (float)W - 1.0f) / 2.0f;              // grid_sample, align_corners = False
  const float iy = ((gy + 1.0f) * (float)H - 1.0f) / 2.0f;
  const bool in = ix > -1.0f && iy > -1.0f && ix < (float)W && iy < (float)H;   // false for NaN / inf too
  const float x0f = in ? floorf(ix) : 0.f, y0f = in ? floorf(iy) : 0.f;
  const int x0 = (int)x0f, y0 = (int)y0f, x1 = x0 + 1, y1 = y0 + 1;
  const float lx = ix - x0f, ly = iy - y0f, hx = 1.0f - lx, hy = 1.0f - ly;
  const bool okx0 = in && x0 >= 0, okx1 = in && x1 <= W - 1, oky0 = in && y0 >= 0, oky1 = in && y1 <= H - 1;
  const int cx0 = max(x0, 0), cx1 = min(x1, W - 1), cy0 = max(y0, 0), cy1 = min(y1, H - 1);
  PlaneSweepCorners r;
  r.idx[0] = cy0 * W + cx0; r.ok[0] = oky0 && okx0; r.w[0] = r.ok[0] ? hx * hy : 0.f;
  r.idx[1] = cy0 * W + cx1; r.ok[1] = oky0 && okx1; r.w[1] = r.ok[1] ? lx * hy : 0.f;
  r.idx[2] = cy1 * W + cx0; r.ok[2] = oky1 && okx0; r.w[2] = r.ok[2] ? hx * ly : 0.f;
  r.idx[3] = cy1 * W + cx1; r.ok[3] = oky1 && okx1; r.w[3] = r.ok[3] ? lx * ly : 0.f;
  return r;
}

}  // namespace sgc
