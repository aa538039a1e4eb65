// 2-D convolutions of the image-side CNNs (DepthNet_Fusion) over channels-last rows, include/sgcdet_amd_image.h.
//
// Reference layers: depth_utils/extractor_matching.py:7-89 (ResNetFPN: 7x7 stride-2 stem, BasicBlocks with stride-2 3x3 and 1x1
// projection shortcuts), depth_utils/depth_est_fusion.py:129-163 (ConvBnReLU2D, SimpleUnet2D: stride-2 3x3 down, ConvTranspose2d
// 3x3 stride 2 up with additive skips), :241-250 (concatenation, depth_reg, softmax).  sgc_conv2d_nhwc_bf16x3 covers the stride-1
// layers; this file adds what it does not:
//
//   conv2d_ex_kernel   the implicit-GEMM tile kernel for images, on the tile core it shares with conv3d_igemm_bf16x3_kernel
//                      (igemm_tile.hpp: LDS plan, staging deal, loads / split / stores of a K step, the MFMA loop, the C scatter and
//                      the float4 epilogue arithmetic).  This file supplies the two policies: ADDRESSING -- GEMM row -> (image, h, w),
//                      per tap the input pixel of every A chunk (a pixel outside the image is an out-of-range offset: zeros) and the
//                      weight slab -- and the STORE -- row pitch, column offset, output parity, softmax.
//                      Geometry: k in {1, 3}, stride in {1, 2}, padding k/2; or the transposed 3x3 stride-2 form (padding 1,
//                      output_padding 1) by OUTPUT PARITY CLASS: output (2h + ph, 2w + pw) sums the taps whose parity matches --
//                      1, 2, 2 and 4 of the 9 -- so no MFMA multiplies an inserted zero.  blockIdx.z is the class.
//                      Epilogue: v = acc * scale + shift; relu; + residual (own row pitch); relu; store at row pitch ldy, column
//                      offset col0 (two producers fill one concatenated buffer); optional softmax over the first columns.
//                      Two entries launch it: sgc_conv2d_nhwc_ex_bf16x3 (stride 2 on even sizes only) and
//                      sgc_conv2d_nhwc_strided_bf16x3 (stride 2 on any size: the ResNet stages on odd maps).
//   conv2d_stem7_kernel  7x7 stride-2 padding-3 convolution of fp32 NCHW images with 3 channels to 64 channels, folded BatchNorm +
//                      ReLU, channels-last rows out.  K = 3 * 49 = 147 padded to 160; the image patch of a tile of 8 x 32 output
//                      pixels and the whole weight matrix sit in LDS, the A fragments are gathered from the patch.
//   nchw_pad_rows_kernel  [N, C, H, W] -> rows [N*H*W, Cp] with zero tail columns (the 12-channel cost volume enters the 32-wide rows).
#include "common.hpp"
#include "igemm_tile.hpp"
#include "../../include/sgcdet_amd_image.h"

namespace sgc {

struct Conv2dExParams {
  const float *x;                 // [N*H*W, Cin]
  const __bf16 *w_hi, *w_lo;      // [k*k][Cout][Cin]
  const float *scale, *shift;     // [Cout] or null
  const float *residual;          // [N*OH*OW, ldr] or null
  float *y;                       // [N*OH*OW, ldy], columns [col0, col0 + Cout)
  int H, W, Cin, Cout;
  int ksize, stride, pad, transposed;
  int gh, gw, M;                  // GEMM rows: one per output pixel (transposed: per INPUT pixel and parity class)
  int OH, OW;
  int relu1, relu2;
  int ldy, col0, ldr, softmax_cols;
};

template <int BN, int NP>
__global__ __launch_bounds__(256) void conv2d_ex_kernel(const Conv2dExParams p) {
  using Tile = IgemmTile<BN, (BN == 128 ? 2 : 4), (BN == 128 ? 2 : 1), NP>;
  constexpr int NT = Tile::NT, ACH = Tile::ACH;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_b[];
  Tile t(smem_b, threadIdx.x);
  const int tid = t.tid;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  const int ph = p.transposed ? (int)(blockIdx.z >> 1) : 0, pw = p.transposed ? (int)(blockIdx.z & 1) : 0;
  const int ntaps = p.transposed ? (ph + 1) * (pw + 1) : p.ksize * p.ksize;
  const int ksteps_c = p.Cin / BK;

  // --- addressing: GEMM row -> (image, h, w); tap -> input pixel and weight slab ---
  int an[ACH], ah_[ACH], aw_[ACH];
  bool arow_ok[ACH];
#pragma unroll
  for (int i = 0; i < ACH; ++i) {
    const int m = m0 + t.a_row(i);
    arow_ok[i] = m < p.M;
    const int mm = arow_ok[i] ? m : 0;
    aw_[i] = mm % p.gw;
    ah_[i] = (mm / p.gw) % p.gh;
    an[i] = mm / (p.gw * p.gh);
  }
  t.bind(p.x, (int64_t)(p.M / (p.gh * p.gw)) * p.H * p.W * p.Cin * 4, p.w_hi, p.w_lo, (int64_t)p.ksize * p.ksize * p.Cout * p.Cin * 2,
         n0, p.Cout, p.Cin);
  int wtap = 0;                                   // the weight slab of the tap being loaded
  auto set_tap = [&](int tap) {
    int dh, dw;
    if (p.transposed) {
      // output row 2 h + ph receives input row ih through kernel row kh = 2 (h - ih) + ph + 1: ph = 0 -> (kh 1, ih h);
      // ph = 1 -> (kh 2, ih h), (kh 0, ih h + 1).  Same along the columns.
      const int nw = pw + 1, th = tap / nw, tw = tap - th * nw;
      const int kh = ph ? (th ? 0 : 2) : 1, kw = pw ? (tw ? 0 : 2) : 1;
      dh = th; dw = tw;
      wtap = kh * 3 + kw;
    } else {
      dh = tap / p.ksize - p.pad; dw = tap % p.ksize - p.pad;
      wtap = tap;
    }
#pragma unroll
    for (int i = 0; i < ACH; ++i) {
      const int hh = ah_[i] * p.stride + dh, ww = aw_[i] * p.stride + dw;
      const bool ok = arow_ok[i] && hh >= 0 && hh < p.H && ww >= 0 && ww < p.W;
      t.aoff[i] = ok ? ((unsigned)((an[i] * p.H + hh) * p.W + ww) * (unsigned)p.Cin + t.c4 * 4) * 4u : Tile::OOB;
    }
  };
  int ld_tap = 0, ld_kc = 0;
  set_tap(0);
  t.run(ntaps * ksteps_c, [&]() {
    t.load(__builtin_amdgcn_readfirstlane(ld_kc * (BK * 4)),
           __builtin_amdgcn_readfirstlane((wtap * p.Cout * p.Cin + ld_kc * BK) * 2));
    if (++ld_kc == ksteps_c) {
      ld_kc = 0;
      if (++ld_tap < ntaps) set_tap(ld_tap);
    }
  });

  // --- store policy: row pitch ldy, column offset col0, output parity of the transposed form, optional row softmax ---
  float *cs = t.scatter();
  auto out_row = [&](int m) -> int64_t {
    if (!p.transposed) return m;
    const int w = m % p.gw, h = (m / p.gw) % p.gh, n = m / (p.gw * p.gh);
    return ((int64_t)n * p.OH + (2 * h + ph)) * p.OW + (2 * w + pw);
  };
  constexpr int C4 = Tile::C4, LDC = Tile::LDC;
  const bool sm = p.softmax_cols > 0;
  for (int e = tid; e < BM * C4; e += NT) {
    const int rl = e / C4, q = e - rl * C4;
    const int m = m0 + rl, col = n0 + q * 4;
    if (m >= p.M || col >= p.Cout) continue;
    const int64_t orow = out_row(m);
    const float4 v = epilogue4(*Tile::c_quad(cs, rl, q), col, p.scale, p.shift, p.relu1, p.residual, orow * p.ldr + col, p.relu2);
    if (sm) *Tile::c_quad(cs, rl, q) = v;                                      // (one column tile: the host checks Cout <= BN)
    else *reinterpret_cast<float4 *>(p.y + orow * p.ldy + p.col0 + col) = v;
  }
  if (!sm) return;
  __syncthreads();
  // row softmax over columns [0, softmax_cols); the columns behind them leave as they are.  One thread per row: the rows are
  // at most BN floats and this is the 12-channel depth_reg layer.
  for (int rl = tid; rl < BM; rl += NT) {
    const int m = m0 + rl;
    if (m >= p.M) continue;
    float *row = cs + rl * LDC;
    float mx = row[0];
    for (int c = 1; c < p.softmax_cols; ++c) mx = fmaxf(mx, row[c]);
    float sum = 0.f;
    for (int c = 0; c < p.softmax_cols; ++c) { const float ev = expf(row[c] - mx); row[c] = ev; sum += ev; }
    const float inv = 1.f / sum;
    for (int c = 0; c < p.softmax_cols; ++c) row[c] *= inv;
    float *dst = p.y + out_row(m) * p.ldy + p.col0;
    for (int c = 0; c < p.Cout; c += 4) *reinterpret_cast<float4 *>(dst + c) = *reinterpret_cast<const float4 *>(row + c);
  }
}

template <int BN, int NP>
static void launch_ex_bn(const Conv2dExParams &p, dim3 grid, hipStream_t st) {
  static std::atomic<uint64_t> done{0};
  constexpr int smem = igemm_tile_lds_bytes(BN);
  ensure_dynamic_lds((const void *)conv2d_ex_kernel<BN, NP>, smem, done);
  hipLaunchKernelGGL((conv2d_ex_kernel<BN, NP>), grid, dim3(256), smem, st, p);
}
template <int NP>
static void launch_ex(const Conv2dExParams &p, int bn, dim3 grid, hipStream_t st) {
  if (bn == 128) launch_ex_bn<128, NP>(p, grid, st);
  else if (bn == 64) launch_ex_bn<64, NP>(p, grid, st);
  else launch_ex_bn<32, NP>(p, grid, st);
}

// columns per workgroup tile: the width that computes the fewest padded columns, the wider tile on a tie
static int ex_tile_cols(int Cout) {
  if (Cout <= 32) return 32;
  const int c128 = ceil_div(Cout, 128) * 128, c64 = ceil_div(Cout, 64) * 64;
  return c128 <= c64 ? 128 : 64;
}

// `any_size`: the strided entry (sgc_conv2d_nhwc_strided_bf16x3) -- a stride-2 layer over any H, W, output ceil(H / 2) x ceil(W / 2)
static const char *ex_unsupported(int N, int H, int W, int Cin, int Cout, int ksize, int stride, int transposed, int ldy, int col0,
                                  int ldr, int softmax_cols, bool has_residual, bool any_size = false) {
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return "non-positive size";
  if (Cin % 32 || Cout % 4) return "needs Cin % 32 == 0 and Cout % 4 == 0";
  if (transposed) {
    if (any_size) return "the any-size strided entry has no transposed form";
    if (ksize != 3 || stride != 2) return "the transposed form is 3x3 stride 2 (padding 1, output_padding 1)";
  } else {
    if ((ksize != 1 && ksize != 3) || (stride != 1 && stride != 2)) return "ksize in {1, 3}, stride in {1, 2}";
    if (stride == 2 && ((H | W) & 1) && !any_size) return "a stride-2 layer needs even H and W";
  }
  if (ldy % 4 || col0 % 4 || col0 < 0 || col0 + Cout > ldy) return "needs ldy % 4 == 0, col0 % 4 == 0 and col0 + Cout <= ldy";
  if (has_residual && (ldr % 4 || ldr < Cout)) return "needs ldr % 4 == 0 and ldr >= Cout";
  if (softmax_cols < 0 || softmax_cols > Cout || (softmax_cols > 0 && Cout > 128)) return "softmax needs softmax_cols <= Cout <= 128";
  const int s = transposed ? 1 : stride;
  const int64_t OH = transposed ? 2 * H : (H + s - 1) / s, OW = transposed ? 2 * W : (W + s - 1) / s;    // == H / s on the sizes !any_size accepts
  if ((int64_t)N * H * W * Cin * 4 >= (int64_t)0xfffffff0u || (int64_t)ksize * ksize * Cout * Cin * 2 >= ((int64_t)1 << 31) ||
      (int64_t)N * OH * OW >= ((int64_t)1 << 31) || (int64_t)N * H * W >= ((int64_t)1 << 31))
    return "tensor too large for 32-bit buffer offsets";
  return nullptr;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The stem.  Tile = 8 x 32 output pixels per pass of a 256-thread workgroup (wave w: output rows 2w, 2w + 1 of the tile, one
// 32 x 64 MFMA strip each); the fp32 patch (21 x 69 x 3) is staged in LDS, element k = (c * 7 + kh) * 7 + kw of a row's
// im2col vector is patch[c][2 r + kh][2 q + kw] -- read through a 160-entry offset table (k >= 147 points at a zero word).
// The weights [64][160] (hi | lo) are staged once per workgroup, which then walks tiles with a grid stride.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int ST_TH = 8, ST_TW = 32, ST_PH = 2 * ST_TH + 5, ST_PW = 2 * ST_TW + 5, ST_PWP = ST_PW + 1;   // patch 21 x 69 (+1 pad)
constexpr int ST_PATCH = 3 * ST_PH * ST_PWP;          // floats; word ST_PATCH is the zero word
constexpr int ST_K = 160, ST_LDW = ST_K + 8;          // bf16 per staged weight row (336 B: conflict-free ds_read_b128)

struct StemParams {
  const float *img;               // [N, 3, H, W]
  const __bf16 *w_hi, *w_lo;      // [64][160]
  const float *scale, *shift;     // [64]
  float *y;                       // [N * OH * OW, 64]
  int N, H, W, OH, OW, tiles_h, tiles_w, ntiles, relu;
};

template <int NP>
__global__ __launch_bounds__(256) void conv2d_stem7_kernel(const StemParams p) {
  __shared__ __attribute__((aligned(16))) __bf16 wh[64 * ST_LDW];
  __shared__ __attribute__((aligned(16))) __bf16 wl[NP == 3 ? 64 * ST_LDW : 8];
  __shared__ float patch[ST_PATCH + 1];
  __shared__ int koff[ST_K];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  for (int e = tid; e < 64 * (ST_K / 8); e += 256) {
    const int n = e / (ST_K / 8), c8 = e - n * (ST_K / 8);
    *reinterpret_cast<uint4 *>(wh + n * ST_LDW + c8 * 8) = *reinterpret_cast<const uint4 *>(p.w_hi + n * ST_K + c8 * 8);
    if constexpr (NP == 3)
      *reinterpret_cast<uint4 *>(wl + n * ST_LDW + c8 * 8) = *reinterpret_cast<const uint4 *>(p.w_lo + n * ST_K + c8 * 8);
  }
  for (int k = tid; k < ST_K; k += 256) {
    const int c = k / 49, kh = (k % 49) / 7, kw = k % 7;
    koff[k] = k < 147 ? (c * ST_PH + kh) * ST_PWP + kw : -1;
  }
  if (tid == 0) patch[ST_PATCH] = 0.f;
  const int fr = lane & 31, fh = lane >> 5;
  for (int tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
    const int tw = tile % p.tiles_w, th = (tile / p.tiles_w) % p.tiles_h, n = tile / (p.tiles_w * p.tiles_h);
    const int oh0 = th * ST_TH, ow0 = tw * ST_TW;
    const int ih0 = 2 * oh0 - 3, iw0 = 2 * ow0 - 3;
    __syncthreads();                                   // the previous tile's fragment reads are done (and the tables are written)
    for (int e = tid; e < 3 * ST_PH * ST_PW; e += 256) {
      const int x = e % ST_PW, yy = (e / ST_PW) % ST_PH, c = e / (ST_PW * ST_PH);
      const int ih = ih0 + yy, iw = iw0 + x;
      const bool ok = ih >= 0 && ih < p.H && iw >= 0 && iw < p.W;
      patch[(c * ST_PH + yy) * ST_PWP + x] = ok ? p.img[(((int64_t)n * 3 + c) * p.H + ih) * p.W + iw] : 0.f;
    }
    __syncthreads();
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int k = 0; k < 16; ++k) acc[i][j][k] = 0.f;
#pragma unroll 2
    for (int kk = 0; kk < ST_K / 16; ++kk) {
      bf16x8 bh[2], bl[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        bh[j] = *reinterpret_cast<const bf16x8 *>(wh + (j * 32 + fr) * ST_LDW + kk * 16 + fh * 8);
        if constexpr (NP == 3) bl[j] = *reinterpret_cast<const bf16x8 *>(wl + (j * 32 + fr) * ST_LDW + kk * 16 + fh * 8);
      }
      int ko[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) ko[e] = koff[kk * 16 + fh * 8 + e];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int rbase = (2 * (2 * wid + i)) * ST_PWP + 2 * fr;      // output pixel (2 wid + i, fr) of the tile
        bf16x8 ah, al;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float v = patch[ko[e] >= 0 ? rbase + ko[e] : ST_PATCH];
          const __bf16 hb = op_hi<NP>(v);
          ah[e] = hb;
          al[e] = op_lo<NP>(v, hb);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = mma_split<NP>(ah, al, bh[j], bl[j], acc[i][j]);
      }
    }
    // C layout: column = lane & 31, row (= pixel of the strip) = (k & 3) + 8 (k >> 2) + 4 (lane >> 5): a wave store covers
    // 2 pixels x 32 consecutive channels (two 128-byte runs)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int oh = oh0 + 2 * wid + i;
      if (oh >= p.OH) continue;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int col = j * 32 + (lane & 31);
        const float sc = p.scale ? p.scale[col] : 1.f, sh = p.shift ? p.shift[col] : 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          const int ow = ow0 + (k & 3) + 8 * (k >> 2) + 4 * (lane >> 5);
          if (ow >= p.OW) continue;
          float v = acc[i][j][k] * sc + sh;
          if (p.relu) v = relu_nan(v);
          p.y[(((int64_t)n * p.OH + oh) * p.OW + ow) * 64 + col] = v;
        }
      }
    }
  }
}

__global__ __launch_bounds__(256) void nchw_pad_rows_kernel(const float *__restrict__ src, float *__restrict__ dst, int64_t pixels,
                                                            int HW, int C, int Cp) {
  const int q4 = Cp / 4;
  const int64_t total = pixels * q4;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t pix = e % pixels;                     // consecutive lanes: consecutive pixels of one channel quad
    const int q = (int)(e / pixels);
    const int64_t n = pix / HW, s = pix - n * HW;
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = q * 4 + j;
      v[j] = c < C ? src[(n * C + c) * HW + s] : 0.f;
    }
    *reinterpret_cast<float4 *>(dst + pix * Cp + q * 4) = make_float4(v[0], v[1], v[2], v[3]);
  }
}
}  // namespace sgc

using namespace sgc;

extern "C" int sgc_conv2d_nhwc_ex_supported(int N, int H, int W, int Cin, int Cout, int ksize, int stride, int transposed,
                                            int ldy, int col0, int ldr, int softmax_cols) {
  return ex_unsupported(N, H, W, Cin, Cout, ksize, stride, transposed, ldy, col0, ldr, softmax_cols, ldr > 0) ? 0 : 1;
}

// The two entries of conv2d_ex_kernel.  Only the host side tells them apart: `any_size` admits odd H, W at stride 2, where the output
// is ceil(H / 2) x ceil(W / 2) (nn.Conv2d with padding k / 2).  The kernel walks M = N * OH * OW GEMM rows and bounds-checks every
// input pixel it addresses (row 2 oh + 1 of a 3x3 window on the last row of an odd image reads as zeros, like the padding), so on
// sizes both entries accept they launch the same kernel with the same parameters.
static int conv2d_ex(const char *who, bool any_size, const float *x, const uint16_t *w_hi, const uint16_t *w_lo, const float *scale,
                     const float *shift, const float *residual_or_null, float *y, int N, int H, int W, int Cin, int Cout, int ksize,
                     int stride, int transposed, int flags, int ldy, int col0, int ldr, int softmax_cols, sgc_stream_t stream) {
  if (!x || !w_hi || !w_lo || !y) return set_error(SGC_EINVAL, "%s: null pointer", who);
  if (flags & ~(SGC_CONV2D_RELU | SGC_CONV2D_RELU_AFTER_ADD)) return set_error(SGC_EINVAL, "%s: unknown flag", who);
  // every tensor moves as 16-byte vectors (buffer loads of x and the weight planes, float4 of scale / shift / residual / y)
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(w_hi) | reinterpret_cast<uintptr_t>(w_lo) |
       reinterpret_cast<uintptr_t>(scale) | reinterpret_cast<uintptr_t>(shift) | reinterpret_cast<uintptr_t>(residual_or_null) |
       reinterpret_cast<uintptr_t>(y)) & 15)
    return set_error(SGC_EUNSUP, "%s: pointers must be 16-byte aligned", who);
  if (const char *why = ex_unsupported(N, H, W, Cin, Cout, ksize, stride, transposed, ldy, col0, ldr, softmax_cols,
                                       residual_or_null != nullptr, any_size))
    return set_error(SGC_EUNSUP, "%s: %s", who, why);
  Conv2dExParams p = {};
  p.x = x; p.w_hi = reinterpret_cast<const __bf16 *>(w_hi); p.w_lo = reinterpret_cast<const __bf16 *>(w_lo);
  p.scale = scale; p.shift = shift; p.residual = residual_or_null; p.y = y;
  p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout;
  p.ksize = ksize; p.transposed = transposed ? 1 : 0;
  p.stride = p.transposed ? 1 : stride;
  p.pad = p.transposed ? 0 : ksize / 2;
  p.OH = p.transposed ? 2 * H : (H + stride - 1) / stride; p.OW = p.transposed ? 2 * W : (W + stride - 1) / stride;
  p.gh = p.transposed ? H : p.OH; p.gw = p.transposed ? W : p.OW;
  p.M = N * p.gh * p.gw;
  p.relu1 = (flags & SGC_CONV2D_RELU) ? 1 : 0; p.relu2 = (flags & SGC_CONV2D_RELU_AFTER_ADD) ? 1 : 0;
  p.ldy = ldy; p.col0 = col0; p.ldr = ldr; p.softmax_cols = softmax_cols;
  const int bn = softmax_cols > 0 ? (Cout <= 32 ? 32 : Cout <= 64 ? 64 : 128) : ex_tile_cols(Cout);
  const dim3 grid(ceil_div(p.M, 128), ceil_div(Cout, bn), p.transposed ? 4 : 1);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  with_products(g_conv_products, [&](auto np) { launch_ex<np()>(p, bn, grid, st); });
  return check_launch("conv2d_ex_kernel");
}

extern "C" int sgc_conv2d_nhwc_ex_bf16x3(const float *x, const uint16_t *w_hi, const uint16_t *w_lo, const float *scale,
                                         const float *shift, const float *residual_or_null, float *y, int N, int H, int W,
                                         int Cin, int Cout, int ksize, int stride, int transposed, int flags, int ldy, int col0,
                                         int ldr, int softmax_cols, sgc_stream_t stream) {
  return conv2d_ex("sgc_conv2d_nhwc_ex_bf16x3", false, x, w_hi, w_lo, scale, shift, residual_or_null, y, N, H, W, Cin, Cout, ksize,
                   stride, transposed, flags, ldy, col0, ldr, softmax_cols, stream);
}

extern "C" int sgc_conv2d_nhwc_strided_supported(int N, int H, int W, int Cin, int Cout, int ksize, int stride, int transposed,
                                                 int ldy, int col0, int ldr, int softmax_cols) {
  return ex_unsupported(N, H, W, Cin, Cout, ksize, stride, transposed, ldy, col0, ldr, softmax_cols, ldr > 0, true) ? 0 : 1;
}

extern "C" int sgc_conv2d_nhwc_strided_bf16x3(const float *x, const uint16_t *w_hi, const uint16_t *w_lo, const float *scale,
                                              const float *shift, const float *residual_or_null, float *y, int N, int H, int W,
                                              int Cin, int Cout, int ksize, int stride, int transposed, int flags, int ldy, int col0,
                                              int ldr, int softmax_cols, sgc_stream_t stream) {
  return conv2d_ex("sgc_conv2d_nhwc_strided_bf16x3", true, x, w_hi, w_lo, scale, shift, residual_or_null, y, N, H, W, Cin, Cout, ksize,
                   stride, transposed, flags, ldy, col0, ldr, softmax_cols, stream);
}

extern "C" int sgc_conv2d_stem7_bf16x3(const float *img, const uint16_t *w_hi, const uint16_t *w_lo, const float *scale,
                                       const float *shift, float *y, int N, int H, int W, int relu, sgc_stream_t stream) {
  if (!img || !w_hi || !w_lo || !y) return set_error(SGC_EINVAL, "sgc_conv2d_stem7_bf16x3: null pointer");
  if (N <= 0 || H <= 0 || W <= 0) return set_error(SGC_EINVAL, "sgc_conv2d_stem7_bf16x3: non-positive size");
  if ((H | W) & 1) return set_error(SGC_EUNSUP, "sgc_conv2d_stem7_bf16x3: needs even H and W");
  if ((reinterpret_cast<uintptr_t>(w_hi) | reinterpret_cast<uintptr_t>(w_lo)) & 15)
    return set_error(SGC_EUNSUP, "sgc_conv2d_stem7_bf16x3: the weight planes must be 16-byte aligned");
  StemParams p = {};
  p.img = img; p.w_hi = reinterpret_cast<const __bf16 *>(w_hi); p.w_lo = reinterpret_cast<const __bf16 *>(w_lo);
  p.scale = scale; p.shift = shift; p.y = y;
  p.N = N; p.H = H; p.W = W; p.OH = H / 2; p.OW = W / 2;
  p.tiles_h = ceil_div(p.OH, ST_TH); p.tiles_w = ceil_div(p.OW, ST_TW);
  const int64_t ntiles = (int64_t)N * p.tiles_h * p.tiles_w;
  if (ntiles >= ((int64_t)1 << 31)) return set_error(SGC_EUNSUP, "sgc_conv2d_stem7_bf16x3: too many tiles");
  p.ntiles = (int)ntiles; p.relu = relu ? 1 : 0;
  const int grid = (int)(ntiles < 4 * device_cus() ? ntiles : 4 * device_cus());
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  with_products(g_conv_products, [&](auto np) { hipLaunchKernelGGL((conv2d_stem7_kernel<np()>), dim3(grid), dim3(256), 0, st, p); });
  return check_launch("conv2d_stem7_kernel");
}

extern "C" int sgc_nchw_to_nhwc_padc(const float *src, float *dst, int N, int C, int H, int W, int Cp, sgc_stream_t stream) {
  if (!src || !dst) return set_error(SGC_EINVAL, "sgc_nchw_to_nhwc_padc: null pointer");
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || Cp < C || Cp % 4) return set_error(SGC_EINVAL, "sgc_nchw_to_nhwc_padc: needs Cp >= C, Cp % 4 == 0");
  if (reinterpret_cast<uintptr_t>(dst) & 15) return set_error(SGC_EUNSUP, "sgc_nchw_to_nhwc_padc: dst must be 16-byte aligned");
  const int64_t pixels = (int64_t)N * H * W, total = pixels * (Cp / 4);
  const int grid = (int)(total / 256 + 1 < 8192 ? total / 256 + 1 : 8192);
  hipLaunchKernelGGL(nchw_pad_rows_kernel, dim3(grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), src, dst, pixels, H * W, C, Cp);
  return check_launch("nchw_pad_rows_kernel");
}
