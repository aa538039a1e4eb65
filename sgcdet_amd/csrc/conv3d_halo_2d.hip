// Halo convolution, 2-D forms over a stack of images: bricks of 16 x 16 pixels or 4 images x 8 x 8, and the virtual Winograd stack
// (bricks of 4 images x 8 x 8 or 2 images x 10 x 10 pixels: plan_conv takes the one with fewer matrix rows for the grid).
#include "conv3d_halo.hpp"

namespace sgc {
int launch_halo_2d(ConvParamsB &p, const ConvPlan &pl, hipStream_t st) {
  if (pl.family == kConvHaloWZ && pl.mfma == 16)      // the Winograd bricks on v_mfma_f32_16x16x32 (`wz_mfma`)
    return pl.bx == 2 ? launch_halo<2, 10, 10, 128, true, true, 16>(p, st) : launch_halo<4, 8, 8, 128, true, true, 16>(p, st);
  if (pl.family == kConvHaloWZ)
    return pl.bx == 2 ? launch_halo<2, 10, 10, 128, true, true>(p, st) : launch_halo<4, 8, 8, 128, true, true>(p, st);
  if (pl.bx == 4) return launch_halo<4, 8, 8, 128, true>(p, st);
  return pl.bn == 64 ? launch_halo<1, 16, 16, 64, true>(p, st) : launch_halo<1, 16, 16, 128, true>(p, st);
}
}  // namespace sgc
