// Halo convolution, 3-D bricks of depth 4: 8x8x4 and the whole-grid bricks 10x10x4 / 6x12x4 (kConvHaloGrid).
#include "conv3d_halo.hpp"

namespace sgc {
int launch_halo_z4(ConvParamsB &p, const ConvPlan &pl, hipStream_t st) {
  if (pl.bx == 8 && pl.by == 8)
    return pl.bn == 32 ? launch_halo<8, 8, 4, 32>(p, st) : pl.bn == 64 ? launch_halo<8, 8, 4, 64>(p, st) : launch_halo<8, 8, 4>(p, st);
  if (pl.bx == 10 && pl.by == 10) return launch_halo<10, 10, 4, 64>(p, st);
  if (pl.bx == 6 && pl.by == 12) return launch_halo<6, 12, 4, 64>(p, st);
  return set_error(SGC_EUNSUP, "conv: no halo kernel of brick %d x %d x %d", pl.bx, pl.by, pl.bz);
}
}  // namespace sgc
