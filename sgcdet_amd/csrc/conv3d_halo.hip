// Halo convolution: which instantiation a plan (plan_conv, conv3d.hip) names, and the deep 3-D bricks (4x4x16, 4x8x8).
#include "conv3d_halo.hpp"

namespace sgc {
// the ladder of instantiations: one per (family, brick, column tile) a plan can name
int launch_halo(ConvParamsB &p, const ConvPlan &pl, hipStream_t st) {
  if (pl.family == kConvHalo2D || pl.family == kConvHaloWZ) return launch_halo_2d(p, pl, st);
  if (pl.bz == 4) return launch_halo_z4(p, pl, st);
  if (pl.bx == 4 && pl.by == 4 && pl.bz == 16)
    return pl.bn == 32 ? launch_halo<4, 4, 16, 32>(p, st) : pl.bn == 64 ? launch_halo<4, 4, 16, 64>(p, st) : launch_halo<4, 4, 16>(p, st);
  if (pl.bx == 4 && pl.by == 8 && pl.bz == 8)
    return pl.bn == 32 ? launch_halo<4, 8, 8, 32>(p, st) : pl.bn == 64 ? launch_halo<4, 8, 8, 64>(p, st) : launch_halo<4, 8, 8>(p, st);
  return set_error(SGC_EUNSUP, "conv: no halo kernel of brick %d x %d x %d", pl.bx, pl.by, pl.bz);
}
}  // namespace sgc

#if defined(SGC_HALO_STAMPS)
extern "C" void sgc_diag_halo_stamp_buffer(unsigned long long *buf) { sgc::g_halo_stamp_buf = buf; }
#endif
