// The tuning knobs of the library (sgc_set_tuning, SGC_TUNE): ONE line per knob -- key, variable, default, meaning.
// Results never depend on a knob (the *_diag ones excepted, which are inert without SGC_DIAG=1, and wz_mfma, whose two values
// differ in the last bits: the instruction sums differently; each value is deterministic).  The variables are defined,
// and the keys looked up, in api.hip; why a default is what it is (A/B numbers, profiles/) is recorded next to the code that
// reads the knob.  Adding or retiring a knob is one line here.
#pragma once

#define SGC_TUNING_KNOBS(X)                                                                                                   \
  /* gather (dfa3d_fwd.hip, dfa3d_tile.hip, dfa3d_bwd_tile.hip) */                                                            \
  X("fwd_variant", g_tune_fwd_variant, 1, "0: block-barrier kernel, 1: wave-private kernel (when the shape allows)")         \
  X("fwd_spl", g_tune_fwd_spl, 1, "samples per lane in phase 1 of the wave kernel (1, 2, 4)")                                \
  X("tile_nw", g_tune_tile_nw, 0, "waves per workgroup (8 or 16); 0: by LDS footprint")                                      \
  X("tile_depth_lds", g_tune_tile_depth_lds, -1, ">= 0 overrides the caller's depth_in_lds")                                 \
  X("tile_diag", g_tune_tile_diag, 0, "timing experiments only (1 no compute, 2 no fill); inert without SGC_DIAG=1")         \
  X("tile_nbuf", g_tune_tile_nbuf, 0, "value-window buffers (2 needs heads per workgroup > 1); 0: one")                      \
  X("tile_xcd", g_tune_tile_xcd, -1, "1: camera n on XCD n % 8, 0: head h on XCD h, -1: 1 at Cm = 32, 0 at Cm = 16")          \
  X("tile_hg", g_tune_tile_hg, 0, "heads per workgroup; 0: one")                                                             \
  X("tile_ds", g_tune_tile_ds, 1, "1: one window test for value and depth where the windows coincide")                       \
  X("bwd_tile_diag", g_tune_bwd_tile_diag, 0, "timing experiments only; inert without SGC_DIAG=1")                           \
  /* projection, inter-view pooling, top-k (project.hip, view_pool.hip, rows.hip) */                                         \
  X("compact2", g_tune_compact2, 1, "1: two-launch segment form of sgc_compact_pairs, 0: the five kernels")                  \
  X("view_depth", g_tune_pq_depth, 4, "pair rows in flight per lane in view_attend / view_mean (1 | 2 | 4 | 8)")             \
  X("view_group", g_tune_view_group, 1, "0: the per-camera loops in view_mean / view_attend")                                \
  X("topk_multi_min", g_tune_topk_multi_min, 32769, "fewest candidates for the many-workgroup top-k")                        \
  /* row GEMMs (rows_gemm.hip) */                                                                                             \
  X("rows_gemm", g_tune_rows_gemm, 1, "0: every row GEMM on the tile implicit-GEMM kernel")                                  \
  X("rows_diag", g_tune_rows_diag, 0, "timing experiments only (bit 0 no stores, 1 no loads, 2 no MFMA); needs SGC_DIAG=1")  \
  X("rows_cu_pct", g_tune_rows_cu_pct, 100, "persistent row GEMM: share of the CUs it occupies")                             \
  X("rows_depth", g_tune_rows_depth, 1, "8-wave form: 2 = two tiles in flight ahead, anything else = one")                   \
  /* convolution plan (conv3d.hip: plan_conv and its helpers) */                                                              \
  X("conv_halo", g_tune_conv_halo, 1, "3x3x3 stride-1 layers: 0 tile kernel, 1 halo-resident kernel")                        \
  X("halo_min_cout", g_tune_halo_min_cout, 16, "fewest output channels for the halo kernel")                                 \
  X("halo_min_m", g_tune_halo_min_m, 2048, "fewest output voxels for the halo kernel")                                       \
  X("halo_brick", g_tune_halo_brick, 0, "0: brick by grid, 1: prefer 4x8x8, 2: force 8x8x4, 3: 4x4x16 at depth >= 16")       \
  X("halo_small", g_tune_halo_small, 1, "1: whole-grid bricks for the 10x10x4 / 12x12x4 grids at Cout >= 512")               \
  X("halo_narrow", g_tune_halo_narrow, 1, "1: 64- and 32-column tiles for few output channels, 64: never below 64, 0: 128")  \
  X("halo_2d", g_tune_halo_2d, 1, "3x3 layers over an image stack: 1 bricks of 16 x 16 pixels, 2 of 4 images x 8 x 8, 0 tile kernel") \
  X("wz_brick", g_tune_wz_brick, 0, "Winograd-z stack: 0 the brick with fewer matrix rows, 1: 4 images x 8 x 8, 2: 2 images x 10 x 10 (where each fits)") \
  X("wz_mfma", g_tune_wz_mfma, 16, "Winograd-z bricks: MFMA shape, 16 = 16x16x32, 32 = 32x32x16 (last-bit differences; each value deterministic)") \
  X("halo_split_target", g_tune_halo_split_target, 192, "halo kernel: channel slices are split until a launch has this many workgroups") \
  X("halo_wave_fix", g_tune_halo_wave_fix, 1, "one more split on a small CU overflow: 1 latency geometry only, 2 always")    \
  X("split_target", g_tune_split_target, 512, "tile kernel: the reduction is split until a launch has this many workgroups") \
  X("split_free", g_tune_split_free, 1, "tile kernel: 1 splits of whole K steps, 0 of whole tap groups")                     \
  X("split_min_steps", g_tune_split_min_steps, 8, "tile kernel: fewest K steps of a split (>= 1)")                           \
  X("split_max", g_tune_split_max, 32, "tile kernel: most splits (>= 1)")                                                    \
  /* convolution launchers (conv3d_igemm.hip, conv3d_halo.hip, conv3d_wgrad.hip) */                                          \
  X("conv_waves", g_tune_conv_waves, 8, "tile kernel: 4 or 8 waves per 128 x 128 tile")                                      \
  X("igemm_xcd", g_tune_igemm_xcd, 0, "tile kernel: XCD deal of the split / transposed layers (ConvParams.xcd_deal)")        \
  X("halo_stagger", g_tune_halo_stagger, 1, "halo kernel: 1 barrier at mid-tap (software-pipelined), 0 lockstep")            \
  X("wgrad_waves", g_tune_wgrad_waves, 8, "weight-gradient tile kernel: 4 or 8 waves")                                       \
  X("wgrad_halo", g_tune_wgrad_halo, 1, "3x3x3 stride-1 weight gradient: 1 double-buffered halo form, 2 single, 0 tile kernel")

namespace sgc {
#define SGC_KNOB_DECLARE(key, var, def, doc) extern int var;
SGC_TUNING_KNOBS(SGC_KNOB_DECLARE)
#undef SGC_KNOB_DECLARE
}  // namespace sgc
