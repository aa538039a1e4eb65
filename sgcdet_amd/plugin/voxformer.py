"""Geometry-and-context-aware aggregation (the VoxFormer stack of SGCDet) for MI355X.

Registry names, constructor kwargs, parameter names and call signatures follow the
reference so that ``configs/SGCDet_*.py`` build unchanged and released checkpoints load
(SURVEY.md appendix A.5); the data flow does not.  Reference classes mirrored
(paths under mmdet3d_plugin/models/im2voxel/transformer_utils/):

=============================  =========================================================
``MSDeformableAttention3D_DFA3D``  deformable_cross_attention.py:119-212,343-501
``DeformCrossAttention_DFA3D``     deformable_cross_attention.py:504-548,691-837
``VoxFormerLayer``                 encoder.py:226-340, custom_base_transformer_layer.py:37-156
``VoxFormerEncoder_DFA3D``         encoder.py:18-48,158-223
``PerceptionTransformer_DFA3D``    transformer.py:26-50,115-185
=============================  =========================================================

What is different on MI355X (inference path, ``torch.is_grad_enabled() == False``):

* projection + visibility mask: one HIP kernel (``sgc_project_points``) instead of ~15 torch
  ops and 3 host->device copies; the 3x4 matrices are still composed on the host with the
  reference's own torch calls, once per scene;
* per-camera ``nonzero`` / rebatch / scatter Python loops (3N iterations, N host syncs):
  one compaction (``sgc_compact_pairs``) into a camera-major (camera, query) pair list and
  ONE host read of 4 ints; no padded ``max_len`` rows, no dense ``[N,1,Nq,C]`` slots;
* geometry sample and deformable gather: fused kernels over the pair list; softmax over
  the sampling points and the ``ref + offset/(W,H,D)`` arithmetic happen in-kernel from the
  raw Linear outputs (one [pairs, C] x [C, 4MP] GEMM instead of three small ones);
* inter-view ``nn.MultiheadAttention``: K/V are projected for visible pairs only (one GEMM),
  the softmax over views is a wave-shuffle kernel.

With autograd enabled the module runs the reference's data layout (padded per-camera
batches, dense slots) through the fused HIP forward/backward autograd Function -- same
numerics, training parity first.
"""
import copy
import math
import warnings

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..mmcv_lite import (ATTENTION, TRANSFORMER, TRANSFORMER_LAYER, TRANSFORMER_LAYER_SEQUENCE,
                         BaseModule, ModuleList, TransformerLayerSequence,
                         build_attention, build_feedforward_network, build_norm_layer,
                         build_transformer_layer_sequence, constant_init, xavier_init)
from ..functions import MultiScale3DDeformableAttnFunction_fp32
from .. import ext
from .conv_plan import BlockDiagSpec, LinearSpec, cached_plan, module_fingerprint


def _ops():
    return ext.ops()


# LDS-tiled deformable gather (csrc/dfa3d_tile.hip): which levels take it and how their windows are cut.  Results never
# depend on these numbers (tests/test_gpu_kernels.py::test_tiled_gather_against_oracle); they were chosen by
# tools/tile_bench.py sweeps on MI355X.  ``min_pixels``: smaller maps keep the wave kernel.
# ``storage``: "f32" (parity mode, the default) or "bf16" -- OPT-IN storage mode (BASELINE.json configs #2/#5): value_proj's
# epilogue writes the head-major value map as bfloat16 and the depth distributions are handed over as bfloat16 too (round 4; the
# reference's fp16 twin casts both, TU/multi_scale_3ddeformable_attn_function.py:353-428); the gather widens the taps and
# accumulates in fp32, outputs fp32.
# Not parity-exact (one bf16 rounding of every value, bound stated in tests/test_gpu_kernels.py); never the headline.
TILED_GATHER = dict(enabled=True, min_pixels=2048, storage="f32",
                    cm32=dict(bin=(16, 22), halo=(3, 3), depth_in_lds=False),
                    cm16=dict(bin=(16, 22), halo=(3, 3), depth_in_lds=True))     # 67.4 KB with the per-head depth window: two
                                                                                  # workgroups per CU (27x30: 130 KB, one)


# LDS-tiled backward of the two DFA3D calls of a TRAINING level (csrc/dfa3d_bwd_tile.hip, sgc_dfa3d_backward_binned): the training
# forward bins its pairs like the inference path and the backward accumulates a (camera, bin) window of grad_value / grad_dist in
# LDS.  ``bin`` / ``halo`` in feature pixels (the window = bin + 2 halo must fit 160 KiB at (Cm + 1 + D) * 4 bytes per pixel); corners
# outside the window fall back to global atomics, so results never depend on these numbers beyond float-atomic order.
# Env (A/B): SGC_TRAIN_BWD=0 (the item kernel, one global atomic per corner contribution) | "bin_w,bin_h,halo_x,halo_y".
# sample + offsets | logits projection in one pass where supported (sgc_pairs_geometry_linear_bf16x3); SGC_GEO_LINEAR=0: the two launches (A/B)
GEO_LINEAR_FUSED = __import__("os").environ.get("SGC_GEO_LINEAR", "1") != "0"

TRAIN_BWD_TILED = dict(enabled=True, bin=(8, 22), halo=(2, 2))       # 12 x 26-pixel windows: 79 KB of LDS at Cm = 32, two workgroups per CU (sweep: profiles/r06_bwd_tile_bench_cfg2.txt)


# The small stages of a TRAINING level on this library's kernels (include/sgcdet_amd_level_train.h): LayerNorm forward
# + backward, ONE concatenated [uv | depth | logits] projection with the sampling locations and the attention softmax behind it in
# one launch each way, the mean over views without float atomics, the slot scatter.  OPT-IN (env SGC_LEVEL_TRAIN_FUSED=1, or flip the
# entry inside a process); it takes effect under autograd on CUDA fp32 tensors with TRAIN_CONV == "hip" on the pair-list path only.
TRAIN_LEVEL_FUSED = dict(enabled=__import__("os").environ.get("SGC_LEVEL_TRAIN_FUSED", "0") == "1")


def _level_fused(x):
    """Does the fused training level apply to the tensor ``x``?"""
    if not TRAIN_LEVEL_FUSED["enabled"] or not torch.is_grad_enabled() or not x.is_cuda or x.dtype != torch.float32:
        return False
    from .conv_plan import TRAIN_CONV, train_products_ok
    return TRAIN_CONV == "hip" and train_products_ok()


def _tiled_env_overrides():
    """Sweeps without editing the file: SGC_TILED=0|1, SGC_TILED_CM32 / SGC_TILED_CM16 = "bin_w,bin_h,halo_x,halo_y,depth_in_lds"."""
    import os
    if "SGC_TILED" in os.environ:
        TILED_GATHER["enabled"] = os.environ["SGC_TILED"] != "0"
    if os.environ.get("SGC_STORAGE") in ("f32", "bf16"):
        TILED_GATHER["storage"] = os.environ["SGC_STORAGE"]
    spec = os.environ.get("SGC_TRAIN_BWD")
    if spec == "0":
        TRAIN_BWD_TILED["enabled"] = False
    elif spec:
        bw, bh, hx, hy = (int(v) for v in spec.split(","))
        TRAIN_BWD_TILED.update(enabled=True, bin=(bw, bh), halo=(hx, hy))
    for key in ("cm32", "cm16"):
        spec = os.environ.get("SGC_TILED_" + key.upper())
        if spec:
            bw, bh, hx, hy, dl = (int(v) for v in spec.split(","))
            TILED_GATHER[key] = dict(bin=(bw, bh), halo=(hx, hy), depth_in_lds=bool(dl))


_tiled_env_overrides()


def _head_major_raw_rows(M, P):
    """Row order of the fused [uv | dz | logit] projection that makes the GEMM emit [pairs][M][P][(du, dv, dz, logit)]."""
    idx = []
    for m in range(M):
        for p in range(P):
            mp = m * P + p
            idx += [mp * 2, mp * 2 + 1, M * P * 2 + mp, M * P * 3 + mp]
    return torch.tensor(idx, dtype=torch.long)


# ----------------------------------------------------------------------------------------
@ATTENTION.register_module()
class MSDeformableAttention3D_DFA3D(BaseModule):
    """Context-aware 3D deformable attention (per camera)."""

    def __init__(self, embed_dims=256, num_heads=8, num_levels=4, num_points=8, im2col_step=64,
                 dropout=0.1, batch_first=True, norm_cfg=None, init_cfg=None):
        super().__init__(init_cfg)
        if embed_dims % num_heads != 0:
            raise ValueError(f"embed_dims must be divisible by num_heads, but got {embed_dims} and {num_heads}")
        dim_per_head = embed_dims // num_heads
        if dim_per_head & (dim_per_head - 1):
            warnings.warn("embed_dims // num_heads is not a power of two: the gather falls back to "
                          "narrower vector loads")
        self.norm_cfg = norm_cfg
        self.batch_first = batch_first
        self.output_proj = None
        self.fp16_enabled = False
        self.im2col_step = im2col_step
        self.embed_dims = embed_dims
        self.num_levels = num_levels
        self.num_heads = num_heads
        self.num_points = num_points
        self.sampling_offsets = nn.Linear(embed_dims, num_heads * num_levels * num_points * 2)
        self.attention_weights = nn.Linear(embed_dims, num_heads * num_levels * num_points)
        self.value_proj = nn.Linear(embed_dims, embed_dims)
        self.sampling_offsets_depth = nn.Linear(embed_dims, num_heads * num_levels * num_points)
        self.init_weights()

    def init_weights(self):
        """deformable_cross_attention.py:194-212 (uv ring) and :351-362 (depth offsets)."""
        M, L, P = self.num_heads, self.num_levels, self.num_points
        thetas = torch.arange(M, dtype=torch.float32) * (2.0 * math.pi / M)
        ring = torch.stack([thetas.cos(), thetas.sin()], -1)
        ring = ring / ring.abs().max(-1, keepdim=True)[0]
        steps = torch.arange(1, P + 1, dtype=torch.float32)
        constant_init(self.sampling_offsets, 0.0)
        self.sampling_offsets.bias.data = (ring.view(M, 1, 1, 2) * steps.view(1, 1, P, 1)).expand(M, L, P, 2).reshape(-1).clone()
        constant_init(self.attention_weights, val=0.0, bias=0.0)
        xavier_init(self.value_proj, distribution="uniform", bias=0.0)
        constant_init(self.sampling_offsets_depth, 0.0)
        dz = (thetas.cos() + thetas.sin()) / 2
        self.sampling_offsets_depth.bias.data = (dz.view(M, 1, 1) * steps.view(1, 1, P)).expand(M, L, P).reshape(-1).clone()
        self._is_init = True

    def get_spatial_shape_3D(self, spatial_shape, depth_dim):
        d = spatial_shape.new_full((*spatial_shape.shape[:-1], 1), depth_dim)
        return torch.cat([spatial_shape, d], dim=-1).contiguous()

    # fused projection weights for the pair-list path: [uv offsets | depth offsets | logits]
    def raw_projection(self, x):
        w = torch.cat([self.sampling_offsets.weight, self.sampling_offsets_depth.weight,
                       self.attention_weights.weight], 0)
        b = torch.cat([self.sampling_offsets.bias, self.sampling_offsets_depth.bias,
                       self.attention_weights.bias], 0)
        return F.linear(x, w, b)

    def forward(self, query, key=None, value=None, value_dpt_dist=None, identity=None, query_pos=None,
                key_padding_mask=None, reference_points=None, spatial_shapes=None,
                level_start_index=None, **kwargs):
        """Reference-compatible batched call (bs = cameras): returns ``(output, weight_update)``.

        query [bs,Q,C]; value [bs,S,C]; value_dpt_dist [bs,S,D]; reference_points [bs,Q,1,3]."""
        if value is None:
            value = query
        if query_pos is not None:
            query = query + query_pos
        if not self.batch_first:
            query = query.permute(1, 0, 2)
            value = value.permute(1, 0, 2)
        bs, num_query, _ = query.shape
        _, num_value, _ = value.shape
        M, L, P = self.num_heads, self.num_levels, self.num_points
        value = self.value_proj(value)
        if key_padding_mask is not None:
            value = value.masked_fill(key_padding_mask[..., None], 0.0)
        value = value.view(bs, num_value, M, -1)
        dim_depth = value_dpt_dist.shape[-1]
        dist = value_dpt_dist.reshape(bs, num_value, 1, dim_depth)      # NOT replicated per head
        off_uv = self.sampling_offsets(query).view(bs, num_query, M, L, P, 2)
        off_d = self.sampling_offsets_depth(query).view(bs, num_query, M, L, P, 1)
        offsets = torch.cat([off_uv, off_d], dim=-1)
        attention_weights = self.attention_weights(query).view(bs, num_query, M, L * P).softmax(-1)
        attention_weights = attention_weights.view(bs, num_query, M, L, P)
        shapes3 = self.get_spatial_shape_3D(spatial_shapes, dim_depth)
        if reference_points.shape[-1] != 3:
            raise ValueError(f"Last dim of reference_points must be 3, but get {reference_points.shape[-1]} instead.")
        num_Z = reference_points.shape[2]
        normalizer = torch.stack([shapes3[..., 1], shapes3[..., 0], shapes3[..., 2]], -1).to(offsets.dtype)
        offsets = offsets / normalizer[None, None, None, :, None, :]
        offsets = offsets.view(bs, num_query, M, L, P // num_Z, num_Z, 3)
        loc = (reference_points[:, :, None, None, None, :, :] + offsets).view(bs, num_query, M, L, P, 3)
        output, depth_score = MultiScale3DDeformableAttnFunction_fp32.apply(
            value, dist, shapes3, level_start_index, loc, attention_weights, self.im2col_step)
        weight_update = (depth_score.mean(dim=-1) * attention_weights).flatten(-2).sum(dim=-1, keepdim=True)
        if not self.batch_first:
            output = output.permute(1, 0, 2)
        return output, weight_update


class _ZeroLinear:
    """Stands where ``sampling_offsets_depth`` is in the DFA3D class: a weight / bias of zeros that is no parameter
    (nothing to learn, nothing in the state dict), on whatever device the module lives."""

    def __init__(self, like, out_features):
        self.weight = like.weight.new_zeros((out_features, like.weight.shape[1]))
        self.bias = like.weight.new_zeros((out_features,))

    def __call__(self, x):
        return F.linear(x, self.weight, self.bias)


@ATTENTION.register_module()
class MSDeformableAttention3D(MSDeformableAttention3D_DFA3D):
    """The 2-D deformable attention (deformable_cross_attention.py:119-341; no SGCDet config selects it).  The reference
    hands it to mmcv's ``MultiScaleDeformableAttnFunction``; here it is the same HIP gather as the DFA3D class, run on a
    one-bin depth map of ones with every sample at the centre of that bin: the depth interpolation then weighs every
    sample with exactly 1.0, and what is left is the bilinear 2-D operator (pinned against ``F.grid_sample`` in
    tests/test_oracle_identity.py and, through the kernels, in tests/test_gpu_modules.py)."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        del self._modules["sampling_offsets_depth"]

    @property
    def sampling_offsets_depth(self):
        if "sampling_offsets_depth" in self._modules:          # only while the parent constructor runs
            return self._modules["sampling_offsets_depth"]
        z = self.__dict__.get("_zero_depth")
        w = self.sampling_offsets.weight
        if z is None or z.weight.device != w.device or z.weight.dtype != w.dtype:
            z = self.__dict__["_zero_depth"] = _ZeroLinear(self.sampling_offsets, self.num_heads * self.num_levels * self.num_points)
        return z

    def init_weights(self):
        super().init_weights()                                  # writes its depth-offset bias into the stand-in ...
        self.__dict__.pop("_zero_depth", None)                  # ... which is dropped: the next access builds zeros again

    def forward(self, query, key=None, value=None, identity=None, query_pos=None, key_padding_mask=None,
                reference_points=None, spatial_shapes=None, level_start_index=None, value_dpt_dist=None, **kwargs):
        """query [bs,Q,C]; value [bs,S,C]; reference_points [bs,Q,Z,2] -> [bs,Q,C] (:215-341)."""
        if reference_points.shape[-1] != 2:
            raise ValueError(f"Last dim of reference_points must be 2, but get {reference_points.shape[-1]} instead.")
        v = query if value is None else value
        n_rows = v.shape[1] if self.batch_first else v.shape[0]
        bs = v.shape[0] if self.batch_first else v.shape[1]
        ones = v.new_ones((bs, n_rows, 1))
        ref3 = torch.cat([reference_points, reference_points.new_full((*reference_points.shape[:-1], 1), 0.5)], -1)
        out, _ = super().forward(query, key, value, ones, identity, query_pos, key_padding_mask, ref3, spatial_shapes,
                                 level_start_index, **kwargs)
        return out


# ----------------------------------------------------------------------------------------
@ATTENTION.register_module()
class DeformCrossAttention_DFA3D(BaseModule):
    """Geometry-aware sample -> context-aware deformable attention -> attention over views."""

    def __init__(self, embed_dims=256, deformable_attn=True, inter_view_aggregation="attn", dropout=0.1,
                 init_cfg=None, batch_first=False, deformable_attention=None, **kwargs):
        super().__init__(init_cfg)
        self.dropout = nn.Dropout(dropout)
        self.fp16_enabled = False
        self.deformable_attention = build_attention(deformable_attention)
        self.embed_dims = embed_dims
        self.output_proj = nn.Linear(embed_dims, embed_dims)
        self.batch_first = batch_first
        self.deformable_attn = deformable_attn
        self.inter_view_aggregation = inter_view_aggregation
        if inter_view_aggregation == "attn":
            self.attention_pooling = nn.MultiheadAttention(embed_dim=embed_dims, num_heads=8, batch_first=False)
        self.init_weight()

    def init_weight(self):
        xavier_init(self.output_proj, distribution="uniform", bias=0.0)

    # the 2-D class adds the sampled feature back onto the deformable attention's output
    # (deformable_cross_attention.py:647 ``queries = queries + queries_per_image``); this one does not (:795-800)
    geo_residual = False

    def _gemm_plan(self):
        """The Linears of a level on the MFMA kernel (value_proj over N*S rows; the fused offset/logit projection
        and the K/V in-projection over the visible pairs; output_proj and the q / out projections of the view
        attention over the visible voxels); rebuilt when a parameter changes.  One kernel for all of them keeps a
        row's result independent of how many rows the call has, so the host-synchronised path and the
        device-count path (``static_counts``) are bit-identical."""
        return cached_plan(self, self._build_gemm_plan, "_gemm_cache")

    def _build_gemm_plan(self):
        da, mha, C = self.deformable_attention, self.attention_pooling, self.embed_dims
        raw_w = torch.cat([da.sampling_offsets.weight, da.sampling_offsets_depth.weight, da.attention_weights.weight], 0)
        raw_b = torch.cat([da.sampling_offsets.bias, da.sampling_offsets_depth.bias, da.attention_weights.bias], 0)
        hm = _head_major_raw_rows(da.num_heads, da.num_points).to(raw_w.device) if da.num_levels == 1 else None
        # a head's mean sampling offset in pixels (the bias of sampling_offsets; the weights add a data-dependent part
        # around it): the tiled gather shifts that head's LDS window by it.  Speed only.
        off = da.sampling_offsets.bias.detach().float().view(da.num_heads, -1, 2).mean(1).round().clamp(-8, 8)
        plan = dict(
            value=LinearSpec(da.value_proj.weight, da.value_proj.bias),
            raw=LinearSpec(raw_w, raw_b),
            raw_hm=LinearSpec(raw_w[hm], raw_b[hm]) if hm is not None else None,
            head_shift=off.to(torch.int32).contiguous(),
            max_shift=(int(off[:, 0].abs().max()), int(off[:, 1].abs().max())),
            kv=LinearSpec(mha.in_proj_weight[C:], mha.in_proj_bias[C:]),
            out=LinearSpec(self.output_proj.weight, self.output_proj.bias),
            # the pooled feature only feeds the query projection (:826-833): q = W_q (W_out mean + b_out) + b_q as ONE
            # Linear with the composed weights (fp32 composition; one GEMM launch less per level)
            qo=LinearSpec(mha.in_proj_weight[:C].detach().float() @ self.output_proj.weight.detach().float(),
                          mha.in_proj_weight[:C].detach().float() @ self.output_proj.bias.detach().float()
                          + mha.in_proj_bias[:C].detach().float()),
            o=LinearSpec(mha.out_proj.weight, mha.out_proj.bias))
        plan.update(self._projected_query_plan(mha, plan))
        return plan

    # Projected-query form of the inter-view attention (sgc_view_attend_pq, round 5): K and V leave the pair list.
    #   "auto": wherever the kernel supports the shape (8 heads, C in {128, 256}, <= 128 views) and a voxel is seen by enough
    #           cameras for the per-voxel GEMMs (C -> heads * C and heads * C -> C) to cost less than the per-pair K | V GEMM
    #           (C -> 2C on every visible pair): break-even MEASURED at ~30 ring views with V head by head (~45 with the dense 8C -> C GEMM);
    #   True / False force it on (where supported) / off.  Same function of the inputs either way (~1e-6: association of sums).
    projected_query = {"0": False, "1": True}.get(__import__("os").environ.get("SGC_PROJECTED_QUERY", ""), "auto")   # env: A/B runs
    # measured with V head by head (round 6, profiles/r06_pq_views.txt, r06_pq_ab.txt; config-2 shapes, four scenes in flight): 8 / 12 / 16 / 20
    # views -2 % / -1.3 % / -1.1 % / -0.6 %, 30 views even, 40 views +1.7 %, 100 views +1.5 % over the dense-V form that was already +9.8 %
    # over the per-pair K | V GEMM there.  (Round 5, dense 8C -> C V projection: break-even at ~45 views, profiles/r05_pq_ab.txt.)
    projected_query_min_views = 32
    # The form's two transients (projected queries and attention-weighted features) are [voxel capacity, heads * C] fp32 EACH: 0.6 GB per
    # level and scene in flight at config 5's 73.7 k voxels.  Past this many bytes for the pair the level keeps the per-pair K | V GEMM
    # (whose transient grows with the pairs instead).  A static rule on shapes: nothing is queried while a graph is being captured.
    projected_query_max_bytes = 2 << 30
    projected_query_blockdiag = __import__("os").environ.get("SGC_PQ_BLOCKDIAG", "1") != "0"     # V head by head (round 6); 0 = the dense 8C -> C GEMM

    def _projected_query_plan(self, mha, plan):
        """qp = scale * W_k,h^T q_h as ONE Linear on the pooled feature (composed with the q / output projections of `qo`), and
        V as a block-diagonal Linear heads * C -> C; composed in float64, stored fp32 (the GEMMs then run like every other)."""
        C, Hn = self.embed_dims, mha.num_heads
        if not _ops().view_attend_pq_supported(1, C, Hn):
            return dict(qp=None, vbd=None, vbd_g=None)
        hd = C // Hn
        w = mha.in_proj_weight.detach().double()
        b = mha.in_proj_bias.detach().double()
        wqo = w[:C] @ self.output_proj.weight.detach().double()                     # q = wqo mean + bqo (as `qo`)
        bqo = w[:C] @ self.output_proj.bias.detach().double() + b[:C]
        wk, wv, bv = w[C:2 * C], w[2 * C:], b[2 * C:]
        scale = (1.0 / hd) ** 0.5                                                    # torch MHA: q * sqrt(1 / head_dim)
        wqp = torch.cat([scale * wk[h * hd:(h + 1) * hd].t() @ wqo[h * hd:(h + 1) * hd] for h in range(Hn)], 0)      # [Hn C, C]
        bqp = torch.cat([scale * wk[h * hd:(h + 1) * hd].t() @ bqo[h * hd:(h + 1) * hd] for h in range(Hn)], 0)      # [Hn C]
        wbd = torch.zeros((C, Hn * C), dtype=torch.float64, device=w.device)
        for h in range(Hn):
            wbd[h * hd:(h + 1) * hd, h * C:(h + 1) * C] = wv[h * hd:(h + 1) * hd]
        # the same V projection kept as its Hn blocks (round 6, sgc_linear_rows_blockdiag_bf16x3: x read once, no zero blocks); the dense
        # form above stays as the A/B twin (SGC_PQ_BLOCKDIAG=0) and for shapes the block kernel does not take
        vg = None
        if self.projected_query_blockdiag and BlockDiagSpec.supported(Hn, C, hd):
            vg = BlockDiagSpec(wv.view(Hn, hd, C).float(), bv.float())
        return dict(qp=LinearSpec(wqp.float(), bqp.float()), vbd=LinearSpec(wbd.float(), bv.float(), useful=1.0 / Hn), vbd_g=vg)

    def _use_projected_query(self, gemm, n_views, n_rows_cap=0):
        if gemm is None or gemm.get("qp") is None or self.projected_query is False:
            return False
        if 2 * n_rows_cap * self.attention_pooling.num_heads * self.embed_dims * 4 > self.projected_query_max_bytes:
            return False
        if not _ops().view_attend_pq_supported(n_views, self.embed_dims, self.attention_pooling.num_heads):
            return False
        return self.projected_query is True or n_views >= self.projected_query_min_views

    # ---- inference: pair-list pipeline --------------------------------------------------
    def _forward_pairs(self, query, feat, dist, ref_cam, mask_u8, H, W, zero_query=False, static_counts=False, want_ctx=False):
        """query [1,Nq,C]; feat [N,S,C]; dist [N,S,D]; ref_cam [N,Nq,3]; mask_u8 [N,Nq].

        ``want_ctx`` (zero queries, attention aggregation on the MFMA path): stop in front of the attention's out
        projection and return ``(ctx [rows, C], row_of [Nq])`` -- VoxFormerLayer hands them to ``sgc_level_tail``, which
        runs out_proj, the slot scatter, both LayerNorms and the FFN in one launch.

        ``static_counts``: nothing is read back to the host.  The pair / visible-voxel counts stay in the
        ``totals`` tensor of ``compact_pairs``; buffers are sized for the worst case (N*Nq pairs, Nq voxels), every
        kernel takes its row count from the device and workgroups past it exit at once.  The launch sequence is
        then independent of the scene -- the precondition for replaying a whole scene as one hipGraph."""
        ops = _ops()
        C = self.embed_dims
        N, Nq = mask_u8.shape
        from .conv_plan import CONV_MODE
        use_mfma = self.deformable_attn and self.inter_view_aggregation == "attn" and C % 32 == 0
        pc = ops.compact_pairs(mask_u8)
        if static_counts:
            if not (use_mfma and CONV_MODE == "bf16x3"):
                raise NotImplementedError("static_counts needs the bf16x3 GEMM path (attn aggregation, C % 32 == 0)")
            n_pairs, n_valid = -1, Nq                      # capacities; the live counts stay on the device
            totals, pairs_cnt, valid_cnt = pc["totals"], pc["totals"][0:1], pc["totals"][1:2]
        else:
            n_pairs, n_valid, _, _ = pc["totals"].tolist()       # the one host sync of this level
            totals = pairs_cnt = valid_cnt = None
        if n_pairs == 0:
            if want_ctx:                                 # no camera sees any voxel: every row_of entry is -1
                return torch.zeros((1, C), dtype=feat.dtype, device=feat.device), pc["row_of"]
            out = torch.zeros((1, Nq, C), dtype=feat.dtype, device=feat.device)
            return out if zero_query else self.dropout(out) + query
        pair_cam, pair_q = pc["pair_cam"], pc["pair_q"]
        gemm = self._gemm_plan() if use_mfma else None
        da = self.deformable_attention
        S = feat.shape[1]              # == H*W, or the camera stride of channels-last maps that kept the cropped rows
        Cm = C // da.num_heads
        tiled = None
        if (self.deformable_attn and use_mfma and CONV_MODE in ("bf16x3", "f32") and TILED_GATHER["enabled"] and da.num_levels == 1
                and da.num_points == 4 and Cm in (16, 32) and TILED_GATHER["min_pixels"] <= H * W < 32767
                and dist.shape[-1] >= 2):
            tiled = TILED_GATHER["cm32" if Cm == 32 else "cm16"]
            bw, bh = min(tiled["bin"][0], W), min(tiled["bin"][1], H)
            # every camera's pairs regrouped by the feature pixel of their reference point; everything below runs in
            # that order (slot is rewritten, so the inter-view stages do not notice)
            pc = ops.bin_pairs(ref_cam, pc, H, W, bw, bh)
            pair_q = pc["pair_q"]
        # The sampled row of a pair has ONE reader, the fused offsets | logits projection: where the entry point takes the shape
        # (C = 128: BASELINE configs 4 / 5) sample and projection are one pass and the [pairs, C] tensor never exists
        # (sgc_pairs_geometry_linear_bf16x3; bit-identical to the two launches)
        fuse_geo = (GEO_LINEAR_FUSED and self.deformable_attn and not self.geo_residual and use_mfma and CONV_MODE == "bf16x3"
                    and da.num_levels == 1 and ops.pairs_geometry_linear_supported(C, da.num_heads * da.num_points * 4, N, S))
        geo = None if fuse_geo else ops.pairs_geometry_sample(feat, dist, ref_cam, pair_cam, pair_q, n_pairs, H, W, totals=totals)

        def raw_projection(spec):
            if fuse_geo:
                return ops.pairs_geometry_linear(feat, dist, ref_cam, pair_cam, pair_q, n_pairs, H, W, spec.w_hi, spec.w_lo, spec.shift,
                                                 totals=totals)
            return spec(geo, count=pairs_cnt)

        if self.deformable_attn:
            if da.num_levels != 1:
                raise NotImplementedError("pair-list path supports num_levels == 1 (all SGCDet configs)")
            if tiled is not None:
                if CONV_MODE == "bf16x3":
                    value = gemm["value"].headmajor(feat.view(N * S, C), N, S, da.num_heads,
                                                    out_dtype=torch.bfloat16 if TILED_GATHER["storage"] == "bf16" else torch.float32)
                else:
                    # strict fp32 products: the fp32 GEMM kernel stores row-major; one permuting copy puts the value map into
                    # the head-major layout the tiled gather stages its windows from (the copy costs ~70 us at the finest
                    # config-2 level, the tiled gather saves ~180 against the wave kernel)
                    value = gemm["value"](feat.view(N * S, C)).view(N, S, da.num_heads, Cm).permute(0, 2, 1, 3).contiguous()
                raw = raw_projection(gemm["raw_hm"])
                if not self.geo_residual:
                    del geo
                # the storage mode covers both maps: bf16 depth distributions beside the bf16 value map (one cast per level)
                dist_g = dist.to(torch.bfloat16) if value.dtype == torch.bfloat16 else dist
                per_pair = ops.pairs_deform_gather_tiled(value, dist_g, pc["pair_ref"], pc["bin_offset"], raw, H, W,
                                                         da.num_points, bw, bh, tiled["halo"][0], tiled["halo"][1],
                                                         head_shift=gemm["head_shift"], max_shift=gemm["max_shift"],
                                                         depth_in_lds=tiled["depth_in_lds"])
                if n_pairs >= 0:
                    per_pair = per_pair[:n_pairs]
            else:
                zero_row = use_mfma and CONV_MODE == "bf16x3"
                value = gemm["value"](feat.view(N * S, C), extra_zero_row=zero_row) if use_mfma else da.value_proj(feat)
                raw = raw_projection(gemm["raw"]) if use_mfma else da.raw_projection(geo)
                if not self.geo_residual:
                    del geo                               # capacity-sized in static mode: let the allocator reuse it
                per_pair = ops.pairs_deform_gather(value.view(N, S, da.num_heads, C // da.num_heads), dist,
                                                   ref_cam, raw, pair_cam, pair_q, n_pairs, H, W,
                                                   da.num_heads, da.num_points, totals=totals,
                                                   dist_pairs=ops.depth_pairs(dist, H, W), zero_row=zero_row)
            del raw, value
            if self.geo_residual:
                per_pair = per_pair.add_(geo[:per_pair.shape[0]])
        else:
            per_pair = geo
        slot, valid_index = pc["slot"], pc["valid_index"]
        mean = ops.view_mean(per_pair, slot, valid_index, n_valid, count=valid_cnt)
        if self.inter_view_aggregation != "attn" or not use_mfma:
            pooled = gemm["out"](mean, count=valid_cnt) if use_mfma else self.output_proj(mean)
        if self.inter_view_aggregation == "attn":
            mha = self.attention_pooling
            w, b = mha.in_proj_weight, mha.in_proj_bias
            if use_mfma and self._use_projected_query(gemm, N, n_valid):
                # K and V off the pair list (sgc_view_attend_pq): one projected query per (voxel, head) against the raw pair
                # features, V applied once per voxel to the attention-weighted feature
                qp = gemm["qp"](mean, count=valid_cnt)                                   # [n_valid, heads * C]
                sw = ops.view_attend_pq(qp, per_pair, slot, valid_index, mha.num_heads, count=valid_cnt)
                del qp
                ctx = (gemm["vbd_g"] if gemm.get("vbd_g") is not None else gemm["vbd"])(sw, count=valid_cnt)     # [n_valid, C]
                del sw
            else:
                if use_mfma:
                    q = gemm["qo"](mean, count=valid_cnt)
                    kv = gemm["kv"](per_pair, count=pairs_cnt)
                else:
                    q = F.linear(pooled, w[:C], b[:C])
                    kv = F.linear(per_pair, w[C:], b[C:])
                ctx = ops.view_attend(q, kv, slot, valid_index, mha.num_heads, count=valid_cnt)
            if want_ctx and use_mfma:
                return ctx, pc["row_of"]
            pooled = gemm["o"](ctx, count=valid_cnt) if use_mfma else F.linear(ctx, mha.out_proj.weight, mha.out_proj.bias)
        out = torch.zeros((1, Nq, C), dtype=feat.dtype, device=feat.device)
        ops.scatter_rows(pooled, valid_index, out.view(Nq, C), count=valid_cnt)
        out = self.dropout(out)
        return out if zero_query else out + query

    # ---- training: pair list, differentiable --------------------------------------------------
    # The reference (and `_forward_reference_layout` below, kept as the checker) pads every camera's visible queries to
    # max_len rows and samples / back-propagates the padding too.  Here the differentiable path runs on the visible pairs
    # only: the fused operator and its backward take an item list (functions.PairListDeformAttnFunction), the Linears are
    # torch ops on [n_pairs, .] rows; the inter-view nn.MultiheadAttention keeps the reference's dense [N, L, C] slots.
    train_pair_list = True

    def _forward_pairs_train(self, query, feat, dist, ref_cam, mask, spatial_shapes, level_start_index, spatial_hw=None):
        from ..functions import PairListDeformAttnFunction
        C = self.embed_dims
        N, Nq = mask.shape
        da = self.deformable_attention
        M, L, P = da.num_heads, da.num_levels, da.num_points
        S = feat.shape[1]
        value = None
        if self.deformable_attn:
            # issued BEFORE the host sync below: the value projection depends on the maps only, and its ~140 us of GPU work (config 2)
            # run while the host waits for the pair count and issues what follows
            from ..functions import linear_rows                    # the Linears' three passes on the MFMA kernels
            value = linear_rows(da.value_proj, feat).view(N, S, M, C // M)
        # The pair list, the per-voxel camera counts, `slot` and the compact voxel rows come from the compaction kernels of the
        # inference path (round 6; before: mask.nonzero / sum / index_put glue, two host syncs and ~10 torch launches per level).
        # With one feature level the pairs are also BINNED by the pixel of their reference point (sgc_bin_pairs): everything below
        # runs in that order (`slot` maps (camera, voxel) -> pair as before) and the backward of both DFA3D calls takes the
        # LDS-tiled kernel (sgc_dfa3d_backward_binned) instead of one global atomic per corner contribution.
        ops = _ops()
        mask_u8 = mask if mask.dtype == torch.uint8 else mask.to(torch.uint8)
        pc = ops.compact_pairs(mask_u8.contiguous())
        bins = None
        if L == 1 and TRAIN_BWD_TILED["enabled"] and feat.is_cuda and C % 16 == 0:
            H, W = spatial_hw if spatial_hw is not None else tuple(int(v) for v in spatial_shapes[0].tolist())
            bw, bh = min(TRAIN_BWD_TILED["bin"][0], W), min(TRAIN_BWD_TILED["bin"][1], H)
            if S >= H * W and ops.dfa3d_backward_binned_fits(H, W, 32 if C % 32 == 0 else 16, dist.shape[-1], bw, bh, TRAIN_BWD_TILED["halo"]):
                pc = ops.bin_pairs(ref_cam.contiguous(), pc, H, W, bw, bh)
                # head m's window follows its mean sampling offset (the bias of sampling_offsets, as the tiled forward's head_shift)
                shift = da.sampling_offsets.bias.detach().float().view(M, -1, 2).mean(1).round().clamp(-8, 8).to(torch.int32).contiguous()
                bins = (pc["bin_offset"], H, W, bw, bh, tuple(TRAIN_BWD_TILED["halo"]), shift)
        n_pairs, n_valid = pc["totals"][:2].tolist()                 # the level's one host sync
        cam, q = pc["pair_cam"][:n_pairs].long(), pc["pair_q"][:n_pairs].long()     # camera-major; inside a camera by bin, or ascending q
        from .conv_plan import TRAIN_CONV
        fused = _level_fused(feat) and C % 32 == 0          # TRAIN_LEVEL_FUSED: the int32 valid_index of the kernels serves throughout
        valid_index = None if fused else pc["valid_index"][:n_valid].long()
        count = pc["vox_count"]
        shapes3 = da.get_spatial_shape_3D(spatial_shapes, dist.shape[-1])
        ref = ref_cam[cam, q]                                          # [n_pairs, 3]
        item = pc["pair_cam"][:n_pairs]
        geo = PairListDeformAttnFunction.apply(feat.view(N, S, 1, C), dist.view(N, S, 1, -1), shapes3, level_start_index,
                                               ref.view(n_pairs, 1, 1, 1, 3).expand(n_pairs, 1, L, 1, 3).contiguous()
                                               if L > 1 else ref.view(n_pairs, 1, 1, 1, 3),
                                               torch.ones((n_pairs, 1, L, 1), dtype=feat.dtype, device=feat.device), item, bins)
        if self.deformable_attn and fused:
            # ONE projection of geo -- [uv | depth | logits], the rows of raw_projection -- and one launch from it to loc / attn
            from ..functions import LinearRowsFunction, SamplingLocationsFunction, train_weight_planes
            # (the 2-D classes' sampling_offsets_depth is a _ZeroLinear: zeros that are no parameter and take no gradient)
            w = torch.cat([da.sampling_offsets.weight, da.sampling_offsets_depth.weight, da.attention_weights.weight], 0)
            b = torch.cat([da.sampling_offsets.bias, da.sampling_offsets_depth.bias, da.attention_weights.bias], 0)
            if n_pairs >= 128:
                train_weight_planes().mark_ephemeral(w)
                proj = LinearRowsFunction.apply(geo, w, b)
            else:
                proj = F.linear(geo, w, b)
            normalizer = torch.stack([shapes3[..., 1], shapes3[..., 0], shapes3[..., 2]], -1).to(feat.dtype)   # (W, H, D) per level
            loc, attn = SamplingLocationsFunction.apply(ref, proj, normalizer, M, L, P)
            per_pair = PairListDeformAttnFunction.apply(value, dist.view(N, S, 1, -1), shapes3, level_start_index, loc, attn, item, bins)
            if self.geo_residual:
                per_pair = per_pair + geo
        elif self.deformable_attn:
            off_uv = linear_rows(da.sampling_offsets, geo).view(n_pairs, M, L, P, 2)
            off_d = (geo.new_zeros((n_pairs, M, L, P, 1)) if isinstance(da.sampling_offsets_depth, _ZeroLinear)
                     else linear_rows(da.sampling_offsets_depth, geo).view(n_pairs, M, L, P, 1))
            attn = linear_rows(da.attention_weights, geo).view(n_pairs, M, L * P).softmax(-1).view(n_pairs, M, L, P)
            normalizer = torch.stack([shapes3[..., 1], shapes3[..., 0], shapes3[..., 2]], -1).to(feat.dtype)   # (W, H, D) per level
            loc = ref.view(n_pairs, 1, 1, 1, 3) + torch.cat([off_uv, off_d], -1) / normalizer[None, None, :, None, :]
            per_pair = PairListDeformAttnFunction.apply(value, dist.view(N, S, 1, -1), shapes3, level_start_index, loc, attn, item, bins)
            if self.geo_residual:
                per_pair = per_pair + geo
        else:
            per_pair = geo
        if TRAIN_CONV == "hip" and C % 32 == 0:
            # inter-view aggregation on the pair list as well: no dense [N, L, C] slots (262 MB at config 2), K/V in-projected
            # for visible pairs only, the softmax over views and its backward on sgc_view_attend(_backward)
            from ..functions import LinearRowsFunction, ViewAttendFunction, linear_rows
            slot = pc["slot"]                        # (camera, voxel) -> pair row (in the binned order when binned), -1 = not visible
            if fused:
                from ..functions import ViewMeanFunction
                mean = ViewMeanFunction.apply(per_pair, slot, pc["valid_index"][:n_valid], n_valid)     # cameras added in camera order
                pooled = linear_rows(self.output_proj, mean)
            else:
                row_of = pc["row_of"].long()         # voxel -> compact row of `valid_index`, -1 = seen by no camera
                mean = torch.zeros((n_valid, C), dtype=per_pair.dtype, device=feat.device).index_add(0, row_of[q], per_pair)
                pooled = linear_rows(self.output_proj, mean / count[valid_index][:, None])
            if self.inter_view_aggregation == "attn":
                mha = self.attention_pooling
                w, b = mha.in_proj_weight, mha.in_proj_bias
                qv = LinearRowsFunction.apply(pooled, w[:C], b[:C])
                kv = LinearRowsFunction.apply(per_pair, w[C:], b[C:])                  # [n_pairs, 2C] = k | v
                ctx = ViewAttendFunction.apply(qv, kv, slot, pc["valid_index"][:n_valid], mha.num_heads)
                pooled = LinearRowsFunction.apply(ctx, mha.out_proj.weight, mha.out_proj.bias)
        else:
            slots = torch.zeros((N, Nq, C), dtype=feat.dtype, device=feat.device).index_put((cam, q), per_pair)
            valid_slots = slots[:, valid_index]                                # [N,L,C]
            valid_mask = mask.bool()[:, valid_index]                           # [N,L]
            pooled = (valid_slots * valid_mask[..., None]).sum(0) / count[valid_index][:, None]
            pooled = self.output_proj(pooled)
            if self.inter_view_aggregation == "attn":
                pooled, _ = self.attention_pooling(pooled[None], valid_slots, valid_slots, ~valid_mask.t())
                pooled = pooled[0]
        if fused:
            from ..functions import ScatterRowsFunction
            return self.dropout(ScatterRowsFunction.apply(pooled, pc["valid_index"][:n_valid], Nq).view(1, Nq, C)) + query
        out = torch.zeros((1, Nq, C), dtype=feat.dtype, device=feat.device)
        out = out.index_put((torch.zeros_like(valid_index), valid_index), pooled)
        return self.dropout(out) + query

    # ---- training: reference data layout, differentiable -----------------------------------
    def _forward_reference_layout(self, query, feat, dist, ref_cam, mask, spatial_shapes, level_start_index,
                                  **kwargs):
        C = self.embed_dims
        N, Nq = mask.shape
        counts = mask.sum(1)
        max_len = int(counts.max())
        order = torch.argsort((~mask).to(torch.uint8), dim=1, stable=True)[:, :max_len]     # visible q first, ascending
        live = torch.arange(max_len, device=mask.device)[None, :] < counts[:, None]          # [N,max_len]
        ref_rebatch = torch.gather(ref_cam, 1, order[..., None].expand(-1, -1, 3)) * live[..., None]
        ref_rebatch = ref_rebatch.view(N, max_len, 1, 3)
        shapes3 = self.deformable_attention.get_spatial_shape_3D(spatial_shapes, dist.shape[-1])
        ones = torch.ones((N, max_len, 1, 1, 1), dtype=feat.dtype, device=feat.device)
        geo, _ = MultiScale3DDeformableAttnFunction_fp32.apply(
            feat.view(N, -1, 1, C), dist.view(N, feat.shape[1], 1, -1), shapes3, level_start_index,
            ref_rebatch.view(N, max_len, 1, 1, 1, 3), ones, 128)
        if self.deformable_attn:
            two_d = isinstance(self.deformable_attention, MSDeformableAttention3D)
            queries = self.deformable_attention(query=geo, key=feat, value=feat, value_dpt_dist=dist,
                                                reference_points=ref_rebatch[..., :2] if two_d else ref_rebatch,
                                                spatial_shapes=spatial_shapes,
                                                level_start_index=level_start_index)
            queries = queries[0] if isinstance(queries, tuple) else queries
            if self.geo_residual:
                queries = queries + geo
        else:
            queries = geo
        slots = torch.zeros((N, Nq, C), dtype=feat.dtype, device=feat.device)
        cam_id = torch.arange(N, device=mask.device)[:, None].expand(-1, max_len)
        slots = slots.index_put((cam_id[live], order[live]), queries[live])
        count = mask.sum(0)
        valid_index = count.nonzero()[:, 0]
        valid_slots = slots[:, valid_index]                                # [N,L,C]
        valid_mask = mask[:, valid_index]                                  # [N,L]
        pooled = (valid_slots * valid_mask[..., None]).sum(0) / count[valid_index][:, None]
        pooled = self.output_proj(pooled)
        if self.inter_view_aggregation == "attn":
            pooled, _ = self.attention_pooling(pooled[None], valid_slots, valid_slots, ~valid_mask.t())
            pooled = pooled[0]
        out = torch.zeros((1, Nq, C), dtype=feat.dtype, device=feat.device)
        out = out.index_put((torch.zeros_like(valid_index), valid_index), pooled)
        return self.dropout(out) + query

    def _depth_inputs(self, value_dpt_dist, reference_points_cam, N, S, Nq, feat):
        return value_dpt_dist.reshape(N, S, -1), reference_points_cam.reshape(N, Nq, 3)

    def forward(self, query, key, value, residual=None, query_pos=None, key_padding_mask=None,
                reference_points=None, spatial_shapes=None, reference_points_cam=None, bev_mask=None,
                level_start_index=None, value_dpt_dist=None, flag="encoder", **kwargs):
        """query [1,Nq,C]; value [N,S,1,C]; value_dpt_dist [N,S,1,D];
        reference_points_cam [N,1,Nq,1,3]; bev_mask [N,1,Nq,1] -> [1,Nq,C]."""
        if value is None:
            value = key
        if query_pos is not None:
            query = query + query_pos
        bs, Nq, C = query.shape
        assert bs == 1
        N, S = value.shape[0], value.shape[1]
        feat = value.reshape(N, S, C)
        dist, ref_cam = self._depth_inputs(value_dpt_dist, reference_points_cam, N, S, Nq, feat)
        if torch.is_grad_enabled() and (query.requires_grad or feat.requires_grad or dist.requires_grad
                                        or any(p.requires_grad for p in self.parameters())):
            if self.train_pair_list:
                return self._forward_pairs_train(query, feat, dist, ref_cam, bev_mask.reshape(N, Nq), spatial_shapes, level_start_index,
                                                 spatial_hw=kwargs.get("spatial_hw"))
            return self._forward_reference_layout(query, feat, dist, ref_cam, bev_mask.reshape(N, Nq).bool(), spatial_shapes,
                                                  level_start_index)
        if spatial_shapes.shape[0] != 1:
            raise NotImplementedError("pair-list path supports one feature level per call (all SGCDet configs)")
        hw = kwargs.get("spatial_hw")
        if hw is None:
            hw = tuple(int(v) for v in spatial_shapes[0].tolist())
        mask_u8 = bev_mask.reshape(N, Nq)
        mask_u8 = mask_u8 if mask_u8.dtype == torch.uint8 else mask_u8.to(torch.uint8)
        return self._forward_pairs(query, feat.contiguous(), dist.contiguous(), ref_cam.contiguous(),
                                   mask_u8.contiguous(), hw[0], hw[1], zero_query=bool(kwargs.get("zero_query")),
                                   static_counts=bool(kwargs.get("static_counts")), want_ctx=bool(kwargs.get("want_ctx")))


@ATTENTION.register_module()
class DeformCrossAttention(DeformCrossAttention_DFA3D):
    """The 2-D cross attention (deformable_cross_attention.py:504-689; no SGCDet config selects it): bilinear sample of the
    feature map at the projected voxel centre, 2-D deformable attention around it PLUS that sample (:647), then the same
    mean / attention over views.  Runs the DFA3D pipeline on a one-bin unit depth map (see ``MSDeformableAttention3D``);
    the tiled gather needs two depth bins, so the per-wave gather serves this class."""
    geo_residual = True

    def _depth_inputs(self, value_dpt_dist, reference_points_cam, N, S, Nq, feat):
        ref = reference_points_cam.reshape(N, Nq, -1)
        if ref.shape[-1] == 2:
            ref = torch.cat([ref, ref.new_full((N, Nq, 1), 0.5)], -1)
        else:                                              # 3-D points from the shared projection kernel: depth is not used
            ref = ref.clone()
            ref[..., 2] = 0.5
        ones = self.__dict__.get("_unit_depth")
        if ones is None or ones.shape != (N, S, 1) or ones.device != feat.device or ones.dtype != feat.dtype:
            ones = self.__dict__["_unit_depth"] = feat.new_ones((N, S, 1))
        return ones, ref


# ----------------------------------------------------------------------------------------
@TRANSFORMER_LAYER.register_module()
class MyCustomBaseTransformerLayer(BaseModule):
    """attention / norm / ffn stack; parameter names ``attentions.i``, ``ffns.i``, ``norms.i``."""

    def __init__(self, attn_cfgs=None, ffn_cfgs=None, operation_order=None, norm_cfg=dict(type="LN"),
                 init_cfg=None, batch_first=True, **kwargs):
        super().__init__(init_cfg)
        if ffn_cfgs is None:
            ffn_cfgs = dict(type="FFN", embed_dims=256, feedforward_channels=1024, num_fcs=2, ffn_drop=0.0,
                            act_cfg=dict(type="ReLU", inplace=True))
        ffn_cfgs = copy.deepcopy(ffn_cfgs)
        for old, new in (("feedforward_channels", "feedforward_channels"), ("ffn_dropout", "ffn_drop"),
                         ("ffn_num_fcs", "num_fcs")):
            if old in kwargs:
                ffn_cfgs[new] = kwargs[old]
        self.batch_first = batch_first
        allowed = {"self_attn", "norm", "ffn", "cross_attn"}
        assert set(operation_order) <= allowed, f"operation_order must be a subset of {sorted(allowed)}"
        num_attn = operation_order.count("self_attn") + operation_order.count("cross_attn")
        if isinstance(attn_cfgs, dict):
            attn_cfgs = [copy.deepcopy(attn_cfgs) for _ in range(num_attn)]
        else:
            attn_cfgs = [copy.deepcopy(c) for c in attn_cfgs]
            assert num_attn == len(attn_cfgs)
        self.num_attn = num_attn
        self.operation_order = tuple(operation_order)
        self.norm_cfg = norm_cfg
        self.pre_norm = operation_order[0] == "norm"
        self.attentions = ModuleList()
        i = 0
        for name in operation_order:
            if name in ("self_attn", "cross_attn"):
                cfg = dict(attn_cfgs[i])
                if "batch_first" in cfg:
                    assert self.batch_first == cfg["batch_first"]
                else:
                    cfg["batch_first"] = self.batch_first
                att = build_attention(cfg)
                att.operation_name = name
                self.attentions.append(att)
                i += 1
        self.embed_dims = self.attentions[0].embed_dims
        self.ffns = ModuleList()
        num_ffns = operation_order.count("ffn")
        if isinstance(ffn_cfgs, dict):
            ffn_cfgs = [copy.deepcopy(ffn_cfgs) for _ in range(num_ffns)]
        assert len(ffn_cfgs) == num_ffns
        for cfg in ffn_cfgs:
            cfg = dict(cfg)
            cfg.setdefault("embed_dims", self.embed_dims)
            assert cfg["embed_dims"] == self.embed_dims
            self.ffns.append(build_feedforward_network(cfg))
        self.norms = ModuleList()
        for _ in range(operation_order.count("norm")):
            self.norms.append(build_norm_layer(norm_cfg, self.embed_dims)[1])


@TRANSFORMER_LAYER.register_module()
class VoxFormerLayer(MyCustomBaseTransformerLayer):
    def __init__(self, attn_cfgs, operation_order=None, act_cfg=dict(type="ReLU", inplace=True),
                 norm_cfg=dict(type="LN"), **kwargs):
        super().__init__(attn_cfgs=attn_cfgs, operation_order=operation_order, norm_cfg=norm_cfg, **kwargs)
        self.fp16_enabled = False

    # inference: ("cross_attn", "norm", "ffn", "norm") -- every SGCDet config -- with the attention's out projection, the
    # slot scatter, both LayerNorms and the FFN in ONE launch (sgc_level_tail; bit-identical to the six launches it replaces)
    fuse_tail = True

    def _fused_tail(self, query, key, value, query_pos, key_pos, ref_3d, reference_points_cam, mask, key_padding_mask,
                    spatial_shapes, level_start_index, kwargs):
        from .conv_plan import CONV_MODE
        # (module in training mode under no_grad: the six-launch path applies the attention / FFN dropouts, this one cannot)
        if (not self.fuse_tail or torch.is_grad_enabled() or self.training or self.operation_order != ("cross_attn", "norm", "ffn", "norm")
                or self.pre_norm or not kwargs.get("zero_query") or CONV_MODE != "bf16x3" or not query.is_cuda
                or query_pos is not None):
            return None
        att, ffn, n1, n2 = self.attentions[0], self.ffns[0], self.norms[0], self.norms[1]
        C = self.embed_dims
        if not (isinstance(att, DeformCrossAttention_DFA3D) and att.deformable_attn and att.inter_view_aggregation == "attn"
                and C % 32 == 0 and isinstance(n1, nn.LayerNorm) and isinstance(n2, nn.LayerNorm)
                and n1.elementwise_affine and n2.elementwise_affine and tuple(n1.normalized_shape) == (C,)
                and tuple(n2.normalized_shape) == (C,) and ffn.num_fcs == 2 and ffn.add_identity and len(ffn.layers) == 3
                and isinstance(ffn.layers[0][1], nn.ReLU) and ffn.embed_dims == C
                and _ops().level_tail_supported(C, ffn.feedforward_channels)):
            return None
        got = att(query, key, value, None, query_pos=None, key_pos=key_pos, reference_points=ref_3d,
                  reference_points_cam=reference_points_cam, mask=mask, key_padding_mask=key_padding_mask,
                  spatial_shapes=spatial_shapes, level_start_index=level_start_index, want_ctx=True, **kwargs)
        if not isinstance(got, tuple):                  # the attention took a path without the shortcut: finish unfused
            x = _layer_norm(n1, got)
            return _layer_norm(n2, _ffn_forward(ffn, x, None))
        ctx, row_of = got
        ops = _ops()

        def build():                                            # weights split to bf16 hi / lo and fragment-packed once
            def packed(weight):
                hi, lo = ops.split_operand(weight.detach().float())
                return ops.pack_b_fragments(hi), ops.pack_b_fragments(lo)
            mha = att.attention_pooling
            lin1, lin2 = ffn.layers[0][0], ffn.layers[1]
            zeros = lambda n: torch.zeros(n, dtype=torch.float32, device=ctx.device)      # noqa: E731
            bias = lambda lin, n: lin.bias.detach().float().contiguous() if lin.bias is not None else zeros(n)   # noqa: E731
            return (packed(mha.out_proj.weight), bias(mha.out_proj, C), packed(lin1.weight), bias(lin1, lin1.out_features),
                    packed(lin2.weight), bias(lin2, C))
        wo, bo, w1, b1, w2, b2 = cached_plan(self, build, "_tail_plan", (module_fingerprint(att), module_fingerprint(ffn)))
        y = ops.level_tail(ctx, row_of, wo, bo, (n1.weight, n1.bias, n1.eps), w1, b1, w2, b2, (n2.weight, n2.bias, n2.eps))
        return y.view(1, -1, C)

    def forward(self, query, key=None, value=None, bev_pos=None, query_pos=None, key_pos=None, attn_masks=None,
                query_key_padding_mask=None, key_padding_mask=None, ref_2d=None, ref_3d=None,
                reference_points_cam=None, mask=None, spatial_shapes=None, level_start_index=None,
                prev_bev=None, **kwargs):
        """encoder.py:262-340: walk ``operation_order``; post-norm layers pass no residual."""
        fused = self._fused_tail(query, key, value, query_pos, key_pos, ref_3d, reference_points_cam, mask, key_padding_mask,
                                 spatial_shapes, level_start_index, kwargs)
        if fused is not None:
            return fused
        norm_i = attn_i = ffn_i = 0
        identity = query
        for op in self.operation_order:
            if op == "norm":
                query = _layer_norm(self.norms[norm_i], query)
                norm_i += 1
            elif op == "cross_attn":
                query = self.attentions[attn_i](
                    query, key, value, identity if self.pre_norm else None, query_pos=query_pos,
                    key_pos=key_pos, reference_points=ref_3d, reference_points_cam=reference_points_cam,
                    mask=mask, key_padding_mask=key_padding_mask, spatial_shapes=spatial_shapes,
                    level_start_index=level_start_index, **kwargs)
                attn_i += 1
                identity = query
            elif op == "ffn":
                query = _ffn_forward(self.ffns[ffn_i], query, identity if self.pre_norm else None)
                ffn_i += 1
            else:
                raise NotImplementedError(f"{op} is not used by any SGCDet config")
        return query


# ----------------------------------------------------------------------------------------
def compute_projection(img_meta, stride=1):
    """``K' @ E_i[:3]`` for every camera, on the host, [N,3,4] fp32.

    The reference loops over cameras (``intrinsic @ extrinsic[:3]``, encoder.py:168-177,
    detectors/utils.py:16-24: N tensor constructions + N tiny matmuls, 0.6 ms at 40 views).  Here all
    cameras go through ONE torch mm, ``K' [3,3] @ [3, 4N]``: every output element is the same
    3-term dot product, and the result is bit-identical to the loop (checked against
    ``compute_projection_loop`` in tests/test_host_logic.py on the host the tests run on)."""
    import numpy as np
    intrinsic = torch.tensor(img_meta["lidar2img"]["intrinsic"][:3, :3])
    ratio = img_meta["ori_shape"][0] / (img_meta["img_shape"][0] / stride)
    intrinsic[:2] /= ratio
    ext_ = torch.from_numpy(np.stack([np.asarray(e, dtype=np.float32) for e in img_meta["lidar2img"]["extrinsic"]]))
    n = ext_.shape[0]
    cols = ext_[:, :3].permute(1, 0, 2).reshape(3, n * 4)
    # single-threaded on purpose: a [3,3]x[3,4N] product must not wake a 256-thread OpenMP pool
    # (measured: ~50 ms per call on the GPU host when BLAS decides to go parallel)
    nt = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        out = intrinsic @ cols
    finally:
        torch.set_num_threads(nt)
    return out.reshape(3, n, 4).permute(1, 0, 2).contiguous()


def compute_projection_loop(img_meta, stride=1):
    """The reference's formulation, kept as the checker of ``compute_projection``."""
    intrinsic = torch.tensor(img_meta["lidar2img"]["intrinsic"][:3, :3])
    ratio = img_meta["ori_shape"][0] / (img_meta["img_shape"][0] / stride)
    intrinsic[:2] /= ratio
    return torch.stack([intrinsic @ torch.tensor(e)[:3] for e in img_meta["lidar2img"]["extrinsic"]])


def scene_constants_host(img_meta):
    """CPU fp32 [N*12 + 3]: the N projection matrices (3x4, row-major) followed by the scene origin -- everything
    the path needs from ``img_meta`` on the device (encoder.py:168-177,187,194 of the reference)."""
    proj = compute_projection(img_meta, stride=1).float()
    return torch.cat([proj.reshape(-1), torch.as_tensor(img_meta["lidar2img"]["origin"], dtype=torch.float32)])


def _layer_norm(norm, x):
    """nn.LayerNorm over the channel rows of a level; inference on the GPU: one launch of ``sgc_layer_norm_rows`` (one wave
    per row) instead of the library kernel -- every kernel of a scene graph then comes from this library."""
    if (isinstance(norm, nn.LayerNorm) and not torch.is_grad_enabled() and x.is_cuda and x.dtype == torch.float32
            and norm.elementwise_affine and len(norm.normalized_shape) == 1 and x.is_contiguous()):
        C = norm.normalized_shape[0]
        return _ops().layer_norm_rows(x.view(-1, C), norm.weight, norm.bias, norm.eps).view(x.shape)
    if (isinstance(norm, nn.LayerNorm) and norm.elementwise_affine and len(norm.normalized_shape) == 1 and x.is_contiguous()
            and _level_fused(x)):
        from ..functions import LayerNormRowsFunction
        C = norm.normalized_shape[0]
        return LayerNormRowsFunction.apply(x.view(-1, C), norm.weight, norm.bias, norm.eps).view(x.shape)
    return norm(x)


def _ffn_forward(ffn, x, identity=None):
    """mmcv ``FFN`` (Linear - ReLU - Linear + identity) of a transformer layer.  Inference on the GPU in the bf16x3
    conv mode: two launches of the MFMA kernel with ReLU and the residual add in their epilogues instead of two
    library GEMMs and two elementwise kernels; anything else goes through the module."""
    from .conv_plan import CONV_MODE
    lin1 = ffn.layers[0][0] if len(ffn.layers) == 3 else None
    fast = (not torch.is_grad_enabled() and x.is_cuda and CONV_MODE == "bf16x3" and ffn.num_fcs == 2 and ffn.add_identity
            and lin1 is not None and isinstance(ffn.layers[0][1], nn.ReLU) and x.dtype == torch.float32
            and ffn.embed_dims % 32 == 0 and ffn.feedforward_channels % 32 == 0)
    if not fast:
        from .conv_plan import TRAIN_CONV
        if (torch.is_grad_enabled() and TRAIN_CONV == "hip" and x.is_cuda and x.dtype == torch.float32 and lin1 is not None
                and ffn.num_fcs == 2 and ffn.embed_dims % 32 == 0 and ffn.feedforward_channels % 32 == 0):
            # training: the two Linears (forward, input and weight gradients) on the MFMA kernels, the rest as the module does
            from ..functions import linear_rows
            out = linear_rows(lin1, x)
            for m in list(ffn.layers[0])[1:]:
                out = m(out)                              # activation, dropout
            out = ffn.layers[2](linear_rows(ffn.layers[1], out))
            if not ffn.add_identity:
                return ffn.dropout_layer(out)
            return (x if identity is None else identity) + ffn.dropout_layer(out)
        return ffn(x, identity)
    lin2 = ffn.layers[1]
    s1, s2 = cached_plan(ffn, lambda: (LinearSpec(lin1.weight, lin1.bias), LinearSpec(lin2.weight, lin2.bias)), "_sgc_plan")
    ops = _ops()
    rows = x.reshape(-1, ffn.embed_dims).contiguous()
    idn = rows if identity is None else identity.reshape(-1, ffn.embed_dims).contiguous()
    M = rows.shape[0]
    h, _ = ops.conv3d_cl_bf16x3(rows, s1.w_hi, s1.w_lo, (M, 1, 1), 1, 1, False, None, s1.shift, None, 2)    # relu(t)
    y, _ = ops.conv3d_cl_bf16x3(h, s2.w_hi, s2.w_lo, (M, 1, 1), 1, 1, False, None, s2.shift, idn, 0)          # t + identity
    return y.view(x.shape)


@TRANSFORMER_LAYER_SEQUENCE.register_module()
class VoxFormerEncoder_DFA3D(TransformerLayerSequence):
    def __init__(self, *args, return_intermediate=False, dbound=None, **kwargs):
        super().__init__(*args, **kwargs)
        self.return_intermediate = return_intermediate
        self.dbound = dbound
        self.fp16_enabled = False
        self._scene_cache = None

    _compute_projection = staticmethod(compute_projection)

    def _scene_constants(self, img_meta, device):
        """(proj [N,3,4], origin [3]) on the device, composed once per scene (img_meta object)."""
        pre = img_meta.get("_sgc_scene_const")
        if pre is not None:          # device-resident [N*12 + 3] (see scene_constants_host): the static-graph input
            n = (pre.numel() - 3) // 12
            return pre[: n * 12].view(n, 3, 4), pre[n * 12:]
        c = self._scene_cache
        if c is not None and c[0] is img_meta and c[1] == device:
            return c[2], c[3]
        # one staging tensor -> one host->device copy for (proj, origin); (a fresh pinned buffer per scene
        # costs a ~50 ms hipHostMalloc -- measured -- so the small pageable copy is the cheaper choice)
        stage = scene_constants_host(img_meta)
        n = (stage.numel() - 3) // 12
        dev = stage.to(device)
        proj, origin = dev[: n * 12].view(n, 3, 4), dev[n * 12:]
        self._scene_cache = (img_meta, device, proj, origin)
        return proj, origin

    def project(self, ref3d, img_meta, sel=None):
        """ref3d [Nq,3] (or all voxels' [Nvox,3] with ``sel`` [Nq] int64 picking the queries) ->
        (ref_cam [N,Nq,3] fp32, mask [N,Nq] uint8) with one HIP launch."""
        proj, origin = self._scene_constants(img_meta, ref3d.device)
        return _ops().project_points(ref3d.contiguous(), origin, proj, img_meta["img_shape"][1],
                                     img_meta["img_shape"][0], self.dbound[0], self.dbound[1], sel=sel)

    def point_sampling(self, reference_points, img_meta=None):
        """Reference signature (encoder.py:179-223): [1,1,Nq,3] ->
        (reference_points_cam [N,1,Nq,1,3], bev_mask [N,1,Nq,1] bool)."""
        assert reference_points.shape[0] == 1
        ref_cam, mask = self.project(reference_points.reshape(-1, 3).float(), img_meta)
        N, Nq = mask.shape
        return ref_cam.view(N, 1, Nq, 1, 3), mask.view(N, 1, Nq, 1).bool()

    def forward(self, bev_query, key, value, *args, ref_3d=None, bev_pos=None, spatial_shapes=None,
                level_start_index=None, img_meta=None, prev_bev=None, **kwargs):
        """bev_query [Nq,1,C]; key/value [N,S,1,C] -> [1,Nq,C]."""
        ref_cam, mask = self.project(ref_3d.reshape(-1, 3).float(), img_meta, sel=kwargs.pop("ref_sel", None))
        N, Nq = mask.shape
        bev_query = bev_query.permute(1, 0, 2)
        if bev_pos is not None:
            bev_pos = bev_pos.permute(1, 0, 2)
        intermediate = []
        output = bev_query
        for layer in self.layers:
            output = layer(bev_query, key, value, *args, bev_pos=bev_pos, ref_3d=ref_3d,
                           spatial_shapes=spatial_shapes, level_start_index=level_start_index,
                           reference_points_cam=ref_cam.view(N, 1, Nq, 1, 3), bev_mask=mask.view(N, 1, Nq, 1),
                           prev_bev=prev_bev, img_meta=img_meta, **kwargs)
            bev_query = output
            if self.return_intermediate:
                intermediate.append(output)
        return torch.stack(intermediate) if self.return_intermediate else output


@TRANSFORMER_LAYER_SEQUENCE.register_module()
class VoxFormerEncoder(VoxFormerEncoder_DFA3D):
    """The 2-D encoder (encoder.py:18-155; no SGCDet config selects it): same projection and visibility mask, the
    reference points keep only (u, v) (:99)."""

    def point_sampling(self, reference_points, img_meta=None):
        ref_cam, mask = super().point_sampling(reference_points, img_meta)
        return ref_cam[..., 0:2], mask

    def forward(self, bev_query, key, value, *args, **kwargs):
        kwargs.pop("value_dpt_dist", None)
        return super().forward(bev_query, key, value, *args, **kwargs)


def _channels_last_rows(t4, h, w):
    """[N, C, h, w] top-rows crop of a map stored channels-last ([N, Hs, Ws, C] in memory, Ws == w) -> zero-copy
    [N, Hs*Ws, C] rows (the kernels take Hs*Ws as the camera stride and never address the cropped rows); None when
    the memory layout is anything else."""
    N, C, hh, ww = t4.shape
    st = t4.stride()
    if hh != h or ww != w or st[1] != 1 or st[3] != C or st[2] != w * C or st[0] % (w * C) or st[0] < h * w * C:
        return None
    return torch.as_strided(t4, (N, st[0] // C, C), (st[0], C, 1))


@TRANSFORMER.register_module()
class PerceptionTransformer_DFA3D(BaseModule):
    def __init__(self, encoder=None, embed_dims=256, **kwargs):
        super().__init__(kwargs.get("init_cfg"))
        self.encoder = build_transformer_layer_sequence(encoder)
        self.embed_dims = embed_dims
        self.fp16_enabled = False

    def init_weights(self):
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)
        for m in self.modules():
            if isinstance(m, (MSDeformableAttention3D_DFA3D, DeformCrossAttention_DFA3D)):
                (m.init_weight if hasattr(m, "init_weight") else m.init_weights)()

    def _shape_tensors(self, shapes, device):
        """(spatial_shapes [L,2] int64, level_start_index [L] int64) on the device, cached: building them
        per call costs a blocking host->device copy (0.8 ms measured) three times per scene."""
        cache = self.__dict__.setdefault("_shape_cache", {})
        key = (shapes, str(device))
        if key not in cache:
            ss = torch.as_tensor(shapes, dtype=torch.long)
            lsi = torch.cat((ss.new_zeros((1,)), ss.prod(1).cumsum(0)[:-1]))
            cache[key] = (ss.to(device), lsi.to(device))
        return cache[key]

    def _coords_are_flat(self, vox_coords):
        """vox_coords[:, 3] == arange: declared by the producer (DenseHead tags the buffer it builds, ``_sgc_flat``); an
        untagged tensor is checked on the host ONCE PER TENSOR OBJECT (the verdict is stored on the tensor itself, so a
        different tensor that later reuses the address can never inherit it) -- and never during a graph capture, where
        the read-back would be illegal."""
        flat = getattr(vox_coords, "_sgc_flat", None)
        if flat is not None and flat[0] == vox_coords._version:
            return flat[1]
        if vox_coords.is_cuda and torch.cuda.is_current_stream_capturing():
            return False                                   # the general (gather) path is always correct
        ok = bool(torch.equal(vox_coords[:, 3].cpu(), torch.arange(vox_coords.shape[0])))
        vox_coords._sgc_flat = (vox_coords._version, ok)
        return ok

    def get_vox_features(self, mlvl_feats, bev_queries, ref_3d, vox_coords, unmasked_idx, bev_pos=None,
                         prev_bev=None, img_meta=None, mlvl_dpt_dists=None, **kwargs):
        """transformer.py:118-185.  mlvl_feats: list of [1,N,C,H,W] (possibly crop views);
        mlvl_dpt_dists: list of [1,N,D,H,W]; returns [1,Nq,C]."""
        assert mlvl_feats[0].size(0) == 1
        ops = _ops()
        ref_sel = None
        if bev_queries is None and not torch.is_grad_enabled() and ref_3d.is_cuda and self._coords_are_flat(vox_coords):
            # inference: vox_coords[:, 3] is the flat voxel index itself (DenseHead.py:32-48), so the reference's two
            # gathers (flat = vox_coords[idx, 3]; ref_3d[flat], transformer.py:145-146) collapse into the projection
            # kernel reading ref_3d[idx[q]] -- no index kernels
            n_q = unmasked_idx.shape[0]
            zero = self.__dict__.get("_zero_scalar")
            if zero is None or zero.device != mlvl_feats[0].device:
                zero = self.__dict__["_zero_scalar"] = torch.zeros(1, device=mlvl_feats[0].device)
            queries = zero.expand(n_q, 1, self.embed_dims)            # content-free (DenseHead.py:63): shape only, no fill
            kwargs["zero_query"] = True
            sel_ref, ref_sel, flat_idx = ref_3d, unmasked_idx, unmasked_idx
        else:
            flat_idx = vox_coords[unmasked_idx, 3]
            if bev_queries is None:   # the reference's queries are all-zero (DenseHead.py:63): skip the gather
                queries = torch.zeros((flat_idx.shape[0], 1, self.embed_dims), device=mlvl_feats[0].device)
                kwargs["zero_query"] = True
            else:
                queries = bev_queries[flat_idx].unsqueeze(1)                  # [Nq,1,C]
            sel_ref = ref_3d[flat_idx].to(queries.device)                     # [Nq,3]
        feats, dists, shapes = [], [], []
        for feat, dpt in zip(mlvl_feats, mlvl_dpt_dists if mlvl_dpt_dists is not None else [None] * len(mlvl_feats)):
            _, n_cam, c, h, w = feat.shape
            shapes.append((h, w))
            if dpt is None:                                 # the 2-D transformer: no depth maps travel
                if torch.is_grad_enabled() and feat.requires_grad:
                    feats.append(feat[0].flatten(2).permute(0, 2, 1))
                else:
                    f_rows = _channels_last_rows(feat[0], h, w) if feat.dtype == torch.float32 else None
                    feats.append(f_rows if f_rows is not None else ops.nchw_to_nhwc_crop(feat[0].float(), h, w))
            elif torch.is_grad_enabled() and (feat.requires_grad or dpt.requires_grad):
                if feat.is_cuda and feat.dtype == torch.float32 and dpt.dtype == torch.float32:
                    # training: the transposes of both directions on the HIP kernels (functions.NchwToRowsFunction)
                    from ..functions import NchwToRowsFunction
                    feats.append(NchwToRowsFunction.apply(feat[0]))
                    dists.append(NchwToRowsFunction.apply(dpt[0]))
                else:
                    feats.append(feat[0].flatten(2).permute(0, 2, 1))
                    dists.append(dpt[0].flatten(2).permute(0, 2, 1))
            else:   # channels-last producers: no copy; otherwise one crop+transpose launch each
                f_rows = _channels_last_rows(feat[0], h, w) if feat.dtype == torch.float32 else None
                d_rows = _channels_last_rows(dpt[0], h, w) if dpt.dtype == torch.float32 else None
                if f_rows is not None and (d_rows is None or f_rows.shape[1] != d_rows.shape[1]):
                    # channels-last feature maps (the FPN of plugin/fpn.py) next to an NCHW depth map: only the small depth
                    # map is transposed, into rows with the feature map's camera stride (the cropped rows are never read)
                    d = ops.nchw_to_nhwc_crop(dpt[0].float(), h, w)
                    if f_rows.shape[1] == h * w:
                        d_rows = d
                    else:
                        d_rows = d.new_empty((n_cam, f_rows.shape[1], d.shape[2]))
                        d_rows[:, :h * w] = d
                elif f_rows is None or d_rows is None:
                    f_rows = ops.nchw_to_nhwc_crop(feat[0].float(), h, w)
                    d_rows = ops.nchw_to_nhwc_crop(dpt[0].float(), h, w)
                feats.append(f_rows)
                dists.append(d_rows)
        feat_flatten = feats[0] if len(feats) == 1 else torch.cat(feats, 1)
        dist_flatten = None if not dists else (dists[0] if len(dists) == 1 else torch.cat(dists, 1))
        spatial_shapes, level_start_index = self._shape_tensors(tuple(shapes), queries.device)
        pos = None
        if bev_pos is not None:
            pos = bev_pos.flatten(2).permute(2, 0, 1)[flat_idx]
        return self.encoder(queries, feat_flatten.unsqueeze(2), feat_flatten.unsqueeze(2),
                            value_dpt_dist=None if dist_flatten is None else dist_flatten.unsqueeze(2), ref_3d=sel_ref[None, None],
                            bev_pos=pos, spatial_shapes=spatial_shapes, level_start_index=level_start_index,
                            img_meta=img_meta, prev_bev=None, spatial_hw=shapes[0] if len(shapes) == 1 else None,
                            ref_sel=ref_sel, **kwargs)


@TRANSFORMER.register_module()
class PerceptionTransformer(PerceptionTransformer_DFA3D):
    """The 2-D transformer (transformer.py:26-112; no SGCDet config selects it): ``get_vox_features`` without depth maps.
    ``bev_queries`` may still be None (zero queries, as the heads of this build pass them)."""

    def get_vox_features(self, mlvl_feats, bev_queries, ref_3d, vox_coords, unmasked_idx, bev_pos=None,
                         prev_bev=None, img_meta=None, **kwargs):
        kwargs.pop("mlvl_dpt_dists", None)
        return super().get_vox_features(mlvl_feats, bev_queries, ref_3d, vox_coords, unmasked_idx, bev_pos=bev_pos,
                                        prev_bev=prev_bev, img_meta=img_meta, mlvl_dpt_dists=None, **kwargs)
