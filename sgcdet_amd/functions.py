"""Autograd Functions with the reference's names and argument order.

Reference classes mirrored (mmdet3d_plugin/models/im2voxel/transformer_utils/
multi_scale_3ddeformable_attn_function.py and the DFA3D package twin
dfa3D/ops/multi_scale_3D_deform_attn.py):

* ``MultiScale3DDeformableAttnFunction_fp32`` (:275-351)  -- returns ``(output, depth_score)``;
* ``MultiScaleDepthScoreSampleFunction_fp32`` (:228-273)
* ``WeightedMultiScaleDeformableAttnFunction_fp32`` (:102-178)

Differences, all behind the same call signature:

* the one-stage Function runs ONE fused HIP kernel forward and ONE backward (no
  ``[B,Q,M,L,P,4]`` round trip, no ``[..., :2].contiguous()`` slice copies);
* ``value_dpt_dist`` may be passed un-replicated (``[B,S,1,D]``) -- the reference's
  ``.repeat(1,1,num_heads,1)`` (TU/deformable_cross_attention.py:422) is not needed, and the
  returned gradient then already holds the sum over heads;
* no host sync in backward: the reference's ``grad_depth_score_.sum() != 0.0`` check
  (:314) is replaced by ``ctx.mark_non_differentiable`` on the returned depth score;
* the ``_fp16`` twins of the reference cannot run (its kernels have no half dispatch,
  SURVEY.md section 0 fact 2); they are aliases of the fp32 Functions here, which is what
  ``custom_fwd(cast_inputs=torch.float32)`` amounts to.
"""
import os

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import ext


class MultiScale3DDeformableAttnFunction_fp32(Function):
    @staticmethod
    def forward(ctx, value, value_dpt_dist, value_spatial_shapes, value_level_start_index,
                sampling_locations, attention_weights, im2col_step=64):
        value = value.float().contiguous()
        value_dpt_dist = value_dpt_dist.float().contiguous()
        sampling_locations = sampling_locations.float().contiguous()
        attention_weights = attention_weights.float().contiguous()
        output, depth_score = ext.ops().dfa3d_forward(
            value, value_dpt_dist, value_spatial_shapes, value_level_start_index,
            sampling_locations, attention_weights, want_score=True)
        ctx.save_for_backward(value, value_dpt_dist, value_spatial_shapes, value_level_start_index,
                              sampling_locations, attention_weights)
        ctx.mark_non_differentiable(depth_score)
        return output, depth_score

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output, grad_depth_score_=None):
        value, dist, shapes3, lsi, loc, attn = ctx.saved_tensors
        gv, gd, gl, ga = ext.ops().dfa3d_backward(value, dist, shapes3, lsi, loc, attn,
                                                  grad_output.float().contiguous())
        return gv, gd, None, None, gl, ga, None


class MultiScaleDepthScoreSampleFunction_fp32(Function):
    @staticmethod
    def forward(ctx, value, value_spatial_shapes, value_level_start_index, sampling_locations,
                im2col_step=64):
        value = value.float().contiguous()
        sampling_locations = sampling_locations.float().contiguous()
        out = ext.ms_depth_score_sample_forward(value, value_spatial_shapes, value_level_start_index,
                                                sampling_locations, im2col_step=im2col_step)
        ctx.save_for_backward(value, value_spatial_shapes, value_level_start_index, sampling_locations)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        value, shapes3, lsi, loc = ctx.saved_tensors
        grad_value = torch.zeros_like(value)
        grad_loc = torch.zeros_like(loc)
        ext.ms_depth_score_sample_backward(value, shapes3, lsi, loc, grad_output.float().contiguous(),
                                           grad_value, grad_loc)
        return grad_value, None, None, grad_loc, None


class WeightedMultiScaleDeformableAttnFunction_fp32(Function):
    @staticmethod
    def forward(ctx, value, value_spatial_shapes, value_level_start_index, sampling_locations,
                attention_weights, depth_score, im2col_step=64):
        value = value.float().contiguous()
        sampling_locations = sampling_locations.float().contiguous()
        attention_weights = attention_weights.float().contiguous()
        depth_score = depth_score.float().contiguous()
        out = ext.wms_deform_attn_forward(value, value_spatial_shapes, value_level_start_index,
                                          sampling_locations, attention_weights, depth_score,
                                          im2col_step=im2col_step)
        ctx.save_for_backward(value, value_spatial_shapes, value_level_start_index, sampling_locations,
                              attention_weights, depth_score)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        value, shapes2, lsi, loc2, attn, score = ctx.saved_tensors
        grad_value = torch.zeros_like(value)
        grad_loc = torch.zeros_like(loc2)
        grad_attn = torch.zeros_like(attn)
        grad_score = torch.zeros_like(score)
        ext.wms_deform_attn_backward(value, shapes2, lsi, loc2, attn, score,
                                     grad_output.float().contiguous(), grad_value, grad_loc,
                                     grad_attn, grad_score)
        return grad_value, None, None, grad_loc, grad_attn, grad_score, None


TRAIN_BWD_TILED_SHARED = os.environ.get("SGC_TRAIN_BWD_SHARED", "0") == "1"     # the one-head geometry sample on the tiled backward too (A/B)


class PairListDeformAttnFunction(Function):
    """The fused DFA3D operator over an ITEM LIST: item i = (camera ``item_batch[i]``, its sampling locations / weights).
    Training-path counterpart of ``MultiScale3DDeformableAttnFunction_fp32`` without the reference's padded
    [N, max_len] rebatch (TU/deformable_cross_attention.py:759-773): only visible (camera, voxel) pairs are sampled and
    back-propagated.  value [B,S,M,Cm], dist [B,S,1|M,D], loc3 [n,M,L,P,3], attn [n,M,L,P] -> [n, M*Cm]."""

    @staticmethod
    def forward(ctx, value, value_dpt_dist, value_spatial_shapes, value_level_start_index, sampling_locations,
                attention_weights, item_batch, bins=None):
        """``bins`` (one level only): (bin_offset, H, W, bin_w, bin_h, halo) when the items are in the (camera, bin) order of
        ``sgc_bin_pairs`` -- the backward then takes the LDS-tiled kernel (``sgc_dfa3d_backward_binned``) instead of the item kernel's
        global atomics.  The forward does not care about the order."""
        value = value.float().contiguous()
        value_dpt_dist = value_dpt_dist.float().contiguous()
        sampling_locations = sampling_locations.float().contiguous()
        attention_weights = attention_weights.float().contiguous()
        item_batch = item_batch.to(torch.int32).contiguous()
        out = ext.ops().dfa3d_forward_items(value, value_dpt_dist, value_spatial_shapes, value_level_start_index,
                                            sampling_locations, attention_weights, item_batch)
        ctx.save_for_backward(value, value_dpt_dist, value_spatial_shapes, value_level_start_index,
                              sampling_locations, attention_weights, item_batch)
        ctx.bins = bins
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        value, dist, shapes3, lsi, loc, attn, item_batch = ctx.saved_tensors
        ops = ext.ops()
        grad_output = grad_output.float().contiguous()
        bins = ctx.bins
        N, S, M, Cm = value.shape
        n, LM, L, P = loc.shape[:4]
        if bins is not None and L == 1 and dist.shape[2] == 1 and n > 0:
            bin_offset, H, W, bw, bh, halo = bins[:6]
            head_shift = bins[6] if len(bins) > 6 and M > 1 else None
            # the kernel's head split: channel groups of 32 (16) channels; one head over C channels (the geometry sample) runs as C / 32
            # groups that share its sample set
            cmb = Cm if Cm in (16, 32) else (32 if Cm % 32 == 0 else 16 if Cm % 16 == 0 else 0)
            # measured (tools/bwd_tile_bench.py, profiles/r06_bwd_tile_bench_cfg2.txt): the deformable call (8 heads x 4 points) 1.25 ms
            # tiled against 1.89 ms on the item kernel; the geometry sample (ONE sample per pair: 4 KB of atomics, not 16) 0.57 against
            # 0.42 -- it keeps the item kernel unless TRAIN_BWD_TILED_SHARED says otherwise
            if M == 1 and Cm != cmb and not TRAIN_BWD_TILED_SHARED:
                cmb = 0
            if cmb and (cmb == Cm or M == 1) and P <= 4 and ops.dfa3d_backward_binned_fits(H, W, cmb, dist.shape[-1], bw, bh, halo):
                mb = M * Cm // cmb
                gv, gd, gl, ga = ops.dfa3d_backward_binned(value.view(N, S, mb, cmb), dist, loc, attn, bin_offset, grad_output, H, W, bw, bh,
                                                           halo, want_grad_loc=ctx.needs_input_grad[4], want_grad_attn=ctx.needs_input_grad[5],
                                                           head_shift=head_shift)
                return gv.view_as(value), gd, None, None, gl, ga, None, None
        gv, gd, gl, ga = ops.dfa3d_backward_items(value, dist, shapes3, lsi, loc, attn, item_batch, grad_output)
        return gv, gd, None, None, gl, ga, None, None


def _require_bf16_planes(who):
    """``sgc_pack_conv_weight`` emits bfloat16 bit patterns; in the fp16 arithmetic mode (``sgc_set_conv_products(2)``) the MFMA
    kernels would read them as IEEE half.  The training Functions therefore refuse that mode instead of computing garbage."""
    from .plugin import conv_plan
    if conv_plan.CONV_PRODUCTS == 2:
        raise RuntimeError(f"{who}: the fp16 arithmetic mode (set_conv_mode('fp16')) is inference-only -- the training Functions "
                           "pack bfloat16 weight planes; switch to 'bf16x3' / 'bf16' or run under torch.no_grad()")


class TrainWeightPlanes:
    """The bf16 hi | lo planes the training Functions multiply with, kept across steps and repacked TOGETHER.

    Every pass of a training step needs each parameter in the kernels' layout: [taps, Cout, Cin] for the forward, [taps, Cin, Cout]
    with mirrored taps for the input gradient (cuDNN does the same internally, necks/imvoxelnet.py:36-64).  Packing them where they
    are used is ~100 launches per config-2 step, most of them a few microseconds of work.  Here a plane pair is allocated the first
    time a (parameter storage, shape, form) is asked for and is registered; ``begin_step()`` -- the detector calls it at the start
    of every training forward -- repacks ALL registered planes in one launch (``sgc_pack_conv_weight_batch``): the same bytes in one
    launch instead of a hundred.  A plane is never served stale: ``get`` compares the version counter the parameter shares with
    the alias kept here (an in-place update between ``begin_step`` and the use repacks); edits through ``.data`` do not move
    that counter, which is why ``begin_step`` repacks unconditionally.  Entries are keyed by storage address + shape, so the
    per-step views of a fused parameter (``in_proj_weight[:C]``) map to one entry; an entry no ``get`` has asked for during two
    steps is dropped (its parameter is gone or has moved).  ``SGC_TRAIN_PACK_BATCH=0`` restores the pack-per-use form."""

    MAX_ENTRIES = 1024             # callers that never reach begin_step (stand-alone Functions, tests) cannot grow the table without bound

    def __init__(self):
        self.entries = {}          # (data_ptr, shape, transpose, flip, pad_rows, pad_cols) -> dict
        self.ephemeral = {}        # data_ptr of a per-step temporary (mark_ephemeral) -> dict(ref=tensor, planes={form key: (hi, lo)})
        self.plans = None          # per device: (entries, launch plan)
        self.enabled = os.environ.get("SGC_TRAIN_PACK_BATCH", "1") != "0"
        self.launches = 0          # batched launches so far (tests)
        self.step = 0

    def mark_ephemeral(self, weight):
        """``weight`` is a temporary of this step (e.g. the head's ``torch.cat`` of three parameters): its planes are packed where they
        are first used and shared by the step's later uses, but never REGISTERED -- a fresh temporary every step would add entries,
        reset the batched plan (a host-side rebuild + a synchronous copy of the item list) and pin the dead storages for two steps."""
        # the entry holds the tensor: its storage cannot be freed and re-used under the same address while the entry lives (entries go at
        # begin_step, or oldest-first beyond eight for callers that never reach it)
        if weight.data_ptr() not in self.ephemeral:
            while len(self.ephemeral) >= 8:
                del self.ephemeral[next(iter(self.ephemeral))]
            self.ephemeral[weight.data_ptr()] = dict(ref=weight, planes={})

    def get(self, weight, transpose=False, flip=False, pad_rows=1, pad_cols=1):
        ops = ext.ops()
        if not self.enabled or not weight.is_cuda or weight.dtype != torch.float32 or not weight.is_contiguous():
            return ops.pack_conv_weight(weight.detach().float(), transpose=transpose, flip=flip, pad_rows=pad_rows, pad_cols=pad_cols)
        eph = self.ephemeral.get(weight.data_ptr())
        if eph is not None:
            fk = (weight.shape, weight._version, transpose, flip, pad_rows, pad_cols)
            if fk not in eph["planes"]:
                eph["planes"][fk] = ops.pack_conv_weight(weight.detach(), transpose=transpose, flip=flip, pad_rows=pad_rows, pad_cols=pad_cols)
            return eph["planes"][fk]
        key = (weight.data_ptr(), weight.shape, transpose, flip, pad_rows, pad_cols)
        e = self.entries.get(key)
        if e is None:
            if len(self.entries) >= self.MAX_ENTRIES:          # least recently used half goes
                for k in sorted(self.entries, key=lambda k: self.entries[k]["used"])[:self.MAX_ENTRIES // 2]:
                    del self.entries[k]
            shape = ops.packed_shape(weight.shape, transpose, pad_rows, pad_cols)
            hi = torch.zeros(shape, dtype=torch.bfloat16, device=weight.device)
            lo = torch.zeros_like(hi)
            w = weight.detach()                        # an alias: keeps the storage where it is, shares the version counter
            ops.pack_conv_weight(w, transpose=transpose, flip=flip, pad_rows=pad_rows, pad_cols=pad_cols, out=(hi, lo))
            self.entries[key] = dict(w=w, hi=hi, lo=lo, version=w._version, transpose=bool(transpose), flip=bool(flip), used=self.step)
            self.plans = None
            return hi, lo
        e["used"] = self.step
        if e["version"] != weight._version:
            self.repack()
        return e["hi"], e["lo"]

    def repack(self):
        """One launch per device over every registered plane pair."""
        if self.plans is None:
            by_dev = {}
            for e in self.entries.values():
                by_dev.setdefault(e["hi"].device, []).append(e)
            ops = ext.ops()
            self.plans = [(es, ops.pack_conv_weight_plan([(e["w"], e["hi"], e["lo"], e["transpose"], e["flip"]) for e in es]))
                          for es in by_dev.values()]
        for es, plan in self.plans:
            ext.ops().run_pack_plan(plan)
            self.launches += 1
            for e in es:
                e["version"] = e["w"]._version

    def begin_step(self):
        self.ephemeral = {}
        if not self.enabled or not self.entries:
            return
        self.step += 1
        stale = [k for k, e in self.entries.items() if e["used"] < self.step - 2]
        for k in stale:
            del self.entries[k]
        if stale:
            self.plans = None
        if self.entries:
            self.repack()

    def clear(self):
        self.entries, self.plans, self.ephemeral = {}, None, {}


_TRAIN_PLANES = TrainWeightPlanes()


def train_weight_planes():
    return _TRAIN_PLANES


class NchwToRowsFunction(Function):
    """[N, C, h, w] map (any strides: the crop view of AdaptiveSparseHead.py:58-59) -> channels-last rows [N, h*w, C]
    (TU/transformer.py:151-170 ``flatten(2).permute``) with the transpose on the HIP kernels in both directions: forward
    ``sgc_nchw_to_nhwc_crop``, backward ``sgc_nhwc_to_nchw_pad`` (a contiguous NCHW gradient).  Autograd's own chain for
    ``flatten / permute / contiguous`` is two strided copies per level (0.26 ms each at config 2's finest level)."""

    @staticmethod
    def forward(ctx, x):
        ctx.hw = (x.shape[2], x.shape[3])
        return ext.ops().nchw_to_nhwc_crop(x.detach().float(), x.shape[2], x.shape[3])

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_rows):
        h, w = ctx.hw
        return ext.ops().nhwc_to_nchw_pad(grad_rows.float().contiguous(), h, w)


class PlaneSweepCorrFunction(Function):
    """Plane-sweep matching cost of ``DepthNet_Fusion`` (depth_est_fusion.py homo_warping :87-126 + the cost-volume loop
    :233-240) with its gradient on the HIP kernels: forward ``sgc_plane_sweep_corr``, backward
    ``sgc_plane_sweep_corr_backward`` (include/sgcdet_amd_train.h).  rows [N, H*W, C] channels-last matching features
    (the only differentiable input: the reference builds the sampling grid under no_grad), nbr [N,K] int32,
    rt [N,K,12], depth [D] -> corr [N,D,H,W].  Saves only its inputs: no warped [N,C,D,H,W] tensor exists."""

    @staticmethod
    def forward(ctx, rows, nbr, rt, depth, H, W):
        rows = rows.detach()
        ctx.hw = (H, W)
        ctx.save_for_backward(rows, nbr, rt, depth)
        return ext.ops().plane_sweep_corr(rows, nbr, rt, depth, H, W)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_corr):
        rows, nbr, rt, depth = ctx.saved_tensors
        H, W = ctx.hw
        grad_rows = ext.ops().plane_sweep_corr_backward(rows, nbr, rt, depth, grad_corr.float().contiguous(), H, W)
        return grad_rows, None, None, None, None, None


class HeadLossFunction(Function):
    """``ImVoxelHeadV2._loss_single`` (imvoxel_head_v2.py:147-235) for one image on the HIP kernels of csrc/head_loss.hip:
    forward ``sgc_head_loss_forward`` (values and unnormalised gradients in one pass), backward ``sgc_head_loss_scale_grads`` -- at most
    four launches for both passes, no host synchronisation.

    ``apply(points, centerness_targets, bbox_targets, labels, n_pos_override, cfg, *head)`` -> (loss_centerness, loss_bbox, loss_cls),
    three scalars.  ``head``: the 4 * n_scales tensors centerness[0..], bbox_pred[0..], cls_score[0..], valid[0..] (bbox_pred after its
    activation, [C,X,Y,Z] each, valid bool / uint8).  ``cfg`` = dict(rotated, gamma, alpha, loss_weights=(centerness, bbox, cls),
    reduce_n_pos): with ``reduce_n_pos`` and an initialised process group the local count of positives is all-reduced (mean) as a
    device tensor and the losses are normalised by it, as mmdet's ``reduce_mean`` does.  ``n_pos_override``: None or a 1-element device
    tensor that replaces the count.  Only the centerness / bbox_pred / cls_score tensors are differentiable; points, targets, labels
    and valid get no gradient."""

    @staticmethod
    def forward(ctx, points, centerness_targets, bbox_targets, labels, n_pos_override, cfg, *head):
        if len(head) % 4 or not head:
            raise RuntimeError("HeadLossFunction: centerness, bbox_pred, cls_score and valid tensors of every scale expected")
        L = len(head) // 4
        for t in head[:3 * L]:
            if t.dtype != torch.float32:      # the kernels read fp32; a silent .float() would hide an autocast region around the loss
                raise TypeError(f"HeadLossFunction: the head tensors must be float32 (got {t.dtype}); run the loss outside autocast")
        ops = ext.ops()
        det = [t.detach() for t in head]
        losses, n_pos, state = ops.head_loss(det[:L], det[L:2 * L], det[2 * L:3 * L], [v.reshape(-1) for v in det[3 * L:]], points,
                                             centerness_targets, bbox_targets, labels, cfg["rotated"], cfg.get("gamma", 2.0),
                                             cfg.get("alpha", 0.25), cfg.get("loss_weights", (1.0, 1.0, 1.0)), n_pos_override)
        if n_pos_override is None and cfg.get("reduce_n_pos") and torch.distributed.is_available() and torch.distributed.is_initialized():
            torch.distributed.all_reduce(n_pos.div_(torch.distributed.get_world_size()))          # mmdet reduce_mean, on the device
            losses, _ = ops.head_loss_finalize(state, n_pos)
        ctx.state, ctx.n_scales = state, L
        return losses[0], losses[1], losses[2]

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_centerness, grad_bbox, grad_cls):
        L = ctx.n_scales
        ctr, reg, cls = ext.ops().head_loss_grads(ctx.state, grad_centerness.float().contiguous(), grad_bbox.float().contiguous(),
                                                  grad_cls.float().contiguous())
        return (None,) * 6 + tuple(ctr) + tuple(reg) + tuple(cls) + (None,) * L


def _pad_cols(t, mult):
    """[rows, C] -> [rows, ceil(C / mult) * mult] with zero columns (a view when nothing is added)."""
    c = t.shape[-1]
    cp = (c + mult - 1) // mult * mult
    return t if cp == c else torch.nn.functional.pad(t, (0, cp - c))


class ChannelsLastConv3dFunction(Function):
    """``nn.Conv3d(k, stride, padding=k//2, bias=False)`` on channels-last rows, forward AND backward on the MFMA kernels
    (the neck / head convolutions in training; the reference gets all three passes from cuDNN,
    necks/imvoxelnet.py:36-64, dense_heads/imvoxel_head_v2.py:75-78).

    x [X*Y*Z, Cin] rows of the volume, weight [Cout, Cin, k, k, k] (the module's parameter, untouched layout), grid =
    (X, Y, Z), k in {1, 3}, stride in {1, 2} -> y [OX*OY*OZ, Cout].  Cin % 32 == 0.

    * forward: ``sgc_conv3d_cl_bf16x3`` (no epilogue: BatchNorm in training mode needs the raw output);
    * input gradient: the same kernel on dy with the taps mirrored and Cin / Cout swapped; for stride 2 on the
      zero-interleaved dy (dy at the even fine-grid positions: 8x the necessary matrix work on two small layers, no new
      kernel -- the two stride-2 layers are 6 % of the neck's FLOPs);
    * weight gradient: ``sgc_conv3d_wgrad_bf16x3``.

    ``scenes`` > 1 (training on scene batches): x holds that many volumes of ``grid`` one after the other
    ([scenes * X*Y*Z, Cin]) and so do y and both gradients; every pass is ONE launch of the ``_batched`` entries and the weight
    gradient -- one per layer, not one per scene -- is summed over the scenes inside its kernel.
    """

    @staticmethod
    def forward(ctx, x, weight, grid, ksize, stride, scenes=1):
        _require_bf16_planes("ChannelsLastConv3dFunction")
        ops = ext.ops()
        cout, cin = weight.shape[:2]
        # parameter [Cout, Cin, k, k, k] -> the kernel's [taps, Cout (multiple of 4), Cin] bf16 hi / lo planes in ONE launch
        hi, lo = _TRAIN_PLANES.get(weight, pad_rows=4)
        x = x.float().contiguous()
        y, og = ops.conv3d_cl_bf16x3(x, hi, lo, grid, ksize, stride, scenes=scenes)
        ctx.save_for_backward(x, weight)
        ctx.geom = (tuple(grid), tuple(og), ksize, stride, int(scenes))
        return y[:, :cout] if y.shape[1] != cout else y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        ops = ext.ops()
        x, weight = ctx.saved_tensors
        grid, og, ksize, stride, scenes = ctx.geom
        cout, cin = weight.shape[:2]
        dy = dy.float().contiguous()
        dx = dw = None
        if ctx.needs_input_grad[0]:
            # dx[i] = sum_d dy[(i - d + pad) / stride] W[d]^T: a stride-1 convolution of (zero-interleaved) dy with the
            # mirrored taps; its "input channels" are Cout, padded to the kernel's multiple of 32
            hi, lo = _TRAIN_PLANES.get(weight, transpose=True, flip=True, pad_cols=32)
            g = _pad_cols(dy, 32)
            if stride == 2:
                up = torch.zeros((scenes, grid[0], grid[1], grid[2], g.shape[1]), dtype=torch.float32, device=dy.device)
                up[:, :2 * og[0]:2, :2 * og[1]:2, :2 * og[2]:2] = g.view(scenes, og[0], og[1], og[2], -1)
                g = up.view(-1, g.shape[1])
            dx, _ = ops.conv3d_cl_bf16x3(g.contiguous(), hi, lo, grid, ksize, 1, scenes=scenes)
        if ctx.needs_input_grad[1]:
            # the halo form of the weight gradient wants 32-channel dy tiles: the head's 3 x 3 x 3 convolutions (Cout = 28 ...)
            # get four zero columns rather than the per-tap tile kernel
            mult = 32 if ksize == 3 and stride == 1 and cin % 32 == 0 else 4
            dwk = ops.conv3d_wgrad_bf16x3(x, _pad_cols(dy, mult).contiguous(), grid, ksize, stride, scenes=scenes)     # [taps, cout_p, cin]
            dw = ops.unpack_conv_wgrad(dwk, weight.shape).to(weight.dtype)
        return dx, dw, None, None, None, None


def _conv2d_rows(*args, **kwargs):
    """``conv_plan.conv2d_rows``, the one dispatch rule of the 2-D entries (imported at the call: conv_plan imports this module)."""
    from .plugin.conv_plan import conv2d_rows
    return conv2d_rows(*args, **kwargs)


def _conv2d_input_grad(g, weight, nhw, k, stride, planes):
    """dx [N*H*W, Cin] of ``nn.Conv2d(k, stride, padding=k//2)`` over nhw = (N, H, W) from g = dL/dy [N*OH*OW, Cout] rows, on the
    forward entries.  ``planes``: ``_TRAIN_PLANES.get`` or ``_padded_planes`` (then both widths are the padded ones).  Stride 1 -- the
    forward entry on g with the taps mirrored and Cin / Cout swapped; 3x3 stride 2 -- the transposed form of
    ``sgc_conv2d_nhwc_ex_bf16x3`` (sums by output parity, 2.25 taps per pixel), cropped to H x W when a side is odd; 1x1 stride 2
    -- the 1x1 GEMM on g, written to the even positions of a zeroed map."""
    N, H, W = nhw
    OH, OW = (H + stride - 1) // stride, (W + stride - 1) // stride
    if stride == 1:
        hi, lo = planes(weight, transpose=True, flip=True)         # [k*k, Cin, Cout], taps mirrored
        return _conv2d_rows(g, hi, lo, (N, H, W), k, relu=False)
    hi, lo = planes(weight, transpose=True)                        # the ConvTranspose2d reading of the parameter
    if k == 3:
        up = _conv2d_rows(g, hi, lo, (N, OH, OW), 3, stride=2, transposed=True, relu=False)      # [N * 2 OH * 2 OW, Cin]
        return up if (2 * OH, 2 * OW) == (H, W) else up.view(N, 2 * OH, 2 * OW, -1)[:, :H, :W].reshape(N * H * W, -1)
    t = _conv2d_rows(g, hi, lo, (N, OH, OW), 1, relu=False)
    dx = torch.zeros((N, H, W, t.shape[1]), dtype=torch.float32, device=g.device)
    dx[:, ::2, ::2] = t.view(N, OH, OW, -1)
    return dx.view(N * H * W, -1)


def _conv2d_weight_grad(x, g, weight, nhw, k, stride):
    """dL/dweight in the parameter's shape and dtype: ``sgc_conv2d_wgrad_bf16x3`` ([k*k, Cout, Cin] at the rows' widths), then
    ``sgc_unpack_conv_wgrad``, which drops any padding."""
    ops = ext.ops()
    return ops.unpack_conv_wgrad(ops.conv2d_wgrad_bf16x3(x, g, tuple(nhw), k, stride), weight.shape).to(weight.dtype)


def _conv2d_bias_grad(g, weight):
    """The column sums of g (``sgc_rows_colsum``) over the parameter's Cout columns."""
    return ext.ops().rows_colsum(g)[:weight.shape[0]].to(weight.dtype)


class FrozenNormConv2dFunction(Function):
    """``act(norm(nn.Conv2d(k, stride, padding=k//2, bias=False)(x)) [+ residual])`` with a FROZEN norm (eval statistics, no
    gradient to its parameters: the ResNet backbone in every reference config) on channels-last rows, all three passes on the
    MFMA kernels.  The norm is the folded per-channel ``scale`` / ``shift`` of the eval lowering, so the
    forward is the eval forward: both reach the entry points through ``conv_plan.conv2d_rows``, the one dispatch rule, and so
    do the input gradients below.  ``conv_plan.FrozenConv2d`` wraps this Function in ``Conv2dSpec``'s call signature.

    ``apply(x, weight, scale, shift, residual, nhw, stride, relu, relu_after_add)``: x [N*H*W, Cin] rows, weight
    [Cout, Cin, k, k] (the module's parameter), scale / shift [Cout] | None, residual [N*OH*OW, Cout] | None, nhw = (N, H, W)
    -> y [N*OH*OW, Cout], OH = ceil(H / stride).  Cin % 32 == 0, Cout % 32 == 0, k in {1, 3}, stride in {1, 2}.
    ``relu``: ReLU behind the norm (no residual); ``relu_after_add``: ReLU behind the skip addition.  ``relu`` WITH a residual
    (``relu(t) + residual``) is refused: its gate cannot be read off y.

    * backward of the epilogue: ``sgc_frozen_norm_act_backward`` (gate y > 0, times scale; the gated dy is the residual's gradient);
    * input gradient: stride 1 -- the forward entry on g with the taps mirrored and Cin / Cout swapped; 3x3 stride 2 -- the
      transposed form of ``sgc_conv2d_nhwc_ex_bf16x3`` (sums by output parity, 2.25 taps per pixel), cropped to H x W when a
      side is odd; 1x1 stride 2 -- the 1x1 GEMM on g, written to the even positions of a zeroed map;
    * weight gradient: ``sgc_conv2d_wgrad_bf16x3``.
    x, y and the weight are saved; a layer's y is the next layer's x, so nothing is kept twice.

    A tenth argument ``bias`` [Cout] makes it ``conv(x) + bias`` with a TRAINABLE bias (the FPN's convolutions: no norm, no
    activation -- DESIGN.md 4.13): it takes the place of ``shift`` in the epilogue (``scale``, ``shift`` and both ReLU flags must
    be None / False), and the backward adds its gradient, the column sums of dy (``sgc_rows_colsum``).
    ``conv_plan.BiasConv2d`` wraps this form."""

    @staticmethod
    def forward(ctx, x, weight, scale, shift, residual, nhw, stride, relu, relu_after_add, bias=None):
        _require_bf16_planes("FrozenNormConv2dFunction")
        cout, cin, k = weight.shape[0], weight.shape[1], weight.shape[2]
        if weight.dim() != 4 or weight.shape[3] != k or k not in (1, 3) or stride not in (1, 2) or cin % 32 or cout % 32:
            raise RuntimeError("FrozenNormConv2dFunction: needs a [Cout, Cin, k, k] weight, k in {1, 3}, stride in {1, 2}, Cin % 32 == 0, Cout % 32 == 0")
        if relu and residual is not None:
            raise RuntimeError("FrozenNormConv2dFunction: relu(norm(conv)) + residual has no gate in its output; "
                               "use relu_after_add (the ReLU behind the skip addition)")
        if relu and relu_after_add:
            raise RuntimeError("FrozenNormConv2dFunction: relu and relu_after_add exclude each other")
        if bias is not None:
            if scale is not None or shift is not None or relu or relu_after_add or bias.shape != (cout,):
                raise RuntimeError("FrozenNormConv2dFunction: a trainable bias [Cout] comes without scale / shift and without a ReLU")
            shift = bias
        hi, lo = _TRAIN_PLANES.get(weight)                     # [k*k, Cout, Cin]
        x = x.float().contiguous()
        res = None if residual is None else residual.detach().float().contiguous()
        scale = None if scale is None else scale.detach().float().contiguous()
        shift = None if shift is None else shift.detach().float().contiguous()
        y = _conv2d_rows(x, hi, lo, nhw, k, stride, scale=scale, shift=shift, residual=res, relu=relu, relu_after_add=relu_after_add)
        ctx.save_for_backward(x, y, weight, scale)
        ctx.geom = (tuple(nhw), k, stride, bool(relu or relu_after_add), residual is not None)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        ops = ext.ops()
        x, y, weight, scale = ctx.saved_tensors
        (N, H, W), k, stride, gated, has_res = ctx.geom
        dy = dy.float().contiguous()
        want_res = has_res and ctx.needs_input_grad[4]
        if gated or scale is not None:
            g, gres = ops.frozen_norm_act_backward(dy, y if gated else None, scale, relu=gated, want_gres=want_res and gated)
            if want_res and not gated:
                gres = dy
        else:
            g, gres = dy, (dy if want_res else None)
        dx = _conv2d_input_grad(g, weight, (N, H, W), k, stride, _TRAIN_PLANES.get) if ctx.needs_input_grad[0] else None
        dw = _conv2d_weight_grad(x, g, weight, (N, H, W), k, stride) if ctx.needs_input_grad[1] else None
        if not ctx.has_bias:
            return dx, dw, None, None, gres, None, None, None, None
        db = _conv2d_bias_grad(g, weight) if ctx.needs_input_grad[9] else None       # g is dy: no gate, no scale
        return dx, dw, None, None, gres, None, None, None, None, db


class Stem7ConvFunction(Function):
    """``nn.Conv2d(3, 64, 7, stride=2, padding=3)(img) [+ bias]`` as channels-last rows, for a stem whose weight trains (the
    ResNet-18 trunk of ``DepthNet_Fusion``; a live BatchNorm follows, so there is no epilogue beyond the bias).

    ``apply(img, weight, bias)``: img [N, 3, H, W] fp32 NCHW with even H, W; weight [64, 3, 7, 7] (the module's parameter); bias
    [64] | None -> y [N * H/2 * W/2, 64].

    * forward: ``sgc_conv2d_stem7_bf16x3`` with no scale, shift = bias, no ReLU, on [64][160] planes packed from the parameter
      here, at every call (they are 2 x 20 KB and never kept, so never stale);
    * weight gradient: ``sgc_conv2d_stem7_wgrad_bf16x3``, which writes the parameter's own layout;
    * bias gradient: ``sgc_rows_colsum`` of dy;
    * images get no gradient: one that requires it is refused (its caller keeps the torch formulation)."""

    @staticmethod
    def forward(ctx, img, weight, bias=None):
        _require_bf16_planes("Stem7ConvFunction")
        if img.requires_grad:
            raise RuntimeError("Stem7ConvFunction: no input gradient -- images that require grad take the torch formulation")
        if tuple(weight.shape) != (64, 3, 7, 7) or (bias is not None and tuple(bias.shape) != (64,)):
            raise RuntimeError("Stem7ConvFunction: needs a [64, 3, 7, 7] weight and a [64] bias (or None)")
        ops = ext.ops()
        w = torch.nn.functional.pad(weight.detach().float().reshape(64, 147), (0, 13)).contiguous()   # column (ci * 7 + kh) * 7 + kw
        hi, lo = ops.split_operand(w)
        img = img.detach().float().contiguous()
        shift = None if bias is None else bias.detach().float().contiguous()
        y = ops.conv2d_stem7_bf16x3(img, hi, lo, scale=None, shift=shift, relu=False)
        ctx.save_for_backward(img)
        ctx.dtypes = (weight.dtype, None if bias is None else bias.dtype)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        ops = ext.ops()
        img, = ctx.saved_tensors
        dy = dy.float().contiguous()
        dw = ops.conv2d_stem7_wgrad_bf16x3(img, dy).to(ctx.dtypes[0]) if ctx.needs_input_grad[1] else None
        db = ops.rows_colsum(dy).to(ctx.dtypes[1]) if ctx.dtypes[1] is not None and ctx.needs_input_grad[2] else None
        return None, dw, db


class UpsampleNearestAddFunction(Function):
    """The FPN's top-down step on channels-last rows: ``fine + nearest_upsample(coarse)`` to the fine map's size,
    forward ``sgc_upsample_nearest_add_nhwc`` (out of place), backward ``sgc_upsample_nearest_add_backward_nhwc`` for the coarse
    rows; the fine rows' gradient is dy itself.  ``apply(fine_rows [N*Hd*Wd, C], coarse_rows [N*Hs*Ws, C], (N, Hd, Wd),
    (N, Hs, Ws))``.  Saves nothing."""

    @staticmethod
    def forward(ctx, fine, coarse, dims_fine, dims_coarse):
        ctx.dims = (tuple(dims_fine), tuple(dims_coarse))
        return ext.ops().upsample_nearest_add_nhwc(fine.detach().float().contiguous(), coarse.detach().float().contiguous(),
                                                   *ctx.dims)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        dy = dy.float().contiguous()
        gcoarse = ext.ops().upsample_nearest_add_backward_nhwc(dy, *ctx.dims) if ctx.needs_input_grad[1] else None
        return (dy if ctx.needs_input_grad[0] else None), gcoarse, None, None


class ChannelsLastConvTranspose3dFunction(Function):
    """``nn.ConvTranspose3d(2, 2, bias=False)`` on channels-last rows (up_block_*, necks/imvoxelnet.py:56-58): forward on the
    parity form of the MFMA kernel, input gradient = the k2 s2 convolution of dy, weight gradient =
    ``sgc_conv3d_wgrad_bf16x3`` with the roles of the two tensors exchanged.  x [X*Y*Z, Cin], weight [Cin, Cout, 2, 2, 2]
    -> y [8*X*Y*Z, Cout]; Cin % 32 == 0, Cout % 32 == 0.  ``scenes`` as in ``ChannelsLastConv3dFunction``."""

    @staticmethod
    def forward(ctx, x, weight, grid, scenes=1):
        _require_bf16_planes("ChannelsLastConvTranspose3dFunction")
        ops = ext.ops()
        cin, cout = weight.shape[:2]
        hi, lo = _TRAIN_PLANES.get(weight, transpose=True)            # [Cin, Cout, 8] -> [8, Cout, Cin]
        x = x.float().contiguous()
        y, og = ops.conv3d_cl_bf16x3(x, hi, lo, grid, 2, 2, True, scenes=scenes)
        ctx.save_for_backward(x, weight)
        ctx.geom = (tuple(grid), tuple(og), int(scenes))
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        ops = ext.ops()
        x, weight = ctx.saved_tensors
        grid, og, scenes = ctx.geom
        cin, cout = weight.shape[:2]
        dy = dy.float().contiguous()
        dx = dw = None
        if ctx.needs_input_grad[0]:
            hi, lo = _TRAIN_PLANES.get(weight)                        # [Cin, Cout, 8] -> [8, Cin, Cout]
            dx, _ = ops.conv3d_cl_bf16x3(dy, hi, lo, og, 2, 2, scenes=scenes)   # dx[x] = sum_p dy[2x + p] W[:, :, p]^T
        if ctx.needs_input_grad[1]:
            dwk = ops.conv3d_wgrad_bf16x3(dy, x, og, 2, 2, scenes=scenes)       # [8, cin, cout]
            dw = ops.unpack_conv_wgrad(dwk, weight.shape).to(weight.dtype)
        return dx, dw, None, None


class BatchNormRowsFunction(Function):
    """Training-mode ``nn.BatchNorm3d`` on channels-last rows [rows, C] (necks/imvoxelnet.py:36-64: every convolution of the neck
    is followed by one): statistics, normalisation and the backward reductions on the ``sgc_bn_rows_*`` kernels (ordered
    reductions: the same bits every run) instead of torch's channels-last batch-norm kernels.  The running statistics are
    updated in place by the forward kernel, as ``F.batch_norm(training=True)`` does.

    ``residual`` / ``tail`` (round 5): the elementwise tail of a block inside the same passes.  ``tail`` 0 (False): bn + residual?;
    1 (True): relu(bn + residual?) -- ``relu(norm(conv))`` and the ResBlock tail ``relu(norm2(conv2) + identity)``, backward the
    incoming gradient masked where ``y > 0`` (torch's ``threshold_backward``) before the BatchNorm backward, the identity's gradient
    being that masked gradient; 2: relu(bn) + residual -- the U-Net skip, whose gate the backward recomputes from the saved input.

    ``channels`` None: the rows are as wide as the norm and ``tail`` is 0 or 1 (``sgc_bn_rows_forward / _backward`` and their
    ``_act_`` forms).  ``channels`` given: rows [R, ld] of which the first C = ``weight.numel()`` columns are
    channels and the rest zero padding, the module's own [C] parameters and running statistics, on ``sgc_bn_rows_padded_forward /
    _backward``; the padding columns of the output and of both gradients are written as zeros whatever the padding of the inputs
    holds.  Both are the same kernels, so the choice decides the entry point and nothing about the values."""

    @staticmethod
    def forward(ctx, rows, weight, bias, running_mean, running_var, momentum, eps, residual=None, tail=0, channels=None):
        ops = ext.ops()
        tail = int(tail)
        if channels is None and tail == 2:
            raise ValueError("BatchNormRowsFunction: tail 2 is a padded-entry tail (pass channels)")
        x = rows.contiguous()
        res = None if residual is None else residual.detach().contiguous()
        w, b = weight.detach().contiguous(), bias.detach().contiguous()
        if channels is None:
            y, mean, invstd = ops.bn_rows_forward(x, w, b, running_mean, running_var, momentum, eps, residual=res, relu=bool(tail))
        else:
            y, mean, invstd = ops.bn_rows_padded_forward(x, w, b, running_mean, running_var, momentum, eps, residual=res, tail=tail)
        ctx.tail, ctx.has_res, ctx.padded = tail, residual is not None, channels is not None
        ctx.save_for_backward(x, mean, invstd, w, b, *((y,) if tail == 1 else ()))
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        ops = ext.ops()
        saved = ctx.saved_tensors
        x, mean, invstd, w, b = saved[:5]
        g = grad_y.float().contiguous()
        want_res = ctx.has_res and ctx.needs_input_grad[7]
        if ctx.padded:
            dx, dw, db, dres = ops.bn_rows_padded_backward(x, g, mean, invstd, w, bias=b, y=saved[5] if ctx.tail == 1 else None,
                                                           tail=ctx.tail, want_dresidual=want_res)
        elif ctx.tail:
            dx, dw, db, dres = ops.bn_rows_backward(x, g, mean, invstd, w, y_relu=saved[5], want_dresidual=want_res)
        else:                                          # no mask: the identity's gradient IS the incoming gradient
            dx, dw, db = ops.bn_rows_backward(x, g, mean, invstd, w)
            dres = g if want_res else None
        return dx, dw, db, None, None, None, None, dres, None, None


def _dist_on():
    import torch.distributed as dist
    return dist.is_available() and dist.is_initialized()


def _sync_world(group):
    import torch.distributed as dist
    return dist.get_world_size(group) if _dist_on() else 1


class SyncBatchNormRowsFunction(Function):
    """Training-mode ``dist.SyncBatchNorm3d`` on channels-last rows [rows, C]: ``BatchNormRowsFunction``'s passes cut at the seam
    between this rank's rows and the rows of all ranks (include/sgcdet_amd_syncbn.h).

    forward   ``bn_rows_sync_stats`` -> ONE all-gather of [mean | M2 | count] (2C + 1 floats) -> ``bn_rows_sync_apply`` (ranks merged
              in rank order on the device: the same bits on every rank; running statistics over the rows of all ranks; the tail
              ``relu?(bn + residual?)`` in the pass)
    backward  ``bn_rows_sync_backward_sums`` -> ONE all-reduce of [sum g | sum g * xhat] (2C floats) ->
              ``bn_rows_sync_backward_apply`` (1 / N_total read from device memory)

    No value is read back to the host between a pass's entry and exit.  ``dweight`` / ``dbias`` are this rank's LOCAL sums: the step's
    gradient all-reduce averages them like every other parameter gradient (``dist._SyncBatchNormFn`` documents the same).  With no
    initialised process group ``world`` is 1 and no collective is called; an initialised group of one rank runs both collectives
    (a copy and the identity).  Either way one rank's results are bit for bit ``BatchNormRowsFunction``'s.  ``tail`` is 0 or 1;
    ``group`` the process group (None: the default group)."""

    @staticmethod
    def forward(ctx, rows, weight, bias, running_mean, running_var, momentum, eps, residual=None, tail=0, group=None):
        ops = ext.ops()
        tail = int(tail)
        if tail not in (0, 1):
            raise ValueError("SyncBatchNormRowsFunction: tail is 0 or 1")
        x = rows.contiguous()
        res = None if residual is None else residual.detach().contiguous()
        w, b = weight.detach().contiguous(), bias.detach().contiguous()
        world, collective = _sync_world(group), _dist_on()
        stats = ops.bn_rows_sync_stats(x)
        gathered = stats
        if collective:
            import torch.distributed as dist
            gathered = torch.empty((world, stats.numel()), dtype=stats.dtype, device=stats.device)
            dist.all_gather_into_tensor(gathered, stats, group=group)
        y, mean, invstd, inv_count = ops.bn_rows_sync_apply(x, gathered, w, b, running_mean, running_var, momentum, eps, residual=res,
                                                            relu=bool(tail))
        ctx.tail, ctx.has_res, ctx.group, ctx.collective = tail, residual is not None, group, collective
        ctx.save_for_backward(x, mean, invstd, inv_count, w, *((y,) if tail == 1 else ()))
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        ops = ext.ops()
        saved = ctx.saved_tensors
        x, mean, invstd, inv_count, w = saved[:5]
        y_relu = saved[5] if ctx.tail == 1 else None
        g = grad_y.float().contiguous()
        want_res = ctx.has_res and ctx.needs_input_grad[7]
        sums = ops.bn_rows_sync_backward_sums(x, g, mean, invstd, y_relu=y_relu)
        local = sums
        if ctx.collective:
            import torch.distributed as dist
            local = sums.clone()                           # dbias | dweight stay this rank's sums
            dist.all_reduce(sums, op=dist.ReduceOp.SUM, group=ctx.group)
        C = w.numel()
        # no mask (tail 0): the identity's gradient IS the incoming gradient
        dx, dres = ops.bn_rows_sync_backward_apply(x, g, mean, invstd, w, sums, inv_count, y_relu=y_relu,
                                                   want_dresidual=want_res and ctx.tail == 1)
        if want_res and ctx.tail == 0:
            dres = g
        return dx, local[C:], local[:C], None, None, None, None, dres, None, None


def _padded_planes(weight, **form):
    """The parameter's planes with both channel counts zero-padded to multiples of 32 (the K tile and the rows' pitch)."""
    return _TRAIN_PLANES.get(weight, pad_rows=32, pad_cols=32, **form)


def _pad32(n):
    return (n + 31) // 32 * 32


class PaddedConv2dFunction(Function):
    """``nn.Conv2d(k, stride, padding=k//2)(x) [+ bias]`` on channels-last rows of PADDED width, for channel counts that are no
    multiple of 32 (the regulation U-Nets of ``DepthNet_Fusion``: 12 / 24 / 48 and 140 / 280 / 560 channels) --
    ``FrozenNormConv2dFunction``'s bias form with the parameter at its true shape and the rows at 32-column pitch.

    ``apply(x, weight, bias, nhw, stride)``: x [N*H*W, Cin_p], weight [Cout, Cin, k, k] (the module's parameter), bias [Cout] | None
    -> y [N*OH*OW, Cout_p], Cin_p / Cout_p = the next multiples of 32.  k = 3 with stride 1 or 2, k = 1 with stride 1.  The padding
    columns of x must be zeros (or at least finite: they meet zero weight columns); those of y are exactly zero.

    * forward and input gradient: ``conv_plan.conv2d_rows`` on planes packed with zero rows / columns;
    * weight gradient: ``sgc_conv2d_wgrad_bf16x3`` at the padded sizes, ``sgc_unpack_conv_wgrad`` drops the padding;
    * bias gradient: ``sgc_rows_colsum`` of dy."""

    @staticmethod
    def forward(ctx, x, weight, bias, nhw, stride):
        _require_bf16_planes("PaddedConv2dFunction")
        cout, cin, k = weight.shape[0], weight.shape[1], weight.shape[2]
        if weight.dim() != 4 or weight.shape[3] != k or (k, stride) not in ((3, 1), (3, 2), (1, 1)):
            raise RuntimeError("PaddedConv2dFunction: needs a [Cout, Cin, k, k] weight with (k, stride) in (3, 1), (3, 2), (1, 1)")
        if x.dim() != 2 or x.shape[1] != _pad32(cin) or (bias is not None and bias.shape != (cout,)):
            raise RuntimeError(f"PaddedConv2dFunction: x must be rows of {_pad32(cin)} columns (Cin = {cin} padded) and bias [Cout]")
        hi, lo = _padded_planes(weight)                        # [k*k, Cout_p, Cin_p]
        x = x.float().contiguous()
        shift = None if bias is None else _pad_cols(bias.detach().float().view(1, -1), 32).view(-1).contiguous()
        y = _conv2d_rows(x, hi, lo, nhw, k, stride, shift=shift, relu=False)
        ctx.save_for_backward(x, weight)
        ctx.geom, ctx.has_bias = (tuple(nhw), k, stride), bias is not None
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        nhw, k, stride = ctx.geom
        g = dy.float().contiguous()
        dx = _conv2d_input_grad(g, weight, nhw, k, stride, _padded_planes) if ctx.needs_input_grad[0] else None
        dw = _conv2d_weight_grad(x, g, weight, nhw, k, stride) if ctx.needs_input_grad[1] else None       # at the padded sizes
        db = _conv2d_bias_grad(g, weight) if ctx.has_bias and ctx.needs_input_grad[2] else None
        return dx, dw, db, None, None


class ConvTranspose2dRowsFunction(Function):
    """``nn.ConvTranspose2d(3, stride 2, padding 1, output_padding 1, bias=False)`` on channels-last rows of padded width, all three
    passes on the existing convolution entries.  ``apply(x, weight, nhw)``: x [N*H*W, Cin_p], weight
    [Cin, Cout, 3, 3] (the module's parameter) -> y [N*2H*2W, Cout_p].

    * forward: the transposed form of ``sgc_conv2d_nhwc_ex_bf16x3`` on the ``transpose=True`` planes [9, Cout_p, Cin_p];
    * input gradient: dx[n,i,j,ci] = sum dy[n, 2i+kh-1, 2j+kw-1, co] w[ci][co][kh][kw] -- the stride-2 3x3 forward entry on dy with
      the parameter read as a Conv2d weight [out = Cin][in = Cout], taps not mirrored;
    * weight gradient: dw[ci][co][kh][kw] = sum x[n,i,j,ci] dy[n, 2i+kh-1, 2j+kw-1, co] -- ``sgc_conv2d_wgrad_bf16x3`` at k = 3,
      s = 2 with the operands swapped (dy as its x, x as its dy); its [9][Cin_p][Cout_p] result is the parameter's own order."""

    @staticmethod
    def forward(ctx, x, weight, nhw):
        _require_bf16_planes("ConvTranspose2dRowsFunction")
        if weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3) or x.dim() != 2 or x.shape[1] != _pad32(weight.shape[0]):
            raise RuntimeError("ConvTranspose2dRowsFunction: needs a [Cin, Cout, 3, 3] weight and rows of Cin padded to 32 columns")
        hi, lo = _padded_planes(weight, transpose=True)        # [9, Cout_p, Cin_p]
        x = x.float().contiguous()
        y = _conv2d_rows(x, hi, lo, nhw, 3, stride=2, transposed=True, relu=False)
        ctx.save_for_backward(x, weight)
        ctx.nhw = tuple(nhw)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        N, H, W = ctx.nhw
        g = dy.float().contiguous()
        dx = None
        if ctx.needs_input_grad[0]:
            hi, lo = _padded_planes(weight)                    # [9, Cin_p, Cout_p]
            dx = _conv2d_rows(g, hi, lo, (N, 2 * H, 2 * W), 3, stride=2, relu=False)
        dw = _conv2d_weight_grad(g, x, weight, (N, 2 * H, 2 * W), 3, 2) if ctx.needs_input_grad[1] else None      # operands swapped
        return dx, dw, None


class DepthRegSoftmaxFunction(Function):
    """``softmax(nn.Conv2d(Cin, D, 3, padding=1)(x) + bias, dim=channels)`` on rows: ``depth_reg`` and the softmax behind it
    (DESIGN.md 4.14b).  ``apply(x, weight, bias, nhw)``: x [N*H*W, Cin_p], weight [D, Cin, 3, 3], bias [D] -> p [N*H*W, D] dense;
    D % 4 == 0, D <= 32.

    * forward: ``sgc_conv2d_nhwc_ex_bf16x3`` with shift = bias and the softmax over its D columns in the epilogue (the eval forward);
    * backward: ``sgc_softmax_rows_backward`` into a 32-column g, then the input gradient (mirrored taps), the weight gradient and
      ``sgc_rows_colsum`` as in ``FrozenNormConv2dFunction``'s bias form."""

    @staticmethod
    def forward(ctx, x, weight, bias, nhw):
        _require_bf16_planes("DepthRegSoftmaxFunction")
        D, cin = weight.shape[0], weight.shape[1]
        if weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3) or D % 4 or D > 32 or bias is None or bias.shape != (D,):
            raise RuntimeError("DepthRegSoftmaxFunction: needs a [D, Cin, 3, 3] weight and a [D] bias with D % 4 == 0, D <= 32")
        if x.dim() != 2 or x.shape[1] != _pad32(cin):
            raise RuntimeError(f"DepthRegSoftmaxFunction: x must be rows of {_pad32(cin)} columns (Cin = {cin} padded)")
        hi, lo = _TRAIN_PLANES.get(weight, pad_rows=4, pad_cols=32)                 # [9, D, Cin_p]
        x = x.float().contiguous()
        p = _conv2d_rows(x, hi, lo, nhw, 3, shift=bias.detach().float().contiguous(), relu=False, softmax_cols=D)
        ctx.save_for_backward(x, p, weight)
        ctx.nhw = tuple(nhw)
        return p

    @staticmethod
    @once_differentiable
    def backward(ctx, dp):
        x, p, weight = ctx.saved_tensors
        g = ext.ops().softmax_rows_backward(p, dp.float().contiguous(), C=weight.shape[0], ldg=32)      # [rows, 32], zero behind D
        dx = _conv2d_input_grad(g, weight, ctx.nhw, 3, 1, _padded_planes) if ctx.needs_input_grad[0] else None     # planes [9, Cin_p, 32]
        dw = _conv2d_weight_grad(x, g, weight, ctx.nhw, 3, 1) if ctx.needs_input_grad[1] else None                # from [9, 32, Cin_p]
        db = _conv2d_bias_grad(g, weight) if ctx.needs_input_grad[2] else None
        return dx, dw, db, None


class LinearRowsFunction(Function):
    """``nn.Linear`` over a row list with all three passes on the MFMA kernels (training path of the view transform:
    value_proj / sampling_offsets / attention_weights / output_proj, TU/deformable_cross_attention.py:417-436,826): forward
    and input gradient on ``sgc_linear_rows_bf16x3`` (the latter with W^T), weight gradient on ``sgc_conv3d_wgrad_bf16x3``
    with ksize 1 (the rows are its "voxels").  x [rows, Cin] (Cin % 32 == 0), weight [Cout, Cin], bias [Cout] | None."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        _require_bf16_planes("LinearRowsFunction")
        ops = ext.ops()
        cout, cin = weight.shape
        x = x.float().contiguous()
        hi, lo = _TRAIN_PLANES.get(weight, pad_rows=4)            # [1, Cout (multiple of 4), Cin]
        shift = None if bias is None else _pad_cols(bias.detach().float().view(1, -1), 4).view(-1).contiguous()
        y = ops.linear_rows_bf16x3(x, hi, lo, shift)
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return y if y.shape[1] == cout else y[:, :cout]

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        ops = ext.ops()
        x, weight = ctx.saved_tensors
        cout, cin = weight.shape
        dy = dy.float().contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            hi, lo = _TRAIN_PLANES.get(weight, transpose=True, pad_cols=32)   # [1, Cin, Cout -> mult of 32]: dx = dy @ W
            dx = ops.linear_rows_bf16x3(_pad_cols(dy, 32).contiguous(), hi, lo, None)
        if ctx.needs_input_grad[1]:
            dwk = ops.conv3d_wgrad_bf16x3(x, _pad_cols(dy, 4).contiguous(), (x.shape[0], 1, 1), 1, 1)     # [1, cout_p, cin]
            dw = dwk[0, :cout].to(weight.dtype)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            # the fused level (plugin/voxformer.py TRAIN_LEVEL_FUSED) takes the fixed-order column sums of this library; the
            # default path keeps dy.sum(0), so its summation order does not move
            db = ops.rows_colsum(dy) if level_fused_enabled() and dy.is_cuda and cout % 4 == 0 and dy.shape[0] > 0 else dy.sum(0)
        return dx, dw, db


def level_fused_enabled():
    from .plugin.voxformer import TRAIN_LEVEL_FUSED
    return bool(TRAIN_LEVEL_FUSED["enabled"])


class LayerNormRowsFunction(Function):
    """``F.layer_norm(x, (C,), gamma, beta, eps)`` over rows x [rows, C]: the forward is the inference kernel
    (``sgc_layer_norm_rows``), the backward ``sgc_layer_norm_rows_backward``, which recomputes the row statistics from x."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        x, gamma, beta = x.float().contiguous(), gamma.float().contiguous(), beta.float().contiguous()
        ctx.save_for_backward(x, gamma)
        ctx.eps = float(eps)
        return ext.ops().layer_norm_rows(x, gamma, beta, ctx.eps)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, gamma = ctx.saved_tensors
        if x.shape[0] == 0:
            return torch.zeros_like(x), torch.zeros_like(gamma), torch.zeros_like(gamma), None
        dx, dgamma, dbeta = ext.ops().layer_norm_rows_backward(x, gamma, dy.float().contiguous(), ctx.eps)
        return dx, dgamma, dbeta, None


class SamplingLocationsFunction(Function):
    """``apply(ref, proj, normalizer, M, L, P)`` -> (loc [n, M, L, P, 3], attn [n, M, L, P]): the sampling locations and the
    attention softmax of the deformable attention from the concatenated [uv | depth | logits] projection, in the
    layouts ``PairListDeformAttnFunction`` takes.  Saves attn only; ref and normalizer take no gradient."""

    @staticmethod
    def forward(ctx, ref, proj, normalizer, M, L, P):
        ref, proj, normalizer = ref.float().contiguous(), proj.float().contiguous(), normalizer.float().contiguous()
        ctx.ldp = proj.shape[1]
        if proj.shape[0] == 0:
            loc, attn = proj.new_zeros((0, M, L, P, 3)), proj.new_zeros((0, M, L, P))
        else:
            loc, attn = ext.ops().sampling_locations_forward(ref, proj, normalizer, M, L, P)
        ctx.save_for_backward(attn, normalizer)
        return loc, attn

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loc, grad_attn):
        attn, normalizer = ctx.saved_tensors
        if attn.shape[0] == 0:
            return None, attn.new_zeros((0, ctx.ldp)), None, None, None, None
        grad_loc = torch.zeros(attn.shape + (3,), dtype=attn.dtype, device=attn.device) if grad_loc is None else grad_loc.float().contiguous()
        grad_attn = torch.zeros_like(attn) if grad_attn is None else grad_attn.float().contiguous()
        return None, ext.ops().sampling_locations_backward(attn, grad_loc, grad_attn, normalizer, ctx.ldp), None, None, None, None


class ViewMeanFunction(Function):
    """``apply(per_pair, slot, valid_index, n_valid)`` -> [n_valid, C]: the mean of a voxel's pair rows over the cameras that see
    it (``sgc_view_mean``: the cameras are added in camera order, unlike ``index_add``) and ``sgc_view_mean_backward``."""

    @staticmethod
    def forward(ctx, per_pair, slot, valid_index, n_valid):
        per_pair = per_pair.float().contiguous()
        ctx.save_for_backward(slot, valid_index)
        ctx.n_pairs = per_pair.shape[0]
        if n_valid == 0 or per_pair.shape[0] == 0:
            return per_pair.new_zeros((n_valid, per_pair.shape[1]))
        return ext.ops().view_mean(per_pair, slot, valid_index, n_valid)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_mean):
        slot, valid_index = ctx.saved_tensors
        if grad_mean.shape[0] == 0 or ctx.n_pairs == 0:
            return grad_mean.new_zeros((ctx.n_pairs, grad_mean.shape[1])), None, None, None
        return ext.ops().view_mean_backward(grad_mean.float().contiguous(), slot, valid_index, ctx.n_pairs), None, None, None


class ScatterRowsFunction(Function):
    """``apply(rows, valid_index, Nq)`` -> [Nq, C]: zeros with ``rows`` at the voxels ``valid_index`` (int32, each at most once):
    a zero fill and ``sgc_scatter_rows``; the backward is the gather of those rows (one ``index_select``)."""

    @staticmethod
    def forward(ctx, rows, valid_index, Nq):
        rows = rows.float().contiguous()
        ctx.save_for_backward(valid_index)
        vol = torch.zeros((Nq, rows.shape[1]), dtype=torch.float32, device=rows.device)
        if rows.shape[0]:
            ext.ops().scatter_rows(rows, valid_index, vol)
        return vol

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_vol):
        valid_index, = ctx.saved_tensors
        return grad_vol.index_select(0, valid_index), None, None


def linear_rows(module, x):
    """``module(x)`` for an ``nn.Linear`` with the passes on the HIP kernels when the shapes allow (CUDA fp32, in_features %
    32 == 0, at least a tile of rows); any leading shape."""
    from .plugin.conv_plan import TRAIN_CONV, train_products_ok
    if (TRAIN_CONV != "hip" or not train_products_ok() or not x.is_cuda or x.dtype != torch.float32 or module.in_features % 32
            or x.numel() // max(1, module.in_features) < 128):
        return module(x)
    y = LinearRowsFunction.apply(x.reshape(-1, module.in_features), module.weight, module.bias)
    return y.reshape(*x.shape[:-1], module.out_features)


class ViewAttendFunction(Function):
    """Softmax over the views that see a voxel (``nn.MultiheadAttention`` with query length 1 and a key-padding mask,
    TU/deformable_cross_attention.py:829-833) on the PAIR LIST, forward and backward: q [n_valid, C] (in-projected query of
    every visible voxel), kv [n_pairs, 2C] (k | v in-projected per visible pair), slot [N, Nq] int32 (pair index or -1),
    valid_index [n_valid] int32 -> ctx [n_valid, C] (before out_proj)."""

    @staticmethod
    def forward(ctx_, q, kv, slot, valid_index, heads):
        ops = ext.ops()
        q, kv = q.float().contiguous(), kv.float().contiguous()
        out = ops.view_attend(q, kv, slot, valid_index, heads)
        ctx_.save_for_backward(q, kv, slot, valid_index, out)
        ctx_.heads = heads
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx_, grad_out):
        q, kv, slot, valid_index, out = ctx_.saved_tensors
        gq, gkv = ext.ops().view_attend_backward(q, kv, slot, valid_index, ctx_.heads, out, grad_out.float().contiguous())
        return gq, gkv, None, None, None


# the DFA3D package spells them without the suffix (dfa3D/ops/multi_scale_3D_deform_attn.py:22,67,146)
MultiScale3DDeformableAttnFunction = MultiScale3DDeformableAttnFunction_fp32
MultiScaleDepthScoreSampleFunction = MultiScaleDepthScoreSampleFunction_fp32
WeightedMultiScaleDeformableAttnFunction = WeightedMultiScaleDeformableAttnFunction_fp32
MultiScale3DDeformableAttnFunction_fp16 = MultiScale3DDeformableAttnFunction_fp32
MultiScaleDepthScoreSampleFunction_fp16 = MultiScaleDepthScoreSampleFunction_fp32
WeightedMultiScaleDeformableAttnFunction_fp16 = WeightedMultiScaleDeformableAttnFunction_fp32
