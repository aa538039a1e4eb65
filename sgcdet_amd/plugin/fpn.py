"""Image FPN whose output convolutions EMIT the layout the view transformation consumes.

Reference call site: ``x = list(self.neck(x))`` (detectors/SGCDet.py:67) with ``neck=dict(type='FPN',
in_channels=[256, 512, 1024, 2048], out_channels=embed_dims, num_outs=4)`` (configs/SGCDet_ScanNet.py:84-88); the maps are
then reshaped to [B, N, C, H, W] (:68-69) and every level is flattened / permuted to [N, H*W, C] per use
(TU/transformer.py:151-170).  The class itself is mmdet's (v2.x ``mmdet/models/necks/fpn.py``), which is NOT vendored in
the reference tree: its semantics are restated here from the published module (lateral 1x1 convolutions with bias, top-down
nearest upsampling to the finer level's size + addition, 3x3 output convolutions with bias; extra levels by stride-2
max-pool subsampling of the last output) and are *unpinned*; state-dict keys are mmdet's
(``lateral_convs.{i}.conv.{weight,bias}``, ``fpn_convs.{i}.conv.{weight,bias}``).

Eval mode on the GPU (``forward`` with CUDA inputs, no grad) runs every convolution on ``sgc_conv2d_nhwc_bf16x3`` over
channels-last rows and returns [N, C, H, W] tensors that ARE channels-last in memory (``y.permute(0, 3, 1, 2)`` of the
[N, H, W, C] result): `SGCDet.forward_features` reads them in place, the NCHW -> NHWC pass of the path disappears, and
nothing else changes for the caller.  Backbone maps that arrive channels-last in memory are read in place too; NCHW ones
are transposed once by ``sgc_nchw_to_nhwc_crop``.

Under autograd on the GPU (``_train_hip_ok``) the same walk runs with every convolution a ``conv_plan.BiasConv2d``
(``functions.FrozenNormConv2dFunction`` with a trainable bias: forward, input, weight and bias gradients on the HIP kernels) and
the top-down step a ``functions.UpsampleNearestAddFunction``; the outputs have the eval path's layout and bits.
``SGC_FPN_TRAIN_HIP=0`` keeps the torch formulation.
"""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ext
from ..mmcv_lite import NECKS
from . import conv_plan
from .conv_plan import BiasConv2d, Conv2dSpec, cached_plan, image_rows

TRAIN_HIP_DEFAULT = "1"      # SGC_FPN_TRAIN_HIP when the environment does not set it (DESIGN.md 4.13 says how it was chosen)


class _ConvModule(nn.Module):
    """mmcv ``ConvModule`` without norm / activation: a Conv2d with bias under the key ``conv``."""

    def __init__(self, cin, cout, k):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, k, padding=k // 2)

    def forward(self, x):
        return self.conv(x)


def _nearest_index(dst, src, device):
    """source index of F.interpolate(mode='nearest') for every destination index: floor(d * src / dst)."""
    return torch.div(torch.arange(dst, device=device) * src, dst, rounding_mode="floor").clamp_(max=src - 1)


@NECKS.register_module()
class FPN(nn.Module):
    def __init__(self, in_channels, out_channels, num_outs, start_level=0, end_level=-1, add_extra_convs=False,
                 relu_before_extra_convs=False, no_norm_on_lateral=False, conv_cfg=None, norm_cfg=None, act_cfg=None,
                 upsample_cfg=dict(mode="nearest"), init_cfg=None):
        super().__init__()
        if add_extra_convs or norm_cfg is not None or act_cfg is not None or conv_cfg is not None:
            raise NotImplementedError("FPN: only the plain configuration of the SGCDet configs is restated")
        if upsample_cfg.get("mode", "nearest") != "nearest" or "scale_factor" in upsample_cfg:
            raise NotImplementedError("FPN: nearest upsampling to the finer level's size only")
        self.in_channels, self.out_channels, self.num_outs = list(in_channels), out_channels, num_outs
        self.start_level = start_level
        self.backbone_end_level = len(in_channels) if end_level in (-1, len(in_channels) - 1) else end_level + 1
        self.lateral_convs = nn.ModuleList(_ConvModule(in_channels[i], out_channels, 1)
                                           for i in range(start_level, self.backbone_end_level))
        self.fpn_convs = nn.ModuleList(_ConvModule(out_channels, out_channels, 3)
                                       for _ in range(start_level, self.backbone_end_level))

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.xavier_uniform_(m.weight)
                nn.init.zeros_(m.bias)

    # ---- reference formulation (any device, autograd) ----------------------------------------------------------
    def _forward_torch(self, inputs):
        lat = [conv(inputs[i + self.start_level]) for i, conv in enumerate(self.lateral_convs)]
        for i in range(len(lat) - 1, 0, -1):
            lat[i - 1] = lat[i - 1] + F.interpolate(lat[i], size=lat[i - 1].shape[2:], mode="nearest")
        outs = [conv(lat[i]) for i, conv in enumerate(self.fpn_convs)]
        while len(outs) < self.num_outs:
            outs.append(F.max_pool2d(outs[-1], 1, stride=2))
        return tuple(outs)

    # ---- MFMA kernels on channels-last rows ----------------------------------------------------------------------
    def _build_plan(self, make=None):
        """The layers as the walker calls them: ``Conv2dSpec`` (eval: bias only, no norm to fold; channel counts are multiples
        of 32, see ``forward``) or ``make(conv)`` (training: ``BiasConv2d``)."""
        if make is None:
            def make(conv):
                return Conv2dSpec(conv, pad_in=False, pad_out=False, unit_scale=False)
        return [make(m.conv) for m in self.lateral_convs], [make(m.conv) for m in self.fpn_convs]

    @staticmethod
    def _top_down(fine, coarse, dims_fine, dims_coarse, train):
        """Nearest upsample of ``coarse`` to the finer size, added to ``fine``: in place without autograd, the Function with it."""
        if train:
            from ..functions import UpsampleNearestAddFunction
            return UpsampleNearestAddFunction.apply(fine, coarse, dims_fine, dims_coarse)
        return ext.ops().upsample_nearest_add_nhwc(fine, coarse, dims_fine, dims_coarse, out=fine)

    def _forward_hip(self, inputs, train=False):
        """THE walk over the layers, in eval and in training alike.  ``train``: the layers are ``BiasConv2d``s (the parameters
        are read live, so that plan never goes stale) and the inputs become rows under autograd -- a view of a map that is
        channels-last in memory, the copy torch makes of an NCHW-contiguous one."""
        if train:
            lat_layers, out_layers = cached_plan(self, lambda: self._build_plan(BiasConv2d), attr="_hip_train_plan", fingerprint=())
        else:
            lat_layers, out_layers = cached_plan(self, self._build_plan)
        lat, dims = [], []
        for i, layer in enumerate(lat_layers):
            x = inputs[i + self.start_level]
            if train:
                N, Cin, H, W = x.shape
                rows, nhw = x.permute(0, 2, 3, 1).reshape(N * H * W, Cin), (N, H, W)
            else:
                rows, nhw = image_rows(x)
            lat.append(layer(rows, nhw, relu=False)[0])
            dims.append(nhw)
        C = self.out_channels
        for i in range(len(lat) - 1, 0, -1):
            lat[i - 1] = self._top_down(lat[i - 1], lat[i], dims[i - 1], dims[i], train)
        outs = []
        for i, layer in enumerate(out_layers):
            N, H, W = dims[i]
            y, _ = layer(lat[i], dims[i], relu=False)
            outs.append(y.view(N, H, W, C).permute(0, 3, 1, 2))          # logical NCHW, channels-last memory
        while len(outs) < self.num_outs:
            outs.append(outs[-1][:, :, ::2, ::2])
        return tuple(outs)

    def _channels_ok(self):
        return all(c % 32 == 0 for c in self.in_channels) and self.out_channels % 32 == 0

    def _train_hip_ok(self, inputs):
        """Does this call train on the HIP kernels?  Autograd is recording and something here wants a gradient;
        the maps the module reads are CUDA float32; every channel count is a multiple of 32; the weight planes' arithmetic mode
        (not fp16); and the environment switch."""
        used = inputs[self.start_level:self.backbone_end_level]
        return (torch.is_grad_enabled()
                and (any(x.requires_grad for x in used) or any(p.requires_grad for p in self.parameters()))
                and all(x.is_cuda and x.dtype == torch.float32 for x in used) and self._channels_ok()
                and conv_plan.CONV_MODE == "bf16x3" and conv_plan.train_products_ok()
                and os.environ.get("SGC_FPN_TRAIN_HIP", TRAIN_HIP_DEFAULT) != "0")

    def forward(self, inputs):
        x0 = inputs[0]
        if self._train_hip_ok(inputs):
            return self._forward_hip(inputs, train=True)
        if not self.training and not torch.is_grad_enabled() and x0.is_cuda and self._channels_ok():
            return self._forward_hip(inputs)
        return self._forward_torch(inputs)
