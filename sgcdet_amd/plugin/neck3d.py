"""``FastIndoorImVoxelNeck``: dense 3D residual U-Net over the voxel volume.

Reference: mmdet3d_plugin/models/necks/imvoxelnet.py:8-67 (neck), :146-173 (BasicBlock3dV2).
State-dict keys are the reference's: ``down_layer_{i}.{b}.{conv1,norm1,conv2,norm2,
downsample.0,downsample.1}``, ``up_block_{i}.{0,1,3,4}``, ``out_block_{i}.{0,1}``.

"Sparse" in SGCDet means sparse QUERIES; the volume entering the neck is dense (every voxel
carries the upsampled coarse feature, AdaptiveSparseHead.py:77-82), so the convolutions
stay dense -- a submanifold-sparse convolution would change the results (SURVEY.md
section 0, fact 3).

On the GPU the network is described once (``_build_plan(make)``) and walked once (``_run``): eval hands the walker prepared
``ConvSpec`` layers (cached), training ``TrainConv3d`` layers over the live modules; the torch modules at the end of ``forward`` are
the reference formulation and the path for everything else.
"""
import functools

import torch
from torch import nn

from ..mmcv_lite import NECKS
from .conv_plan import TrainConv3d, cached_plan, conv_spec, rows_to_ncdhw, to_channels_last_rows, train_conv_on_hip


class BasicBlock3dV2(nn.Module):
    def __init__(self, in_channels, out_channels, stride=1):
        super().__init__()
        self.stride = stride
        self.conv1 = nn.Conv3d(in_channels, out_channels, 3, stride, 1, bias=False)
        self.norm1 = nn.BatchNorm3d(out_channels)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv3d(out_channels, out_channels, 3, 1, 1, bias=False)
        self.norm2 = nn.BatchNorm3d(out_channels)
        if stride != 1:
            self.downsample = nn.Sequential(nn.Conv3d(in_channels, out_channels, 1, stride, bias=False),
                                            nn.BatchNorm3d(out_channels))

    def forward(self, x):
        out = self.relu(self.norm1(self.conv1(x)))
        out = self.norm2(self.conv2(out))
        skip = self.downsample(x) if self.stride != 1 else x
        return self.relu(out + skip)


def _conv_bn_relu(cin, cout):
    return nn.Sequential(nn.Conv3d(cin, cout, 3, 1, 1, bias=False), nn.BatchNorm3d(cout), nn.ReLU(inplace=True))


@NECKS.register_module()
class FastIndoorImVoxelNeck(nn.Module):
    def __init__(self, in_channels, n_blocks, out_channels):
        super().__init__()
        self.n_scales = len(n_blocks)
        width = in_channels
        for i, nb in enumerate(n_blocks):
            stride = 1 if i == 0 else 2
            blocks = []
            for b in range(nb):
                if b == 0 and stride != 1:
                    blocks.append(BasicBlock3dV2(width, width * 2, stride))
                    width *= 2
                else:
                    blocks.append(BasicBlock3dV2(width, width))
            setattr(self, f"down_layer_{i}", nn.Sequential(*blocks))
            if i > 0:
                setattr(self, f"up_block_{i}", nn.Sequential(
                    nn.ConvTranspose3d(width, width // 2, 2, 2, bias=False), nn.BatchNorm3d(width // 2),
                    nn.ReLU(inplace=True),
                    nn.Conv3d(width // 2, width // 2, 3, 1, 1, bias=False), nn.BatchNorm3d(width // 2),
                    nn.ReLU(inplace=True)))
            setattr(self, f"out_block_{i}", _conv_bn_relu(width, out_channels))

    # ---- lowering onto the HIP kernels: the network described once, walked once ---------------------
    def _build_plan(self, make):
        """The layers as ``make(conv, bn)``: ``conv_spec`` in eval (prepared once: norm folded into the MFMA kernel's epilogue),
        ``TrainConv3d`` in training (the modules, live: SURVEY.md 8 f-3, every convolution pass and the BatchNorm on the kernels)."""
        plan = {}
        for i in range(self.n_scales):
            plan[f"down_{i}"] = [dict(c1=make(blk.conv1, blk.norm1), c2=make(blk.conv2, blk.norm2),
                                      ds=make(blk.downsample[0], blk.downsample[1]) if blk.stride != 1 else None)
                                 for blk in getattr(self, f"down_layer_{i}")]
            if i > 0:
                up = getattr(self, f"up_block_{i}")
                plan[f"up_{i}"] = (make(up[0], up[1]), make(up[3], up[4]))
            ob = getattr(self, f"out_block_{i}")
            plan[f"out_{i}"] = make(ob[0], ob[1])
        return plan

    def _run(self, x, plan, tail_masks=None):
        """The one walk over ``plan`` (imvoxelnet.py:22-34,146-173), eval and training.  ``tail_masks`` (eval) = (mask for
        up_block_1's 3x3x3, mask for out_block_0), uint8 [X*Y*Z] of the finest grid: the only layers whose outputs feed nothing but
        the finest head scale (x1 also feeds the next ConvTranspose, so every coarser layer stays dense).  Live rows are
        bit-identical to the dense launch."""
        rows, grid = to_channels_last_rows(x)
        skips = []
        for i in range(self.n_scales):
            for b in plan[f"down_{i}"]:
                h, g1 = b["c1"](rows, grid, relu=1)
                skip = rows if b["ds"] is None else b["ds"](rows, grid)[0]
                rows, grid = b["c2"](h, g1, residual=skip, relu=1)                        # relu(norm2(conv2) + identity)
            skips.append((rows, grid))
        outs = []
        for i in reversed(range(self.n_scales)):
            if i < self.n_scales - 1:
                up_t, up_c = plan[f"up_{i + 1}"]
                h, g = up_t(rows, grid, relu=1)
                m_up = tail_masks[0] if (tail_masks is not None and i == 0) else None
                rows, grid = up_c(h, g, residual=skips[i][0], relu=2, out_mask=m_up)      # relu(bn(conv)) + skip
            layer = plan[f"out_{i}"]
            m_out = tail_masks[1] if (tail_masks is not None and i == 0) else None
            o, g = layer(rows, grid, relu=1, out_mask=m_out)
            outs.append(rows_to_ncdhw(o, g, layer.cout))
        return outs[::-1]

    def forward(self, x, tail_masks=None):
        """[B,C,nx,ny,nz] -> [out@1x, out@1/2, out@1/4], finest first (imvoxelnet.py:22-34).  In training the norms see the statistics of
        the batch (the reference's 2-GPU SyncBN step on one device); ``tail_masks`` for B > 1: one pair per scene."""
        if not self.training and not torch.is_grad_enabled() and x.is_cuda:
            plan = cached_plan(self, lambda: self._build_plan(conv_spec))
            if x.shape[0] == 1:
                return self._run(x, plan, tail_masks)
            # eval norms couple nothing: the single-scene lowering scene by scene (Winograd, masks and graphs as they are), bit-identical
            # to B separate calls
            per = [self._run(x[b:b + 1], plan, None if tail_masks is None else tail_masks[b]) for b in range(x.shape[0])]
            return [torch.cat(level) for level in zip(*per)]
        if train_conv_on_hip(x, [m.in_channels for m in self.modules() if isinstance(m, (nn.Conv3d, nn.ConvTranspose3d))]):
            # built per forward, never cached: the layers only point at the modules, and a cached list would outlive a
            # convert_sync_batchnorm that replaces the norms
            return self._run(x, self._build_plan(functools.partial(TrainConv3d, scenes=x.shape[0])))
        # library convolutions: the voxel head hands over a channels-last strided view, for which MIOpen has only its
        # naive_conv_*_nonpacked kernels (2.6 s per config-2 step instead of ~0.1 s)
        x = x.contiguous()
        skips = []
        for i in range(self.n_scales):
            x = getattr(self, f"down_layer_{i}")(x)
            skips.append(x)
        outs = []
        for i in reversed(range(self.n_scales)):
            if i < self.n_scales - 1:
                x = skips[i] + getattr(self, f"up_block_{i + 1}")(x)
            outs.append(getattr(self, f"out_block_{i}")(x))
        return outs[::-1]

    def init_weights(self):
        pass
