"""``DepthNet_Fusion``: the producer of the depth distribution the view transform consumes.

Reference: mmdet3d_plugin/models/im2voxel/depth_utils/depth_est_fusion.py:166-329 (``DepthNet_Fusion``), :129-164
(``ConvBnReLU2D``, ``SimpleUnet2D``), depth_utils/extractor_matching.py:7-89 (``ResNetFPN``: the 1/4-resolution
matching-feature extractor) and depth_utils/layer_matching.py:107-134 (``BasicBlock``, ``conv1x1`` / ``conv3x3``).
Same ``type=`` name, constructor arguments, call signature ``forward(xs, imgs, img_metas, stride) -> [B, N, D, H, W]``
and state-dict keys, so released checkpoints load (``fnet_mvs.layer2.0.bn3`` and ``...downsample.1`` are the same
BatchNorm registered twice, exactly as in the reference).

What differs on MI355X: in inference the plane-sweep cost volume (homography warp of the K neighbour views at D depth
planes + correlation, :229-240) is ONE fused HIP kernel (``sgc_plane_sweep_corr``, csrc/plane_sweep.hip) -- the warped
features [N, C, D, H, W] (1.18 GB per neighbour at config 2) never exist.  With autograd enabled the same kernel runs
forward and its gradient comes from ``sgc_plane_sweep_corr_backward`` (csrc/plane_sweep_bwd.hip);
``SGC_PLANE_SWEEP_FUSED_GRAD=0`` restores the reference's ``F.grid_sample`` formulation under autograd (A/B runs).  On
the CPU the reference formulation runs.

The 2-D CNNs around the cost volume (``fnet_mvs``, ``fnet_mono``, the three ``SimpleUnet2D`` blocks, ``depth_reg``: about
14 GMAC per view at config 2, twice the arithmetic of the accelerated path behind them) run on the library's MFMA
kernels in eval mode on the GPU without autograd (``_forward_hip``): channels-last rows end to end,
eval BatchNorm and biases folded into the epilogues, the ReLUs, skip additions, the channel concatenation and the softmax
inside the convolution epilogues (``sgc_conv2d_stem7_bf16x3``, ``sgc_conv2d_nhwc_ex_bf16x3``, ``sgc_conv2d_nhwc_bf16x3``).
The result is channels-last in memory, which is what ``SGCDet.depth_pyramid`` and the gathers read in place.  In train mode on
the GPU (with or without autograd) the two feature extractors in front of the regulation U-Nets -- ``fnet_mvs`` and ``fnet_mono``,
half of the module's arithmetic -- run on the same kernels with their BatchNorms live (``_extractors_train_hip``, DESIGN.md 4.14:
``conv_plan.TrainConv2d`` / ``TrainStem7`` layers handed to the one walk ``fnet_mvs_rows``, the stem's weight gradient on
``sgc_conv2d_stem7_wgrad_bf16x3``); the three ``SimpleUnet2D``s, ``depth_reg`` and the softmax keep the torch formulation there, and
``SGC_DEPTH_NET_TRAIN_HIP=0`` restores it for the extractors (on by default: 45.1 against 51.5 ms forward + backward at config 2,
profiles/r18_depth_net_train_bench.json).  ``SGC_DEPTH_NET_TRAIN_UNETS=1`` (opt-in) puts the U-Nets, ``depth_reg`` and
the softmax on the kernels as well (``_regulation_train_hip``: ``_unet`` over ``_unet_train_layers``, rows at 32-column pitch, the live
norms on ``sgc_bn_rows_padded_*``, ``DepthRegSoftmaxFunction``; 37.6 against 44.8 ms, profiles/r22_depth_unets_train_bench.json).  Eval with autograd and CPU tensors keep the torch formulation (library convolutions)
throughout.  ``SGC_DEPTH_NET_HIP=0`` restores
it for the eval forward too (A/B runs); the kernels are the default because the whole-module A/B measured them faster
(6.9 against 16.4 ms per 40-view scene at config 2, profiles/r10_depth_net_bench.json).  A shape the kernels do not take
(an odd map size at a stride-2 stage, ``mono_channels`` not a multiple of 32) runs the torch formulation.
"""
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ext
from ..mmcv_lite import HEADS
from . import conv_plan
from .conv_plan import Conv2dSpec, TrainConv2d, TrainConvTranspose2d, TrainStem7, cached_plan, image_rows, stem7_spec
from .plane_sweep import closest_frame_ids, plane_sweep_correlation


def conv1x1(in_planes, out_planes, stride=1):
    return nn.Conv2d(in_planes, out_planes, kernel_size=1, stride=stride, padding=0)


def conv3x3(in_planes, out_planes, stride=1):
    return nn.Conv2d(in_planes, out_planes, kernel_size=3, stride=stride, padding=1)


class BasicBlock(nn.Module):
    """layer_matching.py:107-134: two 3x3 conv + BN + ReLU, ReLU(x + y) with a 1x1 / BN shortcut when the shape changes."""

    def __init__(self, in_planes, planes, stride=1, norm_layer=nn.BatchNorm2d):
        super().__init__()
        self.conv1 = conv3x3(in_planes, planes, stride)
        self.conv2 = conv3x3(planes, planes)
        self.bn1 = norm_layer(planes)
        self.bn2 = norm_layer(planes)
        self.relu = nn.ReLU(inplace=True)
        if stride == 1 and in_planes == planes:
            self.downsample = None
        else:
            self.bn3 = norm_layer(planes)
            self.downsample = nn.Sequential(conv1x1(in_planes, planes, stride=stride), self.bn3)

    def forward(self, x):
        y = self.relu(self.bn1(self.conv1(x)))
        y = self.relu(self.bn2(self.conv2(y)))
        if self.downsample is not None:
            x = self.downsample(x)
        return self.relu(x + y)


class ResNetFPN(nn.Module):
    """extractor_matching.py:7-89: ResNet-18 stem + layer1 (1/2) + layer2 (1/4) + 1x1 to ``output_dim``."""

    def __init__(self, input_dim=3, output_dim=256, ratio=1.0, norm_layer=nn.BatchNorm2d, init_weight="ImageNet"):
        super().__init__()
        block_dims = [int(d * ratio) for d in (64, 128, 256)]
        self.init_weight = init_weight
        self.input_dim = input_dim
        self.in_planes = 64
        self.conv1 = nn.Conv2d(input_dim, 64, kernel_size=7, stride=2, padding=3)
        self.bn1 = norm_layer(64)
        self.relu = nn.ReLU(inplace=True)
        self.layer1 = self._make_layer(block_dims[0], 1, norm_layer, 2)
        self.layer2 = self._make_layer(block_dims[1], 2, norm_layer, 2)
        self.final_conv_3ddet = conv1x1(block_dims[1], output_dim)
        self._init_weights()

    def _make_layer(self, dim, stride, norm_layer, num):
        layers = [BasicBlock(self.in_planes, dim, stride=stride, norm_layer=norm_layer)]
        layers += [BasicBlock(dim, dim, stride=1, norm_layer=norm_layer) for _ in range(num - 1)]
        self.in_planes = dim
        return nn.Sequential(*layers)

    def _init_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            elif isinstance(m, (nn.BatchNorm2d, nn.InstanceNorm2d, nn.GroupNorm)):
                if m.weight is not None:
                    nn.init.constant_(m.weight, 1)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
        if self.init_weight == "ImageNet":
            # the reference copies torchvision's pretrained resnet18 tensors whose names match (:53-64); torchvision and its
            # weight download are not available in this image -- checkpoints are expected to carry these tensors
            try:
                from torchvision.models import resnet18
                pretrained = resnet18(pretrained=True).state_dict()
                own = self.state_dict()
                own.update({k: v for k, v in pretrained.items() if k in own and v.shape == own[k].shape})
                self.load_state_dict(own, strict=False)
            except Exception:       # noqa: BLE001  (no torchvision / no network: keep the kaiming init)
                pass

    def forward(self, x):
        x = self.relu(self.bn1(self.conv1(x)))
        x = self.layer2(self.layer1(x))
        return self.final_conv_3ddet(x)


class ConvBnReLU2D(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, pad=1):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size, stride=stride, padding=pad, bias=False)
        self.bn = nn.BatchNorm2d(out_channels)

    def forward(self, x):
        return F.relu(self.bn(self.conv(x)), inplace=True)


class SimpleUnet2D(nn.Module):
    """depth_est_fusion.py:139-163: two stride-2 stages down, two transposed 3x3 stages up, additive skips."""

    def __init__(self, in_channel):
        super().__init__()
        c = in_channel
        self.conv1 = ConvBnReLU2D(c, 2 * c, stride=2)
        self.conv2 = ConvBnReLU2D(2 * c, 2 * c)
        self.conv3 = ConvBnReLU2D(2 * c, 4 * c, stride=2)
        self.conv4 = ConvBnReLU2D(4 * c, 4 * c)
        self.conv9 = nn.Sequential(
            nn.ConvTranspose2d(4 * c, 2 * c, kernel_size=3, padding=1, output_padding=1, stride=2, bias=False),
            nn.BatchNorm2d(2 * c), nn.ReLU(inplace=True))
        self.conv11 = nn.Sequential(
            nn.ConvTranspose2d(2 * c, c, kernel_size=3, padding=1, output_padding=1, stride=2, bias=False),
            nn.BatchNorm2d(c), nn.ReLU(inplace=True))

    def forward(self, x):
        conv0 = x
        conv2 = self.conv2(self.conv1(conv0))
        x = self.conv4(self.conv3(conv2))
        x = conv2 + self.conv9(x)
        return conv0 + self.conv11(x)


def homo_warping(src_fea, src_proj, ref_proj, depth_values):
    """Differentiable warp of the neighbour features onto the depth planes of the reference view (:87-126):
    src_fea [B,C,H,W], projections [B,4,4], depth_values [B,D] -> [B,C,D,H,W].  Used only under autograd; inference
    runs the fused kernel."""
    batch, channels, height, width = src_fea.shape
    num_depth = depth_values.shape[1]
    with torch.no_grad():
        proj = torch.matmul(src_proj, torch.inverse(ref_proj))
        rot, trans = proj[:, :3, :3], proj[:, :3, 3:4]
        y, x = torch.meshgrid([torch.arange(0, height, dtype=torch.float32, device=src_fea.device),
                               torch.arange(0, width, dtype=torch.float32, device=src_fea.device)], indexing="ij")
        xyz = torch.stack((x.reshape(-1), y.reshape(-1), torch.ones(height * width, device=src_fea.device)))
        rot_xyz = torch.matmul(rot, xyz.unsqueeze(0).repeat(batch, 1, 1))
        rot_depth_xyz = rot_xyz.unsqueeze(2).repeat(1, 1, num_depth, 1) * depth_values.view(batch, 1, num_depth, 1)
        proj_xyz = rot_depth_xyz + trans.view(batch, 3, 1, 1)
        proj_xy = proj_xyz[:, :2] / proj_xyz[:, 2:3]
        grid = torch.stack((proj_xy[:, 0] / ((width - 1) / 2) - 1, proj_xy[:, 1] / ((height - 1) / 2) - 1), dim=3)
    warped = F.grid_sample(src_fea, grid.view(batch, num_depth * height, width, 2), mode="bilinear", padding_mode="zeros",
                           align_corners=False)
    return warped.view(batch, channels, num_depth, height, width)


HIP_DEFAULT = "1"      # SGC_DEPTH_NET_HIP when the environment does not set it (DESIGN.md 4.10 says how it was chosen)
TRAIN_HIP_DEFAULT = "1"      # SGC_DEPTH_NET_TRAIN_HIP likewise: the feature extractors in train mode
TRAIN_UNETS_DEFAULT = "0"    # SGC_DEPTH_NET_TRAIN_UNETS: the regulation U-Nets, depth_reg and the softmax in train mode too


# ---- the eval-mode plan of the 2-D CNNs: folded, padded, permuted layers (``Conv2dSpec``, on the device of the module) ---------
def _unet_layers(u, in_perm=None, out_perm=None):
    return dict(conv1=Conv2dSpec(u.conv1.conv, u.conv1.bn, in_perm=in_perm), conv2=Conv2dSpec(u.conv2.conv, u.conv2.bn),
                conv3=Conv2dSpec(u.conv3.conv, u.conv3.bn), conv4=Conv2dSpec(u.conv4.conv, u.conv4.bn),
                conv9=Conv2dSpec(u.conv9[0], u.conv9[1]), conv11=Conv2dSpec(u.conv11[0], u.conv11[1], out_perm=out_perm))


def _unet_train_layers(u):
    """``_unet_layers``' training twin: the same six keys, the layers live (``TrainConv2d(pad=True)`` / ``TrainConvTranspose2d``: rows
    at 32-column pitch, the modules held by reference, nothing cached).  ``DepthNet_Fusion._unet`` walks either."""
    d = {k: TrainConv2d(getattr(u, k).conv, getattr(u, k).bn, pad=True) for k in ("conv1", "conv2", "conv3", "conv4")}
    d.update(conv9=TrainConvTranspose2d(u.conv9[0], u.conv9[1]), conv11=TrainConvTranspose2d(u.conv11[0], u.conv11[1]))
    return d


def _block_layers(b, make):
    d = dict(conv1=make(b.conv1, b.bn1), conv2=make(b.conv2, b.bn2))
    if b.downsample is not None:
        d["down"] = make(b.downsample[0], b.downsample[1])   # downsample[1] IS bn3 (registered twice): one layer, folded / normalised once
    return d


def fnet_mvs_plan(f, make, make_stem):
    """The layers of a ``ResNetFPN`` as ``make(conv, bn)`` / ``make_stem(conv, bn)``: ``Conv2dSpec`` and ``stem7_spec`` in eval
    (prepared once, norms folded), ``TrainConv2d`` and ``TrainStem7`` in training (the modules, live).  ``fnet_mvs_rows`` walks it."""
    return dict(stem=make_stem(f.conv1, f.bn1), blocks=[_block_layers(b, make) for b in list(f.layer1) + list(f.layer2)],
                final=make(f.final_conv_3ddet, None))


def fnet_mvs_rows(img, P):
    """THE walk over ``fnet_mvs_plan``'s layers, eval and training: images [N, 3, H, W] -> the matching features as a logical
    NCHW, channels-last-memory view of the final layer's rows.  A layer is called as ``Conv2dSpec`` is, the stem on the images."""
    x, nhw = P["stem"](img)
    for B_ in P["blocks"]:
        y, n1 = B_["conv1"](x, nhw)
        if "down" in B_:
            y, _ = B_["conv2"](y, n1)                                               # relu(bn2(conv2))
            x, _ = B_["down"](x, nhw, residual=y, relu=False, relu_after_add=True)  # relu(bn3(conv1x1(x)) + y)
        else:
            # relu(.) + x with x >= 0: the outer ReLU is a no-op, for the gradient too -- where the sum is 0 both addends are 0 and
            # came through closed ReLU gates, so either formulation sends 0 down both paths
            x, _ = B_["conv2"](y, n1, residual=x)
        nhw = n1
    f, _ = P["final"](x, nhw, relu=False)
    C = P["final"].cout
    return f.view(nhw[0], nhw[1], nhw[2], f.shape[1])[..., :C].permute(0, 3, 1, 2)      # logical NCHW, channels-last memory


def depth_net_plan(net):
    """Every 2-D convolution of ``net`` (a ``DepthNet_Fusion`` in eval mode) as a ``Conv2dSpec``.  The concatenated buffer
    holds [mono_reg (128) | cost_reg (D) | zeros] -- the wide producer at column 0, the narrow one behind it, both starting
    at a multiple of 32 -- so the input channels of ``fusion_regulation.conv1`` and ``depth_reg`` and the output channels of
    ``fusion_regulation.conv11`` (whose skip is that buffer) are permuted to that order here.  ``cat_perm[new] = module index``."""
    D, f = net.depth_channels, net.fnet_mvs
    cat_perm = torch.cat([torch.arange(D, D + 128), torch.arange(D)]).to(net.depth_reg.weight.device)
    return dict(**fnet_mvs_plan(f, Conv2dSpec, stem7_spec),
                corr=_unet_layers(net.correlation_regulation), fnet_mono=Conv2dSpec(net.fnet_mono.conv, net.fnet_mono.bn),
                mono=_unet_layers(net.mono_regulation), fusion=_unet_layers(net.fusion_regulation, in_perm=cat_perm, out_perm=cat_perm),
                depth_reg=Conv2dSpec(net.depth_reg, in_perm=cat_perm, pad_out=False), cat_perm=cat_perm)


@HEADS.register_module()
class DepthNet_Fusion(nn.Module):
    def __init__(self, neighbor_img_num, downsample_factor, dbound, mono_channels=256, loss_weight=0.5, max_tol=0,
                 init_weight="ImageNet"):
        super().__init__()
        self.fp16_enabled = False
        self.max_tol = max_tol
        self.downsample_factor = downsample_factor
        self.loss_weight = loss_weight
        self.neighbor_img_num = neighbor_img_num
        self.dbound = dbound
        self.depth_channels = round((dbound[1] - dbound[0]) / dbound[2])
        self.depth_values = np.arange(dbound[0], dbound[1], dbound[2], dtype=np.float32) + dbound[2] / 2   # bin centres
        self.fnet_mvs = ResNetFPN(input_dim=3, output_dim=128, ratio=1.0, norm_layer=nn.BatchNorm2d, init_weight=init_weight)
        self.correlation_regulation = SimpleUnet2D(in_channel=self.depth_channels)
        self.fnet_mono = ConvBnReLU2D(in_channels=mono_channels, out_channels=128)
        self.mono_regulation = SimpleUnet2D(in_channel=128)
        self.fusion_regulation = SimpleUnet2D(in_channel=self.depth_channels + 128)
        self.depth_reg = nn.Conv2d(self.depth_channels + 128, self.depth_channels, kernel_size=3, stride=1, padding=1)

    def correlation(self, f_mvs, img_meta, stride):
        """Plane-sweep matching cost [N, D, H, W] of the N views against their time-adjacent neighbours (:219-240)."""
        num_src, channel_num, H, W = f_mvs.shape
        k = min(self.neighbor_img_num, num_src - 1)
        needs_grad = torch.is_grad_enabled() and f_mvs.requires_grad
        if f_mvs.is_cuda and not (needs_grad and os.environ.get("SGC_PLANE_SWEEP_FUSED_GRAD", "1") == "0"):
            return plane_sweep_correlation(f_mvs, img_meta, stride, self.depth_values, self.neighbor_img_num)
        dev = f_mvs.device
        src_w2c = torch.tensor(np.array(img_meta["lidar2img"]["extrinsic"]), device=dev)
        intr = torch.tensor(np.array(img_meta["lidar2img"]["intrinsic"]), device=dev).clone()
        ratio = img_meta["ori_shape"][0] / (img_meta["img_shape"][0] / stride)
        if intr.dim() == 2:
            intr[:2] /= ratio
            intr = intr.unsqueeze(0).repeat(num_src, 1, 1)
        else:
            intr[:, :2] /= ratio
        neighbor_ids = closest_frame_ids(num_src, k)
        proj = torch.matmul(intr, src_w2c)
        depth_values = torch.tensor(self.depth_values, device=dev).unsqueeze(0).repeat(num_src, 1)
        corr = torch.zeros((num_src, self.depth_channels, H, W), device=dev)
        for j in range(k):
            warped = homo_warping(f_mvs[neighbor_ids[:, j]], proj[neighbor_ids[:, j]], proj, depth_values)
            corr = corr + (warped * f_mvs.unsqueeze(2)).sum(dim=1) / torch.sqrt(torch.tensor(channel_num).float())
        return corr / k

    # ---- eval mode on the GPU: every 2-D convolution on the MFMA kernels, channels-last rows --------------------------
    def _hip_ok(self, xs, imgs):
        """The shapes ``_forward_hip`` takes: images 4x the map, every stride-2 stage on an even size."""
        H, W = xs.shape[-2:]
        return (xs.dim() == 5 and imgs.dim() == 5 and imgs.shape[2] == 3 and tuple(imgs.shape[-2:]) == (4 * H, 4 * W)
                and H % 4 == 0 and W % 4 == 0 and xs.shape[2] % 32 == 0 and self.depth_channels % 4 == 0
                and self.depth_channels <= 32 and xs.dtype == torch.float32 and imgs.dtype == torch.float32)

    def _unet(self, x, U, nhw, out=None, col0=0):
        """SimpleUnet2D on rows, eval (``_unet_layers``) and training (``_unet_train_layers``): conv0 + conv11(conv2 +
        conv9(conv4(conv3(conv2(conv1(conv0)))))); the skips ride in the epilogues of the transposed layers (in training: in the passes of
        their norms), the last of which may, in eval, write a column range of a wider buffer."""
        c1, n2 = U["conv1"](x, nhw)
        c2, _ = U["conv2"](c1, n2)
        c3, n4 = U["conv3"](c2, n2)
        c4, _ = U["conv4"](c3, n4)
        u2, _ = U["conv9"](c4, n4, residual=c2)
        y, _ = U["conv11"](u2, n2, residual=x, out=out, col0=col0)
        return y

    def _fnet_mvs_hip(self, img, P):
        return fnet_mvs_rows(img, P)

    def _forward_hip(self, xs, imgs, img_metas, stride):
        ops = ext.ops()
        P = cached_plan(self, lambda: depth_net_plan(self))
        B, N, C, H, W = xs.shape
        D = self.depth_channels
        out = torch.empty((B, N, H, W, D), dtype=torch.float32, device=xs.device)
        nhw = (N, H, W)
        catw = P["fusion"]["conv1"].w.shape[2]
        for b, (x, img, img_meta) in enumerate(zip(xs, imgs, img_metas)):
            f_mvs = self._fnet_mvs_hip(img, P)
            corr = plane_sweep_correlation(f_mvs, img_meta, stride, self.depth_values, self.neighbor_img_num)
            cat = torch.empty((N * H * W, catw), dtype=torch.float32, device=xs.device)
            self._unet(ops.nchw_to_nhwc_padc(corr, 32), P["corr"], nhw, out=cat, col0=128)     # columns 128..159: cost_reg | zeros
            m, _ = P["fnet_mono"](image_rows(x)[0], nhw)
            self._unet(m, P["mono"], nhw, out=cat, col0=0)                                       # columns 0..127: mono_reg
            fused = self._unet(cat, P["fusion"], nhw)
            P["depth_reg"](fused, nhw, relu=False, out=out[b].view(N * H * W, D), softmax_cols=D)
        return out.permute(0, 1, 4, 2, 3)                     # [B, N, D, H, W]; every [N, D, H, W] slice channels-last in memory

    # ---- train mode on the GPU: the two feature extractors on the kernels, live BatchNorm ----------
    def _train_hip_ok(self, xs, imgs):
        """Does the train-mode forward run ``fnet_mvs`` and ``fnet_mono`` on the kernels?  Train mode with or without autograd (a
        ``no_grad`` call in train mode computes the numbers of the training step), fp32 GPU tensors of the shapes ``_forward_hip``
        takes, images that need no gradient (the stem has no input gradient), an arithmetic mode the training Functions accept,
        and no ``SGC_DEPTH_NET_TRAIN_HIP=0``."""
        return (self.training and xs.is_cuda and imgs.is_cuda and not imgs.requires_grad
                and os.environ.get("SGC_DEPTH_NET_TRAIN_HIP", TRAIN_HIP_DEFAULT) != "0"
                and conv_plan.CONV_MODE == "bf16x3" and conv_plan.train_products_ok() and self._hip_ok(xs, imgs))

    def _extractors_train_hip(self, x, img):
        """(f_mvs, fnet_mono(x)) of one scene as logical-NCHW, channels-last-memory views of the kernels' rows.  The layers are built
        per forward and only point at the modules: nothing outlives a ``convert_sync_batchnorm`` that replaces the norms."""
        from ..functions import NchwToRowsFunction
        f_mvs = fnet_mvs_rows(img, fnet_mvs_plan(self.fnet_mvs, TrainConv2d, TrainStem7))
        N, C, H, W = x.shape
        if x.is_contiguous(memory_format=torch.channels_last) and x.dtype == torch.float32:
            rows = x.permute(0, 2, 3, 1).reshape(N * H * W, C)
        else:
            rows = NchwToRowsFunction.apply(x).view(N * H * W, C)
        m, _ = TrainConv2d(self.fnet_mono.conv, self.fnet_mono.bn)(rows, (N, H, W))
        return f_mvs, m.view(N, H, W, m.shape[1]).permute(0, 3, 1, 2)

    # ---- train mode on the GPU, opt-in: the U-Nets, depth_reg and the softmax on the kernels as well ----------
    def _train_unets_ok(self):
        """With ``_train_hip_ok``: ``SGC_DEPTH_NET_TRAIN_UNETS=1``, every U-Net norm a plain ``nn.BatchNorm2d`` with parameters (a
        converted SyncBatchNorm keeps the torch formulation for the U-Nets), the norm's HIP passes switched on, and ``depth_reg`` as
        the reference builds it."""
        if os.environ.get("SGC_DEPTH_NET_TRAIN_UNETS", TRAIN_UNETS_DEFAULT) != "1":
            return False
        if not (conv_plan.TRAIN_CONV == "hip" and conv_plan.BN_ON_HIP and conv_plan.BN_FUSE_TAIL):
            return False
        norms = [m for u in (self.correlation_regulation, self.mono_regulation, self.fusion_regulation) for m in u.modules()
                 if isinstance(m, nn.modules.batchnorm._NormBase)]
        reg = self.depth_reg
        return (len(norms) == 18 and all(type(m) is nn.BatchNorm2d and m.weight is not None and m.bias is not None for m in norms)
                and reg.bias is not None and reg.kernel_size == (3, 3) and reg.stride == (1, 1) and reg.padding == (1, 1))

    def _regulation_train_hip(self, f_mvs, mono, img_meta, stride):
        """The part of one scene's forward behind the extractors, on rows: cost volume -> ``correlation_regulation``; ``mono`` ->
        ``mono_regulation``; [cost_reg D | mono_reg 128 | zeros] -> ``fusion_regulation`` -> ``depth_reg`` + softmax.  Returns the
        probabilities as a logical [N, D, H, W], channels-last-memory view.  The concatenation is the module's channel order (no
        permutation) as a ``torch.cat`` of rows; the hand-over of the NCHW cost volume is ``NchwToRowsFunction``."""
        from ..functions import DepthRegSoftmaxFunction, NchwToRowsFunction
        N, _, H, W = mono.shape
        D, nhw = self.depth_channels, (N, H, W)
        corr = self.correlation(f_mvs, img_meta, stride)                                       # [N, D, H, W]
        corr_rows = F.pad(NchwToRowsFunction.apply(corr).view(N * H * W, D), (0, conv_plan._pad_to(D) - D))
        cost_reg = self._unet(corr_rows, _unet_train_layers(self.correlation_regulation), nhw)
        mono_reg = self._unet(mono.permute(0, 2, 3, 1).reshape(N * H * W, -1), _unet_train_layers(self.mono_regulation), nhw)
        c = D + mono_reg.shape[1]
        cat = torch.cat([cost_reg[:, :D], mono_reg, mono_reg.new_zeros((N * H * W, conv_plan._pad_to(c) - c))], dim=1)
        fused = self._unet(cat, _unet_train_layers(self.fusion_regulation), nhw)
        p = DepthRegSoftmaxFunction.apply(fused, self.depth_reg.weight, self.depth_reg.bias, nhw)
        return p.view(N, H, W, D).permute(0, 3, 1, 2)

    def forward(self, xs, imgs, img_metas, stride):
        """xs [B,N,C,H,W] (finest FPN map), imgs [B,N,3,4H,4W], img_metas list of B dicts -> depth probability
        [B,N,D,H,W] (softmax over the D bins).  Eval mode on the GPU without autograd: ``_forward_hip`` (the result is
        channels-last in memory).  Train mode on the GPU: the feature extractors on the kernels (``_extractors_train_hip``), the
        U-Nets, ``depth_reg`` and the softmax in the torch formulation below -- or, with ``SGC_DEPTH_NET_TRAIN_UNETS=1``, on the kernels
        too (``_regulation_train_hip``); everything else is the torch formulation throughout."""
        if (not self.training and not torch.is_grad_enabled() and xs.is_cuda and imgs.is_cuda
                and os.environ.get("SGC_DEPTH_NET_HIP", HIP_DEFAULT) != "0" and self._hip_ok(xs, imgs)):
            return self._forward_hip(xs, imgs, img_metas, stride)
        train_hip = self._train_hip_ok(xs, imgs)
        train_unets = train_hip and self._train_unets_ok()
        B, num_src, C, H, W = xs.shape
        depth_preds = torch.empty((B, num_src, self.depth_channels, H, W), device=xs.device)
        for b, (x, img, img_meta) in enumerate(zip(xs, imgs, img_metas)):
            if train_unets:
                depth_preds[b] = self._regulation_train_hip(*self._extractors_train_hip(x, img), img_meta, stride)
                continue
            if train_hip:
                f_mvs, mono = self._extractors_train_hip(x, img)
                cost_reg = self.correlation_regulation(self.correlation(f_mvs, img_meta, stride))
                mono_reg = self.mono_regulation(mono)
            else:
                f_mvs = self.fnet_mvs(img)
                cost_reg = self.correlation_regulation(self.correlation(f_mvs, img_meta, stride))
                mono_reg = self.mono_regulation(self.fnet_mono(x))
            prob = self.depth_reg(self.fusion_regulation(torch.cat([cost_reg, mono_reg], dim=1)))
            depth_preds[b] = F.softmax(prob, dim=1)
        return depth_preds

    def get_downsampled_gt_depth(self, gt_depths):
        """[B,N,H,W] metric depth maps -> [B*N*h*w, D] one-hot bins at feature resolution (:254-296): min over every
        ds x ds patch ignoring zeros, bin index (d - (near - step)) / step, out-of-range -> no bin."""
        ds = self.downsample_factor
        if ds % 1 == 0:
            ds = int(ds)
            B, N, H, W = gt_depths.shape
            g = gt_depths.view(B * N, H // ds, ds, W // ds, ds, 1).permute(0, 1, 3, 5, 2, 4).contiguous().view(-1, ds * ds)
            g = torch.where(g == 0.0, 1e5 * torch.ones_like(g), g)
            g = torch.min(g, dim=-1).values.view(B * N, H // ds, W // ds)
        else:
            g = F.interpolate(gt_depths, scale_factor=1 / ds, mode="nearest")
            B, N, H, W = g.shape
            g = g.view(B * N, H, W)
        g = (g - (self.dbound[0] - self.dbound[2])) / self.dbound[2]
        g = torch.where((g < self.depth_channels + 1) & (g >= 0.0), g, torch.zeros_like(g))
        onehot = F.one_hot(g.long(), num_classes=self.depth_channels + 1).view(-1, self.depth_channels + 1)[:, 1:]
        return self.error_tol(onehot).float()

    def error_tol(self, onehot_):
        if self.max_tol < 1:
            return onehot_
        padding = onehot_.new_zeros(onehot_.shape[0], 1)
        onehot = onehot_.clone()
        for error in range(-self.max_tol, self.max_tol + 1):
            if error < 0:
                onehot = onehot + torch.cat([onehot[..., 1:], padding], dim=-1)
            elif error > 0:
                onehot = onehot + torch.cat([padding, onehot[..., :-1]], dim=-1)
        return onehot / (onehot + 1e-5)

    def loss(self, depth_labels, depth_preds):
        """BCE between the predicted distribution and the one-hot depth bin on pixels that have a label (:314-329)."""
        if depth_labels.dim() == 3:
            depth_labels = depth_labels.unsqueeze(0)
        labels = self.get_downsampled_gt_depth(depth_labels)
        preds = depth_preds.float().permute(0, 1, 3, 4, 2).contiguous().view(-1, self.depth_channels)
        fg = torch.max(labels, dim=1).values > 0.0
        preds = torch.clamp(preds, min=1e-7, max=1 - 1e-7)
        depth_loss = F.binary_cross_entropy(preds[fg], labels[fg], reduction="none").sum() / max(1.0, fg.sum())
        return {"loss_dpt": self.loss_weight * depth_loss}
