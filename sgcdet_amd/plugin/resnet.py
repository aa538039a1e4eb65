"""``ResNet``: the 2-D image backbone of the SGCDet configs, images -> the four maps the FPN reads.

Reference call site: ``x = self.backbone(img)`` (detectors/SGCDet.py:65) with ``backbone=dict(type='ResNet', depth=50,
num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=1, norm_cfg=dict(type='BN', requires_grad=False), norm_eval=True,
style='pytorch', pretrained='torchvision://resnet50')`` in all four configs (configs/SGCDet_ScanNet.py:73-83).  The class is
mmdet's (v2.x ``mmdet/models/backbones/resnet.py``), which is NOT vendored in the reference tree: its semantics are restated
here from the published module and are *unpinned*.  State-dict keys are mmdet's, which are torchvision's: ``conv1.weight``,
``bn1.*``, ``layer{1..4}.{i}.conv{1,2,3}.weight``, ``layer....bn{1,2,3}.*``, ``layer....downsample.{0,1}.*``; there is no ``fc``.

``pretrained`` / ``init_cfg`` are kept and NEVER fetched: ``torchvision://...`` names a download, and this module opens no
network connection (nor is torchvision needed).  Weights come from checkpoints (``load_state_dict``).

Eval mode on the GPU without autograd (``_forward_hip``) runs every layer on the library's kernels over
channels-last rows: the stem on ``sgc_conv2d_stem7_bf16x3``, the pooling on ``sgc_maxpool2d_nhwc``, every block's
convolutions on the image tile kernels with eval BatchNorm folded into the epilogues and the ReLUs / skip additions inside
them; stride-2 layers over maps with an odd side (15 x 20 -> 8 x 10 at the reference geometry) on
``sgc_conv2d_nhwc_strided_bf16x3``.  The returned maps are logical NCHW and channels-last in memory: ``FPN._forward_hip``
reads them in place.  ``SGC_BACKBONE_HIP=0`` restores the torch formulation for the eval forward (A/B runs).  An image with an
odd side, ``in_channels != 3``, ``base_channels != 64`` or a non-fp32 input runs the torch formulation as well.

Training under autograd with every norm frozen -- the reference configuration: ``frozen_stages=1``, ``norm_eval=True``,
``norm_cfg.requires_grad=False`` -- runs on the kernels too (``_forward_hip_train``), and it IS the eval
forward: one plan builder (``resnet_plan``), one block walker (``run_block``) and one forward (``_run_hip``) serve both, and
every layer reaches its entry point through ``conv_plan.conv2d_rows``.  The frozen prefix (stem, pooling, leading blocks
without a trainable parameter) is ``Conv2dSpec``s under ``no_grad``; from the first trainable block on every layer is a
``conv_plan.FrozenConv2d`` (``functions.FrozenNormConv2dFunction``) -- the same folded scale / shift and fused ReLU / skip
epilogues, the input gradient on the forward kernels and the weight gradient on ``sgc_conv2d_wgrad_bf16x3``.
``SGC_BACKBONE_TRAIN_HIP=0`` keeps the torch formulation; a norm in training mode or with trainable parameters, a trainable
stem, CPU tensors and the fp16 arithmetic mode take it as well.
"""
import os

import torch
import torch.nn as nn

from .. import ext
from ..mmcv_lite import BACKBONES, BaseModule
from . import conv_plan
from .conv_plan import Conv2dSpec, FrozenConv2d, cached_plan, stem7_spec

HIP_DEFAULT = "1"      # SGC_BACKBONE_HIP when the environment does not set it (DESIGN.md 4.11 says how it was chosen)
TRAIN_HIP_DEFAULT = "1"      # SGC_BACKBONE_TRAIN_HIP when the environment does not set it (DESIGN.md 4.12 says how it was chosen)


def _norm(channels, norm_cfg):
    cfg = dict(norm_cfg)
    if cfg.pop("type") not in ("BN", "BN2d"):
        raise NotImplementedError("ResNet: norm_cfg type 'BN' only")
    requires_grad = cfg.pop("requires_grad", True)
    bn = nn.BatchNorm2d(channels, **cfg)
    for p in bn.parameters():
        p.requires_grad = requires_grad
    return bn


class BasicBlock(nn.Module):
    """mmdet ``BasicBlock``: 3x3 (stride) / BN / ReLU, 3x3 / BN, + identity, ReLU."""
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None, norm_cfg=dict(type="BN")):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn1 = _norm(planes, norm_cfg)
        self.conv2 = nn.Conv2d(planes, planes, 3, padding=1, bias=False)
        self.bn2 = _norm(planes, norm_cfg)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample

    @property
    def last_norm(self):
        return self.bn2

    def forward(self, x):
        identity = x if self.downsample is None else self.downsample(x)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        return self.relu(out + identity)


class Bottleneck(nn.Module):
    """mmdet ``Bottleneck`` with ``style='pytorch'``: 1x1 / 3x3 (stride) / 1x1 to 4 x planes, + identity, ReLU."""
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None, norm_cfg=dict(type="BN")):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = _norm(planes, norm_cfg)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn2 = _norm(planes, norm_cfg)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = _norm(planes * 4, norm_cfg)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample

    @property
    def last_norm(self):
        return self.bn3

    def forward(self, x):
        identity = x if self.downsample is None else self.downsample(x)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        return self.relu(out + identity)


def _block_layers(b, make):
    """One residual block as ``make(conv, norm)`` layers -- ``Conv2dSpec`` (eval BatchNorm folded, weight prepared) or
    ``FrozenConv2d`` (the same fold, the live weight under autograd): ``conv3`` only in a Bottleneck, ``down`` only with a
    projection shortcut."""
    d = dict(conv1=make(b.conv1, b.bn1), conv2=make(b.conv2, b.bn2))
    if isinstance(b, Bottleneck):
        d["conv3"] = make(b.conv3, b.bn3)
    if b.downsample is not None:
        d["down"] = make(b.downsample[0], b.downsample[1])
    return d


def resnet_plan(net, n_frozen=None):
    """Every convolution of ``net`` as the kernels take it: the stem (``stem7_spec``) and, per stage, the blocks' layers.  The
    first ``n_frozen`` blocks are ``Conv2dSpec``s, the rest ``FrozenConv2d``s; None: all prepared (the eval plan)."""
    stages, i = [], 0
    for name in net.res_layers:
        stages.append([_block_layers(b, Conv2dSpec if n_frozen is None or i + j < n_frozen else FrozenConv2d)
                       for j, b in enumerate(getattr(net, name))])
        i += len(stages[-1])
    return dict(stem=stem7_spec(net.conv1, net.bn1), stages=stages)


def run_block(B, x, nhw, keep=None):
    """A planned block on rows ``x`` [N*H*W, C]: returns (rows, (N, OH, OW)).  THE layer order and epilogues of the HIP path, in
    eval and in training alike (the layers of ``B`` are ``Conv2dSpec``s or ``FrozenConv2d``s; tests/test_resnet_cpu.py replays
    them with torch convolutions): the last convolution carries the skip addition and the ReLU behind it; a projection shortcut
    is a convolution of its own without a ReLU.  ``keep``: a list that receives every layer's output rows in the order they are
    computed (conv1, [conv2,] down, last)."""
    def layer(name, *args, **kw):
        y, n = B[name](*args, **kw)
        if keep is not None:
            keep.append(y)
        return y, n

    y, n1 = layer("conv1", x, nhw)                                                 # relu(bn1(conv1))
    if "conv3" in B:
        y, n1 = layer("conv2", y, n1)                                              # relu(bn2(conv2)): the stride sits here
    identity = layer("down", x, nhw, relu=False)[0] if "down" in B else x
    last = "conv3" if "conv3" in B else "conv2"
    return layer(last, y, n1, residual=identity, relu=False, relu_after_add=True)[0], n1       # relu(bn(conv) + identity)


@BACKBONES.register_module()
class ResNet(BaseModule):
    arch_settings = {18: (BasicBlock, (2, 2, 2, 2)), 34: (BasicBlock, (3, 4, 6, 3)),
                     50: (Bottleneck, (3, 4, 6, 3)), 101: (Bottleneck, (3, 4, 23, 3))}

    def __init__(self, depth, in_channels=3, stem_channels=None, base_channels=64, num_stages=4, strides=(1, 2, 2, 2),
                 dilations=(1, 1, 1, 1), out_indices=(0, 1, 2, 3), style="pytorch", deep_stem=False, avg_down=False,
                 frozen_stages=-1, conv_cfg=None, norm_cfg=dict(type="BN", requires_grad=True), norm_eval=True, dcn=None,
                 stage_with_dcn=(False, False, False, False), plugins=None, with_cp=False, zero_init_residual=True,
                 pretrained=None, init_cfg=None):
        super().__init__(init_cfg)
        if depth not in self.arch_settings:
            raise KeyError(f"invalid depth {depth} for resnet")
        for name, unused in (("deep_stem", deep_stem), ("avg_down", avg_down), ("dcn", dcn is not None), ("plugins", plugins is not None),
                             ("with_cp", with_cp), ("conv_cfg", conv_cfg is not None), ("style='caffe'", style != "pytorch"),
                             ("dilations != 1", any(d != 1 for d in dilations[:num_stages]))):
            if unused:
                raise NotImplementedError(f"ResNet: {name} is not used by the SGCDet configs and not restated")
        if not 1 <= num_stages <= 4 or len(strides) < num_stages or max(out_indices) >= num_stages:
            raise ValueError("ResNet: needs 1 <= num_stages <= 4, a stride per stage and out_indices below num_stages")
        self.depth, self.in_channels, self.base_channels, self.num_stages = depth, in_channels, base_channels, num_stages
        self.stem_channels = stem_channels or base_channels
        self.strides, self.out_indices, self.style = tuple(strides), tuple(out_indices), style
        self.frozen_stages, self.norm_cfg, self.norm_eval = frozen_stages, dict(norm_cfg), norm_eval
        self.zero_init_residual = zero_init_residual
        self.pretrained = pretrained          # kept, never fetched
        block, stage_blocks = self.arch_settings[depth]
        self.block = block

        self.conv1 = nn.Conv2d(in_channels, self.stem_channels, 7, stride=2, padding=3, bias=False)
        self.bn1 = _norm(self.stem_channels, norm_cfg)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.res_layers = []
        inplanes = self.stem_channels
        for i, n_blocks in enumerate(stage_blocks[:num_stages]):
            planes = base_channels * 2 ** i
            layers = []
            for j in range(n_blocks):
                stride = strides[i] if j == 0 else 1
                downsample = None
                if stride != 1 or inplanes != planes * block.expansion:
                    downsample = nn.Sequential(nn.Conv2d(inplanes, planes * block.expansion, 1, stride=stride, bias=False),
                                               _norm(planes * block.expansion, norm_cfg))
                layers.append(block(inplanes, planes, stride=stride, downsample=downsample, norm_cfg=norm_cfg))
                inplanes = planes * block.expansion
            name = f"layer{i + 1}"
            self.add_module(name, nn.Sequential(*layers))
            self.res_layers.append(name)
        self.feat_dim = inplanes
        self._freeze_stages()

    def init_weights(self):
        """mmdet's default initialisation (kaiming convolutions, unit norms, the last norm of every block zeroed with
        ``zero_init_residual``).  ``pretrained`` / ``init_cfg`` name weights to download: they are not fetched."""
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        if self.zero_init_residual:
            for m in self.modules():
                if isinstance(m, (BasicBlock, Bottleneck)):
                    nn.init.constant_(m.last_norm.weight, 0)
        self._is_init = True

    def _freeze_stages(self):
        if self.frozen_stages >= 0:
            self.bn1.eval()
            for m in (self.conv1, self.bn1):
                for p in m.parameters():
                    p.requires_grad = False
        for i in range(1, min(self.frozen_stages, self.num_stages) + 1):
            m = getattr(self, f"layer{i}")
            m.eval()
            for p in m.parameters():
                p.requires_grad = False

    def train(self, mode=True):
        super().train(mode)
        self._freeze_stages()
        if mode and self.norm_eval:
            for m in self.modules():
                if isinstance(m, nn.modules.batchnorm._BatchNorm):
                    m.eval()
        return self

    # ---- reference formulation (any device, autograd) ----------------------------------------------------------
    def _forward_torch(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        outs = []
        for i, name in enumerate(self.res_layers):
            x = getattr(self, name)(x)
            if i in self.out_indices:
                outs.append(x)
        return tuple(outs)

    # ---- MFMA kernels on channels-last rows ----------------------------------------------------------------------
    def _hip_ok(self, x):
        no_bn_training = not any(m.training for m in self.modules() if isinstance(m, nn.modules.batchnorm._BatchNorm))
        return (x.dim() == 4 and x.dtype == torch.float32 and x.shape[1] == 3 and self.in_channels == 3
                and self.base_channels == 64 and self.stem_channels == 64 and x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0
                and all(s in (1, 2) for s in self.strides[:self.num_stages]) and no_bn_training and conv_plan.CONV_MODE == "bf16x3")

    def _run_hip(self, img, P, n_frozen, keep=None):
        """Plan ``P`` on images: stem, pooling, the blocks through ``run_block`` -- those below ``n_frozen`` under ``no_grad`` --
        and the ``out_indices`` maps.  ``keep``: see ``run_block``; it receives the layers of the blocks from ``n_frozen`` on."""
        ops = ext.ops()
        N, _, Hi, Wi = img.shape
        st = P["stem"]
        with torch.no_grad():
            x = ops.conv2d_stem7_bf16x3(img.contiguous(), st.w_hi, st.w_lo, scale=st.scale, shift=st.shift, relu=True)
            x, nhw = ops.maxpool2d_nhwc(x, (N, Hi // 2, Wi // 2))
        outs, i = [], 0
        for s, blocks in enumerate(P["stages"]):
            for B in blocks:
                if i < n_frozen:
                    with torch.no_grad():
                        x, nhw = run_block(B, x, nhw)
                else:
                    x, nhw = run_block(B, x, nhw, keep)
                i += 1
            if s in self.out_indices:
                outs.append(x.view(nhw[0], nhw[1], nhw[2], x.shape[1]).permute(0, 3, 1, 2))   # logical NCHW, channels-last memory
        return tuple(outs)

    def _forward_hip(self, img):
        return self._run_hip(img, cached_plan(self, lambda: resnet_plan(self)), len(self.blocks()))

    # ---- training with frozen norms: the eval lowering under autograd ---------------------------------------
    def blocks(self):
        """The residual blocks in forward order."""
        return [b for name in self.res_layers for b in getattr(self, name)]

    def frozen_prefix(self):
        """How many leading blocks have no parameter that requires a gradient (they run the eval lowering in training)."""
        n = 0
        for b in self.blocks():
            if any(p.requires_grad for p in b.parameters()):
                break
            n += 1
        return n

    def _train_hip_config_ok(self):
        """The tensor-independent part of the training-path predicate: training mode, every norm frozen (eval statistics, no
        trainable parameter), a frozen stem, the bf16 weight planes' arithmetic modes and the environment switch."""
        norms = [m for m in self.modules() if isinstance(m, nn.modules.batchnorm._BatchNorm)]
        return (self.training and self.frozen_stages >= 0 and not any(p.requires_grad for p in self.conv1.parameters())
                and not any(m.training for m in norms) and not any(p.requires_grad for m in norms for p in m.parameters())
                and conv_plan.CONV_MODE == "bf16x3" and conv_plan.train_products_ok()
                and os.environ.get("SGC_BACKBONE_TRAIN_HIP", TRAIN_HIP_DEFAULT) != "0")

    def _forward_hip_train(self, img, keep=None):
        """The training forward on the kernels (see the module docstring): ``resnet_plan`` with the frozen prefix prepared and
        every later layer a ``FrozenConv2d``.  The plan is rebuilt when a tensor of the prefix or of a norm changes -- not when
        a trainable weight does: those are read through ``train_weight_planes()`` every step.  ``keep``: a list that receives
        the output rows of every trainable layer in layer order (their signs are the ReLU gates of the backward)."""
        nf = self.frozen_prefix()
        norms = [m for m in self.modules() if isinstance(m, nn.modules.batchnorm._BatchNorm)]
        watched = ([self.conv1.weight] + [t for b in self.blocks()[:nf] for t in b.parameters()]
                   + [t for m in norms for t in list(m.parameters()) + list(m.buffers())])
        fp = (conv_plan.CONV_PRODUCTS, nf) + tuple((t.data_ptr(), t._version) for t in watched)
        P = cached_plan(self, lambda: resnet_plan(self, nf), attr="_hip_train_plan", fingerprint=fp)
        return self._run_hip(img, P, nf, keep)

    def forward(self, x):
        """img [B*N, 3, H, W] -> the ``out_indices`` maps [B*N, C_l, H_l, W_l].  Eval mode on the GPU without autograd:
        ``_forward_hip``; training under autograd with frozen norms: ``_forward_hip_train`` (both return maps that are
        channels-last in memory); otherwise the torch formulation."""
        if (self.training and torch.is_grad_enabled() and x.is_cuda and not x.requires_grad and self._train_hip_config_ok()
                and self._hip_ok(x)):
            return self._forward_hip_train(x)
        if (not self.training and not torch.is_grad_enabled() and x.is_cuda
                and os.environ.get("SGC_BACKBONE_HIP", HIP_DEFAULT) != "0" and self._hip_ok(x)):
            return self._forward_hip(x)
        return self._forward_torch(x)
