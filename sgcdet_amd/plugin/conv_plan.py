"""What the eval-mode lowerings of the plugin modules share: a module's layers prepared once for the library's kernels.

``ConvSpec`` (3-D: neck and head, ``sgc_conv3d_cl_*`` / Winograd-z), ``Conv2dSpec`` (2-D: backbone, FPN and depth net),
``LinearSpec`` and ``BlockDiagSpec`` (the row GEMMs of the transformer) each hold one layer as the kernels take it and dispatch
it in ``__call__``.  ``conv2d_rows`` is the one rule that sends a 2-D layer to ``sgc_conv2d_nhwc_bf16x3`` /
``sgc_conv2d_nhwc_ex_bf16x3`` / ``sgc_conv2d_nhwc_strided_bf16x3``: ``Conv2dSpec`` and its training twins ``FrozenConv2d`` (frozen
norm, autograd) and ``BiasConv2d`` (no norm, trainable bias) all reach the entries through it, so the training forward is the eval forward.
``TrainConv3d`` is ``ConvSpec``'s training twin (convolution Function + ``bn_rows`` with a live norm and the fused tail): both are built
by ``make(conv, bn)`` (``conv_spec`` for eval), so the neck walks one plan in either mode; ``TrainConv2d`` and ``TrainStem7`` are the
same for ``Conv2dSpec`` and ``Stem7Spec`` (the depth net's feature extractors with their live norms); ``TrainConv2d(pad=True)`` and
``TrainConvTranspose2d`` are the layers of its regulation U-Nets, on rows zero-padded to 32 columns.  Eval BatchNorm (running statistics)
and the bias are folded into a per-channel scale / shift for the kernel's epilogue (``fold_norm``, the only copy), weights are
permuted once to ``[tap][Cout][Cin]``, and channel counts are zero-padded to multiples of 32 (the K tile; ``_pad_to``) with zero
weight rows, scale 1 and shift 0, so padded output columns are exactly 0.  ``cached_plan`` keeps a module's plan and rebuilds it
when ``module_fingerprint`` changes: a parameter or buffer was updated in place (``Tensor._version``) or moved, or the
arithmetic mode was switched.  ``image_rows`` / ``to_channels_last_rows`` bring NCHW / NCDHW tensors to the channels-last rows
the kernels read.  The process-wide switches (arithmetic mode, Winograd-z, throughput geometry, training path) live here too.
"""
import os

import torch

from .. import ext

_PAD = 32

# "bf16x3": fp32 operands split hi/lo onto the bf16 matrix cores (fp32-faithful to ~1e-5, default);
# "f32": exact fp32 products on the fp32 MFMA (5x slower matrix pipe).  Both are tested against the oracle.
# "bf16" / "fp16" (opt-in, BASELINE.json configs #2 "bf16" / #5 "fp16"): the bf16x3 code path with ONE product per multiply-add
# -- both operands rounded to bfloat16 (sgc_set_conv_products(1)) or to IEEE half (2; v_mfma_f32_32x32x16_f16: the same rate,
# 11 instead of 8 significant bits, operands saturated at +-65504), fp32 accumulate; 1/3 of the matrix work, NOT parity-exact:
# their own bench lines, never the headline.  CONV_MODE stays "bf16x3" (same kernels, same launch sequence); CONV_PRODUCTS says
# which.  Call set_conv_mode BEFORE the modules prepare their weight plans (the planes hold bf16 or half bits accordingly).
CONV_MODE = "bf16x3"
CONV_PRODUCTS = 3


def set_conv_mode(mode):
    global CONV_MODE, CONV_PRODUCTS
    if mode not in ("bf16x3", "f32", "bf16", "fp16"):
        raise ValueError(mode)
    CONV_MODE = "bf16x3" if mode in ("bf16", "fp16") else mode
    CONV_PRODUCTS = {"bf16": 1, "fp16": 2}.get(mode, 3)
    import torch
    if torch.cuda.is_available():
        ext.ops().lib.call("sgc_set_conv_products", CONV_PRODUCTS)


# Winograd F(2,3) along z for the wide 3x3x3 stride-1 layers (sgc_conv3d_winograd_z_bf16x3): 2/3 of the multiply-adds of
# the layers that hold the chip at its power limit, at the price of a transform pass on either side.  "auto" = wherever the entry
# point supports the shape (z extent a multiple of 8; the library tiles a slice with bricks of 8 x 8 or 10 x 10 pixels, whichever
# issues fewer matrix rows: 40 x 40 takes the first, 20 x 20 the second) and the layer has at least WINOGRAD_Z_MIN_CH input
# channels; False = never.  Results differ from the direct kernel by summation order
# (<= 2e-5 of the tensor scale, tested); each choice is deterministic.  Set before the first forward: plans are cached.
WINOGRAD_Z = {"0": False, "1": True}.get(os.environ.get("SGC_WINOGRAD_Z", ""), "auto")
WINOGRAD_Z_MIN_CH = int(os.environ.get("SGC_WINOGRAD_Z_MIN_CH", "256"))
# the 10 x 10 x 4 scale (z extent 4: one 2-image x 10 x 10 brick per position, reduction split over the channel slices): opt-in, see
# ConvSpec._winograd_planes and DESIGN.md 7.4 (per-layer A/B with four scenes in flight, profiles/r15_wz_bricks_layers_ab.txt: neither
# 1024 -> 1024 nor 1024 -> 128 gains, so both keep the direct kernels by default)
WINOGRAD_Z_Z4 = os.environ.get("SGC_WINOGRAD_Z_Z4", "0") == "1"
WINOGRAD_Z_RAGGED = os.environ.get("SGC_WINOGRAD_Z_RAGGED", "1") != "0"     # also slices that are no multiple of 8 x 8 pixels (20 x 20: 10 x 10 bricks)
# layers that keep the direct kernel although "auto" would give them the form: (Cin, Cout, gx, gy, gz) tuples, from per-layer A/B runs
# with scenes in flight (profiles/r06_winograd_layers_ab.txt).  Env (A/B runs): SGC_WINOGRAD_Z_DENY="512:128:20:20:8,512:512:20:20:8"
WINOGRAD_Z_DENY = {tuple(int(v) for v in item.split(":")) for item in os.environ.get("SGC_WINOGRAD_Z_DENY", "").split(",") if item}


def set_winograd_z(mode, min_channels=None):
    global WINOGRAD_Z, WINOGRAD_Z_MIN_CH
    if mode not in ("auto", True, False):
        raise ValueError(mode)
    WINOGRAD_Z = mode
    if min_channels is not None:
        WINOGRAD_Z_MIN_CH = int(min_channels)


def _pad_to(n, m=_PAD):
    return (n + m - 1) // m * m


def fold_norm(cout, bn=None, bias=None, device=None):
    """(scale, shift) [cout] of a convolution's epilogue: eval BatchNorm ``y = (x - mean) / sqrt(var + eps) * gamma + beta``
    behind it with the convolution's bias folded in; without a norm: (1, bias)."""
    if bn is None:
        shift = bias.detach().float() if bias is not None else torch.zeros(cout, dtype=torch.float32, device=device)
        return torch.ones(cout, dtype=torch.float32, device=device), shift
    scale = bn.weight.detach().float() / torch.sqrt(bn.running_var.detach().float() + bn.eps)
    shift = bn.bias.detach().float() - bn.running_mean.detach().float() * scale
    if bias is not None:
        shift = shift + bias.detach().float() * scale
    return scale, shift


class ConvSpec:
    """One prepared convolution: wt [taps, Cout_p, Cin_p], scale/shift [Cout_p]."""

    def __init__(self, weight, bn=None, bias=None, ksize=3, stride=1, transposed=False, pad_out=True):
        w = weight.detach().float()
        if transposed:                       # nn.ConvTranspose3d weight [Cin, Cout, 2, 2, 2]
            cin, cout = w.shape[0], w.shape[1]
            wt = w.permute(2, 3, 4, 1, 0).reshape(8, cout, cin)
        else:                                # nn.Conv3d weight [Cout, Cin, k, k, k]
            cout, cin = w.shape[0], w.shape[1]
            wt = w.permute(2, 3, 4, 0, 1).reshape(ksize ** 3, cout, cin)
        cin_p = _pad_to(cin)
        cout_p = _pad_to(cout) if pad_out else _pad_to(cout, 4)
        wp = torch.zeros((wt.shape[0], cout_p, cin_p), dtype=torch.float32, device=w.device)
        wp[:, :cout, :cin] = wt
        scale = torch.ones(cout_p, dtype=torch.float32, device=w.device)
        shift = torch.zeros(cout_p, dtype=torch.float32, device=w.device)
        scale[:cout], shift[:cout] = fold_norm(cout, bn, bias, w.device)
        self.wt, self.scale, self.shift = wp.contiguous(), scale, shift
        self.w_hi, self.w_lo = ext.ops().split_operand(self.wt) if w.is_cuda else (None, None)
        self.cin, self.cout, self.cin_p, self.cout_p = cin, cout, cin_p, cout_p
        self.ksize, self.stride, self.transposed = ksize, stride, transposed
        self._wino = None                    # (g_hi, g_lo): transformed weight planes, built on first use

    def _winograd_planes(self, grid):
        """The transformed weight planes when this call should take the Winograd-z form, else None.

        Grids of z extent 4 (the 10 x 10 x 4 scale of config 2: 1024 -> 1024 and 1024 -> 128) pass only with ``WINOGRAD_Z_Z4`` and
        where the library supports the shape.  Their transformed planes are larger than the direct ones: 1024 -> 1024 holds
        4 x 9 x 1024^2 x 4 B = 151 MB (bf16 hi + lo) against 27 x 1024^2 x 4 B = 113 MB, built once per module."""
        if (WINOGRAD_Z is False or self.ksize != 3 or self.stride != 1 or self.transposed or CONV_MODE != "bf16x3"
                or (WINOGRAD_Z == "auto" and self.cin_p < WINOGRAD_Z_MIN_CH)
                or (not WINOGRAD_Z_RAGGED and (grid[0] % 8 or grid[1] % 8))):
            return None
        if (self.cin_p, self.cout_p) + tuple(grid) in WINOGRAD_Z_DENY or (grid[2] < 8 and not WINOGRAD_Z_Z4):
            return None
        ops = ext.ops()
        if not ops.conv3d_winograd_z_supported(grid, self.cin_p, self.cout_p):
            return None
        # The transform-domain launch has Z/8 x ceil(X/8) x ceil(Y/8) bricks per position x 4 positions x ceil(Cout/128) column tiles
        # and no reduction split.  A layer ALONE needs enough of them to fill the chip (512 -> 128 @ 20x20x8: 36 workgroups, 154 us
        # against 55 us direct); with scenes in flight the other streams fill it and the saved multiply-adds count (+2 % at config 2).
        if WINOGRAD_Z == "auto" and not WINOGRAD_IN_FLIGHT:
            wgs = -(-grid[2] // 8) * -(-grid[0] // 8) * -(-grid[1] // 8) * 4 * -(-self.cout_p // 128)
            if wgs < 192:
                return None
        if self._wino is None:
            self._wino = ops.split_operand(ops.winograd_z_weights(self.wt))
        return self._wino

    def __call__(self, x, grid, residual=None, relu=0, out_mask=None, act=None):
        """``out_mask`` (uint8 [OV], bf16x3 mode, 3x3x3 stride-1 layers): only rows with 1 are needed downstream.
        ``act`` = (c0, c1, scale tensor): columns [c0, c1) leave as exp(v * scale) (bf16x3 mode; the caller applies it itself in
        the strict-fp32 mode -- ``supports_act``)."""
        if CONV_MODE == "bf16x3":
            wino = self._winograd_planes(grid) if out_mask is None and act is None else None
            if wino is not None:
                return ext.ops().conv3d_winograd_z(x, wino[0], wino[1], grid, self.scale, self.shift, residual, relu)
            return ext.ops().conv3d_cl_bf16x3(x, self.w_hi, self.w_lo, grid, self.ksize, self.stride,
                                              self.transposed, self.scale, self.shift, residual, relu, out_mask=out_mask, act=act)
        if act is not None:
            raise NotImplementedError("the output activation lives in the bf16x3 convolution's epilogue")
        return ext.ops().conv3d_cl(x, self.wt, grid, self.ksize, self.stride, self.transposed, self.scale,
                                   self.shift, residual, relu)


def conv_spec(conv, bn=None):
    """``ConvSpec`` of an ``nn.Conv3d`` / ``nn.ConvTranspose3d`` module and the norm behind it: kernel size, stride, form and bias
    are the module's, so the eval layer and its training twin ``TrainConv3d`` are both built by ``make(conv, bn)``."""
    return ConvSpec(conv.weight, bn, bias=conv.bias, ksize=conv.kernel_size[0], stride=conv.stride[0],
                    transposed=isinstance(conv, torch.nn.ConvTranspose3d))


class Conv2dSpec:
    """One prepared 2-D convolution, the twin of ``ConvSpec`` for image rows: w [k*k, Cout_p, Cin_p] (tap = kh*k + kw, rows =
    output channels; a ConvTranspose2d's [Cin, Cout, k, k] parameter is transposed, not flipped: the kernel sums by output
    parity), scale / shift [Cout_p].  Channels are reordered by ``in_perm`` / ``out_perm`` (new index -> module index), then
    zero-padded to a multiple of 32 (``pad_in`` / ``pad_out`` = False: that dimension stays as it is), so the padded output
    columns of every layer are exactly 0 (zero weight rows, scale 1, shift 0).  ``unit_scale=False``: a layer without a norm
    has ``scale = None`` (the kernels' own no-scale epilogue) instead of a vector of ones."""

    def __init__(self, conv, bn=None, in_perm=None, out_perm=None, pad_in=True, pad_out=True, unit_scale=True):
        self.transposed = isinstance(conv, torch.nn.ConvTranspose2d)
        w = conv.weight.detach().float()
        w = w.permute(2, 3, 1, 0) if self.transposed else w.permute(2, 3, 0, 1)          # [k, k, Cout, Cin]
        scale, shift = fold_norm(w.shape[2], bn, conv.bias, w.device)
        if in_perm is not None:
            w = w[..., in_perm]
        if out_perm is not None:
            w, scale, shift = w[:, :, out_perm], scale[out_perm], shift[out_perm]
        k, _, cout, cin = w.shape
        dout, din = (_pad_to(cout) - cout if pad_out else 0), (_pad_to(cin) - cin if pad_in else 0)
        pad = torch.nn.functional.pad
        self.scale = pad(scale, (0, dout), value=1.0).contiguous() if bn is not None or unit_scale else None
        self.shift = pad(shift, (0, dout)).contiguous()
        self.k, self.stride, self.cin, self.cout = k, conv.stride[0], cin, cout
        self.set_weight(pad(w.reshape(k * k, cout, cin), (0, din, 0, dout)).contiguous())

    def set_weight(self, w):
        """``w`` as the entry point reads it; its operand planes are split where the kernels run (a plan stays constructible on the CPU)."""
        self.w = w
        self.w_hi, self.w_lo = ext.ops().split_operand(w) if w.is_cuda else (None, None)

    def __call__(self, x, nhw, residual=None, relu=True, relu_after_add=False, out=None, col0=0, softmax_cols=0):
        """The layer on rows ``x`` through ``conv2d_rows``; returns (rows, (N, OH, OW))."""
        N, H, W = nhw
        s = self.stride
        onhw = (N, 2 * H, 2 * W) if self.transposed else (N, (H + s - 1) // s, (W + s - 1) // s)
        return conv2d_rows(x, self.w_hi, self.w_lo, nhw, self.k, s, self.transposed, self.scale, self.shift, residual, relu,
                           relu_after_add, out, col0, softmax_cols), onhw


def conv2d_rows(x, w_hi, w_lo, nhw, k, stride=1, transposed=False, scale=None, shift=None, residual=None, relu=True,
                relu_after_add=False, out=None, col0=0, softmax_cols=0):
    """THE dispatch of a 2-D layer on rows ``x`` [N*H*W, Cin] with planes [k*k, Cout, Cin] to its forward entry; returns the
    output rows.  ``Conv2dSpec`` (eval) and ``FrozenNormConv2dFunction`` (training: its forward and its input gradients) both
    come through here, so one layer takes one entry in both.  In this order: a stride-2 layer over a map with an odd side ->
    ``sgc_conv2d_nhwc_strided_bf16x3`` (output ceil(H / 2) x ceil(W / 2), the ResNet stages: DESIGN.md 4.11); a plain stride-1
    layer -> ``sgc_conv2d_nhwc_bf16x3`` (`relu` = 0: no ReLU; 1: ReLU; 2: ReLU, then the skip); everything else -- transposed,
    ReLU behind the skip, an ``out`` buffer, a wider residual, a softmax -> ``sgc_conv2d_nhwc_ex_bf16x3``."""
    ops = ext.ops()
    if stride == 2 and not transposed and (nhw[1] % 2 or nhw[2] % 2):
        return ops.conv2d_nhwc_strided_bf16x3(x, w_hi, w_lo, nhw, k, stride=stride, scale=scale, shift=shift, residual=residual,
                                              relu=relu, relu_after_add=relu_after_add, out=out, col0=col0, softmax_cols=softmax_cols)
    if (stride == 1 and not transposed and out is None and not relu_after_add and softmax_cols == 0
            and (residual is None or residual.shape[1] == w_hi.shape[1])):
        mode = (2 if residual is not None else 1) if relu else 0
        return ops.conv2d_nhwc_bf16x3(x, w_hi, w_lo, nhw, k, scale=scale, shift=shift, residual=residual, relu=mode)
    return ops.conv2d_nhwc_ex_bf16x3(x, w_hi, w_lo, nhw, k, stride=stride, transposed=transposed, scale=scale, shift=shift,
                                     residual=residual, relu=relu, relu_after_add=relu_after_add, out=out, col0=col0,
                                     softmax_cols=softmax_cols)


class Stem7Spec(Conv2dSpec):
    """The prepared 7x7 stride-2 stem.  Called on the NCHW images: ``relu(norm(conv(img)))`` as rows, (N, H / 2, W / 2)."""

    def __call__(self, img):
        N, _, H, W = img.shape
        y = ext.ops().conv2d_stem7_bf16x3(img.contiguous(), self.w_hi, self.w_lo, scale=self.scale, shift=self.shift, relu=True)
        return y, (N, H // 2, W // 2)


def stem7_spec(conv, bn):
    """The 7x7 stride-2 stem as ``sgc_conv2d_stem7_bf16x3`` reads it: [49, 64, 3] -> the [64, 160] matrix, column
    (ci * 7 + kh) * 7 + kw, 147..159 zero."""
    stem = Stem7Spec(conv, bn, pad_in=False)
    stem.set_weight(torch.nn.functional.pad(stem.w.permute(1, 2, 0).reshape(64, 147), (0, 13)).contiguous())
    return stem


class FrozenConv2d:
    """To training what ``Conv2dSpec`` is to eval, with its call signature: an ``nn.Conv2d`` with a FROZEN norm behind it,
    under autograd (``functions.FrozenNormConv2dFunction``).  Holds the module -- its weight is read live through
    ``train_weight_planes()`` at every call -- and the folded (scale, shift)."""

    def __init__(self, conv, bn):
        self.conv = conv
        self.scale, self.shift = (t.contiguous() for t in fold_norm(conv.out_channels, bn, conv.bias, conv.weight.device))

    def __call__(self, x, nhw, residual=None, relu=True, relu_after_add=False):
        from ..functions import FrozenNormConv2dFunction
        s = self.conv.stride[0]
        y = FrozenNormConv2dFunction.apply(x, self.conv.weight, self.scale, self.shift, residual, nhw, s, relu, relu_after_add)
        return y, (nhw[0], (nhw[1] + s - 1) // s, (nhw[2] + s - 1) // s)


class BiasConv2d:
    """``FrozenConv2d``'s sibling for a convolution WITHOUT a norm whose bias trains (the image FPN): stride 1,
    no activation.  Weight and bias are the module's parameters, read live at every call -- the weight through
    ``train_weight_planes()``, the bias as the epilogue's shift -- and both get gradients from ``FrozenNormConv2dFunction``."""

    def __init__(self, conv):
        if conv.bias is None or conv.stride[0] != 1:
            raise ValueError("BiasConv2d: a stride-1 convolution with a bias")
        self.conv = conv

    def __call__(self, x, nhw, residual=None, relu=False, relu_after_add=False):
        from ..functions import FrozenNormConv2dFunction
        if relu or relu_after_add:
            raise NotImplementedError("BiasConv2d: no activation (its gate would have to be saved)")
        y = FrozenNormConv2dFunction.apply(x, self.conv.weight, None, None, residual, nhw, 1, False, False, self.conv.bias)
        return y, tuple(nhw)


# training / autograd path of the neck and head convolutions: "hip" = forward, input and weight gradients on the MFMA
# kernels (functions.ChannelsLastConv3dFunction), "library" = torch's convolutions (MIOpen) as in round 1
TRAIN_CONV = os.environ.get("SGC_TRAIN_CONV", "hip")
BN_ON_HIP = os.environ.get("SGC_BN_HIP", "1") != "0"      # training-mode BatchNorm of the neck on sgc_bn_rows_* (0: torch's kernels)
BN_FUSE_TAIL = os.environ.get("SGC_BN_FUSE_TAIL", "1") != "0"   # `+ identity` / ReLU behind a BatchNorm inside its passes (0: torch ops, A/B)
# OPT-IN (env SGC_SYNCBN_ROWS_HIP=1): a training-mode dist.SyncBatchNorm3d of the neck on the sgc_bn_rows_sync_* kernels with the fused
# tail, one collective per pass (functions.SyncBatchNormRowsFunction); 0: the torch formulation on the NCDHW view
SYNCBN_ROWS_HIP = os.environ.get("SGC_SYNCBN_ROWS_HIP", "0") == "1"
# a batch of scenes through a training convolution: "batched" = one launch per pass on the `_batched` entries, the
# weight gradient summed over the scenes inside its kernel; "loop" = the scene-less entries scene by scene (B launches per pass, B
# weight gradients added by autograd) around the same joint norm -- the timing baseline and a second checker
TRAIN_SCENE_BATCH = os.environ.get("SGC_TRAIN_SCENE_BATCH", "batched")
if TRAIN_SCENE_BATCH not in ("batched", "loop"):
    raise ValueError(f"SGC_TRAIN_SCENE_BATCH={TRAIN_SCENE_BATCH}: batched or loop")


THROUGHPUT_GEOMETRY = False      # set_throughput_mode(True): scenes in flight, kernels sized for CU-time
WINOGRAD_IN_FLIGHT = False       # the Winograd-z gate's view of it: follows set_throughput_mode unless that call says keep_winograd=True


def set_throughput_mode(on, keep_winograd=False):
    """Launch geometry for several scenes in flight (one hipGraph per scene on its own stream, bench.py).  With four scenes
    overlapping the chip is CU-time bound -- the sum of workgroup residency of all kernels, not any kernel's latency, sets the
    throughput -- so kernels are sized for work per CU-second instead of for their own latency:
      * the persistent row GEMM runs on HALF the CUs with two tiles in flight per workgroup (alone: 92 -> 136 us on the
        204 800-row Linear, but 27 % less CU-time; same bits -- a row's result does not depend on the tiling of the call);
      * the layers with few voxels split their reductions over FEWER workgroups (tile kernel: until 256 instead of 512 workgroups,
        halo kernel: 96 instead of 192): less prologue / epilogue and workspace traffic per unit of work, 20 - 30 % more latency
        per layer.  A different split adds the same partial sums in a different order: seven convolution layers of the neck
        differ from the latency geometry by fp32 summation order (<= 1e-5 of the tensor scale, tested); each mode is
        deterministic and bit-identical between graph replays and eager launches.
    Together +3.5 % scenes/s (alternated runs).  Off = the latency-optimal geometry (one scene at a time, the default of the
    library).  Call it before the first scene: captured graphs keep the geometry they were captured with.
    ``keep_winograd``: the reduction splits change, the choice of the Winograd-z form per layer does NOT (bench.py's
    ``--eager-geometry latency`` pass must time the kernels the graphs replay, not another form of the small layers)."""
    global THROUGHPUT_GEOMETRY, WINOGRAD_IN_FLIGHT
    THROUGHPUT_GEOMETRY = bool(on)
    if not keep_winograd:
        WINOGRAD_IN_FLIGHT = bool(on)
    from .. import ext
    lib = ext.ops().lib
    explicit = os.environ.get("SGC_TUNE", "")
    for key, hot, cold in (("rows_cu_pct", 50, 100), ("rows_depth", 2, 1), ("split_target", 256, 512), ("halo_split_target", 96, 192)):
        if key + "=" not in explicit:
            lib.call("sgc_set_tuning", key.encode(), hot if on else cold)


def set_train_conv(mode):
    global TRAIN_CONV
    if mode not in ("hip", "library"):
        raise ValueError(mode)
    TRAIN_CONV = mode


def set_train_scene_batch(mode):
    global TRAIN_SCENE_BATCH
    if mode not in ("batched", "loop"):
        raise ValueError(mode)
    TRAIN_SCENE_BATCH = mode


def train_conv_on_hip(x, channels):
    """Can the autograd path of a conv chain run on the HIP kernels?  (CUDA, any number of scenes, channel counts the K tile accepts)"""
    return (TRAIN_CONV == "hip" and CONV_MODE == "bf16x3" and train_products_ok() and x.is_cuda and x.shape[0] >= 1
            and all(c % _PAD == 0 for c in channels))


def train_conv3d_rows(x, weight, grid, ksize=3, stride=1, transposed=False, scenes=1):
    """A training convolution on the rows of ``scenes`` volumes of ``grid`` ([scenes * V, Cin] -> [scenes * OV, Cout]) under autograd,
    by ``TRAIN_SCENE_BATCH``: one Function call on the batch, or one per scene."""
    from ..functions import ChannelsLastConv3dFunction, ChannelsLastConvTranspose3dFunction
    batched = scenes == 1 or TRAIN_SCENE_BATCH == "batched"
    parts = (x,) if batched else x.view(scenes, -1, x.shape[1]).unbind(0)
    n = scenes if batched else 1
    if transposed:
        out = [ChannelsLastConvTranspose3dFunction.apply(rows, weight, grid, n) for rows in parts]
    else:
        out = [ChannelsLastConv3dFunction.apply(rows, weight, grid, ksize, stride, n) for rows in parts]
    return out[0] if batched else torch.cat(out)


def train_products_ok():
    """The autograd Functions pack their weight planes with ``sgc_pack_conv_weight``, which emits bfloat16 hi / lo bits; the
    forward and input-gradient kernels follow the process-wide arithmetic mode.  Modes 3 and 1 read those bits as bfloat16;
    mode 2 (fp16) would read them as IEEE half (bf16 1.0 = 0x3F80 is 1.875 as a half) -- so the fp16 mode is inference-only:
    with gradients enabled the convolutions / Linears take torch's library path (fp32) instead."""
    return CONV_PRODUCTS != 2


def _count_batch(bn):
    """Counts this batch in ``num_batches_tracked`` as nn.BatchNorm's forward does and returns the momentum of the running-statistics
    update (the cumulative average 1 / count when the module's momentum is None)."""
    momentum = 0.0 if bn.momentum is None else bn.momentum
    if bn.training and bn.track_running_stats and bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
        if bn.momentum is None:
            momentum = 1.0 / float(bn.num_batches_tracked)
    return momentum


def _bn_on_kernels(bn, rows, C):
    """May this norm over the first ``C`` columns of ``rows`` run on ``sgc_bn_rows_*``?  A plain BatchNorm2d / 3d with affine
    parameters that normalises with batch statistics, on the HIP training path, over more than one CUDA fp32 row, norm and rows of a
    width the 16-byte loads accept."""
    return (type(bn) in (torch.nn.BatchNorm3d, torch.nn.BatchNorm2d) and (bn.training or (bn.running_mean is None and bn.running_var is None))
            and TRAIN_CONV == "hip" and BN_ON_HIP and rows.is_cuda and rows.dtype == torch.float32 and C % 4 == 0 and rows.shape[1] % 4 == 0
            and bn.weight is not None and bn.bias is not None and rows.shape[0] > 1)


def _residual_fits(residual, rows):
    return residual is None or (residual.dtype == torch.float32 and residual.shape == rows.shape)


def syncbn_counts_fit(rows, world):
    """The row counts of a SyncBatchNorm travel between the ranks as fp32: exact while this rank's count and the total stay below
    2^24 (the total assumes ranks of equal size, the reference's one scene per rank); the merge kernel's loop bounds ``world``."""
    from .. import _abi
    return 0 < rows < _abi.SYNCBN_MAX_COUNT and world * rows < _abi.SYNCBN_MAX_COUNT and 1 <= world <= _abi.SYNCBN_MAX_WORLD


def _syncbn_on_kernels(bn, rows):
    """May this norm run on ``sgc_bn_rows_sync_*``?  Opted in, a training-mode ``dist.SyncBatchNorm3d`` with a momentum and affine
    parameters, on the HIP training path, over CUDA fp32 rows of a width the 16-byte loads accept, counts that fp32 holds."""
    if not SYNCBN_ROWS_HIP:
        return False
    from .. import dist as sgc_dist
    from ..functions import _sync_world
    return (type(bn) is sgc_dist.SyncBatchNorm3d and bn.training and bn.momentum is not None and bn.weight is not None and bn.bias is not None
            and TRAIN_CONV == "hip" and BN_ON_HIP and rows.is_cuda and rows.dtype == torch.float32 and rows.shape[1] % 4 == 0
            and syncbn_counts_fit(rows.shape[0], _sync_world(bn.process_group)))


def _bn_function(bn, rows, momentum, residual, tail, channels=None):
    from ..functions import BatchNormRowsFunction
    track = bn.training and bn.track_running_stats
    return BatchNormRowsFunction.apply(rows, bn.weight, bn.bias, bn.running_mean if track else None, bn.running_var if track else None,
                                       float(momentum), float(bn.eps), residual, tail, channels)


def bn_rows(bn, rows, grid, residual=None, relu=False, image=False, channels=None, relu_then_add=False):
    """A BatchNorm3d-like module on channels-last rows [V, C], optionally followed by ``+ residual`` and ``relu`` (the tails of the
    neck's blocks; on the HIP path they run inside the normalisation passes).  ``nn.BatchNorm3d`` over [1, C, X, Y, Z] is the
    statistics of the V rows per channel, i.e. ``F.batch_norm`` on the [V, C] matrix (same running-statistics update); any other
    module (SyncBatchNorm3d, GroupNorm ...) gets the 5-D channels-last view -- but for a training-mode ``dist.SyncBatchNorm3d`` under
    ``SYNCBN_ROWS_HIP`` (opt-in), which takes ``SyncBatchNormRowsFunction`` on the rows with the same fused tail.  ``nn.BatchNorm2d`` over [N, C, H, W] is the same
    statistics of the N * H * W rows (``grid`` = (N, H, W)) and takes the same branch; a 2-D norm of any other type
    (``SyncBatchNorm`` ...) gets the 4-D NCHW view of the rows.

    ``channels`` (default None: the rows are as wide as the norm): the rows are zero-padded -- their first ``channels`` columns are
    the norm's, the rest padding that is never read and comes back as zeros (``BatchNormRowsFunction`` with ``channels``; off the
    HIP path the same on the slice).  ``relu_then_add`` (with ``relu``): ``relu(bn(rows)) + residual``, the U-Net skip, instead of
    ``relu(bn(rows) + residual)``; on the HIP path it rides in the padded norm's passes too."""
    if channels is not None or relu_then_add:
        return _bn_rows_padded(bn, rows, grid, residual, relu, image, rows.shape[1] if channels is None else channels, relu_then_add)

    def tail(y):
        if residual is not None:
            y = y + residual
        return torch.relu(y) if relu else y
    if type(bn) in (torch.nn.BatchNorm3d, torch.nn.BatchNorm2d):
        use_batch = bn.training or (bn.running_mean is None and bn.running_var is None)
        momentum = _count_batch(bn)
        if _bn_on_kernels(bn, rows, rows.shape[1]):
            fuse = BN_FUSE_TAIL and _residual_fits(residual, rows)      # else the norm on the kernels, the tail in torch
            y = _bn_function(bn, rows, momentum, residual if fuse else None, bool(relu and fuse))
            return y if fuse else tail(y)
        return tail(torch.nn.functional.batch_norm(rows, bn.running_mean if not bn.training or bn.track_running_stats else None,
                                                   bn.running_var if not bn.training or bn.track_running_stats else None,
                                                   bn.weight, bn.bias, use_batch, momentum, bn.eps))
    if not image and _syncbn_on_kernels(bn, rows):
        from ..functions import SyncBatchNormRowsFunction
        if bn.num_batches_tracked is not None:                 # as SyncBatchNorm3d.forward counts the batch
            bn.num_batches_tracked.add_(1)
        fuse = BN_FUSE_TAIL and _residual_fits(residual, rows)
        y = SyncBatchNormRowsFunction.apply(rows, bn.weight, bn.bias, bn.running_mean, bn.running_var, float(bn.momentum), float(bn.eps),
                                            residual if fuse else None, bool(relu and fuse), bn.process_group)
        return y if fuse else tail(y)
    if image:
        y = bn(rows.view(grid[0], grid[1], grid[2], rows.shape[1]).permute(0, 3, 1, 2))
        return tail(y.permute(0, 2, 3, 1).reshape(rows.shape[0], rows.shape[1]))
    y = bn(rows_to_ncdhw(rows, grid, rows.shape[1]))           # [B, C, X, Y, Z]: a SyncBatchNorm3d sees the batch it was written for
    return tail(y.permute(0, 2, 3, 4, 1).reshape(rows.shape[0], rows.shape[1]))


def _bn_rows_padded(bn, rows, grid, residual, relu, image, C, relu_then_add):
    """``bn_rows`` for padded rows and / or the ReLU-then-add tail.  A plain BatchNorm under the conditions of ``bn_rows``' HIP branch
    whose tail can ride in the passes takes ``BatchNormRowsFunction`` at padded width; everything else is ``bn_rows`` itself on the first ``C`` columns (a view), the tail in torch,
    zero columns behind.  The bookkeeping of ``num_batches_tracked`` and the momentum is the code above, reached either way."""
    if relu_then_add and (not relu or residual is None):
        raise ValueError("bn_rows: relu_then_add is relu(bn) + residual")
    ld = rows.shape[1]
    if _bn_on_kernels(bn, rows, C) and BN_FUSE_TAIL and _residual_fits(residual, rows):      # the padded entries need the fused tail
        return _bn_function(bn, rows, _count_batch(bn), residual, 2 if relu_then_add else int(bool(relu)), C)
    res = None if residual is None else residual[:, :C]
    plain = type(bn) in (torch.nn.BatchNorm3d, torch.nn.BatchNorm2d)
    x = rows[:, :C] if plain else rows[:, :C].contiguous()         # the other norms see an NCHW / NCDHW view of the rows
    if relu_then_add:
        y = bn_rows(bn, x, grid, relu=True, image=image) + res
    else:
        y = bn_rows(bn, x, grid, residual=res, relu=relu, image=image)
    return y if ld == C else torch.nn.functional.pad(y, (0, ld - C))


class TrainConv2d:
    """To training what ``Conv2dSpec`` is to eval, with its call signature: an ``nn.Conv2d`` (k in {1, 3}, padding k // 2, stride 1
    or 2) with a LIVE norm behind it, under autograd on channels-last rows -- ``TrainConv3d``'s 2-D twin.  Holds the
    two modules by reference and nothing else (``convert_sync_batchnorm`` may swap the norm between forwards): the raw convolution and
    its trainable bias run through ``FrozenNormConv2dFunction``'s bias form (no scale, no shift, no ReLU), the norm is whatever
    ``bn_rows`` takes.  ``bn`` None: the convolution and its bias alone (the trunk's final 1x1).  On CPU tensors the convolution is
    torch's, on the NCHW view of the rows; the tails and the norm are the same code."""

    def __init__(self, conv, bn=None, pad=False):
        """``pad`` (the regulation U-Nets): rows come and go at the next multiple of 32 columns with zeros behind the
        channels, for any channel count that is a multiple of 4 -- ``PaddedConv2dFunction`` and the padded norm, which also takes the
        ReLU-then-add tail into its passes.  Default: the rows are as wide as the layer, as before."""
        self.conv, self.bn, self.cout, self.pad = conv, bn, conv.out_channels, bool(pad)

    def _conv(self, x, nhw):
        conv = self.conv
        if x.is_cuda and self.pad:
            from ..functions import PaddedConv2dFunction
            return PaddedConv2dFunction.apply(x, conv.weight, conv.bias, tuple(nhw), conv.stride[0])
        if x.is_cuda:
            from ..functions import FrozenNormConv2dFunction
            args = (x, conv.weight, None, None, None, tuple(nhw), conv.stride[0], False, False)
            return FrozenNormConv2dFunction.apply(*args) if conv.bias is None else FrozenNormConv2dFunction.apply(*args, conv.bias)
        y = conv(x.view(nhw[0], nhw[1], nhw[2], x.shape[1])[..., :conv.in_channels].permute(0, 3, 1, 2))
        y = y.permute(0, 2, 3, 1).reshape(-1, self.cout)
        return torch.nn.functional.pad(y, (0, _pad_to(self.cout) - self.cout)) if self.pad else y

    def __call__(self, x, nhw, residual=None, relu=True, relu_after_add=False, out=None, col0=0):
        """``relu`` / ``relu_after_add`` as ``Conv2dSpec`` has them: relu(bn); relu(bn) + residual; with ``relu_after_add`` (and
        ``relu`` False) relu(bn + residual).  ``out`` / ``col0`` are ``Conv2dSpec``'s way of writing into a wider buffer: eval only."""
        s = self.conv.stride[0]
        onhw = (nhw[0], (nhw[1] + s - 1) // s, (nhw[2] + s - 1) // s)
        if relu and relu_after_add:
            raise NotImplementedError("TrainConv2d: relu and relu_after_add exclude each other")
        if out is not None or col0:
            raise NotImplementedError("TrainConv2d: a training layer returns its own rows (no `out` buffer)")
        y = self._conv(x, nhw)
        if self.bn is None:
            if residual is not None or relu or relu_after_add:
                raise NotImplementedError("TrainConv2d: a layer without a norm has no tail")
            return y, onhw
        if self.pad:
            return bn_rows(self.bn, y, onhw, residual=residual, relu=bool(relu or relu_after_add), image=True, channels=self.cout,
                           relu_then_add=bool(relu and residual is not None)), onhw
        if relu and residual is not None:                  # the identity block: the ReLU in the norm's pass, then the skip
            return bn_rows(self.bn, y, onhw, relu=True, image=True) + residual, onhw
        return bn_rows(self.bn, y, onhw, residual=residual, relu=bool(relu or relu_after_add), image=True), onhw


class TrainConvTranspose2d:
    """``TrainConv2d``'s sibling for the up stages of ``SimpleUnet2D``: ``nn.ConvTranspose2d(3, stride 2, padding 1, output_padding 1,
    bias=False)`` with a LIVE norm behind it on rows of padded width.  Holds the two modules by reference and
    nothing else.  The convolution is ``ConvTranspose2dRowsFunction`` -- all three passes on the existing entries -- the norm is
    ``bn_rows`` at padded width, with ``relu(bn) + residual`` (the additive skip) inside its passes.  On CPU tensors the convolution
    is torch's on the NCHW view of the rows; the norm and the tails are the same code."""

    def __init__(self, conv, bn):
        if (conv.kernel_size, conv.stride, conv.padding, conv.output_padding) != ((3, 3), (2, 2), (1, 1), (1, 1)) or conv.bias is not None:
            raise ValueError("TrainConvTranspose2d: ConvTranspose2d(3, stride 2, padding 1, output_padding 1, bias=False)")
        self.conv, self.bn, self.cout = conv, bn, conv.out_channels

    def __call__(self, x, nhw, residual=None, relu=True, relu_after_add=False, out=None, col0=0):
        onhw = (nhw[0], 2 * nhw[1], 2 * nhw[2])
        if relu_after_add or not relu:
            raise NotImplementedError("TrainConvTranspose2d: relu(bn) [+ residual]")
        if out is not None or col0:
            raise NotImplementedError("TrainConvTranspose2d: a training layer returns its own rows (no `out` buffer)")
        conv = self.conv
        if x.is_cuda:
            from ..functions import ConvTranspose2dRowsFunction
            y = ConvTranspose2dRowsFunction.apply(x, conv.weight, tuple(nhw))
        else:
            y = conv(x.view(nhw[0], nhw[1], nhw[2], x.shape[1])[..., :conv.in_channels].permute(0, 3, 1, 2))
            y = torch.nn.functional.pad(y.permute(0, 2, 3, 1).reshape(-1, self.cout), (0, _pad_to(self.cout) - self.cout))
        return bn_rows(self.bn, y, onhw, residual=residual, relu=True, image=True, channels=self.cout,
                       relu_then_add=residual is not None), onhw


class TrainStem7:
    """``Stem7Spec``'s training twin: ``relu(bn1(conv1(img) + bias))`` with the LIVE norm.  The forward is
    ``sgc_conv2d_stem7_bf16x3`` with the bias as its shift and no ReLU, on [64][160] planes packed from the parameter at every call
    (``functions.Stem7ConvFunction``: its backward is ``sgc_conv2d_stem7_wgrad_bf16x3``; images get no gradient), then ``bn_rows``
    with the ReLU.  On CPU tensors the convolution is torch's."""

    def __init__(self, conv, bn):
        self.conv, self.bn = conv, bn

    def __call__(self, img):
        N, _, H, W = img.shape
        nhw = (N, H // 2, W // 2)
        if img.is_cuda:
            from ..functions import Stem7ConvFunction
            y = Stem7ConvFunction.apply(img, self.conv.weight, self.conv.bias)
        else:
            y = self.conv(img).permute(0, 2, 3, 1).reshape(-1, self.conv.out_channels)
        return bn_rows(self.bn, y, nhw, relu=True, image=True), nhw


class TrainConv3d:
    """To training what ``ConvSpec`` is to eval, with its call signature: an ``nn.Conv3d`` (k in {1, 3}, padding k // 2) or
    ``nn.ConvTranspose3d(2, 2, bias=False)`` with a LIVE norm behind it, under autograd on channels-last rows.  Holds the two modules
    and nothing else: the weight is read through ``train_weight_planes()`` at every call, the norm is whatever ``bn_rows`` takes.
    ``scenes``: the rows hold that many volumes of the grid, one after the other; the convolution treats each on its own
    (``train_conv3d_rows``), the norm sees the rows of all of them -- the statistics of the batch."""

    def __init__(self, conv, bn, scenes=1):
        self.conv, self.bn, self.cout, self.scenes = conv, bn, conv.out_channels, int(scenes)

    def __call__(self, x, grid, residual=None, relu=0, out_mask=None, act=None):
        """``relu`` as ``ConvSpec`` has it -- 0: bn + residual; 1: relu(bn + residual); 2: relu(bn), then + residual."""
        if out_mask is not None or act is not None:
            raise NotImplementedError("TrainConv3d: row masks and the output activation are eval-only (ConvSpec)")
        conv, grid = self.conv, tuple(grid)
        if isinstance(conv, torch.nn.ConvTranspose3d):
            y, og = train_conv3d_rows(x, conv.weight, grid, transposed=True, scenes=self.scenes), tuple(2 * d for d in grid)
        else:
            k, s = conv.kernel_size[0], conv.stride[0]
            y, og = train_conv3d_rows(x, conv.weight, grid, k, s, scenes=self.scenes), tuple((d + 2 * (k // 2) - k) // s + 1 for d in grid)
            if conv.bias is not None:
                y = y + conv.bias
        if relu == 2:
            return bn_rows(self.bn, y, og, relu=True) + residual, og
        return bn_rows(self.bn, y, og, residual=residual, relu=bool(relu)), og


def module_fingerprint(module):
    """Cheap change detector for the cached plans: (storage address, in-place version) of every
    parameter / buffer.  The tensor list itself is cached on the module (rebuilt on .train()/.to())."""
    tensors = module.__dict__.get("_fp_tensors")
    if tensors is None or module.__dict__.get("_fp_training") != module.training:
        tensors = list(module.parameters()) + list(module.buffers())
        module.__dict__["_fp_tensors"] = tensors
        module.__dict__["_fp_training"] = module.training
    return (CONV_PRODUCTS,) + tuple((t.data_ptr(), t._version) for t in tensors)       # a mode switch rebuilds the weight planes


def cached_plan(module, build, attr="_hip_plan", fingerprint=None):
    """``module``'s prepared plan: the one stored under ``module.__dict__[attr]`` while ``fingerprint`` (default:
    ``module_fingerprint(module)``) is the one it was built at, else ``build()``, stored.  Popping the attribute forces a rebuild."""
    fp = module_fingerprint(module) if fingerprint is None else fingerprint
    cached = module.__dict__.get(attr)
    if cached is not None and cached[0] == fp:
        return cached[1]
    plan = build()
    module.__dict__[attr] = (fp, plan)
    return plan


def image_rows(x):
    """[N, C, H, W] (any strides) -> ([N*H*W, C] fp32 rows, (N, H, W)); zero-copy for channels-last fp32 memory."""
    N, C, H, W = x.shape
    if x.is_contiguous(memory_format=torch.channels_last) and x.dtype == torch.float32:
        return x.permute(0, 2, 3, 1).reshape(N * H * W, C), (N, H, W)
    return ext.ops().nchw_to_nhwc_crop(x.float(), H, W).view(N * H * W, C), (N, H, W)


def to_channels_last_rows(x):
    """[B,C,X,Y,Z] (any strides) -> ([B*X*Y*Z, C_padded] contiguous rows, scene b in rows [b*X*Y*Z, (b+1)*X*Y*Z); (X,Y,Z)); no copy
    when the tensor already is channels-last in memory and C % 32 == 0."""
    B, C, X, Y, Z = x.shape
    rows = x.permute(0, 2, 3, 4, 1).reshape(B * X * Y * Z, C)      # view if channels-last, copy otherwise
    cp = _pad_to(C)
    if cp != C:
        rows = torch.nn.functional.pad(rows, (0, cp - C))
    return rows.contiguous().float(), (X, Y, Z)


def rows_to_ncdhw(rows, grid, channels):
    """[B*V, Cp] rows -> [B, channels, X, Y, Z] view (channels-last memory, no copy); B = rows / V."""
    X, Y, Z = grid
    return rows.view(-1, X, Y, Z, rows.shape[1])[..., :channels].permute(0, 4, 1, 2, 3)


class BlockDiagSpec:
    """A block-diagonal Linear [G * K -> G * Nh] kept as its G blocks (``sgc_linear_rows_blockdiag_bf16x3``): group g's K inputs times
    its own [Nh, K] weight.  ``weight`` [G, Nh, K], ``bias`` [G * Nh]."""

    def __init__(self, weight, bias):
        w = weight.detach().float().contiguous()
        self.G, self.Nh, self.K = w.shape
        self.w_hi, self.w_lo = ext.ops().split_operand(w)
        self.shift = bias.detach().float().contiguous() if bias is not None else None

    @staticmethod
    def supported(G, K, Nh):
        return CONV_MODE == "bf16x3" and ext.ops().linear_rows_blockdiag_supported(G, K, Nh)

    def __call__(self, x, count=None):
        return ext.ops().linear_rows_blockdiag(x, self.w_hi, self.w_lo, self.shift, count=count)


class LinearSpec:
    """nn.Linear (or a row-block of stacked weights) prepared for ``sgc_conv3d_cl_bf16x3`` as a 1x1x1
    convolution over M rows: y[M, out] = x[M, in] @ W^T + b on the bf16 matrix cores with the 3-way split."""

    def __init__(self, weight, bias, useful=None):
        """``useful``: fraction of the weight matrix that is structurally non-zero (a block-diagonal matrix run as a dense
        GEMM); only bench.py's flop accounting reads it (the zero blocks are not algorithmic work)."""
        w = weight.detach().float()
        cout, cin = w.shape
        self.useful = useful
        if cin % _PAD:
            raise ValueError("LinearSpec needs in_features % 32 == 0")
        cout_p = _pad_to(cout, 4)
        wp = torch.zeros((1, cout_p, cin), dtype=torch.float32, device=w.device)
        wp[0, :cout] = w
        self.wt = wp
        self.w_hi, self.w_lo = ext.ops().split_operand(wp)
        self.shift = torch.zeros(cout_p, dtype=torch.float32, device=w.device)
        if bias is not None:
            self.shift[:cout] = bias.detach().float()
        self.cout, self.cout_p = cout, cout_p

    def __call__(self, x, extra_zero_row=False, count=None):
        """``extra_zero_row``: the result is a view of an [M+1, out] buffer whose last row is zero (the
        gather kernel points out-of-image corners at it).  ``count``: int32 device tensor with the number of
        live rows of ``x`` (its remaining rows are capacity): rows past it are neither read nor written."""
        M = x.shape[0]
        if CONV_MODE == "bf16x3" and self.cout_p == self.cout:
            return ext.ops().linear_rows_bf16x3(x, self.w_hi, self.w_lo, self.shift, count=count, useful=self.useful,
                                                zero_tail=bool(extra_zero_row) and M > 0)
        if count is not None:
            raise NotImplementedError("device-side row counts need the bf16x3 path and out_features % 4 == 0")
        if CONV_MODE == "bf16x3":
            y, _ = ext.ops().conv3d_cl_bf16x3(x, self.w_hi, self.w_lo, (M, 1, 1), 1, 1, False, None, self.shift)
        else:
            y, _ = ext.ops().conv3d_cl(x, self.wt, (M, 1, 1), 1, 1, False, None, self.shift)
        return y if self.cout_p == self.cout else y[:, :self.cout]

    def headmajor(self, x, N, S, M, out_dtype=torch.float32):
        """x [N*S, in] -> [N, M, S, out/M]: the same GEMM with the result stored head-major (the layout the LDS-tiled
        gather stages a head's window from); bf16x3 path only.  ``out_dtype=torch.bfloat16``: bf16 storage mode."""
        if CONV_MODE != "bf16x3" or self.cout_p != self.cout:
            raise NotImplementedError("head-major output needs the bf16x3 path and out_features % 4 == 0")
        return ext.ops().linear_rows_headmajor_bf16x3(x, self.w_hi, self.w_lo, self.shift, N, S, M, out_dtype=out_dtype)
