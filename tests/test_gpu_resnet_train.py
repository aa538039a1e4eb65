"""The ResNet backbone's training path on the HIP kernels (include/sgcdet_amd_train.h section 12, functions.py
``FrozenNormConv2dFunction``, plugin/resnet.py ``_forward_hip_train``).

Errors are relative to the max-abs of the compared tensor, against float64 on the CPU.  Per kernel and per Function the bound is
1e-4, the project's bf16x3 contract.  Where a ReLU sits between the compared quantities the float64 reference takes its GATE from
the HIP forward (``y > 0``), not from its own pre-activation: a flipped gate moves a whole weight gradient by one term of a short
sum, which no tolerance absorbs.  That the gates themselves are right is checked apart: the two gates may disagree only where the
float64 pre-activation is below 1e-4 of its max-abs, and such elements are rare.

MEASURED below records what an MI355X gave for the whole-backbone case; its bound is four times that (the module-test convention
of DESIGN.md 4.10).
"""
import copy
import json
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from golden_util import max_err
from resnet_train_util import GatedReplica, rows_to_nchw
from resnet_util import fill_resnet

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REF_BACKBONE = dict(type="ResNet", depth=50, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=1,
                    norm_cfg=dict(type="BN", requires_grad=False), norm_eval=True, style="pytorch",
                    pretrained="torchvision://resnet50")

# (depth, input shape) -> worst parameter gradient's error against the gated float64 replica, measured on an MI355X
MEASURED = {
    (18, (2, 3, 64, 96)): 1.330e-5,       # layer2.1.conv1.weight
    (50, (2, 3, 72, 104)): 2.406e-5,      # layer2.2.conv1.weight
}


# ---- 1. sgc_conv2d_wgrad_bf16x3 ------------------------------------------------------------------------------------------------
def _wgrad_ref(x, dy, nhw, k, s):
    """float64 autograd of F.conv2d: rows x [N*H*W, Cin], dy [N*OH*OW, Cout] -> dW in the kernel's layout [k*k, Cout, Cin]."""
    N, H, W = nhw
    Cin, Cout = x.shape[1], dy.shape[1]
    xi = x.double().view(N, H, W, Cin).permute(0, 3, 1, 2)
    w = torch.zeros(Cout, Cin, k, k, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(xi, w, stride=s, padding=k // 2)
    OH, OW = (H + s - 1) // s, (W + s - 1) // s
    assert y.shape == (N, Cout, OH, OW)
    dw, = torch.autograd.grad(y, w, dy.double().view(N, OH, OW, Cout).permute(0, 3, 1, 2))
    return dw.permute(2, 3, 0, 1).reshape(k * k, Cout, Cin)


_WGRAD_SHAPES = [(2, 8, 8), (2, 7, 10), (3, 5, 3), (4, 32, 32)]


@pytest.mark.parametrize("nhw", _WGRAD_SHAPES)
@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("k", [1, 3])
def test_wgrad_kernel_against_float64(gpu_ops, k, s, nhw):
    """Tile tails in both channel dimensions, K-step tails (40, 40 and 18 reduction rows at stride 2), a split reduction (4096
    rows); with the workspace (fixed summation order: two launches are bit-identical) and without it (one workgroup per tile)."""
    ops = gpu_ops
    N, H, W = nhw
    OH, OW = (H + s - 1) // s, (W + s - 1) // s
    for Cin, Cout in ((32, 32), (64, 160), (160, 36)):
        g = torch.Generator().manual_seed(1000 * k + 100 * s + H + Cin)
        x = torch.randn(N * H * W, Cin, generator=g)
        dy = torch.randn(N * OH * OW, Cout, generator=g)
        want = _wgrad_ref(x, dy, nhw, k, s)
        mag = want.abs().max().item()
        floats = ops.conv2d_wgrad_workspace_floats(nhw, Cin, Cout, k, s)
        if nhw == (4, 32, 32) and s == 1:
            assert floats > 0                                    # this shape splits its reduction: the ordered sum is exercised
        xg, dyg = x.cuda(), dy.cuda()
        for workspace in (True, False):
            got = ops.conv2d_wgrad_bf16x3(xg, dyg, nhw, k, s, workspace=workspace)
            assert got.shape == want.shape
            err = max_err(got, want) / mag
            print(f"conv2d_wgrad k{k} s{s} {nhw} {Cin}->{Cout} workspace {workspace} ({floats} floats): err {err:.3e} of max-abs {mag:.2f}")
            assert err < 1e-4
            if workspace:
                assert torch.equal(got, ops.conv2d_wgrad_bf16x3(xg, dyg, nhw, k, s, workspace=True))


def test_wgrad_kernel_refuses_what_it_does_not_cover(gpu_ops):
    from sgcdet_amd._abi import SgcError
    x, dy = torch.randn(2 * 8 * 8, 32).cuda(), torch.randn(2 * 8 * 8, 30).cuda()
    with pytest.raises((SgcError, RuntimeError), match="multiples of 4"):
        gpu_ops.conv2d_wgrad_bf16x3(x, dy, (2, 8, 8), 3, 1)
    with pytest.raises(RuntimeError, match="inconsistent"):
        gpu_ops.conv2d_wgrad_bf16x3(x, torch.randn(2 * 8 * 8, 32).cuda(), (2, 8, 8), 3, 2)


# ---- 2. sgc_frozen_norm_act_backward ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,C", [(37, 36), (1000, 64), (1, 4)])
def test_frozen_norm_act_backward_equals_torch(gpu_ops, rows, C):
    """Bit for bit the three-line expression: the products are single fp32 multiplies.  A NaN of dy goes through where the gate is
    open (and everywhere without a ReLU) and is dropped where the ReLU closed the element, as torch's threshold_backward does."""
    g = torch.Generator().manual_seed(rows + C)
    dy, y = torch.randn(rows, C, generator=g), torch.randn(rows, C, generator=g)
    scale = 0.5 + torch.rand(C, generator=g)
    y[0, 0], y[0, 1] = 1.0, -1.0
    dy[0, 0] = dy[0, 1] = float("nan")                           # one under an open gate, one under a closed one
    for relu in (True, False):
        for sc in (scale, None):
            for want_gres in (True, False):
                gm = torch.where(y > 0, dy, torch.zeros_like(dy)) if relu else dy
                want_g = gm * sc if sc is not None else gm
                want_gres_t = gm
                got_g, got_gres = gpu_ops.frozen_norm_act_backward(dy.cuda(), y.cuda() if relu else None, None if sc is None else sc.cuda(),
                                                                   relu=relu, want_gres=want_gres)
                assert (got_gres is not None) == want_gres
                for got, want in ((got_g, want_g),) + (((got_gres, want_gres_t),) if want_gres else ()):
                    got = got.cpu()
                    assert torch.equal(torch.isnan(got), torch.isnan(want))
                    assert torch.equal(torch.nan_to_num(got, nan=7.0), torch.nan_to_num(want, nan=7.0))
                assert torch.isnan(got_g[0, 0]) and bool(torch.isnan(got_g[0, 1])) == (not relu)


# ---- 3. FrozenNormConv2dFunction ------------------------------------------------------------------------------------------------
def _function_case(k, s, nhw, epilogue, seed, Cin=32, Cout=64):
    N, H, W = nhw
    OH, OW = (H + s - 1) // s, (W + s - 1) // s
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N * H * W, Cin, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (k * Cin ** 0.5)             # fan-in scaled
    scale, shift = 0.5 + torch.rand(Cout, generator=g), 0.1 * torch.randn(Cout, generator=g)
    res = torch.randn(N * OH * OW, Cout, generator=g) if epilogue == "res_relu" else None
    cot = torch.randn(N * OH * OW, Cout, generator=g)
    return x, w, scale, shift, res, cot, (N, OH, OW)


def _function_ref(x, w, scale, shift, res, cot, nhw, onhw, k, s, gate):
    """float64: (pre-activation rows, dx, dw, dres) with the ReLU replaced by ``gate`` (rows, bool) | None."""
    N, H, W = nhw
    xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
    rd = None if res is None else res.double().requires_grad_(True)
    t = F.conv2d(xd.view(N, H, W, -1).permute(0, 3, 1, 2), wd, stride=s, padding=k // 2).permute(0, 2, 3, 1).reshape(-1, w.shape[0])
    assert t.shape[0] == onhw[0] * onhw[1] * onhw[2]
    if scale is not None:
        t = t * scale.double() + shift.double()
    if rd is not None:
        t = t + rd
    y = t if gate is None else t * gate.double()
    (y * cot.double()).sum().backward()
    return t.detach(), xd.grad, wd.grad, None if rd is None else rd.grad


@pytest.mark.parametrize("nhw", [(2, 8, 10), (2, 7, 9)])
@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("k", [1, 3])
def test_function_gradients_against_float64(gpu_ops, k, s, nhw):
    from sgcdet_amd.functions import FrozenNormConv2dFunction
    for epilogue in ("none", "relu", "res_relu", "plain"):       # plain: no scale / shift either
        for needs in ((1, 1, 1), (0, 1, 1), (1, 0, 0), (0, 1, 0)):          # x, weight, residual
            x, w, scale, shift, res, cot, onhw = _function_case(k, s, nhw, epilogue, 10 * k + s + nhw[1])
            if epilogue == "plain":
                scale = shift = None
            xg, wg = x.cuda().requires_grad_(bool(needs[0])), w.cuda().requires_grad_(bool(needs[1]))
            rg = None if res is None else res.cuda().requires_grad_(bool(needs[2]))
            y = FrozenNormConv2dFunction.apply(xg, wg, None if scale is None else scale.cuda(), None if shift is None else shift.cuda(), rg,
                                               nhw, s, epilogue == "relu", epilogue == "res_relu")
            assert y.shape == (onhw[0] * onhw[1] * onhw[2], w.shape[0])
            gated = epilogue in ("relu", "res_relu")
            gate = (y.detach() > 0).cpu() if gated else None
            (y * cot.cuda()).sum().backward()
            pre, dx, dw, dres = _function_ref(x, w, scale, shift, res, cot, nhw, onhw, k, s, gate)
            tag = f"k{k} s{s} {nhw} {epilogue} needs {needs}"
            fwd = pre if gate is None else pre * gate.double()
            e = max_err(y, fwd) / fwd.abs().max().item()
            print(f"function {tag}: forward err {e:.3e}")
            assert e < 1e-4
            if gated:
                # the gates: HIP and float64 may disagree only within rounding of zero, and such elements are rare
                pmax = pre.abs().max().item()
                near = pre.abs() < 1e-4 * pmax
                differ = gate != (pre > 0)
                print(f"function {tag}: {int(differ.sum())} gates differ, {int(near.sum())} of {near.numel()} pre-activations near zero")
                assert not (differ & ~near).any()
                assert near.sum().item() <= 0.01 * near.numel()
            for name, got, want, needed in (("dx", xg.grad, dx, needs[0]), ("dw", wg.grad, dw, needs[1]),
                                            ("dres", None if rg is None else rg.grad, dres, needs[2] and res is not None)):
                if not needed:
                    assert got is None, (tag, name)
                    continue
                assert got is not None and got.shape == want.shape, (tag, name)
                e = max_err(got, want) / want.abs().max().item()
                print(f"function {tag}: {name} err {e:.3e}")
                assert e < 1e-4, (tag, name)


def test_function_refuses_relu_before_the_add_and_the_fp16_mode(gpu_ops, monkeypatch):
    from sgcdet_amd.functions import FrozenNormConv2dFunction
    from sgcdet_amd.plugin import conv_plan
    x, w, scale, shift, res, cot, onhw = _function_case(3, 1, (1, 4, 4), "res_relu", 3)
    args = (x.cuda(), w.cuda().requires_grad_(True), scale.cuda(), shift.cuda(), res.cuda(), (1, 4, 4), 1)
    with pytest.raises(RuntimeError, match="gate"):
        FrozenNormConv2dFunction.apply(*args, True, False)
    monkeypatch.setattr(conv_plan, "CONV_PRODUCTS", 2)
    with pytest.raises(RuntimeError, match="inference-only"):
        FrozenNormConv2dFunction.apply(*args, False, True)


# ---- 3b. the training layer IS the prepared layer --------------------------------------------------------------------------------
@pytest.mark.parametrize("k,s,hw,kw", [(3, 1, (6, 7), dict()), (1, 1, (6, 7), dict(residual=True, relu=False, relu_after_add=True)),
                                       (3, 2, (8, 8), dict()), (3, 2, (5, 7), dict()), (1, 2, (5, 7), dict(relu=False))])
def test_frozen_conv2d_equals_conv2d_spec_bit_for_bit(gpu_ops, k, s, hw, kw):
    """``FrozenConv2d`` (live weight, planes from ``sgc_pack_conv_weight``, under autograd) against ``Conv2dSpec`` (prepared
    weight, planes from ``split_operand``) on one seeded convolution + eval BatchNorm: both go through ``conv2d_rows`` to the same
    entry on the same hi / lo bits, so the rows are ``torch.equal``."""
    from sgcdet_amd.plugin.conv_plan import Conv2dSpec, FrozenConv2d
    g = torch.Generator().manual_seed(100 * k + 10 * s + hw[0])
    conv, bn = nn.Conv2d(32, 32, k, stride=s, padding=k // 2, bias=False), nn.BatchNorm2d(32).eval()
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) / (k * 32 ** 0.5))
        bn.weight.copy_(1.0 + 0.2 * torch.randn(32, generator=g))
        bn.bias.copy_(0.1 * torch.randn(32, generator=g))
        bn.running_mean.copy_(0.1 * torch.randn(32, generator=g))
        bn.running_var.copy_(0.5 + torch.rand(32, generator=g))
    conv, bn = conv.cuda(), bn.cuda()
    nhw = (2,) + hw
    onhw = (2, (hw[0] + s - 1) // s, (hw[1] + s - 1) // s)
    x = torch.randn(nhw[0] * nhw[1] * nhw[2], 32, generator=g).cuda()
    kw = dict(kw)
    if kw.get("residual"):
        kw["residual"] = torch.randn(onhw[0] * onhw[1] * onhw[2], 32, generator=g).cuda()
    with torch.no_grad():
        want, want_nhw = Conv2dSpec(conv, bn)(x, nhw, **kw)
    got, got_nhw = FrozenConv2d(conv, bn)(x, nhw, **kw)
    assert got_nhw == want_nhw == onhw and got.requires_grad and want.abs().max() > 0
    print(f"FrozenConv2d vs Conv2dSpec k{k} s{s} {hw}: max difference {(got.detach() - want).abs().max().item():.3e}")
    assert torch.equal(got.detach(), want)


# ---- 4. the whole backbone -----------------------------------------------------------------------------------------------------
class _NoLibraryLayers:
    """nn.Conv2d / nn.BatchNorm2d / nn.MaxPool2d forward raise while this is active."""

    def __enter__(self):
        self.saved = [(c, c.forward) for c in (nn.Conv2d, nn.BatchNorm2d, nn.MaxPool2d)]

        def boom(self_, *a, **k):
            raise AssertionError(f"{type(self_).__name__}.forward was called: a library convolution / norm / pool ran")
        for c, _ in self.saved:
            c.forward = boom
        return self

    def __exit__(self, *exc):
        for c, f in self.saved:
            c.forward = f


def _net(depth):
    import sgcdet_amd.plugin  # noqa: F401
    from sgcdet_amd.mmcv_lite import build_backbone
    return fill_resnet(build_backbone(dict(REF_BACKBONE, depth=depth))).train()


def _cotangents(maps, seed=4):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(m.shape, generator=g) for m in maps]


@pytest.mark.parametrize("depth,shape", list(MEASURED))
def test_backbone_training_against_the_gated_float64_replica(monkeypatch, depth, shape):
    """Depth 18 on 64 x 96, depth 50 on 72 x 104 (odd maps in layers 3 and 4), the reference freezing.  Forward + backward run with
    the library layers patched to raise; exactly the convolutions of layers 2 - 4 get gradients; a second step repeats them bit
    for bit; the forward maps are the eval HIP maps; every parameter gradient is within 4 x the recorded figure of the float64
    replica on the HIP run's own gates, and those gates differ from float64's only within rounding of zero."""
    monkeypatch.setenv("SGC_BACKBONE_TRAIN_HIP", "1")
    monkeypatch.setenv("SGC_BACKBONE_HIP", "1")
    cpu_net = _net(depth)
    net = copy.deepcopy(cpu_net).cuda().train()
    img = torch.randn(*shape, generator=torch.Generator().manual_seed(depth + shape[2]))
    keep = []
    with _NoLibraryLayers():
        maps = net._forward_hip_train(img.cuda(), keep=keep)
        cots = _cotangents(maps)
        sum((m * c.cuda()).sum() for m, c in zip(maps, cots)).backward()
    grads = {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}
    assert len(grads) == {18: 15, 50: 42}[depth]
    assert all(n.startswith(("layer2.", "layer3.", "layer4.")) and n.endswith(("conv1.weight", "conv2.weight", "conv3.weight", "downsample.0.weight"))
               for n in grads)
    assert all(torch.isfinite(g).all() and g.abs().max() > 0 for g in grads.values())
    assert all(m.is_contiguous(memory_format=torch.channels_last) for m in maps)

    net.zero_grad(set_to_none=True)
    with _NoLibraryLayers():                                     # a second step, through forward(): the same bits
        again = net(img.cuda())
        sum((m * c.cuda()).sum() for m, c in zip(again, cots)).backward()
    assert all(torch.equal(a, b) for a, b in zip(again, maps))
    assert {n for n, p in net.named_parameters() if p.grad is not None} == set(grads)
    assert all(torch.equal(p.grad, grads[n]) for n, p in net.named_parameters() if p.grad is not None)

    with torch.no_grad():
        eval_maps = net.eval()(img.cuda())
    net.train()
    for a, b in zip(maps, eval_maps):
        assert max_err(a, b) <= 1e-4 * b.abs().max().item()

    ref = cpu_net.double()
    rep = GatedReplica(ref)
    own = rep.run(img.double())                                  # float64 on its own gates: pre-activations and map scales
    pre, own_gates = list(rep.pre), list(rep.own_gates)
    assert len(keep) == len(pre)
    gates = [rows_to_nchw(y, p) > 0 for y, p in zip(keep, pre)]
    n_differ = n_near = n_all = 0
    for gate, own_gate, p in zip(gates, own_gates, pre):
        near = p.abs() < 1e-4 * p.abs().max()
        assert not ((gate != own_gate) & ~near).any()
        n_differ, n_near, n_all = n_differ + int((gate != own_gate).sum()), n_near + int(near.sum()), n_all + p.numel()
    print(f"resnet{depth} {shape}: {n_differ} gates differ from float64, {n_near} of {n_all} pre-activations near zero")
    assert n_near <= 0.01 * n_all
    for a, b in zip(maps, own):
        assert max_err(a, b) <= 1e-4 * b.abs().max().item()
    outs = rep.run(img.double(), gates)
    sum((m * c.double()).sum() for m, c in zip(outs, cots)).backward()
    worst, worst_name = 0.0, None
    for n, p in ref.named_parameters():
        assert (p.grad is not None) == (n in grads), n
        if p.grad is not None:
            e = max_err(grads[n], p.grad) / p.grad.abs().max().item()
            if e > worst:
                worst, worst_name = e, n
    print(f"resnet{depth} {shape}: worst parameter gradient error {worst:.3e} ({worst_name}), recorded {MEASURED[(depth, shape)]:.3e}")
    assert MEASURED[(depth, shape)] <= 2.5e-4
    assert worst <= 4 * MEASURED[(depth, shape)]


# ---- 5. a weight update is seen ------------------------------------------------------------------------------------------------
def test_weight_updates_reach_the_next_forward(monkeypatch):
    from sgcdet_amd.functions import train_weight_planes
    monkeypatch.setenv("SGC_BACKBONE_TRAIN_HIP", "1")
    net = _net(18).cuda().train()
    img = torch.randn(1, 3, 64, 96, generator=torch.Generator().manual_seed(8)).cuda()
    p = net.layer3[0].conv1.weight
    first = [m.detach().clone() for m in net(img)]
    assert all(torch.equal(a, b.detach()) for a, b in zip(first, net(img)))
    bump = 0.05 * torch.randn(p.shape, generator=torch.Generator().manual_seed(9)).cuda()
    p.data.add_(bump)                                            # no version bump: the repack of begin_step must pick it up
    train_weight_planes().begin_step()
    second = [m.detach().clone() for m in net(img)]
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    assert not torch.equal(first[2], second[2]) and not torch.equal(first[3], second[3])
    with torch.no_grad():
        p.add_(bump)                                             # bumps the version: seen without begin_step
    third = [m.detach() for m in net(img)]
    assert not torch.equal(second[2], third[2])
    with torch.no_grad():                                        # and the result is the eval path's on the same weights
        want = net.eval()(img)
    assert max_err(third[2], want[2]) <= 1e-5 * want[2].abs().max().item()


# ---- 6. images -> losses -----------------------------------------------------------------------------------------------------------
def test_forward_train_from_images(monkeypatch):
    """The SGCDet_ScanNet model config with the backbone attached, 4 views of 240 x 320: ``forward_train(batch)`` and ``backward()``
    with the backbone on the HIP kernels -- finite losses, a finite non-zero gradient on every trainable backbone parameter, one
    batched weight repack per step -- and, with ``SGC_BACKBONE_TRAIN_HIP=0``, the same call on the torch formulation."""
    import sgcdet_amd.plugin  # noqa: F401
    from sgcdet_amd.functions import train_weight_planes
    from sgcdet_amd.mmcv_lite import _wrap, build_detector
    from sgcdet_amd.scene import make_img_meta
    from targets_contract import random_boxes
    with open(os.path.join(ROOT, "tests", "golden", "ref_configs.json")) as f:
        model = _wrap(json.load(f, object_hook=lambda d: tuple(d["__tuple__"]) if set(d) == {"__tuple__"} else d)["SGCDet_ScanNet"])
    model["depth_head"] = dict(model["depth_head"], init_weight="none")
    torch.manual_seed(21)
    det = build_detector(model).attach_backbone()
    fill_resnet(det.backbone)
    det = det.cuda().train()
    n_views = 4
    meta = make_img_meta(n_views, "scannet", seed=6, img_hw=(240, 320))
    img = torch.randn(1, n_views, 3, 240, 320, generator=torch.Generator().manual_seed(23)).cuda()
    boxes, labels = random_boxes(9, 6, False)
    boxes[:, :3] *= 0.55
    batch = dict(img=img, img_metas=[meta], gt_bboxes_3d=[boxes.cuda()], gt_labels_3d=[labels.cuda()])
    trainable = {n: p for n, p in det.backbone.named_parameters() if p.requires_grad}
    assert len(trainable) == 42

    calls = []
    conv_forward = nn.Conv2d.forward

    def counting(self_, x):
        if any(self_ is m for m in backbone_convs):
            calls.append(1)
        return conv_forward(self_, x)
    backbone_convs = [m for m in det.backbone.modules() if isinstance(m, nn.Conv2d)]
    monkeypatch.setattr(nn.Conv2d, "forward", counting)

    monkeypatch.setenv("SGC_BACKBONE_TRAIN_HIP", "1")
    planes = train_weight_planes()
    launches = []
    for step in range(2):
        det.zero_grad(set_to_none=True)
        losses = det.forward_train(batch)
        assert {"loss_centerness", "loss_bbox", "loss_cls"} <= set(losses)
        assert all(torch.isfinite(v).all() for v in losses.values())
        sum(losses.values()).backward()
        launches.append(planes.launches)
        for n, p in trainable.items():
            assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, n
    assert calls == []                                           # no library convolution of the backbone ran
    assert launches[1] == launches[0] + 1                        # one batched repack per step once the planes are registered
    assert all(p.grad is None for n, p in det.backbone.named_parameters() if not p.requires_grad)

    monkeypatch.setenv("SGC_BACKBONE_TRAIN_HIP", "0")
    det.zero_grad(set_to_none=True)
    losses0 = det.forward_train(batch)
    assert len(calls) == 53                                      # every convolution of ResNet-50 on torch's formulation
    assert all(torch.isfinite(v).all() for v in losses0.values())
