"""``DepthNet_Fusion``'s feature extractors in training on the HIP kernels (include/sgcdet_amd_train.h section 14,
csrc/stem7_wgrad.hip, functions.py ``Stem7ConvFunction``, plugin/conv_plan.py ``TrainConv2d`` / ``TrainStem7``,
plugin/depth_net.py).

References are float64 torch on the CPU, computed here.  The stem's weight gradient is held to exact equality where the arithmetic
is exact (integer operands: every product and partial sum is an integer below 2^24) and to 1e-4 of the gradient's max-abs otherwise,
the bf16x3 bound tests/test_gpu_resnet_train.py holds the sibling weight gradient to; the layers likewise, each compared tensor to
1e-4 of its max-abs.  A gradient that is zero in exact arithmetic (a convolution bias in front of a batch-statistics norm) is held
to 1e-5 of the largest gradient, the "cancelled" rule of tests/test_gpu_plane_sweep_grad.py.  The whole trunk against float64 goes
through nine live norms, which amplify rounding: its bound is four times the measured worst case (MEASURED).

The trunk and the module tests condition their inputs the way the layer test does: no ReLU gate may differ between the two
computations that are compared, and each test counts the gates itself.  Of twelve input seeds tried for each on an MI355X, the
trunk had no flipped gate for 1 (worst gradient error 3.6e-5) and one to three flipped gates for 11 (worst gradient error 4e-3 to
1.4e-1 in 10 of them: one flipped gate moves a 768-row sum by a few per cent); the module had no flipped U-Net gate for 2 seeds (no mismatch) and
one to three for 10 (a mismatch in 7 of them).

Measured on an MI355X (profiles/r18_depth_net_train_parity.json): see MEASURED below."""
import copy
import json
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from golden_util import fill_by_name, max_err

pytestmark = pytest.mark.gpu

# what an MI355X gave: worst error relative to the compared tensor's max-abs
MEASURED = dict(stem_wgrad=7.48e-6, stem_wgrad_no_workspace=7.48e-6, layer=1.014e-5, trunk_forward=1.870e-5, trunk_param_grad=3.642e-5)
TRUNK_MARGIN = 4.0          # the trunk's bound is MEASURED["trunk_param_grad"] * TRUNK_MARGIN: nine live norms amplify rounding


@pytest.fixture(scope="module", autouse=True)
def _leave_nothing_behind():
    """The training Functions register weight planes per parameter storage and keep an alias of it: drop the ones of this module's
    nets (they would pin the dead parameters and be repacked by every later ``begin_step``) and hand the cached blocks back."""
    yield
    if torch.cuda.is_available():
        from sgcdet_amd.functions import train_weight_planes
        train_weight_planes().clear()
        torch.cuda.empty_cache()


def _record(key, value):
    """Print a figure and, when SGC_DEPTH_NET_TRAIN_PARITY_JSON names a file, keep its worst case there."""
    print(f"depth-net train parity: {key} {value:.3e} (recorded {MEASURED.get(key.split('/')[0])})")
    path = os.environ.get("SGC_DEPTH_NET_TRAIN_PARITY_JSON")
    if path:
        rec = json.load(open(path)) if os.path.exists(path) else {}
        rec[key] = max(rec.get(key, 0.0), value)
        with open(path, "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)


# ---- 1. sgc_conv2d_stem7_wgrad_bf16x3 ---------------------------------------------------------------------------------------------
SIZES = [(2, 2), (8, 12), (14, 6), (38, 50), (64, 80)]


def _stem_case(N, H, W, kind):
    g = torch.Generator().manual_seed(1000 * N + 10 * H + W)
    if kind == "integers":
        img = torch.randint(-8, 9, (N, 3, H, W), generator=g).float()
        dy = torch.randint(-8, 9, (N * (H // 2) * (W // 2), 64), generator=g).float()
    else:
        img, dy = torch.randn(N, 3, H, W, generator=g), torch.randn(N * (H // 2) * (W // 2), 64, generator=g)
    w = torch.zeros(64, 3, 7, 7, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(img.double(), w, stride=2, padding=3)
    want, = torch.autograd.grad(y, w, dy.double().view(N, H // 2, W // 2, 64).permute(0, 3, 1, 2))
    return img, dy, want


def test_stem_wgrad_workspace_query(gpu_ops):
    q = gpu_ops.conv2d_stem7_wgrad_workspace_floats
    assert q(1, 64, 80) > 0 and q(3, 64, 80) > q(1, 64, 80)      # the largest shape is split ...
    assert q(1, 2, 2) == 0 and q(1, 8, 12) == 0 and q(1, 14, 6) == 0      # ... and these are not: one tile
    assert q(3, 2, 2) > 0                                        # one tile per image


@pytest.mark.parametrize("hw", SIZES)
@pytest.mark.parametrize("N", [1, 3])
def test_stem_wgrad_against_float64(gpu_ops, N, hw):
    H, W = hw
    img, dy, want = _stem_case(N, H, W, "integers")
    assert want.abs().max() < 2 ** 24
    for ws in (True, False):
        got = gpu_ops.conv2d_stem7_wgrad_bf16x3(img.cuda(), dy.cuda(), workspace=ws)
        assert got.shape == (64, 3, 7, 7) and torch.equal(got.cpu(), want.float()), ("integers", ws)
    img, dy, want = _stem_case(N, H, W, "randn")
    ig, dg = img.cuda(), dy.cuda()
    got = gpu_ops.conv2d_stem7_wgrad_bf16x3(ig, dg)
    scale = want.abs().max().item()
    err = max_err(got, want) / scale
    _record("stem_wgrad", err)
    assert err <= 1e-4
    assert torch.equal(got, gpu_ops.conv2d_stem7_wgrad_bf16x3(ig, dg))           # bit-identical run to run
    err0 = max_err(gpu_ops.conv2d_stem7_wgrad_bf16x3(ig, dg, workspace=False), want) / scale
    _record("stem_wgrad_no_workspace", err0)
    assert err0 <= 1e-4
    assert torch.equal(ig.cpu(), img) and torch.equal(dg.cpu(), dy)            # the operands are read only


def test_stem_wgrad_refusals(gpu_ops):
    from sgcdet_amd._abi import SgcError
    img, dy = torch.zeros(2, 3, 8, 12).cuda(), torch.zeros(2 * 4 * 6, 64).cuda()
    dw = torch.full((64, 3, 7, 7), 7.0).cuda()
    call = lambda *a: gpu_ops._call("sgc_conv2d_stem7_wgrad_bf16x3", *a)       # noqa: E731
    with pytest.raises(RuntimeError, match="even H and W"):                   # the front end, before the entry
        gpu_ops.conv2d_stem7_wgrad_bf16x3(torch.zeros(2, 3, 7, 12).cuda(), dy)
    with pytest.raises(RuntimeError, match="dy must be"):
        gpu_ops.conv2d_stem7_wgrad_bf16x3(img, dy[:-1])
    for args, word in (((img, dy, dw, 2, 7, 12, None, 0), "even"), ((img, dy, dw, 2, 8, 11, None, 0), "even"),
                       ((None, dy, dw, 2, 8, 12, None, 0), "null"), ((img, None, dw, 2, 8, 12, None, 0), "null"),
                       ((img, dy, None, 2, 8, 12, None, 0), "null"),
                       ((img.view(-1)[1:], dy, dw, 1, 8, 12, None, 0), "aligned"), ((img, dy.view(-1)[1:], dw, 1, 8, 12, None, 0), "aligned"),
                       ((img, dy, dw.view(-1)[1:], 1, 2, 2, None, 0), "aligned"),
                       ((img, dy, dw, 0, 8, 12, None, 0), "non-positive"), ((img, dy, dw, 2, -8, 12, None, 0), "non-positive"),
                       ((img, dy, dw, 2, 8, 0, None, 0), "non-positive")):
        with pytest.raises(SgcError, match=word):
            call(*args)
    torch.cuda.synchronize()
    assert (dw == 7.0).all()                                     # nothing was launched
    with pytest.raises(RuntimeError, match="non-positive"):
        gpu_ops.conv2d_stem7_wgrad_workspace_floats(0, 8, 12)


def test_stem_function_against_float64(gpu_ops):
    """``Stem7ConvFunction``: forward, the weight gradient (the new kernel) and the bias gradient (``sgc_rows_colsum``); the planes
    are packed from the live parameter at every call, so an in-place update of the weight is seen by the next forward."""
    from sgcdet_amd.functions import Stem7ConvFunction
    g = torch.Generator().manual_seed(17)
    img, w, b = torch.randn(2, 3, 14, 18, generator=g), 0.1 * torch.randn(64, 3, 7, 7, generator=g), 0.3 * torch.randn(64, generator=g)
    cot = torch.randn(2 * 7 * 9, 64, generator=g)
    wd, bd = w.double().requires_grad_(True), b.double().requires_grad_(True)
    want = F.conv2d(img.double(), wd, bd, stride=2, padding=3).permute(0, 2, 3, 1).reshape(-1, 64)
    (want * cot.double()).sum().backward()
    wg, bg = w.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    y = Stem7ConvFunction.apply(img.cuda(), wg, bg)
    (y * cot.cuda()).sum().backward()
    for name, got, ref in (("forward", y, want), ("dw", wg.grad, wd.grad), ("db", bg.grad, bd.grad)):
        e = max_err(got, ref) / ref.abs().max().item()
        _record("layer/stem_" + name, e)
        assert got.shape == ref.shape and e <= 1e-4, name
    with torch.no_grad():
        wg.mul_(2.0)
        y2 = Stem7ConvFunction.apply(img.cuda(), wg, None)
    assert max_err(y2, 2.0 * (want.detach() - bd.detach())) <= 1e-4 * want.abs().max().item()
    with pytest.raises(RuntimeError, match="no input gradient"):
        Stem7ConvFunction.apply(img.cuda().requires_grad_(True), wg, bg)


# ---- 2. the live-norm layer --------------------------------------------------------------------------------------------------------
FORMS = dict(k3s1_relu=(3, 1, "relu"), k3s2_relu=(3, 2, "relu"), k1s2_add_relu=(1, 2, "add_then_relu"), k3s1_relu_add=(3, 1, "relu_then_add"))
# seeds for which no pre-activation of the float64 reference lies within 1e-4 of its tensor's max-abs of zero (no ReLU gate can
# flip under the kernels' rounding); the test checks the condition itself
LAYER_SEEDS = {
    ("k3s1_relu", (2, 6, 8), 32): 49, ("k3s1_relu", (2, 6, 8), 64): 81, ("k3s1_relu", (2, 5, 7), 32): 14, ("k3s1_relu", (2, 5, 7), 64): 14,
    ("k3s2_relu", (2, 6, 8), 32): 1, ("k3s2_relu", (2, 6, 8), 64): 2, ("k3s2_relu", (2, 5, 7), 32): 3, ("k3s2_relu", (2, 5, 7), 64): 1,
    ("k1s2_add_relu", (2, 6, 8), 32): 5, ("k1s2_add_relu", (2, 6, 8), 64): 1, ("k1s2_add_relu", (2, 5, 7), 32): 1,
    ("k1s2_add_relu", (2, 5, 7), 64): 1,
    ("k3s1_relu_add", (2, 6, 8), 32): 49, ("k3s1_relu_add", (2, 6, 8), 64): 81, ("k3s1_relu_add", (2, 5, 7), 32): 14,
    ("k3s1_relu_add", (2, 5, 7), 64): 14,
}


def _layer_case(form, nhw, cin, seed):
    k, s, tail = FORMS[form]
    N, H, W = nhw
    OH, OW = (H + s - 1) // s, (W + s - 1) // s
    g = torch.Generator().manual_seed(seed)
    conv, bn = nn.Conv2d(cin, 64, k, s, k // 2), nn.BatchNorm2d(64).train()
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) / (k * cin ** 0.5)), conv.bias.copy_(0.3 * torch.randn(64, generator=g))
        bn.weight.copy_(0.5 + torch.rand(64, generator=g)), bn.bias.copy_(0.3 * torch.randn(64, generator=g))
        bn.running_mean.copy_(0.2 * torch.randn(64, generator=g)), bn.running_var.copy_(0.5 + torch.rand(64, generator=g))
    x, res = torch.randn(N * H * W, cin, generator=g), torch.randn(N * OH * OW, 64, generator=g)
    cot = torch.randn(N * OH * OW, 64, generator=g)
    return conv, bn, x, (res if tail != "relu" else None), cot, (N, OH, OW)


def _layer_reference(form, nhw, conv, bn, x, res, cot):
    """float64: (output, pre-activation, gradients by name, running statistics)."""
    tail = FORMS[form][2]
    N, H, W = nhw
    conv, bn = copy.deepcopy(conv).double(), copy.deepcopy(bn).double()
    xd = x.double().requires_grad_(True)
    rd = None if res is None else res.double().requires_grad_(True)
    t = bn(conv(xd.view(N, H, W, -1).permute(0, 3, 1, 2))).permute(0, 2, 3, 1).reshape(-1, 64)
    pre = t + rd if tail == "add_then_relu" else t
    out = F.relu(pre) + rd if tail == "relu_then_add" else F.relu(pre)
    (out * cot.double()).sum().backward()
    grads = dict(dx=xd.grad, dw=conv.weight.grad, dbias=conv.bias.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad)
    if rd is not None:
        grads["dres"] = rd.grad
    return out.detach(), pre.detach(), grads, dict(running_mean=bn.running_mean, running_var=bn.running_var)


def gate_margin(pre):
    return (pre.abs().min() / pre.abs().max()).item()


@pytest.mark.parametrize("cin", [32, 64])
@pytest.mark.parametrize("nhw", [(2, 6, 8), (2, 5, 7)])
@pytest.mark.parametrize("form", list(FORMS))
def test_train_conv2d_against_float64(gpu_ops, form, nhw, cin):
    from sgcdet_amd.plugin.conv_plan import TrainConv2d
    seed = LAYER_SEEDS[(form, nhw, cin)]
    conv, bn, x, res, cot, onhw_want = _layer_case(form, nhw, cin, seed)
    want, pre, ref_grads, ref_stats = _layer_reference(form, nhw, conv, bn, x, res, cot)
    assert gate_margin(pre) > 1e-4, "choose another seed: a ReLU gate could flip"
    tail = FORMS[form][2]
    conv_g, bn_g = conv.cuda(), bn.cuda()
    twin = TrainConv2d(copy.deepcopy(conv_g), copy.deepcopy(bn_g))
    xg = x.cuda().requires_grad_(True)
    rg = None if res is None else res.cuda().requires_grad_(True)
    kw = {"relu": dict(), "relu_then_add": dict(residual=rg), "add_then_relu": dict(residual=rg, relu=False, relu_after_add=True)}[tail]
    names = []
    gpu_ops.event_log, gpu_ops.event_names = [], None
    try:
        got, onhw = TrainConv2d(conv_g, bn_g)(xg, nhw, **kw)
        (got * cot.cuda()).sum().backward()
        torch.cuda.synchronize()
        names = [e[0] for e in gpu_ops.event_log]
    finally:
        gpu_ops.event_log = None
    assert onhw == onhw_want and got.shape == want.shape
    assert names.count("sgc_bn_rows_act_forward") == 1 and names.count("sgc_conv2d_wgrad_bf16x3") == 1 and names.count("sgc_rows_colsum") == 1
    got_grads = dict(dx=xg.grad, dw=conv_g.weight.grad, dbias=conv_g.bias.grad, dgamma=bn_g.weight.grad, dbeta=bn_g.bias.grad)
    if rg is not None:
        got_grads["dres"] = rg.grad
    top = max(v.abs().max().item() for v in ref_grads.values())
    worst = max_err(got, want) / want.abs().max().item()
    assert worst <= 1e-4, "forward"
    for name, ref in ref_grads.items():
        assert got_grads[name] is not None and got_grads[name].shape == ref.shape, name
        if name == "dbias":                                      # zero in exact arithmetic: the batch mean removes the bias
            e = max_err(got_grads[name], ref) / top
            print(f"train conv2d {form} {nhw} {cin}: cancelled dbias err {e:.3e} of the largest gradient")
            assert ref.abs().max().item() <= 1e-9 * top and e <= 1e-5
            continue
        e = max_err(got_grads[name], ref) / ref.abs().max().item()
        worst = max(worst, e)
        assert e <= 1e-4, name
    for name, ref in ref_stats.items():
        e = max_err(getattr(bn_g, name), ref) / ref.abs().max().item()
        worst = max(worst, e)
        assert e <= 1e-4, name
    assert int(bn_g.num_batches_tracked) == 1
    _record("layer/" + form, worst)
    with torch.no_grad():                                        # train mode without autograd: the same numbers
        again, _ = twin(x.cuda(), nhw, **{k_: (v.detach() if torch.is_tensor(v) else v) for k_, v in kw.items()})
    assert torch.equal(again, got.detach())
    assert torch.equal(twin.bn.running_mean, bn_g.running_mean) and torch.equal(twin.bn.running_var, bn_g.running_var)


# ---- 3. the module -----------------------------------------------------------------------------------------------------------------
KERNELS = {"sgc_conv2d_stem7_bf16x3", "sgc_conv2d_stem7_wgrad_bf16x3", "sgc_conv2d_wgrad_bf16x3", "sgc_bn_rows_act_forward"}


INPUT_SEED = 1        # see test_depth_net_trains_its_extractors_on_the_kernels: no ReLU gate of the U-Nets differs between the two runs


class _UnetGates:
    """The ReLU gates of the torch-formulated part of a ``DepthNet_Fusion`` forward: the sign pattern of every U-Net BatchNorm's
    output (a ReLU follows each) and of ``mono_regulation``'s input (``fnet_mono``'s ReLU output)."""

    def __init__(self, net):
        self.gates, self.handles = [], []
        for name, m in net.named_modules():
            if isinstance(m, nn.BatchNorm2d) and name.split(".")[0].endswith("_regulation"):
                self.handles.append(m.register_forward_hook(lambda _m, _i, out: self.gates.append(out.detach() > 0)))
        self.handles.append(net.mono_regulation.register_forward_pre_hook(lambda _m, inp: self.gates.append(inp[0].detach() > 0)))

    def close(self):
        for h in self.handles:
            h.remove()


def _depth_net(seed=INPUT_SEED):
    import sgcdet_amd.plugin as P
    from sgcdet_amd.scene import make_img_meta
    net = P.DepthNet_Fusion(neighbor_img_num=2, downsample_factor=4, dbound=[0.2, 5.0, 0.4], mono_channels=32, loss_weight=0.5,
                            max_tol=0, init_weight="none")
    fill_by_name(net, base_seed=7, scale=0.15)
    g = torch.Generator().manual_seed(seed)
    xs, imgs = torch.randn(1, 4, 32, 8, 12, generator=g), torch.randn(1, 4, 3, 32, 48, generator=g)
    return net.cuda().train(), xs.cuda(), imgs.cuda(), make_img_meta(4, "scannet", seed=3, img_hw=(32, 48))


def _depth_net_step(ops, net, xs, imgs, meta, switch, monkeypatch):
    monkeypatch.setenv("SGC_DEPTH_NET_TRAIN_HIP", switch)
    ops.event_log, ops.event_names = [], KERNELS
    gates = _UnetGates(net)
    try:
        net.zero_grad(set_to_none=True)
        pred = net(xs, imgs, [meta], 4)
        w = torch.linspace(-1, 1, pred.numel(), device=pred.device).view_as(pred)
        (pred * w).sum().backward()
        torch.cuda.synchronize()
        names = [e[0] for e in ops.event_log]
    finally:
        ops.event_log = ops.event_names = None
        gates.close()
    return pred.detach(), {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None}, names, gates.gates


def _gradient_mismatches(grads, grads_r):
    """The criteria of tests/test_gpu_plane_sweep_grad.py's training test: finite; direction (cosine > 0.9999) and 5e-2 of the
    gradient's scale; a gradient below 1e-3 of the largest one (cancelled: a bias in front of a batch-statistics norm) within 1e-5 of
    the largest."""
    top = max(float(r.abs().max()) for r in grads_r.values())
    bad = []
    for n, g in grads.items():
        r = grads_r[n]
        if not torch.isfinite(g).all():
            bad.append((n, "not finite"))
            continue
        scale, err = float(r.abs().max()), float((g - r).abs().max())
        if scale < 1e-3 * top:
            if err > 1e-5 * top:
                bad.append((n, "cancelled", err, top))
            continue
        cos = float(F.cosine_similarity(g.flatten().double(), r.flatten().double(), dim=0))
        if cos <= 0.9999 or err > 5e-2 * scale:
            bad.append((n, cos, err, scale))
    return bad


def test_depth_net_trains_its_extractors_on_the_kernels(gpu_ops, monkeypatch):
    net, xs, imgs, meta = _depth_net()
    net_ref = copy.deepcopy(net)
    pred, grads, names, gates = _depth_net_step(gpu_ops, net, xs, imgs, meta, "1", monkeypatch)
    assert names.count("sgc_conv2d_stem7_bf16x3") == 1 and names.count("sgc_conv2d_stem7_wgrad_bf16x3") == 1
    assert names.count("sgc_conv2d_wgrad_bf16x3") == 11          # the trunk's 10 convolutions + fnet_mono
    assert names.count("sgc_bn_rows_act_forward") == 11          # the stem's norm, 9 in the blocks, fnet_mono's
    pred_r, grads_r, names_r, gates_r = _depth_net_step(gpu_ops, net_ref, xs, imgs, meta, "0", monkeypatch)
    assert names_r == []
    assert float((pred - pred_r).abs().max()) < 1e-5
    assert set(grads) == set(grads_r) == {n for n, _ in net.named_parameters()}
    # condition on the inputs: no ReLU gate of the torch-formulated U-Nets differs between the two runs.  Their maps are tiny here
    # (a 4 x 6 map at the coarsest stage): ONE gate that flips under the 1e-6 rounding difference of the two extractors moves a
    # bias gradient by 10 %, which is no statement about either formulation.  INPUT_SEED is a seed for which none flips.
    flips = sum(int((a != b).sum()) for a, b in zip(gates, gates_r))
    print(f"depth net: {flips} of {sum(a.numel() for a in gates)} U-Net gates differ between the two runs")
    assert len(gates) == len(gates_r) == 19 and flips == 0, "choose another INPUT_SEED: a ReLU gate flipped"
    bad = _gradient_mismatches(grads, grads_r)
    print("depth net gradient mismatches:", bad)
    assert not bad, bad
    bns = {n: m for n, m in net.named_modules() if isinstance(m, nn.BatchNorm2d)}
    bns_r = dict(net_ref.named_modules())
    assert len(bns) >= 11 + 18 and "fnet_mvs.layer2.0.bn3" in bns
    for n, m in bns.items():
        assert int(m.num_batches_tracked) == 1 == int(bns_r[n].num_batches_tracked), n
        for stat in ("running_mean", "running_var"):
            a, b = getattr(m, stat), getattr(bns_r[n], stat)
            assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()), (n, stat)
    # train mode without autograd takes the same path (batch statistics: the running ones do not enter the result)
    monkeypatch.setenv("SGC_DEPTH_NET_TRAIN_HIP", "1")
    gpu_ops.event_log, gpu_ops.event_names = [], KERNELS
    try:
        with torch.no_grad():
            again = net(xs, imgs, [meta], 4)
        torch.cuda.synchronize()
        names = [e[0] for e in gpu_ops.event_log]
    finally:
        gpu_ops.event_log = gpu_ops.event_names = None
    assert names.count("sgc_conv2d_stem7_bf16x3") == 1 and names.count("sgc_bn_rows_act_forward") == 11
    assert float((again - pred).abs().max()) < 1e-5


TRUNK_SEED = 13       # see test_trunk_against_float64: every ReLU gate of the kernels' run equals the float64 reference's


def _walk_with_gates(monkeypatch, img, net):
    """``fnet_mvs_rows`` over the training layers of ``net`` (on the tensors' device: the kernels on the GPU, torch on the CPU --
    tests/test_depth_net_train_cpu.py holds the latter to ``ResNetFPN.forward``) -> (features, the ReLU gates of its ten norms)."""
    from sgcdet_amd.plugin import conv_plan
    from sgcdet_amd.plugin.depth_net import fnet_mvs_plan, fnet_mvs_rows
    gates, real = [], conv_plan.bn_rows

    def spy(*a, **k):
        out = real(*a, **k)
        gates.append((out.detach() > 0).cpu())
        return out
    monkeypatch.setattr(conv_plan, "bn_rows", spy)
    try:
        return fnet_mvs_rows(img, fnet_mvs_plan(net, conv_plan.TrainConv2d, conv_plan.TrainStem7)), gates
    finally:
        monkeypatch.setattr(conv_plan, "bn_rows", real)


def test_trunk_against_float64(gpu_ops, monkeypatch):
    """The extractor alone: ``ResNetFPN.train()`` forward + backward on the kernels against a float64 CPU copy.  Condition on the
    input: no ReLU gate differs from the reference's.  With ~250 000 gates a random image has a handful of pre-activations within
    the kernels' 1e-5 of zero; one flipped gate of the stem moved ``bn1.bias``'s gradient by 2.5 % and ``conv1.weight``'s by 4.7 %
    (sums over 768 rows) while every other gradient agreed to 3e-5 -- that measures the input, not the kernels."""
    from sgcdet_amd.plugin.depth_net import ResNetFPN
    net = fill_by_name(ResNetFPN(output_dim=128, init_weight="none"), base_seed=11, scale=0.15).train()
    g = torch.Generator().manual_seed(TRUNK_SEED)
    img = torch.randn(2, 3, 32, 48, generator=g)
    ref = copy.deepcopy(net).double()
    want, gates_ref = _walk_with_gates(monkeypatch, img.double(), ref)
    assert (want - copy.deepcopy(ref)(img.double())).abs().max() <= 1e-11 * want.abs().max()       # the walk on the CPU is the module
    cot = torch.randn(want.shape, generator=g)
    (want * cot.double()).sum().backward()
    net = net.cuda()
    got, gates = _walk_with_gates(monkeypatch, img.cuda(), net)
    flips = [int((a != b).sum()) for a, b in zip(gates, gates_ref)]
    print(f"trunk: gates that differ from float64, per norm: {flips} of {[a.numel() for a in gates]}")
    assert len(gates) == len(gates_ref) == 10 and sum(flips) == 0, "choose another TRUNK_SEED: a ReLU gate flipped"
    assert got.shape == want.shape and got.is_contiguous(memory_format=torch.channels_last)
    (got * cot.cuda()).sum().backward()
    fwd = max_err(got, want) / want.abs().max().item()
    _record("trunk_forward", fwd)
    top = max(p.grad.abs().max().item() for p in ref.parameters())
    worst = 0.0
    for (n, p), (_, q) in zip(net.named_parameters(), ref.named_parameters()):
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
        scale = q.grad.abs().max().item()
        e = max_err(p.grad, q.grad) / (scale if scale >= 1e-3 * top else top)
        print(f"trunk {n}: gradient err {e:.3e}")
        worst = max(worst, e)
    _record("trunk_param_grad", worst)
    assert all(int(m.num_batches_tracked) == 1 for m in net.modules() if isinstance(m, nn.BatchNorm2d))
    for (n, a), (_, b) in zip(net.named_buffers(), ref.named_buffers()):
        if a.is_floating_point():
            assert max_err(a, b) <= 1e-4 * b.abs().max().item(), n
    assert fwd <= TRUNK_MARGIN * MEASURED["trunk_forward"] and worst <= TRUNK_MARGIN * MEASURED["trunk_param_grad"]


# ---- 4. the detector ---------------------------------------------------------------------------------------------------------------
def test_forward_train_from_fpn_trains_the_extractors_on_the_kernels(gpu_ops, monkeypatch):
    """The plumbing config of tests/test_gpu_plane_sweep_grad.py ``_plumbing_detector`` (4 views, maps 60 x 80, images 240 x 320)."""
    import sgcdet_amd.plugin  # noqa: F401
    from sgcdet_amd.mmcv_lite import build_detector
    from sgcdet_amd.scene import make_scene, model_config, workload
    from targets_contract import random_boxes
    monkeypatch.setenv("SGC_DEPTH_NET_TRAIN_HIP", "1")
    w = workload("cfg1_plumbing")
    cfg = model_config(w)
    cfg["depth_head"] = dict(type="DepthNet_Fusion", neighbor_img_num=2, downsample_factor=4, dbound=[0.2, 5, 0.4],
                             mono_channels=w["embed_dims"], loss_weight=0.5, max_tol=0, init_weight="none")
    cfg["depth_loss"], cfg["use_gt_dpt"] = False, False
    torch.manual_seed(31)
    det = build_detector(cfg).cuda().train()
    for m in det.modules():
        if isinstance(m, nn.Dropout):
            m.p = 0.0
    N = 4
    feats, _, meta = make_scene(N, w["embed_dims"], kind="scannet", seed=14, device="cuda")
    H, W = feats[0].shape[-2:]
    gen = torch.Generator().manual_seed(5)
    img = torch.randn(1, N, 3, 4 * H, 4 * W, generator=gen).cuda()
    boxes, gl = random_boxes(9, 6, False)
    boxes[:, :3] *= 0.55
    assert det.depth_head._train_hip_ok(feats[0], img)
    gpu_ops.event_log, gpu_ops.event_names = [], KERNELS
    try:
        losses = det.forward_train_from_fpn(feats, img, [meta], [boxes.cuda()], [gl.cuda()])
        sum(losses.values()).backward()
        torch.cuda.synchronize()
        names = [e[0] for e in gpu_ops.event_log]
    finally:
        gpu_ops.event_log = gpu_ops.event_names = None
    assert names.count("sgc_conv2d_stem7_bf16x3") == 1 and names.count("sgc_conv2d_stem7_wgrad_bf16x3") == 1
    got = {n: p.grad for n, p in det.named_parameters() if n.startswith("depth_head.")}
    assert got and all(g is not None and torch.isfinite(g).all() for g in got.values())
    assert any(float(g.abs().max()) > 0 for n, g in got.items() if n.startswith("depth_head.fnet_mvs."))
    with torch.no_grad():
        dpt = det.depth_distribution(feats, img, [meta], None)
        want = det.forward_train_from_features(feats, [meta], dpt, [boxes.cuda()], [gl.cuda()])
    assert set(losses) == {"loss_centerness", "loss_bbox", "loss_cls"}
    for kname in losses:
        a, b = float(losses[kname].detach()), float(want[kname])
        assert abs(a - b) <= 1e-4 * max(1.0, abs(b)), (kname, a, b)
