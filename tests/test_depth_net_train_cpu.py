"""CPU checks of ``DepthNet_Fusion``'s feature extractors in training on the HIP kernels (plugin/depth_net.py ``_train_hip_ok`` /
``fnet_mvs_rows``, plugin/conv_plan.py ``TrainConv2d`` / ``TrainStem7`` / ``bn_rows``): the new entry points are
declared, bound and exported and the workspace query answers on the host; the live-norm 2-D layer on CPU tensors is the
``nn.Module`` composition (outputs, gradients, running statistics); the one trunk walk on torch stand-ins is ``ResNetFPN.forward``
in train mode; the path predicate follows its switches; dropping the identity block's outer ReLU does not change a gradient."""
import copy
import os
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sgc_conv2d_stem7_wgrad_bf16x3", "sgc_conv2d_stem7_wgrad_workspace_floats")


def test_new_entry_points_are_declared_bound_and_exported():
    from sgcdet_amd import build
    from sgcdet_amd._abi import ABI_VERSION, TRAIN_INTROSPECTION, TRAIN_SIGNATURES, Library
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sgcdet_amd_train.h")).read(), flags=re.S)
    assert set(NEW) <= set(re.findall(r"\b(sgc_[a-z0-9_]+)\s*\(", text))
    assert len(TRAIN_SIGNATURES["sgc_conv2d_stem7_wgrad_bf16x3"]) == 9 and "sgc_conv2d_stem7_wgrad_workspace_floats" in TRAIN_INTROSPECTION
    assert ABI_VERSION == 4                                      # no existing argument list changed
    lib = Library(build.build(), train=True)                     # raises ImportError on a missing symbol
    assert all(hasattr(lib._dll, name) for name in NEW)


def test_workspace_query_answers_on_the_host():
    from sgcdet_amd import build
    from sgcdet_amd._abi import Library
    lib = Library(build.build(), train=True)
    q = lib._dll.sgc_conv2d_stem7_wgrad_workspace_floats
    assert q(1, 64, 80) == 8 * 64 * 147                          # 4 x 2 tiles of 8 x 32 output pixels: one slot per workgroup
    assert q(40, 240, 320) == 512 * 64 * 147                     # config 2: 3000 tiles over 512 workgroups
    assert q(1, 8, 12) == 0 and q(1, 2, 2) == 0                  # one tile: not split
    assert q(3, 2, 2) == 3 * 64 * 147
    for bad, word in (((1, 7, 12), "even"), ((1, 8, 11), "even"), ((0, 8, 12), "non-positive"), ((-1, 8, 12), "non-positive"),
                      ((1, 0, 12), "non-positive"), ((1 << 14, 512, 512), "4 GiB")):
        assert q(*bad) == -1 and word in lib.last_error(), bad


# ---- the live-norm 2-D layer on CPU tensors -----------------------------------------------------------------------------------------
def _rows(x):
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])


def _randomise(bn, g):
    with torch.no_grad():
        bn.weight.copy_(0.5 + torch.rand(bn.weight.shape, generator=g)), bn.bias.copy_(0.2 * torch.randn(bn.bias.shape, generator=g))
        bn.running_mean.copy_(0.2 * torch.randn(bn.bias.shape, generator=g)), bn.running_var.copy_(0.5 + torch.rand(bn.bias.shape, generator=g))


@pytest.mark.parametrize("tail", ["relu", "relu_then_add", "add_then_relu"])
@pytest.mark.parametrize("k,stride", [(3, 1), (3, 2), (1, 1), (1, 2)])
@pytest.mark.parametrize("bias", [True, False])
def test_train_conv2d_is_the_module_composition(k, stride, tail, bias):
    from sgcdet_amd.plugin.conv_plan import TrainConv2d
    g = torch.Generator().manual_seed(10 * k + stride)
    N, H, W, cin, cout = 2, 5, 7, 6, 8
    conv, bn = nn.Conv2d(cin, cout, k, stride, k // 2, bias=bias).double(), nn.BatchNorm2d(cout).double().train()
    _randomise(bn, g)
    conv2, bn2 = copy.deepcopy(conv), copy.deepcopy(bn)
    x = torch.randn(N, cin, H, W, generator=g, dtype=torch.float64)
    OH, OW = (H + stride - 1) // stride, (W + stride - 1) // stride
    res = torch.randn(N, cout, OH, OW, generator=g, dtype=torch.float64)
    cot = torch.randn(N, cout, OH, OW, generator=g, dtype=torch.float64)

    xa, ra = x.clone().requires_grad_(True), res.clone().requires_grad_(True)
    y = bn(conv(xa))
    want = {"relu": lambda: F.relu(y), "relu_then_add": lambda: F.relu(y) + ra, "add_then_relu": lambda: F.relu(y + ra)}[tail]()
    (want * cot).sum().backward()

    xb, rb = x.clone().requires_grad_(True), res.clone().requires_grad_(True)
    layer = TrainConv2d(conv2, bn2)
    assert layer.conv is conv2 and layer.bn is bn2 and layer.cout == cout
    kw = {"relu": dict(), "relu_then_add": dict(residual=_rows(rb)), "add_then_relu": dict(residual=_rows(rb), relu=False, relu_after_add=True)}[tail]
    got, onhw = layer(_rows(xb), (N, H, W), **kw)
    assert onhw == (N, OH, OW) and got.shape == (N * OH * OW, cout)
    (got * _rows(cot)).sum().backward()

    assert (got - _rows(want)).abs().max() <= 1e-12
    assert (xb.grad - xa.grad).abs().max() <= 1e-11 * xa.grad.abs().max()
    if tail != "relu":
        assert (rb.grad - ra.grad).abs().max() <= 1e-12
    for (n, p), (_, q) in zip(list(conv2.named_parameters()) + list(bn2.named_parameters()), list(conv.named_parameters()) + list(bn.named_parameters())):
        assert p.grad is not None and (p.grad - q.grad).abs().max() <= 1e-11 * max(1.0, q.grad.abs().max().item()), n
    assert (bn2.running_mean - bn.running_mean).abs().max() <= 1e-12 and (bn2.running_var - bn.running_var).abs().max() <= 1e-12
    assert int(bn2.num_batches_tracked) == 1 == int(bn.num_batches_tracked)


def test_train_conv2d_without_a_norm_and_other_norm_modules():
    from sgcdet_amd.plugin.conv_plan import TrainConv2d, bn_rows
    g = torch.Generator().manual_seed(3)
    conv = nn.Conv2d(6, 8, 1)
    x = torch.randn(2, 6, 4, 5, generator=g)
    got, onhw = TrainConv2d(conv, None)(_rows(x), (2, 4, 5), relu=False)
    assert onhw == (2, 4, 5) and (got - _rows(conv(x))).abs().max() <= 1e-6       # fp32, 6 products: the memory format may reorder them
    with pytest.raises(NotImplementedError):
        TrainConv2d(conv, None)(_rows(x), (2, 4, 5))                 # a ReLU without a norm: no such layer in the trunk
    with pytest.raises(NotImplementedError):
        TrainConv2d(conv, nn.BatchNorm2d(8))(_rows(x), (2, 4, 5), relu=True, relu_after_add=True)
    # any other norm module is called as a module on the 4-D NCHW view of the rows
    seen = []

    class Other(nn.GroupNorm):
        def forward(self, t):
            seen.append(tuple(t.shape))
            return super().forward(t)
    gn = Other(2, 8)
    y = conv(x)
    got = bn_rows(gn, _rows(y), (2, 4, 5), relu=True, image=True)
    assert seen == [(2, 8, 4, 5)] and (got - _rows(F.relu(nn.GroupNorm.forward(gn, y)))).abs().max() <= 1e-6


def test_bn_rows_on_a_batchnorm3d_is_unchanged():
    from sgcdet_amd.plugin.conv_plan import bn_rows
    g = torch.Generator().manual_seed(4)
    bn = nn.BatchNorm3d(8).train()
    _randomise(bn, g)
    twin = copy.deepcopy(bn)
    x = torch.randn(1, 8, 3, 4, 5, generator=g)
    res = torch.randn(60, 8, generator=g)
    rows = x[0].permute(1, 2, 3, 0).reshape(60, 8)
    got = bn_rows(bn, rows, (3, 4, 5), residual=res, relu=True)
    want = F.relu(twin(x)[0].permute(1, 2, 3, 0).reshape(60, 8) + res)
    assert (got - want).abs().max() <= 1e-6
    assert torch.allclose(bn.running_mean, twin.running_mean, atol=1e-7) and torch.allclose(bn.running_var, twin.running_var, atol=1e-6)
    assert int(bn.num_batches_tracked) == 1
    got_eval = bn_rows(bn.eval(), rows, (3, 4, 5))
    assert (got_eval - twin.eval()(x)[0].permute(1, 2, 3, 0).reshape(60, 8)).abs().max() <= 1e-6 and int(bn.num_batches_tracked) == 1


# ---- the one walk over the trunk -------------------------------------------------------------------------------------------------------
class TorchLayer:
    """``Conv2dSpec``'s call signature on torch modules, called once per forward each."""

    def __init__(self, conv, bn, log):
        self.conv, self.bn, self.cout, self.log = conv, bn, conv.out_channels, log

    def __call__(self, x, nhw, residual=None, relu=True, relu_after_add=False):
        self.log.append((self.conv, residual is not None, relu, relu_after_add))
        y = self.conv(x.view(nhw[0], nhw[1], nhw[2], -1).permute(0, 3, 1, 2))
        y = _rows(y if self.bn is None else self.bn(y))
        s = self.conv.stride[0]
        if relu:
            y = F.relu(y)
        if residual is not None:
            y = y + residual
        if relu_after_add:
            y = F.relu(y)
        return y, (nhw[0], (nhw[1] + s - 1) // s, (nhw[2] + s - 1) // s)


def _trunk():
    from sgcdet_amd.plugin.depth_net import ResNetFPN
    torch.manual_seed(0)
    net = ResNetFPN(output_dim=16, init_weight="none").double().train()
    g = torch.Generator().manual_seed(1)
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            _randomise(m, g)
    return net, torch.randn(2, 3, 16, 24, generator=g, dtype=torch.float64)


@pytest.mark.parametrize("layers", ["stand-ins", "TrainConv2d"])
def test_the_walk_is_resnetfpn_forward_in_train_mode(layers):
    from sgcdet_amd.plugin.conv_plan import TrainConv2d, TrainStem7
    from sgcdet_amd.plugin.depth_net import fnet_mvs_plan, fnet_mvs_rows
    net, img = _trunk()
    twin = copy.deepcopy(net)
    want = net(img)
    want.square().sum().backward()
    log = []
    if layers == "stand-ins":
        def stem(conv, bn):
            return lambda im: (_rows(F.relu(bn(conv(im)))), (im.shape[0], im.shape[2] // 2, im.shape[3] // 2))
        plan = fnet_mvs_plan(twin, lambda conv, bn: TorchLayer(conv, bn, log), stem)
    else:
        plan = fnet_mvs_plan(twin, TrainConv2d, TrainStem7)
    got = fnet_mvs_rows(img, plan)
    assert got.shape == want.shape and got.is_contiguous(memory_format=torch.channels_last)
    assert (got - want).abs().max() <= 1e-11 * want.abs().max()
    got.square().sum().backward()
    top = max(q.grad.abs().max().item() for q in net.parameters())
    for (n, p), (_, q) in zip(twin.named_parameters(), net.named_parameters()):
        # a convolution bias in front of a batch-statistics norm has a zero gradient in exact arithmetic: rounding noise of the
        # largest gradient in both runs, so it is held to that scale
        scale = q.grad.abs().max().item()
        assert p.grad is not None and (p.grad - q.grad).abs().max() <= 1e-9 * (scale if scale >= 1e-6 * top else top), n
    bns = [m for m in twin.modules() if isinstance(m, nn.BatchNorm2d)]
    assert len(bns) == 10 and twin.layer2[0].downsample[1] is twin.layer2[0].bn3
    assert all(int(m.num_batches_tracked) == 1 for m in bns)                      # bn3 included: normalised and updated once
    for (n, a), (_, b) in zip(twin.named_buffers(), net.named_buffers()):
        assert (a.double() - b.double()).abs().max() <= 1e-12, n
    if layers == "stand-ins":
        assert len(log) == 10 and [c for c, *_ in log].count(twin.layer2[0].downsample[0]) == 1
        # identity blocks: relu(.) + x without the outer ReLU; the projection block: the ReLU behind the add
        assert [(r, relu, after) for _, r, relu, after in log if r] == [(True, True, False)] * 2 + [(True, False, True)] + [(True, True, False)]


def test_eval_plan_keeps_the_prepared_stem():
    from sgcdet_amd.plugin.conv_plan import Conv2dSpec, Stem7Spec
    from sgcdet_amd.plugin.depth_net import ResNetFPN, fnet_mvs_plan, stem7_spec
    net = ResNetFPN(output_dim=16, init_weight="none").eval()
    plan = fnet_mvs_plan(net, Conv2dSpec, stem7_spec)
    assert isinstance(plan["stem"], Stem7Spec) and plan["stem"].w.shape == (64, 160) and len(plan["blocks"]) == 4
    assert isinstance(plan["final"], Conv2dSpec) and plan["final"].cout == 16 and "down" in plan["blocks"][2]


# ---- the path predicate ---------------------------------------------------------------------------------------------------------------
class _OnGpu:
    """A CPU tensor that says it lives on the GPU: the predicate reads flags and shapes only."""

    def __init__(self, t, requires_grad=False):
        self.t, self.requires_grad, self.is_cuda = t, requires_grad, True
        self.shape, self.dtype = t.shape, t.dtype

    def dim(self):
        return self.t.dim()


def test_path_predicate(monkeypatch):
    import sgcdet_amd.plugin  # noqa: F401
    from sgcdet_amd.plugin import conv_plan
    from sgcdet_amd.plugin.depth_net import DepthNet_Fusion
    monkeypatch.delenv("SGC_DEPTH_NET_TRAIN_HIP", raising=False)
    net = DepthNet_Fusion(2, 4, [0.2, 5.0, 0.4], mono_channels=32, init_weight="none").train()
    xs, imgs = torch.zeros(1, 4, 32, 8, 12), torch.zeros(1, 4, 3, 32, 48)
    ok = lambda x=xs, im=imgs, **kw: net._train_hip_ok(_OnGpu(x), _OnGpu(im, **kw))     # noqa: E731
    default = ok()
    from sgcdet_amd.plugin import depth_net
    assert default == (depth_net.TRAIN_HIP_DEFAULT != "0")
    monkeypatch.setenv("SGC_DEPTH_NET_TRAIN_HIP", "1")
    assert ok()
    with torch.no_grad():
        assert ok()                                              # train mode without autograd: the same path, the same numbers
    monkeypatch.setenv("SGC_DEPTH_NET_TRAIN_HIP", "0")
    assert not ok()
    monkeypatch.setenv("SGC_DEPTH_NET_TRAIN_HIP", "1")
    assert not ok(requires_grad=True)                            # the stem has no input gradient
    assert not net.eval()._train_hip_ok(_OnGpu(xs), _OnGpu(imgs))
    net.train()
    monkeypatch.setattr(conv_plan, "CONV_PRODUCTS", 2)           # fp16 mode: inference-only
    assert not ok()
    monkeypatch.setattr(conv_plan, "CONV_PRODUCTS", 3)
    monkeypatch.setattr(conv_plan, "CONV_MODE", "f32")
    assert not ok()
    monkeypatch.setattr(conv_plan, "CONV_MODE", "bf16x3")
    assert not ok(torch.zeros(1, 4, 32, 7, 12), torch.zeros(1, 4, 3, 28, 48))          # an odd stride-2 stage
    assert not ok(torch.zeros(1, 4, 32, 8, 12), torch.zeros(1, 4, 3, 32, 40))          # images that are not 4x the map
    assert not ok(torch.zeros(1, 4, 48, 8, 12))                                       # mono_channels % 32 != 0
    assert not ok(xs.half()) and not ok(xs, imgs.double())
    assert ok()
    assert not net._train_hip_ok(xs, imgs)                       # CPU tensors keep the torch formulation


def test_cpu_tensors_keep_the_torch_formulation(monkeypatch):
    import sgcdet_amd.plugin  # noqa: F401
    from sgcdet_amd.plugin import depth_net
    from sgcdet_amd.scene import make_img_meta
    monkeypatch.setenv("SGC_DEPTH_NET_TRAIN_HIP", "1")
    monkeypatch.setattr(depth_net, "fnet_mvs_rows", lambda *a, **k: pytest.fail("the kernel walk ran on CPU tensors"))
    torch.manual_seed(2)
    net = depth_net.DepthNet_Fusion(2, 4, [0.2, 5.0, 0.4], mono_channels=32, init_weight="none").train()
    meta = make_img_meta(4, "scannet", seed=1, img_hw=(16, 16))
    pred = net(torch.randn(1, 4, 32, 4, 4), torch.randn(1, 4, 3, 16, 16), [meta], 4)
    assert pred.shape == (1, 4, net.depth_channels, 4, 4) and pred.requires_grad
    assert int(net.fnet_mvs.layer2[0].bn3.num_batches_tracked) == 1


# ---- the dropped outer ReLU of the identity block -------------------------------------------------------------------------------------
def test_dropping_the_outer_relu_of_the_identity_block_keeps_every_gradient():
    """relu(x + relu(t)) against x + relu(t) with x = relu(s) >= 0, on inputs where some sums are exactly 0: there both addends
    are 0 and came through closed gates (relu'(0) = 0), so both formulations send 0 down both paths."""
    g = torch.Generator().manual_seed(5)
    s = torch.randint(-3, 4, (64, 16), generator=g).double()     # many exact zeros and negatives
    t = torch.randint(-3, 4, (64, 16), generator=g).double()
    cot = torch.randn(64, 16, generator=g, dtype=torch.float64)
    grads = []
    for outer in (True, False):
        sa, ta = s.clone().requires_grad_(True), t.clone().requires_grad_(True)
        x, y = F.relu(sa), F.relu(ta)
        out = F.relu(x + y) if outer else x + y
        if outer:
            zero = (out.detach() == 0)
            assert zero.any() and (x.detach()[zero] == 0).all() and (y.detach()[zero] == 0).all()
        (out * cot).sum().backward()
        grads.append((out.detach(), sa.grad, ta.grad))
    assert all(torch.equal(a, b) for a, b in zip(*grads))
    assert (grads[0][1] == 0).any() and (grads[0][1] != 0).any()
