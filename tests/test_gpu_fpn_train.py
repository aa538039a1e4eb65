"""The image FPN's training path on the HIP kernels (include/sgcdet_amd_train.h section 13, csrc/fpn_train.hip, functions.py
``FrozenNormConv2dFunction`` with a trainable bias and ``UpsampleNearestAddFunction``, plugin/fpn.py).

References are float64 on the CPU.  The streaming kernels are held to exact equality where the arithmetic is exact (an fp32 sum of
two numbers; sums of small integers in any order) and to bounds that follow from their summation chains otherwise: the top-down
backward adds at most four terms in the tested shapes (3 * 2^-24 of the sum of magnitudes, asserted as 1e-6 of the max-abs), the
column sum passes a value through at most 160 dependent additions (160 * 2^-24 of the column's sum of magnitudes).  Convolution
results are within 1e-4 of the compared tensor's max-abs, the bf16x3 bound of tests/test_gpu_resnet_train.py for the same kernels.

Measured on an MI355X (profiles/r16_fpn_train_parity.json): see MEASURED below.
"""
import copy
import json
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from golden_util import max_err

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# what an MI355X gave for the module case (worst relative error over the 16 parameter gradients / the input gradients / the outputs)
MEASURED = dict(param_grad=1.020e-5, input_grad=7.03e-6, forward=6.57e-6)


def _index(dst, src):
    from sgcdet_amd.plugin.fpn import _nearest_index
    return _nearest_index(dst, src, "cpu")


# ---- 1. the top-down kernels ---------------------------------------------------------------------------------------------------
_TOP_DOWN = [((8, 10), (4, 5)), ((15, 20), (8, 10)), ((9, 13), (5, 7)), ((3, 4), (2, 2)), ((1, 1), (1, 1))]


@pytest.mark.parametrize("C", [32, 96])
@pytest.mark.parametrize("fine_hw,coarse_hw", _TOP_DOWN)
def test_upsample_add_forward_equals_index_and_add(gpu_ops, fine_hw, coarse_hw, C):
    N, (Hd, Wd), (Hs, Ws) = 2, fine_hw, coarse_hw
    g = torch.Generator().manual_seed(Hd * 100 + Wd + C)
    fine, coarse = torch.randn(N, Hd, Wd, C, generator=g), torch.randn(N, Hs, Ws, C, generator=g)
    want = fine + coarse[:, _index(Hd, Hs)][:, :, _index(Wd, Ws)]
    assert torch.equal(want.permute(0, 3, 1, 2), fine.permute(0, 3, 1, 2) + F.interpolate(coarse.permute(0, 3, 1, 2), size=(Hd, Wd), mode="nearest"))
    fg, cg = fine.cuda().view(-1, C), coarse.cuda().view(-1, C)
    got = gpu_ops.upsample_nearest_add_nhwc(fg, cg, (N, Hd, Wd), (N, Hs, Ws))
    assert got.data_ptr() != fg.data_ptr() and torch.equal(fg.cpu(), fine.view(-1, C))          # out of place: fine is untouched
    assert torch.equal(got.cpu().view(N, Hd, Wd, C), want)
    same = gpu_ops.upsample_nearest_add_nhwc(fg, cg, (N, Hd, Wd), (N, Hs, Ws), out=fg)           # the aliased form
    assert same is fg and torch.equal(fg, got)


@pytest.mark.parametrize("C", [32, 96])
@pytest.mark.parametrize("fine_hw,coarse_hw", _TOP_DOWN)
def test_upsample_add_backward_against_float64(gpu_ops, fine_hw, coarse_hw, C):
    N, (Hd, Wd), (Hs, Ws) = 2, fine_hw, coarse_hw
    g = torch.Generator().manual_seed(Hd * 100 + Wd + C + 1)
    for kind in ("integers", "randn"):
        gout = torch.randint(-8, 9, (N, Hd, Wd, C), generator=g).float() if kind == "integers" else torch.randn(N, Hd, Wd, C, generator=g)
        coarse = torch.zeros(N, C, Hs, Ws, dtype=torch.float64, requires_grad=True)
        up = F.interpolate(coarse, size=(Hd, Wd), mode="nearest")
        want, = torch.autograd.grad(up, coarse, gout.double().permute(0, 3, 1, 2))
        want = want.permute(0, 2, 3, 1).reshape(-1, C)
        got = gpu_ops.upsample_nearest_add_backward_nhwc(gout.cuda().view(-1, C), (N, Hd, Wd), (N, Hs, Ws))
        assert got.shape == want.shape
        if kind == "integers":                                   # every sum is exact in any order
            assert torch.equal(got.cpu(), want.float())
        else:
            err = max_err(got, want) / want.abs().max().item()
            print(f"upsample_add_backward {fine_hw} <- {coarse_hw} C {C}: err {err:.3e} of max-abs")
            assert err <= 1e-6
        assert torch.equal(got, gpu_ops.upsample_nearest_add_backward_nhwc(gout.cuda().view(-1, C), (N, Hd, Wd), (N, Hs, Ws)))


def test_top_down_kernels_refuse_bad_arguments(gpu_ops):
    from sgcdet_amd._abi import SgcError
    fine, coarse = torch.zeros(2 * 4 * 4, 32).cuda(), torch.zeros(2 * 2 * 2, 32).cuda()
    with pytest.raises(RuntimeError, match="inconsistent"):
        gpu_ops.upsample_nearest_add_nhwc(fine, coarse, (2, 4, 4), (2, 2, 3))
    with pytest.raises(SgcError, match="larger"):
        gpu_ops.upsample_nearest_add_nhwc(coarse, fine, (2, 2, 2), (2, 4, 4))
    with pytest.raises(SgcError, match="larger"):
        gpu_ops.upsample_nearest_add_backward_nhwc(coarse, (2, 2, 2), (2, 4, 4))
    with pytest.raises(SgcError, match="C % 4"):
        gpu_ops.upsample_nearest_add_nhwc(torch.zeros(2 * 4 * 4, 30).cuda(), torch.zeros(2 * 2 * 2, 30).cuda(), (2, 4, 4), (2, 2, 2))


# ---- 2. sgc_rows_colsum -----------------------------------------------------------------------------------------------------------
COLSUM_CHAIN = 160          # the longest chain of dependent fp32 additions the entry allows itself (csrc/fpn_train.hip)


@pytest.mark.parametrize("C", [32, 36, 256])
@pytest.mark.parametrize("rows", [1, 63, 257, 4097, 19200])
def test_colsum_of_integers_is_exact(gpu_ops, rows, C):
    """|v| <= 8 and rows <= 19 200: every partial sum is an integer below 2^24, so any order gives the float64 sum."""
    x = torch.randint(-8, 9, (rows, C), generator=torch.Generator().manual_seed(rows + C)).float()
    got = gpu_ops.rows_colsum(x.cuda())
    assert got.shape == (C,) and torch.equal(got.cpu(), x.double().sum(0).float())
    assert (gpu_ops.rows_colsum_workspace_floats(rows, C) > 0) == (rows > 64)


def test_colsum_of_randn_within_the_chain_bound(gpu_ops):
    x = torch.randn(19200, 256, generator=torch.Generator().manual_seed(7))
    xg = x.cuda()
    got = gpu_ops.rows_colsum(xg)
    want, mag = x.double().sum(0), x.double().abs().sum(0)
    ratio = ((got.cpu().double() - want).abs() / (2.0 ** -24 * mag)).max().item()
    print(f"rows_colsum 19200 x 256: worst column error {ratio:.3f} x 2^-24 x sum|x| (bound {COLSUM_CHAIN})")
    assert ratio <= COLSUM_CHAIN
    assert torch.equal(got, gpu_ops.rows_colsum(xg))


def test_colsum_refuses_what_it_does_not_cover(gpu_ops):
    calls = []
    real = gpu_ops._call

    def spy(name, *a, **k):
        calls.append(name)
        return real(name, *a, **k)
    gpu_ops._call = spy
    try:
        with pytest.raises(RuntimeError, match="C % 4"):
            gpu_ops.rows_colsum(torch.zeros(8, 30).cuda())
        with pytest.raises(RuntimeError, match="chain bound"):
            gpu_ops.rows_colsum(torch.empty(1 << 25, 4, device="cuda"))        # 16 384 partial sums: 212 additions
        with pytest.raises(RuntimeError, match=r"\[rows, C\]"):
            gpu_ops.rows_colsum(torch.zeros(8, 4, 4).cuda())
    finally:
        del gpu_ops._call
    assert calls == []                                           # refused before the entry point, so nothing was launched
    from sgcdet_amd._abi import SgcError
    x, out = torch.zeros(4097, 32).cuda(), torch.zeros(32).cuda()
    with pytest.raises(SgcError, match="workspace"):             # the entry itself: a split shape without its workspace
        gpu_ops._call("sgc_rows_colsum", x, out, 4097, 32, None, 0)
    with pytest.raises(SgcError, match="aligned"):
        gpu_ops._call("sgc_rows_colsum", x.view(-1)[1:1 + 8 * 32].view(8, 32), out, 8, 32, None, 0)


# ---- 3. the Function: a convolution with a trainable bias ------------------------------------------------------------------------
def _bias_case(k, nhw, cin, cout):
    N, H, W = nhw
    g = torch.Generator().manual_seed(1000 * k + 10 * H + cin + cout)
    x = torch.randn(N * H * W, cin, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) / (k * cin ** 0.5)
    b = 0.3 * torch.randn(cout, generator=g)
    cot = torch.randn(N * H * W, cout, generator=g)
    return x, w, b, cot


@pytest.mark.parametrize("nhw", [(2, 8, 10), (2, 9, 13), (1, 15, 20)])
@pytest.mark.parametrize("k", [1, 3])
def test_bias_function_against_float64(gpu_ops, k, nhw):
    from sgcdet_amd.functions import FrozenNormConv2dFunction
    N, H, W = nhw
    for cin, cout in ((32, 32), (64, 32), (96, 64)):
        x, w, b, cot = _bias_case(k, nhw, cin, cout)
        xd, wd, bd = (t.double().requires_grad_(True) for t in (x, w, b))
        want = F.conv2d(xd.view(N, H, W, cin).permute(0, 3, 1, 2), wd, bd, padding=k // 2).permute(0, 2, 3, 1).reshape(-1, cout)
        (want * cot.double()).sum().backward()
        xg, wg, bg = (t.cuda().requires_grad_(True) for t in (x, w, b))
        y = FrozenNormConv2dFunction.apply(xg, wg, None, None, None, nhw, 1, False, False, bg)
        (y * cot.cuda()).sum().backward()
        tag = f"bias function k{k} {nhw} {cin}->{cout}"
        for name, got, ref in (("forward", y, want), ("dx", xg.grad, xd.grad), ("dw", wg.grad, wd.grad)):
            assert got is not None and got.shape == ref.shape, (tag, name)
            e = max_err(got, ref) / ref.abs().max().item()
            print(f"{tag}: {name} err {e:.3e}")
            assert e < 1e-4, (tag, name)
        assert torch.equal(bg.grad, gpu_ops.rows_colsum(cot.cuda()))
        ratio = ((bg.grad.cpu().double() - bd.grad).abs() / (2.0 ** -24 * cot.double().abs().sum(0))).max().item()
        print(f"{tag}: db err {ratio:.3f} x 2^-24 x sum|dy|")
        assert ratio <= COLSUM_CHAIN


def test_bias_function_computes_only_what_is_asked_for(gpu_ops, monkeypatch):
    from sgcdet_amd.functions import FrozenNormConv2dFunction
    from sgcdet_amd.plugin import conv_plan
    calls = []
    rows_real, wgrad_real, colsum_real = conv_plan.conv2d_rows, gpu_ops.conv2d_wgrad_bf16x3, gpu_ops.rows_colsum
    monkeypatch.setattr(conv_plan, "conv2d_rows", lambda *a, **k: (calls.append("rows"), rows_real(*a, **k))[1])
    monkeypatch.setattr(gpu_ops, "conv2d_wgrad_bf16x3", lambda *a, **k: (calls.append("wgrad"), wgrad_real(*a, **k))[1], raising=False)
    monkeypatch.setattr(gpu_ops, "rows_colsum", lambda *a, **k: (calls.append("colsum"), colsum_real(*a, **k))[1], raising=False)
    nhw = (2, 8, 10)
    x, w, b, cot = _bias_case(3, nhw, 32, 32)
    for needs, want_calls in (((1, 1, 1), ["rows", "rows", "wgrad", "colsum"]), ((0, 1, 1), ["rows", "wgrad", "colsum"]),
                              ((1, 0, 1), ["rows", "rows", "colsum"]), ((1, 1, 0), ["rows", "rows", "wgrad"]), ((0, 0, 1), ["rows", "colsum"])):
        del calls[:]
        xg, wg, bg = (t.cuda().requires_grad_(bool(n)) for t, n in zip((x, w, b), needs))
        y = FrozenNormConv2dFunction.apply(xg, wg, None, None, None, nhw, 1, False, False, bg)
        (y * cot.cuda()).sum().backward()
        assert calls == want_calls, needs
        assert [t.grad is not None for t in (xg, wg, bg)] == [bool(n) for n in needs]
    with pytest.raises(RuntimeError, match="trainable bias"):    # a bias next to a folded norm or a ReLU is refused
        FrozenNormConv2dFunction.apply(xg, wg, b.cuda(), None, None, nhw, 1, False, False, bg)
    with pytest.raises(RuntimeError, match="trainable bias"):
        FrozenNormConv2dFunction.apply(xg, wg, None, None, None, nhw, 1, True, False, bg)


def test_nine_argument_call_is_unchanged(gpu_ops):
    """``FrozenNormConv2dFunction.apply`` without a bias: the bits of its forward and of both gradients equal the composition of
    ``conv2d_rows`` + ``frozen_norm_act_backward`` + the weight gradient it consisted of before the bias form was added."""
    from sgcdet_amd.functions import FrozenNormConv2dFunction, train_weight_planes
    from sgcdet_amd.plugin.conv_plan import conv2d_rows
    nhw = (2, 8, 10)
    x, w, b, cot = _bias_case(3, nhw, 32, 64)
    g = torch.Generator().manual_seed(2)
    scale, shift = (0.5 + torch.rand(64, generator=g)).cuda(), (0.1 * torch.randn(64, generator=g)).cuda()
    xg, wg, dy = x.cuda().requires_grad_(True), w.cuda().requires_grad_(True), cot.cuda()
    y = FrozenNormConv2dFunction.apply(xg, wg, scale, shift, None, nhw, 1, True, False)
    dx, dw = torch.autograd.grad(y, (xg, wg), dy)
    planes = train_weight_planes()
    hi, lo = planes.get(wg)
    y_want = conv2d_rows(xg.detach(), hi, lo, nhw, 3, 1, scale=scale, shift=shift, relu=True)
    gated, _ = gpu_ops.frozen_norm_act_backward(dy, y_want, scale, relu=True)
    hi_t, lo_t = planes.get(wg, transpose=True, flip=True)
    dx_want = conv2d_rows(gated, hi_t, lo_t, nhw, 3, relu=False)
    dw_want = gpu_ops.unpack_conv_wgrad(gpu_ops.conv2d_wgrad_bf16x3(xg.detach(), gated, nhw, 3, 1), w.shape)
    assert y_want.abs().max() > 0 and torch.equal(y.detach(), y_want) and torch.equal(dx, dx_want) and torch.equal(dw, dw_want)


def test_upsample_add_function(gpu_ops):
    from sgcdet_amd.functions import UpsampleNearestAddFunction
    N, (Hd, Wd), (Hs, Ws), C = 2, (9, 13), (5, 7), 32
    g = torch.Generator().manual_seed(11)
    fine, coarse, cot = torch.randn(N * Hd * Wd, C, generator=g), torch.randn(N * Hs * Ws, C, generator=g), torch.randn(N * Hd * Wd, C, generator=g)
    fg, cg = fine.cuda().requires_grad_(True), coarse.cuda().requires_grad_(True)
    y = UpsampleNearestAddFunction.apply(fg, cg, (N, Hd, Wd), (N, Hs, Ws))
    assert torch.equal(y.detach(), gpu_ops.upsample_nearest_add_nhwc(fg.detach(), cg.detach(), (N, Hd, Wd), (N, Hs, Ws)))
    (y * cot.cuda()).sum().backward()
    assert torch.equal(fg.grad, cot.cuda())
    assert torch.equal(cg.grad, gpu_ops.upsample_nearest_add_backward_nhwc(cot.cuda(), (N, Hd, Wd), (N, Hs, Ws)))
    fg2 = fine.cuda().requires_grad_(True)                       # a coarse map without a graph: no backward launch, no gradient
    UpsampleNearestAddFunction.apply(fg2, coarse.cuda(), (N, Hd, Wd), (N, Hs, Ws)).sum().backward()
    assert torch.equal(fg2.grad, torch.ones_like(fg2))


# ---- 4. the module ---------------------------------------------------------------------------------------------------------------
CHANNELS, SIZES = (32, 64, 96, 128), ((15, 20), (8, 10), (4, 5), (2, 3))


def _module():
    from sgcdet_amd.plugin.fpn import FPN
    net = FPN(list(CHANNELS), 32, 4)
    g = torch.Generator().manual_seed(31)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.Conv2d):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) / (m.kernel_size[0] * m.in_channels ** 0.5))
                m.bias.copy_(0.3 * torch.randn(m.bias.shape, generator=g))
    return net


def _inputs(seed=32):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(2, c, h, w, generator=g) for c, (h, w) in zip(CHANNELS, SIZES)]


@pytest.fixture(scope="module")
def float64_reference():
    """float64 autograd of ``_forward_torch`` on the CPU: (outputs, cotangents, parameter gradients by name, input gradients).
    Inputs 1..3 require a gradient; input 0 carries no graph (the backbone's frozen first stage)."""
    net = _module().double()
    xs = [x.double().requires_grad_(i > 0) for i, x in enumerate(_inputs())]
    outs = net._forward_torch(xs)
    g = torch.Generator().manual_seed(33)
    cots = [torch.randn(o.shape, generator=g) for o in outs]
    sum((o * c.double()).sum() for o, c in zip(outs, cots)).backward()
    return ([o.detach() for o in outs], cots, {n: p.grad for n, p in net.named_parameters()}, [x.grad for x in xs])


class _NoLibraryLayers:
    """``nn.Conv2d.forward`` and ``F.interpolate`` raise while this is active."""

    def __enter__(self):
        self.conv, self.interp = nn.Conv2d.forward, F.interpolate

        def boom(*a, **k):
            raise AssertionError("a library convolution / interpolation ran")
        nn.Conv2d.forward, F.interpolate = boom, boom
        return self

    def __exit__(self, *exc):
        nn.Conv2d.forward, F.interpolate = self.conv, self.interp


def _gpu_inputs(layout):
    xs = []
    for i, x in enumerate(_inputs()):
        x = x.cuda()
        x = x.contiguous(memory_format=torch.channels_last) if layout == "channels_last" else x.contiguous()
        xs.append(x.requires_grad_(i > 0))
    return xs


def _step(net, layout, cots, cot_layout="nchw"):
    xs = _gpu_inputs(layout)
    net.zero_grad(set_to_none=True)
    with _NoLibraryLayers():
        outs = net(xs)
        cg = [c.cuda().contiguous(memory_format=torch.channels_last) if cot_layout == "channels_last" else c.cuda().contiguous() for c in cots]
        sum((o * c).sum() for o, c in zip(outs, cg)).backward()
    return outs, {n: p.grad.clone() for n, p in net.named_parameters()}, [x.grad for x in xs]


def test_eval_path_equals_the_index_and_add_formulation(gpu_ops, monkeypatch):
    """The eval lowering with the top-down step on ``sgc_upsample_nearest_add_nhwc`` in place against the formulation it
    replaces, written out: the same prepared layers, torch's index + ``add_`` between them.  fp32 a + b is one number."""
    from sgcdet_amd.plugin.conv_plan import Conv2dSpec, image_rows
    from sgcdet_amd.plugin.fpn import _nearest_index
    net = _module().cuda().eval()
    for layout in ("channels_last", "nchw"):
        xs = [x.detach() for x in _gpu_inputs(layout)]
        with torch.no_grad():
            got = net(xs)
            lat, dims = [], []
            for m, x in zip(net.lateral_convs, xs):
                rows, nhw = image_rows(x)
                lat.append(Conv2dSpec(m.conv, pad_in=False, pad_out=False, unit_scale=False)(rows, nhw, relu=False)[0])
                dims.append(nhw)
            for i in range(3, 0, -1):
                (N, Hs, Ws), (_, Hd, Wd) = dims[i], dims[i - 1]
                src = lat[i].view(N, Hs, Ws, 32)
                lat[i - 1].view(N, Hd, Wd, 32).add_(src[:, _nearest_index(Hd, Hs, src.device)][:, :, _nearest_index(Wd, Ws, src.device)])
            want = []
            for m, rows, (N, H, W) in zip(net.fpn_convs, lat, dims):
                y = Conv2dSpec(m.conv, pad_in=False, pad_out=False, unit_scale=False)(rows, (N, H, W), relu=False)[0]
                want.append(y.view(N, H, W, 32).permute(0, 3, 1, 2))
        assert len(got) == 4 and all(torch.equal(a, b) for a, b in zip(got[:4], want))


@pytest.mark.parametrize("layout", ["channels_last", "nchw"])
def test_module_training_against_float64(gpu_ops, monkeypatch, float64_reference, layout):
    monkeypatch.setenv("SGC_FPN_TRAIN_HIP", "1")
    ref_outs, cots, ref_pgrads, ref_xgrads = float64_reference
    net = _module().cuda().train()
    assert net._train_hip_ok(_gpu_inputs(layout))
    outs, pgrads, xgrads = _step(net, layout, cots)
    with torch.no_grad():
        eval_outs = copy.deepcopy(net).eval()([x.detach() for x in _gpu_inputs(layout)])
    assert len(outs) == 4
    for o, e, r in zip(outs, eval_outs, ref_outs):
        assert o.shape == r.shape and o.requires_grad and o.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(o.detach(), e)                        # the training forward IS the eval forward
    worst = dict(forward=max(max_err(o, r) / r.abs().max().item() for o, r in zip(outs, ref_outs)), param_grad=0.0, input_grad=0.0)
    assert len(pgrads) == 16
    for n, gr in pgrads.items():
        e = max_err(gr, ref_pgrads[n]) / ref_pgrads[n].abs().max().item()
        print(f"fpn {layout}: {n} gradient err {e:.3e}")
        worst["param_grad"] = max(worst["param_grad"], e)
    assert xgrads[0] is None
    for i in (1, 2, 3):
        assert xgrads[i].shape == ref_xgrads[i].shape
        e = max_err(xgrads[i], ref_xgrads[i]) / ref_xgrads[i].abs().max().item()
        print(f"fpn {layout}: input {i} gradient err {e:.3e}")
        worst["input_grad"] = max(worst["input_grad"], e)
    print(f"fpn {layout}: worst {worst}, recorded {MEASURED}")
    if os.environ.get("SGC_FPN_PARITY_JSON"):
        path = os.environ["SGC_FPN_PARITY_JSON"]
        record = json.load(open(path)) if os.path.exists(path) else {}
        record[layout] = worst
        with open(path, "w") as f:
            json.dump(record, f, indent=1)
    assert all(v < 1e-4 for v in worst.values())

    # channels-last cotangents give the same gradients, and a second step repeats every bit
    outs_cl, pgrads_cl, xgrads_cl = _step(net, layout, cots, cot_layout="channels_last")
    outs_2, pgrads_2, xgrads_2 = _step(net, layout, cots)
    for other_p, other_x in ((pgrads_cl, xgrads_cl), (pgrads_2, xgrads_2)):
        assert all(torch.equal(other_p[n], pgrads[n]) for n in pgrads)
        assert all(torch.equal(other_x[i], xgrads[i]) for i in (1, 2, 3))
    assert all(torch.equal(a.detach(), b.detach()) for a, b in zip(outs_2, outs))


def test_switch_keeps_the_torch_formulation(gpu_ops, monkeypatch, float64_reference):
    monkeypatch.setenv("SGC_FPN_TRAIN_HIP", "0")
    calls = []
    conv_forward = nn.Conv2d.forward
    monkeypatch.setattr(nn.Conv2d, "forward", lambda self_, x: (calls.append(1), conv_forward(self_, x))[1])
    net = _module().cuda().train()
    xs = _gpu_inputs("nchw")
    outs = net(xs)
    assert len(calls) == 8
    want = net._forward_torch(xs)
    assert all(torch.equal(a, b) for a, b in zip(outs, want))
    for o, r in zip(outs, float64_reference[0]):
        assert max_err(o, r) <= 1e-3 * r.abs().max().item()


# ---- 5. the detector: images -> losses ---------------------------------------------------------------------------------------------
def test_forward_train_from_images_trains_the_fpn_on_the_kernels(monkeypatch):
    """The set-up of tests/test_gpu_resnet_train.py ``test_forward_train_from_images`` (SGCDet_ScanNet, 4 views of 240 x 320):
    finite losses, a finite non-zero gradient on every FPN parameter the losses depend on, no library convolution of
    ``det.neck``, one batched weight repack per step from the second step on; with ``SGC_FPN_TRAIN_HIP=0`` the torch
    formulation's eight convolutions and gradients on the same parameters.  The detector reads three of the FPN's four outputs
    (sgcdet_amd/scene.py), so ``fpn_convs.3`` gets no gradient on either path: 14 of the 16 parameters do."""
    import sgcdet_amd.plugin  # noqa: F401
    from resnet_util import fill_resnet
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
    params = dict(det.neck.named_parameters())
    assert len(params) == 16 and all(p.requires_grad for p in params.values())
    used = {n: p for n, p in params.items() if not n.startswith("fpn_convs.3.")}
    assert len(used) == 14

    calls = []
    conv_forward = nn.Conv2d.forward
    neck_convs = [m for m in det.neck.modules() if isinstance(m, nn.Conv2d)]

    def counting(self_, x):
        if any(self_ is m for m in neck_convs):
            calls.append(1)
        return conv_forward(self_, x)
    monkeypatch.setattr(nn.Conv2d, "forward", counting)

    monkeypatch.setenv("SGC_BACKBONE_TRAIN_HIP", "1")
    monkeypatch.setenv("SGC_FPN_TRAIN_HIP", "1")
    planes = train_weight_planes()
    launches = []
    for step in range(2):
        det.zero_grad(set_to_none=True)
        losses = det.forward_train(batch)
        assert {"loss_centerness", "loss_bbox", "loss_cls"} <= set(losses)
        assert all(torch.isfinite(v).all() for v in losses.values())
        sum(losses.values()).backward()
        launches.append(planes.launches)
        for n, p in used.items():
            assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, n
        assert all(p.grad is None for n, p in params.items() if n not in used)
    assert calls == []                                           # no library convolution of the FPN ran
    assert launches[1] == launches[0] + 1                        # one batched repack per step once the planes are registered

    monkeypatch.setenv("SGC_FPN_TRAIN_HIP", "0")
    det.zero_grad(set_to_none=True)
    losses0 = det.forward_train(batch)
    assert len(calls) == 8                                       # the parent's call: every FPN convolution on torch's formulation
    assert all(torch.isfinite(v).all() for v in losses0.values())
    sum(losses0.values()).backward()
    assert {n for n, p in params.items() if p.grad is not None} == set(used)          # the same 14 there
