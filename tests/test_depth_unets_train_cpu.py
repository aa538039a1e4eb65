"""CPU checks of ``DepthNet_Fusion``'s U-Nets and ``depth_reg`` in training on the HIP kernels (include/sgcdet_amd_depth_train.h,
plugin/conv_plan.py ``TrainConv2d(pad=True)`` / ``TrainConvTranspose2d`` / ``bn_rows(channels=...)``, plugin/depth_net.py
``_unet_train_layers`` / ``_regulation_train_hip``): the new header equals its binding tables, stays apart from
the others and is exported; every new entry has a buffer case; the identities the transposed layer's gradients and the softmax
backward are built on hold in float64; the one U-Net walk over the training layers on CPU tensors is ``SimpleUnet2D.forward`` +
autograd in float64, with exactly zero padding columns in every intermediate; ``DepthNet_Fusion.forward`` on the CPU does not see
the switch."""
import copy
import os
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sgc_bn_rows_padded_forward", "sgc_bn_rows_padded_backward", "sgc_softmax_rows_backward")


def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(sgc_[a-z0-9_]+)\s*\(", text)))


def test_header_equals_its_tables_and_the_library_exports_them():
    from sgcdet_amd import _abi, build
    new = set(_abi.DEPTH_TRAIN_SIGNATURES) | set(_abi.DEPTH_TRAIN_INTROSPECTION)
    assert _declared("sgcdet_amd_depth_train.h") == sorted(new) and set(NEW) == new
    old = set()
    for table in (_abi.SIGNATURES, _abi.INTROSPECTION, _abi.TRAIN_SIGNATURES, _abi.TRAIN_INTROSPECTION, _abi.IMAGE_SIGNATURES,
                  _abi.IMAGE_INTROSPECTION):
        old |= set(table)
    assert not new & old
    for header in ("sgcdet_amd.h", "sgcdet_amd_train.h", "sgcdet_amd_image.h"):
        assert not new & set(_declared(header)), header
    assert '#include "sgcdet_amd.h"' in open(os.path.join(ROOT, "include", "sgcdet_amd_depth_train.h")).read()
    assert [len(_abi.DEPTH_TRAIN_SIGNATURES[n]) for n in NEW] == [18, 18, 9]          # the stream included
    assert _abi.ABI_VERSION == 4                                  # no existing argument list changed
    lib = _abi.Library(build.build(), train=True)                 # raises ImportError on a missing symbol
    assert all(hasattr(lib._dll, n) for n in NEW)
    assert _abi.Library(build.build())._dll.sgc_softmax_rows_backward.argtypes is None     # bound with the training tables only


def test_every_new_entry_point_that_writes_device_memory_has_a_case():
    """The assertion of tests/test_buffers_cpu.py ``test_every_entry_point_that_writes_device_memory_has_a_case`` for the new tables."""
    from sgcdet_amd import _abi
    from buffer_cases import CASES as OLD
    from buffer_cases_depth_train import CASES
    names = set(_abi.DEPTH_TRAIN_SIGNATURES) | set(_abi.DEPTH_TRAIN_INTROSPECTION)
    excluded = {n for n in names if n.endswith(("_supported", "_workspace_floats", "_workspace_bytes"))}
    covered = set()
    for case in CASES:
        assert case.entries, f"{case}: names no entry point"
        assert set(case.entries) <= names, f"{case}: unknown entry point {set(case.entries) - names}"
        assert case.only == "cuda" and case.ref is not None
        covered |= set(case.entries)
    assert not (covered & excluded)
    uncovered = sorted(names - excluded - covered)
    assert not uncovered, f"{len(uncovered)} entry points that write device memory have no case: {uncovered}"
    ids = [c.name for c in CASES] + [c.name for c in OLD]
    assert len(ids) == len(set(ids))


def test_buffer_cases_build_finite_references_with_safe_gates():
    from buffer_cases_depth_train import BN_CASES, CASES, bn_padded_conditioned, gate_margin
    for case in CASES:
        ref = case.reference(None)
        assert all(bool(torch.isfinite(v.double()).all()) for v in ref.values()), case.name
    for c in BN_CASES:
        if c[3]:
            assert gate_margin(bn_padded_conditioned(*c)[1]["pre"]) > 1e-4, c


# ---- the identities in float64 -----------------------------------------------------------------------------------
def test_transposed_convolution_gradient_identities():
    """For ConvTranspose2d(3, stride 2, padding 1, output_padding 1) with parameter w [Cin, Cout, 3, 3]: the input gradient is the
    stride-2 3x3 convolution of dy with w read as a Conv2d weight [out = Cin][in = Cout], taps not mirrored; the weight gradient is
    the weight gradient of that same convolution with the operands swapped (dy as its input, x as its output gradient)."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 8, 3, 5, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(8, 4, 3, 3, generator=g, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(2, 4, 6, 10, generator=g, dtype=torch.float64)
    y = F.conv_transpose2d(x, w, stride=2, padding=1, output_padding=1)
    assert y.shape == dy.shape
    dx, dw = torch.autograd.grad(y, (x, w), dy)
    assert (F.conv2d(dy, w.detach(), stride=2, padding=1) - dx).abs().max() < 1e-13
    probe = w.detach().clone().requires_grad_(True)
    swapped, = torch.autograd.grad(F.conv2d(dy, probe, stride=2, padding=1), probe, x.detach())
    assert swapped.shape == dw.shape and (swapped - dw).abs().max() < 1e-13
    # the sum the header states, spelled out for one element
    ci, co, kh, kw = 5, 2, 0, 2
    s = sum(x[n, ci, i, j] * dy[n, co, 2 * i + kh - 1, 2 * j + kw - 1] for n in range(2) for i in range(3) for j in range(5)
            if 0 <= 2 * i + kh - 1 < 6 and 0 <= 2 * j + kw - 1 < 10)
    assert abs(float(s.detach()) - float(dw[ci, co, kh, kw])) < 1e-12


def test_softmax_backward_identity():
    g = torch.Generator().manual_seed(4)
    z = torch.randn(7, 12, generator=g, dtype=torch.float64, requires_grad=True)
    dp = torch.randn(7, 12, generator=g, dtype=torch.float64)
    p = torch.softmax(z, 1)
    want, = torch.autograd.grad(p, z, dp)
    got = p.detach() * (dp - (p.detach() * dp).sum(1, keepdim=True))
    assert (got - want).abs().max() < 1e-15


# ---- the walk over the training layers on CPU tensors -------------------------------------------------------------------------------
def _unet(c, seed):
    from sgcdet_amd.plugin.depth_net import SimpleUnet2D
    g = torch.Generator().manual_seed(seed)
    u = SimpleUnet2D(c).double().train()
    with torch.no_grad():
        for p in u.parameters():
            p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) * (0.3 if p.dim() > 1 else 0.5) + (1.0 if p.dim() == 1 else 0.0))
        for m in u.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.copy_(0.2 * torch.randn(m.running_mean.shape, generator=g, dtype=torch.float64))
                m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=g, dtype=torch.float64))
    return u, g


def _pad32(n):
    return (n + 31) // 32 * 32


class _Recording(dict):
    """The layers of a plan, each wrapped so that its output rows are kept."""

    def __init__(self, layers, kept):
        super().__init__({k: self._wrap(v, kept) for k, v in layers.items()})

    @staticmethod
    def _wrap(layer, kept):
        def call(*a, **k):
            y, nhw = layer(*a, **k)
            kept.append((y, layer.cout))
            return y, nhw
        return call


@pytest.mark.parametrize("c", [12, 32, 44])
def test_unet_walk_over_the_training_layers_is_the_module(c):
    from sgcdet_amd.plugin.depth_net import DepthNet_Fusion, _unet_train_layers
    N, H, W = 2, 8, 12
    u, g = _unet(c, 100 + c)
    ref = copy.deepcopy(u)
    x = torch.randn(N, c, H, W, generator=g, dtype=torch.float64)
    cot = torch.randn(N, c, H, W, generator=g, dtype=torch.float64)
    xr = x.clone().requires_grad_(True)
    want = ref(xr)
    (want * cot).sum().backward()
    cp = _pad32(c)
    rows = F.pad(x.permute(0, 2, 3, 1).reshape(-1, c), (0, cp - c)).requires_grad_(True)
    kept = []
    got = DepthNet_Fusion._unet(None, rows, _Recording(_unet_train_layers(u), kept), (N, H, W))
    assert got.shape == (N * H * W, cp) and len(kept) == 6
    for y, cout in kept:                                        # every intermediate: zeros behind its channels, exactly
        assert y.shape[1] == _pad32(cout) and bool((y[:, cout:] == 0).all()) and not bool(torch.signbit(y[:, cout:]).any())
    (got[:, :c] * cot.permute(0, 2, 3, 1).reshape(-1, c)).sum().backward()

    def close(a, b, what):
        assert a.shape == b.shape and (a - b).abs().max() <= 1e-10 * b.abs().max(), what
    close(got[:, :c].detach(), want.detach().permute(0, 2, 3, 1).reshape(-1, c), "output")
    close(rows.grad[:, :c], xr.grad.permute(0, 2, 3, 1).reshape(-1, c), "input gradient")
    assert bool((rows.grad[:, c:] == 0).all())
    for (n, p), (_, q) in zip(u.named_parameters(), ref.named_parameters()):
        assert p.grad is not None, n
        close(p.grad, q.grad, n)
    for (n, a), (_, b) in zip(u.named_buffers(), ref.named_buffers()):
        if a.is_floating_point():
            close(a, b, n)
        else:
            assert int(a) == int(b) == 1, n                     # num_batches_tracked


def test_padded_norm_off_the_kernels_ignores_the_padding_and_returns_zeros():
    from sgcdet_amd.plugin.conv_plan import bn_rows
    g = torch.Generator().manual_seed(9)
    bn, bn2 = nn.BatchNorm2d(12).double().train(), nn.BatchNorm2d(12).double().train()
    x, res = torch.randn(30, 12, generator=g, dtype=torch.float64), torch.randn(30, 12, generator=g, dtype=torch.float64)
    nanpad = lambda t: torch.cat([t, torch.full((30, 20), float("nan"), dtype=torch.float64)], 1)          # noqa: E731
    y = bn_rows(bn, nanpad(x), (1, 5, 6), residual=nanpad(res), relu=True, image=True, channels=12, relu_then_add=True)
    want = F.relu(bn2(x.view(1, 5, 6, 12).permute(0, 3, 1, 2))).permute(0, 2, 3, 1).reshape(30, 12) + res
    assert y.shape == (30, 32) and (y[:, :12] - want).abs().max() < 1e-13 and bool((y[:, 12:] == 0).all())
    assert (bn.running_var - bn2.running_var).abs().max() < 1e-14 and int(bn.num_batches_tracked) == 1
    with pytest.raises(ValueError):
        bn_rows(bn, x, (1, 5, 6), relu=True, image=True, relu_then_add=True)


# ---- the module on the CPU ---------------------------------------------------------------------------------------------------------
def test_forward_on_the_cpu_does_not_see_the_switch(monkeypatch):
    import sgcdet_amd.plugin as P
    from golden_util import fill_by_name
    from sgcdet_amd.scene import make_img_meta
    net = P.DepthNet_Fusion(neighbor_img_num=2, downsample_factor=4, dbound=[0.2, 5.0, 0.4], mono_channels=32, loss_weight=0.5,
                            max_tol=0, init_weight="none")
    fill_by_name(net, base_seed=7, scale=0.15)
    net.train()
    g = torch.Generator().manual_seed(2)
    xs, imgs = torch.randn(1, 4, 32, 8, 8, generator=g), torch.randn(1, 4, 3, 32, 32, generator=g)     # 4 views: the fewest with 2 neighbours each
    meta = make_img_meta(4, "scannet", seed=3, img_hw=(32, 32))
    assert not net._train_hip_ok(xs, imgs)
    outs, stats = [], []
    for value in (None, "1", "0"):
        if value is None:
            monkeypatch.delenv("SGC_DEPTH_NET_TRAIN_UNETS", raising=False)
        else:
            monkeypatch.setenv("SGC_DEPTH_NET_TRAIN_UNETS", value)
        n = copy.deepcopy(net)
        outs.append(n(xs, imgs, [meta], 4))
        stats.append(n.fusion_regulation.conv11[1].running_var.clone())
    n = copy.deepcopy(net)                                        # the reference formulation, spelled out
    f = n.fnet_mvs(imgs[0])
    cost = n.correlation_regulation(n.correlation(f, meta, 4))
    want = F.softmax(n.depth_reg(n.fusion_regulation(torch.cat([cost, n.mono_regulation(n.fnet_mono(xs[0]))], dim=1))), dim=1)
    for o, s in zip(outs, stats):
        assert torch.equal(o[0], want) and torch.equal(s, stats[0])
    monkeypatch.setenv("SGC_DEPTH_NET_TRAIN_UNETS", "1")
    assert net._train_unets_ok()                                  # the switch and the modules would allow it: the device does not
    net.mono_regulation.conv2.bn = nn.SyncBatchNorm(256)
    assert not net._train_unets_ok()                              # a converted norm keeps the torch formulation
