"""The ResNet backbone on the HIP kernels (include/sgcdet_amd_image.h, plugin/resnet.py): the max-pool against
F.max_pool2d bit for bit, the any-size strided entry of the tile kernel against float64 F.conv2d, the whole backbone against
float64 on the CPU with the library convolutions patched out, the switch in a fresh process, and images -> boxes through the
detector against the by-hand composition.

Bound of the backbone test: 1e-4 of each map's max-abs -- the per-layer contract of include/sgcdet_amd_image.h reused for the
stack of 53 layers (rounding errors of successive layers do not add coherently; DepthNet_Fusion's 31 layers measured 2.4e-6).
MEASURED_ERRORS below records what an MI355X gave (max |difference| / max |float64 map|, worst of the four maps), for the HIP path and
for the torch fp32 formulation (library convolutions) on the same device.

The end-to-end test uses 4 views, not 2: the depth head of the SGCDet_ScanNet config (``neighbor_img_num=2``) indexes view
``i +- 2`` at the ends of the sequence (``get_closest_frame_ids``, as in the reference) and needs at least 4.
"""
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from golden_util import max_err
from resnet_util import fill_resnet

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (depth, input shape) -> (HIP path, torch fp32 path), relative to each map's max-abs, against float64 on the CPU
MEASURED_ERRORS = {
    (50, (2, 3, 72, 104)): (1.164e-5, 6.14e-7),
    (18, (2, 3, 64, 96)): (1.128e-5, 3.94e-7),
    (50, (1, 3, 240, 320)): (1.328e-5, 6.86e-7),
}

REF_BACKBONE = dict(type="ResNet", depth=50, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=1,
                    norm_cfg=dict(type="BN", requires_grad=False), norm_eval=True, style="pytorch",
                    pretrained="torchvision://resnet50")


# ---- sgc_maxpool2d_nhwc --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nhwc", [(2, 7, 10, 64), (1, 6, 9, 32), (3, 12, 20, 64), (1, 1, 1, 4), (2, 5, 5, 36)])
@pytest.mark.parametrize("kind", ["normal", "negative"])
def test_maxpool_equals_torch(gpu_ops, nhwc, kind):
    """Bit for bit F.max_pool2d(x, 3, 2, 1); the all-negative input shows that the padding takes no part in the maximum."""
    N, H, W, C = nhwc
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn(N, H, W, C, generator=g)
    if kind == "negative":
        x = -x.abs() - 0.5
    got, onhw = gpu_ops.maxpool2d_nhwc(x.view(-1, C).cuda(), (N, H, W))
    want = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1)
    assert onhw == (N, want.shape[2], want.shape[3]) == (N, (H - 1) // 2 + 1, (W - 1) // 2 + 1)
    assert got.shape == (N * onhw[1] * onhw[2], C)
    assert torch.equal(got.cpu().view(N, onhw[1], onhw[2], C).permute(0, 3, 1, 2), want)
    assert torch.isfinite(got).all() and (kind == "normal" or (got < 0).all())


def test_maxpool_refuses_channels_not_a_multiple_of_4(gpu_ops):
    from sgcdet_amd._abi import SgcError
    x = torch.randn(2 * 3 * 6, 6).cuda()
    with pytest.raises(SgcError, match="status -3") as e:
        gpu_ops.maxpool2d_nhwc(x, (2, 3, 6))
    assert "C % 4" in str(e.value)


# ---- sgc_conv2d_nhwc_strided_bf16x3 --------------------------------------------------------------------------------------------
def _ref_conv(x, w, nhw, k, stride, scale, shift, residual, relu, relu_after_add):
    """float64 on the CPU: x rows [N*H*W, Cin], w [k*k, Cout, Cin] -> rows [N*OH*OW, Cout] of nn.Conv2d(padding=k//2)."""
    N, H, W = nhw
    Cin, Cout = x.shape[1], w.shape[1]
    xi = x.double().view(N, H, W, Cin).permute(0, 3, 1, 2)
    y = F.conv2d(xi, w.double().view(k, k, Cout, Cin).permute(2, 3, 0, 1), stride=stride, padding=k // 2)
    onhw = (N, y.shape[2], y.shape[3])
    y = y.permute(0, 2, 3, 1).reshape(-1, Cout)
    if scale is not None:
        y = y * scale.double()
    if shift is not None:
        y = y + shift.double()
    if relu:
        y = y.clamp_min(0)
    if residual is not None:
        y = y + residual.double()[:, :Cout]
    if relu_after_add:
        y = y.clamp_min(0)
    return y, onhw


def _strided_case(k, nhw, Cout, cout_live, seed):
    N, H, W = nhw
    g = torch.Generator().manual_seed(seed)
    Cin, cin_live = 64, 48
    x = torch.randn(N * H * W, Cin, generator=g)
    x[:, cin_live:] = 0
    w = torch.randn(k * k, Cout, Cin, generator=g) / (k * Cin ** 0.5)
    w[:, cout_live:] = 0
    w[:, :, cin_live:] = 0
    scale, shift = 0.5 + torch.rand(Cout, generator=g), 0.3 * torch.randn(Cout, generator=g)
    scale[cout_live:], shift[cout_live:] = 1, 0
    orows = N * ((H + 1) // 2) * ((W + 1) // 2)
    res = torch.randn(orows, Cout + 32, generator=g)             # a residual with its own row pitch
    res[:, cout_live:Cout] = 0
    return x, w, scale, shift, res


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("nhw", [(2, 15, 20), (1, 5, 7), (3, 9, 9), (1, 1, 3)])
@pytest.mark.parametrize("Cout,cout_live", [(160, 140), (256, 232), (32, 24)])      # 64-, 128- and 32-column workgroup tiles
def test_strided_entry_on_odd_sizes_against_float64(gpu_ops, k, nhw, Cout, cout_live):
    """Stride 2 over odd (and mixed) map sizes, OH = (H + 1) / 2: every epilogue flag alone and combined, with and without
    scale / shift, the residual at its own pitch.  Bound: 1e-4 of the output's max-abs (the header's contract)."""
    ops = gpu_ops
    N, H, W = nhw
    x, w, scale, shift, res = _strided_case(k, nhw, Cout, cout_live, 100 * k + H + Cout)
    hi, lo = ops.split_operand(w.cuda())
    xg, resg = x.cuda(), res.cuda()
    for affine, relu, add, relu2 in [(1, 0, 0, 0), (0, 0, 0, 0), (1, 1, 0, 0), (1, 0, 1, 0), (0, 0, 1, 0), (1, 0, 0, 1), (1, 1, 1, 0),
                                     (1, 0, 1, 1), (0, 1, 1, 1), (1, 1, 1, 1)]:
        sc, sh = (scale, shift) if affine else (None, None)
        r = res if add else None
        got = ops.conv2d_nhwc_strided_bf16x3(xg, hi, lo, nhw, k, stride=2, scale=None if sc is None else sc.cuda(),
                                             shift=None if sh is None else sh.cuda(), residual=resg if add else None,
                                             relu=bool(relu), relu_after_add=bool(relu2))
        want, onhw = _ref_conv(x, w, nhw, k, 2, sc, sh, r, relu, relu2)
        assert onhw == (N, (H + 1) // 2, (W + 1) // 2) and got.shape == want.shape
        err, mag = max_err(got, want), want.abs().max().item()
        print(f"conv2d_strided k{k} {nhw} Cout {Cout} affine {affine} flags {relu}{add}{relu2}: err {err:.3e} scale {mag:.3f}")
        assert err < 1e-4 * mag
        if not add:
            assert got[:, cout_live:].abs().max().item() == 0.0


@pytest.mark.parametrize("nhw", [(2, 8, 12), (1, 64, 80)])
def test_strided_entry_is_bit_identical_to_the_existing_entry_on_even_sizes(gpu_ops, nhw):
    ops = gpu_ops
    for k in (1, 3):
        for stride in (1, 2):
            x, w, scale, shift, res = _strided_case(k, nhw, 160, 140, 5 + k)
            res = res[:nhw[0] * (nhw[1] // stride) * (nhw[2] // stride)].contiguous() if stride == 2 else \
                torch.randn(nhw[0] * nhw[1] * nhw[2], 192, generator=torch.Generator().manual_seed(9))
            hi, lo = ops.split_operand(w.cuda())
            kw = dict(stride=stride, scale=scale.cuda(), shift=shift.cuda(), residual=res.cuda(), relu=True, relu_after_add=True)
            a = ops.conv2d_nhwc_strided_bf16x3(x.cuda(), hi, lo, nhw, k, **kw)
            b = ops.conv2d_nhwc_ex_bf16x3(x.cuda(), hi, lo, nhw, k, **kw)
            assert a.shape == b.shape and torch.equal(a, b)


def test_strided_supported_twin(gpu_ops):
    ops = gpu_ops
    assert ops.conv2d_nhwc_strided_supported((1, 5, 8), 32, 32, 3, stride=2)          # odd H at stride 2: this entry takes it
    assert ops.conv2d_nhwc_strided_supported((1, 5, 7), 64, 256, 1, stride=2, ldr=256)
    assert not ops.conv2d_nhwc_strided_supported((1, 5, 8), 12, 32, 3, stride=2)      # Cin % 32 as for the existing entry
    assert not ops.conv2d_nhwc_strided_supported((1, 5, 8), 32, 32, 3, stride=2, ldr=30)
    assert not ops.lib._dll.sgc_conv2d_nhwc_strided_supported(1, 5, 8, 32, 32, 3, 2, 1, 32, 0, 0, 0)      # no transposed form


# ---- the whole backbone ----------------------------------------------------------------------------------------------------------
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
    return fill_resnet(build_backbone(dict(REF_BACKBONE, depth=depth))).eval()


def patched_run(depth=18, shape=(2, 3, 64, 96)):
    """(net, img, maps, entry names) of the eval forward on the GPU with the library layers patched out -- also the body of the
    child process of the switch test.  The caller's environment selects the variant (SGC_BACKBONE_HIP)."""
    from sgcdet_amd import ext
    net = _net(depth)
    img = torch.randn(*shape, generator=torch.Generator().manual_seed(depth + shape[2]))
    gnet = net.cuda()
    ops = ext.ops()
    ops.event_log = []
    try:
        with torch.no_grad(), _NoLibraryLayers():
            maps = gnet(img.cuda())
        names = [e[0] for e in ops.event_log]
    finally:
        ops.event_log = None
    return gnet, img, maps, names


_BACKBONE_CASES = [(50, (2, 3, 72, 104)), (18, (2, 3, 64, 96)), (50, (1, 3, 240, 320))]


@pytest.mark.parametrize("depth,shape", _BACKBONE_CASES)
def test_backbone_on_hip_matches_float64(monkeypatch, depth, shape):
    """Depth 50 on 72 x 104 (odd sizes at layers 3 and 4), depth 18 on 64 x 96 (all even), depth 50 on 240 x 320 (the reference
    geometry: 15 x 20 -> 8 x 10).  The HIP path ran (library layers patched to raise, entry points counted), every map is
    channels-last in memory and within 1e-4 of its max-abs of the float64 formulation on the CPU."""
    monkeypatch.setenv("SGC_BACKBONE_HIP", "1")
    gnet, img, maps, names = patched_run(depth, shape)
    n_blocks = sum(len(getattr(gnet, n)) for n in gnet.res_layers)
    n_convs = n_blocks * (3 if depth >= 50 else 2) + (4 if depth >= 50 else 3)
    conv_names = ("sgc_conv2d_nhwc_bf16x3", "sgc_conv2d_nhwc_ex_bf16x3", "sgc_conv2d_nhwc_strided_bf16x3")
    assert names.count("sgc_conv2d_stem7_bf16x3") == 1 and names.count("sgc_maxpool2d_nhwc") == 1
    assert sum(names.count(n) for n in conv_names) == n_convs and len(names) == n_convs + 2     # no layout pass, nothing else
    odd = shape[2] % 32 != 0 or shape[3] % 32 != 0
    n_strided = names.count("sgc_conv2d_nhwc_strided_bf16x3")
    assert n_strided == ({(72, 104): 4, (240, 320): 2}[shape[2:]] if odd else 0)       # stride-2 conv + shortcut per odd stage
    with torch.no_grad():
        monkeypatch.setenv("SGC_BACKBONE_HIP", "0")
        torch_maps = gnet(img.cuda())
        want = gnet.cpu().double()(img.double())
    worst_hip = worst_torch = 0.0
    for got, lib, w in zip(maps, torch_maps, want):
        assert got.shape == w.shape
        assert got.is_contiguous(memory_format=torch.channels_last) and (got.shape[2] * got.shape[3] == 1 or not got.is_contiguous())
        mag = w.abs().max().item()
        assert 1.0 < mag < 1e4
        e_hip, e_lib = max_err(got, w) / mag, max_err(lib, w) / mag
        print(f"resnet{depth} {shape} map {tuple(w.shape)} scale {mag:.2f}: HIP path {e_hip:.3e}, torch fp32 path {e_lib:.3e} (of max-abs)")
        worst_hip, worst_torch = max(worst_hip, e_hip), max(worst_torch, e_lib)
    print(f"resnet{depth} {shape}: worst HIP {worst_hip:.3e}, worst torch fp32 {worst_torch:.3e} "
          f"(recorded {MEASURED_ERRORS[(depth, shape)]})")
    assert worst_hip <= 1e-4


def test_switch_restores_the_library_convolutions_in_a_fresh_process():
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_gpu_resnet as t\n"
            "try:\n    t.patched_run()\nexcept AssertionError as e:\n    print('RAISED', e)\n" % (ROOT, os.path.join(ROOT, "tests")))
    env = dict(os.environ, SGC_BACKBONE_HIP="0")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "RAISED" in r.stdout and "library convolution" in r.stdout


def test_fallbacks_take_the_torch_formulation(monkeypatch):
    """An odd image side and a non-fp32 input run the library layers silently; the results have the torch formulation's layout."""
    from sgcdet_amd import ext
    monkeypatch.setenv("SGC_BACKBONE_HIP", "1")
    net = _net(18).cuda()
    ops = ext.ops()
    ops.event_log = []
    try:
        with torch.no_grad():
            a = net(torch.randn(1, 3, 63, 96).cuda())
            b = net.double()(torch.randn(1, 3, 64, 96).cuda().double())
        assert ops.event_log == []
    finally:
        ops.event_log = None
    assert a[0].shape == (1, 64, 16, 24) and a[0].is_contiguous() and b[0].dtype == torch.float64


# ---- images -> boxes ---------------------------------------------------------------------------------------------------------------
def test_simple_test_from_images_matches_the_by_hand_composition(monkeypatch):
    """The SGCDet_ScanNet model config with the backbone attached and seeded weights, 4 views of 240 x 320 images: the FPN reads
    the backbone's maps in place (the rows it consumed ARE the backbone's output memory), and ``simple_test(batch)`` returns the
    boxes of ``simple_test_from_features`` fed by hand with backbone -> image_features -> depth_distribution."""
    import sgcdet_amd.plugin  # noqa: F401
    from sgcdet_amd.mmcv_lite import _wrap, build_detector
    from sgcdet_amd.plugin import fpn as fpn_mod
    from sgcdet_amd.scene import make_img_meta
    with open(os.path.join(ROOT, "tests", "golden", "ref_configs.json")) as f:
        model = _wrap(json.load(f, object_hook=lambda d: tuple(d["__tuple__"]) if set(d) == {"__tuple__"} else d)["SGCDet_ScanNet"])
    model["depth_head"] = dict(model["depth_head"], init_weight="none")
    monkeypatch.setenv("SGC_BACKBONE_HIP", "1")
    monkeypatch.setenv("SGC_DEPTH_NET_HIP", "1")
    torch.manual_seed(21)
    det = build_detector(model).attach_backbone().eval()
    fill_resnet(det.backbone)
    gen = torch.Generator().manual_seed(22)
    with torch.no_grad():
        for _, p in list(det.voxel_head.named_parameters()) + list(det.bbox_head.named_parameters()):
            p.add_(torch.randn(p.shape, generator=gen) * 0.05)
    det = det.cuda()
    det.bbox_head.test_cfg = dict(nms_pre=1000, iou_thr=0.25, score_thr=0.01)
    n_views = 4
    meta = make_img_meta(n_views, "scannet", seed=6, img_hw=(240, 320))
    img = torch.randn(1, n_views, 3, 240, 320, generator=torch.Generator().manual_seed(23)).cuda()

    produced, consumed = [], []
    backbone_forward = det.backbone.forward

    def backbone_spy(x):
        maps = backbone_forward(x)
        produced.append([m.data_ptr() for m in maps])
        return maps
    image_rows = fpn_mod.image_rows

    def rows_spy(x):
        rows, nhw = image_rows(x)
        consumed.append(rows.data_ptr())
        return rows, nhw
    monkeypatch.setattr(det.backbone, "forward", backbone_spy)
    monkeypatch.setattr(fpn_mod, "image_rows", rows_spy)
    with torch.no_grad():
        res, = det.simple_test(dict(img=img, img_metas=[meta]))
        assert len(produced) == 1 and consumed == produced[0]              # no contiguous() copy between backbone and FPN
        maps = det.backbone(img[0])
        assert [tuple(m.shape) for m in maps] == [(4, 256, 60, 80), (4, 512, 30, 40), (4, 1024, 15, 20), (4, 2048, 8, 10)]
        assert all(m.is_contiguous(memory_format=torch.channels_last) for m in maps)
        x = det.image_features(maps)
        assert all(f[0].is_contiguous(memory_format=torch.channels_last) for f in x[:3])
        dpt = det.depth_distribution(x, img, [meta])
        want, = det.simple_test_from_features(x, [meta], dpt, as_results=True)
    assert set(res) == {"boxes_3d", "scores_3d", "labels_3d"} and not res["scores_3d"].is_cuda
    print(f"images -> boxes: {res['boxes_3d'].shape[0]} boxes")
    assert res["boxes_3d"].shape[0] > 0 and res["boxes_3d"].shape[1] == 6
    assert torch.equal(res["boxes_3d"], want["boxes_3d"]) and torch.equal(res["scores_3d"], want["scores_3d"])
    assert torch.equal(res["labels_3d"], want["labels_3d"])
