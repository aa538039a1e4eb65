"""DepthNet_Fusion's 2-D CNNs on the HIP kernels in inference (include/sgcdet_amd_image.h, plugin/depth_net.py):
kernel parity against float64 torch convolutions, the module against the reference class's golden output with the library
convolutions patched out, and the full-resolution module against its torch formulation."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from golden_util import load, img_meta, max_err, fill_by_name

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Bounds of the module tests.  Measured on MI355X (profiles/r10_depth_net_parity.json, max |difference| of the probabilities):
#   golden size        HIP path vs the reference's golden 2.38e-6, torch path vs the golden 3.9e-7 (the existing test: 5e-5)
#   config-2 geometry  HIP path vs the module's torch formulation on the same device 4.59e-6
# The tests assert at 4x the measured HIP figure (MFMA accumulation order may differ between boxes), never above the project's
# feature-parity line of 1e-3 (README "features within 1e-3").
HIP_GOLDEN_ERR = 2.384e-6
HIP_FULL_ERR = 4.590e-6
GOLDEN_BOUND = min(4 * HIP_GOLDEN_ERR, 1e-3)
FULL_BOUND = min(4 * HIP_FULL_ERR, 1e-3)


def _ref_conv(x, w, nhw, k, stride, transposed, scale, shift, residual, relu, relu_after_add, softmax_cols):
    """float64 on the CPU: x rows [N*H*W, Cin], w [k*k, Cout, Cin] -> rows [N*OH*OW, Cout]."""
    N, H, W = nhw
    Cin, Cout = x.shape[1], w.shape[1]
    xi = x.double().cpu().view(N, H, W, Cin).permute(0, 3, 1, 2)
    wk = w.double().cpu().view(k, k, Cout, Cin)
    if transposed:
        y = F.conv_transpose2d(xi, wk.permute(3, 2, 0, 1), stride=2, padding=1, output_padding=1)
    else:
        y = F.conv2d(xi, wk.permute(2, 3, 0, 1), stride=stride, padding=k // 2)
    y = y.permute(0, 2, 3, 1).reshape(-1, Cout)
    if scale is not None:
        y = y * scale.double().cpu()
    if shift is not None:
        y = y + shift.double().cpu()
    if relu:
        y = y.clamp_min(0)
    if residual is not None:
        y = y + residual.double().cpu()[:, :Cout]
    if relu_after_add:
        y = y.clamp_min(0)
    if softmax_cols:
        y = torch.cat([F.softmax(y[:, :softmax_cols], dim=1), y[:, softmax_cols:]], 1)
    return y


FORMS = [(1, 1, False), (1, 2, False), (3, 1, False), (3, 2, False), (3, 2, True)]
SIZES = [(1, 64, 80), (2, 32, 40), (3, 16, 20), (2, 6, 10)]


@pytest.mark.parametrize("k,stride,transposed", FORMS)
@pytest.mark.parametrize("nhw", SIZES)
@pytest.mark.parametrize("Cout,cout_live", [(160, 140), (256, 232), (32, 24)])      # 64-, 128- and 32-column workgroup tiles
def test_conv2d_ex_forms_against_float64(gpu_ops, k, stride, transposed, nhw, Cout, cout_live):
    """Every geometry at every size and tile width, with every epilogue flag alone and combined, Cout that is not a multiple
    of the tile (zero-padded weight rows and input columns: their outputs are exactly 0).  Bound: 1e-4 of the output scale."""
    ops = gpu_ops
    N, H, W = nhw
    g = torch.Generator().manual_seed(100 * k + 10 * stride + int(transposed) + H + Cout)
    Cin, cin_live = 64, 48
    x = torch.randn(N * H * W, Cin, generator=g)
    x[:, cin_live:] = 0
    w = torch.randn(k * k, Cout, Cin, generator=g) / (k * Cin ** 0.5)
    w[:, cout_live:] = 0
    w[:, :, cin_live:] = 0
    scale, shift = 0.5 + torch.rand(Cout, generator=g), 0.3 * torch.randn(Cout, generator=g)
    scale[cout_live:], shift[cout_live:] = 1, 0
    OH, OW = (2 * H, 2 * W) if transposed else (H // stride, W // stride)
    res = torch.randn(N * OH * OW, Cout, generator=g)
    res[:, cout_live:] = 0
    hi, lo = ops.split_operand(w.cuda())
    for relu, add, relu2 in [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 1, 1)]:
        r = res if add else None
        got = ops.conv2d_nhwc_ex_bf16x3(x.cuda(), hi, lo, nhw, k, stride=stride, transposed=transposed, scale=scale.cuda(),
                                        shift=shift.cuda(), residual=None if r is None else r.cuda(), relu=bool(relu),
                                        relu_after_add=bool(relu2))
        want = _ref_conv(x, w, nhw, k, stride, transposed, scale, shift, r, relu, relu2, 0)
        assert got.shape == want.shape
        err, sc = max_err(got, want), want.abs().max().item()
        print(f"conv2d_ex k{k} s{stride} t{int(transposed)} {nhw} Cout {Cout} flags {relu}{add}{relu2}: err {err:.3e} scale {sc:.3f}")
        assert err < 1e-4 * sc
        assert got[:, cout_live:].abs().max().item() == 0.0


@pytest.mark.parametrize("k,stride,transposed", FORMS)
def test_conv2d_ex_writes_a_column_range_of_a_wider_buffer(gpu_ops, k, stride, transposed):
    """ldy / column offset (the channel concatenation) with a residual of its own pitch: neighbouring columns are untouched."""
    ops = gpu_ops
    nhw = (2, 12, 20)
    N, H, W = nhw
    g = torch.Generator().manual_seed(7 + k + stride)
    Cin, Cout, ldy, col0, ldr = 32, 32, 160, 128, 64
    x = torch.randn(N * H * W, Cin, generator=g)
    w = torch.randn(k * k, Cout, Cin, generator=g) / (k * Cin ** 0.5)
    OH, OW = (2 * H, 2 * W) if transposed else (H // stride, W // stride)
    res = torch.randn(N * OH * OW, ldr, generator=g)
    hi, lo = ops.split_operand(w.cuda())
    out = torch.full((N * OH * OW, ldy), 7.25).cuda()
    ops.conv2d_nhwc_ex_bf16x3(x.cuda(), hi, lo, nhw, k, stride=stride, transposed=transposed, residual=res.cuda(), relu=True,
                              out=out, col0=col0)
    want = _ref_conv(x, w, nhw, k, stride, transposed, None, None, res, 1, 0, 0)
    assert max_err(out[:, col0:col0 + Cout], want) < 1e-4 * want.abs().max().item()
    assert (out[:, :col0] == 7.25).all() and (out[:, col0 + Cout:] == 7.25).all()


@pytest.mark.parametrize("nhw", [(1, 64, 80), (2, 6, 10)])
def test_conv2d_ex_softmax_columns(gpu_ops, nhw):
    """depth_reg's form: 3x3 stride 1, Cout = 12 written at row pitch 12, softmax over the 12 columns; and softmax over the
    first 12 of 32 columns with the zero-padded tail left exactly 0."""
    ops = gpu_ops
    N, H, W = nhw
    g = torch.Generator().manual_seed(11)
    Cin = 160
    x = torch.randn(N * H * W, Cin, generator=g)
    shift12 = torch.randn(12, generator=g)
    for Cout in (12, 32):
        w = torch.randn(9, Cout, Cin, generator=g) * (3.0 / (3 * Cin ** 0.5))
        w[:, 12:] = 0
        shift = F.pad(shift12, (0, Cout - 12))
        hi, lo = ops.split_operand(w.cuda())
        got = ops.conv2d_nhwc_ex_bf16x3(x.cuda(), hi, lo, nhw, 3, shift=shift.cuda(), softmax_cols=12)
        want = _ref_conv(x, w, nhw, 3, 1, False, None, shift, None, 0, 0, 12)
        assert got.shape == (N * H * W, Cout)
        assert max_err(got, want) < 1e-4 * want.abs().max().item()
        assert max_err(got[:, :12].sum(1), torch.ones(N * H * W)) < 1e-5
        assert Cout == 12 or got[:, 12:].abs().max().item() == 0.0


@pytest.mark.parametrize("nhw", [(1, 256, 320), (2, 128, 160), (3, 64, 80), (2, 12, 20), (5, 48, 64)])
def test_stem7_against_float64(gpu_ops, nhw):
    ops = gpu_ops
    N, H, W = nhw
    g = torch.Generator().manual_seed(H)
    img = torch.randn(N, 3, H, W, generator=g)
    w = torch.randn(64, 3, 7, 7, generator=g) / 147 ** 0.5
    scale, shift = 0.5 + torch.rand(64, generator=g), 0.3 * torch.randn(64, generator=g)
    hi, lo = ops.split_operand(F.pad(w.reshape(64, 147), (0, 13)).contiguous().cuda())
    for relu in (True, False):
        got = ops.conv2d_stem7_bf16x3(img.cuda(), hi, lo, scale=scale.cuda(), shift=shift.cuda(), relu=relu)
        want = F.conv2d(img.double(), w.double(), stride=2, padding=3) * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
        want = (want.clamp_min(0) if relu else want).permute(0, 2, 3, 1).reshape(-1, 64)
        assert got.shape == want.shape
        err = max_err(got, want)
        print(f"stem7 {nhw} relu {relu}: err {err:.3e} scale {want.abs().max().item():.3f}")
        assert err < 1e-4 * want.abs().max().item()


def _round_to_mode(t, mode):
    """An fp32 operand as the one-product modes multiply it: bfloat16 (mode 1) or saturated IEEE half (mode 2)."""
    return (t.bfloat16() if mode == 1 else t.clamp(-65504.0, 65504.0).half()).float()


@pytest.mark.parametrize("mode", [1, 2])
def test_one_product_modes_against_float64_of_the_rounded_operands(gpu_ops, mode):
    """sgc_set_conv_products 1 / 2 on conv2d_ex_kernel (32- and 64-column tiles, every form, residual and both ReLUs) and on the
    stem.  The yardstick is the float64 formulation of operands ROUNDED to the mode, so only the fp32 accumulation separates the
    two, as in mode 3: the same 1e-4 of the output scale."""
    ops = gpu_ops
    try:
        ops.lib.call("sgc_set_conv_products", mode)
        split = ops.split_operand          # the planes of the mode just selected, as the prepared layers make them
        nhw, Cin = (2, 6, 10), 32
        N, H, W = nhw
        for Cout, cout_live in [(32, 24), (160, 140)]:
            for k, stride, transposed in FORMS:
                g = torch.Generator().manual_seed(1000 * mode + 100 * k + 10 * stride + int(transposed) + Cout)
                x = torch.randn(N * H * W, Cin, generator=g)
                w = torch.randn(k * k, Cout, Cin, generator=g) / (k * Cin ** 0.5)
                w[:, cout_live:] = 0
                scale, shift = 0.5 + torch.rand(Cout, generator=g), 0.3 * torch.randn(Cout, generator=g)
                OH, OW = (2 * H, 2 * W) if transposed else (H // stride, W // stride)
                res = torch.randn(N * OH * OW, Cout, generator=g)
                hi, lo = split(w.cuda())
                got = ops.conv2d_nhwc_ex_bf16x3(x.cuda(), hi, lo, nhw, k, stride=stride, transposed=transposed, scale=scale.cuda(),
                                                shift=shift.cuda(), residual=res.cuda(), relu=True, relu_after_add=True)
                want = _ref_conv(_round_to_mode(x, mode), _round_to_mode(w, mode), nhw, k, stride, transposed, scale, shift, res, 1, 1, 0)
                assert torch.isfinite(want).all() and got.shape == want.shape
                err, sc = max_err(got, want), want.abs().max().item()
                print(f"mode {mode} conv2d_ex k{k} s{stride} t{int(transposed)} Cout {Cout}: err {err:.3e} scale {sc:.3f}")
                assert err < 1e-4 * sc
        N, H, W = 2, 12, 20
        g = torch.Generator().manual_seed(mode)
        img = torch.randn(N, 3, H, W, generator=g)
        w = torch.randn(64, 3, 7, 7, generator=g) / 147 ** 0.5
        scale, shift = 0.5 + torch.rand(64, generator=g), 0.3 * torch.randn(64, generator=g)
        hi, lo = split(F.pad(w.reshape(64, 147), (0, 13)).contiguous().cuda())
        got = ops.conv2d_stem7_bf16x3(img.cuda(), hi, lo, scale=scale.cuda(), shift=shift.cuda(), relu=True)
        want = F.conv2d(_round_to_mode(img, mode).double(), _round_to_mode(w, mode).double(), stride=2, padding=3)
        want = (want * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)).clamp_min(0).permute(0, 2, 3, 1).reshape(-1, 64)
        assert torch.isfinite(want).all() and got.shape == want.shape
        err, sc = max_err(got, want), want.abs().max().item()
        print(f"mode {mode} stem7: err {err:.3e} scale {sc:.3f}")
        assert err < 1e-4 * sc
    finally:
        ops.lib.call("sgc_set_conv_products", 3)


def test_refused_shapes_and_padded_transpose(gpu_ops):
    ops = gpu_ops
    assert not ops.conv2d_nhwc_ex_supported((1, 5, 8), 32, 32, 3, stride=2)           # odd H at a stride-2 stage
    assert not ops.conv2d_nhwc_ex_supported((1, 8, 8), 12, 32, 3)                       # Cin % 32
    assert ops.conv2d_nhwc_ex_supported((1, 8, 8), 32, 12, 3, ldy=12, softmax_cols=12)
    assert ops.conv2d_nhwc_ex_supported((1, 8, 8), 32, 32, 3, ldr=64) and not ops.conv2d_nhwc_ex_supported((1, 8, 8), 32, 32, 3, ldr=30)
    x, w = torch.randn(64, 32).cuda(), torch.randn(9, 32, 32).cuda()
    hi, lo = ops.split_operand(w)
    shift = torch.zeros(33).cuda()[1:]                      # 4-byte aligned only: refused, not launched
    with pytest.raises(Exception, match="aligned"):
        ops.conv2d_nhwc_ex_bf16x3(x, hi, lo, (1, 8, 8), 3, shift=shift)
    src = torch.randn(2, 12, 6, 10).cuda()
    rows = ops.nchw_to_nhwc_padc(src, 32)
    assert torch.equal(rows[:, :12], src.permute(0, 2, 3, 1).reshape(-1, 12)) and rows[:, 12:].abs().max().item() == 0.0


# ---- the module ----------------------------------------------------------------------------------------------------------
def _golden_net():
    import sgcdet_amd.plugin as P
    d, _ = load("depth_net")
    z = np.load(os.path.join(ROOT, "tests", "golden", "depth_net.npz"))
    stride, dbound = int(z["stride"]), [float(v) for v in z["dbound"]]
    net = P.DepthNet_Fusion(neighbor_img_num=2, downsample_factor=stride, dbound=dbound, mono_channels=d["xs"].shape[2],
                            loss_weight=0.5, max_tol=0, init_weight="none").eval()
    fill_by_name(net, base_seed=7, scale=0.15)
    return net.cuda(), d, stride


class _NoLibraryConvolutions:
    """nn.Conv2d / nn.ConvTranspose2d / nn.BatchNorm2d forward raise while this is active."""

    def __enter__(self):
        self.saved = [(c, c.forward) for c in (nn.Conv2d, nn.ConvTranspose2d, nn.BatchNorm2d)]

        def boom(self_, *a, **k):
            raise AssertionError(f"{type(self_).__name__}.forward was called: a library convolution / norm ran")
        for c, _ in self.saved:
            c.forward = boom
        return self

    def __exit__(self, *exc):
        for c, f in self.saved:
            c.forward = f


def golden_run():
    """(pred, event names) of the patched eval run on the golden inputs -- also the body of the child process below.  The
    caller's environment selects the variant (SGC_DEPTH_NET_HIP)."""
    from sgcdet_amd import ext
    net, d, stride = _golden_net()
    ops = ext.ops()
    ops.event_log = []
    try:
        with torch.no_grad(), _NoLibraryConvolutions():
            pred = net(d["xs"].cuda(), d["imgs"].cuda(), [img_meta(d)], stride)
        names = [e[0] for e in ops.event_log]
    finally:
        ops.event_log = None
    return net, d, pred, names


def test_depth_net_module_runs_without_library_convolutions_and_matches_the_golden(monkeypatch):
    """The HIP path against the reference class's own output, with torch's convolution / norm modules patched to raise.
    Measured 2.38e-6 (torch path: 3.9e-7); asserted at 4x that."""
    monkeypatch.setenv("SGC_DEPTH_NET_HIP", "1")
    net, d, pred, names = golden_run()
    assert names.count("sgc_plane_sweep_corr") == 1
    assert names.count("sgc_conv2d_stem7_bf16x3") == 1 and names.count("sgc_conv2d_nhwc_ex_bf16x3") >= 3 * 4 + 3
    # the matching features reach the plane sweep in place; the only layout passes are the cost volume entering the 32-wide
    # rows and the golden's NCHW `xs` (a channels-last `xs` needs none: the full-resolution test)
    assert names.count("sgc_nchw_to_nhwc_crop") == 1 and names.count("sgc_nchw_to_nhwc_padc") == 1
    assert not any("nhwc_to_nchw" in n for n in names)
    assert pred.shape == d["pred"].shape
    assert pred[0].is_contiguous(memory_format=torch.channels_last) and not pred[0].is_contiguous()
    err = max_err(pred, d["pred"])
    print(f"depth_net HIP path vs golden: {err:.3e} (bound {GOLDEN_BOUND:.1e})")
    assert err <= GOLDEN_BOUND
    assert max_err(pred.sum(2), torch.ones_like(pred.sum(2))) < 1e-5
    loss = net.loss(d["depth_maps"].cuda(), pred)["loss_dpt"]
    assert abs(float(loss) - float(d["loss"])) < 1e-4


def test_switch_restores_the_library_convolutions_in_a_fresh_process():
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_gpu_depth_net_hip as t\n"
            "try:\n    t.golden_run()\nexcept AssertionError as e:\n    print('RAISED', e)\n" % (ROOT, os.path.join(ROOT, "tests")))
    env = dict(os.environ, SGC_DEPTH_NET_HIP="0")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "RAISED" in r.stdout and "library convolution" in r.stdout


def _full_res(n_views=6, mono=256, seed=3):
    import sgcdet_amd.plugin as P
    from sgcdet_amd.scene import make_scene
    net = P.DepthNet_Fusion(neighbor_img_num=2, downsample_factor=4, dbound=[0.2, 5.0, 0.4], mono_channels=mono,
                            init_weight="none").eval()
    fill_by_name(net, base_seed=seed, scale=0.15)
    feats, _, meta = make_scene(n_views, mono, kind="scannet", seed=seed, img_hw=(256, 320))
    g = torch.Generator().manual_seed(seed)
    imgs = torch.randn(1, n_views, 3, 256, 320, generator=g)
    return net.cuda(), feats, imgs, meta


def test_depth_net_full_resolution_matches_the_torch_formulation(monkeypatch):
    """Config-2 geometry (256x320 images, 64x80 maps, 256 mono channels, D = 12), 6 views: interior and boundary neighbour
    selections, against the torch formulation on the same device.  Measured 4.59e-6; asserted at 4x that."""
    net, feats, imgs, meta = _full_res()
    xs = feats[0].cuda()
    assert xs.shape[-2:] == (64, 80) and net.depth_channels == 12
    with torch.no_grad():
        monkeypatch.setenv("SGC_DEPTH_NET_HIP", "1")
        got = net(xs, imgs.cuda(), [meta], 4)
        monkeypatch.setenv("SGC_DEPTH_NET_HIP", "0")
        want = net(xs, imgs.cuda(), [meta], 4)
    assert got[0].is_contiguous(memory_format=torch.channels_last) and want.is_contiguous()
    err = max_err(got, want)
    print(f"depth_net full resolution HIP vs torch: {err:.3e} (bound {FULL_BOUND:.1e})")
    assert err <= FULL_BOUND
    assert max_err(got.sum(2), torch.ones_like(got.sum(2))) < 1e-5


def test_build_volume_from_fpn_reads_the_channels_last_distribution_in_place(monkeypatch):
    """The hand-over at config-2 geometry: with channels-last FPN maps and the HIP depth head, `build_volume_from_fpn` launches no
    `sgc_nchw_to_nhwc_crop` at all (the depth maps' NCHW -> NHWC pass is gone), and gives the volume / valid of the same
    distribution handed over as a contiguous NCHW copy (which pays that pass): selection bit-exact, features within 1e-5."""
    import sgcdet_amd.plugin  # noqa: F401
    from sgcdet_amd import ext
    from sgcdet_amd.mmcv_lite import build_detector
    from sgcdet_amd.scene import make_scene, model_config, workload
    w = workload("cfg2_scannet")
    cfg = model_config(w)
    cfg["depth_head"] = dict(type="DepthNet_Fusion", neighbor_img_num=2, downsample_factor=4, dbound=[0.2, 5, 0.4],
                             mono_channels=w["embed_dims"], loss_weight=0.5, max_tol=0, init_weight="none")
    torch.manual_seed(17)
    det = build_detector(cfg).eval()
    fill_by_name(det.depth_head, base_seed=3, scale=0.15)
    gen = torch.Generator().manual_seed(13)
    with torch.no_grad():
        for _, p in det.voxel_head.named_parameters():
            p.add_(torch.randn(p.shape, generator=gen) * 0.02)
    det = det.cuda()
    n_views = 6
    feats, _, meta = make_scene(n_views, w["embed_dims"], kind="scannet", seed=25, img_hw=(256, 320))
    feats = [f[0].cuda().contiguous(memory_format=torch.channels_last).unsqueeze(0) for f in feats]
    imgs = torch.randn(1, n_views, 3, 256, 320, generator=torch.Generator().manual_seed(5)).cuda()
    monkeypatch.setenv("SGC_DEPTH_NET_HIP", "1")
    ops = ext.ops()
    try:
        with torch.no_grad():
            ops.event_log = []
            volume, valid, dpt, occ = det.build_volume_from_fpn(feats, imgs, [meta])
            names_cl = [e[0] for e in ops.event_log]
            assert dpt[0].is_contiguous(memory_format=torch.channels_last) and not dpt[0].is_contiguous()
            ops.event_log = []
            volume_n, valid_n, occ_n = det.build_volume_from_features(feats, [meta], dpt.contiguous())
            names_nchw = [e[0] for e in ops.event_log]
    finally:
        ops.event_log = None
    print(f"sgc_nchw_to_nhwc_crop launches: channels-last distribution {names_cl.count('sgc_nchw_to_nhwc_crop')}, "
          f"NCHW copy {names_nchw.count('sgc_nchw_to_nhwc_crop')}")
    assert names_cl.count("sgc_nchw_to_nhwc_crop") == 0
    assert names_nchw.count("sgc_nchw_to_nhwc_crop") >= 1
    assert torch.equal(valid, valid_n)
    assert max_err(volume, volume_n) <= 1e-5 * max(1.0, volume_n.abs().max().item())
