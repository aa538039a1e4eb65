"""The plane-sweep cost volume under autograd on the HIP kernels (``sgc_plane_sweep_corr`` forward,
``sgc_plane_sweep_corr_backward``, include/sgcdet_amd_train.h): the feature gradient against the reference's own
gradients and float64 autograd of the reference formulation, DepthNet_Fusion trained through it against the
``SGC_PLANE_SWEEP_FUSED_GRAD=0`` formulation, its memory, and the detector's ``forward_train_from_fpn``."""
import copy
import os

import numpy as np
import pytest
import torch

from plane_sweep_grad_contract import golden_cases, reference_grad_f64, to_rows

pytestmark = pytest.mark.gpu


def _cuda(*ts):
    return [t.cuda() for t in ts]


def _backward(ops, f_mvs, nbr, rel, depth, grad_corr):
    N, C, H, W = f_mvs.shape
    rows, nbr32, rt, dep, g = _cuda(to_rows(f_mvs), nbr.to(torch.int32).contiguous(),
                                    rel.reshape(N, nbr.shape[1], 12).contiguous(), depth.contiguous(), grad_corr.contiguous())
    return ops.plane_sweep_corr_backward(rows, nbr32, rt, dep, g, H, W)


def test_plane_sweep_backward_matches_reference_golden_and_float64(gpu_ops):
    for k, (f_mvs, nbr, rel, depth, grad_corr, want) in enumerate(golden_cases()):
        got = _backward(gpu_ops, f_mvs, nbr, rel, depth, grad_corr).cpu()
        scale = float(want.abs().max())
        assert float((got - to_rows(want)).abs().max()) <= 1e-5 * scale, k
        ref64 = to_rows(reference_grad_f64(f_mvs, nbr, rel, depth, grad_corr))
        assert float((got.double() - ref64).abs().max()) <= 1e-5 * scale, k


def _random_case(N, C, H, W, K, D, seed, stride=None):
    """``stride``: intrinsics of a feature map at image / stride as DepthNet_Fusion scales them (:209-213); default: the
    original image's height mapped onto H rows."""
    from sgcdet_amd.plugin.plane_sweep import closest_frame_ids, relative_projections
    from sgcdet_amd.scene import make_img_meta
    meta = make_img_meta(N, "scannet", seed)
    w2c = torch.tensor(np.array(meta["lidar2img"]["extrinsic"]), dtype=torch.float32)
    intr = torch.tensor(np.array(meta["lidar2img"]["intrinsic"]), dtype=torch.float32).clone()
    intr[:2] /= meta["ori_shape"][0] / (H if stride is None else meta["img_shape"][0] / stride)
    nbr = closest_frame_ids(N, K)
    rel = relative_projections(w2c, intr, nbr)
    g = torch.Generator().manual_seed(seed)
    f_mvs = torch.randn(N, C, H, W, generator=g)
    depth = torch.linspace(0.2, 5.0, D)
    return f_mvs, nbr, rel, depth, torch.randn(N, D, H, W, generator=g)


@pytest.mark.parametrize("C", [32, 64, 96, 128, 256])
@pytest.mark.parametrize("K,D", [(2, 12), (2, 32), (4, 12), (4, 32)])
def test_plane_sweep_backward_sweep_against_float64_autograd(gpu_ops, C, K, D):
    f_mvs, nbr, rel, depth, grad_corr = _random_case(7, C, 9, 13, K, D, seed=C + 7 * K + D)   # 117 pixels; K = 4 needs 7 views
    got = _backward(gpu_ops, f_mvs, nbr, rel, depth, grad_corr).cpu().double()
    ref64 = to_rows(reference_grad_f64(f_mvs, nbr, rel, depth, grad_corr))
    assert float((got - ref64).abs().max()) <= 1e-5 * float(ref64.abs().max())


def _list_lengths(nbr, rel, depth, H, W):
    """Entries per destination row (on-image corners landing there), from the forward's position arithmetic in torch."""
    N = nbr.shape[0]
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    xyz = torch.stack([x.reshape(-1), y.reshape(-1), torch.ones(H * W)])
    cnt = torch.zeros(N * H * W, dtype=torch.int64)
    for k in range(nbr.shape[1]):
        r = rel[:, k]
        p = (r[:, :, :3] @ xyz).unsqueeze(2) * depth.view(1, 1, -1, 1) + r[:, :, 3].view(N, 3, 1, 1)
        ix = ((p[:, 0] / p[:, 2] / ((W - 1) / 2) - 1 + 1) * W - 1) / 2
        iy = ((p[:, 1] / p[:, 2] / ((H - 1) / 2) - 1 + 1) * H - 1) / 2
        inside = (ix > -1) & (iy > -1) & (ix < W) & (iy < H)
        x0, y0 = torch.floor(ix).long(), torch.floor(iy).long()
        m = nbr[:, k].view(N, 1, 1)
        for dx in (0, 1):
            for dy in (0, 1):
                xx, yy = x0 + dx, y0 + dy
                ok = inside & (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
                cnt += torch.bincount((m * H * W + yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1))[ok], minlength=N * H * W)
    return cnt


def test_plane_sweep_backward_is_bitwise_reproducible_with_short_lists(gpu_ops):
    """Every list of at most 512 entries is summed in an order fixed by its contents (sorted in LDS): two runs agree
    bit for bit although the list slots are taken with atomics."""
    f_mvs, nbr, rel, depth, grad_corr = _random_case(16, 128, 30, 40, 2, 12, seed=11, stride=8)
    assert int(_list_lengths(nbr, rel, depth, 30, 40).max()) <= 512          # no list takes the split path
    a = _backward(gpu_ops, f_mvs, nbr, rel, depth, grad_corr)
    b = _backward(gpu_ops, f_mvs, nbr, rel, depth, grad_corr)
    assert torch.equal(a, b)


def test_plane_sweep_backward_long_lists_against_float64_autograd(gpu_ops):
    """A degenerate warp (no rotation part: every pixel of every plane lands on one point of the neighbour view) gives four
    destination rows per view thousands of entries each: the split-list path (512-entry chunks added by row atomics)."""
    f_mvs, nbr, rel, depth, grad_corr = _random_case(7, 64, 9, 13, 2, 32, seed=5)
    rel = torch.zeros_like(rel)
    rel[..., 0, 3], rel[..., 1, 3], rel[..., 2, 3] = 3.3, 2.6, 1.0           # (u, v) = (3.3, 2.6) for every sample
    got = _backward(gpu_ops, f_mvs, nbr, rel, depth, grad_corr).cpu().double()
    ref64 = to_rows(reference_grad_f64(f_mvs, nbr, rel, depth, grad_corr))
    assert float((got - ref64).abs().max()) <= 1e-5 * float(ref64.abs().max())


def test_plane_sweep_backward_limits_raise(gpu_ops):
    for C, D in ((257, 12), (32, 33)):
        f_mvs, nbr, rel, depth, grad_corr = _random_case(4, C, 5, 7, 2, D, seed=1)
        with pytest.raises(RuntimeError):
            _backward(gpu_ops, f_mvs, nbr, rel, depth, grad_corr)


def _depth_net_grads(net, xs, imgs, meta, stride, fused):
    from sgcdet_amd import ext
    ops = ext.ops()
    old = os.environ.get("SGC_PLANE_SWEEP_FUSED_GRAD")
    os.environ["SGC_PLANE_SWEEP_FUSED_GRAD"] = "1" if fused else "0"
    ops.event_log, ops.event_names = [], {"sgc_plane_sweep_corr", "sgc_plane_sweep_corr_backward"}
    try:
        net.zero_grad(set_to_none=True)
        pred = net(xs, imgs, [meta], stride)
        w = torch.linspace(-1, 1, pred.numel(), device=pred.device).view_as(pred)
        (pred * w).sum().backward()
        torch.cuda.synchronize()
        names = [e[0] for e in ops.event_log]
    finally:
        ops.event_log = ops.event_names = None
        if old is None:
            os.environ.pop("SGC_PLANE_SWEEP_FUSED_GRAD", None)
        else:
            os.environ["SGC_PLANE_SWEEP_FUSED_GRAD"] = old
    return pred.detach(), {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None}, names


def test_depth_net_trains_through_the_fused_plane_sweep_and_matches_the_reference_formulation(gpu_ops):
    """DepthNet_Fusion in train() with a loss on its output: the cost volume and its gradient come from the HIP entry
    points; every parameter gradient is finite and equals the SGC_PLANE_SWEEP_FUSED_GRAD=0 (homo_warping + grid_sample)
    run: direction (cosine > 0.9999) and 5e-2 of the gradient's scale (BatchNorm in train mode amplifies the rounding
    of both paths, as in the neck / head autograd test)."""
    import sgcdet_amd.plugin as P
    from golden_util import fill_by_name, img_meta, load
    d, _ = load("depth_net")
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "depth_net.npz"))
    stride, dbound = int(z["stride"]), [float(v) for v in z["dbound"]]
    net = P.DepthNet_Fusion(neighbor_img_num=2, downsample_factor=stride, dbound=dbound, mono_channels=d["xs"].shape[2],
                            loss_weight=0.5, max_tol=0, init_weight="none")
    fill_by_name(net, base_seed=7, scale=0.15)
    net = net.cuda().train()
    net_ref = copy.deepcopy(net)
    meta = img_meta(d)
    xs, imgs = d["xs"].cuda(), d["imgs"].cuda()
    pred, grads, names = _depth_net_grads(net, xs, imgs, meta, stride, fused=True)
    assert names.count("sgc_plane_sweep_corr") == 1 and names.count("sgc_plane_sweep_corr_backward") == 1
    pred_r, grads_r, names_r = _depth_net_grads(net_ref, xs, imgs, meta, stride, fused=False)
    assert not names_r
    assert float((pred - pred_r).abs().max()) < 1e-5
    assert set(grads) == set(grads_r) and any(n.startswith("fnet_mvs.") for n in grads)
    # a gradient that is zero in exact arithmetic (the bias of a convolution followed by train-mode BatchNorm: the batch
    # mean removes it) is rounding noise in both runs: held to the bound only, relative to the largest gradient
    top = max(float(r.abs().max()) for r in grads_r.values())
    bad = []
    for n, g in grads.items():
        r = grads_r[n]
        if not torch.isfinite(g).all():
            bad.append((n, "not finite"))
            continue
        scale = float(r.abs().max())
        err = float((g - r).abs().max())
        if scale < 1e-3 * top:
            if err > 1e-5 * top:
                bad.append((n, "cancelled", err, top))
            continue
        cos = float(torch.nn.functional.cosine_similarity(g.flatten().double(), r.flatten().double(), dim=0))
        if cos <= 0.9999 or err > 5e-2 * scale:
            bad.append((n, cos, err, scale))
    assert not bad, bad


def test_fused_plane_sweep_backward_memory_stays_below_one_warped_tensor(gpu_ops):
    """16 views x 128 ch x 60x80 x 12 planes x 2 neighbours: the peak memory that the fused forward + backward adds,
    workspace included, stays below the size of ONE warped [N,C,D,H,W] tensor (472 MB); the reference formulation keeps
    two of them per neighbour step."""
    from sgcdet_amd.plugin.plane_sweep import plane_sweep_correlation
    from sgcdet_amd.scene import make_img_meta
    N, C, H, W, D = 16, 128, 60, 80, 12
    meta = make_img_meta(N, "scannet", 3)
    depth = np.arange(0.2, 5.0, 0.4, dtype=np.float32) + 0.2
    f = torch.randn(N, C, H, W, device="cuda").requires_grad_(True)
    g = torch.randn(N, D, H, W, device="cuda")
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    corr = plane_sweep_correlation(f, meta, 4, depth, 2)
    corr.backward(g)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    warped = N * C * D * H * W * 4
    assert f.grad is not None and torch.isfinite(f.grad).all()
    assert peak < warped, (peak, warped)


def _plumbing_detector(depth_loss=False, use_gt_dpt=False):
    import sgcdet_amd.plugin  # noqa: F401
    from sgcdet_amd.mmcv_lite import build_detector
    from sgcdet_amd.scene import model_config, workload
    w = workload("cfg1_plumbing")
    cfg = model_config(w)
    cfg["depth_head"] = dict(type="DepthNet_Fusion", neighbor_img_num=2, downsample_factor=4, dbound=[0.2, 5, 0.4],
                             mono_channels=w["embed_dims"], loss_weight=0.5, max_tol=0, init_weight="none")
    cfg["depth_loss"] = depth_loss
    cfg["use_gt_dpt"] = use_gt_dpt
    torch.manual_seed(31)
    det = build_detector(cfg).cuda().train()
    for m in det.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    return det, w


def test_forward_train_from_fpn_trains_the_depth_head(gpu_ops):
    from sgcdet_amd.scene import make_scene
    from targets_contract import random_boxes
    # (depth_loss, use_gt_dpt): the reference configs' default, the depth-loss branch, the ground-truth-bins branch
    for depth_loss, use_gt in ((False, False), (True, False), (False, True)):
        det, w = _plumbing_detector(depth_loss, use_gt)
        N = 4                      # the plumbing scene with 4 views: the fewest that give every view its 2 neighbours
        feats, _, meta = make_scene(N, w["embed_dims"], kind="scannet", seed=14, device="cuda")
        H, W = feats[0].shape[-2:]
        gen = torch.Generator().manual_seed(5)
        img = torch.randn(1, N, 3, 4 * H, 4 * W, generator=gen).cuda()
        depth_maps = (torch.rand(1, N, 4 * H, 4 * W, generator=gen) * 4.6 + 0.3).cuda()
        boxes, gl = random_boxes(9, 6, False)
        boxes[:, :3] *= 0.55
        losses = det.forward_train_from_fpn(feats, img, [meta], [boxes.cuda()], [gl.cuda()], depth_maps=depth_maps)
        keys = {"loss_centerness", "loss_bbox", "loss_cls"} | ({"loss_dpt"} if depth_loss else set())
        assert set(losses) == keys, depth_loss
        sum(losses.values()).backward()
        got = {n: p.grad for n, p in det.named_parameters() if n.startswith("depth_head.")}
        if use_gt:                  # the ground-truth bins replace the depth head: it gets no gradient
            assert got and all(g is None for g in got.values())
        else:
            assert got and all(g is not None and torch.isfinite(g).all() for g in got.values()), depth_loss
            assert any(float(g.abs().max()) > 0 for n, g in got.items() if n.startswith("depth_head.fnet_mvs.")), depth_loss
        # the same losses as the depth distribution handed to forward_train_from_features (dropout off, BN batch stats)
        with torch.no_grad():
            dpt = det.depth_distribution(feats, img, [meta], depth_maps)
            if use_gt:
                gt = det.depth_head.get_downsampled_gt_depth(depth_maps).view(1, N, H, W, -1).permute(0, 1, 4, 2, 3)
                assert torch.equal(dpt, gt)
            want = det.forward_train_from_features(feats, [meta], dpt, [boxes.cuda()], [gl.cuda()])
            if depth_loss:
                want.update(det.depth_head.loss(depth_maps, dpt))
        for kname in keys:
            a, b = float(losses[kname].detach()), float(want[kname])
            assert abs(a - b) <= 1e-4 * max(1.0, abs(b)), (kname, depth_loss, use_gt, a, b)
