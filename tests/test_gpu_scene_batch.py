"""Training on scene batches at module level on the GPU: neck_3d and the head on [B, C, X, Y, Z] with every
convolution pass on the batched HIP entries (``SGC_TRAIN_SCENE_BATCH`` = batched) or scene by scene around the joint norm (loop),
against the same modules on torch's library convolutions; the detector on two scenes.

The bounds are those of ``test_neck_and_head_autograd_on_hip_kernels_matches_library_convolutions`` (tests/test_gpu_modules.py), whose
neck, head and per-scene grid these tests use: outputs, loss and running statistics 1e-4 of the tensor scale; every convolution in
isolation 5e-5 against float64; end-to-end gradients (parameters, and the input's) 5e-2 of the gradient's scale and cosine > 0.9999."""
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def max_err(a, b):
    return float((a.detach().double() - b.detach().double()).abs().max())


def _neck_and_head():
    from sgcdet_amd.plugin.neck3d import FastIndoorImVoxelNeck
    from sgcdet_amd.plugin.bbox_head import ScanNetImVoxelHeadV2
    torch.manual_seed(3)
    neck = FastIndoorImVoxelNeck(in_channels=64, n_blocks=[1, 1, 1], out_channels=32).cuda().train()
    head = ScanNetImVoxelHeadV2(n_classes=5, n_channels=32, n_reg_outs=6, n_scales=3, limit=27, centerness_topk=18).cuda().train()
    return neck, head


def _run(nk, hd, inp, mode, scene_batch="batched"):
    from sgcdet_amd.plugin import conv_plan
    conv_plan.set_train_conv(mode)
    conv_plan.set_train_scene_batch(scene_batch)
    try:
        feats = nk(inp)
        ctr, reg, cls = hd(feats)
        loss = sum((t.float() ** 2).mean() for ts in (ctr, reg, cls) for t in ts) + sum((f ** 2).mean() for f in feats)
        loss.backward()
    finally:
        conv_plan.set_train_conv("hip")
        conv_plan.set_train_scene_batch("batched")
    return feats, (ctr, reg, cls), loss.detach()


def _rows(t):
    return t.permute(0, 2, 3, 4, 1).reshape(-1, t.shape[1]).contiguous()


@pytest.mark.parametrize("scene_batch", ["batched", "loop"])
@pytest.mark.parametrize("B", [2, 3])
def test_neck_and_head_train_on_a_scene_batch_as_the_library_convolutions_do(B, scene_batch):
    from sgcdet_amd.functions import ChannelsLastConv3dFunction, ChannelsLastConvTranspose3dFunction
    from sgcdet_amd.plugin import conv_plan
    neck, head = _neck_and_head()
    neck_b, head_b = copy.deepcopy(neck), copy.deepcopy(head)
    x = torch.randn(B, 64, 16, 12, 8, device="cuda")
    xa = x.to(memory_format=torch.channels_last_3d).clone().requires_grad_(True)
    xb = x.clone().requires_grad_(True)
    captured = {}
    for n, m in neck_b.named_modules():
        if isinstance(m, (torch.nn.Conv3d, torch.nn.ConvTranspose3d)):
            m.register_forward_hook(lambda mod, inp, out, n=n: captured.__setitem__(n + ".x", inp[0].detach().clone()))
            m.register_full_backward_hook(lambda mod, gin, gout, n=n: captured.__setitem__(n + ".dy", gout[0].detach().clone()))
    fa, ha, la = _run(neck, head, xa, "hip", scene_batch)
    fb, hb, lb = _run(neck_b, head_b, xb, "library")
    for a, b in list(zip(fa, fb)) + [(a, b) for ta, tb in zip(ha, hb) for a, b in zip(ta, tb)]:
        assert a.shape == b.shape and a.shape[0] == B
        assert max_err(a, b) < 1e-4 * max(1.0, float(b.detach().abs().max()))
    assert abs(float(la) - float(lb)) < 1e-5 * abs(float(lb))
    for (n, ba), (_, bb) in zip(neck.named_buffers(), neck_b.named_buffers()):
        assert max_err(ba.float(), bb.float()) < 1e-4 * max(1.0, float(bb.float().abs().max())), n
    # the norms saw the batch: one update of the running statistics, not one per scene
    assert all(int(m.num_batches_tracked) == 1 for m in neck.modules() if isinstance(m, torch.nn.BatchNorm3d))

    if scene_batch == "batched":              # every convolution in isolation on the real training tensors, all scenes in one launch per pass
        for n, m in neck_b.named_modules():
            if not isinstance(m, (torch.nn.Conv3d, torch.nn.ConvTranspose3d)):
                continue
            xin, dy = captured[n + ".x"], captured[n + ".dy"]
            grid = tuple(xin.shape[2:])
            xr, w = _rows(xin).requires_grad_(True), m.weight.detach().clone().requires_grad_(True)
            xd, wd = xin.double().requires_grad_(True), m.weight.detach().double().requires_grad_(True)
            if isinstance(m, torch.nn.ConvTranspose3d):
                y = ChannelsLastConvTranspose3dFunction.apply(xr, w, grid, B)
                yd = F.conv_transpose3d(xd, wd, None, 2)
            else:
                y = ChannelsLastConv3dFunction.apply(xr, w, grid, m.kernel_size[0], m.stride[0], B)
                yd = F.conv3d(xd, wd, None, m.stride, m.padding)
            y.backward(_rows(dy))
            yd.backward(dy.double())
            assert max_err(y, _rows(yd)) < 5e-5 * float(yd.detach().abs().max()), n
            assert max_err(w.grad, wd.grad) < 5e-5 * float(wd.grad.abs().max()), n
            assert max_err(xr.grad, _rows(xd.grad)) < 5e-5 * float(xd.grad.abs().max()), n

    # dL/dx is the end-to-end gradient with the longest chain (the backward of every norm of the neck): it is held to the bound and the
    # direction of the end-to-end parameter gradients.  Measured: 2.6e-2 (B = 2) and 3.7e-2 (B = 3) of its scale, the same three digits
    # for `batched` and `loop` -- the distance is between the kernel path and the library path, not between the two formulations.
    ga, gb = xa.grad.double().flatten(), xb.grad.double().flatten()
    print(f"B={B} {scene_batch}: input gradient off by {max_err(xa.grad, xb.grad) / float(xb.grad.abs().max()):.2e} of its scale, "
          f"cosine {float(torch.dot(ga, gb) / (ga.norm() * gb.norm())):.7f}")
    assert max_err(xa.grad, xb.grad) < 5e-2 * float(xb.grad.abs().max())
    assert float(torch.dot(ga, gb) / (ga.norm() * gb.norm())) > 0.9999
    for (n, pa), (_, pb) in zip(list(neck.named_parameters()) + list(head.named_parameters()),
                                list(neck_b.named_parameters()) + list(head_b.named_parameters())):
        if pb.grad is None:
            assert pa.grad is None, n
            continue
        ga, gb = pa.grad.double().flatten(), pb.grad.double().flatten()
        print(f"  {n}: off by {float((ga - gb).abs().max()) / max(1e-12, float(gb.abs().max())):.2e} of its scale")
        assert float((ga - gb).abs().max()) < 5e-2 * max(1e-12, float(gb.abs().max())), n
        if gb.numel() > 1:
            assert float(torch.dot(ga, gb) / (ga.norm() * gb.norm())) > 0.9999, n
    assert conv_plan.TRAIN_SCENE_BATCH == "batched"


def test_without_the_joint_norm_a_batch_of_two_is_the_mean_of_its_scenes():
    """With the neck's norms in eval mode nothing couples the scenes: the loss of the batch is the mean of the two single-scene losses
    and so is every parameter gradient, within 1e-4 of the gradient's scale (the splits of a batched launch may differ from the
    single-scene launch's: summation order)."""
    neck, head = _neck_and_head()
    with torch.no_grad():
        for m in neck.modules():
            if isinstance(m, torch.nn.BatchNorm3d):
                m.running_mean.normal_(0, 0.1), m.running_var.uniform_(0.8, 1.2)
                m.eval()
    x = torch.randn(2, 64, 16, 12, 8, device="cuda")
    x[1] *= 1.5
    params = list(neck.parameters()) + list(head.parameters())

    def grads(inp):
        for p in params:
            p.grad = None
        _, _, loss = _run(neck, head, inp.to(memory_format=torch.channels_last_3d).clone().requires_grad_(True), "hip")
        return loss, [None if p.grad is None else p.grad.clone() for p in params]
    l2, g2 = grads(x)
    l0, g0 = grads(x[:1])
    l1, g1 = grads(x[1:])
    assert abs(float(l2) - 0.5 * (float(l0) + float(l1))) < 1e-5 * abs(float(l2))
    n_checked = 0
    for a, b0, b1 in zip(g2, g0, g1):
        assert (a is None) == (b0 is None) == (b1 is None)
        if a is None:
            continue
        want = 0.5 * (b0.double() + b1.double())
        assert max_err(a, want) < 1e-4 * max(1e-12, float(want.abs().max()))
        n_checked += 1
    assert n_checked > 20


def _plumbing_detector():
    import sgcdet_amd.plugin  # noqa: F401
    from sgcdet_amd.mmcv_lite import build_detector
    from sgcdet_amd.scene import model_config, workload
    w = workload("cfg1_plumbing")
    cfg = model_config(w)
    cfg["depth_head"] = dict(type="DepthNet_Fusion", neighbor_img_num=2, downsample_factor=4, dbound=[0.2, 5, 0.4],
                             mono_channels=w["embed_dims"], loss_weight=0.5, max_tol=0, init_weight="none")
    torch.manual_seed(31)
    det = build_detector(cfg).cuda().train()
    for m in det.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    return det, w


def _two_scenes(w, n_views=4):
    from sgcdet_amd.scene import make_scene
    from targets_contract import random_boxes
    scenes = [make_scene(n_views, w["embed_dims"], kind="scannet", seed=s, device="cuda") for s in (14, 15)]
    feats = [torch.cat([sc[0][i] for sc in scenes]) for i in range(len(scenes[0][0]))]
    dpt = torch.cat([sc[1] for sc in scenes])
    metas = [sc[2] for sc in scenes]
    gts = []
    for seed in (6, 7):
        boxes, gl = random_boxes(9, seed, False)
        boxes[:, :3] *= 0.55
        gts.append((boxes.cuda(), gl.cuda()))
    return scenes, feats, dpt, metas, gts


def test_forward_train_from_fpn_on_two_scenes():
    """The plumbing size with two different scenes: finite losses, every parameter that gets a gradient from one scene gets one from
    the batch, and the losses are those of the library formulation."""
    from sgcdet_amd.plugin import conv_plan
    det, w = _plumbing_detector()
    scenes, feats, _, metas, gts = _two_scenes(w)
    H, W = feats[0].shape[-2:]
    img = torch.randn(2, 4, 3, 4 * H, 4 * W, generator=torch.Generator().manual_seed(5)).cuda()
    state = copy.deepcopy(det.state_dict())

    def step(fs, im, ms, gt, mode="hip"):
        det.load_state_dict(state)
        for p in det.parameters():
            p.grad = None
        conv_plan.set_train_conv(mode)
        try:
            losses = det.forward_train_from_fpn(fs, im, ms, [g[0] for g in gt], [g[1] for g in gt])
            sum(losses.values()).backward()
        finally:
            conv_plan.set_train_conv("hip")
        return {k: float(v.detach()) for k, v in losses.items()}, {n for n, p in det.named_parameters() if p.grad is not None}, \
            all(bool(torch.isfinite(p.grad).all()) for p in det.parameters() if p.grad is not None)
    one, with_grad_one, _ = step(scenes[0][0], img[:1], metas[:1], gts[:1])
    two, with_grad_two, finite = step(feats, img, metas, gts)
    lib, _, _ = step(feats, img, metas, gts, "library")
    assert set(two) == set(one) == {"loss_centerness", "loss_bbox", "loss_cls"}
    assert all(torch.isfinite(torch.tensor(v)) for v in two.values()) and finite
    assert with_grad_one and with_grad_one <= with_grad_two
    for k in two:
        assert abs(two[k] - lib[k]) <= 1e-4 * max(1.0, abs(lib[k])), (k, two[k], lib[k])


def test_simple_test_from_features_on_two_scenes_is_the_two_single_scene_calls():
    import sgcdet_amd.plugin  # noqa: F401
    from sgcdet_amd.mmcv_lite import build_detector
    from sgcdet_amd.scene import model_config, workload
    w = workload("cfg1_plumbing")
    torch.manual_seed(19)
    det = build_detector(model_config(w, nms_pre=150)).eval()
    gen = torch.Generator().manual_seed(18)
    with torch.no_grad():
        for _, p in list(det.voxel_head.named_parameters()) + list(det.bbox_head.named_parameters()):
            p.add_(torch.randn(p.shape, generator=gen) * 0.05)
    det = det.cuda()
    scenes, feats, dpt, metas, _ = _two_scenes(w)
    with torch.no_grad():
        both = det.simple_test_from_features(feats, metas, dpt)
        single = [det.simple_test_from_features(sc[0], [sc[2]], sc[1])[0] for sc in scenes]
        r2 = det.forward_features(feats, metas, dpt)
        r1 = [{k: ([t.clone() for t in v] if isinstance(v, list) else v.clone()) for k, v in det.forward_features(sc[0], [sc[2]], sc[1]).items()
               if v is not None} for sc in scenes]
    assert len(both) == 2
    for got, want in zip(both, single):
        for a, b in zip(got, want):
            a, b = (getattr(a, "tensor", a), getattr(b, "tensor", b))
            assert a.shape == b.shape and torch.equal(a, b)
    assert len(both[0][1]) > 0
    for k in ("centerness", "bbox_pred", "cls_score"):
        for i, t in enumerate(r2[k]):
            assert t.shape[0] == 2 and torch.equal(t, torch.cat([r[k][i] for r in r1]))
    assert torch.equal(r2["volume"], torch.cat([r["volume"] for r in r1])) and torch.equal(r2["valid"], torch.cat([r["valid"] for r in r1]))
