"""The ResNet backbone without a GPU (plugin/resnet.py): structure and state-dict keys, mmdet's ``train()``
semantics, the eval-mode plan replayed with torch convolutions, the detector's opt-in attach, and no outside access.

The detector test feeds images through ``simple_test(batch)`` on the CPU.  The voxel head has no CPU path (the product runs on the
GPU), so what runs here is everything in front of it -- backbone, FPN, depth head, all in their torch formulation -- and the test
checks that ``simple_test`` hands ``simple_test_from_features`` exactly the maps and the depth distribution of the by-hand
composition and returns its result dicts untouched; the boxes themselves are compared on the GPU (tests/test_gpu_resnet.py).
It uses 4 views, not 2: ``DepthNet_Fusion`` with the configs' ``neighbor_img_num=2`` indexes view ``i +- 2`` at the ends of the
sequence (``get_closest_frame_ids``, as in the reference), which needs at least 4.
"""
import json
import os
import socket

import pytest
import torch

from golden_util import max_err
from resnet_util import fill_resnet, replay_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_BACKBONE = dict(type="ResNet", depth=50, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=1,
                    norm_cfg=dict(type="BN", requires_grad=False), norm_eval=True, style="pytorch",
                    pretrained="torchvision://resnet50")
PARAMS = {18: 11176512, 34: 21284672, 50: 23508032, 101: 42500160}


def _build(**kw):
    import sgcdet_amd.plugin  # noqa: F401
    from sgcdet_amd.mmcv_lite import build_backbone
    return build_backbone(dict(REF_BACKBONE, **kw))


def _ref_model_cfg(name="SGCDet_ScanNet"):
    from sgcdet_amd.mmcv_lite import _wrap
    with open(os.path.join(ROOT, "tests", "golden", "ref_configs.json")) as f:
        return _wrap(json.load(f, object_hook=lambda d: tuple(d["__tuple__"]) if set(d) == {"__tuple__"} else d)[name])


def test_every_reference_config_builds_this_backbone():
    import sgcdet_amd.plugin  # noqa: F401
    from sgcdet_amd.mmcv_lite import build_backbone
    for name in ("SGCDet_ScanNet", "SGCDet_ARKit", "SGCDet_large_ScanNet200", "SGCDet_large_ARKit"):
        cfg = dict(_ref_model_cfg(name)["backbone"])
        assert cfg == REF_BACKBONE
        assert sum(p.numel() for p in build_backbone(cfg).parameters()) == PARAMS[50]


@pytest.mark.parametrize("depth", [18, 34, 50, 101])
def test_parameter_counts(depth):
    net = _build(depth=depth)
    assert sum(p.numel() for p in net.parameters()) == PARAMS[depth]
    assert not any(k.startswith("fc.") for k in net.state_dict())


def test_resnet50_keys_and_output_shapes():
    net = _build().eval()
    sd = net.state_dict()
    for k in ("conv1.weight", "bn1.running_var", "layer1.0.downsample.0.weight", "layer1.0.downsample.1.running_mean",
              "layer2.0.conv2.weight", "layer4.2.bn3.num_batches_tracked", "layer3.5.conv3.weight"):
        assert k in sd, k
    assert not any("fc." in k for k in sd)
    assert net.layer2[0].conv2.stride == (2, 2) and net.layer2[0].conv1.stride == (1, 1)       # style='pytorch'
    assert net.layer2[0].downsample[0].stride == (2, 2) and net.layer1[0].downsample[0].stride == (1, 1)
    assert net.pretrained == "torchvision://resnet50"
    with torch.no_grad():
        outs = net(torch.randn(2, 3, 72, 104, generator=torch.Generator().manual_seed(0)))
    assert [tuple(o.shape) for o in outs] == [(2, 256, 18, 26), (2, 512, 9, 13), (2, 1024, 5, 7), (2, 2048, 3, 4)]


def test_unused_mmdet_options_are_refused():
    for kw in (dict(deep_stem=True), dict(avg_down=True), dict(dcn=dict(type="DCN")), dict(plugins=[dict()]), dict(style="caffe"),
               dict(dilations=(1, 1, 2, 4)), dict(with_cp=True)):
        with pytest.raises(NotImplementedError):
            _build(**kw)
    with pytest.raises(KeyError):
        _build(depth=42)


def test_train_follows_mmdet():
    net = _build()
    net.train()
    bns = [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    assert len(bns) == 53 and not any(m.training for m in bns)                                   # norm_eval
    assert net.training and net.layer2.training and not net.layer1.training                      # frozen stages sit in eval
    assert not any(p.requires_grad for m in (net.conv1, net.bn1, net.layer1) for p in m.parameters())
    assert all(m.weight.requires_grad for m in net.layer2.modules() if isinstance(m, torch.nn.Conv2d))
    assert not any(p.requires_grad for m in bns for p in m.parameters())                         # norm_cfg requires_grad=False
    free = _build(frozen_stages=-1, norm_eval=False, norm_cfg=dict(type="BN", requires_grad=True)).train()
    assert all(p.requires_grad for p in free.parameters())
    assert all(m.training for m in free.modules() if isinstance(m, torch.nn.BatchNorm2d))
    # the gradient reaches the trainable stages through the torch formulation
    out = net(torch.randn(1, 3, 32, 32, generator=torch.Generator().manual_seed(1)))
    sum(o.sum() for o in out).backward()
    assert net.layer2[0].conv1.weight.grad is not None and net.conv1.weight.grad is None


@pytest.mark.parametrize("depth,shape", [(50, (2, 3, 72, 104)), (18, (2, 3, 64, 96))])
def test_plan_applied_with_torch_convolutions_reproduces_the_eval_forward(depth, shape):
    """Every planned layer with F.conv2d / F.max_pool2d through ``resnet.run_block`` itself (the block lowering of the HIP path)
    against the module's eval output: 1e-4 of each map's max-abs.  Seeded non-trivial BatchNorm statistics and a non-zero last
    norm per block, so the fold is exercised and no block is the identity."""
    from sgcdet_amd.plugin.resnet import resnet_plan
    net = fill_resnet(_build(depth=depth)).eval()
    assert all((m.running_var > 0).all() for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d))
    assert all(b.last_norm.weight.abs().min() > 0 for name in net.res_layers for b in getattr(net, name))
    img = torch.randn(*shape, generator=torch.Generator().manual_seed(depth))
    with torch.no_grad():
        want = net(img)
        P = resnet_plan(net)
        got = replay_plan(net, P, img)
    n_specs = sum(len(B) for blocks in P["stages"] for B in blocks)
    assert n_specs == {50: 16 * 3 + 4, 18: 8 * 2 + 3}[depth]
    assert len(got) == len(want) == 4
    for g, w in zip(got, want):
        assert g.shape == w.shape
        scale = w.abs().max().item()
        assert 1.0 < scale < 1e3
        err = max_err(g, w)
        print(f"resnet{depth} plan replay {tuple(w.shape)}: err {err:.3e} scale {scale:.2f}")
        assert err <= 1e-4 * scale


def test_no_outside_access(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a network connection was attempted")
    monkeypatch.setattr(socket.socket, "connect", refuse)
    monkeypatch.setattr(socket.socket, "connect_ex", refuse)
    monkeypatch.setattr(socket, "create_connection", refuse)
    net = _build(pretrained="torchvision://resnet50", init_cfg=dict(type="Pretrained", checkpoint="torchvision://resnet50"))
    net.init_weights()
    assert net.pretrained == "torchvision://resnet50" and net.init_cfg["checkpoint"] == "torchvision://resnet50"
    assert net.layer1[0].bn3.weight.abs().max() == 0 and net.bn1.weight.min() == 1             # zero_init_residual, unit norms


# ---- the detector ------------------------------------------------------------------------------------------------------------
def test_detector_attaches_the_backbone_on_request():
    import sgcdet_amd.plugin  # noqa: F401
    from sgcdet_amd.mmcv_lite import build_detector
    from sgcdet_amd.optim import reference_param_groups
    model = _ref_model_cfg()
    det = build_detector(model)
    assert det.backbone is None and "backbone" not in dict(det.named_children())
    assert not any(k.startswith("backbone.") for k in det.state_dict())
    n0 = sum(p.numel() for p in det.parameters())
    with pytest.raises(RuntimeError, match="attach_backbone"):
        det.simple_test(dict(img=torch.zeros(1, 4, 3, 64, 96), img_metas=[{}]))
    with pytest.raises(RuntimeError, match="attach_backbone"):
        det.build_volume(dict(img=torch.zeros(1, 4, 3, 64, 96), img_metas=[{}]))
    assert [g["name"] for g in reference_param_groups(det, 1e-4, 1e-2)] == ["others"]
    assert det.attach_backbone() is det
    assert sum(p.numel() for p in det.parameters()) - n0 == PARAMS[50]
    assert "backbone.layer3.5.conv3.weight" in det.state_dict() and "backbone.bn1.running_mean" in det.state_dict()
    groups = {g["name"]: g for g in reference_param_groups(det, 1e-4, 1e-2)}
    assert len(groups["backbone"]["params"]) > 0 and abs(groups["backbone"]["lr"] - 1e-5) < 1e-12
    frozen = {id(p) for m in (det.backbone.conv1, det.backbone.layer1) for p in m.parameters()}
    assert not any(id(p) in frozen for p in groups["backbone"]["params"])
    # an explicit config wins; without any config there is nothing to attach
    det.attach_backbone(dict(REF_BACKBONE, depth=18))
    assert sum(p.numel() for p in det.backbone.parameters()) == PARAMS[18]
    bare = build_detector({k: v for k, v in model.items() if k != "backbone"})
    with pytest.raises(RuntimeError, match="backbone"):
        bare.attach_backbone()


def test_build_optimizer_finds_the_backbone_group():
    import sgcdet_amd.plugin  # noqa: F401
    from sgcdet_amd.mmcv_lite import build_detector
    from sgcdet_amd.optim import build_optimizer
    det = build_detector(_ref_model_cfg()).attach_backbone()
    opt, _ = build_optimizer(det, dict(type="AdamW", lr=1e-4, weight_decay=1e-2),
                             dict(type="OneCycleLR", max_lr=1e-4, total_steps=10, pct_start=0.05, cycle_momentum=False,
                                  anneal_strategy="cos", final_div_factor=1000.0))
    by_name = {g["name"]: g for g in opt.param_groups}
    assert len(by_name["backbone"]["params"]) > 0 and len(by_name["others"]["params"]) > 0


def test_simple_test_composes_backbone_fpn_and_depth_head(monkeypatch):
    import sgcdet_amd.plugin  # noqa: F401
    from sgcdet_amd.mmcv_lite import build_detector
    from sgcdet_amd.scene import make_img_meta, model_config, workload
    w = workload("cfg1_plumbing")
    ref = _ref_model_cfg()
    cfg = model_config(w)                                     # config-1 grids
    cfg.update(backbone=dict(ref["backbone"]), neck=dict(ref["neck"]), depth_head=dict(ref["depth_head"], init_weight="none"))
    torch.manual_seed(3)
    det = build_detector(cfg).attach_backbone().eval()
    fill_resnet(det.backbone)
    n_views = 4
    meta = make_img_meta(n_views, "scannet", seed=2, img_hw=(64, 96))
    img = torch.randn(1, n_views, 3, 64, 96, generator=torch.Generator().manual_seed(4))
    seen = {}
    sentinel = [dict(boxes_3d="boxes", scores_3d="scores", labels_3d="labels")]

    def from_features(x, img_metas, dpt_dist, as_results=False):
        seen.update(x=x, img_metas=img_metas, dpt_dist=dpt_dist, as_results=as_results)
        return sentinel
    monkeypatch.setattr(det, "simple_test_from_features", from_features)
    with torch.no_grad():
        got = det.simple_test(dict(img=img, img_metas=[meta]))
        assert got is sentinel and det.forward_test(dict(img=img, img_metas=[meta])) is sentinel
        maps = det.backbone(img[0])
        x = det.image_features(maps)
        dpt = det.depth_distribution(x, img, [meta])
        via = det.extract_img_feat(img)
    assert [tuple(m.shape) for m in maps] == [(4, 256, 16, 24), (4, 512, 8, 12), (4, 1024, 4, 6), (4, 2048, 2, 3)]
    assert seen["as_results"] is True and seen["img_metas"][0] is meta
    assert len(seen["x"]) == 4 and all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(seen["x"], x, via))
    assert tuple(seen["x"][0].shape) == (1, n_views, 256, 16, 24)
    assert tuple(dpt.shape) == (1, n_views, 12, 16, 24) and torch.equal(seen["dpt_dist"], dpt)
