"""CPU checks of the backbone's training path on the HIP kernels (plugin/resnet.py ``_forward_hip_train``): the
new entry points are declared, bound and exported; the path predicate and the frozen-prefix split follow the module's
configuration; and the gated float64 replica that the GPU test measures against equals plain float64 autograd of the module
when it is fed the module's own gates."""
import copy
import os
import re

import pytest
import torch

from resnet_train_util import GatedReplica
from resnet_util import fill_resnet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sgc_conv2d_wgrad_bf16x3", "sgc_conv2d_wgrad_workspace_floats", "sgc_frozen_norm_act_backward")
REF = dict(type="ResNet", depth=50, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=1,
           norm_cfg=dict(type="BN", requires_grad=False), norm_eval=True, style="pytorch")


def _build(**over):
    import sgcdet_amd.plugin  # noqa: F401
    from sgcdet_amd.mmcv_lite import build_backbone
    return build_backbone(dict(REF, **over))


def test_new_entry_points_are_declared_bound_and_exported():
    from sgcdet_amd import build
    from sgcdet_amd._abi import TRAIN_INTROSPECTION, TRAIN_SIGNATURES, Library
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sgcdet_amd_train.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(sgc_[a-z0-9_]+)\s*\(", text))
    assert set(NEW) <= declared
    assert {"sgc_conv2d_wgrad_bf16x3", "sgc_frozen_norm_act_backward"} <= set(TRAIN_SIGNATURES)
    assert "sgc_conv2d_wgrad_workspace_floats" in TRAIN_INTROSPECTION
    assert len(TRAIN_SIGNATURES["sgc_conv2d_wgrad_bf16x3"]) == 13 and len(TRAIN_SIGNATURES["sgc_frozen_norm_act_backward"]) == 9
    lib = Library(build.build(), train=True)                     # raises ImportError on a missing symbol
    for name in NEW:
        assert hasattr(lib._dll, name)
    # the query runs on the host: a shape that splits its reduction, one that does not, one the entry refuses
    q = lib._dll.sgc_conv2d_wgrad_workspace_floats
    assert q(4, 32, 32, 32, 32, 3, 1) > 0 and q(2, 8, 8, 32, 32, 3, 2) == 0
    assert q(2, 8, 8, 30, 32, 3, 1) == -1 and q(2, 8, 8, 32, 32, 2, 2) == -1 and q(2, 8, 8, 32, 32, 3, 3) == -1


def test_path_predicate(monkeypatch):
    from sgcdet_amd.plugin import conv_plan
    monkeypatch.delenv("SGC_BACKBONE_TRAIN_HIP", raising=False)
    ref = _build(depth=18).train()
    assert ref._train_hip_config_ok()
    assert not ref.eval()._train_hip_config_ok()                 # the eval forward has its own path
    ref.train()
    assert not _build(depth=18, frozen_stages=-1).train()._train_hip_config_ok()
    assert not _build(depth=18, norm_eval=False).train()._train_hip_config_ok()
    assert not _build(depth=18, norm_cfg=dict(type="BN", requires_grad=True)).train()._train_hip_config_ok()
    monkeypatch.setenv("SGC_BACKBONE_TRAIN_HIP", "0")
    assert not ref._train_hip_config_ok()
    monkeypatch.setenv("SGC_BACKBONE_TRAIN_HIP", "1")
    assert ref._train_hip_config_ok()
    monkeypatch.setattr(conv_plan, "CONV_PRODUCTS", 2)           # set_conv_mode("fp16"): the weight planes are bfloat16 bits
    assert not ref._train_hip_config_ok()
    monkeypatch.setattr(conv_plan, "CONV_PRODUCTS", 3)
    # CPU tensors keep the torch formulation whatever the configuration says
    maps = ref(torch.randn(1, 3, 32, 32))
    assert maps[3].requires_grad and maps[0].is_contiguous()


@pytest.mark.parametrize("depth", [18, 50])
def test_frozen_prefix_split(depth):
    for frozen, layers in ((1, ["layer1"]), (2, ["layer1", "layer2"]), (0, []), (4, ["layer1", "layer2", "layer3", "layer4"])):
        net = _build(depth=depth, frozen_stages=frozen).train()
        assert net.frozen_prefix() == sum(len(getattr(net, n)) for n in layers)
        assert net.blocks()[:net.frozen_prefix()] == [b for n in layers for b in getattr(net, n)]
    net = _build(depth=depth, frozen_stages=1).train()
    for p in net.layer2[0].parameters():                         # a block frozen by hand extends the prefix; a later one does not
        p.requires_grad = False
    assert net.frozen_prefix() == len(net.layer1) + 1
    for p in net.layer3[1].parameters():
        p.requires_grad = False
    assert net.frozen_prefix() == len(net.layer1) + 1


@pytest.mark.parametrize("depth,shape", [(18, (2, 3, 64, 96)), (50, (1, 3, 72, 104))])
def test_gated_replica_on_the_modules_own_gates_is_plain_autograd(depth, shape):
    net = fill_resnet(_build(depth=depth)).double().train()
    img = torch.randn(*shape, generator=torch.Generator().manual_seed(depth), dtype=torch.float64)
    maps = net(img)
    g = torch.Generator().manual_seed(3)
    cots = [torch.randn(m.shape, generator=g, dtype=torch.float64) for m in maps]
    sum((m * c).sum() for m, c in zip(maps, cots)).backward()
    want = {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}
    assert want and all(n.startswith(("layer2", "layer3", "layer4")) and ".bn" not in n and "downsample.1" not in n for n in want)

    twin = copy.deepcopy(net)
    twin.zero_grad(set_to_none=True)
    rep = GatedReplica(twin)
    first = rep.run(img)                                         # own gates: records them
    gates = list(rep.own_gates)
    for a, b in zip(first, maps):
        assert (a - b).abs().max() <= 1e-12 * b.abs().max()
    outs = rep.run(img, gates)                                   # the same gates, handed in
    sum((m * c).sum() for m, c in zip(outs, cots)).backward()
    got = {n: p.grad for n, p in twin.named_parameters() if p.grad is not None}
    assert set(got) == set(want)
    for n in want:
        assert (got[n] - want[n]).abs().max() <= 1e-11 * want[n].abs().max(), n
