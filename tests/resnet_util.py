"""Shared by tests/test_resnet_cpu.py and tests/test_gpu_resnet.py: seeded ResNet weights and the replay of its plan."""
import zlib

import torch
import torch.nn.functional as F


def fill_resnet(net, base_seed=11):
    """Every parameter and buffer of a ``ResNet`` from a generator seeded by its state-dict key.  Convolutions: He-scaled
    (std sqrt(2 / fan_in)); running variances in [0.5, 1.5); running means and BatchNorm biases 0.1 randn; BatchNorm weights
    1 + 0.2 randn, except the LAST norm of a block (the one in front of the skip addition): 0.35 + 0.1 randn, non-zero so no
    block degenerates to the identity and small enough that 16 (33 at depth 101) skip additions keep every output map
    between O(1) and O(1e3)."""
    sd = net.state_dict()
    last = "bn3.weight" if any(".bn3." in k for k in sd) else "bn2.weight"
    with torch.no_grad():
        for k in sorted(sd):
            t = sd[k]
            if not t.is_floating_point():
                continue
            g = torch.Generator().manual_seed(base_seed + zlib.crc32(k.encode()))
            if k.endswith("running_var"):
                v = 0.5 + torch.rand(t.shape, generator=g)
            elif k.endswith("running_mean") or (t.dim() == 1 and k.endswith("bias")):
                v = 0.1 * torch.randn(t.shape, generator=g)
            elif t.dim() == 1 and k.startswith("layer") and k.endswith(last):
                v = 0.35 + 0.1 * torch.randn(t.shape, generator=g)
            elif t.dim() == 1:
                v = 1.0 + 0.2 * torch.randn(t.shape, generator=g)
            else:
                v = torch.randn(t.shape, generator=g) * (2.0 / t[0].numel()) ** 0.5
            t.copy_(v.to(t.dtype))
    return net


def apply_spec(x, L, residual=None, relu=True, relu_after_add=False):
    """One planned layer (``Conv2dSpec``) on an NCHW tensor with plain F.conv2d and the epilogue order of the kernels."""
    k = L.k
    _, coutp, cinp = L.w.shape
    assert x.shape[1] == cinp and not L.transposed
    y = F.conv2d(x, L.w.reshape(k, k, coutp, cinp).permute(2, 3, 0, 1).to(x.dtype), stride=L.stride, padding=k // 2)
    y = y * L.scale.view(1, -1, 1, 1).to(x.dtype) + L.shift.view(1, -1, 1, 1).to(x.dtype)
    if relu:
        y = F.relu(y)
    if residual is not None:
        y = y + residual
    if relu_after_add:
        y = F.relu(y)
    return y


class TorchSpec:
    """Stands in for a ``Conv2dSpec`` inside ``resnet.run_block``: the same call signature on NCHW tensors (``nhw`` is carried
    along but the tensor's own shape rules), so the test replays the block lowering itself, not a copy of it."""

    def __init__(self, spec):
        self.spec = spec

    def __call__(self, x, nhw, residual=None, relu=True, relu_after_add=False):
        y = apply_spec(x, self.spec, residual, relu, relu_after_add)
        return y, (y.shape[0], y.shape[2], y.shape[3])


def replay_plan(net, P, img):
    """The plan ``P`` of ``net`` applied with F.conv2d / F.max_pool2d in the order ``ResNet._forward_hip`` uses."""
    from sgcdet_amd.plugin.resnet import run_block
    st = P["stem"]
    assert st.w.shape == (64, 160) and st.w[:, 147:].abs().max() == 0
    x = F.conv2d(img, st.w[:, :147].reshape(64, 3, 7, 7), stride=2, padding=3)
    x = F.relu(x * st.scale.view(1, -1, 1, 1) + st.shift.view(1, -1, 1, 1))
    x = F.max_pool2d(x, 3, 2, 1)
    outs = []
    for i, blocks in enumerate(P["stages"]):
        for B in blocks:
            x, _ = run_block({k: TorchSpec(v) for k, v in B.items()}, x, None)
        if i in net.out_indices:
            outs.append(x)
    return outs
