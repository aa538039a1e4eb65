"""Shared by tests/test_resnet_train_cpu.py and tests/test_gpu_resnet_train.py: the float64 restatement of the ResNet's
trainable blocks whose ReLUs are multiplications with GIVEN gates.

Why gates are given: a ReLU's derivative is a step.  An element whose pre-activation is within rounding of zero may be open in
one arithmetic and closed in another, and a flipped gate moves a weight gradient by a whole term of its sum -- at layer 4 of a
72 x 104 image that sum has 24 terms.  The HIP training path is therefore compared against float64 arithmetic on ITS OWN gates
(the signs of the layer outputs it kept); that the gates themselves are right is a separate, elementwise check.  Fed with the
module's own float64 gates the replica IS plain autograd of the module (tests/test_resnet_train_cpu.py), which keeps it honest.
"""
import torch
import torch.nn.functional as F


def fold64(bn):
    scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    return scale, bn.bias.detach().double() - bn.running_mean.detach().double() * scale


class GatedReplica:
    """``net``: a float64 ``ResNet`` on the CPU.  ``run(img, gates)`` -> the ``out_indices`` maps; ``gates``: None (every ReLU
    takes its gate from its own pre-activation) or one bool NCHW tensor per trainable layer in the order
    ``ResNet._forward_hip_train(keep=...)`` lists them (conv1, [conv2,] down, last -- the entry of a projection shortcut is not
    read: it has no ReLU).  After a run ``self.pre`` holds the pre-activations and ``self.own_gates`` their signs, same order."""

    def __init__(self, net):
        self.net = net

    def _layer(self, conv, bn, x, residual=None, relu=True):
        scale, shift = fold64(bn)
        t = F.conv2d(x, conv.weight, stride=conv.stride, padding=conv.padding) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
        if residual is not None:
            t = t + residual
        i = len(self.pre)
        self.pre.append(t.detach())
        self.own_gates.append(t.detach() > 0)
        if not relu:
            return t
        gate = self.own_gates[i] if self.gates is None else self.gates[i]
        assert gate.shape == t.shape and gate.dtype == torch.bool
        return t * gate.to(t.dtype)

    def _block(self, b, x):
        y = self._layer(b.conv1, b.bn1, x)
        bottleneck = hasattr(b, "conv3")
        if bottleneck:
            y = self._layer(b.conv2, b.bn2, y)
        identity = x if b.downsample is None else self._layer(b.downsample[0], b.downsample[1], x, relu=False)
        return self._layer(b.conv3, b.bn3, y, identity) if bottleneck else self._layer(b.conv2, b.bn2, y, identity)

    def run(self, img, gates=None):
        net = self.net
        self.gates, self.pre, self.own_gates = gates, [], []
        nf = net.frozen_prefix()
        with torch.no_grad():                                    # the frozen prefix: the module itself
            x = net.maxpool(net.relu(net.bn1(net.conv1(img))))
        outs, i = [], 0
        for s, name in enumerate(net.res_layers):
            for b in getattr(net, name):
                if i < nf:
                    with torch.no_grad():
                        x = b(x)
                else:
                    x = self._block(b, x)
                i += 1
            if s in net.out_indices:
                outs.append(x)
        return outs


def rows_to_nchw(rows, like):
    """[N*H*W, C] channels-last rows -> a CPU tensor of the NCHW shape of ``like``."""
    N, C, H, W = like.shape
    return rows.detach().cpu().view(N, H, W, C).permute(0, 3, 1, 2)

