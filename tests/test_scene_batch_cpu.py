"""Training on scene batches, the parts that need no GPU: the declarations of include/sgcdet_amd_scene_batch.h and
their binding, the row helpers on [B, C, X, Y, Z], and the neck's one walker on a batch -- driven, as in tests/test_neck_walker_cpu.py,
with torch stand-ins for the layers on CPU tensors."""
import copy
import functools
import inspect
import os
import re

import pytest
import torch

from sgcdet_amd.plugin import conv_plan
from sgcdet_amd.plugin.conv_plan import TrainConv3d, bn_rows, rows_to_ncdhw, to_channels_last_rows
from sgcdet_amd.plugin.neck3d import FastIndoorImVoxelNeck

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_header_declares_what_the_tables_bind_and_the_library_exports_it():
    from sgcdet_amd import _abi, build
    text = open(os.path.join(ROOT, "include", "sgcdet_amd_scene_batch.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(re.findall(r"\b(sgc_\w+)\s*\(", text))
    new = set(_abi.SCENE_BATCH_SIGNATURES) | set(_abi.SCENE_BATCH_INTROSPECTION)
    assert declared == sorted(new) and len(new) == 4
    for table in (_abi.SIGNATURES, _abi.INTROSPECTION, _abi.TRAIN_SIGNATURES, _abi.TRAIN_INTROSPECTION, _abi.IMAGE_SIGNATURES,
                  _abi.IMAGE_INTROSPECTION, _abi.DEPTH_TRAIN_SIGNATURES, _abi.LEVEL_TRAIN_SIGNATURES, _abi.LEVEL_TRAIN_INTROSPECTION):
        assert not new & set(table)
    # the arguments of the scene-less twins plus `scenes` (the stream is appended by the binding)
    assert len(_abi.SCENE_BATCH_SIGNATURES["sgc_conv3d_cl_bf16x3_batched"]) == len(_abi.SIGNATURES["sgc_conv3d_cl_bf16x3"]) + 1
    assert len(_abi.SCENE_BATCH_SIGNATURES["sgc_conv3d_wgrad_bf16x3_batched"]) == len(_abi.SIGNATURES["sgc_conv3d_wgrad_bf16x3"]) + 1
    assert len(_abi.SCENE_BATCH_INTROSPECTION["sgc_conv3d_batched_workspace_floats"][1]) == len(_abi.INTROSPECTION["sgc_conv3d_workspace_floats"][1]) + 1
    lib = _abi.Library(build.build(), train=True)                 # raises ImportError on a missing symbol
    q = lib._dll.sgc_conv3d_batched_workspace_floats
    # host code: with one scene the batched query IS the scene-less one; the split count may follow the batch, the slab always does
    for args in ((10, 10, 4, 1024, 1024, 3, 1, 0, 1), (6, 5, 3, 64, 96, 3, 1, 0, 1), (16, 16, 8, 128, 160, 3, 1, 0, 1), (5, 5, 2, 64, 96, 2, 2, 1, 1)):
        one = int(lib._dll.sgc_conv3d_workspace_floats(*args))
        assert int(q(*args, 1)) == one
        ox = [2 * d for d in args[:3]] if args[7] else [(d + 2 * (args[5] // 2) - args[5]) // args[6] + 1 for d in args[:3]]
        slab = ox[0] * ox[1] * ox[2] * args[4]
        for scenes in (2, 3):
            n = int(q(*args, scenes))
            assert n % (scenes * slab) == 0 and (one == 0 or 0 < n // (scenes * slab) <= one // slab)      # never more splits than alone
    w1, wq = lib._dll.sgc_conv3d_wgrad_workspace_floats, lib._dll.sgc_conv3d_wgrad_batched_workspace_floats
    for args in ((16, 16, 8, 32, 64, 3, 1), (7, 5, 3, 64, 128, 3, 2), (10, 10, 4, 96, 64, 2, 2)):
        assert int(wq(*args, 1)) == int(w1(*args)) and int(wq(*args, 3)) % (args[5] ** 3 * args[3] * args[4]) == 0
    assert int(wq(16, 16, 8, 32, 64, 3, 1, 0)) == -1 and int(q(10, 10, 4, 32, 32, 3, 1, 0, 1, 0)) == 0


def test_the_row_helpers_round_trip_a_batch():
    torch.manual_seed(0)
    for shape in ((1, 32, 3, 4, 5), (2, 32, 3, 4, 5), (3, 8, 2, 2, 6)):
        x = torch.randn(shape)
        for t in (x, x.to(memory_format=torch.channels_last_3d)):
            rows, grid = to_channels_last_rows(t)
            B, C = shape[0], shape[1]
            V = shape[2] * shape[3] * shape[4]
            assert grid == shape[2:] and rows.shape == (B * V, (C + 31) // 32 * 32) and rows.is_contiguous()
            for b in range(B):                        # scene b occupies rows [b V, (b + 1) V)
                assert torch.equal(rows[b * V:(b + 1) * V, :C], x[b].permute(1, 2, 3, 0).reshape(V, C))
            assert bool((rows[:, C:] == 0).all())
            back = rows_to_ncdhw(rows, grid, C)
            assert back.shape == x.shape and torch.equal(back, x)
            assert back.data_ptr() == rows.data_ptr()                # a view


class BatchTorchLayer:
    """A layer with ``ConvSpec``'s call signature on the rows of a batch: the two modules and the tail in torch."""

    def __init__(self, conv, bn):
        self.conv, self.bn, self.cout = conv, bn, conv.out_channels

    def __call__(self, x, grid, residual=None, relu=0, out_mask=None, act=None):
        y = self.bn(self.conv(rows_to_ncdhw(x, grid, self.conv.in_channels).contiguous()))
        og = tuple(y.shape[2:])
        if residual is not None:
            residual = rows_to_ncdhw(residual, og, self.cout)
        if relu == 2:
            y = torch.relu(y) + residual
        else:
            y = y if residual is None else y + residual
            y = torch.relu(y) if relu else y
        return y.permute(0, 2, 3, 4, 1).reshape(-1, self.cout), og


@pytest.mark.parametrize("training", [False, True])
def test_the_walker_on_torch_layers_is_the_module_on_a_batch_of_two(training):
    torch.manual_seed(0)
    neck = FastIndoorImVoxelNeck(in_channels=8, n_blocks=[1, 2, 1], out_channels=4)
    with torch.no_grad():
        for m in neck.modules():
            if isinstance(m, torch.nn.BatchNorm3d):
                m.weight.uniform_(0.5, 1.5), m.bias.normal_(0, 0.2), m.running_mean.normal_(0, 0.2), m.running_var.uniform_(0.5, 1.5)
    x = torch.randn(2, 8, 8, 8, 4)
    x[1] *= 1.7                                                     # two scenes with different statistics
    neck.train(training)
    twin = copy.deepcopy(neck)
    with torch.no_grad():
        want = neck(x)
        got = twin._run(x, twin._build_plan(BatchTorchLayer))
    assert [tuple(t.shape) for t in got] == [(2, 4, 8, 8, 4), (2, 4, 4, 4, 2), (2, 4, 2, 2, 1)]
    for a, b in zip(got, want):
        assert a.shape == b.shape and float((a - b).abs().max()) <= 1e-6
    for (n, a), (_, b) in zip(twin.named_buffers(), neck.named_buffers()):
        assert float((a.double() - b.double()).abs().max()) <= 1e-6, n
    if training:
        # the norms saw the batch: the two scenes on their own give other outputs
        alone = copy.deepcopy(neck)
        with torch.no_grad():
            solo = alone(x[:1])
        assert float((solo[0] - want[0][:1]).abs().max()) > 1e-3


def test_bn_rows_hands_a_batch_to_norms_of_other_types():
    """A norm that is no plain BatchNorm (SyncBatchNorm3d ...) gets the [B, C, X, Y, Z] view of the rows."""
    seen = []

    class Spy(torch.nn.BatchNorm3d):
        def forward(self, x):
            seen.append(tuple(x.shape))
            return super().forward(x)
    torch.manual_seed(1)
    bn, ref = Spy(8).train(), torch.nn.BatchNorm3d(8).train()
    x = torch.randn(3, 8, 2, 3, 4)
    rows, grid = x.permute(0, 2, 3, 4, 1).reshape(-1, 8), (2, 3, 4)
    res = torch.randn_like(rows)
    got = bn_rows(bn, rows, grid, residual=res, relu=True)
    want = torch.relu(ref(x).permute(0, 2, 3, 4, 1).reshape(-1, 8) + res)
    assert seen == [(3, 8, 2, 3, 4)] and float((got - want).detach().abs().max()) <= 1e-6
    assert float((bn.running_var - ref.running_var).abs().max()) <= 1e-6


def test_the_scene_count_reaches_the_functions_and_the_switch_has_two_values():
    from sgcdet_amd import functions, tensor_api
    assert "scenes" in inspect.signature(functions.ChannelsLastConv3dFunction.forward).parameters
    assert "scenes" in inspect.signature(functions.ChannelsLastConvTranspose3dFunction.forward).parameters
    assert inspect.signature(tensor_api.TensorOps.conv3d_cl_bf16x3).parameters["scenes"].default == 1
    assert inspect.signature(tensor_api.TensorOps.conv3d_wgrad_bf16x3).parameters["scenes"].default == 1
    conv, bn = torch.nn.Conv3d(32, 32, 3, 1, 1, bias=False), torch.nn.BatchNorm3d(32)
    assert TrainConv3d(conv, bn).scenes == 1 and functools.partial(TrainConv3d, scenes=3)(conv, bn).scenes == 3
    assert conv_plan.TRAIN_SCENE_BATCH == os.environ.get("SGC_TRAIN_SCENE_BATCH", "batched")
    try:
        conv_plan.set_train_scene_batch("loop")
        assert conv_plan.TRAIN_SCENE_BATCH == "loop"
        with pytest.raises(ValueError):
            conv_plan.set_train_scene_batch("both")
    finally:
        conv_plan.set_train_scene_batch("batched")
    # a batch on CPU tensors keeps the library formulation (no silent kernel path without a GPU)
    assert not conv_plan.train_conv_on_hip(torch.zeros(2, 32, 2, 2, 2), [32])
