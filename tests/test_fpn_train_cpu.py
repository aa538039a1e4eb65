"""CPU checks of the image FPN's training path on the HIP kernels (plugin/fpn.py ``_train_hip_ok`` / ``_forward_hip``,
csrc/fpn_train.hip): the new entry points are declared, bound and exported and the workspace query answers on the
host; the integer index rule of the top-down kernels and its preimage ranges equal ``F.interpolate(mode="nearest")`` for every
size a stride-2 stage produces; and the path predicate follows the environment, the arithmetic mode, the channel counts and the
autograd state, with CPU tensors keeping the torch formulation."""
import os
import re

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sgc_upsample_nearest_add_nhwc", "sgc_upsample_nearest_add_backward_nhwc", "sgc_rows_colsum", "sgc_rows_colsum_workspace_floats")


def test_new_entry_points_are_declared_bound_and_exported():
    from sgcdet_amd import build
    from sgcdet_amd._abi import TRAIN_INTROSPECTION, TRAIN_SIGNATURES, Library
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sgcdet_amd_train.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(sgc_[a-z0-9_]+)\s*\(", text))
    assert set(NEW) <= declared
    assert set(NEW[:3]) <= set(TRAIN_SIGNATURES) and NEW[3] in TRAIN_INTROSPECTION
    assert [len(TRAIN_SIGNATURES[n]) for n in NEW[:3]] == [10, 9, 7]          # the stream included
    lib = Library(build.build(), train=True)                     # raises ImportError on a missing symbol
    for name in NEW:
        assert hasattr(lib._dll, name)
    # the query runs on the host: shapes that need a workspace (the largest of config 2 among them), one a single workgroup row
    # covers, and refused ones
    q = lib._dll.sgc_rows_colsum_workspace_floats
    assert q(192000, 256) == 256 * 256 and q(19200, 32) == 256 * 32 and q(257, 36) == 5 * 36
    assert q(63, 32) == 0 and q(1, 4) == 0
    assert q(19200, 30) == -1 and "C % 4" in lib.last_error()
    assert q(0, 32) == -1 and q(-5, 32) == -1 and q(1 << 24, 256) == -1


def _preimage(s, dst, src):
    """The destinations whose nearest source index is ``s``, as csrc/fpn_train.hip computes the range."""
    return range(-(-s * dst // src), min(-(-(s + 1) * dst // src), dst))


def test_index_rule_and_preimages_equal_nearest_interpolation():
    from sgcdet_amd.plugin.fpn import _nearest_index
    for dst in range(1, 301):
        for src in sorted({(dst + 1) // 2, dst // 2} - {0}):
            idx = _nearest_index(dst, src, "cpu")
            want = F.interpolate(torch.arange(src, dtype=torch.float32).view(1, 1, 1, src), size=(1, dst), mode="nearest").view(-1).long()
            assert torch.equal(idx, want), (dst, src)
            assert idx.tolist() == [min(d * src // dst, src - 1) for d in range(dst)]          # the kernels' integer expression
            pre = [_preimage(s, dst, src) for s in range(src)]
            # never empty; at most two per axis for src = ceil(dst / 2), three for the floor of an odd dst (5 <- 2: 0 0 0 1 1)
            assert all(1 <= len(p) <= (2 if src == (dst + 1) // 2 else 3) for p in pre), (dst, src)
            assert [d for p in pre for d in p] == list(range(dst)), (dst, src)                 # a partition of [0, dst), in order
            assert all(idx[d] == s for s, p in enumerate(pre) for d in p)


def _fpn(channels=(32, 64, 96, 128), out=32):
    from sgcdet_amd.plugin.fpn import FPN
    return FPN(list(channels), out, 4)


class _Fake:
    """Stands for a CUDA float32 map in the predicate (which reads only these attributes)."""
    is_cuda, dtype = True, torch.float32

    def __init__(self, requires_grad=False):
        self.requires_grad = requires_grad


def test_path_predicate(monkeypatch):
    from sgcdet_amd.plugin import conv_plan, fpn as fpn_mod
    monkeypatch.delenv("SGC_FPN_TRAIN_HIP", raising=False)
    net = _fpn()
    maps = [_Fake() for _ in range(4)]
    monkeypatch.setattr(fpn_mod, "TRAIN_HIP_DEFAULT", "1")
    assert net._train_hip_ok(maps)
    monkeypatch.setattr(fpn_mod, "TRAIN_HIP_DEFAULT", "0")       # the default is what the environment falls back to
    assert not net._train_hip_ok(maps)
    monkeypatch.setenv("SGC_FPN_TRAIN_HIP", "1")
    assert net._train_hip_ok(maps)
    monkeypatch.setenv("SGC_FPN_TRAIN_HIP", "0")
    assert not net._train_hip_ok(maps)
    monkeypatch.setenv("SGC_FPN_TRAIN_HIP", "1")
    monkeypatch.setattr(conv_plan, "CONV_PRODUCTS", 2)           # set_conv_mode("fp16"): the weight planes are bfloat16 bits
    assert not net._train_hip_ok(maps)
    monkeypatch.setattr(conv_plan, "CONV_PRODUCTS", 3)
    assert net._train_hip_ok(maps)
    assert not _fpn((32, 64, 96, 120))._train_hip_ok(maps)       # a channel count that is no multiple of 32
    assert not _fpn(out=48)._train_hip_ok(maps)
    with torch.no_grad():
        assert not net._train_hip_ok(maps)
    for p in net.parameters():                                   # nothing wants a gradient ...
        p.requires_grad = False
    assert not net._train_hip_ok(maps)
    assert net._train_hip_ok([_Fake(), _Fake(True), _Fake(), _Fake()])          # ... but an input
    for p in net.parameters():
        p.requires_grad = True
    half = _Fake()
    half.dtype = torch.float16
    assert not net._train_hip_ok([half] + maps[1:])
    # CPU tensors keep the torch formulation, and give its result
    g = torch.Generator().manual_seed(5)
    xs = [torch.randn(2, c, h, w, generator=g) for c, (h, w) in zip((32, 64, 96, 128), ((15, 20), (8, 10), (4, 5), (2, 3)))]
    assert not net._train_hip_ok(xs)
    got, want = net(xs), net._forward_torch(xs)
    assert len(got) == 4 and all(a.requires_grad and torch.equal(a, b) for a, b in zip(got, want))
