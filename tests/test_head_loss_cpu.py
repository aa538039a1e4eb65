"""CPU checks of the fused head loss's boundary (include/sgcdet_amd_train.h section 11): the symbols are declared, bound and exported, the
host-side refusals work, the new code object carries no packed-FP32 instruction, and on CPU tensors ``head.loss`` keeps the torch path."""
import os
import re
import struct
import subprocess

import torch

from head_loss_contract import torch_path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"sgc_head_loss_forward", "sgc_head_loss_finalize", "sgc_head_loss_scale_grads", "sgc_head_loss_workspace_bytes"}


def test_symbols_are_declared_bound_and_exported():
    from sgcdet_amd import build
    from sgcdet_amd._abi import (HEAD_LOSS_LEVEL_BYTES, HEAD_LOSS_MAX_SCALES, INTROSPECTION, SIGNATURES, TRAIN_INTROSPECTION, TRAIN_SIGNATURES,
                                 Library)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sgcdet_amd_train.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(sgc_[a-z0-9_]+)\s*\(", text))
    assert NEW <= declared
    assert NEW - {"sgc_head_loss_workspace_bytes"} <= set(TRAIN_SIGNATURES) and "sgc_head_loss_workspace_bytes" in TRAIN_INTROSPECTION
    assert not NEW & (set(SIGNATURES) | set(INTROSPECTION))
    assert f"#define SGC_HEAD_LOSS_MAX_SCALES {HEAD_LOSS_MAX_SCALES}" in text and struct.calcsize("<4Qq6i") == HEAD_LOSS_LEVEL_BYTES
    lib = Library(build.build(), train=True)                     # raises ImportError on a missing symbol
    dll = lib._dll
    # the workspace query is host code: 4 header doubles + 5 partial sums per workgroup of 256 points, every level rounded up
    assert dll.sgc_head_loss_workspace_bytes(29200, 3) == 8 * (4 + 5 * (115 + 3)) and dll.sgc_head_loss_workspace_bytes(0, 3) == 0
    # refusals happen before any launch (host code: runs without a GPU); pointers are never dereferenced on the way
    level = struct.pack("<4Qq6i", 8, 8, 8, 8, 100, 1, 100, 1, 100, 1, 0)
    args = lambda n_scales, n_reg, rotated, n=100: (level * max(n_scales, 1), n_scales, 8, 8, 8, 8, n * max(n_scales, 1), n_reg, 18, rotated,
                                                    2.0, 0.25, 1.0, 1.0, 1.0, None, 8, 8, 8, 8, 1 << 20, None)
    assert dll.sgc_head_loss_forward(*args(5, 6, 0)) == -3 and "scales" in lib.last_error()                       # SGC_EUNSUP
    assert dll.sgc_head_loss_forward(*args(1, 5, 0)) == -3 and "n_reg" in lib.last_error()
    assert dll.sgc_head_loss_forward(*args(1, 7, 0)) == -3 and "rotated" in lib.last_error()
    mismatch = list(args(1, 6, 0))
    mismatch[6] = 99
    assert dll.sgc_head_loss_forward(*mismatch) == -3 and "points" in lib.last_error()
    assert dll.sgc_head_loss_forward(None, *args(1, 6, 0)[1:]) == -1                                              # SGC_EINVAL
    small = list(args(1, 6, 0))
    small[-2] = 16
    assert dll.sgc_head_loss_forward(*small) == -1 and "workspace" in lib.last_error()


def test_head_loss_code_object_carries_no_packed_fp32_instructions(tmp_path):
    """The approach of test_kernels_carry_no_packed_fp32_instructions (tests/test_abi_cpu.py) on the new kernels."""
    from sgcdet_amd import build
    from test_abi_cpu import _device_disassembly
    build.build()
    dis = [d for d in _device_disassembly(build.LIB, tmp_path) if "head_loss_main_kernel" in d]
    assert len(dis) == 1
    for kernel in ("head_loss_main_kernel", "head_loss_riou_kernel", "head_loss_final_kernel", "head_loss_scale_kernel"):
        assert kernel in dis[0]
    assert "v_fma_f64" in dis[0] or "v_mul_f64" in dis[0]                       # the disassembly is the real thing
    packed = [ln.strip() for ln in dis[0].splitlines() if re.search(r"\bv_pk_\w+_f32\b", ln)]
    assert not packed, f"{len(packed)} packed-FP32 instructions, e.g. {packed[:3]}"


def test_cpu_tensors_keep_the_torch_path(oracle_ops, monkeypatch):
    """``head.loss`` on CPU tensors returns what it returned before: the losses.py functions composed as _loss_single composes them
    (tests/head_loss_contract.torch_path, float32), bit for bit, for both heads -- and never asks for the fused operator."""
    import sgcdet_amd.plugin  # noqa: F401
    from sgcdet_amd import ext, functions
    from sgcdet_amd.mmcv_lite import HEADS
    from targets_contract import random_boxes
    monkeypatch.setattr(ext, "ops", lambda: oracle_ops)                       # the CPU binding of the same ABI (assign_targets)

    def refuse(*a, **k):
        raise AssertionError("the fused head loss must not be taken on CPU tensors")
    monkeypatch.setattr(functions.HeadLossFunction, "apply", refuse)
    meta = dict(lidar2img=dict(origin=[0.0, 0.0, 0.5]))
    g = torch.Generator().manual_seed(1)
    feats = [torch.randn(1, 32, 8 >> i, 8 >> i, 4 >> i, generator=g) for i in range(3)]
    valid = (torch.rand(1, 1, 8, 8, 4, generator=g) < 0.8).float()
    for kind, n_classes, n_reg in (("ScanNetImVoxelHeadV2", 18, 6), ("SunRgbdImVoxelHeadV2", 17, 7)):
        rotated = n_reg == 7
        boxes, labels = random_boxes(6, 2, rotated)
        boxes[:, :3] *= 0.5
        labels = labels % n_classes
        torch.manual_seed(0)
        head = HEADS.build(dict(type=kind, n_classes=n_classes, n_channels=32, n_reg_outs=n_reg, n_scales=3, limit=27, centerness_topk=18))
        head.voxel_size = [0.8, 0.8, 0.8]
        head.init_weights()
        assert head._fused_loss([feats[0]]) is False
        ctr, reg, cls = (list(t) for t in zip(*[head.forward_single(f, s) for f, s in zip(feats, head.scales)]))
        got, sem, geo = head.loss(ctr, reg, cls, valid, [meta], [boxes], [labels])
        sizes = [c.shape[-3:] for c in ctr]
        pts = head.get_points(sizes, meta["lidar2img"]["origin"], "cpu")
        ct_t, bx_t, lb, _ = head.get_targets(pts, boxes, labels)
        vals = [torch.nn.Upsample(size=s, mode="trilinear")(valid).round().bool()[0] for s in sizes]
        want, _ = torch_path(rotated, [c[0] for c in ctr], [r[0] for r in reg], [s[0] for s in cls], vals, torch.cat(pts), ct_t, bx_t, lb,
                             torch.float32)
        assert int(((lb >= 0) & torch.cat([v.reshape(-1) for v in vals])).sum()) > 0
        for k, w in zip(("loss_centerness", "loss_bbox", "loss_cls"), want):
            assert torch.equal(got[k].detach(), w.detach()), (kind, k, float(got[k]), float(w))
        assert torch.equal(sem[0], lb)
