"""GPU tests of the fused detection-head loss (csrc/head_loss.hip, ``functions.HeadLossFunction``).

The yardstick is never the fused code: it is the torch path of ``ImVoxelHeadV2._loss_single`` (tests/head_loss_contract.py) on the CPU
in float64 (R64) and float32 (R32), with targets from the oracle's ``assign_targets``.  Bound per loss and per gradient tensor
(max-abs): ``|H - R64| <= 4 |R32 - R64| + floor``, floor = 1e-7 for a loss and 1e-7 * max|R64| for a gradient.  Every measured pair
is printed before it is asserted; ``SGC_HEAD_LOSS_RECORD_DIR=<dir>`` also writes them as ``r09_head_loss_parity.json`` (the copy under
profiles/ was made that way)."""
import json
import os

import pytest
import torch

from head_loss_contract import (GRIDS, N_CLASSES, bound_rows, degeneracy_margin, golden_boxes, golden_points, head_tensors, torch_path,
                                torch_path_grads)

pytestmark = pytest.mark.gpu

UPSTREAM = (0.7, 1.3, 2.1)
_RECORD = {}


def _record(key, rows):
    d = os.environ.get("SGC_HEAD_LOSS_RECORD_DIR")
    _RECORD[key] = rows
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "r09_head_loss_parity.json"), "w") as f:
            json.dump(dict(bound="|H - R64| <= 4 |R32 - R64| + floor (1e-7 for a loss, 1e-7 max|R64| for a gradient tensor)",
                           upstream=UPSTREAM, cases=_RECORD), f, indent=1, sort_keys=True)
            f.write("\n")


def _names(n_scales):
    return [f"grad {t}[{l}]" for t in ("centerness", "bbox_pred", "cls_score") for l in range(n_scales)]


def _targets(oracle_ops, rotated, case):
    pts, scales, (n_scales, limit, topk) = golden_points()
    boxes, gl = golden_boxes(rotated, case)
    ct, bt, lb, _ = oracle_ops.assign_targets(pts, scales, boxes, gl, rotated, n_scales, limit, topk)
    return pts, ct, bt, lb


def _fused(rotated, ctr, reg, cls, val, pts, ct, bt, lb, upstream=UPSTREAM, n_pos_override=None, loss_weights=(1.0, 1.0, 1.0)):
    from sgcdet_amd.functions import HeadLossFunction
    leaves = [t.cuda().requires_grad_(True) for t in ctr + reg + cls]
    cfg = dict(rotated=rotated, gamma=2.0, alpha=0.25, loss_weights=loss_weights)
    losses = HeadLossFunction.apply(pts.cuda(), ct.cuda(), bt.cuda(), lb.cuda(), n_pos_override, cfg, *leaves, *[v.cuda() for v in val])
    grads = torch.autograd.grad(losses, leaves, [torch.tensor(u, device="cuda") for u in upstream])
    return losses, grads


# ---- 1. operator parity, both heads ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [0, 1, 2])
@pytest.mark.parametrize("rotated", [False, True])
def test_operator_parity_with_the_torch_path(oracle_ops, rotated, case):
    pts, ct, bt, lb = _targets(oracle_ops, rotated, case)
    ctr, reg, cls, val = head_tensors(rotated, 100 + 10 * case + int(rotated))
    v = torch.cat([x.reshape(-1) for x in val])
    pos = (lb >= 0) & v
    assert int(pos.sum()) >= 1 and int((~v).sum()) > 0.25 * len(v)                # (the single box of set 1 keeps 3 valid positives)
    if rotated:                                              # no exactly degenerate pair (R64, on the CPU) before relying on gradients
        flat = torch.cat([r.permute(1, 2, 3, 0).reshape(-1, 7) for r in reg])
        margin = degeneracy_margin(pts, flat, bt, pos)
        print(f"rotated case {case}: {int(pos.sum())} positives, smallest corner-to-edge side value {margin:.3e}")
        assert margin > 1e-9
    out = {}
    for dtype in (torch.float64, torch.float32):
        losses, leaves = torch_path(rotated, ctr, reg, cls, val, pts, ct, bt, lb, dtype)
        out[dtype] = ([l.detach() for l in losses], torch_path_grads(losses, leaves, UPSTREAM))
    h_losses, h_grads = _fused(rotated, ctr, reg, cls, val, pts, ct, bt, lb)
    what = f"{'rotated' if rotated else 'axis-aligned'} head, box set {case}"
    rows = bound_rows(what, ["loss_centerness", "loss_bbox", "loss_cls"], h_losses, out[torch.float32][0], out[torch.float64][0], None)
    rows += bound_rows(what, _names(len(GRIDS)), h_grads, out[torch.float32][1], out[torch.float64][1], 1.0)
    _record(what, rows)
    assert all(float(l) > 0 for l in out[torch.float64][0])
    assert sum(float(g.abs().max()) > 0 for g in out[torch.float64][1]) >= 5       # cls on every scale, centerness and boxes where positives are
    bad = [r for r in rows if not r["ok"]]
    assert not bad, bad


# ---- 2. bitwise reproducibility -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rotated", [False, True])
def test_five_calls_are_bitwise_equal(oracle_ops, rotated):
    pts, ct, bt, lb = _targets(oracle_ops, rotated, 0)
    ctr, reg, cls, val = head_tensors(rotated, 7)
    runs = [_fused(rotated, ctr, reg, cls, val, pts, ct, bt, lb) for _ in range(5)]
    bits = lambda t: t.detach().contiguous().view(torch.int32)
    for losses, grads in runs[1:]:
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(losses, runs[0][0]))
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(grads, runs[0][1]))


# ---- 3. launches and synchronisation --------------------------------------------------------------------------------------------
def _device_activity(prof):
    dev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    copies = [e.name for e in dev if "emcpy" in e.name or "Copy" in e.name]
    kernels = [e.name for e in dev if e.name not in copies and "emset" not in e.name]
    host = {e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CPU}
    return kernels, copies, host


@pytest.mark.parametrize("rotated", [False, True])
def test_forward_and_backward_are_at_most_four_kernels_and_no_host_synchronisation(oracle_ops, rotated):
    from torch.profiler import ProfilerActivity, profile
    from sgcdet_amd.functions import HeadLossFunction
    pts, ct, bt, lb = (t.cuda() for t in _targets(oracle_ops, rotated, 0))
    ctr, reg, cls, val = head_tensors(rotated, 11)
    leaves = [t.cuda().requires_grad_(True) for t in ctr + reg + cls]
    vals = [v.cuda() for v in val]
    ups = [torch.tensor(u, device="cuda") for u in UPSTREAM]
    cfg = dict(rotated=rotated, gamma=2.0, alpha=0.25, loss_weights=(1.0, 1.0, 1.0))

    def fused():
        losses = HeadLossFunction.apply(pts, ct, bt, lb, None, cfg, *leaves, *vals)
        return torch.autograd.grad(losses, leaves, ups)
    fused()                                                    # code objects loaded, allocator warm
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                    # a synchronising torch call inside raises
    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fused()
            torch.cuda.set_sync_debug_mode("default")
            torch.cuda.synchronize()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    kernels, copies, host = _device_activity(prof)
    print("fused forward + backward, device activity:", kernels, copies)
    assert kernels and all("head_loss_" in k for k in kernels), kernels                       # only this feature's kernels
    assert len(kernels) == (4 if rotated else 3)
    assert not copies, copies
    assert not (host - {"hipDeviceSynchronize"}) & {"hipStreamSynchronize", "hipEventSynchronize", "hipMemcpy", "hipMemcpyDtoH",
                                                   "hipMemcpyWithStream", "hipMemcpyAsync"}, host

    # the same section through the torch path on the GPU: the "before" figure, printed and not asserted
    def torch_side():
        losses, lv = torch_path(rotated, ctr, reg, cls, val, pts, ct, bt, lb, torch.float32, device="cuda")
        return torch.autograd.grad(losses, lv, ups, allow_unused=True)
    torch_side()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        torch_side()
        torch.cuda.synchronize()
    t_kernels, t_copies, _ = _device_activity(prof)
    d2h = [c for c in t_copies if "DtoH" in c or "Device -> Host" in c]
    print(f"torch path forward + backward ({'rotated' if rotated else 'axis-aligned'}): {len(t_kernels)} kernels, {len(t_copies)} copies "
          f"({len(d2h)} device-to-host); fused: {len(kernels)} kernels, 0 copies")


# ---- 4. edge cases --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rotated", [False, True])
def test_empty_cases_are_decided_on_the_device(oracle_ops, rotated):
    pts, ct, bt, lb = _targets(oracle_ops, rotated, 0)
    ctr, reg, cls, val = head_tensors(rotated, 21)
    # no valid point: all three losses and every gradient exactly 0
    losses, grads = _fused(rotated, ctr, reg, cls, [torch.zeros_like(v) for v in val], pts, ct, bt, lb)
    assert all(float(l) == 0.0 for l in losses) and all(int(torch.count_nonzero(g)) == 0 for g in grads)
    # valid points but no positive: cls > 0, the other two and their gradients exactly 0
    losses, grads = _fused(rotated, ctr, reg, cls, val, pts, ct, bt, torch.full_like(lb, -1))
    L = len(GRIDS)
    assert float(losses[2]) > 0 and float(losses[0]) == 0.0 and float(losses[1]) == 0.0
    assert all(int(torch.count_nonzero(g)) == 0 for g in grads[:2 * L]) and all(float(g.abs().max()) > 0 for g in grads[2 * L:])
    want, _ = torch_path(rotated, ctr, reg, cls, val, pts, ct, bt, torch.full_like(lb, -1), torch.float64)
    assert abs(float(losses[2]) - float(want[2])) <= 1e-6 * float(want[2])
    # positives whose weights are all 0: bbox loss and its gradients 0, centerness still trained
    losses, grads = _fused(rotated, ctr, reg, cls, val, pts, torch.zeros_like(ct), bt, lb)
    assert float(losses[1]) == 0.0 and float(losses[0]) > 0 and all(int(torch.count_nonzero(g)) == 0 for g in grads[L:2 * L])


@pytest.mark.parametrize("rotated", [False, True])
def test_logits_of_100_keep_the_clamp_semantics(oracle_ops, rotated):
    pts, ct, bt, lb = _targets(oracle_ops, rotated, 0)
    ctr, reg, cls, val = head_tensors(rotated, 31)
    g = torch.Generator().manual_seed(5)
    big = lambda t: torch.where(torch.rand(t.shape, generator=g) < 0.5, torch.full_like(t, 100.0), torch.full_like(t, -100.0))
    ctr, cls = [big(t) for t in ctr], [big(t) for t in cls]
    losses, grads = _fused(rotated, ctr, reg, cls, val, pts, ct, bt, lb)
    want, _ = torch_path(rotated, ctr, reg, cls, val, pts, ct, bt, lb, torch.float32)
    for k in (0, 2):
        print(f"logits +-100: loss {k}: fused {float(losses[k]):.9g}, float32 torch path {float(want[k]):.9g}")
        assert abs(float(losses[k]) - float(want[k])) <= 1e-6 * abs(float(want[k]))
    assert float(want[2]) > 10.0                                                    # log(FLT_MIN) terms are in the sum
    assert all(bool(torch.isfinite(x).all()) for x in grads) and all(bool(torch.isfinite(l)) for l in losses)


def _one_pair(gpu_ops, pred, target):
    """1 - loss_bbox of ONE positive point at the origin whose decoded box is ``pred`` (cx,cy,cz,w,l,h,a), against ``target``."""
    import math
    cx, cy, cz, w, l, h, a = pred
    # invert SunRgbdImVoxelHeadV2._bbox_pred_to_bbox at the point (0, 0, 0): shift = R(-a) centre
    sx, sy = cx * math.cos(a) + cy * math.sin(a), -cx * math.sin(a) + cy * math.cos(a)
    d = [w / 2 - sx, w / 2 + sx, l / 2 - sy, l / 2 + sy, h / 2 - cz, h / 2 + cz, a]
    reg = torch.tensor(d, dtype=torch.float32, device="cuda").view(7, 1, 1, 1)
    z = lambda c: torch.zeros(c, 1, 1, 1, device="cuda")
    losses, n_pos, state = gpu_ops.head_loss([z(1)], [reg], [z(17)], [torch.ones(1, dtype=torch.bool, device="cuda")],
                                             torch.zeros(1, 3, device="cuda"), torch.ones(1, device="cuda"),
                                             torch.tensor([target], dtype=torch.float32, device="cuda"),
                                             torch.zeros(1, dtype=torch.int64, device="cuda"), True)
    one = torch.ones(1, device="cuda")
    grads = gpu_ops.head_loss_grads(state, one, one, one)
    assert float(n_pos) == 1.0 and all(bool(torch.isfinite(g).all()) for gs in grads for g in gs)
    return 1.0 - float(losses[1])


def test_rotated_iou_of_identical_disjoint_and_nested_boxes(gpu_ops):
    box = (0.3, -0.2, 0.1, 1.6, 0.9, 1.2, 0.7)
    assert abs(_one_pair(gpu_ops, box, box) - 1.0) < 1e-5                                          # identical: IoU 1
    assert _one_pair(gpu_ops, box, (5.0, 4.0, 0.1, 1.0, 1.0, 1.0, -0.4)) == 0.0                    # disjoint: IoU 0
    inner = (0.3, -0.2, 0.1, 0.8, 0.45, 0.6, 0.7)
    assert abs(_one_pair(gpu_ops, inner, box) - 0.125) < 1e-6                                      # nested: the volume ratio
    assert abs(_one_pair(gpu_ops, box, inner) - 0.125) < 1e-6


@pytest.mark.parametrize("rotated", [False, True])
def test_n_pos_override_normalises_and_n_pos_stays_local(gpu_ops, oracle_ops, rotated):
    pts, ct, bt, lb = (t.cuda() for t in _targets(oracle_ops, rotated, 0))
    ctr, reg, cls, val = ([t.cuda() for t in ts] for ts in head_tensors(rotated, 41))
    vals = [v.reshape(-1) for v in val]
    base, n_pos, _ = gpu_ops.head_loss(ctr, reg, cls, vals, pts, ct, bt, lb, rotated)
    local = float(n_pos)
    assert local == float(((lb >= 0) & torch.cat(vals)).sum()) > 20
    over = torch.tensor([123.5], device="cuda")
    losses, n_pos2, state = gpu_ops.head_loss(ctr, reg, cls, vals, pts, ct, bt, lb, rotated, n_pos_override=over)
    assert float(n_pos2) == local
    assert abs(float(losses[0]) - float(base[0]) * local / 123.5) <= 1e-6 * float(losses[0])
    assert abs(float(losses[2]) - float(base[2]) * local / 123.5) <= 1e-6 * float(losses[2])
    assert float(losses[1]) == float(base[1])                                      # normalised by the sum of its weights, not by n_pos
    again, n_pos3 = gpu_ops.head_loss_finalize(state, torch.tensor([local], device="cuda"))           # the distributed run's second step
    assert torch.equal(again, base) and float(n_pos3) == local


def test_function_refuses_half_tensors_and_unsupported_shapes(gpu_ops, oracle_ops):
    from sgcdet_amd.functions import HeadLossFunction
    pts, ct, bt, lb = (t.cuda() for t in _targets(oracle_ops, False, 0))
    ctr, reg, cls, val = ([t.cuda() for t in ts] for ts in head_tensors(False, 3))
    cfg = dict(rotated=False)
    with pytest.raises(TypeError):
        HeadLossFunction.apply(pts, ct, bt, lb, None, cfg, *[t.half() for t in ctr + reg + cls], *val)
    with pytest.raises(RuntimeError, match="unsupported"):
        gpu_ops.head_loss(ctr, [r[:5] for r in reg], cls, [v.reshape(-1) for v in val], pts, ct, bt[:, :5].contiguous(), lb, False)
    with pytest.raises(RuntimeError, match="unsupported"):
        gpu_ops.head_loss(ctr * 2, reg * 2, cls * 2, [v.reshape(-1) for v in val] * 2, pts, ct, bt, lb, False)      # 6 scales


def test_strided_head_tensors_are_read_in_place(gpu_ops, oracle_ops):
    """The training convolutions hand the head channels-last views of their rows; the operator reads them where they lie and gives
    the same bits as for contiguous copies."""
    pts, ct, bt, lb = (t.cuda() for t in _targets(oracle_ops, False, 0))
    ctr, reg, cls, val = ([t.cuda() for t in ts] for ts in head_tensors(False, 9))
    vals = [v.reshape(-1) for v in val]
    rows = [torch.cat([c, r, s], 0).permute(1, 2, 3, 0).contiguous() for c, r, s in zip(ctr, reg, cls)]        # [X,Y,Z,25]
    full = [r.permute(3, 0, 1, 2) for r in rows]
    views = ([f[:1] for f in full], [f[1:7] for f in full], [f[7:] for f in full])
    assert not views[1][0].is_contiguous()
    a, _, sa = gpu_ops.head_loss(ctr, reg, cls, vals, pts, ct, bt, lb, False)
    b, _, sb = gpu_ops.head_loss(*views, vals, pts, ct, bt, lb, False)
    assert torch.equal(a, b) and torch.equal(sa["grads"], sb["grads"])


# ---- 5. module level ------------------------------------------------------------------------------------------------------------
def _detector(head):
    import sgcdet_amd.plugin  # noqa: F401
    from sgcdet_amd.mmcv_lite import build_detector
    from sgcdet_amd.scene import make_scene, model_config, workload
    from targets_contract import random_boxes
    w = workload("cfg1_plumbing")
    rotated = head == "SunRgbdImVoxelHeadV2"
    if rotated:
        w.update(kind="arkit", head="SunRgbdImVoxelHeadV2", n_classes=17, n_reg_outs=7)
    torch.manual_seed(23)
    det = build_detector(model_config(w)).cuda().train()
    for m in det.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    feats, dpt, meta = make_scene(3, w["embed_dims"], kind=w["kind"], seed=14, device="cuda")
    boxes, labels = random_boxes(9, 6, rotated)
    boxes[:, :3] *= 0.5 if rotated else 0.55
    return det, feats, dpt, meta, boxes.cuda(), (labels % 17 if rotated else labels).cuda(), rotated


def _with_env(value, fn):
    old = os.environ.get("SGC_HEAD_LOSS_FUSED")
    if value is None:
        os.environ.pop("SGC_HEAD_LOSS_FUSED", None)
    else:
        os.environ["SGC_HEAD_LOSS_FUSED"] = value
    try:
        return fn()
    finally:
        if old is None:
            os.environ.pop("SGC_HEAD_LOSS_FUSED", None)
        else:
            os.environ["SGC_HEAD_LOSS_FUSED"] = old


@pytest.mark.parametrize("head", ["ScanNetImVoxelHeadV2", "SunRgbdImVoxelHeadV2"])
def test_module_takes_the_fused_path_and_agrees_with_the_torch_path(monkeypatch, oracle_ops, head):
    from sgcdet_amd import ext
    det, feats, dpt, meta, boxes, labels, rotated = _detector(head)
    lib, names = ext.ops().lib, []
    real = lib.call

    def call(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setattr(lib, "call", call)
    # forward_train_from_features: the switch
    fused = _with_env(None, lambda: det.forward_train_from_features(feats, [meta], dpt, [boxes], [labels]))
    assert names.count("sgc_head_loss_forward") == 1
    del names[:]
    plain = _with_env("0", lambda: det.forward_train_from_features(feats, [meta], dpt, [boxes], [labels]))
    assert "sgc_head_loss_forward" not in names and "sgc_assign_targets" in names
    for k in ("loss_centerness", "loss_bbox", "loss_cls"):
        print(f"{head} forward_train_from_features {k}: fused {float(fused[k]):.8f} torch {float(plain[k]):.8f}")
        assert abs(float(fused[k]) - float(plain[k])) <= 2e-4 * max(1.0, abs(float(plain[k])))

    # one forward, its head tensors, both loss paths on them: losses and the head convolutions' weight gradients by the 4 x bound
    bh = det.bbox_head
    volume, valid, occ = det.build_volume_from_features(feats, [meta], dpt)
    ctr, reg, cls = bh(det.neck_3d(volume))
    weights = [bh.centerness_conv.weight, bh.reg_conv.weight, bh.cls_conv.weight]
    ups = [torch.tensor(u, device="cuda") for u in UPSTREAM]

    def run():
        d, _, _ = bh.loss(ctr, reg, cls, valid.float(), [meta], [boxes], [labels])
        ls = [d["loss_centerness"], d["loss_bbox"], d["loss_cls"]]
        return [l.detach() for l in ls], torch.autograd.grad(ls, weights, ups, retain_graph=True)
    h_losses, h_w = _with_env(None, run)
    t_losses, t_w = _with_env("0", run)
    # R64 / R32 from the head tensors of that forward, oracle targets; their gradients go through the same convolution backward
    pts = bh.get_points([c.shape[-3:] for c in ctr], meta["lidar2img"]["origin"], "cpu")
    scales = torch.cat([torch.full((len(p),), i, dtype=torch.int32) for i, p in enumerate(pts)])
    P = torch.cat(pts).float().contiguous()
    ct_t, bx_t, lb, _ = oracle_ops.assign_targets(P, scales, bh._gt_rows(boxes.cpu(), "cpu"), labels.cpu(), rotated, bh.n_scales, bh.limit,
                                                  bh.centerness_topk)
    vals = [torch.nn.Upsample(size=c.shape[-3:], mode="trilinear")(valid.float()).round().bool()[0] for c in ctr]
    heads = [c[0] for c in ctr], [r[0] for r in reg], [s[0] for s in cls]
    ref = {}
    for dtype in (torch.float64, torch.float32):
        ls, leaves = torch_path(rotated, *heads, vals, P, ct_t, bx_t, lb, dtype)
        gs = [g.float().cuda()[None] for g in torch_path_grads(ls, leaves, UPSTREAM)]
        ref[dtype] = ([l.detach() for l in ls], torch.autograd.grad(ctr + reg + cls, weights, gs, retain_graph=True))
    rows = bound_rows(f"{head} module", ["loss_centerness", "loss_bbox", "loss_cls"], h_losses, ref[torch.float32][0], ref[torch.float64][0], None)
    rows += bound_rows(f"{head} module", ["grad centerness_conv.weight", "grad reg_conv.weight", "grad cls_conv.weight"], h_w,
                       ref[torch.float32][1], ref[torch.float64][1], 1.0)
    bound_rows(f"{head} module, torch path on the GPU (not asserted)", ["loss_centerness", "loss_bbox", "loss_cls"], t_losses,
               ref[torch.float32][0], ref[torch.float64][0], None)
    _record(f"{head} module", rows)
    bad = [r for r in rows if not r["ok"]]
    assert not bad, bad


def test_other_reduction_or_loss_module_silently_takes_the_torch_path(monkeypatch):
    import sgcdet_amd.plugin  # noqa: F401
    from sgcdet_amd import ext
    from sgcdet_amd.mmcv_lite import HEADS
    from targets_contract import random_boxes
    lib, names = ext.ops().lib, []
    real = lib.call

    def call(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setattr(lib, "call", call)
    boxes, labels = random_boxes(5, 2, False)
    boxes[:, :3] *= 0.5
    meta = dict(lidar2img=dict(origin=[0.0, 0.0, 0.5]))
    g = torch.Generator().manual_seed(1)
    feats = [torch.randn(1, 32, 8 >> i, 8 >> i, 4 >> i, generator=g).cuda() for i in range(3)]
    valid = torch.ones(1, 1, 8, 8, 4, device="cuda")
    out = {}
    for tag, extra in (("default", {}), ("none", dict(loss_cls=dict(type="FocalLoss", use_sigmoid=True, reduction="none")))):
        torch.manual_seed(0)
        head = HEADS.build(dict(type="ScanNetImVoxelHeadV2", n_classes=18, n_channels=32, n_reg_outs=6, n_scales=3, limit=27,
                                centerness_topk=18, **extra)).cuda().train()
        head.voxel_size = [0.8, 0.8, 0.8]
        head.init_weights()
        ctr, reg, cls = ([t] for t in zip(*[head.forward_single(f, s) for f, s in zip(feats, head.scales)]))
        del names[:]
        out[tag] = head.loss(list(ctr[0]), list(reg[0]), list(cls[0]), valid, [meta], [boxes.cuda()], [labels.cuda()])[0]
        assert ("sgc_head_loss_forward" in names) == (tag == "default") and "sgc_assign_targets" in names, (tag, names)
    assert all(bool(torch.isfinite(v)) for d in out.values() for v in d.values())
    # the element-wise focal loss, averaged by loss(): another number than the normalised sum -- the torch path really ran
    assert float(out["none"]["loss_cls"]) != float(out["default"]["loss_cls"])
    assert float(out["none"]["loss_bbox"]) == pytest.approx(float(out["default"]["loss_bbox"]), rel=1e-5, abs=1e-6)


# ---- 6. it still trains ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head", ["ScanNetImVoxelHeadV2", "SunRgbdImVoxelHeadV2"])
def test_overfit_with_the_fused_loss_reaches_what_the_torch_loss_reaches(head):
    """``overfit_run`` of tests/test_gpu_optim.py, 300 steps with the library's optimiser: the fused loss against SGC_HEAD_LOSS_FUSED=0
    from the same weights.  Fused final loss (mean of the last 10 steps) <= 1.5 x the torch-loss run's, mAP@0.25 >= its."""
    from test_gpu_optim import overfit_run, overfit_setup
    det0, scene, n_classes = overfit_setup(head)
    lt, map_t, _ = _with_env("0", lambda: overfit_run(det0, scene, n_classes, "fused"))
    lh, map_h, _ = _with_env(None, lambda: overfit_run(det0, scene, n_classes, "fused"))
    end_t, end_h = sum(lt[-10:]) / 10, sum(lh[-10:]) / 10
    print(f"overfit {head}: torch loss {lt[0]:.4f} -> {end_t:.4f} mAP@0.25 {map_t:.3f} | fused loss {lh[0]:.4f} -> {end_h:.4f} mAP@0.25 {map_h:.3f}")
    assert abs(lt[0] - lh[0]) <= 1e-3 * abs(lt[0])
    assert end_h <= 1.5 * end_t and map_h >= map_t, (end_h, end_t, map_h, map_t)
