"""GPU tests of ``sgcdet_amd.optim`` (csrc/optim.hip): parity of ``FusedAdamW`` with ``clip_grad_norm_`` +
``torch.optim.AdamW`` measured against torch's own fp32-vs-fp64 rounding, reproducibility, checkpoint exchange with torch, launch
count / no host synchronisation, version counters, and the overfit-to-mAP run that shows the library's gradients train the model.

Figures a run measures are printed before they are asserted; ``SGC_OPTIM_RECORD_DIR=<dir>`` additionally writes them as
``r08_optim_parity.json`` / ``r08_overfit_<head>.json`` (the copies under profiles/ were made that way)."""
import copy
import json
import os
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(128, 64, 27), (257,), (1,), (64, 33), (1024, 129), (2048, 2051)]      # the last: 4.2 M elements, 513 workgroups
UNALIGNED = 999                                                                 # + a view that starts 4 bytes past a 16-byte boundary
N_GROUP0 = 2                                                                    # tensors 0, 1 at lr 2e-5, the rest at 2e-4
SKIPPED, STEPS = 3, 50                                                          # tensor 3 has no gradient every fourth step


def _record(name, payload):
    d = os.environ.get("SGC_OPTIM_RECORD_DIR")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, name), "w") as f:
            json.dump(payload, f, indent=1, sort_keys=True)
            f.write("\n")


def _initial():
    g = torch.Generator().manual_seed(1234)
    return [(torch.rand(s, generator=g) - 0.5) * 0.5 for s in SHAPES + [(UNALIGNED,)]]       # |p| <= 0.25


def _params(init, device, dtype):
    ps = [torch.nn.Parameter(t.to(device=device, dtype=dtype)) for t in init[:-1]]
    base = torch.zeros(UNALIGNED + 5, device=device, dtype=dtype)
    view = base[1:1 + UNALIGNED]
    view.copy_(init[-1])
    ps.append(torch.nn.Parameter(view))
    if dtype == torch.float32:
        assert ps[-1].data_ptr() % 16 == 4 and ps[-1].is_contiguous()
    return ps


def _groups(ps):
    return [dict(params=ps[:N_GROUP0], lr=2e-5), dict(params=ps[N_GROUP0:], lr=2e-4)]


def _grads(step, gen, shapes):
    """Seeded fp32 gradients whose element scale is 30 on every third step (global norm ~7e4: clipped at 35) and 0.01 otherwise
    (norm ~24: not clipped); tensor SKIPPED has none every fourth step."""
    scale = 30.0 if step % 3 == 0 else 0.01
    out = [torch.randn(s, generator=gen) * scale for s in shapes]
    if step % 4 == 3:
        out[SKIPPED] = None
    return out


def _sched(opt, total=60):
    return torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=[2e-5, 2e-4], total_steps=total, pct_start=0.05)


class _TorchSide:
    """The reference's optimiser from torch parts: clip_grad_norm_ + torch.optim.AdamW(foreach=False) + OneCycleLR."""

    def __init__(self, init, device, dtype, max_norm, total=60):
        self.ps = _params(init, device, dtype)
        self.opt = torch.optim.AdamW(_groups(self.ps), weight_decay=1e-4, foreach=False)
        self.sched = _sched(self.opt, total)
        self.max_norm, self.dtype, self.device = max_norm, dtype, device
        self.norms = []

    def step(self, grads):
        for p, g in zip(self.ps, grads):
            p.grad = None if g is None else g.to(device=self.device, dtype=self.dtype, copy=True)      # clip_grad_norm_ scales it in place
        if self.max_norm is not None:
            self.norms.append(float(torch.nn.utils.clip_grad_norm_(self.ps, self.max_norm, foreach=False)))
        self.opt.step()
        self.sched.step()


class _FusedSide:
    def __init__(self, init, max_norm, total=60):
        from sgcdet_amd.optim import FusedAdamW
        self.ps = _params(init, "cuda", torch.float32)
        self.opt = FusedAdamW(_groups(self.ps), weight_decay=1e-4, max_grad_norm=max_norm)
        self.sched = _sched(self.opt, total)
        self.norms = []

    def step(self, grads, read_norm=True):
        for p, g in zip(self.ps, grads):
            p.grad = None if g is None else g.cuda()
        self.opt.step()
        self.sched.step()
        if read_norm and self.opt.max_grad_norm is not None:
            self.norms.append(float(self.opt.last_grad_norm))


def _state(side):
    out = []
    for p in side.ps:
        st = side.opt.state[p]
        out.append((p.detach().double().cpu(), st["exp_avg"].double().cpu(), st["exp_avg_sq"].double().cpu(), float(st["step"])))
    return out


def _check_bound(h, r32, r64, what):
    """max|H - R64| <= 4 max|R32 - R64| + 1e-9 per tensor for the parameter and both moments; the yardstick is torch's own fp32
    rounding against float64.  The factor 4: the kernel may contract multiply-adds and rounds sqrt / the divisions at each of the
    six operations differently from torch's CPU kernels, and both sides are few-ulp quantities."""
    rows = []
    for i, (a, b, c) in enumerate(zip(h, r32, r64)):
        assert a[3] == b[3] == c[3], (what, i, a[3], b[3], c[3])                     # step counts
        for k, name in enumerate(("param", "exp_avg", "exp_avg_sq")):
            eh, er = float((a[k] - c[k]).abs().max()), float((b[k] - c[k]).abs().max())
            rows.append(dict(tensor=i, shape=list(a[k].shape), what=name, err_hip=eh, err_torch_f32=er, ratio=eh / max(er, 1e-30),
                             ok=eh <= 4 * er + 1e-9))
    for r in rows:
        print(f"{what}: tensor {r['tensor']} {r['what']:>10s} |H-R64|={r['err_hip']:.3e} |R32-R64|={r['err_torch_f32']:.3e} ratio={r['ratio']:.2f}")
    return rows


def _run_three(max_norm, steps=STEPS):
    init = _initial()
    shapes = [tuple(t.shape) for t in init]
    r64, r32, h = _TorchSide(init, "cpu", torch.float64, max_norm), _TorchSide(init, "cpu", torch.float32, max_norm), _FusedSide(init, max_norm)
    gen = torch.Generator().manual_seed(99)
    for t in range(steps):
        grads = _grads(t, gen, shapes)
        for side in (r64, r32, h):
            side.step(grads)
    return h, r32, r64


def test_parity_with_clip_grad_norm_and_torch_adamw():
    h, r32, r64 = _run_three(35.0)
    rows = _check_bound(_state(h), _state(r32), _state(r64), "parity")
    clipped = [n > 35.0 for n in r64.norms]
    assert len(clipped) == STEPS and 12 <= sum(clipped) <= 20 and sum(not c for c in clipped) >= 25       # both regimes happen
    norm_rel = max(abs(a - b) / b for a, b in zip(h.norms, r64.norms))
    print(f"parity: last_grad_norm max relative error {norm_rel:.3e}")
    _record("r08_optim_parity.json", dict(
        scenario="50 steps, OneCycleLR(total 60, pct_start 0.05), lr 2e-5 / 2e-4, wd 1e-4, clip 35, gradient scale 30 / 0.01",
        bound="max|H - R64| <= 4 * max|R32 - R64| + 1e-9", rows=rows, grad_norm_max_rel_err=norm_rel,
        steps_clipped=sum(clipped)))
    assert norm_rel <= 1e-5
    # the skipped tensor lags, as torch's does
    assert float(h.opt.state[h.ps[SKIPPED]]["step"]) == STEPS - len([t for t in range(STEPS) if t % 4 == 3]) < STEPS
    assert float(h.opt.state[h.ps[0]]["step"]) == STEPS
    bad = [r for r in rows if not r["ok"]]
    assert not bad, bad


def test_norm_and_whole_run_are_bitwise_reproducible():
    from sgcdet_amd import ext
    ops = ext.ops()
    init = _initial()
    gen = torch.Generator().manual_seed(5)
    gs = [torch.randn(t.shape, generator=gen).cuda() for t in init[:-1]]
    base = torch.randn(UNALIGNED + 5, generator=gen).cuda()
    gs.append(base[1:1 + UNALIGNED])
    blob, n, total = ops.optim_item_list([(g, g, g, g, 0, 1, 0.1, 0.03) for g in gs])
    assert total > 512
    items = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    partials = torch.empty(ops.grad_sqnorm_workspace_floats(total), device="cuda")
    outs = [ops.grad_sqnorm_batch(items, n, total, partials, torch.empty(1, device="cuda")).clone() for _ in range(5)]
    assert all(torch.equal(o.view(torch.int32), outs[0].view(torch.int32)) for o in outs)
    want = float(torch.sqrt(sum((g.double() ** 2).sum() for g in gs)))
    assert abs(float(outs[0]) - want) <= 1e-6 * want

    def run():
        h = _FusedSide(init, 35.0)
        g = torch.Generator().manual_seed(99)
        for t in range(STEPS):
            h.step(_grads(t, g, [tuple(x.shape) for x in init]), read_norm=False)
        return [(p.detach().clone(), h.opt.state[p]["exp_avg"].clone(), h.opt.state[p]["exp_avg_sq"].clone()) for p in h.ps], \
            h.opt.last_grad_norm.clone()
    a, na = run()
    b, nb = run()
    assert torch.equal(na.view(torch.int32), nb.view(torch.int32))
    for x, y in zip(a, b):
        assert all(torch.equal(u.view(torch.int32), v.view(torch.int32)) for u, v in zip(x, y))


def _count_calls(monkeypatch):
    from sgcdet_amd import ext
    lib, names = ext.ops().lib, []
    real = lib.call

    def call(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setattr(lib, "call", call)
    return names


def test_without_max_grad_norm_the_norm_kernel_never_runs(monkeypatch):
    names = _count_calls(monkeypatch)
    h, r32, r64 = _run_three(None, steps=20)
    assert names.count("sgc_adamw_step_batch") == 20 and "sgc_grad_sqnorm_batch" not in names
    assert h.opt.last_grad_norm is None
    rows = _check_bound(_state(h), _state(r32), _state(r64), "no clip")
    assert all(r["ok"] for r in rows), [r for r in rows if not r["ok"]]


@pytest.mark.parametrize("direction", ["fused_to_torch", "torch_to_fused"])
def test_state_dict_moves_between_fused_and_torch_adamw(direction):
    """10 steps with one class, its state_dict loaded into the other class on the same parameters, 10 more steps: parity with the
    float64 run by the bound of the parity test (R32 / R64 run all 20 steps with torch)."""
    from sgcdet_amd.optim import FusedAdamW
    init = _initial()
    shapes = [tuple(t.shape) for t in init]
    r64, r32 = _TorchSide(init, "cpu", torch.float64, 35.0), _TorchSide(init, "cpu", torch.float32, 35.0)
    first = _FusedSide(init, 35.0) if direction == "fused_to_torch" else _TorchSide(init, "cuda", torch.float32, 35.0)
    gen = torch.Generator().manual_seed(99)
    for t in range(10):
        grads = _grads(t, gen, shapes)
        for side in (r64, r32, first):
            side.step(grads)
    sd = copy.deepcopy(first.opt.state_dict())
    second = _TorchSide(init, "cuda", torch.float32, 35.0) if direction == "fused_to_torch" else _FusedSide(init, 35.0)
    with torch.no_grad():
        for p, q in zip(second.ps, first.ps):
            p.copy_(q)
    second.opt.load_state_dict(sd)
    second.sched.load_state_dict(first.sched.state_dict())
    assert isinstance(second.opt, FusedAdamW) == (direction == "torch_to_fused")
    assert all(float(second.opt.state[p]["step"]) == float(first.opt.state[q]["step"]) for p, q in zip(second.ps, first.ps))
    for t in range(10, 20):
        grads = _grads(t, gen, shapes)
        for side in (r64, r32, second):
            side.step(grads)
    rows = _check_bound(_state(second), _state(r32), _state(r64), direction)
    assert all(r["ok"] for r in rows), [r for r in rows if not r["ok"]]


def test_step_is_three_kernels_one_copy_and_no_host_synchronisation(monkeypatch):
    from torch.profiler import ProfilerActivity, profile
    from sgcdet_amd.optim import FusedAdamW
    gen = torch.Generator().manual_seed(3)
    ps = [torch.nn.Parameter(torch.randn(s, generator=gen).cuda()) for s in [(64, 64, 27), (257,), (1,), (300, 129)] * 8]
    for p in ps:
        p.grad = torch.randn(p.shape, generator=gen).cuda()
    opt = FusedAdamW([dict(params=ps[:5], lr=1e-4), dict(params=ps[5:])], lr=1e-3, max_grad_norm=35.0)
    opt.step()                                             # allocates state, staging and device buffers
    opt.step()
    torch.cuda.synchronize()
    names = _count_calls(monkeypatch)
    uploads = opt.item_uploads
    torch.cuda.set_sync_debug_mode("error")                # a synchronising torch call inside step() raises
    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            opt.step()
            opt.step()
            torch.cuda.set_sync_debug_mode("default")
            torch.cuda.synchronize()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert names == ["sgc_grad_sqnorm_batch", "sgc_adamw_step_batch"] * 2          # 2 + 1 kernels per step
    assert opt.item_uploads - uploads <= 2                                          # gradient addresses unchanged: one list per step
    dev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    dev = [e for e in dev if not e.name.startswith("Optimizer.step#")]             # torch.optim's own record_function span, mirrored on the device track
    copies = [e.name for e in dev if "emcpy" in e.name or "Copy" in e.name]
    kernels = [e.name for e in dev if e.name not in copies and "emset" not in e.name]
    print("device activity of two steps:", sorted(set(kernels)), copies)
    ours = [k for k in kernels if "grad_sqnorm_partial_kernel" in k or "grad_sqnorm_final_kernel" in k or "adamw_step_batch_kernel" in k]
    assert len(ours) == 6, kernels                                                  # the profile is the real thing
    assert len(kernels) == 6, [k for k in kernels if k not in ours]                 # ... and holds no torch kernel
    assert len(copies) <= 2 and all("DtoH" not in c and "Device -> Host" not in c for c in copies), copies
    host = {e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CPU}
    step_calls = host - {"hipDeviceSynchronize"}                                    # the test's own synchronize() after the two steps
    assert not step_calls & {"hipStreamSynchronize", "hipEventSynchronize", "hipMemcpy", "hipMemcpyDtoH", "hipMemcpyWithStream"}, step_calls


def test_version_counters_move_and_weight_planes_follow_without_begin_step():
    from sgcdet_amd import ext, functions
    from sgcdet_amd.optim import FusedAdamW
    ops, planes = ext.ops(), functions.train_weight_planes()
    gen = torch.Generator().manual_seed(8)
    w = torch.nn.Parameter((torch.randn(32, 16, 3, 3, 3, generator=gen) * 0.1).cuda())
    b = torch.nn.Parameter(torch.zeros(32).cuda())
    frozen = torch.nn.Parameter(torch.ones(4).cuda())                               # no gradient: untouched, version unchanged
    planes.clear()
    try:
        hi0, lo0 = (t.clone() for t in planes.get(w, pad_rows=4))
        w.grad, b.grad = torch.randn(w.shape, generator=gen).cuda(), torch.randn(32, generator=gen).cuda()
        versions = [t._version for t in (w, b, frozen)]
        before = w.detach().clone()
        FusedAdamW([w, b, frozen], lr=1e-2).step()
        assert w._version > versions[0] and b._version > versions[1] and frozen._version == versions[2]
        assert not torch.equal(w.detach(), before) and torch.equal(frozen.detach(), torch.ones(4).cuda())
        hi, lo = planes.get(w, pad_rows=4)                                         # no begin_step in between
        want_hi, want_lo = ops.pack_conv_weight(w.detach(), pad_rows=4)
        assert torch.equal(hi.view(torch.int16), want_hi.view(torch.int16)) and torch.equal(lo.view(torch.int16), want_lo.view(torch.int16))
        assert not torch.equal(hi.view(torch.int16), hi0.view(torch.int16))
    finally:
        planes.clear()


def test_scene_graph_follows_a_fused_step():
    """The contract of test_scene_graph_follows_weight_updates with FusedAdamW as the writer: the captured graph of the old weights is
    not replayed after a step."""
    import sgcdet_amd.plugin  # noqa: F401
    from sgcdet_amd.mmcv_lite import build_detector
    from sgcdet_amd.optim import FusedAdamW
    from sgcdet_amd.scene import make_scene, model_config, workload
    w = workload("cfg1_plumbing")
    torch.manual_seed(3)
    det = build_detector(model_config(w)).eval().cuda()
    feats, dpt, meta = make_scene(4, w["embed_dims"], kind=w["kind"], seed=5, device="cuda")
    det.scene_graph = True
    params = [p for p in det.parameters() if p.requires_grad]
    opt = FusedAdamW(params, lr=5e-3, max_grad_norm=35.0)
    gen = torch.Generator().manual_seed(4)
    with torch.no_grad():
        a = {k: v.clone() for k, v in det.forward_features(feats, [meta], dpt).items() if torch.is_tensor(v)}
    for p in list(det.voxel_head.parameters())[:6] + list(det.neck_3d.parameters())[:4] + list(det.bbox_head.parameters())[:2]:
        p.grad = torch.randn(p.shape, generator=gen).cuda()
    versions = {id(p): p._version for p in params}
    opt.step()
    assert all((p._version > versions[id(p)]) == (p.grad is not None) for p in params)
    with torch.no_grad():
        b = det.forward_features(feats, [meta], dpt)
        det.scene_graph, det.use_graph = False, False
        want = det.forward_features(feats, [meta], dpt)
        torch.cuda.synchronize()
    assert not torch.equal(a["volume"], b["volume"])
    assert torch.equal(b["volume"], want["volume"]) and torch.equal(b["occ"], want["occ"])
    for x, y in zip(b["centerness"] + b["cls_score"], want["centerness"] + want["cls_score"]):
        assert torch.equal(x, y)


# ---- overfit to convergence (VERDICT.md "Next round" item 2) -------------------------------------------------------------------
OVERFIT_STEPS = 300
OVERFIT_MAX_LR = 1e-3
OVERFIT_GUARD_S = 120.0            # wall-clock guard of ONE training loop
# What the torch-side run (T) reaches at this size, measured on an MI355X (profiles/r08_overfit.json): the total loss falls to 0.3 - 0.4 %
# of its first-step value and then sits on a plateau (0.547 / 0.597 after 300 steps, 0.543 / 0.591 after 600; max_lr 1e-3 and 3e-3
# alike, repeated runs alike), and mAP@0.25 over the ground-truth classes stops at 0.75 (axis-aligned head: 3 of the 4 boxes) and
# 0.5 (rotated head) -- not at the 1.0 VERDICT.md hoped for: at 0.32 m voxels on a 20 x 20 x 8 grid the remaining boxes are never
# recovered, by T or by H, in 300, 400 or 600 steps.  The bar for T is therefore what T was measured to reach, as the issue prescribes.
T_REACHED_MAP_025 = {"ScanNetImVoxelHeadV2": 0.75, "SunRgbdImVoxelHeadV2": 0.5}


def overfit_setup(head):
    import sgcdet_amd.plugin  # noqa: F401
    from sgcdet_amd.mmcv_lite import build_detector
    from sgcdet_amd.scene import make_scene, model_config, workload
    from targets_contract import random_boxes
    w = workload("cfg1_plumbing")
    rotated = head == "SunRgbdImVoxelHeadV2"
    if rotated:
        w.update(kind="arkit", head="SunRgbdImVoxelHeadV2", n_classes=17, n_reg_outs=7)
    cfg = model_config(w)
    cfg["occ_loss"] = True
    torch.manual_seed(23)
    det = build_detector(cfg)
    for m in det.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    feats, dpt, meta = make_scene(3, w["embed_dims"], kind=w["kind"], seed=14, device="cuda")
    boxes, labels = random_boxes(4, 6, rotated)
    boxes[:, :3] *= 0.5 if rotated else 0.55                  # inside the 6.4 x 6.4 x 3.2 m plumbing volume
    if rotated:
        labels = labels % 17
    return det, (feats, dpt, meta, boxes.cuda(), labels.cuda()), w["n_classes"]


def overfit_run(det0, scene, n_classes, which, steps=OVERFIT_STEPS, max_lr=OVERFIT_MAX_LR):
    """One training loop from ``det0``'s weights: ``which`` = "fused" (build_optimizer) or "torch" (clip_grad_norm_ + torch.optim.AdamW
    + the same OneCycleLR).  Returns (total loss per step, mAP@0.25 and mAP@0.5 of the .eval() model on the training scene)."""
    from sgcdet_amd.evaluation import indoor_eval
    from sgcdet_amd.optim import build_optimizer
    feats, dpt, meta, boxes, labels = scene
    det = copy.deepcopy(det0).cuda().train()
    ocfg = dict(type="AdamW", lr=max_lr, weight_decay=1e-4)
    scfg = dict(type="OneCycleLR", max_lr=max_lr, total_steps=steps + 10, pct_start=0.05, cycle_momentum=False, anneal_strategy="cos",
                final_div_factor=1e4, interval="step", frequency=1)
    params = [p for p in det.parameters() if p.requires_grad]
    if which == "fused":
        opt, sched = build_optimizer(det, ocfg, scfg, max_grad_norm=35.0)
    else:
        opt = torch.optim.AdamW([dict(params=params, lr=max_lr, weight_decay=1e-4, name="others")])
        sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=[max_lr], total_steps=steps + 10, pct_start=0.05, cycle_momentum=False,
                                                    anneal_strategy="cos", final_div_factor=1e4)
    losses, t0 = [], time.time()
    for i in range(steps):
        opt.zero_grad(set_to_none=True)
        out = det.forward_train_from_features(feats, [meta], dpt, [boxes], [labels])
        total = sum(out.values())
        total.backward()
        if which == "torch":
            torch.nn.utils.clip_grad_norm_(params, 35.0)
        opt.step()
        sched.step()
        losses.append(total.detach())
        if i % 25 == 24:
            torch.cuda.synchronize()
            assert time.time() - t0 < OVERFIT_GUARD_S, f"{which}: {i + 1} steps took {time.time() - t0:.0f} s"
    losses = torch.stack(losses).cpu().tolist()
    det.eval()
    with torch.no_grad():
        res, = det.simple_test_from_features(feats, [meta], dpt, as_results=True)
    gts = [{"gt_num": len(boxes), "gt_boxes_upright_depth": boxes.cpu().numpy(), "class": labels.cpu().numpy()}]
    ev = indoor_eval(gts, [res], [0.25, 0.5], {i: f"c{i}" for i in range(n_classes)})
    # indoor_eval's own mAP also averages over classes that were only DETECTED; such a class has no ground truth, its recall is 0 / 0
    # and the mean is NaN whenever the head emits one low-score box of it (the rotated head runs with score_thr = 0).  The figure
    # used here is the mean of indoor_eval's per-class APs over the classes that HAVE ground truth.
    gt_classes = sorted(set(labels.cpu().tolist()))
    return losses, sum(ev[f"c{c}_AP_0.25"] for c in gt_classes) / len(gt_classes), sum(ev[f"c{c}_AP_0.50"] for c in gt_classes) / len(gt_classes)


@pytest.mark.parametrize("head", ["ScanNetImVoxelHeadV2", "SunRgbdImVoxelHeadV2"])
def test_overfit_one_scene_to_convergence(head):
    """One seeded scene, 4 ground-truth boxes, OVERFIT_STEPS steps from the same initial weights with the reference's optimiser made
    of torch parts (T, the yardstick) and with ``build_optimizer`` (H).  T must reach a total loss <= 1/10 of its first-step loss and
    the mAP@0.25 it was measured to reach at this size (T_REACHED_MAP_025: 0.75 / 0.5, not 1.0 -- see there); H must reach
    mAP@0.25 >= T's and a final loss (mean of the last 10 steps) <= 1.5 x T's.  Both models are evaluated in .eval() after the same
    number of steps (running BatchNorm statistics on both sides).  Measured: T 194.77 -> 0.547, H -> 0.548 (axis-aligned), T 151.50 ->
    0.597, H -> 0.597 (rotated), equal mAP on both heads."""
    det0, scene, n_classes = overfit_setup(head)
    lt, map_t, map50_t = overfit_run(det0, scene, n_classes, "torch")
    lh, map_h, map50_h = overfit_run(det0, scene, n_classes, "fused")
    end_t, end_h = sum(lt[-10:]) / 10, sum(lh[-10:]) / 10
    print(f"overfit {head}: T loss {lt[0]:.4f} -> {end_t:.4f} mAP@0.25 {map_t:.3f} @0.5 {map50_t:.3f} | "
          f"H loss {lh[0]:.4f} -> {end_h:.4f} mAP@0.25 {map_h:.3f} @0.5 {map50_h:.3f}")
    rec = dict(head=head, steps=OVERFIT_STEPS, max_lr=OVERFIT_MAX_LR, torch=dict(loss_every_10=lt[::10], final_loss=end_t, mAP_025=map_t, mAP_050=map50_t),
               fused=dict(loss_every_10=lh[::10], final_loss=end_h, mAP_025=map_h, mAP_050=map50_h))
    _record(f"r08_overfit_{head}.json", rec)
    assert abs(lt[0] - lh[0]) <= 1e-3 * abs(lt[0])                   # same weights, same scene
    assert end_t <= 0.1 * lt[0] and map_t >= T_REACHED_MAP_025[head], (lt[0], end_t, map_t)
    assert map_h >= map_t and end_h <= 1.5 * end_t, (map_h, map_t, end_h, end_t)
