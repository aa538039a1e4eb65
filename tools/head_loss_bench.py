"""Forward + backward of the detection head's loss alone (``ImVoxelHeadV2._loss_single``: get_points, target assignment, the three
losses and the gradients of the head tensors; the head convolutions excluded) at config-2 head sizes -- 29 200 points on three scales,
18 / 17 classes, 30 seeded boxes -- for both heads: the fused operator (``functions.HeadLossFunction``, csrc/head_loss.hip) against the
torch path (``SGC_HEAD_LOSS_FUSED=0``), alternated in one process.  Per head: ``--pairs`` pairs of ``--iters`` iterations after a
warm-up, ms per iteration of every block (host clock around a block that ends in a device synchronise), medians and spread, and the
device kernels / copies of one iteration of each path from the profiler (a run of its own, not timed)."""
import argparse, json, os, statistics, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sgcdet_amd.plugin  # noqa: F401,E402
from sgcdet_amd.mmcv_lite import HEADS  # noqa: E402
from head_loss_contract import GRIDS, head_tensors  # noqa: E402
from targets_contract import random_boxes  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=5)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--out", default=None, help="also write the JSON result to this file")
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("head_loss_bench needs a GPU: a timing taken anywhere else says nothing")


def activity(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    dev = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    copies = [n for n in dev if "emcpy" in n or "Copy" in n]
    return dict(kernels=len([n for n in dev if n not in copies and "emset" not in n]), copies=len(copies),
                device_to_host=len([c for c in copies if "DtoH" in c or "Device -> Host" in c]))


result = dict(points=sum(x * y * z for x, y, z in GRIDS), boxes=30, pairs=args.pairs, iters=args.iters, heads={})
for kind, n_classes, n_reg in (("ScanNetImVoxelHeadV2", 18, 6), ("SunRgbdImVoxelHeadV2", 17, 7)):
    rotated = n_reg == 7
    head = HEADS.build(dict(type=kind, n_classes=n_classes, n_channels=32, n_reg_outs=n_reg, n_scales=3, limit=27, centerness_topk=18)).cuda()
    head.voxel_size = [0.16, 0.16, 0.2]
    meta = dict(lidar2img=dict(origin=[0.0, 0.0, 0.5]))
    ctr, reg, cls, val = head_tensors(rotated, 5)
    leaves = [t.cuda().requires_grad_(True) for t in ctr + reg + cls]
    ctr, reg, cls = leaves[:3], leaves[3:6], leaves[6:]
    vals = [v.cuda() for v in val]
    boxes, labels = random_boxes(30, 4, rotated)
    boxes, labels = boxes.cuda(), (labels % n_classes).cuda()
    ups = [torch.ones((), device="cuda") for _ in range(3)]

    def one(fused):
        os.environ["SGC_HEAD_LOSS_FUSED"] = "1" if fused else "0"
        lc, lb, ls, _, _ = head._loss_single(ctr, reg, cls, vals, meta, boxes, labels)
        return [lc, lb, ls], torch.autograd.grad([lc, lb, ls], leaves, ups, allow_unused=True)

    def block(fused):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            one(fused)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.iters

    for fused in (True, False):
        for _ in range(args.warmup):
            one(fused)
    lf, lt = one(True)[0], one(False)[0]
    ms = dict(fused=[], torch=[])
    for _ in range(args.pairs):
        ms["fused"].append(block(True))
        ms["torch"].append(block(False))
    stat = lambda v: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), blocks_ms=v)   # noqa: E731
    result["heads"][kind] = dict(fused=stat(ms["fused"]), torch=stat(ms["torch"]),
                                 speedup_of_medians=statistics.median(ms["torch"]) / statistics.median(ms["fused"]),
                                 fused_below_torch_in_every_pair=all(a < b for a, b in zip(ms["fused"], ms["torch"])),
                                 losses_fused=[float(x) for x in lf], losses_torch=[float(x) for x in lt],
                                 device_activity_per_iteration=dict(fused=activity(lambda: one(True)), torch=activity(lambda: one(False))))
os.environ.pop("SGC_HEAD_LOSS_FUSED", None)
line = json.dumps(result)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
