"""The image FPN alone in a training step at config 2 (40 views; backbone maps of 256 / 512 / 1024 / 2048 channels at 60x80, 30x40,
15x20 and 8x10, channels-last in memory as the backbone's HIP path hands them over; out_channels 256): forward + backward on the
HIP kernels (SGC_FPN_TRAIN_HIP=1) against the torch formulation on library convolutions (=0), DESIGN.md 4.13.

    python tools/fpn_bench.py --out profiles/r16_fpn_train_bench.json   # driver: alternates =0 / =1, one fresh process per run, each under
                                                                        # its own time limit, stops at the first failure
    python tools/fpn_bench.py --one                                     # one run in this process (what the driver starts)
    python tools/fpn_bench.py --whole-step --repeats 2 --out ...        # the same alternation around SGCDet.forward_train from images

A step is: begin the weight-plane step, forward, backward from cotangents on the three maps the view transformation reads (the
fourth output is unused by the path).  Maps 1 - 3 require a gradient, map 0 carries no graph (the backbone's frozen first stage).
Times are host clocks around ``--steps`` steps that end in a device synchronise, after warm-up; a process reports the median of
``--blocks`` such blocks, the driver the median and the range over its processes.  The HIP leg's last process also reports the
device-event time per entry point of one step.  Weights are seeded: timing does not depend on their values."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CHANNELS, SIZES, OUT = (256, 512, 1024, 2048), ((60, 80), (30, 40), (15, 20), (8, 10)), 256


def _timed(fn, steps):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def one(args):
    import torch
    import sgcdet_amd.plugin  # noqa: F401
    from sgcdet_amd import ext
    from sgcdet_amd.functions import train_weight_planes
    from sgcdet_amd.plugin.fpn import FPN
    torch.manual_seed(0)
    net = FPN(list(CHANNELS), OUT, 4)
    net.init_weights()
    net = net.cuda().train()
    gen = torch.Generator().manual_seed(2)
    maps = [torch.randn(args.views, c, h, w, generator=gen).cuda().contiguous(memory_format=torch.channels_last).requires_grad_(i > 0)
            for i, (c, (h, w)) in enumerate(zip(CHANNELS, SIZES))]
    cots = None

    def step():
        nonlocal cots
        net.zero_grad(set_to_none=True)
        for m in maps:
            m.grad = None
        train_weight_planes().begin_step()
        outs = net(maps)
        if cots is None:
            cots = [torch.randn_like(o) for o in outs[:3]]
        torch.autograd.backward(list(outs[:3]), cots)
    res = dict(hip=net._train_hip_ok(maps), views=args.views)
    for _ in range(args.warmup):
        step()
    blocks = [_timed(step, args.steps) for _ in range(args.blocks)]
    res["train_blocks_ms"] = blocks
    res["train_ms"] = statistics.median(blocks)
    if res["hip"]:
        ops = ext.ops()
        ops.event_log = []
        step()
        torch.cuda.synchronize()
        groups = {}
        for name, m, e0, e1 in ops.event_log:
            g = groups.setdefault(name, dict(ms=0.0, gflop=0.0, calls=0))
            g["ms"] += e0.elapsed_time(e1)
            g["calls"] += 1
            if "Cin" in m:
                g["gflop"] += 2.0 * m["OV"] * m["taps"] * m["Cin"] * m["Cout"] / 1e9
        ops.event_log = None
        for g in groups.values():
            g["tflops"] = g["gflop"] / g["ms"] if g["ms"] > 0 else 0.0
        res["entry_points"] = groups
        res["entry_points_total_ms"] = sum(g["ms"] for g in groups.values())
    print("RESULT " + json.dumps(res))


def one_whole_step(args):
    """``SGCDet.forward_train`` from images + backward at config 2 (the detector of tools/backbone_bench.py, 30 seeded boxes): the
    step the FPN sits in; only ``SGC_FPN_TRAIN_HIP`` differs between the legs."""
    import torch
    import sgcdet_amd.plugin  # noqa: F401
    from backbone_bench import BACKBONE
    from sgcdet_amd.mmcv_lite import build_detector
    from sgcdet_amd.scene import make_img_meta, model_config, workload
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from targets_contract import random_boxes
    w = workload("cfg2_scannet")
    cfg = model_config(w)
    cfg.update(backbone=BACKBONE, neck=dict(type="FPN", in_channels=list(CHANNELS), out_channels=w["embed_dims"], num_outs=4),
               depth_head=dict(type="DepthNet_Fusion", neighbor_img_num=2, downsample_factor=4, dbound=[0.2, 5, 0.4],
                               mono_channels=w["embed_dims"], loss_weight=0.5, max_tol=0, init_weight="none"))
    torch.manual_seed(0)
    det = build_detector(cfg).attach_backbone()
    gen = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for m in det.backbone.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=gen))
                m.running_mean.copy_(0.1 * torch.randn(m.running_mean.shape, generator=gen))
                m.weight.copy_(0.5 + torch.rand(m.weight.shape, generator=gen))
    det = det.cuda().train()
    meta = make_img_meta(args.views, "scannet", seed=1, img_hw=(240, 320))
    img = torch.randn(1, args.views, 3, 240, 320, generator=torch.Generator().manual_seed(2)).cuda()
    boxes, labels = random_boxes(30, 4, False)
    batch = dict(img=img, img_metas=[meta], gt_bboxes_3d=[boxes.cuda()], gt_labels_3d=[(labels % w["n_classes"]).cuda()])

    def step():
        det.zero_grad(set_to_none=True)
        sum(det.forward_train(batch).values()).backward()
    res = dict(hip=os.environ.get("SGC_FPN_TRAIN_HIP", "") != "0", views=args.views)
    for _ in range(args.warmup):
        step()
    blocks = [_timed(step, args.steps) for _ in range(args.blocks)]
    res["train_blocks_ms"] = blocks
    res["train_ms"] = statistics.median(blocks)
    print("RESULT " + json.dumps(res))


def driver(args):
    runs = {"0": [], "1": []}
    detail = total = None
    for rep in range(args.repeats):
        for v in ("0", "1"):
            env = dict(os.environ, SGC_FPN_TRAIN_HIP=v)
            r = subprocess.run(["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--one",
                                "--views", str(args.views), "--steps", str(args.steps), "--warmup", str(args.warmup),
                                "--blocks", str(args.blocks)] + (["--whole-step"] if args.whole_step else []),
                               env=env, capture_output=True, text=True)
            if r.returncode != 0:
                print(r.stdout[-2000:], r.stderr[-4000:])
                raise SystemExit(f"run SGC_FPN_TRAIN_HIP={v} failed with status {r.returncode}: stopping")
            res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
            if res["hip"] != (v == "1"):
                raise SystemExit(f"run SGC_FPN_TRAIN_HIP={v} took the other path: stopping")
            runs[v].append(res["train_ms"])
            if v == "1":
                detail, total = res.get("entry_points"), res.get("entry_points_total_ms")
            print(f"rep {rep} SGC_FPN_TRAIN_HIP={v}: train_ms {res['train_ms']:.2f} (blocks {', '.join(f'{b:.2f}' for b in res['train_blocks_ms'])})",
                  flush=True)
    what = ("SGCDet.forward_train from images + backward, ms per step: config 2, ResNet-50, 30 boxes; the legs differ in the FPN only"
            if args.whole_step else
            "image FPN alone, forward + backward, ms per step: config-2 maps (channels-last memory), cotangents on outputs 0 - 2")
    out = dict(what=what,
               views=args.views, steps=args.steps, warmup=args.warmup, blocks=args.blocks,
               library_convolutions_ms=runs["0"], hip_ms=runs["1"],
               library_convolutions_median_ms=statistics.median(runs["0"]), hip_median_ms=statistics.median(runs["1"]),
               library_convolutions_spread_ms=max(runs["0"]) - min(runs["0"]), hip_spread_ms=max(runs["1"]) - min(runs["1"]),
               hip_entry_points_last_run=detail, hip_entry_points_total_ms=total)
    print(json.dumps(out, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", action="store_true")
    ap.add_argument("--views", type=int, default=40)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=5, help="blocks of --steps steps per process; the median block is reported")
    ap.add_argument("--repeats", type=int, default=3, help="fresh processes per leg")
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--out", default=None)
    ap.add_argument("--whole-step", action="store_true", help="time SGCDet.forward_train from images + backward instead of the FPN alone")
    a = ap.parse_args()
    if a.one:
        one_whole_step(a) if a.whole_step else one(a)
    else:
        driver(a)
