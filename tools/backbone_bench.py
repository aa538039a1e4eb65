"""The ResNet-50 backbone at config 2 (40 views of 240x320 images): the HIP path against the torch formulation on library
convolutions (SGC_BACKBONE_HIP=0), alone and inside ``SGCDet.simple_test`` from images.

    python tools/backbone_bench.py --out profiles/r13_backbone_bench.json   # driver: alternates =0 / =1, one fresh process per run, each
                                                                            # under its own time limit, stops at the first failure
    python tools/backbone_bench.py --one                                    # one run in this process (what the driver starts; also the
                                                                            # program to put behind `rocprofv3 --kernel-trace --stats --`)

    python tools/backbone_bench.py --train --out profiles/r14_backbone_train_bench.json   # forward + backward of the backbone alone under
                                                                            # the reference freezing: SGC_BACKBONE_TRAIN_HIP=0 (the torch
                                                                            # formulation) alternated with =1

Times are host clocks around forwards that end in a device synchronise, after warm-up; ms per scene.  Only the backbone differs
between the two legs: the FPN, the depth head and everything behind them run on the HIP kernels in both.  The `--one` run of the HIP
variant also reports device-event time per entry point of the backbone from the event log (TFLOP/s from 2 * MAC of the shapes as
launched; GB/s of the pooling from its bytes read + written).  Weights are seeded (no checkpoint is needed): timing does not depend
on their values."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BACKBONE = dict(type="ResNet", depth=50, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=1,
                norm_cfg=dict(type="BN", requires_grad=False), norm_eval=True, style="pytorch", pretrained="torchvision://resnet50")


def _timed(fn, warmup, steps):
    import torch
    for _ in range(warmup):
        fn()
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
    from sgcdet_amd.mmcv_lite import build_detector
    from sgcdet_amd.scene import make_img_meta, model_config, workload
    w = workload("cfg2_scannet")
    cfg = model_config(w)
    cfg.update(backbone=BACKBONE, neck=dict(type="FPN", in_channels=[256, 512, 1024, 2048], out_channels=w["embed_dims"], num_outs=4),
               depth_head=dict(type="DepthNet_Fusion", neighbor_img_num=2, downsample_factor=4, dbound=[0.2, 5, 0.4],
                               mono_channels=w["embed_dims"], loss_weight=0.5, max_tol=0, init_weight="none"))
    torch.manual_seed(0)
    det = build_detector(cfg).attach_backbone().eval()
    gen = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for m in det.backbone.modules():                      # non-trivial BatchNorm statistics (values do not change the timing)
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=gen))
                m.running_mean.copy_(0.1 * torch.randn(m.running_mean.shape, generator=gen))
    det = det.cuda()
    meta = make_img_meta(args.views, "scannet", seed=1, img_hw=(240, 320))
    img = torch.randn(1, args.views, 3, 240, 320, generator=torch.Generator().manual_seed(2)).cuda()
    batch = dict(img=img, img_metas=[meta])
    res = dict(hip=os.environ.get("SGC_BACKBONE_HIP", "1") != "0", views=args.views)
    with torch.no_grad():
        res["backbone_ms"] = _timed(lambda: det.backbone(img[0]), args.warmup, args.steps)
        res["simple_test_ms"] = _timed(lambda: det.simple_test(batch), args.warmup, args.steps)
        maps = det.backbone(img[0])

        def behind_the_backbone():
            x = det.image_features(maps)
            return det.simple_test_from_features(x, [meta], det.depth_distribution(x, img, [meta]), as_results=True)
        res["fpn_to_boxes_ms"] = _timed(behind_the_backbone, args.warmup, args.steps)
        if res["hip"]:
            ops = ext.ops()
            ops.event_log = []
            det.backbone(img[0])
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
            pool = groups.get("sgc_maxpool2d_nhwc")
            if pool:
                h, wd = 120, 160
                pool["gbytes"] = args.views * (h * wd + (h // 2) * (wd // 2)) * 64 * 4 / 1e9
                pool["gb_per_s"] = pool["gbytes"] / (pool["ms"] * 1e-3) if pool["ms"] > 0 else 0.0
            res["entry_points"] = groups
    print("RESULT " + json.dumps(res))


def one_train(args):
    """Forward + backward of the backbone alone in training mode with the reference freezing: the median over ``--blocks`` blocks of
    ``--steps`` steps after warm-up, and for the HIP leg the device-event time per entry point of one step."""
    import torch
    import sgcdet_amd.plugin  # noqa: F401
    from sgcdet_amd import ext
    from sgcdet_amd.functions import train_weight_planes
    from sgcdet_amd.mmcv_lite import build_backbone
    torch.manual_seed(0)
    net = build_backbone(BACKBONE)
    gen = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):                 # non-trivial statistics, non-zero last norms
                m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=gen))
                m.running_mean.copy_(0.1 * torch.randn(m.running_mean.shape, generator=gen))
                m.weight.copy_(0.5 + torch.rand(m.weight.shape, generator=gen))
    net = net.cuda().train()
    img = torch.randn(args.views, 3, 240, 320, generator=torch.Generator().manual_seed(2)).cuda()
    cots = None

    def step():
        nonlocal cots
        net.zero_grad(set_to_none=True)
        train_weight_planes().begin_step()
        maps = net(img)
        if cots is None:
            cots = [torch.randn_like(m) for m in maps]
        live = [i for i, m in enumerate(maps) if m.requires_grad]          # the frozen stages' maps carry no graph
        torch.autograd.backward([maps[i] for i in live], [cots[i] for i in live])
    res = dict(hip=os.environ.get("SGC_BACKBONE_TRAIN_HIP", "1") != "0", views=args.views)
    for _ in range(args.warmup):
        step()
    blocks = [_timed(step, 0, args.steps) for _ in range(args.blocks)]
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
    print("RESULT " + json.dumps(res))


def driver(args):
    keys = ("train_ms",) if args.train else ("backbone_ms", "simple_test_ms", "fpn_to_boxes_ms")
    switch = "SGC_BACKBONE_TRAIN_HIP" if args.train else "SGC_BACKBONE_HIP"
    runs = {v: {k: [] for k in keys} for v in ("0", "1")}
    detail = None
    for rep in range(args.repeats):
        for v in ("0", "1"):
            env = dict(os.environ, **{switch: v})
            r = subprocess.run(["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--one",
                                "--views", str(args.views), "--steps", str(args.steps), "--warmup", str(args.warmup),
                                "--blocks", str(args.blocks)] + (["--train"] if args.train else []),
                               env=env, capture_output=True, text=True)
            if r.returncode != 0:
                print(r.stdout[-2000:], r.stderr[-4000:])
                raise SystemExit(f"run {switch}={v} failed with status {r.returncode}: stopping")
            res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
            for k in keys:
                runs[v][k].append(res[k])
            if v == "1":
                detail = res.get("entry_points")
            print(f"rep {rep} {switch}={v}: " + ", ".join(f"{k} {res[k]:.2f}" for k in keys), flush=True)
    what = ("ResNet-50 backbone alone, training mode with the reference freezing: forward + backward, ms per step (240x320 images)" if args.train
            else "ResNet-50 backbone alone and SGCDet.simple_test from images, config 2 (240x320 images, 40 x 40 x 16 voxels)")
    out = dict(what=what, views=args.views, steps=args.steps, warmup=args.warmup,
               library_convolutions=runs["0"], hip=runs["1"],
               library_convolutions_median={k: statistics.median(runs["0"][k]) for k in keys},
               hip_median={k: statistics.median(runs["1"][k]) for k in keys},
               hip_entry_points_last_run=detail)
    print(json.dumps(out, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", action="store_true")
    ap.add_argument("--views", type=int, default=40)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--out", default=None)
    ap.add_argument("--train", action="store_true", help="forward + backward in training mode; the switch is SGC_BACKBONE_TRAIN_HIP")
    ap.add_argument("--blocks", type=int, default=5, help="--train: blocks of --steps steps; the median block is reported")
    a = ap.parse_args()
    if a.one:
        one_train(a) if a.train else one(a)
    else:
        driver(a)
