"""DepthNet_Fusion eval forward at config-2 geometry: the HIP path against the library-convolution path (SGC_DEPTH_NET_HIP=0).

    python tools/depth_net_bench.py --out profiles/r10_depth_net_bench.json     # driver: alternates =0 / =1, 4 repeats each,
                                                                                # one fresh process per run, stops at the first failure
    python tools/depth_net_bench.py --one                                        # one run in this process (what the driver starts;
                                                                                # also the program to put behind `rocprofv3 --kernel-trace --stats --`)

    python tools/depth_net_bench.py --parity profiles/r10_depth_net_parity.json # the figures the module tests' bounds come from

Times are host clocks around forwards that end in a device synchronise, after warm-up; ms per scene.  The `--one` run of the HIP
variant also reports device-event time and TFLOP/s per entry point from the event log: 2 * MAC of the shapes AS LAUNCHED, i.e. with the
channel padding of the plan (2.6 % above the module's own count over the whole net).  `--xs-layout` is the memory format
of the finest FPN map both legs receive: nhwc (what plugin/fpn.py produces, the default) or nchw."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def one(args):
    import torch
    import sgcdet_amd.plugin as P
    from sgcdet_amd import ext
    from sgcdet_amd.scene import make_scene
    torch.manual_seed(0)
    net = P.DepthNet_Fusion(neighbor_img_num=2, downsample_factor=4, dbound=[0.2, 5.0, 0.4], mono_channels=256,
                            init_weight="none").eval().cuda()
    feats, _, meta = make_scene(args.views, 256, kind="scannet", seed=1, img_hw=(256, 320))
    xs = feats[0].cuda()
    if args.xs_layout == "nhwc":                # what plugin/fpn.py hands over; BOTH legs get the same input
        xs = xs[0].contiguous(memory_format=torch.channels_last).unsqueeze(0)
    imgs = torch.randn(1, args.views, 3, 256, 320).cuda()
    with torch.no_grad():
        for _ in range(args.warmup):
            net(xs, imgs, [meta], 4)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            net(xs, imgs, [meta], 4)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / args.steps
    res = dict(hip=os.environ.get("SGC_DEPTH_NET_HIP", "1") != "0", views=args.views, xs_layout=args.xs_layout, ms_per_scene=ms)
    if res["hip"]:
        ops = ext.ops()
        ops.event_log = []
        with torch.no_grad():
            net(xs, imgs, [meta], 4)
        torch.cuda.synchronize()
        groups = {}
        for name, m, e0, e1 in ops.event_log:
            g = groups.setdefault(name, dict(ms=0.0, gflop=0.0, calls=0))
            g["ms"] += e0.elapsed_time(e1)
            g["calls"] += 1
            if "Cin" in m:
                rows = m["V"] if m.get("transposed") else m["OV"]
                g["gflop"] += 2.0 * rows * m["taps"] * m["Cin"] * m["Cout"] / 1e9
        ops.event_log = None
        for g in groups.values():
            g["tflops"] = g["gflop"] / g["ms"] if g["ms"] > 0 else 0.0
        res["entry_points"] = groups
    print("RESULT " + json.dumps(res))


def parity(args):
    """max |difference| of the HIP path and of the torch path against the reference's golden, and of the two against each other at
    config-2 geometry, on the fixtures of tests/test_gpu_depth_net_hip.py."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import test_gpu_depth_net_hip as t
    from golden_util import max_err, img_meta

    def both(net, xs, imgs, metas, stride):
        res = []
        with torch.no_grad():
            for v in ("1", "0"):
                os.environ["SGC_DEPTH_NET_HIP"] = v
                res.append(net(xs, imgs, metas, stride))
        return res
    net, d, stride = t._golden_net()
    hip, tor = both(net, d["xs"].cuda(), d["imgs"].cuda(), [img_meta(d)], stride)
    out = dict(golden_size=dict(hip_vs_golden=max_err(hip, d["pred"]), torch_vs_golden=max_err(tor, d["pred"]),
                                hip_vs_torch=max_err(hip, tor),
                                hip_channels_last=bool(hip[0].is_contiguous(memory_format=torch.channels_last))))
    net, feats, imgs, meta = t._full_res()
    hip, tor = both(net, feats[0].cuda(), imgs.cuda(), [meta], 4)
    out["config2_geometry_6_views"] = dict(hip_vs_torch=max_err(hip, tor), pred_max=float(tor.max()))
    print(json.dumps(out, indent=1))
    with open(args.parity, "w") as f:
        json.dump(out, f, indent=1)


def driver(args):
    runs = {"0": [], "1": []}
    detail = None
    for rep in range(args.repeats):
        for v in ("0", "1"):
            env = dict(os.environ, SGC_DEPTH_NET_HIP=v)
            r = subprocess.run(["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--one",
                                "--views", str(args.views), "--steps", str(args.steps), "--warmup", str(args.warmup),
                                "--xs-layout", args.xs_layout],
                               env=env, capture_output=True, text=True)
            if r.returncode != 0:
                print(r.stdout[-2000:], r.stderr[-4000:])
                raise SystemExit(f"run SGC_DEPTH_NET_HIP={v} failed with status {r.returncode}: stopping")
            line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
            res = json.loads(line[7:])
            runs[v].append(res["ms_per_scene"])
            if v == "1":
                detail = res.get("entry_points")
            print(f"rep {rep} SGC_DEPTH_NET_HIP={v}: {res['ms_per_scene']:.2f} ms / scene", flush=True)
    out = dict(what="DepthNet_Fusion eval forward, 256x320 images, 64x80 maps, 256 mono channels, D = 12", views=args.views, xs_layout=args.xs_layout,
               library_convolutions_ms=runs["0"], hip_ms=runs["1"],
               library_convolutions_median_ms=statistics.median(runs["0"]), hip_median_ms=statistics.median(runs["1"]),
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
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--timeout", type=int, default=180)
    ap.add_argument("--xs-layout", choices=("nhwc", "nchw"), default="nhwc")
    ap.add_argument("--parity", default=None, metavar="OUT")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    parity(a) if a.parity else one(a) if a.one else driver(a)
