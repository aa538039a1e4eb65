"""DepthNet_Fusion in train mode at config-2 geometry: forward + backward with the feature extractors on the HIP kernels against the
torch formulation (SGC_DEPTH_NET_TRAIN_HIP=0, the parent's), and the stem's weight gradient alone.

    python tools/depth_net_train_bench.py --out profiles/r18_depth_net_train_bench.json

ONE process alternates the two formulations in blocks of `--steps` training steps (the switch is read at every forward), `--blocks`
blocks each after a warm-up block of each, on two copies of one module; a step is zero_grad + forward + a loss on the output +
backward, timed by the host clock around a block that ends in a device synchronise.  Reported: every block's ms per step and the
median per formulation.  `--views 40`: xs [1, 40, 256, 60, 80] channels-last (what plugin/fpn.py hands over, requiring a gradient),
images 240 x 320.

The stem part times `sgc_conv2d_stem7_wgrad_bf16x3` at N = views, 240 x 320 with device events over `--kernel-iters` launches, the
same for `torch.nn.grad.conv2d_weight` on NCHW tensors, and the fraction of the traffic floor (dy + image once, at the measured
copy rate of 6.29 TB/s) the kernel reaches."""
import argparse
import copy
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 6.29e12      # bytes / s, the measured device copy rate


def module_ab(args):
    import torch
    import sgcdet_amd.plugin as P
    from sgcdet_amd.scene import make_scene
    torch.manual_seed(0)
    nets = {"1": P.DepthNet_Fusion(neighbor_img_num=2, downsample_factor=4, dbound=[0.2, 5.0, 0.4], mono_channels=256,
                                   init_weight="none").train().cuda()}
    nets["0"] = copy.deepcopy(nets["1"])
    feats, _, meta = make_scene(args.views, 256, kind="scannet", seed=1)           # the ScanNet config: 239 x 320 padded to 240 x 320
    assert tuple(feats[0].shape[-2:]) == (60, 80)
    xs = feats[0].cuda()[0].contiguous(memory_format=torch.channels_last).unsqueeze(0).requires_grad_(True)
    imgs = torch.randn(1, args.views, 3, 240, 320).cuda()
    weight = None

    def block(v, steps):
        nonlocal weight
        os.environ["SGC_DEPTH_NET_TRAIN_HIP"] = v
        net = nets[v]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            net.zero_grad(set_to_none=True)
            xs.grad = None
            pred = net(xs, imgs, [meta], 4)
            if weight is None:
                weight = torch.linspace(-1, 1, pred.numel(), device=pred.device).view_as(pred)
            (pred * weight).sum().backward()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps
    for v in ("0", "1"):
        block(v, args.warmup)
    runs = {"0": [], "1": []}
    for b in range(args.blocks):
        for v in ("0", "1"):
            runs[v].append(block(v, args.steps))
            print(f"block {b} SGC_DEPTH_NET_TRAIN_HIP={v}: {runs[v][-1]:.2f} ms / step", flush=True)
    return dict(what="DepthNet_Fusion train-mode forward + backward, 240x320 images, 60x80 maps, 256 mono channels, D = 12",
                views=args.views, steps_per_block=args.steps, torch_formulation_ms=runs["0"], hip_extractors_ms=runs["1"],
                torch_formulation_median_ms=statistics.median(runs["0"]), hip_extractors_median_ms=statistics.median(runs["1"]))


def stem_wgrad(args):
    import torch
    from sgcdet_amd import ext
    ops = ext.ops()
    N, H, W = args.views, 240, 320
    img = torch.randn(N, 3, H, W).cuda()
    dy = torch.randn(N * (H // 2) * (W // 2), 64).cuda()
    dy_nchw = dy.view(N, H // 2, W // 2, 64).permute(0, 3, 1, 2).contiguous()

    def timed(fn):
        for _ in range(3):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.kernel_iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.kernel_iters          # us
    ours = timed(lambda: ops.conv2d_stem7_wgrad_bf16x3(img, dy))
    lib = timed(lambda: torch.nn.grad.conv2d_weight(img, (64, 3, 7, 7), dy_nchw, stride=2, padding=3))
    nbytes = dy.numel() * 4 + img.numel() * 4
    floor = nbytes / COPY_RATE * 1e6
    return dict(what="weight gradient of the 7x7 stride-2 stem", N=N, H=H, W=W, rows=dy.shape[0], hip_us=ours, torch_conv2d_weight_us=lib,
                compulsory_bytes=nbytes, floor_us=floor, fraction_of_floor=floor / ours,
                workspace_floats=ops.conv2d_stem7_wgrad_workspace_floats(N, H, W))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=40)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--kernel-iters", type=int, default=50)
    ap.add_argument("--skip-module", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = dict(stem_wgrad=stem_wgrad(a))
    print(json.dumps(out["stem_wgrad"], indent=1), flush=True)
    if not a.skip_module:
        out["module"] = module_ab(a)
    print(json.dumps(out, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
