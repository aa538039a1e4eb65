"""DepthNet_Fusion in train mode at config-2 geometry: forward + backward in three formulations -- torch throughout
(SGC_DEPTH_NET_TRAIN_HIP=0), the feature extractors on the HIP kernels (SGC_DEPTH_NET_TRAIN_HIP=1, the default), and the U-Nets,
depth_reg and the softmax on them as well (SGC_DEPTH_NET_TRAIN_UNETS=1) -- and three kernels alone: the stem's weight gradient, the
padded live BatchNorm and the softmax backward.

    python tools/depth_net_train_bench.py --out profiles/r22_depth_unets_train_bench.json

ONE process alternates the formulations in blocks of `--steps` training steps (the switches are read at every forward), `--blocks`
blocks each after a warm-up block of each, on copies of one module; a step is zero_grad + forward + a loss on the output +
backward, timed by the host clock around a block that ends in a device synchronise.  Reported: every block's ms per step and the
median per formulation.  `--views 40`: xs [1, 40, 256, 60, 80] channels-last (what plugin/fpn.py hands over, requiring a gradient),
images 240 x 320.

The stem part times `sgc_conv2d_stem7_wgrad_bf16x3` at N = views, 240 x 320 with device events over `--kernel-iters` launches, the
same for `torch.nn.grad.conv2d_weight` on NCHW tensors, and the fraction of the traffic floor (dy + image once, at the measured
copy rate of 6.29 TB/s) the kernel reaches.  The U-Net part does the same for `sgc_bn_rows_padded_forward / _backward` (tail 2, the
U-Net skip) and `sgc_softmax_rows_backward` at the finest map's views x 60 x 80 rows, against the bytes each must move."""
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
    arms = {"torch": ("0", "0"), "extractors": ("1", "0"), "unets": ("1", "1")}       # SGC_DEPTH_NET_TRAIN_HIP, SGC_DEPTH_NET_TRAIN_UNETS
    nets = {"torch": P.DepthNet_Fusion(neighbor_img_num=2, downsample_factor=4, dbound=[0.2, 5.0, 0.4], mono_channels=256,
                                       init_weight="none").train().cuda()}
    for v in ("extractors", "unets"):
        nets[v] = copy.deepcopy(nets["torch"])
    feats, _, meta = make_scene(args.views, 256, kind="scannet", seed=1)           # the ScanNet config: 239 x 320 padded to 240 x 320
    assert tuple(feats[0].shape[-2:]) == (60, 80)
    xs = feats[0].cuda()[0].contiguous(memory_format=torch.channels_last).unsqueeze(0).requires_grad_(True)
    imgs = torch.randn(1, args.views, 3, 240, 320).cuda()
    weight = None

    def block(v, steps):
        nonlocal weight
        os.environ["SGC_DEPTH_NET_TRAIN_HIP"], os.environ["SGC_DEPTH_NET_TRAIN_UNETS"] = arms[v]
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
    for v in arms:
        block(v, args.warmup)
    runs = {v: [] for v in arms}
    for b in range(args.blocks):
        for v in arms:
            runs[v].append(block(v, args.steps))
            print(f"block {b} {v} (TRAIN_HIP={arms[v][0]} TRAIN_UNETS={arms[v][1]}): {runs[v][-1]:.2f} ms / step", flush=True)
    assert nets["unets"]._train_unets_ok(), "the third arm did not take the U-Net path"
    return dict(what="DepthNet_Fusion train-mode forward + backward, 240x320 images, 60x80 maps, 256 mono channels, D = 12",
                views=args.views, steps_per_block=args.steps, torch_formulation_ms=runs["torch"], hip_extractors_ms=runs["extractors"],
                hip_extractors_and_unets_ms=runs["unets"], torch_formulation_median_ms=statistics.median(runs["torch"]),
                hip_extractors_median_ms=statistics.median(runs["extractors"]),
                hip_extractors_and_unets_median_ms=statistics.median(runs["unets"]))


def _timed(fn, iters):
    import torch
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters          # us


def unets_kernels(args):
    """The two new kernel families alone, at the rows of the finest map, against the bytes they must move at the copy rate."""
    import torch
    from sgcdet_amd import ext
    ops = ext.ops()
    rows = args.views * 60 * 80
    out = dict(rows=rows, copy_rate_bytes_per_s=COPY_RATE, padded_norm=[], softmax_backward=None)
    for C, ld in ((12, 32), (128, 128), (140, 160)):
        x, res, dy = (torch.randn(rows, ld).cuda() for _ in range(3))
        w, b = torch.rand(C).cuda() + 0.5, torch.randn(C).cuda()
        _, mean, invstd = ops.bn_rows_padded_forward(x, w, b, residual=res, tail=2)
        fwd = _timed(lambda: ops.bn_rows_padded_forward(x, w, b, residual=res, tail=2), args.kernel_iters)
        bwd = _timed(lambda: ops.bn_rows_padded_backward(x, dy, mean, invstd, w, bias=b, tail=2, want_dresidual=True), args.kernel_iters)
        fb = rows * (2 * C + C + ld) * 4           # x twice (statistics, apply), the residual, y at full pitch
        bb = rows * (4 * C + 2 * ld) * 4           # x and dy twice (sums, apply), dx and dresidual at full pitch
        out["padded_norm"].append(dict(C=C, ld=ld, tail=2, forward_us=fwd, forward_bytes=fb, forward_floor_us=fb / COPY_RATE * 1e6,
                                       forward_fraction_of_floor=fb / COPY_RATE * 1e6 / fwd, backward_us=bwd, backward_bytes=bb,
                                       backward_floor_us=bb / COPY_RATE * 1e6, backward_fraction_of_floor=bb / COPY_RATE * 1e6 / bwd))
    C, ldg = 12, 32
    p, dp = torch.softmax(torch.randn(rows, C).cuda(), 1), torch.randn(rows, C).cuda()
    us = _timed(lambda: ops.softmax_rows_backward(p, dp, C=C, ldg=ldg), args.kernel_iters)
    nb = rows * (2 * C + ldg) * 4
    out["softmax_backward"] = dict(C=C, ldg=ldg, us=us, bytes=nb, floor_us=nb / COPY_RATE * 1e6, fraction_of_floor=nb / COPY_RATE * 1e6 / us)
    return out


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
    out = dict(stem_wgrad=stem_wgrad(a), unets_kernels=unets_kernels(a))
    print(json.dumps(out["stem_wgrad"], indent=1), flush=True)
    print(json.dumps(out["unets_kernels"], indent=1), flush=True)
    if not a.skip_module:
        out["module"] = module_ab(a)
    print(json.dumps(out, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
