"""Forward + backward of DepthNet_Fusion's plane-sweep cost volume (DepthNet_Fusion.correlation) with autograd: the fused
HIP form (sgc_plane_sweep_corr + sgc_plane_sweep_corr_backward) against the reference formulation
(SGC_PLANE_SWEEP_FUSED_GRAD=0: homo_warping + grid_sample + product, per neighbour), in alternated runs of one process.
Reports per shape and form: forward / backward ms (device events, median and spread over --reps), the peak memory the
two passes add, and the neighbour-role list lengths (median / max entries per destination row).  The time of each
stage of the fused backward (count / scan / fill / final / long) comes from a separate run of this script under
`rocprofv3 --kernel-trace --stats` (--reps 3 --forms fused)."""
import argparse, json, os, sys, types
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sgcdet_amd.plugin  # noqa: F401,E402
from sgcdet_amd.plugin.depth_net import DepthNet_Fusion  # noqa: E402
from sgcdet_amd.plugin.plane_sweep import closest_frame_ids, relative_projections  # noqa: E402
from sgcdet_amd.scene import make_img_meta  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="40,100", help="view counts (128 ch, 60x80, 12 planes, 2 neighbours)")
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--forms", default="fused,reference")
ap.add_argument("--out", default=None, help="JSON file for the results")
args = ap.parse_args()
C, H, W, K, STRIDE = 128, 60, 80, 2, 4
dbound = (0.2, 5.0, 0.4)


def list_lengths(meta, N, depth):
    """Entries per destination row of the neighbour-role list (on-image corners landing there), from the forward's
    position arithmetic restated in torch float32 (statistics only)."""
    w2c = torch.tensor(np.array(meta["lidar2img"]["extrinsic"]), dtype=torch.float32)
    intr = torch.tensor(np.array(meta["lidar2img"]["intrinsic"]), dtype=torch.float32).clone()
    intr[:2] /= meta["ori_shape"][0] / (meta["img_shape"][0] / STRIDE)
    nbr = closest_frame_ids(N, K)
    rel = relative_projections(w2c, intr, nbr).cuda()
    y, x = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32), torch.arange(W, device="cuda", dtype=torch.float32), indexing="ij")
    xyz = torch.stack([x.reshape(-1), y.reshape(-1), torch.ones(H * W, device="cuda")])
    cnt = torch.zeros(N * H * W, dtype=torch.int64, device="cuda")
    dv = torch.tensor(depth, device="cuda")
    for k in range(K):
        r = rel[:, k]
        p = (r[:, :, :3] @ xyz).unsqueeze(2) * dv.view(1, 1, -1, 1) + r[:, :, 3].view(N, 3, 1, 1)
        u, v = p[:, 0] / p[:, 2], p[:, 1] / p[:, 2]
        ix = ((u / ((W - 1) / 2) - 1 + 1) * W - 1) / 2
        iy = ((v / ((H - 1) / 2) - 1 + 1) * H - 1) / 2
        inside = (ix > -1) & (iy > -1) & (ix < W) & (iy < H)
        x0, y0 = torch.floor(ix).long(), torch.floor(iy).long()
        m = nbr[:, k].cuda().view(N, 1, 1)
        for dx in (0, 1):
            for dy in (0, 1):
                xx, yy = x0 + dx, y0 + dy
                ok = inside & (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
                dst = (m * H * W + yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1))[ok]
                cnt += torch.bincount(dst, minlength=N * H * W)
    c = cnt.float()
    return dict(entries=int(cnt.sum()), median=float(c.median()), mean=float(c.mean()), max=int(cnt.max()),
                rows_over_512=int((cnt > 512).sum()))


results = []
for N in [int(s) for s in args.shapes.split(",")]:
    meta = make_img_meta(N, "scannet", 0)
    net = types.SimpleNamespace(neighbor_img_num=K, depth_channels=round((dbound[1] - dbound[0]) / dbound[2]),
                                depth_values=np.arange(*dbound, dtype=np.float32) + dbound[2] / 2)
    D = net.depth_channels
    gen = torch.Generator().manual_seed(N)
    f0 = torch.randn(N, C, H, W, generator=gen).cuda()
    g = torch.randn(N, D, H, W, generator=gen).cuda()
    forms = args.forms.split(",")
    rec = {f: dict(fwd=[], bwd=[], peak=[]) for f in forms}
    grads = {}
    for rep in range(args.reps + 1):                 # rep 0 warms up every form
        for form in forms:
            os.environ["SGC_PLANE_SWEEP_FUSED_GRAD"] = "1" if form == "fused" else "0"
            f = f0.clone().requires_grad_(True)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            corr = DepthNet_Fusion.correlation(net, f, meta, STRIDE)
            e[1].record()
            corr.backward(g)
            e[2].record()
            torch.cuda.synchronize()
            if rep:
                rec[form]["fwd"].append(e[0].elapsed_time(e[1]))
                rec[form]["bwd"].append(e[1].elapsed_time(e[2]))
                rec[form]["peak"].append((torch.cuda.max_memory_allocated() - base) / 2 ** 20)
            else:
                grads[form] = f.grad.detach()
            del corr, f
    row = dict(N=N, C=C, H=H, W=W, D=D, K=K, warped_tensor_MiB=N * C * D * H * W * 4 / 2 ** 20,
               lists=list_lengths(meta, N, net.depth_values))
    for form in forms:
        r = rec[form]
        tot = [a + b for a, b in zip(r["fwd"], r["bwd"])]
        row[form] = dict(fwd_ms=float(np.median(r["fwd"])), bwd_ms=float(np.median(r["bwd"])), total_ms=float(np.median(tot)),
                         total_ms_min=float(np.min(tot)), total_ms_max=float(np.max(tot)), peak_MiB=float(np.max(r["peak"])))
    if len(grads) == 2:
        a, b = grads["fused"].double(), grads["reference"].double()
        row["grad_max_rel_diff"] = float((a - b).abs().max() / b.abs().max())
    results.append(row)
    print(json.dumps(row), flush=True)
if args.out:
    with open(args.out, "w") as fh:
        json.dump(dict(tool="tools/plane_sweep_grad_bench.py", reps=args.reps, results=results), fh, indent=1)
