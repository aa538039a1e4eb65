"""Two builds of the library against each other on the inter-view pooling kernels (view_pool.hip) and the volume glue
(volume_glue.hip), alternated in one process as rows_ab.py does (same box, same clocks): 5 rounds x 30 launches per line, every
round's result compared bit for bit with the first result seen, us per launch per round.  The first round is the clock ramp; a
line is flagged when this build's median over rounds 2-5 exceeds the other build's largest round 2-5.
python tools/view_pool_ab.py tools/diag/libsgc_prev.so   -- the argument is the OTHER library (e.g. the previous commit's build)."""
import os, statistics, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sgcdet_amd._abi import Library
from sgcdet_amd.tensor_api import TensorOps
from sgcdet_amd import ext
from sgcdet_amd.scene import make_img_meta
from sgcdet_amd.plugin.voxformer import compute_projection
libs = {"this": ext.ops(), "other": TensorOps(Library(os.path.join(ROOT, sys.argv[1])), "cuda")}
ROUNDS, LAUNCHES = 5, 30
flagged = []
def knobs(**kv):
    for ops in libs.values():
        for k, v in kv.items():
            ops.lib.call("sgc_set_tuning", k.encode(), v)
def timed(fn, n=LAUNCHES):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn(); e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3
def line(name, call, result=None):
    """call(ops) -> tensor or tuple of tensors, timed; `result(ops)`: what to compare where `call` works in place on a scratch buffer."""
    t = {nm: [] for nm in libs}
    want = None
    for rnd in range(ROUNDS):
        for nm, ops in libs.items():
            t[nm].append(timed(lambda: call(ops)))
            y = (result or call)(ops)
            y = y if isinstance(y, tuple) else (y,)
            want = tuple(v.clone() for v in y) if want is None else want
            assert all(torch.equal(a, b) for a, b in zip(y, want)), (name, nm, rnd)
    med, worst = statistics.median(t["this"][1:]), max(t["other"][1:])
    if med > worst: flagged.append(name)
    fmt = lambda v: " ".join(f"{x:6.1f}" for x in v)
    print(f"{name:44s} this {fmt(t['this'])} | other {fmt(t['other'])} | median {med:6.1f} vs max {worst:6.1f} {'SLOWER' if med > worst else 'ok'}", flush=True)
def rand(*shape, s=1.0): return torch.randn(*shape, device="cuda") * s
torch.manual_seed(0)

# the pair lists of config 2 (C = 256) and config 5 (C = 128), binned as the path bins them; 8 heads
for name, N, C, grid, vox, topk in [("cfg2", 40, 256, (40, 40, 16), (.16, .16, .2), 6400), ("cfg5", 100, 128, (96, 96, 32), (.08, .08, .1), 73728)]:
    ops = libs["this"]
    H, W = 60, 80
    meta = make_img_meta(N, "scannet", 0)
    proj = compute_projection(meta).float().cuda().contiguous()
    origin = torch.tensor(meta["lidar2img"]["origin"]).cuda()
    g = torch.Generator().manual_seed(0)
    nx, ny, nz = grid
    idx = torch.randperm(nx * ny * nz, generator=g)[:topk].sort().values
    xs = torch.stack([idx // (ny * nz), (idx // nz) % ny, idx % nz], 1).float()
    ref3d = (xs * torch.tensor(vox) - torch.tensor([nx, ny, nz]) / 2 * torch.tensor(vox)).cuda().contiguous()
    ref_cam, mask = ops.project_points(ref3d, origin, proj, 320, H * 4, 0.2, 5.0)
    pc = ops.bin_pairs(ref_cam, ops.compact_pairs(mask), H, W, 16, 22)
    n_pairs, n_valid = int(pc["totals"][0]), int(pc["totals"][1])
    slot, vi = pc["slot"], pc["valid_index"]
    tag = f"{name} {n_valid} voxels {n_pairs} pairs"
    feat, q, kv = rand(n_pairs, C), rand(n_valid, C), rand(n_pairs, 2 * C)
    for group, depth in ((1, 4), (1, 1), (0, 4)):
        knobs(view_group=group, view_depth=depth)
        line(f"view_mean   g{group} d{depth} {tag}", lambda o: o.view_mean(feat, slot, vi, n_valid))
        line(f"view_attend g{group} d{depth} {tag}", lambda o: o.view_attend(q, kv, slot, vi, 8))
    qp = rand(n_valid, 8 * C, s=C ** -0.5)
    for depth in (1, 2, 4, 8):
        knobs(view_group=1, view_depth=depth)
        line(f"view_attend_pq   d{depth} {tag}", lambda o: o.view_attend_pq(qp, feat, slot, vi, 8))
    knobs(view_group=1, view_depth=4)                   # the defaults
    ctx, gctx = ops.view_attend(q, kv, slot, vi, 8), rand(n_valid, C)
    line(f"view_attend_backward  {tag}", lambda o: o.view_attend_backward(q, kv, slot, vi, 8, ctx, gctx))
    del feat, q, kv, qp, ctx, gctx

# the glue at config 2's sizes (bench.py) and the larger shapes of tests/test_gpu_kernels.py
rows, vol = rand(6400, 256), torch.zeros(25600, 256, device="cuda")
idx32 = torch.randperm(25600, device="cuda")[:6400].sort().values.to(torch.int32)
line("scatter_rows 6400 x 256 -> 25600", lambda o: o.scatter_rows(rows, idx32, vol))
src = rand(5, 256, 64, 80)
line("nchw_to_nhwc 5 x 256 x 64 x 80 (64 tile)", lambda o: o.nchw_to_nhwc_crop(src, 64, 80))
src12 = rand(3, 12, 60, 80)
line("nchw_to_nhwc 3 x 12 x 60 x 80 crop 59 (32 tile)", lambda o: o.nchw_to_nhwc_crop(src12, 59, 80))
nhwc = rand(5, 64 * 80, 256)
line("nhwc_to_nchw 5 x 256 x 64 x 80", lambda o: o.nhwc_to_nchw_pad(nhwc, 64, 80))
coarse, w, b = rand(20 * 20 * 8, 256), rand(256, s=0.1), rand(1)
line("upsample2x_occ 20 x 20 x 8, C 256", lambda o: o.upsample2x_occ(coarse, (20, 20, 8), w, b)[:2])
go = rand(1, 256, 40, 40, 16)
line("upsample2x_backward 256 x 20 x 20 x 8", lambda o: o.upsample2x_backward(go))
base, scratch, idx64 = rand(25600, 256), torch.zeros(25600, 256, device="cuda"), idx32.long()
line("scatter_add_rows 6400 x 256 -> 25600", lambda o: o.scatter_add_rows(rows, idx64, scratch), result=lambda o: o.scatter_add_rows(rows, idx64, base.clone()))
print("slower than the other build: " + (", ".join(flagged) if flagged else "none"), flush=True)
