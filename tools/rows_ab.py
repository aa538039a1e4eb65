"""Two builds of the library against each other on the weight-stationary row kernels (rows_gemm.hip, level_tail.hip,
rows_blockdiag.hip), alternated in one process (same box, same clocks): 5 rounds x 30 launches per line, every round's result
compared bit for bit with the first, us per launch per round.  The first round is the clock ramp; a line is flagged when this
build's median over rounds 2-5 exceeds the other build's largest round 2-5.
python tools/rows_ab.py tools/diag/libsgc_prev.so   -- the argument is the OTHER library (e.g. the previous commit's build)."""
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
def line(name, call, want=None):
    """call(ops) -> tensor.  `want`: a result both builds must equal (else: the first result seen)."""
    t = {nm: [] for nm in libs}
    for rnd in range(ROUNDS):
        for nm, ops in libs.items():
            t[nm].append(timed(lambda: call(ops)))
            y = call(ops)
            want = y.clone() if want is None else want
            assert torch.equal(y, want), (name, nm, rnd)
    med, worst = statistics.median(t["this"][1:]), max(t["other"][1:])
    if med > worst: flagged.append(name)
    fmt = lambda v: " ".join(f"{x:6.1f}" for x in v)
    print(f"{name:44s} this {fmt(t['this'])} | other {fmt(t['other'])} | median {med:6.1f} vs max {worst:6.1f} {'SLOWER' if med > worst else 'ok'}", flush=True)
def rand(*shape, s=1.0): return torch.randn(*shape, device="cuda") * s
torch.manual_seed(0)
split = libs["this"].split_bf16

# plain Linear, row-major and head-major, over the loop forms and CU shares
x = rand(204800, 256); hi, lo = split(rand(1, 256, 256, s=0.1)); b = rand(256)
for depth in (1, 2):
    for pct in (100, 50):
        knobs(rows_depth=depth, rows_cu_pct=pct)
        line(f"linear 204800x256->256 depth {depth} cu {pct}", lambda o: o.linear_rows_bf16x3(x, hi, lo, b))
        line(f"  head-major 40x5120x8   depth {depth} cu {pct}", lambda o: o.linear_rows_headmajor_bf16x3(x, hi, lo, b, 40, 5120, 8))
knobs(rows_depth=1, rows_cu_pct=100)
x = rand(73600, 128); hi, lo = split(rand(1, 128, 128, s=0.1)); b = rand(128)
line("linear 73600x128->128", lambda o: o.linear_rows_bf16x3(x, hi, lo, b))
x = rand(6400, 256); hi, lo = split(rand(1, 512, 256, s=0.1)); b = rand(512); sc = torch.rand(512, device="cuda") + 0.5; res = rand(6400, 512)
line("residual 6400x256->512 relu(y + r)", lambda o: o.conv3d_cl_bf16x3(x, hi, lo, (6400, 1, 1), 1, 1, False, sc, b, res, 1)[0])

# sgc_pairs_geometry_linear_bf16x3 on the finest-level shapes of config 2 (C = 256) and config 5 (C = 128), against sample + Linear
for name, N, C, grid, vox, topk in [("cfg2", 40, 256, (40, 40, 16), (.16, .16, .2), 6400), ("cfg5", 100, 128, (96, 96, 32), (.08, .08, .1), 73728)]:
    ops = libs["this"]
    H, W, D = 60, 80, 12
    meta = make_img_meta(N, "scannet", 0)
    proj = compute_projection(meta).float().cuda().contiguous()
    origin = torch.tensor(meta["lidar2img"]["origin"]).cuda()
    g = torch.Generator().manual_seed(0)
    nx, ny, nz = grid
    idx = torch.randperm(nx * ny * nz, generator=g)[:topk].sort().values
    xs = torch.stack([idx // (ny * nz), (idx // nz) % ny, idx % nz], 1).float()
    ref3d = (xs * torch.tensor(vox) - torch.tensor([nx, ny, nz]) / 2 * torch.tensor(vox)).cuda().contiguous()
    ref_cam, mask = ops.project_points(ref3d, origin, proj, 320, H * 4, 0.2, 5.0)
    pc = ops.compact_pairs(mask)
    pc = ops.bin_pairs(ref_cam, pc, H, W, 16, 22)
    n = int(pc["totals"][0])
    feat = rand(N, H * W, C)
    dist = rand(N, H * W, D, s=2.0).softmax(-1).contiguous()
    hi, lo = split(rand(1, 128, C, s=0.1))
    two = ops.linear_rows_bf16x3(ops.pairs_geometry_sample(feat, dist, ref_cam, pc["pair_cam"], pc["pair_q"], n, H, W), hi, lo)
    line(f"geometry + linear {name}: {n} pairs, C {C}",
         lambda o: o.pairs_geometry_linear(feat, dist, ref_cam, pc["pair_cam"], pc["pair_q"], n, H, W, hi, lo), want=two)
    del feat, dist, two

for Nq, C in ((6400, 256), (73728, 128)):
    vis = torch.rand(Nq, device="cuda") < 0.9
    row_of = torch.full((Nq,), -1, dtype=torch.int32, device="cuda")
    row_of[vis] = torch.arange(int(vis.sum()), dtype=torch.int32, device="cuda")
    ctx = rand(int(vis.sum()), C)
    so, s1, s2 = split(rand(1, C, C, s=0.08)), split(rand(1, 2 * C, C, s=0.08)), split(rand(1, C, 2 * C, s=0.06))
    bo, b1, b2 = rand(C, s=0.1), rand(2 * C, s=0.1), rand(C, s=0.1)
    ln1, ln2 = (torch.rand(C, device="cuda") + 0.5, rand(C, s=0.1), 1e-5), (torch.rand(C, device="cuda") + 0.5, rand(C, s=0.1), 1e-5)
    line(f"level tail {Nq} x {C}", lambda o: o.level_tail(ctx, row_of, so, bo, ln1, s1, b1, s2, b2, ln2))

for rows, K in ((73600, 128), (6400, 256)):
    x = rand(rows, 8 * K); hi, lo = split(rand(8, K // 8, K, s=K ** -0.5)); b = rand(K, s=0.1)
    line(f"blockdiag {rows} x 8 x {K}", lambda o: o.linear_rows_blockdiag(x, hi, lo, b))
print("slower than the other build: " + (", ".join(flagged) if flagged else "none"), flush=True)
