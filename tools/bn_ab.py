"""Two builds of the library against each other on the BatchNorm entries (batch_norm.hip), in one process (same box, same clocks).
1. Bits: every output of the six sgc_bn_rows_* entries -- y, mean, invstd, running mean, running var, dx, dweight, dbias, dresidual --
   compared with torch.equal between the builds: the padded entries over ROWS x WIDTHS x TAILS of tests/test_gpu_depth_unets_train.py
   (inputs from bn_padded_conditioned), the dense entries on the same cases compacted to [rows, C] with tails 0 / 1 and on (6, 4) and
   (77, 1040) of tests/buffer_cases.py.  Any difference ends the run with status 1.
2. Speed: the builds alternated, 5 rounds x 30 launches per line, us per launch per round, on preallocated buffers (the entry alone):
   the dense forward and backward, plain and relu(bn + residual), at the neck's layer shapes of config 2
   (profiles/r04_neck_layers.txt), and the padded ones at tail 2 at the U-Net shapes tools/depth_net_train_bench.py times.  The first
   round is the clock ramp; a line is flagged when this build's median over rounds 2-5 exceeds the other build's largest round 2-5.
python tools/bn_ab.py tools/diag/libsgc_prev.so   -- the argument is the OTHER library (e.g. the previous commit's build)."""
import os, statistics, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from sgcdet_amd._abi import Library
from sgcdet_amd.tensor_api import TensorOps
from sgcdet_amd import ext
import nonfinite_contract as nf
from buffer_cases_depth_train import bn_padded_conditioned
from test_gpu_depth_unets_train import ROWS, WIDTHS, TAILS, _padded_step, _dense_step
libs = {"this": ext.ops(), "other": TensorOps(Library(os.path.join(ROOT, sys.argv[1]), train=True), "cuda")}
ROUNDS, LAUNCHES = 5, 30

# ---- 1. bits -------------------------------------------------------------------------------------------------------------------------
different, compared = [], 0
def same(case, run):
    """run(ops) -> dict of outputs; every one of this build's must equal the other build's."""
    global compared
    a, b = run(libs["this"]), run(libs["other"])
    assert a.keys() == b.keys(), case
    for name in a:
        if a[name] is None and b[name] is None:
            continue
        compared += 1
        if not torch.equal(a[name], b[name]):
            different.append(f"{case}: {name}")
for rows in ROWS:
    for C, ld in WIDTHS:
        for tail, with_res in TAILS:
            i, _ = bn_padded_conditioned(rows, C, ld, tail, with_res)
            case = f"{rows} x {C} in {ld}, tail {tail}{' + residual' if with_res else ''}"
            same("padded " + case, lambda o: _padded_step(o, i))
            if tail != 2:
                same("dense  " + case, lambda o: _dense_step(o, i))
for rows, C in ((6, 4), (77, 1040)):
    for tail in (False, True):
        d = nf.bn_inputs(rows, C, "nan", None)
        same(f"dense  {rows} x {C} {'residual + relu' if tail else 'plain'}", lambda o: nf.bn_run(o, d, tail, "cuda"))
print(f"bits: {compared} outputs compared, different: " + ("; ".join(different) if different else "none"), flush=True)
if different:
    sys.exit(1)

# ---- 2. speed ------------------------------------------------------------------------------------------------------------------------
flagged = []
def timed(fn, n=LAUNCHES):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn(); e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3
def line(name, call):
    t = {nm: [] for nm in libs}
    for rnd in range(ROUNDS):
        for nm, ops in libs.items():
            t[nm].append(timed(lambda: call(ops)))
    med, worst = statistics.median(t["this"][1:]), max(t["other"][1:])
    if med > worst: flagged.append(name)
    fmt = lambda v: " ".join(f"{x:6.1f}" for x in v)
    print(f"{name:44s} this {fmt(t['this'])} | other {fmt(t['other'])} | median {med:6.1f} vs max {worst:6.1f} {'SLOWER' if med > worst else 'ok'}", flush=True)
def rand(*shape): return torch.randn(*shape, device="cuda")
torch.manual_seed(0)
def buffers(rows, C, ld):
    x, dy, res, y, dx, dres = (rand(rows, ld) for _ in range(6))
    w, b, rm, rv = torch.rand(C, device="cuda") + 0.5, rand(C), rand(C), torch.rand(C, device="cuda") + 0.5
    mean, invstd, dw, db = (torch.empty(C, device="cuda") for _ in range(4))
    ws = torch.empty(max(4, int(libs["this"].lib._dll.sgc_bn_rows_workspace_floats(rows, C))), device="cuda")
    return x, dy, res, y, dx, dres, w, b, rm, rv, mean, invstd, dw, db, ws
for rows, C in ((25600, 256), (25600, 128), (3200, 512), (400, 1024)):       # norms behind the neck's convolutions, config 2
    x, dy, res, y, dx, dres, w, b, rm, rv, mean, invstd, dw, db, ws = buffers(rows, C, C)
    n = ws.numel()
    line(f"dense forward  {rows} x {C} plain", lambda o: o._call("sgc_bn_rows_forward", x, w, b, rm, rv, 0.1, 1e-5, y, mean, invstd, ws, n, rows, C))
    line(f"dense backward {rows} x {C} plain", lambda o: o._call("sgc_bn_rows_backward", x, dy, mean, invstd, w, dx, dw, db, ws, n, rows, C))
    line(f"dense forward  {rows} x {C} relu(bn + res)",
         lambda o: o._call("sgc_bn_rows_act_forward", x, w, b, rm, rv, 0.1, 1e-5, res, 1, y, mean, invstd, ws, n, rows, C))
    line(f"dense backward {rows} x {C} relu(bn + res)",
         lambda o: o._call("sgc_bn_rows_act_backward", x, dy, y, mean, invstd, w, dx, dw, db, dres, ws, n, rows, C))
for rows, C, ld in ((40 * 60 * 80, 12, 32), (40 * 60 * 80, 128, 128), (40 * 60 * 80, 140, 160)):      # the U-Nets' finest map, 40 views
    x, dy, res, y, dx, dres, w, b, rm, rv, mean, invstd, dw, db, ws = buffers(rows, C, ld)
    n = ws.numel()
    line(f"padded forward  {rows} x {C} in {ld} tail 2",
         lambda o: o._call("sgc_bn_rows_padded_forward", x, w, b, rm, rv, 0.1, 1e-5, res, 2, y, mean, invstd, ws, n, rows, C, ld))
    line(f"padded backward {rows} x {C} in {ld} tail 2",
         lambda o: o._call("sgc_bn_rows_padded_backward", x, dy, None, mean, invstd, w, b, dx, dw, db, dres, 2, ws, n, rows, C, ld))
print("slower than the other build: " + (", ".join(flagged) if flagged else "none"), flush=True)
