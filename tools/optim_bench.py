"""The parameter update alone on a BASELINE workload's real parameter list (synthetic gradients): us and effective TB/s of the two
optimiser kernels (csrc/optim.hip) against clip_grad_norm_ + torch.optim.AdamW with foreach and with fused=True, alternated in one
process, medians over blocks.  Algorithmic bytes: 4 B per element for the norm (the gradient once), 28 B for the update (four fp32
arrays in, three out).  --sweep also times the fused update at several elements-per-workgroup settings."""
import argparse, json, os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sgcdet_amd.plugin  # noqa: F401
from sgcdet_amd import ext
from sgcdet_amd.mmcv_lite import build_detector
from sgcdet_amd.optim import FusedAdamW, reference_param_groups
from sgcdet_amd.scene import model_config, workload

ap = argparse.ArgumentParser()
ap.add_argument("--workload", default="cfg2_scannet")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--iters", type=int, default=20, help="steps per timed block")
ap.add_argument("--sweep", action="store_true")
ap.add_argument("--json", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("optim_bench needs a GPU: a CPU timing says nothing about the MI355X")

torch.manual_seed(0)
det = build_detector(model_config(workload(args.workload))).cuda().train()
params = [p for p in det.parameters() if p.requires_grad]
gen = torch.Generator(device="cuda").manual_seed(1)
for p in params:
    p.grad = torch.randn(p.shape, generator=gen, device="cuda") * 0.01
numel = sum(p.numel() for p in params)
groups = lambda: reference_param_groups(det, 2e-4, 1e-4)      # noqa: E731


def timed(fn):
    torch.cuda.synchronize(); t = time.perf_counter()
    for _ in range(args.iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / args.iters * 1e6


def torch_step(opt):
    def f():
        torch.nn.utils.clip_grad_norm_(params, 35.0)
        opt.step()
    return f


variants = {}
for be in ([4096, 8192, 16384, 32768] if args.sweep else [None]):
    o = FusedAdamW(groups(), max_grad_norm=35.0, block_elems=be)
    variants[f"fused{'' if be is None else '_be' + str(be)}"] = o.step
variants["fused_noclip"] = FusedAdamW(groups(), max_grad_norm=None).step
variants["torch_foreach"] = torch_step(torch.optim.AdamW(groups(), foreach=True))
variants["torch_fused"] = torch_step(torch.optim.AdamW(groups(), fused=True))
for f in variants.values():                                  # state, staging buffers, code objects
    f(); f()
times = {k: [] for k in variants}
for _ in range(args.rounds):                                 # alternated: every variant once per round
    for k, f in variants.items():
        times[k].append(timed(f))
med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}

# device time of the library's kernels alone (events around each entry point; the host is out of the figure)
ops = ext.ops()
kern = {}
o = FusedAdamW(groups(), max_grad_norm=35.0)
o.step(); o.step()
ops.event_log, ops.event_names = [], {"sgc_grad_sqnorm_batch", "sgc_adamw_step_batch"}
for _ in range(30):
    o.step()
torch.cuda.synchronize()
for name, _, e0, e1 in ops.event_log:
    kern.setdefault(name, []).append(e0.elapsed_time(e1) * 1e3)
ops.event_log = None
kmed = {k: sorted(v)[len(v) // 2] for k, v in kern.items()}
out = dict(workload=args.workload, device=torch.cuda.get_device_name(0), tensors=len(params), elements=numel,
           block_elems=ops.OPTIM_BLOCK_ELEMS, wall_us_per_update=dict((k, round(v, 1)) for k, v in med.items()),
           wall_us_min=dict((k, round(min(v), 1)) for k, v in times.items()),
           kernel_us=dict((k, round(v, 1)) for k, v in kmed.items()),
           kernel_TBps=dict(sgc_grad_sqnorm_batch=round(4 * numel / kmed["sgc_grad_sqnorm_batch"] / 1e6, 3),
                            sgc_adamw_step_batch=round(28 * numel / kmed["sgc_adamw_step_batch"] / 1e6, 3)),
           faster_torch_variant=min(("torch_foreach", "torch_fused"), key=lambda k: med[k]),
           note="wall = host clock around iters updates ending in a synchronise; kernel = HIP events around one entry point "
                "(sgc_grad_sqnorm_batch is two launches)")
print(json.dumps(out))
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
