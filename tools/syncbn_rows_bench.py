"""The 3-D neck converted to SyncBatchNorm, forward + backward at the config-2 grid (40 x 40 x 16, 256 -> 128), ONE rank, no process
group: ``SGC_SYNCBN_ROWS_HIP`` off (``dist._SyncBatchNormFn`` on the NCDHW view: the behaviour of the parent commit, the baseline)
against on (``functions.SyncBatchNormRowsFunction``: the sgc_bn_rows_sync_* kernels with the fused tail), alternated block by block
inside one process.

Warm-up of both settings first; then ``--rounds`` rounds, each one block of ``--steps`` steps per setting in alternating order; device
events around every block, a synchronise behind it.  Reported per setting: ms per step of the median block, the fastest and the slowest
block (the spread), and the launches of one step under the torch profiler in a separate pass (device kernels, memcpy / memset).  Both
settings are first compared on the same seeded input: outputs and gradients must agree to 1e-4 of their scale, or the timing is not
taken.  Needs a GPU; there is no CPU fall-back.  No collective runs: this says nothing about a multi-GPU step.

    python tools/syncbn_rows_bench.py [--rounds 8] [--steps 10] [--scenes 1] [--out profiles/r26_syncbn_rows_bench.json]
"""
import argparse
import copy
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--scenes", type=int, default=1)
    ap.add_argument("--grid", type=int, nargs=3, default=(40, 40, 16))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("syncbn_rows_bench: needs a GPU (a timing on the CPU says nothing)")
    from sgcdet_amd import dist as sd
    from sgcdet_amd.plugin import conv_plan
    from sgcdet_amd.plugin.neck3d import FastIndoorImVoxelNeck

    torch.manual_seed(0)
    base = sd.convert_sync_batchnorm(FastIndoorImVoxelNeck(in_channels=256, n_blocks=[1, 1, 1], out_channels=128)).cuda().train()
    necks = {False: copy.deepcopy(base), True: copy.deepcopy(base)}
    x = torch.randn(args.scenes, 256, *args.grid, device="cuda")

    def step(flag, keep=False):
        conv_plan.SYNCBN_ROWS_HIP = flag
        neck = necks[flag]
        for p in neck.parameters():
            p.grad = None
        inp = x.clone().requires_grad_(True)
        feats = neck(inp)
        sum((f ** 2).mean() for f in feats).backward()
        return ([f.detach() for f in feats], inp.grad, [p.grad for p in neck.parameters()]) if keep else None

    # 1. the two settings compute the same thing (section 6 of the measuring guide): outputs, input and parameter gradients
    a, b = step(False, True), step(True, True)
    worst = 0.0
    for u, v in list(zip(a[0], b[0])) + [(a[1], b[1])] + list(zip(a[2], b[2])):
        worst = max(worst, float((u - v).abs().max()) / max(1.0, float(u.abs().max())))
    if not worst < 1e-4:
        raise SystemExit(f"syncbn_rows_bench: the settings differ by {worst:.3e} of the scale; no timing taken")

    # 2. launches of one step per setting, in a pass of its own (tracing slows the host)
    from torch.profiler import ProfilerActivity, profile
    launches = {}
    for flag in (False, True):
        step(flag)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            step(flag)
            torch.cuda.synchronize()
        dev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        copies = [e for e in dev if "emcpy" in e.name or "Copy" in e.name or "emset" in e.name]
        kernels = [e for e in dev if e not in copies]
        launches[flag] = dict(kernels=len(kernels), bn_sync_kernels=sum("bn_" in e.name for e in kernels), memcpy_memset=len(copies))

    # ... and of ONE norm with the ResBlock tail, relu(bn(rows) + identity), per pass: the layer-level count behind the step's
    V, Cl = args.grid[0] * args.grid[1] * args.grid[2], 256
    rows, res, dy = (torch.randn(args.scenes * V, Cl, device="cuda") for _ in range(3))
    bn = sd.SyncBatchNorm3d(Cl).cuda().train()
    per_pass = {}
    for flag in (False, True):
        conv_plan.SYNCBN_ROWS_HIP = flag
        counts = {}
        for timed in (False, True):
            r = rows.clone().requires_grad_(True)
            bn.weight.grad = bn.bias.grad = None               # no accumulation kernels of a second backward in the count
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as pf:
                y = conv_plan.bn_rows(bn, r, tuple(args.grid), residual=res, relu=True)
                torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as pb:
                y.backward(dy)
                torch.cuda.synchronize()
            for name, prof in (("forward", pf), ("backward", pb)):
                counts[name] = sum(e.device_type == torch.autograd.DeviceType.CUDA and "emcpy" not in e.name and "emset" not in e.name
                                   for e in prof.events())
        per_pass[flag] = counts
    for flag in (False, True):
        launches[flag]["one_norm_with_tail_kernels"] = per_pass[flag]

    # 3. timing: warm-up, then alternating blocks
    for _ in range(2):
        for flag in (False, True):
            for _ in range(args.steps):
                step(flag)
    torch.cuda.synchronize()
    blocks = {False: [], True: []}
    for r in range(args.rounds):
        for flag in ((False, True) if r % 2 == 0 else (True, False)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                step(flag)
            e1.record()
            torch.cuda.synchronize()
            blocks[flag].append(e0.elapsed_time(e1) / args.steps)
    conv_plan.SYNCBN_ROWS_HIP = False

    def summary(flag):
        v = blocks[flag]
        return dict(ms_per_step_median=round(statistics.median(v), 3), ms_per_step_min=round(min(v), 3), ms_per_step_max=round(max(v), 3),
                    blocks=len(v), launches_per_step=launches[flag])
    result = dict(what="tools/syncbn_rows_bench.py: FastIndoorImVoxelNeck (256 -> 128) converted to SyncBatchNorm3d, forward + backward, "
                       f"{args.scenes} scene(s) of {'x'.join(map(str, args.grid))}, one rank, no process group, no collective; "
                       f"SGC_SYNCBN_ROWS_HIP off (the parent's path, the baseline) and on alternated in one process, "
                       f"{args.rounds} rounds of {args.steps} steps per setting after warm-up of both",
                  device=torch.cuda.get_device_name(0), max_difference_of_scale=worst, flag_off=summary(False), flag_on=summary(True),
                  not_measured="any multi-GPU step: no collective runs here")
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
