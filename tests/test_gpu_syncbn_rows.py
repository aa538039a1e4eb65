"""SyncBatchNorm of the 3-D neck on the row kernels (include/sgcdet_amd_syncbn.h, ``functions.SyncBatchNormRowsFunction``,
``conv_plan.SYNCBN_ROWS_HIP``) on the GPU.  The reference of the new entries is float64 torch on the concatenation of
all ranks' rows (tests/buffer_cases_syncbn.py); the bounds are those of
tests/test_gpu_kernels.py::test_batch_norm_rows_kernels_against_the_oracle_and_torch: mean 1e-5 of the largest offset, invstd 2e-5
relative, y 2e-4, running mean atol 1e-5, running variance rtol 3e-5, every gradient 2e-4 of max(1, max |ref|).  Most tests need one
process and no process group: the ranks are virtual (the local half once per rank, the collective done on the host side of the
test), and one rank is held bit for bit to ``sgc_bn_rows_act_forward / _backward``."""
import copy
import os
import socket
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import nonfinite_contract as nf
from buffer_cases_syncbn import EPS, MOMENTUM, OFFSETS, sync_inputs, sync_reference, sync_run

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cu(obj):
    if isinstance(obj, torch.Tensor):
        return obj.cuda()
    if isinstance(obj, tuple):
        return tuple(_cu(o) for o in obj)
    if isinstance(obj, dict):
        return {k: _cu(v) for k, v in obj.items()}
    return obj


def _err(got, ref):
    return float((got.detach().cpu().double() - ref.double()).abs().max())


def _grad_close(got, ref, what):
    err, bound = _err(got, ref), 2e-4 * max(1.0, float(ref.abs().max()))
    print(f"{what}: max|err| {err:.3e}, bound {bound:.3e}")
    assert err < bound, what


# ---- 1. virtual ranks -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,C", [((37, 91), 4), ((400, 400), 1024), ((1, 63), 132), ((77, 5, 1237), 1040)],
                         ids=lambda v: "+".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_virtual_ranks_against_float64_on_the_concatenation(rows, C, gpu_ops):
    world = len(rows)
    i = sync_inputs(rows, C, 0, False, seed=sum(rows) + C)
    ref = sync_reference(i)
    got = sync_run(gpu_ops, _cu(i), rm_for_all=True)
    again = sync_run(gpu_ops, _cu(i), rm_for_all=True)
    assert set(got) == set(again)
    for k in got:                                               # ordered merges, no atomics: the same bits every run
        assert torch.equal(got[k], again[k]), k
    for r in range(1, world):                                   # merged in rank order: every rank computes the same bits
        for name in ("mean", "invstd", "rm", "rv"):
            assert torch.equal(got[f"{name}{r}"], got[name]), (name, r)
    off = max(abs(o) for o in OFFSETS[:world])
    err = _err(got["mean"], ref["mean"])
    print(f"mean: max|err| {err:.3e}, bound {1e-5 * off:.3e}")
    assert err < 1e-5 * off
    rel = float(((got["invstd"].cpu().double() - ref["invstd"]) / ref["invstd"]).abs().max())
    print(f"invstd: max rel err {rel:.3e}, bound 2e-5")
    assert rel < 2e-5
    assert float(got["inv_count"]) == pytest.approx(1.0 / sum(rows), rel=1e-7)
    assert torch.allclose(got["rm"].cpu().double(), ref["rm"], atol=1e-5) and torch.allclose(got["rv"].cpu().double(), ref["rv"], rtol=3e-5)
    for r in range(world):
        s, sr = got[f"stats{r}"].cpu().double(), ref[f"stats{r}"]
        assert float(s[2 * C]) == rows[r]
        assert float((s[:C] - sr[:C]).abs().max()) < 1e-5 * abs(OFFSETS[r])
        # invstd = (M2 / N + eps)^-1/2 is held to 2e-5 relative, which is 4e-5 relative in M2
        assert float((s[C:2 * C] - sr[C:2 * C]).abs().max()) <= 4e-5 * float(sr[C:2 * C].abs().max())
        if rows[r] == 1:
            assert bool((s[C:2 * C] == 0).all())                # one row: M2 is exactly zero
        err = _err(got[f"y{r}"], ref[f"y{r}"])
        print(f"y of rank {r}: max|err| {err:.3e}, bound 2e-4")
        assert err < 2e-4
        _grad_close(got[f"dx{r}"], ref[f"dx{r}"], f"dx of rank {r}")
        _grad_close(got[f"sums{r}"][:C], ref[f"sums{r}"][:C], f"dbias of rank {r}")
        _grad_close(got[f"sums{r}"][C:], ref[f"sums{r}"][C:], f"dweight of rank {r}")


# ---- 2. one rank is the plain kernels, bit for bit ------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [False, True], ids=["", "residual"])
@pytest.mark.parametrize("tail", [0, 1])
@pytest.mark.parametrize("rows,C", [(1237, 128), (77, 1040)])
def test_one_rank_is_bit_identical_to_the_plain_entries(rows, C, tail, res, gpu_ops):
    g = torch.Generator().manual_seed(rows + C + tail)
    x = (torch.randn(rows, C, generator=g) * 1.5 + 3.0).cuda()
    w, b = (torch.rand(C, generator=g) + 0.5).cuda(), torch.randn(C, generator=g).cuda()
    r = torch.randn(rows, C, generator=g).cuda() if res else None
    dy = torch.randn(rows, C, generator=g).cuda()
    rm, rv = torch.randn(C, generator=g).cuda(), (torch.rand(C, generator=g) + 0.5).cuda()
    rm0, rv0, rm_before = rm.clone(), rv.clone(), rm.clone()
    y0, mean0, invstd0 = gpu_ops.bn_rows_forward(x, w, b, rm0, rv0, MOMENTUM, EPS, residual=r, relu=bool(tail))
    stats = gpu_ops.bn_rows_sync_stats(x)
    y1, mean1, invstd1, inv_count = gpu_ops.bn_rows_sync_apply(x, stats, w, b, rm, rv, MOMENTUM, EPS, residual=r, relu=bool(tail))
    assert float(stats[2 * C]) == rows and torch.equal(stats[:C], mean0)
    for a, c, name in ((y1, y0, "y"), (mean1, mean0, "mean"), (invstd1, invstd0, "invstd"), (rm, rm0, "running_mean"), (rv, rv0, "running_var")):
        assert torch.equal(a, c), name
    assert not torch.equal(rm, rm_before)                      # and they were updated
    out0 = gpu_ops.bn_rows_backward(x, dy, mean0, invstd0, w, y_relu=y0 if tail else None, want_dresidual=res)
    sums = gpu_ops.bn_rows_sync_backward_sums(x, dy, mean1, invstd1, y_relu=y1 if tail else None)
    dx, dres = gpu_ops.bn_rows_sync_backward_apply(x, dy, mean1, invstd1, w, sums, inv_count, y_relu=y1 if tail else None, want_dresidual=res)
    assert torch.equal(dx, out0[0]) and torch.equal(sums[C:], out0[1]) and torch.equal(sums[:C], out0[2])
    if res:
        assert torch.equal(dres, out0[3])
    else:
        assert dres is None


# ---- 3. the Function against float64 autograd -----------------------------------------------------------------------------------
@pytest.mark.parametrize("res,relu", [(False, False), (True, True), (False, True)])
def test_function_against_float64_autograd_without_a_process_group(res, relu, gpu_ops):
    from sgcdet_amd.functions import SyncBatchNormRowsFunction
    assert not torch.distributed.is_initialized()
    rows, C = 1237, 128
    g = torch.Generator().manual_seed(rows + C + 1)
    x = (torch.randn(rows, C, generator=g) * 1.5 + 3.0).cuda()
    w, b = (torch.rand(C, generator=g) + 0.5).cuda(), torch.randn(C, generator=g).cuda()
    r = torch.randn(rows, C, generator=g).cuda() if res else None
    dy = torch.randn(rows, C, generator=g).cuda()
    rm, rv = torch.randn(C, generator=g).cuda(), (torch.rand(C, generator=g) + 0.5).cuda()
    xg, wg, bg = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    rg = r.clone().requires_grad_(True) if res else None
    rmd, rvd = rm.cpu().double(), rv.cpu().double()
    y = SyncBatchNormRowsFunction.apply(xg, wg, bg, rm, rv, MOMENTUM, EPS, rg, int(relu), None)
    y.backward(dy)
    xd, wd, bd = x.cpu().double().requires_grad_(True), w.cpu().double().requires_grad_(True), b.cpu().double().requires_grad_(True)
    rd = r.cpu().double().requires_grad_(True) if res else None
    t = F.batch_norm(xd, rmd, rvd, wd, bd, True, MOMENTUM, EPS)
    t = t + rd if res else t
    # the float64 reference masks on ITS OWN sign; entries whose fp32 pre-activation is within rounding of zero may differ: use the fp32 mask
    if relu:
        t = t * (y.detach().cpu() > 0).double()
    t.backward(dy.cpu().double())
    assert _err(y, t.detach()) < 2e-4
    assert torch.allclose(rm.cpu().double(), rmd, atol=1e-5) and torch.allclose(rv.cpu().double(), rvd, rtol=3e-5)
    for a, d, name in ((xg.grad, xd.grad, "dx"), (wg.grad, wd.grad, "dweight"), (bg.grad, bd.grad, "dbias")) + (((rg.grad, rd.grad, "dresidual"),) if res else ()):
        _grad_close(a, d, name)


# ---- 4. launches ----------------------------------------------------------------------------------------------------------------
def _device_activity(prof):
    dev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    copies = [e.name for e in dev if "emcpy" in e.name or "Copy" in e.name]
    kernels = [e.name for e in dev if e.name not in copies and "emset" not in e.name]
    host = {e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CPU}
    return kernels, copies, host


def test_forward_is_at_most_four_kernels_backward_three_and_nothing_synchronises(gpu_ops):
    from torch.profiler import ProfilerActivity, profile
    from sgcdet_amd.functions import SyncBatchNormRowsFunction
    rows, C = 3200, 512
    g = torch.Generator().manual_seed(7)
    x, r, dy = (torch.randn(rows, C, generator=g).cuda().requires_grad_(k < 2) for k in range(3))
    w, b = (torch.rand(C, generator=g) + 0.5).cuda().requires_grad_(True), torch.randn(C, generator=g).cuda().requires_grad_(True)
    rm, rv = torch.zeros(C).cuda(), torch.ones(C).cuda()

    def forward():
        return SyncBatchNormRowsFunction.apply(x, w, b, rm, rv, MOMENTUM, EPS, r, 1, None)

    def backward(y):
        return torch.autograd.grad(y, (x, w, b, r), dy)
    backward(forward())                                        # allocator, library and profiler warm
    torch.cuda.synchronize()
    counts = {}
    torch.cuda.set_sync_debug_mode("error")                    # a synchronising torch call inside raises
    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof_f:
            y = forward()
            torch.cuda.set_sync_debug_mode("default")
            torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof_b:
            backward(y)
            torch.cuda.set_sync_debug_mode("default")
            torch.cuda.synchronize()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for name, prof, most in (("forward", prof_f, 4), ("backward", prof_b, 3)):
        kernels, copies, host = _device_activity(prof)
        print(f"{name}: {len(kernels)} kernels {kernels}, copies {copies}")
        assert kernels and all("bn_" in k for k in kernels), kernels           # only this feature's kernels
        assert len(kernels) <= most, kernels
        assert not copies, copies
        assert not (host - {"hipDeviceSynchronize"}) & {"hipStreamSynchronize", "hipEventSynchronize", "hipMemcpy", "hipMemcpyDtoH",
                                                       "hipMemcpyWithStream", "hipMemcpyAsync"}, host
        counts[name] = len(kernels)
    assert counts == dict(forward=4, backward=3)


# ---- 5. the neck ----------------------------------------------------------------------------------------------------------------
def _graph_functions(outputs):
    seen, names, stack = set(), [], [o.grad_fn for o in outputs]
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.append(type(fn).__name__)
        stack.extend(f for f, _ in fn.next_functions)
    return names


def _neck_step(neck, x):
    inp = x.clone().requires_grad_(True)
    feats = neck(inp)
    names = _graph_functions(feats)
    sum((f ** 2).mean() for f in feats).backward()
    return [f.detach() for f in feats], inp.grad, names


@pytest.mark.parametrize("B", [1, 2])
def test_converted_neck_equals_the_plain_neck_bit_for_bit(B, monkeypatch, gpu_ops):
    from sgcdet_amd import dist as sd
    from sgcdet_amd.plugin import conv_plan
    from sgcdet_amd.plugin.neck3d import FastIndoorImVoxelNeck
    assert not torch.distributed.is_initialized()
    torch.manual_seed(3)
    plain = FastIndoorImVoxelNeck(in_channels=64, n_blocks=[1, 1, 1], out_channels=32).cuda().train()
    n_norms = sum(isinstance(m, torch.nn.BatchNorm3d) for m in plain.modules())
    assert n_norms == 15
    sync_on, sync_off = (sd.convert_sync_batchnorm(copy.deepcopy(plain)) for _ in range(2))
    assert sum(type(m) is sd.SyncBatchNorm3d for m in sync_on.modules()) == n_norms
    x = torch.randn(B, 64, 16, 12, 8, device="cuda")
    monkeypatch.setattr(conv_plan, "SYNCBN_ROWS_HIP", False)
    fa, ga, na = _neck_step(plain, x)
    assert na.count("BatchNormRowsFunctionBackward") == n_norms
    _, _, no = _neck_step(sync_off, x)                       # the flag off: today's path, norm for norm
    assert no.count("_SyncBatchNormFnBackward") == n_norms and "SyncBatchNormRowsFunctionBackward" not in no
    monkeypatch.setattr(conv_plan, "SYNCBN_ROWS_HIP", True)
    fb, gb, nb = _neck_step(sync_on, x)
    assert nb.count("SyncBatchNormRowsFunctionBackward") == n_norms and "_SyncBatchNormFnBackward" not in nb
    assert "BatchNormRowsFunctionBackward" not in nb
    assert len(fa) == len(fb) and all(torch.equal(a, b) for a, b in zip(fa, fb))
    assert torch.equal(ga, gb)
    pa, pb = dict(plain.named_parameters()), dict(sync_on.named_parameters())
    assert set(pa) == set(pb) and all(p.grad is not None for p in pa.values())
    for k in pa:
        assert torch.equal(pa[k].grad, pb[k].grad), k
    ba, bb = dict(plain.named_buffers()), dict(sync_on.named_buffers())
    assert set(ba) == set(bb) and len(ba) == 3 * n_norms
    for k in ba:
        assert torch.equal(ba[k], bb[k]), k
    assert all(int(v) == 1 for k, v in bb.items() if k.endswith("num_batches_tracked"))


# ---- 6. non-finite values ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["nan", "+inf"])
def test_a_non_finite_value_in_one_rank_takes_its_channel_on_every_rank(kind, gpu_ops):
    rows, C, c = (37, 91), 132, 7
    clean = sync_inputs(rows, C, 0, False, seed=5)
    i = dict(clean, xs=tuple(x.clone() for x in clean["xs"]))
    i["xs"][1][5, c] = nf.KINDS[kind]
    ref = sync_reference(i)
    got = sync_run(gpu_ops, _cu(i), rm_for_all=True)
    base = sync_run(gpu_ops, _cu(clean), rm_for_all=True)
    others = torch.arange(C) != c
    for name in ("mean", "invstd", "rm", "rv", "mean1", "invstd1", "rm1", "rv1", "y0", "y1", "dx0", "dx1"):
        v = got[name].cpu()
        assert bool(torch.isnan(v[..., c]).all()), f"{name}: channel {c} is not NaN everywhere"
        assert torch.equal(v[..., others], base[name].cpu()[..., others]), f"{name}: another channel changed"
    for name in ("mean", "invstd", "rm", "rv", "stats0", "stats1", "y0", "y1", "sums0", "sums1", "dx0", "dx1"):
        # the one-pass mean meets Inf - Inf where the two-pass float64 mean keeps the infinity (tests/nonfinite_contract.py)
        nf.compare_exact(got[name], ref[name], 2e-4, f"sync bn {kind}: {name}", need_nonfinite=name != "stats0",
                         inf_as_nan=name in ("mean", "rm", "stats1"))
    assert bool(torch.isfinite(got["stats0"]).all()) and float(got["inv_count"]) == pytest.approx(1.0 / sum(rows), rel=1e-7)


# ---- 7. a real process group ----------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.timeout(600)
def test_real_process_group_through_bn_rows():
    """tests/syncbn_rows_worker.py under ``torch.distributed.run``: two RCCL ranks when the box has two GPUs, otherwise one.  A group
    of ONE rank proves that the Function's all-gather and all-reduce run through RCCL with the shapes and dtypes they are given
    (``SyncBatchNormRowsFunction`` calls them whenever a group is initialised), that ``bn_rows`` hands the module's process group
    through, and that the results around a real collective still meet the float64 bounds.  It does NOT prove the merge across
    ranks, the rank order or the local-sum gradients of a rank that holds part of the batch: those are what the virtual-rank tests
    above prove on the kernels, and what the two-rank run proves end to end."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    n = 2 if torch.cuda.device_count() >= 2 else 1
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "syncbn_rows_worker.py")]
    r = subprocess.run(cmd, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"), capture_output=True, text=True, timeout=500)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert f"SYNCBN_ROWS_OK world={n}" in r.stdout
