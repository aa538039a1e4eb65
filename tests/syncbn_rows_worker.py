"""Worker of tests/test_gpu_syncbn_rows.py::test_real_process_group_through_bn_rows: one rank of a torch.distributed.run job on the
GPU box, backend "nccl" (= RCCL on ROCm).  A ``dist.SyncBatchNorm3d`` through ``conv_plan.bn_rows`` -- ``SYNCBN_ROWS_HIP`` on (the
sgc_bn_rows_sync_* kernels around one all-gather and one all-reduce), then off (the torch formulation, today's path) -- against
``nn.BatchNorm3d`` in float64 on the batch of all ranks (every rank can rebuild it: the inputs are seeded by rank): activations, running
statistics, the input gradient, and the parameter gradients as this rank's LOCAL sums.  The bounds are those of
tests/test_gpu_syncbn_rows.py.  With WORLD_SIZE == 1 the process group is still an RCCL group of one rank, and both collectives run."""
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sgcdet_amd import dist as sd  # noqa: E402
from sgcdet_amd import functions  # noqa: E402
from sgcdet_amd.plugin import conv_plan  # noqa: E402

C, GRID, OFFSETS, EPS, MOMENTUM = 16, (5, 4, 3), (40.0, -25.0), 1e-5, 0.1


def _rank_data(r):
    g = torch.Generator().manual_seed(70 + r)
    V = GRID[0] * GRID[1] * GRID[2]
    return (torch.randn(V, C, generator=g) * 1.5 + OFFSETS[r % 2], torch.randn(V, C, generator=g), torch.randn(V, C, generator=g))


def _to_ncdhw(rows):
    return rows.view(1, *GRID, C).permute(0, 4, 1, 2, 3)


def _graph_names(t):
    seen, names, stack = set(), [], [t.grad_fn]
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.append(type(fn).__name__)
        stack.extend(f for f, _ in fn.next_functions)
    return names


def _check(rank, world, dev, flag):
    conv_plan.SYNCBN_ROWS_HIP = flag
    torch.manual_seed(1)
    bn = sd.SyncBatchNorm3d(C, eps=EPS, momentum=MOMENTUM).to(dev).train()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.normal_()
    bn.process_group = dist.group.WORLD
    w0, b0 = bn.weight.detach().cpu().double(), bn.bias.detach().cpu().double()
    data = [_rank_data(r) for r in range(world)]
    x, res, dy = (t.to(dev) for t in data[rank])
    x.requires_grad_(True)
    y = conv_plan.bn_rows(bn, x, GRID, residual=res, relu=True)
    names = _graph_names(y)
    if hasattr(functions, "SyncBatchNormRowsFunction"):
        assert ("SyncBatchNormRowsFunctionBackward" in names) == flag and ("_SyncBatchNormFnBackward" in names) != flag, names
    y.backward(dy)
    assert int(bn.num_batches_tracked) == 1
    # float64: nn.BatchNorm3d on the batch of all ranks, the tail behind it, the fp32 ReLU mask of this rank's output
    ref = torch.nn.BatchNorm3d(C, eps=EPS, momentum=MOMENTUM).double().train()
    with torch.no_grad():
        ref.weight.copy_(w0)
        ref.bias.copy_(b0)
    with torch.no_grad():
        t = ref(torch.cat([_to_ncdhw(d[0]) for d in data]).double()).permute(0, 2, 3, 4, 1).reshape(world, -1, C)
    mask = (y.detach().cpu() > 0).double()
    yr = (t[rank] + data[rank][1].double()) * mask
    err = float((y.detach().cpu().double() - yr).abs().max())
    assert err < 2e-4, ("y", flag, err)
    assert torch.allclose(bn.running_mean.cpu().double(), ref.running_mean, atol=1e-5), ("running_mean", flag)
    assert torch.allclose(bn.running_var.cpu().double(), ref.running_var, rtol=3e-5), ("running_var", flag)
    # this rank's local sums in float64
    xd = torch.cat([d[0] for d in data]).double()
    mean, var = xd.mean(0), xd.var(0, unbiased=False)
    invstd = 1.0 / torch.sqrt(var + EPS)
    g = dy.cpu().double() * mask
    xhat = (data[rank][0].double() - mean) * invstd
    db, dw = g.sum(0), (g * xhat).sum(0)
    for got, want, name in ((bn.bias.grad, db, "dbias"), (bn.weight.grad, dw, "dweight")):
        err = float((got.cpu().double() - want).abs().max())
        assert err < 2e-4 * max(1.0, float(want.abs().max())), (name, flag, err)
    # dx of this rank's rows: the sums of ALL ranks enter it -- every rank's masked gradient, gathered
    masks = [torch.empty_like(y) for _ in range(world)]
    dist.all_gather(masks, (y.detach() > 0).float())
    xa2 = torch.cat([_to_ncdhw(d[0]) for d in data]).double().requires_grad_(True)
    ref2 = torch.nn.BatchNorm3d(C, eps=EPS, momentum=MOMENTUM).double().train()
    with torch.no_grad():
        ref2.weight.copy_(w0)
        ref2.bias.copy_(b0)
    t2 = ref2(xa2).permute(0, 2, 3, 4, 1).reshape(world, -1, C) * torch.stack([m.cpu().double() for m in masks])
    t2.backward(torch.stack([d[2] for d in data]).double())
    want = xa2.grad[rank].permute(1, 2, 3, 0).reshape(-1, C)
    err = float((x.grad.cpu().double() - want).abs().max())
    assert err < 2e-4 * max(1.0, float(want.abs().max())), ("dx", flag, err)


def main():
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    rank, world, _ = sd.init_from_env(backend="nccl", device=dev)
    if world == 1 and not dist.is_initialized():               # a group of one: init_from_env skips it, RCCL should still load
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    assert dist.get_backend() == "nccl" and dist.get_world_size() == world and world <= 2
    for flag in (True, False):
        _check(rank, world, dev, flag)
    dist.barrier()
    if rank == 0:
        print(f"SYNCBN_ROWS_OK world={world}")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
