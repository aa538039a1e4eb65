"""The buffer cases (tests/buffer_contract.py) of include/sgcdet_amd_syncbn.h -- the four halves of SyncBatchNorm over rows -- and the
float64 torch formulation they and tests/test_gpu_syncbn_rows.py compare with: ``F.batch_norm (+ add, relu)`` autograd on the
CONCATENATION of the rows of all ranks.  tests/test_syncbn_rows_cpu.py holds this table to the coverage rule;
tests/test_gpu_buffers_syncbn.py runs it on the GPU.

The ranks are virtual: one process runs the local half once per rank, stacks the statistics as the all-gather would and adds the sums
as the all-reduce would.  The ranks' data sit at different offsets (+40, -25, +3), so the cross-rank term d^2 n_a n_b / n of Chan's
merge dominates the variance.  Where a case ends in a ReLU the residual is conditioned (``sync_inputs``): no float64 pre-activation
lies within 2e-4 of the tensor's max-abs of zero, so no gate can differ between the kernels and the reference."""
import torch
import torch.nn.functional as F

from buffer_contract import Case

CASES = []
EPS, MOMENTUM = 1e-5, 0.1
OFFSETS = (40.0, -25.0, 3.0)


def sync_inputs(rows_per_rank, C, tail, with_res, seed, offsets=OFFSETS):
    """Per rank r: x_r = randn * 1.5 + offsets[r] [rows_r, C], dy_r, res_r?; shared w, b, rm, rv [C]."""
    g = torch.Generator().manual_seed(seed)
    xs = tuple(torch.randn(n, C, generator=g) * 1.5 + offsets[r] for r, n in enumerate(rows_per_rank))
    d = dict(xs=xs, dys=tuple(torch.randn(n, C, generator=g) for n in rows_per_rank), w=0.5 + torch.rand(C, generator=g),
             b=0.3 * torch.randn(C, generator=g), rm=0.2 * torch.randn(C, generator=g), rv=0.5 + torch.rand(C, generator=g), tail=int(tail))
    if with_res:
        d["res"] = tuple(torch.randn(n, C, generator=g) for n in rows_per_rank)
    if tail:
        pre = sync_reference(d)["pre"]
        lim = 2e-4 * float(pre.abs().max())
        small = pre.abs() < lim
        if bool(small.any()):
            assert with_res, "a ReLU case without a residual cannot be conditioned here"
            for r, s in zip(d["res"], small.split(list(rows_per_rank))):       # the residual moves its pre-activation and no statistic
                r[s] += 100 * lim
            assert float(sync_reference(d)["pre"].abs().min()) >= lim
    return d


def sync_reference(i, dtype=torch.float64):
    """Every output of the four entries in ``dtype`` on the CPU: per rank ``stats`` [2C + 1], ``y``, ``dx``, ``dres``, ``sums`` [2C]
    (that rank's dbias | dweight); shared ``mean``, ``invstd``, ``inv_count``, ``rm``, ``rv``; and ``pre``, the values the ReLU tests."""
    ns = [x.shape[0] for x in i["xs"]]
    C = i["xs"][0].shape[1]
    x = torch.cat([t.detach().cpu() for t in i["xs"]]).to(dtype).requires_grad_(True)
    dy = torch.cat([t.detach().cpu() for t in i["dys"]]).to(dtype)
    w, b = (i[k].detach().cpu().to(dtype).requires_grad_(True) for k in ("w", "b"))
    res = torch.cat([t.detach().cpu() for t in i["res"]]).to(dtype).requires_grad_(True) if "res" in i else None
    rm, rv = i["rm"].detach().cpu().to(dtype).clone(), i["rv"].detach().cpu().to(dtype).clone()
    t = F.batch_norm(x, rm, rv, w, b, True, MOMENTUM, EPS)
    pre = t if res is None else t + res
    y = F.relu(pre) if i["tail"] else pre
    y.backward(dy)
    xd = x.detach()
    mean, var = xd.mean(0), xd.var(0, unbiased=False)
    invstd = 1.0 / torch.sqrt(var + EPS)
    g = dy * (pre.detach() > 0).to(dtype) if i["tail"] else dy
    xhat = (xd - mean) * invstd
    out = dict(mean=mean, invstd=invstd, inv_count=torch.tensor([1.0 / sum(ns)], dtype=dtype), rm=rm, rv=rv, pre=pre.detach())
    for r, (xr, yr, dxr, gr, hr) in enumerate(zip(xd.split(ns), y.detach().split(ns), x.grad.split(ns), g.split(ns), xhat.split(ns))):
        m = xr.mean(0)
        out[f"stats{r}"] = torch.cat([m, ((xr - m) ** 2).sum(0), torch.tensor([float(ns[r])], dtype=dtype)])
        out[f"y{r}"], out[f"dx{r}"] = yr, dxr
        out[f"sums{r}"] = torch.cat([gr.sum(0), (gr * hr).sum(0)])
        if res is not None:
            out[f"dres{r}"] = res.grad.split(ns)[r]
    return out


def sync_run(ops, t, rm_for_all=False):
    """The four entries over the virtual ranks of ``t``.  Rank 0 updates ``t['rm']`` / ``t['rv']`` in place; the other ranks pass no
    running statistics (``rm_for_all``: clones of the originals, returned as ``rm1`` ...)."""
    xs, dys, res, tail = t["xs"], t["dys"], t.get("res"), t["tail"]
    world, C = len(xs), xs[0].shape[1]
    out = {}
    rm0, rv0 = t["rm"].clone(), t["rv"].clone()
    gathered = torch.empty((world, 2 * C + 1), dtype=torch.float32, device=xs[0].device)
    for r, x in enumerate(xs):
        out[f"stats{r}"] = ops.bn_rows_sync_stats(x)
        gathered[r].copy_(out[f"stats{r}"])                                    # the all-gather
    fwd = []
    for r, x in enumerate(xs):
        rm, rv = (t["rm"], t["rv"]) if r == 0 else ((rm0.clone(), rv0.clone()) if rm_for_all else (None, None))
        y, mean, invstd, inv_count = ops.bn_rows_sync_apply(x, gathered, t["w"], t["b"], rm, rv, MOMENTUM, EPS,
                                                            residual=None if res is None else res[r], relu=bool(tail))
        fwd.append((y, mean, invstd, inv_count))
        out[f"y{r}"] = y
        if r == 0:
            out.update(mean=mean, invstd=invstd, inv_count=inv_count, rm=rm, rv=rv)
        else:
            out.update({f"mean{r}": mean, f"invstd{r}": invstd})
            if rm_for_all:
                out.update({f"rm{r}": rm, f"rv{r}": rv})
    total = None
    for r, x in enumerate(xs):
        y, mean, invstd, _ = fwd[r]
        out[f"sums{r}"] = ops.bn_rows_sync_backward_sums(x, dys[r], mean, invstd, y_relu=y if tail else None)
        total = out[f"sums{r}"].clone() if total is None else total + out[f"sums{r}"]     # the all-reduce, in rank order
    for r, x in enumerate(xs):
        y, mean, invstd, inv_count = fwd[r]
        dx, dres = ops.bn_rows_sync_backward_apply(x, dys[r], mean, invstd, t["w"], total, inv_count, y_relu=y if tail else None,
                                                   want_dresidual=res is not None)
        out[f"dx{r}"] = dx
        if dres is not None:
            out[f"dres{r}"] = dres
    return out


def _ref(i):
    r = sync_reference(i)
    r.pop("pre")
    world = len(i["xs"])
    for k in range(1, world):                                  # every rank computes the shared statistics
        r[f"mean{k}"], r[f"invstd{k}"] = r["mean"], r["invstd"]
    return r


def _sync_case(rows_per_rank, C, tail, with_res):
    # 2e-4 of max(1, max |ref|), the bound of the padded norm's cases (tests/buffer_cases_depth_train.py); the batch mean 1e-5 of its
    # size, as tests/test_gpu_kernels.py bounds a mean at offset 40
    names = ["mean"] + [f"mean{r}" for r in range(1, len(rows_per_rank))]
    tol = dict({k: 2e-4 for k in ["invstd", "inv_count", "rm", "rv"] + [f"{n}{r}" for n in ("stats", "y", "sums", "dx", "dres", "invstd")
                                                                        for r in range(len(rows_per_rank))]}, **{n: 1e-5 for n in names})
    return Case(f"bn_rows_sync-{'+'.join(map(str, rows_per_rank))}x{C}-tail{tail}{'-residual' if with_res else ''}",
                ("sgc_bn_rows_sync_stats", "sgc_bn_rows_sync_apply", "sgc_bn_rows_sync_backward_sums", "sgc_bn_rows_sync_backward_apply"),
                lambda: sync_inputs(rows_per_rank, C, tail, with_res, 23), sync_run, ref=_ref, tol=tol, accumulated=("rm", "rv"), only="cuda")


# ragged rows at the narrowest width, no tail; a rank of one row behind a ReLU with the identity; three ranks through the column loop
CASES += [_sync_case((37, 91), 4, 0, False), _sync_case((1, 63), 132, 1, True), _sync_case((77, 5, 130), 1040, 1, True)]
