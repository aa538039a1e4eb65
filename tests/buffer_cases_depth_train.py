"""The buffer cases (tests/buffer_contract.py) of include/sgcdet_amd_depth_train.h: the padded live BatchNorm and the softmax
backward.  tests/test_depth_unets_train_cpu.py holds this table to the coverage rule tests/test_buffers_cpu.py states for the other
headers; tests/test_gpu_buffers_depth_train.py runs it on the GPU.  The references are float64 torch.

The inputs carry NaN in every padding column: the header says they are never read.  The norm's inputs are conditioned
(``bn_padded_conditioned``): no float64 pre-activation lies within 1e-4 of its tensor's max-abs of zero (``gate_margin``; the tests
assert it), so no ReLU gate can differ between the kernels and the reference."""
import torch
import torch.nn.functional as F

from buffer_contract import Case

CASES = []
_BN_ACC = ("rm", "rv")           # the running statistics are updated in place (in-out inputs)
EPS, MOMENTUM = 1e-5, 0.1


def bn_padded_inputs(rows, C, ld, tail, with_res, seed, pad_value=float("nan"), spread=None):
    """``spread`` scales x; default 1, and 0.01 over TWO rows.  There xhat = +-sqrt(var / (var + eps)) and
    dx = weight * invstd * (g1 - g2) / 2 * eps / (var + eps): with var far above eps the input gradient is zero up to eps, a
    difference of terms 1 / eps times its size, and comparing it with itself measures that cancellation alone.  A column spread of
    0.01 - 0.1 keeps var within a few hundred eps, where dx is a quantity of the size of its terms."""
    g = torch.Generator().manual_seed(seed)
    pad = lambda t: torch.cat([t, torch.full((rows, ld - C), pad_value)], 1).contiguous()        # noqa: E731
    spread = (0.01 if rows == 2 else 1.0) if spread is None else spread
    d = dict(x=pad((torch.randn(rows, C, generator=g) * 1.5 + 0.3) * spread), dy=pad(torch.randn(rows, C, generator=g)),
             w=0.5 + torch.rand(C, generator=g), b=0.3 * torch.randn(C, generator=g), rm=0.2 * torch.randn(C, generator=g),
             rv=0.5 + torch.rand(C, generator=g), C=C, tail=tail)
    if with_res:
        d["res"] = pad(torch.randn(rows, C, generator=g))
    return d


def bn_padded_reference(i):
    """float64 torch: every output of the two entries, the padding columns as zeros, and ``pre`` -- the values the ReLU gates test."""
    C, tail = i["C"], i["tail"]
    x = i["x"][:, :C].double().requires_grad_(True)
    w, b = i["w"].double().requires_grad_(True), i["b"].double().requires_grad_(True)
    res = i["res"][:, :C].double().requires_grad_(True) if "res" in i else None
    rm, rv = i["rm"].double().clone(), i["rv"].double().clone()
    t = F.batch_norm(x, rm, rv, w, b, True, MOMENTUM, EPS)
    pre = t if tail == 2 or res is None else t + res
    y = pre if tail == 0 else (F.relu(pre) if tail == 1 else F.relu(t) + res)
    y.backward(i["dy"][:, :C].double())
    ld = i["x"].shape[1]
    pad = lambda v: F.pad(v.detach(), (0, ld - C))                                               # noqa: E731
    mean, var = x.detach().mean(0), x.detach().var(0, unbiased=False)
    out = dict(y=pad(y), mean=mean, invstd=1.0 / torch.sqrt(var + EPS), rm=rm, rv=rv, dx=pad(x.grad), dw=w.grad, db=b.grad, pre=pre.detach())
    if res is not None:
        out["dres"] = pad(res.grad)
    return out


def gate_margin(pre):
    return (pre.abs().min() / pre.abs().max()).item()


def bn_padded_conditioned(rows, C, ld, tail, with_res, seed=0, spread=None):
    """(``bn_padded_inputs``, their reference) with the inputs nudged until no float64 pre-activation of a gate lies within 2e-4 of
    the tensor's max-abs of zero: such an element of x moves by 0.03 of the spread, which moves its pre-activation a hundred times further than
    that and the batch statistics by little."""
    i = bn_padded_inputs(rows, C, ld, tail, with_res, seed, spread=spread)
    step = 0.03 * ((0.01 if rows == 2 else 1.0) if spread is None else spread)
    for _ in range(8):
        ref = bn_padded_reference(i)
        pre = ref["pre"]
        small = pre.abs() < 2e-4 * pre.abs().max()
        if tail == 0 or not bool(small.any()):
            return i, ref
        i["x"][:, :C][small] += step
    raise AssertionError("no conditioned input")


def bn_padded_run(ops, t):
    res = t.get("res")
    y, mean, invstd = ops.bn_rows_padded_forward(t["x"], t["w"], t["b"], t["rm"], t["rv"], MOMENTUM, EPS, residual=res, tail=t["tail"])
    dx, dw, db, dres = ops.bn_rows_padded_backward(t["x"], t["dy"], mean, invstd, t["w"], bias=t["b"], y=y, tail=t["tail"],
                                                   want_dresidual=res is not None)
    return dict(y=y, mean=mean, invstd=invstd, rm=t["rm"], rv=t["rv"], dx=dx, dw=dw, db=db, dres=dres)


def _bn_ref(i):
    r = bn_padded_reference(i)
    r.pop("pre")
    return r


# (rows, C, ld, tail, residual, seed)
BN_CASES = [(6, 4, 4, 0, False, 0), (77, 44, 64, 1, True, 0), (77, 12, 32, 2, True, 0), (130, 140, 160, 2, True, 0)]


def _bn_case(rows, C, ld, tail, with_res, seed):
    return Case(f"bn_rows_padded-{rows}x{C}_in_{ld}-tail{tail}{'-residual' if with_res else ''}",
                ("sgc_bn_rows_padded_forward", "sgc_bn_rows_padded_backward"), lambda: bn_padded_conditioned(rows, C, ld, tail, with_res, seed)[0],
                bn_padded_run, ref=_bn_ref, tol=2e-4, accumulated=_BN_ACC, only="cuda")


CASES += [_bn_case(*c) for c in BN_CASES]


def softmax_inputs(rows, C, ldp, lddp, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.softmax(2.0 * torch.randn(rows, C, generator=g), 1)
    pad = lambda t, ld: torch.cat([t, torch.full((rows, ld - C), float("nan"))], 1).contiguous()  # noqa: E731
    return dict(p=pad(p, ldp), dp=pad(torch.randn(rows, C, generator=g), lddp), C=C)


def softmax_reference(i, ldg):
    C = i["C"]
    p, dp = i["p"][:, :C].double(), i["dp"][:, :C].double()
    return F.pad(p * (dp - (p * dp).sum(1, keepdim=True)), (0, ldg - C))


def _softmax_case(rows, C, ldp, lddp, ldg):
    # |g - g64| <= (C + 4) * 2^-24 * max |dp| (the header's bound), as an absolute tolerance
    def tol():
        return (C + 4) * 2.0 ** -24 * float(softmax_inputs(rows, C, ldp, lddp, 5)["dp"][:, :C].abs().max())
    return Case(f"softmax_rows_backward-{rows}x{C}-pitches_{ldp}_{lddp}_{ldg}", ("sgc_softmax_rows_backward",),
                lambda: softmax_inputs(rows, C, ldp, lddp, 5), lambda ops, t: dict(g=ops.softmax_rows_backward(t["p"], t["dp"], C=t["C"], ldg=ldg)),
                ref=lambda i: dict(g=softmax_reference(i, ldg)), tol=tol(), unit_floor="abs", only="cuda")


CASES += [_softmax_case(1, 4, 4, 4, 4), _softmax_case(197, 12, 12, 32, 32), _softmax_case(67, 128, 128, 132, 128)]
