"""``DepthNet_Fusion``'s regulation U-Nets, ``depth_reg`` and the softmax in training on the HIP kernels
(include/sgcdet_amd_depth_train.h, csrc/batch_norm.hip, csrc/softmax_rows.hip, functions.py ``BatchNormRowsFunction`` /
``PaddedConv2dFunction`` / ``ConvTranspose2dRowsFunction`` / ``DepthRegSoftmaxFunction``, plugin/conv_plan.py, plugin/depth_net.py,
DESIGN.md 4.14b).

References are float64 torch on the CPU, or the dense entries ``sgc_bn_rows_act_forward / _backward`` this library already has.
Bounds: 1e-4 of the compared tensor's max-abs for the layers (the project's bf16x3 bound for these layers,
tests/test_gpu_depth_net_train.py); (C + 4) * 2^-24 * max |dp| for the softmax backward, the fp32 bound of a C-term sum; exact
equality where the arithmetic is exact (small-integer operands) or where two entries evaluate the same expressions in the same order.
Over TWO rows dx = weight * invstd * (g1 - g2) / 2 * eps / (var + eps): the two-row inputs keep var within a few hundred eps
(``bn_padded_inputs``), where that is a quantity of the size of its terms and is held to 1e-4 like every other tensor; two rows
far apart, where it is zero up to eps, have ``test_padded_norm_dx_over_two_spread_rows`` and the rounding of the cancelling terms.

A ReLU gate whose pre-activation lies within rounding of zero says nothing about a kernel, so the inputs are conditioned: the padded
norm's inputs are nudged until the float64 pre-activations keep ``gate_margin`` > 1e-4 (``bn_padded_conditioned``; asserted), and the U-Net and module tests
count the gates that differ between the two computations themselves and require zero, on seeds found on an MI355X (UNET_SEEDS,
MODULE_SEED).  One whole U-Net goes through six live norms, which amplify rounding: its bound is four times the measured figure
(MEASURED, profiles/r22_depth_unets_train_parity.json), the margin of the trunk test."""
import copy
import json
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from buffer_cases_depth_train import EPS, MOMENTUM, bn_padded_conditioned, gate_margin, softmax_inputs, softmax_reference
from golden_util import fill_by_name, max_err

pytestmark = pytest.mark.gpu

# what an MI355X gave: worst error relative to the compared tensor's max-abs
MEASURED = dict(unet_forward={12: 9.604e-06, 32: 1.197e-05, 44: 1.312e-05}, unet_param_grad={12: 2.338e-05, 32: 2.569e-05, 44: 2.048e-05},
                module_forward=1.514e-05)
MARGIN = 4.0
# no ReLU gate of the kernels' run differs from the float64 reference's (c = 32: seed 0 flips one gate, which moves a gradient by 21 %)
UNET_SEEDS = {12: 0, 32: 1, 44: 0}
# no U-Net gate differs between the switch-on run and SGC_DEPTH_NET_TRAIN_HIP=1 alone; seeds 0 - 3 flip 1, 2, 3 and 1 of 215 040 gates
# and fail 3, 45, 22 and 1 of the gradient criteria
MODULE_SEED = 4


@pytest.fixture(scope="module", autouse=True)
def _leave_nothing_behind():
    yield
    if torch.cuda.is_available():
        from sgcdet_amd.functions import train_weight_planes
        train_weight_planes().clear()
        torch.cuda.empty_cache()


def _record(key, value):
    """Print a figure and, when SGC_DEPTH_UNETS_TRAIN_PARITY_JSON names a file, keep its worst case there."""
    print(f"depth-net U-Nets train parity: {key} {value:.3e}")
    path = os.environ.get("SGC_DEPTH_UNETS_TRAIN_PARITY_JSON")
    if path:
        rec = json.load(open(path)) if os.path.exists(path) else {}
        rec[key] = max(rec.get(key, 0.0), value)
        with open(path, "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)


def _pad32(n):
    return (n + 31) // 32 * 32


def _plus_zero(t):
    return bool((t == 0).all()) and not bool(torch.signbit(t).any())


# ---- 1. the padded norm ------------------------------------------------------------------------------------------------------------
ROWS = [2, 7, 192, 16500]        # 16500: above the 256 slabs of 64 rows bn_stats_partial_kernel splits into (65 rows per slab, a ragged last one)
WIDTHS = [(12, 32), (24, 32), (44, 64), (140, 160), (64, 64)]
TAILS = [(0, False), (0, True), (1, False), (1, True), (2, True)]      # (tail, residual)


def _padded_step(ops, i, dev="cuda"):
    t = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in i.items()}
    res = t.get("res")
    y, mean, invstd = ops.bn_rows_padded_forward(t["x"], t["w"], t["b"], t["rm"], t["rv"], MOMENTUM, EPS, residual=res, tail=i["tail"])
    dx, dw, db, dres = ops.bn_rows_padded_backward(t["x"], t["dy"], mean, invstd, t["w"], bias=t["b"], y=y, tail=i["tail"], want_dresidual=res is not None)
    out = dict(y=y, mean=mean, invstd=invstd, rm=t["rm"], rv=t["rv"], dx=dx, dw=dw, db=db)
    if res is not None:
        out["dres"] = dres
    return out


def _dense_step(ops, i):
    """The same layer through the dense entries on the compacted [rows, C] matrices: tails 0 / 1 directly, tail 2 as the dense
    relu(bn(x)) followed by torch's fp32 add -- the one addition the padded kernel performs."""
    C, tail = i["C"], i["tail"]
    cut = lambda v: v[:, :C].contiguous().cuda()                                                 # noqa: E731
    x, dy, res = cut(i["x"]), cut(i["dy"]), (cut(i["res"]) if "res" in i else None)
    w, b, rm, rv = (i[k].cuda() for k in ("w", "b", "rm", "rv"))
    y, mean, invstd = ops.bn_rows_forward(x, w, b, rm, rv, MOMENTUM, EPS, residual=None if tail == 2 else res, relu=tail != 0)
    if tail == 0 and res is None:
        dx, dw, db = ops.bn_rows_backward(x, dy, mean, invstd, w)
        dres = None
    else:
        dx, dw, db, dres = ops.bn_rows_backward(x, dy, mean, invstd, w, y_relu=y if tail else None, want_dresidual=res is not None)
    if tail == 2:
        y, dres = y + res, dy
    out = dict(y=y, mean=mean, invstd=invstd, rm=rm, rv=rv, dx=dx, dw=dw, db=db)
    if res is not None:
        out["dres"] = dres
    return out


@pytest.mark.parametrize("C,ld", WIDTHS)
@pytest.mark.parametrize("rows", ROWS)
def test_padded_norm_against_float64_and_the_dense_entries(gpu_ops, rows, C, ld):
    for tail, with_res in TAILS:
        i, ref = bn_padded_conditioned(rows, C, ld, tail, with_res)
        if tail:
            assert gate_margin(ref["pre"]) > 1e-4, "a ReLU gate could flip"
        assert bool(torch.isnan(i["x"][:, C:]).all()) and bool(torch.isnan(i["dy"][:, C:]).all())     # NaN in every padding column of the inputs
        got = _padded_step(gpu_ops, i)
        for name, g in got.items():
            r = ref[name]
            assert g.shape == r.shape, (tail, with_res, name)
            scale = float(r.abs().max())
            e = max_err(g, r)
            print(f"padded norm {rows} x {C} in {ld}, tail {tail}{' + residual' if with_res else ''}: {name} {e / scale:.3e}")
            assert e <= 1e-4 * scale, (tail, with_res, name, e, scale)
        for name in ("y", "dx", "dres"):                          # the padding: +0.0, whatever the inputs' padding held
            if name in got and ld > C:
                assert _plus_zero(got[name][:, C:]), (tail, with_res, name)
        dense = _dense_step(gpu_ops, i)
        for name, g in got.items():                               # the same expressions in the same order: the same bits
            assert torch.equal(g[:, :C] if g.dim() == 2 else g, dense[name]), (tail, with_res, name)


@pytest.mark.parametrize("C,ld", WIDTHS)
def test_padded_norm_dx_over_two_spread_rows(gpu_ops, C, ld):
    """Two rows whose values lie far apart (spread 1: var up to 1e6 eps), which the test above does not draw
    (``bn_padded_inputs``): dx = weight * invstd * (g1 - g2) / 2 * eps / (var + eps) is zero up to eps there, and the kernels -- like
    the dense entries, whose bits they share -- evaluate it as a difference of terms of size weight * invstd * |g|.  Its error is held
    to the rounding of those terms, 16 roundings of 2^-24 each.  It is NOT within 1e-4 of dx's own max-abs there: an MI355X gave up to
    1.9e-5 absolute where that is 1.8e-6 (64 in 64), 6.1e-6 against 3.3e-6 (12 in 32)."""
    for tail, with_res in TAILS:
        i, ref = bn_padded_conditioned(2, C, ld, tail, with_res, spread=1.0)
        got, r = _padded_step(gpu_ops, i)["dx"], ref["dx"]
        e, scale = max_err(got, r), float(r.abs().max())
        terms = 16 * 2.0 ** -24 * float((i["w"].double() * ref["invstd"]).abs().max()) * float(i["dy"][:, :C].abs().max())
        print(f"padded norm 2 x {C} in {ld}, spread 1, tail {tail}{' + residual' if with_res else ''}: dx err {e:.3e}, rounding of the "
              f"cancelling terms {terms:.3e}, max-abs {scale:.3e}")
        assert e <= terms, (tail, with_res, e, terms)
        if ld > C:
            assert _plus_zero(got[:, C:])


def test_padded_norm_nan_and_refusals(gpu_ops):
    from sgcdet_amd._abi import SgcError
    i, _ = bn_padded_conditioned(7, 12, 32, 2, True)
    i["x"][3, 5] = float("nan")
    got = _padded_step(gpu_ops, i)
    y = got["y"][:, :12]
    assert bool(torch.isnan(y[:, 5]).all()) and bool(torch.isfinite(y[:, [c for c in range(12) if c != 5]]).all())
    assert _plus_zero(got["y"][:, 12:]) and _plus_zero(got["dx"][:, 12:])
    dx = got["dx"][:, :12]
    assert bool(torch.isnan(dx[:, 5]).all()) and bool(torch.isfinite(dx[:, [c for c in range(12) if c != 5]]).all())
    # gates are selects: a NaN gradient behind a closed gate is dropped, behind an open one it stays
    i, ref = bn_padded_conditioned(7, 12, 32, 2, True)
    closed, opened = (ref["pre"] < 0).nonzero()[0].tolist(), (ref["pre"] > 0).nonzero()[0].tolist()
    i["dy"][closed[0], closed[1]] = float("nan")
    assert bool(torch.isfinite(_padded_step(gpu_ops, i)["dx"]).all())
    i["dy"][opened[0], opened[1]] = float("nan")
    dx = _padded_step(gpu_ops, i)["dx"][:, :12]
    assert bool(torch.isnan(dx[:, opened[1]]).all()) and bool(torch.isfinite(dx[:, [c for c in range(12) if c != opened[1]]]).all())
    x = torch.zeros(8, 32).cuda()
    v, ws = torch.zeros(32).cuda(), torch.zeros(4096).cuda()
    y = torch.full((8, 32), 7.0).cuda()
    fwd = lambda *a: gpu_ops._call("sgc_bn_rows_padded_forward", *a)       # noqa: E731
    for args, word in (((x, v, v, None, None, 0.1, 1e-5, None, 0, y, v, v, ws, 4096, 8, 12, 8), "pitch"),      # ld < C
                       ((x, v, v, None, None, 0.1, 1e-5, None, 0, y, v, v, ws, 4096, 8, 12, 30), "pitch"),     # ld % 4
                       ((x, v, v, None, None, 0.1, 1e-5, None, 0, y, v, v, ws, 4096, 8, 10, 32), "C %"),
                       ((x, v, v, None, None, 0.1, 1e-5, None, 3, y, v, v, ws, 4096, 8, 12, 32), "tail"),
                       ((x, v, v, None, None, 0.1, 1e-5, None, 2, y, v, v, ws, 4096, 8, 12, 32), "residual"),
                       ((x, v, v, None, None, 0.1, 1e-5, None, 0, y, v, v, ws, 4, 8, 12, 32), "workspace"),
                       ((x.view(-1)[1:], v, v, None, None, 0.1, 1e-5, None, 0, y, v, v, ws, 4096, 7, 12, 32), "aligned"),
                       ((x, v, v, None, None, 0.1, 1e-5, None, 0, y, v, v, ws, 4096, 0, 12, 32), "bad size")):
        with pytest.raises(SgcError, match=word):
            fwd(*args)
    bwd = lambda *a: gpu_ops._call("sgc_bn_rows_padded_backward", *a)      # noqa: E731
    for args, word in (((x, x, None, v, v, v, v, y, v, v, None, 1, ws, 4096, 8, 12, 32), "y is null"),
                       ((x, x, None, v, v, v, None, y, v, v, None, 2, ws, 4096, 8, 12, 32), "bias is null"),
                       ((x, x, None, v, v, v, v, y, v, v, None, 0, ws, 4096, 8, 12, 8), "pitch")):
        with pytest.raises(SgcError, match=word):
            bwd(*args)
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())                                 # nothing was launched


def test_dense_norm_backward_refuses_a_misaligned_weight(gpu_ops):
    """The dense entries are the padded kernels at ld == C, whose backward apply pass reads weight, dweight and dbias with 16-byte
    loads: ``sgc_bn_rows_act_backward`` with a weight pointer 4 bytes off is refused, and nothing is launched."""
    from sgcdet_amd._abi import SgcError
    x, ws = torch.zeros(8, 32).cuda(), torch.zeros(4096).cuda()
    v = torch.ones(36).cuda()
    dx, dw, db = torch.full((8, 32), 7.0).cuda(), torch.full((32,), 7.0).cuda(), torch.full((32,), 7.0).cuda()
    with pytest.raises(SgcError, match="aligned"):
        gpu_ops._call("sgc_bn_rows_act_backward", x, x, x, v[:32], v[:32], v[1:33], dx, dw, db, None, ws, 4096, 8, 32)
    torch.cuda.synchronize()
    assert bool((dx == 7.0).all()) and bool((dw == 7.0).all()) and bool((db == 7.0).all())      # nothing was launched


# ---- 2. the softmax backward -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [4, 12, 32, 128])
@pytest.mark.parametrize("rows", [1, 197, 4099])
def test_softmax_backward_against_float64(gpu_ops, rows, C):
    for ldg in sorted({C, _pad32(C)}):
        for ldp, lddp in ((C, C), (C + 4, _pad32(C) + 4)):
            i = softmax_inputs(rows, C, ldp, lddp, 100 * C + rows)
            want = softmax_reference(i, ldg)
            got = gpu_ops.softmax_rows_backward(i["p"].cuda(), i["dp"].cuda(), C=C, ldg=ldg)
            bound = (C + 4) * 2.0 ** -24 * float(i["dp"][:, :C].abs().max())
            e = max_err(got, want)
            print(f"softmax backward {rows} x {C}, pitches {ldp} {lddp} {ldg}: {e:.3e} of {bound:.3e}")
            assert got.shape == (rows, ldg) and e <= bound
            if ldg > C:
                assert _plus_zero(got[:, C:])
            if rows > 1:                                          # a NaN poisons its row and no other
                r = rows // 2
                i["dp"][r, C - 1] = float("nan")
                g2 = gpu_ops.softmax_rows_backward(i["p"].cuda(), i["dp"].cuda(), C=C, ldg=ldg)
                keep = torch.arange(rows) != r
                assert bool(torch.isnan(g2[r, :C]).all()) and torch.equal(g2[keep.cuda()], got[keep.cuda()])
                if ldg > C:
                    assert _plus_zero(g2[:, C:])


def test_softmax_backward_refusals(gpu_ops):
    from sgcdet_amd._abi import SgcError
    p, g = torch.zeros(4, 136).cuda(), torch.full((4, 136), 7.0).cuda()
    call = lambda *a: gpu_ops._call("sgc_softmax_rows_backward", *a)       # noqa: E731
    for args, word in (((p, p, g, 4, 132, 136, 136, 136), "C <= 128"), ((p, p, g, 4, 10, 136, 136, 136), "C %"), ((p, p, g, 4, 0, 136, 136, 136), "C %"),
                       ((p, p, g, 4, 12, 8, 136, 136), "below C"), ((p, p, g, 4, 12, 136, 136, 8), "below C"), ((p, p, g, 4, 12, 136, 134, 136), "pitches"),
                       ((p, p, g, 0, 12, 136, 136, 136), "bad size"), ((p.view(-1)[1:], p, g, 3, 12, 136, 136, 136), "aligned"),
                       ((None, p, g, 4, 12, 136, 136, 136), "null")):
        with pytest.raises(SgcError, match=word):
            call(*args)
    torch.cuda.synchronize()
    assert bool((g == 7.0).all())


# ---- 3. the Functions --------------------------------------------------------------------------------------------------------------
class _TorchConvolutions:
    """Counts the library convolutions torch runs while it is open."""

    def __init__(self, monkeypatch):
        self.n = 0
        for name in ("conv2d", "conv_transpose2d"):
            real = getattr(F, name)
            monkeypatch.setattr(F, name, self._counting(real))

    def _counting(self, real):
        def f(*a, **k):
            self.n += 1
            return real(*a, **k)
        return f


def _logged(ops, fn, names=None):
    ops.event_log, ops.event_names = [], names
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, [e[0] for e in ops.event_log]
    finally:
        ops.event_log = ops.event_names = None


@pytest.mark.parametrize("cin,cout", [(64, 32), (48, 24)])
@pytest.mark.parametrize("nhw", [(2, 3, 5), (2, 4, 6)])
def test_transposed_function_against_float64(gpu_ops, monkeypatch, nhw, cin, cout):
    from sgcdet_amd.functions import ConvTranspose2dRowsFunction
    N, H, W = nhw
    cin_p, cout_p = _pad32(cin), _pad32(cout)
    for kind in ("integers", "randn"):
        g = torch.Generator().manual_seed(1000 * H + cin)
        if kind == "integers":
            draw = lambda *s: torch.randint(-4, 5, s, generator=g).float()                       # noqa: E731
        else:
            draw = lambda *s: torch.randn(*s, generator=g)                                       # noqa: E731
        x, w, cot = draw(N * H * W, cin), draw(cin, cout, 3, 3), draw(N * 4 * H * W, cout)
        xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
        want = F.conv_transpose2d(xd.view(N, H, W, cin).permute(0, 3, 1, 2), wd, stride=2, padding=1, output_padding=1)
        want = want.permute(0, 2, 3, 1).reshape(-1, cout)
        (want * cot.double()).sum().backward()
        xg, wg = F.pad(x, (0, cin_p - cin)).cuda().requires_grad_(True), w.cuda().requires_grad_(True)
        counter = _TorchConvolutions(monkeypatch)

        def step():
            y = ConvTranspose2dRowsFunction.apply(xg, wg, nhw)
            (y * F.pad(cot, (0, cout_p - cout)).cuda()).sum().backward()
            return y
        y, names = _logged(gpu_ops, step)
        monkeypatch.undo()
        assert names.count("sgc_conv2d_wgrad_bf16x3") == 1 and counter.n == 0
        assert y.shape == (N * 4 * H * W, cout_p) and _plus_zero(y[:, cout:]) and _plus_zero(xg.grad[:, cin:])
        for name, got, ref in (("y", y[:, :cout], want), ("dx", xg.grad[:, :cin], xd.grad), ("dw", wg.grad, wd.grad)):
            assert got.shape == ref.shape, name
            if kind == "integers":
                assert float(ref.abs().max()) < 2 ** 24 and torch.equal(got.detach().cpu().double(), ref.detach()), (kind, name)
            else:
                e = max_err(got, ref) / float(ref.abs().max())
                _record(f"transposed/{name}", e)
                assert e <= 1e-4, (kind, name, e)


@pytest.mark.parametrize("cin,cout,k,stride", [(12, 24, 3, 2), (24, 24, 3, 1), (140, 280, 3, 2), (44, 88, 1, 1)])
def test_padded_convolution_function_against_float64(gpu_ops, monkeypatch, cin, cout, k, stride):
    from sgcdet_amd.functions import PaddedConv2dFunction
    N, H, W = 2, 6, 8
    OH, OW = (H + stride - 1) // stride, (W + stride - 1) // stride
    g = torch.Generator().manual_seed(cin + k)
    x, w, b = torch.randn(N * H * W, cin, generator=g), torch.randn(cout, cin, k, k, generator=g) / (k * cin ** 0.5), torch.randn(cout, generator=g)
    cot = torch.randn(N * OH * OW, cout, generator=g)
    xd, wd, bd = (t.double().requires_grad_(True) for t in (x, w, b))
    want = F.conv2d(xd.view(N, H, W, cin).permute(0, 3, 1, 2), wd, bd, stride=stride, padding=k // 2).permute(0, 2, 3, 1).reshape(-1, cout)
    (want * cot.double()).sum().backward()
    xg = F.pad(x, (0, _pad32(cin) - cin)).cuda().requires_grad_(True)
    wg, bg = w.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    counter = _TorchConvolutions(monkeypatch)

    def step():
        y = PaddedConv2dFunction.apply(xg, wg, bg, (N, H, W), stride)
        (y * F.pad(cot, (0, _pad32(cout) - cout)).cuda()).sum().backward()
        return y
    y, names = _logged(gpu_ops, step)
    monkeypatch.undo()
    assert names.count("sgc_conv2d_wgrad_bf16x3") == 1 and names.count("sgc_rows_colsum") == 1 and counter.n == 0
    assert y.shape == (N * OH * OW, _pad32(cout)) and _plus_zero(y[:, cout:]) and _plus_zero(xg.grad[:, cin:])
    for name, got, ref in (("y", y[:, :cout], want), ("dx", xg.grad[:, :cin], xd.grad), ("dw", wg.grad, wd.grad), ("db", bg.grad, bd.grad)):
        e = max_err(got, ref) / float(ref.abs().max())
        _record(f"padded_conv/{name}", e)
        assert got.shape == ref.shape and e <= 1e-4, (name, e)


def test_depth_reg_softmax_function_against_float64(gpu_ops, monkeypatch):
    from sgcdet_amd.functions import DepthRegSoftmaxFunction
    N, H, W, cin, D = 2, 4, 8, 140, 12
    g = torch.Generator().manual_seed(21)
    x, w, b = torch.randn(N * H * W, cin, generator=g), torch.randn(D, cin, 3, 3, generator=g) / (3 * cin ** 0.5), 0.3 * torch.randn(D, generator=g)
    cot = torch.randn(N * H * W, D, generator=g)
    xd, wd, bd = (t.double().requires_grad_(True) for t in (x, w, b))
    want = F.softmax(F.conv2d(xd.view(N, H, W, cin).permute(0, 3, 1, 2), wd, bd, padding=1), dim=1).permute(0, 2, 3, 1).reshape(-1, D)
    (want * cot.double()).sum().backward()
    xg = F.pad(x, (0, 160 - cin)).cuda().requires_grad_(True)
    wg, bg = w.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    counter = _TorchConvolutions(monkeypatch)

    def step():
        p = DepthRegSoftmaxFunction.apply(xg, wg, bg, (N, H, W))
        (p * cot.cuda()).sum().backward()
        return p
    p, names = _logged(gpu_ops, step)
    monkeypatch.undo()
    assert names.count("sgc_softmax_rows_backward") == 1 and names.count("sgc_conv2d_wgrad_bf16x3") == 1 and counter.n == 0
    assert p.shape == (N * H * W, D) and _plus_zero(xg.grad[:, cin:])
    for name, got, ref in (("p", p, want), ("dx", xg.grad[:, :cin], xd.grad), ("dw", wg.grad, wd.grad), ("db", bg.grad, bd.grad)):
        e = max_err(got, ref) / float(ref.abs().max())
        _record(f"depth_reg/{name}", e)
        assert got.shape == ref.shape and e <= 1e-4, (name, e)


# ---- 4. one SimpleUnet2D -----------------------------------------------------------------------------------------------------------
def _walk_with_gates(monkeypatch, rows, u, nhw):
    """``DepthNet_Fusion._unet`` over the training layers of ``u`` (the kernels on the GPU, torch on the CPU) -> (output rows, the ReLU
    gates of its six norms as [rows, C] masks: where relu(bn) is positive -- for the two skip stages the output minus the skip)."""
    from sgcdet_amd.plugin import conv_plan
    from sgcdet_amd.plugin.depth_net import DepthNet_Fusion, _unet_train_layers
    gates, real = [], conv_plan.bn_rows

    def spy(bn, y, grid, residual=None, relu=False, **k):
        out = real(bn, y, grid, residual=residual, relu=relu, **k)
        if "channels" not in k:                                   # the padded norm off the kernels calls bn_rows on the slice
            return out
        C = k["channels"]
        act = out.detach() - residual.detach() if k.get("relu_then_add") else out.detach()
        gates.append((act[:, :C] > 0).cpu())
        return out
    monkeypatch.setattr(conv_plan, "bn_rows", spy)
    try:
        return DepthNet_Fusion._unet(None, rows, _unet_train_layers(u), nhw), gates
    finally:
        monkeypatch.setattr(conv_plan, "bn_rows", real)


def _unet_case(c, seed):
    from sgcdet_amd.plugin.depth_net import SimpleUnet2D
    N, H, W = 2, 8, 12
    u = fill_by_name(SimpleUnet2D(c), base_seed=40 + c, scale=0.3).train()
    g = torch.Generator().manual_seed(seed)
    x, cot = torch.randn(N * H * W, c, generator=g), torch.randn(N * H * W, c, generator=g)
    return u, x, cot, (N, H, W)


def unet_against_float64(monkeypatch, c, seed):
    """-> (gates that differ, forward error, worst parameter-gradient error, the two nets) for one seed."""
    u, x, cot, nhw = _unet_case(c, seed)
    cp = _pad32(c)
    ref = copy.deepcopy(u).double()
    xr = F.pad(x.double(), (0, cp - c)).requires_grad_(True)
    want, gates_ref = _walk_with_gates(monkeypatch, xr, ref, nhw)
    (want[:, :c] * cot.double()).sum().backward()
    u = u.cuda()
    xg = F.pad(x, (0, cp - c)).cuda().requires_grad_(True)
    got, gates = _walk_with_gates(monkeypatch, xg, u, nhw)
    (got[:, :c] * cot.cuda()).sum().backward()
    assert len(gates) == len(gates_ref) == 6 and got.shape == want.shape and _plus_zero(got[:, c:])
    flips = sum(int((a != b).sum()) for a, b in zip(gates, gates_ref))
    fwd = max_err(got, want) / float(want.detach().abs().max())
    top = max(float(p.grad.abs().max()) for p in ref.parameters())
    worst = max_err(xg.grad[:, :c], xr.grad[:, :c]) / float(xr.grad.abs().max())
    for (n, p), (_, q) in zip(u.named_parameters(), ref.named_parameters()):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
        scale = float(q.grad.abs().max())
        worst = max(worst, max_err(p.grad, q.grad) / (scale if scale >= 1e-3 * top else top))
    return flips, fwd, worst, u, ref


@pytest.mark.parametrize("c", [12, 32, 44])
def test_unet_against_float64(gpu_ops, monkeypatch, c):
    ref64 = copy.deepcopy(_unet_case(c, 0)[0]).double()           # the walk on the CPU is the module
    probe = torch.randn(2, c, 8, 12, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    rows = F.pad(probe.permute(0, 2, 3, 1).reshape(-1, c), (0, _pad32(c) - c))
    walked, _ = _walk_with_gates(monkeypatch, rows, copy.deepcopy(ref64), (2, 8, 12))
    assert max_err(walked[:, :c], copy.deepcopy(ref64)(probe).permute(0, 2, 3, 1).reshape(-1, c)) <= 1e-11 * float(walked.abs().max())
    assert UNET_SEEDS[c] is not None, "no seed recorded"
    (flips, fwd, worst, u, ref), names = _logged(gpu_ops, lambda: unet_against_float64(monkeypatch, c, UNET_SEEDS[c]))
    print(f"unet c = {c}: {flips} gates differ from float64")
    assert flips == 0, "choose another seed: a ReLU gate flipped"
    assert names.count("sgc_bn_rows_padded_forward") == 6 and names.count("sgc_bn_rows_padded_backward") == 6
    assert names.count("sgc_conv2d_wgrad_bf16x3") == 6
    _record(f"unet_forward/{c}", fwd)
    _record(f"unet_param_grad/{c}", worst)
    for m, r in zip(u.modules(), ref.modules()):
        if isinstance(m, nn.BatchNorm2d):
            assert int(m.num_batches_tracked) == 1
            for stat in ("running_mean", "running_var"):
                assert max_err(getattr(m, stat), getattr(r, stat)) <= 1e-4 * float(getattr(r, stat).abs().max()), stat
    assert fwd <= MARGIN * MEASURED["unet_forward"][c] and worst <= MARGIN * MEASURED["unet_param_grad"][c]


# ---- 5. the module -----------------------------------------------------------------------------------------------------------------
NEW_KERNELS = {"sgc_conv2d_stem7_bf16x3", "sgc_conv2d_stem7_wgrad_bf16x3", "sgc_conv2d_wgrad_bf16x3", "sgc_bn_rows_act_forward",
               "sgc_bn_rows_padded_forward", "sgc_bn_rows_padded_backward", "sgc_softmax_rows_backward"}


def _module(seed):
    """The smallest size that runs: 8 x 8 maps, 32 x 32 images, and 4 views -- the plane sweep takes an even number of neighbours,
    and ``closest_frame_ids`` names a view beyond the sequence for fewer than four views with two neighbours each (two or three views
    cannot run the module at all); 16 rows at the coarsest stage."""
    import sgcdet_amd.plugin as P
    from sgcdet_amd.scene import make_img_meta
    net = P.DepthNet_Fusion(neighbor_img_num=2, downsample_factor=4, dbound=[0.2, 5.0, 0.4], mono_channels=32, loss_weight=0.5,
                            max_tol=0, init_weight="none")
    fill_by_name(net, base_seed=7, scale=0.15)
    g = torch.Generator().manual_seed(seed)
    xs, imgs = torch.randn(1, 4, 32, 8, 8, generator=g), torch.randn(1, 4, 3, 32, 32, generator=g)
    return net.cuda().train(), xs.cuda(), imgs.cuda(), make_img_meta(4, "scannet", seed=3, img_hw=(32, 32))


class _RowGates:
    """The U-Net gates of a switch-on forward, in the order and layout ``_UnetGates`` of tests/test_gpu_depth_net_train.py collects
    them from the norm modules: [N, C, H, W] masks of bn > 0, and ``mono_regulation``'s input."""

    def __init__(self, monkeypatch):
        from sgcdet_amd.plugin import conv_plan
        self.gates, self.real, self.mp, self.cp = [], conv_plan.bn_rows, monkeypatch, conv_plan
        monkeypatch.setattr(conv_plan, "bn_rows", self._spy)

    def _spy(self, bn, y, grid, residual=None, relu=False, **k):
        out = self.real(bn, y, grid, residual=residual, relu=relu, **k)
        if k.get("channels") is not None:
            act = out.detach() - residual.detach() if k.get("relu_then_add") else out.detach()
            self.gates.append((act.view(grid[0], grid[1], grid[2], -1)[..., :k["channels"]] > 0).permute(0, 3, 1, 2))
        return out

    def close(self):
        self.mp.setattr(self.cp, "bn_rows", self.real)


def module_step(ops, net, xs, imgs, meta, unets, monkeypatch):
    from test_gpu_depth_net_train import _UnetGates
    monkeypatch.setenv("SGC_DEPTH_NET_TRAIN_HIP", "1")
    if unets is None:
        monkeypatch.delenv("SGC_DEPTH_NET_TRAIN_UNETS", raising=False)
    else:
        monkeypatch.setenv("SGC_DEPTH_NET_TRAIN_UNETS", unets)
    gates = _RowGates(monkeypatch) if unets == "1" else _UnetGates(net)
    counter = _TorchConvolutions(monkeypatch)

    def step():
        net.zero_grad(set_to_none=True)
        pred = net(xs, imgs, [meta], 4)
        w = torch.linspace(-1, 1, pred.numel(), device=pred.device).view_as(pred)
        (pred * w).sum().backward()
        return pred
    try:
        pred, names = _logged(ops, step, NEW_KERNELS)
    finally:
        gates.close()
        monkeypatch.undo()
    g = [x for x in gates.gates]
    if unets != "1":                                              # drop mono_regulation's input: the hooks' seventh entry
        g = g[:6] + g[7:]
    return pred.detach(), {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None}, names, g, counter.n


def module_against_the_parent(ops, monkeypatch, seed):
    net, xs, imgs, meta = _module(seed)
    net_ref = copy.deepcopy(net)
    on = module_step(ops, net, xs, imgs, meta, "1", monkeypatch)
    off = module_step(ops, net_ref, xs, imgs, meta, None, monkeypatch)
    flips = sum(int((a != b).sum()) for a, b in zip(on[3], off[3]))
    return net, net_ref, on, off, flips, (xs, imgs, meta)


def test_depth_net_trains_its_unets_on_the_kernels(gpu_ops, monkeypatch):
    """4 views, 8 x 8 maps: with the switch on against SGC_DEPTH_NET_TRAIN_HIP=1 alone (the parent's formulation)."""
    from test_gpu_depth_net_train import _gradient_mismatches
    assert MODULE_SEED is not None, "no seed recorded"
    net, net_ref, on, off, flips, (xs, imgs, meta) = module_against_the_parent(gpu_ops, monkeypatch, MODULE_SEED)
    pred, grads, names, gates, n_torch = on
    pred_r, grads_r, names_r, gates_r, n_torch_r = off
    assert names.count("sgc_conv2d_wgrad_bf16x3") == 11 + 19     # the extractors' 11; 18 U-Net convolutions and depth_reg
    assert names.count("sgc_bn_rows_padded_forward") == 18 and names.count("sgc_bn_rows_padded_backward") == 18
    assert names.count("sgc_softmax_rows_backward") == 1 and names.count("sgc_bn_rows_act_forward") == 11
    assert n_torch == 0 and n_torch_r == 19                       # no library convolution is left
    assert names_r.count("sgc_conv2d_wgrad_bf16x3") == 11 and not any("padded" in n or "softmax" in n for n in names_r)
    assert set(grads) == set(grads_r) == {n for n, _ in net.named_parameters()}
    print(f"depth net: {flips} of {sum(a.numel() for a in gates)} U-Net gates differ between the two runs")
    assert len(gates) == len(gates_r) == 18 and flips == 0, "choose another MODULE_SEED: a ReLU gate flipped"
    bad = _gradient_mismatches(grads, grads_r)
    print("depth net gradient mismatches:", bad)
    assert not bad, bad
    bns_r = dict(net_ref.named_modules())
    for n, m in net.named_modules():
        if isinstance(m, nn.BatchNorm2d):
            assert int(m.num_batches_tracked) == 1 == int(bns_r[n].num_batches_tracked), n
            for stat in ("running_mean", "running_var"):
                a, b = getattr(m, stat), getattr(bns_r[n], stat)
                assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()), (n, stat)
    fwd = float((pred - pred_r).abs().max()) / float(pred_r.abs().max())
    _record("module_forward", fwd)
    assert pred.shape == pred_r.shape and fwd <= MARGIN * MEASURED["module_forward"]
    monkeypatch.setenv("SGC_DEPTH_NET_TRAIN_UNETS", "1")          # train mode without autograd: the same prediction
    with torch.no_grad():
        again, names2 = _logged(gpu_ops, lambda: net(xs, imgs, [meta], 4), NEW_KERNELS)
    assert names2.count("sgc_bn_rows_padded_forward") == 18 and float((again - pred).abs().max()) <= 1e-6 * float(pred.abs().max())


def test_switch_unset_is_the_parent(gpu_ops, monkeypatch):
    """Unset and "0": the launches of SGC_DEPTH_NET_TRAIN_HIP=1 alone, entry for entry, and its prediction."""
    net, xs, imgs, meta = _module(1)
    runs = [module_step(gpu_ops, copy.deepcopy(net), xs, imgs, meta, v, monkeypatch) for v in (None, "0")]
    assert runs[0][2] == runs[1][2]
    # torch's convolutions pick their algorithm per run: two runs of this one formulation differ by 1e-6 (measured: 9.8e-7 of 0.86);
    # the bound is the one tests/test_gpu_depth_net_train.py holds the two extractor formulations to
    assert float((runs[0][0] - runs[1][0]).abs().max()) < 1e-5
    assert runs[0][2].count("sgc_bn_rows_act_forward") == 11 and runs[0][2].count("sgc_conv2d_wgrad_bf16x3") == 11
    assert not any("padded" in n or "softmax" in n for n in runs[0][2]) and runs[0][4] == 19
