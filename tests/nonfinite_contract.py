"""Shared pieces of the non-finite tests (tests/test_nonfinite_cpu.py, tests/test_gpu_nonfinite.py; DESIGN.md "Non-finite values"):
the poison pattern, the class map and the two comparisons.  A reference here is NEVER the code under test: the oracle
(``oracle_ops``) where the operation has an oracle twin, else the float64 torch formulation its existing test uses.

exact    streaming and reduction kernels: the class (finite / NaN / +Inf / -Inf) of every element equals the reference's; the finite
         elements stay inside the bound of the kernel's existing test, taken over the finite reference elements only.
traced   MFMA kernels, every product mode.  F = the reference's non-finite set under a NaN poison = the set of outputs that read a
         poisoned input.  NaN poison: the kernel's non-finite set == F, all of it NaN.  +-Inf poison: reference's non-finite set for
         that input <= kernel's non-finite set <= F.  The two wider bounds, each for a structural reason:
           * the operand split computes lo = v - hi, which is Inf - Inf for an infinite v (csrc/mma.hpp): an Inf operand reaches the
             accumulator as NaN, so where the reference keeps +-Inf, or removes a -Inf in a ReLU, the kernel gives NaN.  It may never
             lose an infinity (superset of the reference's set) and never spread beyond the receptive field (subset of F);
           * Winograd F(2,3) along z mixes four input planes per output pair (2k, 2k + 1): F is widened to whole z pairs
             (``widen_z_pairs``) and the kernel's set must contain F and lie inside the widened F.
         Finite elements are bounded as in the exact comparison.
One exact comparison carries a wider bound too (``inf_as_nan``): the batch mean and the running mean of sgc_bn_rows_forward may be NaN
where the reference has an infinity, never finite -- the one-pass mean (Welford / Chan) meets Inf - Inf where the two-pass float64 mean
keeps the Inf.

Every comparison asserts its own preconditions: F is not empty, F covers less than half of the output, at least one finite element is
compared, and (Inf poison) the reference has an Inf that survives or one that a ReLU removed."""
import torch

FINITE, NAN, POS_INF, NEG_INF = 0, 1, 2, 3
KINDS = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}


def classes(t):
    """Per element: FINITE, NAN, POS_INF or NEG_INF (int8, on the CPU)."""
    t = t.detach().cpu()
    c = torch.zeros(t.shape, dtype=torch.int8)
    c[torch.isnan(t)] = NAN
    c[t == float("inf")] = POS_INF
    c[t == float("-inf")] = NEG_INF
    return c


def poison_sites(rows, C, image_rows=None, live=None):
    """The three (row, channel) sites of a rows tensor [rows, C] with ``image_rows`` rows per image (None: one image) and ``live``
    live channels (None: all): an interior row; the last row of image 0 (its last line, last column position: a border and, with more
    than one image, an image boundary); the very last row.  All in the last live channel.  Coinciding sites are listed once."""
    image_rows = rows if image_rows is None else image_rows
    c = (C if live is None else live) - 1
    if not (0 < image_rows <= rows and rows % image_rows == 0 and 0 <= c < C):
        raise ValueError(f"poison_sites: rows {rows}, image_rows {image_rows}, C {C}, live {live}")
    sites = []
    for r in (image_rows // 2, image_rows - 1, rows - 1):
        if (r, c) not in sites:
            sites.append((r, c))
    return sites


def poison(t, kind, image_rows=None, live=None, spread="row"):
    """A copy of the rows tensor ``t`` [rows, C] with ``KINDS[kind]`` at ``poison_sites``.  ``spread`` is the least the operation does
    with one poisoned element -- "element" (moves, pooling), "row" (a GEMM or a normalisation over the channels), "column" (a
    reduction over the rows) -- and the tensor is refused when these footprints alone would leave less than half of it untouched."""
    if t.dim() != 2:
        raise ValueError("poison: expects a rows tensor [rows, C]")
    rows, C = t.shape
    sites = poison_sites(rows, C, image_rows, live)
    touched = {"element": len(sites), "row": len({r for r, _ in sites}) * C, "column": len({c for _, c in sites}) * rows}[spread]
    if 2 * touched > t.numel():
        raise ValueError(f"poison: [{rows}, {C}] is too small: the {len(sites)} {spread} footprints cover {touched} of {t.numel()} elements")
    out = t.clone()
    for r, c in sites:
        out[r, c] = KINDS[kind]
    return out


def widen_z_pairs(F, grid):
    """A non-finite set F [X*Y*Z, C] (bool) widened to whole output z pairs (2k, 2k + 1) of ``grid`` = (X, Y, Z), Z even."""
    X, Y, Z = grid
    if Z % 2 or F.shape[0] != X * Y * Z:
        raise ValueError("widen_z_pairs: needs an even Z and F of [X*Y*Z, C]")
    pairs = F.view(X, Y, Z // 2, 2, -1).any(3, keepdim=True)
    return pairs.expand(X, Y, Z // 2, 2, F.shape[1]).reshape(F.shape)


def _finite_bound(got, ref, tol, what, unit_floor=True):
    """max |got - ref| over the elements finite in both <= tol * max(1, max |ref| over its finite elements); at least one compared.
    ``unit_floor`` False: the existing test of the kernel scales by max |ref| alone, and so does this."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    both = torch.isfinite(got) & torch.isfinite(ref)
    assert bool(both.any()), f"{what}: no finite element to compare"
    scale = float(ref[torch.isfinite(ref)].abs().max())
    scale = max(1.0, scale) if unit_floor else scale
    err = float((got[both] - ref[both]).abs().max())
    print(f"{what}: finite elements {int(both.sum())} of {ref.numel()}, max|err| {err:.3e}, scale {scale:.3e}, bound {tol * scale:.3e}")
    assert err <= tol * scale, f"{what}: finite elements off by {err:.3e} > {tol:.1e} * {scale:.3e}"


def _check_F(F, what):
    assert bool(F.any()), f"{what}: precondition: the reference's non-finite set is empty -- the poison reached nothing"
    assert 2 * int(F.sum()) < F.numel(), f"{what}: precondition: the non-finite set covers {int(F.sum())} of {F.numel()} outputs (>= half)"


def compare_exact(got, ref, tol, what, bit_equal=False, need_nonfinite=True, unit_floor=True, inf_as_nan=False):
    """Class for class against ``ref``; finite elements within ``tol`` of the finite reference scale (``bit_equal``: a pure move,
    the finite elements are equal).  ``need_nonfinite`` False: a secondary output that the poison may legitimately not reach.
    ``inf_as_nan``: the wider bound of the batch statistics -- a NaN is accepted where the reference has an infinity, never a finite
    value (a one-pass running mean meets Inf - Inf where the two-pass float64 mean keeps the Inf; see the module docstring)."""
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} != {tuple(ref.shape)}"
    cg, cr = classes(got), classes(ref)
    if need_nonfinite:
        _check_F(cr != FINITE, what)
    bad = cg != cr
    if inf_as_nan:
        bad &= ~((cg == NAN) & ((cr == POS_INF) | (cr == NEG_INF)))
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} elements of another class than the reference's; first at "
                                 f"{tuple(int(i) for i in bad.nonzero()[0])}: got class {int(cg[bad][0])}, reference {int(cr[bad][0])}")
    if bit_equal:
        fin = cr == FINITE
        assert bool(fin.any()), f"{what}: no finite element to compare"
        assert torch.equal(got.detach().cpu()[fin], ref.detach().cpu()[fin].to(got.dtype)), f"{what}: a move changed a finite value"
    else:
        _finite_bound(got, ref, tol, what, unit_floor)


def compare_traced(got, ref_nan, tol, what, kind="nan", ref_kind=None, z_pair_grid=None, unit_floor=True):
    """The traced comparison of ``got`` (the kernel under a ``kind`` poison).  ``ref_nan``: the reference under the NaN poison (defines
    F); ``ref_kind``: the reference under the same poison as ``got`` (None for kind "nan": it is ``ref_nan``).  ``z_pair_grid``:
    the Winograd-z entry's grid (X, Y, Z)."""
    assert got.shape == ref_nan.shape, f"{what}: shape {tuple(got.shape)} != {tuple(ref_nan.shape)}"
    cr = classes(ref_nan)
    F = cr != FINITE
    _check_F(F, what)
    assert bool((cr[F] == NAN).all()), f"{what}: precondition: the reference turns a NaN poison into an infinity"
    outer = F if z_pair_grid is None else widen_z_pairs(F, z_pair_grid)
    if z_pair_grid is not None:
        assert 2 * int(outer.sum()) < outer.numel(), f"{what}: precondition: the widened set covers {int(outer.sum())} of {outer.numel()}"
    cg = classes(got)
    G = cg != FINITE
    if kind == "nan":
        ref, inner = ref_nan, F
        assert bool((cg[G] == NAN).all()), f"{what}: a NaN poison came out as an infinity"
    else:
        assert ref_kind is not None and ref_kind.shape == ref_nan.shape
        ref, ck = ref_kind, classes(ref_kind)
        inner = ck != FINITE
        assert not bool((inner & ~F).any()), f"{what}: precondition: the reference's {kind} set leaves its NaN set"
        survives = bool(((ck == POS_INF) | (ck == NEG_INF)).any())
        removed = bool((F & ~inner).any())                         # read the poison, came out finite: a ReLU took a -Inf (or +Inf * negative)
        assert survives or removed, f"{what}: precondition: no infinity survives in the reference and no ReLU removes one"
    lost, spread = inner & ~G, G & ~outer
    assert not bool(lost.any()), (f"{what}: {int(lost.sum())} outputs that read the poison came out finite; first at "
                                  f"{tuple(int(i) for i in lost.nonzero()[0])}")
    assert not bool(spread.any()), (f"{what}: {int(spread.sum())} outputs outside the receptive field are non-finite; first at "
                                    f"{tuple(int(i) for i in spread.nonzero()[0])}")
    if kind == "nan" and z_pair_grid is None:
        assert torch.equal(G, F)
    _finite_bound(got, ref, tol, what, unit_floor)
    return dict(F=int(F.sum()), got=int(G.sum()), total=F.numel())


# ---- seeded cases shared by the CPU file (oracle against float64 torch) and the GPU file (kernel against the oracle) ----------------
def _relu_mode(relu):
    return 2 if relu == 2 else int(bool(relu))


def conv3d_inputs(case, kind, where="x"):
    """A row of ``CASES`` of tests/test_gpu_conv3d.py (Cin, Cout, grid, ksize, stride, transposed, residual, relu) with the poison in
    ``where``: "x" (the three sites), "residual" (the three elements) or "shift" (its last element: one output column)."""
    Cin, Cout, grid, k, s, tr, use_res, relu = case
    g = torch.Generator().manual_seed(sum(grid) + Cin + Cout + k + s)
    V = grid[0] * grid[1] * grid[2]
    taps = 8 if tr else k ** 3
    x = torch.randn(V, Cin, generator=g)
    wt = torch.randn(taps, Cout, Cin, generator=g) * (1.0 / (taps * Cin) ** 0.5)
    sc, sh = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g)
    pad = 0 if k == 2 else k // 2
    og = tuple(2 * d for d in grid) if tr else tuple((d + 2 * pad - k) // s + 1 for d in grid)
    res = torch.randn(og[0] * og[1] * og[2], Cout, generator=g) if use_res else None
    if where == "x":
        x = poison(x, kind)
    elif where == "residual":
        res = poison(res, kind, spread="element")
    elif where == "shift":
        sh[Cout - 1] = KINDS[kind]
    else:
        raise ValueError(where)
    return dict(x=x, wt=wt, grid=grid, k=k, s=s, tr=tr, sc=sc, sh=sh, res=res, relu=_relu_mode(relu), og=og)


def epilogue64(y, sc, sh, res, relu):
    """The library's epilogue in float64: y * scale + shift; relu mode 2: relu(.) + residual; mode 1: relu(. + residual)."""
    if sc is not None:
        y = y * sc.double()
    if sh is not None:
        y = y + sh.double()
    if relu == 2:
        y = y.clamp_min(0)
    if res is not None:
        y = y + res.double()
    if relu == 1:
        y = y.clamp_min(0)
    return y


def conv3d_torch64(i):
    """float64 torch formulation of ``conv3d_inputs`` (the weight layouts of tests/test_oracle_conv.py)."""
    import torch.nn.functional as F
    Cin, Cout, k = i["x"].shape[1], i["wt"].shape[1], i["k"]
    x = i["x"].double().view(*i["grid"], Cin).permute(3, 0, 1, 2).unsqueeze(0)
    if i["tr"]:
        y = F.conv_transpose3d(x, i["wt"].double().view(2, 2, 2, Cout, Cin).permute(4, 3, 0, 1, 2), None, 2)
    else:
        y = F.conv3d(x, i["wt"].double().view(k, k, k, Cout, Cin).permute(3, 4, 0, 1, 2), None, i["s"], 0 if k == 2 else k // 2)
    assert tuple(y.shape[2:]) == tuple(i["og"])
    return epilogue64(y[0].permute(1, 2, 3, 0).reshape(-1, Cout), i["sc"], i["sh"], i["res"], i["relu"])


def conv2d_inputs(nhw, cin, cout, k, relu, use_res, kind, where="x"):
    """sgc_conv2d_nhwc_bf16x3 (tests/test_gpu_conv3d.py): images of H*W rows each."""
    N, H, W = nhw
    g = torch.Generator().manual_seed(N * H + cin + cout)
    x = torch.randn(N * H * W, cin, generator=g)
    wt = (torch.randn(cout, cin, k, k, generator=g) * 0.05).permute(2, 3, 0, 1).reshape(k * k, cout, cin).contiguous()
    sc, sh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    res = torch.randn(N * H * W, cout, generator=g) if use_res else None
    if where == "x":
        x = poison(x, kind, image_rows=H * W)
    elif where == "residual":
        res = poison(res, kind, image_rows=H * W, spread="element")
    elif where == "shift":
        sh[cout - 1] = KINDS[kind]
    else:
        raise ValueError(where)
    return dict(x=x, wt=wt, nhw=nhw, k=k, sc=sc, sh=sh, res=res, relu=_relu_mode(relu))


def conv2d_torch64(i):
    import torch.nn.functional as F
    (N, H, W), k = i["nhw"], i["k"]
    cin, cout = i["x"].shape[1], i["wt"].shape[1]
    y = F.conv2d(i["x"].double().view(N, H, W, cin).permute(0, 3, 1, 2), i["wt"].double().view(k, k, cout, cin).permute(2, 3, 0, 1), None, 1, k // 2)
    return epilogue64(y.permute(0, 2, 3, 1).reshape(-1, cout), i["sc"], i["sh"], i["res"], i["relu"])


def bn_inputs(rows, C, kind, where):
    """tests/test_gpu_kernels.py's BatchNorm case; ``where``: "x", "residual" (forward), "dy" (backward) or None (no poison)."""
    # the seed offset was chosen on the CPU (float64 torch alone): at (77, 1040) the fused tail's output is 0 at one poison site and
    # positive at the other, at (6, 4) positive at both -- the ReLU gate of the backward both removes and passes a poisoned dy
    g = torch.Generator().manual_seed(rows + C + 3)
    d = dict(x=torch.randn(rows, C, generator=g) * 1.5 + 3.0, w=torch.rand(C, generator=g) + 0.5, b=torch.randn(C, generator=g),
             rm=torch.randn(C, generator=g), rv=torch.rand(C, generator=g) + 0.5, res=torch.randn(rows, C, generator=g),
             dy=torch.randn(rows, C, generator=g))
    if where == "x":
        d["x"] = poison(d["x"], kind, spread="column")
    elif where == "residual":
        d["res"] = poison(d["res"], kind, spread="element")
    elif where == "dy":
        d["dy"] = poison(d["dy"], kind, spread="column")
    elif where is not None:
        raise ValueError(where)
    return d


def bn_torch64(d, tail, momentum=0.1, eps=1e-5):
    """F.batch_norm (+ residual, relu with ``tail``) in float64 with autograd -> dict(y, mean, invstd, rm, rv, dx, dw, db, dres)."""
    import torch.nn.functional as F
    x, w, b = (d[k].double().requires_grad_(True) for k in ("x", "w", "b"))
    res = d["res"].double().requires_grad_(True)
    rm, rv = d["rm"].double().clone(), d["rv"].double().clone()
    y = F.batch_norm(x, rm, rv, w, b, True, momentum, eps)
    if tail:
        y = torch.relu(y + res)
    y.backward(d["dy"].double())
    xd = x.detach()
    return dict(y=y.detach(), mean=xd.mean(0), invstd=1 / (xd.var(0, unbiased=False) + eps).sqrt(), rm=rm, rv=rv, dx=x.grad, dw=w.grad,
                db=b.grad, dres=res.grad if tail else None)


def bn_run(ops, d, tail, dev="cpu", momentum=0.1, eps=1e-5):
    """The same through ``ops`` (the oracle on the CPU, the kernels on the GPU)."""
    t = {k: v.to(dev) for k, v in d.items()}
    rm, rv = t["rm"].clone(), t["rv"].clone()
    y, mean, invstd = ops.bn_rows_forward(t["x"], t["w"], t["b"], rm, rv, momentum=momentum, eps=eps, residual=t["res"] if tail else None, relu=tail)
    if tail:
        dx, dw, db, dres = ops.bn_rows_backward(t["x"], t["dy"], mean, invstd, t["w"], y_relu=y, want_dresidual=True)
    else:
        (dx, dw, db), dres = ops.bn_rows_backward(t["x"], t["dy"], mean, invstd, t["w"]), None
    return dict(y=y, mean=mean, invstd=invstd, rm=rm, rv=rv, dx=dx, dw=dw, db=db, dres=dres)
