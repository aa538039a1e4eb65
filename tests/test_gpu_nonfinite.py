"""Non-finite values through the HIP kernels (tests/nonfinite_contract.py, DESIGN.md "Non-finite values"): one poisoned launch per
case, compared with a reference that is never the code under test -- the oracle where the operation has a twin, else the float64
torch formulation of the kernel's existing test.  Streaming and reduction kernels are held to the exact comparison (every element's
class equals the reference's), the MFMA kernels to the traced one (the set of outputs that turn non-finite is the set that read the
poison: a NaN works as an exact tracer of data flow -- a tile that reads across an image boundary, a row that wraps at W, a padding
done as clamp-and-mask and an unhandled tile tail all show as a set that differs from the reference's).  Shapes and bounds are those of
the existing parametrisations of each kernel.

Left out on purpose: the deformable-gather, plane-sweep and attention kernels (dfa3d_*, pairs_*, plane_sweep_*, view_attend*).
Their reference semantics are the reference project's CUDA kernels, not torch, and their edge behaviour has contract tests of its own
(tests/gather_edge_contract.py; tests/plane_sweep_edge_contract.py, which places pz == 0, +-inf, NaN and huge positions)."""
import pytest
import torch
import torch.nn.functional as F

import nonfinite_contract as nf
from nonfinite_contract import FINITE, KINDS as VALUES

pytestmark = pytest.mark.gpu
KINDS = ("nan", "+inf", "-inf")


def _cu(t):
    return t.cuda() if isinstance(t, torch.Tensor) else t


def _traced(what, build, run_ref, run_gpu, tol, kinds=KINDS, z_pair_grid=None, unit_floor=True):
    """``build(kind)`` -> the poisoned inputs (CPU); ``run_ref`` / ``run_gpu``: inputs -> output rows."""
    ref_nan = run_ref(build("nan"))
    for kind in kinds:
        inp = build(kind)
        ref_kind = ref_nan if kind == "nan" else run_ref(inp)
        nf.compare_traced(run_gpu(inp), ref_nan, tol, f"{what}, {kind}", kind, ref_kind, z_pair_grid, unit_floor)


def _rows_to_nchw(rows, N, H, W):
    return rows.view(N, H, W, -1).permute(0, 3, 1, 2).contiguous()


# ======================================================================================================================================
# exact comparison: streaming and reduction kernels
# ======================================================================================================================================
BN_OUTPUTS = ("y", "mean", "invstd", "rm", "rv", "dx", "dw", "db", "dres")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("tail", [False, True], ids=["plain", "residual_relu"])
@pytest.mark.parametrize("rows,C", [(77, 1040), (6, 4)])
def test_bn_rows_forward_and_backward(rows, C, tail, kind, oracle_ops, gpu_ops):
    """sgc_bn_rows_forward / _backward and the fused tail y = relu(bn(x) + residual): poison in x, in the residual (forward) and in dy
    (backward); output, batch and running statistics and every gradient against the oracle (which tests/test_nonfinite_cpu.py pins to
    F.batch_norm in float64), bound 2e-4 of the scale as in tests/test_gpu_kernels.py."""
    for where in ("x", "dy") + (("residual",) if tail else ()):
        d = nf.bn_inputs(rows, C, kind, where)
        ref = nf.bn_run(oracle_ops, d, tail)
        got = nf.bn_run(gpu_ops, d, tail, "cuda")
        reached = False
        for name in BN_OUTPUTS:
            if ref[name] is None:
                continue
            hit = bool((nf.classes(ref[name]) != FINITE).any())
            reached |= hit
            # the one-pass mean (Welford / Chan, csrc/batch_norm.hip) meets Inf - Inf where the two-pass float64 mean keeps the infinity:
            # the batch mean and the running mean may be NaN there, never finite (the wider bound of DESIGN.md "Non-finite values")
            nf.compare_exact(got[name], ref[name], 2e-4, f"bn_rows {rows}x{C} {kind} in {where}: {name}", need_nonfinite=hit,
                             inf_as_nan=name in ("mean", "rm"))
        assert reached or kind != "nan", f"{where}: the poison reached no output of the reference"


@pytest.mark.parametrize("kind", KINDS)
def test_layer_norm_rows(kind, oracle_ops, gpu_ops):
    rows, C = 100, 96
    g = torch.Generator().manual_seed(rows + C)
    x = nf.poison(torch.randn(rows, C, generator=g) * 3 + 0.7, kind)
    w, b = torch.randn(C, generator=g), torch.randn(C, generator=g)
    want = F.layer_norm(x.double(), (C,), w.double(), b.double(), 1e-5)
    nf.compare_exact(gpu_ops.layer_norm_rows(x.cuda(), w.cuda(), b.cuda(), 1e-5), want, 2e-6, f"layer_norm_rows {kind}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nhwc", [(2, 7, 10, 64), (1, 1, 1, 4)])
def test_maxpool_keeps_nan(nhwc, kind, gpu_ops):
    """csrc/maxpool2d.hip's header says a NaN in a window gives NaN, as F.max_pool2d does: here is its test.  Bit equality on the
    finite elements, as in tests/test_gpu_resnet.py."""
    N, H, W, C = nhwc
    g = torch.Generator().manual_seed(H * 100 + W)
    x = nf.poison(torch.randn(N * H * W, C, generator=g), kind, image_rows=H * W, spread="element")
    got, onhw = gpu_ops.maxpool2d_nhwc(x.cuda(), (N, H, W))
    want = F.max_pool2d(_rows_to_nchw(x, N, H, W), 3, 2, 1).permute(0, 2, 3, 1).reshape(-1, C)
    nf.compare_exact(got, want, 0.0, f"maxpool {nhwc} {kind}", bit_equal=True, need_nonfinite=kind != "-inf")    # a -Inf loses every maximum
    if kind == "-inf" and H > 1:
        assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fine_hw,coarse_hw", [((3, 4), (2, 2)), ((1, 1), (1, 1))])
def test_upsample_nearest_add_and_its_backward(fine_hw, coarse_hw, kind, gpu_ops):
    """The two smallest pairs of _TOP_DOWN (tests/test_gpu_fpn_train.py): index-and-add, and the float64 autograd of F.interpolate for
    the backward (1e-6 of the max-abs)."""
    from sgcdet_amd.plugin.fpn import _nearest_index
    N, (Hd, Wd), (Hs, Ws), C = 2, fine_hw, coarse_hw, 32
    g = torch.Generator().manual_seed(Hd * 100 + Wd + C)
    fine, coarse = torch.randn(N * Hd * Wd, C, generator=g), torch.randn(N * Hs * Ws, C, generator=g)
    ih, iw = _nearest_index(Hd, Hs, "cpu"), _nearest_index(Wd, Ws, "cpu")
    for where in ("fine", "coarse"):
        f = nf.poison(fine, kind, image_rows=Hd * Wd, spread="element") if where == "fine" else fine
        c = nf.poison(coarse, kind, image_rows=Hs * Ws, spread="element") if where == "coarse" else coarse
        want = (f.view(N, Hd, Wd, C) + c.view(N, Hs, Ws, C)[:, ih][:, :, iw]).view(-1, C)
        got = gpu_ops.upsample_nearest_add_nhwc(f.cuda(), c.cuda(), (N, Hd, Wd), (N, Hs, Ws))
        nf.compare_exact(got, want, 0.0, f"upsample_nearest_add {kind} in {where}", bit_equal=True)
    gout = nf.poison(torch.randn(N * Hd * Wd, C, generator=g), kind, image_rows=Hd * Wd, spread="element")
    z = torch.zeros(N, C, Hs, Ws, dtype=torch.float64, requires_grad=True)
    want, = torch.autograd.grad(F.interpolate(z, size=(Hd, Wd), mode="nearest"), z, _rows_to_nchw(gout.double(), N, Hd, Wd))
    got = gpu_ops.upsample_nearest_add_backward_nhwc(gout.cuda(), (N, Hd, Wd), (N, Hs, Ws))
    nf.compare_exact(got, want.permute(0, 2, 3, 1).reshape(-1, C), 1e-6, f"upsample_nearest_add_backward {kind}", unit_floor=False)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rows,C", [(63, 36), (257, 32)])
def test_rows_colsum(rows, C, kind, gpu_ops):
    """One workgroup row (63) and the workspace form (257) against x.sum(0) in float64; finite columns within the chain bound of
    tests/test_gpu_fpn_train.py (160 * 2^-24 of the column's sum of magnitudes)."""
    x = nf.poison(torch.randn(rows, C, generator=torch.Generator().manual_seed(rows + C)), kind, spread="column")
    got, want = gpu_ops.rows_colsum(x.cuda()).cpu(), x.double().sum(0)
    cg, cr = nf.classes(got), nf.classes(want)
    assert bool((cr != FINITE).any()) and 2 * int((cr != FINITE).sum()) < C and torch.equal(cg, cr), (cg.tolist(), cr.tolist())
    fin = cr == FINITE
    ratio = ((got.double()[fin] - want[fin]).abs() / (2.0 ** -24 * x.double().abs().sum(0)[fin])).max().item()
    print(f"rows_colsum {rows}x{C} {kind}: worst finite column {ratio:.3f} x 2^-24 x sum|x|")
    assert ratio <= 160


@pytest.mark.parametrize("kind", KINDS)
def test_upsample2x_occ_and_backward(kind, oracle_ops, gpu_ops):
    C, grid = 32, (3, 4, 2)
    g = torch.Generator().manual_seed(C)
    V = grid[0] * grid[1] * grid[2]
    vol = nf.poison(torch.randn(V, C, generator=g), kind, spread="element")
    w, b = torch.randn(C, generator=g) * 0.1, torch.randn(1, generator=g)
    up_c, occ_c, _ = oracle_ops.upsample2x_occ(vol, grid, w, b)
    up_g, occ_g, _ = gpu_ops.upsample2x_occ(vol.cuda(), grid, w.cuda(), b.cuda())
    nf.compare_exact(up_g, up_c, 1e-6, f"upsample2x {kind}")
    nf.compare_exact(occ_g, occ_c, 2e-6, f"upsample2x occupancy {kind}", need_nonfinite=False)       # up to 2 x 27 of 192 voxels ...
    assert bool((nf.classes(occ_c) != FINITE).any()) and int((nf.classes(occ_c) != FINITE).sum()) < occ_c.numel()    # ... read the poison
    go = torch.randn(8 * V, 3, generator=g)
    go = nf.poison(go, kind, spread="element").view(2 * grid[0], 2 * grid[1], 2 * grid[2], 3).permute(3, 0, 1, 2)[None].contiguous()
    nf.compare_exact(gpu_ops.upsample2x_backward(go.cuda()), oracle_ops.upsample2x_backward(go), 1e-5, f"upsample2x_backward {kind}")


@pytest.mark.parametrize("kind", KINDS)
def test_scatter_rows_scatter_add_rows_and_view_mean(kind, oracle_ops, gpu_ops):
    from count_contract import _scene
    N, Nq, C = 6, 700, 32
    ref3d, origin, proj = _scene(N, Nq, 4)
    _, mk = oracle_ops.project_points(ref3d, origin, proj, 320., 239., 0.2, 5.0)
    pc = oracle_ops.compact_pairs(mk)
    n_pairs, n_valid = int(pc["totals"][0]), int(pc["totals"][1])
    g = torch.Generator().manual_seed(11)
    feat = nf.poison(torch.randn(n_pairs, C, generator=g), kind, spread="element")
    want = oracle_ops.view_mean(feat, pc["slot"], pc["valid_index"], n_valid)
    got = gpu_ops.view_mean(feat.cuda(), pc["slot"].cuda(), pc["valid_index"].cuda(), n_valid)
    nf.compare_exact(got, want, 1e-5, f"view_mean {kind}")
    rows = nf.poison(torch.randn(n_valid, C, generator=g), kind, spread="element")
    idx = pc["valid_index"][:n_valid].contiguous()
    want = oracle_ops.scatter_rows(rows, idx, torch.zeros(Nq, C))
    got = gpu_ops.scatter_rows(rows.cuda(), idx.cuda(), torch.zeros(Nq, C).cuda())
    nf.compare_exact(got, want, 0.0, f"scatter_rows {kind}", bit_equal=True)
    base = torch.randn(Nq, C, generator=g)
    idx64 = torch.randperm(Nq, generator=g)[:n_valid].sort().values
    want = oracle_ops.scatter_add_rows(rows, idx64, base.clone())
    got = gpu_ops.scatter_add_rows(rows.cuda(), idx64.cuda(), base.clone().cuda())
    nf.compare_exact(got, want, 1e-6, f"scatter_add_rows {kind}")


@pytest.mark.parametrize("kind", KINDS)
def test_layout_moves_are_bit_exact_on_the_class_map(kind, oracle_ops, gpu_ops):
    """nchw_to_nhwc_crop, nhwc_to_nchw_pad (the rows transpose and its adjoint) and nchw_to_nhwc_padc: pure moves -- the class map and
    the finite bits equal the reference's (the oracle twins; a torch permute / pad for padc, which has no twin)."""
    N, C, Hs, Ws, H, W = 2, 40, 17, 23, 15, 20
    g = torch.Generator().manual_seed(N * C + H)
    src = _rows_to_nchw(nf.poison(torch.randn(N * Hs * Ws, C, generator=g), kind, image_rows=Hs * Ws, spread="element"), N, Hs, Ws)
    src[0, C - 1, H - 1, W - 1] = VALUES[kind]                  # the last pixel INSIDE the crop (the three sites above lie in or behind it)
    nf.compare_exact(gpu_ops.nchw_to_nhwc_crop(src.cuda(), H, W), oracle_ops.nchw_to_nhwc_crop(src, H, W), 0.0, f"nchw_to_nhwc_crop {kind}",
                     bit_equal=True)
    rows = nf.poison(torch.randn(N * H * W, C, generator=g), kind, image_rows=H * W, spread="element").view(N, H * W, C)
    nf.compare_exact(gpu_ops.nhwc_to_nchw_pad(rows.cuda(), H, W, Hs, Ws), oracle_ops.nhwc_to_nchw_pad(rows, H, W, Hs, Ws), 0.0,
                     f"nhwc_to_nchw_pad {kind}", bit_equal=True)
    img = _rows_to_nchw(nf.poison(torch.randn(N * H * W, 3, generator=g), kind, image_rows=H * W, spread="element"), N, H, W)
    want = F.pad(img.permute(0, 2, 3, 1).reshape(-1, 3), (0, 5))
    nf.compare_exact(gpu_ops.nchw_to_nhwc_padc(img.cuda(), 8), want, 0.0, f"nchw_to_nhwc_padc {kind}", bit_equal=True)


# ======================================================================================================================================
# traced comparison: MFMA kernels
# ======================================================================================================================================
CONV3D = [  # rows of CASES in tests/test_gpu_conv3d.py: Cin, Cout, grid, ksize, stride, transposed, residual, relu
    (32, 128, (10, 10, 4), 3, 1, False, True, True),      # single-pass, fused epilogue
    (64, 128, (8, 6, 4), 3, 2, False, False, True),       # stride 2
    (64, 256, (5, 5, 2), 3, 1, False, True, True),        # split-K + epilogue kernel
    (32, 32, (7, 5, 3), 3, 1, False, False, False),       # narrow tile
    (64, 128, (5, 4, 3), 2, 2, True, False, True),        # ConvTranspose3d k2 s2
    (64, 128, (9, 7, 4), 3, 1, False, True, 2),           # decoder epilogue: relu(t) + skip
    (64, 128, (16, 16, 16), 3, 1, False, True, True),     # halo bricks 4x4x16
    (64, 192, (17, 13, 16), 3, 1, False, True, True),     # partial halo bricks, Cout % 128 != 0
    (64, 512, (10, 10, 4), 3, 1, False, True, True),      # whole-grid brick
]


def _conv3d_ref(oracle_ops):
    def run(i):
        hi, lo = oracle_ops.split_bf16(i["wt"])
        return oracle_ops.conv3d_cl_bf16x3(i["x"], hi, lo, i["grid"], i["k"], i["s"], i["tr"], i["sc"], i["sh"], i["res"], i["relu"])[0]
    return run


def _conv3d_gpu(gpu_ops, split=None, **kw):
    def run(i):
        hi, lo = (split or gpu_ops.split_bf16)(i["wt"].cuda())
        return gpu_ops.conv3d_cl_bf16x3(i["x"].cuda(), hi, lo, i["grid"], i["k"], i["s"], i["tr"], i["sc"].cuda(), i["sh"].cuda(), _cu(i["res"]),
                                        i["relu"], **kw)[0]
    return run


@pytest.mark.parametrize("case", CONV3D, ids=lambda c: f"{c[0]}-{c[1]}-{'x'.join(map(str, c[2]))}-k{c[3]}s{c[4]}{'t' if c[5] else ''}-relu{int(c[7])}")
def test_conv3d_cl_bf16x3(case, oracle_ops, gpu_ops):
    """The three sites in x under every kind; one NaN in shift (that whole column) and, with a residual, the three elements of it
    (exactly those).  Bound of tests/test_gpu_conv3d.py: 1e-4 of the scale against the oracle."""
    ref, gpu = _conv3d_ref(oracle_ops), _conv3d_gpu(gpu_ops)
    _traced(f"conv3d {case} in x", lambda kind: nf.conv3d_inputs(case, kind, "x"), ref, gpu, 1e-4)
    small = case[2][0] * case[2][1] * case[2][2] <= 1000            # the epilogue is the same code on the large grids: keep those cases quick
    for where in (("shift", "residual") if case[6] else ("shift",)) if small else ():
        _traced(f"conv3d {case} in {where}", lambda kind: nf.conv3d_inputs(case, kind, where), ref, gpu, 1e-4)
    if small:
        i = nf.conv3d_inputs(case, "nan", "shift")
        bad = nf.classes(gpu(i)) != FINITE
        assert bool(bad[:, case[1] - 1].all()) and int(bad.sum()) == bad.shape[0]                 # that whole column, nothing else
        if case[6]:
            i = nf.conv3d_inputs(case, "nan", "residual")
            assert torch.equal(nf.classes(gpu(i)) != FINITE, nf.classes(i["res"]) != FINITE)       # exactly those elements


@pytest.mark.parametrize("case", [CONV3D[0], CONV3D[3], CONV3D[5]], ids=["single_pass", "narrow", "relu2"])
def test_conv3d_cl_fp32_entry(case, oracle_ops, gpu_ops):
    """sgc_conv3d_cl_f32 (fp32 MFMA products, no operand split): bound 2e-5 of the scale as in tests/test_gpu_conv3d.py."""
    def ref(i):
        return oracle_ops.conv3d_cl(i["x"], i["wt"], i["grid"], i["k"], i["s"], i["tr"], i["sc"], i["sh"], i["res"], i["relu"])[0]

    def gpu(i):
        return gpu_ops.conv3d_cl(i["x"].cuda(), i["wt"].cuda(), i["grid"], i["k"], i["s"], i["tr"], i["sc"].cuda(), i["sh"].cuda(), _cu(i["res"]),
                                 i["relu"])[0]
    _traced(f"conv3d fp32 {case}", lambda kind: nf.conv3d_inputs(case, kind, "x"), ref, gpu, 2e-5)


@pytest.mark.parametrize("mode", [1, 2])
def test_conv3d_in_the_one_product_modes(mode, oracle_ops, gpu_ops):
    """sgc_set_conv_products(1 / 2) on one case (relu(t) + skip): against the oracle in the same mode, 1e-5 of the scale as in
    tests/test_gpu_conv3d.py.  Mode 2 saturates an infinity at +-65504 (csrc/mma.hpp keeps only a NaN): the reference does too."""
    case = CONV3D[5]
    split = gpu_ops.split_f16 if mode == 2 else gpu_ops.split_bf16

    def ref(i):
        hi, lo = split(i["wt"])
        return oracle_ops.conv3d_cl_bf16x3(i["x"], hi, lo, i["grid"], i["k"], i["s"], i["tr"], i["sc"], i["sh"], i["res"], i["relu"])[0]
    try:
        for ops in (gpu_ops, oracle_ops):
            ops.lib.call("sgc_set_conv_products", mode)
        _traced(f"conv3d mode {mode}", lambda kind: nf.conv3d_inputs(case, kind, "x"), ref, _conv3d_gpu(gpu_ops, split), 1e-5)
    finally:
        for ops in (gpu_ops, oracle_ops):
            ops.lib.call("sgc_set_conv_products", 3)


def test_output_masked_conv(oracle_ops, gpu_ops):
    """sgc_conv3d_cl_bf16x3_masked at ((20, 12, 8), 32, 32, relu 2, residual): the live rows under the traced comparison; a dead row
    holds, by the header's contract, the epilogue of a zero accumulator or the dense value -- finite unless it read the poison."""
    case = (32, 32, (20, 12, 8), 3, 1, False, True, 2)
    grid = case[2]
    blob = torch.zeros(grid)
    blob[: grid[0] // 3, grid[1] // 4: grid[1] // 2, :] = 1
    blob[-3:, -2:, -1:] = 1                                                       # the corner cluster holds the last poison site
    blob[grid[0] // 2 - 1: grid[0] // 2 + 2, :3, :3] = 1                          # and this one the interior site (row V / 2)
    mask = blob.reshape(-1).to(torch.uint8)
    live = mask.bool()
    ref = _conv3d_ref(oracle_ops)
    ref_nan = ref(nf.conv3d_inputs(case, "nan"))
    for kind in KINDS:
        i = nf.conv3d_inputs(case, kind)
        got = _conv3d_gpu(gpu_ops, out_mask=mask.cuda())(i).cpu()
        nf.compare_traced(got[live], ref_nan[live], 1e-4, f"masked conv, live rows, {kind}", kind, ref(i)[live])
        dead_bad = (nf.classes(got) != FINITE) & ~live[:, None]
        assert not bool((dead_bad & (nf.classes(ref_nan) == FINITE)).any()), f"{kind}: a dead row outside the receptive field is non-finite"


WZ_CASES = [((16, 16, 16), 64, 128, 1), ((12, 20, 8), 64, 72, 2), ((10, 10, 4), 64, 72, 1)]


@pytest.mark.parametrize("grid,cin,cout,relu", WZ_CASES)
def test_conv3d_winograd_z(grid, cin, cout, relu, oracle_ops, gpu_ops):
    """sgc_conv3d_winograd_z_bf16x3 against the oracle's DIRECT convolution (2e-5 of the scale as in tests/test_gpu_conv3d.py): F is
    widened to whole output z pairs (the F(2,3) transform mixes four input planes per pair)."""
    case = (cin, cout, grid, 3, 1, False, True, relu)

    def gpu(i):
        ghi, glo = gpu_ops.split_bf16(gpu_ops.winograd_z_weights(i["wt"]))
        return gpu_ops.conv3d_winograd_z(i["x"].cuda(), ghi.cuda(), glo.cuda(), grid, i["sc"].cuda(), i["sh"].cuda(), i["res"].cuda(), i["relu"])[0]
    assert gpu_ops.conv3d_winograd_z_supported(grid, cin, cout)
    _traced(f"winograd-z {grid} {cin}->{cout}", lambda kind: nf.conv3d_inputs(case, kind, "x"), _conv3d_ref(oracle_ops), gpu, 2e-5, z_pair_grid=grid)


def _ex_inputs(k, stride, transposed, nhw, Cout, cout_live, kind, where):
    """The case of tests/test_gpu_depth_net_hip.py::test_conv2d_ex_forms_against_float64: 48 of 64 input and cout_live of Cout output
    channels live."""
    N, H, W = nhw
    g = torch.Generator().manual_seed(100 * k + 10 * stride + int(transposed) + H + Cout)
    Cin, cin_live = 64, 48
    x = torch.randn(N * H * W, Cin, generator=g)
    x[:, cin_live:] = 0
    w = torch.randn(k * k, Cout, Cin, generator=g) / (k * Cin ** 0.5)
    w[:, cout_live:] = 0
    w[:, :, cin_live:] = 0
    scale, shift = 0.5 + torch.rand(Cout, generator=g), 0.3 * torch.randn(Cout, generator=g)
    scale[cout_live:], shift[cout_live:] = 1, 0
    OH, OW = (2 * H, 2 * W) if transposed else ((H + stride - 1) // stride, (W + stride - 1) // stride)
    res = torch.randn(N * OH * OW, Cout, generator=g)
    res[:, cout_live:] = 0
    if where == "x":
        x = nf.poison(x, kind, image_rows=H * W, live=cin_live)
        if k == 1 and stride == 2:                  # a 1 x 1 stride-2 layer reads even pixels only and the three sites are odd ones: add the
            x[(H - 2) * W + W - 2, cin_live - 1] = VALUES[kind]                  # last pixel of image 0 that it does read
    elif where == "residual":
        res = nf.poison(res, kind, image_rows=OH * OW, live=cout_live, spread="element")
    else:
        shift[cout_live - 1] = VALUES[kind]
    return dict(x=x, w=w, scale=scale, shift=shift, res=res)


@pytest.mark.parametrize("Cout,cout_live", [(160, 140), (32, 24)])
@pytest.mark.parametrize("k,stride,transposed", [(1, 1, False), (1, 2, False), (3, 1, False), (3, 2, False), (3, 2, True)])
def test_conv2d_ex_forms(k, stride, transposed, Cout, cout_live, gpu_ops):
    """Every entry of FORMS (tests/test_gpu_depth_net_hip.py) at (2, 6, 10), epilogue flags (1, 1, 1) and (0, 0, 0), against that file's
    float64 formulation, 1e-4 of the output's max-abs: two images of 60 rows, so the second site sits on an image boundary."""
    from test_gpu_depth_net_hip import _ref_conv
    nhw = (2, 6, 10)
    for relu, add, relu2 in ((1, 1, 1), (0, 0, 0)):
        def ref(i):
            return _ref_conv(i["x"], i["w"], nhw, k, stride, transposed, i["scale"], i["shift"], i["res"] if add else None, relu, relu2, 0)

        def gpu(i):
            hi, lo = gpu_ops.split_operand(i["w"].cuda())
            return gpu_ops.conv2d_nhwc_ex_bf16x3(i["x"].cuda(), hi, lo, nhw, k, stride=stride, transposed=transposed, scale=i["scale"].cuda(),
                                                 shift=i["shift"].cuda(), residual=i["res"].cuda() if add else None, relu=bool(relu),
                                                 relu_after_add=bool(relu2))
        for where in ("x", "shift") + (("residual",) if add else ()):
            _traced(f"conv2d_ex k{k} s{stride} t{int(transposed)} Cout {Cout} flags {relu}{add}{relu2} in {where}",
                    lambda kind: _ex_inputs(k, stride, transposed, nhw, Cout, cout_live, kind, where), ref, gpu, 1e-4, unit_floor=False)


def test_conv2d_ex_softmax_columns(gpu_ops):
    """depth_reg's form at (2, 6, 10): a poisoned logit turns its pixel's twelve probabilities NaN (under an infinity too: Inf - Inf in
    the softmax), so only the NaN kind has a reference with a surviving class to compare."""
    from test_gpu_depth_net_hip import _ref_conv
    nhw, Cin = (2, 6, 10), 160
    g = torch.Generator().manual_seed(11)
    x = torch.randn(120, Cin, generator=g)
    shift12 = torch.randn(12, generator=g)
    for Cout in (12, 32):
        w = torch.randn(9, Cout, Cin, generator=g) * (3.0 / (3 * Cin ** 0.5))
        w[:, 12:] = 0
        shift = F.pad(shift12, (0, Cout - 12))
        hi, lo = gpu_ops.split_operand(w.cuda())
        _traced(f"conv2d_ex softmax Cout {Cout}", lambda kind: nf.poison(x, kind, image_rows=60),
                lambda xi: _ref_conv(xi, w, nhw, 3, 1, False, None, shift, None, 0, 0, 12),
                lambda xi: gpu_ops.conv2d_nhwc_ex_bf16x3(xi.cuda(), hi, lo, nhw, 3, shift=shift.cuda(), softmax_cols=12), 1e-4, kinds=("nan",),
                unit_floor=False)


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("nhw", [(1, 5, 7), (3, 9, 9)])
def test_conv2d_strided_entry_on_odd_sizes(nhw, k, gpu_ops):
    from test_gpu_resnet import _ref_conv, _strided_case
    N, H, W = nhw
    Cout, cout_live = 160, 140
    x, w, scale, shift, res = _strided_case(k, nhw, Cout, cout_live, 100 * k + H + Cout)
    hi, lo = gpu_ops.split_operand(w.cuda())
    _traced(f"conv2d_strided k{k} {nhw}", lambda kind: nf.poison(x, kind, image_rows=H * W, live=48),
            lambda xi: _ref_conv(xi, w, nhw, k, 2, scale, shift, res, 1, 1)[0],
            lambda xi: gpu_ops.conv2d_nhwc_strided_bf16x3(xi.cuda(), hi, lo, nhw, k, stride=2, scale=scale.cuda(), shift=shift.cuda(),
                                                          residual=res.cuda(), relu=True, relu_after_add=True), 1e-4, unit_floor=False)


@pytest.mark.parametrize("relu", [True, False])
def test_conv2d_stem7(relu, gpu_ops):
    N, H, W = 2, 12, 20
    g = torch.Generator().manual_seed(H)
    img = torch.randn(N, 3, H, W, generator=g)
    w = torch.randn(64, 3, 7, 7, generator=g) / 147 ** 0.5
    scale, shift = 0.5 + torch.rand(64, generator=g), 0.3 * torch.randn(64, generator=g)
    hi, lo = gpu_ops.split_operand(F.pad(w.reshape(64, 147), (0, 13)).contiguous().cuda())

    def build(kind):
        return _rows_to_nchw(nf.poison(img.permute(0, 2, 3, 1).reshape(-1, 3), kind, image_rows=H * W), N, H, W)

    def ref(im):
        y = F.conv2d(im.double(), w.double(), stride=2, padding=3) * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
        return (y.clamp_min(0) if relu else y).permute(0, 2, 3, 1).reshape(-1, 64)
    _traced(f"stem7 relu {relu}", build, ref, lambda im: gpu_ops.conv2d_stem7_bf16x3(im.cuda(), hi, lo, scale=scale.cuda(), shift=shift.cuda(), relu=relu),
            1e-4, unit_floor=False)


def _linear_case(rows, cin, cout):
    g = torch.Generator().manual_seed(rows + cout)
    return torch.randn(rows, cin, generator=g), torch.randn(1, cout, cin, generator=g) * 0.05, torch.randn(cout, generator=g)


@pytest.mark.parametrize("zero_tail", [False, True], ids=["plain", "zero_row"])
def test_linear_rows(zero_tail, oracle_ops, gpu_ops):
    """sgc_linear_rows_bf16x3 and its zero-row form at (1237, 128, 96): poison in x and in shift; the zero row stays zero."""
    rows, cin, cout = 1237, 128, 96
    x, w, b = _linear_case(rows, cin, cout)
    hi, lo = gpu_ops.split_bf16(w)

    def build(where):
        def f(kind):
            if where == "x":
                return nf.poison(x, kind), b
            s = b.clone()
            s[cout - 1] = VALUES[kind]
            return x, s
        return f

    def gpu(i):
        y = gpu_ops.linear_rows_bf16x3(i[0].cuda(), hi.cuda(), lo.cuda(), i[1].cuda(), zero_tail=zero_tail)
        if zero_tail:
            tail = torch.as_strided(y, (1, cout), (cout, 1), storage_offset=y.storage_offset() + rows * cout)
            assert torch.equal(tail, torch.zeros_like(tail))
        return y
    for where in ("x", "shift"):
        _traced(f"linear_rows zero_tail {zero_tail} in {where}", build(where), lambda i: oracle_ops.linear_rows_bf16x3(i[0], hi, lo, i[1]), gpu, 1e-4)


@pytest.mark.parametrize("relu", [1, 2])
def test_row_gemm_epilogues(relu, oracle_ops, gpu_ops):
    """The 1x1x1 entry on rows (the persistent row GEMM's scale / shift / relu / residual epilogue, csrc/rows_core.hpp) at 1237 ragged
    rows: poison in x, in the residual and in shift."""
    case = (128, 96, (1237, 1, 1), 1, 1, False, True, relu)
    ref, gpu = _conv3d_ref(oracle_ops), _conv3d_gpu(gpu_ops)
    for where in ("x", "residual", "shift"):
        _traced(f"row GEMM relu {relu} in {where}", lambda kind: nf.conv3d_inputs(case, kind, where), ref, gpu, 1e-4)


def test_linear_rows_headmajor(oracle_ops, gpu_ops):
    N, S, Cin, M, Cm = 3, 333, 64, 8, 16
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N * S, Cin, generator=g)
    w, b = torch.randn(1, M * Cm, Cin, generator=g) * 0.2, torch.randn(M * Cm, generator=g)
    hi, lo = gpu_ops.split_bf16(w)
    _traced("linear_rows_headmajor", lambda kind: nf.poison(x, kind, image_rows=S),
            lambda xi: oracle_ops.linear_rows_headmajor_bf16x3(xi, hi, lo, b, N, S, M).reshape(N * M * S, Cm),
            lambda xi: gpu_ops.linear_rows_headmajor_bf16x3(xi.cuda(), hi.cuda(), lo.cuda(), b.cuda(), N, S, M).reshape(N * M * S, Cm), 1e-4)


def test_linear_rows_blockdiag(oracle_ops, gpu_ops):
    """(33, 128): the poisoned input column belongs to the last group -- only that group's Nh output columns may turn."""
    rows, K, G = 33, 128, 8
    Nh = K // 8
    g = torch.Generator().manual_seed(rows + K)
    x = torch.randn(rows, G * K, generator=g)
    w, b = torch.randn(G, Nh, K, generator=g) * (1.0 / K ** 0.5), torch.randn(G * Nh, generator=g) * 0.1
    hi, lo = gpu_ops.split_bf16(w)
    _traced("linear_rows_blockdiag", lambda kind: nf.poison(x, kind), lambda xi: oracle_ops.linear_rows_blockdiag(xi, hi, lo, b),
            lambda xi: gpu_ops.linear_rows_blockdiag(xi.cuda(), hi.cuda(), lo.cuda(), b.cuda()), 1e-5)


def test_level_tail(oracle_ops, gpu_ops):
    """sgc_level_tail at (31, 128), every voxel seen.  Both LayerNorms turn a row that holds an infinity into NaN in the reference
    too, so no infinity survives and no ReLU removes one: the NaN kind is the one with a class to compare."""
    from test_gpu_kernels import _level_tail_case
    ctx, row_of, vis, (wo, w1, w2), (bo, b1, b2), ln1, ln2 = _level_tail_case(31, 128, 1.0)
    sp = lambda w: gpu_ops.split_bf16(w.view(1, *w.shape))             # noqa: E731
    so, s1, s2 = sp(wo), sp(w1), sp(w2)
    cup = lambda pr: tuple(_cu(t) for t in pr)                         # noqa: E731
    _traced("level_tail", lambda kind: nf.poison(ctx, kind), lambda c: oracle_ops.level_tail(c, row_of, so, bo, ln1, s1, b1, s2, b2, ln2),
            lambda c: gpu_ops.level_tail(c.cuda(), row_of.cuda(), cup(so), bo.cuda(), cup(ln1), cup(s1), b1.cuda(), cup(s2), b2.cuda(), cup(ln2)),
            1e-4, kinds=("nan",))


# ---- weight gradients: the poisoned set of dW equals the float64 set ---------------------------------------------------------------------
def _wgrad_traced(what, x, dy, x_image_rows, dy_image_rows, ref, gpu, tol, unit_floor=True):
    for where in ("x", "dy"):
        def build(kind):
            return (nf.poison(x, kind, image_rows=x_image_rows), dy) if where == "x" else (x, nf.poison(dy, kind, image_rows=dy_image_rows))
        _traced(f"{what} in {where}", build, lambda i: _flat(ref(*i)), lambda i: _flat(gpu(i[0].cuda(), i[1].cuda())), tol, unit_floor=unit_floor)


def _flat(dw):
    return dw.reshape(-1, dw.shape[-1])


def test_conv3d_wgrad(oracle_ops, gpu_ops):
    """(36, 4, (5, 5, 3), 1, 1) and the 3x3x3 (32, 28, (7, 5, 6)) of WGRAD_CASES against the double-accumulating oracle, 1e-4."""
    for cin, cout, grid, k, s in ((36, 4, (5, 5, 3), 1, 1), (32, 28, (7, 5, 6), 3, 1)):
        g = torch.Generator().manual_seed(sum(grid) + cin + cout)
        V = grid[0] * grid[1] * grid[2]
        x, dy = torch.randn(V, cin, generator=g), torch.randn(V, cout, generator=g)
        _wgrad_traced(f"conv3d_wgrad {cin}->{cout} {grid} k{k}", x, dy, None, None, lambda a, b: oracle_ops.conv3d_wgrad_bf16x3(a, b, grid, k, s),
                      lambda a, b: gpu_ops.conv3d_wgrad_bf16x3(a, b, grid, k, s), 1e-4)


@pytest.mark.parametrize("k,s", [(1, 1), (3, 1), (3, 2)])
def test_conv2d_wgrad(k, s, gpu_ops):
    from test_gpu_resnet_train import _wgrad_ref
    nhw, Cin, Cout = (3, 5, 3), 32, 32
    N, H, W = nhw
    OH, OW = (H + s - 1) // s, (W + s - 1) // s
    g = torch.Generator().manual_seed(1000 * k + 100 * s + H + Cin)
    x, dy = torch.randn(N * H * W, Cin, generator=g), torch.randn(N * OH * OW, Cout, generator=g)
    _wgrad_traced(f"conv2d_wgrad k{k} s{s}", x, dy, H * W, OH * OW, lambda a, b: _wgrad_ref(a, b, nhw, k, s),
                  lambda a, b: gpu_ops.conv2d_wgrad_bf16x3(a, b, nhw, k, s), 1e-4, unit_floor=False)


def test_conv2d_stem7_wgrad(gpu_ops):
    N, H, W = 3, 8, 12
    g = torch.Generator().manual_seed(1000 * N + 10 * H + W)
    img, dy = torch.randn(N * H * W, 3, generator=g), torch.randn(N * (H // 2) * (W // 2), 64, generator=g)

    def ref(im_rows, d):
        w = torch.zeros(64, 3, 7, 7, dtype=torch.float64, requires_grad=True)
        y = F.conv2d(_rows_to_nchw(im_rows.double(), N, H, W), w, stride=2, padding=3)
        return torch.autograd.grad(y, w, _rows_to_nchw(d.double(), N, H // 2, W // 2))[0]
    _wgrad_traced("stem7_wgrad", img, dy, H * W, (H // 2) * (W // 2), ref,
                  lambda a, b: gpu_ops.conv2d_stem7_wgrad_bf16x3(_rows_to_nchw(a, N, H, W), b), 1e-4, unit_floor=False)


# ======================================================================================================================================
# optimiser and head loss: exact comparison
# ======================================================================================================================================
@pytest.mark.parametrize("kind", ["nan", "+inf"])
def test_fused_adamw_poisons_what_clip_grad_norm_and_adamw_poison(kind):
    """One step of FusedAdamW (sgc_grad_sqnorm_batch + sgc_adamw_step_batch, max_norm 35) over three small tensors with ONE non-finite
    gradient element: clip_grad_norm_ turns a NaN norm into a NaN coefficient and poisons every gradient of every tensor; an infinite
    norm gives coefficient 0, so the infinite element becomes Inf * 0 = NaN and every other gradient 0.  Every parameter and both
    moments carry the classes of clip_grad_norm_ + torch.optim.AdamW in float64; the finite ones agree to 1e-6 of the scale."""
    from sgcdet_amd.optim import FusedAdamW
    g = torch.Generator().manual_seed(7)
    shapes = [(64, 33), (257,), (5, 4, 3)]
    init = [(torch.rand(s, generator=g) - 0.5) * 0.5 for s in shapes]
    grads = [torch.randn(s, generator=g) for s in shapes]
    grads[1][100] = VALUES[kind]
    sides = {}
    for name, dev, dt in (("ref", "cpu", torch.float64), ("hip", "cuda", torch.float32)):
        ps = [torch.nn.Parameter(t.to(device=dev, dtype=dt)) for t in init]
        for p, gr in zip(ps, grads):
            p.grad = gr.to(device=dev, dtype=dt, copy=True)
        if name == "ref":
            opt = torch.optim.AdamW(ps, lr=2e-4, weight_decay=1e-4, foreach=False)
            torch.nn.utils.clip_grad_norm_(ps, 35.0, foreach=False)
        else:
            opt = FusedAdamW(ps, lr=2e-4, weight_decay=1e-4, max_grad_norm=35.0)
        opt.step()
        sides[name] = [(p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]) for p in ps]
    n_bad = 0
    for i, (h, r) in enumerate(zip(sides["hip"], sides["ref"])):
        for what, a, b in zip(("param", "exp_avg", "exp_avg_sq"), h, r):
            ca, cb = nf.classes(a), nf.classes(b)
            n_bad += int((cb != FINITE).sum())
            assert torch.equal(ca, cb), f"{kind}: tensor {i} {what}: {int((ca != cb).sum())} of {cb.numel()} elements of another class than torch's"
            fin = cb == FINITE
            if bool(fin.any()):
                err = float((a.cpu().double()[fin] - b[fin]).abs().max())
                assert err <= 1e-6 * max(1.0, float(b[fin].abs().max())), (i, what, err)
    assert n_bad >= 3                                              # the poison reached the parameter and both moments
    if kind == "nan":
        assert all(bool(torch.isnan(t).all()) for trip in sides["hip"] for t in trip)       # the whole model is NaN: loud


def test_head_loss_with_one_nan_logit(oracle_ops):
    """One NaN in cls_score (a valid point of the coarsest scale) on the smallest head case (axis-aligned, one box): the three losses and
    every gradient carry the classes of the torch path in float64; finite entries within the bound of tests/test_gpu_head_loss.py."""
    from head_loss_contract import GRIDS, bound_rows, head_tensors, torch_path, torch_path_grads
    from test_gpu_head_loss import UPSTREAM, _fused, _names, _targets
    rotated, case = False, 1
    pts, ct, bt, lb = _targets(oracle_ops, rotated, case)
    ctr, reg, cls, val = head_tensors(rotated, 100 + 10 * case + int(rotated))
    spot = tuple(int(v) for v in val[2][0].nonzero()[0])
    cls[2][(3,) + spot] = float("nan")
    out = {}
    for dtype in (torch.float64, torch.float32):
        losses, leaves = torch_path(rotated, ctr, reg, cls, val, pts, ct, bt, lb, dtype)
        out[dtype] = ([l.detach() for l in losses], torch_path_grads(losses, leaves, UPSTREAM))
    h_losses, h_grads = _fused(rotated, ctr, reg, cls, val, pts, ct, bt, lb)
    r64 = torch.stack(out[torch.float64][0])
    assert nf.classes(r64).tolist() == [FINITE, FINITE, nf.NAN]                     # precondition: loss_cls alone is poisoned
    assert nf.classes(torch.stack([l.detach() for l in h_losses])).tolist() == nf.classes(r64).tolist()
    n_bad = 0
    for name, h, a, b in zip(_names(len(GRIDS)), h_grads, out[torch.float32][1], out[torch.float64][1]):
        ch, cb = nf.classes(h), nf.classes(b)
        n_bad += int((cb != FINITE).sum())
        assert torch.equal(ch, cb), f"{name}: {int((ch != cb).sum())} elements of another class than the torch path's"
        fin = cb == FINITE
        hh, aa, bb = (torch.where(fin, t.detach().cpu().double(), torch.zeros((), dtype=torch.float64)) for t in (h, a, b))
        assert all(r["ok"] for r in bound_rows("one NaN logit", [name], [hh], [aa], [bb], 1.0))
    assert 0 < n_bad < sum(g.numel() for g in h_grads) // 2
    assert all(r["ok"] for r in bound_rows("one NaN logit", ["loss_centerness", "loss_bbox"], h_losses[:2], out[torch.float32][0][:2],
                                           out[torch.float64][0][:2], None))
