"""The Winograd-z convolution (sgc_conv3d_winograd_z_bf16x3) on its two bricks -- 4 images x 8 x 8 and 2 images x 10 x 10 pixels of
the virtual transform-domain stack -- and on the z extent the small brick opens (Z = 4: the 10 x 10 x 4 scale).  Every case is a
few hundred to a few thousand voxels with 64 -> 72 channels (two channel slices: the halo image is restaged; a partial 128-column
tile), seeded, through the C ABI."""
import pytest
import torch

CIN, COUT = 64, 72
# (scale, shift, residual, relu): everything with each ReLU order (1: behind the skip, 2: in front of it), and nothing at all
EPILOGUES = [(True, 1), (True, 2), (False, 0)]


def _case(grid, full, seed=0):
    g = torch.Generator().manual_seed(seed + sum(grid) + CIN)
    V = grid[0] * grid[1] * grid[2]
    x = torch.randn(V, CIN, generator=g)
    w = torch.randn(27, COUT, CIN, generator=g) * (1.0 / (27 * CIN) ** 0.5)
    scale, shift = torch.rand(COUT, generator=g) + 0.5, torch.randn(COUT, generator=g)
    residual = torch.randn(V, COUT, generator=g)
    if not full:
        scale = shift = residual = None
    return x, w, scale, shift, residual


def _cu(t):
    return None if t is None else t.cuda()


def _wino(ops, x, ghi, glo, grid, scale, shift, residual, relu):
    return ops.conv3d_winograd_z(_cu(x), _cu(ghi), _cu(glo), grid, _cu(scale), _cu(shift), _cu(residual), relu)[0]


@pytest.mark.gpu
@pytest.mark.parametrize("full,relu", EPILOGUES)
@pytest.mark.parametrize("grid", [(20, 20, 8), (12, 20, 8)])
def test_both_bricks_give_the_same_bits(grid, full, relu, gpu_ops):
    """An accumulator sees (tap, k-half, product) in the same order whatever the brick: the call forced onto 4 x 8 x 8 (`wz_brick`
    = 1) and onto 2 x 10 x 10 (2) is equal ELEMENTWISE -- on 20 x 20 slices (8 bricks of 10 x 10 against 9 ragged ones of 8 x 8)
    and on 12 x 20, which both tile raggedly -- and so is the plan's own choice (0)."""
    x, w, scale, shift, residual = _case(grid, full)
    ghi, glo = gpu_ops.split_bf16(gpu_ops.winograd_z_weights(w))
    outs = {}
    try:
        for brick in (1, 2, 0):
            gpu_ops.lib.call("sgc_set_tuning", b"wz_brick", brick)
            assert gpu_ops.conv3d_winograd_z_supported(grid, CIN, COUT)
            outs[brick] = _wino(gpu_ops, x, ghi, glo, grid, scale, shift, residual, relu)
    finally:
        gpu_ops.lib.call("sgc_set_tuning", b"wz_brick", 0)
    assert torch.isfinite(outs[1]).all()
    assert torch.equal(outs[1], outs[2])
    assert torch.equal(outs[0], outs[1])


@pytest.mark.gpu
@pytest.mark.parametrize("full,relu", EPILOGUES)
@pytest.mark.parametrize("grid", [(10, 10, 4), (20, 10, 4), (12, 10, 4)])
def test_z_extent_4_against_the_direct_form_and_the_twin(grid, full, relu, oracle_ops, gpu_ops):
    """Z = 4 (two images per position: one, two and -- ragged, 12 = 10 + 2 -- two 2 x 10 x 10 bricks per position), with the bounds of
    tests/test_gpu_conv3d.py::test_winograd_z_convolution_against_the_direct_form: 2e-5 of the tensor scale against the oracle's and
    the GPU's direct convolution on the original weights, 1e-5 against the oracle's Winograd twin; two calls on the same buffers
    are equal elementwise."""
    x, w, scale, shift, residual = _case(grid, full)
    hi, lo = gpu_ops.split_bf16(w)
    ghi, glo = gpu_ops.split_bf16(gpu_ops.winograd_z_weights(w))
    assert gpu_ops.conv3d_winograd_z_supported(grid, CIN, COUT)
    args = (_cu(x), _cu(ghi), _cu(glo), grid, _cu(scale), _cu(shift), _cu(residual), relu)
    got, _ = gpu_ops.conv3d_winograd_z(*args)
    again, _ = gpu_ops.conv3d_winograd_z(*args)
    assert torch.equal(got, again)
    direct_gpu, _ = gpu_ops.conv3d_cl_bf16x3(_cu(x), _cu(hi), _cu(lo), grid, 3, 1, False, _cu(scale), _cu(shift), _cu(residual), relu)
    want, _ = oracle_ops.conv3d_cl_bf16x3(x, hi, lo, grid, 3, 1, False, scale, shift, residual, relu)
    twin, _ = oracle_ops.conv3d_winograd_z(x, ghi, glo, grid, scale, shift, residual, relu)
    sc = max(1.0, float(want.abs().max()))
    errs = [float((got.cpu() - want).abs().max()) / sc, float((got - direct_gpu).abs().max()) / sc, float((got.cpu() - twin).abs().max()) / sc]
    print(f"{grid} relu={relu} full={full}: vs oracle direct {errs[0]:.2e}, vs GPU direct {errs[1]:.2e}, vs twin {errs[2]:.2e}")
    assert errs[0] < 2e-5 and errs[1] < 2e-5 and errs[2] < 1e-5, errs


@pytest.mark.gpu
@pytest.mark.parametrize("grid", [(20, 20, 8), (12, 20, 8)])
def test_the_small_brick_is_deterministic_at_z_extent_8(grid, gpu_ops):
    x, w, scale, shift, residual = _case(grid, True)
    ghi, glo = gpu_ops.split_bf16(gpu_ops.winograd_z_weights(w))
    try:
        gpu_ops.lib.call("sgc_set_tuning", b"wz_brick", 2)
        a = _wino(gpu_ops, x, ghi, glo, grid, scale, shift, residual, 1)
        b = _wino(gpu_ops, x, ghi, glo, grid, scale, shift, residual, 1)
    finally:
        gpu_ops.lib.call("sgc_set_tuning", b"wz_brick", 0)
    assert torch.equal(a, b)


@pytest.mark.gpu
def test_split_reduction_of_a_small_stack(gpu_ops):
    """10 x 10 x 4 is 4 bricks x 1 column tile: `halo_split_target` = 192 splits its two channel slices over two workgroups each
    (1: unsplit).  The partial tiles go to the workspace BEYOND the 2 V Cout floats of the transform-domain tensor -- seen here by
    what the call leaves of a NaN fill: exactly two partial tensors written when it splits, none when the workspace has no room
    or the plan does not ask -- and are summed in split order: equal to the unsplit result within 1e-5 of the tensor scale (the
    bound of tests/test_gpu_conv3d.py::test_tile_kernel_splits_of_whole_steps_against_the_oracle), bitwise reproducible."""
    grid = (10, 10, 4)
    x, w, scale, shift, residual = _case(grid, True, seed=3)
    ghi, glo = gpu_ops.split_bf16(gpu_ops.winograd_z_weights(w))
    V = x.shape[0]
    m = int(gpu_ops.lib._dll.sgc_conv3d_winograd_z_workspace_floats(*grid, CIN, COUT))
    assert m == 2 * V * COUT
    dev = [_cu(t) for t in (x, ghi, glo, scale, shift, residual)]

    def run(target, ws_floats):
        ws = torch.full((m * 4,), float("nan"), device="cuda")
        y = torch.empty(V, COUT, device="cuda")
        gpu_ops.lib.call("sgc_set_tuning", b"halo_split_target", target)
        gpu_ops._call("sgc_conv3d_winograd_z_bf16x3", *dev, y, *grid, CIN, COUT, 1, ws, ws_floats)
        torch.cuda.synchronize()
        written = [bool(torch.isfinite(ws[i * m:(i + 1) * m]).all()) for i in range(4)]
        untouched = [bool(torch.isnan(ws[i * m:(i + 1) * m]).all()) for i in range(4)]
        return y, written, untouched

    try:
        y_split, wr, un = run(192, 4 * m)
        assert wr[:3] == [True] * 3 and un[3], (wr, un)           # m, two partial tensors, nothing further
        y_again, _, _ = run(192, 4 * m)
        y_tight, wr, un = run(192, m)                             # no room: one split rather than atomics
        assert wr[0] and un[1:] == [True] * 3, (wr, un)
        y_one, wr, un = run(1, 4 * m)                             # the plan asks for none
        assert wr[0] and un[1:] == [True] * 3, (wr, un)
    finally:
        gpu_ops.lib.call("sgc_set_tuning", b"halo_split_target", 192)
    assert torch.equal(y_split, y_again)
    assert torch.equal(y_tight, y_one)
    sc = max(1.0, float(y_one.abs().max()))
    err = float((y_split - y_one).abs().max()) / sc
    print(f"split vs unsplit: {err:.2e} of the tensor scale")
    assert err <= 1e-5
    # the tensor API sizes the workspace of a Z = 4 call for the split, so this is the form the plugin's layers run
    assert torch.equal(_wino(gpu_ops, x, ghi, glo, grid, scale, shift, residual, 1), y_split)


def test_gate_of_the_winograd_entry():
    """Host side only (the plan is pure): the entry takes 10 x 10 x 4 and 20 x 20 x 8, refuses an odd z extent, one that is not a
    multiple of 4, fewer than 65 output channels and slices under 8 pixels; its workspace is the 2 X Y Z Cout floats of the four
    transform-domain outputs."""
    from sgcdet_amd import build
    from sgcdet_amd._abi import Library
    dll = Library(build.build())._dll
    for grid in [(10, 10, 4), (20, 20, 8), (20, 10, 4), (12, 10, 4), (12, 20, 8)]:
        for cin, cout in [(CIN, COUT), (1024, 1024), (512, 128)]:
            assert dll.sgc_conv3d_winograd_z_supported(*grid, cin, cout) == 1, (grid, cin, cout)
            assert dll.sgc_conv3d_winograd_z_workspace_floats(*grid, cin, cout) == 2 * grid[0] * grid[1] * grid[2] * cout
    for grid in [(10, 10, 5), (10, 10, 6), (10, 10, 2), (7, 10, 4), (10, 10, 3)]:
        assert dll.sgc_conv3d_winograd_z_supported(*grid, CIN, COUT) == 0, grid
        assert dll.sgc_conv3d_winograd_z_workspace_floats(*grid, CIN, COUT) == 0
    assert dll.sgc_conv3d_winograd_z_supported(10, 10, 4, CIN, 64) == 0
    assert dll.sgc_conv3d_winograd_z_supported(10, 10, 4, 48, COUT) == 0


@pytest.mark.gpu
def test_neck_and_head_with_the_z4_layers_on_the_winograd_form():
    """Config 2's neck and head (40 x 40 x 16, 20 x 20 x 8 and 10 x 10 x 4 scales) with every layer the gate admits on the Winograd
    form -- the 10 x 10 x 4 pair through ``conv_plan.WINOGRAD_Z_Z4`` -- against every layer on the direct kernel: each head tensor
    within 1e-4 of its scale (the bound of tests/test_gpu_conv3d.py::test_winograd_z_through_the_neck_keeps_parity), and the nine
    layers really took the form (seven without the switch)."""
    import sgcdet_amd.plugin  # noqa: F401
    from sgcdet_amd import ext
    from sgcdet_amd.mmcv_lite import build_detector
    from sgcdet_amd.plugin import conv_plan
    from sgcdet_amd.scene import model_config, workload
    w = workload("cfg2_scannet")
    torch.manual_seed(2)
    det = build_detector(model_config(w)).eval().cuda()
    det.use_graph = det.scene_graph = False
    vol = torch.randn(1, w["embed_dims"], *w["n_voxels_list"][-1], device="cuda")
    outs, grids = {}, {}
    ops = ext.ops()
    z4 = conv_plan.WINOGRAD_Z_Z4
    orig = ops.conv3d_winograd_z
    try:
        for mode in (False, True):
            conv_plan.set_winograd_z(mode, min_channels=256)
            conv_plan.WINOGRAD_Z_Z4 = bool(mode)
            det.neck_3d.__dict__.pop("_hip_plan", None)
            log = grids[mode] = []
            ops.conv3d_winograd_z = lambda *a, **k: (log.append(tuple(a[3])), orig(*a, **k))[1]
            with torch.no_grad():
                o = det._neck_head_eager(vol)
            torch.cuda.synchronize()
            outs[mode] = [t.clone() for part in o for t in part]
    finally:
        ops.conv3d_winograd_z = orig
        conv_plan.WINOGRAD_Z_Z4 = z4
        conv_plan.set_winograd_z("auto", min_channels=256)
        det.neck_3d.__dict__.pop("_hip_plan", None)
    assert grids[False] == []
    assert len(grids[True]) == 9 and grids[True].count((10, 10, 4)) == 2 and grids[True].count((20, 20, 8)) == 3, grids[True]
    for a, b in zip(outs[True], outs[False]):
        err = float((a - b).abs().max()) / max(1.0, float(b.abs().max()))
        print(f"head tensor {tuple(a.shape)}: {err:.2e} of its scale")
        assert err <= 1e-4
