"""The Winograd-z bricks on v_mfma_f32_16x16x32 (`wz_mfma` = 16, the default) beside the 32x32x16 form (32), through the C ABI.

Shapes: 64 -> 72 channels (two channel slices: the halo image is restaged; a partial 128-column tile) and 32 -> 160 (one slice; a
second, partial column tile).  Grids: 8 x 8 x 8 (one exact 4 x 8 x 8 brick per position; 1024 stack rows, so `halo_min_m` is lowered
for it), 12 x 20 x 8 (ragged on both bricks), 20 x 20 x 8 (exact 2 x 10 x 10) and 10 x 10 x 4 at `halo_split_target` 192 (the
split path; the small brick only).  Each grid runs on `wz_brick` 1 and 2 where each fits.  References are computed once per case
and shared."""
import contextlib
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SHAPES = [(64, 72), (32, 160)]
GRIDS = [(8, 8, 8), (12, 20, 8), (20, 20, 8), (10, 10, 4)]
# (scale, shift, residual, relu) of tests/test_gpu_conv3d_wz_bricks.py: everything with each ReLU order, and nothing at all
EPILOGUES = [(True, 1), (True, 2), (False, 0)]
DEFAULTS = {"wz_mfma": 16, "wz_brick": 0, "halo_min_m": 2048, "halo_split_target": 192}


def _bricks(grid):
    return (2,) if grid[2] == 4 else (1, 2)


@contextlib.contextmanager
def _tuned(ops, grid, **knobs):
    """The knobs of one call; 8 x 8 x 8 is 1024 stack rows and takes the Winograd bricks only below the default `halo_min_m`."""
    if grid == (8, 8, 8):
        knobs["halo_min_m"] = 1024
    try:
        for k, v in knobs.items():
            ops.lib.call("sgc_set_tuning", k.encode(), v)
        yield
    finally:
        for k in knobs:
            ops.lib.call("sgc_set_tuning", k.encode(), DEFAULTS[k])


def _cu(t):
    return None if t is None else t.cuda()


def _wino(ops, x, ghi, glo, grid, scale, shift, residual, relu):
    assert ops.conv3d_winograd_z_supported(grid, x.shape[1], ghi.shape[2])
    return ops.conv3d_winograd_z(_cu(x), _cu(ghi), _cu(glo), grid, _cu(scale), _cu(shift), _cu(residual), relu)[0]


def _conv64(x, w, grid):
    """The direct 3 x 3 x 3 convolution in float64: x [V, Cin], w [27, Cout, Cin] with tap = (dx * 3 + dy) * 3 + dz -> [V, Cout]."""
    cout, cin = w.shape[1:]
    xv = x.double().view(1, *grid, cin).permute(0, 4, 1, 2, 3)
    wv = w.double().view(3, 3, 3, cout, cin).permute(3, 4, 0, 1, 2)
    return F.conv3d(xv, wv, padding=1)[0].permute(1, 2, 3, 0).reshape(-1, cout)


# ---- exact arithmetic ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _exact_case(grid, cin, cout):
    g = torch.Generator().manual_seed(sum(grid) + cin + cout)
    V = grid[0] * grid[1] * grid[2]
    x = torch.randint(-3, 4, (V, cin), generator=g).float() + torch.randint(-3, 4, (V, cin), generator=g).float() * 2.0 ** -10
    w = torch.randint(-1, 2, (27, cout, cin), generator=g).float() * 2.0
    return x, w, _conv64(x, w, grid)


@pytest.mark.parametrize("cin,cout", SHAPES)
@pytest.mark.parametrize("grid", GRIDS)
def test_exact_arithmetic_on_both_shapes_and_bricks(grid, cin, cout, gpu_ops):
    """x = a + b / 1024 with integers a, b in [-3, 3], weights in {-2, 0, 2}: the transformed weights are integers (their lo plane
    is zero), and every transform, split and partial sum is exact in fp32 (|sum| <= 9 * 64 * 18 < 2^14 units of 2^-10).  The
    result is then independent of the summation order and must EQUAL the float64 direct convolution -- any row, column or chunk
    mix-up of either MFMA shape shows."""
    x, w, want = _exact_case(grid, cin, cout)
    ghi, glo = gpu_ops.split_bf16(gpu_ops.winograd_z_weights(w))
    assert not bool(glo.float().any()) and torch.equal(want.float().double(), want)
    for key in (32, 16):
        for brick in _bricks(grid):
            with _tuned(gpu_ops, grid, wz_mfma=key, wz_brick=brick, halo_split_target=192):
                got = _wino(gpu_ops, x, ghi, glo, grid, None, None, None, 0)
            bad = got.cpu().double() != want
            assert not bool(bad.any()), (f"wz_mfma {key}, brick {brick}: {int(bad.sum())} of {bad.numel()} elements differ, first at "
                                         f"{tuple(int(i) for i in bad.nonzero()[0])}")


# ---- random data, both key values ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _random_case(grid, cin, cout, full):
    g = torch.Generator().manual_seed(sum(grid) + cin + cout)
    V = grid[0] * grid[1] * grid[2]
    x = torch.randn(V, cin, generator=g)
    w = torch.randn(27, cout, cin, generator=g) * (1.0 / (27 * cin) ** 0.5)
    scale, shift = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    residual = torch.randn(V, cout, generator=g)
    if not full:
        scale = shift = residual = None
    return x, w, scale, shift, residual


@functools.lru_cache(maxsize=None)
def _oracle_refs(grid, cin, cout, full, relu):
    import oracle
    o = oracle.ops()
    x, w, scale, shift, residual = _random_case(grid, cin, cout, full)
    hi, lo = o.split_bf16(w)
    ghi, glo = o.split_bf16(o.winograd_z_weights(w))
    want, _ = o.conv3d_cl_bf16x3(x, hi, lo, grid, 3, 1, False, scale, shift, residual, relu)
    twin, _ = o.conv3d_winograd_z(x, ghi, glo, grid, scale, shift, residual, relu)
    return want, twin


@pytest.mark.parametrize("full,relu", EPILOGUES)
@pytest.mark.parametrize("cin,cout", SHAPES)
@pytest.mark.parametrize("grid", GRIDS)
def test_random_data_under_both_key_values(grid, cin, cout, full, relu, oracle_ops, gpu_ops):
    """The bounds of tests/test_gpu_conv3d.py::test_winograd_z_convolution_against_the_direct_form under each key value and brick:
    2e-5 of the tensor scale against the oracle's direct convolution, 1e-5 against the oracle's Winograd twin; two calls are equal
    elementwise.  The two key values differ in how the instruction sums 32 products: their distance is printed and held to the
    twin bound, 1e-5 (measured: profiles/r21_wz_mfma_shape.md)."""
    x, w, scale, shift, residual = _random_case(grid, cin, cout, full)
    want, twin = _oracle_refs(grid, cin, cout, full, relu)
    ghi, glo = gpu_ops.split_bf16(gpu_ops.winograd_z_weights(w))
    sc = max(1.0, float(want.abs().max()))
    for brick in _bricks(grid):
        outs = {}
        for key in (32, 16):
            with _tuned(gpu_ops, grid, wz_mfma=key, wz_brick=brick, halo_split_target=192):
                got = _wino(gpu_ops, x, ghi, glo, grid, scale, shift, residual, relu)
                again = _wino(gpu_ops, x, ghi, glo, grid, scale, shift, residual, relu)
            assert torch.equal(got, again), (key, brick)
            outs[key] = got.cpu()
            errs = float((outs[key] - want).abs().max()) / sc, float((outs[key] - twin).abs().max()) / sc
            print(f"{grid} {cin}->{cout} relu={relu} full={full} brick {brick} wz_mfma {key}: vs oracle direct {errs[0]:.2e}, vs twin {errs[1]:.2e}")
            assert errs[0] < 2e-5 and errs[1] < 1e-5, (key, brick, errs)
        dist = float((outs[16] - outs[32]).abs().max()) / sc
        print(f"{grid} {cin}->{cout} relu={relu} full={full} brick {brick}: wz_mfma 16 against 32: {dist:.2e} of the tensor scale")
        assert dist < 1e-5, (brick, dist)


def test_both_bricks_give_the_same_bits_under_key_16(gpu_ops):
    """As tests/test_gpu_conv3d_wz_bricks.py::test_both_bricks_give_the_same_bits: every accumulator sees (tap, product) in one order
    on either brick."""
    grid, (cin, cout) = (12, 20, 8), SHAPES[0]
    x, w, scale, shift, residual = _random_case(grid, cin, cout, True)
    ghi, glo = gpu_ops.split_bf16(gpu_ops.winograd_z_weights(w))
    outs = []
    for brick in (1, 2):
        with _tuned(gpu_ops, grid, wz_mfma=16, wz_brick=brick):
            outs.append(_wino(gpu_ops, x, ghi, glo, grid, scale, shift, residual, 1))
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])


# ---- one-product modes ----------------------------------------------------------------------------------------------------------------
def _wino64_rounded(x, g, grid, rnd):
    """The Winograd form in float64 on operands ROUNDED to the mode: the input transform in fp32 as the kernel makes it (one
    rounding per element), then ``rnd``; the transformed weights ``g`` [4, 9, Cout, Cin] already rounded."""
    X, Y, Z = grid
    cout, cin = g.shape[2:]
    d = F.pad(x.view(X, Y, Z, cin), (0, 0, 1, 1))                        # d[z + 1] = x[z], zero rows at -1 and Z
    d0, d1, d2, d3 = d[:, :, 0:Z:2], d[:, :, 1:Z + 1:2], d[:, :, 2:Z + 2:2], d[:, :, 3:Z + 3:2]
    t = [d0 - d2, d1 + d2, d2 - d1, d1 - d3]
    m = []
    for k in range(4):
        tk = rnd(t[k]).double().permute(2, 3, 0, 1)                       # [J, Cin, X, Y]
        wk = g[k].double().view(3, 3, cout, cin).permute(2, 3, 0, 1)      # [Cout, Cin, 3, 3]
        m.append(F.conv2d(tk, wk, padding=1))                             # [J, Cout, X, Y]
    y = torch.stack([m[0] + m[1] + m[2], m[1] - m[2] - m[3]], 1)          # [J, 2, Cout, X, Y]
    return y.permute(3, 4, 0, 1, 2).reshape(X * Y * Z, cout)


@pytest.mark.parametrize("mode,grid,shape,brick", [(1, (12, 20, 8), SHAPES[0], 1), (2, (20, 20, 8), SHAPES[1], 2)])
def test_one_product_modes_under_key_16(mode, grid, shape, brick, gpu_ops):
    """sgc_set_conv_products 1 (bf16) and 2 (fp16) on one shape each.  The oracle's Winograd twin has no reduced mode, so the
    yardstick is the float64 formulation on operands rounded to the mode -- only the fp32 accumulation separates the two -- with
    the bound the reduced-precision convolution tests hold against the same-mode oracle: 1e-5 of the tensor scale."""
    cin, cout = shape
    x, w, _, _, _ = _random_case(grid, cin, cout, False)
    g = gpu_ops.winograd_z_weights(w)
    if mode == 2:
        ghi, glo = gpu_ops.split_f16(g)
        rnd = lambda t: t.clamp(-65504.0, 65504.0).to(torch.float16)
        g_rounded = ghi.view(torch.float16)
    else:
        ghi, glo = gpu_ops.split_bf16(g)
        rnd = lambda t: t.to(torch.bfloat16)
        g_rounded = ghi
    want = _wino64_rounded(x, g_rounded, grid, rnd)
    try:
        gpu_ops.lib.call("sgc_set_conv_products", mode)
        with _tuned(gpu_ops, grid, wz_mfma=16, wz_brick=brick):
            got = _wino(gpu_ops, x, ghi, glo, grid, None, None, None, 0)
    finally:
        gpu_ops.lib.call("sgc_set_conv_products", 3)
    sc = max(1.0, float(want.abs().max()))
    err = float((got.cpu().double() - want).abs().max()) / sc
    print(f"mode {mode} {grid} {cin}->{cout} brick {brick} wz_mfma 16: {err:.2e} of the tensor scale")
    assert err < 1e-5


# ---- output coverage and non-finite input ---------------------------------------------------------------------------------------------
def _coverage_cases():
    from buffer_cases import _wz_case
    return [(_wz_case(grid, 64, 72, relu, True), grid, brick) for grid, relu, brick in (((12, 20, 8), 1, 1), ((12, 20, 8), 2, 2), ((10, 10, 4), 1, 2))]


@pytest.mark.parametrize("case,grid,brick", _coverage_cases(), ids=lambda v: str(v))
def test_every_output_element_is_written_and_nothing_beyond(case, grid, brick, oracle_ops, gpu_ops):
    """The buffer contract (tests/buffer_contract.py) under key 16: y and the workspace pre-filled with NaN and with a large finite
    value, guard bands around every allocation -- every output element written, nothing beyond, the result independent of the
    fill.  10 x 10 x 4 takes the split path."""
    from buffer_contract import run_case
    with _tuned(gpu_ops, grid, wz_mfma=16, wz_brick=brick, halo_split_target=192):
        run_case(case, gpu_ops, "cuda", ref_ops=oracle_ops)
    torch.cuda.synchronize()


@pytest.mark.parametrize("brick", [1, 2])
def test_non_finite_input_under_key_16(brick, oracle_ops, gpu_ops):
    """NaN and Inf input elements (tests/nonfinite_contract.py, the case of tests/test_gpu_nonfinite.py::test_conv3d_winograd_z): the
    outputs the float64-pinned oracle says depend on them are non-finite, all others finite and within 2e-5 of the scale."""
    import nonfinite_contract as nf
    from test_gpu_nonfinite import _conv3d_ref, _traced
    grid, cin, cout, relu = (12, 20, 8), 64, 72, 2
    case = (cin, cout, grid, 3, 1, False, True, relu)

    def gpu(i):
        ghi, glo = gpu_ops.split_bf16(gpu_ops.winograd_z_weights(i["wt"]))
        return _wino(gpu_ops, i["x"], ghi, glo, grid, i["sc"], i["sh"], i["res"], i["relu"])
    with _tuned(gpu_ops, grid, wz_mfma=16, wz_brick=brick):
        _traced(f"winograd-z {grid} wz_mfma 16 brick {brick}", lambda kind: nf.conv3d_inputs(case, kind, "x"), _conv3d_ref(oracle_ops), gpu,
                2e-5, kinds=("nan", "+inf"), z_pair_grid=grid)
