"""Checks of the convolutions and of the NCHW hand-over on the shapes nothing else runs -- odd grids under stride 2, axes of extent 1
and 2, output widths that are no multiple of 4, strided source views -- shared by the CPU (oracle) and the GPU (HIP library) test
modules: the same case lists and the same assertions run against either TensorOps.

The reference is float64 torch on the CPU (``F.conv3d`` / ``F.conv_transpose3d`` / ``F.conv2d``, their autograd, plain indexing),
never the oracle; the weight layouts are those of tests/test_oracle_conv.py.  Every bound is the one an existing test holds the same
entry to (named where it is used); nothing here introduces a tolerance.

"Refuse or be right": a case either computes -- torch's output shape, within the bound, a second call bit-identical -- or is refused
with SGC_EINVAL / SGC_EUNSUP where ``*_refusal`` below predicts it.  The predicates restate include/sgcdet_amd.h and nothing else; a
refusal they do not predict fails, and so does a predicted refusal that computes.  Two of the header's rules are limits of the HIP
kernels (``kernel_limits``): the oracle has one form of everything, never splits a reduction and computes those shapes."""
import functools
import re

import torch
import torch.nn.functional as F

CINS = (32, 96)
COUTS = (1, 3, 4, 7, 28, 33, 130)
FORMS = ((3, 1, False), (3, 2, False), (1, 1, False), (1, 2, False), (2, 2, False), (2, 2, True))      # ksize, stride, transposed
SMALL_GRIDS = ((1, 1, 1), (1, 1, 7), (1, 6, 1), (5, 1, 1), (2, 2, 2), (3, 3, 3), (7, 5, 3), (9, 7, 5), (13, 1, 11), (13, 11, 9))
HALO_GRIDS = ((17, 11, 13), (1, 48, 48), (45, 47, 1))       # >= 2048 voxels, 3 x 3 x 3 stride 1: bricks 4x8x8, 4x4x16 and 8x8x4, each ragged
HALO_COUTS = (28, 33, 130)
# Few output voxels -> the library splits the reduction, and a split layer refuses Cout % 4 != 0: on every grid above for the 27-tap
# forms.  A width that the split rule refuses on ALL listed grids of a form also runs on this grid (Cin 32), whose >= 512 row tiles
# fill the chip without a split: 65 559 and 41 x 41 x 40 = 67 240 output voxels.
LARGE_GRIDS = {(3, 1, False): (41, 41, 39), (3, 2, False): (81, 81, 79)}
ENTRIES = ("f32", "bf16x3")
FWD_TOL = {"f32": 2e-5, "bf16x3": 1e-4}     # of max(1, max |ref|): tests/test_gpu_conv3d.py, test_conv3d_cl_matches_oracle / test_conv3d_bf16x3_is_fp32_faithful
# epilogue of case i: EPILOGUES[i % 6] = (scale and shift, shift alone, residual, relu)
EPILOGUES = ((False, False, False, 0), (True, False, False, 0), (True, False, True, 1), (True, False, True, 2), (False, True, False, 1),
             (False, False, True, 0))

WGRAD_FORMS = ((3, 2), (1, 2), (2, 2))
WGRAD_GRIDS = ((7, 5, 3), (9, 7, 5), (1, 6, 1), (2, 2, 2), (13, 1, 11))
WGRAD_CINS = (32, 64)
WGRAD_COUTS = (4, 28, 132)

FUNCTION_FORMS = ((1, 2), (3, 2), (3, 1))
FUNCTION_GRIDS = ((7, 5, 3), (1, 6, 1), (2, 2, 2), (5, 1, 1), (13, 1, 11))
FUNCTION_COUTS = (25, 64)
TRANSPOSE_GRIDS = ((1, 1, 1), (1, 4, 1), (5, 1, 3))

# (1, 1, 2304): the pixels of the 16 x 16-pixel halo form on one row; (1, 47, 45): that form itself, ragged in both directions, so that
# a width that is no multiple of 4 also meets its element-wise stores
CONV2D_NHW = ((1, 1, 1), (2, 1, 9), (3, 7, 1), (1, 2, 2), (2, 17, 1), (1, 1, 2304), (1, 47, 45))
CONV2D_COUTS = (4, 28, 33)

CROP_SOURCES = ((1, 4, 8, 12), (2, 4, 8, 12), (3, 64, 9, 12), (2, 5, 15, 21), (1, 64, 16, 16), (2, 128, 16, 20), (2, 3, 7, 5), (1, 1, 1, 9),
                (2, 2, 9, 1))


# ======================================================================================================================================
# outcomes
# ======================================================================================================================================
def kernel_limits(ops):
    """The rules of the header that are limits of the HIP kernels, not of the operation."""
    return ops.device_type == "cuda"


def refused(fn):
    """(result, None) of ``fn()``, or (None, "SGC_EINVAL" | "SGC_EUNSUP") when the library refused the call.  Any other error -- a
    launch failure, a shape check of the Python front end -- propagates."""
    try:
        return fn(), None
    except RuntimeError as e:
        m = re.search(r"failed with status (-?\d+)", str(e))
        code = {-1: "SGC_EINVAL", -3: "SGC_EUNSUP"}.get(int(m.group(1))) if m else None
        if code is None:
            raise
        return None, code


def out_grid(grid, k, s, transposed=False):
    if transposed:
        return tuple(2 * d for d in grid)
    pad = 0 if k == 2 else k // 2
    return tuple((d + 2 * pad - k) // s + 1 for d in grid)


def split_floats(ops, entry, cin, cout, grid, form):
    k, s, tr = form
    return int(ops.lib._dll.sgc_conv3d_workspace_floats(*grid, cin, cout, k, s, int(tr), 1 if entry == "bf16x3" else 0))


def forward_refusal(ops, entry, cin, cout, grid, form):
    """sgcdet_amd.h, section 7: the reason for which sgc_conv3d_cl_f32 / _bf16x3 may refuse the layer, or None."""
    if 0 in out_grid(grid, *form):
        return "ksize 2 on an axis of extent 1 leaves no output"
    if cout % 4 and split_floats(ops, entry, cin, cout, grid, form) > 0:
        return "Cout % 4 != 0 on a layer that sgc_conv3d_workspace_floats reports as split"
    return None


def wgrad_refusal(ops, cin, cout, grid, k, s):
    """sgcdet_amd.h, sgc_conv3d_wgrad_bf16x3: Cin % 4 == 0 and Cout % 4 == 0 hold for every case here."""
    if 0 in out_grid(grid, k, s):
        return "ksize 2 on an axis of extent 1 leaves no output"
    if kernel_limits(ops) and k == 2 and any(d % 2 for d in grid):
        return "the kernels refuse ksize 2 on a grid with an odd axis"
    return None


def conv2d_refusal(ops, cout):
    """sgcdet_amd.h, sgc_conv2d_nhwc_bf16x3: Cin % 32 == 0 holds for every case here; any Cout, any image size, no split."""
    return None


class Tally:
    """computed / refused counts of one sweep, and the widths that were computed"""

    def __init__(self, what):
        self.what, self.computed, self.refused, self.couts, self.worst = what, 0, 0, set(), 0.0

    def line(self):
        return f"{self.what}: {self.computed} computed, {self.refused} refused, worst error {self.worst:.2e} of its bound"


def _settle(tally, got, code, why, label):
    """the two outcomes against the predicate; True when the case was computed"""
    if why is not None:
        assert got is None, f"{label}: computed although the header refuses it ({why})"
        tally.refused += 1
        return False
    assert code is None, f"{label}: refused with {code} and no rule of the header says so"
    tally.computed += 1
    return True


def _within(tally, got, ref, tol, floor, label):
    scale = float(ref.abs().max())
    bound = tol * (max(1.0, scale) if floor else scale)
    err = float((got.double().cpu() - ref).abs().max())
    tally.worst = max(tally.worst, err / bound if bound > 0 else float(err > 0))
    assert err < bound or (err == 0.0 and bound == 0.0), f"{label}: off by {err:.3e}, bound {bound:.3e}"


# ======================================================================================================================================
# float64 references, computed once per (layer, grid) at the widest Cout and sliced
# ======================================================================================================================================
def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * int(v) for i, v in enumerate(key)) % (2 ** 31))


def rows_of(t):
    """[1, C, X, Y, Z] -> channels-last rows [X*Y*Z, C]"""
    return t[0].permute(1, 2, 3, 0).reshape(-1, t.shape[1]).contiguous()


def volume_of(rows, grid):
    """channels-last rows [X*Y*Z, C] -> [1, C, X, Y, Z]"""
    return rows.view(*grid, rows.shape[1]).permute(3, 0, 1, 2).unsqueeze(0)


@functools.lru_cache(None)
def forward_weights(cin, form, cmax=max(COUTS)):
    """(the torch parameter, the entry points' [taps, Cout, Cin]) at the widest Cout; a narrower layer takes the first rows"""
    k, s, tr = form
    g = _gen(cin, k, s, tr, 7)
    if tr:
        w = torch.randn(cin, cmax, 2, 2, 2, generator=g) * (1.0 / cin ** 0.5)
        return w, w.permute(2, 3, 4, 1, 0).reshape(8, cmax, cin).contiguous()
    w = torch.randn(cmax, cin, k, k, k, generator=g) * (1.0 / (k ** 3 * cin) ** 0.5)
    return w, w.permute(2, 3, 4, 0, 1).reshape(k ** 3, cmax, cin).contiguous()


@functools.lru_cache(None)
def forward_input(cin, grid):
    return torch.randn(grid[0] * grid[1] * grid[2], cin, generator=_gen(cin, *grid))


@functools.lru_cache(64)
def forward_raw(cin, form, grid, cmax=max(COUTS)):
    """float64 rows [OV, cmax] of the bare convolution, or None where torch has no output either"""
    k, s, tr = form
    if 0 in out_grid(grid, k, s, tr):
        return None
    w = forward_weights(cin, form)[0].double()
    x = volume_of(forward_input(cin, grid).double(), grid)
    y = F.conv_transpose3d(x, w[:, :cmax], None, 2) if tr else F.conv3d(x, w[:cmax], None, s, 0 if k == 2 else k // 2)
    assert tuple(y.shape[2:]) == out_grid(grid, k, s, tr)
    return rows_of(y)


def epilogue_of(index, cout, rows):
    """(scale, shift, residual, relu) of case ``index``: fp32 tensors or None"""
    both, shift_only, use_res, relu = EPILOGUES[index % len(EPILOGUES)]
    g = _gen(index, cout, rows, 3)
    sc = torch.rand(cout, generator=g) + 0.5 if both else None
    sh = torch.randn(cout, generator=g) if both or shift_only else None
    res = torch.randn(rows, cout, generator=g) if use_res else None
    return sc, sh, res, relu


def apply_epilogue(raw, sc, sh, res, relu):
    """sgcdet_amd.h section 7 in float64: relu 1 = max(t + residual, 0), relu 2 = max(t, 0) + residual"""
    t = raw.clone()
    if sc is not None:
        t = t * sc.double()
    if sh is not None:
        t = t + sh.double()
    if relu == 2:
        t = t.clamp_min(0.0)
    if res is not None:
        t = t + res.double()
    if relu == 1:
        t = t.clamp_min(0.0)
    return t


# ======================================================================================================================================
# 2. forward sweep
# ======================================================================================================================================
def forward_cases(ops, entry, form):
    """[(cin, cout, grid)] of one entry and form: the listed grids; for 3 x 3 x 3 stride 1 the halo grids; and the large grid for every
    width that the header's split rule refuses on all of those."""
    cases = [(cin, cout, grid) for cin in CINS for grid in SMALL_GRIDS for cout in COUTS]
    if form == (3, 1, False):
        cases += [(cin, cout, grid) for cin in CINS for grid in HALO_GRIDS for cout in HALO_COUTS]
    if form in LARGE_GRIDS:
        open_widths = {cout for cin, cout, grid in cases if forward_refusal(ops, entry, cin, cout, grid, form) is None}
        cases += [(CINS[0], cout, LARGE_GRIDS[form]) for cout in COUTS if cout not in open_widths]
    return cases


def run_forward(ops, entry, x, wt, grid, form, sc, sh, res, relu):
    k, s, tr = form
    if entry == "f32":
        return ops.conv3d_cl(x, wt, grid, k, s, tr, sc, sh, res, relu)
    hi, lo = ops.split_bf16(wt)
    return ops.conv3d_cl_bf16x3(x, hi, lo, grid, k, s, tr, sc, sh, res, relu)


def check_forward_sweep(ops, device, entry, form):
    """Every case of ``forward_cases`` computes right or is refused by the header's rule; every width is computed at least once."""
    dev = lambda t: None if t is None else t.to(device)      # noqa: E731
    tally = Tally(f"{'sgc_conv3d_cl_' + entry} k{form[0]} s{form[1]}{' transposed' if form[2] else ''}")
    wt_all = {cin: dev(forward_weights(cin, form)[1]) for cin in CINS}
    x_dev = {}
    for index, (cin, cout, grid) in enumerate(forward_cases(ops, entry, form)):
        label = f"{tally.what}, Cin {cin}, Cout {cout}, grid {grid}, epilogue {index % len(EPILOGUES)}"
        why = forward_refusal(ops, entry, cin, cout, grid, form)
        raw = forward_raw(cin, form, grid)
        og = out_grid(grid, *form)
        ov = og[0] * og[1] * og[2]
        sc, sh, res, relu = epilogue_of(index, cout, ov)
        if (cin, grid) not in x_dev:
            x_dev = {(cin, grid): dev(forward_input(cin, grid))}
        x, wt = x_dev[(cin, grid)], wt_all[cin][:, :cout].contiguous()
        call = lambda: run_forward(ops, entry, x, wt, grid, form, dev(sc), dev(sh), dev(res), relu)      # noqa: E731
        got, code = refused(call)
        if not _settle(tally, got, code, why, label):
            continue
        y, og_got = got
        assert tuple(og_got) == og and tuple(y.shape) == (ov, cout), f"{label}: output grid {og_got}, torch's is {og}"
        _within(tally, y, apply_epilogue(raw[:, :cout], sc, sh, res, relu), FWD_TOL[entry], True, label)
        assert torch.equal(call()[0], y), f"{label}: the second call differs in bits"
        tally.couts.add(cout)
    print(tally.line())
    assert tally.couts == set(COUTS), f"{tally.what}: widths never computed: {sorted(set(COUTS) - tally.couts)}"
    return tally


def check_no_output_is_refused_before_any_store(ops, device):
    """ksize 2 on an axis of extent 1: C's (1 - 2) / 2 + 1 is 1, the callers' floor gives 0 rows.  The entry must refuse the call
    itself -- also when the caller hands it a real buffer -- and leave that buffer alone."""
    cin, cout, grid = 32, 4, (1, 6, 1)
    x = forward_input(cin, grid).to(device)
    wt = forward_weights(cin, (2, 2, False))[1][:, :cout].contiguous().to(device)
    hi, lo = ops.split_bf16(wt)
    for name, args in (("sgc_conv3d_cl_f32", (x, wt)), ("sgc_conv3d_cl_bf16x3", (x, hi, lo))):
        y = torch.full((3, cout), 7.0, device=device)             # the rows a truncating division would address
        _, code = refused(lambda: ops._call(name, *args, None, None, None, y, *grid, cin, cout, 2, 2, 0, 0, None, 0))
        assert code == "SGC_EINVAL", f"{name}: {code}"
        assert bool((y == 7.0).all()), f"{name}: wrote into the output of a call it refused"


# ======================================================================================================================================
# 3. training passes
# ======================================================================================================================================
@functools.lru_cache(None)
def wgrad_reference(k, s, grid, cin, cmax=max(WGRAD_COUTS)):
    """(x rows, dy rows [OV, cmax], float64 dW [k^3, cmax, cin] from torch's conv3d autograd), or None where there is no output"""
    og = out_grid(grid, k, s)
    if 0 in og:
        return None
    g = _gen(k, s, cin, *grid, 11)
    x = torch.randn(grid[0] * grid[1] * grid[2], cin, generator=g)
    dy = torch.randn(og[0] * og[1] * og[2], cmax, generator=g)
    w = torch.zeros(cmax, cin, k, k, k, dtype=torch.float64, requires_grad=True)
    y = F.conv3d(volume_of(x.double(), grid), w, None, s, 0 if k == 2 else k // 2)
    y.backward(volume_of(dy.double(), og))
    return x, dy, w.grad.permute(2, 3, 4, 0, 1).reshape(k ** 3, cmax, cin)


def wgrad_direct(ops, x, dy, grid, k, s):
    """sgc_conv3d_wgrad_bf16x3 itself, with the workspace its query asks for"""
    cin, cout = x.shape[1], dy.shape[1]
    n = int(ops.lib._dll.sgc_conv3d_wgrad_workspace_floats(*grid, cin, cout, k, s))
    ws = torch.empty(n, dtype=torch.float32, device=x.device) if n > 0 else None
    dw = torch.empty((k ** 3, cout, cin), dtype=torch.float32, device=x.device)
    ops._call("sgc_conv3d_wgrad_bf16x3", x, dy, dw, *grid, cin, cout, k, s, ws, max(n, 0))
    return dw


def check_wgrad_sweep(ops, device, k, s):
    """Bound: 1e-4 of max(1, max |ref|), two launches bit-identical (tests/test_gpu_conv3d.py, test_conv3d_wgrad_matches_oracle)."""
    tally = Tally(f"sgc_conv3d_wgrad_bf16x3 k{k} s{s}")
    for grid in WGRAD_GRIDS:
        for cin in WGRAD_CINS:
            ref = wgrad_reference(k, s, grid, cin)
            og = out_grid(grid, k, s)
            for cout in WGRAD_COUTS:
                label = f"{tally.what}, Cin {cin}, Cout {cout}, grid {grid}"
                why = wgrad_refusal(ops, cin, cout, grid, k, s)
                if ref is None:
                    x, dy = forward_input(cin, grid).to(device), torch.empty((0, cout), device=device)
                else:
                    x, dy = ref[0].to(device), ref[1][:, :cout].contiguous().to(device)
                got, code = refused(lambda: wgrad_direct(ops, x, dy, grid, k, s))
                if not _settle(tally, got, code, why, label):
                    continue
                _within(tally, got, ref[2][:, :cout], 1e-4, True, label)
                assert torch.equal(wgrad_direct(ops, x, dy, grid, k, s), got), f"{label}: the second launch differs in bits"
                if k == 2 and any(d % 2 for d in grid):
                    # no padding, stride 2: the last plane of an odd axis feeds no tap -- whatever it holds, dW stays what torch gives
                    xp = x.clone().view(*grid, cin)
                    xp[2 * og[0]:], xp[:, 2 * og[1]:], xp[:, :, 2 * og[2]:] = 1e6, 1e6, 1e6
                    assert torch.equal(wgrad_direct(ops, xp.view(-1, cin), dy, grid, k, s), got), f"{label}: the dropped plane reached dW"
                tally.couts.add(cout)
    print(tally.line())
    assert tally.couts == set(WGRAD_COUTS), f"{tally.what}: widths never computed: {sorted(set(WGRAD_COUTS) - tally.couts)}"
    return tally


class _ops_in_functions:
    """``sgcdet_amd.functions`` reaches the library through ``ext.ops()``: hand it ``ops`` (the oracle on the CPU) for the block"""

    def __init__(self, ops):
        self.ops = ops

    def __enter__(self):
        from sgcdet_amd import ext
        self.ext, self.saved = ext, ext.ops
        ext.ops = lambda: self.ops

    def __exit__(self, *exc):
        self.ext.ops = self.saved


def _rel(got, ref, label):
    """1e-4 of the tensor's max-abs: tests/test_gpu_conv3d.py, test_channels_last_conv_function_matches_torch_autograd"""
    err, scale = float((got.detach().double().cpu() - ref).abs().max()), float(ref.abs().max())
    assert scale > 0 and err < 1e-4 * scale, f"{label}: off by {err:.3e}, bound {1e-4 * scale:.3e}"
    return err / (1e-4 * scale)


def check_conv_function(ops, device, k, s, cin=32):
    """ChannelsLastConv3dFunction: y, dx (for stride 2 through the zero-interleaved dy, ``up[:2 * og:2]``) and dw against float64 autograd."""
    from sgcdet_amd.functions import ChannelsLastConv3dFunction
    worst = 0.0
    with _ops_in_functions(ops):
        for grid in FUNCTION_GRIDS:
            for cout in FUNCTION_COUTS:
                label = f"ChannelsLastConv3dFunction k{k} s{s}, Cin {cin}, Cout {cout}, grid {grid}"
                g = _gen(k, s, cout, *grid, 5)
                x = torch.randn(grid[0] * grid[1] * grid[2], cin, generator=g)
                w = torch.randn(cout, cin, k, k, k, generator=g) * 0.05
                xr, wr = volume_of(x.double(), grid).requires_grad_(True), w.double().requires_grad_(True)
                yr = F.conv3d(xr, wr, None, s, k // 2)
                gy = torch.randn(yr.shape, generator=g, dtype=torch.float64)
                yr.backward(gy)
                xg, wg = x.to(device).requires_grad_(True), w.to(device).requires_grad_(True)
                y = ChannelsLastConv3dFunction.apply(xg, wg, grid, k, s)
                assert tuple(y.shape) == tuple(rows_of(yr).shape), f"{label}: output rows {tuple(y.shape)}"
                worst = max(worst, _rel(y, rows_of(yr.detach()), label + ": y"))
                y.backward(rows_of(gy).float().to(device))
                worst = max(worst, _rel(xg.grad, rows_of(xr.grad), label + ": dx"), _rel(wg.grad, wr.grad, label + ": dw"))
    print(f"ChannelsLastConv3dFunction k{k} s{s}: {len(FUNCTION_GRIDS) * len(FUNCTION_COUTS)} layers, worst error {worst:.2e} of its bound")


def check_conv_transpose_function(ops, device, cin=64, cout=32):
    from sgcdet_amd.functions import ChannelsLastConvTranspose3dFunction
    worst = 0.0
    with _ops_in_functions(ops):
        for grid in TRANSPOSE_GRIDS:
            label = f"ChannelsLastConvTranspose3dFunction, grid {grid}"
            g = _gen(cin, cout, *grid, 9)
            x = torch.randn(grid[0] * grid[1] * grid[2], cin, generator=g)
            w = torch.randn(cin, cout, 2, 2, 2, generator=g) * 0.05
            xr, wr = volume_of(x.double(), grid).requires_grad_(True), w.double().requires_grad_(True)
            yr = F.conv_transpose3d(xr, wr, None, 2)
            gy = torch.randn(yr.shape, generator=g, dtype=torch.float64)
            yr.backward(gy)
            xg, wg = x.to(device).requires_grad_(True), w.to(device).requires_grad_(True)
            y = ChannelsLastConvTranspose3dFunction.apply(xg, wg, grid)
            assert tuple(y.shape) == (8 * x.shape[0], cout), label
            worst = max(worst, _rel(y, rows_of(yr.detach()), label + ": y"))
            y.backward(rows_of(gy).float().to(device))
            worst = max(worst, _rel(xg.grad, rows_of(xr.grad), label + ": dx"), _rel(wg.grad, wr.grad, label + ": dw"))
    print(f"ChannelsLastConvTranspose3dFunction: {len(TRANSPOSE_GRIDS)} layers, worst error {worst:.2e} of its bound")


# ======================================================================================================================================
# 4. the 2-D entry
# ======================================================================================================================================
@functools.lru_cache(None)
def conv2d_reference(nhw, k, cin, cmax=max(CONV2D_COUTS)):
    N, H, W = nhw
    g = _gen(N, H, W, k, cin, 13)
    x = torch.randn(N * H * W, cin, generator=g)
    w = torch.randn(cmax, cin, k, k, generator=g) * (1.0 / (k * k * cin) ** 0.5)
    y = F.conv2d(x.double().view(N, H, W, cin).permute(0, 3, 1, 2), w.double(), None, 1, k // 2)
    return x, w.permute(2, 3, 0, 1).reshape(k * k, cmax, cin).contiguous(), y.permute(0, 2, 3, 1).reshape(N * H * W, cmax)


def check_conv2d_sweep(ops, device, k):
    """sgc_conv2d_nhwc_bf16x3 on images with a unit side; bound 1e-4 of max(1, max |ref|) (test_conv2d_nhwc_matches_oracle_and_torch)."""
    dev = lambda t: None if t is None else t.to(device)      # noqa: E731
    tally = Tally(f"sgc_conv2d_nhwc_bf16x3 k{k}")
    index = 0
    for nhw in CONV2D_NHW:
        for cin in CINS:
            x, wt, raw = conv2d_reference(nhw, k, cin)
            for cout in CONV2D_COUTS:
                label = f"{tally.what}, Cin {cin}, Cout {cout}, (N, H, W) {nhw}, epilogue {index % len(EPILOGUES)}"
                sc, sh, res, relu = epilogue_of(index, cout, x.shape[0])
                index += 1
                hi, lo = ops.split_bf16(dev(wt[:, :cout].contiguous()))
                call = lambda: ops.conv2d_nhwc_bf16x3(dev(x), hi, lo, nhw, k, dev(sc), dev(sh), dev(res), relu)      # noqa: E731
                got, code = refused(call)
                if not _settle(tally, got, code, conv2d_refusal(ops, cout), label):
                    continue
                assert tuple(got.shape) == (x.shape[0], cout), label
                _within(tally, got, apply_epilogue(raw[:, :cout], sc, sh, res, relu), 1e-4, True, label)
                assert torch.equal(call(), got), f"{label}: the second call differs in bits"
                tally.couts.add(cout)
    print(tally.line())
    return tally


# ======================================================================================================================================
# 5. sgc_nchw_to_nhwc_crop on views
# ======================================================================================================================================
def crop_views(base):
    """[(name, view)] of one source: every-``s``-th-pixel views with and without an offset, and the views the front end must copy"""
    N, C, Hs, Ws = base.shape
    views = [(f"[{oy}::{sy}, {ox}::{sx}]", base[..., oy::sy, ox::sx]) for sy in (1, 2, 4) for sx in (1, 2, 4) for oy in (0, 1) for ox in (0, 1)]
    views += [("channel slice", base[:, C // 2:]), ("image slice", base[N // 2:]), ("[::2] over images", base[::2]),
              ("H and W transposed", base.transpose(2, 3)), ("expanded channel", base[:, :1].expand(-1, 3, -1, -1))]
    return [(n, v) for n, v in views if v.numel() > 0]


def crops_of(h, w):
    return sorted({(h, w), (max(1, h - 1), w), (h, max(1, w - 1)), (max(1, h // 2), max(1, w // 2))})


def check_crop_views(ops, device):
    """Bit-exact against ``v[..., :H, :W].permute(0, 2, 3, 1).reshape(N, H * W, C)``.  Returns what reached the library: the steps of
    the launches that read the caller's storage in place, and how many launches met the conditions of the 16-byte form."""
    in_place, vector_form, n = {}, 0, 0
    seen = []
    orig = ops._call

    def spy(name, *args, **kw):
        seen.append((name, args))
        return orig(name, *args, **kw)
    ops._call = spy
    try:
        for shape in CROP_SOURCES:
            numel = shape[0] * shape[1] * shape[2] * shape[3]
            base = (torch.arange(numel, dtype=torch.float32) - numel // 2).view(shape)        # every element its own value
            base_dev = base.to(device)
            for (name, v), (_, v_dev) in zip(crop_views(base), crop_views(base_dev)):
                for H, W in crops_of(v.shape[2], v.shape[3]):
                    del seen[:]
                    got = ops.nchw_to_nhwc_crop(v_dev, H, W)
                    want = v[..., :H, :W].permute(0, 2, 3, 1).reshape(v.shape[0], H * W, v.shape[1])
                    assert torch.equal(got.cpu(), want), f"source {shape}, view {name}, crop {(H, W)}"
                    n += 1
                    (entry, args), = seen
                    assert entry == "sgc_nchw_to_nhwc_crop"
                    src, C, Ws, step = args[0], args[3], args[5], args[8]
                    if src.data_ptr() == v_dev.data_ptr() and not v_dev.is_contiguous():
                        in_place[step] = in_place.get(step, 0) + 1
                    vector_form += int(step == 1 and C % 64 == 0 and W % 4 == 0 and Ws % 4 == 0 and src.data_ptr() % 16 == 0)
    finally:
        del ops.__dict__["_call"]
    print(f"sgc_nchw_to_nhwc_crop: {n} view / crop combinations; read in place by step: {dict(sorted(in_place.items()))}; "
          f"{vector_form} met the conditions of the 16-byte form")
    return in_place, vector_form
