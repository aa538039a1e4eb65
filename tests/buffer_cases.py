"""The case table of the buffer tests (tests/buffer_contract.py): one ``Case`` per kernel family an entry point can dispatch to, at the
smallest shape of the existing parametrisations that reaches the family.  Shapes, seeds' style, references and bounds are those of the
tests named in each section; nothing here introduces a tolerance.  Pair lists and other derived INPUTS are made with the oracle (as the
existing tests make them); a reference is the oracle's twin of the entry (``ref=None``) or a float64 torch formulation."""
import functools

import torch
import torch.nn.functional as F

from buffer_contract import Case

CASES = []


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(None)
def _oracle():
    import oracle
    oracle.build()
    return oracle.ops()


def _cuda(ops):
    return ops.device_type == "cuda"


def _tuned(ops, key, value, back, fn):
    """``fn()`` with the tuning key set (on the GPU library; the oracle has one form of everything), put back afterwards."""
    if not _cuda(ops):
        return fn()
    ops.lib.call("sgc_set_tuning", key, value)
    try:
        return fn()
    finally:
        ops.lib.call("sgc_set_tuning", key, back)


# ======================================================================================================================================
# 3-D convolution forward (tests/test_gpu_conv3d.py: CASES; bounds 1e-4 bf16x3 / 2e-5 f32 of the scale against the oracle)
# ======================================================================================================================================
def _conv3d_build(c):
    Cin, Cout, grid, k, s, tr, use_res, relu = c

    def build():
        g = _gen(sum(grid) + Cin + Cout + k + s)
        V = grid[0] * grid[1] * grid[2]
        taps = 8 if tr else k ** 3
        x = torch.randn(V, Cin, generator=g)
        wt = torch.randn(taps, Cout, Cin, generator=g) * (1.0 / (taps * Cin) ** 0.5)
        sc, sh = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g)
        pad = 0 if k == 2 else k // 2
        og = tuple(2 * d for d in grid) if tr else tuple((d + 2 * pad - k) // s + 1 for d in grid)
        res = torch.randn(og[0] * og[1] * og[2], Cout, generator=g) if use_res else None
        hi, lo = _oracle().split_bf16(wt)
        return dict(x=x, wt=wt, hi=hi, lo=lo, sc=sc, sh=sh, res=res)
    return build


def _conv3d_run(c, f32=False, **kw):
    Cin, Cout, grid, k, s, tr, use_res, relu = c

    def run(ops, t):
        if f32:
            return dict(y=ops.conv3d_cl(t["x"], t["wt"], grid, k, s, tr, t["sc"], t["sh"], t["res"], relu)[0])
        return dict(y=ops.conv3d_cl_bf16x3(t["x"], t["hi"], t["lo"], grid, k, s, tr, t["sc"], t["sh"], t["res"], relu, **kw)[0])
    return run


def _is_split(c, bf16x3):
    Cin, Cout, grid, k, s, tr, _, _ = c

    def needs(ops):
        if _cuda(ops):
            assert int(ops.lib._dll.sgc_conv3d_workspace_floats(*grid, Cin, Cout, k, s, int(tr), bf16x3)) > 0, "the layer is not split"
    return needs


CONV3D = [  # family, (Cin, Cout, grid, ksize, stride, transposed, residual, relu)
    ("tile", (32, 128, (10, 10, 4), 3, 1, False, True, True)),
    ("split_k", (64, 256, (5, 5, 2), 3, 1, False, True, True)),
    ("narrow", (32, 32, (7, 5, 3), 3, 1, False, False, False)),
    ("k1s2", (64, 128, (6, 4, 4), 1, 2, False, False, False)),
    ("transposed", (64, 128, (5, 4, 3), 2, 2, True, False, True)),
    ("k2s2", (64, 96, (8, 6, 4), 2, 2, False, False, False)),
    ("halo_4x4x16", (64, 128, (16, 16, 16), 3, 1, False, True, True)),
    ("halo_4x8x8", (64, 128, (20, 20, 8), 3, 1, False, True, 2)),
    ("halo_8x8x4", (32, 64, (24, 24, 4), 3, 1, False, False, True)),
    ("halo_ragged", (64, 192, (17, 13, 16), 3, 1, False, True, True)),
    ("whole_grid_512", (64, 512, (10, 10, 4), 3, 1, False, True, True)),
    ("whole_grid_576", (96, 576, (12, 12, 4), 3, 1, False, True, 2)),
    ("head_28_columns", (128, 28, (20, 20, 8), 3, 1, False, False, False)),
]
for _fam, _c in CONV3D:
    CASES.append(Case(f"conv3d_bf16x3-{_fam}", ("sgc_conv3d_cl_bf16x3",), _conv3d_build(_c), _conv3d_run(_c), tol=1e-4,
                      needs=_is_split(_c, 1) if _fam == "split_k" else None))
    if _fam in ("tile", "split_k", "narrow", "k1s2", "transposed", "k2s2", "halo_ragged"):          # the f32 entry shares the dispatch: the
        CASES.append(Case(f"conv3d_f32-{_fam}", ("sgc_conv3d_cl_f32",), _conv3d_build(_c), _conv3d_run(_c, f32=True), tol=2e-5,     # families
                          needs=_is_split(_c, 0) if _fam == "split_k" else None))                                                   # it has


def _split_without_workspace(ops, t):
    """The split layer with no workspace: float atomics into an output the entry zero-fills itself (tests/test_gpu_conv3d.py)."""
    y = torch.empty((5 * 5 * 2, 256), dtype=torch.float32, device=t["x"].device)
    ops._call("sgc_conv3d_cl_bf16x3", t["x"], t["hi"], t["lo"], t["sc"], t["sh"], t["res"], y, 5, 5, 2, 64, 256, 3, 1, 0, 1, None, 0)
    return dict(y=y)


CASES.append(Case("conv3d_bf16x3-split_k_no_workspace", ("sgc_conv3d_cl_bf16x3",), _conv3d_build(CONV3D[1][1]), _split_without_workspace, tol=1e-4,
                  bits=False, needs=_is_split(CONV3D[1][1], 1)))


def _act_build(grid, cin, cout):
    def build():
        g = _gen(sum(grid) + cout)
        x = torch.randn(grid[0] * grid[1] * grid[2], cin, generator=g)
        hi, lo = _oracle().split_bf16(torch.randn(27, cout, cin, generator=g) * 0.02)
        return dict(x=x, hi=hi, lo=lo, sh=torch.randn(cout, generator=g) * 0.1, s=torch.tensor(0.83))
    return build


CASES.append(Case("conv3d_act-head_epilogue", ("sgc_conv3d_cl_bf16x3_act",), _act_build((10, 10, 4), 128, 28),
                  lambda ops, t: dict(y=ops.conv3d_cl_bf16x3(t["x"], t["hi"], t["lo"], (10, 10, 4), 3, 1, False, None, t["sh"], None, 0,
                                                            act=(1, 7, t["s"]))[0]), tol=1e-4))

_MASKED = (64, 28, (16, 16, 4), 3, 1, False, False, 0)


def _masked_build():
    d = _conv3d_build(_MASKED)()
    grid = _MASKED[2]
    blob = torch.zeros(grid)
    blob[: grid[0] // 3, grid[1] // 4: grid[1] // 2, :] = 1           # a slab: whole bricks dead elsewhere
    blob[-3:, -2:, -1:] = 1                                              # and a small corner cluster
    d["mask"] = blob.reshape(-1).to(torch.uint8)
    return d


def _masked_run(ops, t):
    return dict(y=ops.conv3d_cl_bf16x3(t["x"], t["hi"], t["lo"], _MASKED[2], 3, 1, False, t["sc"], t["sh"], None, 0, out_mask=t["mask"])[0])


def _masked_ref_run(ops, t):
    return dict(y=ops.conv3d_cl_bf16x3(t["x"], t["hi"], t["lo"], _MASKED[2], 3, 1, False, t["sc"], t["sh"], None, 0)[0])


CASES.append(Case("conv3d_masked-live_rows", ("sgc_conv3d_cl_bf16x3_masked",), _masked_build, _masked_run, ref_run=_masked_ref_run, tol=1e-4,
                  extent=lambda r, i: dict(y=i["mask"].bool()[:, None]),
                  undefined="sgcdet_amd.h, sgc_conv3d_cl_bf16x3_masked: rows with mask 0 hold the epilogue of a zero accumulator or the dense value"))


def _wz_build(grid, cin, cout, res):
    def build():
        g = _gen(sum(grid) + cin)
        V = grid[0] * grid[1] * grid[2]
        x = torch.randn(V, cin, generator=g)
        w = torch.randn(27, cout, cin, generator=g) * (1.0 / (27 * cin) ** 0.5)
        o = _oracle()
        hi, lo = o.split_bf16(w)
        ghi, glo = o.split_bf16(o.winograd_z_weights(w))
        return dict(x=x, hi=hi, lo=lo, ghi=ghi, glo=glo, sc=torch.rand(cout, generator=g) + 0.5, sh=torch.randn(cout, generator=g),
                    res=torch.randn(V, cout, generator=g) if res else None)
    return build


def _wz_case(grid, cin, cout, relu, res):
    def run(ops, t):
        return dict(y=ops.conv3d_winograd_z(t["x"], t["ghi"], t["glo"], grid, t["sc"], t["sh"], t["res"], relu)[0])

    def direct(ops, t):                # the reference of tests/test_gpu_conv3d.py: the oracle's DIRECT convolution, 2e-5 of the scale
        return dict(y=ops.conv3d_cl_bf16x3(t["x"], t["hi"], t["lo"], grid, 3, 1, False, t["sc"], t["sh"], t["res"], relu)[0])

    def needs(ops):
        if _cuda(ops):
            assert ops.conv3d_winograd_z_supported(grid, cin, cout)
            assert grid[2] != 4 or int(ops.lib._dll.sgc_conv3d_winograd_z_workspace_floats(*grid, cin, cout)) > 0
    return Case(f"conv3d_winograd_z-{'x'.join(map(str, grid))}", ("sgc_conv3d_winograd_z_bf16x3",), _wz_build(grid, cin, cout, res), run,
                ref_run=direct, tol=2e-5, needs=needs)


CASES += [_wz_case((16, 16, 16), 64, 128, 1, True), _wz_case((10, 10, 4), 64, 72, 1, True), _wz_case((12, 10, 4), 64, 72, 2, True)]


def _out_of(rows, cols, like):
    return torch.empty((rows, cols), dtype=torch.float32, device=like.device)


# ``out=``: the caller's buffer of the full shape (guarded like any allocation)
_c = CONV3D[0][1]
CASES.append(Case("conv3d_bf16x3-tile-out", ("sgc_conv3d_cl_bf16x3",), _conv3d_build(_c),
                  lambda ops, t: dict(y=ops.conv3d_cl_bf16x3(t["x"], t["hi"], t["lo"], (10, 10, 4), 3, 1, False, t["sc"], t["sh"], t["res"], True,
                                                            out=_out_of(400, 128, t["x"]))[0]), tol=1e-4))
CASES.append(Case("conv3d_winograd_z-10x10x4-out", ("sgc_conv3d_winograd_z_bf16x3",), _wz_build((10, 10, 4), 64, 72, True),
                  lambda ops, t: dict(y=ops.conv3d_winograd_z(t["x"], t["ghi"], t["glo"], (10, 10, 4), t["sc"], t["sh"], t["res"], 1, out=_out_of(400, 72, t["x"]))[0]),
                  ref_run=lambda ops, t: dict(y=ops.conv3d_cl_bf16x3(t["x"], t["hi"], t["lo"], (10, 10, 4), 3, 1, False, t["sc"], t["sh"], t["res"], 1)[0]),
                  tol=2e-5))


# ======================================================================================================================================
# 3-D weight gradient, pack / unpack (tests/test_gpu_conv3d.py: WGRAD_CASES, 1e-4 of the scale; the layout passes are exact)
# ======================================================================================================================================
WGRAD = [(64, 128, (10, 9, 4), 3, 1), (32, 28, (7, 5, 6), 3, 1), (64, 128, (8, 6, 4), 3, 2), (64, 132, (6, 4, 4), 1, 2), (96, 64, (8, 6, 4), 2, 2),
         (64, 96, (9, 10, 5), 3, 1), (32, 64, (17, 8, 4), 3, 1)]


def _wgrad_case(c, halo=None):
    Cin, Cout, grid, k, s = c

    def build():
        g = _gen(sum(grid) + Cin + Cout)
        pad = 0 if k == 2 else k // 2
        og = tuple((d + 2 * pad - k) // s + 1 for d in grid)
        return dict(x=torch.randn(grid[0] * grid[1] * grid[2], Cin, generator=g), dy=torch.randn(og[0] * og[1] * og[2], Cout, generator=g))

    def run(ops, t):
        go = lambda: dict(dw=ops.conv3d_wgrad_bf16x3(t["x"], t["dy"], grid, k, s))               # noqa: E731
        return go() if halo is None else _tuned(ops, b"wgrad_halo", halo, 1, go)
    name = f"conv3d_wgrad-{Cin}-{Cout}-{'x'.join(map(str, grid))}-k{k}s{s}" + ("" if halo is None else f"-halo{halo}")
    return Case(name, ("sgc_conv3d_wgrad_bf16x3",), build, run, tol=1e-4, only="cuda" if halo in (0, 2) else None)


CASES += [_wgrad_case(c) for c in WGRAD] + [_wgrad_case((64, 128, (24, 17, 9), 3, 1), h) for h in (0, 1, 2)]

_PACK_SHAPE, _PACK_FORMS = (70, 33, 3, 3, 3), ((False, False, 4, 1), (True, True, 1, 32))


def _pack_build():
    return dict(w=torch.randn(*_PACK_SHAPE, generator=_gen(sum(_PACK_SHAPE))))


def _packed_torch(w, transpose, flip, pr, pc):
    A, B = w.shape[0], w.shape[1]
    w3 = w.reshape(A, B, -1)
    src = w3.flip(2) if flip else w3
    ref = src.permute(2, 1, 0) if transpose else src.permute(2, 0, 1)
    full = torch.zeros(ref.shape[0], -(-ref.shape[1] // pr) * pr, -(-ref.shape[2] // pc) * pc)
    full[:, :ref.shape[1], :ref.shape[2]] = ref
    return full


def _pack_run(ops, t):
    out = {}
    for n, (tr, fl, pr, pc) in enumerate(_PACK_FORMS):
        hi, lo = ops.pack_conv_weight(t["w"], transpose=tr, flip=fl, pad_rows=pr, pad_cols=pc)
        out[f"hi{n}"], out[f"lo{n}"] = hi, lo
    return out


def _pack_ref(i):
    out = {}
    for n, form in enumerate(_PACK_FORMS):
        hi, lo = _oracle().split_bf16(_packed_torch(i["w"], *form))
        out[f"hi{n}"], out[f"lo{n}"] = hi, lo
    return out


CASES.append(Case("pack_conv_weight", ("sgc_pack_conv_weight",), _pack_build, _pack_run, ref=_pack_ref, tol=0.0))


def _pack_out_run(ops, t):
    out = {}
    for n, (tr, fl, pr, pc) in enumerate(_PACK_FORMS):
        T, R, Cc = ops.packed_shape(_PACK_SHAPE, tr, pr, pc)
        planes = tuple(torch.empty((T, R, Cc), dtype=torch.bfloat16, device=t["w"].device) for _ in range(2))
        out[f"hi{n}"], out[f"lo{n}"] = ops.pack_conv_weight(t["w"], transpose=tr, flip=fl, pad_rows=pr, pad_cols=pc, out=planes)
    return out


CASES.append(Case("pack_conv_weight-out", ("sgc_pack_conv_weight",), _pack_build, _pack_out_run, ref=_pack_ref, tol=0.0))


def _pack_batch_run(ops, t):
    """The batch form keeps the planes' padding as allocated (sgcdet_amd.h: "NOT written: allocate them zeroed"): the planes are made
    here, guarded, and zeroed as the header asks."""
    entries, out = [], {}
    for n, (tr, fl, pr, pc) in enumerate(_PACK_FORMS):
        T, R, Cc = ops.packed_shape(_PACK_SHAPE, tr, pr, pc)
        hi = torch.empty((T, R, Cc), dtype=torch.bfloat16, device=t["w"].device).zero_()
        lo = torch.empty_like(hi).zero_()
        entries.append((t["w"], hi, lo, tr, fl))
        out[f"hi{n}"], out[f"lo{n}"] = hi, lo
    ops.run_pack_plan(ops.pack_conv_weight_plan(entries))
    return out


CASES.append(Case("pack_conv_weight_batch", ("sgc_pack_conv_weight_batch", "sgc_pack_conv_weight_blocks"), _pack_build, _pack_batch_run,
                  ref=_pack_ref, tol=0.0))


def _unpack_run(ops, t):
    return {f"w{n}": ops.unpack_conv_wgrad(t[f"full{n}"], _PACK_SHAPE, transpose=tr, flip=fl) for n, (tr, fl, _, _) in enumerate(_PACK_FORMS)}


CASES.append(Case("unpack_conv_wgrad", ("sgc_unpack_conv_wgrad",),
                  lambda: {f"full{n}": _packed_torch(_pack_build()["w"], *form) for n, form in enumerate(_PACK_FORMS)}, _unpack_run,
                  ref=lambda i: {f"w{n}": _pack_build()["w"] for n in range(len(_PACK_FORMS))}, tol=0.0))


# ======================================================================================================================================
# 2-D convolution with an oracle twin, mask kernels
# ======================================================================================================================================
def _conv2d_case(N, H, W, cin, cout, k, relu, res, halo, out=False):
    """Rows of tests/test_gpu_conv3d.py::test_conv2d_nhwc_matches_oracle_and_torch (1e-4 of the scale against the oracle).  ``halo``: a
    3 x 3 launch with >= 2048 pixels and H, W >= 8 takes the 2-D form of the halo kernel (16 x 16-pixel bricks: ragged last rows and
    columns, 28 or 160 live columns of a 64- / 128-column tile); the others take the tile kernel.  ``out``: into the caller's buffer."""
    def build():
        g = _gen(N * H + cin + cout)
        x = torch.randn(N * H * W, cin, generator=g)
        wt = (torch.randn(cout, cin, k, k, generator=g) * 0.05).permute(2, 3, 0, 1).reshape(k * k, cout, cin).contiguous()
        hi, lo = _oracle().split_bf16(wt)
        return dict(x=x, hi=hi, lo=lo, sc=torch.rand(cout, generator=g) + 0.5, sh=torch.randn(cout, generator=g),
                    res=torch.randn(N * H * W, cout, generator=g) if res else None)

    def run(ops, t):
        o = torch.empty((N * H * W, cout), dtype=torch.float32, device=t["x"].device) if out else None
        return dict(y=ops.conv2d_nhwc_bf16x3(t["x"], t["hi"], t["lo"], (N, H, W), k, t["sc"], t["sh"], t["res"], relu, out=o))

    def needs(ops):
        assert (k == 3 and N * H * W >= 2048 and min(H, W) >= 8) == halo
    return Case(f"conv2d_nhwc-{N}x{H}x{W}-{cin}-{cout}-{'halo_2d' if halo else 'tile'}" + ("-out" if out else ""), ("sgc_conv2d_nhwc_bf16x3",), build, run,
                tol=1e-4, needs=needs)


CASES += [_conv2d_case(1, 7, 5, 96, 28, 3, 2, True, False), _conv2d_case(1, 7, 5, 96, 28, 3, 2, True, False, out=True),
          _conv2d_case(7, 16, 20, 96, 160, 3, 0, False, True),           # 2240 pixels: bricks of 16 x 16, a ragged last column brick (20 = 16 + 4)
          _conv2d_case(5, 37, 45, 64, 28, 3, 1, True, True)]             # ragged in both directions (37 = 32 + 5, 45 = 32 + 13), 28 live columns


def _mask_build(grid, density, seed=0):
    return lambda: dict(mask=(torch.rand(grid[0] * grid[1] * grid[2], generator=_gen(sum(grid) + seed)) < density).to(torch.uint8))


def dilate3_ref(mask, grid):
    return F.max_pool3d(mask.view(1, 1, *grid).float(), 3, 1, 1).view(-1).to(torch.uint8)


def valid_pyramid_ref(valid, grid, factor):
    """The formulation the entry's comment cites: nn.Upsample(size, mode='trilinear')(valid.float()).round().bool()."""
    size = tuple(d // factor for d in grid)
    return torch.nn.Upsample(size=size, mode="trilinear")(valid.view(1, 1, *grid).float()).round().bool().view(-1).to(torch.uint8)


for _grid in ((8, 8, 4), (4, 12, 8)):
    CASES.append(Case(f"mask_dilate3-{'x'.join(map(str, _grid))}", ("sgc_mask_dilate3",), _mask_build(_grid, 0.1),
                      lambda ops, t, g=_grid: dict(out=ops.mask_dilate3(t["mask"], g)), ref=lambda i, g=_grid: dict(out=dilate3_ref(i["mask"], g)), tol=0.0))
    for _f in (1, 2, 4):
        CASES.append(Case(f"valid_pyramid-{'x'.join(map(str, _grid))}-f{_f}", ("sgc_valid_pyramid",),
                          lambda g=_grid: dict(valid=_mask_build(g, 0.5, 1)()["mask"].to(torch.int64)),
                          lambda ops, t, g=_grid, f=_f: dict(out=ops.valid_pyramid(t["valid"], g, f)),
                          ref=lambda i, g=_grid, f=_f: dict(out=valid_pyramid_ref(i["valid"], g, f)), tol=0.0))


# ======================================================================================================================================
# the DFA3D operators (tests/test_gpu_kernels.py: SHAPES; forward 1e-5, backward 2e-5 of the scale against the oracle).  The backward
# kernels accumulate with float atomics (sgcdet_amd.h): no bit identity, each kind meets the bound on its own.
# ======================================================================================================================================
def _dfa3d_build(shape, seed):
    def build():
        from test_gpu_kernels import make_inputs
        B, M, Cm, D, Q, P, levels, rep = shape
        d = make_inputs(shape, seed)
        d["go"] = torch.randn(B, Q, M * Cm, generator=_gen(9))
        return d
    return build


def _dfa3d_fwd(ops, t):
    out, score = ops.dfa3d_forward(t["value"], t["dist"], t["shapes3"], t["lsi"], t["loc"], t["attn"], want_score=True)
    return dict(out=out, score=score)


def _dfa3d_bwd(ops, t):
    gv, gd, gl, ga = ops.dfa3d_backward(t["value"], t["dist"], t["shapes3"], t["lsi"], t["loc"], t["attn"], t["go"])
    return dict(grad_value=gv, grad_dist=gd, grad_loc=gl, grad_attn=ga)


def _split_ext(ops, t):
    s2, l2 = t["shapes3"][:, :2].contiguous(), t["loc"][..., :2].contiguous()
    score = ops.depth_score_forward(t["dist"], t["shapes3"], t["lsi"], t["loc"])
    out = ops.wms_forward(t["value"], s2, t["lsi"], l2, t["attn"], score)
    gv, gl2, ga, gs = torch.zeros_like(t["value"]), torch.zeros_like(l2), torch.zeros_like(t["attn"]), torch.zeros_like(score)
    ops.wms_backward(t["value"], s2, t["lsi"], l2, t["attn"], score, t["go"], gv, gl2, ga, gs)
    gd, gl3 = torch.zeros_like(t["dist"]), torch.zeros_like(t["loc"])
    ops.depth_score_backward(t["dist"], t["shapes3"], t["lsi"], t["loc"], gs, gd, gl3)
    return dict(score=score, out=out, grad_value=gv, grad_loc2=gl2, grad_attn=ga, grad_score=gs, grad_dist=gd, grad_loc3=gl3)


_BWD_NAMES = ("grad_value", "grad_loc2", "grad_attn", "grad_score", "grad_dist", "grad_loc3")
for _tag, _shape in (("C32_replicated_depth", (2, 8, 4, 12, 77, 4, [(7, 9)], True)), ("scalar_path", (2, 2, 5, 7, 33, 2, [(6, 5)], False))):
    CASES.append(Case(f"dfa3d_forward-{_tag}", ("sgc_dfa3d_forward",), _dfa3d_build(_shape, 0), _dfa3d_fwd, tol=1e-5))
    CASES.append(Case(f"dfa3d_backward-{_tag}", ("sgc_dfa3d_backward",), _dfa3d_build(_shape, 2), _dfa3d_bwd, tol=2e-5, bits=False,
                      accumulated=("grad_value", "grad_dist")))
CASES.append(Case("dfa3d_split_operators", ("sgc_depth_score_forward", "sgc_wms_forward", "sgc_wms_backward", "sgc_depth_score_backward"),
                  _dfa3d_build((2, 8, 4, 12, 77, 4, [(7, 9)], True), 3), _split_ext, tol=dict(score=1e-5, out=1e-5, **{k: 2e-5 for k in _BWD_NAMES}),
                  bits=dict(score=True, out=True, **{k: False for k in _BWD_NAMES}), accumulated=_BWD_NAMES))


def _items_build():
    B, S_hw, M, Cm, D, L, P, n = 4, (9, 11), 8, 8, 6, 1, 4, 333
    g = _gen(77)
    S = S_hw[0] * S_hw[1]
    return dict(value=torch.randn(B, S, M, Cm, generator=g), dist=torch.randn(B, S, 1, D, generator=g).mul(2).softmax(-1).contiguous(),
                shapes3=torch.tensor([[S_hw[0], S_hw[1], D]], dtype=torch.int64), lsi=torch.zeros(1, dtype=torch.int64),
                loc=(torch.rand(n, M, L, P, 3, generator=g) * 1.3 - 0.15).contiguous(), attn=torch.rand(n, M, L, P, generator=g),
                item=torch.randint(0, B, (n,), generator=g, dtype=torch.int32).sort().values.contiguous(), go=torch.randn(n, M * Cm, generator=g))


def _items_run(ops, t):
    a = (t["value"], t["dist"], t["shapes3"], t["lsi"], t["loc"], t["attn"], t["item"])
    gv, gd, gl, ga = ops.dfa3d_backward_items(*a, t["go"])
    return dict(out=ops.dfa3d_forward_items(*a), grad_value=gv, grad_dist=gd, grad_loc=gl, grad_attn=ga)


CASES.append(Case("dfa3d_items", ("sgc_dfa3d_forward_items", "sgc_dfa3d_backward_items"), _items_build, _items_run,
                  tol=dict(out=1e-5, grad_value=2e-5, grad_dist=2e-5, grad_loc=2e-5, grad_attn=2e-5),
                  bits=dict(out=True, grad_value=False, grad_dist=False, grad_loc=False, grad_attn=False), accumulated=("grad_value", "grad_dist")))


# ======================================================================================================================================
# projection, pair lists and gathers (tests/test_gpu_kernels.py: test_pair_list_gathers_and_view_pool at (32, 8, 4, (7, 10)),
# test_tiled_gather_against_oracle at (128, (14, 20), (20, 14), (0, 0)), test_binned_backward_against_oracle at (16, (14, 20), ...)).
# Every scene has 0 < count < capacity, so that the capacity tails exist.
# ======================================================================================================================================
def _scene_build(N, Nq, seed, with_sel=False):
    def build():
        from count_contract import _scene
        ref3d, origin, proj = _scene(N, Nq, seed)
        d = dict(ref3d=ref3d, origin=origin, proj=proj)
        if with_sel:
            d["sel"] = torch.randperm(Nq, generator=_gen(1))[: Nq // 3].sort().values
        return d
    return build


def _project_run(ops, t):
    rc, mk = ops.project_points(t["ref3d"], t["origin"], t["proj"], 320., 239., 0.2, 5.0, sel=t.get("sel"))
    return dict(ref_cam=rc, mask=mk)


CASES.append(Case("project_points", ("sgc_project_points",), _scene_build(5, 400, 3), _project_run, tol=0.0))
CASES.append(Case("project_points-selection", ("sgc_project_points",), _scene_build(7, 500, 9, True), _project_run, tol=0.0))


@functools.lru_cache(None)
def _pairs(N, Nq, seed):
    from count_contract import _scene
    o = _oracle()
    ref3d, origin, proj = _scene(N, Nq, seed)
    rc, mk = o.project_points(ref3d, origin, proj, 320., 239., 0.2, 5.0)
    pc = o.compact_pairs(mk)
    n_pairs, n_valid = int(pc["totals"][0]), int(pc["totals"][1])
    assert 0 < n_pairs < pc["pair_q"].numel() and 0 < n_valid < Nq
    return rc, mk, {k: v.clone() for k, v in pc.items()}, n_pairs, n_valid


def _compact_run(form):
    def run(ops, t):
        pc = _tuned(ops, b"compact2", form, 1, lambda: ops.compact_pairs(t["mask"]))
        return dict(pc)
    return run


def _compact_extent(r, i):
    n_pairs, n_valid = int(r["totals"][0]), int(r["totals"][1])
    return dict(pair_cam=slice(0, n_pairs), pair_q=slice(0, n_pairs), valid_index=slice(0, n_valid))


_TAILS = "sgcdet_amd.h, sgc_compact_pairs: pair_cam / pair_q beyond totals[0] and valid_index beyond totals[1] are not written"
CASES.append(Case("compact_pairs", ("sgc_compact_pairs",), lambda: dict(mask=_pairs(5, 400, 3)[1]), _compact_run(1), tol=0.0,
                  extent=_compact_extent, undefined=_TAILS))
CASES.append(Case("compact_pairs-five_kernels", ("sgc_compact_pairs",), lambda: dict(mask=_pairs(5, 400, 3)[1]), _compact_run(0), tol=0.0,
                  extent=_compact_extent, undefined=_TAILS, only="cuda"))

_G = dict(N=6, Nq=700, D=12, C=32, M=8, P=4, H=7, W=10)


def _gather_build():
    N, Nq, D, C, M, P, H, W = (_G[k] for k in ("N", "Nq", "D", "C", "M", "P", "H", "W"))
    rc, mk, pc, n_pairs, n_valid = _pairs(N, Nq, 4)
    g = _gen(11)
    feat = torch.randn(N, H * W, C, generator=g)
    dist = torch.randn(N, H * W, D, generator=g).mul(2).softmax(-1).contiguous()
    raw = torch.randn(pc["pair_q"].numel(), M * P * 4, generator=g)
    raw[:, :M * P * 3] *= 3.0
    return dict(feat=feat, dist=dist, rc=rc, raw=raw, pair_cam=pc["pair_cam"], pair_q=pc["pair_q"], totals=pc["totals"], slot=pc["slot"],
                valid_index=pc["valid_index"], n_valid_dev=pc["totals"][1:2].clone(), q=torch.randn(n_valid, C, generator=g),
                kv=torch.randn(n_pairs, 2 * C, generator=g), pair_feat=torch.randn(n_pairs, C, generator=g), gctx=torch.randn(n_valid, C, generator=g),
                n_pairs=n_pairs, n_valid=n_valid)


def _rows_extent(*names, key="n_pairs"):
    return lambda r, i: {n: slice(0, i[key]) for n in names}


_PAIR_ROWS = "sgcdet_amd.h: rows of the pair-list outputs beyond the device count (totals[0]) are not written"
CASES.append(Case("pairs_geometry_sample-host_count", ("sgc_pairs_geometry_sample",), _gather_build,
                  lambda ops, t: dict(out=ops.pairs_geometry_sample(t["feat"], t["dist"], t["rc"], t["pair_cam"], t["pair_q"], t["n_pairs"], _G["H"], _G["W"])),
                  tol=1e-5))
CASES.append(Case("pairs_geometry_sample-device_count", ("sgc_pairs_geometry_sample",), _gather_build,
                  lambda ops, t: dict(out=ops.pairs_geometry_sample(t["feat"], t["dist"], t["rc"], t["pair_cam"], t["pair_q"], -1, _G["H"], _G["W"],
                                                                    totals=t["totals"])), tol=1e-5, extent=_rows_extent("out"), undefined=_PAIR_ROWS))


def _deform_run(count, with_pairs):
    def run(ops, t):
        H, W, M, P = (_G[k] for k in ("H", "W", "M", "P"))
        value = t["feat"].view(_G["N"], H * W, M, _G["C"] // M)
        dp = ops.depth_pairs(t["dist"], H, W) if with_pairs else None
        out = ops.pairs_deform_gather(value, t["dist"], t["rc"], t["raw"], t["pair_cam"], t["pair_q"], t["n_pairs"] if count == "host" else -1, H, W, M, P,
                                      totals=None if count == "host" else t["totals"], dist_pairs=dp)
        return dict(out=out, dist_pairs=dp)
    return run


CASES.append(Case("pairs_deform_gather-host_count", ("sgc_pairs_deform_gather",), _gather_build, _deform_run("host", False), tol=1e-5))
CASES.append(Case("pairs_deform_gather-device_count_depth_pairs", ("sgc_pairs_deform_gather", "sgc_depth_pairs"), _gather_build,
                  _deform_run("device", True), tol=dict(out=1e-5, dist_pairs=0.0), extent=_rows_extent("out"), undefined=_PAIR_ROWS))
def _deform_cm_case(C, H, W, form):
    """The M = 8, Cm = 16 / 32 specialisations of the gather (what the production levels run; tests/test_gpu_kernels.py at (128, 8, 4,
    (14, 20)) and (256, 8, 4, (15, 20))) -- plain, and in the zero-row form: ``value`` is a view of a buffer that holds ONE all-zero row
    behind its N * S rows (made here, inside one guarded allocation), with and without the pair-interleaved depth taps."""
    N, Nq, D, M, P = 6, 700, 12, 8, 4

    def build():
        rc, mk, pc, n_pairs, n_valid = _pairs(N, Nq, 4)
        g = _gen(11 + C)
        raw = torch.randn(pc["pair_q"].numel(), M * P * 4, generator=g)
        raw[:, :M * P * 3] *= 3.0
        return dict(value=torch.randn(N * H * W, C, generator=g), dist=torch.randn(N, H * W, D, generator=g).mul(2).softmax(-1).contiguous(), rc=rc, raw=raw,
                    pair_cam=pc["pair_cam"], pair_q=pc["pair_q"], n_pairs=n_pairs)

    def run(ops, t):
        value, zero_row = t["value"], form != "plain"
        if zero_row:
            buf = torch.empty((N * H * W + 1, C), dtype=torch.float32, device=value.device)
            buf[:N * H * W].copy_(value)
            buf[N * H * W:].zero_()
            value = buf[:N * H * W]
        dp = ops.depth_pairs(t["dist"], H, W) if form == "zero_row_depth_pairs" else None
        return dict(out=ops.pairs_deform_gather(value.view(N, H * W, M, C // M), t["dist"], t["rc"], t["raw"], t["pair_cam"], t["pair_q"], t["n_pairs"], H, W, M, P,
                                                dist_pairs=dp, zero_row=zero_row))
    return Case(f"pairs_deform_gather-Cm{C // M}-{form}", ("sgc_pairs_deform_gather",), build, run, tol=1e-5)


CASES += [_deform_cm_case(C, H, W, form) for C, H, W in ((128, 14, 20), (256, 15, 20)) for form in ("plain", "zero_row", "zero_row_depth_pairs")]
CASES.append(Case("view_mean", ("sgc_view_mean",), _gather_build,
                  lambda ops, t: dict(mean=ops.view_mean(t["pair_feat"], t["slot"], t["valid_index"], t["n_valid"])), tol=1e-5))
CASES.append(Case("view_mean-device_count", ("sgc_view_mean",), _gather_build,
                  lambda ops, t: dict(mean=ops.view_mean(t["pair_feat"], t["slot"], t["valid_index"], _G["Nq"], count=t["n_valid_dev"])), tol=1e-5,
                  extent=_rows_extent("mean", key="n_valid"), undefined="sgcdet_amd.h, sgc_view_mean: rows beyond *count are not written"))


def _attend_run(ops, t):
    ctx = ops.view_attend(t["q"], t["kv"], t["slot"], t["valid_index"], 8)
    gq, gkv = ops.view_attend_backward(t["q"], t["kv"], t["slot"], t["valid_index"], 8, ctx, t["gctx"])
    return dict(ctx=ctx, grad_q=gq, grad_kv=gkv)


CASES.append(Case("view_attend_and_backward", ("sgc_view_attend", "sgc_view_attend_backward"), _gather_build, _attend_run,
                  tol=dict(ctx=1e-5, grad_q=2e-5, grad_kv=2e-5), bits=dict(ctx=True, grad_q=False, grad_kv=False), accumulated=("grad_q", "grad_kv")))


def _pq_build():
    from test_oracle_identity import _pq_case
    N, Nq, C, heads = 3, 100, 256, 8
    pooled, x, slot, valid_index, mha = _pq_case(N, Nq, C, heads, seed=5 + N, vis=0.6)
    hd = C // heads
    w, b = mha.in_proj_weight.detach().double(), mha.in_proj_bias.detach().double()
    q = pooled.double() @ w[:C].t() + b[:C]
    qp = torch.cat([(1.0 / hd) ** 0.5 * q[:, h * hd:(h + 1) * hd] @ w[C:2 * C][h * hd:(h + 1) * hd] for h in range(heads)], 1).float().contiguous()
    return dict(qp=qp, x=x, slot=slot, valid_index=valid_index)


CASES.append(Case("view_attend_pq", ("sgc_view_attend_pq",), _pq_build,
                  lambda ops, t: dict(s=ops.view_attend_pq(t["qp"], t["x"], t["slot"], t["valid_index"], 8)), tol=1e-5))


def _scatter_run(ops, t):
    """scatter_rows / scatter_add_rows write into the caller's volume: it is made here (guarded) and initialised as the caller does."""
    Nq, C = _G["Nq"], _G["C"]
    idx = t["valid_index"][:t["n_valid"]].contiguous()
    vol = ops.scatter_rows(t["q"], idx, torch.empty((Nq, C), dtype=torch.float32, device=t["q"].device).zero_())
    add = torch.empty((Nq, C), dtype=torch.float32, device=t["q"].device).copy_(t["base"])
    ops.scatter_add_rows(t["q"], idx.to(torch.int64), add)
    return dict(vol=vol, add=add)


def _scatter_build():
    d = _gather_build()
    d["base"] = torch.randn(_G["Nq"], _G["C"], generator=_gen(12))
    return d


def _scatter_ref(i):
    idx = i["valid_index"][:i["n_valid"]].long()
    vol = torch.zeros(_G["Nq"], _G["C"], dtype=torch.float64)
    vol[idx] = i["q"].double()
    add = i["base"].double().clone()
    add[idx] += i["q"].double()
    return dict(vol=vol, add=add)


CASES.append(Case("scatter_rows_and_scatter_add_rows", ("sgc_scatter_rows", "sgc_scatter_add_rows"), _scatter_build, _scatter_run, ref=_scatter_ref,
                  tol=dict(vol=0.0, add=1e-6)))

_T = dict(N=6, Nq=900, D=12, C=128, M=8, P=4, H=14, W=20, bw=20, bh=14)


@functools.lru_cache(None)
def _tiled_inputs():
    from tile_contract import check_bins, raw_to_headmajor, value_to_headmajor
    N, Nq, D, C, M, P, H, W, bw, bh = (_T[k] for k in ("N", "Nq", "D", "C", "M", "P", "H", "W", "bw", "bh"))
    o = _oracle()
    rc, mk, pc, n_pairs, _ = _pairs(N, Nq, 4)
    cap = pc["pair_q"].numel()
    g = _gen(21)
    value = torch.randn(N, H * W, M, C // M, generator=g)
    dist = torch.randn(N, H * W, D, generator=g).mul(2).softmax(-1).contiguous()
    raw = torch.randn(cap, M * P * 4, generator=g)
    raw[:, :M * P * 3] *= 2.0
    before = dict(pc, slot=pc["slot"].clone())
    b = o.bin_pairs(rc, dict(pc, slot=pc["slot"].clone()), H, W, bw, bh)
    old = check_bins(b, before, rc, n_pairs, H, W, bw, bh)
    raw_new = torch.zeros_like(raw)
    raw_new[:n_pairs] = raw[old]
    return dict(rc=rc, pc={k: v for k, v in pc.items() if k in ("pair_cam", "pair_q", "cam_offset", "slot")}, vhm=value_to_headmajor(value), dist=dist,
                rhm=raw_to_headmajor(raw_new, M, P), pair_ref=b["pair_ref"], bin_offset=b["bin_offset"], n_pairs=n_pairs,
                shift=torch.randint(-3, 4, (M, 2), generator=g, dtype=torch.int32))


def _bin_run(ops, t):
    b = ops.bin_pairs(t["rc"], dict(t["pc"]), _T["H"], _T["W"], _T["bw"], _T["bh"])
    return dict(pair_q=b["pair_q"], pair_ref=b["pair_ref"], bin_offset=b["bin_offset"], slot=b["slot"])


CASES.append(Case("bin_pairs", ("sgc_bin_pairs",), lambda: dict(_tiled_inputs()), _bin_run, tol=0.0, accumulated=("slot",),
                  extent=_rows_extent("pair_q", "pair_ref"), undefined="sgcdet_amd.h, sgc_bin_pairs: pair_q_out / pair_ref beyond the pair count are not written"))


def _tiled_run(shift):
    def run(ops, t):
        return dict(out=ops.pairs_deform_gather_tiled(t["vhm"], t["dist"], t["pair_ref"], t["bin_offset"], t["rhm"], _T["H"], _T["W"], _T["P"], _T["bw"],
                                                      _T["bh"], 0, 0, head_shift=t["shift"] if shift else None, max_shift=(3, 3) if shift else (0, 0)))
    return run


for _s in (False, True):
    CASES.append(Case("pairs_deform_gather_tiled" + ("-head_shift" if _s else ""), ("sgc_pairs_deform_gather_tiled",), lambda: dict(_tiled_inputs()),
                      _tiled_run(_s), tol=1e-5, extent=_rows_extent("out"),
                      undefined="sgcdet_amd.h, sgc_pairs_deform_gather_tiled: rows past the pair count (bin_offset's last entry) are not written"))


CASES.append(Case("pairs_deform_gather_tiled-out", ("sgc_pairs_deform_gather_tiled",), lambda: dict(_tiled_inputs()),
                  lambda ops, t: dict(out=ops.pairs_deform_gather_tiled(t["vhm"], t["dist"], t["pair_ref"], t["bin_offset"], t["rhm"], _T["H"], _T["W"], _T["P"],
                                                                        _T["bw"], _T["bh"], 0, 0, out=_out_of(t["rhm"].shape[0], _T["C"], t["rhm"]))),
                  tol=1e-5, extent=_rows_extent("out"),
                  undefined="sgcdet_amd.h, sgc_pairs_deform_gather_tiled: rows past the pair count (bin_offset's last entry) are not written"))


def _tiled_bf16_inputs():
    d = dict(_tiled_inputs())
    d["vhm"], d["dist"] = d["vhm"].to(torch.bfloat16), d["dist"].to(torch.bfloat16)          # the storage mode covers both maps
    return d


# the bf16 STORAGE mode against the oracle fed the same bf16 maps: the same arithmetic, 1e-5 (tests/test_gpu_kernels.py)
CASES.append(Case("pairs_deform_gather_tiled-bf16_storage", ("sgc_pairs_deform_gather_tiled",), _tiled_bf16_inputs, _tiled_run(False), tol=1e-5,
                  extent=_rows_extent("out"),
                  undefined="sgcdet_amd.h, sgc_pairs_deform_gather_tiled: rows past the pair count (bin_offset's last entry) are not written"))


def _geolin_build(C=128):
    from test_gpu_kernels import _geometry_linear_case
    feat, dist, rc, pc, n, w, b = _geometry_linear_case((15, 20), 0, C, _oracle())
    hi, lo = _oracle().split_bf16(w)
    assert 0 < n < pc["pair_q"].numel()
    return dict(feat=feat, dist=dist, rc=rc, pair_cam=pc["pair_cam"], pair_q=pc["pair_q"], totals=pc["totals"], hi=hi, lo=lo, b=b, n_pairs=n)


def _geolin_run(count):
    def run(ops, t):
        return dict(y=ops.pairs_geometry_linear(t["feat"], t["dist"], t["rc"], t["pair_cam"], t["pair_q"], t["n_pairs"] if count == "host" else -1, 15, 20,
                                                t["hi"], t["lo"], t["b"], totals=None if count == "host" else t["totals"]))
    return run


def _geolin_needs(ops):
    if _cuda(ops):
        assert ops.pairs_geometry_linear_supported(128, 128, 5, 300)


CASES.append(Case("pairs_geometry_linear-host_count", ("sgc_pairs_geometry_linear_bf16x3",), _geolin_build, _geolin_run("host"), tol=1e-4, needs=_geolin_needs))
CASES.append(Case("pairs_geometry_linear-device_count", ("sgc_pairs_geometry_linear_bf16x3",), _geolin_build, _geolin_run("device"), tol=1e-4,
                  needs=_geolin_needs, extent=_rows_extent("y"), undefined=_PAIR_ROWS))
# C = 256: the producer / consumer form of the gathering row GEMM (tests/test_gpu_kernels.py::test_geometry_sample_fused_with_its_linear)
CASES.append(Case("pairs_geometry_linear-C256-device_count", ("sgc_pairs_geometry_linear_bf16x3",), lambda: _geolin_build(256), _geolin_run("device"), tol=1e-4,
                  extent=_rows_extent("y"), undefined=_PAIR_ROWS))

_B = dict(N=5, Nq=700, D=12, M=8, P=4, Cm=16, H=14, W=20, bw=20, bh=14)


@functools.lru_cache(None)
def _binned_inputs():
    N, Nq, D, M, P, Cm, H, W, bw, bh = (_B[k] for k in ("N", "Nq", "D", "M", "P", "Cm", "H", "W", "bw", "bh"))
    o = _oracle()
    rc, mk, pc, n, _ = _pairs(N, Nq, 9)
    g = _gen(5 + Cm)
    b = o.bin_pairs(rc, dict(pc, slot=pc["slot"].clone()), H, W, bw, bh)
    cam, q = b["pair_cam"][:n].long(), b["pair_q"][:n].long()
    ref = rc[cam, q]
    return dict(value=torch.randn(N, H * W, M, Cm, generator=g), dist=torch.randn(N, H * W, 1, D, generator=g).mul(2).softmax(-1).contiguous(),
                loc=(ref.view(n, 1, 1, 1, 3) + (torch.rand(n, M, 1, P, 3, generator=g) - 0.5) * 0.30).contiguous(), attn=torch.rand(n, M, 1, P, generator=g),
                go=torch.randn(n, M * Cm, generator=g), bin_offset=b["bin_offset"],
                loc1=(ref.view(n, 1, 1, 1, 3) + (torch.rand(n, 1, 1, 1, 3, generator=g) - 0.5) * 0.30).contiguous())


def _binned_run(ops, t):
    """Both forms in one case: with one sample set shared by the M channel groups every gradient is accumulated with atomics into
    torch.zeros (sgcdet_amd.h), so that form alone allocates nothing through the patched functions."""
    a = (t["bin_offset"], t["go"], _B["H"], _B["W"], _B["bw"], _B["bh"], (0, 0))
    gv, gd, gl, ga = ops.dfa3d_backward_binned(t["value"], t["dist"], t["loc"], t["attn"], *a)
    sv, sd, sl, sa = ops.dfa3d_backward_binned(t["value"], t["dist"], t["loc1"], None, *a)
    return dict(grad_value=gv, grad_dist=gd, grad_loc=gl, grad_attn=ga, shared_grad_value=sv, shared_grad_dist=sd, shared_grad_loc=sl, shared_grad_attn=sa)


CASES.append(Case("dfa3d_backward_binned", ("sgc_dfa3d_backward_binned",), lambda: dict(_binned_inputs()), _binned_run, tol=2e-5, bits=False,
                  accumulated=("grad_value", "grad_dist", "shared_grad_value", "shared_grad_dist", "shared_grad_loc", "shared_grad_attn")))


def _up_build():
    C, grid = 32, (3, 4, 2)
    g = _gen(C)
    V = grid[0] * grid[1] * grid[2]
    return dict(vol=torch.randn(V, C, generator=g), w=torch.randn(C, generator=g) * 0.1, b=torch.randn(1, generator=g),
                go=torch.randn(1, 3, 8, 10, 6, generator=_gen(5)))


def _up_run(ops, t):
    up, occ, _ = ops.upsample2x_occ(t["vol"], (3, 4, 2), t["w"], t["b"])
    return dict(up=up, occ=occ, grad_in=ops.upsample2x_backward(t["go"]))


CASES.append(Case("upsample2x_occ_and_backward", ("sgc_upsample2x_occ", "sgc_upsample2x_backward"), _up_build, _up_run,
                  tol=dict(up=1e-6, occ=2e-6, grad_in=1e-5)))


def _occ_slice_run(ops, t):
    """``occ_out``: the scores land in a slice of the level-concatenated occupancy vector; its neighbours belong to other levels."""
    V8 = 8 * 3 * 4 * 2
    occ_all = torch.empty(V8 + 100, dtype=torch.float32, device=t["vol"].device)
    up, occ, _ = ops.upsample2x_occ(t["vol"], (3, 4, 2), t["w"], t["b"], occ_out=occ_all[36:36 + V8])
    return dict(up=up, occ_all=occ_all)


def _occ_slice_masks(live):
    def f(r, i):
        m = torch.zeros(8 * 24 + 100, dtype=torch.bool)
        m[36:36 + 8 * 24] = True
        return dict(occ_all=m if live else ~m)
    return f


CASES.append(Case("upsample2x_occ-into_a_slice_of_the_level_vector", ("sgc_upsample2x_occ",), _up_build, _occ_slice_run, tol=dict(up=1e-6, occ_all=2e-6),
                  extent=_occ_slice_masks(True), keep=_occ_slice_masks(False), undefined="sgcdet_amd.h, sgc_upsample2x_occ: occ holds 8 X Y Z scores, nothing else is written"))


# ======================================================================================================================================
# row kernels (tests/test_gpu_kernels.py, tests/test_gpu_nonfinite.py: bf16x3 1e-4 of the scale against the oracle)
# ======================================================================================================================================
def _linear_build(rows, cin, cout):
    def build():
        g = _gen(rows + cout)
        hi, lo = _oracle().split_bf16(torch.randn(1, cout, cin, generator=g) * 0.05)
        return dict(x=torch.randn(rows, cin, generator=g), hi=hi, lo=lo, b=torch.randn(cout, generator=g), cnt=torch.tensor([(rows * 2) // 3], dtype=torch.int32))
    return build


def _zrow_run(ops, t):
    y = ops.linear_rows_bf16x3(t["x"], t["hi"], t["lo"], t["b"], zero_tail=True)
    rows, cout = y.shape
    return dict(y=y, zero_row=torch.as_strided(y, (1, cout), (cout, 1), y.storage_offset() + rows * cout))


def _count_out_run(ops, t):
    """A caller's ``out`` with a device count: rows past the count belong to the caller and stay as they were."""
    out = torch.empty((t["x"].shape[0], t["hi"].shape[-2]), dtype=torch.float32, device=t["x"].device)
    return dict(out=ops.linear_rows_bf16x3(t["x"], t["hi"], t["lo"], t["b"], count=t["cnt"], out=out))


def _count_masks(name):
    def rows_mask(r, i, live):
        m = torch.zeros(r[name].shape, dtype=torch.bool)
        m[: int(i["cnt"])] = True
        return {name: m if live else ~m}
    return (lambda r, i: rows_mask(r, i, True)), (lambda r, i: rows_mask(r, i, False))


def _linear_function_build():
    g = _gen(777 + 33)
    return dict(x=torch.randn(777, 64, generator=g), w=torch.randn(33, 64, generator=g) * 0.05)


def _linear_function_run(ops, t):
    from sgcdet_amd.functions import LinearRowsFunction
    return dict(y=LinearRowsFunction.apply(t["x"], t["w"], None))


# 33 output columns: the entry takes Cout % 4 == 0, the Function pads (tests/test_gpu_conv3d.py, 1e-4 of the max-abs against float64)
CASES.append(Case("linear_rows-777x64x33-through_the_function", ("sgc_linear_rows_bf16x3", "sgc_pack_conv_weight"), _linear_function_build,
                  _linear_function_run, ref=lambda i: dict(y=F.linear(i["x"].double(), i["w"].double())), tol=1e-4, unit_floor=False, only="cuda"))
for _rows, _cin, _cout in ((1237, 128, 96), (777, 64, 36)):
    CASES.append(Case(f"linear_rows-{_rows}x{_cin}x{_cout}", ("sgc_linear_rows_bf16x3",), _linear_build(_rows, _cin, _cout),
                      lambda ops, t: dict(y=ops.linear_rows_bf16x3(t["x"], t["hi"], t["lo"], t["b"])), tol=1e-4))
_ext, _keep = _count_masks("out")
CASES.append(Case("linear_rows-device_count_into_a_callers_buffer", ("sgc_linear_rows_bf16x3",), _linear_build(1237, 128, 96), _count_out_run, tol=1e-4,
                  extent=_ext, keep=_keep, undefined="sgcdet_amd.h, sgc_linear_rows_bf16x3: rows past the count are neither read nor written"))
CASES.append(Case("linear_rows-zero_row", ("sgc_linear_rows_zrow_bf16x3",), _linear_build(1237, 128, 96), _zrow_run, tol=1e-4))


def _many_tiles_run(ops, t):
    def go():
        return _tuned(ops, b"rows_depth", 2, 1, lambda: dict(y=ops.linear_rows_bf16x3(t["x"], t["hi"], t["lo"], t["b"])))
    return _tuned(ops, b"rows_cu_pct", 25, 100, go)


CASES.append(Case("linear_rows-a_workgroup_owns_many_tiles", ("sgc_linear_rows_bf16x3",), _linear_build(10001, 128, 256), _many_tiles_run, tol=1e-4))


def _headmajor_build():
    N, S, Cin, M, Cm = 3, 333, 64, 8, 16
    g = _gen(3)
    hi, lo = _oracle().split_bf16(torch.randn(1, M * Cm, Cin, generator=g) * 0.2)
    return dict(x=torch.randn(N * S, Cin, generator=g), hi=hi, lo=lo, b=torch.randn(M * Cm, generator=g))


CASES.append(Case("linear_rows_headmajor-bf16_storage", ("sgc_linear_rows_headmajor_bf16x3",), _headmajor_build,
                  lambda ops, t: dict(y=ops.linear_rows_headmajor_bf16x3(t["x"], t["hi"], t["lo"], t["b"], 3, 333, 8, out_dtype=torch.bfloat16)),
                  tol=2.0 ** -8))            # the RNE of an fp32 result held to 1e-4: the two sides may round to neighbouring bf16 values, one ulp = 2^-8 of the value
CASES.append(Case("linear_rows_headmajor", ("sgc_linear_rows_headmajor_bf16x3",), _headmajor_build,
                  lambda ops, t: dict(y=ops.linear_rows_headmajor_bf16x3(t["x"], t["hi"], t["lo"], t["b"], 3, 333, 8)), tol=1e-4))


def _blockdiag_build():
    rows, K, G = 33, 128, 8
    g = _gen(rows + K)
    hi, lo = _oracle().split_bf16(torch.randn(G, K // 8, K, generator=g) * (1.0 / K ** 0.5))
    return dict(x=torch.randn(rows, G * K, generator=g), hi=hi, lo=lo, b=torch.randn(G * (K // 8), generator=g) * 0.1)


CASES.append(Case("linear_rows_blockdiag-33x128", ("sgc_linear_rows_blockdiag_bf16x3",), _blockdiag_build,
                  lambda ops, t: dict(y=ops.linear_rows_blockdiag(t["x"], t["hi"], t["lo"], t["b"])), tol=1e-5))


def _ln_build():
    rows, C = 100, 96
    g = _gen(rows + C)
    return dict(x=torch.randn(rows, C, generator=g) * 3 + 0.7, w=torch.randn(C, generator=g), b=torch.randn(C, generator=g),
                cnt=torch.tensor([rows // 2], dtype=torch.int32))


def _ln_ref(i):
    return F.layer_norm(i["x"].double(), (96,), i["w"].double(), i["b"].double(), 1e-5)


def _ln_count_run(ops, t):
    return dict(out=ops.layer_norm_rows(t["x"], t["w"], t["b"], 1e-5, count=t["cnt"], out=torch.empty_like(t["x"])))


CASES.append(Case("layer_norm_rows", ("sgc_layer_norm_rows",), _ln_build, lambda ops, t: dict(y=ops.layer_norm_rows(t["x"], t["w"], t["b"], 1e-5)),
                  ref=lambda i: dict(y=_ln_ref(i)), tol=2e-6))
_ext, _keep = _count_masks("out")
CASES.append(Case("layer_norm_rows-device_count_into_a_callers_buffer", ("sgc_layer_norm_rows",), _ln_build, _ln_count_run, ref=lambda i: dict(out=_ln_ref(i)),
                  tol=2e-6, extent=_ext, keep=_keep, undefined="sgcdet_amd.h, sgc_layer_norm_rows: rows past *count are not written"))


def _level_tail_build(seen):
    def build():
        from test_gpu_kernels import _level_tail_case
        ctx, row_of, vis, (wo, w1, w2), (bo, b1, b2), ln1, ln2 = _level_tail_case(31, 128, seen)
        sp = lambda w: _oracle().split_bf16(w.view(1, *w.shape))             # noqa: E731
        return dict(ctx=ctx, row_of=row_of, so=sp(wo), s1=sp(w1), s2=sp(w2), bo=bo, b1=b1, b2=b2, ln1=ln1, ln2=ln2)
    return build


for _seen in (1.0, 0.5):
    CASES.append(Case(f"level_tail-seen_{_seen}", ("sgc_level_tail",), _level_tail_build(_seen),
                      lambda ops, t: dict(y=ops.level_tail(t["ctx"], t["row_of"], t["so"], t["bo"], t["ln1"], t["s1"], t["b1"], t["s2"], t["b2"], t["ln2"])),
                      tol=1e-4))

_BN_ACC = ("rm", "rv")           # the running statistics are updated in place (in-out inputs)


def _bn_case(rows, C, tail):
    import nonfinite_contract as nf

    def run(ops, t):
        return {k: v for k, v in nf.bn_run(ops, t, tail, t["x"].device.type).items() if v is not None}
    entries = ("sgc_bn_rows_act_forward", "sgc_bn_rows_act_backward") if tail else ("sgc_bn_rows_forward", "sgc_bn_rows_backward")
    return Case(f"bn_rows-{rows}x{C}-{'residual_relu' if tail else 'plain'}", entries, lambda: nf.bn_inputs(rows, C, "nan", None), run, tol=2e-4,
                accumulated=_BN_ACC)


CASES += [_bn_case(r, c, tail) for r, c in ((6, 4), (77, 1040)) for tail in (False, True)]


CASES.append(Case("level_tail-out", ("sgc_level_tail",), _level_tail_build(0.5),
                  lambda ops, t: dict(y=ops.level_tail(t["ctx"], t["row_of"], t["so"], t["bo"], t["ln1"], t["s1"], t["b1"], t["s2"], t["b2"], t["ln2"],
                                                       out=_out_of(31, 128, t["ctx"]))), tol=1e-4))


def _topk_run(form):
    def run(ops, t):
        s, n, k = t["score"], 1000, 100
        if form == "one_launch_entry":
            idx = torch.empty(k, dtype=torch.int64, device=s.device)
            valid = torch.empty(n, dtype=torch.int64, device=s.device)
            mask = torch.empty(n, dtype=torch.float32, device=s.device)
            ops._call("sgc_topk_select", s, n, k, idx, valid, mask)
        elif form == "many_workgroups":
            idx, valid, mask = _tuned(ops, b"topk_multi_min", 1, 32769, lambda: ops.topk_select(s, k, want_valid=True, want_mask=True))
        else:
            idx, valid, mask = ops.topk_select(s, k, want_valid=True, want_mask=True)
        return dict(idx=idx, valid=valid, mask=mask)
    return run


def _topk_build():
    g = _gen(1100)
    s = torch.sigmoid(torch.randn(1000, generator=g))
    s[torch.randperm(1000, generator=g)[:400]] = float(s.sort(descending=True).values[100])         # heavy exact ties at the cut
    return dict(score=s)


def _topk_ref(i):
    s = i["score"].double()
    order = torch.argsort(-s, stable=True)[:100]                   # ties at the cut: the lowest indices win
    idx = order.sort().values
    valid = torch.zeros(1000, dtype=torch.int64)
    valid[idx] = 1
    return dict(idx=idx, valid=valid, mask=valid.float())


for _form, _entry in (("one_launch_entry", "sgc_topk_select"), ("one_workgroup", "sgc_topk_select_ws"), ("many_workgroups", "sgc_topk_select_ws")):
    CASES.append(Case(f"topk_select-{_form}", (_entry,), _topk_build, _topk_run(_form), ref=_topk_ref, tol=0.0,
                      only="cuda" if _form == "many_workgroups" else None))


def _layout_build():
    N, C, Hs, Ws, H, W = 2, 40, 17, 23, 15, 20
    g = _gen(N * C + H)
    return dict(src=torch.randn(N, C, Hs, Ws, generator=g), rows=torch.randn(N, H * W, C, generator=g))


def _layout_run(ops, t):
    return dict(crop=ops.nchw_to_nhwc_crop(t["src"], 15, 20), pad=ops.nhwc_to_nchw_pad(t["rows"], 15, 20, 17, 23))


def _layout_ref(i):
    N, C = 2, 40
    return dict(crop=i["src"][:, :, :15, :20].permute(0, 2, 3, 1).reshape(N, 300, C),
                pad=F.pad(i["rows"].view(N, 15, 20, C).permute(0, 3, 1, 2), (0, 3, 0, 2)))


CASES.append(Case("nchw_to_nhwc_crop_and_nhwc_to_nchw_pad", ("sgc_nchw_to_nhwc_crop", "sgc_nhwc_to_nchw_pad"), _layout_build, _layout_run, ref=_layout_ref,
                  tol=0.0))


def _crop64_case(n, c, hs, ws, h, w):
    """The 64 x 64 / 16-byte form of the crop (C % 64 == 0, W and the source pitch % 4 == 0; tests/test_gpu_kernels.py): partial pixel tiles."""
    return Case(f"nchw_to_nhwc_crop-{n}x{c}x{hs}x{ws}-to-{h}x{w}", ("sgc_nchw_to_nhwc_crop",), lambda: dict(src=torch.randn(n, c, hs, ws, generator=_gen(c + hs + ws))),
                lambda ops, t: dict(crop=ops.nchw_to_nhwc_crop(t["src"], h, w)),
                ref=lambda i: dict(crop=i["src"][:, :, :h, :w].permute(0, 2, 3, 1).reshape(n, h * w, c)), tol=0.0)


CASES += [_crop64_case(2, 64, 9, 12, 7, 8), _crop64_case(2, 64, 5, 8, 5, 4)]


def _crop_views_run(ops, t):
    """The every-2nd- and every-4th-pixel views of the depth pyramid (tests/odd_shape_contract.py), read where they lie: the source
    stays inside its NaN parent, a pixel read past the view's last row or column would show."""
    out, seen, orig = {}, [], ops._call
    ops._call = lambda name, *a, **k: (seen.append(a), orig(name, *a, **k))[1]
    try:
        for step, (h, w) in ((2, (7, 10)), (4, (4, 6))):
            v = t["src"][..., ::step, ::step]
            out[f"step{step}"] = ops.nchw_to_nhwc_crop(v, h, w)
            assert seen[-1][0].data_ptr() == v.data_ptr() and seen[-1][8] == step, "the view went through .contiguous()"
    finally:
        del ops.__dict__["_call"]
    return out


CASES.append(Case("nchw_to_nhwc_crop-step_2_and_4_views", ("sgc_nchw_to_nhwc_crop",), lambda: dict(src=torch.randn(2, 5, 15, 21, generator=_gen(15 + 21))),
                  _crop_views_run, tol=0.0,
                  ref=lambda i: {f"step{s}": i["src"][..., ::s, ::s][..., :h, :w].permute(0, 2, 3, 1).reshape(2, h * w, 5) for s, h, w in ((2, 7, 10), (4, 4, 6))}))


# 3 x 3 x 3 stride 2 on an odd grid (tests/odd_shape_contract.py; float64 torch, 1e-4 of the scale): output (4, 3, 2), the last tap of every
# axis outside the volume.  Cout 28: at 7 the library splits this layer's reduction and a split layer refuses Cout % 4 != 0.
def _odd_stride2_build():
    import odd_shape_contract as oc
    g = _gen(7 + 5 + 3)
    hi, lo = _oracle().split_bf16(oc.forward_weights(32, (3, 2, False))[1][:, :28].contiguous())
    return dict(x=oc.forward_input(32, (7, 5, 3)), hi=hi, lo=lo, sc=torch.rand(28, generator=g) + 0.5, sh=torch.randn(28, generator=g),
                res=torch.randn(24, 28, generator=g))


def _odd_stride2_ref(i):
    import odd_shape_contract as oc
    return dict(y=oc.apply_epilogue(oc.forward_raw(32, (3, 2, False), (7, 5, 3))[:, :28], i["sc"], i["sh"], i["res"], 1))


CASES.append(Case("conv3d_bf16x3-odd_grid_stride_2", ("sgc_conv3d_cl_bf16x3",), _odd_stride2_build,
                  lambda ops, t: dict(y=ops.conv3d_cl_bf16x3(t["x"], t["hi"], t["lo"], (7, 5, 3), 3, 2, False, t["sc"], t["sh"], t["res"], 1)[0]),
                  ref=_odd_stride2_ref, tol=1e-4))


# ======================================================================================================================================
# heads and post-processing (tests/test_gpu_kernels.py; kept indices, targets and masks are exact against the oracle)
# ======================================================================================================================================
def _nms_build(n):
    def build():
        g = _gen(21 + n)
        c = (torch.rand(n, 3, generator=g) - 0.5) * torch.tensor([6.4, 6.4, 2.5])
        c = c[torch.randint(0, max(2, n // 20), (n,), generator=g)] + torch.randn(n, 3, generator=g) * 0.05
        s = 0.4 + torch.rand(n, 3, generator=g)
        return dict(boxes=torch.cat([c - s / 2, c + s / 2], 1), scores=torch.rand(n, generator=g), labels=torch.randint(0, 3, (n,), generator=g))
    return build


for _n in (65, 130):
    CASES.append(Case(f"aligned_nms3d-{_n}", ("sgc_aligned_nms3d",), _nms_build(_n),
                      lambda ops, t: dict(keep=ops.aligned_nms3d(t["boxes"], t["scores"], t["labels"], 0.25)), tol=0.0,
                      undefined="sgcdet_amd.h, sgc_aligned_nms3d: keep beyond n_keep is not written (the wrapper returns keep[:n_keep])"))


def _rotated_build():
    from nms_rotated_contract import arkit_like, bev_of
    boxes, scores = arkit_like(65, 3, 11)
    bev = bev_of(boxes)
    xywhr = torch.stack(((bev[:, 0] + bev[:, 2]) / 2, (bev[:, 1] + bev[:, 3]) / 2, bev[:, 2] - bev[:, 0], bev[:, 3] - bev[:, 1], bev[:, 4]), 1).contiguous()
    return dict(bev=bev, scores=scores, xywhr=xywhr)


def _rotated_run(ops, t):
    keep, n_keep = ops.nms_rotated_bev(t["bev"], t["scores"], 0.0, 0.15)
    return dict(keep=keep, n_keep=n_keep)


def _rotated_extent(r, i):
    m = torch.zeros(r["keep"].shape, dtype=torch.bool)
    for c in range(m.shape[0]):
        assert 0 < int(r["n_keep"][c]) < m.shape[1]
        m[c, : int(r["n_keep"][c])] = True
    return dict(keep=m)


CASES.append(Case("nms_rotated_bev-65x3", ("sgc_nms_rotated_bev",), _rotated_build, _rotated_run, tol=0.0, extent=_rotated_extent,
                  accumulated=("keep", "n_keep"), undefined="sgcdet_amd.h, sgc_nms_rotated_bev: keep[c] beyond n_keep[c] is not written"))
CASES.append(Case("box_iou_rotated-65", ("sgc_box_iou_rotated",), _rotated_build, lambda ops, t: dict(iou=ops.box_iou_rotated(t["xywhr"], t["xywhr"])),
                  tol=1e-6, unit_floor="abs"))


def _targets_build():
    from head_loss_contract import golden_points
    from targets_contract import random_boxes
    pts, scales, _ = golden_points()
    boxes, gl = random_boxes(7, 2, False)
    return dict(pts=pts, scales=scales, boxes=boxes, gl=gl)


def _targets_run(ops, t):
    ct, bt, lb, occ = ops.assign_targets(t["pts"], t["scales"], t["boxes"], t["gl"], False, 3, 27, 18)
    return dict(centerness=ct, bbox=bt, labels=lb, occ=occ)


CASES.append(Case("assign_targets-7_boxes", ("sgc_assign_targets",), _targets_build, _targets_run, tol=0.0,
                  accumulated=("occ",),              # the wrapper returns occ.bool(): a converted copy of the uint8 output
                  nan_values=("centerness", "bbox")))      # background points carry box 0's (possibly NaN) value, bit for bit as the oracle


def _sweep_build():
    import os
    import numpy as np
    from test_oracle_golden import _plane_sweep_case
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plane_sweep.npz"))
    f_mvs, rows, nbr, rt, depth, (H, W) = _plane_sweep_case(d, 0)
    return dict(rows=rows.contiguous(), nbr=nbr.contiguous(), rt=rt.contiguous(), depth=depth.contiguous(), H=H, W=W)


CASES.append(Case("plane_sweep_corr-golden_0", ("sgc_plane_sweep_corr",), _sweep_build,
                  lambda ops, t: dict(corr=ops.plane_sweep_corr(t["rows"], t["nbr"], t["rt"], t["depth"], t["H"], t["W"])), tol=2e-5))


# ======================================================================================================================================
# image-side and training-only entry points (no oracle twin: float64 torch formulations of the existing tests; GPU only)
# ======================================================================================================================================
def _rows_to_nchw(rows, N, H, W):
    return rows.view(N, H, W, -1).permute(0, 3, 1, 2).contiguous()


def _ex_build(k, stride, transposed, nhw, Cout, cout_live):
    """The case of tests/test_gpu_depth_net_hip.py::test_conv2d_ex_forms_against_float64: 48 of 64 input, cout_live of Cout output channels."""
    def build():
        N, H, W = nhw
        g = _gen(100 * k + 10 * stride + int(transposed) + H + Cout)
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
        hi, lo = _oracle().split_bf16(w)
        return dict(x=x, w=w, hi=hi, lo=lo, scale=scale, shift=shift, res=res, orows=N * OH * OW)
    return build


def _ex_case(k, stride, transposed, Cout, cout_live, wide):
    nhw, col0 = (2, 6, 10), 32

    def run(ops, t):
        kw = dict(stride=stride, transposed=transposed, scale=t["scale"], shift=t["shift"], residual=t["res"], relu=True, relu_after_add=True)
        if not wide:
            return dict(y=ops.conv2d_nhwc_ex_bf16x3(t["x"], t["hi"], t["lo"], nhw, k, **kw))
        buf = torch.empty((t["orows"], Cout + 64), dtype=torch.float32, device=t["x"].device)       # the launch owns columns [32, 32 + Cout)
        return dict(y=ops.conv2d_nhwc_ex_bf16x3(t["x"], t["hi"], t["lo"], nhw, k, out=buf, col0=col0, **kw))

    def ref(i):
        from test_gpu_depth_net_hip import _ref_conv
        y = _ref_conv(i["x"], i["w"], nhw, k, stride, transposed, i["scale"], i["shift"], i["res"], 1, 1, 0)
        return dict(y=F.pad(y, (col0, 32)) if wide else y)

    def cols(r, i, live):
        m = torch.zeros(r["y"].shape, dtype=torch.bool)
        m[:, col0:col0 + Cout] = True
        return dict(y=m if live else ~m)

    def needs(ops):
        assert ops.conv2d_nhwc_ex_supported(nhw, 64, Cout, k, stride, transposed, ldy=Cout + 64 if wide else None, col0=col0 if wide else 0, ldr=Cout)
    name = f"conv2d_ex-k{k}s{stride}{'t' if transposed else ''}-Cout{Cout}" + ("-column_range_of_a_wider_buffer" if wide else "")
    return Case(name, ("sgc_conv2d_nhwc_ex_bf16x3",), _ex_build(k, stride, transposed, nhw, Cout, cout_live), run, ref=ref, tol=1e-4, unit_floor=False,
                needs=needs, only="cuda", extent=(lambda r, i: cols(r, i, True)) if wide else None, keep=(lambda r, i: cols(r, i, False)) if wide else None,
                undefined="sgcdet_amd_image.h, sgc_conv2d_nhwc_ex_bf16x3: columns outside [col0, col0 + Cout) are not touched" if wide else None)


for _k, _s, _t in [(1, 1, False), (1, 2, False), (3, 1, False), (3, 2, False), (3, 2, True)]:
    for _co, _live in ((160, 140), (256, 232), (32, 24)):
        CASES.append(_ex_case(_k, _s, _t, _co, _live, False))
    CASES.append(_ex_case(_k, _s, _t, 32, 24, True))


def _softmax_case(Cout):
    nhw, Cin = (2, 6, 10), 160

    def build():
        g = _gen(11)
        x = torch.randn(120, Cin, generator=g)
        shift = F.pad(torch.randn(12, generator=g), (0, Cout - 12))
        w = torch.randn(9, Cout, Cin, generator=_gen(11 + Cout)) * (3.0 / (3 * Cin ** 0.5))
        w[:, 12:] = 0
        hi, lo = _oracle().split_bf16(w)
        return dict(x=x, w=w, hi=hi, lo=lo, shift=shift)

    def ref(i):
        from test_gpu_depth_net_hip import _ref_conv
        return dict(y=_ref_conv(i["x"], i["w"], nhw, 3, 1, False, None, i["shift"], None, 0, 0, 12))
    return Case(f"conv2d_ex-softmax_columns-Cout{Cout}", ("sgc_conv2d_nhwc_ex_bf16x3",), build,
                lambda ops, t: dict(y=ops.conv2d_nhwc_ex_bf16x3(t["x"], t["hi"], t["lo"], nhw, 3, shift=t["shift"], softmax_cols=12)), ref=ref, tol=1e-4,
                unit_floor=False, only="cuda")


CASES += [_softmax_case(12), _softmax_case(32)]


def _strided_case_(k, nhw):
    Cout, cout_live = 160, 140
    N, H, W = nhw

    def build():
        from test_gpu_resnet import _strided_case
        x, w, scale, shift, res = _strided_case(k, nhw, Cout, cout_live, 100 * k + H + Cout)
        hi, lo = _oracle().split_bf16(w)
        return dict(x=x, w=w, hi=hi, lo=lo, scale=scale, shift=shift, res=res)

    def ref(i):
        from test_gpu_resnet import _ref_conv
        return dict(y=_ref_conv(i["x"], i["w"], nhw, k, 2, i["scale"], i["shift"], i["res"], 1, 1)[0])
    return Case(f"conv2d_strided-k{k}-{N}x{H}x{W}", ("sgc_conv2d_nhwc_strided_bf16x3",), build,
                lambda ops, t: dict(y=ops.conv2d_nhwc_strided_bf16x3(t["x"], t["hi"], t["lo"], nhw, k, stride=2, scale=t["scale"], shift=t["shift"],
                                                                     residual=t["res"], relu=True, relu_after_add=True)),
                ref=ref, tol=1e-4, unit_floor=False, only="cuda")


CASES += [_strided_case_(k, nhw) for k in (1, 3) for nhw in ((1, 5, 7), (1, 1, 3))]


def _strided_range_case(k):
    """The strided entry into columns [32, 32 + 160) of a buffer of row pitch 224: the neighbours stay as they were."""
    nhw, Cout, col0, ldy = (1, 5, 7), 160, 32, 224
    base = _strided_case_(k, nhw)

    def run(ops, t):
        buf = torch.empty((12, ldy), dtype=torch.float32, device=t["x"].device)
        return dict(y=ops.conv2d_nhwc_strided_bf16x3(t["x"], t["hi"], t["lo"], nhw, k, stride=2, scale=t["scale"], shift=t["shift"], residual=t["res"], relu=True,
                                                     relu_after_add=True, out=buf, col0=col0))

    def cols(r, i, live):
        m = torch.zeros(r["y"].shape, dtype=torch.bool)
        m[:, col0:col0 + Cout] = True
        return dict(y=m if live else ~m)

    def needs(ops):
        assert ops.conv2d_nhwc_strided_supported(nhw, 64, Cout, k, 2, ldy=ldy, col0=col0, ldr=Cout + 32)
    return Case(f"conv2d_strided-k{k}-1x5x7-column_range_of_a_wider_buffer", ("sgc_conv2d_nhwc_strided_bf16x3",), base.build, run,
                ref=lambda i: dict(y=F.pad(base.ref(i)["y"], (col0, ldy - col0 - Cout))), tol=1e-4, unit_floor=False, only="cuda", needs=needs,
                extent=lambda r, i: cols(r, i, True), keep=lambda r, i: cols(r, i, False),
                undefined="sgcdet_amd_image.h, sgc_conv2d_nhwc_strided_bf16x3: columns outside [col0, col0 + Cout) are not touched")


CASES += [_strided_range_case(1), _strided_range_case(3)]


def _stem7_build():
    N, H, W = 2, 12, 20
    g = _gen(H)
    w = torch.randn(64, 3, 7, 7, generator=g) / 147 ** 0.5
    hi, lo = _oracle().split_bf16(F.pad(w.reshape(64, 147), (0, 13)).contiguous())
    return dict(img=torch.randn(N, 3, H, W, generator=_gen(H + 1)), w=w, hi=hi, lo=lo, scale=0.5 + torch.rand(64, generator=g), shift=0.3 * torch.randn(64, generator=g))


def _stem7_ref(i):
    y = F.conv2d(i["img"].double(), i["w"].double(), stride=2, padding=3) * i["scale"].double().view(1, -1, 1, 1) + i["shift"].double().view(1, -1, 1, 1)
    return dict(y=y.clamp_min(0).permute(0, 2, 3, 1).reshape(-1, 64))


CASES.append(Case("conv2d_stem7-2x12x20", ("sgc_conv2d_stem7_bf16x3",), _stem7_build,
                  lambda ops, t: dict(y=ops.conv2d_stem7_bf16x3(t["img"], t["hi"], t["lo"], scale=t["scale"], shift=t["shift"], relu=True)), ref=_stem7_ref,
                  tol=1e-4, unit_floor=False, only="cuda"))


def _maxpool_case(nhwc):
    N, H, W, C = nhwc
    return Case(f"maxpool2d-{N}x{H}x{W}x{C}", ("sgc_maxpool2d_nhwc",), lambda: dict(x=torch.randn(N * H * W, C, generator=_gen(H * 100 + W))),
                lambda ops, t: dict(y=ops.maxpool2d_nhwc(t["x"], (N, H, W))[0]),
                ref=lambda i: dict(y=F.max_pool2d(_rows_to_nchw(i["x"], N, H, W), 3, 2, 1).permute(0, 2, 3, 1).reshape(-1, C)), tol=0.0, only="cuda")


CASES += [_maxpool_case((1, 1, 1, 4)), _maxpool_case((2, 5, 5, 36))]
CASES.append(Case("nchw_to_nhwc_padc", ("sgc_nchw_to_nhwc_padc",), lambda: dict(img=torch.randn(2, 3, 15, 20, generator=_gen(95))),
                  lambda ops, t: dict(rows=ops.nchw_to_nhwc_padc(t["img"], 8)),
                  ref=lambda i: dict(rows=F.pad(i["img"].permute(0, 2, 3, 1).reshape(-1, 3), (0, 5))), tol=0.0, only="cuda"))


def _wgrad2d_case(k, s, workspace):
    nhw, Cin, Cout = (3, 5, 3), 32, 32
    N, H, W = nhw
    OH, OW = (H + s - 1) // s, (W + s - 1) // s

    def ref(i):
        from test_gpu_resnet_train import _wgrad_ref
        return dict(dw=_wgrad_ref(i["x"], i["dy"], nhw, k, s))
    return Case(f"conv2d_wgrad-k{k}s{s}" + ("" if workspace else "-no_workspace"), ("sgc_conv2d_wgrad_bf16x3",),
                lambda: dict(x=torch.randn(N * H * W, Cin, generator=_gen(1000 * k + 100 * s + H + Cin)),
                             dy=torch.randn(N * OH * OW, Cout, generator=_gen(1000 * k + 100 * s + H + Cin + 1))),
                lambda ops, t: dict(dw=ops.conv2d_wgrad_bf16x3(t["x"], t["dy"], nhw, k, s, workspace=workspace)), ref=ref, tol=1e-4, unit_floor=False,
                only="cuda")


CASES += [_wgrad2d_case(k, s, True) for k in (1, 3) for s in (1, 2)] + [_wgrad2d_case(3, 1, False)]


def _split_wgrad2d_needs(ops):
    assert ops.conv2d_wgrad_workspace_floats((4, 32, 32), 32, 32, 3, 1) > 0, "the reduction is not split"


CASES.append(Case("conv2d_wgrad-k3s1-split_reduction", ("sgc_conv2d_wgrad_bf16x3",),
                  lambda: dict(x=torch.randn(4096, 32, generator=_gen(3132)), dy=torch.randn(4096, 32, generator=_gen(3133))),
                  lambda ops, t: dict(dw=ops.conv2d_wgrad_bf16x3(t["x"], t["dy"], (4, 32, 32), 3, 1)),
                  ref=lambda i: dict(dw=__import__("test_gpu_resnet_train")._wgrad_ref(i["x"], i["dy"], (4, 32, 32), 3, 1)), tol=1e-4, unit_floor=False,
                  needs=_split_wgrad2d_needs, only="cuda"))


def _stem7_wgrad_case(H, W):
    N = 3

    def ref(i):
        w = torch.zeros(64, 3, 7, 7, dtype=torch.float64, requires_grad=True)
        y = F.conv2d(i["img"].double(), w, stride=2, padding=3)
        return dict(dw=torch.autograd.grad(y, w, _rows_to_nchw(i["dy"].double(), N, H // 2, W // 2))[0])
    return Case(f"conv2d_stem7_wgrad-3x{H}x{W}", ("sgc_conv2d_stem7_wgrad_bf16x3",),
                lambda: dict(img=torch.randn(N, 3, H, W, generator=_gen(1000 * N + 10 * H + W)),
                             dy=torch.randn(N * (H // 2) * (W // 2), 64, generator=_gen(1000 * N + 10 * H + W + 1))),
                lambda ops, t: dict(dw=ops.conv2d_stem7_wgrad_bf16x3(t["img"], t["dy"])), ref=ref, tol=1e-4, unit_floor=False, only="cuda")


CASES += [_stem7_wgrad_case(2, 2), _stem7_wgrad_case(8, 12)]


def _frozen_case(rows, C):
    def build():
        g = _gen(rows + C)
        return dict(dy=torch.randn(rows, C, generator=g), y=torch.randn(rows, C, generator=g), scale=0.5 + torch.rand(C, generator=g))

    def run(ops, t):
        g, gres = ops.frozen_norm_act_backward(t["dy"], t["y"], t["scale"], relu=True, want_gres=True)
        g2, _ = ops.frozen_norm_act_backward(t["dy"], None, None, relu=False)
        return dict(g=g, gres=gres, g_plain=g2)

    def ref(i):
        gm = torch.where(i["y"] > 0, i["dy"], torch.zeros_like(i["dy"]))
        return dict(g=gm * i["scale"], gres=gm, g_plain=i["dy"])
    return Case(f"frozen_norm_act_backward-{rows}x{C}", ("sgc_frozen_norm_act_backward",), build, run, ref=ref, tol=0.0, only="cuda")


CASES += [_frozen_case(37, 36), _frozen_case(1, 4)]


def _topdown_case(fine_hw, coarse_hw):
    N, (Hd, Wd), (Hs, Ws), C = 2, fine_hw, coarse_hw, 32

    def build():
        g = _gen(Hd * 100 + Wd + C)
        return dict(fine=torch.randn(N * Hd * Wd, C, generator=g), coarse=torch.randn(N * Hs * Ws, C, generator=g), gout=torch.randn(N * Hd * Wd, C, generator=g))

    def run(ops, t):
        return dict(out=ops.upsample_nearest_add_nhwc(t["fine"], t["coarse"], (N, Hd, Wd), (N, Hs, Ws)),
                    gcoarse=ops.upsample_nearest_add_backward_nhwc(t["gout"], (N, Hd, Wd), (N, Hs, Ws)))

    def ref(i):
        up = F.interpolate(_rows_to_nchw(i["coarse"], N, Hs, Ws), size=(Hd, Wd), mode="nearest")
        z = torch.zeros(N, C, Hs, Ws, dtype=torch.float64, requires_grad=True)
        gc, = torch.autograd.grad(F.interpolate(z, size=(Hd, Wd), mode="nearest"), z, _rows_to_nchw(i["gout"].double(), N, Hd, Wd))
        return dict(out=i["fine"] + up.permute(0, 2, 3, 1).reshape(-1, C), gcoarse=gc.permute(0, 2, 3, 1).reshape(-1, C))
    return Case(f"upsample_nearest_add-{Hd}x{Wd}-from-{Hs}x{Ws}", ("sgc_upsample_nearest_add_nhwc", "sgc_upsample_nearest_add_backward_nhwc"), build, run,
                ref=ref, tol=dict(out=0.0, gcoarse=1e-6), unit_floor=False, only="cuda")


CASES += [_topdown_case((1, 1), (1, 1)), _topdown_case((3, 4), (2, 2))]


def _topdown_in_place_run(ops, t):
    """``out=fine``: the fine rows are updated in place (an in-out input); the backward's allocation keeps the case from being vacuous."""
    return dict(out=ops.upsample_nearest_add_nhwc(t["fine"], t["coarse"], (2, 3, 4), (2, 2, 2), out=t["fine"]),
                gcoarse=ops.upsample_nearest_add_backward_nhwc(t["gout"], (2, 3, 4), (2, 2, 2)))


_td = _topdown_case((3, 4), (2, 2))
CASES.append(Case("upsample_nearest_add-3x4-from-2x2-in_place", _td.entries, _td.build, _topdown_in_place_run, ref=_td.ref, tol=_td.tol, unit_floor=False,
                  only="cuda", accumulated=("out",)))


def _colsum_case(rows):
    def check(got, i):                    # the chain bound of tests/test_gpu_fpn_train.py: 160 * 2^-24 of the column's sum of magnitudes
        x = i["x"].double()
        ratio = ((got["sum"].double() - x.sum(0)).abs() / (2.0 ** -24 * x.abs().sum(0))).max().item()
        assert ratio <= 160, f"rows_colsum {rows}: worst column {ratio:.1f} x 2^-24 x sum|x|"
    return Case(f"rows_colsum-{rows}x36", ("sgc_rows_colsum",), lambda: dict(x=torch.randn(rows, 36, generator=_gen(rows + 36))),
                lambda ops, t: dict(sum=ops.rows_colsum(t["x"])), ref=lambda i: {}, check=check, only="cuda")


CASES += [_colsum_case(1), _colsum_case(63), _colsum_case(257)]


def _sweep_bwd_build():
    from plane_sweep_grad_contract import to_rows
    from test_gpu_plane_sweep_grad import _random_case
    C, K, D = 32, 2, 12
    f_mvs, nbr, rel, depth, grad_corr = _random_case(7, C, 9, 13, K, D, seed=C + 7 * K + D)
    return dict(f_mvs=f_mvs, rows=to_rows(f_mvs).contiguous(), nbr64=nbr, nbr=nbr.to(torch.int32).contiguous(), rel=rel, rt=rel.reshape(7, K, 12).contiguous(),
                depth=depth.contiguous(), grad_corr=grad_corr.contiguous())


def _sweep_bwd_ref(i):
    from plane_sweep_grad_contract import reference_grad_f64, to_rows
    return dict(grad_feat=to_rows(reference_grad_f64(i["f_mvs"], i["nbr64"], i["rel"], i["depth"], i["grad_corr"])))


CASES.append(Case("plane_sweep_corr_backward-C32_K2_D12", ("sgc_plane_sweep_corr_backward",), _sweep_bwd_build,
                  lambda ops, t: dict(grad_feat=ops.plane_sweep_corr_backward(t["rows"], t["nbr"], t["rt"], t["depth"], t["grad_corr"], 9, 13)),
                  ref=_sweep_bwd_ref, tol=1e-5, unit_floor=False, only="cuda"))

_OPT_SHAPES = [(64, 33), (257,), (5, 4, 3)]


def _optim_build():
    g = _gen(7)
    d = {}
    for n, s in enumerate(_OPT_SHAPES):
        d[f"p{n}"], d[f"g{n}"] = (torch.rand(s, generator=g) - 0.5) * 0.5, torch.randn(s, generator=g) * 30
    return d


def _optim_run(ops, t):
    """One FusedAdamW step with clipping (sgc_grad_sqnorm_batch with its workspace + sgc_adamw_step_batch).  The parameters and
    moments are updated in place; ``grad`` is NOT written (sgcdet_amd_train.h): it must come back bit for bit."""
    from sgcdet_amd.optim import FusedAdamW
    ps = [torch.nn.Parameter(t[f"p{n}"]) for n in range(len(_OPT_SHAPES))]
    for n, p in enumerate(ps):
        p.grad = t[f"g{n}"]
    opt = FusedAdamW(ps, lr=2e-4, weight_decay=1e-4, max_grad_norm=35.0)
    opt.step()
    out = dict(norm=opt._norm)
    for n, p in enumerate(ps):
        out[f"p{n}"], out[f"g{n}"], out[f"m{n}"], out[f"v{n}"] = p.detach(), p.grad, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]
    return out


def _optim_ref(i):
    ps = [torch.nn.Parameter(i[f"p{n}"].double()) for n in range(len(_OPT_SHAPES))]
    for n, p in enumerate(ps):
        p.grad = i[f"g{n}"].double()
    opt = torch.optim.AdamW(ps, lr=2e-4, weight_decay=1e-4, foreach=False)
    norm = torch.nn.utils.clip_grad_norm_(ps, 35.0, foreach=False)
    assert float(norm) > 35.0                             # the clip is active
    opt.step()
    out = {}
    for n, p in enumerate(ps):
        out[f"p{n}"], out[f"m{n}"], out[f"v{n}"] = p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]
    return out


def _optim_check(got, i):
    for n in range(len(_OPT_SHAPES)):
        assert torch.equal(got[f"g{n}"], i[f"g{n}"]), f"adamw_step_batch wrote grad {n}"


CASES.append(Case("fused_adamw_step", ("sgc_grad_sqnorm_batch", "sgc_adamw_step_batch"), _optim_build, _optim_run, ref=_optim_ref, tol=1e-6, check=_optim_check,
                  accumulated=tuple(f"{k}{n}" for k in "pgmv" for n in range(len(_OPT_SHAPES))), only="cuda"))

_UPSTREAM = (0.7, 1.3, 2.1)


@functools.lru_cache(None)
def _head_loss_inputs():
    from head_loss_contract import golden_boxes, golden_points, head_tensors, torch_path, torch_path_grads
    pts, scales, (n_scales, limit, topk) = golden_points()
    boxes, gl = golden_boxes(False, 1)
    ct, bt, lb, _ = _oracle().assign_targets(pts, scales, boxes, gl, False, n_scales, limit, topk)
    ctr, reg, cls, val = head_tensors(False, 110)
    ref = {}
    for dtype in (torch.float64, torch.float32):
        losses, leaves = torch_path(False, ctr, reg, cls, val, pts, ct, bt, lb, dtype)
        ref[dtype] = ([l.detach() for l in losses], torch_path_grads(losses, leaves, _UPSTREAM))
    return dict(pts=pts, ct=ct, bt=bt, lb=lb, ctr=ctr, reg=reg, cls=cls, val=[v.reshape(-1) for v in val], ones=torch.ones(1)), ref


def _head_loss_run(ops, t):
    losses, n_pos, state = ops.head_loss(t["ctr"], t["reg"], t["cls"], t["val"], t["pts"], t["ct"], t["bt"], t["lb"], False)
    up = [torch.tensor(u, device=losses.device) for u in _UPSTREAM]
    ctr, reg, cls = ops.head_loss_grads(state, *up)
    losses2, n_pos2 = ops.head_loss_finalize(state, n_pos)
    out = dict(losses=losses, n_pos=n_pos, stash=state["grads"], losses_again=losses2, n_pos_again=n_pos2)
    for l, (a, b, c) in enumerate(zip(ctr, reg, cls)):
        out[f"grad_centerness{l}"], out[f"grad_bbox{l}"], out[f"grad_cls{l}"] = a, b, c
    return out


def _head_loss_check(got, i):
    from head_loss_contract import bound_rows
    _, ref = _head_loss_inputs()
    names = ["loss_centerness", "loss_bbox", "loss_cls"]
    rows = bound_rows("buffers", names, list(got["losses"]), ref[torch.float32][0], ref[torch.float64][0], None)
    rows += bound_rows("buffers, finalize", names, list(got["losses_again"]), ref[torch.float32][0], ref[torch.float64][0], None)
    L = len(i["ctr"])
    gnames = [f"grad_{k}{l}" for k in ("centerness", "bbox", "cls") for l in range(L)]
    rows += bound_rows("buffers", gnames, [got[n] for n in gnames], ref[torch.float32][1], ref[torch.float64][1], 1.0)
    assert all(r["ok"] for r in rows), [r for r in rows if not r["ok"]]
    assert torch.equal(got["n_pos"], got["n_pos_again"]) and float(got["n_pos"]) >= 1


CASES.append(Case("head_loss-forward_grads_finalize", ("sgc_head_loss_forward", "sgc_head_loss_scale_grads", "sgc_head_loss_finalize"),
                  lambda: dict(_head_loss_inputs()[0]), _head_loss_run, ref=lambda i: {}, check=_head_loss_check, only="cuda"))


# ======================================================================================================================================
# the two mask kernels, directly (their only other use is the opt-in masked tail): bit-exact against torch
# ======================================================================================================================================
MASK_GRIDS, MASK_FACTORS, MASK_DENSITIES = ((8, 8, 4), (4, 12, 8)), (1, 2, 4), (0.1, 0.5, 0.9)


def counted_valid(grid, factor):
    """A valid mask in which the coarse voxels of scale ``factor`` (2 or 4) have exactly 3, 4 and 5 (in turn) of their 8 contributing
    fine voxels set -- fine voxels f d + f/2 - 1 and f d + f/2 on each axis; the mean is 0.5 at exactly 4, which round() takes to the
    even 0 -- and, at factor 4, random values in the fine voxels that contribute to nothing.  Returns (valid int64 [X*Y*Z], counts)."""
    X, Y, Z = grid
    f, o = factor, factor // 2 - 1
    g = _gen(sum(grid) + factor)
    valid = (torch.rand(X, Y, Z, generator=g) < 0.5).to(torch.int64)
    counts = torch.zeros(X // f, Y // f, Z // f, dtype=torch.int64)
    j = 0
    for x in range(X // f):
        for y in range(Y // f):
            for z in range(Z // f):
                n = (3, 4, 5)[j % 3]
                on = torch.zeros(8, dtype=torch.int64)
                on[torch.randperm(8, generator=g)[:n]] = 1
                valid[x * f + o:x * f + o + 2, y * f + o:y * f + o + 2, z * f + o:z * f + o + 2] = on.view(2, 2, 2)
                counts[x, y, z] = n
                j += 1
    return valid.reshape(-1), counts.reshape(-1)


def check_mask_kernels(ops, device):
    """sgc_mask_dilate3 against max_pool3d(mask, 3, 1, 1) and sgc_valid_pyramid against nn.Upsample(size, mode='trilinear')(valid.float())
    .round().bool() (the formulation its comment cites), bit for bit; the refusals the entry points document."""
    for grid in MASK_GRIDS:
        V = grid[0] * grid[1] * grid[2]
        for density in MASK_DENSITIES:
            mask = (torch.rand(V, generator=_gen(V + int(10 * density))) < density).to(torch.uint8)
            assert 0 < int(mask.sum()) < V
            assert torch.equal(ops.mask_dilate3(mask.to(device), grid).cpu(), dilate3_ref(mask, grid)), (grid, density)
            for f in MASK_FACTORS:
                got = ops.valid_pyramid(mask.to(torch.int64).to(device), grid, f).cpu()
                assert got.dtype == torch.uint8 and torch.equal(got, valid_pyramid_ref(mask.to(torch.int64), grid, f)), (grid, density, f)
        for f in (2, 4):
            valid, counts = counted_valid(grid, f)
            want = valid_pyramid_ref(valid, grid, f)
            assert torch.equal(want, (counts >= 5).to(torch.uint8)) and {3, 4, 5} <= set(counts.tolist())       # 4 of 8 rounds to the even 0
            assert torch.equal(ops.valid_pyramid(valid.to(device), grid, f).cpu(), want), (grid, f)
        one = (torch.rand(V, generator=_gen(V)) < 0.5).to(torch.int64)                                        # factor 1: one contributing voxel
        assert torch.equal(ops.valid_pyramid(one.to(device), grid, 1).cpu(), one.to(torch.uint8))
    import re
    from sgcdet_amd._abi import SgcError
    m = torch.zeros(8 * 8 * 4, dtype=torch.uint8, device=device)
    for what, bad in (("aliased", lambda: ops._call("sgc_mask_dilate3", m, m, 8, 8, 4)),                                   # aliased pointers
                      ("factor", lambda: ops.valid_pyramid(torch.zeros(8 * 8 * 6, dtype=torch.int64, device=device), (8, 8, 6), 4)),      # 4 does not divide Z = 6
                      ("factor", lambda: ops.valid_pyramid(torch.zeros(6 * 8 * 4, dtype=torch.int64, device=device), (6, 8, 4), 4))):     # nor 4 X = 6
        try:
            bad()
        except SgcError as e:                                  # the entry point's own refusal, not a check of the wrapper
            assert re.search(r"sgc_(mask_dilate3|valid_pyramid) failed", str(e)) and what in str(e), str(e)
            continue
        raise AssertionError(f"a documented refusal ({what}) did not raise")
