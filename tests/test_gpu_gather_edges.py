"""Every form of the deformable gather on exact gate coordinates against the float64 reference of
tests/gather_edge_contract.py: t_im = -1, integers, T - 1 and T on every axis, faces and corners in combination, rows of
+-1e3 at the camera borders.  Every coordinate is exact in fp32, so no sample is excluded anywhere.  Bounds: the `close`
helper of tests/test_gpu_kernels.py (1e-5 of max(1, scale) forward, 2e-5 backward), and for forward results the same 1e-5
element by element of max(1, sum |terms|).  Knob variants are bit-identical to their form's default (csrc/tuning.hpp: results
never depend on a knob); tests/test_gather_edges_cpu.py shows what the bounds catch."""
import pytest
import torch

import gather_edge_contract as gc
from gather_edge_contract import BWD_TOL, FWD_TOL, check, check_rows
from tile_contract import check_bins, raw_to_headmajor, value_to_headmajor

pytestmark = pytest.mark.gpu

GRADS = ("grad_value", "grad_dist", "grad_loc", "grad_attn")
TILE_DEFAULTS = dict(tile_nw=0, tile_depth_lds=-1, tile_nbuf=0, tile_hg=0, tile_ds=1)
FWD_DEFAULTS = dict(fwd_variant=1, fwd_spl=1)
cu = lambda t: t.cuda()


def set_knobs(gpu_ops, **knobs):
    for key, val in knobs.items():
        gpu_ops.lib.call("sgc_set_tuning", key.encode(), int(val))


@pytest.fixture(scope="module")
def fused(request):
    cache = {}

    def get(name):
        if name not in cache:
            case = next(c for c in gc.FUSED_CASES if c[0] == name)
            c = gc.fused_inputs(case)
            d = lambda k: c[k].double()
            c["out"], c["score"] = gc.dfa3d_forward_ref(d("value"), d("dist"), c["shapes3"], c["lsi"], d("loc"), d("attn"))
            c["mag"], _ = gc.dfa3d_forward_ref(d("value").abs(), d("dist"), c["shapes3"], c["lsi"], d("loc"), d("attn"))
            c["out1"], _ = gc.dfa3d_forward_ref(d("value"), d("dist"), c["shapes3"], c["lsi"], d("loc"), None)
            _, c["grads"] = gc.dfa3d_backward_ref(c["value"], c["dist"], c["shapes3"], c["lsi"], c["loc"], c["attn"], c["go"])
            cache[name] = c
        return cache[name]
    return get


@pytest.fixture(scope="module")
def pairs(request):
    cache = {}

    def get(name):
        if name not in cache:
            _, Cm, HW, D = next(c for c in gc.PAIR_CASES if c[0] == name)
            p = gc.pair_inputs(Cm, HW, D)
            a = (p["dist"], p["ref_cam"], p["raw"], p["pair_cam"], p["pair_q"], p["H"], p["W"], p["M"], p["P"])
            p["out"] = gc.pairs_deform_gather_ref(p["value"], *a)
            p["mag"] = gc.pairs_deform_gather_ref(p["value"].abs(), *a)
            cache[name] = p
        return cache[name]
    return get


# ---- the fused batch operator and the item-list form -----------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in gc.FUSED_CASES])
def test_fused_batch_operator_and_backward(name, fused, gpu_ops):
    c = fused(name)
    g = {k: cu(c[k]) for k in ("value", "dist", "shapes3", "lsi", "loc", "attn", "go")}
    out, score = gpu_ops.dfa3d_forward(g["value"], g["dist"], g["shapes3"], g["lsi"], g["loc"], g["attn"], want_score=True)
    check(out, c["out"], FWD_TOL, f"fused {name} forward")
    check_rows(out, c["out"], c["mag"], f"fused {name} forward")
    check(score, c["score"], FWD_TOL, f"fused {name} score")
    out1, _ = gpu_ops.dfa3d_forward(g["value"], g["dist"], g["shapes3"], g["lsi"], g["loc"], None)
    check(out1, c["out1"], FWD_TOL, f"fused {name} forward, no weights")
    grads = gpu_ops.dfa3d_backward(g["value"], g["dist"], g["shapes3"], g["lsi"], g["loc"], g["attn"], g["go"])
    for gname, a, b in zip(GRADS, grads, c["grads"]):
        check(a, b, BWD_TOL, f"fused {name} {gname}")


@pytest.mark.parametrize("name", [c[0] for c in gc.FUSED_CASES])
def test_item_list_operator_and_backward(name, fused, gpu_ops):
    """The same items, cameras interleaved: item i samples map i % B."""
    c = fused(name)
    B = c["value"].shape[0]
    loc, attn, go = (c[k].flatten(0, 1).contiguous() for k in ("loc", "attn", "go"))
    item = (torch.arange(loc.shape[0]) % B).to(torch.int32)
    d = lambda t: t.double()
    want, _ = gc.dfa3d_forward_items_ref(d(c["value"]), d(c["dist"]), c["shapes3"], c["lsi"], d(loc), d(attn), item)
    mag, _ = gc.dfa3d_forward_items_ref(d(c["value"]).abs(), d(c["dist"]), c["shapes3"], c["lsi"], d(loc), d(attn), item)
    _, want_g = gc.dfa3d_backward_ref(c["value"], c["dist"], c["shapes3"], c["lsi"], loc, attn, go, item_batch=item)
    a = (cu(c["value"]), cu(c["dist"]), cu(c["shapes3"]), cu(c["lsi"]), cu(loc), cu(attn), cu(item))
    out = gpu_ops.dfa3d_forward_items(*a)
    check(out, want, FWD_TOL, f"items {name} forward")
    check_rows(out, want, mag, f"items {name} forward")
    for gname, x, y in zip(GRADS, gpu_ops.dfa3d_backward_items(*a, cu(go)), want_g):
        check(x, y, BWD_TOL, f"items {name} {gname}")


# ---- the four split `_ext` operators: depth_score_forward -> wms_forward, wms_backward -> depth_score_backward -----------
@pytest.fixture(scope="module")
def split():
    cache = {}

    def get(name):
        if name not in cache:
            c = gc.fused_inputs(next(c for c in gc.SPLIT_CASES if c[0] == name))
            cache[name] = (c, gc.split_reference(c))
        return cache[name]
    return get


@pytest.mark.parametrize("name", [c[0] for c in gc.SPLIT_CASES])
def test_split_ext_operators_and_backward(name, split, gpu_ops):
    c, ref = split(name)
    for l, (h, w) in enumerate(c["levels"]):
        gc.assert_coverage(gc.t_im_of(c["loc"][:, :, :, l], h, w, c["D"]), h, w, c["D"], f"split {name} level {l}")
    gc.check_split(gc.split_operators(gpu_ops, c, cu), ref, f"split {name}")


# ---- the pair-list gather: both kernels, 1 / 2 / 4 samples per lane, three sources of the depth taps -------------------
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("name", [c[0] for c in gc.PAIR_CASES])
def test_pair_list_gather(name, variant, pairs, gpu_ops):
    p = pairs(name)
    H, W, M, P, n, N = p["H"], p["W"], p["M"], p["P"], p["n"], p["N"]
    value, dist, rc, raw = cu(p["value"]), cu(p["dist"]), cu(p["ref_cam"]), cu(p["raw"])
    pc = gpu_ops.compact_pairs(cu(p["mask"]))
    assert int(pc["totals"][0]) == n and torch.equal(pc["pair_cam"].cpu(), p["pair_cam"]) and torch.equal(pc["pair_q"].cpu(), p["pair_q"])
    dp = gpu_ops.depth_pairs(dist, H, W)
    C = value.shape[2] * value.shape[3]
    vbuf = torch.cat([value.reshape(N * H * W, C), torch.zeros(1, C, device=value.device)])
    vz = vbuf[:N * H * W].view(N, H * W, M, C // M)
    run = lambda v=value, **kw: gpu_ops.pairs_deform_gather(v, dist, rc, raw, pc["pair_cam"], pc["pair_q"], kw.pop("count", n), H, W, M, P, **kw)
    set_knobs(gpu_ops, fwd_variant=variant, fwd_spl=1)
    try:
        base, base_dp = run(), run(dist_pairs=dp)
        check(base, p["out"], FWD_TOL, f"pairs {name} variant {variant}")
        check_rows(base, p["out"], p["mag"], f"pairs {name} variant {variant}")
        for what, got in (("device count", run(count=-1, totals=pc["totals"])[:n]), ("depth_pairs", run(dist_pairs=dp)),
                          ("zero_row", run(vz, dist_pairs=dp, zero_row=True)), ("zero_row, plain depth", run(vz, zero_row=True))):
            check(got, p["out"], FWD_TOL, f"pairs {name} variant {variant} {what}")
            check_rows(got, p["out"], p["mag"], f"pairs {name} variant {variant} {what}")
        if variant == 1 and name == "cm32":
            for spl in (2, 4):                                     # samples per lane: a scheduling choice, bit for bit
                set_knobs(gpu_ops, fwd_spl=spl)
                assert torch.equal(run(), base), f"fwd_spl {spl}"
                assert torch.equal(run(dist_pairs=dp), base_dp), f"fwd_spl {spl}, depth_pairs"
                check(run(vz, dist_pairs=dp, zero_row=True), p["out"], FWD_TOL, f"pairs {name} fwd_spl {spl} zero_row")
                check(run(count=-1, totals=pc["totals"])[:n], p["out"], FWD_TOL, f"pairs {name} fwd_spl {spl} device count")
    finally:
        set_knobs(gpu_ops, **FWD_DEFAULTS)


# ---- the geometry sample, alone and fused with its Linear ---------------------------------------------------------------
@pytest.fixture(scope="module")
def geometry():
    cache = {}

    def get(name):
        if name not in cache:
            _, C, HW, D = next(c for c in gc.GEOMETRY_CASES if c[0] == name)
            p = gc.geometry_inputs(C, HW, D)
            a = (p["dist"], p["ref_cam"], p["pair_cam"], p["pair_q"], p["H"], p["W"])
            p["out"] = gc.pairs_geometry_sample_ref(p["feat"], *a)
            p["mag"] = gc.pairs_geometry_sample_ref(p["feat"].abs(), *a)
            cache[name] = p
        return cache[name]
    return get


@pytest.mark.parametrize("name", [c[0] for c in gc.GEOMETRY_CASES])
def test_geometry_sample(name, geometry, gpu_ops):
    p = geometry(name)
    pc = gpu_ops.compact_pairs(cu(p["mask"]))
    assert int(pc["totals"][0]) == p["n"] and torch.equal(pc["pair_cam"].cpu(), p["pair_cam"]) and torch.equal(pc["pair_q"].cpu(), p["pair_q"])
    a = (cu(p["feat"]), cu(p["dist"]), cu(p["ref_cam"]), pc["pair_cam"], pc["pair_q"])
    got = gpu_ops.pairs_geometry_sample(*a, p["n"], p["H"], p["W"])
    check(got, p["out"], FWD_TOL, f"geometry {name}")
    check_rows(got, p["out"], p["mag"], f"geometry {name}")
    got = gpu_ops.pairs_geometry_sample(*a, -1, p["H"], p["W"], totals=pc["totals"])[:p["n"]]
    check(got, p["out"], FWD_TOL, f"geometry {name} device count")
    check_rows(got, p["out"], p["mag"], f"geometry {name} device count")


@pytest.mark.parametrize("name", [c[0] for c in gc.GEOMETRY_CASES])
def test_geometry_sample_fused_with_its_linear(name, geometry, gpu_ops):
    """sample @ W^T + shift in float64, at the bf16x3 bound the project uses for this kernel (1e-4 of the scale)."""
    p = geometry(name)
    C, Cout, N, S = p["feat"].shape[-1], 128, p["N"], p["H"] * p["W"]
    if not gpu_ops.pairs_geometry_linear_supported(C, Cout, N, S):
        reason = f"pairs_geometry_linear_supported({C}, {Cout}, {N}, {S}) says no"
        print(reason)
        pytest.skip(reason)
    g = torch.Generator().manual_seed(17)
    w = torch.randn(1, Cout, C, generator=g) * 0.1
    b = torch.randn(Cout, generator=g)
    hi, lo = gpu_ops.split_bf16(w)
    want = p["out"] @ w[0].double().t() + b.double()
    pc = gpu_ops.compact_pairs(cu(p["mask"]))
    a = (cu(p["feat"]), cu(p["dist"]), cu(p["ref_cam"]), pc["pair_cam"], pc["pair_q"])
    one = gpu_ops.pairs_geometry_linear(*a, p["n"], p["H"], p["W"], cu(hi), cu(lo), cu(b))
    check(one, want, 1e-4, f"geometry {name} + linear")
    dev = gpu_ops.pairs_geometry_linear(*a, -1, p["H"], p["W"], cu(hi), cu(lo), cu(b), totals=pc["totals"])[:p["n"]]
    check(dev, want, 1e-4, f"geometry {name} + linear, device count")


# ---- the LDS-tiled gather: window test, fix-up pass, every tile knob ---------------------------------------------------
def _binnings():
    """(case, bin_w, bin_h, halo): small windows that the lattice offsets leave, and bins (16, 8) without a halo -- the whole
    8 x 16 map; the 16 x 8 map also gets its own whole-map bin (8, 16)."""
    out = []
    for name, _, (H, W), _ in gc.PAIR_CASES:
        out += [(name, 4, 4, (1, 1)), (name, 16, 8, (0, 0))]
        if (W, H) != (16, 8):
            out.append((name, W, H, (0, 0)))
    return out


BINNINGS = _binnings()
BIN_IDS = [f"{b[0]}-{b[1]}x{b[2]}" for b in BINNINGS]


TILE_KNOBS = [dict(tile_nw=8), dict(tile_nw=16), dict(tile_hg=2), dict(tile_hg=8), dict(tile_hg=2, tile_nbuf=2),
              dict(tile_hg=8, tile_nbuf=2, tile_nw=16), dict(tile_nbuf=1, tile_nw=8), dict(tile_depth_lds=0), dict(tile_depth_lds=1),
              dict(tile_ds=0), dict(tile_ds=0, tile_depth_lds=1, tile_nw=16), dict(tile_depth_lds=0, tile_hg=2, tile_nbuf=2, tile_nw=8)]


@pytest.mark.parametrize("shifted", [False, True], ids=["plain", "head_shift"])
@pytest.mark.parametrize("binning", BINNINGS, ids=BIN_IDS)
def test_tiled_gather(binning, shifted, pairs, gpu_ops):
    name, bw, bh, halo = binning
    p = pairs(name)
    H, W, M, P, n = p["H"], p["W"], p["M"], p["P"], p["n"]
    rc = cu(p["ref_cam"])
    pc = gpu_ops.compact_pairs(cu(p["mask"]))
    before = {k: v.cpu() for k, v in pc.items()}
    b = gpu_ops.bin_pairs(rc, dict(pc, slot=pc["slot"].clone()), H, W, bw, bh)
    old = check_bins(b, before, p["ref_cam"], n, H, W, bw, bh)
    vhm, dist, rhm = cu(value_to_headmajor(p["value"])), cu(p["dist"]), cu(raw_to_headmajor(p["raw"][old], M, P))
    shift = None
    if shifted:
        shift = cu(torch.randint(-3, 4, (M, 2), generator=torch.Generator().manual_seed(5), dtype=torch.int32))
    run = lambda: gpu_ops.pairs_deform_gather_tiled(vhm, dist, b["pair_ref"], b["bin_offset"], rhm, H, W, P, bw, bh, halo[0], halo[1],
                                                    head_shift=shift, max_shift=(3, 3))[:n]
    what = f"tiled {name} bins {bw}x{bh} halo {halo}{' head_shift' if shifted else ''}"
    try:
        set_knobs(gpu_ops, **TILE_DEFAULTS)
        base = run()
        check(base, p["out"][old], FWD_TOL, what)
        check_rows(base, p["out"][old], p["mag"][old], what)
        for knobs in TILE_KNOBS:
            set_knobs(gpu_ops, **dict(TILE_DEFAULTS, **knobs))
            assert torch.equal(run(), base), f"{what}: {knobs} changes the result"
    finally:
        set_knobs(gpu_ops, **TILE_DEFAULTS)


# ---- the LDS-binned backward: owner waves, halo, global fall-back ------------------------------------------------------
@pytest.mark.parametrize("loc_heads", ["M", 1])
@pytest.mark.parametrize("binning", BINNINGS, ids=BIN_IDS)
def test_binned_backward(binning, loc_heads, gpu_ops):
    name, bw, bh, halo = binning
    _, Cm, (H, W), D = next(c for c in gc.PAIR_CASES if c[0] == name)
    if not gpu_ops.dfa3d_backward_binned_fits(H, W, Cm, D, bw, bh, halo):
        reason = f"dfa3d_backward_binned_fits({H}, {W}, {Cm}, {D}, {bw}, {bh}, {halo}) says no"
        print(reason)
        pytest.skip(reason)
    M, P, N, S = gc.PAIR_M, gc.PAIR_P, gc.PAIR_N, H * W
    LM = M if loc_heads == "M" else 1
    p = gc.pair_inputs(Cm, (H, W), D, loc_heads=LM)
    n = p["n"]
    pc = gpu_ops.compact_pairs(cu(p["mask"]))
    before = {k: v.cpu() for k, v in pc.items()}
    b = gpu_ops.bin_pairs(cu(p["ref_cam"]), dict(pc, slot=pc["slot"].clone()), H, W, bw, bh)
    old = check_bins(b, before, p["ref_cam"], n, H, W, bw, bh)
    g = torch.Generator().manual_seed(3)
    loc = p["loc"][old].view(n, LM, 1, P, 3).contiguous()               # items in the binned order, direct locations
    attn = torch.rand(n, LM, 1, P, generator=g)
    go = torch.randn(n, M * Cm, generator=g)
    cam = p["pair_cam"][old]
    assert torch.equal(cam, p["pair_cam"])                               # bin_pairs keeps the camera-major layout
    shapes3, lsi = torch.tensor([[H, W, D]]), torch.zeros(1, dtype=torch.int64)
    value, dist = p["value"], p["dist"].view(N, S, 1, D)
    if LM == 1:      # one sample set shared by the M channel groups: the one-head operator over C = M * Cm channels, weights 1
        _, want = gc.dfa3d_backward_ref(value.view(N, S, 1, M * Cm), dist, shapes3, lsi, loc, torch.ones(n, 1, 1, P), go, item_batch=cam)
        got = gpu_ops.dfa3d_backward_binned(cu(value), cu(dist), cu(loc), None, b["bin_offset"], cu(go), H, W, bw, bh, halo)
    else:
        _, want = gc.dfa3d_backward_ref(value, dist, shapes3, lsi, loc, attn, go, item_batch=cam)
        got = gpu_ops.dfa3d_backward_binned(cu(value), cu(dist), cu(loc), cu(attn), b["bin_offset"], cu(go), H, W, bw, bh, halo)
    what = f"binned backward {name} bins {bw}x{bh} halo {halo} loc_heads {loc_heads}"
    for gname, x, y in zip(GRADS, got, want):
        check(x.reshape(y.shape), y, BWD_TOL, f"{what} {gname}")
