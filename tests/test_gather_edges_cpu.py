"""The float64 reference of tests/gather_edge_contract.py against the C oracle, on exact gate coordinates and on a random
interior set; the gate-class coverage of every tensor the GPU file uses; and the teeth: three deliberately wrong sampling
rules must miss the true reference by more than 100 x the forward bound.  No sample is left out anywhere: the bounds
(1e-5 of max(1, scale) forward, 2e-5 backward) are met by the fp32 oracle on the whole lattice."""
import pytest
import torch

import gather_edge_contract as gc
from gather_edge_contract import BWD_TOL, FWD_TOL, check, check_rows

GRADS = ("grad_value", "grad_dist", "grad_loc", "grad_attn")


def _interior_fused(case, seed):
    _, B, M, Cm, P, D, levels, rep = case
    c = gc.fused_inputs(case, seed)
    ts = [gc.interior_items(h, w, D, M, P, c["loc"].shape[0] * c["loc"].shape[1], seed + l)[0] for l, (h, w) in enumerate(levels)]
    loc = torch.stack([gc.loc_of(t, h, w, D) for t, (h, w) in zip(ts, levels)], 2)
    c["loc"] = loc.view(c["loc"].shape).contiguous()
    return c


@pytest.mark.parametrize("interior", [False, True], ids=["lattice", "interior"])
@pytest.mark.parametrize("case", gc.FUSED_CASES, ids=[c[0] for c in gc.FUSED_CASES])
def test_reference_matches_oracle_fused_forward_and_backward(case, interior, oracle_ops):
    c = _interior_fused(case, 3) if interior else gc.fused_inputs(case)
    d = lambda k: c[k].double()
    out_o, sc_o = oracle_ops.dfa3d_forward(c["value"], c["dist"], c["shapes3"], c["lsi"], c["loc"], c["attn"], want_score=True)
    out_r, sc_r = gc.dfa3d_forward_ref(d("value"), d("dist"), c["shapes3"], c["lsi"], d("loc"), d("attn"))
    check(out_o, out_r, FWD_TOL, "oracle forward")
    check(sc_o, sc_r, FWD_TOL, "oracle score")
    mag, _ = gc.dfa3d_forward_ref(d("value").abs(), d("dist"), c["shapes3"], c["lsi"], d("loc"), d("attn"))
    check_rows(out_o, out_r, mag, "oracle forward")
    out1_o, _ = oracle_ops.dfa3d_forward(c["value"], c["dist"], c["shapes3"], c["lsi"], c["loc"], None)
    check(out1_o, gc.dfa3d_forward_ref(d("value"), d("dist"), c["shapes3"], c["lsi"], d("loc"), None)[0], FWD_TOL, "oracle forward, no weights")
    g_o = oracle_ops.dfa3d_backward(c["value"], c["dist"], c["shapes3"], c["lsi"], c["loc"], c["attn"], c["go"])
    _, g_r = gc.dfa3d_backward_ref(c["value"], c["dist"], c["shapes3"], c["lsi"], c["loc"], c["attn"], c["go"])
    for name, a, b in zip(GRADS, g_o, g_r):
        check(a, b, BWD_TOL, f"oracle {name}")
    if not interior:
        assert float(out_r.abs().max()) > 100 and float(g_r[2].abs().max()) > 100      # the +-1e3 rows are sampled


def test_reference_matches_oracle_item_list(oracle_ops):
    case = gc.FUSED_CASES[0]
    c = gc.fused_inputs(case)
    B = case[1]
    loc, attn, go = c["loc"].flatten(0, 1).contiguous(), c["attn"].flatten(0, 1).contiguous(), c["go"].flatten(0, 1).contiguous()
    item = (torch.arange(loc.shape[0]) % B).to(torch.int32)
    out_o = oracle_ops.dfa3d_forward_items(c["value"], c["dist"], c["shapes3"], c["lsi"], loc, attn, item)
    out_r, _ = gc.dfa3d_forward_items_ref(c["value"].double(), c["dist"].double(), c["shapes3"], c["lsi"], loc.double(), attn.double(), item)
    check(out_o, out_r, FWD_TOL, "oracle item forward")
    g_o = oracle_ops.dfa3d_backward_items(c["value"], c["dist"], c["shapes3"], c["lsi"], loc, attn, item, go)
    _, g_r = gc.dfa3d_backward_ref(c["value"], c["dist"], c["shapes3"], c["lsi"], loc, attn, go, item_batch=item)
    for name, a, b in zip(GRADS, g_o, g_r):
        check(a, b, BWD_TOL, f"oracle item {name}")


@pytest.mark.parametrize("interior", [False, True], ids=["lattice", "interior"])
@pytest.mark.parametrize("case", gc.PAIR_CASES, ids=[c[0] for c in gc.PAIR_CASES])
def test_reference_matches_oracle_pairs_deform_gather(case, interior, oracle_ops):
    _, Cm, HW, D = case
    p = gc.pair_inputs(Cm, HW, D, interior=interior)
    want = gc.pairs_deform_gather_ref(p["value"], p["dist"], p["ref_cam"], p["raw"], p["pair_cam"], p["pair_q"], p["H"], p["W"], p["M"], p["P"])
    got = oracle_ops.pairs_deform_gather(p["value"], p["dist"], p["ref_cam"], p["raw"], p["pair_cam"], p["pair_q"], p["n"],
                                         p["H"], p["W"], p["M"], p["P"])
    check(got, want, FWD_TOL, "oracle pairs_deform_gather")
    mag = gc.pairs_deform_gather_ref(p["value"].abs(), p["dist"], p["ref_cam"], p["raw"], p["pair_cam"], p["pair_q"], p["H"], p["W"], p["M"], p["P"])
    check_rows(got, want, mag, "oracle pairs_deform_gather")
    print(f"largest offset: {p['max_offset']} pixels")


@pytest.mark.parametrize("interior", [False, True], ids=["lattice", "interior"])
@pytest.mark.parametrize("case", gc.GEOMETRY_CASES, ids=[c[0] for c in gc.GEOMETRY_CASES])
def test_reference_matches_oracle_pairs_geometry_sample(case, interior, oracle_ops):
    _, C, HW, D = case
    p = gc.geometry_inputs(C, HW, D, interior=interior)
    want = gc.pairs_geometry_sample_ref(p["feat"], p["dist"], p["ref_cam"], p["pair_cam"], p["pair_q"], p["H"], p["W"])
    got = oracle_ops.pairs_geometry_sample(p["feat"], p["dist"], p["ref_cam"], p["pair_cam"], p["pair_q"], p["n"], p["H"], p["W"])
    check(got, want, FWD_TOL, "oracle pairs_geometry_sample")
    mag = gc.pairs_geometry_sample_ref(p["feat"].abs(), p["dist"], p["ref_cam"], p["pair_cam"], p["pair_q"], p["H"], p["W"])
    check_rows(got, want, mag, "oracle pairs_geometry_sample")


@pytest.fixture(scope="module")
def split(oracle_ops):
    """case name -> (inputs, the oracle's split operators on them): computed once, shared by the comparison and the teeth."""
    cache = {}

    def get(name):
        if name not in cache:
            c = gc.fused_inputs(next(c for c in gc.SPLIT_CASES if c[0] == name))
            cache[name] = (c, gc.split_operators(oracle_ops, c))
        return cache[name]
    return get


@pytest.mark.parametrize("name", [c[0] for c in gc.SPLIT_CASES])
def test_reference_matches_oracle_split_operators(name, split):
    """Largest error over the three cases: 1.2e-07 of the scale forward (score 6.0e-08), 2.6e-07 backward (grad_loc, two-level)."""
    c, got = split(name)
    for l, (h, w) in enumerate(c["levels"]):
        gc.assert_coverage(gc.t_im_of(c["loc"][:, :, :, l], h, w, c["D"]), h, w, c["D"], f"split {name} level {l}")
    gc.check_split(got, gc.split_reference(c), f"oracle split {name}")


@pytest.mark.parametrize("variant", gc.VARIANTS)
def test_wrong_sampling_rules_fail_the_split_comparison(variant, split):
    """The split path's own results against the reference under each wrong rule: more than 100 bounds away, where
    test_wrong_sampling_rules_miss_the_reference_by_100_bounds says the rule can show (the inclusive gate: grad_loc only)."""
    for case in gc.SPLIT_CASES:
        c, got = split(case[0])
        ref = gc.split_reference(c, variant)
        fwd = gc.rel_err(got["out"], ref["out"])
        bwd = {n: gc.rel_err(got[n], w) for n, w in zip(GRADS, ref["grads"])}
        print(f"{variant} / split {case[0]}: forward {fwd:.3e}, backward {max(bwd.values()):.3e} of the scale")
        if variant == "inclusive":
            assert fwd <= FWD_TOL and bwd["grad_loc"] > 100 * FWD_TOL
        else:
            assert fwd > 100 * FWD_TOL and max(bwd.values()) > 100 * FWD_TOL


def test_every_gpu_tensor_covers_every_gate_class():
    for case in gc.FUSED_CASES:
        c = gc.fused_inputs(case)
        for l, (h, w) in enumerate(c["levels"]):
            t = gc.t_im_of(c["loc"][:, :, :, l], h, w, c["D"])             # from the fp32 tensor the kernels read
            counts, combo = gc.assert_coverage(t, h, w, c["D"], f"fused {case[0]} level {l}")
            print(case[0], l, "rarest class", min(counts.values()), "rarest corner pair", combo)
    for case in gc.SPLIT_CASES:
        c = gc.fused_inputs(case)
        for l, (h, w) in enumerate(c["levels"]):
            gc.assert_coverage(gc.t_im_of(c["loc"][:, :, :, l], h, w, c["D"]), h, w, c["D"], f"split {case[0]} level {l}")
    for _, Cm, HW, D in gc.PAIR_CASES:
        p = gc.pair_inputs(Cm, HW, D)
        gc.assert_coverage(gc.t_im_of(p["loc"], *HW, D), *HW, D, f"pairs Cm {Cm}")
        p1 = gc.pair_inputs(Cm, HW, D, loc_heads=1)                          # the binned backward's shared sample set
        gc.assert_coverage(gc.t_im_of(p1["loc"], *HW, D), *HW, D, f"pairs Cm {Cm}, one sample set")
    for _, C, HW, D in gc.GEOMETRY_CASES:
        p = gc.geometry_inputs(C, HW, D)
        gc.assert_coverage(gc.t_im_of(p["ref_cam"], *HW, D), *HW, D, f"geometry C {C}")


@pytest.mark.parametrize("variant", gc.VARIANTS)
def test_wrong_sampling_rules_miss_the_reference_by_100_bounds(variant):
    """An inclusive gate at -1, truncation instead of floor, corner index T clamped to T - 1: each is far outside the bound
    on the lattice, on every case the GPU file runs.  ``trunc`` and ``clamp`` move the forward result.  The inclusive gate
    cannot: at t_im = -1 the only corner that exists has weight 0 -- it shows in the location gradient (d weight / d t = 1),
    so the forms with a backward see it and a forward-only form is the same function either way."""
    for case in gc.FUSED_CASES:
        c = gc.fused_inputs(case)
        out, grads = gc.dfa3d_backward_ref(c["value"], c["dist"], c["shapes3"], c["lsi"], c["loc"], c["attn"], c["go"])
        out_v, grads_v = gc.dfa3d_backward_ref(c["value"], c["dist"], c["shapes3"], c["lsi"], c["loc"], c["attn"], c["go"], variant=variant)
        fwd = gc.rel_err(out_v, out)
        bwd = max(gc.rel_err(a, b) for a, b in zip(grads_v, grads))
        print(f"{variant} / {case[0]}: forward {fwd:.3e}, backward {bwd:.3e} of the scale")
        if variant == "inclusive":
            assert fwd == 0.0 and gc.rel_err(grads_v[2], grads[2]) > 100 * FWD_TOL
        else:
            assert fwd > 100 * FWD_TOL and bwd > 100 * FWD_TOL
    if variant == "inclusive":
        return
    for _, Cm, HW, D in gc.PAIR_CASES:
        p = gc.pair_inputs(Cm, HW, D)
        a = (p["value"], p["dist"], p["ref_cam"], p["raw"], p["pair_cam"], p["pair_q"], p["H"], p["W"], p["M"], p["P"])
        assert gc.rel_err(gc.pairs_deform_gather_ref(*a, variant=variant), gc.pairs_deform_gather_ref(*a)) > 100 * FWD_TOL
    for _, C, HW, D in gc.GEOMETRY_CASES:
        p = gc.geometry_inputs(C, HW, D)
        a = (p["feat"], p["dist"], p["ref_cam"], p["pair_cam"], p["pair_q"], p["H"], p["W"])
        assert gc.rel_err(gc.pairs_geometry_sample_ref(*a, variant=variant), gc.pairs_geometry_sample_ref(*a)) > 100 * FWD_TOL
