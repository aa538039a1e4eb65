"""The plane-sweep edge contract (tests/plane_sweep_edge_contract.py) on the CPU: the lattice positions are exact in fp32, the
float64 definition reproduces the reference project's recorded results (tests/golden/plane_sweep.npz, plane_sweep_grad.npz), the C
oracle's ``sgc_plane_sweep_corr`` passes every forward check the HIP kernel is held to (tests/test_gpu_plane_sweep_edges.py), five
deliberately wrong sampling rules fail them, and the list lengths, chunk counts and scan sizes that the backward's cases are built for
are what the contract's own fp32 walk of the positions gives.  No sample is left out anywhere."""
import os

import numpy as np
import pytest
import torch

import plane_sweep_edge_contract as pc
from plane_sweep_edge_contract import BWD_TOL, FWD_TOL, check_backward, check_forward

LATTICE = [c[0] for c in pc.LATTICE_CASES]


def _oracle(oracle_ops, c):
    return oracle_ops.plane_sweep_corr(*pc.kernel_args(c), c["H"], c["W"])


@pytest.mark.parametrize("name", LATTICE)
def test_lattice_positions_are_exact_and_cover_every_quarter_pixel(name):
    c = pc.lattice(name)
    pc.assert_exact(c)
    pc.assert_lattice_coverage(c)
    assert bool((c["nbr"] == torch.arange(c["N"]).view(-1, 1)).any())          # a view that is its own neighbour
    # the walk of the backward sees what the reference sees: the corners that count, one entry each
    corners = pc._corners(pc.walk_f32(c["rel"], c["depth"], c["H"], c["W"]), c["H"], c["W"])
    assert int(pc.list_walk(c["nbr"], c["rel"], c["depth"], c["H"], c["W"])["count"].sum()) == sum(int(ok.sum()) for _, _, ok in corners)


def test_nonfinite_case_holds_the_classes_it_names():
    c = pc.nonfinite_case()
    assert c["N"] == len(pc.NONFINITE_KINDS)
    pc.assert_nonfinite_classes(c)


def test_non_finite_and_huge_positions_contribute_nothing_in_the_definition():
    """corr and the gradient equal those of the k = 1 pairs alone, halved (1 / K stays 1 / 2); on the "one-plane" view only the
    plane with pz == 0 drops out, and the planes behind the camera (pz < 0) are sampled like those in front of it."""
    c = pc.nonfinite_case()
    corr, grad = pc.reference(pc.nonfinite_case)
    corr1, grad1 = pc.grad_f64(c["rows"], c["nbr"][:, 1:], c["rel"][:, 1:], c["depth"], c["grad_corr"] / 2, c["H"], c["W"])
    one = pc.NONFINITE_KINDS.index("one-plane")
    assert torch.equal(corr[:one], corr1[:one] / 2)
    assert float((corr[one, 2] - corr1[one, 2] / 2).abs().max()) == 0.0
    for d in (0, 1, 3, 4):
        assert float((corr[one, d] - corr1[one, d] / 2).abs().max()) > 1e-3
    first = corr[one] - corr1[one] / 2                                         # what pair k = 0 adds
    assert float((first[0] - first[4]).abs().max()) <= 1e-12                   # the same position from behind and from the front
    # the gradient: the gated-off pairs add nothing in either role; only the on-image planes of view `one` add to its neighbour
    m = int(c["nbr"][one, 0])
    other = [n for n in range(c["N"]) if n not in (one, m)]
    assert float((grad[other] - grad1[other]).abs().max()) <= 1e-12 * float(grad.abs().max())
    assert float((grad[m] - grad1[m]).abs().max()) > 1e-3


def test_definition_reproduces_the_reference_projects_recorded_results():
    """tests/golden/plane_sweep.npz (cost volumes) and plane_sweep_grad.npz (gradients), at the bounds the kernels are held to."""
    from plane_sweep_grad_contract import GOLDEN, golden_cases, to_rows
    d = np.load(os.path.join(GOLDEN, "plane_sweep.npz"))
    cases = golden_cases()
    assert int(d["n_cases"]) == 3 and len(cases) == 5
    for k, (f_mvs, nbr, rel, depth, grad_corr, want_grad) in enumerate(cases):
        H, W = f_mvs.shape[2:]
        corr, grad = pc.grad_f64(to_rows(f_mvs), nbr, rel, depth, grad_corr, H, W)
        if k < 3:
            assert torch.equal(torch.from_numpy(d[f"f_mvs{k}"]), f_mvs)
            check_forward(corr, torch.from_numpy(d[f"corr{k}"]), f"definition, golden {k}")
        check_backward(grad, to_rows(want_grad), f"definition, golden {k}")


@pytest.mark.parametrize("name", LATTICE + ["nonfinite"])
def test_oracle_forward_on_the_lattice_behind_the_camera_and_on_non_finite_positions(name, oracle_ops):
    if name == "nonfinite":
        c, ref = pc.nonfinite_case(), pc.reference(pc.nonfinite_case)
    else:
        c, ref = pc.lattice(name), pc.reference(pc.lattice, name)
    check_forward(_oracle(oracle_ops, c), ref[0], f"oracle {name}")
    assert float((ref[0] != 0).double().mean()) > 0.2                         # the case samples the image


@pytest.mark.parametrize("name", list(pc.RAGGED))
def test_oracle_forward_and_definition_on_ragged_shapes(name, oracle_ops):
    """The oracle against reference_correlation(warp_f64); and the definition of this contract against the same (grid_sample in
    float64) with its autograd: two independent float64 formulations on real geometry."""
    from plane_sweep_grad_contract import to_rows
    f_mvs, nbr, rel, depth, grad_corr = pc.ragged_inputs(name)
    N, C, H, W, K, D = pc.RAGGED[name]
    assert f_mvs.shape == (N, C, H, W) and nbr.shape == (N, K) and depth.numel() == D
    corr, grad = pc.ragged_reference(name)
    got = oracle_ops.plane_sweep_corr(to_rows(f_mvs), nbr.to(torch.int32).contiguous(), rel.reshape(N, K, 12).contiguous(), depth, H, W)
    check_forward(got, corr, f"oracle {name}")
    corr_d, grad_d = pc.grad_f64(to_rows(f_mvs), nbr, rel, depth, grad_corr, H, W)
    check_forward(corr_d, corr, f"definition {name}")
    check_backward(grad_d, grad, f"definition {name}")
    assert float((corr != 0).double().mean()) > 0.2


@pytest.mark.parametrize("variant", pc.VARIANTS)
def test_wrong_sampling_rules_fail_the_lattice_checks(variant, oracle_ops):
    """Border clamping, trunc for floor, align_corners = True, W / 2 for (W - 1) / 2: each misses the definition on every lattice
    case, forward and backward, and the oracle's result fails the forward check against it.  A pz > 0 gate is the same function
    wherever pz > 0: it is the lattice behind the camera that rejects it."""
    cases = [n for n in LATTICE if n.endswith("behind")] if variant == "pz_gate" else LATTICE
    for name in cases:
        c = pc.lattice(name)
        corr, grad = pc.reference(pc.lattice, name)
        corr_v, grad_v = pc.grad_f64(c["rows"], c["nbr"], c["rel"], c["depth"], c["grad_corr"], c["H"], c["W"], variant=variant)
        fwd = float((corr_v - corr).abs().max()) / (FWD_TOL * max(1.0, float(corr.abs().max())))
        bwd = float((grad_v - grad).abs().max()) / (BWD_TOL * float(grad.abs().max()))
        print(f"{variant} / {name}: forward {fwd:.3g} bounds, backward {bwd:.3g} bounds")
        assert fwd > 1 and bwd > 1
        with pytest.raises(AssertionError):
            check_forward(_oracle(oracle_ops, c), corr_v, f"oracle against the {variant} rule, {name}")
    if variant == "pz_gate":
        for name in LATTICE[:2]:                                               # pz = 1 there: nothing to tell apart
            c = pc.lattice(name)
            corr_v, _ = pc.grad_f64(c["rows"], c["nbr"], c["rel"], c["depth"], c["grad_corr"], c["H"], c["W"], variant=variant)
            assert torch.equal(corr_v, pc.reference(pc.lattice, name)[0])


def test_list_lengths_of_the_list_edge_case():
    c = pc.list_edge_case()
    HW = c["H"] * c["W"]
    count = pc.list_walk(c["nbr"], c["rel"], c["depth"], c["H"], c["W"])["count"]
    assert {m: int(count[m * HW]) for m in c["lengths"]} == {0: 511, 1: 512, 2: 513, 3: 1024, 4: 1025}
    rest = count.clone()
    rest[[m * HW for m in c["lengths"]]] = 0
    assert 0 < int(rest.max()) <= 256 and int((rest > 0).sum()) > 50          # ordinary short lists in the same launch
    pos = pc.walk_f32(c["rel"], c["depth"], c["H"], c["W"])                     # every position is a multiple of 1/8: exact
    fin = pos["ix"].double() * 8
    assert torch.equal(fin, fin.round()) and torch.equal(c["rel"].double(), c["rel64"])


def test_identical_entries_of_the_identical_case():
    c = pc.identical_case()
    walk = pc.list_walk(c["nbr"], c["rel"], c["depth"], c["H"], c["W"], c["grad_corr"])
    assert int(walk["count"].max()) == 512 and int((walk["count"] == 512).sum()) == 2
    assert pc.identical_entries(walk) == walk["dst"].numel() and walk["dst"].numel() % 8 == 0
    assert int((walk["count"] % 8 != 0).sum()) == 0


def test_chunk_count_of_the_work_list_case():
    c = pc.work_list_case()
    count = pc.list_walk(c["nbr"], c["rel"], c["depth"], c["H"], c["W"])["count"]
    assert pc.chunk_count(count) > pc.PSB_LONG_WAVES and int(count.max()) <= 4096
    assert sorted(set(count.tolist())) == [0, 512, 1024, 2048]


@pytest.mark.parametrize("name", [c[0] for c in pc.SCAN_CASES])
def test_scan_sizes(name):
    _, N, H, W, K = next(c for c in pc.SCAN_CASES if c[0] == name)
    assert f"rows{N * H * W}" == name
    assert N * H * W in (2047, 2048, 2049) or pc.scan_blocks(N * H * W) > 256
    if N * H * W < 4096:
        c = pc.scan_case(name)
        count = pc.list_walk(c["nbr"], c["rel"], c["depth"], H, W)["count"]
        assert int(count[:pc.PSB_SCAN].sum()) > 0 and len(set(count.tolist())) > 4      # uneven counts on both sides of the block edge
        assert N * H * W == 2047 or int(count[pc.PSB_SCAN - 1:].sum()) > 0


def test_empty_cases_have_no_entries_and_keep_the_reference_role_alone():
    c = pc.empty_case("unnamed")
    HW = c["H"] * c["W"]
    count = pc.list_walk(c["nbr"], c["rel"], c["depth"], c["H"], c["W"])["count"]
    assert int(count[2 * HW:].sum()) == 0 and int(count[:2 * HW].sum()) > 0
    _, grad = pc.reference(pc.empty_case, "unnamed")
    _, own = pc.grad_f64(c["rows"], c["nbr"], c["rel"], c["depth"], c["grad_corr"], c["H"], c["W"], role="reference")
    assert torch.equal(grad[2], own[2]) and float(own[2].abs().max()) > 0 and not torch.equal(grad[0], own[0])
    c = pc.empty_case("off-image")
    assert int(pc.list_walk(c["nbr"], c["rel"], c["depth"], c["H"], c["W"])["count"].sum()) == 0
    corr, grad = pc.reference(pc.empty_case, "off-image")
    assert not corr.any() and not grad.any()


def test_id_guard_of_the_definition_equals_pairs_that_see_nothing():
    """An id outside [0, N) == a pair with a valid id whose warp puts every sample off the image: nothing in either role, 1 / K kept."""
    c = pc.id_guard_case()
    bad = (c["nbr"] < 0) | (c["nbr"] >= c["N"])
    assert int(bad.sum()) == 4 and bool((c["nbr"] == -1).any()) and bool((c["nbr"] == c["N"]).any()) and bool(bad[3].all())
    nbr, rel = c["nbr"].clone(), c["rel64"].clone()
    nbr[bad] = 0
    rel[bad] = pc.warp(c["H"], c["W"], *pc.OFF)
    _, want = pc.grad_f64(c["rows"], nbr, rel.float(), c["depth"], c["grad_corr"], c["H"], c["W"])
    _, grad = pc.reference(pc.id_guard_case)
    assert torch.equal(grad, want) and bool(grad[3].any())
    walk = pc.list_walk(c["nbr"], c["rel"], c["depth"], c["H"], c["W"])
    assert torch.equal(walk["count"], pc.list_walk(nbr, rel.float(), c["depth"], c["H"], c["W"])["count"])
