"""tests/odd_shape_contract.py on the CPU oracle: the case lists, the refusal predicates and the float64 references are proved here,
where nothing splits a reduction and every shape with an output is computed; tests/test_gpu_odd_shapes.py runs the same checks on the
HIP library."""
import pytest

import odd_shape_contract as oc

FORM_IDS = [f"k{k}s{s}{'t' if tr else ''}" for k, s, tr in oc.FORMS]


@pytest.mark.parametrize("form", oc.FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("entry", oc.ENTRIES)
def test_forward_sweep_refuses_or_is_right(entry, form, oracle_ops):
    tally = oc.check_forward_sweep(oracle_ops, "cpu", entry, form)
    no_output = sum(0 in oc.out_grid(grid, *form) for cin, cout, grid in oc.forward_cases(oracle_ops, entry, form))
    assert tally.refused == no_output                       # the oracle refuses a layer only where torch has no output either
    assert (no_output > 0) == (form == (2, 2, False))


def test_case_lists_are_the_ones_the_issue_sets(oracle_ops):
    cases = oc.forward_cases(oracle_ops, "bf16x3", (3, 1, False))
    assert len(cases) == len(oc.CINS) * (len(oc.SMALL_GRIDS) * len(oc.COUTS) + len(oc.HALO_GRIDS) * len(oc.HALO_COUTS))
    assert len(oc.forward_cases(oracle_ops, "f32", (2, 2, True))) == len(oc.CINS) * len(oc.SMALL_GRIDS) * len(oc.COUTS)
    assert all(g[0] * g[1] * g[2] >= 2048 for g in oc.HALO_GRIDS)
    # the large grids leave >= 512 row tiles of 128 output voxels: no split at any width
    assert all(v[0] * v[1] * v[2] > 511 * 128 for v in (oc.out_grid(g, *f) for f, g in oc.LARGE_GRIDS.items()))
    assert {e[3] for e in oc.EPILOGUES} == {0, 1, 2}


def test_a_layer_without_output_is_refused_before_any_store(oracle_ops):
    oc.check_no_output_is_refused_before_any_store(oracle_ops, "cpu")


@pytest.mark.parametrize("k,s", oc.WGRAD_FORMS)
def test_weight_gradient_on_odd_grids(k, s, oracle_ops):
    tally = oc.check_wgrad_sweep(oracle_ops, "cpu", k, s)
    assert tally.refused == (2 * len(oc.WGRAD_CINS) * len(oc.WGRAD_COUTS) if k == 2 else 0)       # (1, 6, 1) and (13, 1, 11) under ksize 2


@pytest.mark.parametrize("k,s", oc.FUNCTION_FORMS)
def test_conv_function_on_odd_grids(k, s, oracle_ops):
    oc.check_conv_function(oracle_ops, "cpu", k, s)


def test_conv_transpose_function_on_unit_axes(oracle_ops):
    oc.check_conv_transpose_function(oracle_ops, "cpu")


@pytest.mark.parametrize("k", [1, 3])
def test_conv2d_on_unit_sides(k, oracle_ops):
    tally = oc.check_conv2d_sweep(oracle_ops, "cpu", k)
    assert tally.refused == 0 and tally.couts == set(oc.CONV2D_COUTS)


def test_crop_of_strided_views_is_plain_indexing(oracle_ops):
    in_place, _ = oc.check_crop_views(oracle_ops, "cpu")
    assert in_place.get(2, 0) > 0 and in_place.get(4, 0) > 0          # the front end's stride deduction hands the views over in place
