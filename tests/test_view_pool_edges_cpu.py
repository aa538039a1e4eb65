"""tests/view_pool_edge_contract.py on the CPU oracle: the contract's own preconditions (every visibility pattern present for
its N, an odd n_valid, the score gaps of the dominant-camera cases -- asserted inside the case builders) and its float64
references and exact cases hold on the oracle, so a miss of the HIP library in tests/test_gpu_view_pool_edges.py is the
library's.  The oracle has one form of every entry point: the knob settings are the GPU module's."""
import pytest

import view_pool_edge_contract as vc


@pytest.mark.parametrize("N", vc.NS)
def test_scene_holds_every_pattern(N):
    assert vc.check_scene(N) % 2 == 1


@pytest.mark.parametrize("N", vc.NS)
@pytest.mark.parametrize("C", vc.MEAN_GROUP_C + vc.MEAN_PLAIN_C)
def test_view_mean(C, N, oracle_ops):
    for variant in vc.VARIANTS:
        vc.check_mean_reference(oracle_ops, "cpu", C, N, variant)
        vc.check_mean_exact(oracle_ops, "cpu", C, N, variant)


@pytest.mark.parametrize("N", vc.NS)
@pytest.mark.parametrize("C,heads", vc.ATTEND_GROUP + vc.ATTEND_PLAIN)
def test_view_attend(C, heads, N, oracle_ops):
    for variant in vc.VARIANTS:
        vc.check_attend_reference(oracle_ops, "cpu", C, heads, N, variant)
        vc.check_attend_exact(oracle_ops, "cpu", C, heads, N, variant)


@pytest.mark.parametrize("N", vc.NS)
@pytest.mark.parametrize("C", vc.PQ_C)
def test_view_attend_pq(C, N, oracle_ops):
    for variant in vc.VARIANTS:
        vc.check_pq_reference(oracle_ops, "cpu", C, N, variant)
        vc.check_pq_exact(oracle_ops, "cpu", C, N, variant)


@pytest.mark.parametrize("N", vc.NS)
@pytest.mark.parametrize("C,heads", vc.BACKWARD)
def test_view_attend_backward(C, heads, N, oracle_ops):
    for variant in vc.VARIANTS:
        vc.check_backward_reference(oracle_ops, "cpu", C, heads, N, variant)
        vc.check_backward_exact(oracle_ops, "cpu", C, heads, N, variant)


def test_head_dim_3_on_the_oracle(oracle_ops):
    vc.check_unsupported_head_dim(oracle_ops, "cpu")


def test_projected_query_capacity(oracle_ops):
    vc.check_pq_capacity(oracle_ops, "cpu")


@pytest.mark.parametrize("grid", vc.UP_GRIDS, ids=lambda g: "x".join(map(str, g)))
@pytest.mark.parametrize("C", vc.UP_CHANNELS)
def test_upsample2x_occ_unit_axes_and_odd_channels(C, grid, oracle_ops):
    vc.check_upsample(oracle_ops, "cpu", C, grid)
