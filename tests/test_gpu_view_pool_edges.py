"""Every compiled form of ``sgc_view_mean``, ``sgc_view_attend``, ``sgc_view_attend_pq`` and ``sgc_view_attend_backward`` on
the visibility and softmax edges of tests/view_pool_edge_contract.py, and ``sgc_upsample2x_occ`` on unit axes and odd channel
counts; tests/test_view_pool_edges_cpu.py runs the same checks on the oracle.

Which kernel a parametrisation reaches (the dispatch at the end of view_pool.hip), g / d = view_group / view_depth:
  view_mean    C 256 | 128: g1 d4 view_mean_group_kernel<64 | 32, 4>, g1 d1 <64 | 32, 1>, g0 view_mean_kernel<float4>;
               C 32 view_mean_kernel<float4>; C 6 view_mean_kernel<float>
  view_attend  (C, heads) with heads * head_dim / 4 = 64: (256, 8 | 1 | 2 | 16), = 32: (128, 8 | 4):
               g1 d4 view_attend_group_kernel<64 | 32, 4>, g1 d1 <64 | 32, 1>, g0 view_attend_kernel<4>;
               C 64, 32 (8 heads) view_attend_kernel<4>; C 16, 8 view_attend_kernel<1>; C 24 raises
  view_attend_pq  C 256 | 128, d 1, 2, 4, 8: view_attend_pq_kernel<64 | 32, d>
  view_attend_backward  C 256 (8 heads and 1 head), 128, 64, 32: view_attend_backward_kernel<4> with 8 (64), 4, 2, 1 lanes
               per head; C 16, 8: view_attend_backward_kernel<1>; C 24 raises"""
import pytest
import torch

import view_pool_edge_contract as vc

pytestmark = pytest.mark.gpu

_KNOB_IDS = [f"g{g}d{d}" for g, d in vc.KNOBS]
_LAST_N = 65


@pytest.fixture(scope="module", autouse=True)
def default_form_results(gpu_ops):
    """one default-form case of every entry point, run before this module touches a knob; the last test runs them again"""
    return (vc.check_mean_reference(gpu_ops, "cuda", 256, _LAST_N, "production"),
            vc.check_attend_reference(gpu_ops, "cuda", 128, 8, _LAST_N, "production"),
            vc.check_pq_reference(gpu_ops, "cuda", 256, _LAST_N, "production"))


def _both(check, ops, *args):
    for variant in vc.VARIANTS:
        check(ops, "cuda", *args, variant)


@pytest.mark.parametrize("N", vc.NS)
@pytest.mark.parametrize("knobs", vc.KNOBS, ids=_KNOB_IDS)
@pytest.mark.parametrize("C", vc.MEAN_GROUP_C)
def test_view_mean_group_sizes(C, knobs, N, gpu_ops):
    vc.tuned(gpu_ops, *knobs, lambda: (_both(vc.check_mean_reference, gpu_ops, C, N), _both(vc.check_mean_exact, gpu_ops, C, N)))


@pytest.mark.parametrize("N", vc.NS)
@pytest.mark.parametrize("C", vc.MEAN_PLAIN_C)
def test_view_mean_float4_and_scalar(C, N, gpu_ops):
    _both(vc.check_mean_reference, gpu_ops, C, N)
    _both(vc.check_mean_exact, gpu_ops, C, N)


@pytest.mark.parametrize("N", vc.NS)
@pytest.mark.parametrize("knobs", vc.KNOBS, ids=_KNOB_IDS)
@pytest.mark.parametrize("C,heads", vc.ATTEND_GROUP)
def test_view_attend_group_sizes(C, heads, knobs, N, gpu_ops):
    vc.tuned(gpu_ops, *knobs, lambda: (_both(vc.check_attend_reference, gpu_ops, C, heads, N), _both(vc.check_attend_exact, gpu_ops, C, heads, N)))


@pytest.mark.parametrize("N", vc.NS)
@pytest.mark.parametrize("C,heads", vc.ATTEND_PLAIN)
def test_view_attend_generic(C, heads, N, gpu_ops):
    _both(vc.check_attend_reference, gpu_ops, C, heads, N)
    _both(vc.check_attend_exact, gpu_ops, C, heads, N)


@pytest.mark.parametrize("N", vc.NS)
@pytest.mark.parametrize("depth", vc.PQ_DEPTHS)
@pytest.mark.parametrize("C", vc.PQ_C)
def test_view_attend_pq_depths(C, depth, N, gpu_ops):
    vc.tuned(gpu_ops, 1, depth, lambda: (_both(vc.check_pq_reference, gpu_ops, C, N), _both(vc.check_pq_exact, gpu_ops, C, N)))


@pytest.mark.parametrize("N", vc.NS)
@pytest.mark.parametrize("C,heads", vc.BACKWARD)
def test_view_attend_backward(C, heads, N, gpu_ops):
    _both(vc.check_backward_reference, gpu_ops, C, heads, N)
    _both(vc.check_backward_exact, gpu_ops, C, heads, N)


@pytest.mark.parametrize("N", vc.NS)
@pytest.mark.parametrize("C", vc.MEAN_GROUP_C)
def test_view_mean_forms_are_bit_identical(C, N, gpu_ops):
    vc.check_mean_forms(gpu_ops, "cuda", C, N)


@pytest.mark.parametrize("N", vc.NS)
@pytest.mark.parametrize("C,heads", vc.ATTEND_GROUP)
def test_view_attend_forms_are_bit_identical(C, heads, N, gpu_ops):
    vc.check_attend_forms(gpu_ops, "cuda", C, heads, N)


@pytest.mark.parametrize("N", vc.NS)
@pytest.mark.parametrize("C", vc.PQ_C)
def test_view_attend_pq_depths_are_bit_identical(C, N, gpu_ops):
    vc.check_pq_forms(gpu_ops, "cuda", C, N)


def test_head_dim_3_raises_in_forward_and_backward(gpu_ops):
    vc.check_unsupported_head_dim(gpu_ops, "cuda")


def test_projected_query_capacity(gpu_ops):
    vc.check_pq_capacity(gpu_ops, "cuda")


@pytest.mark.parametrize("grid", vc.UP_GRIDS, ids=lambda g: "x".join(map(str, g)))
@pytest.mark.parametrize("C", vc.UP_CHANNELS)
def test_upsample2x_occ_unit_axes_and_odd_channels(C, grid, gpu_ops):
    vc.check_upsample(gpu_ops, "cuda", C, grid)


def test_knobs_are_back_at_their_defaults(gpu_ops, default_form_results):
    """last in the module: without touching a knob, one case of every entry point gives the result it gave before the first test"""
    mean, ctx, s = default_form_results
    assert torch.equal(vc.check_mean_reference(gpu_ops, "cuda", 256, _LAST_N, "production"), mean)
    assert torch.equal(vc.check_attend_reference(gpu_ops, "cuda", 128, 8, _LAST_N, "production"), ctx)
    assert torch.equal(vc.check_pq_reference(gpu_ops, "cuda", 256, _LAST_N, "production"), s)
