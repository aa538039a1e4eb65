"""tests/odd_shape_contract.py on the HIP library: the convolutions on odd grids under stride 2, on axes of extent 1 and 2 and with
output widths that are no multiple of 4, straight through the C ABI; the training passes on the same edges; the 2-D entry on images
with a unit side; sgc_nchw_to_nhwc_crop on strided views.  References are float64 torch on the CPU; every case computes right or is
refused by a rule of include/sgcdet_amd.h (tests/test_odd_shapes_cpu.py proves the case lists and the references on the oracle)."""
import pytest
import torch

import odd_shape_contract as oc

pytestmark = pytest.mark.gpu

FORM_IDS = [f"k{k}s{s}{'t' if tr else ''}" for k, s, tr in oc.FORMS]


@pytest.mark.parametrize("form", oc.FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("entry", oc.ENTRIES)
def test_forward_sweep_refuses_or_is_right(entry, form, gpu_ops):
    """The counts are printed per entry and form; every Cout of the list is computed at least once in each (on the large grid where the
    split rule refuses it on all listed ones)."""
    tally = oc.check_forward_sweep(gpu_ops, "cuda", entry, form)
    assert tally.computed >= len(oc.COUTS)


def test_the_large_odd_grids_take_the_halo_kernel(gpu_ops):
    """The three >= 2048-voxel grids of the 3 x 3 x 3 stride-1 sweep -- one brick thin in x, in z, ragged in all three -- run on the
    halo-resident kernel wherever Cout reaches `halo_min_cout` (16).  The launch follows the plan that sgc_conv3d_workspace_floats
    answers from (csrc/conv3d.hip, plan_conv): with `conv_halo` 0 the same query describes the tile kernel, which splits these layers
    differently (Cin 32: 3 splits of 9 taps against none; Cin 96: 9 against 3 channel slices)."""
    for grid in oc.HALO_GRIDS:
        for cin in oc.CINS:
            for cout in oc.HALO_COUTS:
                planned = oc.split_floats(gpu_ops, "bf16x3", cin, cout, grid, (3, 1, False))
                try:
                    gpu_ops.lib.call("sgc_set_tuning", b"conv_halo", 0)
                    tile = oc.split_floats(gpu_ops, "bf16x3", cin, cout, grid, (3, 1, False))
                finally:
                    gpu_ops.lib.call("sgc_set_tuning", b"conv_halo", 1)
                ov = grid[0] * grid[1] * grid[2] * cout
                assert tile > 0 and planned != tile and planned % ov == 0, (grid, cin, cout, planned / ov, tile / ov)
                assert planned // ov <= cin // 32 and (cin > 32 or planned == 0)       # the halo kernel splits channel slices of 32, nothing else


def test_a_layer_without_output_is_refused_before_any_store(gpu_ops):
    oc.check_no_output_is_refused_before_any_store(gpu_ops, "cuda")


@pytest.mark.parametrize("k,s", oc.WGRAD_FORMS)
def test_weight_gradient_on_odd_grids(k, s, gpu_ops):
    oc.check_wgrad_sweep(gpu_ops, "cuda", k, s)


@pytest.mark.parametrize("k,s", oc.FUNCTION_FORMS)
def test_conv_function_on_odd_grids(k, s, gpu_ops):
    oc.check_conv_function(gpu_ops, "cuda", k, s)


def test_conv_transpose_function_on_unit_axes(gpu_ops):
    oc.check_conv_transpose_function(gpu_ops, "cuda")


@pytest.mark.parametrize("k", [1, 3])
def test_conv2d_on_unit_sides(k, gpu_ops):
    tally = oc.check_conv2d_sweep(gpu_ops, "cuda", k)
    assert tally.refused == 0 and tally.couts == set(oc.CONV2D_COUTS)


def test_conv2d_on_one_long_row_stays_on_the_tile_kernel(gpu_ops):
    """(N, H, W) = (1, 1, 2304) has the >= 2048 pixels of the 16 x 16-pixel halo form, but plan_conv asks for 8 rows and 8 columns: the
    tile kernel runs it.  Recorded here: the launch with `halo_2d` 0 (the tile kernel by decree) gives the same bits."""
    nhw, k, cin, cout = (1, 1, 2304), 3, 32, 28
    x, wt, _ = oc.conv2d_reference(nhw, k, cin)
    hi, lo = gpu_ops.split_bf16(wt[:, :cout].contiguous().cuda())
    got = gpu_ops.conv2d_nhwc_bf16x3(x.cuda(), hi, lo, nhw, k)
    try:
        gpu_ops.lib.call("sgc_set_tuning", b"halo_2d", 0)
        tile = gpu_ops.conv2d_nhwc_bf16x3(x.cuda(), hi, lo, nhw, k)
    finally:
        gpu_ops.lib.call("sgc_set_tuning", b"halo_2d", 1)
    assert torch.equal(got, tile)
    print("sgc_conv2d_nhwc_bf16x3 (1, 1, 2304) k3: tile kernel")
    # for the record, the same comparison on the image of the sweep that the plan gives to the halo form (another order of summation)
    nhw, cin, cout = (1, 47, 45), 96, 33
    x, wt, _ = oc.conv2d_reference(nhw, k, cin)
    hi, lo = gpu_ops.split_bf16(wt[:, :cout].contiguous().cuda())
    got = gpu_ops.conv2d_nhwc_bf16x3(x.cuda(), hi, lo, nhw, k)
    try:
        gpu_ops.lib.call("sgc_set_tuning", b"halo_2d", 0)
        tile = gpu_ops.conv2d_nhwc_bf16x3(x.cuda(), hi, lo, nhw, k)
    finally:
        gpu_ops.lib.call("sgc_set_tuning", b"halo_2d", 1)
    assert float((got - tile).abs().max()) < 2e-5 * max(1.0, float(tile.abs().max()))      # the bound test_conv2d_nhwc_matches_oracle_and_torch holds the pair to
    print(f"sgc_conv2d_nhwc_bf16x3 (1, 47, 45) k3, Cout 33: {'same bits as' if torch.equal(got, tile) else 'other bits than'} the tile kernel")


def test_crop_of_strided_views_is_plain_indexing(gpu_ops):
    in_place, vector_form = oc.check_crop_views(gpu_ops, "cuda")
    assert in_place.get(2, 0) > 0 and in_place.get(4, 0) > 0        # read where they lie, not through .contiguous()
    assert vector_form > 0                                             # the C = 64 / 128 sources reached the 64 x 64 / 16-byte form
