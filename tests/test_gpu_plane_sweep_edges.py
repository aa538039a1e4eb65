"""The plane sweep on its decision edges (tests/plane_sweep_edge_contract.py): ``sgc_plane_sweep_corr`` and
``sgc_plane_sweep_corr_backward`` against the float64 definition on an exact lattice of gate positions, behind the camera and on
non-finite positions; against the float64 reference formulation on ragged channel, plane, pixel and neighbour counts; and the scan,
list-length, tie, work-list, empty-list and id-guard edges of the backward, each asserted from the contract's own fp32 walk of the
positions inside the test that relies on it.  Bounds: 2e-5 of max(1, max |want|) forward, 1e-5 of max |ref| backward, on every
element -- no sample is left out.  tests/test_plane_sweep_edges_cpu.py holds the C oracle to the same forward checks and shows that
five wrong sampling rules fail them."""
import pytest
import torch

import plane_sweep_edge_contract as pc
from plane_sweep_edge_contract import check_backward, check_forward

pytestmark = pytest.mark.gpu


def _cuda(t):
    return t.cuda()


def _forward(ops, c):
    return ops.plane_sweep_corr(*pc.kernel_args(c, _cuda), c["H"], c["W"])


def _backward(ops, c):
    return ops.plane_sweep_corr_backward(*pc.kernel_args(c, _cuda), c["grad_corr"].cuda().contiguous(), c["H"], c["W"])


def _counts(c):
    return pc.list_walk(c["nbr"], c["rel"], c["depth"], c["H"], c["W"])["count"]


@pytest.mark.parametrize("name", [c[0] for c in pc.LATTICE_CASES])
def test_lattice_of_exact_gate_positions(gpu_ops, name):
    """Every quarter pixel from -1.5 to T + 0.5 on each axis against five fixed values of the other, 4 x 8 and 8 x 16 maps, K = 1, 2, 3,
    views that are their own neighbour; "behind": the same positions with pz = -1 (sampled: there is no gate on pz)."""
    c = pc.lattice(name)
    pc.assert_exact(c)
    corr, grad = pc.reference(pc.lattice, name)
    check_forward(_forward(gpu_ops, c), corr, name)
    check_backward(_backward(gpu_ops, c), grad, name)


def test_non_finite_and_huge_positions_contribute_nothing(gpu_ops):
    """pz == 0 (+inf, -inf, NaN positions), positions near +-1e30 and a single plane with pz == 0 between planes behind and in front of
    the camera, next to ordinary pairs: forward and backward equal the definition, in which such a sample adds nothing."""
    c = pc.nonfinite_case()
    pc.assert_nonfinite_classes(c)
    corr, grad = pc.reference(pc.nonfinite_case)
    check_forward(_forward(gpu_ops, c), corr, "nonfinite")
    check_backward(_backward(gpu_ops, c), grad, "nonfinite")


@pytest.mark.parametrize("name", list(pc.RAGGED))
def test_ragged_shapes_on_real_geometry(gpu_ops, name):
    """C = 1 .. 256 across the channel templates and their tails, D = 1 .. 32 across the plane groups of 4, 63 .. 260 pixels across the
    64-pixel tiles and the 4 rows per workgroup, K = 1 and 4: forward against reference_correlation(warp_f64), backward against its
    float64 autograd."""
    from plane_sweep_grad_contract import to_rows
    f_mvs, nbr, rel, depth, grad_corr = pc.ragged_inputs(name)
    N, C, H, W, K, D = pc.RAGGED[name]
    corr, grad = pc.ragged_reference(name)
    args = (to_rows(f_mvs).cuda(), nbr.to(torch.int32).contiguous().cuda(), rel.reshape(N, K, 12).contiguous().cuda(), depth.cuda())
    check_forward(gpu_ops.plane_sweep_corr(*args, H, W), corr, name)
    check_backward(gpu_ops.plane_sweep_corr_backward(*args, grad_corr.cuda().contiguous(), H, W), grad, name)


def test_forward_refuses_what_the_backward_refuses(gpu_ops):
    for C, D in ((257, 5), (65, 33)):
        rows, nbr = torch.zeros(3, 35, C, device="cuda"), torch.tensor([[1, 2], [0, 2], [0, 1]], dtype=torch.int32, device="cuda")
        rt, depth = torch.zeros(3, 2, 12, device="cuda"), torch.linspace(0.2, 5.0, D, device="cuda")
        with pytest.raises(RuntimeError):
            gpu_ops.plane_sweep_corr(rows, nbr, rt, depth, 5, 7)
    assert gpu_ops.plane_sweep_corr(torch.zeros(3, 35, 256, device="cuda"), nbr, rt, depth[:32].contiguous(), 5, 7).shape == (3, 32, 5, 7)


@pytest.mark.parametrize("name", [c[0] for c in pc.SCAN_CASES])
def test_backward_scan_boundaries(gpu_ops, name):
    """N * H * W = 2047, 2048, 2049: on and beside one 2048-count scan block; 525 312 rows: 257 block totals, so the top scan carries
    from its first 256 into the last (C = 4, D = 2, K = 1: the largest case of this file)."""
    c = pc.scan_case(name)
    rows = c["N"] * c["H"] * c["W"]
    assert f"rows{rows}" == name
    if rows > 4096:
        assert pc.scan_blocks(rows) > 256 and c["C"] <= 8 and c["D"] <= 2 and c["K"] == 1
        count = _counts(c)
        assert int(count[256 * pc.PSB_SCAN:].sum()) > 0 and int(count.max()) <= pc.PSB_CHUNK      # the last block has lists to place
    _, grad = pc.reference(pc.scan_case, name)
    check_backward(_backward(gpu_ops, c), grad, name)


def test_backward_list_lengths_511_to_1025(gpu_ops):
    """One destination row each with exactly 511, 512 (all 8 entries per lane of the sorted path), 513 (the first split: 512 + 1), 1024
    and 1025 entries, among ordinary short lists.  Rows of unsplit lists are bit-identical run to run."""
    c = pc.list_edge_case()
    HW = c["H"] * c["W"]
    count = _counts(c)
    assert [int(count[m * HW]) for m in range(5)] == [511, 512, 513, 1024, 1025]
    assert int((count > pc.PSB_CHUNK).sum()) == 3 and int(((count > 0) & (count < 256)).sum()) > 50
    _, grad = pc.reference(pc.list_edge_case)
    a, b = _backward(gpu_ops, c), _backward(gpu_ops, c)
    check_backward(a, grad, "list-edges")
    check_backward(b, grad, "list-edges, second run")
    short = (count <= pc.PSB_CHUNK).view(c["N"], HW)
    assert bool(short[0, 0]) and bool(short[1, 0])                            # the 511- and the 512-entry rows among them
    assert torch.equal(a.cpu()[short], b.cpu()[short])


def test_backward_identical_entries_keep_their_slots(gpu_ops):
    """Equal depths and a grad_corr equal across planes: every entry has seven twins with the same key.  The rank sort's tie rule
    must give each its own slot (a slot taken twice leaves another uninitialised): the float64 result, and the same bits twice."""
    c = pc.identical_case()
    walk = pc.list_walk(c["nbr"], c["rel"], c["depth"], c["H"], c["W"], c["grad_corr"])
    assert int(walk["count"].max()) == pc.PSB_CHUNK and pc.identical_entries(walk) == walk["dst"].numel() > 0
    _, grad = pc.reference(pc.identical_case)
    a, b = _backward(gpu_ops, c), _backward(gpu_ops, c)
    check_backward(a, grad, "identical")
    assert torch.equal(a, b)


def test_backward_work_list_beyond_one_wave_per_chunk(gpu_ops):
    """More chunks than the 4096 waves psb_long_kernel is launched with: its grid-stride loop.  No list is longer than 4096."""
    c = pc.work_list_case()
    count = _counts(c)
    assert pc.chunk_count(count) > pc.PSB_LONG_WAVES and int(count.max()) <= 4096
    _, grad = pc.reference(pc.work_list_case)
    check_backward(_backward(gpu_ops, c), grad, "work-list")


@pytest.mark.parametrize("kind", ["unnamed", "off-image"])
def test_backward_empty_lists(gpu_ops, kind):
    """A view nobody names as neighbour; every position off the image: no entries there, the reference-role term alone."""
    c = pc.empty_case(kind)
    count = _counts(c).view(c["N"], -1)
    assert int(count[2].sum() if kind == "unnamed" else count.sum()) == 0 and (kind == "off-image" or int(count.sum()) > 0)
    _, grad = pc.reference(pc.empty_case, kind)
    got = _backward(gpu_ops, c)
    check_backward(got, grad, kind)
    if kind == "off-image":
        assert not grad.any() and not got.any()


def test_backward_id_guard(gpu_ops):
    """nbr = -1 and nbr = N: the pair adds nothing in either role, 1 / K stays, every other row is as the definition has it.  The
    backward alone documents this guard (include/sgcdet_amd_train.h); the forward is not given such ids."""
    c = pc.id_guard_case()
    assert bool((c["nbr"] == -1).any()) and bool((c["nbr"] == c["N"]).any())
    _, grad = pc.reference(pc.id_guard_case)
    check_backward(_backward(gpu_ops, c), grad, "id-guard")
