"""The scene axis of the 3-D convolution passes (include/sgcdet_amd_scene_batch.h) on the GPU: ``sgc_conv3d_cl_bf16x3_batched`` and
``sgc_conv3d_wgrad_bf16x3_batched`` on every kernel family the plan can choose for a plain 3-D call (tests/buffer_cases_scene_batch.py),
for two and three scenes, against float64 ``F.conv3d`` / ``conv_transpose3d`` per scene.

Bound: 1e-4 of the tensor scale, the bound tests/test_gpu_conv3d.py holds a bf16x3 convolution pass to.  Bit identities are asserted
wherever the header promises them; a split launch WITHOUT a workspace accumulates with float atomics (include/sgcdet_amd.h: "same
values up to the rounding of a different summation order") and is held to the bound instead."""
import pytest
import torch

import buffer_cases_scene_batch as sb

pytestmark = pytest.mark.gpu

TOL = sb.TOL


def _dev(t, ops):
    d = {k: v.cuda() for k, v in t.items()}
    if "wt" in d:
        d["hi"], d["lo"] = ops.split_bf16(d["wt"])
    return d


def _bound(got, ref, what):
    scale = max(1.0, float(ref.abs().max()))
    err = float((got.double().cpu() - ref).abs().max())
    print(f"{what}: max|err| {err:.3e}, bound {TOL * scale:.3e}")
    assert torch.isfinite(got).all(), what
    assert err <= TOL * scale, f"{what}: off by {err:.3e} > {TOL:.0e} * {scale:.3e}"


@pytest.mark.parametrize("scenes", [2, 3])
@pytest.mark.parametrize("c", sb.FWD, ids=repr)
def test_batched_forward(c, scenes, gpu_ops):
    t = _dev(sb.fwd_inputs(c), gpu_ops)
    og = c.out_grid
    V, OV = c.grid[0] * c.grid[1] * c.grid[2], og[0] * og[1] * og[2]
    ref = sb.fwd_reference(c)
    atomic = sb.fwd_is_atomic(gpu_ops, c, scenes)
    # accuracy: every scene against its own float64 convolution
    y = sb.launch_fwd(gpu_ops, c, t, scenes)
    _bound(y, ref[:scenes * OV], f"{c} B={scenes}")
    # reproducibility
    y2 = sb.launch_fwd(gpu_ops, c, t, scenes)
    if atomic:
        _bound(y2, ref[:scenes * OV], f"{c} B={scenes} second launch (float atomics)")
    else:
        assert torch.equal(y, y2), "two launches differ"
    # scenes = 1: the batched entry is the scene-less entry
    if scenes == 2 and not sb.fwd_is_atomic(gpu_ops, c, 1):
        one = sb.launch_fwd(gpu_ops, c, t, 1)
        assert torch.equal(one, sb.launch_fwd(gpu_ops, c, t, 1, entry="sgc_conv3d_cl_bf16x3"))
        _bound(one, ref[:OV], f"{c} B=1")
    # isolation: a scene of NaN reaches no other scene
    for bad in range(scenes):
        xn, xz = t["x"][:scenes * V].clone(), t["x"][:scenes * V].clone()
        xn[bad * V:(bad + 1) * V] = float("nan")
        xz[bad * V:(bad + 1) * V] = 0.0
        yn, yz = sb.launch_fwd(gpu_ops, c, t, scenes, x=xn), sb.launch_fwd(gpu_ops, c, t, scenes, x=xz)
        keep = torch.ones(scenes * OV, dtype=torch.bool, device="cuda")
        keep[bad * OV:(bad + 1) * OV] = False
        assert torch.isfinite(yn[keep]).all(), f"NaN of scene {bad} reached another scene"
        if atomic:
            _bound(yn[keep], ref[:scenes * OV][keep.cpu()], f"{c} B={scenes} beside a NaN scene (float atomics)")
        else:
            assert torch.equal(yn[keep], yz[keep]) and torch.equal(yz[keep], y[keep])


@pytest.mark.parametrize("scenes", [2, 3])
@pytest.mark.parametrize("c", sb.WGRAD, ids=repr)
def test_batched_weight_gradient(c, scenes, gpu_ops):
    t = _dev(sb.wgrad_inputs(c), gpu_ops)
    og = c.out_grid
    V, OV = c.grid[0] * c.grid[1] * c.grid[2], og[0] * og[1] * og[2]
    dw = sb.launch_wgrad(gpu_ops, c, t, scenes)
    _bound(dw, sb.wgrad_reference(c, scenes), f"{c} B={scenes}")
    assert torch.equal(dw, sb.launch_wgrad(gpu_ops, c, t, scenes)), "two launches differ"
    if scenes == 2:
        one = sb.launch_wgrad(gpu_ops, c, t, 1)
        assert torch.equal(one, sb.launch_wgrad(gpu_ops, c, t, 1, entry="sgc_conv3d_wgrad_bf16x3"))
        _bound(one, sb.wgrad_reference(c, 1), f"{c} B=1")
    # isolation.  dW is a sum over the scenes, so the statement is about taps: with dy = 0 in the last scene, that scene's x is only
    # ever multiplied by zeros -- unless a tap of another scene reads across the border.  Huge finite values there (1e30; NaN and inf
    # would turn 0 * x into NaN, which the kernels propagate as float64 does) must leave dW bit-identical to zeros
    # there, and equal to the gradient of the remaining scenes.
    xz, xh, dz = t["x"][:scenes * V].clone(), t["x"][:scenes * V].clone(), t["dy"][:scenes * OV].clone()
    xz[(scenes - 1) * V:] = 0.0
    xh[(scenes - 1) * V:] = 1e30
    dz[(scenes - 1) * OV:] = 0.0
    got = sb.launch_wgrad(gpu_ops, c, dict(x=xz, dy=dz), scenes)
    _bound(got, sb.wgrad_reference(c, scenes - 1), f"{c} B={scenes}, last scene zero")
    assert torch.equal(sb.launch_wgrad(gpu_ops, c, dict(x=xh, dy=dz), scenes), got), "a tap crossed a scene border"
    # ... and every other scene in turn (at B = 3 the middle one: a neighbour on either side), zeros against 1e30
    for bad in range(scenes - 1):
        xz, xh, dz = t["x"][:scenes * V].clone(), t["x"][:scenes * V].clone(), t["dy"][:scenes * OV].clone()
        xz[bad * V:(bad + 1) * V] = 0.0
        xh[bad * V:(bad + 1) * V] = 1e30
        dz[bad * OV:(bad + 1) * OV] = 0.0
        want = sb.launch_wgrad(gpu_ops, c, dict(x=xz, dy=dz), scenes)
        assert torch.isfinite(want).all()
        assert torch.equal(sb.launch_wgrad(gpu_ops, c, dict(x=xh, dy=dz), scenes), want), f"a tap crossed the border of scene {bad}"


@pytest.mark.parametrize("scenes", [3])
@pytest.mark.parametrize("c", sb.FWD + sb.WGRAD, ids=repr)
def test_batched_entries_write_all_of_their_output_and_nothing_beyond(c, scenes, gpu_ops):
    from buffer_contract import run_case
    run_case(sb.buffer_case(gpu_ops, c, scenes), gpu_ops, "cuda", ref_ops=None)


def test_refusals_come_before_any_store(gpu_ops):
    """scenes < 1 is SGC_EINVAL (-1); what the batched entries do not take is SGC_EUNSUP (-3); either way y keeps its sentinel."""
    from sgcdet_amd._abi import SgcError
    c = sb.FWD[0]
    t = _dev(sb.fwd_inputs(c), gpu_ops)
    V = c.grid[0] * c.grid[1] * c.grid[2]
    y = torch.full((2 * V, c.cout), 7.25, device="cuda")
    dw = torch.full((c.taps, c.cout, c.cin), 7.25, device="cuda")

    def fwd(grid, cin, k, s, tr, scenes):
        gpu_ops._call("sgc_conv3d_cl_bf16x3_batched", t["x"], t["hi"], t["lo"], None, None, None, y, *grid, cin, c.cout, k, s, tr, 0, scenes, None, 0)
    for args, status in (((c.grid, c.cin, 1, 1, 0, 0), -1), ((c.grid, c.cin, 1, 1, 0, -2), -1),
                         ((c.grid, 40, 1, 1, 0, 2), -3),                     # Cin % 32
                         ((c.grid, c.cin, 3, 1, 1, 2), -3),                  # transposed is k2 s2
                         ((c.grid, c.cin, 5, 1, 0, 2), -3),                  # no such kernel size
                         (((1024, 1024, 64), c.cin, 1, 1, 0, 4), -3)):       # 4 x 2^26 rows x 8 reaches 2^31: beyond the 32-bit row arithmetic
        with pytest.raises(SgcError, match=f"status {status}:"):
            fwd(*args)
    with pytest.raises(SgcError, match="status -1:"):
        gpu_ops._call("sgc_conv3d_wgrad_bf16x3_batched", t["x"], t["x"], dw, *c.grid, c.cin, c.cout, 1, 1, 0, None, 0)
    with pytest.raises(SgcError, match="status -3:"):
        gpu_ops._call("sgc_conv3d_wgrad_bf16x3_batched", t["x"], t["x"], dw, *c.grid, c.cin, c.cout, 5, 1, 2, None, 0)
    # the forms without a scene axis: refused by the wrapper before any launch, and the fp32 query knows no batch
    hi, lo = t["hi"].new_zeros(27, 32, 32), t["lo"].new_zeros(27, 32, 32)
    x3 = torch.zeros(2 * 64, 32, device="cuda")
    n0 = gpu_ops.n_calls
    with pytest.raises(RuntimeError, match="one scene per launch"):
        gpu_ops.conv3d_cl_bf16x3(x3, hi, lo, (4, 4, 4), 3, 1, out_mask=torch.ones(128, dtype=torch.uint8, device="cuda"), scenes=2)
    with pytest.raises(RuntimeError, match="one scene per launch"):
        gpu_ops.conv3d_cl_bf16x3(x3, hi, lo, (4, 4, 4), 3, 1, act=(0, 4, torch.ones(1, device="cuda")), scenes=2)
    assert gpu_ops.n_calls == n0
    assert int(gpu_ops.lib._dll.sgc_conv3d_batched_workspace_floats(10, 10, 4, 1024, 1024, 3, 1, 0, 0, 2)) == 0
    torch.cuda.synchronize()
    assert bool((y == 7.25).all()) and bool((dw == 7.25).all())


def test_wrappers_take_the_scene_count(gpu_ops):
    """``TensorOps.conv3d_cl_bf16x3 / conv3d_wgrad_bf16x3(..., scenes=)`` are the raw launches above."""
    c = next(x for x in sb.FWD if x.name == "tile_k3s1_span_ws")
    t = _dev(sb.fwd_inputs(c), gpu_ops)
    V = c.grid[0] * c.grid[1] * c.grid[2]
    y, og = gpu_ops.conv3d_cl_bf16x3(t["x"][:2 * V], t["hi"], t["lo"], c.grid, c.k, c.s, False, t["scale"], t["shift"],
                                     t["residual"][:2 * V], c.epi, scenes=2)
    assert og == c.out_grid and torch.equal(y, sb.launch_fwd(gpu_ops, c, t, 2))
    w = next(x for x in sb.WGRAD if x.name == "wgrad_tile_k3s2_7x5x3")
    tw = _dev(sb.wgrad_inputs(w), gpu_ops)
    Vw, OVw = 7 * 5 * 3, 4 * 3 * 2
    dw = gpu_ops.conv3d_wgrad_bf16x3(tw["x"][:3 * Vw], tw["dy"][:3 * OVw], w.grid, w.k, w.s, scenes=3)
    assert torch.equal(dw, sb.launch_wgrad(gpu_ops, w, tw, 3))
