"""Every HIP entry point that writes device memory under the buffer contract (tests/buffer_contract.py, DESIGN.md "Buffers"): outputs
and workspaces pre-filled with a NaN and with a large finite sentinel, guard bands around every allocation, inputs inside NaN-filled
parents.  One case per kernel family at the smallest shape that reaches it (tests/buffer_cases.py); references are the oracle or
float64 torch, bounds those of each kernel's existing test."""
import pytest
import torch

from buffer_cases import CASES, check_mask_kernels
from buffer_contract import run_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_buffer_contract(case, oracle_ops, gpu_ops):
    run_case(case, gpu_ops, "cuda", ref_ops=oracle_ops)
    torch.cuda.synchronize()


def test_mask_kernels_against_torch(gpu_ops):
    check_mask_kernels(gpu_ops, "cuda")


# ---- the modules must not read what the kernels leave undefined -------------------------------------------------------------------------
def _under_each_kind(body):
    """``body()`` under each sentinel kind -> {kind: result}; every allocation's guard bands are checked after the run."""
    from buffer_contract import KINDS, prefilled
    out = {}
    for kind in KINDS:
        with prefilled(kind) as ledger:
            out[kind] = body()
            torch.cuda.synchronize()
        assert ledger.n_allocations > 50, f"kind {kind}: only {ledger.n_allocations} allocations went through the patched functions"
        bad = ledger.damaged()
        assert not bad, f"kind {kind}: guard band damaged: {bad[:4]}"
    return out


def test_eval_with_device_counts_reads_no_capacity_tail(gpu_ops):
    """cfg1 through the eager hot path in the static-capacity mode (the mode of the scene graph, without a capture: pair and voxel
    counts stay on the device, every buffer is sized cap = N * Nq, so every capacity tail exists and holds the sentinel): against
    the oracle path within the bounds and the tie allowance of tests/test_gpu_modules.py::test_hot_path_against_oracle, every head
    output finite, and everything bit-identical between the two sentinel kinds."""
    import sgcdet_amd.plugin  # noqa: F401
    from golden_util import depth_pyramid, max_err
    from oracle.compare import check_sparse_head
    from oracle.ref_path import RefPath
    from sgcdet_amd.mmcv_lite import build_detector
    from sgcdet_amd.plugin.voxformer import scene_constants_host
    from sgcdet_amd.scene import make_scene, model_config, workload
    from test_gpu_modules import _check_neck_head_on
    w = workload("cfg1_plumbing")
    torch.manual_seed(7)
    det = build_detector(model_config(w)).eval()
    gen = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for n, p in det.voxel_head.named_parameters():
            p.add_(torch.randn(p.shape, generator=gen) * 0.05)
    feats, dpt, meta = make_scene(2, w["embed_dims"], kind=w["kind"], seed=5)
    rp = RefPath(det.voxel_head.state_dict(), dict(embed_dims=w["embed_dims"], n_voxels_list=w["n_voxels_list"], voxel_size_list=w["voxel_size_list"],
                                                   topk_list=w["topk_list"], dbound=(0.2, 5.0), num_heads=8, num_points=4))
    vol_c, valid_c, occ_c = rp.adaptive_sparse_head(feats, meta, depth_pyramid(dpt))
    det = det.cuda()
    det.use_graph = det.scene_graph = False                    # the patched allocator must not run inside a capture
    rp2 = RefPath({**{"neck." + k: v for k, v in det.neck_3d.state_dict().items()}, **{"head." + k: v for k, v in det.bbox_head.state_dict().items()}},
                  dict(head="scannet" if w["head"].startswith("ScanNet") else "sunrgbd", n_classes=w["n_classes"], nms_pre=1000))
    x, d = [f.cuda() for f in feats], dpt.cuda()
    static = dict(meta)
    static["_sgc_scene_const"] = scene_constants_host(meta).cuda()
    static["_sgc_static"] = True
    n_fin = w["n_voxels_list"][-1][0] * w["n_voxels_list"][-1][1] * w["n_voxels_list"][-1][2]

    def body():
        with torch.no_grad():
            volume, valid, occ = det.build_volume_from_features(x, [static], d)
            outs = det._neck_head_eager(volume, valid)
            _check_neck_head_on(det, vol_c, rp2)               # the HIP neck + head on the oracle's volume, 1e-3 of the scale
        return dict(volume=volume, valid=valid, occ=occ, head=list(outs[0]) + list(outs[1]) + list(outs[2]))
    runs = _under_each_kind(body)
    for kind, r in runs.items():
        assert all(bool(torch.isfinite(t).all()) for t in r["head"]), kind
        res = check_sparse_head(r["volume"], r["valid"], r["occ"], vol_c, valid_c, occ_c, n_fin, w["topk_list"])
        assert res["tie_flips"] <= 4, (kind, res)
        if res["tie_flips"] == 0:
            ctr, reg, cls = rp2.head(rp2.neck(vol_c, prefix="neck."), prefix="head.")
            for a, b in zip(r["head"], ctr + reg + cls):
                assert max_err(a, b) < 1e-3 * max(1.0, b.abs().max().item()), kind
    a, b = runs["A"], runs["B"]
    assert torch.equal(a["volume"], b["volume"]) and torch.equal(a["valid"], b["valid"]) and torch.equal(a["occ"], b["occ"])
    assert all(torch.equal(s, t) for s, t in zip(a["head"], b["head"]))


def test_one_training_step_reads_no_capacity_tail(gpu_ops):
    """The first step of tests/test_gpu_modules.py::test_three_sgd_steps_with_the_batched_weight_planes (cfg1, three views, its loss).

    (1) The whole step under each sentinel kind: the loss and every parameter gradient finite, the loss within that test's first-step
    bound (1e-6) of the step without the patch.
    (2) The gradient VALUES are compared on one fixed forward, not step against step: the training forward carries float-atomic noise
    of 1e-8 (relative), and the training-mode BatchNorms of the coarsest neck scale (5 x 5 x 2 = 50 voxels, channels of tiny variance
    at initialisation) amplify it -- two steps WITHOUT the patch differ by up to 8.5e-2 of a gradient tensor's max-abs (measured:
    neck_3d.down_layer_2.0.conv2.weight; 4.9e-2 for up_block_2.3.weight), and a step under either sentinel differs from a plain one by
    the same figures, so a step-against-step bound would test the conditioning of the model, not the buffers.  On a fixed forward the
    backward is reproducible to 7e-8, and the gradients under each kind are held to the bound tests/test_gpu_kernels.py holds two
    runs of the training level to (1e-4 of the scale; the backward kernels use float atomics, so no bit equality): for a forward made
    without the patch, and for a forward made UNDER the patch (what it saved for the backward lies in sentinel-filled buffers) against
    the plain backward of that same graph.
    (3) So that a gross error from a wrong tensor saved by a forward under the patch still fails, the gradients of the whole step under
    the patch are also held against the plain step, loosely: 0.25 of the tensor's max-abs, three times the largest spread two plain steps
    show among themselves (tools/train_step_spread.py, profiles/r20_train_step_spread.json: plain against plain 4.1e-2 ... 4.9e-2 in that
    run and 8.5e-2 in another, a sentinel step against a plain one 4.9e-2 ... 8.5e-2; the spread takes a few discrete values), plus
    1e-6 of the largest gradient of the model for the tensors that are rounding noise alone.  A sentinel that reached a gradient is NaN
    or 1e30."""
    import sgcdet_amd.plugin  # noqa: F401
    from buffer_contract import KINDS, prefilled
    from sgcdet_amd import functions
    from sgcdet_amd.mmcv_lite import build_detector
    from sgcdet_amd.scene import make_scene, model_config, workload
    from test_gpu_kernels import close
    w = workload("cfg1_plumbing")
    feats, dpt, meta = make_scene(3, w["embed_dims"], kind="scannet", seed=14, device="cuda")
    planes = functions.train_weight_planes()

    def forward():
        torch.manual_seed(23)
        det = build_detector(model_config(w)).cuda().train()
        det.use_graph = det.scene_graph = False
        for m in det.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.0
        planes.clear()
        r = det.forward_features(feats, [meta], dpt)
        loss = sum((t ** 2).mean() for k in ("centerness", "bbox_pred", "cls_score") for t in r[k]) + r["occ"].mean()
        return loss, [(k, p) for k, p in det.named_parameters() if p.requires_grad]

    def backward(loss, params):
        gs = torch.autograd.grad(loss, [p for _, p in params], retain_graph=True, allow_unused=True)
        torch.cuda.synchronize()
        return {k: g.detach().clone() for (k, _), g in zip(params, gs) if g is not None}

    def same(grads, want, what):
        assert grads.keys() == want.keys()
        for k, g in grads.items():
            assert bool(torch.isfinite(g).all()), (what, k)
            try:
                close(g, want[k], tol=1e-4)
            except AssertionError as e:
                raise AssertionError(f"{what}: {k}: {e}")
    try:
        loss0, params0 = forward()
        grads0, loss_plain = backward(loss0, params0), float(loss0.detach())
        assert len(grads0) > 20 and sum(float(g.abs().max()) > 0 for g in grads0.values()) > 20
        assert all(bool(torch.isfinite(g).all()) for g in grads0.values())
        for kind in KINDS:
            with prefilled(kind) as ledger:                                   # the plain forward, the backward under the patch
                got = backward(loss0, params0)
            assert ledger.n_allocations > 20 and ledger.guards_intact(), kind
            same(got, grads0, f"kind {kind}, backward of the plain forward")
        del loss0, params0
        for kind in KINDS:
            with prefilled(kind) as ledger:                                   # the whole step under the patch
                loss, params = forward()
                got = backward(loss, params)
            assert ledger.n_allocations > 50 and ledger.guards_intact(), kind
            value = float(loss.detach())
            assert value == value and abs(value) < float("inf") and abs(value - loss_plain) <= 1e-6 * abs(loss_plain), (kind, value, loss_plain)
            same(got, backward(loss, params), f"kind {kind}, step under the patch against the plain backward of its graph")
            floor = 1e-6 * max(float(g.abs().max()) for g in grads0.values())
            for k, g in got.items():
                err, lim = float((g - grads0[k]).abs().max()), 0.25 * float(grads0[k].abs().max()) + floor
                assert err <= lim, f"kind {kind}: {k}: the step under the patch is {err:.3e} from the plain step (bound {lim:.3e})"
            del loss, params
    finally:
        planes.clear()

