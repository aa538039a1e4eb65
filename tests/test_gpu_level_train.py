"""A view-transform level in training on the HIP kernels of include/sgcdet_amd_level_train.h, on the GPU.

Every kernel is compared with float64 torch on the CPU: autograd of the formulation the default training path uses, evaluated on the
same float32 inputs (tests/buffer_cases_level_train.py).  The bound of a kernel output is FOUR TIMES the error torch's own float32
CPU evaluation of that formulation has against float64 on the same inputs, relative to the output's max-abs, and never below 2e-6 of
that max-abs (the bound of the LayerNorm forward, tests/test_gpu_kernels.py): a different but equally valid summation order may cost a
small multiple of what torch's order costs, not more.  The test computes the CPU error itself and prints both figures.

The level tests run the ``voxel_head`` golden with ``TRAIN_LEVEL_FUSED`` off and on, with the bounds
tests/test_gpu_modules.py::test_pair_list_training_path_equals_the_padded_reference_layout uses for two formulations of a level."""
import contextlib

import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

from buffer_cases_level_train import (EPS, ln_inputs, ln_reference, sampling_inputs, sampling_reference, view_mean_inputs,
                                      view_mean_reference)
from golden_util import depth_pyramid, img_meta, load, max_err

pytestmark = pytest.mark.gpu

FLOOR = 2e-6


def _held(what, got, want64, cpu32):
    """|got - want64| <= max(4 * |cpu32 - want64|, FLOOR * scale), scale = max |want64|; non-finite elements must agree in kind."""
    got, cpu32 = got.detach().cpu().double(), cpu32.detach().cpu().double()
    fin = torch.isfinite(want64)
    assert torch.equal(torch.isnan(got), torch.isnan(want64)), f"{what}: NaN pattern differs from float64"
    assert torch.equal(got[~fin & ~torch.isnan(want64)], want64[~fin & ~torch.isnan(want64)]), f"{what}: infinities differ"
    scale = float(want64[fin].abs().max())
    cpu_err = float((cpu32[fin] - want64[fin]).abs().max()) / scale
    err = float((got[fin] - want64[fin]).abs().max()) / scale
    bound = max(4.0 * cpu_err, FLOOR)
    print(f"{what}: GPU {err:.3e}, torch float32 on the CPU {cpu_err:.3e}, bound {bound:.3e} (of max-abs {scale:.3e})")
    assert err <= bound, f"{what}: {err:.3e} > {bound:.3e}"


# ---- LayerNorm backward -----------------------------------------------------------------------------------------------------------------
LN_SHAPES = [(C, rows) for C in (128, 256) for rows in (1, 3, 4, 5, 1030)] + [(96, 5), (32, 5)]


@pytest.mark.parametrize("C,rows", LN_SHAPES)
def test_layer_norm_backward(C, rows, gpu_ops):
    """C 128 / 256: the register forms, rows below, on and above the four of a workgroup step, and 1 030 (no multiple of four, 129
    partials); C 96 / 32: the generic form with more / fewer columns than lanes.  The five-row cases hold a constant row, a row of
    zeros and a row with mean 10 and spread 3."""
    i = ln_inputs(rows, C, 100 + rows, special=rows == 5)
    want, cpu = ln_reference(i), ln_reference(i, torch.float32)
    c = {k: v.cuda() for k, v in i.items()}
    got = dict(zip(("dx", "dgamma", "dbeta"), gpu_ops.layer_norm_rows_backward(c["x"], c["gamma"], c["dy"], EPS)))
    again = gpu_ops.layer_norm_rows_backward(c["x"], c["gamma"], c["dy"], EPS)
    for k, b in zip(("dx", "dgamma", "dbeta"), again):
        assert torch.equal(got[k], b), f"{k}: a second launch gives other bits"
        _held(f"layer_norm_backward C {C} rows {rows} {k}", got[k], want[k], cpu[k])


def test_layer_norm_function_is_the_inference_forward_and_the_kernel_backward(gpu_ops):
    from sgcdet_amd.functions import LayerNormRowsFunction
    i = {k: v.cuda() for k, v in ln_inputs(37, 128, 7).items()}
    x, gamma, beta = (i[k].clone().requires_grad_(True) for k in ("x", "gamma", "beta"))
    y = LayerNormRowsFunction.apply(x, gamma, beta, EPS)
    assert torch.equal(y, gpu_ops.layer_norm_rows(i["x"], i["gamma"], i["beta"], EPS))
    y.backward(i["dy"])
    for got, want in zip((x.grad, gamma.grad, beta.grad), gpu_ops.layer_norm_rows_backward(i["x"], i["gamma"], i["dy"], EPS)):
        assert torch.equal(got, want)
    empty = LayerNormRowsFunction.apply(x[:0], gamma, beta, EPS)
    assert empty.shape == (0, 128)


# ---- sampling locations -------------------------------------------------------------------------------------------------------------------
SAMPLING_SHAPES = [(8, 1, 4, 128), (4, 2, 2, 64), (1, 1, 4, 32)]       # the configs' shape; two levels with different (W, H, D); padding columns


def _sampling_gpu(ops, i):
    c = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in i.items()}
    loc, attn = ops.sampling_locations_forward(c["ref"], c["proj"], c["normalizer"], c["M"], c["L"], c["P"])
    gp = ops.sampling_locations_backward(attn, c["grad_loc"], c["grad_attn"], c["normalizer"], c["proj"].shape[1])
    return dict(loc=loc, attn=attn, grad_proj=gp)


@pytest.mark.parametrize("M,L,P,ldp", SAMPLING_SHAPES)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_sampling_locations(n, M, L, P, ldp, gpu_ops):
    """The first (pair, head) items carry logits with equal values, a spread of +-80 and a -inf among finite ones (the very first all
    three at once, so that n = 1, M = 1 has them too); the padding columns of proj hold NaN."""
    i = sampling_inputs(n, M, L, P, ldp, 200 + n, edge_logits=True)
    want, cpu = sampling_reference(i), sampling_reference(i, torch.float32)
    got, again = _sampling_gpu(gpu_ops, i), _sampling_gpu(gpu_ops, i)
    for k in ("loc", "attn", "grad_proj"):
        assert torch.equal(got[k], again[k]), f"{k}: a second launch gives other bits"
        _held(f"sampling_locations n {n} MLP {M, L, P} {k}", got[k], want[k], cpu[k])
    pad = got["grad_proj"][:, 4 * M * L * P:]
    assert pad.numel() == n * (ldp - 4 * M * L * P) and bool((pad == 0).all()) and not bool(torch.signbit(pad).any())


def test_sampling_locations_nan_logit_stays_in_its_pair_and_head(gpu_ops):
    n, M, L, P, ldp = 9, 8, 1, 4, 128
    i = sampling_inputs(n, M, L, P, ldp, 31)
    pair, head = 4, 3
    i["proj"][pair, 3 * M * L * P + head * L * P + 2] = float("nan")
    want, cpu = sampling_reference(i), sampling_reference(i, torch.float32)
    got = _sampling_gpu(gpu_ops, i)
    nan_attn = torch.zeros(n, M, L, P, dtype=torch.bool)
    nan_attn[pair, head] = True
    nan_gp = torch.zeros(n, ldp, dtype=torch.bool)
    nan_gp[pair, 3 * M * L * P + head * L * P:3 * M * L * P + (head + 1) * L * P] = True
    assert torch.equal(torch.isnan(want["attn"]), nan_attn) and torch.equal(torch.isnan(want["grad_proj"]), nan_gp)    # as float64 does
    assert not bool(torch.isnan(got["loc"]).any())
    for k in ("loc", "attn", "grad_proj"):
        _held(f"sampling_locations with a NaN logit, {k}", got[k], want[k], cpu[k])


def test_sampling_locations_function(gpu_ops):
    from sgcdet_amd.functions import SamplingLocationsFunction
    i = sampling_inputs(65, 8, 1, 4, 128, 41, pad_value=0.0)
    c = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in i.items()}
    proj = c["proj"].clone().requires_grad_(True)
    loc, attn = SamplingLocationsFunction.apply(c["ref"], proj, c["normalizer"], 8, 1, 4)
    torch.autograd.backward((loc, attn), (c["grad_loc"], c["grad_attn"]))
    want = _sampling_gpu(gpu_ops, i)
    assert torch.equal(loc, want["loc"]) and torch.equal(attn, want["attn"]) and torch.equal(proj.grad, want["grad_proj"])
    loc0, attn0 = SamplingLocationsFunction.apply(c["ref"][:0], proj[:0], c["normalizer"], 8, 1, 4)
    assert loc0.shape == (0, 8, 1, 4, 3) and attn0.shape == (0, 8, 1, 4)


# ---- mean over views ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [32, 128])
def test_view_mean_backward(C, gpu_ops):
    from sgcdet_amd.functions import ViewMeanFunction
    i = view_mean_inputs(3, 70, C, 23)
    want = view_mean_reference(i)
    c = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in i.items()}
    n_pairs, n_valid = i["n_pairs"], i["valid_index"].numel()
    count = (i["slot"] >= 0).sum(0)
    assert int(count.min()) == 0 and int((count == 1).sum()) > 0 and int((count == 3).sum()) > 0        # seen by none, by one, by all
    got = gpu_ops.view_mean_backward(c["grad_mean"], c["slot"], c["valid_index"], n_pairs).cpu()
    ref = want["grad_feat"]
    assert bool(((got.double() - ref).abs() <= 2.0 ** -24 * ref.abs()).all())          # one rounding of the division
    # every pair row written, no row beyond: a NaN-filled buffer with two rows to spare
    buf = torch.full((n_pairs + 2, C), float("nan"), device="cuda")
    gpu_ops._call("sgc_view_mean_backward", c["grad_mean"], c["slot"], c["valid_index"], buf, 3, 70, C, n_valid, n_pairs)
    torch.cuda.synchronize()
    assert torch.equal(buf[:n_pairs].cpu(), got) and bool(torch.isnan(buf[n_pairs:]).all())
    # the Function: the forward is sgc_view_mean, the backward this kernel
    feat = c["feat"].clone().requires_grad_(True)
    mean = ViewMeanFunction.apply(feat, c["slot"], c["valid_index"], n_valid)
    assert torch.equal(mean, gpu_ops.view_mean(c["feat"], c["slot"], c["valid_index"], n_valid))
    # two adds of partial sums below 3 max |feat| and one division, half an ulp each
    assert max_err(mean.detach().cpu().double(), want["mean"]) <= 7 * 2.0 ** -24 * float(i["feat"].abs().max())
    mean.backward(c["grad_mean"])
    assert torch.equal(feat.grad.cpu(), got)


def test_scatter_rows_function(gpu_ops):
    from sgcdet_amd.functions import ScatterRowsFunction
    g = torch.Generator().manual_seed(3)
    rows = torch.randn(20, 32, generator=g).cuda().requires_grad_(True)
    idx = torch.randperm(70, generator=g)[:20].to(torch.int32).cuda()
    vol = ScatterRowsFunction.apply(rows, idx, 70)
    want = torch.zeros(70, 32, device="cuda").index_put((idx.long(),), rows.detach())
    assert torch.equal(vol, want)
    cot = torch.randn(70, 32, generator=g).cuda()
    vol.backward(cot)
    assert torch.equal(rows.grad, cot[idx.long()])


# ---- the level, switch off against switch on -------------------------------------------------------------------------------------------------
# Gradients that pass the float atomics of the DFA3D backward (grad_value / grad_dist: global atomics in the item kernel, LDS atomics
# in the binned one) and so depend on their order from run to run: the feature maps, the depth maps, and value_proj behind grad_value.
ORDER_DEPENDENT = ("value_proj",)


def _build_voxel_head(d, C=32):
    import sgcdet_amd.plugin  # noqa: F401  (registers the type= names)
    from sgcdet_amd.mmcv_lite import build_head
    from sgcdet_amd.scene import model_config
    w = dict(embed_dims=C, n_voxels_list=[tuple(int(v) for v in g) for g in d["grids"]],
             voxel_size_list=[tuple(float(v) for v in s) for s in d["sizes"]], topk_list=[int(v) for v in d["topk"]],
             head="ScanNetImVoxelHeadV2", n_classes=18, n_reg_outs=6)
    return build_head(model_config(w)["voxel_head"])


def _run_level(enabled, record=None):
    from sgcdet_amd.plugin import voxformer as vf
    d, sd = load("voxel_head")
    head = _build_voxel_head(d)
    head.load_state_dict(sd)
    head = head.cuda().train()
    for m in head.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    feats = [d[f"feat{i}"].cuda().requires_grad_() for i in range(4)]
    dpt = d["dpt"].cuda().requires_grad_()
    before = vf.TRAIN_LEVEL_FUSED["enabled"]
    vf.TRAIN_LEVEL_FUSED["enabled"] = enabled
    try:
        with (record if record is not None else contextlib.nullcontext()):
            volume, valid, occ = head(feats, img_meta(d), depth_pyramid(dpt))
            g = torch.Generator().manual_seed(1)
            w = torch.randn(volume.shape, generator=g).cuda()
            ((volume * w).sum() + occ.square().sum()).backward()
    finally:
        vf.TRAIN_LEVEL_FUSED["enabled"] = before
    return (volume.detach(), valid, [f.grad for f in feats[:3]], dpt.grad, {n: p.grad for n, p in head.named_parameters() if p.grad is not None})


@pytest.fixture(scope="module")
def level_runs():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return dict(off=_run_level(False), on=_run_level(True), on_again=_run_level(True))


def test_level_with_the_switch_on_equals_the_default_path(level_runs):
    v0, m0, fg0, dg0, pg0 = level_runs["off"]
    v1, m1, fg1, dg1, pg1 = level_runs["on"]
    assert torch.equal(m1, m0)
    print(f"volume: {max_err(v1, v0) / max(1.0, v0.abs().max().item()):.3e} of its scale")
    assert max_err(v1, v0) < 1e-5 * max(1.0, v0.abs().max().item())
    for k, (a, b) in enumerate(zip(fg1, fg0)):
        print(f"feat{k}.grad: {max_err(a, b) / max(1.0, b.abs().max().item()):.3e}")
        assert max_err(a, b) < 2e-4 * max(1.0, b.abs().max().item())
    print(f"dpt.grad: {max_err(dg1, dg0) / max(1.0, dg0.abs().max().item()):.3e}")
    assert max_err(dg1, dg0) < 2e-4 * max(1.0, dg0.abs().max().item())
    assert set(pg1) == set(pg0) and len(pg1) > 20
    worst = max((max_err(pg1[k], pg0[k]) / max(1.0, pg0[k].abs().max().item()), k) for k in pg0)
    print(f"parameter gradients: worst {worst[0]:.3e} ({worst[1]})")
    for k in pg0:
        assert max_err(pg1[k], pg0[k]) < 2e-4 * max(1.0, pg0[k].abs().max().item()), k


def test_level_with_the_switch_on_repeats_bit_for_bit(level_runs):
    v1, m1, _, _, pg1 = level_runs["on"]
    v2, m2, _, _, pg2 = level_runs["on_again"]
    assert torch.equal(m1, m2) and torch.equal(v1, v2)
    compared = [k for k in pg1 if not any(s in k for s in ORDER_DEPENDENT)]
    assert set(pg1) == set(pg2) and len(compared) > 20 and len(compared) < len(pg1)
    differ = [k for k in compared if not torch.equal(pg1[k], pg2[k])]
    assert not differ, differ


class _Recorder(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.names = set()

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.names.add(func._schema.name)
        return func(*args, **(kwargs or {}))


LIBRARY_OPS = ("aten::native_layer_norm", "aten::native_layer_norm_backward", "aten::_softmax", "aten::_softmax_backward_data",
               "aten::index_add")


def test_no_library_norm_softmax_or_index_add_is_left_in_a_fused_level(gpu_ops):
    off, on = _Recorder(), _Recorder()
    _run_level(False, record=off)
    _run_level(True, record=on)
    assert all(n in off.names for n in LIBRARY_OPS), sorted(set(LIBRARY_OPS) - off.names)        # the probe sees them, backward included
    left = sorted(n for n in LIBRARY_OPS if n in on.names)
    assert not left, left
