"""CPU checks of a view-transform level in training on the HIP kernels (include/sgcdet_amd_level_train.h, sgcdet_amd/functions.py
``LayerNormRowsFunction`` / ``SamplingLocationsFunction`` / ``ViewMeanFunction`` / ``ScatterRowsFunction``, plugin/voxformer.py
``TRAIN_LEVEL_FUSED``): the new header equals its binding tables, stays apart from the others and is exported; every
new entry has a buffer case with a finite float64 reference; the three backward formulas the kernels evaluate hold in float64 against
autograd of the default path's formulation; a ``VoxFormerLayer`` on CPU tensors does not see the switch."""
import copy
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sgc_layer_norm_rows_backward", "sgc_sampling_locations_forward", "sgc_sampling_locations_backward", "sgc_view_mean_backward")
NEW_QUERIES = ("sgc_layer_norm_rows_backward_workspace_floats",)


def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(sgc_[a-z0-9_]+)\s*\(", text)))


def test_header_equals_its_tables_and_the_library_exports_them():
    from sgcdet_amd import _abi, build
    new = set(_abi.LEVEL_TRAIN_SIGNATURES) | set(_abi.LEVEL_TRAIN_INTROSPECTION)
    assert _declared("sgcdet_amd_level_train.h") == sorted(new)
    assert set(NEW) == set(_abi.LEVEL_TRAIN_SIGNATURES) and set(NEW_QUERIES) == set(_abi.LEVEL_TRAIN_INTROSPECTION)
    old = set()
    for table in (_abi.SIGNATURES, _abi.INTROSPECTION, _abi.TRAIN_SIGNATURES, _abi.TRAIN_INTROSPECTION, _abi.IMAGE_SIGNATURES,
                  _abi.IMAGE_INTROSPECTION, _abi.DEPTH_TRAIN_SIGNATURES, _abi.DEPTH_TRAIN_INTROSPECTION):
        old |= set(table)
    assert not new & old
    for header in ("sgcdet_amd.h", "sgcdet_amd_train.h", "sgcdet_amd_image.h", "sgcdet_amd_depth_train.h"):
        assert not new & set(_declared(header)), header
    assert '#include "sgcdet_amd.h"' in open(os.path.join(ROOT, "include", "sgcdet_amd_level_train.h")).read()
    assert [len(_abi.LEVEL_TRAIN_SIGNATURES[n]) for n in NEW] == [12, 11, 11, 10]          # the stream included
    assert _abi.ABI_VERSION == 4                                  # no existing argument list changed
    lib = _abi.Library(build.build(), train=True)                 # raises ImportError on a missing symbol
    assert all(hasattr(lib._dll, n) for n in NEW + NEW_QUERIES)
    plain = _abi.Library(build.build())._dll
    assert all(getattr(plain, n).argtypes is None for n in NEW + NEW_QUERIES)             # bound with the training tables only


def test_every_new_entry_point_that_writes_device_memory_has_a_case():
    """The assertion of tests/test_buffers_cpu.py ``test_every_entry_point_that_writes_device_memory_has_a_case`` for the new tables."""
    from sgcdet_amd import _abi
    from buffer_cases import CASES as OLD
    from buffer_cases_depth_train import CASES as OLD_DEPTH
    from buffer_cases_level_train import CASES
    names = set(_abi.LEVEL_TRAIN_SIGNATURES) | set(_abi.LEVEL_TRAIN_INTROSPECTION)
    excluded = {n for n in names if n.endswith(("_supported", "_workspace_floats", "_workspace_bytes"))}
    covered = set()
    for case in CASES:
        assert case.entries, f"{case}: names no entry point"
        assert set(case.entries) <= names, f"{case}: unknown entry point {set(case.entries) - names}"
        assert case.only == "cuda" and case.ref is not None
        covered |= set(case.entries)
    assert not (covered & excluded)
    uncovered = sorted(names - excluded - covered)
    assert not uncovered, f"{len(uncovered)} entry points that write device memory have no case: {uncovered}"
    ids = [c.name for c in CASES] + [c.name for c in OLD] + [c.name for c in OLD_DEPTH]
    assert len(ids) == len(set(ids))


def test_buffer_cases_build_finite_float64_references():
    from buffer_cases_level_train import CASES
    for case in CASES:
        ref = case.reference(None)
        assert ref and all(v.dtype == torch.float64 and bool(torch.isfinite(v).all()) for v in ref.values()), case.name


# ---- the formulas of include/sgcdet_amd_level_train.h in float64 --------------------------------------------------------------------
def test_layer_norm_backward_identity():
    from buffer_cases_level_train import EPS, ln_inputs, ln_reference
    i = {k: v.double() for k, v in ln_inputs(9, 24, 3, special=True).items()}
    want = ln_reference(i)
    x, dy, gamma = i["x"], i["dy"], i["gamma"]
    mean = x.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(1, keepdim=True) + EPS)
    xhat, g = (x - mean) * rstd, dy * gamma
    dx = rstd * (g - g.mean(1, keepdim=True) - xhat * (g * xhat).mean(1, keepdim=True))
    scale = want["dx"].abs().max()
    assert (dx - want["dx"]).abs().max() < 1e-12 * scale
    assert ((dy * xhat).sum(0) - want["dgamma"]).abs().max() < 1e-12 and (dy.sum(0) - want["dbeta"]).abs().max() < 1e-12


def test_sampling_locations_backward_identity():
    from buffer_cases_level_train import sampling_inputs, sampling_reference
    for n, M, L, P, ldp in ((5, 8, 1, 4, 128), (6, 4, 2, 2, 64), (3, 1, 1, 4, 32), (4, 2, 1, 3, 24)):
        i = sampling_inputs(n, M, L, P, ldp, 5, edge_logits=L * P == 4)
        want = sampling_reference(i)
        MLP = M * L * P
        nz = i["normalizer"].double()                                                 # [L, 3]
        gl, ga, a = i["grad_loc"].double(), i["grad_attn"].double().view(n, M, L * P), want["attn"].view(n, M, L * P)
        got = torch.zeros(n, ldp, dtype=torch.float64)
        got[:, :2 * MLP] = (gl[..., :2] / nz[None, None, :, None, :2]).reshape(n, -1)
        got[:, 2 * MLP:3 * MLP] = (gl[..., 2] / nz[None, None, :, None, 2]).reshape(n, -1)
        got[:, 3 * MLP:4 * MLP] = (a * (ga - (a * ga).sum(-1, keepdim=True))).reshape(n, -1)
        assert bool(torch.isfinite(want["grad_proj"]).all())
        assert (got - want["grad_proj"]).abs().max() < 1e-13 * max(1.0, float(want["grad_proj"].abs().max()))
        assert bool((want["grad_proj"][:, 4 * MLP:] == 0).all())


def test_view_mean_backward_identity():
    from buffer_cases_level_train import view_mean_inputs, view_mean_reference
    i = view_mean_inputs(3, 70, 8, 2)
    want = view_mean_reference(i)
    slot, vi = i["slot"].long(), i["valid_index"].long()
    count = (slot >= 0).sum(0)
    assert int(count.min()) == 0 and int((count == 1).sum()) > 0 and int((count == 3).sum()) > 0       # seen by none, by one, by all
    assert bool((count[vi] > 0).all()) and vi.numel() == int((count > 0).sum())
    got = torch.full((i["n_pairs"], 8), float("nan"), dtype=torch.float64)
    writes = torch.zeros(i["n_pairs"], dtype=torch.long)
    for r, v in enumerate(vi.tolist()):
        for n in range(slot.shape[0]):
            if slot[n, v] >= 0:
                got[slot[n, v]] = i["grad_mean"][r].double() / float(count[v])
                writes[slot[n, v]] += 1
    assert bool((writes == 1).all())                                                  # every pair row exactly once
    assert (got - want["grad_feat"]).abs().max() < 1e-15
    # the forward: the mean over the cameras in camera order is the index_add formulation
    mean = torch.stack([sum(i["feat"][slot[n, v]].double() for n in range(slot.shape[0]) if slot[n, v] >= 0) / float(count[v])
                        for v in vi.tolist()])
    assert (mean - want["mean"]).abs().max() < 1e-14


# ---- the switch on the CPU -------------------------------------------------------------------------------------------------------------
def _layer_and_inputs():
    import sgcdet_amd.plugin  # noqa: F401
    from sgcdet_amd.mmcv_lite import TRANSFORMER_LAYER
    C, N, H, W, D, Nq = 32, 3, 6, 8, 8, 50
    cfg = dict(type="VoxFormerLayer",
               attn_cfgs=[dict(type="DeformCrossAttention_DFA3D", embed_dims=C, inter_view_aggregation="attn", dropout=0,
                               deformable_attention=dict(type="MSDeformableAttention3D_DFA3D", embed_dims=C, num_heads=8, num_points=4,
                                                         num_levels=1, im2col_step=128))],
               ffn_cfgs=dict(type="FFN", embed_dims=C, feedforward_channels=C * 2, num_fcs=2, ffn_drop=0.0, act_cfg=dict(type="ReLU", inplace=True)),
               operation_order=("cross_attn", "norm", "ffn", "norm"))
    torch.manual_seed(0)
    layer = TRANSFORMER_LAYER.build(cfg).train()
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for p in layer.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=g))
    mask = torch.rand(N, Nq, generator=g) < 0.6
    mask[:, 0] = False                                             # a voxel no camera sees
    t = dict(query=torch.randn(1, Nq, C, generator=g), value=torch.randn(N, H * W, 1, C, generator=g),
             dist=torch.softmax(torch.randn(N, H * W, 1, D, generator=g), -1), ref_cam=torch.rand(N, 1, Nq, 1, 3, generator=g),
             mask=mask.view(N, 1, Nq, 1), shapes=torch.tensor([[H, W]]), lsi=torch.zeros(1, dtype=torch.long),
             cot=torch.randn(1, Nq, C, generator=g))
    return layer, t


def test_layer_on_cpu_tensors_does_not_see_the_switch(monkeypatch, oracle_ops):
    from sgcdet_amd import ext
    from sgcdet_amd.plugin import voxformer as vf
    monkeypatch.setattr(ext, "ops", lambda: oracle_ops)            # the CPU binding of include/sgcdet_amd.h
    assert vf.TRAIN_LEVEL_FUSED == dict(enabled=os.environ.get("SGC_LEVEL_TRAIN_FUSED", "0") == "1")
    layer0, t = _layer_and_inputs()
    results = []
    for enabled in (False, True):
        monkeypatch.setitem(vf.TRAIN_LEVEL_FUSED, "enabled", enabled)
        layer = copy.deepcopy(layer0)
        q, v, d = (t[k].clone().requires_grad_(True) for k in ("query", "value", "dist"))
        assert not vf._level_fused(q)
        out = layer(q, v, v, reference_points_cam=t["ref_cam"], bev_mask=t["mask"], spatial_shapes=t["shapes"], level_start_index=t["lsi"],
                    value_dpt_dist=d)
        (out * t["cot"]).sum().backward()
        grads = {n: p.grad for n, p in layer.named_parameters() if p.grad is not None}
        results.append((out.detach(), q.grad, v.grad, d.grad, grads))
    a, b = results
    assert len(a[4]) > 10 and set(a[4]) == set(b[4])
    for x, y in zip(a[:4], b[:4]):
        assert torch.equal(x, y)
    for k in a[4]:
        assert torch.equal(a[4][k], b[4][k]), k
