"""CPU checks of ``sgcdet_amd.optim``: the boundary of the two optimiser kernels (header, binding tables, exported
symbols, item layout), ``build_optimizer`` on the settings of the reference's four configs against the reference's own construction
restated from torch parts, and the errors ``FusedAdamW`` documents.  No kernel runs here."""
import ctypes
import json
import os
import re
import struct
import warnings

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = os.path.join(ROOT, "tests", "golden", "ref_train_settings.json")       # tests/golden/make_golden_train_settings.py
NAMES = ("SGCDet_ScanNet", "SGCDet_ARKit", "SGCDet_large_ScanNet200", "SGCDet_large_ARKit")


def _header():
    return open(os.path.join(ROOT, "include", "sgcdet_amd_train.h")).read()


def test_optimiser_entry_points_in_header_tables_and_library():
    from sgcdet_amd import build
    from sgcdet_amd._abi import (Library, OptimGroup, OPTIM_ITEM_BYTES, SIGNATURES, INTROSPECTION, TRAIN_SIGNATURES,
                                 TRAIN_INTROSPECTION)
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = set(re.findall(r"\b(sgc_[a-z0-9_]+)\s*\(", text))
    assert {"sgc_grad_sqnorm_batch", "sgc_adamw_step_batch"} <= declared & set(TRAIN_SIGNATURES)
    assert "sgc_grad_sqnorm_batch_workspace_bytes" in declared & set(TRAIN_INTROSPECTION)
    assert not {"sgc_grad_sqnorm_batch", "sgc_adamw_step_batch", "sgc_grad_sqnorm_batch_workspace_bytes"} & (set(SIGNATURES) | set(INTROSPECTION))
    # argument counts of the header's prototypes equal the tables'
    for name, table in (("sgc_grad_sqnorm_batch", TRAIN_SIGNATURES), ("sgc_adamw_step_batch", TRAIN_SIGNATURES)):
        args = re.search(name + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
        assert len(args.split(",")) == len(table[name]), name
    lib = Library(build.build(), train=True)            # ImportError on a missing symbol
    assert lib.backend == "hip-gfx950"
    q = lib._dll.sgc_grad_sqnorm_batch_workspace_bytes
    assert q(0) == 0 and q(1) == 16 and q(4) == 16 and q(5) == 32 and q(3000) == 12000
    # the item: the header's fields in order, 64 bytes (a power of two), as TensorOps.optim_item_list packs it
    body = re.search(r"typedef struct sgc_optim_item \{(.*?)\} sgc_optim_item;", text, flags=re.S).group(1)
    fields = re.findall(r"\*?\s*(\w+)\s*[,;]", body)
    assert fields == ["param", "grad", "exp_avg", "exp_avg_sq", "numel", "group", "step", "block_start", "block_elems",
                      "bias_correction1", "bias_correction2_sqrt"]
    assert struct.calcsize("<4Qq4i2f") == OPTIM_ITEM_BYTES == 64 and "/* 64 bytes */" in _header()
    assert ctypes.sizeof(OptimGroup) == 40 and [f for f, _ in OptimGroup._fields_] == ["lr", "weight_decay", "beta1", "beta2", "eps"]
    assert re.search(r"#define SGC_OPTIM_MAX_GROUPS 8\b", text)
    # sgc_adamw_step_batch refuses more groups than fit its argument block, before any launch (host code: runs without a GPU)
    groups = (OptimGroup * 9)(*[OptimGroup(1e-3, 0.0, 0.9, 0.999, 1e-8)] * 9)
    assert lib._dll.sgc_adamw_step_batch(1, 1, 1, groups, 9, None, 0.0, None) == -3              # SGC_EUNSUP
    assert "9 parameter groups" in lib.last_error()
    assert lib._dll.sgc_adamw_step_batch(None, 1, 1, groups, 1, None, 0.0, None) == -1           # SGC_EINVAL
    assert lib._dll.sgc_grad_sqnorm_batch(1, 0, 1, 1, 1, None) == -1


def test_item_list_layout_and_block_accounting():
    from sgcdet_amd._abi import Library
    from sgcdet_amd import build
    from sgcdet_amd.tensor_api import TensorOps
    ops = TensorOps(Library(build.build(), train=True), "cuda")       # host-side packing only: nothing is launched
    a, b, c = torch.zeros(10000), torch.zeros(0), torch.zeros(1)
    entries = [(a, a, a, a, 0, 3, 0.271, 0.0547), (b, b, b, b, 0, 3, 0.271, 0.0547), (c, c, c, c, 1, 1, 0.1, 0.0316)]
    blob, n, total = ops.optim_item_list(entries, block_elems=4096)
    assert n == 2 and total == 3 + 1 and len(blob) == 2 * 64                    # the empty tensor owns no item
    i0, i1 = struct.unpack_from("<4Qq4i2f", blob, 0), struct.unpack_from("<4Qq4i2f", blob, 64)
    assert i0[0] == a.data_ptr() and i0[4:9] == (10000, 0, 3, 0, 4096) and abs(i0[9] - 0.271) < 1e-7
    assert i1[3] == c.data_ptr() and i1[4:9] == (1, 1, 1, 3, 4096)
    with pytest.raises(ValueError):
        ops.optim_item_list(entries, block_elems=1022)


class _TwoPart(torch.nn.Module):
    """Stands in for the reference's model where only the parameter NAMES matter: an image backbone and the rest."""

    def __init__(self):
        super().__init__()
        self.backbone = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.BatchNorm2d(4))
        self.neck = torch.nn.Conv2d(4, 4, 1)
        self.bbox_head = torch.nn.Linear(4, 2)
        self.neck.bias.requires_grad_(False)              # frozen: in neither group


def _reference_construction(model, cfg):
    """LightningTools/pl_model.py:92-136 restated: torch.optim.AdamW over the two name-selected groups + OneCycleLR."""
    o, s = cfg["optimizer"], cfg["lr_scheduler"]
    assert o["type"] == "AdamW" and s["type"] == "OneCycleLR"
    groups = [
        {"params": [p for n, p in model.named_parameters() if p.requires_grad and "backbone" in n],
         "lr": o["lr"] * 0.1, "weight_decay": o["weight_decay"] * 1.0, "name": "backbone"},
        {"params": [p for n, p in model.named_parameters() if p.requires_grad and "backbone" not in n],
         "lr": o["lr"], "weight_decay": o["weight_decay"], "name": "others"},
    ]
    opt = torch.optim.AdamW(groups)
    sched = torch.optim.lr_scheduler.OneCycleLR(
        opt, max_lr=[s["max_lr"] * 0.1, s["max_lr"]], total_steps=s["total_steps"], pct_start=s["pct_start"],
        cycle_momentum=s["cycle_momentum"], anneal_strategy=s["anneal_strategy"], final_div_factor=s["final_div_factor"])
    return opt, sched


def _lr_trace(opt, sched, total_steps):
    """Learning rates of every group over the first 200 and the last 10 scheduler steps (OneCycleLR is a closed form of
    ``last_epoch``: the stretch between the two windows is jumped over, identically for both sides)."""
    out = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                    # "lr_scheduler.step() before optimizer.step()": step() is never called here
        out.append([g["lr"] for g in opt.param_groups])
        for _ in range(200):
            sched.step()
            out.append([g["lr"] for g in opt.param_groups])
        sched.last_epoch = total_steps - 11
        for _ in range(10):
            sched.step()
            out.append([g["lr"] for g in opt.param_groups])
    assert sched.last_epoch == total_steps - 1
    return out


@pytest.mark.parametrize("name", NAMES)
def test_build_optimizer_equals_the_reference_construction(name):
    from sgcdet_amd.optim import FusedAdamW, build_optimizer
    cfg = json.load(open(SETTINGS))[name]
    assert cfg["lr_scheduler"]["total_steps"] == cfg["training_steps"] + 10
    torch.manual_seed(0)
    model = _TwoPart()
    opt, sched = build_optimizer(model, cfg["optimizer"], cfg["lr_scheduler"])
    ropt, rsched = _reference_construction(model, cfg)
    assert isinstance(opt, FusedAdamW) and isinstance(opt, torch.optim.Optimizer) and opt.max_grad_norm == 35.0
    assert isinstance(sched, torch.optim.lr_scheduler.OneCycleLR)
    assert len(opt.param_groups) == len(ropt.param_groups) == 2
    for g, r in zip(opt.param_groups, ropt.param_groups):
        assert [id(p) for p in g["params"]] == [id(p) for p in r["params"]] and g["name"] == r["name"]
        for k in ("lr", "initial_lr", "max_lr", "min_lr", "weight_decay", "betas", "eps", "amsgrad", "maximize"):
            assert g[k] == r[k], (k, g[k], r[k])
    assert opt.param_groups[0]["weight_decay"] == opt.param_groups[1]["weight_decay"] == 1e-4
    assert opt.param_groups[0]["max_lr"] == 0.1 * cfg["lr_scheduler"]["max_lr"] and opt.param_groups[1]["max_lr"] == cfg["lr_scheduler"]["max_lr"]
    assert all(model.neck.bias is not p for g in opt.param_groups for p in g["params"])
    a = _lr_trace(opt, sched, cfg["lr_scheduler"]["total_steps"])
    b = _lr_trace(ropt, rsched, cfg["lr_scheduler"]["total_steps"])
    assert len(a) == 211 and a == b                             # exact: it is the same scheduler on the same numbers
    assert a[0][1] < a[200][1] and a[-1][1] < a[0][1] and all(x[0] < x[1] for x in a)


def test_build_optimizer_drops_the_empty_group_and_refuses_unknown_types():
    import sgcdet_amd.plugin  # noqa: F401
    from sgcdet_amd.mmcv_lite import build_detector
    from sgcdet_amd.optim import build_optimizer, reference_param_groups
    from sgcdet_amd.scene import model_config, workload
    cfg = json.load(open(SETTINGS))["SGCDet_ScanNet"]
    det = build_detector(model_config(workload("cfg1_plumbing")))         # built from feature maps on: no image backbone
    groups = reference_param_groups(det, 2e-4, 1e-4)
    assert [g["name"] for g in groups] == ["others"] and groups[0]["lr"] == 2e-4
    assert len(groups[0]["params"]) == sum(p.requires_grad for p in det.parameters())
    opt, sched = build_optimizer(det, cfg["optimizer"], cfg["lr_scheduler"], max_grad_norm=None)
    assert len(opt.param_groups) == 1 and opt.param_groups[0]["max_lr"] == 2e-4 and opt.max_grad_norm is None
    with pytest.raises(NotImplementedError):
        build_optimizer(det, dict(cfg["optimizer"], type="SGD"), cfg["lr_scheduler"])
    with pytest.raises(NotImplementedError):
        build_optimizer(det, cfg["optimizer"], dict(cfg["lr_scheduler"], type="StepLR"))


def test_fused_adamw_refuses_what_it_documents():
    from sgcdet_amd.optim import FusedAdamW
    # the product has no CPU fallback: a CPU parameter raises at step(), before anything is launched
    p = torch.nn.Parameter(torch.zeros(8))
    opt = FusedAdamW([p], lr=1e-3)
    p.grad = torch.ones(8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step()
    assert torch.equal(p.detach(), torch.zeros(8)) and len(opt.state) == 0
    # only float32, by name where the caller gave names
    half = torch.nn.Parameter(torch.zeros(4, dtype=torch.float16))
    with pytest.raises(TypeError, match=r"param_groups\[0\]\['params'\]\[1\].*float16"):
        FusedAdamW([torch.nn.Parameter(torch.zeros(4)), half], lr=1e-3)
    with pytest.raises(TypeError, match="float64"):
        FusedAdamW([torch.nn.Parameter(torch.zeros(4, dtype=torch.float64))], lr=1e-3)
    lin = torch.nn.Linear(2, 2).half()
    with pytest.raises(TypeError, match="weight.*float16"):
        FusedAdamW(lin.named_parameters(), lr=1e-3)
    with pytest.raises(ValueError):
        FusedAdamW([p], lr=1e-3, max_grad_norm=0.0)
    with pytest.raises(ValueError):
        FusedAdamW([p], lr=-1.0)
    with pytest.raises(ValueError):
        FusedAdamW([dict(params=[torch.nn.Parameter(torch.zeros(1))]) for _ in range(9)], lr=1e-3)


def test_state_dict_has_torch_adamw_layout():
    """The groups carry torch.optim.AdamW's keys, so a checkpoint moves between the two classes (the state itself is covered on the
    GPU, tests/test_gpu_optim.py)."""
    from sgcdet_amd.optim import FusedAdamW
    ps = [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2, 2))]
    a = FusedAdamW([dict(params=ps[:1], lr=1e-4), dict(params=ps[1:])], lr=1e-3, weight_decay=1e-4, max_grad_norm=35.0)
    b = torch.optim.AdamW([dict(params=ps[:1], lr=1e-4), dict(params=ps[1:])], lr=1e-3, weight_decay=1e-4)
    sa, sb = a.state_dict(), b.state_dict()
    assert sa["state"] == sb["state"] == {}
    for ga, gb in zip(sa["param_groups"], sb["param_groups"]):
        assert set(gb) <= set(ga) and all(ga[k] == gb[k] for k in gb), (ga, gb)
    b.load_state_dict(sa)
    a.load_state_dict(sb)
    assert a.param_groups[0]["lr"] == 1e-4 and b.param_groups[1]["weight_decay"] == 1e-4
